"""The rate of the ``demfi_rgb_lut3d`` launch (``--lut``) at 720p and 1080p for cubes of 17, 33 and 65 lattice points over two contents: a
natural-like frame (smooth gradients plus mild noise, where neighbouring pixels share lattice cells) and a frame of uniformly random
colours (the worst case for the cube's locality in L2).  Per case: milliseconds per payload, payload bytes per second (12 bytes a pixel:
6 read, 6 written) and their share of the stage's memory bound at the HBM rate of 6.3 TB/s that a streaming kernel achieves on an
MI355X; at 17 lattice points also the variant that keeps the cube in LDS (``cube_in_lds`` = 1), launch for launch beside the one that
reads it through L2.  Device events around every launch.  The figures of profiles/lut3d.md come from this script.

    python tools/lut3d_rate.py [--payloads 8] [--rounds 5] [--launches 10] [--shapes 720p,1080p] [--depth 10] [--out FILE]

Before the timing the first payload of every case at 720p is compared with ``lut3d.lut_payload_np``, whole.  Needs a GPU; fails without
one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from demfi_amd import _lib as L                                          # noqa: E402
from demfi_amd import lut3d as LU                                        # noqa: E402

SHAPES = {'720p': (720, 1280), '1080p': (1080, 1920)}
SIZES = (17, 33, 65)
HBM_BYTES_PER_S = 6.3e12                                                 # what a streaming copy achieves of the 8 TB/s peak


def content(kind, n, h, w, depth, seed):
    """n frames of codes [n, 3, h, w]: 'natural' = three smooth ramps that drift from frame to frame plus noise of about 1 % of the
    peak; 'random' = uniformly random colours."""
    peak, rng = (1 << depth) - 1, np.random.default_rng(seed)
    if kind == 'random':
        return rng.integers(0, peak + 1, (n, 3, h, w))
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        base = np.stack([(x + 13 * i) / (w + 13 * n), (y + 7 * i) / (h + 7 * n),
                         0.5 + 0.25 * np.sin((x + y + 29 * i) / 97.0) + 0.2 * np.cos(y / 53.0)])
        out.append(np.clip(np.rint(base * peak + rng.normal(0, peak / 100, base.shape)), 0, peak).astype(np.int64))
    return np.stack(out)


def timed(launch, rounds, launches):
    """ms per launch: the median over ``rounds`` of the mean over ``launches``, and the rounds' least and greatest."""
    per = []
    for _ in range(rounds + 1):                                          # the first round warms up
        evs = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        per.append(sum(a.elapsed_time(b) for a, b in evs) / launches)
    per = per[1:]
    return float(np.median(per)), min(per), max(per)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--payloads', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--shapes', default='720p,1080p')
    ap.add_argument('--depth', type=int, default=10)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lut3d_rate.py: no GPU visible')
    lib, dev, st = L.load(), 'cuda:0', torch.cuda.current_stream().cuda_stream
    n, depth, out = a.payloads, a.depth, []
    fwd, inv_in = LU.tables(depth)
    inv_dev = torch.from_numpy(inv_in.view(np.int16)).to(dev)
    host_offs = None
    for shape in a.shapes.split(','):
        h, w = SHAPES[shape]
        Pb = 6 * h * w
        host_offs = np.arange(n, dtype=np.int64) * Pb
        offs = torch.from_numpy(host_offs).to(dev)
        for kind in ('natural', 'random'):
            pays = fwd[content(kind, n, h, w, depth, 5)].astype('<u2')
            src = torch.from_numpy(pays.view(np.int16).reshape(n, -1)).to(dev)
            dst = torch.empty_like(src)
            for size in SIZES:
                cube = LU.Cube(size, np.random.default_rng(size).integers(0, 65536, (size, size, size, 3)))
                axt = torch.from_numpy(LU.axis_table(depth, size).view(np.int32)).to(dev)
                words = torch.from_numpy(LU.cube_words(cube).view(np.int64).reshape(-1)).to(dev)

                def launch(in_lds, count=n):
                    L.check(lib.demfi_rgb_lut3d(src.data_ptr(), host_offs.ctypes.data, offs.data_ptr(), count, h, w, depth, inv_dev.data_ptr(),
                                                size, words.data_ptr(), axt.data_ptr(), in_lds, dst.data_ptr(), Pb, st), 'rgb_lut3d')
                for in_lds in ((0, 1) if size <= 17 else (0,)):
                    if shape == '720p':
                        dst.zero_()
                        launch(in_lds, 1)
                        torch.cuda.synchronize()
                        got = dst[0].cpu().numpy().view(np.uint16).reshape(3, h, w)
                        if not np.array_equal(got, LU.lut_payload_np(pays[0], inv_in, depth, cube)):
                            raise SystemExit('lut3d_rate.py: the kernel differs from the definition at %s %s N=%d lds=%d' % (shape, kind, size, in_lds))
                    ms, lo, hi = timed(lambda: launch(in_lds), a.rounds, a.launches)
                    rate = n * 2 * Pb / ms * 1e3                         # bytes read and written per second
                    rec = {'launch': 'rgb_lut3d', 'shape': shape, 'size': '%dx%d' % (w, h), 'content': kind, 'cube': size,
                           'cube_in_lds': in_lds, 'depth': depth, 'payloads': n, 'ms_per_launch': round(ms, 4),
                           'ms_rounds': [round(lo, 4), round(hi, 4)], 'ms_per_payload': round(ms / n, 4),
                           'payload_TB_per_s': round(rate / 1e12, 3), 'share_of_memory_bound': round(rate / HBM_BYTES_PER_S, 3)}
                    out.append(rec)
                    print(json.dumps(rec), flush=True)
            del src, dst
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
