"""The rate of the ``demfi_payload_deblock`` launch (``--deblock``) beside its yardsticks, ``demfi_yuv_bob`` and ``demfi_payload_promote``, over the
same payloads in one process: payload bytes per second, device events around every launch.  All three read and write every payload byte
once (the promotion writes the wider sample), so the rates compare.  The figures of profiles/deblock.md come from this script.

    python tools/deblock_rate.py [--payloads 64] [--height 1080] [--width 1920] [--rounds 5] [--launches 10] [--out FILE]

The deblocker works in place, so every launch starts from a fresh device copy of the input (made outside the events): the branch mix is
that of coded-looking material (8x8 blocks of random levels plus noise), not of an already smoothed picture.  Before the timing one payload
of every shape is compared with ``deblock.deblock_payload_np``.  Needs a GPU; fails without one."""
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
from demfi_amd import deblock as DB                                      # noqa: E402
from demfi_amd import interlace as IL                                    # noqa: E402
from demfi_amd import y4m                                                # noqa: E402


def blocky(h, w, layout, depth, seed):
    """8x8 blocks of random levels (jumps of up to +-20 steps) plus noise of +-3 steps, in every plane."""
    g = np.random.RandomState(seed)
    out = []
    for r, c in IL.plane_shapes(h, w, layout):
        lev = g.randint(30, 220) + g.randint(-10, 11, (r // 8 + 1, c // 8 + 1))
        out.append((np.clip(lev.repeat(8, 0).repeat(8, 1)[:r, :c] + g.randint(-3, 4, (r, c)), 0, 255) << (depth - 8)).reshape(-1))
    return np.concatenate(out).astype(np.uint8 if depth == 8 else np.uint16)


def timed(launch, restore, rounds, launches):
    """ms per launch: the median over ``rounds`` of the mean over ``launches``, and the rounds' least and greatest."""
    per = []
    for _ in range(rounds + 1):                                          # the first round warms up
        evs = []
        for _ in range(launches):
            restore()
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
    ap.add_argument('--payloads', type=int, default=64)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('deblock_rate.py: no GPU visible')
    lib, dev, st = L.load(), 'cuda:0', torch.cuda.current_stream().cuda_stream
    h, w, n = a.height, a.width, a.payloads
    rows = []
    for layout, depth in (('420', 8), ('422', 10)):
        es, P = (1 if depth == 8 else 2), y4m.payload_size(h, w, layout)
        Pb = P * es
        host = np.stack([blocky(h, w, layout, depth, s) for s in range(min(n, 4))])
        src = torch.from_numpy(host.view(np.uint8).reshape(len(host), Pb)).to(dev).repeat(-(-n // len(host)), 1)[:n].contiguous()
        work = torch.empty_like(src)
        restore = lambda: work.copy_(src)                                # noqa: E731
        thr = DB.thresholds(depth)
        for fields in (None, 't'):
            tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields), dtype=np.int64)
            launch = lambda: L.check(lib.demfi_payload_deblock(work.data_ptr(), Pb, n, tab.ctypes.data, len(tab), es, *thr, st), 'deblock')   # noqa: E731
            restore()
            launch()
            torch.cuda.synchronize()
            got = work[0].cpu().numpy().view(host.dtype)
            exp = DB.deblock_payload_np(host[0], h, w, depth, layout, fields=fields)
            if not np.array_equal(got, exp):
                raise SystemExit('deblock_rate.py: the kernel differs from the definition at %dx%d %s %d-bit' % (w, h, layout, depth))
            rows.append(('deblock %s' % ('fields' if fields else 'progressive'), layout, depth, float((exp != host[0]).mean()),
                         timed(launch, restore, a.rounds, a.launches)))
        # the yardsticks: the bob in place over the same buffer; the promotion of the same payloads to the next depth
        mask = sum((i & 1) << i for i in range(min(n, 64)))
        bob = lambda: [L.check(lib.demfi_yuv_bob(work[c0].data_ptr(), Pb, min(64, n - c0), h, w, L.YUV_LAYOUT[layout], es, mask, st), 'bob')   # noqa: E731
                       for c0 in range(0, n, 64)]
        rows.append(('yuv_bob', layout, depth, None, timed(bob, restore, a.rounds, a.launches)))
        d_out = depth + 2
        planes = np.ascontiguousarray(IL.plane_shapes(h, w, layout), dtype=np.int32)
        offs = np.arange(n, dtype=np.int64) * Pb
        offs_dev = torch.from_numpy(offs).to(dev)
        wide = torch.empty((n, 2 * P), dtype=torch.uint8, device=dev)
        pro = lambda: L.check(lib.demfi_payload_promote(work.data_ptr(), offs.ctypes.data, offs_dev.data_ptr(), n, planes.ctypes.data,    # noqa: E731
                                                        len(planes), es, 2, depth, d_out, 0, wide.data_ptr(), 2 * P, st), 'promote')
        rows.append(('payload_promote %d -> %d' % (depth, d_out), layout, depth, None, timed(pro, restore, a.rounds, a.launches)))
        del src, work, wide
    out = []
    for name, layout, depth, changed, (ms, lo, hi) in rows:
        Pb = y4m.payload_size(h, w, layout) * (1 if depth == 8 else 2)
        rec = {'launch': name, 'layout': layout, 'depth': depth, 'payloads': n, 'size': '%dx%d' % (w, h), 'payload_bytes': Pb,
               'ms_per_launch': round(ms, 4), 'ms_rounds': [round(lo, 4), round(hi, 4)], 'us_per_payload': round(1e3 * ms / n, 3),
               'payload_GB_per_s': round(n * Pb / ms / 1e6, 1), 'samples_changed': None if changed is None else round(changed, 4)}
        out.append(rec)
        print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
