"""The rate of the ``demfi_payload_nlmeans`` launch (``--nlmeans``) at 3:1:3, 3:2:5 and 3:3:7, of the device copy into the scratch buffer
that the stage makes in front of it, and of ``demfi_payload_deband`` at 2:16 over the same payloads in the same process as the yardstick:
microseconds per payload, payload bytes per second and, for the denoising launch, candidate samples per second (samples times (2R + 1)^2:
the candidates skipped at the borders are counted whole) and the vector instructions per second that implies at the instructions per
candidate sample counted in the device assembly (``VALU_PER_CANDIDATE``; profiles/nlmeans.md says how), device events around every launch.
The figures of profiles/nlmeans.md come from this script.

    python tools/nlmeans_rate.py [--payloads 8] [--rounds 5] [--launches 10] [--shapes 576i,720p,1080p] [--bench-fps F] [--out FILE]

Shapes: 576i (720 x 576, filtered by fields), 720p and 1080p, each as 8-bit 4:2:0 and 10-bit 4:2:2.  The input is that of the GPU tests
(ramps, texture, hard edges, noise, flat areas).  Before the timing one payload of every shape is compared with
``nlmeans.nlmeans_payload_np``, whole, at 3:1:3 (the definition makes (2R + 1)^2 passes over the payload in numpy; the GPU tests hold every
radius to the definition).  ``--bench-fps``: the frames/s ``bench.py`` printed on the same machine in the same session; with it the cost
of the default on a 720p 8-bit 4:2:0 payload is also given as a share of the benchmark's time per 720p output frame.  Needs a GPU; fails
without one."""
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
from demfi_amd import nlmeans as NL                                      # noqa: E402
from demfi_amd import y4m                                                # noqa: E402
from tests.test_nlmeans import noisy_payload                             # noqa: E402

SHAPES = {'576i': (576, 720, 't'), '720p': (720, 1280, None), '1080p': (1080, 1920, None)}
TRIPLES = ((3, 1, 3), (3, 2, 5), (3, 3, 7))
# vector instructions of the offset loop per candidate sample (a thread's loop body serves 16), by bytes per sample and P, counted in the
# device assembly of `build.sh --asm` (profiles/nlmeans.md)
VALU_PER_CANDIDATE = {(1, 1): 18.4, (1, 2): 28.0, (1, 3): 38.4, (2, 1): 20.8, (2, 2): 32.4, (2, 3): 45.4}


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
    ap.add_argument('--shapes', default='576i,720p,1080p')
    ap.add_argument('--bench-fps', type=float, default=None)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nlmeans_rate.py: no GPU visible')
    lib, dev, st = L.load(), 'cuda:0', torch.cuda.current_stream().cuda_stream
    n, out = a.payloads, []
    for shape in a.shapes.split(','):
        h, w, fields = SHAPES[shape]
        for layout, depth in (('420', 8), ('422', 10)):
            es, P = (1 if depth == 8 else 2), y4m.payload_size(h, w, layout)
            Pb = P * es
            host = np.stack([noisy_payload(h, w, layout, depth, s, fields) for s in range(2)])
            src = torch.from_numpy(host.view(np.uint8).reshape(len(host), Pb)).to(dev).repeat(-(-n // len(host)), 1)[:n].contiguous()
            work, scratch = torch.empty_like(src), torch.empty_like(src)
            tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields), dtype=np.int64)
            tables = {spr: NL.weight_table(depth, spr[0], spr[1]) for spr in TRIPLES}

            def nlmeans(spr, count=n):
                t, g = tables[spr]
                L.check(lib.demfi_payload_nlmeans(scratch.data_ptr(), Pb, work.data_ptr(), Pb, count, tab.ctypes.data, len(tab), es, depth, spr[1],
                                                  spr[2], t.ctypes.data, g, st), 'nlmeans')
            copy = lambda: scratch.copy_(src)                            # noqa: E731
            copy()
            nlmeans(TRIPLES[0], 1)
            torch.cuda.synchronize()
            exp = NL.nlmeans_payload_np(host[0], h, w, depth, layout, *TRIPLES[0], fields=fields)
            if not np.array_equal(work[0].cpu().numpy().view(host.dtype), exp):
                raise SystemExit('nlmeans_rate.py: the kernel differs from the definition at %s %s %d-bit' % (shape, layout, depth))
            rows = [('scratch copy', None, timed(copy, a.rounds, a.launches))]
            for spr in TRIPLES:
                rows.append(('payload_nlmeans %d:%d:%d' % spr, spr, timed(lambda: nlmeans(spr), a.rounds, a.launches)))
            deband = lambda: L.check(lib.demfi_payload_deband(scratch.data_ptr(), Pb, work.data_ptr(), Pb, n, tab.ctypes.data, len(tab), es,   # noqa: E731
                                                              depth, 2, 16, st), 'deband')
            rows.append(('payload_deband 2:16', None, timed(deband, a.rounds, a.launches)))
            for name, spr, (ms, lo, hi) in rows:
                rec = {'launch': name, 'shape': shape, 'layout': layout, 'depth': depth, 'payloads': n, 'size': '%dx%d' % (w, h),
                       'payload_bytes': Pb, 'ms_per_launch': round(ms, 4), 'ms_rounds': [round(lo, 4), round(hi, 4)],
                       'us_per_payload': round(1e3 * ms / n, 3), 'payload_GB_per_s': round(n * Pb / ms / 1e6, 2)}
                if spr is not None:
                    cand = n * P * (2 * spr[2] + 1) ** 2 / ms * 1e3
                    rec.update(candidates_per_s=float('%.4g' % cand), valu_per_candidate=VALU_PER_CANDIDATE[es, spr[1]],
                               valu_instructions_per_s=float('%.4g' % (cand * VALU_PER_CANDIDATE[es, spr[1]] / 64)))     # wave instructions
                    if a.bench_fps and (shape, layout, depth, spr) == ('720p', '420', 8, NL.DEFAULTS):
                        rec['share_of_a_720p_bench_frame'] = round(1e3 * ms / n / (1e6 / a.bench_fps), 4)
                out.append(rec)
                print(json.dumps(rec), flush=True)
            del src, work, scratch
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
