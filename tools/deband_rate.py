"""The rate of the ``demfi_payload_deband`` launch (``--deband``) at R = 4, 8 and 16 with T = 2, of the device copy into the scratch buffer
that the stage makes in front of it, and of ``demfi_payload_dering`` and ``demfi_payload_deblock`` over the same payloads in the same process
as yardsticks: payload bytes per second, microseconds per payload and, for the debanding launch, tap evaluations per second (samples times
(2R + 1)^2: the windows clipped at the borders are counted whole), device events around every launch.  The figures of profiles/deband.md
come from this script.

    python tools/deband_rate.py [--payloads 8] [--rounds 5] [--launches 10] [--shapes 576i,720p,1080p] [--out FILE]

Shapes: 576i (720 x 576, filtered by fields), 720p and 1080p, each as 8-bit 4:2:0 and 10-bit 4:2:2.  The deblocker works in place, so each
of its launches starts from a fresh device copy of the input (made outside the events); the others read the input and write elsewhere.
The input is that of the GPU tests (promoted ramps, texture, hard edges).  Before the timing one payload of every shape is compared with
``deband.deband_payload_np``, whole, at 2:4 (the definition makes (2R + 1)^2 passes over the payload in numpy: at R = 16 that is a minute
a shape; the radii share one kernel body that differs in its unrolled trip counts, and the GPU tests hold every radius to the definition).
Needs a GPU; fails without one."""
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
from demfi_amd import deband as BA                                       # noqa: E402
from demfi_amd import deblock as DB                                      # noqa: E402
from demfi_amd import dering as DR                                       # noqa: E402
from demfi_amd import y4m                                                # noqa: E402
from tests.test_deband import banded_payload                             # noqa: E402

SHAPES = {'576i': (576, 720, 't'), '720p': (720, 1280, None), '1080p': (1080, 1920, None)}
RADII, T = (4, 8, 16), 2


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
    ap.add_argument('--payloads', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--shapes', default='576i,720p,1080p')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('deband_rate.py: no GPU visible')
    lib, dev, st = L.load(), 'cuda:0', torch.cuda.current_stream().cuda_stream
    n, out = a.payloads, []
    nothing = lambda: None                                               # noqa: E731
    for shape in a.shapes.split(','):
        h, w, fields = SHAPES[shape]
        for layout, depth in (('420', 8), ('422', 10)):
            es, P = (1 if depth == 8 else 2), y4m.payload_size(h, w, layout)
            Pb = P * es
            host = np.stack([banded_payload(h, w, layout, depth, s, fields) for s in range(2)])
            src = torch.from_numpy(host.view(np.uint8).reshape(len(host), Pb)).to(dev).repeat(-(-n // len(host)), 1)[:n].contiguous()
            work, scratch = torch.empty_like(src), torch.empty_like(src)
            tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields), dtype=np.int64)

            def deband(r, count=n):
                L.check(lib.demfi_payload_deband(scratch.data_ptr(), Pb, work.data_ptr(), Pb, count, tab.ctypes.data, len(tab), es, depth, T, r,
                                                 st), 'deband')
            copy = lambda: scratch.copy_(src)                            # noqa: E731
            copy()
            deband(4, 1)
            torch.cuda.synchronize()
            exp = BA.deband_payload_np(host[0], h, w, depth, layout, T, 4, fields=fields)
            if not np.array_equal(work[0].cpu().numpy().view(host.dtype), exp):
                raise SystemExit('deband_rate.py: the kernel differs from the definition at %s %s %d-bit' % (shape, layout, depth))
            rows = [('scratch copy', None, None, timed(copy, nothing, a.rounds, a.launches))]
            for r in RADII:
                rows.append(('payload_deband %d:%d' % (T, r), r, None, timed(lambda: deband(r), nothing, a.rounds, a.launches)))
            # the yardsticks over the same payloads: the deringing filter out of place, the deblocker in place
            dering = lambda: L.check(lib.demfi_payload_dering(scratch.data_ptr(), Pb, work.data_ptr(), Pb, n, tab.ctypes.data, len(tab), es,   # noqa: E731
                                                              depth, *DR.DEFAULTS, st), 'dering')
            rows.append(('payload_dering %d:%d:%d' % DR.DEFAULTS, None, None, timed(dering, nothing, a.rounds, a.launches)))
            thr = DB.thresholds(depth)
            restore = lambda: work.copy_(src)                            # noqa: E731
            deblock = lambda: L.check(lib.demfi_payload_deblock(work.data_ptr(), Pb, n, tab.ctypes.data, len(tab), es, *thr, st), 'deblock')   # noqa: E731
            rows.append(('payload_deblock 16:4', None, None, timed(deblock, restore, a.rounds, a.launches)))
            for name, r, _, (ms, lo, hi) in rows:
                rec = {'launch': name, 'shape': shape, 'layout': layout, 'depth': depth, 'payloads': n, 'size': '%dx%d' % (w, h),
                       'payload_bytes': Pb, 'ms_per_launch': round(ms, 4), 'ms_rounds': [round(lo, 4), round(hi, 4)],
                       'us_per_payload': round(1e3 * ms / n, 3), 'payload_GB_per_s': round(n * Pb / ms / 1e6, 2),
                       'taps_per_s': None if r is None else float('%.4g' % (n * P * (2 * r + 1) ** 2 / ms * 1e3))}
                out.append(rec)
                print(json.dumps(rec), flush=True)
            del src, work, scratch
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
