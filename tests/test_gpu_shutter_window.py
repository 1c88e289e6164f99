"""Weighted shutter windows (``--shutter-window``) on a real MI355X: ``demfi_payload_mix_w`` (csrc/shutter.hip) equal to
``shutter.mix_np(..., weights=...)`` byte for byte, and ``VideoRunner(shutter_window=..., down=...)`` byte-identical to an expectation that
never runs the new code: the fine stream a run WITHOUT the switches writes from the same input, mixed on the host.  The clips, the model
and the stream helpers are those of tests/test_gpu_shutter.py."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import shutter as SH                                                  # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_shutter as G                                              # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV, ERR_ARG, POISON = G.DEV, G.ERR_ARG, G.POISON


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _mix_w_gpu(src, rows, weights, P, es, shift, gap):
    """``test_gpu_shutter._mix_gpu`` for the weighted entry: ``src`` [m, P es] placed ``shift`` bytes behind a 16-byte boundary each, rows of
    indices into it (row r keeps its first len(rows[r]) samples, weighted by the first as many of ``weights``) -> the mixed rows; the poisoned
    bytes between the rows of dst and behind the last one come back untouched, and so do the sources."""
    lib, n, Pb, smax = L.load(), len(rows), P * es, len(weights)
    pitch = -(-Pb // 16) * 16 + 16
    buf = np.full(len(src) * pitch + 16, 0xEE, np.uint8)
    offs_src = [i * pitch + shift for i in range(len(src))]
    for o, p in zip(offs_src, src):
        buf[o:o + Pb] = p
    stride = Pb + gap
    table = np.full((n, smax), -1, np.int64)
    for r, ks in enumerate(rows):
        table[r, :len(ks)] = [offs_src[j] for j in ks]
    w = np.ascontiguousarray(weights, dtype=np.int32)
    dev = torch.from_numpy(buf).to(DEV)
    assert dev.data_ptr() % 16 == 0
    od = torch.from_numpy(table).to(DEV)
    dst = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_payload_mix_w(dev.data_ptr(), table.ctypes.data, od.data_ptr(), n, smax, P, es, dst.data_ptr(), stride, w.ctypes.data,
                                    torch.cuda.current_stream().cuda_stream), 'payload_mix_w')
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    body = out[:n * stride].reshape(n, stride)
    assert (body[:, Pb:] == POISON).all() and (out[n * stride:] == POISON).all(), 'write outside the payloads'
    assert np.array_equal(dev.cpu().numpy(), buf)
    return body[:, :Pb]


def _check_kernel(P, es, weights, n, shift, gap, seed=0):
    smax = len(weights)
    m = smax + 3
    src = G._sources(m, P, es, seed + P + smax)
    rows = G._rows(n, smax, m)                                           # full rows, truncated prefixes, rows of the all-peak source alone
    got = _mix_w_gpu(src, rows, weights, P, es, shift, gap)
    want = SH.mix_np(src, rows, es, [list(weights[:len(ks)]) for ks in rows])
    diff = int((got != want).sum())
    print('P=%d es=%d w=%s.. n=%d shift=%d gap=%d: %d of %d bytes differ' % (P, es, list(weights[:5]), n, shift, gap, diff, want.size))
    assert np.array_equal(got, want)
    peak_rows = [r for r, ks in enumerate(rows) if set(ks) == {m - 1}]
    assert all((got[r] == 0xFF).all() for r in peak_rows) and (peak_rows or n < 5)     # the accumulator bound: W x 65535 averages to the peak


def _heavy(smax):
    """A weight vector of sum 4096, the most the entry takes."""
    return [4096 - (smax - 1)] + [1] * (smax - 1)


@pytest.mark.parametrize('es', [1, 2], ids=['bytes', '16-bit'])
@pytest.mark.parametrize('P', [1, 15, 16, 17, 33, 4099, 64 * 96 * 3 // 2])
def test_kernel_equals_the_numpy_definition(P, es):
    """Aligned sources, dst and stride take the 16-byte path (with its sample-by-sample tail when P es is no multiple of 16); sources at odd
    byte offsets (2 mod 16 for 16-bit samples) and an odd stride take the sample-by-sample path.  Row 9 of 37 at S = 32 is the all-peak
    source 32 times under the triangle."""
    for smax in (1, 2, 5, 32):
        for weights in (SH.window_weights('triangle', smax), _heavy(smax)):
            for n in (1, 37):
                _check_kernel(P, es, weights, n, 0, 32 + -(P * es) % 16)     # the vector path: the gap makes the stride a multiple of 16
                _check_kernel(P, es, weights, n, 1 if es == 1 else 2, 3 if es == 1 else 6)
    _check_kernel(P, es, [1, 2, 3, 2, 1], 3, 0, 8)                       # aligned sources, a stride that is not: sample by sample


def test_unit_weights_give_the_bytes_of_the_box_entry():
    src = G._sources(8, 4099, 2, 5)
    rows = G._rows(11, 5, 8)
    assert np.array_equal(_mix_w_gpu(src, rows, [1] * 5, 4099, 2, 0, 32 + -(4099 * 2) % 16), G._mix_gpu(src, rows, 5, 4099, 2, 0, 32 + -(4099 * 2) % 16))


def test_rows_beyond_one_grid():
    _check_kernel(1, 1, [7], 4099, 0, 16)                                # more rows than the grid has: rows are strided over
    _check_kernel(3, 2, [1, 2, 1], 4099, 2, 6)


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((64,), POISON, dtype=torch.uint8, device=DEV)
    table = np.array([[0, 32, -1], [64, -1, -1]], np.int64)
    od = torch.from_numpy(table).to(DEV)
    w = np.array([1, 2, 1], np.int32)
    fn = lib.demfi_payload_mix_w
    ok = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, 3, 16, 1, dst.data_ptr(), 32, w.ctypes.data, st)

    def bad(i, v, tab=None):
        a = list(ok)
        a[i] = v
        if tab is not None:
            a[1] = tab.ctypes.data
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 2, 7, 9))                    # NULL buffers, the weights among them
    for ws in ([1, 0, 1], [1, -1, 1], [4095, 1, 1], [1, 1, 4095], [4097, 1, 1], [2 ** 31 - 1, 2 ** 31 - 1, 2]):
        assert bad(9, np.array(ws, np.int32).ctypes.data), ws            # a weight below 1; a sum of 4097 and more
    assert b'demfi_payload_mix_w' in lib.demfi_last_error()
    assert all(bad(4, v) for v in (0, 33, -1)) and all(bad(6, v) for v in (0, 3, 4)) and bad(5, 0) and bad(8, 15)   # the box entry's cases
    for tab in ([[0, 32, -1], [-1, -1, -1]], [[0, -1, 32], [64, -1, -1]], [[0, 32, -2], [64, -1, -1]]):
        assert bad(3, 2, np.array(tab, np.int64))                        # a row that keeps nothing; a kept offset behind a -1; a bad offset
    odd = np.array([[1, -1, -1], [64, -1, -1]], np.int64)
    a = list(ok)
    a[1], a[5], a[6] = odd.ctypes.data, 8, 2                             # 16-bit samples at an odd address
    assert fn(*a) == ERR_ARG
    a = list(ok)
    a[5], a[6], a[8] = 8, 2, 17                                          # and at an odd stride
    assert fn(*a) == ERR_ARG
    for n in (0, -3):                                                    # no row: nothing to do, nothing written
        a = list(ok)
        a[3] = n
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    heavy = np.array([4094, 1, 1], np.int32)                             # a sum of exactly 4096 is taken
    a = list(ok)
    a[9] = heavy.ctypes.data
    assert fn(*a) == 0 and fn(*ok) == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:16] == 0xA5).all() and (out[32:48] == 0xA5).all() and (out[16:32] == POISON).all() and (out[48:] == POISON).all()
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _clip(n, fps):
    return Y._clip(n, 48, 80, '420', 8, fps=fps, seed=3)[0]


@pytest.fixture(scope='module')
def clip60():
    return _clip(13, b'60:1')


@pytest.fixture(scope='module')
def clip24():
    return _clip(11, b'24:1')


def _mixed(fine_pays, data, fps_out, s, d, window, full=False):
    """The expectation: the fine payloads mixed on the host under the window's weights; the header of the stream at F_out."""
    hdr = y4m.parse_header(data[:data.index(b'FRAME\n')], y4m.DEPTHS, y4m.LAYOUTS)
    n, r = data.count(b'FRAME\n'), Fraction(fps_out) / hdr.fps
    n_out = R.n_output_frames(n, r, full)
    assert len(fine_pays) >= R.n_output_frames(n, r * d, full)
    fine_pays = fine_pays[:R.n_output_frames(n, r * d, full)]
    groups = SH.groups(len(fine_pays), n_out, s, d)
    x = np.stack([np.frombuffer(p, np.uint8) for p in fine_pays])
    out = SH.mix_np(x, groups, 1, SH.group_weights(groups, d, SH.window_weights(window, s)))
    return R.output_header(hdr, Fraction(fps_out)).encode() + b''.join(b'FRAME\n' + p.tobytes() for p in out), groups


def _instants(n, fine, s, d, full=False):
    """(the instants ``filter_plan`` leaves of the windows of an n-frame clip without cuts at the fine ratio, the windows it leaves nothing)."""
    k0, nw, total, skipped = R.first_window(n, full), R.n_windows(n, full), 0, 0
    for k in range(k0, k0 + nw):
        ts, o = R.window_plan(k, fine, k == k0 + nw - 1, full)
        runs = SH.filter_plan([(None, ts)] if ts else [], [(i, 0, kind, j) for i, kind, j in o], s, d)[0]
        total += sum(len(t) for _, t in runs)
        skipped += not runs
    return total, skipped


@pytest.fixture(scope='module')
def fine_60_to_24(model16, clip60):
    """The fine stream of 60 -> 24 at 180 degrees of four samples (D = 8, R = 16/5): a run without either switch at 192 frames/s."""
    return D._split(G._run(model16, clip60, fps=Fraction(192))[3])[1]


@pytest.mark.parametrize('window', ['box', 'triangle'])
def test_a_down_rate_shutter_equals_the_mix_of_the_fine_stream(window, model16, clip60, fine_60_to_24):
    exp, groups = _mixed(fine_60_to_24, clip60, 24, 4, 8, window)
    assert len(groups) == 5 and [len(g) for g in groups] == [4, 4, 4, 4, 1]
    for batch, pipe in ((4, False), (1, True), (3, False)):
        vr, nw, nf, got = G._run(model16, clip60, batch=batch, pipe=pipe, fps=Fraction(24), down=True, shutter=180, shutter_window=window)
        Y._same(got, exp)
        assert (nw, nf) == (10, 5) and vr.last_shutter == (4, 8) and vr.last_shutter_window == window and vr.last_fps_out == 24
        assert vr.last_st_frames == sum(map(len, groups))
        assert (vr.last_instants[0], vr.last_windows_skipped) == _instants(13, Fraction(16, 5), 4, 8) == (15, 3)
    if window == 'triangle':
        assert exp != _mixed(fine_60_to_24, clip60, 24, 4, 8, 'box')[0]


def test_a_triangle_without_a_down_rate(model16, clip24):
    """24 -> 60 at 360 degrees of four samples (D = 4: the fine stream is x10), full groups, truncated ones at the end, groups carried."""
    fine = D._split(G._run(model16, clip24, fps=Fraction(240))[3])[1]
    exp, groups = _mixed(fine, clip24, 60, 4, 4, 'triangle')
    box = G._run(model16, clip24, batch=3, fps=Fraction(60), shutter=360)
    assert box[3] == _mixed(fine, clip24, 60, 4, 4, 'box')[0] != exp
    for batch in (4, 1):
        vr, nw, nf, got = G._run(model16, clip24, batch=batch, fps=Fraction(60), shutter=360, shutter_window='triangle')
        Y._same(got, exp)
        assert nf == len(groups) == 21 and vr.last_shutter_window == 'triangle' and vr.last_windows_skipped == 0
    # the box by name: the bytes and the launch counters of a run without the switch
    vr, nw, nf, got = G._run(model16, clip24, batch=3, fps=Fraction(60), shutter=360, shutter_window='box')
    assert got == box[3] and vr.last_shutter_window == 'box' == box[0].last_shutter_window
    assert (vr.last_instants, vr.last_st_frames, vr.last_shutter_carried) == (box[0].last_instants, box[0].last_st_frames, box[0].last_shutter_carried)


def test_a_fine_ratio_below_one(model16, clip60):
    """60 -> 6 at 360 degrees of two samples: (S, D) = (2, 2), r = 1/10, R = 1/5.  The fine stream is every fifth frame of the run at the
    ratio R m = 1 (m = 5), which runs today."""
    m = math.ceil(1 / Fraction(1, 5))
    plain = D._split(G._run(model16, clip60, fps=Fraction(60))[3])[1]
    for window in ('box', 'triangle'):                                   # two samples: the triangle is the box
        exp, groups = _mixed(plain[::m], clip60, 6, 2, 2, window)
        assert groups == [[0, 1], [2]]
        for batch in (4, 1):
            vr, nw, nf, got = G._run(model16, clip60, batch=batch, fps=Fraction(6), down=True, shutter=360, shutter_samples=2, shutter_window=window)
            Y._same(got, exp)
            assert (nw, nf) == (10, 2) and vr.last_instants[0] == 3 and vr.last_windows_skipped == 7
