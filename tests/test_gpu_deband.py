"""The debanding filter in front of the network (``--deband``) on a real MI355X: ``demfi_payload_deband`` (csrc/deband.hip) equal to
``deband.deband_payload_np`` byte for byte, out of place, inside poisoned guard bytes with the source untouched, and
``VideoRunner(deband=...)`` byte-identical to an expectation that never runs the new kernel: the same runner WITHOUT ``deband`` on the
stream debanded on the host with ``deband_stream_np``.  The inputs are ``banded_payload``, ``banded_clip`` and ``count_payload`` of
tests/test_deband.py, which proves there that they cover the rule; model and helpers are those of the neighbouring files.  The kernel's
tile is 64 x 32 samples; tiles within R of a plane border take another path than those inside."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fractions import Fraction                                                       # noqa: E402

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import bitdepth as BD                                                 # noqa: E402
from demfi_amd import deband as BA                                                   # noqa: E402
from demfi_amd import deblock as DB                                                  # noqa: E402
from demfi_amd import dering as DR                                                   # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402
from tests.test_deband import banded_clip, banded_payload, count_payload             # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD, SRC_GUARD = 0xC7, 0x5B


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _launch(pays, h, w, depth, layout, fields=None, rect=None, tr=BA.DEFAULTS, lead=0, gap=0, table=None):
    """``pays``: payloads (1-D sample arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes, source and
    destination alike but with different strides -> the destination payloads after ONE demfi_payload_deband launch over all of them.
    Every byte before, between and behind the destination payloads is intact and the source buffer is unchanged."""
    es, pb, n = pays[0].itemsize, pays[0].nbytes, len(pays)
    stride, sstride = pb + gap, pb + 2 * gap + 16 * es
    src = np.full(lead + n * sstride + 64, SRC_GUARD, np.uint8)
    for i, p in enumerate(pays):
        src[lead + i * sstride:lead + i * sstride + pb] = p.view(np.uint8)
    dev_src = torch.from_numpy(src).to(DEV)
    dev = torch.full((lead + n * stride + 64,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields, rect) if table is None else table, dtype=np.int64)
    L.check(L.load().demfi_payload_deband(dev_src.data_ptr() + lead, sstride, dev.data_ptr() + lead, stride, n, tab.ctypes.data, len(tab), es,
                                          depth, *tr, torch.cuda.current_stream().cuda_stream), 'payload_deband')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert np.array_equal(dev_src.cpu().numpy(), src), 'the source changed'
    assert (out[:lead] == GUARD).all() and (out[lead + max(n - 1, 0) * stride + (pb if n else 0):] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(pays[0].dtype) for i in range(n)]


def _check_launch(pays, h, w, depth, layout, fields=None, rect=None, tr=BA.DEFAULTS, **kw):
    got = _launch(pays, h, w, depth, layout, fields, rect, tr, **kw)
    assert len(got) == len(pays)
    for i, (g, p) in enumerate(zip(got, pays)):
        exp = BA.deband_payload_np(p, h, w, depth, layout, *tr, fields, rect)
        bad = np.flatnonzero(g != exp)
        assert bad.size == 0, ('%dx%d %s depth %d fields=%r rect=%r %r payload %d: %d of %d samples differ'
                               % (w, h, layout, depth, fields, rect, tr, i, bad.size, exp.size), bad[:10], g[bad[:10]], exp[bad[:10]])


FORMATS = [(8, np.uint8), (8, np.uint16), (10, np.uint16), (16, np.uint16)]
FORMAT_IDS = ['bytes', '8-bit-in-16', '10-bit', '16-bit']
# luma sizes (w, h): below, at and above one window of R = 16; at and either side of the tile of 64 x 32; two and three tiles each way
SIZES = [(2, 2), (7, 5), (16, 16), (33, 33), (34, 35), (63, 31), (64, 32), (65, 33), (96, 64), (150, 90)]
RADII, THRESHOLDS = (1, 2, 7, 16), (1, 2, 8)
PAIRS = [(t, r) for r in RADII for t in THRESHOLDS]


def _lead_gap(dtype, k):
    """Strides wider than the payload; every other case off a 16-byte boundary (odd for bytes, even for 16-bit samples)."""
    es = np.dtype(dtype).itemsize
    return (dict(lead=0, gap=16), dict(lead=3 * es, gap=5 * es))[k & 1]


@pytest.mark.parametrize('depth,dtype', FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize('fields', [None, 't'], ids=['progressive', 'fields'])
def test_kernel_equals_the_numpy_definition(fields, depth, dtype):
    """Every size in every layout, two payloads a launch; the twelve (T, R) pairs take turns in steps of 7 from a start the format gives
    (7 and 12 have no common factor, so the 40 cases of every format meet every pair more than once)."""
    k, fmt = 0, FORMATS.index((depth, dtype))
    for w, h in SIZES:
        for layout in y4m.LAYOUTS:
            pays = [banded_payload(h, w, layout, depth, 1000 * k + i, fields, dtype=dtype) for i in range(2)]     # two payloads in one launch
            _check_launch(pays, h, w, depth, layout, fields, tr=PAIRS[(7 * k + fmt) % 12], **_lead_gap(dtype, k))
            k += 1


@pytest.mark.parametrize('t,r', PAIRS, ids=['%d:%d' % p for p in PAIRS])
def test_every_radius_and_threshold(t, r):
    """Three tiles each way at 10 bits, 4:2:0 (chroma planes of 75 x 45: a tile and a ragged one) and a plane of exactly one window."""
    _check_launch([banded_payload(90, 150, '420', 10, 40 + r)], 90, 150, 10, '420', None, None, (t, r), lead=6, gap=10)
    s = 2 * r + 1
    _check_launch([banded_payload(s, s, 'mono', 8, 50 + r)], s, s, 8, 'mono', None, None, (t, r), lead=1, gap=3)


def test_every_radius_at_the_default_threshold():
    for r in range(1, 17):                                                # 200 x 100: one tile of the six lies inside at every radius
        _check_launch([banded_payload(100, 200, 'mono', 10, r)], 100, 200, 10, 'mono', None, None, (2, r), **_lead_gap(np.uint16, r))


@pytest.mark.parametrize('depth,dtype', FORMATS, ids=FORMAT_IDS)
def test_every_n_and_both_extremes_of_the_numerator(depth, dtype):
    """``count_payload``: centres that see exactly n near samples at c + thr - 1 and at c - (thr - 1): every n for R = 1, 2, 4; for
    R = 16, n = 1, 2, 1088, 1089 and one in every 64 between.  The division by 2 n is exact at each."""
    for r in (1, 2, 4, 16):
        for t in (1, 2, 8):
            pay, h, w, centres = count_payload(depth, t, r, dtype)
            got = _launch([pay], h, w, depth, 'mono', tr=(t, r), lead=2 * pay.itemsize, gap=6)[0]
            exp = BA.deband_payload_np(pay, h, w, depth, 'mono', t, r)
            assert np.array_equal(got, exp)
            thr = t << (depth - 8)
            for y, x, n, sign in centres:                                 # and by hand: c + floor((2 (n - 1) s (thr - 1) + n) / 2 n)
                c = int(pay[y * w + x])
                assert int(got[y * w + x]) == c + (2 * (n - 1) * sign * (thr - 1) + n) // (2 * n), (r, t, n, sign)


def test_full_range_16_bit_samples_near_0_and_65535():
    g = np.random.RandomState(2)
    h, w = 70, 100
    for k, (t, r) in enumerate(((8, 16), (1, 16), (8, 3), (2, 7))):
        thr = t << 8
        top = np.where(g.randint(0, 2, (h, w)) > 0, 65535 - g.randint(0, thr, (h, w)), g.randint(0, thr, (h, w)))
        top[20:40, 30:70] = 65535
        top[50:60, 10:50] = 0
        _check_launch([top.reshape(-1).astype(np.uint16)], h, w, 16, 'mono', None, None, (t, r), **_lead_gap(np.uint16, k))
    # any stored bits of a 16-bit container are samples: 0xffff at depth 10 next to ordinary ones
    pay = banded_payload(40, 72, 'mono', 10, 9)
    pay[g.randint(0, pay.size, 200)] = 0xFFFF
    pay[g.randint(0, pay.size, 200)] = g.randint(1024, 65536, 200)
    _check_launch([pay], 40, 72, 10, 'mono', None, None, (8, 16), lead=2, gap=6)


def test_phases_are_carried_and_ignored():
    h, w = 46, 150
    for k, (top, left) in enumerate(((4, 6), (6, 14))):
        for fields in (None, 'b'):
            if fields is not None and top % 4:
                continue
            rect = (top, top + h, left, left + w)
            pays = [banded_payload(h, w, '420', 10, 50 + k, fields, rect) for _ in range(2)]
            got = _launch(pays, h, w, 10, '420', fields, rect, (2, 7), **_lead_gap(np.uint16, k))
            for g, p in zip(got, pays):
                assert np.array_equal(g, BA.deband_payload_np(p, h, w, 10, '420', 2, 7, fields))       # the table without the rectangle


def test_the_identity_n_0_and_three_and_forty_payloads_in_one_launch():
    pays = [banded_payload(40, 72, '420', 8, 7 + i) for i in range(40)]
    _check_launch(pays[:3], 40, 72, 8, '420', tr=(2, 4), lead=3, gap=21)
    _check_launch(pays, 40, 72, 8, '420', tr=(2, 4), lead=3, gap=21)
    _check_launch([p.astype(np.uint16) << 8 for p in pays[:3]], 40, 72, 16, '420', 't', tr=(2, 16), lead=16, gap=48)
    # T = 0 through the entry point: every sample written, none changed
    one = [banded_payload(45, 100, '422', 8, 5)]
    assert np.array_equal(_launch(one, 45, 100, 8, '422', tr=(0, 16), gap=7)[0], one[0])
    # n = 0: a success that launches and writes nothing
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), SRC_GUARD, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    assert lib.demfi_payload_deband(src.data_ptr(), 360, dst.data_ptr(), 360, 0, tab.ctypes.data, 3, 1, 8, 2, 16, st) == 0
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((src == SRC_GUARD).all())


def test_samples_no_entry_names_are_copied():
    """A table of the luma plane alone over 4:2:0 payloads whose last chroma sample it still reaches through a one-sample entry: the chroma
    planes arrive in dst as they are."""
    h, w = 24, 40
    g = np.random.RandomState(31)
    pays = [banded_payload(h, w, '420', 8, 31 + i) for i in range(2)]
    for p in pays:                                                        # a luma plane the filter is sure to change: texture within T
        p[:h * w] = 128 + g.randint(-3, 4, h * w)
    table = [DB.plane_table(h, w, '420')[0], (pays[0].size - 1, 1, 1, 1, 0, 0)]
    got = _launch(pays, h, w, 8, '420', tr=(8, 5), table=table, lead=1, gap=9)
    for g, p in zip(got, pays):
        exp = p.copy()
        exp[:h * w] = BA.deband_plane_np(p[:h * w].reshape(h, w), 8, 8, 5).reshape(-1)
        assert np.array_equal(g, exp) and not np.array_equal(g[:h * w], p[:h * w])


def test_a_576i_point_by_fields():
    """Many tiles, most of them inside; 3:6 keeps the definition's 169 passes over the payload within a second or two."""
    h, w = 576, 720
    pays = [banded_payload(h, w, '420', 10, 11, 't')]
    got = _launch(pays, h, w, 10, '420', 't', tr=(3, 6), lead=16, gap=32)
    exp = BA.deband_payload_np(pays[0], h, w, 10, '420', 3, 6, fields='t')
    assert np.array_equal(got[0], exp) and (exp != pays[0]).mean() > 0.2


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    fn = lib.demfi_payload_deband
    ok = [src.data_ptr(), 360, dst.data_ptr(), 360, 2, tab.ctypes.data, 3, 1, 8, 2, 16, st]

    def bad(i, v, table=None, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        if table is not None:
            a[5] = table.ctypes.data
        return fn(*a) == ERR_ARG

    def t(p, c, v):
        x = tab.copy()
        x[p, c] = v
        return x
    assert bad(0, None) and bad(2, None) and bad(5, None) and bad(4, -1)
    assert bad(7, 0) and bad(7, 3) and bad(6, 0) and bad(6, 7) and bad(8, 9) and bad(8, 10)
    assert bad(5, 0, t(0, 1, 0)) and bad(5, 0, t(0, 2, 16385)) and bad(5, 0, t(1, 3, 9)) and bad(5, 0, t(2, 4, 8)) and bad(5, 0, t(2, 5, -1))
    assert bad(1, 359) and bad(3, 359) and bad(0, src.data_ptr() + 1, _7=2, _1=720, _3=720) and bad(3, 721, _7=2, _1=720)
    assert bad(9, -1) and bad(9, 9) and bad(10, 0) and bad(10, 17)
    assert bad(2, src.data_ptr()) and bad(2, src.data_ptr() + 100) and bad(2, src.data_ptr(), _9=0)   # in place, overlapping
    assert b'demfi_payload_deband' in lib.demfi_last_error()
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((src == 0xA5).all())
    assert fn(*ok) == 0                                                   # flat payloads stay flat, and are written
    torch.cuda.synchronize()
    assert bool((dst[:720] == 0xA5).all()) and bool((dst[720:] == GUARD).all()) and bool((src == 0xA5).all())
    assert L.ABI_VERSION == 8                                             # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _host(data, fn, *args, rect=None):
    """The stream ``data`` through the stream function ``fn`` of a stage on the host, payload by payload (an interlaced one field by
    field), header untouched."""
    hdr, pays = D._parse(data)
    smp = [np.frombuffer(p, _dtype(hdr.depth)) for p in pays]
    fields = hdr.interlace if hdr.interlace in ('t', 'b') else None
    outs = fn(smp, hdr.h, hdr.w, hdr.depth, hdr.layout, *args, fields, rect)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + o.tobytes() for o in outs)


def _debanded(data, tr=BA.DEFAULTS):
    return _host(data, BA.deband_stream_np, *tr)


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')

    def seekable(self):
        return False


def _run(model, data, batch=4, pipe=False, **kw):
    vr = VideoRunner(model, 1, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(_Pipe(data) if pipe else io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


ON = dict(deband=True)


def _check(model, data, batch=4, pipe=False, host=None, on=ON, **kw):
    """``VideoRunner(..., deband=..., **kw)`` on ``data`` == the same runner WITHOUT ``deband`` on the stream debanded on the host
    (``host``: that stream and the switches it runs with, where they differ), header, counts, cuts and instants included."""
    prog, hkw = (_debanded(data), kw) if host is None else host
    ve, nwe, nfe, exp = _run(model, prog, batch, **hkw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **on, **kw)
    assert (nw, nf) == (nwe, nfe) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_cut_windows, vr.last_dups) == (ve.last_instants, ve.last_st_frames, ve.last_cuts,
                                                                                                     ve.last_cut_windows, ve.last_dups)
    assert vr.last_debanded > 0 and ve.last_debanded == 0
    return vr, got


def _probe(monkeypatch, calls):
    """Every ``demfi_payload_deband`` launch from here on appends its payload count to ``calls``."""
    lib = L.load()
    real = lib.demfi_payload_deband
    monkeypatch.setattr(lib, 'demfi_payload_deband', lambda *a: (calls.append(a[4]), real(*a))[1])


@pytest.fixture(scope='module')
def clip8():
    return banded_clip(7, 64, 96, '420', 8, seed=3)[0]


def test_work_depth_10_on_an_8_bit_input_every_frame_once_and_the_ramps_step_by_one(model16, clip8, monkeypatch):
    """What the switch is for: host promote, then host deband at 10 bits, then the ``high_depth`` run."""
    n = 7
    host = _debanded(BD.promote_stream_np(clip8, 10))
    kw = dict(mfi=2, work_depth=10, out_depth=10)
    vr, got = _check(model16, clip8, batch=2, host=(host, dict(mfi=2, high_depth=True)), **kw)
    assert vr.last_depths == (8, 10, 10, None) and vr.last_depth_promoted == vr.last_debanded == n and b' C420p10' in got[:80]
    assert vr.deband == (2, 16) and len(D._parse(got)[1]) == R.n_output_frames(n, 2)
    plain = _run(model16, clip8, 2, **kw)[3]
    assert len(plain) == len(got) and plain != got
    for batch in (1, 3):                                                  # batches of one and several
        assert _run(model16, clip8, batch, **kw, **ON)[3] == got
    # ONE launch per run of consecutive newly uploaded slots
    calls = []
    _probe(monkeypatch, calls)
    out = io.BytesIO()
    vr.run_stream(io.BytesIO(clip8), out)
    assert out.getvalue() == got and sum(calls) == n and len(calls) < n
    # the stage's own output: where the promoted input steps by 4 over plateaus 16 to 32 wide, the debanded payload steps by at most 1
    hdr, pays = D._parse(BD.promote_stream_np(clip8, 10))
    src = np.frombuffer(pays[0], np.uint16)
    dev = _launch([src], hdr.h, hdr.w, 10, '420')[0]
    assert np.array_equal(dev, np.frombuffer(D._parse(host)[1][0], np.uint16))


def test_ramps_through_the_kernel_step_by_at_most_one_code():
    """Done when: a 10-bit stream whose ramps step by at most one code where the 8-bit input's plateaus are 16 to 32 samples wide; here
    on the stage's own output, the promoted ramp through the kernel."""
    h, w = 80, 300
    yy, xx = np.mgrid[0:h, 0:w]
    for width in (16, 24, 32):
        v8 = np.round(xx / width + 50).astype(np.uint8)
        up = (v8.astype(np.uint16) << 2).reshape(-1)
        out = _launch([up], h, w, 10, 'mono', lead=4, gap=12)[0].reshape(h, w).astype(np.int64)[16:-16, 16:-16]
        dx = np.diff(out, axis=1)
        assert np.diff(up.reshape(h, w).astype(np.int64), axis=1).max() == 4 and dx.min() >= 0 and dx.max() <= 1 and not np.diff(out, axis=0).any()


def test_a_10_bit_stream_fps_a_pipe_full_length_and_a_scene_cut(model16, clip8):
    data = banded_clip(6, 48, 80, '420', 10, seed=5, fps=b'25:1')[0]
    vr, got = _check(model16, data, fps=Fraction(60), high_depth=True)
    assert vr.last_fps_out == 60 and vr.last_depth == 10 and b' C420p10' in got[:80]
    vr, exp = _check(model16, clip8, batch=2, pipe=True, mfi=2)
    assert vr.last_decode_peak <= 2 + 5                                   # no look-ahead: what a run without the switch holds
    vr, exp = _check(model16, clip8, batch=3, mfi=2, full_length=True)
    assert len(D._parse(exp)[1]) == 7 * 2 and _run(model16, clip8, 1, mfi=2, full_length=True, **ON)[3] == exp
    # two scenes: the cut is found at the same frame
    from demfi_amd import scene as S
    head, a = banded_clip(1, 64, 96, '420', 8, seed=1)
    b = banded_clip(1, 64, 96, '420', 8, seed=2)[1]
    g = np.random.RandomState(0)
    pays = [np.clip((a[0] if f < 4 else (255 - b[0]) // 3).astype(np.int64) + g.randint(-1, 2, a[0].size), 0, 255).astype(np.uint8) for f in range(8)]
    cut = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    vr, got = _check(model16, cut, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [4] and vr.last_cut_windows >= 1


def test_with_dedup_repeats_stay_repeats(model16):
    head, p = banded_clip(6, 48, 80, '420', 8, seed=6)
    pays = [p[0], p[0], p[1], p[2], p[2], p[3], p[4], p[5]]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + x.tobytes() for x in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, full_length=True, dedup=True)
    assert vr.last_dups == [1, 4] and vr.last_debanded == len(pays)


@pytest.mark.parametrize('mode', ['bob', 'adaptive'])
def test_under_deinterlace_every_field_is_a_plane_of_its_own(mode, model16):
    n = 6
    data = D._interlaced(banded_clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], 't')
    kw = dict(mfi=2, deinterlace=True, deinterlace_mode=mode)
    vr, got = _check(model16, data, on=dict(deband=(2, 5)), host=(_debanded(data, (2, 5)), kw), **kw)
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_debanded == 2 * n        # a payload is uploaded once per field
    assert got != _run(model16, data, **kw)[3]
    as_frames = _debanded(D._retag(data, b't', b'p'), (2, 5))             # filtered as woven frames: not what the rule asks for
    assert got != _run(model16, D._retag(as_frames, b'p', b't'), **kw)[3]


@pytest.mark.parametrize('layout,depth', [('422', 8), ('444', 8), ('mono', 8), ('422', 10)])
def test_any_layout(layout, depth, model16):
    data = banded_clip(6, 48, 80, layout, depth, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, layouts=True, high_depth=depth > 8)
    assert (vr.last_depth, vr.last_layout) == (depth, layout)


def test_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data = banded_clip(6, h, w, '420', 8, seed=4)[0]
    vr, got = _check(model16, data, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def _cropped(data, rect):
    """The stream cropped to ``rect`` on the host: header of the rectangle's size, payloads through ``letterbox.crop_payload_np``."""
    hdr, pays = D._parse(data)
    t, b, l, r = rect
    head = data[:data.index(b'FRAME\n')].replace(b' W%d ' % hdr.w, b' W%d ' % (r - l)).replace(b' H%d ' % hdr.h, b' H%d ' % (b - t))
    return head + b''.join(b'FRAME\n' + LB.crop_payload_np(np.frombuffer(p, _dtype(hdr.depth)), hdr.h, hdr.w, hdr.depth, hdr.layout, rect).tobytes()
                           for p in pays)


def test_behind_a_crop_the_window_stops_at_the_cropped_plane(model16):
    h, w, bars = 80, 112, (4, 4, 6, 2)
    rect = LB.bars_rect(bars, h, w)
    data = banded_clip(6, h, w, '420', 8, seed=6, fps=b'25:1')[0]
    host = _debanded(_cropped(data, rect))
    vr, got = _check(model16, data, crop=bars, crop_output='cropped', host=(host, dict(mfi=2)), mfi=2)
    assert vr.last_crop == rect and got.startswith(b'YUV4MPEG2 W104 H72 ')


def test_behind_deblock_and_dering_in_front_of_the_denoiser_the_scaler_and_the_grain(model16, clip8):
    """deblock -> dering -> deband on the host is the expectation's input; everything behind is the expectation's own."""
    host = _debanded(_host(_host(clip8, DB.deblock_stream_np, 16, 4), DR.dering_stream_np, *DR.DEFAULTS))
    kw = dict(mfi=4, denoise=True, scale=(80, 48), grain=2)
    vr, got = _check(model16, clip8, batch=2, on=dict(deband=True, dering=True, deblock=True), host=(host, kw), **kw)
    assert b' W80 H48 ' in got[:40] and vr.last_denoised == vr.last_deblocked == vr.last_deringed == vr.last_debanded == 7
    other = _host(_debanded(_host(clip8, DB.deblock_stream_np, 16, 4)), DR.dering_stream_np, *DR.DEFAULTS)      # deband in front of dering
    assert other != host
    wrong = _run(model16, other, 2, **kw)[3]
    assert len(wrong) == len(got) and wrong != got
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.bd_scratch is edge.ingest.dr_scratch               # one scratch buffer serves both


def test_behind_the_inverse_telecine(model16):
    from tests import test_gpu_telecine as TC
    film, tele, st = TC._clips()
    vr, got = _check(model16, tele, mfi=2, ivtc=True, on=dict(deband=(8, 4)), host=(_debanded(film, (8, 4)), dict(mfi=2)))
    assert vr.last_matches == st.matches and vr.last_dropped == st.dropped and vr.last_debanded == len(D._parse(film)[1])


def test_files_one_rank_and_two_ranks_of_two(model16, tmp_path):
    n = 10
    data = banded_clip(n, 48, 80, '420', 8, seed=8)[0]
    vr, exp = _check(model16, data, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (n - 3, R.n_output_frames(n, 2)) and one.last_debanded == n
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        assert 0 < v.last_debanded < n
    assert tot == [nw, nf]
    Y._same(dst.read_bytes(), exp)


def test_deband_0_and_no_switch_give_the_same_bytes_and_launch_nothing(model16, clip8, monkeypatch):
    calls = []
    plain = _run(model16, clip8, mfi=2)
    _probe(monkeypatch, calls)
    for kw in (dict(), dict(deband=0), dict(deband=(0, 4)), dict(deband='0:16'), dict(deband=False), dict(deband=None)):
        vr, nw, nf, got = _run(model16, clip8, mfi=2, **kw)
        assert got == plain[3] and vr.last_debanded == 0 and vr.deband is None and not calls
        assert (vr.last_instants, vr.last_deringed, vr.last_deblocked, vr.last_denoised) == (plain[0].last_instants, 0, 0, 0)
        edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
        assert edge.ingest.deband is None and not hasattr(edge.ingest, 'bd_planes') and not hasattr(edge.ingest, 'bd_scratch')
        assert edge.spec.deband is None
    vr, nw, nf, got = _run(model16, clip8, mfi=2, **ON)                  # and the probe sees a run with the switch
    assert got != plain[3] and sum(calls) == vr.last_debanded == 7
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.bd_scratch.shape == edge.ingest.yuv_in.shape and not hasattr(edge.ingest, 'dr_scratch')


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the switch reaches the runner, the stream owns stdout, the JSON line says what the stage
    did."""
    exp = _run(model16, _debanded(BD.promote_stream_np(clip8, 10), (3, 8)), mfi=2, high_depth=True)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '1', '--matrix',
                        'bt601', '--work-depth', '10', '--out-depth', '10', '--deband', '3:8'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['deband'] == {'t': 3, 'r': 8, 'payloads': 7} and (last['windows'], last['frames_written']) == (4, 9)
