"""The spatial denoiser in front of the network (``--nlmeans``) on a real MI355X: ``demfi_payload_nlmeans`` (csrc/nlmeans.hip) equal to
``nlmeans.nlmeans_payload_np`` byte for byte, out of place, inside poisoned guard bytes with the source untouched, and
``VideoRunner(nlmeans=...)`` byte-identical to an expectation that never runs the new kernel: the same runner WITHOUT ``nlmeans`` on the
stream filtered on the host with ``nlmeans_stream_np``.  The inputs are ``noisy_payload``, ``noisy_clip``, ``stripes_payload`` and
``peaks_payload`` of tests/test_nlmeans.py, which proves there that they cover the rule; model and helpers are those of the neighbouring
files.  The kernel's tile is 64 x 32 samples, a thread's block 8 x 2."""
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
from demfi_amd import deband as BA                                                   # noqa: E402
from demfi_amd import deblock as DB                                                  # noqa: E402
from demfi_amd import dering as DR                                                   # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import nlmeans as NL                                                  # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402
from tests.test_nlmeans import BOX, QUOTIENT_CASES, noisy_clip, noisy_payload, peaks_payload, stripes_payload     # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD, SRC_GUARD = 0xC7, 0x5B


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _weights(depth, spr, weights=None):
    t, g = NL.weight_table(depth, spr[0], spr[1]) if weights is None else weights
    return np.ascontiguousarray(t, dtype=np.uint16), int(g)


def _launch(pays, h, w, depth, layout, fields=None, rect=None, spr=NL.DEFAULTS, lead=0, gap=0, table=None, weights=None):
    """``pays``: payloads (1-D sample arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes, source and
    destination alike but with different strides -> the destination payloads after ONE demfi_payload_nlmeans launch over all of them.
    Every byte before, between and behind the destination payloads is intact and the source buffer is unchanged."""
    es, pb, n = pays[0].itemsize, pays[0].nbytes, len(pays)
    stride, sstride = pb + gap, pb + 2 * gap + 16 * es
    src = np.full(lead + n * sstride + 64, SRC_GUARD, np.uint8)
    for i, p in enumerate(pays):
        src[lead + i * sstride:lead + i * sstride + pb] = p.view(np.uint8)
    dev_src = torch.from_numpy(src).to(DEV)
    dev = torch.full((lead + n * stride + 64,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields, rect) if table is None else table, dtype=np.int64)
    wt, g = _weights(depth, spr, weights)
    L.check(L.load().demfi_payload_nlmeans(dev_src.data_ptr() + lead, sstride, dev.data_ptr() + lead, stride, n, tab.ctypes.data, len(tab), es,
                                           depth, spr[1], spr[2], wt.ctypes.data, g, torch.cuda.current_stream().cuda_stream), 'payload_nlmeans')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert np.array_equal(dev_src.cpu().numpy(), src), 'the source changed'
    assert (out[:lead] == GUARD).all() and (out[lead + max(n - 1, 0) * stride + (pb if n else 0):] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(pays[0].dtype) for i in range(n)]


def _check_launch(pays, h, w, depth, layout, fields=None, rect=None, spr=NL.DEFAULTS, weights=None, **kw):
    got = _launch(pays, h, w, depth, layout, fields, rect, spr, weights=weights, **kw)
    assert len(got) == len(pays)
    for i, (g, p) in enumerate(zip(got, pays)):
        exp = NL.nlmeans_payload_np(p, h, w, depth, layout, *spr, fields, rect, table=weights)
        bad = np.flatnonzero(g != exp)
        assert bad.size == 0, ('%dx%d %s depth %d fields=%r rect=%r %r payload %d: %d of %d samples differ'
                               % (w, h, layout, depth, fields, rect, spr, i, bad.size, exp.size), bad[:10], g[bad[:10]], exp[bad[:10]])
    return got


FORMATS = [(8, np.uint8), (8, np.uint16), (10, np.uint16), (16, np.uint16)]
FORMAT_IDS = ['bytes', '8-bit-in-16', '10-bit', '16-bit']
# luma sizes (w, h): below, at and above the tile of 64 x 32; two and three tiles each way
SIZES = [(2, 2), (7, 5), (16, 16), (33, 33), (63, 31), (64, 32), (65, 33), (96, 64), (150, 90)]
TRIPLES = [(s, p, r) for s in (1, 3, 16) for p in (1, 2, 3) for r in range(1, 8)]          # 63: every (P, R) pair at every S


def _lead_gap(dtype, k):
    """Strides wider than the payload; every other case off a 16-byte boundary (odd for bytes, even for 16-bit samples)."""
    es = np.dtype(dtype).itemsize
    return (dict(lead=0, gap=16), dict(lead=3 * es, gap=5 * es))[k & 1]


@pytest.mark.parametrize('depth,dtype', FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize('fields', [None, 't'], ids=['progressive', 'fields'])
def test_kernel_equals_the_numpy_definition(fields, depth, dtype):
    """Every size in every layout, two payloads a launch; the 63 triples take turns in steps of 11 from a start the case gives (11 and 63
    have no common factor: the 288 launches of the eight cases meet every triple four times or more)."""
    k, case = 0, 36 * (2 * FORMATS.index((depth, dtype)) + (fields is not None))
    for w, h in SIZES:
        for layout in y4m.LAYOUTS:
            pays = [noisy_payload(h, w, layout, depth, 1000 * k + i, fields, dtype=dtype) for i in range(2)]      # two payloads in one launch
            _check_launch(pays, h, w, depth, layout, fields, spr=TRIPLES[11 * (case + k) % 63], **_lead_gap(dtype, k))
            k += 1


def test_the_turns_meet_every_triple():
    assert sorted({11 * k % 63 for k in range(288)}) == list(range(63)) and len(SIZES) * len(y4m.LAYOUTS) == 36


@pytest.mark.parametrize('p,r', [(2, r) for r in range(1, 8)] + [(1, 7), (3, 7)], ids=lambda v: str(v))
def test_every_search_radius(p, r):
    """200 x 100 at 10 bits: one tile of the twelve lies wholly inside at every radius."""
    _check_launch([noisy_payload(100, 200, 'mono', 10, 10 * p + r)], 100, 200, 10, 'mono', None, None, (3, p, r), **_lead_gap(np.uint16, r))


def test_full_range_16_bit_samples_near_0_and_65535():
    g = np.random.RandomState(2)
    h, w = 70, 100
    for k, spr in enumerate(((16, 3, 7), (1, 1, 7), (8, 2, 3), (3, 2, 5))):
        amp = spr[0] << 9
        top = np.where(g.randint(0, 2, (h, w)) > 0, 65535 - g.randint(0, amp, (h, w)), g.randint(0, amp, (h, w)))
        top[20:40, 30:70] = 65535
        top[50:60, 10:50] = 0
        _check_launch([top.reshape(-1).astype(np.uint16)], h, w, 16, 'mono', None, None, spr, **_lead_gap(np.uint16, k))
    # any stored bits of a 16-bit container are samples: 0xffff at depth 10 and 14 next to ordinary ones (differences clamp at 4095)
    for depth, spr in ((10, (16, 3, 7)), (10, (3, 2, 5)), (14, (16, 2, 4))):
        pay = noisy_payload(40, 72, 'mono', depth, 9)
        pay[g.randint(0, pay.size, 200)] = 0xFFFF
        pay[g.randint(0, pay.size, 200)] = g.randint(1 << depth, 65536, 200)
        _check_launch([pay], 40, 72, depth, 'mono', None, None, spr, lead=2, gap=6)


@pytest.mark.parametrize('depth,dtype,spr', QUOTIENT_CASES, ids=['%d-%s-%d:%d:%d' % ((d, np.dtype(t).name) + s) for d, t, s in QUOTIENT_CASES])
def test_the_quotient_on_the_device(depth, dtype, spr):
    """The planes tests/test_nlmeans.py proves to reach W = 256, every candidate at 256, the table's ends and half of what lies between,
    numerators of both signs, every clamped patch and skipped candidates."""
    _check_launch([noisy_payload(90, 150, 'mono', depth, 21, dtype=dtype)], 90, 150, depth, 'mono', None, None, spr, lead=2 * np.dtype(dtype).itemsize, gap=6)


def test_ties_and_sums_beyond_the_definitions_32_bits():
    for depth, dtype in ((8, np.uint8), (10, np.uint16), (16, np.uint16)):
        pay, h, w = stripes_payload(depth, dtype)
        got = _check_launch([pay], h, w, depth, 'mono', None, None, (16, 1, 1), lead=4, gap=2)[0].reshape(h, w)
        assert (got[1:-1, 0] == pay.reshape(h, w)[1:-1, 0] + 1).all() and (got[1:-1, -1] == pay.reshape(h, w)[1:-1, -1]).all()       # ties up
    pay, h, w = peaks_payload()                                           # the box table at 16 bits: the definition's numerator leaves int32
    _check_launch([pay], h, w, 16, 'mono', None, None, (1, 3, 7), weights=BOX, lead=6, gap=10)
    _check_launch([pay], h, w, 16, 'mono', None, None, (1, 1, 2), weights=BOX, lead=6, gap=10)
    ident = (np.r_[256, np.zeros(1023)].astype(np.uint16), 0)             # 0 behind table[0]: the identity, every sample written
    assert np.array_equal(_check_launch([pay], h, w, 16, 'mono', None, None, (1, 2, 5), weights=ident, gap=4)[0], pay)


def test_phases_are_carried_and_ignored():
    h, w = 46, 150
    for k, (top, left) in enumerate(((4, 6), (6, 14))):
        for fields in (None, 'b'):
            if fields is not None and top % 4:
                continue
            rect = (top, top + h, left, left + w)
            pays = [noisy_payload(h, w, '420', 10, 50 + k, fields, rect) for _ in range(2)]
            got = _launch(pays, h, w, 10, '420', fields, rect, (3, 2, 3), **_lead_gap(np.uint16, k))
            for g, p in zip(got, pays):
                assert np.array_equal(g, NL.nlmeans_payload_np(p, h, w, 10, '420', 3, 2, 3, fields))       # the table without the rectangle


def test_n_0_and_three_and_forty_payloads_in_one_launch():
    pays = [noisy_payload(40, 72, '420', 8, 7 + i) for i in range(40)]
    _check_launch(pays[:3], 40, 72, 8, '420', spr=(3, 1, 2), lead=3, gap=21)
    _check_launch(pays, 40, 72, 8, '420', spr=(3, 1, 2), lead=3, gap=21)
    _check_launch([p.astype(np.uint16) << 8 for p in pays[:3]], 40, 72, 16, '420', 't', spr=(3, 2, 5), lead=16, gap=48)
    # n = 0: a success that launches and writes nothing
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), SRC_GUARD, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    wt, g = _weights(8, NL.DEFAULTS)
    assert lib.demfi_payload_nlmeans(src.data_ptr(), 360, dst.data_ptr(), 360, 0, tab.ctypes.data, 3, 1, 8, 2, 5, wt.ctypes.data, g, st) == 0
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((src == SRC_GUARD).all())


def test_samples_no_entry_names_are_copied():
    """A table of the luma plane alone over 4:2:0 payloads whose last chroma sample it still reaches through a one-sample entry: the chroma
    planes arrive in dst as they are."""
    h, w = 24, 40
    pays = [noisy_payload(h, w, '420', 8, 31 + i) for i in range(2)]
    table = [DB.plane_table(h, w, '420')[0], (pays[0].size - 1, 1, 1, 1, 0, 0)]
    got = _launch(pays, h, w, 8, '420', spr=(8, 2, 5), table=table, lead=1, gap=9)
    for g, p in zip(got, pays):
        exp = p.copy()
        exp[:h * w] = NL.nlmeans_plane_np(p[:h * w].reshape(h, w), 8, 8, 2, 5).reshape(-1)
        assert np.array_equal(g, exp) and not np.array_equal(g[:h * w], p[:h * w])


def test_a_576i_point_by_fields():
    """Many tiles, most of them inside; 3:1:2 keeps the definition's 25 passes over the payload within a second or two."""
    h, w = 576, 720
    pays = [noisy_payload(h, w, '420', 10, 11, 't')]
    got = _launch(pays, h, w, 10, '420', 't', spr=(3, 1, 2), lead=16, gap=32)
    exp = NL.nlmeans_payload_np(pays[0], h, w, 10, '420', 3, 1, 2, fields='t')
    assert np.array_equal(got[0], exp) and (exp != pays[0]).mean() > 0.2


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    wt, g = _weights(8, NL.DEFAULTS)
    fn = lib.demfi_payload_nlmeans
    ok = [src.data_ptr(), 360, dst.data_ptr(), 360, 2, tab.ctypes.data, 3, 1, 8, 2, 5, wt.ctypes.data, g, st]

    def bad(i, v, table=None, weights=None, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        if table is not None:
            a[5] = table.ctypes.data
        if weights is not None:
            a[11] = weights.ctypes.data
        return fn(*a) == ERR_ARG

    def t(p, c, v):
        x = tab.copy()
        x[p, c] = v
        return x

    def wts(k, v):
        x = wt.copy()
        x[k] = v
        return x
    assert bad(0, None) and bad(2, None) and bad(5, None) and bad(11, None) and bad(4, -1)
    assert bad(7, 0) and bad(7, 3) and bad(6, 0) and bad(6, 7) and bad(8, 9) and bad(8, 10)
    assert bad(5, 0, t(0, 1, 0)) and bad(5, 0, t(0, 2, 16385)) and bad(5, 0, t(1, 3, 9)) and bad(5, 0, t(2, 4, 8)) and bad(5, 0, t(2, 5, -1))
    assert bad(1, 359) and bad(3, 359) and bad(0, src.data_ptr() + 1, _7=2, _1=720, _3=720) and bad(3, 721, _7=2, _1=720)
    assert bad(9, 0) and bad(9, 4) and bad(10, 0) and bad(10, 8) and bad(12, -1) and bad(12, 32)
    assert bad(11, 0, weights=wts(0, 255)) and bad(11, 0, weights=wts(3, 257)) and bad(11, 0, weights=wts(900, 5))
    assert bad(2, src.data_ptr()) and bad(2, src.data_ptr() + 100)       # in place, overlapping
    assert b'demfi_payload_nlmeans' in lib.demfi_last_error()
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


def _filtered(data, spr=NL.DEFAULTS):
    return _host(data, NL.nlmeans_stream_np, *spr)


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


ON = dict(nlmeans=True)


def _check(model, data, batch=4, pipe=False, host=None, on=ON, **kw):
    """``VideoRunner(..., nlmeans=..., **kw)`` on ``data`` == the same runner WITHOUT ``nlmeans`` on the stream filtered on the host
    (``host``: that stream and the switches it runs with, where they differ), header, counts, cuts and instants included."""
    prog, hkw = (_filtered(data), kw) if host is None else host
    ve, nwe, nfe, exp = _run(model, prog, batch, **hkw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **on, **kw)
    assert (nw, nf) == (nwe, nfe) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_cut_windows, vr.last_dups) == (ve.last_instants, ve.last_st_frames, ve.last_cuts,
                                                                                                     ve.last_cut_windows, ve.last_dups)
    assert vr.last_nlm_filtered > 0 and ve.last_nlm_filtered == 0
    return vr, got


def _probe(monkeypatch, calls):
    """Every ``demfi_payload_nlmeans`` launch from here on appends its payload count to ``calls``."""
    lib = L.load()
    real = lib.demfi_payload_nlmeans
    monkeypatch.setattr(lib, 'demfi_payload_nlmeans', lambda *a: (calls.append(a[4]), real(*a))[1])


@pytest.fixture(scope='module')
def clip8():
    return noisy_clip(7, 64, 96, '420', 8, seed=3)[0]


def test_an_8_bit_stream_every_frame_once_one_launch_a_run(model16, clip8, monkeypatch):
    n = 7
    vr, got = _check(model16, clip8, batch=2, mfi=2)
    assert vr.nlmeans == (3, 2, 5) and vr.last_nlm_filtered == n and len(D._parse(got)[1]) == R.n_output_frames(n, 2)
    plain = _run(model16, clip8, 2, mfi=2)[3]
    assert len(plain) == len(got) and plain != got
    for batch in (1, 3):                                                  # batches of one and several
        assert _run(model16, clip8, batch, mfi=2, **ON)[3] == got
    # ONE launch per run of consecutive newly uploaded slots
    calls = []
    _probe(monkeypatch, calls)
    out = io.BytesIO()
    vr.run_stream(io.BytesIO(clip8), out)
    assert out.getvalue() == got and sum(calls) == n and len(calls) < n


def test_a_10_bit_stream_fps_a_pipe_full_length_and_a_scene_cut(model16, clip8):
    data = noisy_clip(6, 48, 80, '420', 10, seed=5, fps=b'25:1')[0]
    vr, got = _check(model16, data, fps=Fraction(60), high_depth=True)
    assert vr.last_fps_out == 60 and vr.last_depth == 10 and b' C420p10' in got[:80]
    vr, exp = _check(model16, clip8, batch=2, pipe=True, mfi=2)
    assert vr.last_decode_peak <= 2 + 5                                   # no look-ahead: what a run without the switch holds
    vr, exp = _check(model16, clip8, batch=3, mfi=2, full_length=True)
    assert len(D._parse(exp)[1]) == 7 * 2 and _run(model16, clip8, 1, mfi=2, full_length=True, **ON)[3] == exp
    # two scenes: the cut is found at the same frame
    from demfi_amd import scene as S
    head, a = noisy_clip(1, 64, 96, '420', 8, seed=1)
    b = noisy_clip(1, 64, 96, '420', 8, seed=2)[1]
    g = np.random.RandomState(0)
    pays = [np.clip((a[0] if f < 4 else (255 - b[0]) // 3).astype(np.int64) + g.randint(-1, 2, a[0].size), 0, 255).astype(np.uint8) for f in range(8)]
    cut = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    vr, got = _check(model16, cut, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [4] and vr.last_cut_windows >= 1


def test_with_dedup_repeats_stay_repeats(model16):
    head, p = noisy_clip(6, 48, 80, '420', 8, seed=6)
    pays = [p[0], p[0], p[1], p[2], p[2], p[3], p[4], p[5]]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + x.tobytes() for x in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, full_length=True, dedup=True)
    assert vr.last_dups == [1, 4] and vr.last_nlm_filtered == len(pays)


@pytest.mark.parametrize('mode', ['bob', 'adaptive'])
def test_under_deinterlace_every_field_is_a_plane_of_its_own(mode, model16):
    n = 6
    data = D._interlaced(noisy_clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], 't')
    kw = dict(mfi=2, deinterlace=True, deinterlace_mode=mode)
    vr, got = _check(model16, data, on=dict(nlmeans=(4, 1, 3)), host=(_filtered(data, (4, 1, 3)), kw), **kw)
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_nlm_filtered == 2 * n     # a payload is uploaded once per field
    assert got != _run(model16, data, **kw)[3]
    as_frames = _filtered(D._retag(data, b't', b'p'), (4, 1, 3))         # filtered as woven frames: not what the rule asks for
    assert got != _run(model16, D._retag(as_frames, b'p', b't'), **kw)[3]


@pytest.mark.parametrize('layout,depth', [('422', 8), ('444', 8), ('mono', 8), ('422', 10)])
def test_any_layout(layout, depth, model16):
    data = noisy_clip(6, 48, 80, layout, depth, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, layouts=True, high_depth=depth > 8)
    assert (vr.last_depth, vr.last_layout) == (depth, layout)


def test_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data = noisy_clip(6, h, w, '420', 8, seed=4)[0]
    vr, got = _check(model16, data, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def _cropped(data, rect):
    """The stream cropped to ``rect`` on the host: header of the rectangle's size, payloads through ``letterbox.crop_payload_np``."""
    hdr, pays = D._parse(data)
    t, b, l, r = rect
    head = data[:data.index(b'FRAME\n')].replace(b' W%d ' % hdr.w, b' W%d ' % (r - l)).replace(b' H%d ' % hdr.h, b' H%d ' % (b - t))
    return head + b''.join(b'FRAME\n' + LB.crop_payload_np(np.frombuffer(p, _dtype(hdr.depth)), hdr.h, hdr.w, hdr.depth, hdr.layout, rect).tobytes()
                           for p in pays)


def test_behind_a_crop_the_patches_replicate_the_edge_of_the_cropped_plane(model16):
    h, w, bars = 80, 112, (4, 4, 6, 2)
    rect = LB.bars_rect(bars, h, w)
    data = noisy_clip(6, h, w, '420', 8, seed=6, fps=b'25:1')[0]
    host = _filtered(_cropped(data, rect))
    vr, got = _check(model16, data, crop=bars, crop_output='cropped', host=(host, dict(mfi=2)), mfi=2)
    assert vr.last_crop == rect and got.startswith(b'YUV4MPEG2 W104 H72 ')


def test_behind_deblock_and_dering_in_front_of_deband_the_denoiser_the_scaler_and_the_grain(model16, clip8):
    """deblock -> dering -> nlmeans -> deband on the host is the expectation's input; everything behind is the expectation's own."""
    deringed = _host(_host(clip8, DB.deblock_stream_np, 16, 4), DR.dering_stream_np, *DR.DEFAULTS)
    host = _host(_filtered(deringed), BA.deband_stream_np, 4, 6)
    kw = dict(mfi=4, denoise=True, scale=(80, 48), grain=2)
    vr, got = _check(model16, clip8, batch=2, on=dict(nlmeans=True, deband=(4, 6), dering=True, deblock=True), host=(host, kw), **kw)
    assert b' W80 H48 ' in got[:40] and vr.last_denoised == vr.last_deblocked == vr.last_deringed == vr.last_debanded == vr.last_nlm_filtered == 7
    other = _filtered(_host(deringed, BA.deband_stream_np, 4, 6))         # deband in front of nlmeans
    assert other != host
    wrong = _run(model16, other, 2, **kw)[3]
    assert len(wrong) == len(got) and wrong != got
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.nl_scratch is edge.ingest.dr_scratch and edge.ingest.bd_scratch is edge.ingest.dr_scratch      # one scratch buffer
    vr, got = _check(model16, clip8, batch=2, mfi=2, on=dict(nlmeans=True, deband=(4, 6)),
                     host=(_host(_filtered(clip8), BA.deband_stream_np, 4, 6), dict(mfi=2)))
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.bd_scratch is edge.ingest.nl_scratch and not hasattr(edge.ingest, 'dr_scratch')


def test_behind_the_inverse_telecine(model16):
    from tests import test_gpu_telecine as TC
    film, tele, st = TC._clips()
    vr, got = _check(model16, tele, mfi=2, ivtc=True, on=dict(nlmeans=(8, 1, 2)), host=(_filtered(film, (8, 1, 2)), dict(mfi=2)))
    assert vr.last_matches == st.matches and vr.last_dropped == st.dropped and vr.last_nlm_filtered == len(D._parse(film)[1])


def test_files_one_rank_and_two_ranks_of_two(model16, tmp_path):
    n = 10
    data = noisy_clip(n, 48, 80, '420', 8, seed=8)[0]
    vr, exp = _check(model16, data, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (n - 3, R.n_output_frames(n, 2)) and one.last_nlm_filtered == n
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        assert 0 < v.last_nlm_filtered < n
    assert tot == [nw, nf]
    Y._same(dst.read_bytes(), exp)


def test_nlmeans_0_and_no_switch_give_the_same_bytes_and_launch_nothing(model16, clip8, monkeypatch):
    calls = []
    plain = _run(model16, clip8, mfi=2)
    _probe(monkeypatch, calls)
    for kw in (dict(), dict(nlmeans=0), dict(nlmeans=(0, 1, 1)), dict(nlmeans='0:2:5'), dict(nlmeans=False), dict(nlmeans=None)):
        vr, nw, nf, got = _run(model16, clip8, mfi=2, **kw)
        assert got == plain[3] and vr.last_nlm_filtered == 0 and vr.nlmeans is None and not calls
        assert (vr.last_instants, vr.last_debanded, vr.last_deringed, vr.last_deblocked, vr.last_denoised) == (plain[0].last_instants, 0, 0, 0, 0)
        edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
        assert edge.ingest.nlmeans is None and not any(hasattr(edge.ingest, a) for a in ('nl_planes', 'nl_scratch', 'nl_table', 'bd_scratch'))
        assert edge.spec.nlmeans is None
    vr, nw, nf, got = _run(model16, clip8, mfi=2, **ON)                  # and the probe sees a run with the switch
    assert got != plain[3] and sum(calls) == vr.last_nlm_filtered == 7
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.nl_scratch.shape == edge.ingest.yuv_in.shape and not hasattr(edge.ingest, 'dr_scratch') and not hasattr(edge.ingest, 'bd_scratch')


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the switch reaches the runner, the stream owns stdout, the JSON line says what the stage
    did; ``--nlmeans`` without an argument runs 3:2:5."""
    exp = _run(model16, _filtered(clip8), mfi=2)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '1', '--matrix',
                        'bt601', '--nlmeans'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['nlmeans'] == {'s': 3, 'p': 2, 'r': 5, 'payloads': 7} and (last['windows'], last['frames_written']) == (4, 9)
