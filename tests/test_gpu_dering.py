"""The deringing filter in front of the network (``--dering``) on a real MI355X: ``demfi_payload_dering`` (csrc/dering.hip) equal to
``dering.dering_payload_np`` byte for byte, out of place, inside poisoned guard bytes with the source untouched, and
``VideoRunner(dering=...)`` byte-identical to an expectation that never runs the new kernel: the same runner WITHOUT ``dering`` on the
stream deringed on the host with ``dering_stream_np``.  The inputs are ``ringing_payload``, ``ringing_clip`` and ``clamp_payload`` of
tests/test_dering.py, which proves there that they cover the rule; model and helpers are those of the neighbouring files.  The kernel's
tile is 64 x 32 samples on the block grid."""
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
from demfi_amd import deblock as DB                                                  # noqa: E402
from demfi_amd import dering as DR                                                   # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import pipeline as P                                                  # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402
from tests.test_dering import clamp_payload, ringing_clip, ringing_payload           # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD, SRC_GUARD = 0xC7, 0x5B


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _launch(pays, h, w, depth, layout, fields=None, rect=None, psd=DR.DEFAULTS, lead=0, gap=0, table=None):
    """``pays``: payloads (1-D sample arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes, source and
    destination alike but with different strides -> the destination payloads after ONE demfi_payload_dering launch over all of them.
    Every byte before, between and behind the destination payloads is intact and the source buffer is unchanged."""
    es, pb, n = pays[0].itemsize, pays[0].nbytes, len(pays)
    stride, sstride = pb + gap, pb + 2 * gap + 16 * es
    src = np.full(lead + n * sstride + 64, SRC_GUARD, np.uint8)
    for i, p in enumerate(pays):
        src[lead + i * sstride:lead + i * sstride + pb] = p.view(np.uint8)
    dev_src = torch.from_numpy(src).to(DEV)
    dev = torch.full((lead + n * stride + 64,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields, rect) if table is None else table, dtype=np.int64)
    L.check(L.load().demfi_payload_dering(dev_src.data_ptr() + lead, sstride, dev.data_ptr() + lead, stride, n, tab.ctypes.data, len(tab), es,
                                          depth, *psd, torch.cuda.current_stream().cuda_stream), 'payload_dering')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert np.array_equal(dev_src.cpu().numpy(), src), 'the source changed'
    assert (out[:lead] == GUARD).all() and (out[lead + max(n - 1, 0) * stride + (pb if n else 0):] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(pays[0].dtype) for i in range(n)]


def _check_launch(pays, h, w, depth, layout, fields=None, rect=None, psd=DR.DEFAULTS, **kw):
    got = _launch(pays, h, w, depth, layout, fields, rect, psd, **kw)
    assert len(got) == len(pays)
    for i, (g, p) in enumerate(zip(got, pays)):
        exp = DR.dering_payload_np(p, h, w, depth, layout, *psd, fields, rect)
        bad = np.flatnonzero(g != exp)
        assert bad.size == 0, ('%dx%d %s depth %d fields=%r rect=%r %r payload %d: %d of %d samples differ'
                               % (w, h, layout, depth, fields, rect, psd, i, bad.size, exp.size), bad[:10], g[bad[:10]], exp[bad[:10]])


FORMATS = [(8, np.uint8), (8, np.uint16), (10, np.uint16), (16, np.uint16)]
FORMAT_IDS = ['bytes', '8-bit-in-16', '10-bit', '16-bit']
# luma sizes (w, h): smaller than a block; one block and a ragged one; the strips' and the tile's remainders; one sample less, equal and more
# than the tile of 64 x 32 each way; two and three tiles each way
SIZES = [(7, 5), (8, 8), (12, 9), (9, 12), (16, 16), (63, 24), (64, 24), (65, 24), (40, 31), (40, 32), (40, 33), (128, 64), (150, 90)]
CORNERS = [(15, 4, 3), (15, 4, 6), (0, 4, 5), (15, 0, 5), (1, 1, 6)]


def _lead_gap(dtype, k):
    """Strides wider than the payload; every other case off a 16-byte boundary (odd for bytes, even for 16-bit samples)."""
    es = np.dtype(dtype).itemsize
    return (dict(lead=0, gap=16), dict(lead=3 * es, gap=5 * es))[k & 1]


@pytest.mark.parametrize('depth,dtype', FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize('fields', [None, 't'], ids=['progressive', 'fields'])
def test_kernel_equals_the_numpy_definition(fields, depth, dtype):
    k = 0
    for w, h in SIZES:
        for layout in y4m.LAYOUTS:
            pays = [ringing_payload(h, w, layout, depth, 1000 * k + i, fields, dtype=dtype) for i in range(2)]     # two payloads in one launch
            _check_launch(pays, h, w, depth, layout, fields, **_lead_gap(dtype, k))
            k += 1


@pytest.mark.parametrize('depth,dtype', [(8, np.uint8), (10, np.uint16)], ids=['bytes', '10-bit'])
@pytest.mark.parametrize('w,h', [(40, 24), (100, 45)], ids=['one-tile', 'four-tiles'])
def test_all_64_phases(w, h, depth, dtype):
    for top in range(8):
        for left in range(8):
            rect = (top, top + h, left, left + w)
            tab = DB.plane_table(h, w, 'mono', None, rect)
            assert all(e[4:] == (left, top) for e in tab)
            pays = [ringing_payload(h, w, 'mono', depth, 8 * top + left, None, rect, dtype)]
            _check_launch(pays, h, w, depth, 'mono', None, rect, (9, 3, 4), **_lead_gap(dtype, top + left))


@pytest.mark.parametrize('depth,dtype', [(8, np.uint8), (10, np.uint16)], ids=['bytes', '10-bit'])
def test_phases_of_a_cropped_420_stream_progressive_and_by_fields(depth, dtype):
    """Luma and chroma phases that differ, and the halved top of fields: the rectangles ``--crop`` allows (even; rows in fours for fields)."""
    for k, (top, left) in enumerate(((4, 6), (2, 2), (6, 14), (12, 10), (8, 4))):
        for fields in (None, 'b'):
            if fields is not None and top % 4:
                continue
            h, w = 46, 150
            rect = (top, top + h, left, left + w)
            pays = [ringing_payload(h, w, '420', depth, 50 + k, fields, rect, dtype) for _ in range(2)]
            _check_launch(pays, h, w, depth, '420', fields, rect, **_lead_gap(dtype, k))


@pytest.mark.parametrize('psd', CORNERS, ids=['%d:%d:%d' % c for c in CORNERS])
def test_the_corners_of_the_strengths(psd):
    k = 0
    for depth, dtype in ((8, np.uint8), (10, np.uint16), (16, np.uint16)):
        for fields in (None, 'b'):
            pays = [ringing_payload(45, 100, '420', depth, 70 + k, fields, dtype=dtype)]
            _check_launch(pays, 45, 100, depth, '420', fields, None, psd, **_lead_gap(dtype, k))
            k += 1


def test_the_clamp_the_identity_and_stored_bits_above_the_depth():
    pay = clamp_payload()
    got = _launch([pay], 16, 16, 8, 'mono', psd=(15, 4, 6), lead=5, gap=3)[0]
    exp = DR.dering_payload_np(pay, 16, 16, 8, 'mono', 15, 4, 6)
    assert np.array_equal(got, exp) and got[4 * 16 + 5] == 104 and DR.plane_cases(pay.reshape(16, 16), 8, 15, 4, 6)['clamped'][4, 5]
    # 0:0 through the entry point: every sample written, none changed
    pays = [ringing_payload(45, 100, '422', 8, 5)]
    assert np.array_equal(_launch(pays, 45, 100, 8, '422', psd=(0, 0, 5), gap=7)[0], pays[0])
    # any stored bits of a 16-bit container are samples: 0xffff at depth 10 next to ordinary ones
    g = np.random.RandomState(4)
    pay = ringing_payload(40, 72, 'mono', 10, 9)
    pay[g.randint(0, pay.size, 200)] = 0xFFFF
    pay[g.randint(0, pay.size, 200)] = g.randint(1024, 65536, 200)
    _check_launch([pay], 40, 72, 10, 'mono', None, None, (15, 4, 6), lead=2, gap=6)


def test_n_0_and_three_and_seventy_payloads_in_one_launch():
    pays = [ringing_payload(40, 72, '420', 8, 7 + i) for i in range(70)]
    _check_launch(pays[:3], 40, 72, 8, '420', lead=3, gap=21)
    _check_launch(pays, 40, 72, 8, '420', lead=3, gap=21)
    _check_launch([p.astype(np.uint16) << 8 for p in pays[:3]], 40, 72, 16, '420', 't', lead=16, gap=48)
    # n = 0: a success that launches and writes nothing
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), SRC_GUARD, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    assert lib.demfi_payload_dering(src.data_ptr(), 360, dst.data_ptr(), 360, 0, tab.ctypes.data, 3, 1, 8, 4, 2, 5, st) == 0
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((src == SRC_GUARD).all())


def test_samples_no_entry_names_are_copied():
    """A table of the luma plane alone over 4:2:0 payloads whose last chroma sample it still reaches through a one-sample entry: the chroma
    planes arrive in dst as they are."""
    h, w = 24, 40
    pays = [ringing_payload(h, w, '420', 8, 31 + i) for i in range(2)]
    table = [DB.plane_table(h, w, '420')[0], (pays[0].size - 1, 1, 1, 1, 0, 0)]
    got = _launch(pays, h, w, 8, '420', table=table, lead=1, gap=9)
    for g, p in zip(got, pays):
        exp = p.copy()
        exp[:h * w] = DR.dering_plane_np(p[:h * w].reshape(h, w), 8).reshape(-1)
        assert np.array_equal(g, exp) and not np.array_equal(g[:h * w], p[:h * w])


def test_a_720p_point():
    h, w = 720, 1280
    pays = [ringing_payload(h, w, '420', 8, 11)]
    for fields in (None, 't'):
        got = _launch(pays, h, w, 8, '420', fields, lead=16, gap=32)
        exp = DR.dering_payload_np(pays[0], h, w, 8, '420', fields=fields)
        assert np.array_equal(got[0], exp) and (exp != pays[0]).mean() > 0.2


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), GUARD, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    fn = lib.demfi_payload_dering
    ok = [src.data_ptr(), 360, dst.data_ptr(), 360, 2, tab.ctypes.data, 3, 1, 8, 4, 2, 5, st]

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
    assert bad(9, 16) and bad(10, 5) and bad(11, 2) and bad(11, 7)
    assert bad(2, src.data_ptr()) and bad(2, src.data_ptr() + 100)                                  # in place, overlapping
    assert b'demfi_payload_dering' in lib.demfi_last_error()
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


def _deringed(data, psd=DR.DEFAULTS, rect=None):
    """The stream ``data`` deringed on the host, payload by payload (an interlaced one field by field), header untouched."""
    hdr, pays = D._parse(data)
    smp = [np.frombuffer(p, _dtype(hdr.depth)) for p in pays]
    fields = hdr.interlace if hdr.interlace in ('t', 'b') else None
    outs = DR.dering_stream_np(smp, hdr.h, hdr.w, hdr.depth, hdr.layout, *psd, fields, rect)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + o.tobytes() for o in outs)


def _deblocked(data, rect=None):
    hdr, pays = D._parse(data)
    smp = [np.frombuffer(p, _dtype(hdr.depth)) for p in pays]
    fields = hdr.interlace if hdr.interlace in ('t', 'b') else None
    outs = DB.deblock_stream_np(smp, hdr.h, hdr.w, hdr.depth, hdr.layout, 16, 4, fields, rect)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + o.tobytes() for o in outs)


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


ON = dict(dering=True)


def _check(model, data, batch=4, pipe=False, host=None, on=ON, **kw):
    """``VideoRunner(..., dering=..., **kw)`` on ``data`` == the same runner WITHOUT ``dering`` on the stream deringed on the host
    (``host``: that stream and the switches it runs with, where they differ), header, counts, cuts and instants included."""
    prog, hkw = (_deringed(data), kw) if host is None else host
    ve, nwe, nfe, exp = _run(model, prog, batch, **hkw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **on, **kw)
    assert (nw, nf) == (nwe, nfe) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_cut_windows, vr.last_dups) == (ve.last_instants, ve.last_st_frames, ve.last_cuts,
                                                                                                     ve.last_cut_windows, ve.last_dups)
    assert vr.last_deringed > 0 and ve.last_deringed == 0
    return vr, got


def _probe(monkeypatch, calls):
    """Every ``demfi_payload_dering`` launch from here on appends its payload count to ``calls``."""
    lib = L.load()
    real = lib.demfi_payload_dering
    monkeypatch.setattr(lib, 'demfi_payload_dering', lambda *a: (calls.append(a[4]), real(*a))[1])


@pytest.fixture(scope='module')
def clip8():
    return ringing_clip(7, 64, 96, '420', 8, seed=3)[0]


def test_x2_uploads_every_frame_once_and_the_switch_matters(model16, clip8, monkeypatch):
    n = 7
    ups, calls = [], []
    up = P.Y4mEdge.upload
    monkeypatch.setattr(P.Y4mEdge, 'upload', lambda self, sl, idx, f: (ups.append(idx), up(self, sl, idx, f))[1])
    vr, got = _check(model16, clip8, mfi=2)
    assert sorted(ups[n:]) == list(range(n)) and vr.last_deringed == n       # after the expectation's n: every frame once, deringed once
    assert vr.dering == (4, 2, 5) and len(D._parse(got)[1]) == R.n_output_frames(n, 2)
    plain = _run(model16, clip8, mfi=2)[3]
    assert len(plain) == len(got) and plain != got
    _check(model16, clip8, mfi=2, on=dict(dering=(15, 4, 6)), host=(_deringed(clip8, (15, 4, 6)), dict(mfi=2)))
    # ONE launch per run of consecutive newly uploaded slots
    _probe(monkeypatch, calls)
    out = io.BytesIO()
    vr.run_stream(io.BytesIO(clip8), out)
    assert out.getvalue() == got and sum(calls) == n and len(calls) <= 3      # batch 4 of 4 windows: the first batch's frames, then the rest


def test_fps_12_5_a_pipe_batch_sizes_and_a_scene_cut(model16, clip8):
    data = ringing_clip(6, 48, 80, '420', 8, seed=4, fps=b'25:1')[0]
    vr, got = _check(model16, data, fps=Fraction(60))
    assert vr.last_fps_out == 60
    vr, exp = _check(model16, clip8, batch=2, pipe=True, mfi=2)
    assert vr.last_decode_peak <= 2 + 5                                   # no look-ahead: what a run without the switch holds
    for batch in (1, 3):
        assert _run(model16, clip8, batch, mfi=2, **ON)[3] == exp
    vr, exp = _check(model16, clip8, batch=3, mfi=2, full_length=True)
    assert len(D._parse(exp)[1]) == 7 * 2 and _run(model16, clip8, 1, mfi=2, full_length=True, **ON)[3] == exp
    # two scenes: the cut is found at the same frame
    from demfi_amd import scene as S
    head, a = ringing_clip(1, 64, 96, '420', 8, seed=1)
    b = ringing_clip(1, 64, 96, '420', 8, seed=2)[1]
    g = np.random.RandomState(0)                                          # two still scenes with a little noise from frame to frame
    pays = [np.clip((a[0] if f < 4 else (255 - b[0]) // 3).astype(np.int64) + g.randint(-1, 2, a[0].size), 0, 255).astype(np.uint8) for f in range(8)]
    cut = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    vr, got = _check(model16, cut, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [4] and vr.last_cut_windows >= 1


def test_with_dedup_repeats_stay_repeats(model16):
    """A A B C C D E F: a repeat is deringed to the same bytes as the frame it repeats, so both runs drop the same frames; every frame
    staged by the probe is deringed, kept or not."""
    head, p = ringing_clip(6, 48, 80, '420', 8, seed=6)
    pays = [p[0], p[0], p[1], p[2], p[2], p[3], p[4], p[5]]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + x.tobytes() for x in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, full_length=True, dedup=True)
    assert vr.last_dups == [1, 4] and vr.last_deringed == len(pays)


@pytest.mark.parametrize('mode', ['bob', 'adaptive'])
@pytest.mark.parametrize('order', ['t', 'b'])
def test_under_deinterlace_every_field_is_a_plane_of_its_own(order, mode, model16):
    """The interlaced stream deringed field by field on the host, then the same deinterlacing run without the switch."""
    n = 6
    data = D._interlaced(ringing_clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], order)
    kw = dict(mfi=2, deinterlace=True, deinterlace_mode=mode)
    vr, got = _check(model16, data, **kw)
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_deringed == 2 * n        # a payload is uploaded once per field
    assert got != _run(model16, data, **kw)[3]
    as_frames = _deringed(D._retag(data, order.encode(), b'p'))          # filtered as woven frames: not what the rule asks for
    assert got != _run(model16, D._retag(as_frames, b'p', order.encode()), **kw)[3]


def test_work_depth_10_on_an_8_bit_input_and_a_10_bit_stream(model16, clip8):
    """Host promote, then host dering at 10 bits, then the ``high_depth`` run."""
    host = _deringed(BD.promote_stream_np(clip8, 10))
    vr, got = _check(model16, clip8, batch=2, mfi=2, work_depth=10, out_depth=10, host=(host, dict(mfi=2, high_depth=True)))
    assert vr.last_depths == (8, 10, 10, None) and vr.last_depth_promoted == vr.last_deringed == 7 and b' C420p10' in got[:80]
    data = ringing_clip(6, 48, 80, '420', 10, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, high_depth=True)
    assert vr.last_depth == 10 and b' C420p10' in got[:80]


@pytest.mark.parametrize('layout,depth', [('422', 8), ('444', 8), ('mono', 8), ('422', 10)])
def test_any_layout(layout, depth, model16):
    data = ringing_clip(6, 48, 80, layout, depth, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, layouts=True, high_depth=depth > 8)
    assert (vr.last_depth, vr.last_layout) == (depth, layout)


def test_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data = ringing_clip(6, h, w, '420', 8, seed=4)[0]
    vr, got = _check(model16, data, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def _cropped(data, rect):
    """The stream cropped to ``rect`` on the host: header of the rectangle's size, payloads through ``letterbox.crop_payload_np``."""
    hdr, pays = D._parse(data)
    t, b, l, r = rect
    head = data[:data.index(b'FRAME\n')].replace(b' W%d ' % hdr.w, b' W%d ' % (r - l)).replace(b' H%d ' % hdr.h, b' H%d ' % (b - t))
    return head + b''.join(b'FRAME\n' + LB.crop_payload_np(np.frombuffer(p, _dtype(hdr.depth)), hdr.h, hdr.w, hdr.depth, hdr.layout, rect).tobytes()
                           for p in pays)


@pytest.mark.parametrize('interlaced', [False, True], ids=['progressive', 'fields'])
def test_behind_a_crop_the_grid_is_that_of_the_uncropped_stream(interlaced, model16):
    """--crop 4:4:6:2: the first luma blocks start at column 2 and row 4, the first chroma blocks at column 5 and row 6 (fields: the top
    halved).  The expectation crops on the host, derings the cropped stream with the rectangle's phases and runs without either switch."""
    h, w, bars = 80, 112, (4, 4, 6, 2)
    rect = LB.bars_rect(bars, h, w)
    data = ringing_clip(6, h, w, '420', 8, seed=6, fps=b'25:1')[0]
    kw = dict(mfi=2)
    if interlaced:
        data, kw = D._interlaced(data, 't'), dict(mfi=2, deinterlace=True)
    host = _deringed(_cropped(data, rect), rect=rect)
    vr, got = _check(model16, data, crop=bars, crop_output='cropped', host=(host, kw), **kw)
    assert vr.last_crop == rect and got.startswith(b'YUV4MPEG2 W104 H72 ')
    wrong = _run(model16, _deringed(_cropped(data, rect)), **kw)[3]      # the cropped stream's own grid: other bytes
    assert len(wrong) == len(got) and wrong != got


def test_behind_the_deblocker_in_front_of_the_denoiser_the_shutter_the_scaler_and_the_weave(model16, clip8):
    """deblock -> dering on the host is the expectation's input; the denoiser of that stream is the expectation's own."""
    host = _deringed(_deblocked(clip8))
    kw = dict(mfi=4, denoise=True, shutter=180, shutter_samples=2, scale=(80, 48), interlace='tff')
    vr, got = _check(model16, clip8, batch=2, on=dict(dering=True, deblock=True), host=(host, kw), **kw)
    assert b' W80 H48 ' in got[:40] and b' It ' in got[:80] and vr.last_denoised == vr.last_deblocked == vr.last_deringed == 7
    other = _run(model16, _deblocked(_deringed(clip8)), 2, **kw)[3]      # the other order: other bytes
    assert len(other) == len(got) and other != got


def test_behind_the_inverse_telecine(model16):
    from tests import test_gpu_telecine as TC
    film, tele, st = TC._clips()
    vr, got = _check(model16, tele, mfi=2, ivtc=True, host=(_deringed(film), dict(mfi=2)))
    assert vr.last_matches == st.matches and vr.last_dropped == st.dropped and vr.last_deringed == len(D._parse(film)[1])


def test_files_one_rank_and_two_ranks_of_two(model16, tmp_path):
    n = 10
    data = ringing_clip(n, 48, 80, '420', 8, seed=8)[0]
    vr, exp = _check(model16, data, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (n - 3, R.n_output_frames(n, 2)) and one.last_deringed == n
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        assert 0 < v.last_deringed < n
    assert tot == [nw, nf]
    Y._same(dst.read_bytes(), exp)


def test_dering_0_0_and_no_switch_give_the_same_bytes_and_launch_nothing(model16, clip8, monkeypatch):
    calls = []
    plain = _run(model16, clip8, mfi=2)
    _probe(monkeypatch, calls)
    for kw in (dict(), dict(dering=0), dict(dering=(0, 0)), dict(dering='0:0:6'), dict(dering=False), dict(dering=None)):
        vr, nw, nf, got = _run(model16, clip8, mfi=2, **kw)
        assert got == plain[3] and vr.last_deringed == 0 and vr.dering is None and not calls
        edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
        assert edge.ingest.dering is None and not hasattr(edge.ingest, 'dr_planes') and not hasattr(edge.ingest, 'dr_scratch')
        assert edge.spec.dering is None
    vr, nw, nf, got = _run(model16, clip8, mfi=2, **ON)                  # and the probe sees a run with the switch
    assert got != plain[3] and sum(calls) == vr.last_deringed == 7
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.ingest.dr_scratch.shape == edge.ingest.yuv_in.shape


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the switch reaches the runner, the stream owns stdout, the JSON line says what the stage
    did."""
    exp = _run(model16, _deringed(clip8, (6, 3, 5)), mfi=2)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '1', '--matrix',
                        'bt601', '--dering', '6'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['dering'] == {'p': 6, 's': 3, 'd': 5, 'payloads': 7} and (last['windows'], last['frames_written']) == (4, 9)
