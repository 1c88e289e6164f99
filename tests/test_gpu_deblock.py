"""The deblocking filter in front of the network (``--deblock``) on a real MI355X: ``demfi_payload_deblock`` (csrc/deblock.hip) equal to
``deblock.deblock_payload_np`` byte for byte, in place, inside poisoned guard bytes, and ``VideoRunner(deblock=...)`` byte-identical to an
expectation that never runs the new kernel: the same runner WITHOUT ``deblock`` on the stream deblocked on the host with
``deblock_stream_np``.  The inputs are ``blocky_payload`` and ``blocky_clip`` of tests/test_deblock.py, which checks there that they exercise
every branch; model and helpers are those of the neighbouring files."""
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
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import pipeline as P                                                  # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402
from tests.test_deblock import blocky_clip, blocky_payload, coverage, edge_lines     # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD = 0xC7
FLOOR = 0.01                                                                         # every case: at least 1 % of a test's edge lines


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _launch(pays, h, w, depth, layout, fields=None, rect=None, a=16, b=4, lead=0, gap=0):
    """``pays``: payloads (1-D sample arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes -> the payloads after
    ONE demfi_payload_deblock launch over all of them, in place.  Every byte before, between and behind the payloads is intact."""
    es, pb, n = pays[0].itemsize, pays[0].nbytes, len(pays)
    stride = pb + gap
    buf = np.full(lead + n * stride + 64, GUARD, np.uint8)
    for i, p in enumerate(pays):
        buf[lead + i * stride:lead + i * stride + pb] = p.view(np.uint8)
    dev = torch.from_numpy(buf).to(DEV)
    tab = np.ascontiguousarray(DB.plane_table(h, w, layout, fields, rect), dtype=np.int64)
    L.check(L.load().demfi_payload_deblock(dev.data_ptr() + lead, stride, n, tab.ctypes.data, len(tab), es, *DB.thresholds(depth, a, b),
                                           torch.cuda.current_stream().cuda_stream), 'payload_deblock')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert (out[:lead] == GUARD).all() and (out[lead + (n - 1) * stride + pb:] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(pays[0].dtype) for i in range(n)]


def _check_launch(lines, pays, h, w, depth, layout, fields=None, rect=None, a=16, b=4, **kw):
    got = _launch(pays, h, w, depth, layout, fields, rect, a, b, **kw)
    for i, (g, p) in enumerate(zip(got, pays)):
        exp = DB.deblock_payload_np(p, h, w, depth, layout, a, b, fields, rect)
        bad = np.flatnonzero(g != exp)
        assert bad.size == 0, ('%dx%d %s depth %d fields=%r rect=%r payload %d: %d of %d samples differ'
                               % (w, h, layout, depth, fields, rect, i, bad.size, exp.size), bad[:10])
        lines.append(edge_lines(p, h, w, layout, fields, rect))


def _covered(lines, depth, a=16, b=4):
    """From the numpy definition alone: each of the five cases covers at least ``FLOOR`` of the edge lines this test put in."""
    share = coverage(np.concatenate(lines), depth, a, b)
    print('edge lines %d, shares %s' % (sum(len(x) for x in lines), np.round(share, 4)))
    assert (share >= FLOOR).all(), share


FORMATS = [(8, np.uint8), (8, np.uint16), (10, np.uint16), (16, np.uint16)]
FORMAT_IDS = ['bytes', '8-bit-in-16', '10-bit', '16-bit']
# luma sizes (w, h): no edge; one edge each way; the tile's remainders; one column more and less than the 16-byte chunks; two and three
# tiles of 128 x 32 each way (the first border of phase 0 is 4: tiles end at 132, 260 and at 36, 68)
SIZES = [(8, 8), (9, 12), (12, 9), (16, 16), (20, 12), (12, 20), (24, 40), (40, 24), (63, 24), (64, 24), (65, 24), (72, 24), (129, 24),
         (132, 36), (133, 37), (140, 45), (270, 80)]


def _lead_gap(dtype, k):
    """Strides wider than the payload; every other case off a 16-byte boundary (odd for bytes, even for 16-bit samples)."""
    es = np.dtype(dtype).itemsize
    return (dict(lead=0, gap=16), dict(lead=3 * es, gap=5 * es))[k & 1]


@pytest.mark.parametrize('depth,dtype', FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize('fields', [None, 't'], ids=['progressive', 'fields'])
def test_kernel_equals_the_numpy_definition(fields, depth, dtype):
    lines, k = [], 0
    for w, h in SIZES:
        for layout in y4m.LAYOUTS:
            pays = [blocky_payload(h, w, layout, depth, 1000 * k + i, fields, dtype=dtype) for i in range(2)]
            _check_launch(lines, pays, h, w, depth, layout, fields, **_lead_gap(dtype, k))
            k += 1
    _covered(lines, depth)


@pytest.mark.parametrize('depth,dtype', [(8, np.uint8), (10, np.uint16)], ids=['bytes', '10-bit'])
@pytest.mark.parametrize('w,h', [(40, 24), (140, 45)], ids=['one-tile', 'four-tiles'])
def test_all_64_phases(w, h, depth, dtype):
    lines = []
    for top in range(8):
        for left in range(8):
            rect = (top, top + h, left, left + w)
            tab = DB.plane_table(h, w, '444', None, rect)
            assert all(e[4:] == (left, top) for e in tab)
            pays = [blocky_payload(h, w, '444', depth, 8 * top + left, None, rect, dtype)]
            _check_launch(lines, pays, h, w, depth, '444', None, rect, **_lead_gap(dtype, top + left))
    _covered(lines, depth)


@pytest.mark.parametrize('depth,dtype', [(8, np.uint8), (10, np.uint16)], ids=['bytes', '10-bit'])
def test_phases_of_a_cropped_420_stream_progressive_and_by_fields(depth, dtype):
    """Luma and chroma phases that differ, and the halved top of fields: the rectangles ``--crop`` allows (even; rows in fours for fields)."""
    lines = []
    for k, (top, left) in enumerate(((4, 6), (2, 2), (6, 14), (12, 10), (8, 4))):
        for fields in (None, 'b'):
            if fields is not None and top % 4:
                continue
            h, w = 46, 150
            rect = (top, top + h, left, left + w)
            pays = [blocky_payload(h, w, '420', depth, 50 + k, fields, rect, dtype) for _ in range(2)]
            _check_launch(lines, pays, h, w, depth, '420', fields, rect, **_lead_gap(dtype, k))
    _covered(lines, depth)


@pytest.mark.parametrize('n', [1, 3, 70])
@pytest.mark.parametrize('depth,dtype', [(8, np.uint8), (16, np.uint16)], ids=['bytes', '16-bit'])
def test_any_number_of_payloads_in_one_launch(depth, dtype, n):
    lines, (w, h) = [], (72, 40)
    pays = [blocky_payload(h, w, '420', depth, 7 * n + i, dtype=dtype) for i in range(n)]
    _check_launch(lines, pays, h, w, depth, '420', lead=3 * np.dtype(dtype).itemsize, gap=21 * np.dtype(dtype).itemsize)
    _check_launch(lines, pays[:3], h, w, depth, '420', 't', lead=16, gap=48)
    _covered(lines, depth)


def test_every_step_across_an_edge_on_flat_sides():
    """p0 - q0 from -a-1 to a+1 at 8 bits, one step a row, on flat sides; the rows are 35 and cross four horizontal edges too."""
    a, b, s = DB.thresholds(8)
    steps = np.arange(-a - 1, a + 2)
    plane = np.full((steps.size, 24), 100, np.int64)
    plane[:, 8:16] += steps[:, None]
    plane[:, 16:] += 2 * steps[:, None]                                   # a second edge with the same step
    pay = plane.astype(np.uint8).reshape(-1)
    got = _launch([pay], steps.size, 24, 8, 'mono')[0]
    assert np.array_equal(got, DB.deblock_payload_np(pay, steps.size, 24, 8, 'mono'))
    rows = DB.deblock_plane_np(plane.astype(np.uint8), a, b, s, order='v')     # the vertical edges alone: what each step does
    changed = (rows != plane).any(1)
    assert changed[(np.abs(steps) >= 2) & (np.abs(steps) < a)].all() and not changed[np.abs(steps) >= a].any() and not changed[steps == 0].any()
    cases = DB.line_cases(plane[:, 4:12], a, b, s)
    assert set(cases[np.abs(steps) < s]) == {4} and set(cases[(np.abs(steps) >= s) & (np.abs(steps) < a)]) == {1} and set(cases[np.abs(steps) >= a]) == {0}
    for thr in ((0, 0), (255, 255), (255, 0), (1, 1)):                    # and the ends of the thresholds' range
        assert np.array_equal(_launch([pay], steps.size, 24, 8, 'mono', a=thr[0], b=thr[1])[0],
                              DB.deblock_payload_np(pay, steps.size, 24, 8, 'mono', *thr))


def test_full_size_point():
    h, w = 1080, 1920
    pays = [blocky_payload(h, w, '420', 8, 11), blocky_payload(h, w, '420', 8, 12)]
    for fields in (None, 't'):
        got = _launch(pays, h, w, 8, '420', fields, lead=16, gap=32)
        for g, p in zip(got, pays):
            exp = DB.deblock_payload_np(p, h, w, 8, '420', fields=fields)
            assert np.array_equal(g, exp) and (exp != p).mean() > 0.2


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    tab = np.ascontiguousarray(DB.plane_table(12, 20, '420'), dtype=np.int64)
    fn = lib.demfi_payload_deblock
    ok = [buf.data_ptr(), 360, 2, tab.ctypes.data, 3, 1, 16, 4, 6, st]

    def bad(i, v, table=None, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        if table is not None:
            a[3] = table.ctypes.data
        return fn(*a) == ERR_ARG

    def t(p, c, v):
        x = tab.copy()
        x[p, c] = v
        return x
    assert bad(0, None) and bad(3, None) and bad(2, -1)
    assert bad(5, 0) and bad(5, 3) and bad(4, 0) and bad(4, 7)
    assert bad(3, 0, t(0, 1, 0)) and bad(3, 0, t(0, 2, 16385)) and bad(3, 0, t(1, 3, 9)) and bad(3, 0, t(2, 4, 8)) and bad(3, 0, t(2, 5, -1))
    assert bad(1, 359) and bad(0, buf.data_ptr() + 1, _5=2, _1=720) and bad(1, 721, _5=2)
    assert bad(7, 17) and bad(6, 256) and bad(8, -1)
    assert b'demfi_payload_deblock' in lib.demfi_last_error()
    a = list(ok)
    a[2] = 0
    assert fn(*a) == 0                                                    # n = 0: a no-op success
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert fn(*ok) == 0                                                   # flat payloads stay flat
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert L.ABI_VERSION == 8                                             # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _deblocked(data, a=16, b=4, rect=None):
    """The stream ``data`` deblocked on the host, payload by payload (an interlaced one field by field), header untouched."""
    hdr, pays = D._parse(data)
    smp = [np.frombuffer(p, _dtype(hdr.depth)) for p in pays]
    fields = hdr.interlace if hdr.interlace in ('t', 'b') else None
    outs = DB.deblock_stream_np(smp, hdr.h, hdr.w, hdr.depth, hdr.layout, a, b, fields, rect)
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


ON = dict(deblock=True)


def _check(model, data, batch=4, pipe=False, host=None, on=ON, **kw):
    """``VideoRunner(..., deblock=..., **kw)`` on ``data`` == the same runner WITHOUT ``deblock`` on the stream deblocked on the host
    (``host``: that stream and the switches it runs with, where they differ), header, counts, cuts and instants included."""
    prog, hkw = (_deblocked(data), kw) if host is None else host
    ve, nwe, nfe, exp = _run(model, prog, batch, **hkw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **on, **kw)
    assert (nw, nf) == (nwe, nfe) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_cut_windows, vr.last_dups) == (ve.last_instants, ve.last_st_frames, ve.last_cuts,
                                                                                                     ve.last_cut_windows, ve.last_dups)
    assert vr.last_deblocked > 0 and ve.last_deblocked == 0
    return vr, got


def _probe(monkeypatch, calls):
    """Every ``demfi_payload_deblock`` launch from here on appends its payload count to ``calls``."""
    lib = L.load()
    real = lib.demfi_payload_deblock
    monkeypatch.setattr(lib, 'demfi_payload_deblock', lambda *a: (calls.append(a[2]), real(*a))[1])


@pytest.fixture(scope='module')
def clip8():
    return blocky_clip(7, 64, 96, '420', 8, seed=3)[0]


def test_x2_uploads_every_frame_once_and_the_switch_matters(model16, clip8, monkeypatch):
    n = 7
    ups, calls = [], []
    up = P.Y4mEdge.upload
    monkeypatch.setattr(P.Y4mEdge, 'upload', lambda self, sl, idx, f: (ups.append(idx), up(self, sl, idx, f))[1])
    vr, got = _check(model16, clip8, mfi=2)
    assert sorted(ups[n:]) == list(range(n)) and vr.last_deblocked == n      # after the expectation's n: every frame once, deblocked once
    assert vr.deblock == (16, 4) and len(D._parse(got)[1]) == R.n_output_frames(n, 2)
    plain = _run(model16, clip8, mfi=2)[3]
    assert len(plain) == len(got) and plain != got
    _check(model16, clip8, mfi=2, on=dict(deblock=(24, 3)), host=(_deblocked(clip8, 24, 3), dict(mfi=2)))
    # ONE launch per run of consecutive newly uploaded slots
    _probe(monkeypatch, calls)
    out = io.BytesIO()
    vr.run_stream(io.BytesIO(clip8), out)
    assert out.getvalue() == got and sum(calls) == n and len(calls) <= 3      # batch 4 of 4 windows: the first batch's frames, then the rest


def test_the_clip_of_the_denoise_tests(model16):
    """Material without a block structure: per-sample noise on one half, a smooth moving pattern on the other.  The filter still finds lines
    below its thresholds, and the bytes are still those of the host's."""
    from tests.test_denoise import noisy_clip
    data = noisy_clip(7, 64, 96, '420', 8, seed=3)[0]
    vr, got = _check(model16, data, mfi=2)
    assert got != _run(model16, data, mfi=2)[3] and vr.last_deblocked == 7


def test_fps_12_5_a_pipe_and_batch_sizes(model16, clip8):
    data = blocky_clip(6, 48, 80, '420', 8, seed=4, fps=b'25:1')[0]
    vr, got = _check(model16, data, fps=Fraction(60))
    assert vr.last_fps_out == 60
    vr, exp = _check(model16, clip8, batch=2, pipe=True, mfi=2)
    assert vr.last_decode_peak <= 2 + 5                                   # no look-ahead: what a run without the switch holds
    for batch in (1, 3):
        assert _run(model16, clip8, batch, mfi=2, **ON)[3] == exp
    vr, exp = _check(model16, clip8, batch=3, mfi=2, full_length=True)
    assert len(D._parse(exp)[1]) == 7 * 2 and _run(model16, clip8, 1, mfi=2, full_length=True, **ON)[3] == exp


def test_scene_cut_is_found_at_the_same_frame(model16):
    """Two still scenes with a little noise from frame to frame (the blocks of ``blocky_clip`` jump in every frame, which hides a cut from the
    detector with and without the switch): the score stands out at the cut alone."""
    h, w, n, cut = 64, 96, 8, 4
    head, a = blocky_clip(1, h, w, '420', 8, seed=1)
    b = blocky_clip(1, h, w, '420', 8, seed=2)[1]
    g = np.random.RandomState(0)
    pays = [np.clip((a[0] if f < cut else (255 - b[0]) // 3).astype(np.int64) + g.randint(-1, 2, a[0].size), 0, 255).astype(np.uint8) for f in range(n)]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [cut] and vr.last_cut_windows >= 1


def test_with_dedup_repeats_stay_repeats(model16):
    """A A B C C D E F: a repeat is deblocked to the same bytes as the frame it repeats, so both runs drop the same frames; every frame
    staged by the probe is deblocked, kept or not."""
    head, p = blocky_clip(6, 48, 80, '420', 8, seed=6)
    pays = [p[0], p[0], p[1], p[2], p[2], p[3], p[4], p[5]]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + x.tobytes() for x in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, full_length=True, dedup=True)
    assert vr.last_dups == [1, 4] and vr.last_deblocked == len(pays)


@pytest.mark.parametrize('mode', ['bob', 'adaptive'])
@pytest.mark.parametrize('order', ['t', 'b'])
def test_under_deinterlace_every_field_is_a_plane_of_its_own(order, mode, model16):
    """The interlaced stream deblocked field by field on the host, then the same deinterlacing run without the switch."""
    n = 6
    data = D._interlaced(blocky_clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], order)
    kw = dict(mfi=2, deinterlace=True, deinterlace_mode=mode)
    vr, got = _check(model16, data, **kw)
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_deblocked == 2 * n       # a payload is uploaded once per field
    assert got != _run(model16, data, **kw)[3]
    as_frames = _deblocked(D._retag(data, order.encode(), b'p'))         # filtered as woven frames: not what the rule asks for
    assert got != _run(model16, D._retag(as_frames, b'p', order.encode()), **kw)[3]


def test_work_depth_10_on_an_8_bit_input_takes_the_thresholds_at_10_bits(model16, clip8):
    """Host promote, then host deblock at 10 bits (thresholds 64, 16 and 24), then the ``high_depth`` run."""
    host = _deblocked(BD.promote_stream_np(clip8, 10))
    vr, got = _check(model16, clip8, batch=2, mfi=2, work_depth=10, out_depth=10, host=(host, dict(mfi=2, high_depth=True)))
    assert vr.last_depths == (8, 10, 10, None) and vr.last_depth_promoted == vr.last_deblocked == 7 and b' C420p10' in got[:80]


def test_420p10_with_high_depth(model16):
    data = blocky_clip(6, 48, 80, '420', 10, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, high_depth=True)
    assert vr.last_depth == 10 and b' C420p10' in got[:80]


@pytest.mark.parametrize('layout,depth', [('422', 8), ('444', 8), ('mono', 8), ('422', 10)])
def test_any_layout(layout, depth, model16):
    data = blocky_clip(6, 48, 80, layout, depth, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, layouts=True, high_depth=depth > 8)
    assert (vr.last_depth, vr.last_layout) == (depth, layout)


def test_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data = blocky_clip(6, h, w, '420', 8, seed=4)[0]
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
    """--crop 4:4:6:2: the first luma edges at column 2 and row 4, the first chroma edges at column 5 and row 6 (fields: the top halved).
    The expectation crops on the host, deblocks the cropped stream with the rectangle's phases and runs without either switch."""
    h, w, bars = 80, 112, (4, 4, 6, 2)
    rect = LB.bars_rect(bars, h, w)
    data = blocky_clip(6, h, w, '420', 8, seed=6, fps=b'25:1')[0]
    kw = dict(mfi=2)
    if interlaced:
        data, kw = D._interlaced(data, 't'), dict(mfi=2, deinterlace=True)
    tab = DB.plane_table(h - 8, w - 8, '420', 't' if interlaced else None, rect)
    assert [e[4:] for e in tab[::len(tab) // 3]] == ([(6, 2), (3, 1), (3, 1)] if interlaced else [(6, 4), (3, 2), (3, 2)])
    host = _deblocked(_cropped(data, rect), rect=rect)
    vr, got = _check(model16, data, crop=bars, crop_output='cropped', host=(host, kw), **kw)
    assert vr.last_crop == rect and got.startswith(b'YUV4MPEG2 W104 H72 ')
    wrong = _run(model16, _deblocked(_cropped(data, rect)), **kw)[3]     # the cropped stream's own grid: other bytes
    assert len(wrong) == len(got) and wrong != got
    padded = _run(model16, data, crop=bars, **ON, **kw)[3]               # and with the bars back on
    assert padded.startswith(b'YUV4MPEG2 W112 H80 ') and _cropped(padded, rect)[got.index(b'FRAME\n'):] == got[got.index(b'FRAME\n'):]


def test_in_front_of_the_denoiser_the_shutter_the_scaler_and_the_weave(model16, clip8):
    vr, got = _check(model16, clip8, batch=2, mfi=4, denoise=True, shutter=180, shutter_samples=2, scale=(80, 48), interlace='tff')
    assert b' W80 H48 ' in got[:40] and b' It ' in got[:80] and vr.last_denoised == vr.last_deblocked == 7
    # deblock first, then denoise: the denoiser of the host-deblocked stream is the expectation's own
    assert got != _run(model16, clip8, 2, mfi=4, shutter=180, shutter_samples=2, scale=(80, 48), interlace='tff', **ON)[3]


def test_files_one_rank_and_two_ranks_of_two(model16, tmp_path):
    n = 10
    data = blocky_clip(n, 48, 80, '420', 8, seed=8)[0]
    vr, exp = _check(model16, data, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (n - 3, R.n_output_frames(n, 2)) and one.last_deblocked == n
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        assert 0 < v.last_deblocked < n
    assert tot == [nw, nf]
    Y._same(dst.read_bytes(), exp)


def test_deblock_0_and_no_switch_give_the_same_bytes_and_launch_nothing(model16, clip8, monkeypatch):
    calls = []
    plain = _run(model16, clip8, mfi=2)
    _probe(monkeypatch, calls)
    for kw in (dict(), dict(deblock=0), dict(deblock=(0, 0)), dict(deblock='0'), dict(deblock=False)):
        vr, nw, nf, got = _run(model16, clip8, mfi=2, **kw)
        assert got == plain[3] and vr.last_deblocked == 0 and vr.deblock is None and not calls
        edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
        assert edge.ingest.deblock is None and not hasattr(edge.ingest, 'db_planes') and edge.spec.deblock is None
    vr, nw, nf, got = _run(model16, clip8, mfi=2, **ON)                  # and the probe sees a run with the switch
    assert got != plain[3] and sum(calls) == vr.last_deblocked == 7


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the switch reaches the runner, the stream owns stdout, the JSON line says what the stage
    did."""
    exp = _run(model16, _deblocked(clip8, 20, 5), mfi=2)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '1', '--matrix',
                        'bt601', '--deblock', '20'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['deblock'] == {'a': 20, 'b': 5, 'payloads': 7} and (last['windows'], last['frames_written']) == (4, 9)
