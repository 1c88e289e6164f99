"""Bit depth (``--work-depth`` / ``--out-depth`` / ``--dither``) on a real MI355X: ``demfi_payload_promote`` and ``demfi_payload_requant``
(csrc/bitdepth.hip) equal to ``bitdepth.convert_payload_np`` byte for byte inside poisoned destinations, their arithmetic over its whole
range, and ``VideoRunner(work_depth=..., out_depth=...)`` byte-identical, header included, to expectations that never run the new code:
A, a promoting run equals the ``--high-depth`` run of the stream promoted on the host; B, a demoting run equals the plain run's stream
requantised on the host; C, both.  The clips, the model and the stream helpers are those of tests/test_gpu_y4m_layouts.py,
tests/test_gpu_dedup.py and tests/test_gpu_interlace.py."""
import io
import itertools
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import bitdepth as BD                                                 # noqa: E402
from demfi_amd import interlace as IL                                                # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from demfi_amd.y4m_edge import Requantizer                                           # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_interlace as TI                                           # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
POISON = 0xC3
PAIRS = [(8, 10), (8, 16), (10, 16), (10, 8), (16, 8), (16, 10), (12, 10)]
WIDTHS, HEIGHTS = (1, 7, 8, 9, 15, 16, 17, 33, 130), (1, 2, 7, 8, 9, 17)
DOWN = [(a, b) for a in y4m.DEPTHS for b in y4m.DEPTHS if b < a]


def _es(d):
    return 2 if d > 8 else 1


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------
def _sources(P, d, seed):
    """Four source payloads of P samples at d bits: random over the whole range, all zero, all peak, and a ramp that walks through every
    value (so through every residue of every den): [4, P es] bytes."""
    rng = np.random.default_rng(seed)
    peak = (1 << d) - 1
    x = rng.integers(0, peak + 1, (4, P)).astype('<u2' if d > 8 else np.uint8)
    x[1], x[2] = 0, peak
    x[3] = (np.arange(P) * (257 if P > 4096 else 1) + seed) % (peak + 1)
    return x.view(np.uint8).reshape(4, P * _es(d))


class _Launch:
    """Sources placed ``shift`` bytes behind a 16-byte boundary each, and a poisoned dst whose rows lie ``gap`` bytes apart."""

    def __init__(self, src, order, Pb_in, Pb_out, shift, gap):
        self.n, self.Pb = len(order), Pb_out
        pitch = -(-Pb_in // 16) * 16 + 16
        self.buf = np.full(len(src) * pitch + 16, 0xEE, np.uint8)
        at = [i * pitch + shift for i in range(len(src))]
        for o, p in zip(at, src):
            self.buf[o:o + Pb_in] = p
        self.stride = Pb_out + gap
        self.table = np.array([at[a] for a in order], np.int64)
        self.dev = torch.from_numpy(self.buf).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.od = torch.from_numpy(self.table).to(DEV)
        self.dst = torch.empty((self.n * self.stride + 64,), dtype=torch.uint8, device=DEV)
        assert self.dst.data_ptr() % 16 == 0

    def run(self, shapes, d_in, d_out, full, dither, field_rows):
        """One launch -> the converted rows [n, Pb]; the poisoned bytes between the rows of dst and behind the last one come back
        untouched, and so do the sources."""
        self.dst.fill_(POISON)
        pl, lib, st = np.ascontiguousarray(shapes, np.int32), L.load(), torch.cuda.current_stream().cuda_stream
        head = (self.dev.data_ptr(), self.table.ctypes.data, self.od.data_ptr(), self.n, pl.ctypes.data, len(pl), _es(d_in), _es(d_out), d_in,
                d_out, int(full))
        if d_out > d_in:
            L.check(lib.demfi_payload_promote(*head, self.dst.data_ptr(), self.stride, st), 'payload_promote')
        else:
            L.check(lib.demfi_payload_requant(*head, int(dither == 'bayer'), int(field_rows), self.dst.data_ptr(), self.stride, st),
                    'payload_requant')
        torch.cuda.synchronize()
        out = self.dst.cpu().numpy()
        body = out[:self.n * self.stride].reshape(self.n, self.stride)
        assert (body[:, self.Pb:] == POISON).all() and (out[self.n * self.stride:] == POISON).all(), 'write outside the payloads'
        assert np.array_equal(self.dev.cpu().numpy(), self.buf), 'a source was written'
        return body[:, :self.Pb]


def _ref(src, shapes, d_in, d_out, full, dither, field_rows):
    """``bitdepth.convert_plane_np`` of every plane of the source payload ``src`` (bytes), the first as luma -> the bytes written."""
    smp = src.view('<u2') if d_in > 8 else src
    out, pos = [], 0
    for i, (r, c) in enumerate(shapes):
        out.append(BD.convert_plane_np(smp[pos:pos + r * c].reshape(r, c), d_in, d_out, full, i > 0, dither, field_rows).reshape(-1))
        pos += r * c
    return np.concatenate(out).astype('<u2' if d_out > 8 else np.uint8).view(np.uint8)


def _check(shapes, d_in, d_out, full=False, dither='bayer', field_rows=False, n=4, seed=0, placements=None):
    """The planes ``shapes`` of n payloads drawn from the four sources in a scattered order, on an aligned placement (the wide path where
    the planes allow it) and on bases one sample off a 16-byte boundary with a stride that keeps no row of dst aligned (sample by sample),
    against the numpy rule."""
    P = sum(r * c for r, c in shapes)
    src = _sources(P, d_in, seed + 7 * sum(r + c for r, c in shapes))
    order = [(3, 0, 2, 1, 0, 3, 1)[i % 7] for i in range(n)]
    ref = {a: _ref(src[a], shapes, d_in, d_out, full, dither, field_rows) for a in set(order)}
    exp = np.stack([ref[a] for a in order])
    Pb_in, Pb_out = src.shape[1], exp.shape[1]
    for shift, gap in placements or ((0, 32 + -Pb_out % 16), (_es(d_in), 3 * _es(d_out) + (-Pb_out % 16 if _es(d_out) == 2 else 0))):
        got = _Launch(src, order, Pb_in, Pb_out, shift, gap).run(shapes, d_in, d_out, full, dither, field_rows)
        diff = int((got != exp).sum())
        if diff:
            print('%s %d -> %d full=%s %s field_rows=%s n=%d shift=%d: %d of %d bytes differ' % (shapes, d_in, d_out, full, dither, field_rows, n,
                                                                                                shift, diff, exp.size))
        assert np.array_equal(got, exp), (shapes, d_in, d_out, full, dither, field_rows, n, shift)


@pytest.mark.parametrize('d_in,d_out', PAIRS, ids=['%d-%d' % p for p in PAIRS])
def test_kernel_equals_the_numpy_definition_at_every_plane_size(d_in, d_out):
    """Planes of 1, 7, 8, 9, 15, 16, 17, 33 and 130 columns by 1, 2, 7, 8, 9 and 17 rows (widths of 8 and 16 take the wide path on the
    aligned placement, everything else goes sample by sample); the range, the dither mode and the field-row flag walk through their eight
    combinations over the sizes, and every combination meets a wide and a narrow size."""
    for i, (w, h) in enumerate(itertools.product(WIDTHS, HEIGHTS)):
        k = i + i // 8
        _check([(h, w)], d_in, d_out, bool(k & 1), ('bayer', 'none')[(k >> 1) & 1], bool((k >> 2) & 1), seed=i)
    for full, dither, fr in itertools.product((False, True), BD.DITHERS, (False, True)):     # every combination on the wide path and off it
        _check([(9, 16)], d_in, d_out, full, dither, fr, seed=3)
        _check([(10, 24), (5, 16), (5, 16)], d_in, d_out, full, dither, fr, n=2, seed=4)


@pytest.mark.parametrize('layout', y4m.LAYOUTS)
def test_payloads_of_every_layout(layout):
    """Odd frame sizes, so chroma planes start off vector boundaries and the launch goes sample by sample; 32x48 and 64x16, where every
    plane of every layout starts and ends on 8 samples and the launch goes wide; n = 1, 3 and 7 payloads at scattered offsets; chroma
    planes take the chroma offsets of full range.  The payload reference is ``convert_payload_np`` itself."""
    for k, ((h, w), n) in enumerate((((5, 7), 3), ((37, 53), 1), ((32, 48), 7), ((64, 16), 3))):
        shapes = IL.plane_shapes(h, w, layout)
        for j, (d_in, d_out) in enumerate(PAIRS):
            full, dither, fr = bool((j + k) & 1), BD.DITHERS[(j >> 1) & 1], bool(k & 1)
            _check(shapes, d_in, d_out, full, dither, fr, n=n, seed=k)
            src = _sources(sum(r * c for r, c in shapes), d_in, 99)[0]
            smp = (src.view('<u2') if d_in > 8 else src).astype(np.uint16 if d_in > 8 else np.uint8)
            exp = BD.convert_payload_np(smp, h, w, layout, d_in, d_out, full, dither if d_out < d_in else None, fr)
            assert np.array_equal(exp.astype('<u2' if d_out > 8 else np.uint8).view(np.uint8), _ref(src, shapes, d_in, d_out, full, dither, fr))


def test_more_payloads_than_the_grid_has_rows():
    shapes = IL.plane_shapes(4, 6, '420')
    _check(shapes, 8, 10, n=1400, placements=((0, 4),))                   # 4200 (payload, plane) pairs over 4096 grid rows
    _check(shapes, 10, 8, True, 'bayer', True, n=1400, placements=((2, 1),))
    _check(IL.plane_shapes(8, 16, '420'), 16, 10, n=1400, placements=((0, 0),))      # the wide path


@pytest.mark.parametrize('full', [False, True], ids=['limited', 'full'])
@pytest.mark.parametrize('d_in,d_out', DOWN, ids=['%d-%d' % p for p in DOWN])
def test_the_arithmetic_over_its_whole_range(d_in, d_out, full):
    """A 4:4:4 payload of 8 rows by 8 * 2^d_in columns whose column x holds v = x >> 3: every value meets every Bayer cell, in luma and in
    chroma, with the dither and with ``none``; on the wide path and, one sample off, sample by sample."""
    cols = 8 << d_in
    plane = np.tile(np.arange(cols) >> 3, (8, 1)).astype('<u2')
    src = np.concatenate([plane.reshape(-1)] * 3).view(np.uint8)
    shapes = [(8, cols)] * 3
    for dither, (shift, gap) in (('bayer', (0, 0)), ('none', (0, 16)), ('bayer', (2, 2))):
        exp = _ref(src, shapes, d_in, d_out, full, dither, False)
        got = _Launch(src[None], [0], src.size, exp.size, shift, gap).run(shapes, d_in, d_out, full, dither, False)
        assert np.array_equal(got[0], exp), (d_in, d_out, full, dither, shift, int((got[0] != exp).sum()))
    if (d_in, d_out) in ((10, 8), (16, 10)):                            # field rows: every value meets every cell there too
        rows16 = [(16, cols // 2)] * 3
        src16 = np.concatenate([np.tile(np.arange(cols // 2) >> 3, (16, 1)).astype('<u2').reshape(-1)] * 3).view(np.uint8)
        exp = _ref(src16, rows16, d_in, d_out, full, 'bayer', True)
        got = _Launch(src16[None], [0], src16.size, exp.size, 0, 0).run(rows16, d_in, d_out, full, 'bayer', True)
        assert np.array_equal(got[0], exp)


@pytest.mark.parametrize('d_in,d_out', [(8, 10), (8, 16), (10, 16), (14, 16)], ids=['8-10', '8-16', '10-16', '14-16'])
def test_promotion_over_every_stored_value(d_in, d_out):
    """Every value a stored sample can hold, those above the peak of a deep stream too, in luma and in chroma, both ranges."""
    top = 65536 if d_in > 8 else 256
    vals = np.arange(top).astype('<u2' if d_in > 8 else np.uint8)
    shapes = [(4, top // 4), (2, top // 2), (1, top)]
    src = np.concatenate([vals] * 3).view(np.uint8)
    for full in (False, True):
        smp = src.view('<u2') if d_in > 8 else src
        exp = np.concatenate([BD.convert_plane_np(smp[i * top:(i + 1) * top].reshape(s), d_in, d_out, full, i > 0).reshape(-1)
                              for i, s in enumerate(shapes)]).astype('<u2').view(np.uint8)
        for shift, gap in ((0, 0), (_es(d_in), 2)):
            got = _Launch(src[None], [0], src.size, exp.size, shift, gap).run(shapes, d_in, d_out, full, None, False)
            assert np.array_equal(got[0], exp), (d_in, d_out, full, shift)


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((160,), POISON, dtype=torch.uint8, device=DEV)
    table = np.array([0, 64], np.int64)
    od = torch.from_numpy(table).to(DEV)
    pl = np.array([[2, 8], [1, 4], [1, 4]], np.int32)                    # 24 samples
    up = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, pl.ctypes.data, 3, 1, 2, 8, 10, 0, dst.data_ptr(), 64, st)
    down = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, pl.ctypes.data, 3, 2, 1, 10, 8, 0, 1, 0, dst.data_ptr(), 32, st)

    def bad(fn, ok, i, v, **kw):
        a = list(ok)
        a[i] = v
        for k, x in kw.items():
            a[int(k[1:])] = x
        return fn(*a) == ERR_ARG
    for fn, ok, i_dst, i_stride in ((lib.demfi_payload_promote, up, 11, 12), (lib.demfi_payload_requant, down, 13, 14)):
        assert all(bad(fn, ok, i, None) for i in (0, 1, 2, 4, i_dst))    # NULL buffers
        assert bad(fn, ok, 3, -1)                                        # n < 0
        assert all(bad(fn, ok, 5, v) for v in (0, 4, -1))                # no plane, more than three
        assert all(bad(fn, ok, 8, v) for v in (0, 9, 18)) and all(bad(fn, ok, 9, v) for v in (0, 11, 32))     # depths off the list
        assert bad(fn, ok, 8, ok[9], a9=ok[8], a6=ok[7], a7=ok[6])       # the wrong way round
        assert bad(fn, ok, 8, ok[9], a6=ok[7])                           # equal depths
        assert bad(fn, ok, 6, 3 - ok[6]) and bad(fn, ok, 7, 3 - ok[7])   # sample bytes that do not fit the depths
        assert bad(fn, ok, 10, 2) and bad(fn, ok, 10, -1)                # the range flag
        assert bad(fn, ok, i_stride, ok[i_stride] - 17)                  # dst_stride below the payload
        for tab in ([0, -1], [-16, 0]):
            assert bad(fn, ok, 1, np.array(tab, np.int64).ctypes.data)   # a negative offset
        for shape in ([[0, 8], [1, 4], [1, 4]], [[2, 8], [1, 0], [1, 4]], [[2, 8], [1, 4], [1 << 21, 4]], [[1 << 16, 1 << 16], [1, 4], [1, 4]]):
            assert bad(fn, ok, 4, np.array(shape, np.int32).ctypes.data)  # an empty or oversized plane
    assert bad(lib.demfi_payload_requant, down, 11, 2) and bad(lib.demfi_payload_requant, down, 12, 2)        # the dither and field-row flags
    assert b'demfi_payload_requant' in lib.demfi_last_error()
    assert bad(lib.demfi_payload_promote, up, 11, dst.data_ptr() + 1) and bad(lib.demfi_payload_promote, up, 12, 65)    # 16-bit samples written at odd places
    assert bad(lib.demfi_payload_requant, down, 0, src.data_ptr() + 1) and bad(lib.demfi_payload_requant, down, 1, np.array([1, 64], np.int64).ctypes.data)
    assert bad(lib.demfi_payload_promote, up, 8, 10, a6=2, a9=16, a0=src.data_ptr() + 1)
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    for fn, ok in ((lib.demfi_payload_promote, up), (lib.demfi_payload_requant, down)):
        a = list(ok)
        a[3] = 0                                                         # no payload: nothing to do, nothing written
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())
    assert lib.demfi_payload_promote(*up) == 0                           # 0xA5 << 2 = 0x0294 in 24 samples of each row, nothing else
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:48].view('<u2') == 0xA5 << 2).all() and (out[64:112].view('<u2') == 0xA5 << 2).all()
    assert (out[48:64] == POISON).all() and (out[112:] == POISON).all()
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


@pytest.fixture(scope='module')
def clip8():
    return Y._clip(6, 48, 72, '420', 8, seed=3)[0]


@pytest.fixture(scope='module')
def clip10():
    return Y._clip(6, 48, 72, '420', 10, seed=3)[0]


_run, _run_file = TI._run, TI._run_file


def _header(data):
    return y4m.parse_header(data[:data.index(b'\n') + 1], y4m.DEPTHS, y4m.LAYOUTS, fields=True)


def _promoted(model, data, W, batch=2, **kw):
    """A: ``data`` run with a working and output depth of W == the --high-depth run of the stream promoted on the host."""
    hd = dict(kw, high_depth=True)
    exp = _run(model, BD.promote_stream_np(data, W), **hd)[3]
    if _header(data).depth > 8:
        kw = hd
    vr, nw, nf, got = _run(model, data, batch=batch, work_depth=W, out_depth=W, **kw)
    Y._same(got, exp)
    assert _header(got).depth == W == vr.last_depth and nf > 0 and vr.last_depths[:3] == (_header(data).depth, W, W)
    assert vr.last_depth_promoted > 0 and vr.last_depth_requantised == 0
    return vr


def _demoted(model, data, Dd, dither=None, batch=2, **kw):
    """B: ``data`` run with an output depth of D == the stream of a run without it, requantised on the host (field rows where the
    output is interlaced: the header says so)."""
    plain = _run(model, data, **kw)[3]
    exp = BD.requant_stream_np(plain, Dd, dither or 'bayer')
    dk = {'dither': dither} if dither is not None else {}
    vr, nw, nf, got = _run(model, data, batch=batch, out_depth=Dd, **dk, **kw)
    Y._same(got, exp)
    assert _header(got).depth == Dd == vr.last_depth and nf == plain.count(b'FRAME\n') > 0
    assert vr.last_depth_requantised == nf and vr.last_depth_promoted == 0 and vr.last_depths[3] == (dither or 'bayer')
    return vr, got


def test_a_promotion_8_to_10(model16, clip8, tmp_path):
    """The test that needs the feature: 8 -> 10 bits at 4:2:0 through a stream, a pipe and a file at three batch sizes."""
    exp = _run(model16, BD.promote_stream_np(clip8, 10), mfi=2, high_depth=True)[3]
    assert exp.startswith(b'YUV4MPEG2 W72 H48 F48:1 Ip C420p10\n')
    for batch, how in ((1, 'stream'), (2, 'pipe'), (4, 'file')):
        if how == 'file':
            vr, nw, nf, got = _run_file(model16, clip8, tmp_path, batch=batch, mfi=2, out_depth=10)
        else:
            vr, nw, nf, got = _run(model16, clip8, batch=batch, pipe=how == 'pipe', mfi=2, out_depth=10)
        Y._same(got, exp)
        assert (nw, nf) == (3, 7) and vr.last_depths == (8, 10, 10, None) and vr.last_depth_promoted == 6
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        assert not any(isinstance(st, Requantizer) for st in edge.stages) and edge.ingest.staged.shape[1] * 2 == edge.ingest.yuv_in.shape[1]     # H2D carries the input's bytes


def test_a_promotion_8_to_12_422_full_range_and_a_rate(model16):
    _promoted(model16, Y._clip(6, 48, 72, '422', 8, seed=4)[0], 12, mfi=2, layouts=True)
    _promoted(model16, Y._clip(6, 48, 72, '444', 8, 'bt601', True, seed=5)[0], 10, fps=Fraction(60000, 1001), layouts=True)     # full range, a non-integer rate
    _promoted(model16, Y._clip(5, 48, 72, '420', 10, full=True, seed=6)[0], 16, mfi=2)      # a deep input goes up too


def test_a_promotion_in_front_of_the_deinterlacer(model16):
    from tests import test_gpu_deint as DI
    fields = DI._interlaced(Y._clip(4, 64, 80, '420', 8, seed=6, fps=b'25:1')[0], 't')
    for mode in ('bob', 'adaptive'):
        vr = _promoted(model16, fields, 10, deinterlace=True, deinterlace_mode=mode, mfi=2)
        assert vr.last_fields == 'tff'


def test_a_promotion_with_scene_cuts_and_repeated_frames(model16, clip8):
    vr = _promoted(model16, TI._cut_clip(), 10, batch=1, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [3] and vr.last_cut_windows >= 1
    vr = _promoted(model16, D._repeat(clip8, [1, 2, 1, 1, 2, 1]), 10, mfi=2, dedup=True)
    assert vr.last_dups == [2, 6]


def test_a_promotion_with_tiles(model16):
    data = Y._clip(5, 96, 128, '420', 8, seed=4)[0]
    vr = _promoted(model16, data, 10, batch=1, mfi=2, tile=(64, 64), tile_margin=16, tile_high_depth=True)
    assert vr.last_plan is not None and vr.last_plan.n_tiles > 1


def test_a_promotion_behind_the_inverse_telecine_and_the_auto_crop(model16, tmp_path):
    """``--ivtc`` and ``--crop auto`` decide in front of the device stages on the input's own samples; their thresholds are 8-bit steps
    shifted by the depth and their comparisons are on integers, so on a limited-range stream the decisions are those of the promoted
    stream and identity A holds."""
    from demfi_amd import telecine as TC
    from tests import test_gpu_crop as CR
    h, w = 64, 80
    head, pays = D._split(Y._clip(8, h, w, '420', 8, seed=5, fps=b'24000:1001')[0])
    tele = [t.view(np.uint8) for t in TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], h, w, 8, '420', 't', 0)]
    thead = b' '.join(b'F30000:1001' if f.startswith(b'F') else b'It' if f.startswith(b'I') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    vr = _promoted(model16, thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele), 10, mfi=2, ivtc=True)
    assert len(vr.last_dropped) == 2
    boxed = CR._boxed(Y._clip(6, 64, 96, '420', 8, seed=3, look=CR._bright)[0], (16, 18, 0, 0))[0]
    exp = CR._run_file(model16, BD.promote_stream_np(boxed, 10), tmp_path, mfi=2, crop='auto', high_depth=True)
    got = CR._run_file(model16, boxed, tmp_path, mfi=2, crop='auto', out_depth=10)
    Y._same(got[2], exp[2])
    assert got[0][0].last_crop == exp[0][0].last_crop == (16, 80, 0, 96) and got[1] == exp[1]


@pytest.mark.parametrize('dither', [None, 'none'])
def test_b_demotion_10_to_8(dither, model16, clip10, tmp_path):
    vr, got = _demoted(model16, clip10, 8, dither, mfi=2, high_depth=True)
    assert got.startswith(b'YUV4MPEG2 W72 H48 F48:1 Ip C420jpeg\n')
    other = _run(model16, clip10, mfi=2, high_depth=True, out_depth=8, dither='none' if dither is None else 'bayer')[3]
    assert other != got and len(other) == len(got)
    vr2, nw, nf, got2 = _run_file(model16, clip10, tmp_path, batch=1, mfi=2, high_depth=True, out_depth=8, **({'dither': dither} if dither else {}))
    assert got2 == got and nf == 7


def test_b_demotion_16_to_10_and_the_d2h_size(model16):
    data = Y._clip(5, 48, 72, '422', 16, seed=2)[0]
    vr, got = _demoted(model16, data, 10, mfi=2, high_depth=True, layouts=True)
    vr, got = _demoted(model16, data, 8, 'none', mfi=2, high_depth=True, layouts=True)
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        assert isinstance(edge.stages[-1], Requantizer) and edge.written is edge.stages[-1].out and edge.ingest.staged is None
        assert edge.h_yuv[0].shape[1] * 2 == edge.yuv_out[0].shape[1] == 2 * y4m.payload_size(48, 72, '422')     # 16 -> 8: half the bytes cross D2H


def test_b_demotion_behind_the_shutter_and_the_scaler(model16, clip10):
    vr, _ = _demoted(model16, clip10, 8, batch=1, fps=Fraction(60), shutter=360, high_depth=True)
    assert vr.last_shutter_carried > 0
    vr, got = _demoted(model16, clip10, 8, mfi=2, scale=(96, 64), high_depth=True)
    assert vr.last_scale == (96, 64, 'lanczos3') and (_header(got).w, _header(got).h) == (96, 64)


def test_b_demotion_behind_the_weave_takes_field_rows(model16):
    """``--interlace tff``: the dither's row is the row within its field (the header of the expectation says ``It``); an odd frame count,
    and ``--dedup`` for the flush behind the last batch."""
    data = Y._clip(6, 48, 72, '420', 10, seed=3)[0]
    vr, got = _demoted(model16, data, 8, batch=1, mfi=2, interlace='tff', high_depth=True)        # 7 frames: an odd tail
    assert _header(got).interlace == 't' and got.count(b'FRAME\n') == 4
    plain = _run(model16, data, mfi=2, interlace='tff', high_depth=True)[3]
    assert got != BD.requant_stream_np(plain, 8, 'bayer', field_rows=False)
    vr, got = _demoted(model16, D._repeat(data, [1, 2, 1, 1, 2, 1]), 8, mfi=2, interlace='bff', dedup=True, high_depth=True)
    assert vr.last_dups == [2, 6]


def test_b_demotion_behind_the_whole_chain_at_every_batch_size(model16, clip10):
    """gather -> mix -> scale -> weave -> requant in one run: the bytes are those of the run without ``out_depth`` requantised on the host,
    whatever the batch size, and at batch 1 both carries ran; with ``--dedup`` the flush goes through resized buffers and the requantiser."""
    kw = dict(fps=Fraction(60), shutter=360, scale=(96, 64), interlace='tff', high_depth=True)
    vr, got = _demoted(model16, clip10, 8, batch=1, **kw)
    assert vr.last_shutter_carried > 0 and vr.last_interlace_carried > 0
    assert (_header(got).w, _header(got).h, _header(got).interlace) == (96, 64, 't')
    for batch in (2, 4):
        assert _run(model16, clip10, batch=batch, out_depth=8, **kw)[3] == got
    vr, got = _demoted(model16, D._repeat(clip10, [1, 2, 1, 1, 2, 1]), 8, mfi=2, dedup=True, scale=(96, 64), interlace='bff', high_depth=True)
    assert vr.last_dups == [2, 6] and (_header(got).w, _header(got).h, _header(got).interlace) == (96, 64, 'b')


def test_b_demotion_with_a_crop_pads_with_exact_black_at_the_output_depth(model16):
    boxed = Y._clip(6, 80, 96, '420', 10, seed=2)[0]
    vr, got = _demoted(model16, boxed, 8, mfi=2, crop=(8, 8, 0, 0), high_depth=True)
    assert vr.last_crop == (8, 72, 0, 96)
    hdr, pays = Y._read(got)
    assert hdr.depth == 8 and (hdr.h, hdr.w) == (80, 96)
    for p in pays:
        yy, cb, cr = y4m.split_planes_layout(p, 80, 96, '420')
        assert (yy[:8] == 16).all() and (yy[72:] == 16).all() and (cb[:4] == 128).all() and (cr[36:] == 128).all()


def test_c_both_ways_8_10_8(model16, clip8):
    for dither in (None, 'none'):
        dk = {'dither': dither} if dither else {}
        exp = BD.requant_stream_np(_run(model16, BD.promote_stream_np(clip8, 10), mfi=2, high_depth=True)[3], 8, dither or 'bayer')
        vr, nw, nf, got = _run(model16, clip8, mfi=2, work_depth=10, **dk)               # --work-depth alone: the output keeps 8 bits
        Y._same(got, exp)
        assert vr.last_depths == (8, 10, 8, dither or 'bayer') and (vr.last_depth_promoted, vr.last_depth_requantised) == (6, 7)
        assert vr.last_depth == 8 and got.startswith(b'YUV4MPEG2 W72 H48 F48:1 Ip C420jpeg\n')
        assert _run(model16, clip8, mfi=2, work_depth=10, out_depth=8, **dk)[3] == exp != _run(model16, clip8, mfi=2)[3]


def test_two_ranks_in_file_mode(model16, clip8, clip10, tmp_path):
    """Both stages keep nothing between payloads, so a rank's block of windows lands at its own offset, computed from the OUTPUT header's
    payload size."""
    for data, exp, kw in ((clip8, _run(model16, BD.promote_stream_np(clip8, 10), fps=Fraction(60), high_depth=True)[3], {'out_depth': 10}),
                          (clip10, BD.requant_stream_np(_run(model16, clip10, fps=Fraction(60), high_depth=True)[3], 8),
                           {'out_depth': 8, 'high_depth': True})):
        src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
        src.write_bytes(data)
        tot = [0, 0]
        for rank in range(2):
            vr = VideoRunner(model16, 2, batch=2, matrix='bt601', fps=Fraction(60), **kw)
            nw, nf = vr.run_file(str(src), str(dst), world=2, rank=rank)
            tot = [tot[0] + nw, tot[1] + nf]
            assert nf > 0
        Y._same(dst.read_bytes(), exp)
        assert tot == [3, exp.count(b'FRAME\n')]


def test_switches_that_resolve_to_the_input_depth_build_nothing(model16, clip8, clip10):
    plain = _run(model16, clip8, mfi=2)[3]
    for kw in ({'work_depth': 8}, {'out_depth': 8}, {'work_depth': 8, 'out_depth': 8}):
        vr, nw, nf, got = _run(model16, clip8, mfi=2, **kw)
        assert got == plain and vr.last_depths is None and (vr.last_depth_promoted, vr.last_depth_requantised) == (0, 0)
        for cr in vr._runners.values():
            edge = cr.runner._pipeline.edge
            assert not any(isinstance(st, Requantizer) for st in edge.stages) and edge.ingest.staged is None and edge.written is edge.yuv_out and edge.spec.depths is None
    plain10 = _run(model16, clip10, mfi=2, high_depth=True)[3]
    assert _run(model16, clip10, mfi=2, high_depth=True, work_depth=10, out_depth=10)[3] == plain10


def test_refusals_before_anything_is_allocated(model16, clip8, clip10):
    for data, kw, what in ((clip10, {'work_depth': 8, 'high_depth': True}, 'below the input'),
                           (clip8, {'out_depth': 10, 'dither': 'none'}, 'without a requantisation'),
                           (clip8, {'out_depth': 10, 'tile': (64, 64)}, '--tile-high-depth'),
                           (clip8, {'work_depth': 12, 'tile': (64, 64)}, '--tile-high-depth')):
        vr = VideoRunner(model16, 2, mfi=2, **kw)
        with pytest.raises(ValueError, match=what):
            vr.run_stream(io.BytesIO(data), io.BytesIO())
        assert not vr._runners
    for kw, what in (({'work_depth': 10, 'out_depth': 12}, 'above --work-depth'), ({'out_depth': 9}, 'must be one of'),
                     ({'work_depth': 20}, 'must be one of'), ({'dither': 'bayer'}, 'says how')):
        with pytest.raises(ValueError, match=what):
            VideoRunner(model16, 2, mfi=2, **kw)
    with pytest.raises(y4m.Y4MError, match='--high-depth'):              # an input above 8 bits still needs the flag that says what is taken
        VideoRunner(model16, 2, mfi=2, out_depth=8).run_stream(io.BytesIO(clip10), io.BytesIO())


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the three switches reach the runner, the stream owns stdout, the JSON line's ``depth``
    tells the whole story."""
    exp = _run(model16, clip8, mfi=2, work_depth=12, out_depth=10, dither='none')[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '2', '--matrix',
                        'bt601', '--work-depth', '12', '--out-depth', '10', '--dither', 'none'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp and exp.startswith(b'YUV4MPEG2 W72 H48 F48:1 Ip C420p10\n')
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['depth'] == {'in': 8, 'work': 12, 'out': 10, 'dither': 'none', 'promoted': 6, 'requantised': 7}
    assert (last['windows'], last['frames_written'], last['fps_out']) == (3, 7, '48')
