"""Interlaced output (``--interlace``) on a real MI355X: ``demfi_payload_weave`` (csrc/interlace.hip) equal to
``interlace.weave_payload_np`` byte for byte, and ``VideoRunner(interlace=...)`` byte-identical, header included, to an expectation that
never runs the new code: the progressive stream a run WITHOUT the switch writes from the same input, woven on the host by
``interlace.weave_stream_np``.  The clips, the model and the stream helpers are those of tests/test_gpu_y4m_layouts.py and
tests/test_gpu_dedup.py."""
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
from demfi_amd import interlace as IL                                                # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from demfi_amd.y4m_edge import Interlacer                                            # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
POISON = 0xC3
ROWS, COLS = (1, 2, 3, 4, 5, 6, 37), (1, 15, 16, 17, 33, 96)
KINDS = {'bytes': (1, 8), '10-bit': (2, 10), '16-bit': (2, 16)}          # sample bytes, depth (peak = 2^depth - 1)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _sources(P, es, depth, seed):
    """Four source payloads of P samples: two random ones over the whole range, an all-zero and an all-peak one; [4, P es] bytes."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << depth, (4, P)).astype('<u2' if es == 2 else np.uint8)
    x[2], x[3] = 0, (1 << depth) - 1
    return x.view(np.uint8).reshape(4, P * es)


def _pairs(n):
    """n rows of (first, second): different sources, equal ones (the odd tail), zero against peak and peak against random."""
    return [((0, 1), (1, 1), (2, 3), (3, 0), (1, 0), (2, 2), (3, 3))[i % 7] for i in range(n)]


class _Launch:
    """Sources placed ``shift`` bytes behind a 16-byte boundary each, and a poisoned dst whose rows lie ``gap`` bytes apart."""

    def __init__(self, src, pairs, P, es, shift, gap):
        self.n, self.Pb = len(pairs), P * es
        pitch = -(-self.Pb // 16) * 16 + 16
        self.buf = np.full(len(src) * pitch + 16, 0xEE, np.uint8)
        at = [i * pitch + shift for i in range(len(src))]
        for o, p in zip(at, src):
            self.buf[o:o + self.Pb] = p
        self.stride = self.Pb + gap
        self.table = np.array([[at[a], at[b]] for a, b in pairs], np.int64)
        self.dev = torch.from_numpy(self.buf).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.od = torch.from_numpy(self.table).to(DEV)
        self.dst = torch.empty((self.n * self.stride + 64,), dtype=torch.uint8, device=DEV)

    def run(self, planes, es, peak, q0, mode):
        """One launch -> the woven rows [n, P es]; the poisoned bytes between the rows of dst and behind the last one come back untouched,
        and so do the sources."""
        self.dst.fill_(POISON)
        pl = np.ascontiguousarray(planes, np.int32)
        L.check(L.load().demfi_payload_weave(self.dev.data_ptr(), self.table.ctypes.data, self.od.data_ptr(), self.n, pl.ctypes.data, len(pl), es,
                                             peak, q0, mode, self.dst.data_ptr(), self.stride, torch.cuda.current_stream().cuda_stream),
                'payload_weave')
        torch.cuda.synchronize()
        out = self.dst.cpu().numpy()
        body = out[:self.n * self.stride].reshape(self.n, self.stride)
        assert (body[:, self.Pb:] == POISON).all() and (out[self.n * self.stride:] == POISON).all(), 'write outside the payloads'
        assert np.array_equal(self.dev.cpu().numpy(), self.buf), 'a source was written'
        return body[:, :self.Pb]


def _check_shape(rows, cols, layout, es, depth, n, seed=0):
    """Every (q0, mode) on the aligned placement (the wide path where the shape allows it) and on bases shifted by one sample with an odd
    stride (the sample path), against ``weave_payload_np`` of the same pairs."""
    P = y4m.payload_size(rows, cols, layout)
    planes = IL.plane_shapes(rows, cols, layout)
    src = _sources(P, es, depth, seed + rows * 131 + cols)
    smp = [s.view('<u2') if es == 2 else s for s in src]
    pairs = _pairs(n)
    want = {}
    for order, mode in itertools.product(('t', 'b'), IL.LOWPASS):
        ref = {pr: IL.weave_payload_np(smp[pr[0]], smp[pr[1]], rows, cols, depth, layout, order, mode).view(np.uint8) for pr in set(pairs)}
        want[order, mode] = np.stack([ref[pr] for pr in pairs])
    for shift, gap in ((0, 32 + -(P * es) % 16), (es, 3 * es)):
        launch = _Launch(src, pairs, P, es, shift, gap)
        for (order, mode), exp in want.items():
            got = launch.run(planes, es, (1 << depth) - 1, int(order == 'b'), IL.LOWPASS.index(mode))
            diff = int((got != exp).sum())
            if diff:
                print('%dx%d %s es=%d depth=%d n=%d shift=%d %s %s: %d of %d bytes differ' % (rows, cols, layout, es, depth, n, shift, order, mode, diff, exp.size))
            assert np.array_equal(got, exp), (rows, cols, layout, es, depth, n, shift, order, mode)


@pytest.mark.parametrize('layout', ['mono', '420', '422', '444'])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_kernel_equals_the_numpy_definition(kind, layout):
    """Planes of 1 .. 6 and 37 rows (the five-row clamp, the strip walk) and 1 .. 96 columns (the tail of a 16-byte row): both field
    orders, the three modes, equal and different sources, all-zero and all-peak ones, n = 1 and 37."""
    es, depth = KINDS[kind]
    for rows, cols in itertools.product(ROWS, COLS):
        _check_shape(rows, cols, layout, es, depth, 37 if (rows, cols) in ((37, 96), (5, 17)) else 1 if rows == 1 else 4)


def test_the_wide_path_takes_strips_of_every_length():
    """2-byte and 1-byte planes whose rows are whole 16-byte words, tall enough for several strips and a short last one."""
    for rows, cols, layout, (es, depth) in ((203, 64, '420', KINDS['bytes']), (133, 32, '444', KINDS['10-bit']), (70, 16, 'mono', KINDS['16-bit'])):
        assert all(c * es % 16 == 0 for _, c in IL.plane_shapes(rows, cols, layout))
        _check_shape(rows, cols, layout, es, depth, 3)


def test_rows_and_chunks_beyond_one_grid():
    rng = np.random.default_rng(9)
    for cols, shift in ((16, 0), (1, 1)):                                # 16-byte rows: the wide path; single samples: the sample path
        src = rng.integers(0, 256, (64, cols)).astype(np.uint8)
        pairs = [tuple(p) for p in rng.integers(0, 64, (4100, 2))]       # more (payload, plane) pairs than the grid has rows
        got = _Launch(src, pairs, cols, 1, shift, 16 - cols + shift)
        out = got.run([(1, cols)], 1, 255, 0, 1)
        assert np.array_equal(out, np.stack([src[a] for a, _ in pairs]))  # one row of parity 0: the first source's, its own neighbour
    rows, cols = 1100, 1000                                              # more chunks of 256 samples than the grid has
    src = _sources(rows * cols, 1, 8, 1)[:2]
    out = _Launch(src, [(0, 1)], rows * cols, 1, 1, 3).run([(rows, cols)], 1, 255, 1, 2)
    assert np.array_equal(out[0], IL.weave_payload_np(src[0], src[1], rows, cols, 8, 'mono', 'b', 'complex'))


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((96,), POISON, dtype=torch.uint8, device=DEV)
    table = np.array([[0, 32], [64, 64]], np.int64)
    od = torch.from_numpy(table).to(DEV)
    planes = np.array([[2, 8], [1, 4], [1, 4]], np.int32)                # 24 samples
    fn = lib.demfi_payload_weave
    ok = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, planes.ctypes.data, 3, 1, 255, 0, 1, dst.data_ptr(), 32, st)

    def bad(i, v, **kw):
        a = list(ok)
        a[i] = v
        for k, x in kw.items():
            a[int(k[1:])] = x
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 2, 4, 10))                   # NULL buffers
    assert all(bad(6, v) for v in (0, 3, 4))                             # sample_bytes
    assert all(bad(7, v) for v in (0, -1, 65536, 256))                   # peak (above 255 with bytes)
    assert bad(7, 65536, a6=2, a11=64)
    assert all(bad(8, v) for v in (-1, 2)) and all(bad(9, v) for v in (-1, 3))        # q0, mode
    assert all(bad(5, v) for v in (0, 4, -1))                            # no plane, more than three
    assert bad(11, 23)                                                   # dst_stride below the payload
    for tab in ([[0, -1], [64, 64]], [[-16, 0], [64, 64]], [[0, 32], [64, -2]]):
        t = np.array(tab, np.int64)
        assert bad(1, t.ctypes.data)                                     # a negative offset
    for pl in ([[0, 8], [1, 4], [1, 4]], [[2, 8], [1, 0], [1, 4]], [[2, 8], [1, 4], [40000, 4]]):
        p = np.array(pl, np.int32)
        assert bad(4, p.ctypes.data)                                     # an empty or oversized plane
    assert b'demfi_payload_weave' in lib.demfi_last_error()
    odd = np.array([[1, 32], [64, 64]], np.int64)                        # 16-bit samples at an odd offset, base, dst and stride
    assert bad(1, odd.ctypes.data, a6=2, a7=1023, a11=64)
    assert bad(0, src.data_ptr() + 1, a6=2, a7=1023, a11=64) and bad(10, dst.data_ptr() + 1, a6=2, a7=1023, a11=48)
    assert bad(11, 49, a6=2, a7=1023)
    for n in (0, -3):                                                    # no row: nothing to do, nothing written
        a = list(ok)
        a[3] = n
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    assert fn(*ok) == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:24] == 0xA5).all() and (out[32:56] == 0xA5).all() and (out[24:32] == POISON).all() and (out[56:] == POISON).all()
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _run(model, data, batch=4, pipe=False, **kw):
    vr = VideoRunner(model, 2, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(D._Pipe(data) if pipe else io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _run_file(model, data, tmp_path, **kw):
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    vr = VideoRunner(model, 2, batch=kw.pop('batch', 4), matrix='bt601', **kw)
    nw, nf = vr.run_file(str(src), str(dst))
    return vr, nw, nf, dst.read_bytes()


def _woven(plain, order, lowpass=None):
    """The expectation: the progressive stream ``plain`` woven on the host under the interlaced header.  Returns (bytes, payloads)."""
    head, pays = D._split(plain) if plain.count(b'FRAME\n') else (plain, [])
    hdr = y4m.parse_header(head, y4m.DEPTHS, y4m.LAYOUTS)
    assert hdr.encode() == head and hdr.interlace == 'p'
    out = IL.weave_stream_np(pays, hdr.h, hdr.w, hdr.depth, hdr.layout, order, IL.check_lowpass(lowpass))
    return IL.interlaced_header(hdr, order).encode() + b''.join(b'FRAME\n' + p.tobytes() for p in out), len(out)


def _read_back(got, order, plain):
    """The woven stream through ``y4m.Reader(fields=True)``: its tag, its rate (half the progressive stream's) and its payload count."""
    rd = y4m.Reader(io.BytesIO(got), y4m.DEPTHS, y4m.LAYOUTS, fields=True)
    phdr = y4m.parse_header(plain[:plain.index(b'\n') + 1], y4m.DEPTHS, y4m.LAYOUTS)
    buf, n = np.empty(rd.header.payload, np.uint8), 0
    while rd.read_into(buf):
        n += 1
    assert rd.header.interlace == IL.parse_order(order) and rd.header.fps == phdr.fps / 2 and rd.header.payload == phdr.payload
    assert n == IL.n_payloads(plain.count(b'FRAME\n'))
    return n


def _carried(n, r, batch, full=False):
    """The frames a run of an n-frame clip without cuts carries between its batches: the stage's bookkeeping replayed on the host."""
    from demfi_amd.pipeline import EdgeSpec
    from demfi_amd.y4m_edge import plan_fine
    k0, nw = R.first_window(n, full), R.n_windows(n, full)
    spec, wins = EdgeSpec(y4m=True, full=full), [S.runner_order((k, k + 1, k + 2, k + 3)) for k in range(k0, k0 + nw)]
    slot, still_open, total = {f: f for f in range(-4, n + 4)}, None, 0
    for b0 in range(0, nw, batch):
        bw = wins[b0:b0 + batch]
        plan = plan_fine(spec, r, bw, b0, lambda j: k0 + j, lambda j: j == nw - 1, None, None, [list(w) for w in bw], slot)
        total += still_open is not None
        _, _, still_open = IL.close_pairs(0 if still_open is not None else None, [len(o) for o in plan[1]], plan[5], 1)
    assert still_open is None
    return total


@pytest.fixture(scope='module')
def clip7():
    return Y._clip(7, 64, 96, '420', 8, seed=3)[0]


RATES = {'x2': ({'mfi': 2}, Fraction(2)), '5/2': ({'fps': Fraction(60)}, Fraction(5, 2)), 'x3': ({'mfi': 3}, Fraction(3))}


@pytest.mark.parametrize('full', [False, True], ids=['reference timeline', 'full length'])
@pytest.mark.parametrize('rate', sorted(RATES))
def test_a_stream_equals_the_weave_of_the_progressive_stream_at_every_batch_size(rate, full, model16, clip7, tmp_path):
    """The test that needs the feature: x2, 5/2 and x3 on both timelines, batches of 1, 2 and 4 windows with identical bytes, through
    streams, a pipe and files; the frames carried between batches are those of the host replay."""
    kw, r = RATES[rate]
    kw = dict(kw, full_length=full)
    plain = _run(model16, clip7, **kw)[3]
    exp, n_exp = _woven(plain, 'tff')
    n_prog = plain.count(b'FRAME\n')
    assert n_prog == R.n_output_frames(7, r, full) and exp != plain and exp[:exp.index(b'\n')].endswith(b'C420jpeg') and b' It ' in exp[:80]
    carried = []
    for batch, how in ((1, 'stream'), (2, 'pipe'), (4, 'file')):
        if how == 'file':
            vr, nw, nf, got = _run_file(model16, clip7, tmp_path, batch=batch, interlace='tff', **kw)
        else:
            vr, nw, nf, got = _run(model16, clip7, batch=batch, pipe=how == 'pipe', interlace='tff', **kw)
        Y._same(got, exp)
        assert nf == n_exp == IL.n_payloads(n_prog) and vr.last_interlace == 't'
        assert vr.last_interlace_carried == _carried(7, r, batch, full), (batch, vr.last_interlace_carried)
        carried.append(vr.last_interlace_carried)
    assert _read_back(got, 'tff', plain) == n_exp
    if rate != 'x2':
        assert carried[0] > 0                        # windows of an odd number of frames leave one open at a batch's end
    assert vr.last_fps_out == 24 * r / 2


def test_odd_and_even_lengths(model16, clip7):
    """N odd: the last payload weaves the last frame with itself.  x3 of 7 frames is 13 frames, of 6 frames 10; full length 21 and 18."""
    head, pays = D._split(clip7)
    seen = set()
    for n, full in ((7, False), (6, False), (7, True), (6, True), (1, True)):
        data = head + b''.join(b'FRAME\n' + p for p in pays[:n])
        plain = _run(model16, data, mfi=3, full_length=full)[3]
        exp, n_exp = _woven(plain, 'bff', 'off')
        vr, nw, nf, got = _run(model16, data, batch=2, mfi=3, full_length=full, interlace='bff', interlace_lowpass='off')
        Y._same(got, exp)
        assert nf == n_exp and b' Ib ' in got[:80]
        seen.add(plain.count(b'FRAME\n') % 2)
    assert seen == {0, 1}


def test_a_clip_too_short_for_a_window_writes_the_header_alone(model16, clip7):
    head, pays = D._split(clip7)
    data = head + b''.join(b'FRAME\n' + p for p in pays[:3])
    vr, nw, nf, got = _run(model16, data, mfi=2, interlace='tff')
    assert (nw, nf) == (0, 0) and got == _woven(_run(model16, data, mfi=2)[3], 'tff')[0] and got.count(b'FRAME') == 0


@pytest.mark.parametrize('lowpass', [None, 'off', 'linear', 'complex'])
@pytest.mark.parametrize('order', ['tff', 'bff'])
def test_each_low_pass_mode_and_both_orders(order, lowpass, model16, clip7):
    plain = _run(model16, clip7, mfi=2)[3]
    exp, n_exp = _woven(plain, order, lowpass)
    kw = {'interlace_lowpass': lowpass} if lowpass is not None else {}
    vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, interlace=order, **kw)
    Y._same(got, exp)
    assert vr.interlace == (order[0], lowpass or 'linear') and nf == n_exp == 5
    if lowpass is None:
        assert got == _woven(plain, order, 'linear')[0]
    if lowpass == 'off':                             # the fields are the progressive frames' own rows
        p0, p1 = (np.frombuffer(p, np.uint8)[:64 * 96].reshape(64, 96) for p in D._split(plain)[1][:2])
        w0 = np.frombuffer(D._split(_retag_p(got))[1][0], np.uint8)[:64 * 96].reshape(64, 96)
        q0 = int(order == 'bff')
        assert np.array_equal(w0[q0::2], p0[q0::2]) and np.array_equal(w0[1 - q0::2], p1[1 - q0::2])


def _retag_p(data):
    """The woven stream tagged progressive, for helpers that read progressive streams."""
    at = data.index(b'\n')
    return data[:at].replace(b' It ', b' Ip ').replace(b' Ib ', b' Ip ') + data[at:]


def _composed(model, data, order='tff', lowpass=None, batch=2, **kw):
    """``data`` with the switches ``kw`` and ``--interlace`` == the stream of the same switches woven on the host: the stage sits behind
    whole payloads, whatever made the frames."""
    plain = _run(model, data, **kw)[3]
    exp, n_exp = _woven(plain, order, lowpass)
    ikw = {'interlace_lowpass': lowpass} if lowpass is not None else {}
    vr, nw, nf, got = _run(model, data, batch=batch, interlace=order, **ikw, **kw)
    Y._same(got, exp)
    assert nf == n_exp > 0 and got != plain and _read_back(got, order, plain) == n_exp
    return vr


def _cut_clip():
    def look(i, bgr, peak):                                              # a hard cut before frame 3: another scene's colours
        return bgr if i < 3 else ((peak - bgr) // 3).astype(bgr.dtype)
    return Y._clip(7, 64, 96, '420', 8, seed=1, look=look)[0]


def test_scene_cut(model16):
    """x3: window 1 is the cut window and the frames 6 .. 8 | 9 .. 11 of the two scenes pair up as they come: a payload may hold fields of
    two scenes, which is ordinary interlaced video."""
    vr = _composed(model16, _cut_clip(), batch=1, mfi=3, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [3] and vr.last_cut_windows == 1 and vr.last_interlace_carried > 0


def test_a_10_bit_stream(model16):
    vr = _composed(model16, Y._clip(7, 64, 96, '420', 10, seed=3)[0], lowpass='complex', mfi=3, high_depth=True)
    assert vr.last_depth == 10


def test_a_mono_stream_of_odd_width_takes_the_sample_path(model16):
    h, w = 65, 97
    assert y4m.payload_size(h, w, 'mono') % 2 == 1
    for lowpass in ('linear', 'complex'):
        vr = _composed(model16, Y._clip(6, h, w, 'mono', 8, seed=5)[0], 'bff', lowpass, batch=1, mfi=3, layouts=True)
        assert vr.last_layout == 'mono'


def test_the_other_layouts(model16):
    for layout in ('422', '444'):
        assert _composed(model16, Y._clip(5, 64, 96, layout, 8, seed=2)[0], mfi=3, layouts=True).last_layout == layout


def test_behind_the_shutter(model16, clip7):
    """The mixed frames are what is woven; 24 -> 60 at 360 degrees carries samples of open groups AND the open frame between batches."""
    vr = _composed(model16, clip7, mfi=2, shutter=180, shutter_samples=2)
    assert vr.last_shutter == (2, 4)
    vr = _composed(model16, clip7, batch=1, fps=Fraction(60), shutter=360)
    assert vr.last_shutter_carried > 0 and vr.last_interlace_carried > 0


def test_interlaced_in_and_interlaced_out(model16):
    """50i -> 100i and, the standards conversion, 25i frames/s -> 59.94i: header ``F30000:1001 It``."""
    from tests import test_gpu_deint as DI
    fields = DI._interlaced(Y._clip(4, 64, 96, '420', 8, seed=6, fps=b'25:1')[0], 't')
    assert _composed(model16, fields, mfi=2, deinterlace=True).last_fields == 'tff'
    assert _composed(model16, fields, 'bff', mfi=2, deinterlace=True, deinterlace_mode='adaptive').last_fields == 'tff'
    vr, nw, nf, got = _run(model16, fields, deinterlace=True, fps=Fraction(60000, 1001), interlace='tff')
    assert b' F30000:1001 It ' in got[:60] and vr.last_fps_out == Fraction(30000, 1001)
    Y._same(got, _woven(_run(model16, fields, deinterlace=True, fps=Fraction(60000, 1001))[3], 'tff')[0])


def test_behind_the_inverse_telecine(model16):
    from demfi_amd import telecine as TC
    h, w = 64, 80
    head, pays = D._split(Y._clip(8, h, w, '420', 8, seed=5, fps=b'24000:1001')[0])
    tele = [t.view(np.uint8) for t in TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], h, w, 8, '420', 't', 0)]
    thead = b' '.join(b'F30000:1001' if f.startswith(b'F') else b'It' if f.startswith(b'I') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    vr = _composed(model16, thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele), mfi=2, ivtc=True)
    assert len(vr.last_dropped) == 2 and vr.last_fps_out == Fraction(24000, 1001)


def test_with_repeated_frames(model16, clip7):
    """--dedup never tells the edge which window is the last: the odd tail is woven by the flush behind the last batch."""
    data = D._repeat(clip7, [1, 2, 1, 1, 2, 1, 1])
    for batch in (1, 4):
        vr = _composed(model16, data, batch=batch, mfi=2, dedup=True)
        assert vr.last_dups == [2, 6]
    plain = _run(model16, data, mfi=2, dedup=True)[3]
    assert plain.count(b'FRAME\n') % 2 == 1


def test_with_tiles(model16):
    vr = _composed(model16, Y._clip(5, 96, 128, '420', 8, seed=4)[0], batch=1, mfi=3, tile=(64, 64), tile_margin=16)
    assert vr.last_plan is not None and vr.last_plan.n_tiles > 1


def test_with_a_crop(model16):
    """Bars of 8 rows keep field parity (units of 4 rows at 4:2:0).  ``cropped``: the weave of the cropped progressive stream.  ``pad``: the
    bars go back on the host BEHIND the weave, so the stream is the woven cropped stream padded with black: with the low-pass off that is the
    weave of the padded progressive stream too; with a filter the picture's edge rows replicate and the bars stay exact black, where a
    filter run over padded frames would have mixed picture and bar rows."""
    boxed = Y._clip(6, 80, 96, '420', 8, seed=2)[0]
    kw = dict(mfi=3, crop=(8, 8, 0, 0))
    assert _composed(model16, boxed, crop_output='cropped', **kw).last_crop == (8, 72, 0, 96)
    assert _composed(model16, boxed, lowpass='off', **kw).last_crop == (8, 72, 0, 96)
    cropped = _run(model16, boxed, crop_output='cropped', **kw)[3]
    padded = _run(model16, boxed, **kw)[3]
    for lowpass in ('linear', 'complex'):
        woven, n_exp = _woven(cropped, 'tff', lowpass)
        head, pays = D._split(_retag_p(woven))
        full_hdr = y4m.parse_header(padded[:padded.index(b'\n') + 1])
        cropper = LB.Cropper(full_hdr, (8, 72, 0, 96))
        full = np.empty((len(pays), cropper.Pf), np.uint8)
        cropper.pad_into(np.stack([np.frombuffer(p, np.uint8) for p in pays]), full)
        exp = IL.interlaced_header(full_hdr, 'tff').encode() + b''.join(b'FRAME\n' + p.tobytes() for p in full)
        vr, nw, nf, got = _run(model16, boxed, batch=2, interlace='tff', interlace_lowpass=lowpass, **kw)
        Y._same(got, exp)
        assert nf == n_exp and _read_back(got, 'tff', padded) == n_exp
    with pytest.raises(ValueError, match='multiples of 4 rows'):
        _run(model16, boxed, mfi=3, crop=(6, 6, 0, 0), interlace='tff')


def test_a_run_without_the_switch_builds_no_interlacer(model16, clip7):
    vr, nw, nf, got = _run(model16, clip7, mfi=2)
    assert vr.last_interlace is None and vr.last_interlace_carried == 0
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        assert not any(isinstance(st, Interlacer) for st in edge.stages) and edge.written is edge.yuv_out and cr.runner.interlace_woven == 0
    vr, nw, nf, got = _run(model16, clip7, mfi=2, interlace='tff')
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        (interlacer,) = [st for st in edge.stages if isinstance(st, Interlacer)]
        assert edge.written is interlacer.out and cr.runner.interlace_woven == nf == 5
        assert edge.h_yuv[0].shape[0] == interlacer.rows < edge.yuv_out[0].shape[0]      # the pinned buffers hold woven payloads


def test_more_than_one_rank_is_refused_before_anything_runs(model16, clip7, tmp_path):
    vr = VideoRunner(model16, 2, mfi=2, interlace='tff')
    (tmp_path / 'in.y4m').write_bytes(clip7)
    with pytest.raises(ValueError, match='interlace with 2 ranks'):
        vr.run_file(str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m'), world=2, rank=1)
    assert not vr._runners and not (tmp_path / 'out.y4m').exists()


def test_cli_through_pipes(model16, clip7):
    """The command line is what this test is about: the two switches reach the runner, the stream owns stdout, the JSON line gains ``interlace``."""
    exp = _run(model16, clip7, mfi=2, interlace='bff', interlace_lowpass='complex')[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '2', '--matrix',
                        'bt601', '--interlace', 'bff', '--interlace-lowpass', 'complex'],
                       input=clip7, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['interlace'] == {'order': 'b', 'lowpass': 'complex', 'carried': 0}
    assert (last['windows'], last['frames_written'], last['fps_out']) == (4, 5, '24')
