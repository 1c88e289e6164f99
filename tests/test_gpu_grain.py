"""Film grain (``--grain``) on a real MI355X: ``demfi_payload_grain`` (csrc/grain.hip) equal to ``grain.grain_payload_np`` byte for byte
inside poisoned guard bytes, and ``VideoRunner(grain=...)`` byte-identical, header included, to an expectation that never runs the new
code: the stream a run WITHOUT the switch writes from the same input, grained on the host by ``grain.grain_stream_np`` (with
``--interlace``: then woven by ``interlace.weave_stream_np``; with ``--out-depth``: then requantised by ``bitdepth.requant_stream_np``).
The clips, the model and the stream helpers are those of tests/test_gpu_y4m_layouts.py, tests/test_gpu_dedup.py and
tests/test_gpu_interlace.py."""
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
from demfi_amd import grain as G                                                     # noqa: E402
from demfi_amd import interlace as IL                                                # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from demfi_amd.y4m_edge import Encoder, Grain, Interlacer, Requantizer               # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_interlace as TI                                           # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
POISON, GUARD = 0xC3, 0xEE
SIZES = ((1, 1), (15, 3), (63, 15), (64, 16), (65, 17), (130, 36))      # luma w x h around the 64 x 16 tile and the 16-byte vector
COMBOS = tuple(itertools.product((False, True), G.CURVES))              # (full range, curve)
SEED = 0x5EED


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _sources(h, w, layout, depth, seed):
    """Four source payloads [4, P] of samples: random over everything the storage holds (at 16-bit storage also above the peak); a luma
    ramp over every 8-bit code, so every gain entry is read; the clip rule's values 0, lo, hi, peak (chroma hi too) and at 16-bit storage
    65535, sample after sample; random midtones."""
    rng = np.random.default_rng(seed)
    es, peak, P = (2 if depth > 8 else 1), (1 << depth) - 1, y4m.payload_size(h, w, layout)
    top = 65535 if es == 2 else 255
    x = np.empty((4, P), np.uint16 if es == 2 else np.uint8)
    x[0] = rng.integers(0, top + 1, P)
    x[1] = rng.integers(0, peak + 1, P)
    x[1, :h * w] = np.minimum(((np.arange(h * w) * 37 + 11) % 256) << (depth - 8) | rng.integers(0, 1 << (depth - 8), h * w), peak)
    edge = [0, 16 << (depth - 8), 235 << (depth - 8), 240 << (depth - 8), peak, top, (16 << (depth - 8)) - 1 if depth > 8 else 15]
    x[2] = np.array(edge)[(np.arange(P) * 5 + 3) % len(edge)]
    x[3] = rng.integers(peak // 4, 3 * peak // 4, P)
    return x


class _Launch:
    """The sources in one slab of guard bytes, each ``shift`` bytes behind a 16-byte boundary, and a poisoned dst whose rows lie ``gap`` bytes
    apart; after the launch everything outside the written payloads is still poison and the slab of the sources is unchanged."""

    def __init__(self, src, order, shift, gap):
        self.n, self.Pb = len(order), src.shape[1] * src.itemsize
        raw = src.view(np.uint8).reshape(len(src), self.Pb)
        pitch = -(-self.Pb // 16) * 16 + 48
        self.buf = np.full(len(src) * pitch + 64, GUARD, np.uint8)
        at = [32 + i * pitch + shift for i in range(len(src))]
        for o, p in zip(at, raw):
            self.buf[o:o + self.Pb] = p
        self.stride = self.Pb + gap
        self.table = np.array([at[a] for a in order], np.int64)
        self.dev = torch.from_numpy(self.buf).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.od = torch.from_numpy(self.table).to(DEV)
        self.dst = torch.empty((64 + self.n * self.stride + 64,), dtype=torch.uint8, device=DEV)

    def run(self, shapes, es, depth, full, r, keys, gains):
        self.dst.fill_(POISON)
        planes = np.ascontiguousarray(shapes, np.int32)
        keys = np.ascontiguousarray(keys, np.uint32)
        gains = np.ascontiguousarray(gains, np.int32)
        kd, gd = torch.from_numpy(keys.view(np.int32)).to(DEV), torch.from_numpy(gains).to(DEV)
        L.check(L.load().demfi_payload_grain(self.dev.data_ptr(), self.table.ctypes.data, self.od.data_ptr(), keys.ctypes.data, kd.data_ptr(),
                                             self.n, planes.ctypes.data, len(planes), es, depth, int(full), r, gains.ctypes.data,
                                             gd.data_ptr(), self.dst.data_ptr() + 64, self.stride,
                                             torch.cuda.current_stream().cuda_stream), 'payload_grain')
        torch.cuda.synchronize()
        out = self.dst.cpu().numpy()
        body = out[64:64 + self.n * self.stride].reshape(self.n, self.stride)
        assert (out[:64] == POISON).all() and (body[:, self.Pb:] == POISON).all() and (out[64 + self.n * self.stride:] == POISON).all(), \
            'write outside the payloads'
        assert np.array_equal(self.dev.cpu().numpy(), self.buf), 'a source was written'
        return body[:, :self.Pb]


def _check(h, w, layout, depth, full, params, n=4, seed=0, placements=None):
    """n payloads drawn from the four sources in a scattered order, row j as frame 3 j + 1, on an aligned placement (16-byte loads where
    the rows allow) and on bases one sample off a 16-byte boundary with a stride that keeps no row of dst aligned, against the numpy rule."""
    es = 2 if depth > 8 else 1
    src = _sources(h, w, layout, depth, seed + 7 * (h + w))
    order = [(3, 0, 2, 1, 0, 3, 1)[i % 7] for i in range(n)]
    frames = [(3 * j + 1) % 11 for j in range(n)]
    ref = {}
    for a, f in zip(order, frames):
        if (a, f) not in ref:
            ref[a, f] = G.grain_payload_np(src[a], h, w, layout, depth, full, f, params).view(np.uint8)
    exp = np.stack([ref[a, f] for a, f in zip(order, frames)])
    keys = [[G.plane_key(params[4], f, p) for p in range(3)] for f in frames]
    gains = G.gain_tables(depth, params, full)
    Pb = exp.shape[1]
    for shift, gap in placements or ((0, 32 + -Pb % 16), (es, 3 * es)):
        got = _Launch(src, order, shift, gap).run(IL.plane_shapes(h, w, layout), es, depth, full, params[1], keys, gains)
        diff = int((got != exp).sum())
        if diff:
            print('%dx%d %s depth=%d full=%s %r n=%d shift=%d: %d of %d bytes differ' % (w, h, layout, depth, full, params, n, shift, diff, exp.size))
        assert np.array_equal(got, exp), (h, w, layout, depth, full, params, n, shift)
    return src, exp


@pytest.mark.parametrize('layout', ['420', '422', '444', 'mono'])
@pytest.mark.parametrize('depth', [8, 10, 16])
def test_kernel_equals_the_numpy_definition_around_the_tile_edges(depth, layout):
    """Every size with every grain size; over them every (grain size, range, curve) triple.  The sources hold 0, lo, hi, peak, values above
    the peak at 16-bit storage and a ramp over every luma code; strong grain (S = 8, C = 1) so the clip is hit from both sides."""
    seen = set()
    for i, ((w, h), r) in enumerate(itertools.product(SIZES, (0, 1, 2))):
        full, curve = COMBOS[i % 4]
        seen.add((r, full, curve))
        src, exp = _check(h, w, layout, depth, full, (128, r, 16, curve, SEED), seed=i)
        if (w, h) == (130, 36):                                          # the test's own sources do what they are there for
            smp, out = src[[3, 0, 2, 1]].reshape(-1).astype(np.int64), exp.view(src.dtype).reshape(-1).astype(np.int64)
            lo, hi = G.nominal_range(depth, full, False)
            assert (out != smp).any() and ((out == lo) & (smp > lo)).any() and ((out == hi) & (smp < hi)).any()
            assert len(set((src[1, :h * w] >> (depth - 8)).tolist())) == 256
            if depth == 10:
                assert (smp > 1023).any() and (out[smp > 1023] <= smp[smp > 1023]).all()
    assert len(seen) == 12


def test_weaker_grain_and_no_chroma_grain():
    for (w, h), layout, depth, params in (((65, 17), '420', 8, (24, 1, 0, 'film', 1)), ((130, 36), '422', 10, (8, 2, 0, 'flat', 2)),
                                          ((63, 15), '444', 16, (1, 0, 3, 'film', 3)), ((33, 9), '420', 12, (40, 2, 16, 'film', 4)),
                                          ((40, 10), '420', 14, (128, 1, 8, 'flat', 0xFFFFFFFF))):
        src, exp = _check(h, w, layout, depth, False, params)
        if params[2] == 0:                                               # C = 0: the chroma planes come through untouched
            es = 2 if depth > 8 else 1
            assert np.array_equal(exp[:, h * w * es:], src[[3, 0, 2, 1]].view(np.uint8).reshape(4, -1)[:, h * w * es:])


def test_more_payloads_than_the_grid_has_rows():
    _check(4, 6, '420', 8, False, (64, 1, 8, 'film', 9), n=1400, placements=((0, 2),))     # 4200 (payload, plane) pairs over 4096 grid rows


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((96,), POISON, dtype=torch.uint8, device=DEV)
    table, keys = np.array([0, 64], np.int64), np.arange(6, dtype=np.uint32)
    gains = np.zeros((2, 256), np.int32)
    planes = np.array([[2, 8], [1, 4], [1, 4]], np.int32)                # 24 samples
    od, kd, gd = torch.from_numpy(table).to(DEV), torch.from_numpy(keys.view(np.int32)).to(DEV), torch.from_numpy(gains).to(DEV)
    fn = lib.demfi_payload_grain
    ok = (src.data_ptr(), table.ctypes.data, od.data_ptr(), keys.ctypes.data, kd.data_ptr(), 2, planes.ctypes.data, 3, 1, 8, 0, 1,
          gains.ctypes.data, gd.data_ptr(), dst.data_ptr(), 32, st)

    def bad(i, v, **kw):
        a = list(ok)
        a[i] = v
        for k, x in kw.items():
            a[int(k[1:])] = x
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 2, 3, 4, 6, 12, 13, 14))     # NULL buffers
    assert bad(5, -1) and bad(5, -3)                                     # n < 0
    assert all(bad(7, v) for v in (0, 2, 4, -1))                         # one plane or three
    assert all(bad(8, v) for v in (0, 2, 3)) and bad(9, 10) and bad(9, 16)       # sample bytes that do not fit the depth
    assert all(bad(9, v, a8=2) for v in (8, 9, 11, 18, 0))               # a depth that is none of the five
    assert bad(10, 2) and bad(10, -1) and bad(11, 3) and bad(11, -1)     # the range flag, the grain size
    assert bad(15, 23)                                                   # dst_stride below the payload
    for tab in ([0, -1], [-16, 0]):
        assert bad(1, np.array(tab, np.int64).ctypes.data)               # a negative offset
    for pl in ([[0, 8], [1, 4], [1, 4]], [[2, 8], [1, 0], [1, 4]], [[2, 65532], [1, 4], [1, 4]], [[2, 8], [1, 4], [2, 4]], [[2, 8], [1, 3], [1, 3]],
               [[5, 8], [2, 4], [2, 4]]):
        assert bad(6, np.array(pl, np.int32).ctypes.data, a15=1 << 20), pl      # empty, oversized, unequal or unfitting planes
    for at, v, size in ((0, -1, 1), (300, -5, 0), (511, 16448, 2), (7, 263169, 1), (256, 1 << 23, 0)):
        g = gains.copy()
        g.reshape(-1)[at] = v
        assert bad(12, g.ctypes.data, a11=size), (at, v)                 # a negative gain, or one that takes F G + 2^15 out of int32
    assert b'demfi_payload_grain' in lib.demfi_last_error()
    assert bad(1, np.array([1, 64], np.int64).ctypes.data, a8=2, a9=10, a15=64)          # 16-bit samples at an odd offset, base, dst, stride
    assert bad(0, src.data_ptr() + 1, a8=2, a9=10, a15=64) and bad(14, dst.data_ptr() + 1, a8=2, a9=10, a15=48)
    assert bad(15, 49, a8=2, a9=10)
    assert bad(13, gd.data_ptr() + 2) and bad(4, kd.data_ptr() + 2)      # the device tables off a 4-byte boundary
    huge = np.array([[40000, 65531]], np.int32)                          # a payload of 2^31 bytes and more
    assert bad(6, huge.ctypes.data, a7=1, a15=1 << 32)
    a = list(ok)
    a[5] = 0                                                             # no payload: nothing to do, nothing written
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    assert fn(*ok) == 0                                                  # gains of zero: the payloads come through as they are
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:24] == 0xA5).all() and (out[32:56] == 0xA5).all() and (out[24:32] == POISON).all() and (out[56:] == POISON).all()
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


@pytest.fixture(scope='module')
def clip7():
    return Y._clip(7, 64, 96, '420', 8, seed=3)[0]


_run, _run_file = TI._run, TI._run_file
GKW = dict(grain='3', grain_size=1, grain_chroma='0.75', grain_seed=11)
PARAMS = (48, 1, 12, 'film', 11)


def _stages(vr):
    (cr,) = vr._runners.values()
    return cr.runner, cr.runner._pipeline.edge


def _composed(model, data, batch=2, gkw=GKW, params=PARAMS, **kw):
    """``data`` with the switches ``kw`` and ``--grain`` == the host grain of the stream the same switches write."""
    plain = _run(model, data, **kw)[3]
    exp = G.grain_stream_np(plain, params)
    assert exp != plain and len(exp) == len(plain)
    vr, nw, nf, got = _run(model, data, batch=batch, **gkw, **kw)
    Y._same(got, exp)
    assert vr.grain == params == vr.last_grain and vr.last_grain_payloads == plain.count(b'FRAME\n') > 0
    return vr, got


def test_a_stream_equals_the_host_grain_of_the_plain_stream(model16, clip7, tmp_path):
    """The test that needs the feature: x2 through streams, a pipe and files at batches of 1, 3 and 4 windows with identical bytes."""
    plain = _run(model16, clip7, mfi=2)[3]
    exp = G.grain_stream_np(plain, PARAMS)
    assert plain.count(b'FRAME\n') == 9 and exp != plain and exp[:exp.index(b'\n')] == plain[:plain.index(b'\n')]
    for batch, how in ((1, 'stream'), (3, 'pipe'), (4, 'file')):
        if how == 'file':
            vr, nw, nf, got = _run_file(model16, clip7, tmp_path, batch=batch, mfi=2, **GKW)
        else:
            vr, nw, nf, got = _run(model16, clip7, batch=batch, pipe=how == 'pipe', mfi=2, **GKW)
        Y._same(got, exp)
        rn, edge = _stages(vr)
        assert (nw, nf) == (4, 9) and vr.last_grain_payloads == 9 == rn.grain_payloads
        assert [type(st) for st in edge.stages] == [Grain] and edge.written is edge.stages[0].out


def test_flat_curve_other_sizes_and_full_range(model16):
    data = Y._clip(5, 64, 96, '420', 8, seed=2, full=True)[0]
    for size, curve in ((0, 'flat'), (2, 'film')):
        _composed(model16, data, mfi=2, gkw=dict(grain='1.5', grain_size=size, grain_curve=curve, grain_chroma=0), params=(24, size, 0, curve, 0))


def test_behind_the_shutter_and_behind_the_scaler(model16, clip7):
    vr, _ = _composed(model16, clip7, batch=1, fps=Fraction(60), shutter=360)
    assert vr.last_shutter_carried > 0
    vr, got = _composed(model16, clip7, batch=3, mfi=2, scale=(72, 48))
    assert vr.last_scale_payloads == 9 and got.startswith(b'YUV4MPEG2 W72 H48 ')


def test_in_linear_light_the_stage_sits_behind_the_encode(model16, clip7):
    vr, _ = _composed(model16, clip7, batch=1, fps=Fraction(60), shutter=360, linear_light='bt709', out_range='full')
    rn, edge = _stages(vr)
    assert [type(st).__name__ for st in edge.stages] == ['Shutter', 'Encoder', 'Grain'] and vr.last_colour_encoded == vr.last_grain_payloads
    assert isinstance(edge.stages[1], Encoder) and edge.stages[2].full_range == 1       # the range written, not the input's


def _composed_over_progressive(model, data, after, batch=2, **kw):
    """For switches whose plain output is no longer what the stage saw (woven, requantised): ``progressive`` switches give that stream."""
    def run(progressive, **sw):
        plain = _run(model, data, **progressive)[3]
        vr, nw, nf, got = _run(model, data, batch=batch, **GKW, **sw)
        Y._same(got, after(G.grain_stream_np(plain, PARAMS)))
        assert vr.last_grain_payloads == plain.count(b'FRAME\n')
        return vr
    return run


def test_in_front_of_the_weave(model16, clip7):
    """``--interlace tff``: the host weave of the grained progressive stream; n counts progressive frames, and the carried frame is a
    grained one."""
    run = _composed_over_progressive(model16, clip7, lambda s: TI._woven(s, 'tff')[0], batch=1)
    vr = run(dict(mfi=3), mfi=3, interlace='tff')
    rn, edge = _stages(vr)
    assert vr.last_interlace_carried > 0 and [type(st) for st in edge.stages] == [Grain, Interlacer]


def test_in_front_of_the_requantisation(model16, clip7):
    """8 -> 10 -> 8: the grain is added at 10 bits and the dither sees it."""
    run = _composed_over_progressive(model16, clip7, lambda s: BD.requant_stream_np(s, 8, 'bayer'))
    vr = run(dict(mfi=2, work_depth=10, out_depth=10), mfi=2, work_depth=10, out_depth=8)
    rn, edge = _stages(vr)
    assert [type(st) for st in edge.stages] == [Grain, Requantizer] and vr.last_depth_requantised == 9 and edge.stages[0].depth == 10


def test_with_repeated_frames_and_the_flush(model16, clip7):
    data = D._repeat(clip7, [1, 2, 1, 1, 2, 1, 1])
    vr, _ = _composed(model16, data, mfi=2, dedup=True)
    assert vr.last_dups == [2, 6]
    run = _composed_over_progressive(model16, data, lambda s: TI._woven(s, 'tff')[0])
    vr = run(dict(mfi=2, dedup=True), mfi=2, dedup=True, interlace='tff')       # the open frame is flushed through the weave
    assert vr.last_dups == [2, 6] and vr.last_grain_payloads % 2 == 1


def test_with_a_crop_the_bars_stay_exact_black(model16):
    boxed, rect = Y._clip(6, 80, 96, '420', 8, seed=2)[0], (8, 72, 0, 96)
    vr, cropped = _composed(model16, boxed, mfi=3, crop=(8, 8, 0, 0), crop_output='cropped')
    assert vr.last_crop == rect
    head, pays = D._split(cropped)
    exp = [LB.pad_payload_np(np.frombuffer(p, np.uint8), 80, 96, 8, '420', rect) for p in pays]
    vr, nw, nf, got = _run(model16, boxed, mfi=3, crop=(8, 8, 0, 0), **GKW)
    ghead, gpays = D._split(got)
    assert ghead.startswith(b'YUV4MPEG2 W96 H80 ') and len(gpays) == len(exp)
    for g, e in zip(gpays, exp):
        g = np.frombuffer(g, np.uint8)
        assert np.array_equal(g, e)
        assert (g[:8 * 96] == 16).all() and (g[72 * 96:80 * 96] == 16).all() and (g[80 * 96:80 * 96 + 4 * 48] == 128).all()


def test_with_tiles(model16):
    vr, _ = _composed(model16, Y._clip(5, 96, 128, '420', 8, seed=4)[0], batch=1, mfi=3, tile=(64, 64), tile_margin=16)
    assert vr.last_plan is not None and vr.last_plan.n_tiles > 1


def test_a_10_bit_422_stream(model16):
    vr, _ = _composed(model16, Y._clip(6, 64, 96, '422', 10, seed=3)[0], mfi=3, high_depth=True, layouts=True)
    assert (vr.last_depth, vr.last_layout) == (10, '422')


def test_no_strength_builds_no_stage(model16, clip7):
    plain_vr, nw, nf, plain = _run(model16, clip7, mfi=2)
    vr, nw, nf, got = _run(model16, clip7, mfi=2, grain=0, grain_size=2, grain_seed=5)
    assert got == plain and vr.grain is None and vr.last_grain is None and vr.last_grain_payloads == 0
    for v in (plain_vr, vr):
        rn, edge = _stages(v)
        assert len(edge.stages) == 0 and edge.written is edge.yuv_out and rn.grain_payloads == 0 and edge.spec.grain is None


def test_seeds(model16, clip7):
    a = _run(model16, clip7, mfi=2, grain=2, grain_seed=1)[3]
    b = _run(model16, clip7, batch=1, mfi=2, grain=2, grain_seed=1)[3]
    c = _run(model16, clip7, mfi=2, grain=2, grain_seed=2)[3]
    assert a == b and a != c and len(a) == len(c)


def test_refusals_before_anything_runs(model16, clip7, tmp_path):
    for kw in (dict(grain='8.5'), dict(grain=-1), dict(grain=2, grain_size=3), dict(grain=2, grain_chroma='1.01'), dict(grain_size=1),
               dict(grain_curve='film'), dict(grain=2, grain_curve='log'), dict(grain=2, grain_seed=1 << 32)):
        with pytest.raises(ValueError):
            VideoRunner(model16, 2, mfi=2, **kw)
    src = tmp_path / 'in.y4m'
    src.write_bytes(clip7)
    vr = VideoRunner(model16, 2, mfi=2, grain=2)
    with pytest.raises(ValueError, match='grain with 2 ranks.*one rank'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'), world=2, rank=0)
    assert not vr._runners and not (tmp_path / 'out.y4m').exists()


def test_cli_through_pipes(model16, clip7):
    """The command line is what this test is about: the five switches reach the runner, the stream owns stdout, the JSON line gains ``grain``."""
    plain = _run(model16, clip7, mfi=2)[3]
    exp = G.grain_stream_np(plain, (24, 2, 4, 'flat', 42))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '2', '--matrix',
                        'bt601', '--grain', '1.5', '--grain-size', '2', '--grain-chroma', '0.25', '--grain-curve', 'flat', '--grain-seed', '0x2a'],
                       input=clip7, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['grain'] == {'strength': 1.5, 'size': 2, 'chroma': 0.25, 'curve': 'flat', 'seed': 42, 'payloads': 9}
    assert (last['windows'], last['frames_written']) == (4, 9)
