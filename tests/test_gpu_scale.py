"""Resized output (``--scale``) on a real MI355X: ``demfi_payload_scale`` (csrc/scale.hip) equal to ``scale.scale_payload_np`` byte for
byte, and ``VideoRunner(scale=...)`` byte-identical, header included, to an expectation that never runs the new code: the stream a run
WITHOUT the switch writes from the same input, resized on the host by ``scale.scale_stream_np`` (with ``--interlace``: the progressive
stream resized on the host, then woven by ``interlace.weave_stream_np``).  The clips, the model and the stream helpers are those of
tests/test_gpu_y4m_layouts.py, tests/test_gpu_dedup.py and tests/test_gpu_interlace.py."""
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
from demfi_amd import scale as SC                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from demfi_amd.y4m_edge import Scaler                                                # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_interlace as TI                                           # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
POISON = 0xC3
KINDS = {'bytes': (1, 8), '10-bit': (2, 10), '16-bit': (2, 16)}          # sample bytes, depth (peak = 2^depth - 1)
WIDTHS, HEIGHTS = (1, 63, 64, 65, 130), (1, 15, 16, 17, 33)              # output sizes on either side of the tile's edges
RATIOS = ((4, 1), (1, 8), (37, 35), (33, 40))                            # n_in : n_out


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _sources(shapes, es, depth, seed):
    """Four source payloads of the planes ``shapes``: a random one over the whole range, an all-zero one, an all-peak one and one whose
    rows alternate between peak and 0 (every plane's row 0 at peak): [4, P es] bytes."""
    rng = np.random.default_rng(seed)
    peak, P = (1 << depth) - 1, sum(r * c for r, c in shapes)
    x = rng.integers(0, peak + 1, (4, P)).astype('<u2' if es == 2 else np.uint8)
    x[1], x[2] = 0, peak
    x[3] = np.concatenate([np.where(np.arange(r)[:, None] % 2 == 0, peak, 0).repeat(c, 1).reshape(-1) for r, c in shapes])
    return x.view(np.uint8).reshape(4, P * es)


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

    def run(self, shapes_in, shapes_out, es, peak, filt):
        """One launch -> the resized rows [n, Pb]; the poisoned bytes between the rows of dst and behind the last one come back untouched,
        and so do the sources."""
        self.dst.fill_(POISON)
        pin, pout = np.ascontiguousarray(shapes_in, np.int32), np.ascontiguousarray(shapes_out, np.int32)
        blob, desc = SC.table_blob(shapes_in, shapes_out, filt)
        tables = torch.from_numpy(blob).to(DEV)
        L.check(L.load().demfi_payload_scale(self.dev.data_ptr(), self.table.ctypes.data, self.od.data_ptr(), self.n, pin.ctypes.data,
                                             pout.ctypes.data, len(pin), es, peak, tables.data_ptr(), desc.ctypes.data, self.dst.data_ptr(),
                                             self.stride, torch.cuda.current_stream().cuda_stream), 'payload_scale')
        torch.cuda.synchronize()
        out = self.dst.cpu().numpy()
        body = out[:self.n * self.stride].reshape(self.n, self.stride)
        assert (body[:, self.Pb:] == POISON).all() and (out[self.n * self.stride:] == POISON).all(), 'write outside the payloads'
        assert np.array_equal(self.dev.cpu().numpy(), self.buf), 'a source was written'
        return body[:, :self.Pb]


def _ref_planes(src, shapes_in, shapes_out, es, depth, filt):
    """``scale.resize_plane_np`` of every plane of the source payload ``src`` (bytes) -> the bytes of the resized payload."""
    smp = src.view('<u2') if es == 2 else src
    out, pos = [], 0
    for (ri, ci), (ro, co) in zip(shapes_in, shapes_out):
        out.append(SC.resize_plane_np(smp[pos:pos + ri * ci].reshape(ri, ci), ro, co, filt, (1 << depth) - 1).reshape(-1))
        pos += ri * ci
    return np.concatenate(out).view(np.uint8)


def _check(shapes_in, shapes_out, es, depth, filt, n=4, seed=0):
    """The planes ``shapes_in`` -> ``shapes_out`` of n payloads drawn from the four sources in a scattered order, on an aligned
    placement (word stores where the rows allow) and on bases one sample off a 16-byte boundary with a stride that keeps no row of dst
    aligned (sample stores), against the numpy rule."""
    src = _sources(shapes_in, es, depth, seed + 7 * sum(r + c for r, c in shapes_in))
    order = [(3, 0, 2, 1, 0, 3, 1)[i % 7] for i in range(n)]
    ref = {a: _ref_planes(src[a], shapes_in, shapes_out, es, depth, filt) for a in set(order)}
    exp = np.stack([ref[a] for a in order])
    Pb_in, Pb_out = src.shape[1], exp.shape[1]
    for shift, gap in ((0, 32 + -Pb_out % 16), (es, 3 * es)):
        got = _Launch(src, order, Pb_in, Pb_out, shift, gap).run(shapes_in, shapes_out, es, (1 << depth) - 1, filt)
        diff = int((got != exp).sum())
        if diff:
            print('%s -> %s es=%d depth=%d %s n=%d shift=%d: %d of %d bytes differ' % (shapes_in, shapes_out, es, depth, filt, n, shift, diff, exp.size))
        assert np.array_equal(got, exp), (shapes_in, shapes_out, es, depth, filt, n, shift)


def _n_in(n_out, ratio):
    return max(1, -(-n_out * ratio[0] // ratio[1]))


@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('filt', SC.FILTERS)
def test_kernel_equals_the_numpy_definition_around_the_tile_edges(filt, kind):
    """Output planes of 1, 63, 64, 65 and 130 columns by 1, 15, 16, 17 and 33 rows; each axis at one of the ratios 4:1 (24 taps under
    lanczos3), 1:8, 37:35 and 33:40, every ratio on every size over the two axes; random, all-zero, all-peak and alternating-row sources
    (the last drives the vertical sum past both ends of the range: the clip, and above 8 bits the 64-bit sum)."""
    es, depth = KINDS[kind]
    for i, (wo, ho) in enumerate(itertools.product(WIDTHS, HEIGHTS)):
        rx, ry = RATIOS[i % 4], RATIOS[(i // 4 + i) % 4]
        _check([(_n_in(ho, ry), _n_in(wo, rx))], [(ho, wo)], es, depth, filt, seed=i)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_the_named_ratios_and_one_sample_inputs(kind):
    es, depth = KINDS[kind]
    cases = [((64, 260), (16, 65)),                  # 4:1 on both axes
             ((80, 176), (15, 33)),                  # 16:3, the 32 taps of lanczos3 (bicubic 22, bilinear 12)
             ((3, 9), (24, 72)),                     # 1:8
             ((37, 37), (35, 35)), ((33, 33), (40, 40)),
             ((1, 1), (1, 1)), ((1, 1), (17, 70)), ((1, 20), (33, 5)), ((20, 1), (5, 130))]      # one-sample inputs
    for (filt, (sin, sout)) in itertools.product(SC.FILTERS, cases):
        _check([sin], [sout], es, depth, filt)


def test_shrinks_beyond_four_to_one_take_fewer_rows_per_tile():
    """16:1 under bilinear and 8:1 under bicubic (32 taps each): 16 output rows would need more source rows than a tile holds, so the
    entry point gives such a plane fewer rows per tile; and a plane whose axes go opposite ways."""
    for filt, (sin, sout), (es, depth) in (('bilinear', ((528, 70), (33, 70)), KINDS['bytes']), ('bicubic', ((264, 130), (33, 65)), KINDS['10-bit']),
                                           ('bilinear', ((330, 9), (33, 72)), KINDS['16-bit']), ('lanczos3', ((170, 20), (32, 66)), KINDS['bytes'])):
        _check([sin], [sout], es, depth, filt, n=2)


@pytest.mark.parametrize('layout', ['420', '422', '444', 'mono'])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_payloads_of_every_layout_with_odd_sizes(kind, layout):
    """Odd frame sizes, so the chroma planes have ratios of their own; n = 1, 3 and 7 payloads at scattered offsets; the payload
    reference is ``scale_payload_np`` itself."""
    es, depth = KINDS[kind]
    for k, ((h, w), (ho, wo), n) in enumerate((((37, 53), (35, 61), 3), ((33, 41), (71, 131), 1), ((66, 130), (17, 33), 7))):
        filt = SC.FILTERS[(k + len(layout)) % 3]
        sin, sout = IL.plane_shapes(h, w, layout), IL.plane_shapes(ho, wo, layout)
        _check(sin, sout, es, depth, filt, n=n, seed=k)
        src = _sources(sin, es, depth, 99)[0]
        smp = src.view('<u2') if es == 2 else src
        assert np.array_equal(SC.scale_payload_np(smp, h, w, ho, wo, depth, layout, filt).view(np.uint8), _ref_planes(src, sin, sout, es, depth, filt))


def test_more_payloads_than_the_grid_has_rows():
    shapes_in, shapes_out = IL.plane_shapes(4, 6, '420'), IL.plane_shapes(6, 4, '420')
    _check(shapes_in, shapes_out, 1, 8, 'bilinear', n=1400)              # 4200 (payload, plane) pairs over 4096 grid rows


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((96,), POISON, dtype=torch.uint8, device=DEV)
    table = np.array([0, 64], np.int64)
    od = torch.from_numpy(table).to(DEV)
    pin, pout = np.array([[2, 8], [1, 4], [1, 4]], np.int32), np.array([[2, 8], [1, 4], [1, 4]], np.int32)      # 24 samples either way
    blob, desc = SC.table_blob(pin.tolist(), pout.tolist(), 'bilinear')
    tables = torch.from_numpy(blob).to(DEV)
    fn = lib.demfi_payload_scale
    ok = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, pin.ctypes.data, pout.ctypes.data, 3, 1, 255, tables.data_ptr(), desc.ctypes.data,
          dst.data_ptr(), 32, st)

    def bad(i, v, **kw):
        a = list(ok)
        a[i] = v
        for k, x in kw.items():
            a[int(k[1:])] = x
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 2, 4, 5, 9, 10, 11))         # NULL buffers
    assert bad(3, -1) and bad(3, -3)                                     # n < 0
    assert all(bad(7, v) for v in (0, 3, 4))                             # sample_bytes
    assert all(bad(8, v) for v in (0, -1, 65536, 256))                   # peak (above 255 with bytes)
    assert all(bad(6, v) for v in (0, 4, -1))                            # no plane, more than three
    assert bad(12, 23)                                                   # dst_stride below the payload
    for tab in ([0, -1], [-16, 0]):
        assert bad(1, np.array(tab, np.int64).ctypes.data)               # a negative offset
    for pl in ([[0, 8], [1, 4], [1, 4]], [[2, 8], [1, 0], [1, 4]], [[2, 8], [1, 4], [40000, 4]]):
        p = np.array(pl, np.int32)
        assert bad(4, p.ctypes.data) and bad(5, p.ctypes.data)           # an empty or oversized plane, source or output
    for word, v in ((2, 33), (2, 0), (5, 33), (5, -2), (0, -4), (1, 3), (3, 2), (4, 1 << 20), (18, 16)):
        d = desc.copy()
        d[word] = v
        assert bad(10, d.ctypes.data), (word, v)                         # taps outside 1..32, table offsets negative, misaligned, behind the blob
    assert b'demfi_payload_scale' in lib.demfi_last_error()
    assert bad(1, np.array([1, 64], np.int64).ctypes.data, a7=2, a8=1023, a12=64)        # 16-bit samples at an odd offset, base, dst, stride
    assert bad(0, src.data_ptr() + 1, a7=2, a8=1023, a12=64) and bad(11, dst.data_ptr() + 1, a7=2, a8=1023, a12=48)
    assert bad(12, 49, a7=2, a8=1023)
    assert bad(9, tables.data_ptr() + 2)                                 # the blob off a 4-byte boundary
    huge = np.array([[32768, 32768], [32768, 32768]], np.int32)          # a payload of 2^31 bytes
    assert bad(4, huge.ctypes.data, a6=2) and bad(5, huge.ctypes.data, a6=2, a12=1 << 32)
    a = list(ok)
    a[3] = 0                                                             # no payload: nothing to do, nothing written
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    assert fn(*ok) == 0                                                  # the same size: the unit taps copy the payloads
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


SHRINK, ENLARGE = (72, 48), (128, 80)                                    # (w, h) around the 96x64 clips; rows on the 4:2:0 interlaced grid
_run, _run_file = TI._run, TI._run_file


def _scaled(plain, size, filt=None, order=None, lowpass=None):
    """The expectation: the stream ``plain`` resized on the host and, with ``order``, then woven.  Returns (bytes, payloads)."""
    out = SC.scale_stream_np(plain, size[0], size[1], filt)
    if order is not None:
        return TI._woven(out, order, lowpass)
    return out, out.count(b'FRAME\n')


def _composed(model, data, sizes=(SHRINK, ENLARGE), filt=None, batch=2, interlace=None, **kw):
    """``data`` with the switches ``kw`` and ``--scale`` == the stream of the same switches resized on the host, for a shrink and an
    enlargement: the stage sits behind whole payloads, whatever made the frames."""
    plain = _run(model, data, **kw)[3]
    phdr = y4m.parse_header(plain[:plain.index(b'\n') + 1], y4m.DEPTHS, y4m.LAYOUTS)
    skw = {'scale_filter': filt} if filt is not None else {}
    ikw = {'interlace': interlace} if interlace is not None else {}
    for size in sizes:
        exp, n_exp = _scaled(plain, size, filt, interlace)
        vr, nw, nf, got = _run(model, data, batch=batch, scale=size, **skw, **ikw, **kw)
        Y._same(got, exp)
        ohdr = y4m.parse_header(got[:got.index(b'\n') + 1], y4m.DEPTHS, y4m.LAYOUTS, fields=True)
        assert (ohdr.w, ohdr.h) == size != (phdr.w, phdr.h) and nf == n_exp > 0
        assert vr.last_scale == (size[0], size[1], filt or 'lanczos3') and vr.last_scale_payloads == plain.count(b'FRAME\n')
    return vr


@pytest.mark.parametrize('filt', [None, 'bicubic', 'bilinear'])
def test_a_stream_equals_the_host_resize_of_the_plain_stream(filt, model16, clip7, tmp_path):
    """The test that needs the feature: x2 through streams, a pipe and files at batches of 1, 2 and 4 windows with identical bytes."""
    plain = _run(model16, clip7, mfi=2)[3]
    skw = {'scale_filter': filt} if filt is not None else {}
    for size in (SHRINK, ENLARGE):
        exp, n_exp = _scaled(plain, size, filt)
        assert n_exp == 9 and exp != plain and exp.startswith(b'YUV4MPEG2 W%d H%d F48:1 Ip C420jpeg\n' % size)
        for batch, how in ((1, 'stream'), (2, 'pipe'), (4, 'file')):
            if how == 'file':
                vr, nw, nf, got = _run_file(model16, clip7, tmp_path, batch=batch, mfi=2, scale=size, **skw)
            else:
                vr, nw, nf, got = _run(model16, clip7, batch=batch, pipe=how == 'pipe', mfi=2, scale=size, **skw)
            Y._same(got, exp)
            assert (nw, nf) == (4, 9) and vr.scale == size + (filt or 'lanczos3',) == vr.last_scale and vr.last_scale_payloads == 9


def _cut_clip():
    return TI._cut_clip()


def test_a_rate_with_scene_cuts_on_the_full_length_timeline(model16):
    vr = _composed(model16, _cut_clip(), batch=1, fps=Fraction(60), scene_cut=S.DEFAULT_THRESHOLD, full_length=True)
    assert vr.last_cuts == [3] and vr.last_cut_windows >= 1 and vr.last_fps_out == 60


def test_a_10_bit_422_stream(model16):
    vr = _composed(model16, Y._clip(6, 64, 96, '422', 10, seed=3)[0], filt='bicubic', mfi=3, high_depth=True, layouts=True)
    assert (vr.last_depth, vr.last_layout) == (10, '422')


def test_with_tiles(model16):
    vr = _composed(model16, Y._clip(5, 96, 128, '420', 8, seed=4)[0], sizes=((100, 72), (160, 120)), batch=1, mfi=3, tile=(64, 64), tile_margin=16)
    assert vr.last_plan is not None and vr.last_plan.n_tiles > 1


def test_with_repeated_frames(model16, clip7):
    vr = _composed(model16, D._repeat(clip7, [1, 2, 1, 1, 2, 1, 1]), mfi=2, dedup=True)
    assert vr.last_dups == [2, 6]


def test_behind_the_shutter(model16, clip7):
    """The mixed frames are what is resized; 24 -> 60 at 360 degrees carries samples of open groups between batches."""
    vr = _composed(model16, clip7, batch=1, fps=Fraction(60), shutter=360)
    assert vr.last_shutter_carried > 0


def test_in_front_of_the_weave(model16, clip7):
    """``--interlace tff``: the progressive stream resized on the host, THEN woven: the scaler never sees fields, and the open frame that
    carries over between batches is a resized one."""
    vr = _composed(model16, clip7, batch=1, mfi=3, interlace='tff')
    assert vr.last_interlace == 't' and vr.last_interlace_carried > 0
    vr = _composed(model16, clip7, sizes=(SHRINK,), filt='bilinear', batch=1, fps=Fraction(60), shutter=360, interlace='bff')      # mix -> scale -> weave
    assert vr.last_shutter_carried > 0
    vr = _composed(model16, D._repeat(clip7, [1, 2, 1, 1, 2, 1, 1]), sizes=(ENLARGE,), mfi=2, dedup=True, interlace='tff')   # the flush
    assert vr.last_dups == [2, 6]


def test_interlaced_in_resized_and_interlaced_out(model16):
    """The standards conversion: 50i -> 59.94i at another size."""
    from tests import test_gpu_deint as DI
    fields = DI._interlaced(Y._clip(4, 64, 96, '420', 8, seed=6, fps=b'25:1')[0], 't')
    for mode in ('bob', 'adaptive'):
        vr = _composed(model16, fields, sizes=(SHRINK,), deinterlace=True, deinterlace_mode=mode, fps=Fraction(60000, 1001), interlace='tff')
        assert vr.last_fields == 'tff' and vr.last_fps_out == Fraction(30000, 1001)


def test_behind_the_inverse_telecine(model16):
    from demfi_amd import telecine as TC
    h, w = 64, 80
    head, pays = D._split(Y._clip(8, h, w, '420', 8, seed=5, fps=b'24000:1001')[0])
    tele = [t.view(np.uint8) for t in TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], h, w, 8, '420', 't', 0)]
    thead = b' '.join(b'F30000:1001' if f.startswith(b'F') else b'It' if f.startswith(b'I') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    vr = _composed(model16, thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele), sizes=((60, 48),), mfi=2, ivtc=True)
    assert len(vr.last_dropped) == 2


def test_with_a_crop_the_picture_rectangle_is_scaled(model16):
    boxed = Y._clip(6, 80, 96, '420', 8, seed=2)[0]
    vr = _composed(model16, boxed, mfi=3, crop=(8, 8, 0, 0), crop_output='cropped')
    assert vr.last_crop == (8, 72, 0, 96)
    with pytest.raises(ValueError, match='--crop-output cropped'):
        VideoRunner(model16, 2, mfi=3, crop=(8, 8, 0, 0), scale=SHRINK)
    with pytest.raises(ValueError, match='--crop-output cropped'):
        VideoRunner(model16, 2, mfi=3, crop=(8, 8, 0, 0), crop_output='pad', scale=SHRINK)


def test_two_ranks_in_file_mode(model16, clip7, tmp_path):
    """The stage keeps nothing between payloads, so a rank's block of windows is resized on its own and lands at its own offset."""
    plain = _run(model16, clip7, fps=Fraction(60))[3]
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(clip7)
    for size in (SHRINK, ENLARGE):
        exp, n_exp = _scaled(plain, size)
        tot = [0, 0]
        for rank in range(2):
            vr = VideoRunner(model16, 2, batch=2, matrix='bt601', fps=Fraction(60), scale=size)
            nw, nf = vr.run_file(str(src), str(dst), world=2, rank=rank)
            tot = [tot[0] + nw, tot[1] + nf]
            assert vr.last_scale_payloads == nf > 0
        Y._same(dst.read_bytes(), exp)
        assert tot == [4, n_exp]


def test_the_run_s_own_size_builds_no_scaler(model16, clip7):
    plain_vr, nw, nf, plain = _run(model16, clip7, mfi=2)
    for cr in plain_vr._runners.values():
        edge = cr.runner._pipeline.edge
        assert not any(isinstance(st, Scaler) for st in edge.stages) and edge.written is edge.yuv_out and cr.runner.scale_payloads == 0
    assert plain_vr.last_scale is None and plain_vr.last_scale_payloads == 0
    vr, nw, nf, got = _run(model16, clip7, mfi=2, scale=(96, 64), scale_filter='bicubic')
    assert got == plain and vr.last_scale is None and vr.last_scale_payloads == 0
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        assert not any(isinstance(st, Scaler) for st in edge.stages) and edge.written is edge.yuv_out and cr.runner.scale_payloads == 0
    vr, nw, nf, got = _run(model16, clip7, mfi=2, scale=SHRINK)
    for cr in vr._runners.values():
        edge = cr.runner._pipeline.edge
        (scaler,) = [st for st in edge.stages if isinstance(st, Scaler)]
        assert edge.written is scaler.out and cr.runner.scale_payloads == nf == 9
        assert edge.h_yuv[0].shape[1] == scaler.Pb == y4m.payload_size(48, 72) < edge.yuv_out[0].shape[1]   # only resized payloads cross D2H


def test_refusals_before_anything_runs(model16, clip7):
    with pytest.raises(ValueError, match='--scale with --interlace.*multiple of 4'):
        _run(model16, clip7, mfi=2, scale=(72, 50), interlace='tff')
    with pytest.raises(ValueError, match='--scale-filter.*--scale'):
        VideoRunner(model16, 2, mfi=2, scale_filter='bicubic')
    vr = VideoRunner(model16, 2, mfi=2, scale=(96, 10))                  # 64 -> 10 rows under lanczos3: more than 32 taps
    with pytest.raises(ValueError, match='more than 32'):
        vr.run_stream(io.BytesIO(clip7), io.BytesIO())
    assert not vr._runners


def test_cli_through_pipes(model16, clip7):
    """The command line is what this test is about: the two switches reach the runner, width comes first, the stream owns stdout, the
    header carries W, H and the pixel aspect that keeps the display aspect, the JSON line gains ``scale``."""
    data = clip7.replace(b' Ip ', b' Ip A16:15 ', 1)
    plain = _run(model16, data, mfi=2)[3]
    assert plain.startswith(b'YUV4MPEG2 W96 H64 F48:1 Ip A16:15 C420jpeg\n')
    exp = _scaled(plain, (72, 32), 'bicubic')[0]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '2', '--matrix',
                        'bt601', '--scale', '72x32', '--scale-filter', 'bicubic'],
                       input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    hdr = y4m.parse_header(p.stdout[:p.stdout.index(b'\n') + 1])
    assert (hdr.w, hdr.h, hdr.aspect) == (72, 32, '32:45')                # 16 * 96 * 32 : 15 * 64 * 72
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['scale'] == {'size': '72x32', 'filter': 'bicubic', 'resized': True, 'payloads': 9}
    assert (last['windows'], last['frames_written'], last['fps_out']) == (4, 9, '48')
