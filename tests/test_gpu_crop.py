"""Letterbox and pillarbox bars (``--crop``) on a real MI355X: ``demfi_luma_line_counts`` (csrc/crop.hip) equal to
``letterbox.line_counts_np`` integer for integer, and ``VideoRunner(crop=...)`` on a boxed clip byte-identical to an expectation that
never runs the new code: ``VideoRunner()`` without the switch on the picture clip the boxed one was made from, its output padded
on the host with ``letterbox.pad_payload_np``.  The clips, the model and the stream helpers are those of
tests/test_gpu_y4m_layouts.py, tests/test_gpu_dedup.py and tests/test_gpu_deint.py."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import telecine as TC                                                 # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_deint as DI                                               # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
GUARD = 0x5A5A5A5A


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _plane(h, w, sb, seed):
    """A luma plane (uint8, or uint16 samples at 10 bits) with dark bars at the top and on the left (about an eighth and a sixth of
    the frame, at black, 16 s), picture of every value from 1 to the peak in the rest, a few specks at the peak in the bars below
    row 0, and a last row at the peak: at the default limit row 0 counts nothing, the last row everything, the others in between."""
    rng = np.random.default_rng(seed)
    s, peak = (1, 255) if sb == 1 else (4, 1023)
    y = rng.integers(1, peak + 1, (h, w))
    y[:h // 8] = 16 * s
    y[:, :w // 6] = 16 * s
    for _ in range(3):
        y[rng.integers(1, max(h // 8, 2)), rng.integers(0, w)] = peak
        y[rng.integers(1, h), rng.integers(0, max(w // 6, 1))] = peak
    y[h - 1] = peak
    return y.astype(np.uint8 if sb == 1 else np.uint16).reshape(-1)


def _counts_gpu(buf, offs, h, w, sb, thresh):
    """buf: the bytes of a device buffer with planes at the byte offsets ``offs`` -> [(rows, cols)] per plane; the guard words around
    both outputs hold and the buffer is unchanged."""
    lib, n = L.load(), len(offs)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    od = torch.tensor(list(offs), dtype=torch.int64, device=DEV)
    rows = torch.from_numpy(np.full(n * h + 2, GUARD, np.uint32).view(np.int32)).to(DEV)
    cols = torch.from_numpy(np.full(n * w + 2, GUARD, np.uint32).view(np.int32)).to(DEV)
    L.check(lib.demfi_luma_line_counts(dev.data_ptr(), od.data_ptr(), n, h, w, sb, thresh, rows[1:].data_ptr(), cols[1:].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), 'luma_line_counts')
    torch.cuda.synchronize()
    r, c = rows.cpu().numpy().view(np.uint32), cols.cpu().numpy().view(np.uint32)
    assert r[0] == r[-1] == c[0] == c[-1] == GUARD, 'write outside the outputs'
    assert bytes(dev.cpu().numpy()) == bytes(np.ascontiguousarray(buf))
    return [(r[1 + i * h:1 + (i + 1) * h], c[1 + i * w:1 + (i + 1) * w]) for i in range(n)]


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
@pytest.mark.parametrize('h,w', [(2, 2), (2, 7), (9, 17), (33, 47), (64, 64), (65, 257), (70, 1030), (1088, 1920)])
def test_kernel_equals_the_numpy_definition(h, w, sb):
    depth = 8 if sb == 1 else 10
    plane = _plane(h, w, sb, h * 31 + w)
    buf = np.concatenate([plane.view(np.uint8), np.full(64, 0xEE, np.uint8)])
    peak = (1 << depth) - 1
    for thresh in (0, LB.DEFAULT_LIMIT << (depth - 8), peak):
        er, ec = LB.line_counts_np(plane, h, w, thresh)
        (gr, gc), = _counts_gpu(buf, [0], h, w, sb, thresh)
        print('%dx%d, %d bytes per sample, threshold %d: lit samples kernel %d numpy %d' % (h, w, sb, thresh, gr.sum(), er.sum()))
        assert np.array_equal(gr, er) and np.array_equal(gc, ec)
        if thresh == peak:
            assert er.sum() == 0
        elif thresh == 0:
            assert (er == w).all() and (ec == h).all()           # every sample is lit: full counts
        elif h >= 33:                                            # zero, partial and full counts all occur
            assert er[0] == 0 and er[h - 1] == w and ((er > 0) & (er < w // 6)).any() and ((er > w // 2) & (er < w)).any()
            assert ((ec > 0) & (ec < h // 8)).any() and ((ec > h // 2) & (ec < h)).any()


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
def test_a_batch_of_planes_at_unaligned_offsets(sb):
    h, w = 37, 61                                        # rows start at every alignment
    depth = 8 if sb == 1 else 10
    planes = [_plane(h, w, sb, 40 + i) for i in range(3)]
    buf, offs = [], []
    for p, gap in zip(planes, [3, 5, 1] if sb == 1 else [2, 6, 10]):      # byte offsets: odd for bytes, 2 mod 4 for samples
        buf.append(np.full(gap, 0xEE, np.uint8))
        offs.append(sum(b.size for b in buf))
        buf.append(p.view(np.uint8))
    buf = np.concatenate(buf + [np.full(64, 0xEE, np.uint8)])
    assert all(o % 2 == 1 for o in offs) if sb == 1 else all(o % 4 == 2 for o in offs)
    order = [2, 0, 1, 2]                                 # not monotonic, one plane twice
    got = _counts_gpu(buf, [offs[i] for i in order], h, w, sb, LB.DEFAULT_LIMIT << (depth - 8))
    for (gr, gc), i in zip(got, order):
        er, ec = LB.line_counts_np(planes[i], h, w, LB.DEFAULT_LIMIT << (depth - 8))
        assert np.array_equal(gr, er) and np.array_equal(gc, ec)
    assert not np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[3][1])


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(2, dtype=torch.int64, device=DEV)
    rows = torch.full((5,), 0x5A5A, dtype=torch.int32, device=DEV)
    cols = torch.full((2,), 0x5A5A, dtype=torch.int32, device=DEV)
    fn = lib.demfi_luma_line_counts
    ok = (buf.data_ptr(), offs.data_ptr(), 1, 5, 2, 1, 24, rows.data_ptr(), cols.data_ptr(), st)

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 7, 8)) and bad(2, -1)
    assert all(bad(i, v) for i in (3, 4) for v in (1, 16385)) and all(bad(5, v) for v in (0, 3, 4))
    assert bad(6, -1) and bad(6, 65536)
    a = list(ok)
    a[0], a[5] = buf.data_ptr() + 1, 2                       # 16-bit samples at an odd address
    assert fn(*a) == ERR_ARG
    assert b'demfi_luma_line_counts' in lib.demfi_last_error()
    a = list(ok)
    a[2] = 0                                                 # no plane: nothing to do, nothing written
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((rows == 0x5A5A).all()) and bool((cols == 0x5A5A).all()) and bool((buf == 0xA5).all())
    assert fn(*ok) == 0
    torch.cuda.synchronize()
    assert rows.tolist() == [2] * 5 and cols.tolist() == [5] * 2 and bool((buf == 0xA5).all())       # 0xA5 = 165 > 24 everywhere
    assert L.ABI_VERSION == 8                                # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _bright(i, bgr, peak):
    """The clip's frames lifted off black, so that every row and column of the picture is lit."""
    return (bgr // 2 + peak // 4).astype(bgr.dtype)


def _resize(head, h, w):
    return b' '.join(b'W%d' % w if f[:1] == b'W' else b'H%d' % h if f[:1] == b'H' else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'


def _boxed(data, bars, **reader_kw):
    """(the stream with every payload padded on the host by the bar widths (T, B, L, R), the rectangle of the picture in it, its
    frame size)."""
    at = data.index(b'FRAME\n')
    hdr = y4m.parse_header(data[:at], y4m.DEPTHS, y4m.LAYOUTS, **reader_kw)
    t, b, l, r = bars
    H, W = hdr.h + t + b, hdr.w + l + r
    rect = (t, t + hdr.h, l, l + hdr.w)
    step = 6 + hdr.payload
    pays = [np.frombuffer(data[i + 6:i + step], np.uint8) for i in range(at, len(data), step)]
    out = [LB.pad_payload_np(p, H, W, hdr.depth, hdr.layout, rect, hdr.full_range).tobytes() for p in pays]
    return _resize(data[:at], H, W) + b''.join(b'FRAME\n' + p for p in out), rect, (H, W)


def _run(model, data, **kw):
    vr = VideoRunner(model, 2, batch=kw.pop('batch', 4), matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _run_file(model, data, tmp_path, world=1, **kw):
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tot, vrs = [0, 0], []
    for rank in range(world):
        vr = VideoRunner(model, 2, batch=kw.get('batch', 4 if world == 1 else 2), matrix='bt601', **{k: v for k, v in kw.items() if k != 'batch'})
        nw, nf = vr.run_file(str(src), str(dst), world=world, rank=rank)
        tot[0] += nw
        tot[1] += nf
        vrs.append(vr)
    return vrs, tuple(tot), dst.read_bytes()


def _check(model, pic, bars, tmp_path=None, world=1, crop='auto', pipe=False, reader_kw={}, crop_kw={}, **kw):
    """The boxed clip with ``crop`` == the picture clip without it, padded on the host; returns (the cropped run's runners, bytes)."""
    boxed, rect, (H, W) = _boxed(pic, bars, **reader_kw)
    ve, nwe, nfe, exp_pic = _run(model, pic, **kw)
    exp = _boxed(exp_pic, bars)[0]
    assert exp[:exp.index(b'FRAME\n')] == _resize(exp_pic[:exp_pic.index(b'FRAME\n')], H, W)
    if crop != 'auto':
        crop = bars
    if tmp_path is not None:
        vrs, (nw, nf), got = _run_file(model, boxed, tmp_path, world, crop=crop, **crop_kw, **kw)
    else:
        vr = VideoRunner(model, 2, batch=kw.pop('batch', 4), matrix='bt601', crop=crop, **crop_kw, **kw)
        out = io.BytesIO()
        nw, nf = vr.run_stream(D._Pipe(boxed) if pipe else io.BytesIO(boxed), out)
        vrs, got = [vr], out.getvalue()
    assert (nw, nf) == (nwe, nfe) and nf > 0
    Y._same(got, exp)
    for vr in vrs:
        assert vr.last_crop == rect and vr.last_crop_note is None
        assert vr.last_cuts == ve.last_cuts or world > 1
    assert ve.last_crop is None and ve.last_crop_probed == 0
    return vrs, got


def test_a_auto_on_a_letterboxed_file_on_one_rank_and_two(model16, tmp_path):
    """The test that needs the feature: scope picture in a taller container, bars found by the pre-pass."""
    n = 7
    pic = Y._clip(n, 64, 96, '420', 8, seed=3, look=_bright)[0]
    (vr,), got = _check(model16, pic, (16, 18, 0, 0), tmp_path, mfi=2)
    assert vr.last_crop_probed == n and got.startswith(b'YUV4MPEG2 W96 H98 F48:1 Ip ')
    vrs, got2 = _check(model16, pic, (16, 18, 0, 0), tmp_path, world=2, mfi=2, crop_kw={'crop_probe': 3})
    assert [v.last_crop_probed for v in vrs] == [3, 3] and got2 == got
    plain = _run(model16, _boxed(pic, (16, 18, 0, 0))[0], mfi=2)[3]            # without the switch the network runs over the bars
    assert len(plain) == len(got) and plain != got


def test_b_a_pipe_with_an_explicit_rectangle_at_a_non_integer_ratio_422p10(model16):
    pic = Y._clip(7, 64, 80, '422', 10, seed=4, look=_bright)[0]
    (vr,), got = _check(model16, pic, (3, 5, 8, 6), crop='bars', pipe=True, fps=Fraction(60), high_depth=True, layouts=True)
    assert vr.last_fps_out == 60 and vr.last_crop_probed == 0 and (vr.last_depth, vr.last_layout) == (10, '422')
    assert got.startswith(b'YUV4MPEG2 W94 H72 F60:1 Ip C422p10\n')


def test_c_cropped_output_is_the_run_of_the_picture_clip(model16, tmp_path):
    pic = Y._clip(6, 64, 96, '420', 8, seed=5, look=_bright)[0]
    boxed, rect, _ = _boxed(pic, (0, 0, 16, 16))                               # pillarbox
    exp = _run(model16, pic, mfi=2)[3]
    vr, nw, nf, got = _run(model16, boxed, mfi=2, crop=(0, 0, 16, 16), crop_output='cropped')
    assert vr.last_crop == rect and got == exp and got.startswith(b'YUV4MPEG2 W96 H64 ')
    (vr,), tot, got = _run_file(model16, boxed, tmp_path, crop='auto', crop_output='cropped', mfi=2)
    assert vr.last_crop == rect and tot == (nw, nf) and got == exp


def test_d_scene_cut_on_a_planted_cut_with_full_length(model16, tmp_path):
    cut = 5

    def look(i, bgr, peak):                                                     # a hard cut before frame 5: another scene's colours
        b = _bright(i, bgr, peak)
        return b if i < cut else (peak - b // 2).astype(b.dtype)
    pic = Y._clip(9, 64, 96, '420', 8, seed=1, look=look)[0]
    kw = dict(mfi=2, scene_cut=S.DEFAULT_THRESHOLD, full_length=True)
    (vr,), got = _check(model16, pic, (8, 8, 0, 0), tmp_path, **kw)
    assert vr.last_cuts == [cut] and vr.last_cut_windows >= 1
    _check(model16, pic, (8, 8, 0, 0), crop='bars', **kw)                       # and through run_stream


def test_e_interlaced_payloads_are_cropped_in_units_of_four_rows(model16):
    pic = DI._interlaced(Y._clip(5, 64, 96, '420', 8, seed=6, fps=b'25:1', look=_bright)[0], 't')
    (vr,), got = _check(model16, pic, (8, 4, 0, 0), crop='bars', reader_kw={'fields': True}, mfi=2, deinterlace=True)
    assert vr.last_fields == 'tff' and got.startswith(b'YUV4MPEG2 W96 H76 F100:1 Ip ')
    boxed = _boxed(pic, (6, 6, 0, 0), fields=True)[0]                           # even, but not whole row pairs of both fields
    with pytest.raises(ValueError, match='multiples of 4 rows'):
        VideoRunner(model16, 2, mfi=2, deinterlace=True, crop=(6, 6, 0, 0)).run_stream(io.BytesIO(boxed), io.BytesIO())


def test_f_inverse_telecine_with_auto_on_a_file(model16, tmp_path):
    h, w = 64, 80
    film = Y._clip(12, h, w, '420', 8, seed=5, fps=b'24000:1001', look=_bright)[0]
    head, pays = D._split(film)
    tele = [t.view(np.uint8) for t in TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], h, w, 8, '420', 't', 0)]
    thead = b' '.join(b'F30000:1001' if f.startswith(b'F') else b'It' if f.startswith(b'I') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    pic = thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele)
    # a top bar of whole 16x16 blocks: the comb scorer, which keeps the full size, cuts the picture into the blocks of the unboxed clip
    (vr,), got = _check(model16, pic, (16, 12, 0, 0), tmp_path, reader_kw={'telecine': True}, mfi=2, ivtc=True)
    assert vr.last_crop_probed == 15 and len(vr.last_dropped) == 3 and vr.last_fps_out == Fraction(48000, 1001)
    assert got.startswith(b'YUV4MPEG2 W80 H92 F48000:1001 Ip ')


def test_g_windowbox_on_all_four_sides_with_tiles(model16, tmp_path):
    pic = Y._clip(5, 96, 160, '420', 8, seed=4, look=_bright)[0]
    (vr,), _ = _check(model16, pic, (10, 12, 16, 14), tmp_path, mfi=2, batch=2, tile=(64, 96), tile_margin=16)
    assert vr.last_plan is not None and vr.last_plan.n_tiles == 4 and (vr.last_plan.h, vr.last_plan.w) == (96, 160)


def test_h_a_clip_without_bars_and_an_all_black_clip_are_left_alone(model16, tmp_path):
    h, w, n = 64, 96, 5
    pic = Y._clip(n, h, w, '420', 8, seed=2, look=_bright)[0]
    black = pic[:pic.index(b'FRAME\n')] + (b'FRAME\n' + bytes([16]) * (h * w) + bytes([128]) * (h * w // 2)) * n
    for data, note in ((pic, None), (black, 'no probed frame has picture')):
        exp = _run_file(model16, data, tmp_path, mfi=2)[2]
        (vr,), _, got = _run_file(model16, data, tmp_path, mfi=2, crop='auto')
        assert vr.last_crop is None and vr.last_crop_probed == n and got == exp
        assert vr.last_crop_note == note or note in vr.last_crop_note
        assert _run(model16, data, mfi=2, crop=(0, 0, 0, 0))[3] == exp          # no bars given: no crop stage either
    small = _boxed(Y._clip(n, 48, 80, '420', 8, seed=2, look=_bright)[0], (16, 16, 0, 0))[0]      # a picture below 64 rows: whole, reported
    (vr,), _, got = _run_file(model16, small, tmp_path, mfi=2, crop='auto')
    assert vr.last_crop is None and '80x48' in vr.last_crop_note and got == _run(model16, small, mfi=2)[3]
