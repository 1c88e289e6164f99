"""10- to 16-bit Y4M video as tiles (``--tile`` with ``--high-depth`` and ``--tile-high-depth``) on a real MI355X.  The two kernels that
address a tile inside full frames (csrc/frames16.hip): ``demfi_u16_ingest_rect`` against ``demfi_u16_ingest`` on the contiguous crop,
``demfi_frame_to_u16_rect`` against ``tiling.stitch_np`` of the per-tile ``demfi_frame_to_u16`` results, between guards.  Then the video
path against the composition it stands for: numpy payload -> BGR16, ``tiling.crop_np``, every run of every window per tile in ONE
``run_windows_u16`` of an untiled tile-sized runner, ``tiling.stitch_np``, numpy BGR16 -> payload.  Every compare is exact: the same
kernels and the same arithmetic on the same pixels."""
import ctypes as C
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict, synthetic_window   # noqa: E402
from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import cadence as K                                                   # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
GUARD = 0xA5C3
ERR_ARG = -1
ANY = {'depths': y4m.DEPTHS, 'layouts': y4m.LAYOUTS}
H, W, TILE, MARGIN = 96, 160, (64, 96), 16

# the plans of tests/test_gpu_tiling.py
KERNEL_PLANS = [(96, 160, (64, 96), 16), (97, 131, (64, 96), 0), (70, 1283, (70, 320), 32), (131, 97, (96, 64), 8), (40, 100, (32, 64), 4),
                (50, 97, (32, 96), 0)] + [(33, 64 + r, (32, 64), 0) for r in range(1, 17)]


def _dev16(a):
    """uint16 numpy array -> int16 GPU tensor holding the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(DEV)


def _np16(t):
    return t.cpu().numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pad32(n):
    return (n + 31) // 32 * 32


# ---- 1. the ingest of a rectangle ----------------------------------------------------------------------------------------------
def _ingest(fn, frames, args, H_, W_, dt, dtype):
    x = torch.zeros(3, 4, H_, W_, device=DEV)
    s2d = torch.zeros(H_ // 2, W_ // 2, 48, device=DEV, dtype=dtype)
    ov = torch.zeros(3, H_, W_, device=DEV)
    ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in frames])
    L.check(fn(ptrs, *args, x.data_ptr(), s2d.data_ptr(), ov.data_ptr(), dt, H_, W_, _stream()), 'ingest')
    torch.cuda.synchronize()
    return x, s2d, ov


# reflect padding on both axes at even and odd x0 and in the frame's far corner; no padding
RECTS = [(50, 70, 64, 96, 0, 0), (50, 70, 64, 96, 20, 61), (50, 70, 64, 96, 7, 33), (50, 70, 64, 96, 13, 2), (64, 96, 64, 96, 6, 35)]


@pytest.mark.parametrize('h,w,H_,W_,y0,x0', RECTS)
@pytest.mark.parametrize('d', [8, 10, 16])
def test_ingest_rect_equals_the_ingest_of_the_crop(h, w, H_, W_, y0, x0, d):
    lib, (fh, fw) = L.load(), (70, 131)
    g = np.random.RandomState(d * 100 + y0 + x0)
    full = [g.randint(0, 1 << d, (fh, fw, 3)).astype(np.uint16) for _ in range(4)]
    full[0][y0:y0 + 2, x0:x0 + 3] = [[[0, (1 << d) - 1, (1 << d) // 2]] * 3] * 2
    dev = [_dev16(f) for f in full]
    before = [f.clone() for f in dev]
    crops = [f[y0:y0 + h, x0:x0 + w].contiguous() for f in dev]
    for dtype, dt in ((torch.float16, L.F16), (torch.float32, L.F32)):
        ref = _ingest(lib.demfi_u16_ingest, crops, (h, w, d), H_, W_, dt, dtype)
        got = _ingest(lib.demfi_u16_ingest_rect, dev, (fh, fw, y0, x0, h, w, d), H_, W_, dt, dtype)
        for name, a, b in zip(('x', 's2d', 'overlay'), got, ref):
            assert torch.equal(a, b), (name, dtype)
        assert float(ref[0].std()) > 0.1
        # the whole frame as its own rectangle is the plain ingest
        whole = _ingest(lib.demfi_u16_ingest_rect, crops, (h, w, 0, 0, h, w, d), H_, W_, dt, dtype)
        for a, b in zip(whole, ref):
            assert torch.equal(a, b), dtype
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


# ---- 2. the egress of a kept rectangle -----------------------------------------------------------------------------------------
def test_the_kernel_plans_cover_every_destination_alignment():
    """A pixel is 6 bytes: over the plans the first kept column of a tile starts at every even residue modulo 16."""
    res = {6 * t.keep.x0 % 16 for h, w, tile, m in KERNEL_PLANS for t in T.plan_tiles(h, w, tile, m).tiles}
    assert res == set(range(0, 16, 2))


def _tile_outputs(p, seed):
    """One random fp32 [3, H, W] network output per tile, H x W the tile padded to multiples of 32; values below -1 and above 1."""
    th, tw = p.tile
    g = torch.Generator().manual_seed(seed)
    fr = torch.randn(p.n_tiles, 3, _pad32(th), _pad32(tw), generator=g) * 0.8
    assert bool((fr < -1).any()) and bool((fr > 1).any())
    return fr.to(DEV)


def _per_tile_u16(fr, p, d):
    """[n_tiles, th, tw, 3] uint16: ``demfi_frame_to_u16`` of every tile output."""
    lib, (th, tw) = L.load(), p.tile
    out = torch.zeros((p.n_tiles, th, tw, 3), dtype=torch.int16, device=DEV)
    for j in range(p.n_tiles):
        L.check(lib.demfi_frame_to_u16(fr[j].data_ptr(), out[j].data_ptr(), th, tw, fr.shape[2], fr.shape[3], d, _stream()), 'to_u16')
    torch.cuda.synchronize()
    return _np16(out)


def _guarded(h, w, lead):
    """A guard-filled buffer holding an [h,w,3] frame behind 3 guard rows and ``lead`` samples, with 3 guard rows after it:
    (buffer, sample offset of the frame)."""
    at = 3 * w * 3 + lead
    return _dev16(np.full(at + h * w * 3 + 3 * w * 3 + 8, GUARD, np.uint16)), at


def _to_rect(fr, buf, at, p, j, d):
    t, lib = p.tiles[j], L.load()
    L.check(lib.demfi_frame_to_u16_rect(fr[j].data_ptr(), buf.data_ptr() + 2 * at, p.h, p.w, t.src.y0, t.src.x0, t.keep.y0, t.keep.x0,
                                        t.keep.y1, t.keep.x1, fr.shape[2], fr.shape[3], d, _stream()), 'to_u16_rect')


@pytest.mark.parametrize('h,w,tile,margin', KERNEL_PLANS)
@pytest.mark.parametrize('d', [10, 16])
def test_frame_to_u16_rect_is_stitch_of_the_per_tile_frames(h, w, tile, margin, d):
    p = T.plan_tiles(h, w, tile, margin)
    fr = _tile_outputs(p, h * 1000 + w + d)
    exp_frame = T.stitch_np(_per_tile_u16(fr, p, d), p, h, w)
    lead = (7 * h + w) % 8                                    # frames at every 2-byte alignment of a 16-byte line
    buf, at = _guarded(h, w, lead)
    for j in range(p.n_tiles):
        _to_rect(fr, buf, at, p, j, d)
    torch.cuda.synchronize()
    exp = np.full(buf.numel(), GUARD, np.uint16)
    exp[at:at + h * w * 3] = exp_frame.reshape(-1)
    assert np.array_equal(_np16(buf), exp)
    # one tile alone: its kept rectangle and nothing else
    j = p.n_tiles - 1
    buf, at = _guarded(h, w, lead)
    _to_rect(fr, buf, at, p, j, d)
    torch.cuda.synchronize()
    k = p.tiles[j].keep
    one = np.full((h, w, 3), GUARD, np.uint16)
    one[k.y0:k.y1, k.x0:k.x1] = exp_frame[k.y0:k.y1, k.x0:k.x1]
    exp = np.full(buf.numel(), GUARD, np.uint16)
    exp[at:at + h * w * 3] = one.reshape(-1)
    assert np.array_equal(_np16(buf), exp)


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), _stream()
    frames = _dev16(np.full(70 * 131 * 3 + 8, GUARD, np.uint16))
    buf = _dev16(np.full(96 * 160 * 3 + 8, GUARD, np.uint16))
    f32 = torch.full((12 * 64 * 96,), 0.25, device=DEV)
    ptrs = (C.c_void_p * 4)(*[frames.data_ptr()] * 4)

    def bad(fn, ok, i, v):
        a = list(ok)
        a[i] = v
        return fn(*a) == ERR_ARG
    fn = lib.demfi_u16_ingest_rect      # frames, fh, fw, y0, x0, h, w, depth, x, s2d, overlay, dtype, H, W, stream
    ok = (ptrs, 70, 131, 7, 33, 50, 70, 10, f32.data_ptr(), f32.data_ptr(), f32.data_ptr(), L.F32, 64, 96, st)
    assert bad(fn, ok, 3, -1) and bad(fn, ok, 4, -1) and bad(fn, ok, 3, 21) and bad(fn, ok, 4, 62)       # the rectangle leaves the frame
    assert bad(fn, ok, 1, 56) and bad(fn, ok, 2, 102) and bad(fn, ok, 3, 2 ** 31 - 1) and bad(fn, ok, 4, 2 ** 31 - 1)
    assert bad(fn, ok, 7, 7) and bad(fn, ok, 7, 17)                                                      # depth
    assert bad(fn, ok, 5, 1) and bad(fn, ok, 12, 63) and bad(fn, ok, 13, 69) and bad(fn, ok, 11, 9)      # the checks of demfi_u16_ingest
    assert bad(fn, ok, 0, None) and bad(fn, ok, 8, None) and bad(fn, ok, 9, None) and bad(fn, ok, 10, None)
    assert bad(fn, ok, 0, (C.c_void_p * 4)(frames.data_ptr(), frames.data_ptr() + 1, frames.data_ptr(), frames.data_ptr()))
    assert bad(fn, ok, 0, (C.c_void_p * 4)(frames.data_ptr(), None, frames.data_ptr(), frames.data_ptr()))
    assert b'demfi_u16_ingest_rect' in lib.demfi_last_error()
    fn = lib.demfi_frame_to_u16_rect    # frame, out, fh, fw, y0, x0, ky0, kx0, ky1, kx1, H, W, depth, stream
    ok = (f32.data_ptr(), buf.data_ptr(), 96, 160, 32, 64, 40, 80, 96, 160, 64, 96, 10, st)
    assert bad(fn, ok, 6, 96) and bad(fn, ok, 7, 160) and bad(fn, ok, 8, 40) and bad(fn, ok, 9, 79)      # an empty kept rectangle
    assert bad(fn, ok, 6, 31) and bad(fn, ok, 7, 63) and bad(fn, ok, 4, 31) and bad(fn, ok, 5, 63)       # ... outside its tile
    assert bad(fn, ok, 8, 97) and bad(fn, ok, 9, 161) and bad(fn, ok, 2, 95) and bad(fn, ok, 3, 159)     # ... outside the frame
    assert bad(fn, ok, 4, -1) and bad(fn, ok, 5, -1) and bad(fn, ok, 10, 0) and bad(fn, ok, 11, 0)
    assert bad(fn, ok, 12, 7) and bad(fn, ok, 12, 17)
    assert bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 1, buf.data_ptr() + 1) and bad(fn, ok, 0, f32.data_ptr() + 2)
    assert b'demfi_frame_to_u16_rect' in lib.demfi_last_error()
    assert L.ABI_VERSION == 8                                                                            # the ABI is additive
    torch.cuda.synchronize()
    assert (_np16(buf) == GUARD).all() and (_np16(frames) == GUARD).all() and bool((f32 == 0.25).all())


# ---- 3. the video path ---------------------------------------------------------------------------------------------------------
def _model(dtype):
    m = DeMFInet(HyperParams(), dtype=dtype)
    m.load_state_dict(synthetic_state_dict(0))
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model16():
    return _model(torch.float16)


@pytest.fixture(scope='module')
def model32():
    return _model(torch.float32)


def _clip(n, h, w, header, d, layout='420', matrix='bt601', full=False, seed=0, look=None):
    """A seeded clip of n frames of a moving pattern as a Y4M stream at depth d (16-bit samples above 8): (bytes, payloads)."""
    peak = (1 << d) - 1
    base = synthetic_window(h + 2 * n, w + 2 * n, seed)[0, :, 0]
    pays = []
    for i in range(n):
        f = base[:, i:i + h, 2 * i:2 * i + w].permute(1, 2, 0).numpy().astype(np.float64)
        bgr = ((f + 1) / 2 * peak).clip(0, peak).astype(np.uint16)
        if look is not None:
            bgr = look(i, bgr, peak)
        pays.append(y4m.bgr16_to_yuv_np(bgr, d, layout, matrix, full) if d > 8 else y4m.bgr_to_yuv_np(bgr.astype(np.uint8), layout, matrix, full))
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def _read(data):
    rd = y4m.Reader(io.BytesIO(data), **ANY)
    pays, buf = [], np.empty(rd.header.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    return rd.header, pays


def _repeat(data, times):
    """The clip with frame i shown times[i] times in a row."""
    at = data.index(b'FRAME\n')
    hdr, pays = _read(data)
    return data[:at] + b''.join(b'FRAME\n' + p.tobytes() for p, c in zip(pays, times) for _ in range(c))


def _expected(model, data, n_tst, r, matrix, p, full_length=False, cuts=None, kept=None):
    """numpy payload -> BGR16 (of the kept frames when ``kept``), ``crop_np``; every run of every window (``scene.window_runs``, or
    ``cadence.window_runs`` over the kept frames) once per tile in ONE ``run_windows_u16`` of the untiled runner of the tile's size;
    every output picked by the window's outputs, ``stitch_np``, numpy BGR16 -> payload.  Returns (bytes, cut windows, runs)."""
    hdr, pays = _read(data)
    d, lay, n, nt = hdr.depth, hdr.layout, len(pays), p.n_tiles
    site = (hdr.chroma,) if lay == '420' else ()
    frames = [y4m.yuv_to_bgr16_np(y4m.as_samples16(pays[i]), hdr.h, hdr.w, d, lay, matrix, hdr.full_range, *site)
              for i in (kept if kept is not None else range(n))]
    tiles = [[_dev16(t) for t in T.crop_np(f, p)] for f in frames]
    cuts = cuts or []
    runs, outs, n_cut = [], [], 0
    if kept is not None:
        is_cut = (lambda j: j in cuts) if cuts else None
        for k in K.windows(kept, n, full_length, r):
            wr, wo = K.window_runs(k, r, kept, n, is_cut, full_length)
            n_cut += K.is_cut_window(k, is_cut)
            outs += [(len(runs) + run, kind, j) for _, run, kind, j in wo]
            runs += wr
    else:
        is_cut = S.with_sentinels(lambda j: j in cuts, n) if full_length else (lambda j: j in cuts)
        k0, nw = R.first_window(n, full_length), R.n_windows(n, full_length)
        for k in range(k0, k0 + nw):
            wr, wo = S.window_runs(k, r, k == k0 + nw - 1, is_cut, full_length)
            n_cut += len(wr) - 1
            outs += [(len(runs) + run, kind, j) for _, run, kind, j in wo]
            runs += wr
    rn = ClipRunner(model, p.tile[0], p.tile[1], n_tst, 8, retime=r).runner
    st, s01 = rn.run_windows_u16([[tiles[x][j] for x in S.runner_order(tup)] for tup, _ in runs for j in range(nt)], d,
                                 ts=[ts for _, ts in runs for _ in range(nt)])
    torch.cuda.synchronize()
    st, s01 = _np16(st), _np16(s01)
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    for run, kind, j in outs:
        rows = slice(run * nt, (run + 1) * nt)
        f = T.stitch_np(s01[rows, 0] if kind == R.S0 else s01[rows, 1] if kind == R.S1 else st[rows, j], p, hdr.h, hdr.w)
        out += [b'FRAME\n', y4m.bgr16_to_yuv_np(f, d, lay, matrix, hdr.full_range).tobytes()]
    assert len(outs) == R.n_output_frames(n, r, full_length)
    return b''.join(out), n_cut, runs


def _run(model, data, n_tst, batch=2, matrix='bt601', **kw):
    kw = dict(dict(high_depth=True, tile=TILE, tile_margin=MARGIN, tile_high_depth=True), **kw)
    vr = VideoRunner(model, n_tst, batch=batch, matrix=matrix, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _same(got, exp):
    g, e = got.split(b'FRAME\n'), exp.split(b'FRAME\n')
    assert len(g) == len(e), (len(g), len(e))
    bad = [i for i, (a, b) in enumerate(zip(g, e)) if a != b]
    assert not bad, 'frames differ (0 = header): %s' % bad[:10]
    assert got == exp


PLAN = T.plan_tiles(H, W, TILE, MARGIN)


def test_the_plan_is_two_by_two():
    assert PLAN.grid == (2, 2) and PLAN.n_tiles == 4


def test_10_bit_x4_fp16_is_crop_run_stitch(model16):
    data, pays = _clip(6, H, W, b'YUV4MPEG2 W160 H96 F25:1 Ip A1:1 C420p10\n', 10, seed=3)
    assert max(int(q.max()) for q in pays) > 255 * 2                                        # the upper bits are in use
    exp, _, runs = _expected(model16, data, 2, Fraction(4), 'bt601', PLAN)
    vr, nw, nf, got = _run(model16, data, 2, mfi=4)
    assert (nw, nf, vr.last_depth) == (3, R.n_output_frames(6, 4), 10) and vr.last_plan == PLAN
    assert vr.last_instants[0] == sum(len(ts) for _, ts in runs) * PLAN.n_tiles            # every run once per tile
    _same(got, exp)
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge                       # nothing to crop into or stitch from
    assert edge.in_place and not hasattr(edge, 'tcomb') and not hasattr(edge.tiler, 'tin')
    vr2, _, _, again = _run(model16, data, 2, batch=4, mfi=4)                               # another batch split, the same bytes
    assert again == got


def test_16_bit_full_range_24_to_60_full_length_fp32_stream_and_ranks(model32, tmp_path):
    r = Fraction(5, 2)
    data, _ = _clip(6, H, W, b'YUV4MPEG2 W160 H96 F24:1 Ip C420p16 XCOLORRANGE=FULL\n', 16, matrix='bt709', full=True, seed=4)
    exp, _, _ = _expected(model32, data, 1, r, 'bt709', PLAN, full_length=True)
    kw = dict(matrix='bt709', fps=Fraction(60), full_length=True)
    vr, nw, nf, got = _run(model32, data, 1, **kw)
    assert nf == R.n_output_frames(6, r, True) and vr.last_depth == 16 and vr.last_plan == PLAN
    _same(got, exp)
    # two ranks of one file, run one after the other in this process (rank 0 sizes the file first)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model32, 1, batch=2, high_depth=True, tile=TILE, tile_margin=MARGIN, tile_high_depth=True, **kw)
        nw_r, nf_r = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += nw_r
        tot[1] += nf_r
    assert tot == [nw, nf]
    _same(dst.read_bytes(), exp)


def test_10_bit_422_keeps_its_layout(model16):
    data, _ = _clip(5, H, W, b'YUV4MPEG2 W160 H96 F24:1 Ip C422p10\n', 10, layout='422', seed=5)
    exp, _, _ = _expected(model16, data, 1, Fraction(2), 'bt601', PLAN)
    vr, nw, nf, got = _run(model16, data, 1, mfi=2, layouts=True)
    assert (nw, nf) == (2, 5) and (vr.last_depth, vr.last_layout) == (10, '422') and b' C422p10' in got[:80]
    _same(got, exp)


def test_scene_cut_at_10_bits(model16):
    d, cut = 10, 4

    def look(i, bgr, peak):                                                 # a hard cut before frame 4: another scene's colours
        return bgr if i < cut else ((peak - bgr) // 3).astype(np.uint16)
    data, pays = _clip(8, H, W, b'YUV4MPEG2 W160 H96 F24:1 Ip C420p10\n', d, seed=1, look=look)
    sads = [S.sad_np(pays[j], pays[j - 1]) for j in range(1, len(pays))]
    cuts = S.cuts_of(sads, pays[0].size, S.DEFAULT_THRESHOLD, peak=(1 << d) - 1)              # the numpy detector, on full payloads
    assert cuts == [cut]
    exp, n_cut, _ = _expected(model16, data, 1, Fraction(2), 'bt601', PLAN, cuts=cuts)
    vr, nw, nf, got = _run(model16, data, 1, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert (nw, nf) == (5, R.n_output_frames(8, 2)) and vr.last_cuts == cuts and vr.last_cut_windows == n_cut >= 1
    _same(got, exp)
    plain = _run(model16, data, 1, mfi=2)[3]
    assert len(plain) == len(got) and plain != got


def test_dedup_at_10_bits(model16):
    base, _ = _clip(4, H, W, b'YUV4MPEG2 W160 H96 F24:1 Ip C420p10\n', 10, seed=2)
    data = _repeat(base, [1, 2, 1, 2])
    hdr, pays = _read(data)
    kept = K.kept_of(pays, hdr.h, hdr.w, hdr.depth)
    assert kept == [0, 1, 3, 4]
    exp, _, _ = _expected(model16, data, 1, Fraction(2), 'bt601', PLAN, full_length=True, kept=kept)
    vr, nw, nf, got = _run(model16, data, 1, mfi=2, full_length=True, dedup=True)
    assert (nw, nf) == (3, 12) and vr.last_dups == [2, 5] and vr.last_depth == 10
    _same(got, exp)


def test_an_8_bit_stream_takes_the_8_bit_tiled_path(model16):
    data, _ = _clip(5, H, W, b'YUV4MPEG2 W160 H96 F24:1 Ip C420jpeg\n', 8, seed=6)
    ref = _run(model16, data, 1, mfi=2, high_depth=False, tile_high_depth=False)
    for kw in ({'high_depth': False}, {}):                                  # the switch alone, and with --high-depth
        vr, nw, nf, got = _run(model16, data, 1, mfi=2, **kw)
        assert (nw, nf, vr.last_depth) == (ref[1], ref[2], 8) and vr.last_plan == PLAN
        assert got == ref[3]


def test_a_one_tile_plan_is_the_untiled_high_depth_run(model16):
    data, _ = _clip(5, 48, 80, b'YUV4MPEG2 W80 H48 F24:1 Ip C420p10\n', 10, seed=7)
    ref = _run(model16, data, 1, mfi=2, tile=None, tile_high_depth=False)
    vr, nw, nf, got = _run(model16, data, 1, mfi=2, tile='auto')
    assert vr.last_plan is None and (nw, nf) == (ref[1], ref[2]) and got == ref[3]
    assert _run(model16, data, 1, mfi=2, tile=None)[3] == ref[3]             # the switch without --tile changes nothing


def test_without_the_switch_the_refusal_is_unchanged(model16, tmp_path):
    data, _ = _clip(5, 48, 80, b'YUV4MPEG2 W80 H48 F24:1 Ip C420p10\n', 10)
    vr = VideoRunner(model16, 1, mfi=2, batch=2, high_depth=True, tile='auto')
    assert vr.tile_high_depth is False
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError) as e:
        vr.run_stream(io.BytesIO(data), io.BytesIO())
    assert 'tile' in str(e.value) and '10-bit' in str(e.value) and '--tile-high-depth' in str(e.value)
    src = tmp_path / 'in.y4m'
    src.write_bytes(data)
    with pytest.raises(ValueError):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert not vr._runners and torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)             # nothing was allocated for it
