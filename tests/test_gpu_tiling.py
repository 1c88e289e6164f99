"""GPU tests of tiled frames: demfi_u8_tile_crop / demfi_u8_tile_stitch against tiling.crop_np / stitch_np byte for byte, and the
tiled folder and Y4M pipelines against the composition they stand for: crop every input frame, run each tile's clip untiled at
the tile's size, stitch the outputs.  No tolerance anywhere: byte copies, and the same kernels on the same inputs."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict, synthetic_window   # noqa: E402
from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.harness import module_window_ts_u8                                    # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
H, W, TILE, MARGIN = 96, 160, (64, 96), 16
HDR24 = b'YUV4MPEG2 W160 H96 F24:1 Ip C420jpeg\n'

# (h, w, tile, margin): the last column of tiles starts at x0 = w - tw; over the set 3 * x0 takes every residue modulo 16
KERNEL_PLANS = [(96, 160, (64, 96), 16), (97, 131, (64, 96), 0), (70, 1283, (70, 320), 32), (131, 97, (96, 64), 8), (40, 100, (32, 64), 4),
                (50, 97, (32, 96), 0)] + [(33, 64 + r, (32, 64), 0) for r in range(1, 17)]


def test_the_kernel_plans_cover_every_alignment():
    res = {3 * t.src.x0 % 16 for h, w, tile, m in KERNEL_PLANS for t in T.plan_tiles(h, w, tile, m).tiles}
    assert res == set(range(16))


def _dev_plan(p):
    rects = np.ascontiguousarray(p.rects(), dtype=np.int32)
    return rects, torch.from_numpy(rects).to(DEV)


@pytest.mark.parametrize('h,w,tile,margin', KERNEL_PLANS)
def test_crop_and_stitch_bit_exact_against_numpy(h, w, tile, margin):
    lib = L.load()
    p = T.plan_tiles(h, w, tile, margin)
    (th, tw), nt, n = p.tile, p.n_tiles, 3
    rects, rects_dev = _dev_plan(p)
    rng = np.random.default_rng(h * 1000 + w)
    pad = 7                                                   # frames 7 bytes apart: every frame at another alignment
    stride = h * w * 3 + pad
    src = rng.integers(0, 256, n * stride, dtype=np.uint8)
    frames = [src[i * stride:i * stride + h * w * 3].reshape(h, w, 3) for i in range(n)]
    d_src = torch.from_numpy(src).to(DEV)
    d_tiles = torch.full((n * nt * th * tw * 3 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_u8_tile_crop(d_src.data_ptr(), stride, d_tiles.data_ptr(), n, h, w, th, tw, nt, rects.ctypes.data, rects_dev.data_ptr(),
                                   None), 'crop')
    got = d_tiles.cpu().numpy()
    exp = np.stack([T.crop_np(f, p) for f in frames])
    assert (got[:exp.size].reshape(exp.shape) == exp).all()
    assert (got[exp.size:] == 0xA5).all()
    # stitch: tiles taken from a pool in any order, with repeats; frames written at scattered offsets between canaries
    pool = rng.integers(0, 256, (5, th, tw, 3), dtype=np.uint8)
    pick = rng.integers(0, 5, (n, nt))
    pick[1] = pick[0]                                         # two frames of the same tiles
    fsz, gap = h * w * 3, 3 * w * 3 + 5                       # canary rows (and 5 bytes: odd alignments) around every frame
    dst_offs = np.array([gap + i * (fsz + gap) for i in (2, 0, 1)], np.int64)
    total = gap + n * (fsz + gap)
    offs = torch.from_numpy(np.concatenate([(pick * (th * tw * 3)).astype(np.int64).reshape(-1), dst_offs])).to(DEV)
    d_pool = torch.from_numpy(pool).to(DEV)
    d_out = torch.full((total,), 0x5A, dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_u8_tile_stitch(d_pool.data_ptr(), offs.data_ptr(), d_out.data_ptr(), offs[n * nt:].data_ptr(), n, h, w, th, tw, nt,
                                     rects.ctypes.data, rects_dev.data_ptr(), None), 'stitch')
    got = d_out.cpu().numpy()
    exp = np.full(total, 0x5A, np.uint8)
    for i in range(n):
        exp[dst_offs[i]:dst_offs[i] + fsz] = T.stitch_np(pool[pick[i]], p, h, w).reshape(-1)
    assert (got == exp).all()
    # the round trip on the GPU: stitch(crop(f)) == f
    offs = torch.from_numpy(np.concatenate([np.arange(n * nt, dtype=np.int64) * (th * tw * 3), np.arange(n, dtype=np.int64) * fsz])).to(DEV)
    d_back = torch.zeros(n * fsz, dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_u8_tile_stitch(d_tiles.data_ptr(), offs.data_ptr(), d_back.data_ptr(), offs[n * nt:].data_ptr(), n, h, w, th, tw, nt,
                                     rects.ctypes.data, rects_dev.data_ptr(), None), 'stitch')
    assert (d_back.cpu().numpy().reshape(n, h, w, 3) == np.stack(frames)).all()


def test_bad_arguments_are_rejected_without_a_launch():
    lib = L.load()
    p = T.plan_tiles(H, W, TILE, MARGIN)
    rects, rects_dev = _dev_plan(p)
    src = torch.zeros(H * W * 3, dtype=torch.uint8, device=DEV)
    tiles = torch.full((p.n_tiles * 64 * 96 * 3,), 7, dtype=torch.uint8, device=DEV)
    out = torch.full((H * W * 3,), 9, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(p.n_tiles + 1, dtype=torch.int64, device=DEV)
    good = dict(n=1, h=H, w=W, th=64, tw=96, nt=p.n_tiles, rects=rects, a=src.data_ptr(), b=tiles.data_ptr(), dev=rects_dev.data_ptr(),
                stride=H * W * 3)

    def crop(**kw):
        a = dict(good, **kw)
        return lib.demfi_u8_tile_crop(a['a'], a['stride'], a['b'], a['n'], a['h'], a['w'], a['th'], a['tw'], a['nt'],
                                      a['rects'].ctypes.data if a['rects'] is not None else None, a['dev'], None)

    def stitch(**kw):
        a = dict(good, a=tiles.data_ptr(), b=out.data_ptr(), offs=offs.data_ptr())
        a.update(kw)
        return lib.demfi_u8_tile_stitch(a['a'], a['offs'], a['b'], a['offs'] and offs[p.n_tiles:].data_ptr(), a['n'], a['h'], a['w'],
                                        a['th'], a['tw'], a['nt'], a['rects'].ctypes.data if a['rects'] is not None else None, a['dev'], None)

    def moved(j, col, v):
        r = rects.copy()
        r[j, col] = v
        return r
    bad = [dict(a=None), dict(b=None), dict(rects=None), dict(dev=None), dict(n=-1), dict(h=1), dict(w=16385), dict(th=1), dict(tw=W + 1),
           dict(th=H + 32), dict(nt=0), dict(rects=moved(3, 0, H - 63)), dict(rects=moved(1, 1, W - 95)), dict(rects=moved(0, 0, -1)),
           dict(rects=moved(0, 4, 65)), dict(rects=moved(3, 2, 31)), dict(rects=moved(2, 5, 97)), dict(rects=moved(0, 4, 0))]
    for fn in (crop, stitch):
        for kw in bad:
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert fn.__name__.encode() in lib.demfi_last_error()
    assert crop(n=2, stride=H * W * 3 - 1) == -1 and b'src_stride' in lib.demfi_last_error()
    assert stitch(offs=None) == -1
    assert crop(n=0) == 0 and stitch(n=0) == 0
    torch.cuda.synchronize()
    assert (tiles == 7).all() and (out == 9).all()             # nothing was launched


# ---- the pipelines ---------------------------------------------------------------------------------------------------------
def _model(dtype):
    m = DeMFInet(HyperParams(), dtype=torch.float16 if dtype == 'fp16' else torch.float32)
    m.load_state_dict(synthetic_state_dict(0))
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model16():
    return _model('fp16')


@pytest.fixture(scope='module')
def model32():
    return _model('fp32')


def _bgr_clip(n, seed=3, h=H, w=W, look=lambda x: x):
    base = synthetic_window(h + 2 * n, w + 2 * n, seed)[0, :, 0]
    return [look(np.ascontiguousarray(((base[:, i:i + h, 2 * i:2 * i + w].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)))
            for i in range(n)]


def _run_frames(cr, frames):
    got = {}

    def sink(k, st, s01):
        got[k] = (st.numpy().copy(), s01.numpy().copy())
    n = cr.run_frames(frames, sink)
    assert sorted(got) == list(range(n))
    return [got[k] for k in range(n)]


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
def test_folder_path_is_crop_run_stitch(dtype, model16, model32):
    model = model16 if dtype == 'fp16' else model32
    frames = _bgr_clip(6)
    p = T.plan_tiles(H, W, TILE, MARGIN)
    assert p.n_tiles == 4
    cr = ClipRunner(model, H, W, 2, 2, batch=2, tile=TILE, tile_margin=MARGIN)
    assert cr.plan == p and cr.n_tiles == 4 and (cr.runner.h, cr.runner.w) == TILE
    got = _run_frames(cr, frames)
    plain = ClipRunner(model, TILE[0], TILE[1], 2, 2, batch=2)
    tiles = [T.crop_np(f, p) for f in frames]
    per_tile = [_run_frames(plain, [t[j] for t in tiles]) for j in range(p.n_tiles)]
    assert len(got) == 3
    for k in range(3):
        for part in range(2):                                  # St [M-1], S0S1 [2]
            exp = np.stack([T.stitch_np(np.stack([per_tile[j][k][part][i] for j in range(p.n_tiles)]), p, H, W)
                            for i in range(got[k][part].shape[0])])
            assert (got[k][part] == exp).all(), (k, part)
    again = _run_frames(cr, frames)                            # the buffers of a runner are reused: same bytes again
    assert all((a[0] == b[0]).all() and (a[1] == b[1]).all() for a, b in zip(got, again))


def test_one_tile_plan_and_no_tile_are_the_untiled_run(model16):
    frames = _bgr_clip(5, h=48, w=80)
    base = _run_frames(ClipRunner(model16, 48, 80, 2, 2, batch=2), frames)
    for kw in ({'tile': None}, {'tile': (64, 96)}, {'tile': 'auto'}):
        cr = ClipRunner(model16, 48, 80, 2, 2, batch=2, **kw)
        assert cr.plan is None and cr.n_tiles == 1 and cr.runner.tiles is None
        got = _run_frames(cr, frames)
        assert all((a[0] == b[0]).all() and (a[1] == b[1]).all() for a, b in zip(got, base))
    data = _y4m([y4m.bgr_to_yuv420_np(f, 'bt601', False) for f in frames], b'YUV4MPEG2 W80 H48 F24:1 Ip C420jpeg\n')
    ref = _stream(model16, data, 2, mfi=2)[3]
    for kw in ({'tile': None}, {'tile': (64, 96)}, {'tile': 'auto'}):
        vr, nw, nf, got = _stream(model16, data, 2, mfi=2, **kw)
        assert vr.last_plan is None and got == ref


def _y4m(payloads, header=HDR24):
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in payloads)


def _stream(model, data, n_tst, batch=2, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _same(got, exp):
    g, e = got.split(b'FRAME\n'), exp.split(b'FRAME\n')
    assert len(g) == len(e), (len(g), len(e))
    bad = [i for i, (a, b) in enumerate(zip(g, e)) if a != b]
    assert not bad, 'frames differ (0 = header): %s' % bad[:10]


def _decode(data):
    rd = y4m.Reader(io.BytesIO(data))
    hdr = rd.header
    buf, pays = np.empty(hdr.payload, np.uint8), []
    while rd.read_into(buf):
        pays.append(buf.copy())
    matrix = y4m.auto_matrix(hdr.h)
    return hdr, matrix, [y4m.yuv420_to_bgr_np(q, hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma) for q in pays]


def _expected(model, data, n_tst, r, p, cuts=(), full=False):
    """numpy YUV -> BGR, crop; per tile the untiled expectation of tests/test_gpu_retime.py, test_gpu_scene.py and
    test_gpu_full_length.py at the tile's size (one module forward per instant of every run of ``scene.window_runs``, each
    output picked by the window's plan); stitch, numpy BGR -> YUV.  Returns (stream, windows)."""
    hdr, matrix, frames = _decode(data)
    tiles = [torch.from_numpy(T.crop_np(f, p)) for f in frames]
    n = len(frames)
    is_cut = S.with_sentinels(lambda j: j in cuts, n) if full else (lambda j: j in cuts)
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    k0, nw = R.first_window(n, full), R.n_windows(n, full)
    for k in range(k0, k0 + nw):
        runs, outs = S.window_runs(k, r, k == k0 + nw - 1, is_cut, full)
        res = [[[a.cpu().numpy() for a in module_window_ts_u8(model, [tiles[x][j] for x in S.runner_order(tup)], n_tst, ts)]
                for j in range(p.n_tiles)] for tup, ts in runs]
        for _, run, kind, i in outs:
            f = np.stack([s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[i] for st, s01 in res[run]])
            out += [b'FRAME\n', y4m.bgr_to_yuv420_np(T.stitch_np(f, p, hdr.h, hdr.w), matrix, hdr.full_range).tobytes()]
    return b''.join(out), nw


def _payloads(frames):
    return [y4m.bgr_to_yuv420_np(f, 'bt601', False) for f in frames]


def test_y4m_mfi_is_crop_run_stitch(model16):
    """--mfi: the per-tile side is the plain untiled ClipRunner at the tile's size."""
    data = _y4m(_payloads(_bgr_clip(6, seed=4)))
    p = T.plan_tiles(H, W, TILE, MARGIN)
    vr, nw, nf, got = _stream(model16, data, 2, mfi=2, tile=TILE, tile_margin=MARGIN)
    assert (nw, nf) == (3, 3 * 2 + 1) and vr.last_plan == p
    assert vr.last_instants[0] == 3 * 1 * p.n_tiles                # every run once per tile
    hdr, matrix, frames = _decode(data)
    tiles = [T.crop_np(f, p) for f in frames]
    plain = ClipRunner(model16, TILE[0], TILE[1], 2, 2, batch=2)
    per_tile = [_run_frames(plain, [t[j] for t in tiles]) for j in range(p.n_tiles)]

    def full(k, part, i):
        return y4m.bgr_to_yuv420_np(T.stitch_np(np.stack([per_tile[j][k][part][i] for j in range(p.n_tiles)]), p, H, W), matrix, hdr.full_range)
    exp = [R.output_header(hdr, hdr.fps * 2).encode()]
    for k in range(3):
        exp += [b'FRAME\n', full(k, 1, 0).tobytes(), b'FRAME\n', full(k, 0, 0).tobytes()]
    exp += [b'FRAME\n', full(2, 1, 1).tobytes()]
    _same(got, b''.join(exp))
    exp2, nw2 = _expected(model16, data, 2, Fraction(2), p)       # and the module path agrees with it
    assert nw2 == 3
    _same(got, exp2)


def test_y4m_non_integer_ratio_is_crop_run_stitch(model16):
    data = _y4m(_payloads(_bgr_clip(7, seed=5)))
    p = T.plan_tiles(H, W, TILE, MARGIN)
    exp, nw_exp = _expected(model16, data, 2, Fraction(5, 2), p)
    vr, nw, nf, got = _stream(model16, data, 2, fps=Fraction(60), tile=TILE, tile_margin=MARGIN)
    assert nw == nw_exp == 4 and nf == R.n_output_frames(7, Fraction(5, 2), False)
    _same(got, exp)


def _cut_clip():
    """Frames 0-3 scene A, 4-7 scene B: one cut, before frame 4."""
    fr = _payloads(_bgr_clip(4, seed=0) + _bgr_clip(4, seed=1, look=lambda x: (255 - x) // 3))
    sc = S.scores([S.sad_np(fr[j], fr[j - 1]) for j in range(1, 8)], fr[0].size)
    assert [j for j, s in enumerate(sc, 1) if s >= S.DEFAULT_THRESHOLD] == [4]
    return _y4m(fr)


def test_y4m_scene_cut_is_crop_run_stitch(model16):
    data = _cut_clip()
    p = T.plan_tiles(H, W, TILE, MARGIN)
    exp, nw_exp = _expected(model16, data, 2, Fraction(4), p, cuts=(4,))
    vr, nw, nf, got = _stream(model16, data, 2, mfi=4, scene_cut=S.DEFAULT_THRESHOLD, tile=TILE, tile_margin=MARGIN)
    assert nw == nw_exp == 5 and nf == 5 * 4 + 1
    assert vr.last_cuts == [4] and vr.last_cut_windows >= 1       # the SADs are those of the full payloads
    _same(got, exp)
    plain = _stream(model16, data, 2, mfi=4, tile=TILE, tile_margin=MARGIN)[3]
    assert len(plain) == len(got) and plain != got


def test_y4m_full_length_is_crop_run_stitch(model16):
    data = _y4m(_payloads(_bgr_clip(5, seed=6)))
    p = T.plan_tiles(H, W, TILE, MARGIN)
    exp, nw_exp = _expected(model16, data, 2, Fraction(5, 2), p, full=True)
    vr, nw, nf, got = _stream(model16, data, 2, fps=Fraction(60), full_length=True, tile=TILE, tile_margin=MARGIN)
    assert nw == nw_exp and nf == R.n_output_frames(5, Fraction(5, 2), True)
    _same(got, exp)


def test_an_oversized_untiled_frame_names_the_way_out(model16, monkeypatch):
    """Whatever the runner raises for a frame above the largest size run in one forward reaches the user with --tile auto in it
    (here: the workspace check, made to fail without allocating anything)."""
    from demfi_amd import runner as RN

    def refuse(*a, **kw):
        raise RuntimeError('WindowRunner: workspace exceeds the GPU memory')
    monkeypatch.setattr(RN, 'choose_config', refuse)
    with pytest.raises(RuntimeError, match='--tile auto'):
        ClipRunner(model16, 2176, 3840, 2, 2)
    with pytest.raises(RuntimeError) as e:
        ClipRunner(model16, 96, 160, 2, 2)
    assert '--tile' not in str(e.value)
