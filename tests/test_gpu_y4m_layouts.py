"""4:2:2, 4:4:4 and mono Y4M (``--any-layout``) on a real MI355X: the kernels of csrc/yuv_family.hip bit-exact against their numpy
definitions (byte samples and 16-bit samples, padded strides, shuffled gathers, argument errors), and ``VideoRunner(layouts=True)``
byte-identical to the expectation composed from the numpy definitions around the BGR window path: the module path of
tests/test_gpu_scene.py / test_gpu_tiling.py for 8-bit streams, ``WindowRunner.run_windows_u16`` as in tests/test_gpu_y4m_depth.py
for deep ones."""
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
MCODE = {'bt601': L.BT601, 'bt709': L.BT709}
NEW = ('422', '444', 'mono')
ERR_ARG = -1
ANY = {'depths': y4m.DEPTHS, 'layouts': y4m.LAYOUTS}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _types(d):
    """(numpy sample type, guard value) of a payload at depth d: bytes at 8 bits, 16-bit samples above."""
    return (np.uint8, 0xA5) if d == 8 else (np.uint16, 0xA5C3)


def _dev(a, d):
    """numpy samples -> GPU tensor holding the same bits (uint8, or int16 storage of uint16)."""
    dt, _ = _types(d)
    a = np.ascontiguousarray(a, dt)
    return torch.from_numpy(a if d == 8 else a.view(np.int16)).to(DEV)


def _host(t, d):
    a = t.cpu().numpy()
    return a if d == 8 else a.view(np.uint16)


def _to_bgr_gpu(pays, h, w, d, layout, matrix, full, src_pad=0, dst_pad=0):
    """pays [n, P] -> [n, h, w, 3] through demfi_yuvl_to_bgr (d = 8: byte strides) / demfi_yuvl16_to_bgr16 (sample strides) at
    padded strides; the padding stays untouched and the source is unmodified."""
    dt, guard = _types(d)
    n, P = pays.shape
    F = h * w * 3
    src = np.zeros((n, P + src_pad), dt)
    src[:, :P] = pays
    src = _dev(src, d)
    before = src.clone()
    dst = _dev(np.full((n, F + dst_pad), guard, dt), d)
    lib = L.load()
    if d == 8:
        st = lib.demfi_yuvl_to_bgr(src.data_ptr(), P + src_pad, dst.data_ptr(), F + dst_pad, n, h, w, L.YUV_LAYOUT[layout], MCODE[matrix],
                                   int(full), _stream())
    else:
        st = lib.demfi_yuvl16_to_bgr16(src.data_ptr(), P + src_pad, dst.data_ptr(), F + dst_pad, n, h, w, d, L.YUV_LAYOUT[layout],
                                       MCODE[matrix], int(full), _stream())
    L.check(st, 'yuvl_to_bgr')
    out = _host(dst, d)
    assert (out[:, F:] == guard).all(), 'write outside the frames'
    assert torch.equal(src, before)
    return out[:, :F].reshape(n, h, w, 3)


def _gather_gpu(frames, order, d, layout, matrix, full, src_pad=0, dst_pad=0, lead=0):
    """frames [nb, h, w, 3] kept at a padded stride behind ``lead`` samples; frame order[f] -> payload f."""
    dt, guard = _types(d)
    nb, h, w = frames.shape[:3]
    F, P = h * w * 3, y4m.payload_size(h, w, layout)
    fs = F + src_pad
    base = np.zeros(lead + nb * fs + 64, dt)
    for i in range(nb):
        base[lead + i * fs:lead + i * fs + F] = frames[i].reshape(-1)
    base = _dev(base, d)
    before = base.clone()
    offs = torch.tensor([lead + i * fs for i in order], dtype=torch.int64, device=DEV)
    ds = P + dst_pad
    dst = _dev(np.full((len(order), ds), guard, dt), d)
    lib = L.load()
    if d == 8:
        st = lib.demfi_bgr_to_yuvl_gather(base.data_ptr(), offs.data_ptr(), dst.data_ptr(), ds, len(order), h, w, L.YUV_LAYOUT[layout],
                                          MCODE[matrix], int(full), _stream())
    else:
        st = lib.demfi_bgr16_to_yuvl16_gather(base.data_ptr(), offs.data_ptr(), dst.data_ptr(), ds, len(order), h, w, d, L.YUV_LAYOUT[layout],
                                              MCODE[matrix], int(full), _stream())
    L.check(st, 'bgr_to_yuvl_gather')
    out = _host(dst, d)
    assert (out[:, P:] == guard).all(), 'write outside the payloads'
    assert torch.equal(base, before)
    return out[:, :P]


def _to_bgr_np(pay, h, w, d, layout, matrix, full):
    return y4m.yuv_to_bgr_np(pay, h, w, layout, matrix, full) if d == 8 else y4m.yuv_to_bgr16_np(pay, h, w, d, layout, matrix, full)


def _to_yuv_np(bgr, d, layout, matrix, full):
    return y4m.bgr_to_yuv_np(bgr, layout, matrix, full) if d == 8 else y4m.bgr16_to_yuv_np(bgr, d, layout, matrix, full)


SIZES = [(2, 2), (3, 5), (5, 3), (37, 53), (70, 98), (64, 128), (720, 1280)]          # those of tests/test_gpu_y4m.py
DEPTHS = [8, 10, 12, 16]


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('d', DEPTHS)
@pytest.mark.parametrize('matrix,full', [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)])
def test_kernels_bit_exact_against_numpy(h, w, d, matrix, full):
    dt, _ = _types(d)
    g = np.random.RandomState(h * 7 + w + d)
    peak = (1 << d) - 1
    for layout in NEW:
        pays = g.randint(0, peak + 1, (2, y4m.payload_size(h, w, layout))).astype(dt)
        bgr = g.randint(0, peak + 1, (2, h, w, 3)).astype(dt)
        if d > 8:                                      # values above the peak: taken as they are, like numpy
            pays[1, ::3] = g.randint(0, 65536, pays[1, ::3].size)
            bgr[1, ::2, ::3] = g.randint(0, 65536, bgr[1, ::2, ::3].shape)
        got = _to_bgr_gpu(pays, h, w, d, layout, matrix, full)
        for i in range(2):
            assert np.array_equal(got[i], _to_bgr_np(pays[i], h, w, d, layout, matrix, full)), (layout, i)
        got = _gather_gpu(bgr, [1, 0], d, layout, matrix, full)
        for f, i in enumerate([1, 0]):
            assert np.array_equal(got[f], _to_yuv_np(bgr[i], d, layout, matrix, full)), (layout, i)


@pytest.mark.parametrize('layout', NEW)
def test_16_bit_kernels_at_depth_8_equal_the_byte_kernels(layout):
    h, w = 37, 53
    g = np.random.RandomState(5)
    pays = g.randint(0, 256, (3, y4m.payload_size(h, w, layout))).astype(np.uint8)
    a = _to_bgr_gpu(pays, h, w, 8, layout, 'bt709', False)
    lib, F, P = L.load(), h * w * 3, pays.shape[1]
    src, dst = _dev(pays.astype(np.uint16), 16), _dev(np.zeros((3, F), np.uint16), 16)
    L.check(lib.demfi_yuvl16_to_bgr16(src.data_ptr(), P, dst.data_ptr(), F, 3, h, w, 8, L.YUV_LAYOUT[layout], L.BT709, 0, _stream()))
    assert np.array_equal(_host(dst, 16).reshape(3, h, w, 3), a.astype(np.uint16))
    offs = torch.tensor([2 * F, 0, F], dtype=torch.int64, device=DEV)
    out = _dev(np.zeros((3, P), np.uint16), 16)
    L.check(lib.demfi_bgr16_to_yuvl16_gather(dst.data_ptr(), offs.data_ptr(), out.data_ptr(), P, 3, h, w, 8, L.YUV_LAYOUT[layout], L.BT601, 1,
                                             _stream()))
    assert np.array_equal(_host(out, 16), _gather_gpu(a, [2, 0, 1], 8, layout, 'bt601', True).astype(np.uint16))


@pytest.mark.parametrize('h,w', [(37, 53), (64, 128), (70, 98)])
@pytest.mark.parametrize('pad', [0, 8, 13])
@pytest.mark.parametrize('d', [8, 10, 16])
def test_strided_batches_and_gather_order(h, w, pad, d):
    """Several frames per launch at strides larger than a frame (0, 8, 13 units: aligned and only sample-aligned), and gather
    offsets in shuffled order with repeats behind an odd number of leading samples."""
    dt, _ = _types(d)
    g = np.random.RandomState(pad + d)
    peak = (1 << d) - 1
    order = [4, 0, 0, 5, 2, 2, 1, 3, 4]
    for layout in NEW:
        pays = g.randint(0, peak + 1, (5, y4m.payload_size(h, w, layout))).astype(dt)
        got = _to_bgr_gpu(pays, h, w, d, layout, 'bt709', False, src_pad=pad, dst_pad=2 * pad + (1 if pad == 13 else 0))
        for i in range(5):
            assert np.array_equal(got[i], _to_bgr_np(pays[i], h, w, d, layout, 'bt709', False)), (layout, i)
        bgr = g.randint(0, peak + 1, (6, h, w, 3)).astype(dt)
        got = _gather_gpu(bgr, order, d, layout, 'bt601', True, src_pad=pad, dst_pad=2 * pad + 3, lead=pad)
        for f, i in enumerate(order):
            assert np.array_equal(got[f], _to_yuv_np(bgr[i], d, layout, 'bt601', True)), (layout, f, i)


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), _stream()
    buf8 = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    buf16 = _dev(np.full(256, 0xA5C3, np.uint16), 16)
    offs = torch.zeros(4, dtype=torch.int64, device=DEV)

    def bad(fn, ok, i, v):
        a = list(ok)
        a[i] = v
        return fn(*a) == ERR_ARG
    for layout in NEW:
        lc, p, fsz = L.YUV_LAYOUT[layout], y4m.payload_size(2, 2, layout), 12
        ok = (buf8.data_ptr(), p, buf8.data_ptr() + 128, fsz, 2, 2, 2, lc, 0, 0, st)               # byte samples, to BGR
        fn = lib.demfi_yuvl_to_bgr
        assert bad(fn, ok, 0, None) and bad(fn, ok, 2, None) and bad(fn, ok, 1, p - 1) and bad(fn, ok, 3, fsz - 1) and bad(fn, ok, 4, -1)
        assert bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385) and bad(fn, ok, 7, 0) and bad(fn, ok, 7, 4) and bad(fn, ok, 8, 2) and bad(fn, ok, 9, 2)
        ok = (buf8.data_ptr(), offs.data_ptr(), buf8.data_ptr() + 128, p, 2, 2, 2, lc, 0, 0, st)   # byte samples, gather
        fn = lib.demfi_bgr_to_yuvl_gather
        assert bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 2, None) and bad(fn, ok, 3, p - 1) and bad(fn, ok, 4, -1)
        assert bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385) and bad(fn, ok, 7, 0) and bad(fn, ok, 7, -1) and bad(fn, ok, 8, 2) and bad(fn, ok, 9, 2)
        ok = (buf16.data_ptr(), p, buf16.data_ptr() + 256, fsz, 2, 2, 2, 10, lc, 0, 0, st)         # 16-bit samples, to BGR
        fn = lib.demfi_yuvl16_to_bgr16
        assert bad(fn, ok, 7, 7) and bad(fn, ok, 7, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 2, None)
        assert bad(fn, ok, 1, p - 1) and bad(fn, ok, 3, fsz - 1) and bad(fn, ok, 4, -1) and bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385)
        assert bad(fn, ok, 8, 0) and bad(fn, ok, 8, 4) and bad(fn, ok, 9, 2) and bad(fn, ok, 10, 2)
        assert bad(fn, ok, 0, buf16.data_ptr() + 1) and bad(fn, ok, 2, buf16.data_ptr() + 257)      # odd addresses
        ok = (buf16.data_ptr(), offs.data_ptr(), buf16.data_ptr() + 256, p, 2, 2, 2, 10, lc, 0, 0, st)   # 16-bit samples, gather
        fn = lib.demfi_bgr16_to_yuvl16_gather
        assert bad(fn, ok, 7, 7) and bad(fn, ok, 7, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 2, None)
        assert bad(fn, ok, 3, p - 1) and bad(fn, ok, 4, -1) and bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385)
        assert bad(fn, ok, 8, 0) and bad(fn, ok, 8, 4) and bad(fn, ok, 9, 2) and bad(fn, ok, 10, 2) and bad(fn, ok, 0, buf16.data_ptr() + 1)
    torch.cuda.synchronize()
    assert bool((buf8 == 0xA5).all()) and (_host(buf16, 16) == 0xA5C3).all()
    assert L.ABI_VERSION == 8                                                                      # the ABI is additive


# ---- 2. end to end -------------------------------------------------------------------------------------------------------------
def _model(dtype):
    m = DeMFInet(HyperParams(), dtype=dtype)
    m.load_state_dict(synthetic_state_dict(0))
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model16():
    return _model(torch.float16)


def _tag(layout, d):
    if layout == '420':
        return '420jpeg' if d == 8 else '420p%d' % d
    return layout if d == 8 else ('mono%d' if layout == 'mono' else layout + 'p%d') % d


def _clip(n, h, w, layout, d, matrix='bt601', full=False, fps=b'24:1', seed=0, look=None):
    """A seeded clip of n frames of a moving pattern as a Y4M stream in ``layout`` at depth d: (bytes, payloads, BGR frames)."""
    peak = (1 << d) - 1
    header = b'YUV4MPEG2 W%d H%d F%s Ip C%s%s\n' % (w, h, fps, _tag(layout, d).encode(), b' XCOLORRANGE=FULL' if full else b'')
    base = synthetic_window(h + 2 * n, w + 2 * n, seed)[0, :, 0]
    pays, frames = [], []
    for i in range(n):
        f = base[:, i:i + h, 2 * i:2 * i + w].permute(1, 2, 0).numpy().astype(np.float64)
        bgr = ((f + 1) / 2 * peak).clip(0, peak).astype(_types(d)[0])
        if look is not None:
            bgr = look(i, bgr, peak)
        frames.append(bgr)
        pays.append(_to_yuv_np(bgr, d, layout, matrix, full))
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays, frames


def _read(data):
    rd = y4m.Reader(io.BytesIO(data), **ANY)
    buf, pays = np.empty(rd.header.payload, np.uint8), []
    while rd.read_into(buf):
        pays.append(buf.copy())
    return rd.header, pays


def _expected(model, data, n_tst, r, matrix, full_length=False, cuts=None, plan=None):
    """numpy payload -> BGR in the stream's layout and depth; every run of every window (``scene.window_runs``; a window that touches
    no cut is ``retime.window_plan``) on its own instants through the BGR window path -- 8 bits: one module forward per instant
    (``module_window_ts_u8``), per tile and stitched when ``plan`` is given; above: ONE ``run_windows_u16`` --; each output picked
    by the window's outputs; numpy BGR -> payload in the same layout.  Returns (bytes, cut windows)."""
    hdr, pays = _read(data)
    d, lay, n = hdr.depth, hdr.layout, len(pays)
    frames = [_to_bgr_np(p if d == 8 else y4m.as_samples16(p), hdr.h, hdr.w, d, lay, matrix, hdr.full_range) if lay != '420' else
              y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma) for p in pays]
    cuts = cuts or []
    is_cut = S.with_sentinels(lambda j: j in cuts, n) if full_length else (lambda j: j in cuts)
    k0, nw = R.first_window(n, full_length), R.n_windows(n, full_length)
    runs, outs, n_cut = [], [], 0
    for k in range(k0, k0 + nw):
        wr, wo = S.window_runs(k, r, k == k0 + nw - 1, is_cut, full_length)
        n_cut += len(wr) - 1
        outs += [(len(runs) + run, kind, j) for _, run, kind, j in wo]
        runs += wr
    if d > 8:
        dev = [_dev(f, d) for f in frames]
        rn = ClipRunner(model, hdr.h, hdr.w, n_tst, 8, retime=r).runner                  # the runner the video path builds
        st, s01 = rn.run_windows_u16([[dev[x] for x in S.runner_order(tup)] for tup, _ in runs], d, ts=[ts for _, ts in runs])
        torch.cuda.synchronize()
        st, s01 = _host(st, d), _host(s01, d)
        res = [(st[i], s01[i]) for i in range(len(runs))]
    elif plan is None:
        tf = [torch.from_numpy(f) for f in frames]
        res = [[a.cpu().numpy() for a in module_window_ts_u8(model, [tf[x] for x in S.runner_order(tup)], n_tst, ts)] for tup, ts in runs]
    else:
        tiles = [torch.from_numpy(T.crop_np(f, plan)) for f in frames]
        res = []
        for tup, ts in runs:
            per = [[a.cpu().numpy() for a in module_window_ts_u8(model, [tiles[x][j] for x in S.runner_order(tup)], n_tst, ts)]
                   for j in range(plan.n_tiles)]
            res.append(tuple(np.stack([T.stitch_np(np.stack([per[j][part][i] for j in range(plan.n_tiles)]), plan, hdr.h, hdr.w)
                                       for i in range(per[0][part].shape[0])]) for part in range(2)))
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    for run, kind, j in outs:
        st, s01 = res[run]
        f = s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[j]
        out += [b'FRAME\n', _to_yuv_np(np.ascontiguousarray(f), d, lay, matrix, hdr.full_range).tobytes()]
    assert len(outs) == R.n_output_frames(n, r, full_length)
    return b''.join(out), n_cut


def _same(got, exp):
    g, e = got.split(b'FRAME\n'), exp.split(b'FRAME\n')
    assert len(got) == len(exp) and len(g) == len(e), (len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(g, e)) if a != b]
    assert not bad, 'frames differ (0 = header): %s' % bad[:10]


def _run(model, data, n_tst, batch=4, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, layouts=True, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _two_ranks(model, data, n_tst, tmp_path, **kw):
    """Two ranks of one file, run one after the other in this process (rank 0 sizes the file first)."""
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tot = [0, 0]
    for rank in range(2):
        nw, nf = VideoRunner(model, n_tst, batch=2, layouts=True, **kw).run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += nw
        tot[1] += nf
    return tot, dst.read_bytes()


STREAMS = [('422', 8), ('444', 8), ('mono', 8), ('422', 10)]


@pytest.mark.parametrize('layout,d', STREAMS, ids=['422', '444', 'mono', '422p10'])
def test_stream_and_two_ranks_equal_the_composed_expectation(layout, d, model16, tmp_path):
    h, w, n = 48, 80, 7
    matrix, full = ('bt709', True) if layout == '444' else ('bt601', False)
    data, pays, _ = _clip(n, h, w, layout, d, matrix, full, seed=3)
    hd = {'high_depth': True} if d > 8 else {}
    exp, _ = _expected(model16, data, 2, Fraction(4), matrix)
    nf_exp = R.n_output_frames(n, 4)
    tag = _tag(layout, d).encode()
    assert exp.startswith(b'YUV4MPEG2 W80 H48 F96:1 Ip C' + tag + (b' ' if full else b'\n'))
    assert len(exp) == exp.index(b'FRAME') + nf_exp * (6 + y4m.payload_bytes(h, w, d, layout))
    vr, nw, nf, got = _run(model16, data, 2, mfi=4, matrix=matrix, **hd)
    assert (nw, nf, vr.last_depth, vr.last_layout) == (n - 3, nf_exp, d, layout)
    _same(got, exp)
    assert vr.last_decode_peak <= 4 + 5
    tot, got = _two_ranks(model16, data, 2, tmp_path, mfi=4, matrix=matrix, **hd)
    assert tot == [n - 3, nf_exp]
    _same(got, exp)
    if d > 8:                                                               # a deep layout needs both switches
        with pytest.raises(y4m.Y4MError, match='--high-depth'):
            VideoRunner(model16, 2, mfi=4, layouts=True).run_stream(io.BytesIO(data), io.BytesIO())
        with pytest.raises(y4m.Y4MError, match='--any-layout'):
            VideoRunner(model16, 2, mfi=4, high_depth=True).run_stream(io.BytesIO(data), io.BytesIO())


@pytest.mark.parametrize('layout,d', [('422', 8), ('422', 10)], ids=['422', '422p10'])
def test_non_integer_ratio(layout, d, model16, tmp_path):
    data, _, _ = _clip(7, 48, 80, layout, d, seed=4)
    r = Fraction(5, 2)
    hd = {'high_depth': True} if d > 8 else {}
    exp, _ = _expected(model16, data, 2, r, 'bt601')
    vr, nw, nf, got = _run(model16, data, 2, fps=Fraction(60), matrix='bt601', **hd)
    assert (nw, nf) == (4, R.n_output_frames(7, r)) and vr.last_fps_out == 60
    _same(got, exp)
    tot, got = _two_ranks(model16, data, 2, tmp_path, fps=Fraction(60), matrix='bt601', **hd)
    assert tot == [4, R.n_output_frames(7, r)]
    _same(got, exp)


def test_full_length_444(model16, tmp_path):
    data, _, _ = _clip(5, 48, 80, '444', 8, seed=2, fps=b'30:1')
    exp, _ = _expected(model16, data, 2, Fraction(2), 'bt601', full_length=True)
    vr, nw, nf, got = _run(model16, data, 2, batch=2, mfi=2, matrix='bt601', full_length=True)
    assert (nw, nf) == (4, 10)
    _same(got, exp)
    tot, got = _two_ranks(model16, data, 2, tmp_path, mfi=2, matrix='bt601', full_length=True)
    assert tot == [4, 10]
    _same(got, exp)


@pytest.mark.parametrize('layout,d,thr', [('422', 8, S.DEFAULT_THRESHOLD), ('444', 10, 8.0)], ids=['422', '444p10'])
def test_scene_cut_on_a_planted_cut(layout, d, thr, model16):
    """The planted cut scores about 13 over a 4:2:2 payload and about 9.4 over a 4:4:4 one (two thirds of its samples are chroma,
    which the cut changes less than luma), so the 4:4:4 stream is run at T = 8."""
    h, w, cut = 48, 80, 6

    def look(i, bgr, peak):                                                 # a hard cut before frame 6: another scene's colours
        return bgr if i < cut else ((peak - bgr) // 3).astype(bgr.dtype)
    data, pays, _ = _clip(11, h, w, layout, d, seed=1, look=look)
    P, peak = y4m.payload_size(h, w, layout), (1 << d) - 1
    assert pays[0].size == P
    sads = [S.sad_np(pays[j], pays[j - 1]) for j in range(1, len(pays))]
    cuts = S.cuts_of(sads, P, thr, peak=peak)                               # the numpy detector over the layout's P samples
    assert cuts == [cut]
    hd = {'high_depth': True} if d > 8 else {}
    exp, n_cut = _expected(model16, data, 2, Fraction(4), 'bt601', cuts=cuts)
    vr, nw, nf, got = _run(model16, data, 2, mfi=4, matrix='bt601', scene_cut=thr, **hd)
    assert (nw, nf) == (8, R.n_output_frames(11, 4))
    assert vr.last_cuts == cuts and vr.last_cut_windows == n_cut == 1
    _same(got, exp)
    plain = _run(model16, data, 2, mfi=4, matrix='bt601', **hd)[3]
    assert len(plain) == len(exp) and plain != exp


def test_tiles_on_an_8_bit_444_stream(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data, _, _ = _clip(5, h, w, '444', 8, seed=4)
    p = T.plan_tiles(h, w, tile, margin)
    assert p.n_tiles == 4
    exp, _ = _expected(model16, data, 2, Fraction(2), 'bt601', plan=p)
    vr, nw, nf, got = _run(model16, data, 2, batch=2, mfi=2, matrix='bt601', tile=tile, tile_margin=margin)
    assert (nw, nf) == (2, 5) and vr.last_plan == p and vr.last_layout == '444'
    _same(got, exp)


def test_tiles_with_a_deep_layout_stay_refused(model16):
    data, _, _ = _clip(5, 48, 80, '422', 10)
    vr = VideoRunner(model16, 1, mfi=2, batch=2, high_depth=True, layouts=True, tile='auto')
    with pytest.raises(ValueError) as e:
        vr.run_stream(io.BytesIO(data), io.BytesIO())
    assert 'tile' in str(e.value) and '10-bit' in str(e.value) and not vr._runners


def test_mono_luma_equals_the_420_stream_with_neutral_chroma(model16):
    """The BGR frames of a mono stream and of the 4:2:0 stream with the same luma and chroma at 128 are the same, so the forward
    is the same and the output Y planes are byte-identical."""
    h, w, n = 48, 80, 6
    mono, pays, _ = _clip(n, h, w, 'mono', 8, seed=6)
    nc = 2 * (h // 2) * (w // 2)
    d420 = b'YUV4MPEG2 W80 H48 F24:1 Ip C420jpeg\n' + b''.join(b'FRAME\n' + p.tobytes() + bytes([128]) * nc for p in pays)
    _, nw, nf, got = _run(model16, mono, 2, mfi=4, matrix='bt601')
    out420 = io.BytesIO()
    assert VideoRunner(model16, 2, mfi=4, batch=4, matrix='bt601').run_stream(io.BytesIO(d420), out420) == (nw, nf)
    hm, pm = _read(got)
    h4, p4 = _read(out420.getvalue())
    assert (hm.layout, h4.layout, len(pm), len(p4)) == ('mono', '420', nf, nf) and nf == R.n_output_frames(n, 4)
    for a, b in zip(pm, p4):
        assert a.size == h * w and np.array_equal(a, b[:h * w])
    assert np.stack(pm).std() > 5                                          # pictures, not a constant


def test_switch_off_is_the_default_path(model16, tmp_path):
    data, _, _ = _clip(7, 48, 80, '420', 8, seed=5)
    outs = []
    for on in (False, True):
        vr = VideoRunner(model16, 2, mfi=4, batch=4, layouts=on)
        out = io.BytesIO()
        assert vr.run_stream(io.BytesIO(data), out) == (4, 17) and vr.last_layout == '420'
        outs.append(out.getvalue())
    assert outs[0] == outs[1] and b' C420jpeg' in outs[1][:80]
    c422, _, _ = _clip(5, 48, 80, '422', 8)
    vr = VideoRunner(model16, 2, mfi=4, batch=4)
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(y4m.Y4MError) as e:
        vr.run_stream(io.BytesIO(c422), io.BytesIO())
    assert y4m.FIX in str(e.value) and '--any-layout' in str(e.value)
    src = tmp_path / 'in.y4m'
    src.write_bytes(c422)
    with pytest.raises(y4m.Y4MError):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert not vr._runners and torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)             # nothing was allocated for it
