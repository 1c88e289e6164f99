"""The 16-bit frame path of the Y4M edge (``--high-depth``: C420p10 .. C420p16) on a real MI355X: its kernels (csrc/yuv_family.hip,
csrc/yuv.hip, csrc/frames16.hip) bit-exact against their numpy definitions, the uint16 ingest / egress against the uint8 kernels (depth 8) and against numpy, the
whole 16-bit container path anchored to the 8-bit emit path value for value, and ``VideoRunner(high_depth=True)`` byte-identical
to the expectation composed from the numpy definitions and ``WindowRunner.run_windows_u16``."""
import ctypes as C
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
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.runner import WindowRunner                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
MCODE = {'bt601': L.BT601, 'bt709': L.BT709}
SCODE = {'420jpeg': L.SITING_420JPEG, '420mpeg2': L.SITING_420MPEG2}
GUARD = 0xA5C3
ERR_ARG = -1


def _dev16(a):
    """uint16 numpy array -> int16 GPU tensor holding the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(DEV)


def _np16(t):
    return t.cpu().numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _to_bgr16_gpu(pays, h, w, d, matrix, full, siting, src_pad=0, dst_pad=0):
    """pays [n, P] uint16 -> [n, h, w, 3] through demfi_yuv420p16_to_bgr16 at padded strides (samples); the padding stays untouched."""
    n, P = pays.shape
    F = h * w * 3
    src = np.zeros((n, P + src_pad), np.uint16)
    src[:, :P] = pays
    src = _dev16(src)
    dst = _dev16(np.full((n, F + dst_pad), GUARD, np.uint16))
    L.check(L.load().demfi_yuv420p16_to_bgr16(src.data_ptr(), P + src_pad, dst.data_ptr(), F + dst_pad, n, h, w, d, MCODE[matrix], int(full),
                                              SCODE[siting], _stream()), 'yuv420p16_to_bgr16')
    out = _np16(dst)
    assert (out[:, F:] == GUARD).all(), 'write outside the frames'
    return out[:, :F].reshape(n, h, w, 3)


def _gather_gpu(frames, order, d, matrix, full, src_pad=0, dst_pad=0, lead=0):
    """frames [nb, h, w, 3] uint16 kept at a padded stride behind ``lead`` samples; frame order[f] -> payload f."""
    nb, h, w = frames.shape[:3]
    F, P = h * w * 3, y4m.payload_size(h, w)
    fs = F + src_pad
    base = np.zeros(lead + nb * fs + 64, np.uint16)
    for i in range(nb):
        base[lead + i * fs:lead + i * fs + F] = frames[i].reshape(-1)
    base = _dev16(base)
    before = base.clone()
    offs = torch.tensor([lead + i * fs for i in order], dtype=torch.int64, device=DEV)
    ds = P + dst_pad
    dst = _dev16(np.full((len(order), ds), GUARD, np.uint16))
    L.check(L.load().demfi_bgr16_to_yuv420p16_gather(base.data_ptr(), offs.data_ptr(), dst.data_ptr(), ds, len(order), h, w, d,
                                                     MCODE[matrix], int(full), _stream()), 'bgr16_to_yuv420p16_gather')
    out = _np16(dst)
    assert (out[:, P:] == GUARD).all(), 'write outside the payloads'
    assert torch.equal(base, before)
    return out[:, :P]


SIZES = [(2, 2), (3, 5), (5, 3), (6, 9), (37, 53), (70, 98), (64, 128), (720, 1280)]  # those of tests/test_gpu_y4m.py, and a width of 8k + 1
DEPTHS = [8, 10, 12, 16]


# ---- 1. conversion and SAD kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('d', DEPTHS)
@pytest.mark.parametrize('matrix,full', [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)])
def test_kernels_bit_exact_against_numpy(h, w, d, matrix, full):
    g = np.random.RandomState(h * 7 + w + d)
    peak = (1 << d) - 1
    pays = g.randint(0, peak + 1, (2, y4m.payload_size(h, w))).astype(np.uint16)
    pays[1, ::3] = g.randint(0, 65536, pays[1, ::3].size)                  # values above the peak: taken as they are, like numpy
    for siting in y4m.SITINGS:
        got = _to_bgr16_gpu(pays, h, w, d, matrix, full, siting)
        for i in range(2):
            assert np.array_equal(got[i], y4m.yuv420_to_bgr16_np(pays[i], h, w, d, matrix, full, siting)), (siting, i)
    bgr = g.randint(0, peak + 1, (2, h, w, 3)).astype(np.uint16)
    bgr[1, ::2, ::3] = g.randint(0, 65536, bgr[1, ::2, ::3].shape)
    got = _gather_gpu(bgr, [1, 0], d, matrix, full)
    for f, i in enumerate([1, 0]):
        assert np.array_equal(got[f], y4m.bgr16_to_yuv420_np(bgr[i], d, matrix, full)), i


@pytest.mark.parametrize('h,w', [(37, 53), (70, 98)])
def test_depth_8_equals_the_8_bit_kernels(h, w):
    g = np.random.RandomState(w)
    lib, st = L.load(), _stream()
    P, F = y4m.payload_size(h, w), h * w * 3
    pays = g.randint(0, 256, (3, P)).astype(np.uint8)
    src, dst = torch.from_numpy(pays).to(DEV), torch.zeros((3, F), dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_yuv420_to_bgr(src.data_ptr(), P, dst.data_ptr(), F, 3, h, w, L.BT709, 0, L.SITING_420MPEG2, st))
    got = _to_bgr16_gpu(pays.astype(np.uint16), h, w, 8, 'bt709', False, '420mpeg2')
    assert np.array_equal(got.reshape(3, F), dst.cpu().numpy().astype(np.uint16))
    offs = torch.tensor([2 * F, 0, F], dtype=torch.int64, device=DEV)
    pay8 = torch.zeros((3, P), dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_bgr_to_yuv420_gather(dst.data_ptr(), offs.data_ptr(), pay8.data_ptr(), P, 3, h, w, L.BT601, 1, st))
    got = _gather_gpu(got, [2, 0, 1], 8, 'bt601', True)
    assert np.array_equal(got, pay8.cpu().numpy().astype(np.uint16))


@pytest.mark.parametrize('h,w', [(6, 9), (37, 53), (64, 128), (70, 98)])
@pytest.mark.parametrize('pad', [0, 8, 13])
@pytest.mark.parametrize('d', [10, 16])
def test_strided_batches_and_gather_order(h, w, pad, d):
    """Several frames per launch at strides larger than a frame (0, 8, 13 samples: aligned and only 2-byte aligned), and gather
    offsets in shuffled order with repeats behind an odd number of leading samples."""
    g = np.random.RandomState(pad + d)
    peak = (1 << d) - 1
    pays = g.randint(0, peak + 1, (5, y4m.payload_size(h, w))).astype(np.uint16)
    got = _to_bgr16_gpu(pays, h, w, d, 'bt709', False, '420mpeg2', src_pad=pad, dst_pad=2 * pad + (1 if pad == 13 else 0))
    for i in range(5):
        assert np.array_equal(got[i], y4m.yuv420_to_bgr16_np(pays[i], h, w, d, 'bt709', False, '420mpeg2')), i
    bgr = g.randint(0, peak + 1, (6, h, w, 3)).astype(np.uint16)
    order = [4, 0, 0, 5, 2, 2, 1, 3, 4]
    got = _gather_gpu(bgr, order, d, 'bt601', True, src_pad=pad, dst_pad=2 * pad + 3, lead=pad)
    for f, i in enumerate(order):
        assert np.array_equal(got[f], y4m.bgr16_to_yuv420_np(bgr[i], d, 'bt601', True)), (f, i)


def _sad(base, a_offs, b_offs, samples):
    n = len(a_offs)
    od = torch.tensor(list(a_offs) + list(b_offs), dtype=torch.int64, device=DEV)
    sad = torch.full((n + 1,), 77, dtype=torch.int64, device=DEV)
    L.check(L.load().demfi_yuv420p16_sad(base.data_ptr(), od.data_ptr(), od[n:].data_ptr(), n, samples, sad.data_ptr(), _stream()), 'sad')
    out = sad.cpu().tolist()
    assert out[n] == 77, 'write past the n sums'
    return out[:n]


@pytest.mark.parametrize('samples', [1, 7, 8, 9, 23, 1000, y4m.payload_size(37, 53), y4m.payload_size(70, 98), y4m.payload_size(720, 1280)])
@pytest.mark.parametrize('d', DEPTHS)
def test_sad_bit_exact_against_numpy(samples, d):
    g = np.random.RandomState(samples % 9973 + d)
    peak = (1 << d) - 1
    a_offs = [0, 1, 3, 8, 5, 2 * samples + 37]                             # even and odd sample offsets, a pair on itself, repeats
    b_offs = [samples + 19, samples + 24, 2, 8, 2 * samples + 40, 1]
    host = g.randint(0, peak + 1, 3 * samples + 64).astype(np.uint16)
    got = _sad(_dev16(host), a_offs, b_offs, samples)
    for f, (a, b) in enumerate(zip(a_offs, b_offs)):
        assert got[f] == S.sad_np(host[a:a + samples], host[b:b + samples]), (f, a, b)
    assert got[3] == 0


def test_sad_of_extreme_frames_is_exact():
    samples = y4m.payload_size(1080, 1920)
    host = np.zeros(2 * samples + 1, np.uint16)
    host[samples + 1:] = 65535
    assert _sad(_dev16(host), [0, 1], [samples + 1, samples], samples) == [65535 * samples, 65535 * (samples - 1)]   # > 2^32


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib = L.load()
    buf = _dev16(np.full(256, GUARD, np.uint16))
    offs = torch.zeros(4, dtype=torch.int64, device=DEV)
    sad = torch.full((2,), 77, dtype=torch.int64, device=DEV)
    f32 = torch.full((3 * 32 * 32,), 0.25, device=DEV)
    st = _stream()
    p, fsz = y4m.payload_size(2, 2), 12

    def bad(fn, ok, i, v):
        a = list(ok)
        a[i] = v
        return fn(*a) == ERR_ARG
    ok = (buf.data_ptr(), p, buf.data_ptr() + 128, fsz, 2, 2, 2, 10, 0, 0, 0, st)            # to_bgr16
    fn = lib.demfi_yuv420p16_to_bgr16
    assert bad(fn, ok, 7, 7) and bad(fn, ok, 7, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 2, None)
    assert bad(fn, ok, 1, p - 1) and bad(fn, ok, 3, fsz - 1) and bad(fn, ok, 4, -1)
    assert bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385) and bad(fn, ok, 8, 2) and bad(fn, ok, 9, 2) and bad(fn, ok, 10, 5)
    assert bad(fn, ok, 0, buf.data_ptr() + 1)                                                # odd address
    ok = (buf.data_ptr(), offs.data_ptr(), buf.data_ptr() + 128, p, 2, 2, 2, 10, 0, 0, st)   # gather
    fn = lib.demfi_bgr16_to_yuv420p16_gather
    assert bad(fn, ok, 7, 7) and bad(fn, ok, 7, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 2, None)
    assert bad(fn, ok, 3, p - 1) and bad(fn, ok, 4, -1) and bad(fn, ok, 5, 1) and bad(fn, ok, 6, 16385) and bad(fn, ok, 8, 2) and bad(fn, ok, 9, 2)
    ok = (buf.data_ptr(), offs.data_ptr(), offs.data_ptr() + 16, 2, 6, sad.data_ptr(), st)   # sad
    fn = lib.demfi_yuv420p16_sad
    assert bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 2, None) and bad(fn, ok, 5, None)
    assert bad(fn, ok, 3, -1) and bad(fn, ok, 4, 0) and bad(fn, ok, 0, buf.data_ptr() + 1)
    ptrs = (C.c_void_p * 4)(*[buf.data_ptr()] * 4)
    ok = (ptrs, 20, 20, 10, f32.data_ptr(), f32.data_ptr(), f32.data_ptr(), L.F32, 32, 32, st)  # ingest
    fn = lib.demfi_u16_ingest
    assert bad(fn, ok, 3, 7) and bad(fn, ok, 3, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 4, None) and bad(fn, ok, 7, 9)
    assert bad(fn, ok, 1, 1) and bad(fn, ok, 8, 31) and bad(fn, ok, 0, (C.c_void_p * 4)(buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr()))
    ok = (f32.data_ptr(), buf.data_ptr(), 2, 2, 32, 32, 10, st)                              # frame_to_u16
    fn = lib.demfi_frame_to_u16
    assert bad(fn, ok, 6, 7) and bad(fn, ok, 6, 17) and bad(fn, ok, 0, None) and bad(fn, ok, 1, None) and bad(fn, ok, 4, 1)
    torch.cuda.synchronize()
    assert (_np16(buf) == GUARD).all() and sad.cpu().tolist() == [77, 77] and bool((f32 == 0.25).all())


# ---- 2. uint16 ingest / egress ------------------------------------------------------------------------------------------------
def _ingest(fn, frames, h, w, H, W, dt, dtype, *depth):
    x = torch.zeros(3, 4, H, W, device=DEV)
    s2d = torch.zeros(H // 2, W // 2, 48, device=DEV, dtype=dtype)
    ov = torch.zeros(3, H, W, device=DEV)
    ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in frames])
    L.check(fn(ptrs, h, w, *depth, x.data_ptr(), s2d.data_ptr(), ov.data_ptr(), dt, H, W, _stream()), 'ingest')
    torch.cuda.synchronize()
    return x, s2d, ov


@pytest.mark.parametrize('h,w,H,W', [(50, 70, 64, 96), (64, 96, 64, 96)])
def test_u16_ingest(h, w, H, W):
    lib = L.load()
    g = np.random.RandomState(h)
    for dtype, dt in ((torch.float16, L.F16), (torch.float32, L.F32)):
        f8 = [g.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(4)]
        ref = _ingest(lib.demfi_u8_ingest, [torch.from_numpy(f).to(DEV) for f in f8], h, w, H, W, dt, dtype)
        got = _ingest(lib.demfi_u16_ingest, [_dev16(f.astype(np.uint16)) for f in f8], h, w, H, W, dt, dtype, 8)
        for a, b in zip(got, ref):                                         # depth 8 on widened frames: the bits of the uint8 ingest
            assert torch.equal(a, b)
        for d in (10, 16):
            peak = (1 << d) - 1
            f16 = [g.randint(0, peak + 1, (h, w, 3)).astype(np.uint16) for _ in range(4)]
            f16[0][:2, :3] = [[[0, peak, peak // 2]] * 3] * 2
            x, s2d, ov = _ingest(lib.demfi_u16_ingest, [_dev16(f) for f in f16], h, w, H, W, dt, dtype, d)
            v = np.stack(f16).astype(np.float32) / np.float32(peak)        # the three-step fp32 expression
            v = v - np.float32(0.5)
            v = v * np.float32(2.0)
            assert v.dtype == np.float32
            exp = torch.from_numpy(np.ascontiguousarray(v.transpose(3, 0, 1, 2)))              # [3,4,h,w]
            exp = torch.nn.functional.pad(exp.reshape(1, 12, h, w), [0, W - w, 0, H - h], mode='reflect').reshape(3, 4, H, W) \
                if (H, W) != (h, w) else exp
            assert torch.equal(x.cpu(), exp), d
            s2d1, ov1 = torch.zeros_like(s2d), torch.zeros_like(ov)        # the record and the overlay: those of the fp32 planes
            L.check(lib.demfi_space_to_depth(x.data_ptr(), s2d1.data_ptr(), dt, H, W, _stream()))
            L.check(lib.demfi_overlay_mean(x.data_ptr(), ov1.data_ptr(), H, W, _stream()))
            torch.cuda.synchronize()
            assert torch.equal(s2d, s2d1) and torch.equal(ov, ov1), d


def test_frame_to_u16():
    lib, st = L.load(), _stream()
    h, w, H, W = 50, 70, 64, 96
    g = torch.Generator().manual_seed(3)
    fr = (torch.randn(3, H, W, generator=g) * 0.8)
    out8 = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    out16 = torch.zeros(h, w, 3, dtype=torch.int16, device=DEV)
    L.check(lib.demfi_frame_to_u8(fr.to(DEV).data_ptr(), out8.data_ptr(), h, w, H, W, st))
    L.check(lib.demfi_frame_to_u16(fr.to(DEV).data_ptr(), out16.data_ptr(), h, w, H, W, 8, st))
    torch.cuda.synchronize()
    assert np.array_equal(_np16(out16), out8.cpu().numpy().astype(np.uint16))
    for d in (10, 16):
        peak = (1 << d) - 1
        a = fr.numpy().copy()                                               # randn * 0.8 holds values below -1 and above 1
        assert (a < -1).any() and (a > 1).any()
        k = np.random.RandomState(d).randint(0, peak + 1, a[:, :h, :w].shape)
        k[0, 0, :4] = [0, 1, peak - 1, peak]
        grid = (np.float32(2.0) * k.astype(np.float32) / np.float32(peak) - np.float32(1.0)).astype(np.float32)
        step = np.random.RandomState(d + 1).randint(-1, 2, grid.shape)     # the grid point k / peak, or one fp32 ulp to either side
        grid = np.where(step < 0, np.nextafter(grid, np.float32(-2)), np.where(step > 0, np.nextafter(grid, np.float32(2)), grid))
        a[:, 8:h, :w] = grid[:, 8:, :]
        a[:, 0, :4] = grid[:, 0, :4]
        dev = torch.from_numpy(a).to(DEV)
        L.check(lib.demfi_frame_to_u16(dev.data_ptr(), out16.data_ptr(), h, w, H, W, d, st))
        torch.cuda.synchronize()
        exp = (np.clip((a[:, :h, :w].astype(np.float64) + 1.0) / 2.0, 0.0, 1.0) * float(peak)).astype(np.uint16)
        assert np.array_equal(_np16(out16), exp.transpose(1, 2, 0)), d


# ---- 3. the 16-bit container path against the 8-bit emit path -------------------------------------------------------------------
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


def _u8_emit_path(rn, wins):
    """``run_windows_u8`` with the emit path (``sink_rows=None``) whatever the engine."""
    out = torch.empty((len(wins), rn.mfi - 1, rn.h, rn.w, 3), dtype=torch.uint8, device=DEV)
    s01 = torch.empty((len(wins), 2, rn.h, rn.w, 3), dtype=torch.uint8, device=DEV)
    io_ = [rn._u8_io(wins[i], out[i], s01[i], None) for i in range(len(wins))]
    cur = rn._begin()
    for load, emit, pre in io_:
        rn._window(load, emit, body_only=True, pre=pre)
    rn._end(cur)
    torch.cuda.synchronize()
    return out, s01


@pytest.mark.parametrize('dtype', ['fp32', 'fp16'])
def test_depth_8_container_path_equals_the_8_bit_emit_path(dtype, model16, model32):
    model = model16 if dtype == 'fp16' else model32
    h, w = 50, 70
    g = np.random.RandomState(11)
    base = ((synthetic_window(h + 8, w + 8, 4)[0, :, 0].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
    fr = [np.ascontiguousarray(base[i:i + h, 2 * i:2 * i + w]) for i in range(5)]
    fr[2] = g.randint(0, 256, (h, w, 3)).astype(np.uint8)                  # noise too: every byte value on the way in
    wins = [(1, 2, 0, 3), (2, 3, 1, 4), (3, 3, 3, 3)]
    rn = WindowRunner(model, h, w, n_tst=2, mfi=4)
    d8 = [torch.from_numpy(f).to(DEV) for f in fr]
    d16 = [_dev16(f.astype(np.uint16)) for f in fr]
    st8, s8 = _u8_emit_path(rn, [[d8[i] for i in win] for win in wins])
    st16, s16 = rn.run_windows_u16([[d16[i] for i in win] for win in wins], 8)
    torch.cuda.synchronize()
    assert np.array_equal(_np16(st16), st8.cpu().numpy().astype(np.uint16))
    assert np.array_equal(_np16(s16), s8.cpu().numpy().astype(np.uint16))
    assert st8.cpu().numpy().std() > 5                                     # pictures, not a constant
    stq, sq = rn.run_windows_u8([[d8[i] for i in win] for win in wins])     # fp16: the fused sink; fp32: the emit path again
    torch.cuda.synchronize()
    diff = int((stq != st8).sum()) + int((sq != s8).sum())
    print('%s: run_windows_u8 (%s) differs from the emit path in %d of %d bytes'
          % (dtype, 'fused uint8 sink' if rn.engine.supports_u8_sink else 'emit path', diff, st8.numel() + s8.numel()))
    # a uint8 run after a 16-bit one, and a 16-bit one after a uint8 sink run, on the same engine: nothing leaks
    st16b, _ = rn.run_windows_u16([[d16[i] for i in win] for win in wins], 8)
    torch.cuda.synchronize()
    assert torch.equal(st16b, st16)


def test_run_windows_u16_checks_its_frames(model32):
    rn = WindowRunner(model32, 48, 80, n_tst=1, mfi=2)
    ok = [torch.zeros((48, 80, 3), dtype=torch.int16, device=DEV) for _ in range(4)]
    with pytest.raises(ValueError):
        rn.run_windows_u16([ok], 9)
    with pytest.raises(ValueError):
        rn.run_windows_u16([ok[:3]], 10)
    with pytest.raises(ValueError):
        rn.run_windows_u16([[f.to(torch.uint8) for f in ok]], 10)
    with pytest.raises(ValueError):
        rn.run_windows_u16([[f.cpu() for f in ok]], 10)
    with pytest.raises(ValueError):
        rn.run_windows_u16([ok], 10, ts=[[0.5], [0.5]])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
def _clip16(n, h, w, header, d, matrix, full, seed=0, look=None):
    """A seeded clip of n frames of a moving pattern as a Y4M stream of 16-bit samples at depth d (bytes)."""
    peak = (1 << d) - 1
    base = synthetic_window(h + 2 * n, w + 2 * n, seed)[0, :, 0]
    pays = []
    for i in range(n):
        f = base[:, i:i + h, 2 * i:2 * i + w].permute(1, 2, 0).numpy().astype(np.float64)
        bgr = ((f + 1) / 2 * peak).clip(0, peak).astype(np.uint16)
        if look is not None:
            bgr = look(i, bgr, peak)
        pays.append(y4m.bgr16_to_yuv420_np(bgr, d, matrix, full))
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def _expected16(model, data, n_tst, r, matrix, full_length=False, cuts=None):
    """numpy YUV -> BGR at the stream's depth, every run of every window (``scene.window_runs``; a window that touches no cut is
    ``retime.window_plan``) in ONE ``run_windows_u16`` on its own instants, each output picked by the window's outputs, numpy
    BGR -> YUV.  Returns (bytes, cut windows)."""
    rd = y4m.Reader(io.BytesIO(data), depths=y4m.DEPTHS)
    hdr = rd.header
    pays, buf = [], np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    d, n = hdr.depth, len(pays)
    frames = [_dev16(y4m.yuv420_to_bgr16_np(p, hdr.h, hdr.w, d, matrix, hdr.full_range, hdr.chroma)) for p in pays]
    cuts = cuts or []
    is_cut = S.with_sentinels(lambda j: j in cuts, n) if full_length else (lambda j: j in cuts)
    k0, nw = R.first_window(n, full_length), R.n_windows(n, full_length)
    runs, outs, n_cut = [], [], 0
    for k in range(k0, k0 + nw):
        wr, wo = S.window_runs(k, r, k == k0 + nw - 1, is_cut, full_length)
        n_cut += len(wr) - 1
        outs += [(len(runs) + run, kind, j) for _, run, kind, j in wo]
        runs += wr
    rn = ClipRunner(model, hdr.h, hdr.w, n_tst, 8, retime=r).runner                      # the runner the video path builds
    st, s01 = rn.run_windows_u16([[frames[x] for x in S.runner_order(tup)] for tup, _ in runs], d, ts=[ts for _, ts in runs])
    torch.cuda.synchronize()
    st, s01 = _np16(st), _np16(s01)
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    for run, kind, j in outs:
        f = s01[run, 0] if kind == R.S0 else s01[run, 1] if kind == R.S1 else st[run, j]
        out += [b'FRAME\n', y4m.bgr16_to_yuv420_np(f, d, matrix, hdr.full_range).tobytes()]
    assert len(outs) == R.n_output_frames(n, r, full_length)
    return b''.join(out), n_cut


CASES = [  # (dtype, n_tst, h, w, header, depth, matrix, full range, runner arguments, r)
    ('fp16', 3, 70, 98, b'YUV4MPEG2 W98 H70 F25:1 Ip A1:1 C420p10\n', 10, 'bt601', False, {'mfi': 4}, Fraction(4)),
    ('fp32', 2, 48, 80, b'YUV4MPEG2 W80 H48 F24:1 Ip C420p16 XCOLORRANGE=FULL\n', 16, 'bt709', True, {'fps': Fraction(60)}, Fraction(5, 2)),
]


@pytest.mark.parametrize('case', CASES, ids=['p10_x4_fp16', 'p16_full_24to60_fp32'])
def test_video_stream_and_ranks_equal_the_16_bit_frame_pipeline(case, model16, model32, tmp_path):
    dtype, n_tst, h, w, header, d, matrix, full, kw, r = case
    model = model16 if dtype == 'fp16' else model32
    data, pays = _clip16(9, h, w, header, d, matrix, full, seed=3)
    assert max(int(p.max()) for p in pays) > 255 * (1 << (d - 9))                            # the upper bits are in use
    exp, _ = _expected16(model, data, n_tst, r, matrix)
    nf_exp = R.n_output_frames(9, r)
    ohdr = R.output_header(y4m.parse_header(header, y4m.DEPTHS), y4m.parse_header(header, y4m.DEPTHS).fps * r).encode()
    assert b' C420p%d' % d in ohdr and exp.startswith(ohdr)
    assert len(exp) == len(ohdr) + nf_exp * (6 + 2 * y4m.payload_size(h, w))
    vr = VideoRunner(model, n_tst, batch=4, matrix=matrix, high_depth=True, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    assert (nw, nf, vr.last_depth) == (6, nf_exp, d)
    assert out.getvalue() == exp
    assert vr.last_decode_peak <= 4 + 5
    with pytest.raises(y4m.Y4MError):                                                        # off by default
        VideoRunner(model, n_tst, batch=4, matrix=matrix, **kw).run_stream(io.BytesIO(data), io.BytesIO())
    # two ranks of one file, run one after the other in this process (rank 0 sizes the file first)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tot = [0, 0]
    for rank in range(2):
        nw_r, nf_r = VideoRunner(model, n_tst, batch=2, matrix=matrix, high_depth=True, **kw).run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += nw_r
        tot[1] += nf_r
    assert tot == [6, nf_exp]
    assert dst.read_bytes() == exp


def test_scene_cut_at_10_bits(model16):
    h, w, d, cut = 48, 80, 10, 6

    def look(i, bgr, peak):                                                 # a hard cut before frame 6: another scene's colours
        return bgr if i < cut else ((peak - bgr) // 3).astype(np.uint16)
    data, pays = _clip16(11, h, w, b'YUV4MPEG2 W80 H48 F24:1 Ip C420p10\n', d, 'bt601', False, seed=1, look=look)
    sads = [S.sad_np(pays[j], pays[j - 1]) for j in range(1, len(pays))]
    cuts = S.cuts_of(sads, pays[0].size, S.DEFAULT_THRESHOLD, peak=(1 << d) - 1)              # the numpy detector
    assert cuts == [cut]
    exp, n_cut = _expected16(model16, data, 2, Fraction(4), 'bt601', cuts=cuts)
    vr = VideoRunner(model16, 2, mfi=4, batch=4, high_depth=True, scene_cut=S.DEFAULT_THRESHOLD)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    assert (nw, nf) == (8, R.n_output_frames(11, 4))
    assert vr.last_cuts == cuts and vr.last_cut_windows == n_cut == 1
    assert out.getvalue() == exp
    plain = io.BytesIO()
    VideoRunner(model16, 2, mfi=4, batch=4, high_depth=True).run_stream(io.BytesIO(data), plain)
    assert len(plain.getvalue()) == len(exp) and plain.getvalue() != exp


def test_full_length_at_12_bits(model16, tmp_path):
    h, w, d = 48, 80, 12
    data, _ = _clip16(6, h, w, b'YUV4MPEG2 W80 H48 F30:1 Ip C420p12\n', d, 'bt601', False, seed=2)
    exp, _ = _expected16(model16, data, 2, Fraction(2), 'bt601', full_length=True)
    vr = VideoRunner(model16, 2, mfi=2, batch=2, high_depth=True, full_length=True)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    assert (nw, nf) == (5, 12)
    assert out.getvalue() == exp
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    for rank in range(2):
        VideoRunner(model16, 2, mfi=2, batch=2, high_depth=True, full_length=True).run_file(str(src), str(dst), world=2, rank=rank)
    assert dst.read_bytes() == exp


def test_high_depth_leaves_an_8_bit_stream_alone(model16):
    base = synthetic_window(48 + 14, 80 + 14, 5)[0, :, 0]
    pays = []
    for i in range(7):
        bgr = ((base[:, i:i + 48, 2 * i:2 * i + 80].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        pays.append(y4m.bgr_to_yuv420_np(bgr, 'bt601', False))
    data = b'YUV4MPEG2 W80 H48 F24:1 Ip C420mpeg2\n' + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    outs = []
    for hd in (False, True):
        vr = VideoRunner(model16, 2, mfi=4, batch=4, high_depth=hd)
        out = io.BytesIO()
        assert vr.run_stream(io.BytesIO(data), out) == (4, 17) and vr.last_depth == 8
        outs.append(out.getvalue())
    assert outs[0] == outs[1] and b' C420jpeg' in outs[1][:80]


def test_tiles_with_a_10_bit_stream_are_refused(model16, tmp_path):
    data, _ = _clip16(5, 48, 80, b'YUV4MPEG2 W80 H48 F24:1 Ip C420p10\n', 10, 'bt601', False)
    vr = VideoRunner(model16, 1, mfi=2, batch=2, high_depth=True, tile='auto')
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError) as e:
        vr.run_stream(io.BytesIO(data), io.BytesIO())
    assert 'tile' in str(e.value) and '10-bit' in str(e.value)
    src = tmp_path / 'in.y4m'
    src.write_bytes(data)
    with pytest.raises(ValueError):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert not vr._runners and torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)             # nothing was allocated for it
