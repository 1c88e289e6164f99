"""The motion, gather, frame-I/O, visualisation and metric kernels inside poisoned guards (tests/guarded_arena.py) on a real MI355X:
every `extern "C"` compute entry point of pointwise.hip, fgac_window.hip, viz.hip and metrics.hip.

The convolution families already meet this contract (tests/test_gpu_guarded.py); these are the kernels whose ADDRESSES COME FROM
DATA -- flows that point out of the frame, splat targets, reflected indices, tile halos.  Every NHWC or planar demfi_view is a pitched
crop of a poisoned block (sy != W * sx, sc != H * W, sb != H * sy), every bare pointer a tight item between poison, every batched
launch gets the byte strides of those blocks, and a workspace has exactly the bytes its size query names.  Each launch asserts, in
this order:

  (b) nothing outside the listed destinations changed: guards, sources, workspaces beyond their contract, scratch;
  (c) no NaN / inf in what was written: no guard value consumed ("clamped address, weight 0" reads a FINITE in-frame neighbour: only
      a NaN neighbour shows a clamp that is off by one), no element left unwritten;
  (d) the reference comparison of the value tests (the shared bodies of tests/test_gpu_motion.py and tests/test_gpu_fgac_window.py:
      fp64 per element for the motion kernels, the oracle for the window FGAC and the metrics, equality for frame I/O; the single
      launches also write their debug index maps, which must equal the integer maps of the oracle);
  (e) the written bytes equal those of the same case and seed on plain contiguous tensors: nothing depends on addresses (the CFR
      splat is order-independent fixed point).

The shapes are the smallest at which each kernel's border logic has every branch live.  Out of reach on purpose: a non-finite
in-frame border pixel leaks into out-of-frame samples of gather4 / the fat-warp records (weight 0 times NaN); the arena never
poisons frame interiors.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from oracle import demfi_oracle as O                 # noqa: E402
from tests import guarded_arena as GA                # noqa: E402
from tests import motion_ref as R                    # noqa: E402
from tests import test_gpu_fgac_window as FW         # noqa: E402
from tests import test_gpu_motion as M               # noqa: E402

DEV = 'cuda:0'
f32 = np.float32
F16, F32 = torch.float16, torch.float32
FRAMES = [(37, 130), (16, 64)]                       # CFR tiles are 16x64: three ragged tile rows and columns / exactly one tile


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _both(body, capacity=32 << 20):
    """body(al) on plain contiguous tensors (the expectation of (e)), then inside the arena, where every launch asserts (b), (c) and
    the body asserts (d); then (e)."""
    plain = GA.Plain(DEV, recording=True)
    body(plain)
    arena = GA.Arena(DEV, capacity)
    body(arena)
    GA.assert_bit_identical(arena, plain)


def _refused(al, call):
    """An argument error, and nothing was launched: the arena is untouched."""
    al.snapshot()
    assert call() == -1
    torch.cuda.synchronize()
    al.check([])


def test_the_arena_detects_on_the_device():
    """tests/test_guarded_arena.py on the GPU in short: a torch "kernel" that stores at column W, and one that reads it."""
    al = GA.Arena(DEV, 1 << 20)
    src = al.fill(al.fat(1, 5, 7, 8, F16, name='src'), torch.ones(1, 5, 7, 8))
    dst = al.fat(1, 5, 7, 8, F16, name='dst')
    wide = lambda t: torch.as_strided(t, (1, 5, 8, 8), t.stride(), t.storage_offset())
    al.snapshot()
    dst.copy_(src)
    al.check([dst])
    al.assert_finite([dst])
    wide(dst)[0, 2, 7, 3] = 0
    with pytest.raises(GA.GuardError, match=r'"dst".*column 7 \(= W\) of image 0 written, at \(image 0, row 2, column 7, channel 3\)'):
        al.check([dst])
    dst[0, :, 6] = wide(src)[0, :, 7]
    with pytest.raises(GA.GuardError, match=r'"dst".*nan at index \[0, 0, 6, 0\]'):
        al.assert_finite([dst])


# ------------------------------------------------------------------------------------------------------------------------------
# CFR: demfi_cfr_flow_align, _batched, _pack
# ------------------------------------------------------------------------------------------------------------------------------
def test_outward_family_sends_the_edge_sources_across_every_edge():
    """CPU check of the new flow family: with t = 0.5 the splat corners of the sources within 2 px of an edge fall on both sides of it."""
    H, W = 16, 64
    f = M._cfr_flow('outward', H, W, np.random.default_rng(1))
    tx = np.arange(W)[None, :] + 0.5 * f[0]
    ty = np.arange(H)[:, None] + 0.5 * f[1]
    for tgt, n, edge in ((tx[:, :2], W, 'left'), (tx[:, -2:], W, 'right'), (ty[:2], H, 'top'), (ty[-2:], H, 'bottom')):
        lo = tgt.min() if edge in ('left', 'top') else tgt.min() - n
        hi = tgt.max() if edge in ('left', 'top') else tgt.max() - n
        assert lo == -1.75 and hi == 0.75, edge
        assert np.array_equal(tgt * 4, np.round(tgt * 4)), edge                # quarter steps: t * f is exact
    inner = np.abs(0.5 * f[:, 2:-2, 2:-2])
    assert inner.max() < 31                                                    # the rest of the field is near


@pytest.mark.parametrize('pack', [None, F16, F32], ids=['batched', 'pack16', 'pack32'])
@pytest.mark.parametrize('kind', ['threshold', 'edges', 'spikes', 'outward'])
@pytest.mark.parametrize('H,W', FRAMES)
def test_cfr(H, W, kind, pack):
    far = []
    _both(lambda al: far.append(M._cfr_body(al, H, W, 3, True, [kind], pack, seed=H + len(kind), dbg=True)))
    assert far[0] == far[1] and (far[0] > 0 or kind == 'outward')              # the far path ran (outward is near by construction)


# ------------------------------------------------------------------------------------------------------------------------------
# Fat warp: demfi_warp_blend, demfi_warp_blend_batched with _pad 0 and 1
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ab_ctx', [False, True], ids=['window_ab', 'ctx_ab'])
@pytest.mark.parametrize('dtype,Cc', [(F16, 8), (F16, 64), (F16, 512), (F32, 4), (F32, 64)])      # 1, 8, 64, 1, 16 lanes per pixel
@pytest.mark.parametrize('H,W', [(37, 130), (5, 65)])                          # 5x65: two tile rows, one column of one pixel
def test_fat_warp(H, W, dtype, Cc, ab_ctx):
    image = (H + 2 * GA.G) * (W + 2 * GA.G) * Cc * (2 if dtype == F16 else 4)
    _both(lambda al: M._fat_body(al, H, W, dtype, Cc, ab_ctx, seed=Cc + 1000 * ab_ctx + H, dbg=True), capacity=(8 << 20) + 18 * image)


# ------------------------------------------------------------------------------------------------------------------------------
# Thin warp + pack: demfi_warp_blend on planar views, demfi_warp_blend_pack, demfi_warp_blend_batched with a packed record
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ab_ctx', [False, True], ids=['window_ab', 'ctx_ab'])
@pytest.mark.parametrize('pack', [F16, F32], ids=['pack16', 'pack32'])
@pytest.mark.parametrize('H,W', [(37, 130), (9, 2)])                           # W = 2: the smallest frame the 8-byte pair path accepts
def test_thin_warp_pack(H, W, pack, ab_ctx):
    _both(lambda al: M._thin_pack_body(al, H, W, pack, ab_ctx, 3, seed=H + W, dbg=True))


@pytest.mark.parametrize('H,W', [(37, 130), (9, 2)])
def test_thin_warp_on_an_nhwc_view_takes_the_element_path(H, W):
    """fp16 NHWC with C = 12: not a 16-byte record, so the thin kernel without its pair loads."""
    _both(lambda al: M._nhwc_thin_body(al, H, W, F16, 12, dbg=True))


# ------------------------------------------------------------------------------------------------------------------------------
# demfi_fgac_gather + demfi_gate_blend
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F16, F32])
def test_fgac_gather_and_gate_blend(dtype):
    """Absolute positions from -3 to W + 2 / H + 2."""
    _both(lambda al: M._gather_gate_body(al, dtype, 37, 75, 64, far=(3.0,), dbg=True))


# ------------------------------------------------------------------------------------------------------------------------------
# demfi_fgac_window + demfi_avg_pool_fat
# ------------------------------------------------------------------------------------------------------------------------------
def _window_flow(H, W, rng):
    """Absolute positions, uniform in [-64, W + 64] x [-64, H + 64] -- across both clamps of the staged window base (-8 and W + 8 /
    H + 8) on both sides -- a quarter of them rounded to integers; all finite."""
    fl = np.stack([rng.uniform(-64, W + 64, (H, W)), rng.uniform(-64, H + 64, (H, W))]).astype(f32)
    m = rng.random((H, W)) < 0.25
    fl[:, m] = np.round(fl[:, m])
    return np.ascontiguousarray(fl)


@pytest.mark.parametrize('sr', [0, 1])
@pytest.mark.parametrize('dtype', [F16, F32])
@pytest.mark.parametrize('rr', [1, 2])
@pytest.mark.parametrize('H,W', [(13, 19), (16, 24)])                          # 247 pixels: the last workgroup has dead lanes
def test_fgac_window(H, W, rr, dtype, sr):
    rng = np.random.default_rng(H + 10 * rr + sr)
    rk = torch.from_numpy(np.tanh(rng.standard_normal((H, W, 64))).astype(f32)).to(DEV).to(dtype)
    sk = torch.from_numpy(np.tanh(rng.standard_normal((H, W, 64))).astype(f32)).to(DEV).to(dtype)
    fl = torch.from_numpy(_window_flow(H, W, rng)).to(DEV)
    nchw = lambda t: t.float().cpu().permute(2, 0, 1)[None]
    rkq, skq = nchw(rk), nchw(sk)
    if dtype == F16:                                  # the oracle on the SAME fp16-rounded inputs (pooled in fp32, rounded like the fp16 store)
        if sr:
            rkq = F.avg_pool2d(rkq, 2 * sr + 1, 1, sr).half().float()
            skq = F.avg_pool2d(skq, 2 * sr + 1, 1, sr).half().float()
        osr, tol_fac, tol_att, tol_sum = 0, 4e-3, 2e-3, 1e-5
    else:
        osr, tol_fac, tol_att, tol_sum = sr, 1e-4, 1e-5, 1e-6
    expect = {mode: O.fgac_window(rkq, skq, fl.cpu()[None], rr, osr, mode) for mode in (0, 1)}      # once, shared by both runs

    def body(al):
        for mode in (0, 1):
            efac, eatt = expect[mode]
            fac, att = FW._run(rk, sk, fl, rr, mode, sr, al=al)
            assert (att - eatt).abs().max() < tol_att and (fac - efac[0]).abs().max() < tol_fac, mode
            assert abs(float(att.sum(0).mean()) - 1.0) < tol_sum
            fac2, none = FW._run(rk, sk, fl, rr, mode, sr, al=al, want_attn=False)
            assert none is None and torch.equal(fac2, fac)

    _both(body)


@pytest.mark.parametrize('sr', [1, 2, 4])
@pytest.mark.parametrize('dtype', [F16, F32])
@pytest.mark.parametrize('H,W', [(13, 19), (16, 24)])
def test_avg_pool_fat(H, W, dtype, sr):
    """fp64 avg_pool2d with count_include_pad; the kernel adds `taps` fp32 terms in turn and divides once: at most
    (taps + 1) * 2^-24 * sum|v| / taps, plus half an fp16 ulp of the reference when the result is stored as fp16."""
    lib = L.load()
    rng = np.random.default_rng(sr + H)
    Cc, taps = 64, (2 * sr + 1) ** 2
    x = torch.from_numpy(np.tanh(rng.standard_normal((1, H, W, Cc))).astype(f32)).to(dtype)
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(x64, 2 * sr + 1, 1, sr)[0].permute(1, 2, 0).numpy()
    sabs = F.avg_pool2d(x64.abs(), 2 * sr + 1, 1, sr)[0].permute(1, 2, 0).numpy() * taps
    tol = (taps + 1) * 2.0 ** -24 * sabs / taps + (0.5 * R.fp16_ulp(ref) if dtype == F16 else 0.0)

    def body(al):
        src = al.fill(al.fat(1, H, W, Cc, dtype, name='src'), x)[0]
        out = al.fat(1, H, W, Cc, dtype, name='pooled')[0]
        vs, vo = FW._nhwc(src), FW._nhwc(out)
        GA.launch(al, lambda: lib.demfi_avg_pool_fat(C.byref(vs), C.byref(vo), Cc, H, W, sr, _stream()), [out], 'avg pool')
        err = np.abs(out.double().cpu().numpy() - ref)
        assert (err <= tol).all(), (float((err - tol).max()), int((err > tol).sum()))

    _both(body)


# ------------------------------------------------------------------------------------------------------------------------------
# demfi_pack_planes, demfi_pack_planes_batched
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F16, F32])
@pytest.mark.parametrize('nch', [8, 32])
def test_pack_planes(nch, dtype):
    """nb = 3, per-context and shared planes, two NULL planes, dst a channel slice of a wider record: the launch's channels equal
    planes.to(dtype), the other channels of the record keep their poison."""
    _both(lambda al: M._pack_body(al, nch, dtype, 37, 75, n_null=2))


# ------------------------------------------------------------------------------------------------------------------------------
# Frame I/O: demfi_u8_to_window, demfi_u8_ingest, demfi_u8_to_planar, demfi_frame_to_u8, demfi_reflect_pad,
# demfi_space_to_depth, demfi_overlay_mean
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,H,W', [(50, 70, 64, 96), (17, 33, 32, 64)])      # h = H/2 + 1: the largest legal padding, the reflected index reaches 0
def test_frame_io(h, w, H, W):
    lib = L.load()
    g = torch.Generator().manual_seed(h + W)
    frames = [torch.randint(0, 255, (h, w, 3), generator=g, dtype=torch.uint8) for _ in range(4)]   # never 255, the poison byte
    ref = O.frames_u8_to_tensor([f.numpy() for f in frames])                                          # [3,4,h,w]
    refp = F.pad(ref.reshape(1, 12, h, w), [0, W - w, 0, H - h], mode='reflect').reshape(3, 4, H, W)
    cat = refp.permute(1, 0, 2, 3).reshape(1, 12, H, W)
    s2d_ref = O.space_to_depth(cat, 2)[0].permute(1, 2, 0)
    ov_ref = torch.mean(refp[:, 0:2], dim=1)
    fr = torch.randn(3, H, W, generator=g) * 0.8
    u8_ref = O.frame_to_u8(fr.numpy()[:, :h, :w])

    def body(al):
        st = _stream()
        dev = [al.fill(al.flat(1, (h, w, 3), torch.uint8, name='frame %d' % i), f[None]) for i, f in enumerate(frames)]
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in dev])
        x = al.flat(1, (3, 4, H, W), F32, name='x')
        GA.launch(al, lambda: lib.demfi_u8_to_window(ptrs, h, w, x.data_ptr(), H, W, st), [x], 'u8_to_window')
        assert torch.equal(x[0].cpu(), refp)
        for dtype, dt in ((F16, L.F16), (F32, L.F32)):
            x2 = al.flat(1, (3, 4, H, W), F32, name='x (ingest)')
            s2d2 = al.flat(1, (H // 2, W // 2, 48), dtype, name='s2d (ingest)')
            ov2 = al.flat(1, (3, H, W), F32, name='overlay (ingest)')
            GA.launch(al, lambda: lib.demfi_u8_ingest(ptrs, h, w, x2.data_ptr(), s2d2.data_ptr(), ov2.data_ptr(), dt, H, W, st),
                      [x2, s2d2, ov2], 'u8_ingest')
            s2d1 = al.flat(1, (H // 2, W // 2, 48), dtype, name='s2d')
            GA.launch(al, lambda: lib.demfi_space_to_depth(x.data_ptr(), s2d1.data_ptr(), dt, H, W, st), [s2d1], 'space_to_depth')
            ov1 = al.flat(1, (3, H, W), F32, name='overlay')
            GA.launch(al, lambda: lib.demfi_overlay_mean(x.data_ptr(), ov1.data_ptr(), H, W, st), [ov1], 'overlay_mean')
            assert torch.equal(x2[0].cpu(), refp)
            assert torch.equal(s2d1[0].cpu().float(), s2d_ref.to(dtype).float()) and torch.equal(s2d2[0].cpu(), s2d1[0].cpu())
            assert torch.equal(ov1[0].cpu(), ov_ref) and torch.equal(ov2[0].cpu(), ov_ref)
        planar = al.flat(1, (3, h, w), F32, name='planar')
        GA.launch(al, lambda: lib.demfi_u8_to_planar(dev[2].data_ptr(), h, w, planar.data_ptr(), st), [planar], 'u8_to_planar')
        assert torch.equal(planar[0].cpu(), O.frames_u8_to_tensor([frames[2].numpy()])[:, 0])
        xs = al.fill(al.flat(1, (12, h, w), F32, name='unpadded'), ref.reshape(1, 12, h, w))
        xp = al.flat(1, (12, H, W), F32, name='padded')
        GA.launch(al, lambda: lib.demfi_reflect_pad(xs.data_ptr(), xp.data_ptr(), 12, h, w, H, W, st), [xp], 'reflect_pad')
        assert torch.equal(xp[0].cpu(), F.pad(ref.reshape(1, 12, h, w), [0, W - w, 0, H - h], mode='reflect')[0])
        frd = al.fill(al.flat(1, (3, H, W), F32, name='frame f32'), fr[None])
        u8 = al.flat(1, (h, w, 3), torch.uint8, name='frame u8')
        GA.launch(al, lambda: lib.demfi_frame_to_u8(frd.data_ptr(), u8.data_ptr(), h, w, H, W, st), [u8], 'frame_to_u8')
        assert np.array_equal(u8[0].cpu().numpy(), u8_ref)

    _both(body)


def test_frame_io_refuses_a_padding_of_the_frame_size():
    """(h, w, H, W) = (16, 32, 32, 64): one step past the largest legal padding the reflected index would be -1."""
    lib = L.load()
    h, w, H, W = 16, 32, 32, 64
    al = GA.Arena(DEV, 8 << 20)
    dev = [al.fill(al.flat(1, (h, w, 3), torch.uint8), torch.zeros(1, h, w, 3, dtype=torch.uint8)) for _ in range(4)]
    ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in dev])
    x, s2d, ov = al.flat(1, (3, 4, H, W), F32), al.flat(1, (H // 2, W // 2, 48), F16), al.flat(1, (3, H, W), F32)
    xs = al.fill(al.flat(1, (12, h, w), F32), torch.zeros(1, 12, h, w))
    _refused(al, lambda: lib.demfi_u8_to_window(ptrs, h, w, x.data_ptr(), H, W, _stream()))
    _refused(al, lambda: lib.demfi_u8_ingest(ptrs, h, w, x.data_ptr(), s2d.data_ptr(), ov.data_ptr(), L.F16, H, W, _stream()))
    _refused(al, lambda: lib.demfi_reflect_pad(xs.data_ptr(), x.data_ptr(), 12, h, w, H, W, _stream()))


# ------------------------------------------------------------------------------------------------------------------------------
# viz: demfi_absmean_map, demfi_one_minus, demfi_minmax_normalize
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_b', [False, True], ids=['abs_a', 'abs_a_minus_b'])
@pytest.mark.parametrize('dtype,Cc', [(F16, 8), (F16, 64), (F32, 8), (F32, 64)])
def test_absmean_map(dtype, Cc, with_b):
    """fp64 mean of |a - b| over the channels; the kernel rounds the difference, C - 1 sums and the division in fp32 (C + 1 roundings of
    partial sums that never exceed the sum of the terms): within (C + 2) * 2^-24 * mean|terms|."""
    lib = L.load()
    H, W = 13, 19
    rng = np.random.default_rng(Cc + with_b)
    a = torch.from_numpy(rng.standard_normal((1, H, W, Cc)).astype(f32)).to(dtype)
    b = torch.from_numpy(rng.standard_normal((1, H, W, Cc)).astype(f32)).to(dtype)
    ref = ((a.double() - b.double()) if with_b else a.double()).abs().mean(-1)[0].numpy()
    tol = (Cc + 2) * 2.0 ** -24 * ref

    def body(al):
        da = al.fill(al.fat(1, H, W, Cc, dtype, name='a'), a)[0]
        db = al.fill(al.fat(1, H, W, Cc, dtype, name='b'), b)[0] if with_b else None      # (a view holds a pointer, not the tensor)
        va, vb = FW._nhwc(da), FW._nhwc(db) if with_b else None
        out = al.flat(1, (H, W), F32, name='absmean')
        GA.launch(al, lambda: lib.demfi_absmean_map(C.byref(va), C.byref(vb) if with_b else None, out.data_ptr(), Cc, H, W, _stream()),
                  [out], 'absmean')
        err = np.abs(out[0].double().cpu().numpy() - ref)
        assert (err <= tol).all(), float((err / tol).max())

    _both(body)


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65537])                  # 65537: the 256-part cap makes minmax_part_kernel stride
def test_one_minus_and_minmax_normalize_bit_equal_numpy(n):
    """fl(1 - x), and fl(fl(x - min) / fl(max - min)) as numpy float32 computes them (IEEE, correctly rounded), bit for bit.  n = 1:
    max - min = 0, so only one_minus runs there."""
    lib = L.load()
    x = np.random.default_rng(n).standard_normal(n).astype(f32)
    mn = x.min()
    with np.errstate(invalid='ignore', divide='ignore'):
        norm = ((x - mn).astype(f32) / f32(x.max() - mn)).astype(f32)
    nscr = lib.demfi_minmax_scratch_floats()

    def body(al):
        src = al.fill(al.flat(1, (n,), F32, name='in'), x[None])
        out = al.flat(1, (n,), F32, name='1 - in')
        GA.launch(al, lambda: lib.demfi_one_minus(src.data_ptr(), out.data_ptr(), n, _stream()), [out], 'one_minus')
        assert np.array_equal(out[0].cpu().numpy().view(np.int32), (f32(1) - x).astype(f32).view(np.int32))
        if n == 1:
            return
        plane = al.fill(al.flat(1, (n,), F32, name='plane'), x[None])
        scratch = al.flat(1, (nscr,), F32, name='min-max scratch')            # exactly demfi_minmax_scratch_floats() floats
        GA.launch(al, lambda: lib.demfi_minmax_normalize(plane.data_ptr(), n, scratch.data_ptr(), _stream()), [plane, scratch],
                  'minmax_normalize', finite=[plane])
        assert np.array_equal(plane[0].cpu().numpy().view(np.int32), norm.view(np.int32))
        assert float(plane.min()) == 0.0 and float(plane.max()) == 1.0

    _both(body)


# ------------------------------------------------------------------------------------------------------------------------------
# demfi_eval_frame
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_rounds_half_to_even_at_0():
    """pred = 0.0 is 127.5 on the [0, 255] scale, which np.around takes to the even 128 (and 126.5 to 126)."""
    assert O.denorm255(np.float64(0.0)) == 127.5 and np.around(O.denorm255(np.float64(0.0))) == 128.0
    assert np.around(126.5) == 126.0


@pytest.mark.parametrize('round_gt', [0, 1])
@pytest.mark.parametrize('h,w', [(11, 11), (11, 43), (27, 11), (21, 37), (17, 33), (40, 72)])   # tiles are 16x32 with a halo of 5
def test_eval_frame(h, w, round_gt):
    """11x11: one valid SSIM pixel; 21x37: the valid rows end exactly at the first tile edge.  pred / gt are pitched planes; values in
    [-1.3, 1.3] exercise both clamps; 5 % of pred is exactly 0.0 (127.5: round half to even)."""
    lib = L.load()
    rng = np.random.default_rng(h * 100 + w)
    pred = rng.uniform(-1.3, 1.3, (3, h, w)).astype(f32)
    pred[rng.random((3, h, w)) < 0.05] = 0.0
    gt = rng.uniform(-1.3, 1.3, (3, h, w)).astype(f32)
    po, so = O.eval_frame(pred, gt, round_gt=bool(round_gt))
    a = np.around(O.denorm255(pred.astype(np.float64)))
    b = O.denorm255(gt.astype(np.float64))
    mse = float(np.mean(((np.around(b) if round_gt else b) - a) ** 2))
    nws = lib.demfi_eval_workspace_bytes(h, w)
    assert nws % 8 == 0 and nws > 0

    def body(al):
        dp, dg = al.fill(al.thin(3, h, w, name='pred'), pred), al.fill(al.thin(3, h, w, name='gt'), gt)
        outs = []
        for _ in range(2):
            ws = al.flat(1, (nws // 8,), torch.float64, name='eval workspace')       # exactly demfi_eval_workspace_bytes
            out3 = al.flat(1, (3,), torch.float64, name='out3')
            GA.launch(al, lambda: lib.demfi_eval_frame(dp.data_ptr(), dp.stride(1), dp.stride(0), dg.data_ptr(), dg.stride(1), dg.stride(0),
                                                       h, w, round_gt, ws.data_ptr(), out3.data_ptr(), _stream()), [ws, out3], 'eval_frame')
            outs.append(out3[0].cpu())
        p, s, m = (float(v) for v in outs[0])
        assert abs(p - po) < 1e-9 and abs(s - so) < 1e-9 and abs(m - mse) < 1e-9, (p, po, s, so, m, mse)
        assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))    # run to run: the same bytes

    _both(body)


def test_eval_frame_refuses_10x11():
    lib = L.load()
    al = GA.Arena(DEV, 1 << 20)
    dp = al.fill(al.thin(3, 10, 11), torch.zeros(3, 10, 11))
    ws, out3 = al.flat(1, (6,), torch.float64), al.flat(1, (3,), torch.float64)
    _refused(al, lambda: lib.demfi_eval_frame(dp.data_ptr(), dp.stride(1), dp.stride(0), dp.data_ptr(), dp.stride(1), dp.stride(0), 10, 11, 0,
                                              ws.data_ptr(), out3.data_ptr(), _stream()))
    _refused(al, lambda: lib.demfi_eval_frame(dp.data_ptr(), dp.stride(1), dp.stride(0), dp.data_ptr(), dp.stride(1), dp.stride(0), 11, 10, 0,
                                              ws.data_ptr(), out3.data_ptr(), _stream()))
