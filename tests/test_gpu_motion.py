"""The motion kernels as the batched per-t plan runs them -- CFR splat (near and far paths), fat / thin backward warp + Eq.(2)
blend, FGAC gather + gate blend, plane packs -- against the float64 references of tests/motion_ref.py, per element.

Shapes are the product's: padded 720p / 1080p frames (736x1280, 1088x1920; warps checked on a row subset there), ragged frames,
n_ctx = 7 contexts per launch with window-level (stride 0) and per-context inputs, and the t values of the --fps retime
schedules (23.976 -> 60 fps gives t = 1/1001 ... 1000/1001).  Every output buffer starts as NaN, so an element a kernel leaves
unwritten fails.  Tolerances (motion_ref.check): fp32 outputs within a few fp32 ulps of the per-element bound, fp16 outputs
within one fp16 ulp of the float64 value plus that bound; CFR targets that receive no source must be exactly 0."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from demfi_amd import retime                         # noqa: E402
from tests import motion_ref as R                    # noqa: E402

DEV = 'cuda:0'
f32 = np.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync_check(st, what):
    L.check(st, what)
    torch.cuda.synchronize()


def _schedule():
    """Seven distinct t of the retime schedules: 23.976 -> 60 fps (t = k/1001) and 24 -> 60 fps (t = 0.2, 0.4, 0.6, 0.8)."""
    r = retime.ratio(Fraction(24000, 1001), 60)
    ts = sorted({t for k in range(400) for t in retime.instants(k, r)})
    lo, hi = retime.float32_of(Fraction(1, 1001)), retime.float32_of(Fraction(1000, 1001))
    assert ts[0] == lo and ts[-1] == hi
    five = sorted({t for k in range(2) for t in retime.instants(k, retime.ratio(24, 60))})
    assert five == [retime.float32_of(Fraction(j, 5)) for j in (1, 2, 3, 4)]
    return [lo] + five[:2] + [0.5] + five[2:] + [hi]


T7 = _schedule()


def _rows(H, rng, n=24):
    """The first and last 4 rows, both sides of ~8 warp-tile edges (4-row tiles) and n random rows."""
    edges = rng.integers(1, H // 4, 8) * 4
    return np.unique(np.concatenate([np.arange(4), np.arange(H - 4, H), edges - 1, edges, rng.integers(0, H, n)]))


def _tdev(ts):
    return torch.tensor([float(f32(t)) for t in ts], device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# CFR
# ------------------------------------------------------------------------------------------------------------------------------
def _cfr_flow(kind, H, W, rng):
    """[2,H,W] fp32 flow (channel 0: column displacement, 1: row displacement) of one family."""
    f = (rng.standard_normal((2, H, W)) * 2.5).astype(f32)
    if kind == 'global':                      # whole-frame motion of 40-300 px, with a small local field on top
        f += np.array([rng.uniform(40, 300) * rng.choice([-1, 1]), rng.uniform(40, 120) * rng.choice([-1, 1])], f32)[:, None, None]
    elif kind == 'spikes':                    # sparse far sources on a near field
        m = rng.random((H, W)) < 0.02
        f[:, m] = (rng.uniform(40, 300, (2, int(m.sum()))) * rng.choice([-1, 1], (2, int(m.sum())))).astype(f32)
    elif kind == 'threshold':                 # with t = 0.5: floor(t f) in {-33, -32, 31, 32} exactly (0.5 f is exact)
        k = rng.choice([-33, -32, 31, 32], (2, H, W))
        frac = rng.choice([0.0, 0.25, 0.5, 0.999], (2, H, W))
        f = (2 * (k + frac)).astype(f32)
        m = rng.random((H, W)) < 0.3          # some sources stay near, so both paths meet on the same tiles
        f[:, m] = (rng.standard_normal((2, int(m.sum()))) * 2).astype(f32)
    elif kind == 'edges':                     # with t = 0.5: integer targets on tile edges (rows 0 / 15 mod 16, columns 0 / 63 mod 64)
        y, x = np.mgrid[0:H, 0:W]
        ty = (y // 16) * 16 + rng.choice([0, 15, 16, 31], (H, W))
        tx = (x // 64) * 64 + rng.choice([0, 63, 64, 127], (H, W))
        f = np.stack([2.0 * (tx - x), 2.0 * (ty - y)]).astype(f32)
    elif kind == 'collide':                   # with t = 0.5: blocks of 8x32 sources all land on a 2x2 patch (many-to-one)
        y, x = np.mgrid[0:H, 0:W]
        f = np.stack([2.0 * ((x // 32) * 32 + 7.5 - x), 2.0 * ((y // 8) * 8 + 3.25 - y)]).astype(f32)
    return np.ascontiguousarray(f)


def _cfr_check(out, f01, f10, t, what):
    r = R.cfr(f01, f10, t)
    got = out.cpu().numpy()
    R.check(got, r['ft'], r['bound'], 16, what, exact_zero=np.broadcast_to(~r['hit'], got.shape))
    return r


# (H, W, nb, per-context flows, flow families per context, pack dtype of the _pack entry point or None)
CFR_CASES = [
    (736, 1280, 7, False, ['global'], torch.float16),
    (1088, 1920, 7, False, ['spikes'], None),
    (736, 1280, 2, True, ['threshold', 'spikes'], None),
    (1088, 1920, 2, True, ['edges', 'global'], torch.float32),
    (100, 130, 7, True, ['threshold', 'edges', 'collide', 'spikes', 'global', 'threshold', 'collide'], torch.float32),
    (100, 130, 2, False, ['threshold'], torch.float16),
]


@pytest.mark.parametrize('H,W,nb,per_ctx,kinds,pack', CFR_CASES)
def test_cfr_batched_matches_fp64_and_single_launches(H, W, nb, per_ctx, kinds, pack):
    lib = L.load()
    rng = np.random.default_rng(H * 7 + W + nb)
    # families made for t = 0.5 put it first; the others take the retime schedule
    ts = ([0.5] if kinds[0] in ('threshold', 'edges', 'collide') else []) + [t for t in T7 if t != 0.5]
    ts = ts[:nb] if nb < 7 else T7
    nf = nb if per_ctx else 1
    f01 = np.stack([_cfr_flow(kinds[q % len(kinds)], H, W, rng) for q in range(nf)])
    f10 = np.stack([_cfr_flow(kinds[q % len(kinds)], H, W, rng) for q in range(nf)])
    d01, d10 = torch.from_numpy(f01).to(DEV), torch.from_numpy(f10).to(DEV)
    t = _tdev(ts)
    hw = H * W
    nacc = lib.demfi_cfr_workspace_bytes(H, W) // 8
    fstride = 2 * hw * 4 if per_ctx else 0
    bt = L.Batch()
    bt.nb, bt.t = nb, 4
    bt.p[0] = bt.p[1] = fstride
    bt.p[2], bt.p[3] = nacc * 8, 4 * hw * 4
    logit = rec = None
    if pack is not None:
        logit = torch.from_numpy(rng.standard_normal((nb, H, W)).astype(f32)).to(DEV)
        rec = torch.full((nb, H, W, 16), float('nan'), dtype=pack, device=DEV)
        bt.p[4], bt.p[5] = hw * 4, hw * 16 * rec.element_size()

    def run():
        acc = torch.zeros(nb, nacc, dtype=torch.int64, device=DEV)
        out = torch.full((nb, 4, H, W), float('nan'), device=DEV)
        if pack is None:
            st = lib.demfi_cfr_flow_align_batched(d01.data_ptr(), d10.data_ptr(), t.data_ptr(), H, W, acc.data_ptr(), out.data_ptr(),
                                                  C.byref(bt), _stream())
        else:
            st = lib.demfi_cfr_flow_align_pack(d01.data_ptr(), d10.data_ptr(), logit.data_ptr(), t.data_ptr(), H, W, acc.data_ptr(),
                                               out.data_ptr(), rec.data_ptr(), L.F32 if pack == torch.float32 else L.F16, C.byref(bt),
                                               _stream())
        _sync_check(st, 'cfr batched')
        # the whole workspace of every context -- six int64 planes and the tile flags -- is left all-zero, far path included
        assert int(torch.count_nonzero(acc)) == 0
        return out

    out = run()
    assert torch.equal(out, run())                                             # run to run: the same bytes
    nfar = 0
    for q in range(nb):
        g01, g10 = d01[q if per_ctx else 0], d10[q if per_ctx else 0]
        acc1 = torch.zeros(nacc, dtype=torch.int64, device=DEV)
        out1 = torch.full((4, H, W), float('nan'), device=DEV)
        _sync_check(lib.demfi_cfr_flow_align(g01.data_ptr(), g10.data_ptr(), t[q:q + 1].data_ptr(), H, W, acc1.data_ptr(), out1.data_ptr(),
                                             None, _stream()), 'cfr single')
        assert torch.equal(out[q], out1), q                                     # batched == one launch per context
        assert int(torch.count_nonzero(acc1)) == 0
        a01, a10 = f01[q if per_ctx else 0], f10[q if per_ctx else 0]
        _cfr_check(out[q], a01, a10, ts[q], 'cfr %dx%d ctx %d t=%.6g' % (H, W, q, ts[q]))
        for fl, s in ((a01, f32(ts[q])), (a10, f32(1) - f32(ts[q]))):
            y1 = np.floor((fl * s).astype(f32))
            nfar += int(((y1 < -32) | (y1 > 31)).any(0).sum())
        if pack is not None:
            planes = torch.cat([out[q], g01, g10, logit[q][None]], 0)
            assert torch.equal(rec[q][..., :9], planes.permute(1, 2, 0).to(pack))
            assert int(torch.count_nonzero(rec[q][..., 9:])) == 0
    assert nfar > 0                                                             # the far path ran in every case


def test_cfr_far_threshold_single_launch():
    """floor(t f) = -33 / -32 / 31 / 32 exactly at t = 0.5, on a ragged frame: the far / near split and the flagged-tile finish."""
    lib = L.load()
    rng = np.random.default_rng(3)
    H, W = 93, 141
    f01, f10 = _cfr_flow('threshold', H, W, rng), _cfr_flow('threshold', H, W, rng)
    acc = torch.zeros(lib.demfi_cfr_workspace_bytes(H, W) // 8, dtype=torch.int64, device=DEV)
    out = torch.full((4, H, W), float('nan'), device=DEV)
    t = _tdev([0.5])
    d01, d10 = torch.from_numpy(f01).to(DEV), torch.from_numpy(f10).to(DEV)
    _sync_check(lib.demfi_cfr_flow_align(d01.data_ptr(), d10.data_ptr(), t.data_ptr(), H, W, acc.data_ptr(), out.data_ptr(), None,
                                         _stream()), 'cfr')
    assert int(torch.count_nonzero(acc)) == 0
    r = _cfr_check(out, f01, f10, 0.5, 'cfr threshold')
    assert (~r['hit']).any() and r['hit'].any()


# ------------------------------------------------------------------------------------------------------------------------------
# Backward warp + Eq.(2) blend
# ------------------------------------------------------------------------------------------------------------------------------
def _warp_flow(H, W, rng):
    """[2,H,W] fp32 flows: sub-pixel, integer-exact, partly out of frame at the s < 0.999 validity edge, entirely out of frame."""
    f = (rng.standard_normal((2, H, W)) * 4).astype(f32)
    band = np.arange(H) % 4
    f[:, band == 1] = np.round(f[:, band == 1])
    y, x = np.mgrid[0:H, 0:W]
    edge = band == 2                                                            # sample at x = -d or W - 1 + d, d around 1e-3
    d = rng.choice([0.0, 5e-4, 9.9e-4, 1.2e-3, 0.3, 1.0], (H, W))
    left = rng.random((H, W)) < 0.5
    f[0][edge] = np.where(left, -x - d, W - 1 + d - x)[edge]
    f[1][edge] = rng.uniform(-1, 1, (H, W))[edge]
    out = (band == 3)[:, None] & (rng.random((H, W)) < 0.5)
    f[0][out] = f32(2.0 * W + 7)
    return np.ascontiguousarray(f.astype(f32))


def _logit(H, W, rng):
    lg = (rng.standard_normal((H, W)) * 3).astype(f32)
    m = rng.random((H, W))
    lg[m < 0.2] = rng.choice([-90.0, -30.0, 30.0, 90.0], int((m < 0.2).sum()))
    return np.ascontiguousarray(lg)


class _WarpSet:
    """Inputs of nb contexts on the GPU.  ab_ctx: A / B have a copy per context (else one window-level copy, stride 0)."""

    def __init__(self, H, W, Cc, dtype, nb, ab_ctx, seed, planar=False):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.C, self.dtype, self.nb, self.planar = H, W, Cc, dtype, nb, planar
        na = nb if ab_ctx else 1
        shape = (na, Cc, H, W) if planar else (na, H, W, Cc)
        self.A = torch.from_numpy(np.tanh(rng.standard_normal(shape)).astype(f32)).to(DEV).to(dtype)
        self.B = torch.from_numpy(np.tanh(rng.standard_normal(shape)).astype(f32)).to(DEV).to(dtype)
        self.fa = np.stack([_warp_flow(H, W, rng) for _ in range(nb)])
        self.fb = np.stack([_warp_flow(H, W, rng) for _ in range(nb)])
        self.lg = np.stack([_logit(H, W, rng) for _ in range(nb)])
        self.dfa, self.dfb, self.dlg = (torch.from_numpy(a).to(DEV) for a in (self.fa, self.fb, self.lg))
        self.ts = [T7[(q * 3 + seed) % 7] for q in range(nb)]
        self.t = _tdev(self.ts)
        self.esz = self.A.element_size()
        self.ab_stride = H * W * Cc * self.esz if ab_ctx else 0

    def view(self, t, q=0):
        H, W, Cc = self.H, self.W, self.C
        f = 1 if t.dtype == torch.float32 else 0
        if self.planar:
            return L.View(t[q].data_ptr(), 1, W, H * W, 0, f, 0)
        return L.View(t[q].data_ptr(), Cc, W * Cc, 1, 0, f, 0)

    def new_out(self, nb):
        shape = (nb, self.C, self.H, self.W) if self.planar else (nb, self.H, self.W, self.C)
        return torch.full(shape, float('nan'), dtype=self.dtype, device=DEV)

    def single(self, q, lib):
        out = self.new_out(1)
        occ = torch.full((self.H, self.W), float('nan'), device=DEV)
        qa = q if self.ab_stride else 0
        va, vb, vo = self.view(self.A, qa), self.view(self.B, qa), self.view(out)
        _sync_check(lib.demfi_warp_blend(C.byref(va), self.dfa[q].data_ptr(), C.byref(vb), self.dfb[q].data_ptr(), self.dlg[q].data_ptr(),
                                         self.t[q:q + 1].data_ptr(), C.byref(vo), self.C, self.H, self.W, occ.data_ptr(), None, _stream()),
                    'warp single')
        return out[0], occ

    def batched(self, lib, outer, pack=None):
        H, W = self.H, self.W
        out = self.new_out(self.nb)
        occ = torch.full((self.nb, H, W), float('nan'), device=DEV)
        bt = L.Batch()
        bt.nb, bt._pad = self.nb, outer
        bt.a = bt.b = self.ab_stride
        bt.o = out[0].numel() * self.esz
        bt.t = 4
        bt.p[0] = bt.p[1] = 2 * H * W * 4
        bt.p[2] = bt.p[3] = H * W * 4
        rec, pdt = None, 0
        if pack is not None:
            rec = torch.full((self.nb, H, W, 8), float('nan'), dtype=pack, device=DEV)
            bt.p[4] = H * W * 8 * rec.element_size()
            pdt = L.F32 if pack == torch.float32 else L.F16
        va, vb, vo = self.view(self.A), self.view(self.B), self.view(out)
        _sync_check(lib.demfi_warp_blend_batched(C.byref(va), self.dfa.data_ptr(), C.byref(vb), self.dfb.data_ptr(), self.dlg.data_ptr(),
                                                 self.t.data_ptr(), C.byref(vo), self.C, H, W, occ.data_ptr(),
                                                 rec.data_ptr() if rec is not None else None, pdt, C.byref(bt), _stream()),
                    'warp batched')
        return out, occ, rec

    def check(self, q, out, occ, rows=None):
        """out: [H,W,C] (or planar [C,H,W]) of context q; rows: the checked subset (None: all)."""
        qa = q if self.ab_stride else 0
        A, B = self.A[qa], self.B[qa]
        if self.planar:
            A, B, out = A.permute(1, 2, 0), B.permute(1, 2, 0), out.permute(1, 2, 0)
        rr = np.arange(self.H) if rows is None else rows
        ri = torch.from_numpy(rr).to(DEV)
        r = R.warp_blend(A.cpu().numpy(), self.fa[q], B.cpu().numpy(), self.fb[q], self.lg[q], self.ts[q], rr)
        f16 = self.dtype == torch.float16
        what = 'warp %s C=%d %dx%d ctx %d t=%.6g' % ('fp16' if f16 else 'fp32', self.C, self.H, self.W, q, self.ts[q])
        R.check(out.index_select(0, ri).float().cpu().numpy(), r['out'], r['bound'], 16, what, ulp16=f16)
        R.check(occ.index_select(0, ri).cpu().numpy(), r['occ'], r['occ'] + 2.0 ** -100, 4, what + ' occ')


FAT = [(torch.float16, c) for c in (8, 16, 32, 64, 128, 512)] + [(torch.float32, c) for c in (4, 16, 64, 256)]


@pytest.mark.parametrize('dtype,Cc', FAT)
@pytest.mark.parametrize('ab_ctx', [False, True])
def test_fat_warp_all_lane_counts_single_inner_outer(dtype, Cc, ab_ctx):
    """Ragged frame (H % 4 != 0, W % 64 != 0), lpp = 1 ... 64 lanes per pixel: nb single launches, one batched launch with the
    contexts innermost (_pad = 0) and one with a grid slice per context (_pad = 1) give the same bytes, and match fp64."""
    lib = L.load()
    ws = _WarpSet(37, 130, Cc, dtype, 3, ab_ctx, seed=Cc + 1000 * ab_ctx)
    singles = [ws.single(q, lib) for q in range(3)]
    for outer in (0, 1):
        out, occ, _ = ws.batched(lib, outer)
        for q in range(3):
            assert torch.equal(out[q], singles[q][0]) and torch.equal(occ[q], singles[q][1]), (outer, q)
    for q in range(3):
        ws.check(q, *singles[q])


@pytest.mark.parametrize('H,W,dtype,nb,outer', [(1088, 1920, torch.float16, 7, 1), (736, 1280, torch.float16, 7, 0),
                                                (736, 1280, torch.float32, 2, 1)])
def test_fat_warp_full_frame_rows(H, W, dtype, nb, outer):
    """The plan's shape: C = 64, window-level A / B (stride 0), n_ctx contexts in one launch; checked on a row subset."""
    lib = L.load()
    ws = _WarpSet(H, W, 64, dtype, nb, False, seed=H + nb)
    out, occ, _ = ws.batched(lib, outer)
    rows = _rows(H, np.random.default_rng(H))
    for q in range(nb):
        ws.check(q, out[q], occ[q], rows)
    o1, c1 = ws.single(nb - 1, lib)
    assert torch.equal(out[nb - 1], o1) and torch.equal(occ[nb - 1], c1)


@pytest.mark.parametrize('dtype,Cc', [(torch.float16, 1024), (torch.float16, 2048), (torch.float32, 512)])
def test_fat_warp_refuses_pixels_wider_than_64_lanes(dtype, Cc):
    """A pixel of more than 1 KiB cannot be walked by phase 2 (64 >> lpp_shift pixels per iteration would be 0): DEMFI_ERR_ARG,
    and the output is left untouched."""
    lib = L.load()
    ws = _WarpSet(8, 16, Cc, dtype, 2, False, seed=5)
    out = ws.new_out(2)
    va, vb, vo = ws.view(ws.A), ws.view(ws.B), ws.view(out)
    st = lib.demfi_warp_blend(C.byref(va), ws.dfa.data_ptr(), C.byref(vb), ws.dfb.data_ptr(), ws.dlg.data_ptr(), ws.t.data_ptr(),
                              C.byref(vo), Cc, 8, 16, None, None, _stream())
    assert st == -1 and b'64' in lib.demfi_last_error()
    bt = L.Batch()
    bt.nb, bt.o, bt.t = 2, out[0].numel() * ws.esz, 4
    bt.p[0] = bt.p[1] = 2 * 8 * 16 * 4
    bt.p[2] = 8 * 16 * 4
    for outer in (0, 1):
        bt._pad = outer
        assert lib.demfi_warp_blend_batched(C.byref(va), ws.dfa.data_ptr(), C.byref(vb), ws.dfb.data_ptr(), ws.dlg.data_ptr(),
                                            ws.t.data_ptr(), C.byref(vo), Cc, 8, 16, None, None, 0, C.byref(bt), _stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())


@pytest.mark.parametrize('dtype,Cc', [(torch.float16, 12), (torch.float32, 3)])
def test_nhwc_views_that_are_not_16_byte_records_take_the_thin_kernel(dtype, Cc):
    lib = L.load()
    ws = _WarpSet(37, 130, Cc, dtype, 3, True, seed=Cc)
    out, occ, _ = ws.batched(lib, 0)
    for q in range(3):
        o1, c1 = ws.single(q, lib)
        assert torch.equal(out[q], o1) and torch.equal(occ[q], c1)
        ws.check(q, out[q], occ[q])


@pytest.mark.parametrize('H,W,pack,ab_ctx', [(100, 130, torch.float16, True), (100, 130, torch.float32, False),
                                             (736, 1280, torch.float16, False)])
def test_thin_warp_pack_batched_seven_contexts(H, W, pack, ab_ctx):
    """Planar fp32 3-channel frames, nb = 7 in one launch with the packed record [out | fa | fb | sigmoid(logit)]: values against
    fp64, the record equal to the planes rounded to the pack dtype, each context equal to its own demfi_warp_blend_pack launch."""
    lib = L.load()
    ws = _WarpSet(H, W, 3, torch.float32, 7, ab_ctx, seed=H, planar=True)
    out, occ, rec = ws.batched(lib, 0, pack)
    rows = None if H < 200 else _rows(H, np.random.default_rng(1))
    pdt = L.F32 if pack == torch.float32 else L.F16
    for q in range(7):
        ws.check(q, out[q], occ[q], rows)
        planes = torch.cat([out[q], ws.dfa[q], ws.dfb[q], occ[q][None]], 0)
        assert torch.equal(rec[q], planes.permute(1, 2, 0).to(pack)), q
        qa = q if ab_ctx else 0
        o1 = ws.new_out(1)
        c1 = torch.full((H, W), float('nan'), device=DEV)
        r1 = torch.full((H, W, 8), float('nan'), dtype=pack, device=DEV)
        va, vb, vo = ws.view(ws.A, qa), ws.view(ws.B, qa), ws.view(o1)
        _sync_check(lib.demfi_warp_blend_pack(C.byref(va), ws.dfa[q].data_ptr(), C.byref(vb), ws.dfb[q].data_ptr(), ws.dlg[q].data_ptr(),
                                              ws.t[q:q + 1].data_ptr(), C.byref(vo), H, W, c1.data_ptr(), r1.data_ptr(), pdt, _stream()),
                    'warp pack')
        assert torch.equal(o1[0], out[q]) and torch.equal(c1, occ[q]) and torch.equal(r1, rec[q]), q


# ------------------------------------------------------------------------------------------------------------------------------
# FGAC gather + gate blend
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_fgac_gather_and_gate_blend_full_width(dtype):
    lib = L.load()
    rng = np.random.default_rng(9)
    H, W, Cc = 24, 1920, 64
    S = torch.from_numpy(np.tanh(rng.standard_normal((H, W, Cc))).astype(f32)).to(DEV).to(dtype)
    fl = np.stack([rng.uniform(0, W - 1, (H, W)), rng.uniform(0, H - 1, (H, W))]).astype(f32)
    fl[:, 1::4] = np.round(fl[:, 1::4])                                         # integer-exact
    fl[0, 2::4] = rng.choice([W - 1, W - 0.75, W - 1 + 1e-3, W + 3.0, -0.5, -2.0], (len(range(2, H, 4)), W))  # beyond the last column
    fl[1, 3::4] = rng.choice([H - 1, H - 0.5, H + 2.0, -0.25], (len(range(3, H, 4)), W))                      # ... and the last row
    fl = np.ascontiguousarray(fl.astype(f32))
    dfl = torch.from_numpy(fl).to(DEV)
    out = torch.full((H, W, Cc), float('nan'), dtype=dtype, device=DEV)
    f = 1 if dtype == torch.float32 else 0
    nv = lambda t: L.View(t.data_ptr(), Cc, W * Cc, 1, 0, f, 0)
    vs, vo = nv(S), nv(out)
    _sync_check(lib.demfi_fgac_gather(C.byref(vs), dfl.data_ptr(), C.byref(vo), Cc, H, W, None, _stream()), 'fgac gather')
    f16 = dtype == torch.float16
    v, a = R.fgac_gather(S.cpu().numpy(), fl)
    R.check(out.float().cpu().numpy(), v, a, 8, 'fgac gather', ulp16=f16)
    w = rng.random((H, W)).astype(f32)
    w[:, :3] = [0.0, 1.0, 0.5]
    E = torch.from_numpy(rng.standard_normal((H, W, Cc)).astype(f32)).to(DEV).to(dtype)
    o2 = torch.full((H, W, Cc), float('nan'), dtype=dtype, device=DEV)
    dw = torch.from_numpy(w).to(DEV)
    ve, v2 = nv(E), nv(o2)
    _sync_check(lib.demfi_gate_blend(dw.data_ptr(), C.byref(vo), C.byref(ve), C.byref(v2), Cc, H, W, _stream()), 'gate blend')
    g, ga = R.gate_blend(w, out.cpu().numpy(), E.cpu().numpy())
    R.check(o2.float().cpu().numpy(), g, ga, 8, 'gate blend', ulp16=f16)


# ------------------------------------------------------------------------------------------------------------------------------
# Plane packs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nch', [8, 16, 24, 32])
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_pack_planes_batched(nch, dtype):
    """nb = 3 contexts, planes with a per-context copy or window-level (stride 0), NULL planes (zeros), a destination record wider
    than nch (the channels past nch stay untouched); fp16 rounding equal to torch's .half()."""
    lib = L.load()
    rng = np.random.default_rng(nch)
    H, W, nb = 37, 130, 3
    hw = H * W
    sx = nch + 8
    planes = torch.from_numpy((rng.standard_normal((nch, nb, H, W)) * 100).astype(f32)).to(DEV)
    null = rng.random(nch) < 0.25
    per_ctx = rng.random(nch) < 0.5
    dst = torch.full((nb, H, W, sx), float('nan'), dtype=dtype, device=DEV)
    ptrs = (C.c_void_p * nch)(*[None if null[i] else planes[i].data_ptr() for i in range(nch)])
    bt = L.Batch()
    bt.nb, bt.o = nb, hw * sx * dst.element_size()
    for i in range(nch):
        bt.p[i] = hw * 4 if per_ctx[i] else 0
    dt = L.F32 if dtype == torch.float32 else L.F16
    _sync_check(lib.demfi_pack_planes_batched(ptrs, nch, dst.data_ptr(), dt, sx, H, W, C.byref(bt), _stream()), 'pack batched')
    for q in range(nb):
        for i in range(nch):
            exp = torch.zeros(H, W, device=DEV) if null[i] else planes[i, q if per_ctx[i] else 0]
            assert torch.equal(dst[q, ..., i], exp.to(dtype)), (q, i)
    assert bool(torch.isnan(dst[..., nch:].float()).all())
