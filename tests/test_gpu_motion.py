"""The motion kernels as the batched per-t plan runs them -- CFR splat (near and far paths), fat / thin backward warp + Eq.(2)
blend, FGAC gather + gate blend, plane packs -- against the float64 references of tests/motion_ref.py, per element.

Shapes are the product's: padded 720p / 1080p frames (736x1280, 1088x1920; warps checked on a row subset there), ragged frames,
n_ctx = 7 contexts per launch with window-level (stride 0) and per-context inputs, and the t values of the --fps retime
schedules (23.976 -> 60 fps gives t = 1/1001 ... 1000/1001).  Every output buffer starts as NaN, so an element a kernel leaves
unwritten fails.  Tolerances (motion_ref.check): fp32 outputs within a few fp32 ulps of the per-element bound, fp16 outputs
within one fp16 ulp of the float64 value plus that bound; CFR targets that receive no source must be exactly 0.

Every body takes an allocator of tests/guarded_arena.py: ``Plain`` (contiguous torch tensors, the tests of this file) or ``Arena``
(pitched views and strided items inside poison, tests/test_gpu_guarded_motion.py), and every launch goes through ``GA.launch``."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from demfi_amd import retime                         # noqa: E402
from tests import guarded_arena as GA                # noqa: E402
from tests import motion_ref as R                    # noqa: E402
from oracle import demfi_oracle as O                 # noqa: E402

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


def _dbg_expected(m, H, W, valid=None):
    """What the kernels' debug maps hold for the maps m of O.sample_maps: the floor indices (clamped to [-4, W + 4] / [-4, H + 4] before
    the int conversion), and the in-bounds bits of (nw, ne, sw, se) | 16 * validity -- int32 [3,H,W]."""
    inb = sum(m['inb'][k].astype(np.int32) << k for k in range(4))
    v = np.ones(inb.shape, bool) if valid is None else valid
    return np.stack([np.clip(m['ix0'], -4, W + 4), np.clip(m['iy0'], -4, H + 4), inb | (v.astype(np.int32) << 4)]).astype(np.int32)


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
    elif kind == 'outward':                   # with t = 0.5: every source within 2 px of a frame edge lands at -1.75 .. 0.75 or
        y, x = np.mgrid[0:H, 0:W]             # W - 1.75 .. W + 0.75 (likewise in y), in quarter steps: the four splat corners fall just
        q = np.arange(-1.75, 1.0, 0.25)       # inside and just outside every edge; the rest of the field stays near
        for ch, (p, n) in enumerate(((x, W), (y, H))):
            lo, hi = p < 2, p >= n - 2
            tgt = np.where(lo, rng.choice(q, (H, W)), n + rng.choice(q, (H, W)))
            f[ch] = np.where(lo | hi, 2.0 * (tgt - p), f[ch]).astype(f32)
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


def _cfr_body(al, H, W, nb, per_ctx, kinds, pack, seed=None, dbg=False):
    """One batched launch (twice: run to run the same bytes), nb single launches, fp64 per context; returns the number of far
    sources.  Flows, t, logits, the workspaces (exactly demfi_cfr_workspace_bytes each, zero-filled), out and the packed records are
    bare pointers: flat items of ``al``, the batch strides are the byte strides of those items.  dbg: the single launches also write
    their debug index maps, which must equal sample_one's ids / mask (O.splat_maps)."""
    lib = L.load()
    rng = np.random.default_rng(H * 7 + W + nb if seed is None else seed)
    # families made for t = 0.5 put it first; the others take the retime schedule
    ts = ([0.5] if kinds[0] in ('threshold', 'edges', 'collide', 'outward') else []) + [t for t in T7 if t != 0.5]
    ts = ts[:nb] if nb < 7 else T7
    nf = nb if per_ctx else 1
    f01 = np.stack([_cfr_flow(kinds[q % len(kinds)], H, W, rng) for q in range(nf)])
    f10 = np.stack([_cfr_flow(kinds[q % len(kinds)], H, W, rng) for q in range(nf)])
    d01 = al.fill(al.flat(nf, (2, H, W), torch.float32, name='flow01'), f01)
    d10 = al.fill(al.flat(nf, (2, H, W), torch.float32, name='flow10'), f10)
    t = al.fill(al.flat(nb, (1,), torch.float32, name='t'), _tdev(ts)[:, None])
    nacc = lib.demfi_cfr_workspace_bytes(H, W) // 8
    acc = al.flat(nb, (nacc,), torch.int64, zero=True, name='cfr workspace')
    acc1 = al.flat(1, (nacc,), torch.int64, zero=True, name='cfr workspace (single)')
    bt = L.Batch()
    bt.nb, bt.t = nb, GA.bstride(t)
    bt.p[0] = GA.bstride(d01) if per_ctx else 0
    bt.p[1] = GA.bstride(d10) if per_ctx else 0
    bt.p[2] = GA.bstride(acc)
    logit = None
    if pack is not None:
        logit = al.fill(al.flat(nb, (H, W), torch.float32, name='logit'), rng.standard_normal((nb, H, W)).astype(f32))
        bt.p[4] = GA.bstride(logit)

    def run():
        out = al.flat(nb, (4, H, W), torch.float32, name='cfr out')
        bt.p[3] = GA.bstride(out)
        if pack is None:
            GA.launch(al, lambda: lib.demfi_cfr_flow_align_batched(d01.data_ptr(), d10.data_ptr(), t.data_ptr(), H, W, acc.data_ptr(),
                                                                   out.data_ptr(), C.byref(bt), _stream()), [out], 'cfr batched')
            rec = None
        else:
            rec = al.flat(nb, (H, W, 16), pack, name='pack16')
            bt.p[5] = GA.bstride(rec)
            GA.launch(al, lambda: lib.demfi_cfr_flow_align_pack(d01.data_ptr(), d10.data_ptr(), logit.data_ptr(), t.data_ptr(), H, W,
                                                                acc.data_ptr(), out.data_ptr(), rec.data_ptr(),
                                                                L.F32 if pack == torch.float32 else L.F16, C.byref(bt), _stream()),
                      [out, rec], 'cfr pack')
        # the whole workspace of every context -- six int64 planes and the tile flags -- is left all-zero, far path included
        assert int(torch.count_nonzero(acc)) == 0
        return out, rec

    out, rec = run()
    assert torch.equal(out, run()[0])                                          # run to run: the same bytes
    nfar = 0
    for q in range(nb):
        g01, g10 = d01[q if per_ctx else 0], d10[q if per_ctx else 0]
        out1 = al.flat(1, (4, H, W), torch.float32, name='cfr out (single)')
        idx = al.flat(1, (2, 4, H * W), torch.int32, name='dbg_idx') if dbg else None
        GA.launch(al, lambda: lib.demfi_cfr_flow_align(g01.data_ptr(), g10.data_ptr(), t[q].data_ptr(), H, W, acc1.data_ptr(),
                                                       out1.data_ptr(), idx.data_ptr() if dbg else None, _stream()),
                  [out1] + ([idx] if dbg else []), 'cfr single')
        assert torch.equal(out[q], out1[0]), q                                  # batched == one launch per context
        assert int(torch.count_nonzero(acc1)) == 0
        a01, a10 = f01[q if per_ctx else 0], f10[q if per_ctx else 0]
        _cfr_check(out[q], a01, a10, ts[q], 'cfr %dx%d ctx %d t=%.6g' % (H, W, q, ts[q]))
        for k, (fl, s) in enumerate(((a01, f32(ts[q])), (a10, f32(1) - f32(ts[q])))):
            y1 = np.floor((fl * s).astype(f32))
            nfar += int(((y1 < -32) | (y1 > 31)).any(0).sum())
            if dbg:                                                             # splat targets: sample_one's idxx / idxy / mask
                for c, m in enumerate(O.splat_maps((fl * s).astype(f32), H, W)):
                    exp = np.where(m['mask'], m['row'] * W + m['col'], -1).astype(np.int32).reshape(-1)
                    assert np.array_equal(idx[0, k, c].cpu().numpy(), exp), (q, k, c)
        if pack is not None:
            planes = torch.cat([out[q], g01, g10, logit[q][None]], 0)
            assert torch.equal(rec[q][..., :9], planes.permute(1, 2, 0).to(pack))
            assert int(torch.count_nonzero(rec[q][..., 9:])) == 0
    return nfar


@pytest.mark.parametrize('H,W,nb,per_ctx,kinds,pack', CFR_CASES)
def test_cfr_batched_matches_fp64_and_single_launches(H, W, nb, per_ctx, kinds, pack):
    assert _cfr_body(GA.Plain(DEV), H, W, nb, per_ctx, kinds, pack) > 0        # the far path ran in every case


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
    """Inputs of nb contexts on the GPU.  ab_ctx: A / B have a copy per context (else one window-level copy, stride 0).  al: the
    allocator (GA.Plain by default): A / B / out are views (fat NHWC, or thin planar fp32) with the strides al gives them; flows,
    logits, t, occ_out and the packed records are bare pointers -- flat items of al, batched at their byte strides."""

    def __init__(self, H, W, Cc, dtype, nb, ab_ctx, seed, planar=False, al=None):
        rng = np.random.default_rng(seed)
        self.al = al = al if al is not None else GA.Plain(DEV)
        self.H, self.W, self.C, self.dtype, self.nb, self.planar = H, W, Cc, dtype, nb, planar
        na = nb if ab_ctx else 1
        shape = (na, Cc, H, W) if planar else (na, H, W, Cc)
        assert not planar or dtype == torch.float32
        new = (lambda name: al.thin(Cc, H, W, n=na, name=name)) if planar else (lambda name: al.fat(na, H, W, Cc, dtype, name=name))
        self.A = al.fill(new('A'), np.tanh(rng.standard_normal(shape)).astype(f32))
        self.B = al.fill(new('B'), np.tanh(rng.standard_normal(shape)).astype(f32))
        self.fa = np.stack([_warp_flow(H, W, rng) for _ in range(nb)])
        self.fb = np.stack([_warp_flow(H, W, rng) for _ in range(nb)])
        self.lg = np.stack([_logit(H, W, rng) for _ in range(nb)])
        self.dfa = al.fill(al.flat(nb, (2, H, W), torch.float32, name='fa'), self.fa)
        self.dfb = al.fill(al.flat(nb, (2, H, W), torch.float32, name='fb'), self.fb)
        self.dlg = al.fill(al.flat(nb, (H, W), torch.float32, name='logit'), self.lg)
        self.ts = [T7[(q * 3 + seed) % 7] for q in range(nb)]
        self.t = al.fill(al.flat(nb, (1,), torch.float32, name='t'), _tdev(self.ts)[:, None])
        self.esz = self.A.element_size()
        self.ab_stride = GA.bstride(self.A) if ab_ctx else 0

    def view(self, t, q=0):
        """demfi_view of image q of t ([n,H,W,C] NHWC or [n,C,H,W] planar), strides from the tensor itself."""
        f = 1 if t.dtype == torch.float32 else 0
        if self.planar:
            return L.View(t[q].data_ptr(), t.stride(3), t.stride(2), t.stride(1), 0, f, 0)
        return L.View(t[q].data_ptr(), t.stride(2), t.stride(1), 1, 0, f, 0)

    def new_out(self, nb):
        if self.planar:
            return self.al.thin(self.C, self.H, self.W, n=nb, name='out')
        return self.al.fat(nb, self.H, self.W, self.C, self.dtype, name='out')

    def single(self, q, lib, dbg=False):
        """dbg: the launch also writes its debug maps, which must equal the integer maps of grid_sample (R.warp_maps)."""
        H, W = self.H, self.W
        out = self.new_out(1)
        occ = self.al.flat(1, (H, W), torch.float32, name='occ')
        maps = self.al.flat(1, (2, 3, H, W), torch.int32, name='dbg_maps') if dbg else None
        qa = q if self.ab_stride else 0
        va, vb, vo = self.view(self.A, qa), self.view(self.B, qa), self.view(out)
        GA.launch(self.al, lambda: lib.demfi_warp_blend(C.byref(va), self.dfa[q].data_ptr(), C.byref(vb), self.dfb[q].data_ptr(),
                                                        self.dlg[q].data_ptr(), self.t[q].data_ptr(), C.byref(vo), self.C, H, W,
                                                        occ.data_ptr(), maps.data_ptr() if dbg else None, _stream()),
                  [out, occ] + ([maps] if dbg else []), 'warp single')
        if dbg:
            for which, fl in ((0, self.fa[q]), (1, self.fb[q])):
                m = R.warp_maps(fl)
                assert np.array_equal(maps[0, which].cpu().numpy(), _dbg_expected(m, H, W, m['valid'])), (q, which)
        return out[0], occ[0]

    def single_pack(self, q, lib, pack):
        """demfi_warp_blend_pack of context q (planar 3-channel views): (out [3,H,W], occ [H,W], pack8 [H,W,8])."""
        out = self.new_out(1)
        occ = self.al.flat(1, (self.H, self.W), torch.float32, name='occ')
        rec = self.al.flat(1, (self.H, self.W, 8), pack, name='pack8')
        qa = q if self.ab_stride else 0
        va, vb, vo = self.view(self.A, qa), self.view(self.B, qa), self.view(out)
        GA.launch(self.al, lambda: lib.demfi_warp_blend_pack(C.byref(va), self.dfa[q].data_ptr(), C.byref(vb), self.dfb[q].data_ptr(),
                                                             self.dlg[q].data_ptr(), self.t[q].data_ptr(), C.byref(vo), self.H, self.W,
                                                             occ.data_ptr(), rec.data_ptr(), L.F32 if pack == torch.float32 else L.F16,
                                                             _stream()), [out, occ, rec], 'warp pack')
        return out[0], occ[0], rec[0]

    def batched(self, lib, outer, pack=None):
        H, W = self.H, self.W
        out = self.new_out(self.nb)
        occ = self.al.flat(self.nb, (H, W), torch.float32, name='occ')
        bt = L.Batch()
        bt.nb, bt._pad = self.nb, outer
        bt.a, bt.b = self.ab_stride, (GA.bstride(self.B) if self.ab_stride else 0)      # each its own: tests/far_memory.py moves one of them apart
        bt.o = GA.bstride(out)
        bt.t = GA.bstride(self.t)
        bt.p[0], bt.p[1] = GA.bstride(self.dfa), GA.bstride(self.dfb)
        bt.p[2], bt.p[3] = GA.bstride(self.dlg), GA.bstride(occ)
        rec, pdt = None, 0
        if pack is not None:
            rec = self.al.flat(self.nb, (H, W, 8), pack, name='pack8')
            bt.p[4] = GA.bstride(rec)
            pdt = L.F32 if pack == torch.float32 else L.F16
        va, vb, vo = self.view(self.A), self.view(self.B), self.view(out)
        GA.launch(self.al, lambda: lib.demfi_warp_blend_batched(C.byref(va), self.dfa.data_ptr(), C.byref(vb), self.dfb.data_ptr(),
                                                                self.dlg.data_ptr(), self.t.data_ptr(), C.byref(vo), self.C, H, W,
                                                                occ.data_ptr(), rec.data_ptr() if rec is not None else None, pdt,
                                                                C.byref(bt), _stream()),
                  [out, occ] + ([rec] if rec is not None else []), 'warp batched')
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


def _fat_body(al, H, W, dtype, Cc, ab_ctx, seed, dbg=False):
    lib = L.load()
    ws = _WarpSet(H, W, Cc, dtype, 3, ab_ctx, seed=seed, al=al)
    singles = [ws.single(q, lib, dbg) for q in range(3)]
    for outer in (0, 1):
        out, occ, _ = ws.batched(lib, outer)
        for q in range(3):
            assert torch.equal(out[q], singles[q][0]) and torch.equal(occ[q], singles[q][1]), (outer, q)
    for q in range(3):
        ws.check(q, *singles[q])


@pytest.mark.parametrize('dtype,Cc', FAT)
@pytest.mark.parametrize('ab_ctx', [False, True])
def test_fat_warp_all_lane_counts_single_inner_outer(dtype, Cc, ab_ctx):
    """Ragged frame (H % 4 != 0, W % 64 != 0), lpp = 1 ... 64 lanes per pixel: nb single launches, one batched launch with the
    contexts innermost (_pad = 0) and one with a grid slice per context (_pad = 1) give the same bytes, and match fp64."""
    _fat_body(GA.Plain(DEV), 37, 130, dtype, Cc, ab_ctx, seed=Cc + 1000 * ab_ctx)


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


def _nhwc_thin_body(al, H, W, dtype, Cc, dbg=False):
    lib = L.load()
    ws = _WarpSet(H, W, Cc, dtype, 3, True, seed=Cc, al=al)
    out, occ, _ = ws.batched(lib, 0)
    for q in range(3):
        o1, c1 = ws.single(q, lib, dbg)
        assert torch.equal(out[q], o1) and torch.equal(occ[q], c1)
        ws.check(q, out[q], occ[q])


@pytest.mark.parametrize('dtype,Cc', [(torch.float16, 12), (torch.float32, 3)])
def test_nhwc_views_that_are_not_16_byte_records_take_the_thin_kernel(dtype, Cc):
    _nhwc_thin_body(GA.Plain(DEV), 37, 130, dtype, Cc)


def _thin_pack_body(al, H, W, pack, ab_ctx, nb, seed, dbg=False):
    lib = L.load()
    ws = _WarpSet(H, W, 3, torch.float32, nb, ab_ctx, seed=seed, planar=True, al=al)
    out, occ, rec = ws.batched(lib, 0, pack)
    rows = None if H < 200 else _rows(H, np.random.default_rng(1))
    for q in range(nb):
        ws.check(q, out[q], occ[q], rows)
        planes = torch.cat([out[q], ws.dfa[q], ws.dfb[q], occ[q][None]], 0)
        assert torch.equal(rec[q], planes.permute(1, 2, 0).to(pack)), q
        o1, c1, r1 = ws.single_pack(q, lib, pack)
        assert torch.equal(o1, out[q]) and torch.equal(c1, occ[q]) and torch.equal(r1, rec[q]), q
        o2, c2 = ws.single(q, lib, dbg)                                          # demfi_warp_blend on the planar views, no record
        assert torch.equal(o2, out[q]) and torch.equal(c2, occ[q]), q


@pytest.mark.parametrize('H,W,pack,ab_ctx', [(100, 130, torch.float16, True), (100, 130, torch.float32, False),
                                             (736, 1280, torch.float16, False)])
def test_thin_warp_pack_batched_seven_contexts(H, W, pack, ab_ctx):
    """Planar fp32 3-channel frames, nb = 7 in one launch with the packed record [out | fa | fb | sigmoid(logit)]: values against
    fp64, the record equal to the planes rounded to the pack dtype, each context equal to its own demfi_warp_blend_pack launch."""
    _thin_pack_body(GA.Plain(DEV), H, W, pack, ab_ctx, 7, seed=H)


# ------------------------------------------------------------------------------------------------------------------------------
# FGAC gather + gate blend
# ------------------------------------------------------------------------------------------------------------------------------
def _nhwc_view(t):
    """demfi_view of one NHWC image [H,W,C], strides from the tensor."""
    return L.View(t.data_ptr(), t.stride(1), t.stride(0), 1, 0, 1 if t.dtype == torch.float32 else 0, 0)


def _gather_gate_body(al, dtype, H, W, Cc, far=(), dbg=False):
    """far: further absolute positions (dx, dy beyond the frame: x = -dx or W - 1 + dx, y likewise) added to the out-of-frame choices."""
    lib = L.load()
    rng = np.random.default_rng(9)
    S = al.fill(al.fat(1, H, W, Cc, dtype, name='S'), np.tanh(rng.standard_normal((1, H, W, Cc))).astype(f32))[0]
    fl = np.stack([rng.uniform(0, W - 1, (H, W)), rng.uniform(0, H - 1, (H, W))]).astype(f32)
    fl[:, 1::4] = np.round(fl[:, 1::4])                                         # integer-exact
    xs = [W - 1, W - 0.75, W - 1 + 1e-3, W + 3.0, -0.5, -2.0] + [v for d in far for v in (-d, W - 1 + d)]
    ys = [H - 1, H - 0.5, H + 2.0, -0.25] + [v for d in far for v in (-d, H - 1 + d)]
    fl[0, 2::4] = rng.choice(xs, (len(range(2, H, 4)), W))                      # beyond the last column
    fl[1, 3::4] = rng.choice(ys, (len(range(3, H, 4)), W))                      # ... and the last row
    fl = np.ascontiguousarray(fl.astype(f32))
    dfl = al.fill(al.flat(1, (2, H, W), torch.float32, name='flow'), fl[None])
    out = al.fat(1, H, W, Cc, dtype, name='gathered')[0]
    vs, vo = _nhwc_view(S), _nhwc_view(out)
    maps = al.flat(1, (3, H, W), torch.int32, name='dbg_maps') if dbg else None
    GA.launch(al, lambda: lib.demfi_fgac_gather(C.byref(vs), dfl.data_ptr(), C.byref(vo), Cc, H, W, maps.data_ptr() if dbg else None,
                                                _stream()), [out] + ([maps] if dbg else []), 'fgac gather')
    if dbg:                                                                     # the integer maps of grid_sample, no validity mask
        assert np.array_equal(maps[0].cpu().numpy(), _dbg_expected(O.sample_maps(fl[0], fl[1], H, W), H, W))
    f16 = dtype == torch.float16
    v, a = R.fgac_gather(S.cpu().numpy(), fl)
    R.check(out.float().cpu().numpy(), v, a, 8, 'fgac gather', ulp16=f16)
    w = rng.random((H, W)).astype(f32)
    w[:, :3] = [0.0, 1.0, 0.5]
    E = al.fill(al.fat(1, H, W, Cc, dtype, name='E'), rng.standard_normal((1, H, W, Cc)).astype(f32))[0]
    o2 = al.fat(1, H, W, Cc, dtype, name='blended')[0]
    dw = al.fill(al.flat(1, (H, W), torch.float32, name='w'), w[None])
    ve, v2 = _nhwc_view(E), _nhwc_view(o2)
    GA.launch(al, lambda: lib.demfi_gate_blend(dw.data_ptr(), C.byref(vo), C.byref(ve), C.byref(v2), Cc, H, W, _stream()), [o2], 'gate blend')
    g, ga = R.gate_blend(w, out.cpu().numpy(), E.cpu().numpy())
    R.check(o2.float().cpu().numpy(), g, ga, 8, 'gate blend', ulp16=f16)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_fgac_gather_and_gate_blend_full_width(dtype):
    _gather_gate_body(GA.Plain(DEV), dtype, 24, 1920, 64)


# ------------------------------------------------------------------------------------------------------------------------------
# Plane packs
# ------------------------------------------------------------------------------------------------------------------------------
def _pack_body(al, nch, dtype, H, W, n_null=None):
    """n_null: exactly that many NULL planes (None: each plane with probability 1/4).  dst is a channel slice of a record that is
    8 channels wider than nch; each context is also packed by a demfi_pack_planes launch of its own into a second record."""
    lib = L.load()
    rng = np.random.default_rng(nch)
    nb = 3
    sx = nch + 8
    vals = (rng.standard_normal((nch, nb, H, W)) * 100).astype(f32)
    null = rng.random(nch) < 0.25
    per_ctx = rng.random(nch) < 0.5
    if n_null is not None:
        null[:] = False
        null[rng.choice(nch, n_null, replace=False)] = True
    planes = [al.fill(al.flat(nb if per_ctx[i] else 1, (H, W), torch.float32, name='plane %d' % i), vals[i, :nb if per_ctx[i] else 1])
              for i in range(nch)]
    dst = al.flat(nb, (H, W, sx), dtype, name='record')
    dst1 = al.flat(nb, (H, W, sx), dtype, name='record (single launches)')
    ptrs = (C.c_void_p * nch)(*[None if null[i] else planes[i].data_ptr() for i in range(nch)])
    bt = L.Batch()
    bt.nb, bt.o = nb, GA.bstride(dst)
    for i in range(nch):
        bt.p[i] = GA.bstride(planes[i]) if per_ctx[i] else 0
    dt = L.F32 if dtype == torch.float32 else L.F16
    GA.launch(al, lambda: lib.demfi_pack_planes_batched(ptrs, nch, dst.data_ptr(), dt, sx, H, W, C.byref(bt), _stream()), [dst[..., :nch]],
              'pack batched')
    for q in range(nb):
        for i in range(nch):
            exp = torch.zeros(H, W, device=DEV) if null[i] else planes[i][q if per_ctx[i] else 0]
            assert torch.equal(dst[q, ..., i], exp.to(dtype)), (q, i)
        p1 = (C.c_void_p * nch)(*[None if null[i] else planes[i][q if per_ctx[i] else 0].data_ptr() for i in range(nch)])
        GA.launch(al, lambda: lib.demfi_pack_planes(p1, nch, dst1[q].data_ptr(), dt, sx, H, W, _stream()), [dst1[q, ..., :nch]], 'pack')
        assert torch.equal(dst1[q, ..., :nch], dst[q, ..., :nch]), q
    # the channels of the record that the launch does not own are what they were (NaN / poison)
    assert bool(torch.isnan(dst[..., nch:].float()).all()) and bool(torch.isnan(dst1[..., nch:].float()).all())


@pytest.mark.parametrize('nch', [8, 16, 24, 32])
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_pack_planes_batched(nch, dtype):
    """nb = 3 contexts, planes with a per-context copy or window-level (stride 0), NULL planes (zeros), a destination record wider
    than nch (the channels past nch stay untouched); fp16 rounding equal to torch's .half()."""
    _pack_body(GA.Plain(DEV), nch, dtype, 37, 130)
