"""float64 references of the motion kernels -- the CFR forward splat + finish, the Eq.(2) backward warp + occlusion blend, the FGAC
gather and the Eq.(4) gate blend.  Test infrastructure only; imports nothing from the GPU side.

Every integer decision (splat target rows / columns and masks, grid-sample floor indices, in-bounds bits, validity) and every
corner weight is taken from the oracle's fp32-exact maps (O.splat_maps, O.sample_maps, O.backward_warp_maps), which
tests/test_gpu_kernels.py proves bit-identical to the kernels.  Everything after the maps runs in float64: gathers, splat sums,
sigmoid, Eq.(2), the CFR finish.

Besides the value, every reference returns a per-element ``bound``: an upper bound, in units of one fp32 ulp (2^-23), of what the
kernel's fp32 steps may legitimately add (sums of absolute values of the terms that make up an element, and the sensitivity to
the fp32 rounding of the blend factors).  A test then checks |kernel - ref| <= k * 2^-23 * bound per element, which stays tight
where terms cancel and where a blend is badly conditioned, instead of a global maximum.

The warp and gather references take an optional row subset, so that full frames (1088x1920) are checked on selected rows.
"""
import numpy as np

from oracle import demfi_oracle as O

f32 = np.float32
f64 = np.float64
EPS32 = 2.0 ** -23
FIX_ULP = 2.0 ** -32                  # the CFR accumulators are 2^-32 fixed point: each summand is rounded to it


def fp16_ulp(x):
    """One fp16 ulp at |x| (subnormal spacing below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


# ------------------------------------------------------------------------------------------------------------------------------
# CFR: fwarp (DeMFInet.py:625-729) of both flows + CFR_flow_t_align (606-622)
# ------------------------------------------------------------------------------------------------------------------------------
def splat_sums(img, flo):
    """Forward splat of img [C,H,W] along the fp32 displacement flo [2,H,W] (already scaled).  The summands are the fp32 products
    img * w, as the kernel's cfr_fix sees them; the sums are float64 (np.bincount).  Returns (val [C,H,W], one [H,W], absval [C,H,W],
    count [H,W]): weighted values, weight sum, sum of |summand| and the number of summands per target."""
    C, H, W = img.shape
    hw = H * W
    val, absval = np.zeros((C, hw)), np.zeros((C, hw))
    one, cnt = np.zeros(hw), np.zeros(hw)
    for m in O.splat_maps(flo.astype(f32), H, W):
        mask = m['mask']
        ids = (m['row'] * W + m['col'])[mask]
        one += np.bincount(ids, m['w'][mask].astype(f64), hw)
        cnt += np.bincount(ids, minlength=hw)
        for c in range(C):
            p = (img[c].astype(f32) * m['w']).astype(f32)[mask].astype(f64)
            val[c] += np.bincount(ids, p, hw)
            absval[c] += np.bincount(ids, np.abs(p), hw)
    return val.reshape(C, H, W), one.reshape(H, W), absval.reshape(C, H, W), cnt.reshape(H, W)


def cfr(f01, f10, t):
    """CFR_flow_t_align for flows [2,H,W] fp32 and the fp32 device value t.  Returns dict(ft [4,H,W] = flow_t0 (2), flow_t1 (2),
    bound [4,H,W], hit [H,W] (norm > 0: some source lands there), norm [H,W])."""
    t32 = f32(t)
    s01 = splat_sums(f01, (f01.astype(f32) * t32).astype(f32))             # fwarp(f01, t * f01)
    s10 = splat_sums(f10, (f10.astype(f32) * (f32(1) - t32)).astype(f32))   # fwarp(f10, (1 - t) * f10)
    t = f64(t32)
    omt = 1.0 - t
    norm = omt * s01[1] + t * s10[1]
    hit = norm > 0
    den = np.where(hit, norm, 1.0)
    ca, cb, cc, cd = -omt * t, t * t, omt * omt, t * omt
    ft = np.zeros((4,) + norm.shape)
    bound = np.zeros_like(ft)
    for ch in range(2):
        ft[ch] = (ca * s01[0][ch] + cb * s10[0][ch]) / den
        ft[2 + ch] = (cc * s01[0][ch] - cd * s10[0][ch]) / den
        for j, (x, y) in enumerate(((ca, cb), (cc, cd))):
            terms = abs(x) * s01[2][ch] + abs(y) * s10[2][ch]
            fix = (abs(x) * s01[3] + abs(y) * s10[3]) * FIX_ULP / EPS32   # fixed-point rounding of the summands, in fp32 ulps
            bound[2 * j + ch] = (terms + fix) / den + np.abs(ft[2 * j + ch])
    return dict(ft=ft, bound=bound, hit=hit, norm=norm)


# ------------------------------------------------------------------------------------------------------------------------------
# Backward warp + Eq.(2) blend (DeMFInet.py:66-71, 732-766), FGAC sampling (413-419, 499-514), gate blend (452)
# ------------------------------------------------------------------------------------------------------------------------------
def _rows(rows, H):
    return np.arange(H) if rows is None else np.asarray(rows, np.int64)


def warp_maps(flo, rows=None):
    """O.backward_warp_maps restricted to the given rows of flo [2,H,W]: sample maps at (col + flo[0], row + flo[1]) plus the
    validity of the all-ones warp (sum of in-bounds weights >= 0.999, > 0)."""
    _, H, W = flo.shape
    r = _rows(rows, H)
    fl = flo[:, r].astype(f32)
    px = (np.arange(W, dtype=f32)[None, :] + fl[0]).astype(f32)
    py = (r.astype(f32)[:, None] + fl[1]).astype(f32)
    m = O.sample_maps(px, py, H, W)
    s = np.zeros(px.shape, f32)
    for w, inb in zip(m['w'], m['inb']):
        s = (s + np.where(inb, w, f32(0))).astype(f32)
    m['valid'] = ~(s < f32(0.999)) & (s > 0)
    return m


def gather(img, m):
    """Zero-padded bilinear gather of img [H,W,C] (NHWC, any float dtype) at the maps m over [R,W'] -> (value, sum of |term|), both
    float64 [R,W',C]."""
    H, W, _ = img.shape
    out = absout = 0.0
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):          # nw, ne, sw, se
        xi = np.clip(m['ix0'] + dx, 0, W - 1)
        yi = np.clip(m['iy0'] + dy, 0, H - 1)
        w = np.where(m['inb'][k], m['w'][k], f32(0)).astype(f64)[..., None]
        v = img[yi, xi].astype(f64)
        out = out + v * w
        absout = absout + np.abs(v) * w
    return out, absout


def bwarp(img, flo, rows=None):
    """bwarp (DeMFInet.py:732-766) of img [H,W,C] by flo [2,H,W] on the given rows: (value, sum of |term|), float64 [R,W,C]."""
    m = warp_maps(flo, rows)
    v, a = gather(img, m)
    keep = m['valid'][..., None]
    return np.where(keep, v, 0.0), np.where(keep, a, 0.0)


def warp_blend(A, fa, B, fb, logit, t, rows=None):
    """Eq.(2): ((1-t) o0 bwarp(A, fa) + t (1-o0) bwarp(B, fb)) / ((1-t) o0 + t (1-o0)), o0 = sigmoid(logit), for NHWC A / B [H,W,C]
    (planar sources: pass a [H,W,C] view).  Returns dict(out [R,W,C], occ [R,W] = o0, bound [R,W,C]).

    bound: the absolute terms of the numerator over the denominator, plus the sensitivity to the fp32 rounding of o0 and 1 - o0
    (|d out / d o0| = |a - b| t (1-t) / den^2), which dominates where the denominator is small."""
    H = A.shape[0]
    r = _rows(rows, H)
    a, aa = bwarp(A, fa, r)
    b, ba = bwarp(B, fb, r)
    t = f64(f32(t))
    with np.errstate(over='ignore'):                                         # logits below -709: exp -> inf, o0 = 0, as intended
        o0 = 1.0 / (1.0 + np.exp(-logit[r].astype(f64)))
    ka = ((1.0 - t) * o0)[..., None]
    kb = (t * (1.0 - o0))[..., None]
    den = ka + kb
    out = (ka * a + kb * b) / den
    bound = (ka * aa + kb * ba) / den + np.abs(out) + np.abs(a - b) * (t * (1.0 - t)) / (den * den)
    return dict(out=out, occ=o0, bound=bound)


def fgac_gather(S, flow, rows=None):
    """bilinear_sampler at ABSOLUTE coordinates (flow [2,H,W] = x, y), zero padding, no validity mask, of S [H,W,C]:
    (value, sum of |term|) float64 [R,W,C]."""
    H = S.shape[0]
    r = _rows(rows, H)
    fl = flow[:, r].astype(f32)
    return gather(S, O.sample_maps(fl[0], fl[1], H, S.shape[1]))


def gate_blend(w, S, E, rows=None):
    """Eq.(4): w * S + (1 - w) * E for w [H,W], S / E [H,W,C] -> (value, sum of |term|) float64 [R,W,C]."""
    r = _rows(rows, S.shape[0])
    g = w[r].astype(f64)[..., None]
    s, e = S[r].astype(f64), E[r].astype(f64)
    return g * s + (1.0 - g) * e, np.abs(g * s) + np.abs((1.0 - g) * e)


def check(got, ref, bound, k, what, ulp16=False, exact_zero=None):
    """|got - ref| <= k * 2^-23 * bound (+ one fp16 ulp of ref with ulp16) element by element; NaN in got (an unwritten sentinel)
    fails.  exact_zero: mask of elements that must be exactly 0.  Raises AssertionError naming the worst element."""
    got = np.asarray(got, f64)
    tol = k * EPS32 * bound
    if ulp16:
        tol = tol + fp16_ulp(ref)
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    if exact_zero is not None:
        bad |= exact_zero & (got != 0)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(err / np.maximum(tol, 1e-300), nan=np.inf), -1.0)), bad.shape)
        raise AssertionError('%s: %d of %d elements off, worst at %s: got %r, ref %r, tol %.3g'
                             % (what, int(bad.sum()), bad.size, tuple(int(v) for v in i), float(got[i]), float(ref[i]), float(tol[i])))
