"""float64 references of the fused convolution epilogues and a per-element error bound.  Test infrastructure only: plain numpy / torch
on the CPU, nothing from the GPU side, no kernel code.

What an epilogue is here: an fp32 accumulator  acc = sum_k x_k w_k  over fp16 operands, the fp32 bias added to it, then one of

    ACT_NONE / ACT_RELU / ACT_TANH / ACT_SIGMOID      (optionally a residual added BEFORE the activation),
    MODE_MUL      sigmoid(v) * h,
    MODE_GRU      (1 - z) h + z tanh(v)       with z READ AS STORED (the fp16 / fp32 value the z launch wrote),
    fused zq      (1 - z) h + z tanh(v_q),  z = sigmoid(v_z)  with z in fp32: demfi_gru_zq (gru.hip, pass 1 / pass 2 of its
                  epilogue) keeps  r = 1 / ((e^{2q'} + 1)(1 + e^{-z'}))  in an fp32 accumulator register and never rounds z to
                  fp16; the reference therefore does not round z either (``ref_zq``).

and a store as fp16 (NHWC) or fp32 (planes, the fp32 path).

The bound
---------
``bound(ref, sens, S, out_dtype, ...)`` is the largest |got - ref| an honest kernel may show at one element; u = 2^-24.

1. Accumulation:  sens * C_ACC * u * S.   S = conv(|x|, |w|) + |bias| is the sum of the absolute terms; fp32
   accumulation in any order differs from the exact sum by at most (n - 1) u S and in practice by a random walk far below it.
   ``measure_c`` measures  |fp32 sum - fp64 sum| / (u S)  on the CPU for two summation orders -- torch's fp32 conv2d and a numpy
   accumulation in 16-channel blocks, tap-major, the shape of an MFMA k-walk -- over 64->64 3x3, 128->64 1x5, 128->64 5x1 and
   192->64 7x7 with N(0,1) activations and unit-variance outputs.  Measured maxima (tests/test_epilogue_ref.py prints them):

       shape             torch fp32 conv2d    16-channel blocks, tap-major
       64->64  3x3         2.15 .. 4.08                     0.89
       128->64 1x5             0.90                       1.09
       128->64 5x1             0.87                       0.94
       192->64 7x7             0.58                       0.87

   (torch picks its summation order per run and thread count: 2.15 and 4.08 were both seen for 3x3; the larger one counts.)
   C_ACC = 8 x the measured maximum (4.08), rounded up = 33.  The factor 8 covers the MFMA's unspecified internal order and the fused
   multiply-add paths.  The reference, not a kernel, sets it.  sens = max |f'| over [v - d, v + d] with d = C_ACC u S, f the
   activation: 1 for none / relu, <= 1 for tanh, <= 1/4 for sigmoid; the gated modes multiply it by |h| or |z| (see each ref_*).
   The constant is recorded here, not re-derived per run: a fresh measurement on another CPU or thread count may come out up to twice
   the recorded one before the CPU test objects, so the effective margin over a fresh measurement may be as low as 4.
   The bound is only meaningful while this term stays below 2^-12 (a quarter of the fp16 spacing at 1.0): QUARTER_ULP, asserted for
   every case by the CPU tests.

2. Evaluation (transcendental):  4 u M  +  sens * u * |K v| * ln 2.
   The kernels evaluate sigmoid(v) = rcp(1 + exp2(K v)), K = -log2 e, and tanh(v) = 1 - 2 rcp(1 + exp2(K v)), K = 2 log2 e, on
   v_exp_f32 / v_rcp_f32 (about 1 ulp each), i.e. three or four fp32 roundings of relative size <= 2u.  For the sigmoid the result
   itself carries them: M = |sigmoid|.  The tanh form ends in a SUBTRACTION of two numbers of size <= 2, so its error is absolute:
   M = 1 + |tanh| (not |tanh|: no kernel here claims relative accuracy of tanh near 0, and the honest form does not have it).
   The gated forms add their own fp32 blend arithmetic on terms of size |h|, |z|, |z tanh|:  MODE_MUL M = |sigmoid h|,
   MODE_GRU and zq  M = |h| + |z| (1 + |h|).
   The argument K v is rounded once to fp32 (relative u), which moves exp2 by the relative amount u |K v| ln 2, i.e. the
   pre-activation by u |v|: the second term.  Inside saturation sens = 0 and it vanishes.

3. Storage:  0.5 * spacing_out(|ref| + terms 1 and 2).  fp16: the fp16 spacing, subnormals included, never below 2^-24.
   fp32: the fp32 spacing; in addition results below the smallest normal fp32 (2^-126) may be flushed to zero by the hardware
   transcendentals (v_rcp_f32 of a number above 2^126), so 2^-126 is added for fp32 outputs.  That is the only absolute floor.  It
   follows from the instruction set, not from a run: v_rcp_f32 and v_exp_f32 do not support denormals -- they flush denormal
   inputs and results whatever the wave's denormal mode is (which is why compilers expand an IEEE division around v_rcp_f32 with
   scaling) -- so the smallest normal is the resolution of a result that comes straight out of v_rcp_f32.

Saturation: where the activation rounds to the same value 0 / +-1 of the output type over the whole interval [v - d, v + d]
(``saturated``; the interval of values widened by the evaluation term), the kernel's result must be EXACTLY that value; the tests assert equality there, not the bound.

The old rule of the kernel tests, for comparison: |got - ref| < 4e-3 max(1, max |ref|) on the whole tensor.
"""
import math

import numpy as np
import torch

F = torch.nn.functional
f64 = torch.float64
U = 2.0 ** -24
QUARTER_ULP = 2.0 ** -12
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3      # include/demfi_hip.h (tests/test_epilogue_ref.py checks them against _lib)

# measured by measure_c() (see the table above); C_ACC = 8 x max, rounded up
MEASURED_C = {(64, 64, 3, 3): (4.08, 0.89), (128, 64, 1, 5): (0.90, 1.09), (128, 64, 5, 1): (0.87, 0.94), (192, 64, 7, 7): (0.58, 0.87)}
C_ACC = 33.0

_G = [0.0, 1e-4, 1e-3, 0.1, 1.0, 4.0, 8.5, 9.1, 12.0, 17.0, 20.7, 20.9, 30.0, 44.0, 45.0, 88.0, 89.0, 200.0, 1e4]
GRID = [s * g for g in _G for s in (1.0, -1.0)]            # 38 values; +0.0 and -0.0 both occur
# bias[c] = GRID[(7 c + k) % 38]: 7 is a unit mod 38, so one run already puts every value on some channel.  Which lane half, register
# quad and 32-cout sub-tile a channel lands on is a function of its bits -- plain packed order: cout = 32 s + 8 g + 4 hi + j; cout_perm
# order of the 64-channel kernels: channel = 32 s + 16 m2 + 8 hi + j.  (0, 1, 16) is the smallest set of rotations over which every value
# meets both lane halves of both orders, both sub-tiles and all four quads (found by enumeration; tests/test_epilogue_ref.py asserts it).
ROTATIONS = (0, 1, 16)


def grid_bias(cout, k, grid=GRID):
    return torch.tensor([grid[(7 * c + k) % len(grid)] for c in range(cout)], dtype=torch.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# pre-activation
# --------------------------------------------------------------------------------------------------------------------------------
def preact(x16, w16, bias32, pad, stride=1):
    """x16 [B,C,H,W], w16 [O,C,kh,kw]: fp16 values (any dtype holding them), bias32 [O] fp32 values.
    Returns (v, S): the float64 convolution plus bias, and S = conv(|x|, |w|) + |b|."""
    x, w, b = x16.to(f64), w16.to(f64), bias32.to(f64)
    v = F.conv2d(x, w, b, stride=stride, padding=pad)
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
    return v, S


def spacing(x, out_dtype):
    """Spacing of out_dtype at |x| (float64 tensor): fp16 with subnormals (>= 2^-24), fp32 (>= 2^-149)."""
    a = x.abs()
    if out_dtype == torch.float16:
        e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -14)))
        return torch.pow(torch.tensor(2.0, dtype=f64), e - 10)
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=f64), e - 23)


def round_to(x, out_dtype):
    """Round-to-nearest-even of float64 values to out_dtype, returned as float64 (inf above the format's range)."""
    return x.to(out_dtype).to(f64)


def _act(v, act):
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def _dact_max(v, d, act):
    """max |f'| over [v - d, v + d]."""
    if act in (ACT_NONE, ACT_RELU):
        return torch.ones_like(v)
    near = torch.clamp(v.abs() - d, min=0.0)                 # the point of the interval closest to 0, where f' peaks
    if act == ACT_TANH:
        return 1.0 / torch.cosh(torch.clamp(near, max=350.0)) ** 2
    e = torch.exp(-near)                                      # sigmoid' = e^-x / (1 + e^-x)^2, without the cancellation of s (1 - s)
    return e / (1.0 + e) ** 2


def _delta(S, c=None):
    return (C_ACC if c is None else c) * U * S


class Ref:
    """ref: expected value (float64); acc: accumulation term of the bound; ev: evaluation term; sat: mask of elements that must be
    EXACT, sat_val: their value in float64; kink: elements within the accumulation allowance of ReLU's kink (may be excluded)."""
    __slots__ = ('ref', 'acc', 'ev', 'sat', 'sat_val', 'kink')

    def __init__(self, ref, acc, ev, sat=None, sat_val=None, kink=None):
        self.ref, self.acc, self.ev = ref, acc, ev
        self.sat = torch.zeros_like(ref, dtype=torch.bool) if sat is None else sat
        self.sat_val = ref if sat_val is None else sat_val
        self.kink = torch.zeros_like(ref, dtype=torch.bool) if kink is None else kink

    def bound(self, out_dtype):
        return bound(self.ref, None, None, out_dtype, acc=self.acc, ev=self.ev)


def bound(ref, sens, S, out_dtype, mag=None, arg=None, c=None, acc=None, ev=None):
    """Largest honest |got - ref| per element (module docstring).  sens, S: arrays, or equally long lists of arrays whose products
    are summed (the zq form has two accumulators).  mag: M of the evaluation term (default |ref|; None-activation callers pass 0),
    arg: |K v| of the rounded exponent argument.  acc / ev: precomputed terms instead of (sens, S) / (mag, arg)."""
    if acc is None:
        if not isinstance(sens, (list, tuple)):
            sens, S = [sens], [S]
        acc = sum(s * _delta(Si, c) for s, Si in zip(sens, S))
    if ev is None:
        mag = ref.abs() if mag is None else mag
        ev = 4.0 * U * mag
        if arg is not None:
            s0 = sens[0] if isinstance(sens, (list, tuple)) else sens
            ev = ev + s0 * U * arg * LN2
    rest = acc + ev
    st = 0.5 * spacing(ref.abs() + rest, out_dtype)
    if out_dtype == torch.float32:
        st = st + 2.0 ** -126
    return st + rest


def saturated(v, d, act, out_dtype):
    """Elements whose activation rounds to the same 0 / +-1 of out_dtype over [v - d, v + d]; returns (mask, value)."""
    # What the kernel may do differently from the exact function: round K v (u |v| in v), evaluate exp2 / rcp to a relative 2^-22 (2^-20
    # in v is ample); an fp32 result then saturates where 1 + e rounds to 1, up to a factor 2 in e = ln 2 in v from where the exact value
    # does; an fp16 result is the rounding of an fp32 value that is 8u (the evaluation term's ceiling) off at most.
    w = d + 4.0 * U * v.abs() + 2.0 ** -20 + (0.70 if out_dtype == torch.float32 else 0.0)
    e = 8.0 * U if out_dtype == torch.float16 else 0.0
    lo, hi = round_to(_act(v - w, act) - e, out_dtype), round_to(_act(v + w, act) + e, out_dtype)
    m = (lo == hi) & ((lo == 0.0) | (lo.abs() == 1.0))
    return m, lo


# --------------------------------------------------------------------------------------------------------------------------------
# references, one per epilogue mode
# --------------------------------------------------------------------------------------------------------------------------------
def ref_store(v, S, act, out_dtype, res=None, c=None):
    """MODE_STORE: act(v + res).  res: the residual as stored (float64 of the fp16 / fp32 values);
    its addition is a single fp32 rounding and widens the allowance by 2 u |res|."""
    d = _delta(S, c)
    if res is not None:                                           # one or two fp32 roundings of a sum of size <= |v| + |res|, not a k-walk
        v, d = v + res, d + 2.0 * U * res.abs()
    ref = _act(v, act)
    sens = _dact_max(v, d, act)
    acc = sens * d
    if act == ACT_TANH:
        ev = 4.0 * U * (1.0 + ref.abs()) + sens * U * (2.0 * LOG2E * v.abs()) * LN2
    elif act == ACT_SIGMOID:
        ev = 4.0 * U * ref.abs() + sens * U * (LOG2E * v.abs()) * LN2
    else:
        ev = torch.zeros_like(v)                                  # acc + bias (+ res): the roundings of the sum are the accumulation term
    sat, sv = (saturated(v, d, act, out_dtype) if act in (ACT_TANH, ACT_SIGMOID) else (None, None))
    kink = (v.abs() <= d) if act == ACT_RELU else None
    return Ref(ref, acc, ev, sat, sv, kink)


def ref_mul(v, S, h, out_dtype, c=None):
    """MODE_MUL: sigmoid(v) * h, h as stored.  sens = max sigmoid' * |h|.  Saturated: exactly 0 or exactly h."""
    d = _delta(S, c)
    sg = torch.sigmoid(v)
    ref = sg * h
    sens = _dact_max(v, d, ACT_SIGMOID) * h.abs()
    ev = 4.0 * U * ref.abs() + sens * U * (LOG2E * v.abs()) * LN2
    sat, sv = saturated(v, d, ACT_SIGMOID, torch.float32)        # the gate itself is fp32 in every kernel: it must be exactly 0 / 1 there
    return Ref(ref, sens * d, ev, sat, round_to(sv * h, out_dtype))


def ref_gru(v, S, h, z, out_dtype, c=None):
    """MODE_GRU: (1 - z) h + z tanh(v) with h and z as stored (z is an operand here: the buffer the z launch wrote).
    sens = max tanh' * |z|.  Exact only where it cannot depend on the blend's fp32 roundings: z == 0 (h) and z == 1 with tanh
    saturated (+-1); elsewhere in saturation the bound collapses to half a spacing plus 4u M, which is the same statement up to
    double rounding at midpoints."""
    d = _delta(S, c)
    t = torch.tanh(v)
    ref = (1.0 - z) * h + z * t
    sens = _dact_max(v, d, ACT_TANH) * z.abs()
    M = h.abs() + z.abs() * (1.0 + h.abs())
    ev = 4.0 * U * M + sens * U * (2.0 * LOG2E * v.abs()) * LN2
    tsat, tv = saturated(v, d, ACT_TANH, torch.float32)
    # z == 1 goes through h + (tanh - h) in the fused-multiply forms: exactly +-1 once stored as fp16, not necessarily as fp32
    sat = (z == 0.0) | ((z == 1.0) & tsat & (out_dtype == torch.float16))
    sv = torch.where(z == 0.0, h, tv)
    return Ref(ref, sens * d, ev, sat, round_to(sv, out_dtype))


def ref_zq(vz, Sz, vq, Sq, h, out_dtype, c=None):
    """The fused form of demfi_gru_zq: z = sigmoid(vz) stays in fp32 on chip (NOT rounded to fp16), h' = (1 - z) h + z tanh(vq).
    Two accumulators: d h'/d vz = sigmoid'(vz) (tanh(vq) - h), d h'/d vq = z tanh'(vq).
    Exact where z is saturated in fp32: h' == h (z = 0), h' == +-1 (z = 1 and tanh saturated)."""
    dz, dq = _delta(Sz, c), _delta(Sq, c)
    z, t = torch.sigmoid(vz), torch.tanh(vq)
    ref = (1.0 - z) * h + z * t
    zmax = torch.sigmoid(vz + dz)
    sz = _dact_max(vz, dz, ACT_SIGMOID) * ((t - h).abs() + _dact_max(vq, dq, ACT_TANH) * dq)
    sq = _dact_max(vq, dq, ACT_TANH) * zmax
    M = h.abs() + zmax * (1.0 + h.abs())
    ev = 4.0 * U * M + sz * U * (LOG2E * vz.abs()) * LN2 + sq * U * (2.0 * LOG2E * vq.abs()) * LN2
    # the one reciprocal's denominator (e^{2q'} + 1)(1 + e^{-z'}) overflows fp32 once z / (b + 1) < 2^-128; b <= 2^60 by the clamp, so
    # an update gate below 2^-67 is flushed to 0: h' = h there.  Invisible in fp16, an absolute floor for an fp32 store.
    ev = ev + 2.0 ** -67 * (1.0 + h.abs())
    zsat, zv = saturated(vz, dz, ACT_SIGMOID, torch.float32)
    tsat, tv = saturated(vq, dq, ACT_TANH, torch.float32)
    # z == 0 exactly only when e^-z' overflows fp32 (z' < -88.8); below the fp16 resolution of h' the result is h anyway
    z0 = zmax * (1.0 + h.abs()) < 0.25 * spacing(h, out_dtype)
    # z == 1: h' = h + (tanh - h) goes through fp32 roundings of size u (1 + |h|): exactly +-1 once stored as fp16, not as fp32
    sat = z0 | (zsat & (zv == 1.0) & tsat & (out_dtype == torch.float16))
    sv = torch.where(z0, h, tv)
    return Ref(ref, sz * dz + sq * dq, ev, sat, round_to(sv, out_dtype))


# the layers the GPU tests drive (tests/test_gpu_epilogue.py), by the kernel that owns them: cin, cout, kh, kw
LAYERS = {
    'general': (48, 27, 5, 5),        # 5x5 from 48 channels: no persistent kernel takes it
    'c64': (64, 64, 3, 3),
    'thin_sig': (64, 1, 3, 3),        # w_gen_2
    'thin_tanh': (16, 10, 3, 3),
    'thin_none': (32, 5, 3, 3),       # flow_occ.conv2
    'wstream': (192, 64, 7, 7),       # Ch_Reducer
    'sep15': (128, 64, 1, 5),
    'sep51': (128, 64, 5, 1),
}
FRAMES = [(37, 75, 2), (64, 96, 1)]   # ragged, two images / whole tiles


def operands(name, H, W, B, seed=0, wscale=1.0):
    """The designed convolution part of a case: N(0,1) activations, contribution ~ N(0, wscale^2), as fp16 values in float32."""
    cin, cout, kh, kw = LAYERS[name]
    g = torch.Generator().manual_seed(seed * 7919 + cin * 1000 + cout + kh * 10 + kw + H)
    x = torch.randn(B, cin, H, W, generator=g).half().float()
    w = (torch.randn(cout, cin, kh, kw, generator=g) * (wscale / (cin * kh * kw) ** 0.5)).half().float()
    return x, w


H_SPECIAL = [0.0, 1.0, -1.0, 1.0 - 2.0 ** -11, -1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, -1.0 - 2.0 ** -10]


def gru_state(shape, seed=0):
    """GRU state h (fp16 values): tanh of N(0,1), with exactly 0, +-1 and the fp16 neighbours of +-1 strewn in (one element in four)."""
    g = torch.Generator().manual_seed(seed + 99)
    h = torch.tanh(torch.randn(shape, generator=g)).half().float()
    pick = torch.randint(0, 4 * len(H_SPECIAL), shape, generator=g)
    sp = torch.tensor(H_SPECIAL)[pick % len(H_SPECIAL)]
    return torch.where(pick < len(H_SPECIAL), sp, h)


ACC_TAP = 12.0


def operands_acc(name, H, W, B, seed=0):
    """The ACCUMULATOR regime (bias 0): the pre-activation walks the range through the MFMA accumulator instead of the bias.
    A uniform weight scale cannot do it under the quarter-ulp condition: S / sigma_out = 0.64 sqrt(n) (16 for the 640 terms of a 1x5
    128 -> 64 layer), reaching +-45 on these frames needs sigma_out >= 11.5, and C_ACC u S is then 3.9e-4 > 2^-12 on unsaturated
    elements (measured on the CPU for scales 10 .. 12).  So that case's operand scale is shrunk back to 1 -- every tap and channel
    still contributes ~ N(0,1) -- and ONE weight per output channel, on the centre tap of an x channel (the second 64-channel piece, which
    no launch overwrites), is set to ACC_TAP = 12: the accumulator receives 12 x with x ~ N(0,1), i.e. +-45 and beyond where |x| > 3.75,
    while S = S_1 + 12 |x| stays small wherever the output is not saturated.  tests/test_epilogue_ref.py asserts reach and condition."""
    cin, cout, kh, kw = LAYERS[name]
    x, w = operands(name, H, W, B, seed)
    for o in range(cout):
        w[o, 64 + (5 * o + seed) % 64, kh // 2, kw // 2] = ACC_TAP
    return x, w


def assert_inside(got, R, out_dtype, what, cond=True):
    """The per-element assertions every GPU test makes: finite, |got - ref| <= bound outside ReLU's kink (at most 0.5 % excluded),
    saturated elements exact, and (cond) the accumulation term of THIS case below a quarter of the fp16 spacing at 1.0.
    Returns (largest fraction of the bound, its index)."""
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), (what + ': NaN / inf (or the sentinel survived)', int(bad.sum()), 'first at (b,c,y,x)', torch.nonzero(bad)[0].tolist(),
                                 'channels', sorted(set(torch.nonzero(bad)[:, 1].tolist()))[:40])
    if cond:
        assert float(R.acc.max()) < QUARTER_ULP, (what, 'accumulation term above 2^-12: the bound would be vacuous', float(R.acc.max()))
    assert float(R.kink.double().mean()) <= 0.005, what + ': more than 0.5 % of the case sits on the ReLU kink'
    frac = ((got - R.ref).abs() / R.bound(out_dtype)).masked_fill(R.kink, 0.0)
    top = float(frac.max())
    idx = torch.nonzero(frac == frac.max())[0].tolist()
    bad = got[R.sat] != R.sat_val[R.sat]
    assert not bool(bad.any()), (what, 'saturated elements not exact', int(bad.sum()), got[R.sat][bad][:4].tolist(), R.sat_val[R.sat][bad][:4].tolist())
    assert top <= 1.0, (what, top, idx, float(got[tuple(idx)]), float(R.ref[tuple(idx)]))
    return top, idx


def old_rule_accepts(got, ref):
    """The tolerance the kernel tests used before: one number for the whole tensor."""
    return bool((got - ref).abs().max() < 4e-3 * max(1.0, float(ref.abs().max())))


# --------------------------------------------------------------------------------------------------------------------------------
# measuring C_ACC
# --------------------------------------------------------------------------------------------------------------------------------
C_SHAPES = [(64, 64, 3, 3), (128, 64, 1, 5), (128, 64, 5, 1), (192, 64, 7, 7)]


def conv_case(cin, cout, kh, kw, H=12, W=20, seed=0, wscale=1.0):
    """N(0,1) fp16 activations, weights scaled to unit output variance (times wscale), as fp16 values in float32 tensors."""
    g = torch.Generator().manual_seed(seed * 7919 + cin * 1000 + cout + kh * 10 + kw)
    x = torch.randn(1, cin, H, W, generator=g).half().float()
    w = (torch.randn(cout, cin, kh, kw, generator=g) * (wscale / (cin * kh * kw) ** 0.5)).half().float()
    return x, w


def blocked_fp32_conv(x, w, pad):
    """fp32 accumulation in the order of an MFMA k-walk: tap-major, 16-channel blocks, each block's 16 products summed first (fp32,
    pairwise by numpy), then added to the running fp32 accumulator.  x [1,C,H,W], w [O,C,kh,kw] float32 numpy; returns [O,H,W] fp32."""
    _, C, H, W = x.shape
    O, _, kh, kw = w.shape
    xp = np.zeros((C, H + 2 * pad[0], W + 2 * pad[1]), np.float32)
    xp[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x[0]
    acc = np.zeros((O, H, W), np.float32)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, ky:ky + H, kx:kx + W]
            for c0 in range(0, C, 16):
                part = np.einsum('oc,chw->ohw', w[:, c0:c0 + 16, ky, kx], win[c0:c0 + 16], optimize=False).astype(np.float32)
                acc = (acc + part).astype(np.float32)
    return acc


def measure_c(shapes=C_SHAPES, H=12, W=20):
    """max |fp32 sum - fp64 sum| / (u S) per shape for the two summation orders; returns {shape: (torch, blocked)}."""
    out = {}
    for cin, cout, kh, kw in shapes:
        x, w = conv_case(cin, cout, kh, kw, H, W)
        pad = (kh // 2, kw // 2)
        zero = torch.zeros(cout)
        v, S = preact(x, w, zero, pad)
        a = F.conv2d(x, w, None, padding=pad).to(f64)
        b = torch.from_numpy(blocked_fp32_conv(x.numpy(), w.numpy(), pad)).to(f64)[None]
        out[(cin, cout, kh, kw)] = (float(((a - v).abs() / (U * S)).max()), float(((b - v).abs() / (U * S)).max()))
    return out
