"""CPU tests of tests/epilogue_ref.py: honest fp32 emulations of the epilogue formulas stay inside the bound over the whole value
grid, every listed mutant leaves it (or turns non-finite), the accumulation constant is what the reference measures, and the
accumulation term of every GPU case stays below a quarter of the fp16 spacing at 1.0.  No GPU, no HIP."""
import numpy as np
import pytest
import torch

from tests import epilogue_ref as E

f32, f64 = np.float32, np.float64
K_SIG, K_TANH = f32(-1.4426950408889634), f32(2.8853900817779268)
H, W = 10, 24


def _fma(a, b, c):
    """fp32 fused multiply-add: exact product and sum in float64 (53 bits hold a 24 x 24 bit product), one rounding."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _rcp(x):
    with np.errstate(divide='ignore', over='ignore'):
        return (f32(1.0) / x).astype(f32)


def _exp2(x):
    with np.errstate(over='ignore', under='ignore'):
        return np.exp2(x.astype(f32)).astype(f32)


def _store(v, out_dtype, trunc=False):
    """fp32 -> out_dtype (round to nearest even; trunc: toward zero, the mutant), returned as a float64 tensor."""
    if out_dtype == torch.float32:
        return torch.from_numpy(v.astype(f64))
    r = v.astype(np.float16)
    if trunc:
        a = np.abs(r.astype(f32)) > np.abs(v)
        r = np.where(a, np.nextafter(r, np.float16(0.0)), r)
    return torch.from_numpy(r.astype(f64))


def _layer(name, k, seed=0, wscale=1.0, bias=None):
    """fp32 accumulator (torch's fp32 conv2d, no bias) + the grid bias of rotation k, and the fp64 pre-activation / S."""
    cin, cout, kh, kw = E.LAYERS[name]
    x, w = E.operands(name, H, W, 1, seed, wscale)
    b = E.grid_bias(cout, k) if bias is None else bias
    pad = (kh // 2, kw // 2)
    acc = torch.nn.functional.conv2d(x, w, None, padding=pad).numpy()
    v, S = E.preact(x, w, b, pad)
    return acc, b.numpy().reshape(1, -1, 1, 1), v, S, x, w


# ---- honest emulations of the four formula families ---------------------------------------------------------------------------
def emu_sigmoid(acc, b):                                   # common.h: rcp(1 + exp2(K x)), x = acc + bias in fp32
    return _rcp(f32(1.0) + _exp2(K_SIG * (acc + b).astype(f32)))


def emu_tanh(acc, b):
    return (f32(1.0) - f32(2.0) * _rcp(f32(1.0) + _exp2(K_TANH * (acc + b).astype(f32)))).astype(f32)


def emu_sigmoid_prescaled(acc, b, K=K_SIG):                # conv_sep.hip: the host pre-multiplies the bias: 2^(K acc + K b), one fma
    return _rcp(f32(1.0) + _exp2(_fma(acc, np.full_like(acc, K), (b * K).astype(f32) + np.zeros_like(acc))))


def emu_gru_prescaled(acc, b, h16, z16):                   # conv_sep.hip MODE_GRU: q = 1 - 2 rcp(..), dlt = q - h, h + z dlt
    q = _fma(np.full_like(acc, f32(-2.0)), emu_sigmoid_prescaled(acc, b, K_TANH), np.ones_like(acc))
    dlt = (q - h16).astype(f32)
    return _fma(z16, dlt, h16)


def emu_mul_packed(acc, b, h16):                           # gru.hip demfi_gru_r: bias inside the accumulator, packed pairs, fma(sg, h, 0)
    e = (_exp2(((acc + b).astype(f32) * K_SIG).astype(f32)) + f32(1.0)).astype(f32)
    return (_rcp(e) * h16).astype(f32)


def emu_zq(accz, bz, accq, bq, h16, clamp=True, z_fp16=False):
    """gru.hip demfi_gru_zq: a = e^-z' + 1, b = e^2q' (exponent clamped at 60), r = 1 / ((b + 1) a), h' = h + ((b - 1) - h (b + 1)) r."""
    ez = (accz * K_SIG + (bz * K_SIG).astype(f32)).astype(f32)
    eq = (accq * K_TANH + (bq * K_TANH).astype(f32)).astype(f32)
    if clamp:
        eq = np.minimum(eq, f32(60.0))
    with np.errstate(over='ignore', invalid='ignore'):
        av = (_exp2(ez) + f32(1.0)).astype(f32)
        bv = _exp2(eq)
        if z_fp16:                                         # the mutant: z leaves the chip as fp16 and the blend reads it back
            z = _rcp(av).astype(np.float16).astype(f32)
            q = ((bv - f32(1.0)) * _rcp(bv + f32(1.0))).astype(f32)
            return _fma(z, (q - h16).astype(f32), h16)
        r = _rcp(((bv + f32(1.0)) * av).astype(f32))
        n = _fma(-(bv + f32(1.0)), h16 + np.zeros_like(bv), bv - f32(1.0))
        return _fma(n, r, h16 + np.zeros_like(bv))


def _inside(got, R, out_dtype, what):
    assert torch.isfinite(got).all(), what + ': non-finite'
    frac = ((got - R.ref).abs() / R.bound(out_dtype)).max().item()
    assert frac <= 1.0, (what, frac)
    sat_ok = bool((got[R.sat] == R.sat_val[R.sat]).all())
    assert sat_ok, what + ': a saturated element is not exact'
    return frac


def _violates(got, R, out_dtype):
    if not torch.isfinite(got).all():
        return True
    return bool(((got - R.ref).abs() > R.bound(out_dtype)).any()) or not bool((got[R.sat] == R.sat_val[R.sat]).all())


def _gru_operands(shape, seed=0):
    h = E.gru_state(shape, seed)
    g = torch.Generator().manual_seed(seed + 5)
    z = torch.rand(shape, generator=g).half().float()
    z = torch.where(torch.rand(shape, generator=g) < 0.2, torch.round(z), z)         # exactly 0 and 1 as well
    return h, z


# ---- the constants ------------------------------------------------------------------------------------------------------------
def test_abi_constants_and_grid():
    from demfi_amd import _lib as L
    assert (E.ACT_NONE, E.ACT_RELU, E.ACT_TANH, E.ACT_SIGMOID) == (L.ACT_NONE, L.ACT_RELU, L.ACT_TANH, L.ACT_SIGMOID)
    assert len(E.GRID) == 38 and set(abs(g) for g in E.GRID) >= {0.0, 1e-4, 20.7, 20.9, 44.0, 45.0, 88.0, 89.0, 1e4}


def test_rotations_put_every_value_on_every_lane_half_and_subtile():
    """Plain packed order: cout = 32 s + 8 g + 4 hi + j; cout_perm order of the 64-channel kernels: channel = 32 s + 16 m2 + 8 hi + j.
    Over the rotations every grid value must meet both lane halves (both orders) and both 32-cout sub-tiles, and every register quad."""
    seen = {}
    for k in E.ROTATIONS:
        for c in range(64):
            i = (7 * c + k) % 38
            seen.setdefault(i, set()).update({('hi', (c >> 2) & 1), ('hip', (c >> 3) & 1), ('s', c >> 5), ('g', (c >> 3) & 3)})
    full = {('hi', 0), ('hi', 1), ('hip', 0), ('hip', 1), ('s', 0), ('s', 1)} | {('g', g) for g in range(4)}
    assert all(seen[i] == full for i in range(38)), {i: full - seen[i] for i in range(38) if seen[i] != full}


def test_accumulation_constant_is_what_the_reference_measures():
    m = E.measure_c()
    for shp, (a, b) in m.items():
        print('c ratio %-18s torch fp32 conv2d %.2f   16-channel blocks tap-major %.2f' % (shp, a, b))
    top = max(max(v) for v in m.values())
    print('largest ratio %.2f, C_ACC = %.1f (8 x the recorded maximum %.2f)' % (top, E.C_ACC, max(max(v) for v in E.MEASURED_C.values())))
    assert E.C_ACC >= 8.0 * max(max(v) for v in E.MEASURED_C.values())
    # torch may sum in another order on another CPU: the constant must keep a margin of at least 4 over whatever this machine shows
    assert top <= E.C_ACC / 4.0, top


@pytest.mark.parametrize('name', sorted(E.LAYERS))
def test_accumulation_term_below_a_quarter_ulp_for_every_gpu_case(name):
    """Condition of the issue: sens * C_ACC * u * S < 2^-12 on every element of every case the GPU tests run (bias regime, every rotation,
    on the ragged two-image frame; S does not depend on the frame beyond its border)."""
    cin, cout, kh, kw = E.LAYERS[name]
    Hh, Ww, B = (16, 32, 1) if name == 'wstream' else (37, 75, 1)
    x, w = E.operands(name, Hh, Ww, B)
    act = {'thin_sig': E.ACT_SIGMOID, 'thin_none': E.ACT_NONE, 'sep15': E.ACT_SIGMOID, 'sep51': E.ACT_SIGMOID}.get(name, E.ACT_TANH)
    worst = 0.0
    for k in E.ROTATIONS:
        b = E.grid_bias(cout, k) if act != E.ACT_NONE else torch.zeros(cout)
        v, S = E.preact(x, w, b, (kh // 2, kw // 2))
        for a in ((act, E.ACT_TANH) if name.startswith('sep') else (act,)):
            R = E.ref_store(v, S, a, torch.float16)
            worst = max(worst, float(R.acc.max()))
    print('%-10s largest accumulation term %.3e (limit 2^-12 = %.3e)' % (name, worst, E.QUARTER_ULP))
    assert worst < E.QUARTER_ULP


@pytest.mark.parametrize('name', ['sep15', 'sep51'])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_accumulator_regime_reaches_the_range_and_keeps_the_condition(name, H, W, B):
    """Second regime (bias 0, the ACCUMULATOR walks the range; epilogue_ref.operands_acc says why one tap per output channel carries it
    instead of a uniform weight scale): on the frames and seeds of the GPU test, +-45 is reached and sens * C_ACC * u * S < 2^-12 holds
    for both activations.  The GPU test asserts the same on the Ref objects it builds (assert_inside), gated modes included."""
    cin, cout, kh, kw = E.LAYERS[name]
    for seed in (10, 20, 30):
        x, w = E.operands_acc(name, H, W, B, seed=seed)
        x[:, :64] = E.gru_state((B, 64, H, W), 0)
        v, S = E.preact(x, w, torch.zeros(cout), (kh // 2, kw // 2))
        assert float(v.max()) > 45.0 and float(v.min()) < -45.0, (float(v.min()), float(v.max()))
        for a in (E.ACT_TANH, E.ACT_SIGMOID):
            worst = float(E.ref_store(v, S, a, torch.float16).acc.max())
            print('%-6s %dx%dx%d seed %d act %d: range %.1f .. %.1f, largest accumulation term %.3e' % (name, H, W, B, seed, a, float(v.min()), float(v.max()), worst))
            assert worst < E.QUARTER_ULP


# ---- honest emulations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_dtype', [torch.float16, torch.float32])
def test_honest_emulations_stay_inside_the_bound(out_dtype):
    top = {}
    for k in E.ROTATIONS:
        acc, b, v, S, x, w = _layer('sep15', k)
        h, z = _gru_operands(v.shape, k)
        hn, zn = h.numpy(), z.numpy()
        h64, z64 = h.to(torch.float64), z.to(torch.float64)
        runs = [
            ('rcp(1+exp2) sigmoid', emu_sigmoid(acc, b), E.ref_store(v, S, E.ACT_SIGMOID, out_dtype)),
            ('rcp(1+exp2) tanh', emu_tanh(acc, b), E.ref_store(v, S, E.ACT_TANH, out_dtype)),
            ('pre-scaled bias sigmoid', emu_sigmoid_prescaled(acc, b), E.ref_store(v, S, E.ACT_SIGMOID, out_dtype)),
            ('pre-scaled bias mul', (emu_sigmoid_prescaled(acc, b) * hn).astype(f32), E.ref_mul(v, S, h64, out_dtype)),
            ('pre-scaled bias gru', emu_gru_prescaled(acc, b, hn, zn), E.ref_gru(v, S, h64, z64, out_dtype)),
            ('packed-pair mul', emu_mul_packed(acc, b, hn), E.ref_mul(v, S, h64, out_dtype)),
        ]
        # zq: an independent rotation for q' so that the corners (z' << 0, q' >> 0) ... all occur
        for kq in (3, 17):
            accq, bq, vq, Sq, _, _ = _layer('sep51', kq, seed=1)
            runs.append(('fused zq', emu_zq(acc, b, accq, bq, hn), E.ref_zq(v, S, vq, Sq, h64, out_dtype)))
        for what, got, R in runs:
            top[what] = max(top.get(what, 0.0), _inside(_store(got, out_dtype), R, out_dtype, what))
    for what, fr in top.items():
        print('%-8s %-26s largest fraction of the bound used %.3f' % (str(out_dtype)[6:], what, fr))
    assert max(top.values()) <= 1.0


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _plain_case(name='c64'):
    cin, cout, kh, kw = E.LAYERS[name]
    g = torch.Generator().manual_seed(4)
    return _layer(name, 0, bias=(torch.randn(cout, generator=g) * 0.1))


def test_mutant_fp16_store_by_truncation():
    for name in ('c64', 'sep15', 'wstream'):
        acc, b, v, S, x, w = _plain_case(name)
        R = E.ref_store(v, S, E.ACT_NONE, torch.float16)
        honest = (acc + b).astype(f32)
        _inside(_store(honest, torch.float16), R, torch.float16, 'honest none ' + name)
        mut = _store(honest, torch.float16, trunc=True)
        share = float(((mut - R.ref).abs() > R.bound(torch.float16)).double().mean())
        print('%-8s truncating store: %.2f %% of the elements leave the bound; the old rule accepts it: %s' % (name, 100 * share, E.old_rule_accepts(mut, R.ref)))
        assert _violates(mut, R, torch.float16)
        assert E.old_rule_accepts(mut, R.ref)               # why the new bound exists


def test_mutant_textbook_tanh():
    acc, b, v, S, x, w = _layer('sep15', 0)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp((f32(2.0) * (acc + b)).astype(f32)).astype(f32)
        mut = ((e - f32(1.0)) / (e + f32(1.0))).astype(f32)
    assert _violates(_store(mut, torch.float16), E.ref_store(v, S, E.ACT_TANH, torch.float16), torch.float16)
    assert not np.isfinite(mut).all()                       # NaN from x = 45


def _zq_case():
    acc, b, v, S, _, _ = _layer('sep15', 0)
    accq, bq, vq, Sq, _, _ = _layer('sep51', 3, seed=1)
    h = E.gru_state(v.shape, 0)
    return acc, b, accq, bq, h.numpy(), E.ref_zq(v, S, vq, Sq, h.to(torch.float64), torch.float16)


def test_mutant_zq_without_the_clamp():
    acc, b, accq, bq, hn, R = _zq_case()
    _inside(_store(emu_zq(acc, b, accq, bq, hn), torch.float16), R, torch.float16, 'honest zq')
    mut = emu_zq(acc, b, accq, bq, hn, clamp=False)
    assert not np.isfinite(mut).all() and _violates(_store(mut, torch.float16), R, torch.float16)


def test_mutant_zq_with_z_rounded_to_fp16():
    """demfi_gru_zq keeps z in fp32 (see ref_zq); a form that rounds z to fp16 on the way is the mutant."""
    acc, b, accq, bq, hn, R = _zq_case()
    assert _violates(_store(emu_zq(acc, b, accq, bq, hn, z_fp16=True), torch.float16), R, torch.float16)


def test_mutant_one_dropped_input_channel_at_one_tap():
    acc, b, v, S, x, w = _plain_case('c64')
    R = E.ref_store(v, S, E.ACT_NONE, torch.float16)
    w2 = w.clone()
    w2[:, 17, 0, 2] = 0.0
    mut = (torch.nn.functional.conv2d(x, w2, None, padding=1).numpy() + b).astype(f32)
    got = _store(mut, torch.float16)
    # the old rule does NOT accept this one on this shape (one term is ~0.04 |x|, above 4e-3 max|ref|): only the bound is asserted
    print('dropped term: largest error %.3e, old rule accepts: %s' % (float((got - R.ref).abs().max()), E.old_rule_accepts(got, R.ref)))
    assert _violates(got, R, torch.float16)
    # one output channel only, a weight of that tap small enough for the old rule: the bound still sees it
    w3 = w.clone()
    o = int((w[:, 17, 0, 2].abs() - 0.004).abs().argmin())
    w3[o, 17, 0, 2] = 0.0
    got3 = _store((torch.nn.functional.conv2d(x, w3, None, padding=1).numpy() + b).astype(f32), torch.float16)
    print('dropped term, one cout (w = %.2e): old rule accepts: %s' % (float(w[o, 17, 0, 2]), E.old_rule_accepts(got3, R.ref)))
    assert _violates(got3, R, torch.float16)
    assert E.old_rule_accepts(got3, R.ref)


def test_mutant_bias_after_the_activation():
    acc, b, v, S, x, w = _layer('sep15', 0)
    mut = (emu_tanh(acc, np.zeros_like(b)) + b).astype(f32)
    assert _violates(_store(mut, torch.float32), E.ref_store(v, S, E.ACT_TANH, torch.float32), torch.float32)
    g = torch.Generator().manual_seed(4)
    acc, b, v, S, x, w = _layer('sep15', 0, bias=torch.randn(64, generator=g) * 0.1)       # also with the suite's small biases
    mut = (emu_tanh(acc, np.zeros_like(b)) + b).astype(f32)
    assert _violates(_store(mut, torch.float16), E.ref_store(v, S, E.ACT_TANH, torch.float16), torch.float16)


def test_mutant_z_and_one_minus_z_swapped():
    acc, b, v, S, x, w = _layer('sep15', 0)
    h, z = _gru_operands(v.shape)
    R = E.ref_gru(v, S, h.to(torch.float64), z.to(torch.float64), torch.float16)
    _inside(_store(emu_gru_prescaled(acc, b, h.numpy(), z.numpy()), torch.float16), R, torch.float16, 'honest gru')
    mut = emu_gru_prescaled(acc, b, h.numpy(), (1.0 - z).numpy().astype(f32))
    assert _violates(_store(mut, torch.float16), R, torch.float16)


def test_mutant_sigmoid_sign_flipped_on_one_output_channel():
    acc, b, v, S, x, w = _layer('sep15', 0)
    R = E.ref_store(v, S, E.ACT_SIGMOID, torch.float16)
    mut = emu_sigmoid(acc, b)
    mut[:, 41] = emu_sigmoid(-acc, -b)[:, 41]
    assert _violates(_store(mut, torch.float16), R, torch.float16)
    assert not _violates(_store(emu_sigmoid(acc, b), torch.float16), R, torch.float16)
