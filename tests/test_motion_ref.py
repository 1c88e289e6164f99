"""The float64 motion references (tests/motion_ref.py) against the frozen upstream fixtures and the fp32 oracle, on any host:
what tests/test_gpu_motion.py holds the kernels to is itself pinned here."""
import os

import numpy as np
import pytest
import torch

from oracle import demfi_oracle as O
from tests import motion_ref as R

FAMS = ['zeros', 'ints', 'halves', 'smooth', 'large', 'edges', 'collide']
f32 = np.float32


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _nhwc(a):
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))


def test_warp_maps_equal_the_oracle_maps_on_any_row_subset(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    rows = [0, 3, 4, 11, 23]
    for f in FAMS:
        full = O.backward_warp_maps(g['flo_' + f])
        mine = R.warp_maps(g['flo_' + f])
        sub = R.warp_maps(g['flo_' + f], rows)
        for key in ('ix0', 'iy0', 'valid'):
            assert np.array_equal(mine[key], full[key]), (f, key)
            assert np.array_equal(sub[key], full[key][rows]), (f, key)
        for k in range(4):
            assert np.array_equal(mine['w'][k], full['w'][k]) and np.array_equal(mine['inb'][k], full['inb'][k]), f
            assert np.array_equal(sub['w'][k], full['w'][k][rows]), f


def test_bwarp_matches_the_reference_fixtures(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    for f in FAMS:
        for img in ('img3', 'img8'):
            v, a = R.bwarp(_nhwc(g[img]), g['flo_' + f])
            exp = _nhwc(g['bwarp%s_%s' % (img[3:], f)])
            R.check(exp, v, a, 4, 'bwarp %s %s' % (img, f))


def test_splat_sums_match_the_reference_fixtures(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    for f in FAMS:
        flo = g['flo_' + f]
        val, one, absval, cnt = R.splat_sums(flo, (flo * f32(0.375)).astype(f32))
        # the fixtures are sequential fp32 sums: each add rounds once
        R.check(g['fwarp_img_' + f], val, absval * (cnt + 1), 1, 'splat values ' + f)
        for c in range(2):
            R.check(g['fwarp_one_' + f][c], one, one * (cnt + 1), 1, 'splat weights ' + f)
        assert np.array_equal(cnt == 0, g['fwarp_one_' + f][0] == 0), f


def test_cfr_matches_the_reference_fixtures(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    for i in range(4):
        r = R.cfr(g['cfr%d_f01' % i], g['cfr%d_f10' % i], g['cfr%d_t' % i])
        exp = np.concatenate([g['cfr%d_ft0' % i], g['cfr%d_ft1' % i]], 0)
        R.check(exp, r['ft'], r['bound'], 16, 'cfr fixture %d' % i, exact_zero=np.broadcast_to(~r['hit'], exp.shape))


@pytest.mark.parametrize('t', [1 / 1001, 0.4, 0.5, 1000 / 1001])
def test_cfr_matches_the_oracle_with_far_and_colliding_sources(t):
    rng = np.random.default_rng(7)
    H, W = 40, 72
    f01 = (rng.standard_normal((2, H, W)) * 5).astype(f32)
    f10 = (rng.standard_normal((2, H, W)) * 5).astype(f32)
    f01[:, ::7, ::5] = (rng.standard_normal((2, 6, 15)) * 70).astype(f32)    # far sources (|floor| > 32 at most t)
    f10[0, 10:14, 20:30] = f32(-90.0)                                          # a block that lands on one column band
    f01[:, 5:9, 5:9] = f32(0.5)                                                # many-to-one
    f01[:, 30:] = 0.0
    f01[1, 30:] = f32(-15.0 / f32(t))                                          # both flows move rows 30.. up: a hole at the bottom
    f10[:, 30:] = 0.0
    f10[1, 30:] = f32(-15.0 / (1 - f32(t)))
    r = R.cfr(f01, f10, t)
    a, b = O.cfr_flow_align(torch.from_numpy(f01)[None], torch.from_numpy(f10)[None], torch.tensor(float(f32(t))).view(1, 1, 1, 1))
    exp = torch.cat([a[0], b[0]], 0).numpy()
    # the oracle sums in fp32, up to (count + 1) roundings per element: the bound is loose enough for that, tight enough for a
    # dropped or doubled source
    R.check(exp, r['ft'], r['bound'], 64, 'cfr t=%g' % t, exact_zero=np.broadcast_to(~r['hit'], exp.shape))
    assert (~r['hit']).any() and r['hit'].any()


@pytest.mark.parametrize('t', [1 / 1001, 0.6, 1000 / 1001])
def test_warp_blend_matches_the_oracle(t):
    rng = np.random.default_rng(11)
    H, W, Cc = 21, 70, 8
    A = np.tanh(rng.standard_normal((H, W, Cc))).astype(f32)
    B = np.tanh(rng.standard_normal((H, W, Cc))).astype(f32)
    fa = (rng.standard_normal((2, H, W)) * 4).astype(f32)
    fb = (rng.standard_normal((2, H, W)) * 4).astype(f32)
    fa[:, :, :6] = np.round(fa[:, :, :6])                                       # integer-exact
    fb[0, :3] = f32(500.0)                                                      # entirely out of frame
    logit = (rng.standard_normal((H, W)) * 3).astype(f32)
    logit[::5, ::3] = f32(30.0)
    logit[1::5, ::3] = f32(-90.0)
    r = R.warp_blend(A, fa, B, fb, logit, t)
    tt = torch.tensor(float(f32(t))).view(1, 1, 1, 1)
    nchw = lambda z: torch.from_numpy(np.moveaxis(z, -1, 0).copy())[None]
    exp = O.warp_blend(nchw(A), torch.from_numpy(fa)[None], nchw(B), torch.from_numpy(fb)[None], torch.from_numpy(logit)[None, None], tt)
    R.check(np.moveaxis(exp[0].numpy(), 0, -1), r['out'], r['bound'], 16, 'warp_blend t=%g' % t)
    assert np.abs(torch.sigmoid(torch.from_numpy(logit)).numpy() - r['occ']).max() < 2 * R.EPS32
    rows = [0, 4, 7, 20]
    rs = R.warp_blend(A, fa, B, fb, logit, t, rows)
    assert np.array_equal(rs['out'], r['out'][rows]) and np.array_equal(rs['bound'], r['bound'][rows])


def test_fgac_gather_and_gate_blend_match_the_reference_fixtures(golden_dir, synthetic_sd):
    g = _load(golden_dir, 'fgac_16x24')
    ref = torch.from_numpy(g['ref'])[None]
    src = _nhwc(g['src'])
    name = 'FAC_FB_Module.shared_FGAC'
    with torch.no_grad():
        rk = O.conv(synthetic_sd, name + '.conv_ref_k', ref)
    for fam in ('inrange', 'mixed', 'beyond'):
        fl = g['flow_' + fam]
        # the gather alone against grid_sample (the op the reference calls)
        v, a = R.fgac_gather(_nhwc(g['ref']), fl)
        exp = O.fgac_sample(ref, torch.from_numpy(fl)[None])[0].numpy()
        R.check(np.moveaxis(exp, 0, -1), v, a, 4, 'fgac gather ' + fam)
        assert np.array_equal(R.fgac_gather(_nhwc(g['ref']), fl, [2, 15])[0], v[[2, 15]])
        # the whole FGAC: fp64 gather of conv_ref_k -> fusion conv -> fp64 gate blend with the reference's gate == its output
        e, _ = R.fgac_gather(_nhwc(rk[0].numpy()), fl)
        with torch.no_grad():
            e = O.conv(synthetic_sd, name + '.fusion', torch.from_numpy(np.moveaxis(e, -1, 0).astype(f32))[None])[0].numpy()
        out, _ = R.gate_blend(g['gate_' + fam][0], src, _nhwc(e))
        assert np.abs(np.moveaxis(out, -1, 0) - g['out_' + fam]).max() < 1e-5, fam


def test_check_is_per_element_and_catches_unwritten_outputs():
    ref = np.array([1.0, 1e-3, 0.0])
    bound = np.abs(ref)
    R.check(ref * (1 + 2 * R.EPS32), ref, bound, 4, 'ok')
    with pytest.raises(AssertionError):
        R.check(ref + 1e-6, ref, bound, 4, 'a small element off by a large element\'s tolerance')
    with pytest.raises(AssertionError):
        R.check([1.0, np.nan, 0.0], ref, bound, 4, 'NaN sentinel')
    with pytest.raises(AssertionError):
        R.check([1.0, 1e-3, 1e-30], ref, bound + 1, 4, 'not exactly zero', exact_zero=np.array([False, False, True]))
    assert R.fp16_ulp(1.0) == 2.0 ** -10 and R.fp16_ulp(1e-9) == 2.0 ** -24
    R.check(np.float16(0.1), 0.1, 0.0, 4, 'fp16 rounding', ulp16=True)
