"""The fused epilogues of the convolution kernels over their whole input range, per element, against float64.

Every kernel runs the designed cases of tests/epilogue_ref.py: random fp16 operands with a contribution ~ N(0,1) (all taps and
channels matter) and an fp32 bias that walks GRID -- 0, the cancellation region, both sides of fp16 / fp32 saturation, of the clamp
of demfi_gru_zq (q' = 20.79), of e^{2x} and e^{x} overflow, up to 1e4 -- rotated so that every value meets every lane half, register
quad and 32-cout sub-tile (epilogue_ref.ROTATIONS).  Assertions per element: |got - ref| <= bound (storage + accumulation +
evaluation, derived in epilogue_ref, nothing tuned on a GPU), no NaN / inf anywhere (outputs are pre-filled with a sentinel, ragged
tiles included), saturated elements EXACTLY 0 / +-1 / h.  Each test keeps the routing asserts of tests/test_gpu_kernels.py, so it
provably reaches the kernel it names.  Every test prints the largest fraction of the bound it used and where (run with -s)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from demfi_amd.engine import Plan, _Dst              # noqa: E402
from tests import epilogue_ref as E                  # noqa: E402

DEV = 'cuda:0'
f64 = torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nchw(t):
    return t.permute(0, 3, 1, 2).to(f64).cpu()


def _put(buf, x):
    """[B,C,H,W] CPU values -> the NHWC buffer."""
    buf.copy_(x.permute(0, 2, 3, 1).to(buf.dtype).to(DEV))


def _check(what, got, R, out_dtype, bias=None, cond=True):
    """got [B,C,H,W] float64.  bias [C]: the grid value of each channel, for the report.  cond: see epilogue_ref.assert_inside."""
    top, idx = E.assert_inside(got, R, out_dtype, what, cond)
    at = '' if bias is None else ' at bias %g' % float(bias[idx[1]])
    print('EPI %-44s %-7s fraction of the bound %.3f%s (b,c,y,x = %s), %d exact-saturated elements'
          % (what, str(out_dtype)[6:], top, at, idx, int(R.sat.sum())))


def _grid_residual(b, B, H, W, g):
    """A residual [B,C,H,W] that carries grid magnitudes with the SIGN of its channel's bias: bias + residual then saturates harder and
    never cancels (a bias of 1e4 against a residual of -1e4 would leave an unsaturated element with S ~ 1e4, where no fp32 sum is
    accurate to 2^-12 and the bound would be vacuous)."""
    mag = torch.tensor(E.GRID).abs()[torch.randint(0, 38, (B, len(b), H, W), generator=g)]
    return mag * torch.where(b < 0, -1.0, 1.0).view(1, -1, 1, 1)


def _conv_layer(pl, name, H, W, B, k, srcs_of, dsts_of, bias=None, seed=0):
    """One launch of LAYERS[name] on the designed operands with the grid bias of rotation k.  Returns (x, w, bias, desc index)."""
    cin, cout, kh, kw = E.LAYERS[name]
    x, w = E.operands(name, H, W, B, seed)
    b = E.grid_bias(cout, k) if bias is None else bias
    xb = pl._fat(H, W, cin, B)
    _put(xb, x)
    if pl.dtype == torch.float32:
        x = xb.permute(0, 3, 1, 2).float().cpu()
    pl.conv([], name, srcs_of(xb), dsts_of(), H, W, batch=B, weight=w, bias=b)
    return x, w, b, len(pl._descs) - 1


# ------------------------------------------------------------------------------------------------------------------------------
# general kernel: fp32 and fp16, TANH / SIGMOID to fat NHWC, TANH to thin planes with a residual
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_general_kernel_tanh_sigmoid_fat_and_thin_with_residual(dtype, H, W, B):
    cin, cout, kh, kw = E.LAYERS['general']                # 27 couts: 12 tanh fat | 12 sigmoid fat | 3 tanh planes + residual
    for k in E.ROTATIONS:
        pl = Plan(H, W, dtype, DEV)
        o_t, o_s = pl._fat(H, W, 12, B), pl._fat(H, W, 12, B)
        o_p = torch.full((B * 3, H, W), -77.0, dtype=torch.float32, device=DEV)
        g = torch.Generator().manual_seed(k)
        resv = _grid_residual(E.grid_bias(cout, k)[24:], B, H, W, g).float()                    # the residual carries grid values too
        r_p = resv.view(B * 3, H, W).to(DEV).contiguous()
        sb = 3 * H * W if B > 1 else 0
        x, w, b, i = _conv_layer(pl, 'general', H, W, B, k, lambda xb: [pl.fsrc(xb, 0)],
                                 lambda: [_Dst(pl.fview(o_t), range(0, 12), L.ACT_TANH), _Dst(pl.fview(o_s), range(12, 24), L.ACT_SIGMOID),
                                          _Dst(pl.tview(o_p, 0, sb=sb), range(24, 27), L.ACT_TANH, res=pl.tview(r_p, 0, sb=sb))])
        assert pl._descs[i].cout_perm == 0                  # no persistent kernel's packing: the general kernel
        pl._upload()
        o_t.fill_(float('nan')); o_s.fill_(float('nan'))
        pl.launch_conv(i, _stream())
        torch.cuda.synchronize()
        v, S = E.preact(x, w, b, (kh // 2, kw // 2))
        tag = 'general %s k=%d %dx%dx%d ' % (str(dtype)[6:], k, H, W, B)
        _check(tag + 'tanh fat', _nchw(o_t), E.ref_store(v[:, :12], S[:, :12], E.ACT_TANH, dtype), dtype, b[:12])
        _check(tag + 'sigmoid fat', _nchw(o_s), E.ref_store(v[:, 12:24], S[:, 12:24], E.ACT_SIGMOID, dtype), dtype, b[12:24])
        _check(tag + 'tanh planes + res', o_p.view(B, 3, H, W).to(f64).cpu(),
               E.ref_store(v[:, 24:], S[:, 24:], E.ACT_TANH, torch.float32, res=resv.to(f64)), torch.float32, b[24:])


# ------------------------------------------------------------------------------------------------------------------------------
# conv_c64.hip: 64 -> 64 3x3, tanh after the residual add; the residual carries grid values, so the sum saturates
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_c64_tanh_after_residual(H, W, B):
    for k in E.ROTATIONS:
        pl = Plan(H, W, torch.float16, DEV)
        out, res = pl._fat(H, W, 64, B), pl._fat(H, W, 64, B)
        g = torch.Generator().manual_seed(k + 1)
        resv = _grid_residual(E.grid_bias(64, k), B, H, W, g).half().float()
        _put(res, resv)
        x, w, b, i = _conv_layer(pl, 'c64', H, W, B, k, lambda xb: [pl.fsrc(xb, 0)],
                                 lambda: [_Dst(pl.fview(out), range(64), L.ACT_TANH, res=pl.fview(res))])
        assert pl._descs[i].cout_perm == 1                  # packed for the persistent 64-channel kernel
        pl._upload()
        out.fill_(float('nan'))
        pl.launch_conv(i, _stream())
        torch.cuda.synchronize()
        v, S = E.preact(x, w, b, (1, 1))
        _check('c64 tanh(acc + b + res) k=%d %dx%dx%d' % (k, H, W, B), _nchw(out),
               E.ref_store(v, S, E.ACT_TANH, torch.float16, res=resv.to(f64)), torch.float16, b)


def test_c64_tanh_after_residual_of_the_opposite_sign():
    """The case _grid_residual avoids, once: residual signs independent of the bias, so a bias of 1e4 meets a residual of -1e4 and the
    sum is moderate.  S ~ 1e4 there, the allowance C_ACC u S is of the order 1e-2 on those few elements and the 2^-12 condition cannot hold
    (cond=False) -- what this case still pins is that the cancelled sum is finite, lands within that allowance of tanh of the exact sum,
    and that every element that stays saturated is exact."""
    H, W, B = 37, 75, 2
    pl = Plan(H, W, torch.float16, DEV)
    out, res = pl._fat(H, W, 64, B), pl._fat(H, W, 64, B)
    g = torch.Generator().manual_seed(77)
    resv = torch.tensor(E.GRID)[torch.randint(0, 38, (B, 64, H, W), generator=g)].half().float()
    _put(res, resv)
    x, w, b, i = _conv_layer(pl, 'c64', H, W, B, 0, lambda xb: [pl.fsrc(xb, 0)], lambda: [_Dst(pl.fview(out), range(64), L.ACT_TANH, res=pl.fview(res))])
    assert pl._descs[i].cout_perm == 1
    pl._upload()
    out.fill_(float('nan'))
    pl.launch_conv(i, _stream())
    torch.cuda.synchronize()
    v, S = E.preact(x, w, b, (1, 1))
    cancel = ((v + resv.to(f64)).abs() < 8.0) & (resv.abs() >= 8.5)
    assert int(cancel.sum()) > 1000
    _check('c64 tanh(acc + b + res), opposite signs', _nchw(out), E.ref_store(v, S, E.ACT_TANH, torch.float16, res=resv.to(f64)), torch.float16, b, cond=False)


# ------------------------------------------------------------------------------------------------------------------------------
# narrow kernel, thin epilogue: planar fp32 stores
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,act,dsts', [('thin_sig', L.ACT_SIGMOID, [(1, False)]), ('thin_tanh', L.ACT_TANH, [(8, True), (2, False)]),
                                           ('thin_none', L.ACT_NONE, [(5, True)])])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_narrow_thin_epilogue(name, act, dsts, H, W, B):
    cin, cout, kh, kw = E.LAYERS[name]
    for k in E.ROTATIONS:
        pl = Plan(H, W, torch.float16, DEV)
        outs, ress = [], []
        g = torch.Generator().manual_seed(k + 2)
        cc = 0
        for n, has_res in dsts:
            outs.append(torch.full((B * n, H, W), -77.0, dtype=torch.float32, device=DEV))
            if not has_res:
                ress.append(None)
            elif act == L.ACT_NONE:                         # a large residual: planar fp32 stores at large magnitude
                ress.append((torch.randn((B * n, H, W), generator=g) * 3.0e4).to(DEV))
            else:
                ress.append(_grid_residual(E.grid_bias(cout, k)[cc:cc + n], B, H, W, g).float().view(B * n, H, W).to(DEV))
            cc += n

        def dsts_of():
            D, c = [], 0
            for (n, has_res), o, r in zip(dsts, outs, ress):
                sb = n * H * W if B > 1 else 0
                D.append(_Dst(pl.tview(o, 0, sb=sb), range(c, c + n), act, res=pl.tview(r, 0, sb=sb) if has_res else None))
                c += n
            return D
        bias = None if act != L.ACT_NONE else torch.randn(cout, generator=g) * 0.1
        x, w, b, i = _conv_layer(pl, name, H, W, B, k, lambda xb: [pl.fsrc(xb, 0)], dsts_of, bias=bias)
        d = pl._descs[i]
        # what the dispatcher asks of the narrow kernel's thin epilogue: one chunk, one 32-cout sub-tile routed per octet, no cout_perm
        assert d.n_chunks == 1 and d.nco == 1 and d.cout_pad == 32 and d.cout_perm == 0 and d.rec_bytes in (32, 64, 128)
        pl._upload()
        pl.launch_conv(i, _stream())
        torch.cuda.synchronize()
        v, S = E.preact(x, w, b, (1, 1))
        c0 = 0
        for (n, has_res), o, r in zip(dsts, outs, ress):
            R = E.ref_store(v[:, c0:c0 + n], S[:, c0:c0 + n], act, torch.float32, res=r.view(B, n, H, W).to(f64).cpu() if has_res else None)
            # ACT_NONE at |value| ~ 1e5: the allowance is relative to that magnitude, the 2^-12 condition is about activations
            _check('narrow thin %s k=%d %dx%dx%d couts %d..%d' % (name, k, H, W, B, c0, c0 + n), o.view(B, n, H, W).to(f64).cpu(), R, torch.float32,
                   b[c0:c0 + n], cond=act != L.ACT_NONE)
            c0 += n


# ------------------------------------------------------------------------------------------------------------------------------
# conv_wstream.hip: Ch_Reducer's tanh
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,B', [(37, 75, 2)])
def test_wstream_7x7_tanh(H, W, B):
    x, w = E.operands('wstream', H, W, B)
    v0, S0 = E.preact(x, w, torch.zeros(64), (3, 3))       # the fp64 convolution once; the rotations only change the bias
    for k in E.ROTATIONS:
        pl = Plan(H, W, torch.float16, DEV)
        out = pl._fat(H, W, 64, B)
        _, _, b, i = _conv_layer(pl, 'wstream', H, W, B, k, lambda xb: [pl.fsrc(xb, 0, 0, 64), pl.fsrc(xb, 64, 64, 64), pl.fsrc(xb, 128, 128, 64)],
                                 lambda: [_Dst(pl.fview(out), range(64), L.ACT_TANH)])
        assert pl._descs[i].cout_perm == 1, 'the layer must be packed for the streamed-weight kernel'
        pl._upload()
        out.fill_(float('nan'))
        pl.launch_conv(i, _stream())
        torch.cuda.synchronize()
        bb = b.to(f64).view(1, -1, 1, 1)
        _check('wstream 7x7 tanh k=%d %dx%dx%d' % (k, H, W, B), _nchw(out), E.ref_store(v0 + bb, S0 + bb.abs(), E.ACT_TANH, torch.float16),
               torch.float16, b)


# ------------------------------------------------------------------------------------------------------------------------------
# SepConvGRU half-step: conv_sep.hip (fused z|r launch, q launch) and gru.hip (demfi_gru_r, demfi_gru_zq), both orientations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['bias', 'acc'])
@pytest.mark.parametrize('kh,kw', [(1, 5), (5, 1)])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_sep_gru_epilogues_conv_sep_and_gru_hip(kh, kw, H, W, B, regime):
    """z', r' and q' get INDEPENDENT rotations of the grid, so the corners (z' << 0, q' >> 0), ... all occur; h holds exactly 0, +-1
    and the fp16 neighbours of +-1.  regime 'bias': the fp32 bias walks the grid.  regime 'acc': bias 0, the ACCUMULATOR walks the range
    (epilogue_ref.operands_acc) -- conv_sep.hip's pre-scaled-bias fma and gru.hip's bias-in-accumulator start take other paths for it.
    Both implementations are checked against float64 under the bound, and against each other: they compute the same function of the
    same operands (both q launches read the r*h that demfi_gru_r stored), so
      r*h:  |gru_r - MODE_MUL| <= 2 bound(r*h)                                 (one fp16 spacing plus ~1e-5),
      h':   |zq - MODE_GRU|    <= bound(zq) + bound(GRU) + bound(z) |tanh(q') - h|,
    the last term because the fused form blends with z in fp32 and the two-launch form with the fp16 z it stored."""
    name = 'sep15' if kw == 5 else 'sep51'
    pad = (kh // 2, kw // 2)
    T16 = torch.float16
    ops = E.operands if regime == 'bias' else E.operands_acc
    for n, (kz, kr, kq) in enumerate([(0, 5, 23), (1, 30, 9), (16, 12, 2)] if regime == 'bias' else [(0, 0, 0)]):
        pl = Plan(H, W, T16, DEV)
        h, xx = pl._fat(H, W, 64, B), pl._fat(H, W, 64, B)
        hx, wz = ops(name, H, W, B, seed=10 + n)
        _, wr = ops(name, H, W, B, seed=20 + n)
        _, wq = ops(name, H, W, B, seed=30 + n)
        hx[:, :64] = E.gru_state((B, 64, H, W), n)
        _put(h, hx[:, :64]); _put(xx, hx[:, 64:])
        if regime == 'bias':
            bz, br, bq = E.grid_bias(64, kz), E.grid_bias(64, kr), E.grid_bias(64, kq)
        else:
            bz, br, bq = torch.zeros(64), torch.zeros(64), torch.zeros(64)
        zb, rh, hn, rh2, hn2 = (pl._fat(H, W, 64, B) for _ in range(5))
        S_ = [pl.fsrc(h, 0), pl.fsrc(xx, 64)]
        seg = []
        # 0..2: the layers of the gru.hip launches; 3, 4: the fused z|r launch and the q launch of conv_sep.hip
        pl.conv(seg, 'r', S_, [_Dst(pl.fview(rh), range(64), mode=L.MODE_MUL, res=pl.fview(h))], H, W, batch=B, weight=wr, bias=br)
        pl.conv(seg, 'z', S_, [_Dst(pl.fview(zb), range(64), L.ACT_SIGMOID)], H, W, batch=B, weight=wz, bias=bz)
        pl.conv(seg, 'q', [pl.fsrc(rh, 0), pl.fsrc(xx, 64)], [_Dst(pl.fview(hn), range(64), mode=L.MODE_GRU, res=pl.fview(h), aux=pl.fview(zb))],
                H, W, batch=B, weight=wq, bias=bq)
        pl.conv(seg, 'zr', S_, [_Dst(pl.fview(zb), range(0, 64), L.ACT_SIGMOID), _Dst(pl.fview(rh2), range(64, 128), mode=L.MODE_MUL, res=pl.fview(h))],
                H, W, batch=B, weight=torch.cat([wz, wr]), bias=torch.cat([bz, br]))
        pl.conv(seg, 'q2', [pl.fsrc(rh, 0), pl.fsrc(xx, 64)], [_Dst(pl.fview(hn2), range(64), mode=L.MODE_GRU, res=pl.fview(h), aux=pl.fview(zb))],
                H, W, batch=B, weight=wq, bias=bq)
        pl._upload()
        assert pl.lib.demfi_gru_r_eligible(C.byref(pl._descs[0])) == 1
        assert pl.lib.demfi_gru_zq_eligible(C.byref(pl._descs[1]), C.byref(pl._descs[2])) == 1
        assert pl._descs[3].cout_perm == 1 and pl._descs[4].cout_perm == 1 and pl._descs[3].cout_pad == 128      # the persistent 1x5 / 5x1 kernel
        for t in (zb, rh, hn, rh2, hn2):
            t.fill_(float('nan'))
        pl.launch_gru_r(0, _stream())
        pl.launch_gru_zq(1, 2, _stream())
        pl.launch_conv(3, _stream())
        pl.launch_conv(4, _stream())
        torch.cuda.synchronize()
        tag = ' %dx%d %s k=%d,%d,%d %dx%dx%d' % (kh, kw, regime, kz, kr, kq, H, W, B)
        h64 = hx[:, :64].to(f64)
        vz, Sz = E.preact(hx, wz, bz, pad)
        vr, Sr = E.preact(hx, wr, br, pad)
        Rr = E.ref_mul(vr, Sr, h64, T16)
        _check('gru.hip demfi_gru_r  sigmoid*h' + tag, _nchw(rh), Rr, T16, br)
        _check('conv_sep MODE_MUL    sigmoid*h' + tag, _nchw(rh2), Rr, T16, br)
        Rz = E.ref_store(vz, Sz, E.ACT_SIGMOID, T16)
        _check('conv_sep SIGMOID     z' + tag, _nchw(zb), Rz, T16, bz)
        # q: the operand r*h as demfi_gru_r stored it, for both forms; z on chip in fp32 (zq) / as the z launch stored it (MODE_GRU)
        vq, Sq = E.preact(torch.cat([_nchw(rh), hx[:, 64:].to(f64)], 1), wq, bq, pad)
        if regime == 'acc':
            for vv in (vz, vr, vq):
                assert float(vv.max()) > 45.0 and float(vv.min()) < -45.0
        Rzq, Rg = E.ref_zq(vz, Sz, vq, Sq, h64, T16), E.ref_gru(vq, Sq, h64, _nchw(zb), T16)
        _check('gru.hip demfi_gru_zq h\'' + tag, _nchw(hn), Rzq, T16, bq)
        _check('conv_sep MODE_GRU    h\'' + tag, _nchw(hn2), Rg, T16, bq)
        # the two forms against each other
        d = (_nchw(rh) - _nchw(rh2)).abs()
        assert bool((d <= 2.0 * Rr.bound(T16)).all()), ('r*h: gru.hip vs conv_sep', float((d / Rr.bound(T16)).max()))
        dq = (_nchw(hn) - _nchw(hn2)).abs()
        lim = Rzq.bound(T16) + Rg.bound(T16) + Rz.bound(T16) * (torch.tanh(vq) - h64).abs()
        assert bool((dq <= lim).all()), ("h': gru.hip vs conv_sep", float((dq / lim).max()))
        print('EPI gru.hip vs conv_sep%s: r*h differs on %.4f %% (largest %.3f of its limit), h\' on %.4f %% (largest %.3f of its limit)'
              % (tag, 100.0 * float((d > 0).double().mean()), float((d / (2.0 * Rr.bound(T16))).max()),
                 100.0 * float((dq > 0).double().mean()), float((dq / lim).max())))


# ------------------------------------------------------------------------------------------------------------------------------
# general kernel, gated modes: a MODE_MUL + SIGMOID two-destination launch and MODE_GRU (conv_common.h), fp32 and fp16
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_general_kernel_mul_sigmoid_and_gru(dtype, H, W, B):
    """The 5x5 48 -> 27 layer again (no persistent kernel takes it): couts 0..11 sigmoid -> z, 12..23 sigmoid * h (two destinations of one
    launch), then a second launch of the same layer whose couts 0..11 blend (1 - z) h + z tanh with the z just stored."""
    cin, cout, kh, kw = E.LAYERS['general']
    for k in E.ROTATIONS:
        pl = Plan(H, W, dtype, DEV)
        hb, zb, rh, hn, rest12 = (pl._fat(H, W, 12, B) for _ in range(5))
        rest = torch.zeros((B * 3, H, W), dtype=torch.float32, device=DEV)      # every cout must be routed: the others go here, unchecked
        hv = E.gru_state((B, 12, H, W), k)
        _put(hb, hv)
        x, w, b, i = _conv_layer(pl, 'general', H, W, B, k, lambda xb: [pl.fsrc(xb, 0)],
                                 lambda: [_Dst(pl.fview(zb), range(0, 12), L.ACT_SIGMOID), _Dst(pl.fview(rh), range(12, 24), mode=L.MODE_MUL, res=pl.fview(hb)),
                                          _Dst(pl.tview(rest, 0, sb=3 * H * W if B > 1 else 0), range(24, 27))])
        x2, w2, b2, i2 = _conv_layer(pl, 'general', H, W, B, k + 3, lambda xb: [pl.fsrc(xb, 0)],
                                     lambda: [_Dst(pl.fview(hn), range(0, 12), mode=L.MODE_GRU, res=pl.fview(hb), aux=pl.fview(zb)),
                                              _Dst(pl.fview(rest12), range(12, 24)),
                                              _Dst(pl.tview(rest, 0, sb=3 * H * W if B > 1 else 0), range(24, 27))], seed=1)
        assert pl._descs[i].cout_perm == 0 and pl._descs[i2].cout_perm == 0       # the general kernel
        pl._upload()
        for t in (zb, rh, hn):
            t.fill_(float('nan'))
        pl.launch_conv(i, _stream())
        pl.launch_conv(i2, _stream())
        torch.cuda.synchronize()
        h64 = hv.to(f64)
        v, S = E.preact(x, w, b, (2, 2))
        tag = 'general %s k=%d %dx%dx%d ' % (str(dtype)[6:], k, H, W, B)
        _check(tag + 'sigmoid z', _nchw(zb), E.ref_store(v[:, :12], S[:, :12], E.ACT_SIGMOID, dtype), dtype, b[:12])
        _check(tag + 'MODE_MUL sigmoid*h', _nchw(rh), E.ref_mul(v[:, 12:24], S[:, 12:24], h64, dtype), dtype, b[12:24])
        v2, S2 = E.preact(x2, w2, b2, (2, 2))
        _check(tag + 'MODE_GRU', _nchw(hn), E.ref_gru(v2[:, :12], S2[:, :12], h64, _nchw(zb), dtype), dtype, b2[:12])


# ------------------------------------------------------------------------------------------------------------------------------
# fp16 stores without a transcendental: bit equality with round-to-nearest-even on exact midpoints
# ------------------------------------------------------------------------------------------------------------------------------
def _int_operands(shape_x, shape_w, cout, seed, scale=2.0 ** -8, m0=2048, res_shape=None):
    """Small-integer inputs and weights and an integer bias, everything times a power of two: every product and every partial sum is an
    integer below 2^24 (times the scale), so the fp32 accumulator is EXACT in any summation order, and so is the float64 reference.
    |sum| runs through [2048, 8192) (times the scale): in [2048, 4096) every odd integer, in [4096, 8192) every n = 2 (mod 4) lies exactly
    half way between two fp16 values.  The store must then round to nearest EVEN; truncation, round-half-up or a double rounding differ."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, shape_x, generator=g).float()
    w = torch.randint(-3, 4, shape_w, generator=g).float() * scale
    m = torch.tensor([(-1.0) ** c * (m0 + 61 * c) for c in range(cout)]) * scale
    res = torch.randint(-1000, 1001, res_shape, generator=g).float() * scale if res_shape else None
    return x, w, m, res


def _assert_rne(what, out, ref, min_mid=0.05):
    """out: the fp16 NHWC buffer; ref: float64 [B,C,H,W], exact.  Bit equality with round-to-nearest-even of the reference."""
    want = ref.to(torch.float16)
    got = out.permute(0, 3, 1, 2).cpu()
    lo = want.to(f64)
    mid = (ref != lo) & ((ref - lo).abs() == 0.5 * E.spacing(torch.minimum(ref.abs(), lo.abs()), torch.float16))
    share = float(mid.double().mean())
    print('EPI %-52s %.1f %% of the elements are exact fp16 midpoints' % (what, 100 * share))
    assert share >= min_mid, (what, 'the designed operands do not land on midpoints', share)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (what, int((got.view(torch.int16) != want.view(torch.int16)).sum()))


MIDPOINT_CASES = [
    # name, pieces (channels), cout, k, stride, act, residual, routing check on the descriptor
    ('c64 none', [64], 64, 3, 1, L.ACT_NONE, False, lambda d: d.cout_perm == 1 and d.n_chunks == 1),
    ('c64 relu + res', [64], 64, 3, 1, L.ACT_RELU, True, lambda d: d.cout_perm == 1 and d.n_chunks == 1),
    ('narrow 32->32 relu', [32], 32, 3, 1, L.ACT_RELU, False, lambda d: d.cout_perm == 1 and d.n_chunks == 1 and d.rec_bytes == 64),
    ('narrow 32->64 none + res', [32], 64, 3, 1, L.ACT_NONE, True, lambda d: d.cout_perm == 1 and d.n_chunks == 1 and d.rec_bytes == 64),
    ('wsconv 3x3 64|64->64 relu', [64, 64], 64, 3, 1, L.ACT_RELU, False, lambda d: d.rec_bytes == 64 and d.nco == 2 and d.cout_perm == 1 and d.n_chunks == 4),
    ('wsconv 4x4 s2 64|64->64 none', [64, 64], 64, 4, 2, L.ACT_NONE, False, lambda d: d.rec_bytes == 64 and d.nco == 2 and d.cout_perm == 1 and d.n_chunks == 4),
    ('wsconv 4x4 s2 64->128 relu + res', [64], 128, 4, 2, L.ACT_RELU, True, lambda d: d.rec_bytes == 64 and d.nco == 2 and d.cout_perm == 1 and d.n_chunks == 2),
]


def _run_int_case(pieces, cout, ks, stride, act, with_res, H, W, B, routed, scale=2.0 ** -8, m0=2048, seed=0):
    cin = sum(pieces)
    x, w, m, res = _int_operands((B, cin, H * stride, W * stride), (cout, cin, ks, ks), cout, seed, scale, m0, (B, cout, H, W) if with_res else None)
    pl = Plan(H, W, torch.float16, DEV)
    srcs, c0 = [], 0
    for pc in pieces:
        bfr = pl._fat(H * stride, W * stride, pc, B)
        _put(bfr, x[:, c0:c0 + pc])
        srcs.append(pl.fsrc(bfr, c0))
        c0 += pc
    out = pl._fat(H, W, cout, B)
    rb = pl._fat(H, W, cout, B)
    if with_res:
        _put(rb, res)
    pl.conv([], 'int', srcs, [_Dst(pl.fview(out), range(cout), act, res=pl.fview(rb) if with_res else None)], H, W, stride=stride, batch=B, weight=w, bias=m)
    assert routed(pl._descs[0]), 'the layer does not reach the kernel this case names'
    pl._upload()
    out.fill_(float('nan'))
    pl.launch_conv(0, _stream())
    torch.cuda.synchronize()
    ref, _ = E.preact(x, w, m, (1, 1) if stride == 2 else (ks // 2, ks // 2), stride)
    if with_res:
        ref = ref + res.to(f64)
    if act == L.ACT_RELU:
        ref = torch.relu(ref)
    return out, ref


@pytest.mark.parametrize('case', MIDPOINT_CASES, ids=[c[0].replace(' ', '_') for c in MIDPOINT_CASES])
@pytest.mark.parametrize('H,W,B', E.FRAMES)
def test_fp16_store_rounds_to_nearest_even_on_exact_midpoints(case, H, W, B):
    """ACT_NONE / ACT_RELU stores of conv_c64.hip, the narrow kernel's NHWC epilogue and wsconv.hip (3x3 and 4x4 stride 2): hand-written
    (half_t) conversions and v_fma_mix residual adds.  The sums are exact (see _int_operands), so there is no tolerance at all."""
    what, pieces, cout, ks, stride, act, with_res, routed = case
    out, ref = _run_int_case(pieces, cout, ks, stride, act, with_res, H, W, B, routed)
    _assert_rne('%s %dx%dx%d' % (what, H, W, B), out, ref, 0.02 if act == L.ACT_RELU else 0.05)


def test_fp16_store_at_the_top_of_the_range():
    """|value| around 65504, the largest fp16: exact integer sums from 64000 to 67000 and their negatives through conv_c64.hip.
    Found on the MI355X and pinned here: the store is a plain round-to-nearest-even conversion -- up to 65519 it gives 65504, from 65520
    (the midpoint to the next binade) on it gives +-inf; there is no saturation.  Part of the fp16 contract."""
    H, W, B = 37, 75, 2
    out, ref = _run_int_case([64], 64, 3, 1, L.ACT_NONE, False, H, W, B, lambda d: d.cout_perm == 1, scale=1.0, m0=64000, seed=3)
    want = ref.to(torch.float16)
    got = out.permute(0, 3, 1, 2).cpu()
    n_inf, n_top = int(torch.isinf(want).sum()), int((want.abs() == 65504.0).sum())
    print('EPI c64 none near 65504: %d elements beyond 65520 (inf expected), %d at +-65504' % (n_inf, n_top))
    assert n_inf > 1000 and n_top > 100 and int((ref.abs() < 65504.0).sum()) > 1000
    assert not torch.isnan(got).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())


def test_fused_resblock_store_rounds_to_nearest_even_on_exact_midpoints():
    """resblock.hip: y = x + conv2(relu(conv1(x))) in one launch; conv2 accumulates onto bias + identity, a store path of its own.
    Exact through BOTH layers: x, w1 small integers and b1 small, so the intermediate relu(.) 2^-6 is an integer below 2048 times 2^-6
    -- exactly representable in fp16, the rounding of the intermediate changes nothing (asserted); w2 integers 2^-8, so every
    product of the second layer is an integer times 2^-14 and every partial sum stays below 2^24 of them, identity and bias included."""
    for H, W, B in E.FRAMES:
        g = torch.Generator().manual_seed(H)
        x = torch.randint(-3, 4, (B, 64, H, W), generator=g).float()
        w1 = torch.randint(-3, 4, (64, 64, 3, 3), generator=g).float() * 2.0 ** -6
        b1 = torch.randint(-40, 41, (64,), generator=g).float() * 2.0 ** -6
        w2 = torch.randint(-3, 4, (64, 64, 3, 3), generator=g).float() * 2.0 ** -8
        b2 = torch.tensor([(-1.0) ** c * (8192 + 61 * c) for c in range(64)]) * 2.0 ** -14
        pl = Plan(H, W, torch.float16, DEV)
        xb, t, y1 = (pl._fat(H, W, 64, B) for _ in range(3))
        _put(xb, x)
        seg = []
        pl.conv(seg, 'conv1', [pl.fsrc(xb, 0)], [_Dst(pl.fview(t), range(64), L.ACT_RELU)], H, W, batch=B, weight=w1, bias=b1)
        pl.conv(seg, 'conv2', [pl.fsrc(t, 0)], [_Dst(pl.fview(y1), range(64), L.ACT_NONE, res=pl.fview(xb))], H, W, batch=B, weight=w2, bias=b2)
        pl._upload()
        assert pl.lib.demfi_resblock_eligible(C.byref(pl._descs[0]), C.byref(pl._descs[1])) == 1
        y1.fill_(float('nan'))
        pl.launch_resblock(0, 1, _stream())
        torch.cuda.synchronize()
        assert float(t.abs().max()) == 0.0                   # the fused kernel ran: the intermediate never went to memory
        m, _ = E.preact(x, w1, b1, (1, 1))
        m = torch.relu(m)
        assert torch.equal(m, m.to(torch.float16).to(f64)) and float(m.max()) * 64 < 2048        # the intermediate is exact in fp16
        ref, _ = E.preact(m, w2, b2, (1, 1))
        _assert_rne('fused resblock %dx%dx%d' % (H, W, B), y1, ref + x.to(f64))


# ------------------------------------------------------------------------------------------------------------------------------
# pointwise.hip: sigmoidf_(logit) inside the warp blend and its packed record (drivers of tests/test_gpu_motion.py)
# ------------------------------------------------------------------------------------------------------------------------------
from tests import test_gpu_motion as M               # noqa: E402

BLEND_TS = [0.125, 0.5, 0.875]
BLEND_LOGITS = [g for g in E.GRID if abs(g) >= 20.0] + [0.0, 1.0, -1.0, 4.0, -4.0]


def _blend_set(H, W, Cc, dtype, planar, seed):
    """A _WarpSet of three contexts at t = 1/8, 1/2, 7/8 that share ONE pair of flows, with the logit plane drawn from the grid
    (+-20.7 ... +-1e4, and a few unsaturated values so that the fp64 comparison still sees a real blend)."""
    ws = M._WarpSet(H, W, Cc, dtype, 3, False, seed=seed, planar=planar)
    rng = M.np.random.default_rng(seed)
    ws.fa[:], ws.fb[:] = ws.fa[0], ws.fb[0]
    ws.lg[:] = M.np.asarray(BLEND_LOGITS, M.f32)[rng.integers(0, len(BLEND_LOGITS), (3, H, W))]
    ws.ts = list(BLEND_TS)
    ws.t = M._tdev(ws.ts)
    ws.dfa, ws.dfb, ws.dlg = (torch.from_numpy(a).to(DEV) for a in (ws.fa, ws.fb, ws.lg))
    return ws


def _one_frame(ws, lib, logit):
    """The single warped frame: a launch at t = 1/2 with a constant logit of +-1e4.  o0 is exactly 1 / 0 there, the surviving factor
    and the denominator are both exactly 1/2, and (1/2 v) / (1/2) = v exactly: the output IS bwarp(A, fa) resp. bwarp(B, fb) in fp32."""
    keep = ws.dlg
    ws.dlg = torch.full_like(keep, logit)
    out, occ = ws.single(1, lib)
    ws.dlg = keep
    assert bool((occ == (1.0 if logit > 0 else 0.0)).all())
    return out


@pytest.mark.parametrize('dtype,Cc,planar', [(torch.float16, 64, False), (torch.float32, 16, False), (torch.float32, 3, True)])
def test_warp_blend_logits_over_the_range(dtype, Cc, planar):
    """demfi_warp_blend and demfi_warp_blend_batched with logits from the grid at t in {1/8, 1/2, 7/8}: against motion_ref in fp64
    (M._WarpSet.check), finite everywhere, the stored occlusion plane exactly 0 below e^-x overflow (logit <= -89) and exactly 1 from
    logit >= 20.7 on (1 + e^-20.7 rounds to 1 in fp32), never anything else beyond +-89.  Where the stored weight is exactly 0 or 1 the
    blend must be the single warped frame: BIT-equal when the surviving factor (t for o0 = 0, 1 - t for o0 = 1) is a power of two
    (the scaling and the division are then exact), and within 2 fp32 ulps otherwise ((0.875 v) * (1 / 0.875): two roundings) -- for an
    fp16 output that means equal, or one fp16 ulp apart where those ulps straddle a rounding boundary."""
    lib = L.load()
    H, W = 37, 130
    ws = _blend_set(H, W, Cc, dtype, planar, seed=Cc)
    frame = {1.0: _one_frame(ws, lib, 1e4), 0.0: _one_frame(ws, lib, -1e4)}
    bout, bocc, _ = ws.batched(lib, 0)
    for q, t in enumerate(BLEND_TS):
        out, occ = ws.single(q, lib)
        assert torch.equal(out, bout[q]) and torch.equal(occ, bocc[q])
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(occ).all())
        ws.check(q, out, occ)
        lg = ws.dlg[q]
        assert bool((occ[lg <= -89.0] == 0.0).all()) and bool((occ[lg >= 20.7] == 1.0).all())
        assert bool(((occ[lg.abs() >= 89.0] == 0.0) | (occ[lg.abs() >= 89.0] == 1.0)).all())
        for o0, keep_factor in ((0.0, t), (1.0, 1.0 - t)):
            m = occ == o0
            assert int(m.sum()) > 100
            mm = (m[None] if planar else m[..., None]).expand_as(out)
            got, want = out[mm].float(), frame[o0][mm].float()
            if keep_factor in (0.125, 0.5):
                assert torch.equal(got, want), (t, o0, int((got != want).sum()))
            else:
                ulp = 2.0 ** -23 * want.abs().clamp(min=2.0 ** -126) if dtype == torch.float32 else torch.from_numpy(M.R.fp16_ulp(want.cpu().numpy())).to(DEV).float()
                assert bool(((got - want).abs() <= (2.0 if dtype == torch.float32 else 1.0) * ulp).all()), (t, o0)
                print('EPI warp blend %s C=%d t=%g o0=%g: %.4f %% of the saturated elements differ from the single frame'
                      % (str(dtype)[6:], Cc, t, o0, 100.0 * float((got != want).float().mean())))


@pytest.mark.parametrize('pack', [torch.float16, torch.float32])
def test_warp_blend_pack_record_carries_the_stored_occlusion_bit_for_bit(pack):
    """demfi_warp_blend_pack / the batched launch with a packed record, logits from the grid: channel 7 of the record must be the
    conversion of the stored fp32 occlusion plane to the pack type bit for bit (0 and 1 exactly where the plane is), the other channels
    the conversion of out | fa | fb, and each context equal to its own demfi_warp_blend_pack launch."""
    lib = L.load()
    H, W = 37, 130
    ws = _blend_set(H, W, 3, torch.float32, True, seed=7)
    out, occ, rec = ws.batched(lib, 0, pack)
    pdt = L.F32 if pack == torch.float32 else L.F16
    bits = torch.int32 if pack == torch.float32 else torch.int16
    for q in range(3):
        ws.check(q, out[q], occ[q])
        assert bool(torch.isfinite(rec[q].float()).all())
        assert torch.equal(rec[q][..., 7].contiguous().view(bits), occ[q].to(pack).contiguous().view(bits)), q
        sat = (occ[q] == 0.0) | (occ[q] == 1.0)
        assert int(sat.sum()) > 1000 and torch.equal(rec[q][..., 7][sat].float(), occ[q][sat])
        planes = torch.cat([out[q], ws.dfa[q], ws.dfb[q], occ[q][None]], 0)
        assert torch.equal(rec[q], planes.permute(1, 2, 0).to(pack)), q
        o1 = ws.new_out(1)
        c1 = torch.full((H, W), float('nan'), device=DEV)
        r1 = torch.full((H, W, 8), float('nan'), dtype=pack, device=DEV)
        va, vb, vo = ws.view(ws.A, 0), ws.view(ws.B, 0), ws.view(o1)
        M._sync_check(lib.demfi_warp_blend_pack(C.byref(va), ws.dfa[q].data_ptr(), C.byref(vb), ws.dfb[q].data_ptr(), ws.dlg[q].data_ptr(),
                                                ws.t[q:q + 1].data_ptr(), C.byref(vo), H, W, c1.data_ptr(), r1.data_ptr(), pdt, _stream()),
                      'warp pack')
        assert torch.equal(o1[0], out[q]) and torch.equal(c1, occ[q]) and torch.equal(r1, rec[q]), q
