"""The guarded-plan harness (tests/guarded_plan.py) itself, on the CPU: its stride overrides describe the memory they claim to (the plan
interpreter reads raw pointers with as_strided), and its checks FAIL when a store or a read leaves the frame.  The guarded GPU tests
(tests/test_gpu_guarded.py) are worth what these are worth."""
import pytest
import torch

from demfi_amd import _lib as L
from demfi_amd.engine import Plan, _Dst
from tests.guarded_plan import G, GuardedPlan, GuardError
from tests.plan_sim import PlanSim

CAP = 4 << 20


def _fat_case(cls, **kw):
    """64 -> 64 3x3, ReLU, NHWC residual, 13x45, batch 2 (the 64-channel persistent kernel's layer)."""
    H, W, B = 13, 45, 2
    torch.manual_seed(7)
    pl = cls(H, W, torch.float16, 'cpu', **kw)
    x, res, out = pl._fat(H, W, 64, B), pl._fat(H, W, 64, B), pl._fat(H, W, 64, B)
    x.copy_(torch.randn(B, H, W, 64))
    res.copy_(torch.randn(B, H, W, 64))
    wt = torch.randn(64, 64, 3, 3) * (1.0 / 24.0)
    bs = torch.randn(64) * 0.1
    pl.conv([], 'fat', [pl.fsrc(x, 0)], [_Dst(pl.fview(out), range(64), L.ACT_RELU, res=pl.fview(res))], H, W, batch=B, weight=wt, bias=bs)
    pl._upload()
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    ref = torch.relu(torch.nn.functional.conv2d(nchw(x), wt.half().double(), bs.double(), padding=1) + nchw(res))
    return pl, dict(x=x, res=res, out=out), [out], ref, lambda: nchw(out)


def _thin_case(cls, **kw):
    """NARROW_CASES' two-piece record (16 + 8 channels -> one 64-byte chunk) feeding a thin layer: 5 planar fp32 outputs with a planar
    residual and 2 without, tanh, 9x21 -- NHWC pieces of different pixel strides in, planes out."""
    H, W = 9, 21
    torch.manual_seed(9)
    pl = cls(H, W, torch.float16, 'cpu', **kw)
    a, b = pl._fat(H, W, 16), pl._fat(H, W, 8)
    a.copy_(torch.randn(1, H, W, 16))
    b.copy_(torch.randn(1, H, W, 8))
    o1, o2, r1 = pl._thin(5), pl._thin(2), pl._thin(5)
    r1.copy_(torch.randn(5, H, W))
    wt = torch.randn(7, 24, 3, 3) * (1.0 / (24 * 9) ** 0.5)
    bs = torch.randn(7) * 0.1
    pl.conv([], 'thin', [pl.fsrc(a, 0), pl.fsrc(b, 16)],
            [_Dst(pl.tview(o1), range(0, 5), L.ACT_TANH, res=pl.tview(r1)), _Dst(pl.tview(o2), range(5, 7), L.ACT_TANH)], H, W, weight=wt, bias=bs)
    pl._upload()
    xin = torch.cat([a, b], 3).permute(0, 3, 1, 2).double()
    ref = torch.nn.functional.conv2d(xin, wt.half().double(), bs.double(), padding=1)[0]
    ref = torch.tanh(torch.cat([ref[:5] + r1.double(), ref[5:]], 0))
    return pl, dict(a=a, b=b, o1=o1, o2=o2, r1=r1), [o1, o2], ref, lambda: torch.cat([o1, o2], 0).double()


CASES = {'fat': _fat_case, 'thin': _thin_case}


def _guarded(case):
    pl, bufs, written, ref, got = CASES[case](GuardedPlan, capacity=CAP)
    return pl, bufs, written, ref, got


@pytest.mark.parametrize('case', ['fat', 'thin'])
def test_guarded_plan_interprets_like_a_plain_plan(case):
    """The same descriptor builder on guarded memory: pitched rows, poisoned guards -- the interpreted result equals the fp64 reference
    (tolerance of test_conv_vs_torch for fp16), equals the plain Plan's bit for bit, and the launch left everything else alone."""
    pl, bufs, written, ref, got = _guarded(case)
    d = pl._descs[0]
    x = next(iter(bufs.values()))
    assert d.pieces[0].v.sy == (x.shape[2] + 2 * G) * x.shape[3] != x.shape[2] * x.shape[3]      # the row pitch is not the row
    pl.snapshot()
    PlanSim(pl).conv(d)
    pl.check(written)
    pl.assert_finite(written)
    err = (got() - ref).abs().max().item()
    assert err < 4e-3 * max(1.0, ref.abs().max().item()), err
    pp, _, _, _, plain = CASES[case](Plan)
    PlanSim(pp).conv(pp._descs[0])
    assert torch.equal(got(), plain())
    assert L.load().demfi_conv_owner(d) == L.load().demfi_conv_owner(pp._descs[0])


def test_slab_layout():
    """Zero page: 256 zero bytes, poison directly behind; blob followed by poison; >= 256 poisoned bytes between any two blocks; frames
    start poisoned."""
    pl, bufs, written, _, _ = _guarded('fat')
    base = pl.slab.data_ptr()
    z = pl.zero_page.data_ptr() - base
    assert pl.zero_page.numel() == 256 and int(pl.zero_page.max()) == 0
    assert bool((pl.slab[z + 256:z + 512] == 0xFF).all())
    b = pl.weight_blob.data_ptr() - base
    assert bool((pl.slab[b + pl.weight_blob.numel():] == 0xFF).all())
    ends = sorted([(k.off, k.off + k.nbytes) for k in pl._blocks] + [(z, z + 256), (b, b + pl.weight_blob.numel())])
    assert ends[0][0] >= 256
    for (_, e0), (s1, _) in zip(ends, ends[1:]):
        assert s1 - e0 >= 256 and bool((pl.slab[e0:s1] == 0xFF).all())
    assert torch.isnan(bufs['out']).all()                                 # a destination nobody wrote
    assert torch.isfinite(bufs['x']).all() and torch.isnan(pl.block_of(bufs['x']).of(pl.slab)[:, :G]).all()
    assert pl.regions()[0] is pl.slab


def _poke(pl, where, bufs):
    H, W = pl.H, pl.W
    if where == 'row H':
        pl.block_of(bufs['out']).of(pl.slab)[0, G + H, G + 5, 3] = 1.0
    elif where == 'column -1':
        pl.block_of(bufs['out']).of(pl.slab)[1, G + 2, G - 1, 0] = 1.0
    elif where == 'zero page':
        pl.slab[pl.zero_page.data_ptr() - pl.slab.data_ptr() + 256] = 0
    elif where == 'source':
        bufs['x'][0, 4, 7, 9] += 1.0
    elif where == 'channel':
        bufs['out'][1, 3, 2, 40] = 0.5


@pytest.mark.parametrize('where,says', [('row H', r'row 13 \(= H\) of image 0 written'), ('column -1', r'column -1 of image 1 written'),
                                        ('zero page', r'byte 0 behind the zero page written'),
                                        ('source', r'buffer 0 .*source interior written at \(image 0, row 4, column 7, channel 9\)'),
                                        ('channel', r'unwritten channel 40 of a destination written at \(image 1, row 3, column 2, channel 40\)')])
def test_check_catches_a_stray_store(where, says):
    """One element stored where a launch must not store: check() raises and names the place."""
    pl, bufs, _, _, _ = _guarded('fat')
    written = [(bufs['out'], 0, 32)]                                      # as if the launch owned channels [0, 32) of out
    pl.snapshot()
    PlanSim(pl).conv(pl._descs[0])
    with pytest.raises(GuardError, match='unwritten channel 32'):         # the interpreted layer writes all 64: 32.. are not its own
        pl.check(written)
    pl.snapshot()
    pl.check(written)                                                     # nothing happened since
    _poke(pl, where, bufs)
    with pytest.raises(GuardError, match=says):
        pl.check(written)


def test_a_source_view_one_row_up_reads_poison():
    """A descriptor whose source view starts one row early (ptr - sy: pointer arithmetic on CPU tensors, interpreted, never launched):
    row -1 is guard memory, so the output is NaN where it took part and the shared assertion on the written region fires."""
    pl, bufs, written, ref, got = _guarded('fat')
    d = pl._descs[0]
    d.pieces[0].v.ptr -= d.pieces[0].v.sy * 2
    pl.snapshot()
    PlanSim(pl).conv(d)
    pl.check(written)                                                     # a read changes nothing...
    assert torch.isnan(got()).any()
    with pytest.raises(GuardError, match=r'nan at \(image 0, row 0, column 0, channel 0\)'):
        pl.assert_finite(written)                                         # ...but what it read was poison


def test_an_unwritten_pixel_is_found():
    pl, bufs, written, _, _ = _guarded('thin')
    pl.snapshot()
    PlanSim(pl).conv(pl._descs[0])
    pl.assert_finite(written)
    pl.poison(bufs['o2'][1, 8:, 20:])
    with pytest.raises(GuardError, match=r'nan at \(plane 1, row 8, column 20\)'):
        pl.assert_finite(written)
