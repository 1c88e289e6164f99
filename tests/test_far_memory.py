"""The far-memory harness (tests/far_memory.py) itself, on the CPU.  Placement is integer arithmetic on a base address: the pure functions
are checked with synthetic base pointers at the real period of 2^32, without any large allocation; the checks (a store between far rows,
a store in the far guard rows, a consumed poison) run on a slab with a period of 2^26.  tests/test_gpu_far.py is worth what these are
worth."""
import os
import re

import numpy as np
import pytest
import torch

from demfi_amd import _lib as L
from demfi_amd.engine import _Dst
from tests import far_memory as FM
from tests.far_memory import G, GAP, FarPlan, GuardError, Space
from tests.plan_sim import PlanSim

P32 = 1 << 32
BASES = [0x7F0000000000 + k for k in (0, 256, P32 - 256, P32 // 2, P32 // 2 - 256, 3 * (P32 // 4) + 0x1234500, 0x0FFFFF00, P32 - (1 << 27),
                                      P32 - (1 << 28) - 256, (1 << 31) + (1 << 28))] + [0x7F0000000000 + 0x9E3779B1 * k // 256 * 256 for k in range(1, 40)]
FULLS = [(True, (2, 13 + 2 * G, 45 + 2 * G, 64), 2), (True, (1, 16 + 2 * G, 64 + 2 * G, 64), 2), (True, (2, 37 + 2 * G, 75 + 2 * G, 8), 2),
         (True, (1, 13 + 2 * G, 45 + 2 * G, 48), 4), (False, (5, 37 + 2 * G, 75 + 2 * G), 4), (False, (3, 33 + 2 * G, 8 + 2 * G), 4)]


def test_the_slab_fits_the_memory_cap():
    sp = Space()
    assert 8 << 30 < sp.slab_bytes < 11 << 30                     # one slab, a peak below 12 GiB with the chunked scans
    assert sp.batch_stride == P32 + 4096


@pytest.mark.parametrize('base', BASES)
def test_cross_puts_the_boundary_inside_a_middle_row_for_every_alignment_of_the_base(base):
    sp = Space()
    end = base + sp.slab_bytes
    A = sp.boundary(base)
    assert A % P32 == 0
    assert A - base >= P32 and end - A >= 2 << 30                 # >= 2 GiB on either side; in front even 4 GiB (a lost carry stays inside)
    lo, hi = sp.near_range(base, 'cross')
    assert base + (2 << 30) <= lo < hi <= A - sp.near             # the ordinary blocks: 2 GiB of slab in front of them, in front of the far one
    for fat, full, esz in FULLS:
        addr, st = FM.layout(sp, base, 'cross', fat, full, esz)
        assert addr % 16 == 0 and hi + GAP <= addr and addr + FM.span(full, st, esz) <= end
        FH, FW = full[1], full[2]
        sy, sx = (st[1], st[2])
        row = addr + (FH // 2) * sy                                # image / plane 0, frame row h // 2
        first, last = row + G * sx, row + (FW - G) * sx - 1        # the frame's part of that row
        assert first < A < last
        assert G < FH // 2 < FH - G - 1                           # a middle row: not the first, not the last of the frame


@pytest.mark.parametrize('base', BASES[:12])
def test_batch_and_pitch_margins(base):
    sp = Space()
    end = base + sp.slab_bytes
    for kind, fat, full, esz, param in [('batch', True, (2, 37 + 2 * G, 75 + 2 * G, 64), 2, None),
                                        ('pitch', True, (1, 11 + 2 * G, 45 + 2 * G, 64), 2, ('sy', FM.pitch_strides(10)[2])),
                                        ('pitch', True, (1, 13 + 2 * G, 45 + 2 * G, 64), 2, ('sx', FM.pitch_strides(34)[2])),
                                        ('pitch', False, (3, 8 + 2 * G, 32 + 2 * G), 4, ('sc', 1 << 31)),
                                        ('pitch', False, (3, 8 + 2 * G, 32 + 2 * G), 4, ('sy', 1 << 28))]:
        addr, st = FM.layout(sp, base, kind, fat, full, esz, param)
        assert addr - base >= 2 << 30                             # a sign-extended 32-bit offset from anywhere in the block stays inside
        assert end - addr >= P32                                  # a zero-extended one too: the slab reaches base + 4 GiB
        assert addr + FM.span(full, st, esz) <= end
        lo, hi = sp.near_range(base, kind)
        assert base + (2 << 30) <= lo and hi + GAP <= addr
        if kind == 'batch':
            assert st[0] == P32 + 4096 and st[1:] == FM.contiguous_strides(full, esz)[1:]


@pytest.mark.parametrize('kind,param', [('batch', None), ('pitch', ('sy', 1 << 16)), ('pitch', ('sx', 1 << 16))])
def test_far_elements_do_not_overlap(kind, param):
    """Every element of a far block (guards included) has bytes of its own -- with ``sx`` the rows interleave between two records."""
    sp = Space(1 << 26)
    full, esz = (2, 5 + 2 * G, 7 + 2 * G, 16), 2
    addr, st = FM.layout(sp, 0x7F0000000100, kind, True, full, esz, param)
    idx = np.indices(full).reshape(4, -1)
    a = sum(idx[d].astype(np.int64) * st[d] for d in range(4))
    assert len(np.unique(a)) == a.size and int(np.diff(np.sort(a)).min()) >= esz
    assert FM.span(full, st, esz) == int(a.max()) + esz
    for rel, i in zip(a[::97], idx.T[::97]):                      # and locate() inverts the layout; one byte further on lies in a gap
        assert FM.locate(full, st, esz, int(rel) + 1) == (list(i), None)
    assert FM.locate(full, st, esz, int(a.max()) - 1 + esz + 16 * esz)[1] is not None


@pytest.mark.parametrize('family', sorted(FM.PITCH_FAMILIES))
@pytest.mark.parametrize('axis', ['sy', 'sx'])
def test_pitch_cases_reach_the_lane_offsets_they_claim(family, axis):
    """For the frame of the case: the source extent's three strides put the largest lane offset of one tile below 2^31, into [2^31, 2^32)
    and at or above 2^32; the frame has the rows / columns for a tile to reach that extent; the block fits into the slab."""
    sp = Space()
    fam = FM.PITCH_FAMILIES[family]
    h, w = fam[axis + '_hw']
    cases = FM.pitch_cases(family, axis)
    src = [c for c in cases if c[1] == 'src']
    assert [c[2] for c in src] == ['lt31', '31to32', 'ge32']
    assert {c[2] for c in cases if c[1] == 'out'} >= {'lt31', '31to32'} or family.startswith('sep') or fam['out'] == fam['src']
    ext = fam['src'][0 if axis == 'sy' else 1]
    for S, kind, cls in cases:
        e = fam[kind][0 if axis == 'sy' else 1]
        off = e * S
        assert {'lt31': off < 1 << 31, '31to32': 1 << 31 <= off < P32, 'ge32': off >= P32}[cls]
        assert S % 256 == 0 and S >= 16 << 20                      # far above any row or record
        fat_full = (1, h + 2 * G, w + 2 * G, 64)
        addr, st = FM.layout(sp, BASES[3], 'pitch', True, fat_full, 2, (axis, S))       # asserts that the span fits
    if family.startswith('c64'):
        # the window of tile 0 starts at pixel (-2, -2) (NCO 2) / (-1, -1) (NCO 1): its last row and column are in the frame
        lead = 2 if family == 'c64_nco2' else 1
        assert (h if axis == 'sy' else w) > ext - lead


# ---- the checks, on a slab with a period of 2^26 ---------------------------------------------------------------------------------------------
SMALL = Space(1 << 26)


@pytest.fixture(scope='module')
def slab():
    return torch.empty(SMALL.slab_bytes, dtype=torch.uint8)


def _case(slab, far):
    """64 -> 64 3x3, ReLU, NHWC residual, 13x21 (the 64-channel persistent kernel's layer), interpreted by PlanSim."""
    H, W = 13, 21
    torch.manual_seed(7)
    pl = FarPlan(H, W, torch.float16, 'cpu', slab=slab, space=SMALL, far=far)
    x, res, out = pl._fat(H, W, 64, 2), pl._fat(H, W, 64, 2), pl._fat(H, W, 64, 2)
    x.copy_(torch.randn(2, H, W, 64))
    res.copy_(torch.randn(2, H, W, 64))
    wt = torch.randn(64, 64, 3, 3) * (1.0 / 24.0)
    bs = torch.randn(64) * 0.1
    pl.conv([], 'fat', [pl.fsrc(x, 0)], [_Dst(pl.fview(out), range(64), L.ACT_RELU, res=pl.fview(res))], H, W, batch=2, weight=wt, bias=bs)
    pl._upload()
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    ref = torch.relu(torch.nn.functional.conv2d(nchw(x), wt.half().double(), bs.double(), padding=1) + nchw(res))
    return pl, dict(x=x, res=res, out=out), ref, lambda: nchw(out)


FARS = [None, ('cross', 0, None), ('cross', 2, None), ('cross', 'zero page', None), ('cross', 'weights', None), ('batch', 0, None), ('batch', 2, None),
        ('pitch', 0, ('sy', 1 << 20)), ('pitch', 2, ('sy', 1 << 20)), ('pitch', 1, ('sx', 1 << 19)), ('pitch', 2, ('sx', 1 << 19))]


@pytest.mark.parametrize('far', FARS, ids=str)
def test_far_plan_interprets_like_a_plain_plan(slab, far):
    pl, bufs, ref, got = _case(slab, far)
    roles, batched = pl.operands()
    assert roles == {0: {'src'}, 1: {'res'}, 2: {'dst'}} and all(batched.values())
    if far and far[0] == 'cross':
        pl.assert_crosses()
    if far and far[0] == 'batch':
        t = bufs['x' if far[1] == 0 else 'out']
        assert t[1].data_ptr() - t[0].data_ptr() == SMALL.batch_stride
        assert pl._descs[0].pieces[0].v.sb * 2 == (SMALL.batch_stride if far[1] == 0 else (13 + 2 * G) * (21 + 2 * G) * 128)
    if far and far[0] == 'pitch' and far[1] == 2:
        v = pl._descs[0].segs[0].dst
        assert (v.sy if far[2][0] == 'sy' else v.sx) * 2 == far[2][1]
    pl.snapshot()
    PlanSim(pl).conv(pl._descs[0])
    pl.check([bufs['out']])
    pl.assert_finite([bufs['out']])
    err = (got() - ref).abs().max().item()
    assert err < 4e-3 * max(1.0, ref.abs().max().item()), err


def _poke(pl, bufs, where):
    out = pl.block_of(bufs['out'])
    full = out.of(pl.slab)
    if where == 'between far rows':
        pl.slab[out.off + (G + 3) * out.strides[1] + (21 + 2 * G) * 128 + 4096] = 0      # behind the last guard column of the row, far before the next row
    elif where == 'between far records':
        pl.slab[out.off + (G + 5) * out.strides[2] + 2 * (13 + 2 * G) * 384 + 640] = 0   # behind the last interleaved row slot of this column
    elif where == 'far guard row':
        full[1, G + 13, G + 2, 7] = 1.0                            # row H of image 1
    elif where == 'far guard column':
        full[0, G + 2, G - 1, 0] = 1.0
    elif where == 'source':
        bufs['x'][0, 4, 7, 9] += 1.0
    elif where == 'nowhere near':
        pl.slab[pl.slab.numel() - 9] = 7


@pytest.mark.parametrize('far,where,says', [
    (('pitch', 2, ('sy', 1 << 20)), 'between far rows', r'buffer 2 \(FAR fat .*a store between far rows, behind \(image 0, row 3, column'),
    (('pitch', 2, ('sx', 1 << 19)), 'between far records', r'buffer 2 \(FAR fat .*a store between far records, behind \(image'),
    (('pitch', 2, ('sy', 1 << 20)), 'far guard row', r'buffer 2 \(FAR.*row 13 \(= H\) of image 1 written \(guard rows\), at \(image 1, row 13, column 2, channel 7\)'),
    (('pitch', 2, ('sx', 1 << 19)), 'far guard column', r'buffer 2 \(FAR.*column -1 of image 0 written \(guard columns\), at \(image 0, row 2, column -1, channel 0\)'),
    (('batch', 2, None), 'far guard row', r'row 13 \(= H\) of image 1 written'),
    (('cross', 2, None), 'source', r'buffer 0 .*source interior written at \(image 0, row 4, column 7, channel 9\)'),
    (('cross', 0, None), 'nowhere near', r'far from every block'),
])
def test_check_names_block_and_coordinates(slab, far, where, says):
    pl, bufs, _, _ = _case(slab, far)
    pl.snapshot()
    PlanSim(pl).conv(pl._descs[0])
    pl.check([bufs['out']])
    before = pl.slab[::4099].clone()
    _poke(pl, bufs, where)
    with pytest.raises(GuardError, match=says):
        pl.check([bufs['out']])
    if where != 'nowhere near':
        after = pl.slab[::4099]
        assert int((after != before).sum()) <= 1                  # check() put every frame back


@pytest.mark.parametrize('far', [('pitch', 0, ('sy', 1 << 20)), ('pitch', 0, ('sx', 1 << 19)), ('cross', 0, None)], ids=str)
def test_a_far_source_one_row_up_reads_poison(slab, far):
    """A source view that starts one far row early: row -1 is guard memory at the far stride, the output is NaN where it took part."""
    pl, bufs, _, got = _case(slab, far)
    d = pl._descs[0]
    d.pieces[0].v.ptr -= d.pieces[0].v.sy * 2
    pl.snapshot()
    PlanSim(pl).conv(d)
    pl.check([bufs['out']])
    with pytest.raises(GuardError, match=r'buffer 2 .*nan at \(image 0, row 0, column 0, channel 0\)'):
        pl.assert_finite([bufs['out']])


def test_a_refusal_must_leave_the_slab_untouched(slab):
    pl, bufs, _, _ = _case(slab, ('pitch', 2, ('sy', 1 << 20)))
    pl.snapshot()
    with pytest.raises(FM.Refused):
        pl._status(-1, 'conv')
    bufs['out'][0, 0, 0, 0] = 1.0
    with pytest.raises(GuardError, match='source interior written'):          # nothing is listed as written: a store of a refused launch
        pl._status(-1, 'conv')


# ---- FarArena --------------------------------------------------------------------------------------------------------------------------------
def _arena(slab, far):
    al = FM.FarArena('cpu', slab, SMALL, far)
    src = al.fill(al.fat(2, 5, 7, 8, torch.float16, name='src'), torch.ones(2, 5, 7, 8))
    dst = al.fat(2, 5, 7, 8, torch.float16, name='dst')
    pl = al.fill(al.thin(3, 5, 7, n=2, name='planes'), torch.ones(2, 3, 5, 7))
    ws = al.flat(3, (40,), torch.int32, zero=True, name='ws')
    rgb = al.fill(al.thin(3, 5, 7, name='rgb'), torch.ones(3, 5, 7))      # no copies: 'batch' spreads its planes
    assert al.counts == [2, 2, 2, 3, 3] and rgb.shape == (3, 5, 7)
    return al, src, dst, pl, ws


@pytest.mark.parametrize('far', [None] + [(kind, k) for kind in ('cross', 'batch') for k in range(5)], ids=str)
def test_far_arena_places_checks_and_restores(slab, far):
    al, src, dst, pl, ws = _arena(slab, far)
    if far:
        al.assert_far()
        assert al.far_block is al._blocks[far[1]]
    if far == ('batch', 3):
        assert GA_bstride(ws) == SMALL.batch_stride
    al.snapshot()
    dst.copy_(src * 2)
    ws[1, 3:5] = 7
    al.check([dst, ws[1]])
    al.assert_finite([dst])
    assert float(dst.min()) == 2.0 and int(ws[1].sum()) == 14 and float(pl.sum()) == 2 * 3 * 5 * 7      # check() put everything back
    ws[2, 0] = 1
    with pytest.raises(GuardError, match='"ws".*does not own'):
        al.check([dst, ws[1]])
    ws[2, 0] = 0
    wide = torch.as_strided(dst, (2, 5, 8, 8), dst.stride(), dst.storage_offset())
    wide[1, 2, 7, 3] = 0
    with pytest.raises(GuardError, match=r'"dst"'):
        al.check([dst, ws[1]])


def GA_bstride(t):
    from tests.guarded_arena import bstride
    return bstride(t)


def test_planar_pitch_cases():
    """Planar destinations: two classes of the row stride fit (the planes interleave inside one row stride), all three of the plane stride."""
    assert [c[3] for c in FM.thin_pitch_cases('narrow_thin', 'sy', 3)] == ['lt31', '31to32']
    assert [(c[0], c[3]) for c in FM.thin_pitch_cases('narrow_thin', 'sx', 3)] == [('sc', 'lt31'), ('sc', '31to32'), ('sc', 'ge32')]
    full, esz = (3, 5 + 2 * G, 7 + 2 * G), 4
    for param in (('sy', 1 << 16), ('sc', 1 << 16)):
        addr, st = FM.layout(Space(1 << 26), 0x7F0000000100, 'pitch', False, full, esz, param)
        idx = np.indices(full).reshape(3, -1)
        a = sum(idx[d].astype(np.int64) * st[d] for d in range(3))
        assert len(np.unique(a)) == a.size and int(np.diff(np.sort(a)).min()) >= esz


def test_the_extents_are_those_of_the_kernels_tile_constants():
    """PITCH_FAMILIES is written in numbers; the kernels' sources are where they come from.  c64: the haloed window and the output tile
    from TH / TW (conv_common.h) and P_LW / P_LH (conv_c64.hip); the others: the multipliers in their eligibility bounds.  A tile
    constant or a bound that changes fails here, before the < 2^31 / [2^31, 2^32) / >= 2^32 labels stop meaning what they say."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'demfi_amd', 'csrc')
    src = {n: open(os.path.join(csrc, n)).read() for n in ('conv_common.h', 'conv_c64.hip', 'conv.hip', 'conv_sep.hip', 'conv_wstream.hip',
                                                            'wsconv.hip', 'resblock.hip', 'gru.hip')}
    TH = int(re.search(r'constexpr int TH = (\d+);', src['conv_common.h']).group(1))
    TW = int(re.search(r'constexpr int TW = (\d+);', src['conv_common.h']).group(1))
    assert 'constexpr int P_LW = TW + 2, P_LH = TH + 2;' in src['conv_c64.hip']
    assert '(s.sy * P_LH + s.sx * P_LW) * 2 + 128 >= P_OFF_LIMIT' in src['conv_c64.hip'] and '(d.sy * TH + d.sx * TW) * 2 + 128 >= P_OFF_LIMIT' in src['conv_c64.hip']
    F = FM.PITCH_FAMILIES
    assert F['c64_nco2']['src'] == (TH + 2, TW + 2) and F['c64_nco1']['src'] == (TH + 1, TW + 1)      # off[]: (ly + 1, lxx + 1) and (ly, lxx) at most
    assert F['c64_nco2']['out'] == F['c64_nco1']['out'] == (TH - 1, TW - 1)
    bytes_per = {'conv.hip': 2, 'conv_sep.hip': 2, 'conv_wstream.hip': 2, 'wsconv.hip': 2, 'resblock.hip': 2, 'gru.hip': 2}      # fp16 elements
    for fams, unit, text in [(('narrow_nhwc', 'narrow_thin', 'narrow_7x7', 'thin_packed_copy'), 'conv.hip', 'p.v.sy * 2 * %d + p.v.sx * 2 * %d >= (int64_t)1 << 31'),
                             (('sep_1x5', 'sep_5x1'), 'conv_sep.hip', 'p.v.sy * 2 * %d + p.v.sx * 2 * %d >= (int64_t)1 << 31'),
                             (('wstream7',), 'conv_wstream.hip', 'p.v.sy * 2 * %d + p.v.sx * 2 * %d >= (int64_t)1 << 31'),
                             (('fused_resblock',), 'resblock.hip', 'x.sy * 2 * %d + x.sx * 2 * %d >= (int64_t)1 << 31'),
                             (('gru_1x5', 'gru_5x1'), 'gru.hip', 'p.v.sy * 2 * %d + p.v.sx * 2 * %d >= (int64_t)1 << 31')]:
        for f in fams:
            assert text % F[f]['src'] in src[unit], (f, unit)
    for f in ('ws2_units', 'rdb_growth', 'ws2_stride2', 'ws2_two_piece_tail'):            # (sy + sx) * 4 * 40 elements = 80 bytes' worth each
        assert 'p.v.sy * 4 * 40 + p.v.sx * 4 * 40 >= (int64_t)1 << 31' in src['wsconv.hip'] and F[f]['src'] == (80, 80)
        assert 'v->sy * 2 * 8 >= (int64_t)1 << 31' in src['wsconv.hip'] and F[f]['out'][0] == 8 - 1
    assert bytes_per


def test_planar_batch_layout():
    """A planar block of B images of n planes: image k lies at least k * (2^32 + 4096) behind image 0, at one plane stride."""
    sp = Space()
    for n, B in ((4, 2), (1, 2), (3, 2)):
        full = (n * B, 37 + 2 * G, 75 + 2 * G)
        addr, st = FM.layout(sp, BASES[5], 'batch', False, full, 4, n)
        assert n * st[0] >= sp.batch_stride and st[0] % 256 == 0 and addr + FM.span(full, st, 4) <= BASES[5] + sp.slab_bytes
        assert addr - BASES[5] >= 2 << 30
    with pytest.raises(AssertionError):
        FM.layout(sp, BASES[5], 'batch', False, (9, 45, 83), 4, 3)                         # batch 3 of three planes: more than the slab
