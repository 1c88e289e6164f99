"""The deringing filter in front of the network (``--dering``, ``demfi_amd.dering``) without a GPU: the direction lines, hand-built blocks, the
constraint function and the rounding by hand, what follows from the rule, partial blocks at every phase against a scalar reading of the
rule, taps outside the plane, the clamp, fields, the switch from the command line to the ``EdgeSpec``, the place of the stage in the ingest,
and the inputs of the GPU tests with the proof that they cover the rule."""
import types

import numpy as np
import pytest

from demfi_amd import deblock as DB
from demfi_amd import dering as DR
from demfi_amd import pipeline as P
from demfi_amd import video
from demfi_amd import y4m
from demfi_amd.y4m_edge import Ingest


# ---- the direction search --------------------------------------------------------------------------------------------------------------
def test_the_lines_of_every_direction_partition_the_block_and_their_sizes_divide_840():
    for k in range(8):
        counts = {}
        for i in range(8):
            for j in range(8):
                line = DR.line_index(k, i, j)
                assert 0 <= line < 15
                counts[line] = counts.get(line, 0) + 1
        assert sum(counts.values()) == 64 and all(1 <= n <= 8 and 840 % n == 0 for n in counts.values())
        assert len(counts) == (15, 11, 8, 11, 15, 11, 8, 11)[k]
        assert sorted(counts) == list(range(len(counts)))


def ramp_block(k, step=12, base=20):
    """A block that is constant along the lines of direction k and rises from line to line."""
    i, j = np.mgrid[0:8, 0:8]
    return (DR.line_index(k, i, j) * step + base).astype(np.uint8)


def test_eight_hand_built_blocks_give_their_direction_and_a_flat_block_none():
    for k in range(8):
        d, var, costs = DR.block_direction_np(ramp_block(k), 8)
        assert d == k and var > 0 and costs[k] == max(costs) and costs.count(max(costs)) == 1, (k, d, var, costs)
        # the depth does not change the search when the block is shifted up
        assert DR.block_direction_np(ramp_block(k).astype(np.uint16) << 2, 10) == (d, var, costs)
    for level in (0, 1, 128, 255):
        d, var, costs = DR.block_direction_np(np.full((8, 8), level, np.uint8), 8)
        assert (d, var) == (0, 0) and len(set(costs)) == 1 and costs[0] == 840 * 64 * (level - 128) ** 2
    with pytest.raises(ValueError):
        DR.block_direction_np(np.zeros((8, 7), np.uint8), 8)


def test_the_cost_bound_is_reached_by_the_extreme_blocks_and_by_no_other():
    assert DR.COST_BOUND == 64 * 840 * 128 ** 2 == 880803840 < 2 ** 31
    assert DR.block_direction_np(np.zeros((8, 8), np.uint8), 8)[2] == [DR.COST_BOUND] * 8        # x = -128 everywhere
    assert max(DR.block_direction_np(np.full((8, 8), 255, np.uint8), 8)[2]) == 64 * 840 * 127 ** 2
    # stored bits above the depth: min(v >> sh, 255) keeps x <= 127
    assert DR.block_direction_np(np.full((8, 8), 65535, np.uint16), 10)[2] == [64 * 840 * 127 ** 2] * 8
    assert DR.block_direction_np(np.full((8, 8), 65535, np.uint16), 8)[2] == [64 * 840 * 127 ** 2] * 8
    # Cauchy-Schwarz: (sum over a line of n samples)^2 <= n * sum of squares, so cost <= 840 * sum x^2 <= the bound; random and
    # two-level blocks stay below it
    g = np.random.RandomState(0)
    blocks = np.concatenate([g.randint(0, 256, (500, 8, 8)), g.randint(0, 2, (500, 8, 8)) * 255])
    costs = DR.block_costs_np(blocks, 8)
    x = blocks.astype(np.int64) - 128
    assert (costs <= 840 * (x * x).sum((1, 2))[:, None]).all() and costs.max() <= DR.COST_BOUND and costs.min() >= 0


# ---- strengths, the constraint function, the rounding --------------------------------------------------------------------------------------
def test_adjust_by_hand():
    assert DR.adjust_np(4, 0) == 0 and DR.adjust_np(15, 0) == 0                   # a flat block: no primary filtering
    assert DR.adjust_np(4, 1) == 1 and DR.adjust_np(15, 1) == 4 and DR.adjust_np(4, 63) == 1        # var >> 6 == 0: i = 0, (4 P + 8) >> 4
    assert DR.adjust_np(4, 64) == 1 and DR.adjust_np(4, 128) == 1 and DR.adjust_np(4, 256) == 2     # i = 0, 1, 2: 24, 28, 32 >> 4
    assert DR.adjust_np(15, 64 << 11) == 14 and DR.adjust_np(15, 64 << 12) == 15                    # i = 11: 233 >> 4; i = 12: 248 >> 4
    assert DR.adjust_np(15, 1 << 30) == 15 and DR.adjust_np(4, 1 << 30) == 4                        # i capped at 12: the full P
    assert DR.adjust_np(0, 1 << 20) == 0 and DR.adjust_np(1, 1 << 20) == 1
    assert DR.adjust_np(7, np.array([0, 5, 1 << 12])).tolist() == [0, 2, 4]                         # 36 >> 4; i = 6: 78 >> 4
    assert DR.ilog2([1, 2, 3, 4, 255, 256, 3840]).tolist() == [0, 1, 1, 2, 7, 8, 11]


def test_constrain_by_hand():
    c = DR.constrain_np
    assert c(5, 0, 5) == 0 and c(-200, 0, 3) == 0                                   # thr = 0
    # thr = 4, damp = 5: shift 5 - 2 = 3, so thr << shift = 32
    assert [int(c(d, 4, 5)) for d in (0, 1, 3, 4, 5, 7, 8, 15, 16, 23, 24, 31, 32, 33, 255)] == [0, 1, 3, 4, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0, 0]
    assert [int(c(-d, 4, 5)) for d in (1, 5, 31, 32)] == [-1, -4, -1, 0]
    # thr = 15, damp = 3: the shift 3 - 3 is 0; thr = 15, damp = 2 would be negative and is clamped at 0 (damp = 3 at ilog2 = 11 likewise)
    assert [int(c(d, 15, 3)) for d in (7, 8, 14, 15, 16)] == [7, 7, 1, 0, 0]
    assert [int(c(d, 3840, 3)) for d in (1000, 1920, 1921, 3839, 3840)] == [1000, 1920, 1919, 1, 0]
    # at depth 10 the threshold and the damping are both shifted: thr = 16, damp = 7, shift 3 again, thr << shift = 128
    assert [int(c(d, 16, 7)) for d in (12, 16, 17, 127, 128)] == [12, 14, 14, 1, 0]
    assert c(np.array([3, -3, 40]), np.array([4, 0, 4]), 5).tolist() == [3, 0, 0]


def test_the_rounding_is_to_nearest_with_ties_away_from_zero():
    assert DR.round_np([-25, -24, -23, -9, -8, -7, -1, 0, 1, 7, 8, 9, 23, 24, 25]).tolist() == [-2, -2, -1, -1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2]
    assert 12 * (15 + 4) << 8 == 58368                                        # |s| stays far below 2^31 at 16 bits


# ---- a scalar reading of the rule --------------------------------------------------------------------------------------------------------
def _ilog2(n):
    return n.bit_length() - 1


def _constrain(diff, thr, damp):
    if thr == 0:
        return 0
    mag = min(abs(diff), max(0, thr - (abs(diff) >> max(0, damp - _ilog2(thr)))))
    return -mag if diff < 0 else mag


def by_hand(plane, depth, P_, S_, D_, left=0, top=0):
    """The rule, sample by sample, with the direction search on a plane padded by edge replication."""
    p = np.asarray(plane).astype(np.int64)
    rows, cols = p.shape
    sh = depth - 8
    padded = np.pad(p, ((top, -(rows + top) % 8), (left, -(cols + left) % 8)), mode='edge')
    info = {}
    for by in range(padded.shape[0] // 8):
        for bx in range(padded.shape[1] // 8):
            k, var, _ = DR.block_direction_np(padded[8 * by:8 * by + 8, 8 * bx:8 * bx + 8], depth)
            i = min(_ilog2(var >> 6), 12) if var >> 6 else 0
            info[by, bx] = (k, ((P_ * (4 + i) + 8) >> 4 if var else 0) << sh)
    out = p.copy()
    for y in range(rows):
        for x in range(cols):
            k, pri = info[(y + top) // 8, (x + left) // 8]
            c, s, seen = int(p[y, x]), 0, [int(p[y, x])]
            for kk, thr, weights in ((k, pri, (4, 2)), ((k + 2) & 7, S_ << sh, (2, 1)), ((k + 6) & 7, S_ << sh, (2, 1))):
                for dist in (0, 1):
                    for sign in (1, -1):
                        ty, tx = y + sign * DR.TAPS[kk][dist][0], x + sign * DR.TAPS[kk][dist][1]
                        if 0 <= ty < rows and 0 <= tx < cols:
                            s += weights[dist] * _constrain(int(p[ty, tx]) - c, thr, D_ + sh)
                            seen.append(int(p[ty, tx]))
            out[y, x] = min(max(c + ((8 + s - (s < 0)) >> 4), min(seen)), max(seen))
    return out.astype(np.asarray(plane).dtype)


def _noisy_edges(g, rows, cols, depth):
    yy, xx = np.mgrid[0:rows, 0:cols]
    v = np.where((xx + yy // 2) % 11 < 5, 60, 170) + g.randint(-9, 10, (rows, cols))
    return (np.clip(v, 0, 255) << (depth - 8)).astype(np.uint8 if depth == 8 else np.uint16)


def test_partial_blocks_at_all_64_phases_against_the_scalar_reading():
    g = np.random.RandomState(5)
    plane = _noisy_edges(g, 13, 19, 8)
    for top in range(8):
        for left in range(8):
            got = DR.dering_plane_np(plane, 8, 9, 3, 4, left, top)
            assert np.array_equal(got, by_hand(plane, 8, 9, 3, 4, left, top)), (top, left)
            cases = DR.plane_cases(plane, 8, 9, 3, 4, left, top)
            assert cases['dir'].shape == ((13 + top + 7) // 8, (19 + left + 7) // 8)
    assert not np.array_equal(DR.dering_plane_np(plane, 8, 9, 3, 4, 0, 0), DR.dering_plane_np(plane, 8, 9, 3, 4, 3, 5))     # the phase matters
    assert np.array_equal(DR.dering_plane_np(plane, 8, 9, 3, 4, 11, 21), DR.dering_plane_np(plane, 8, 9, 3, 4, 3, 5))       # mod 8


@pytest.mark.parametrize('depth,psd', [(8, (4, 2, 5)), (8, (15, 4, 3)), (10, (15, 4, 6)), (16, (1, 1, 6)), (10, (0, 4, 5)), (12, (15, 0, 5))])
def test_planes_smaller_than_a_block_and_ragged_ones_against_the_scalar_reading(depth, psd):
    g = np.random.RandomState(depth)
    for rows, cols in ((1, 1), (2, 3), (5, 7), (8, 8), (9, 12), (12, 9), (17, 16)):
        plane = _noisy_edges(g, rows, cols, depth)
        assert np.array_equal(DR.dering_plane_np(plane, depth, *psd), by_hand(plane, depth, *psd)), (rows, cols)


# ---- what follows from the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [8, 10, 16])
def test_identity_constant_bounds_and_edges(depth):
    g = np.random.RandomState(depth)
    sh = depth - 8
    plane = _noisy_edges(g, 40, 56, depth)
    for psd in ((0, 0, 3), (0, 0, 6)):
        assert np.array_equal(DR.dering_plane_np(plane, depth, *psd), plane)                        # 0:0 is the identity
    for level in (0, 77 << sh, (1 << depth) - 1):
        flat = np.full((19, 21), level, plane.dtype)
        assert np.array_equal(DR.dering_plane_np(flat, depth, 15, 4, 3), flat)                      # a constant plane stays constant
    # every output lies between the extremes of the 13 samples it read: within the 5x5 neighbourhood's extremes a fortiori, and within
    # the extremes of the samples of ``by_hand`` exactly (which the comparison with it above pins)
    out = DR.dering_plane_np(plane, depth, 15, 4, 6).astype(np.int64)
    pad = np.pad(plane.astype(np.int64), 2, mode='edge')
    win = np.stack([pad[dy:dy + 40, dx:dx + 56] for dy in range(5) for dx in range(5)])
    assert (out >= win.min(0)).all() and (out <= win.max(0)).all() and (out != plane).mean() > 0.3
    # an edge of thr << shift or more contributes nothing: two flat halves 64 steps apart stay as they are at the strongest setting
    step = np.full((24, 24), 50 << sh, plane.dtype)
    step[:, 12:] = 114 << sh
    assert np.array_equal(DR.dering_plane_np(step, depth, 15, 4, 6), step)
    # ... while a ripple of 3 steps beside the edge is smoothed
    ripple = step.copy()
    ripple[:, 10] -= 3 << sh
    out = DR.dering_plane_np(ripple, depth, 15, 4, 6)
    assert (np.abs(out[4:20, 10].astype(np.int64) - (50 << sh)) < (3 << sh)).all() and np.array_equal(out[:, 12:], step[:, 12:])


def test_a_plane_shifted_up_keeps_directions_and_strengths():
    g = np.random.RandomState(3)
    p8 = _noisy_edges(g, 48, 64, 8)
    c8, out8 = DR.plane_cases(p8, 8, 15, 4, 5), DR.dering_plane_np(p8, 8, 15, 4, 5).astype(np.int64)
    for depth in (10, 12, 16):
        sh = depth - 8
        up = p8.astype(np.uint16) << sh
        c = DR.plane_cases(up, depth, 15, 4, 5)
        assert np.array_equal(c['dir'], c8['dir']) and np.array_equal(c['t'], c8['t']) and np.array_equal(c['flat'], c8['flat'])
        assert DR.strengths(depth, 15, 4, 5) == (15, 4 << sh, 5 + sh, sh)
        # each constrained term lies within (1 << sh) - 1 below the shifted one (the floor of |diff| >> shift), the weights sum to 24, and
        # the rounding of s / 16 adds half a step on each side: |out - (out8 << sh)| <= (24 ((1 << sh) - 1) / 16 + (1 << sh) / 2 + 1 / 2
        bound = int(np.ceil(24 * ((1 << sh) - 1) / 16 + (1 << sh) / 2 + 0.5))
        diff = np.abs(DR.dering_plane_np(up, depth, 15, 4, 5).astype(np.int64) - (out8 << sh))
        assert diff.max() <= bound, (depth, diff.max(), bound)
    assert DR.strengths(8) == (4, 2, 5, 0) and DR.strengths(10, 7) == (7, 16, 7, 2)
    with pytest.raises(ValueError):
        DR.strengths(9)


def test_taps_outside_the_plane_contribute_nothing_and_do_not_enter_the_clamp():
    # a single row: direction 2 (horizontal), every tap with dy != 0 lies outside; the result is that of the in-row taps alone
    g = np.random.RandomState(9)
    row = _noisy_edges(g, 1, 40, 8)
    assert np.array_equal(DR.dering_plane_np(row, 8, 15, 4, 5), by_hand(row, 8, 15, 4, 5))
    cases = DR.plane_cases(row, 8, 15, 4, 5)
    assert cases['outside'].all()
    # the corner sample of a plane whose only other values are far away on the diagonal: nothing it may read is within the threshold
    plane = np.full((16, 16), 100, np.uint8)
    plane[0, 0] = 90
    out = DR.dering_plane_np(plane, 8, 15, 4, 6)
    assert 90 < out[0, 0] <= 100 and np.array_equal(out, by_hand(plane, 8, 15, 4, 6))
    inner = DR.plane_cases(_noisy_edges(g, 24, 24, 8), 8)['outside']
    assert not inner[2:-2, 2:-2].any() and inner[0].all() and inner[:, -1].all()


def clamp_plane():
    """104 everywhere, two columns of 0 at the left, one sample of 100 at (4, 5)."""
    plane = np.full((16, 16), 104, np.uint8)
    plane[:, :2] = 0
    plane[4, 5] = 100
    return plane


def test_the_clamp_acts_on_the_hand_built_plane():
    plane = clamp_plane()
    out, cases = DR.dering_plane_np(plane, 8, 15, 4, 6), DR.plane_cases(plane, 8, 15, 4, 6)
    assert out[4, 5] == 104 and cases['clamped'][4, 5] and np.array_equal(out, by_hand(plane, 8, 15, 4, 6))
    # without the clamp the sample would overshoot: its taps pull it up by more than the 4 steps to its greatest neighbour
    p = plane.astype(np.int64)
    k, t = int(cases['dir'][0, 0]), int(cases['t'][0, 0])
    s = sum(w * _constrain(int(p[4 + sg * DR.TAPS[kk][d][0], 5 + sg * DR.TAPS[kk][d][1]]) - 100, thr, 6)
            for kk, thr, ws in ((k, t, (4, 2)), ((k + 2) & 7, 4, (2, 1)), ((k + 6) & 7, 4, (2, 1))) for d, w in enumerate(ws) for sg in (1, -1))
    assert 100 + ((8 + s) >> 4) > 104


def test_fields_are_planes_of_their_own():
    g = np.random.RandomState(11)
    h, w = 34, 40
    pay = np.concatenate([_noisy_edges(g, h, w, 8).reshape(-1), _noisy_edges(g, h // 2, w // 2, 8).reshape(-1), _noisy_edges(g, h // 2, w // 2, 8).reshape(-1)])
    out = DR.dering_payload_np(pay, h, w, 8, '420', 9, 3, 5, fields='t')
    luma, got = pay[:h * w].reshape(h, w), out[:h * w].reshape(h, w)
    for q in (0, 1):
        assert np.array_equal(got[q::2], DR.dering_plane_np(luma[q::2], 8, 9, 3, 5))
    cb, gcb = pay[h * w:h * w + (h // 2) * (w // 2)].reshape(h // 2, w // 2), out[h * w:h * w + (h // 2) * (w // 2)].reshape(h // 2, w // 2)
    for q in (0, 1):
        assert np.array_equal(gcb[q::2], DR.dering_plane_np(cb[q::2], 8, 9, 3, 5))
    prog = DR.dering_payload_np(pay, h, w, 8, '420', 9, 3, 5)
    assert not np.array_equal(prog, out) and np.array_equal(prog[:h * w].reshape(h, w), DR.dering_plane_np(luma, 8, 9, 3, 5))
    # the crop rectangle gives the phases, the top halved over fields
    rect = (4, 4 + h, 6, 6 + w)
    out = DR.dering_payload_np(pay, h, w, 8, '420', 9, 3, 5, fields='b', rect=rect)
    assert np.array_equal(out[:h * w].reshape(h, w)[1::2], DR.dering_plane_np(luma[1::2], 8, 9, 3, 5, left=6, top=2))
    assert np.array_equal(out[h * w:h * w + (h // 2) * (w // 2)].reshape(h // 2, w // 2)[0::2], DR.dering_plane_np(cb[0::2], 8, 9, 3, 5, left=3, top=1))
    assert [np.array_equal(a, b) for a, b in zip(DR.dering_stream_np([pay, pay[::-1].copy()], h, w, 8, '420', 9, 3, 5),
                                                 [prog, DR.dering_payload_np(pay[::-1].copy(), h, w, 8, '420', 9, 3, 5)])] == [True, True]
    with pytest.raises(ValueError):
        DR.dering_payload_np(pay[:-1], h, w, 8, '420')
    with pytest.raises(ValueError):
        DR.dering_plane_np(pay, 8)


# ---- the switch --------------------------------------------------------------------------------------------------------------------------
def test_parse_dering_and_check_params():
    assert DR.DEFAULTS == (4, 2, 5) and DR.parse_dering('4:2:5') == (4, 2, 5) and DR.parse_dering(' 6 ') == (6, 3, 5) and DR.parse_dering('7') == (7, 4, 5)
    assert DR.parse_dering('15') == (15, 4, 5) and DR.parse_dering('0') == (0, 0, 5) and DR.parse_dering('0:0') == (0, 0, 5)
    assert DR.parse_dering('0:4') == (0, 4, 5) and DR.parse_dering('15:0:3') == (15, 0, 3) and DR.parse_dering('1:1:6') == (1, 1, 6)
    assert DR.check_params() == (4, 2, 5) and DR.check_params(np.int64(8), np.int32(2), 4) == (8, 2, 4) and DR.check_params(1) == (1, 1, 5)
    for bad in ('', 'x', '4:', ':4', '16', '4:5', '4:2:2', '4:2:7', '-1', '4:2:5:1', '1.5', '4:2:x'):
        with pytest.raises(ValueError):
            DR.parse_dering(bad)
    for bad in ((-1,), (16,), (4, 5), (4, -1), (4, 2, 2), (4, 2, 7), (True,), (4.0,), (4, 2.0), (4, 2, 5.0)):
        with pytest.raises(ValueError):
            DR.check_params(*bad)


def test_edge_spec_with_dering_deblock_and_denoise():
    args = (True, True, False, 10, '422', None, 't', 'adaptive')
    plain = P.EdgeSpec(*args)
    dr = P.EdgeSpec(*args, dering=(4, 2, 5))
    assert dr.dering == (4, 2, 5) and plain.dering is None and tuple(dr) == tuple(plain) and len(plain) == 8
    assert dr != plain and plain != dr and dr != tuple(dr) and plain == tuple(plain)
    assert hash(plain) == hash((tuple(plain), None))                      # as before there was the field
    assert dr == P.EdgeSpec(*args, dering=[4, 2, 5]) and hash(dr) == hash(dr._replace())
    assert dr != dr._replace(dering=(4, 2, 6)) and dr._replace(dering=None) == plain and plain._replace(dering=(4, 2, 5)) == dr
    assert 'dering=(4, 2, 5)' in repr(dr) and 'dering' not in repr(plain) and repr(plain) == repr(dr._replace(dering=None))
    for none in ((0, 0, 5), (0, 0, 3), None):                             # P = S = 0: no stage
        assert P.EdgeSpec(True, dering=none) == P.EdgeSpec(True) and P.EdgeSpec(True, dering=none).dering is None
        assert hash(P.EdgeSpec(True, dering=none)) == hash(P.EdgeSpec(True)) and repr(P.EdgeSpec(True, dering=none)) == repr(P.EdgeSpec(True))
    assert P.EdgeSpec(True, dering=(0, 4, 5)).dering == (0, 4, 5) and P.EdgeSpec(True, dering=(15, 0, 5)).dering == (15, 0, 5)
    # every combination with deblock and denoise: each field survives the others' _replace, equality and hash tell them all apart
    seen = set()
    for db in (None, (16, 4)):
        for dn in (None, (5, 10, 2)):
            for d in (None, (4, 2, 5)):
                spec = P.EdgeSpec(*args, deblock=db, denoise=dn, dering=d)
                assert (spec.deblock, spec.denoise, spec.dering) == (db, dn, d)
                assert spec == plain._replace(dering=d)._replace(denoise=dn)._replace(deblock=db) and spec._replace(depth=8).dering == d
                assert spec._replace(dering=None) == P.EdgeSpec(*args, deblock=db, denoise=dn)
                assert ('dering' in repr(spec)) == (d is not None) and ('deblock' in repr(spec)) == (db is not None)
                if d is None:
                    assert repr(spec) == repr(P.EdgeSpec(*args, deblock=db, denoise=dn)) and hash(spec) == hash(P.EdgeSpec(*args, deblock=db, denoise=dn))
                seen.add(spec)
    assert len(seen) == 8
    assert dr.reach == plain.reach == 2 and P.EdgeSpec(True, dering=(4, 2, 5)).reach == 0           # no look-ahead of its own
    edge = video.YuvEdge('bt601', False, '420jpeg', None, dering=(6, 3, 4), crop_rect=(4, 60, 6, 90))
    assert edge.dering == (6, 3, 4) and edge.deblock is None and edge.crop_rect == (4, 60, 6, 90) and P.EdgeSpec.of(edge).dering == (6, 3, 4)
    plain_edge = video.YuvEdge('bt601', False, '420jpeg', None)
    assert plain_edge.dering is None and P.EdgeSpec.of(plain_edge) == P.EdgeSpec(True)
    assert video.YuvEdge('bt601', False, '420jpeg', None, dering=(0, 0)).dering is None
    with pytest.raises(ValueError):
        video.YuvEdge('bt601', False, '420jpeg', None, dering=(4, 5))
    # nothing is refused: repeated frames, the adaptive mode, the denoiser, deep streams, layouts
    dr.check(True, True, True)
    P.EdgeSpec(True, True, True, 16, '444', (7, 5, 0, 4), 't', 'bob', dering=(4, 2, 5), deblock=(16, 4)).check(True, True, True)
    P.EdgeSpec(True, denoise=(5, 10, 2), dering=(4, 2, 5), shutter=(2, 4), grain=(16, 1, 8, 'film', 0)).check(True, False, True)
    for spec, a, msg in ((P.EdgeSpec(True, dering=(16, 2, 5)), (True, False, True), 'dering must be'),
                         (P.EdgeSpec(True, dering=(4, 5, 5)), (True, False, True), 'dering must be'),
                         (P.EdgeSpec(True, dering=(4, 2, 7)), (True, False, True), 'dering must be'),
                         (P.EdgeSpec(True, dering=(4, 2)), (True, False, True), 'dering must be'),
                         (P.EdgeSpec(False, dering=(4, 2, 5)), (False, False, True), 'Y4M edge')):
        with pytest.raises(ValueError, match=msg):
            spec.check(*a)


def test_runner_arguments_counter_and_the_crop_rectangle():
    vr = video.VideoRunner(None)
    assert vr.dering is None and vr.last_deringed == 0
    assert video.VideoRunner(None, dering=True).dering == (4, 2, 5) and video.VideoRunner(None, dering=False).dering is None
    assert video.VideoRunner(None, dering=6).dering == (6, 3, 5) and video.VideoRunner(None, dering='12:3:4').dering == (12, 3, 4)
    assert video.VideoRunner(None, dering=(9, 0)).dering == (9, 0, 5) and video.VideoRunner(None, dering=(0, 0, 4)).dering is None
    assert video.VideoRunner(None, dering=0).dering is None and video.VideoRunner(None, dering='0:0').dering is None
    assert video.check_dering(None) is None and video.check_dering((15, None, None)) == (15, 4, 5) and video.check_dering('0:3') == (0, 3, 5)
    vr = video.VideoRunner(None, dering=True, dedup=True, deinterlace=True)
    assert vr.dering == (4, 2, 5) and vr._behind('t') == 0
    vr = video.VideoRunner(None, dering=True, deblock=True, deinterlace=True, deinterlace_mode='adaptive', tile='auto', high_depth=True,
                           tile_high_depth=True, layouts=True)
    assert vr._behind('t') == 2 and (vr.deblock, vr.dering) == ((16, 4), (4, 2, 5))
    assert video.VideoRunner(None, dering=True, denoise=True, denoise_radius=3)._behind(None) == 3
    video.check_one_rank(4, dering=(4, 2, 5))                             # any number of ranks
    assert 'dering' not in video.ONE_RANK and 'dering' not in video.ONE_RANK_EGRESS
    for kw, msg in ((dict(dering=(4, 5)), 'secondary'), (dict(dering=16), '0 .. 15'), (dict(dering=(1, 2, 3, 4)), 'dering must be'),
                    (dict(dering=2.5), 'dering must be'), (dict(dering='x'), 'expected P'), (dict(dering=(4, 2, 9)), 'damping')):
        with pytest.raises(ValueError, match=msg):
            video.VideoRunner(None, **kw)
    assert video.INGEST_COUNTERS['deringed'] == 'last_deringed' and video.INGEST_COUNTERS['deblocked'] == 'last_deblocked'
    vr = video.VideoRunner(None, mfi=2, dering=True)
    vr._counted(types.SimpleNamespace(w=96, h=64, layout='420'), dict({name: 0 for name in video.COUNTERS}, deringed=9), [], 0)
    assert vr.last_deringed == 9 and vr.last_deblocked == 0
    import inspect
    from demfi_amd.runner import WindowRunner
    assert 'self.deringed = 0' in inspect.getsource(WindowRunner.__init__)
    # the rectangle reaches the edge whenever either stage needs the phases
    hdr = y4m.Header(96, 64, 25, 'p', None, '420jpeg', None, (), '420jpeg', 8, '420')
    for kw, want in ((dict(dering=True), True), (dict(deblock=True), True), (dict(dering=True, deblock=True), True), (dict(), False)):
        vr = video.VideoRunner(None, mfi=2, crop=(4, 4, 6, 2), **kw)
        vr.last_crop = (4, 60, 6, 94)
        edge = vr._edge(hdr, None)
        assert edge.crop_rect == ((4, 60, 6, 94) if want else None) and edge.dering == vr.dering and edge.deblock == vr.deblock


def test_command_line(capsys):
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).dering is None and p.parse_args(['-', '-', '--dering']).dering == (4, 2, 5)
    assert p.parse_args(['a', 'b', '--dering', '6']).dering == (6, 3, 5) and p.parse_args(['a', 'b', '--dering', '12:3:4', '--dedup']).dering == (12, 3, 4)
    assert p.parse_args(['a', 'b', '--dering', '0:0']).dering == (0, 0, 5) and '--dering' in p.format_help()
    assert p.parse_args(['a', 'b', '--deblock', '--dering']).deblock == (16, 4)
    for argv, msg in ((['a.y4m', 'b.y4m', '--dering', '3:9'], 'secondary'), (['a.y4m', 'b.y4m', '--dering', '16'], '0 .. 15'),
                      (['a.y4m', 'b.y4m', '--dering', 'x'], 'expected P')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
    from demfi_amd import clip
    with pytest.raises(SystemExit) as ex:                                 # the folder path has no such switch
        clip.parser().parse_args(['frames', '--dering'])
    assert ex.value.code == 2
    for doc in (video.__doc__, video.VideoRunner.__doc__, DB.__doc__):
        assert '--dering' in doc or 'dering' in doc
    assert 'deringing;' not in DB.__doc__ and 'deringing;' not in video.__doc__       # no longer under Not offered


# ---- the place of the stage in the ingest ------------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self, on_call=None):
        self.calls, self.on_call = [], on_call

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if self.on_call is not None:
                self.on_call(name, args)
            return 0
        return call


def _ingest(spec, monkeypatch, h=12, w=20, nslot=8, on_call=None):
    import torch
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    rn = types.SimpleNamespace(lib=_FakeLib(on_call), engine=types.SimpleNamespace(device='cpu'), depth_promoted=0, denoised=0, deblocked=0, deringed=0)
    return Ingest(rn, P.FrameSlots(nslot, 2, 2, 'cpu'), spec, h, w), rn


def test_the_ingest_order_and_the_scratch_copy(monkeypatch):
    spec = P.EdgeSpec(True, depth=10, fields='t', denoise=(5, 10, 1), deblock=(16, 4), dering=(6, 3, 4), depths=(8, 10, 10, None))
    seen = {}

    def on_call(name, args):                                              # at the launch the scratch already holds the run's payloads
        if name == 'demfi_payload_dering':
            seen['scratch'] = ing.dr_scratch[:6].clone()
    ing, rn = _ingest(spec, monkeypatch, on_call=on_call)
    ing.attach(types.SimpleNamespace(full_range=False, crop_rect=(4, 16, 6, 26)))
    ing.yuv_in.copy_(__import__('torch').arange(ing.yuv_in.numel(), dtype=__import__('torch').int64).reshape(ing.yuv_in.shape) % 251)
    ing.dr_scratch.zero_()
    stream = types.SimpleNamespace(cuda_stream=0)
    near = ing.around({2, 3}, lambda g: g < 6)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2, 3})]
    assert [sl for _, sl in new] == list(range(6))
    done = ing.rebuilt(new, stream)
    names = [name for name, _ in rn.lib.calls]
    assert names == ['demfi_payload_promote', 'demfi_payload_deblock', 'demfi_payload_dering', 'demfi_yuv_bob', 'demfi_payload_denoise']
    assert [f for f, _ in done] == [2, 3] and (rn.depth_promoted, rn.deblocked, rn.deringed, rn.denoised) == (6, 6, 6, 2)
    args = dict(rn.lib.calls)['demfi_payload_dering']
    # from the scratch back into yuv_in, slot for slot
    assert args[0] == ing.dr_scratch[0].data_ptr() and args[2] == ing.yuv_in[0].data_ptr() and args[1] == args[3] == ing.Pb == 2 * y4m.payload_size(12, 20)
    assert args[4] == 6 and ing.dr_scratch.shape == ing.yuv_in.shape and ing.dr_scratch.dtype == ing.yuv_in.dtype
    assert bool((seen['scratch'] == ing.yuv_in[:6]).all()) and not bool((ing.dr_scratch[6:] != 0).any())
    tab = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int64 * (6 * args[6])).from_address(args[5])).reshape(-1, 6)
    assert tab.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))] and args[6] == 6
    assert args[7:12] == (2, 10, 6, 3, 4)                                 # sample size, working depth, P, S, D at the 8-bit scale
    # two runs of slots: two copies and two launches; nothing new: none
    rn.lib.calls.clear()
    ing.deringed([(8, 1), (9, 2), (11, 5)], stream)
    assert [(name, a[0] - ing.dr_scratch.data_ptr(), a[2] - ing.yuv_in.data_ptr(), a[4]) for name, a in rn.lib.calls] == [
        ('demfi_payload_dering', ing.Pb, ing.Pb, 2), ('demfi_payload_dering', 5 * ing.Pb, 5 * ing.Pb, 1)]
    rn.lib.calls.clear()
    ing.deringed([], stream)
    assert not rn.lib.calls and rn.deringed == 9


def test_alone_with_the_adaptive_mode_and_with_the_probe_of_repeated_frames(monkeypatch):
    ing, rn = _ingest(P.EdgeSpec(True, fields='b', deint_mode='adaptive', dering=(4, 2, 5)), monkeypatch)
    stream = types.SimpleNamespace(cuda_stream=0)
    near = ing.around({2}, lambda g: g < 8)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2})]
    ing.rebuilt(new, stream)
    assert [name for name, _ in rn.lib.calls] == ['demfi_payload_dering', 'demfi_yuv_deint_adaptive'] and rn.deringed == len(new) == 5
    assert ing.deblock is None and not hasattr(ing, 'db_planes') and rn.deblocked == 0
    assert ing.dr_planes.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 'b')]
    ing, rn = _ingest(P.EdgeSpec(True, dedup=(7, 5, 0, 4), fields='t', dering=(4, 2, 5)), monkeypatch)
    ing.rebuilt([(0, 3)], stream)
    assert [name for name, _ in rn.lib.calls] == ['demfi_payload_dering', 'demfi_yuv_bob'] and rn.deringed == 1


def test_without_the_switch_the_ingest_is_what_it_was(monkeypatch):
    assert object.__new__(Ingest).dering is None
    for spec in (P.EdgeSpec(True, fields='t'), P.EdgeSpec(True, dering=(0, 0, 5), fields='t'), P.EdgeSpec(True, deblock=(16, 4), fields='t')):
        ing, rn = _ingest(spec, monkeypatch)
        assert ing.dering is None and not hasattr(ing, 'dr_planes') and not hasattr(ing, 'dr_scratch')
        ing.attach(types.SimpleNamespace(full_range=True, crop_rect=(4, 16, 6, 26)))
        assert ing.full_range is True and not hasattr(ing, 'dr_planes')
        ing.rebuilt([(0, 0), (1, 1)], types.SimpleNamespace(cuda_stream=0))
        assert 'demfi_payload_dering' not in [name for name, _ in rn.lib.calls] and rn.deringed == 0


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
_VEC = ((-1, 1), (-1, 2), (0, 1), (1, 2), (1, 1), (2, 1), (1, 0), (2, -1))       # along the lines of direction k: (dy, dx)


def ringing_plane(rows, cols, depth, seed, noise, shift=0, dtype=None):
    """Oriented bars with ripples and noise: cells of 16 x 16 samples, each with bars along one of the 8 directions (a step of 80 every 6
    samples across, a ripple of +-6 with a period of 3 beside it, noise of +-2) or, two cells in ten, flat without noise.  ``shift`` moves
    the whole pattern to the left; ``noise``: the generator of the noise, which does not move."""
    kind = np.random.RandomState(seed).randint(0, 10, (64, 64))
    yy, xx = np.mgrid[0:rows, 0:cols]
    xx = xx + shift
    k = kind[(yy // 16) % 64, (xx // 16) % 64]
    vec = np.array(_VEC)[k % 8]
    across = (yy * vec[..., 1] - xx * vec[..., 0]) / np.hypot(vec[..., 0], vec[..., 1])
    v = 128 + np.where(np.sin(2 * np.pi * across / 12) > 0, 40, -40) + np.round(6 * np.sin(2 * np.pi * across / 3)) + noise.randint(-2, 3, (rows, cols))
    v = np.where(k >= 8, 60 + 40 * (k - 8), v).astype(np.int64)
    return (np.clip(v, 0, 255) << (depth - 8)).astype(dtype or (np.uint8 if depth == 8 else np.uint16))


def plane_view(pay, entry):
    """The [rows, cols] view of one entry of a plane table into the flat payload ``pay``."""
    first, rows, cols, pitch = entry[:4]
    return np.lib.stride_tricks.as_strided(pay[first:], (rows, cols), (pitch * pay.itemsize, pay.itemsize))


def ringing_payload(h, w, layout, depth, seed, fields=None, rect=None, dtype=None, shift=0):
    """A payload every entry of whose plane table is a ``ringing_plane`` of its own."""
    g = np.random.RandomState(seed)
    out = np.zeros(y4m.payload_size(h, w, layout), dtype or (np.uint8 if depth == 8 else np.uint16))
    for n, entry in enumerate(DB.plane_table(h, w, layout, fields, rect)):
        plane_view(out, entry)[...] = ringing_plane(entry[1], entry[2], depth, 10 * seed + n, g, shift, out.dtype)
    return out


def ringing_clip(n, h, w, layout, d, seed=0, fps=b'24:1'):
    """A Y4M stream of ``ringing_payload`` frames whose bars move 3 samples a frame under noise that differs in every frame.  Returns
    (bytes, payloads as sample arrays); the header is that of the clips of tests/test_gpu_y4m_layouts.py."""
    from tests import test_gpu_y4m_layouts as Y
    data = Y._clip(1, h, w, layout, d, seed=seed, fps=fps)[0]
    pays = []
    for f in range(n):
        g = np.random.RandomState(3000 + 17 * seed + f)
        out = np.zeros(y4m.payload_size(h, w, layout), np.uint8 if d == 8 else np.uint16)
        for m, entry in enumerate(DB.plane_table(h, w, layout)):
            plane_view(out, entry)[...] = ringing_plane(entry[1], entry[2], d, 10 * seed + m, g, 3 * f, out.dtype)
        pays.append(out)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def clamp_payload():
    """The hand-built plane on which the clamp acts, as a 16 x 16 mono payload for 15:4:6."""
    return clamp_plane().reshape(-1)


def coverage(pays, h, w, depth, layout, psd=DR.DEFAULTS, fields=None, rect=None):
    """From the numpy definition alone, over every entry of every payload: the share of the blocks with each direction [8], with var == 0
    and with t > 0; the share of the samples with a tap outside the plane, and the number of samples the clamp acted on."""
    dirs, flat, t, outside, clamped, samples = np.zeros(8), 0, 0, 0, 0, 0
    for pay in pays:
        for entry in DB.plane_table(h, w, layout, fields, rect):
            c = DR.plane_cases(plane_view(pay, entry), depth, *psd, left=entry[4], top=entry[5])
            dirs += np.bincount(c['dir'].reshape(-1), minlength=8)
            flat, t = flat + c['flat'].sum(), t + (c['t'] > 0).sum()
            outside, clamped, samples = outside + c['outside'].sum(), clamped + c['clamped'].sum(), samples + c['outside'].size
    blocks = dirs.sum()
    return dirs / blocks, flat / blocks, t / blocks, outside / samples, int(clamped)


def assert_covered(share):
    """Every direction on at least 2 % of the blocks, var == 0 and t > 0 both on at least 5 %, a tap outside the plane on at least 1 % of
    the samples."""
    dirs, flat, t, outside, _ = share
    assert (dirs >= 0.02).all() and flat >= 0.05 and t >= 0.05 and outside >= 0.01, share


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_the_gpu_tests_payloads_cover_the_rule(depth):
    pays = [ringing_payload(96, 160, '444', depth, s) for s in range(4)]
    share = coverage(pays, 96, 160, depth, '444')
    print(share)
    assert_covered(share)
    # the prototype's figures: every direction on at least 6 % of the blocks of such a pattern
    assert (share[0] >= 0.06).all()
    fshare = coverage([ringing_payload(46, 150, '420', depth, 7, 'b', (4, 50, 6, 156))], 46, 150, depth, '420', fields='b', rect=(4, 50, 6, 156))
    assert_covered(fshare)
    # an input of one kind fails the floors
    with pytest.raises(AssertionError):
        assert_covered(coverage([np.full(96 * 160, 50 << (depth - 8), pays[0].dtype)], 96, 160, depth, 'mono'))
    # the clamp acts at least once, through the hand-built payload
    assert coverage([clamp_payload()], 16, 16, 8, 'mono', (15, 4, 6))[4] >= 1


@pytest.mark.parametrize('h,w,layout,d', [(64, 96, '420', 8), (48, 80, '420', 8), (48, 80, '422', 10), (96, 160, '420', 10), (48, 80, '444', 8),
                                          (48, 80, 'mono', 8)])
def test_the_gpu_tests_clip_moves_and_is_filtered(h, w, layout, d):
    data, pays = ringing_clip(6, h, w, layout, d, seed=3)
    assert len(pays) == 6 and pays[0].size == y4m.payload_size(h, w, layout) and data.count(b'FRAME\n') == 6
    out = DR.dering_stream_np(pays, h, w, d, layout)
    changed = np.mean([(o != p).mean() for o, p in zip(out, pays)])
    moved = np.mean([(x != y).mean() for x, y in zip(pays, pays[1:])])
    dirs, flat, t, outside, _ = coverage(pays, h, w, d, layout)
    print(dirs, flat, t, outside, changed, moved)
    assert changed > 0.2 and moved > 0.5 and (dirs > 0).sum() >= 6 and t > 0.3 and outside >= 0.01
