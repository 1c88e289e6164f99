"""The debanding filter in front of the network (``--deband``, ``demfi_amd.deband``) without a GPU: the rule against a scalar reading and
planes computed by hand, what follows from the rule (identity, bounds, affine planes, edges, corners, locality), what it does to bands, the
accumulator bounds, the switch from the command line to the ``EdgeSpec``, the place of the stage in the ingest and the scratch it shares
with the deringing filter, and the inputs of the GPU tests with the proof that they cover the rule."""
import types

import numpy as np
import pytest

from demfi_amd import deband as BA
from demfi_amd import deblock as DB
from demfi_amd import pipeline as P
from demfi_amd import video
from demfi_amd import y4m
from demfi_amd.y4m_edge import Ingest


# ---- a scalar reading of the rule --------------------------------------------------------------------------------------------------------
def by_hand(plane, depth, T, R):
    """The rule, sample by sample -> (out, n, lo, hi): the output, the number of near samples, the least and greatest of them."""
    p = np.asarray(plane).astype(np.int64)
    rows, cols = p.shape
    thr = T << (depth - 8)
    out, cnt, lo, hi = p.copy(), np.ones_like(p), p.copy(), p.copy()
    for y in range(rows):
        for x in range(cols):
            rx, ry, c = min(R, x, cols - 1 - x), min(R, y, rows - 1 - y), int(p[y, x])
            near = [int(p[y + j, x + i]) for j in range(-ry, ry + 1) for i in range(-rx, rx + 1) if abs(int(p[y + j, x + i]) - c) < thr]
            if T:
                assert c in near
                out[y, x], cnt[y, x], lo[y, x], hi[y, x] = (2 * sum(near) + len(near)) // (2 * len(near)), len(near), min(near), max(near)
    return out.astype(np.asarray(plane).dtype), cnt, lo, hi


def test_small_planes_by_hand():
    # one row of a 3 x 5 plane has windows (ry = 1); the first and last column have rx = 0.  T = 2 at 8 bits: near means |v - c| <= 1
    p = np.array([[10, 10, 11, 11, 30], [10, 11, 11, 12, 30], [10, 10, 12, 12, 12]], np.uint8)
    out = BA.deband_plane_np(p, 8, 2, 1)
    # (1, 1): c = 11, window 10 10 11 / 10 11 11 / 10 10 12: all nine near, sum 95, (190 + 9) // 18 = 11
    # (1, 2): c = 11, window 10 11 11 / 11 11 12 / 10 12 12: all near, sum 100, (200 + 9) // 18 = 11
    # (1, 3): c = 12, window 11 11 30 / 11 12 30 / 12 12 12: seven near (30 is not), sum 81, (162 + 7) // 14 = 12
    assert out.tolist() == [[10, 10, 11, 11, 30], [10, 11, 11, 12, 30], [10, 10, 12, 12, 12]]
    # ties go up: a window whose near samples are 10 and 11 in equal number does not exist with c among nine, so take R = 1 on a row
    # pair: c = 10 with the near samples 10 10 10 11 11 11 (a 3 x 3 window, three far ones): sum 63, (126 + 6) // 12 = 11
    p = np.array([[10, 10, 11], [11, 10, 11], [90, 90, 90]], np.uint8)
    assert BA.deband_plane_np(p, 8, 2, 1)[1, 1] == 11 and BA.plane_cases(p, 8, 2, 1)['n'][1, 1] == 6
    # and the mean below a half goes down: 10 10 10 10 11 -> (102 + 5) // 10 = 10
    p = np.array([[90, 10, 90], [10, 10, 10], [90, 11, 90]], np.uint8)
    assert BA.deband_plane_np(p, 8, 2, 1)[1, 1] == 10 and BA.plane_cases(p, 8, 2, 1)['n'][1, 1] == 5
    # a column by hand at 10 bits, T = 2 (thr = 8), R = 2, one column wide: rx = 0 everywhere, ry = 0 1 2 1 0, so a plane with a side of 1
    # is filtered along its other side: 400 404 404 -> (2416 + 3) // 6 = 403; 400 404 404 408 (500 is far) -> (3232 + 4) // 8 = 404;
    # 404 408 (500 is far) -> (1624 + 2) // 4 = 406
    col = np.array([[400], [404], [404], [408], [500]], np.uint16)
    assert BA.deband_plane_np(col, 10, 2, 2)[:, 0].tolist() == [400, 403, 404, 406, 500] == BA.deband_plane_np(col.T.copy(), 10, 2, 2)[0].tolist()
    assert np.array_equal(BA.deband_plane_np(col[:1], 10, 2, 2), col[:1])       # one sample: rx = ry = 0
    # the same column three wide: (2, 1) has rx = 1, ry = 2: 15 samples, rows 400 404 404 408 500 three times: 12 near (500 is 96 away,
    # and |408 - 404| = 4 < 8), sum 3 * 1616 = 4848, (9696 + 12) // 24 = 404
    wide = np.repeat(col, 3, axis=1)
    out = BA.deband_plane_np(wide, 10, 2, 2)
    assert out[2, 1] == 404 and BA.plane_cases(wide, 10, 2, 2)['n'][2, 1] == 12
    # (1, 1): ry = 1, rows 400 404 404: sum 3 * 1208 = 3624, n = 9, (7248 + 9) // 18 = 403; (3, 1): ry = 1, rows 404 408 (500 far): n = 6,
    # sum 3 * 812 = 2436, (4872 + 6) // 12 = 406
    # the first column has rx = 0 and is the column alone; the first row has ry = 0 and is constant
    assert out[1, 1] == 403 and out[3, 1] == 406 and out[:, 0].tolist() == [400, 403, 404, 406, 500] and out[0].tolist() == [400] * 3


@pytest.mark.parametrize('depth,T,R', [(8, 1, 1), (8, 2, 3), (8, 8, 16), (10, 2, 16), (10, 1, 2), (12, 3, 7), (16, 8, 4), (16, 1, 16)])
def test_random_planes_against_the_scalar_reading(depth, T, R):
    g = np.random.RandomState(depth * 100 + T * 17 + R)
    sh, dtype = depth - 8, np.uint8 if depth == 8 else np.uint16
    for rows, cols in ((1, 1), (1, 9), (2, 2), (5, 7), (2 * R + 1, 2 * R + 1), (2 * R, 2 * R + 3), (37, 41)):
        base = g.randint(0, 2, (rows, cols)) * (40 << sh) + (100 << sh)
        p = (base + g.randint(-(2 << sh), (2 << sh) + 1, (rows, cols))).astype(dtype)
        want, n, lo, hi = by_hand(p, depth, T, R)
        got = BA.deband_plane_np(p, depth, T, R)
        assert got.dtype == p.dtype and np.array_equal(got, want)
        c = BA.plane_cases(p, depth, T, R)
        assert np.array_equal(c['n'], n) and np.array_equal(c['changed'], want != p)
        # |out - c| < thr, and out lies between the least and the greatest near sample: no clip is needed
        o, v = got.astype(np.int64), p.astype(np.int64)
        assert (np.abs(o - v) < (T << sh)).all() and (o >= lo).all() and (o <= hi).all()
        ys, xs = np.mgrid[0:rows, 0:cols]
        assert np.array_equal(c['rx'], np.minimum(R, np.minimum(xs, cols - 1 - xs))) and np.array_equal(c['ry'], np.minimum(R, np.minimum(ys, rows - 1 - ys)))


# ---- what follows from the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [8, 10, 16])
def test_identity_constant_corners_and_planes_with_a_side_of_one(depth):
    g = np.random.RandomState(depth)
    dtype = np.uint8 if depth == 8 else np.uint16
    p = g.randint(0, 1 << depth, (40, 50)).astype(dtype)
    for R in (1, 16):
        assert np.array_equal(BA.deband_plane_np(p, depth, 0, R), p) and BA.deband_plane_np(p, depth, 0, R) is not p
    for level in (0, 1, (1 << depth) - 1):
        flat = np.full((40, 50), level, dtype)
        assert np.array_equal(BA.deband_plane_np(flat, depth, 8, 16), flat) and (BA.plane_cases(flat, depth, 8, 16)['n'][20, 25] == 1089)
    noisy = (g.randint(-3, 4, (40, 50)) + (1 << (depth - 1))).astype(dtype)
    out = BA.deband_plane_np(noisy, depth, 8, 16)
    assert not np.array_equal(out, noisy)
    for y, x in ((0, 0), (0, 49), (39, 0), (39, 49)):                     # rx = ry = 0
        assert out[y, x] == noisy[y, x]
    # a plane with a side of 1 has no window across that side and is filtered along the other; a plane of one sample is itself
    assert np.array_equal(BA.deband_plane_np(noisy[:1], depth, 8, 16), by_hand(noisy[:1], depth, 8, 16)[0]) and np.array_equal(BA.deband_plane_np(noisy[:1, :1], depth, 8, 16), noisy[:1, :1])
    assert np.array_equal(BA.deband_plane_np(noisy[:, :1], depth, 8, 16)[:, 0], BA.deband_plane_np(noisy[:, :1].T.copy(), depth, 8, 16)[0])
    assert BA.deband_plane_np(noisy[:1], depth, 8, 16)[0, 0] == noisy[0, 0] and BA.deband_plane_np(noisy[:1], depth, 8, 16)[0, -1] == noisy[0, -1]
    # a legal sample stays legal: the extremes of the range
    edge = np.where(g.randint(0, 2, (40, 50)) > 0, (1 << depth) - 1 - g.randint(0, 3, (40, 50)), g.randint(0, 3, (40, 50))).astype(dtype)
    out = BA.deband_plane_np(edge, depth, 8, 16).astype(np.int64)
    assert out.min() >= 0 and out.max() <= (1 << depth) - 1


@pytest.mark.parametrize('R', [1, 4, 16])
def test_every_affine_plane_comes_back_exactly(R):
    """N is point-symmetric about c: with (x + i, y + j) it holds (x - i, y - j), whose values add up to 2 c.  Planes whose sides are below,
    equal to and above 2R + 1; slopes that keep the whole window within thr, slopes that cut it, and slopes beyond thr."""
    side = 2 * R + 1
    for rows, cols in ((side - 1, side + 5), (side, side), (side + 7, side - 1), (side + 9, side + 12), (3, 70)):
        yy, xx = np.mgrid[0:rows, 0:cols].astype(np.int64)
        for a, b, e in ((1, 0, 5), (0, 1, 0), (1, 1, 100), (3, -2, 300), (-7, 5, 900), (40, 0, 0), (0, -33, 3000), (2, 9, 17), (-1, -1, 200)):
            p = a * xx + b * yy + e
            p = (p - min(int(p.min()), 0)).astype(np.uint16)
            for depth, T in ((10, 2), (10, 8), (16, 1), (12, 3)):
                assert np.array_equal(BA.deband_plane_np(p, depth, T, R), p), (rows, cols, a, b, depth, T)
    # an edge-clamped window has no such property: the reading that clamps the window at the border instead changes a ramp's border
    yy, xx = np.mgrid[0:side + 9, 0:side + 12].astype(np.int64)
    p = (xx + 100).astype(np.uint16)
    x, c = 1, 101
    clamped = [int(p[0, i]) for i in range(0, x + R + 1) if abs(int(p[0, i]) - c) < 8]
    assert (2 * sum(clamped) + len(clamped)) // (2 * len(clamped)) != c or R == 1


def test_a_step_of_thr_or_more_is_an_edge_and_one_below_is_not():
    for depth, T in ((8, 2), (10, 2), (16, 8)):
        thr, dtype = T << (depth - 8), np.uint8 if depth == 8 else np.uint16
        g = np.random.RandomState(T)
        left = g.randint(0, thr // 2 + 1, (40, 30)) + (50 << (depth - 8))
        for step, edge in ((thr + thr // 2, True), (thr // 2, False)):
            right = g.randint(0, thr // 2 + 1, (40, 34)) + (50 << (depth - 8)) + thr // 2 + step
            p = np.concatenate([left, right], 1).astype(dtype)
            out = BA.deband_plane_np(p, depth, T, 16)
            alone = np.concatenate([BA.deband_plane_np(p[:, :30], depth, T, 16), BA.deband_plane_np(p[:, 30:], depth, T, 16)], 1)
            # with the other side out of reach every sample sees what a window cut at the step would see: but such a cut window is not
            # the symmetric one, so compare with the other side replaced by far values instead
            far = p.copy().astype(np.int64)
            far[:, 30:] += 20 * thr
            lone = BA.deband_plane_np(far.astype(np.uint16 if depth > 8 else np.int64), depth, T, 16).astype(np.int64)
            same = np.array_equal(out[:, :30].astype(np.int64), lone[:, :30]) and np.array_equal(out[:, 30:].astype(np.int64), lone[:, 30:] - 20 * thr)
            assert same == edge, (depth, T, step)
            assert alone.shape == out.shape


def test_an_output_depends_on_its_window_and_on_nothing_else():
    g = np.random.RandomState(5)
    R, y, x = 4, 20, 22
    p = (g.randint(-3, 4, (41, 45)) + 512).astype(np.uint16)
    base = BA.deband_plane_np(p, 10, 2, R)
    for dy, dx, inside in ((R, R, True), (-R, 0, True), (0, -R, True), (R + 1, 0, False), (0, R + 1, False), (-R - 1, -R - 1, False), (R, R + 1, False)):
        q = p.copy()
        q[y + dy, x + dx] = 512 + 3 if p[y + dy, x + dx] != 515 else 509
        # enough of a change to move the mean of 81 samples?  not always; what must hold is the other direction
        out = BA.deband_plane_np(q, 10, 2, R)
        if not inside:
            assert out[y, x] == base[y, x]
    q = p.copy()
    q[y - R:y + R + 1, x - R:x + R + 1] = 519                             # the whole window (c too): the output follows
    assert BA.deband_plane_np(q, 10, 2, R)[y, x] == 519 != base[y, x]
    q = np.full_like(p, 519)
    q[y - R:y + R + 1, x - R:x + R + 1] = p[y - R:y + R + 1, x - R:x + R + 1]      # everything but the window: it does not
    assert BA.deband_plane_np(q, 10, 2, R)[y, x] == base[y, x]


# ---- what the rule does to bands ---------------------------------------------------------------------------------------------------------
def ramp(width, rows=80, cols=300, diagonal=False):
    """(input, true): an 8-bit ramp promoted to 10 bits whose plateaus are ``width`` samples wide (diagonal: (2x + y) / 40), and the ramp
    it was quantised from, at 10 bits."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    t = ((2 * xx + yy) / 40 if diagonal else xx / width) + 50
    return (np.round(t).astype(np.int64) << 2).astype(np.uint16), 4 * t


CASES = [(16, False), (24, False), (32, False), (0, True), (64, False)]


@pytest.mark.parametrize('width,diagonal', CASES, ids=['16', '24', '32', 'diagonal', '64'])
def test_bands_become_ramps(width, diagonal):
    inp, true = ramp(width, diagonal=diagonal)
    out = BA.deband_plane_np(inp, 10, *BA.DEFAULTS).astype(np.int64)
    inner = (slice(16, -16), slice(16, -16))                              # the samples with a whole window
    o, i, t = out[inner], inp[inner].astype(np.int64), true[inner]
    dx, dy = np.diff(o, axis=1), np.diff(o, axis=0)
    d_in, d_out = np.abs(i - t).mean(), np.abs(o - t).mean()
    print(width, diagonal, d_in, d_out, dx.min(), dx.max(), dy.min(), dy.max())
    assert np.diff(i, axis=1).max() == 4                                  # the input's steps
    assert dx.min() >= 0 and dy.min() >= 0 and dx.max() <= 1 and dy.max() <= 1     # monotone, no step above one code
    assert d_out <= d_in
    if width in (16, 32):
        assert d_out <= 0.3                                               # the rounding floor of 10 bits is 0.25; plateaus of 24 give 0.26 to 0.28
    if width == 64:
        assert (dx == 0).mean() > 0.8                                     # a flat middle stays


def test_narrow_bands_and_equal_depths_come_back_unchanged():
    for width in (2, 4, 6):                                               # below R / T = 8: every band within thr lies wholly inside the window
        inp, _ = ramp(width)
        out = BA.deband_plane_np(inp, 10, *BA.DEFAULTS)
        assert np.array_equal(out[16:-16, 16:-16], inp[16:-16, 16:-16])
    for width in (16, 24, 32):                                            # a band of one code at equal input and working depth rounds to itself
        yy, xx = np.mgrid[0:80, 0:300]
        p = np.round(xx / width + 50).astype(np.uint8)
        assert np.array_equal(BA.deband_plane_np(p, 8, *BA.DEFAULTS), p)
    # and fine detail pays: uniform noise of +-3 codes loses standard deviation as T grows
    g = np.random.RandomState(0)
    noise = (g.randint(-3, 4, (120, 160)) + 128).astype(np.uint8)
    left = [BA.deband_plane_np(noise, 8, T, 16)[16:-16, 16:-16].std() / noise[16:-16, 16:-16].std() for T in (1, 2, 3, 4)]
    print(left)
    assert left[0] == 1.0 and 1.0 > left[1] > left[2] > left[3] > 0.3


# ---- the parameters ----------------------------------------------------------------------------------------------------------------------
def test_parse_deband_check_params_and_thresholds():
    assert BA.DEFAULTS == (2, 16) and BA.parse_deband('2:16') == (2, 16) and BA.parse_deband(' 3 ') == (3, 16) and BA.parse_deband('8:1') == (8, 1)
    assert BA.parse_deband('0') == (0, 16) and BA.parse_deband('0:5') == (0, 5) and BA.parse_deband('1:7') == (1, 7)
    assert BA.check_params() == (2, 16) and BA.check_params(np.int64(4), np.int32(9)) == (4, 9) and BA.check_params(1) == (1, 16)
    for bad in ('', 'x', '2:', ':2', '9', '2:0', '2:17', '-1', '2:16:1', '1.5', '2:x'):
        with pytest.raises(ValueError):
            BA.parse_deband(bad)
    for bad in ((-1,), (9,), (2, 0), (2, 17), (2, -1), (True,), (2.0,), (2, 16.0), (2, True)):
        with pytest.raises(ValueError):
            BA.check_params(*bad)
    assert [BA.thresholds(d, 2) for d in (8, 10, 12, 14, 16)] == [2, 8, 32, 128, 512] and BA.thresholds(16, 8) == 2048 and BA.thresholds(10, 0) == 0
    with pytest.raises(ValueError):
        BA.thresholds(9, 2)
    with pytest.raises(ValueError):
        BA.plane_cases(np.zeros((3, 3), np.uint8), 8, 0, 1)
    with pytest.raises(ValueError):
        BA.deband_plane_np(np.zeros(3, np.uint8), 8)
    with pytest.raises(ValueError):
        BA.deband_payload_np(np.zeros(7, np.uint8), 4, 4, 8, '420')


def test_the_accumulator_bounds_by_brute_force():
    n, total, d, num = BA.accumulator_bounds()
    assert (n, total, d, num) == (1089, 1089 * 65535, 1089 * 2047, 1089 * (4 * 2048 - 3))
    assert total < 2 ** 27 and d < 2 ** 22 and num < 2 ** 24 and BA.MAX_N == 1089
    assert BA.accumulator_bounds(8, 1, 1) == (9, 9 * 65535, 0, 9)
    # the extremes are reached: a plane of 65535 (n and the sum), the count payload (|D| = (n - 1)(thr - 1), one sample short of the bound)
    c = BA.plane_cases(np.full((33, 33), 65535, np.uint16), 16, 8, 16)
    assert c['n'][16, 16] == n and int(c['n'][16, 16]) * 65535 == total and c['D'][16, 16] == 0
    pay, h, w, centres = count_payload(16, 8, 16)
    c = BA.plane_cases(pay.reshape(h, w), 16, 8, 16)
    ds = [int(c['D'][y, x]) for y, x, _, _ in centres]
    assert max(ds) == 1088 * 2047 == -min(ds) and max(ds) <= d
    # and nothing goes beyond them: every depth, threshold and radius, on planes of the extremes of the range and of noise about a level
    g = np.random.RandomState(1)
    for depth, T, R in ((8, 8, 2), (10, 8, 3), (16, 8, 5), (16, 1, 16), (12, 5, 16)):
        thr = T << (depth - 8)
        for p in (g.randint(0, 2, (40, 40)) * 65535, 65535 - g.randint(0, thr, (40, 40)), g.randint(0, thr, (40, 40)), g.randint(0, 65536, (40, 40))):
            c = BA.plane_cases(p.astype(np.uint16), depth, T, R)
            bn, bt, bd, bnum = BA.accumulator_bounds(depth, T, R)
            assert c['n'].max() <= bn and (c['n'] >= 1).all() and (np.abs(c['D']) <= c['n'] * (thr - 1)).all() and np.abs(c['D']).max() <= bd
            e_sum = c['D'] + c['n'] * (thr - 1)                           # what the kernel sums: e = v - c + thr - 1 >= 0
            assert e_sum.min() >= 0 and (2 * e_sum + c['n']).max() <= bnum
            # the difference form and the kernel's biased form are the definition
            v = p.astype(np.int64)
            out = BA.deband_plane_np(p.astype(np.uint16), depth, T, R).astype(np.int64)
            assert np.array_equal(out, v + (2 * c['D'] + c['n']) // (2 * c['n']))
            assert np.array_equal(out, v - (thr - 1) + (2 * e_sum + c['n']) // (2 * c['n']))


def test_fields_are_planes_of_their_own():
    h, w = 40, 48
    pay = banded_payload(h, w, '420', 10, 3)
    out = BA.deband_payload_np(pay, h, w, 10, '420', 2, 4, fields='t')
    luma, got = pay[:h * w].reshape(h, w), out[:h * w].reshape(h, w)
    for q in (0, 1):                                                      # R counts field rows
        assert np.array_equal(got[q::2], BA.deband_plane_np(luma[q::2], 10, 2, 4))
    assert not np.array_equal(out, BA.deband_payload_np(pay, h, w, 10, '420', 2, 4))
    # the phases of a crop rectangle are carried and ignored
    assert np.array_equal(BA.deband_payload_np(pay, h, w, 10, '420', 2, 4, rect=(4, 44, 6, 54)), BA.deband_payload_np(pay, h, w, 10, '420', 2, 4))
    assert [len(e) for e in DB.plane_table(h, w, '420', 't', (4, 44, 6, 54))] == [6] * 6
    outs = BA.deband_stream_np([pay, pay[::-1].copy()], h, w, 10, '420', 2, 4)
    assert np.array_equal(outs[0], BA.deband_payload_np(pay, h, w, 10, '420', 2, 4)) and len(outs) == 2
    assert np.array_equal(BA.deband_payload_np(pay, h, w, 10, '420', 0, 4), pay)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------
def test_edge_spec_with_deband_dering_and_deblock():
    args = (True, True, False, 10, '422', None, 't', 'adaptive')
    plain = P.EdgeSpec(*args)
    bd = P.EdgeSpec(*args, deband=(2, 16))
    assert bd.deband == (2, 16) and plain.deband is None and tuple(bd) == tuple(plain) and len(plain) == 8
    assert bd != plain and plain != bd and bd != tuple(bd) and plain == tuple(plain)
    assert hash(plain) == hash((tuple(plain), None))                      # as before there was the field
    assert bd == P.EdgeSpec(*args, deband=[2, 16]) and hash(bd) == hash(bd._replace())
    assert bd != bd._replace(deband=(2, 8)) and bd._replace(deband=None) == plain and plain._replace(deband=(2, 16)) == bd
    assert 'deband=(2, 16)' in repr(bd) and 'deband' not in repr(plain) and repr(plain) == repr(bd._replace(deband=None))
    for none in ((0, 16), (0, 1), None):                                  # T = 0: no stage
        assert P.EdgeSpec(True, deband=none) == P.EdgeSpec(True) and P.EdgeSpec(True, deband=none).deband is None
        assert hash(P.EdgeSpec(True, deband=none)) == hash(P.EdgeSpec(True)) and repr(P.EdgeSpec(True, deband=none)) == repr(P.EdgeSpec(True))
    seen = set()
    for db in (None, (16, 4)):
        for dr in (None, (4, 2, 5)):
            for d in (None, (2, 16)):
                spec = P.EdgeSpec(*args, deblock=db, dering=dr, deband=d)
                assert (spec.deblock, spec.dering, spec.deband) == (db, dr, d)
                assert spec == plain._replace(deband=d)._replace(dering=dr)._replace(deblock=db) and spec._replace(depth=8).deband == d
                assert spec._replace(deband=None) == P.EdgeSpec(*args, deblock=db, dering=dr)
                assert ('deband' in repr(spec)) == (d is not None) and ('dering' in repr(spec)) == (dr is not None)
                if d is None:
                    assert repr(spec) == repr(P.EdgeSpec(*args, deblock=db, dering=dr)) and hash(spec) == hash(P.EdgeSpec(*args, deblock=db, dering=dr))
                seen.add(spec)
    assert len(seen) == 8
    assert bd.reach == plain.reach == 2 and P.EdgeSpec(True, deband=(2, 16)).reach == 0             # no look-ahead of its own
    edge = video.YuvEdge('bt601', False, '420jpeg', None, deband=(3, 8))
    assert edge.deband == (3, 8) and edge.dering is None and P.EdgeSpec.of(edge).deband == (3, 8)
    plain_edge = video.YuvEdge('bt601', False, '420jpeg', None)
    assert plain_edge.deband is None and P.EdgeSpec.of(plain_edge) == P.EdgeSpec(True)
    assert video.YuvEdge('bt601', False, '420jpeg', None, deband=(0, 4)).deband is None
    with pytest.raises(ValueError):
        video.YuvEdge('bt601', False, '420jpeg', None, deband=(2, 17))
    bd.check(True, True, True)                                            # nothing is refused
    P.EdgeSpec(True, True, True, 16, '444', (7, 5, 0, 4), 't', 'bob', dering=(4, 2, 5), deblock=(16, 4), deband=(8, 1)).check(True, True, True)
    P.EdgeSpec(True, denoise=(5, 10, 2), deband=(2, 16), shutter=(2, 4), grain=(16, 1, 8, 'film', 0)).check(True, False, True)
    for spec, a, msg in ((P.EdgeSpec(True, deband=(9, 16)), (True, False, True), 'deband must be'),
                         (P.EdgeSpec(True, deband=(2, 17)), (True, False, True), 'deband must be'),
                         (P.EdgeSpec(True, deband=(2, 0)), (True, False, True), 'deband must be'),
                         (P.EdgeSpec(True, deband=(2, 16, 1)), (True, False, True), 'deband must be'),
                         (P.EdgeSpec(False, deband=(2, 16)), (False, False, True), 'Y4M edge')):
        with pytest.raises(ValueError, match=msg):
            spec.check(*a)


def test_runner_arguments_and_counter():
    vr = video.VideoRunner(None)
    assert vr.deband is None and vr.last_debanded == 0
    assert video.VideoRunner(None, deband=True).deband == (2, 16) and video.VideoRunner(None, deband=False).deband is None
    assert video.VideoRunner(None, deband=3).deband == (3, 16) and video.VideoRunner(None, deband='4:8').deband == (4, 8)
    assert video.VideoRunner(None, deband=(1, 2)).deband == (1, 2) and video.VideoRunner(None, deband=(0, 4)).deband is None
    assert video.VideoRunner(None, deband=0).deband is None and video.VideoRunner(None, deband='0').deband is None
    assert video.check_deband(None) is None and video.check_deband((8, None)) == (8, 16) and video.check_deband('1:1') == (1, 1)
    assert video.check_deband([2, 5]) == (2, 5) and video.check_deband(np.int64(0)) is None if isinstance(np.int64(0), int) else True
    vr = video.VideoRunner(None, deband=True, dedup=True, deinterlace=True)
    assert vr.deband == (2, 16) and vr._behind('t') == 0                  # no look-ahead
    vr = video.VideoRunner(None, deband=True, dering=True, deblock=True, deinterlace=True, deinterlace_mode='adaptive', tile='auto',
                           high_depth=True, tile_high_depth=True, layouts=True, work_depth=12)
    assert vr._behind('t') == 2 and (vr.deblock, vr.dering, vr.deband) == ((16, 4), (4, 2, 5), (2, 16))
    video.VideoRunner(None, deband=True)                                  # not refused without a working depth
    video.check_one_rank(4, deband=(2, 16))                               # any number of ranks
    assert 'deband' not in video.ONE_RANK and 'deband' not in video.ONE_RANK_EGRESS
    for kw, msg in ((dict(deband=9), '0 .. 8'), (dict(deband=(2, 17)), 'radius'), (dict(deband=(1, 2, 3)), 'deband must be'),
                    (dict(deband=2.5), 'deband must be'), (dict(deband='x'), 'expected T'), (dict(deband=(2, 0)), 'radius')):
        with pytest.raises(ValueError, match=msg):
            video.VideoRunner(None, **kw)
    assert video.INGEST_COUNTERS['debanded'] == 'last_debanded' and video.INGEST_COUNTERS['deringed'] == 'last_deringed'
    vr = video.VideoRunner(None, mfi=2, deband=True)
    vr._counted(types.SimpleNamespace(w=96, h=64, layout='420'), dict({name: 0 for name in video.COUNTERS}, debanded=9), [], 0)
    assert vr.last_debanded == 9 and vr.last_deringed == 0
    import inspect
    from demfi_amd.runner import WindowRunner
    assert 'self.debanded = 0' in inspect.getsource(WindowRunner.__init__)
    hdr = y4m.Header(96, 64, 25, 'p', None, '420jpeg', None, (), '420jpeg', 8, '420')
    edge = video.VideoRunner(None, mfi=2, deband='3:5')._edge(hdr, None)
    assert edge.deband == (3, 5) and edge.dering is None and edge.crop_rect is None


def test_command_line(capsys):
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).deband is None and p.parse_args(['-', '-', '--deband']).deband == (2, 16)
    assert p.parse_args(['a', 'b', '--deband', '3']).deband == (3, 16) and p.parse_args(['a', 'b', '--deband', '4:8', '--dedup']).deband == (4, 8)
    assert p.parse_args(['a', 'b', '--deband', '0']).deband == (0, 16)
    a = p.parse_args(['a', 'b', '--work-depth', '10', '--out-depth', '10', '--deblock', '--dering', '--deband'])
    assert (a.deblock, a.dering, a.deband, a.work_depth) == ((16, 4), (4, 2, 5), (2, 16), 10)
    text = ' '.join(p.format_help().split())
    assert '--deband' in text and '--work-depth 10' in text and 'not tuned against this network' in text
    for argv, msg in ((['a.y4m', 'b.y4m', '--deband', '9'], '0 .. 8'), (['a.y4m', 'b.y4m', '--deband', '2:17'], 'radius'),
                      (['a.y4m', 'b.y4m', '--deband', 'x'], 'expected T')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
    from demfi_amd import clip
    with pytest.raises(SystemExit) as ex:                                 # the folder path has no such switch
        clip.parser().parse_args(['frames', '--deband'])
    assert ex.value.code == 2
    for doc in (video.__doc__, video.VideoRunner.__doc__, BA.__doc__):
        assert 'deband' in doc and 'tuned' in doc and 'work' in doc


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
    rn = types.SimpleNamespace(lib=_FakeLib(on_call), engine=types.SimpleNamespace(device='cpu'), depth_promoted=0, denoised=0, deblocked=0, deringed=0,
                               debanded=0)
    return Ingest(rn, P.FrameSlots(nslot, 2, 2, 'cpu'), spec, h, w), rn


def test_the_ingest_order_the_scratch_copy_and_the_shared_scratch(monkeypatch):
    import torch
    spec = P.EdgeSpec(True, depth=10, fields='t', denoise=(5, 10, 1), deblock=(16, 4), dering=(6, 3, 4), deband=(3, 5), depths=(8, 10, 10, None))
    seen = {}

    def on_call(name, args):                                              # at each launch the scratch already holds what the stage reads
        if name in ('demfi_payload_dering', 'demfi_payload_deband'):
            seen[name] = ing.bd_scratch[:6].clone()
            ing.yuv_in[:6] += 1                                           # "the stage": the next copy must pick this up
    ing, rn = _ingest(spec, monkeypatch, on_call=on_call)
    assert ing.bd_scratch is ing.dr_scratch                               # one buffer serves both
    ing.attach(types.SimpleNamespace(full_range=False, crop_rect=(4, 16, 6, 26)))
    ing.yuv_in.copy_(torch.arange(ing.yuv_in.numel(), dtype=torch.int64).reshape(ing.yuv_in.shape) % 199)
    start = ing.yuv_in[:6].clone()
    ing.bd_scratch.zero_()
    stream = types.SimpleNamespace(cuda_stream=0)
    near = ing.around({2, 3}, lambda g: g < 6)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2, 3})]
    assert [sl for _, sl in new] == list(range(6))
    done = ing.rebuilt(new, stream)
    names = [name for name, _ in rn.lib.calls]
    assert names == ['demfi_payload_promote', 'demfi_payload_deblock', 'demfi_payload_dering', 'demfi_payload_deband', 'demfi_yuv_bob',
                     'demfi_payload_denoise']
    assert [f for f, _ in done] == [2, 3] and (rn.depth_promoted, rn.deblocked, rn.deringed, rn.debanded, rn.denoised) == (6, 6, 6, 6, 2)
    assert bool((seen['demfi_payload_dering'] == start).all()) and bool((seen['demfi_payload_deband'] == start + 1).all())     # in order
    args = dict(rn.lib.calls)['demfi_payload_deband']
    assert args[0] == ing.bd_scratch[0].data_ptr() and args[2] == ing.yuv_in[0].data_ptr() and args[1] == args[3] == ing.Pb == 2 * y4m.payload_size(12, 20)
    assert args[4] == 6 and ing.bd_scratch.shape == ing.yuv_in.shape and ing.bd_scratch.dtype == ing.yuv_in.dtype
    assert not bool((ing.bd_scratch[6:] != 0).any())
    tab = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int64 * (6 * args[6])).from_address(args[5])).reshape(-1, 6)
    assert tab.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))] and args[6] == 6
    assert args[7:11] == (2, 10, 3, 5) and len(args) == 12                # sample size, working depth, T at the 8-bit scale, R; the stream
    # two runs of slots: two copies and two launches; nothing new: none
    rn.lib.calls.clear()
    ing.debanded([(8, 1), (9, 2), (11, 5)], stream)
    assert [(name, a[0] - ing.bd_scratch.data_ptr(), a[2] - ing.yuv_in.data_ptr(), a[4]) for name, a in rn.lib.calls] == [
        ('demfi_payload_deband', ing.Pb, ing.Pb, 2), ('demfi_payload_deband', 5 * ing.Pb, 5 * ing.Pb, 1)]
    rn.lib.calls.clear()
    ing.debanded([], stream)
    assert not rn.lib.calls and rn.debanded == 9


def test_alone_and_in_every_combination_with_deblock_and_dering(monkeypatch):
    stream = types.SimpleNamespace(cuda_stream=0)
    for db in (None, (16, 4)):
        for dr in (None, (4, 2, 5)):
            for bd in (None, (2, 16)):
                ing, rn = _ingest(P.EdgeSpec(True, fields='b', deint_mode='adaptive', deblock=db, dering=dr, deband=bd), monkeypatch)
                near = ing.around({2}, lambda g: g < 8)
                new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2})]
                ing.rebuilt(new, stream)
                want = [n for n, on in (('demfi_payload_deblock', db), ('demfi_payload_dering', dr), ('demfi_payload_deband', bd)) if on is not None]
                assert [name for name, _ in rn.lib.calls] == want + ['demfi_yuv_deint_adaptive']
                assert (rn.deblocked, rn.deringed, rn.debanded) == tuple(len(new) if on is not None else 0 for on in (db, dr, bd))
                assert hasattr(ing, 'dr_scratch') == (dr is not None) and hasattr(ing, 'bd_scratch') == (bd is not None)
                assert hasattr(ing, 'bd_planes') == (bd is not None) and hasattr(ing, 'dr_planes') == (dr is not None)
                if bd is not None:
                    assert (ing.bd_scratch is getattr(ing, 'dr_scratch', None)) == (dr is not None) and ing.bd_scratch.shape == ing.yuv_in.shape
                    assert ing.bd_planes.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 'b')] and ing.deband == (8, 2, 16)
                else:
                    assert ing.deband is None
    ing, rn = _ingest(P.EdgeSpec(True, dedup=(7, 5, 0, 4), fields='t', deband=(2, 16)), monkeypatch)
    ing.rebuilt([(0, 3)], stream)
    assert [name for name, _ in rn.lib.calls] == ['demfi_payload_deband', 'demfi_yuv_bob'] and rn.debanded == 1


def test_without_the_switch_the_ingest_is_what_it_was(monkeypatch):
    assert object.__new__(Ingest).deband is None
    for spec in (P.EdgeSpec(True, fields='t'), P.EdgeSpec(True, deband=(0, 16), fields='t'), P.EdgeSpec(True, dering=(4, 2, 5), fields='t')):
        ing, rn = _ingest(spec, monkeypatch)
        assert ing.deband is None and not hasattr(ing, 'bd_planes') and not hasattr(ing, 'bd_scratch')
        ing.attach(types.SimpleNamespace(full_range=True, crop_rect=(4, 16, 6, 26)))
        assert ing.full_range is True and not hasattr(ing, 'bd_planes')
        ing.rebuilt([(0, 0), (1, 1)], types.SimpleNamespace(cuda_stream=0))
        assert 'demfi_payload_deband' not in [name for name, _ in rn.lib.calls] and rn.debanded == 0


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
CELL = 24


def banded_plane(rows, cols, depth, seed, noise, shift=0, dtype=None):
    """Cells of 24 x 24 samples of eight kinds: 8-bit ramps promoted to ``depth`` with plateaus 16, 24 and 32 samples wide, a diagonal one
    ((2x + y) / 40), a vertical one of 12 rows, texture (noise of +-3 codes at 10 bits and below, scaled up above) about a level, hard
    edges (bars of 40 and 200 every 5 samples) and a flat cell.  ``shift`` moves the whole pattern to the left; ``noise``: the generator
    of the texture, which does not move."""
    sh = depth - 8
    kind = np.random.RandomState(seed).randint(0, 8, (64, 64))
    yy, xx = np.mgrid[0:rows, 0:cols]
    xx = xx + shift
    k = kind[(yy // CELL) % 64, (xx // CELL) % 64]
    ramps = (60 + xx / 16, 60 + xx / 24, 90 + xx / 32, 120 + (2 * xx + yy) / 40, 150 + yy / 12)
    v = np.select([k == i for i in range(5)], [np.round(r).astype(np.int64) % 256 << sh for r in ramps], 0)
    s = 1 << max(sh - 2, 0)
    v = np.where(k == 5, (128 << sh) + noise.randint(-3 * s, 3 * s + 1, (rows, cols)), v)
    v = np.where(k == 6, np.where((xx + yy // 2) % 10 < 5, 40, 200) << sh, v)
    v = np.where(k == 7, 180 << sh, v)
    return v.astype(dtype or (np.uint8 if depth == 8 else np.uint16))


def plane_view(pay, entry):
    """The [rows, cols] view of one entry of a plane table into the flat payload ``pay``."""
    first, rows, cols, pitch = entry[:4]
    return np.lib.stride_tricks.as_strided(pay[first:], (rows, cols), (pitch * pay.itemsize, pay.itemsize))


def banded_payload(h, w, layout, depth, seed, fields=None, rect=None, dtype=None, shift=0):
    """A payload every entry of whose plane table is a ``banded_plane`` of its own."""
    g = np.random.RandomState(seed)
    out = np.zeros(y4m.payload_size(h, w, layout), dtype or (np.uint8 if depth == 8 else np.uint16))
    for n, entry in enumerate(DB.plane_table(h, w, layout, fields, rect)):
        plane_view(out, entry)[...] = banded_plane(entry[1], entry[2], depth, 10 * seed + n, g, shift, out.dtype)
    return out


def banded_clip(n, h, w, layout, d, seed=0, fps=b'24:1'):
    """A Y4M stream of ``banded_payload`` frames whose bands move 3 samples a frame under texture that differs in every frame.  Returns
    (bytes, payloads as sample arrays); the header is that of the clips of tests/test_gpu_y4m_layouts.py."""
    from tests import test_gpu_y4m_layouts as Y
    data = Y._clip(1, h, w, layout, d, seed=seed, fps=fps)[0]
    pays = []
    for f in range(n):
        g = np.random.RandomState(4000 + 17 * seed + f)
        out = np.zeros(y4m.payload_size(h, w, layout), np.uint8 if d == 8 else np.uint16)
        for m, entry in enumerate(DB.plane_table(h, w, layout)):
            plane_view(out, entry)[...] = banded_plane(entry[1], entry[2], d, 10 * seed + m, g, 3 * f, out.dtype)
        pays.append(out)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def count_ns(r):
    """The numbers of near samples the count payload of radius ``r`` holds a patch for: every n up to (2r + 1)^2 for r <= 4; above, 1, 2,
    the last two and one in every 64 between."""
    top = (2 * r + 1) ** 2
    return list(range(1, top + 1)) if r <= 4 else sorted({1, 2, top - 1, top} | set(range(33, top, 64)))


def count_payload(depth, t, r, dtype=None):
    """A mono payload of isolated patches of (2r + 1)^2 samples on a far background: the centre c of a patch sees exactly n near samples,
    itself and the first n - 1 others of its window in raster order, which all hold c + thr - 1 or all c - (thr - 1): both extremes of D for
    that n, and both extremes of the quotient's numerator.  Returns (payload, h, w, [(y, x, n, sign)])."""
    sh, side, thr = depth - 8, 2 * r + 1, t << (depth - 8)
    todo = [(n, sign) for n in count_ns(r) for sign in (1, -1)]
    per_row = int(np.ceil(np.sqrt(len(todo))))
    h, w = side * ((len(todo) + per_row - 1) // per_row), side * per_row
    c, far = 100 << sh, 160 << sh
    plane = np.full((h, w), far, np.int64)
    centres = []
    for m, (n, sign) in enumerate(todo):
        y0, x0 = side * (m // per_row), side * (m % per_row)
        patch = np.full(side * side, far, np.int64)
        others = [i for i in range(side * side) if i != side * r + r][:n - 1]
        patch[others] = c + sign * (thr - 1)
        patch[side * r + r] = c
        plane[y0:y0 + side, x0:x0 + side] = patch.reshape(side, side)
        centres.append((y0 + r, x0 + r, n, sign))
    return plane.reshape(-1).astype(dtype or (np.uint8 if depth == 8 else np.uint16)), h, w, centres


@pytest.mark.parametrize('depth,t', [(8, 1), (8, 8), (10, 2), (16, 8)])
@pytest.mark.parametrize('r', [1, 2, 4, 16])
def test_the_count_payload_reaches_every_n_at_both_extremes(r, depth, t):
    pay, h, w, centres = count_payload(depth, t, r)
    thr = t << (depth - 8)
    c = BA.plane_cases(pay.reshape(h, w), depth, t, r)
    got = {}
    for y, x, n, sign in centres:
        assert c['n'][y, x] == n and c['D'][y, x] == sign * (n - 1) * (thr - 1) and (c['rx'][y, x], c['ry'][y, x]) == (r, r)
        got.setdefault(n, set()).add(sign)
    top = (2 * r + 1) ** 2
    if r <= 4:
        assert sorted(got) == list(range(1, top + 1))
    else:
        assert {1, 2, top - 1, top} <= set(got) and all(any(lo <= n < lo + 64 for n in got) for lo in range(1, top - 63))
    assert all(s == {1, -1} for s in got.values())
    out = BA.deband_plane_np(pay.reshape(h, w), depth, t, r)
    changed = [bool(c['changed'][y, x]) for y, x, _, _ in centres]
    if thr > 2:
        assert any(changed) and not all(changed)                          # n = 1 stays; a full patch moves the centre
    assert np.array_equal(out != pay.reshape(h, w), c['changed'])


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_the_gpu_tests_payloads_cover_the_rule(depth):
    """Every (rx, ry) pair, samples that change and that do not, and a wide spread of n, through ``plane_cases``."""
    for r in (1, 2, 7, 16):
        pairs, ns, changed, total = set(), set(), 0, 0
        for seed in range(2):
            pay = banded_payload(90, 150, '444', depth, seed)
            for entry in DB.plane_table(90, 150, '444'):
                c = BA.plane_cases(plane_view(pay, entry), depth, 2, r)
                pairs |= set(zip(c['rx'].reshape(-1).tolist(), c['ry'].reshape(-1).tolist()))
                ns |= set(c['n'].reshape(-1).tolist())
                changed, total = changed + int(c['changed'].sum()), total + c['changed'].size
        top = (2 * r + 1) ** 2
        print(depth, r, len(pairs), len(ns), changed / total)
        assert pairs == {(a, b) for a in range(r + 1) for b in range(r + 1)}
        assert 1 in ns and max(ns) > top // 2 and len(ns) >= min(top, 200) // 2 and 0.02 < changed / total < 0.95     # at equal depths only the texture cells change, one kind in eight
    # an input of one kind has one n a pair
    c = BA.plane_cases(np.full((90, 150), 50 << (depth - 8), np.uint16), depth, 2, 16)
    assert not c['changed'].any()


@pytest.mark.parametrize('h,w,layout,d', [(64, 96, '420', 8), (48, 80, '420', 8), (48, 80, '422', 10), (96, 160, '420', 10), (48, 80, '444', 8),
                                          (48, 80, 'mono', 8)])
def test_the_gpu_tests_clip_moves_and_is_filtered(h, w, layout, d):
    data, pays = banded_clip(6, h, w, layout, d, seed=3)
    assert len(pays) == 6 and pays[0].size == y4m.payload_size(h, w, layout) and data.count(b'FRAME\n') == 6
    out = BA.deband_stream_np(pays, h, w, d, layout)
    changed = np.mean([(o != p).mean() for o, p in zip(out, pays)])
    moved = np.mean([(x != y).mean() for x, y in zip(pays, pays[1:])])
    print(changed, moved)
    assert changed > 0.02 and moved > 0.1
    if d == 8:                                                            # promoted to 10 bits the bands themselves go
        up = [p.astype(np.uint16) << 2 for p in pays]
        assert np.mean([(o != p).mean() for o, p in zip(BA.deband_stream_np(up, h, w, 10, layout), up)]) > 2 * changed
