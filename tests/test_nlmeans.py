"""The spatial denoiser in front of the network (``--nlmeans``) on the CPU: the rule of ``demfi_amd.nlmeans`` against a scalar reading in
plain Python loops and exact fractions, its weight table by hand, what follows from the rule, the noise figure, the accumulator bounds by
brute force, the kernel's quotient against the floor, the switch, ``EdgeSpec.nlmeans``, the place of the stage in the ingest and the scratch
buffer it shares, and the generators of the GPU tests' inputs (tests/test_gpu_nlmeans.py) with the proof that they reach every case of the
rule."""
import math
import types
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import deblock as DB
from demfi_amd import nlmeans as NL
from demfi_amd import pipeline as P
from demfi_amd import video
from demfi_amd import y4m
from demfi_amd.y4m_edge import Ingest


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def by_hand(plane, depth, S, Pr, R):
    """The rule read sample by sample: plain loops, ``math.exp`` and exact fractions."""
    rows, cols = len(plane), len(plane[0])
    s = depth - 8
    b = min(s, 4)
    h2 = (2 * Pr + 1) ** 2 * 4 ** b * S * S
    g = 0
    while (1023 << g) < math.log(512) * h2:
        g += 1

    def u(x, y):
        return int(plane[min(max(y, 0), rows - 1)][min(max(x, 0), cols - 1)])
    out = [[0] * cols for _ in range(rows)]
    for y in range(rows):
        for x in range(cols):
            wv, W = 0, 0
            for j in range(-R, R + 1):
                for i in range(-R, R + 1):
                    if not (0 <= x + i < cols and 0 <= y + j < rows):
                        continue
                    D = sum(min(abs(u(x + a, y + e) - u(x + i + a, y + j + e)) >> (s - b), 4095) ** 2
                            for a in range(-Pr, Pr + 1) for e in range(-Pr, Pr + 1))
                    w = int(math.floor(256 * math.exp(-(min(D >> g, 1023) << g) / h2) + 0.5))
                    W += w
                    wv += w * u(x + i, y + j)
            out[y][x] = math.floor(Fraction(wv, W) + Fraction(1, 2))       # the weighted mean to nearest, ties up
    return np.array(out)


@pytest.mark.parametrize('depth,S,Pr,R,shape', [(8, 3, 2, 5, (9, 11)), (8, 16, 1, 1, (12, 14)), (10, 3, 1, 3, (12, 14)), (10, 8, 3, 2, (7, 8)),
                                               (16, 3, 2, 2, (8, 9)), (16, 16, 3, 7, (5, 6)), (8, 1, 1, 7, (6, 9)), (12, 5, 2, 3, (6, 7)),
                                               (14, 2, 1, 2, (8, 8)), (8, 3, 2, 5, (1, 1)), (10, 16, 3, 7, (1, 5)), (16, 4, 2, 3, (2, 2)),
                                               (8, 6, 3, 1, (5, 1))])
def test_the_rule_against_a_scalar_reading(depth, S, Pr, R, shape):
    g = np.random.RandomState(depth + 31 * S + R)
    peak = (1 << depth) - 1
    base = g.randint(0, peak + 1)
    noise = g.randint(-2 * S << (depth - 8), (2 * S << (depth - 8)) + 1, shape)
    plane = np.clip(base + noise, 0, peak)
    if shape[0] > 4:
        plane[:2] = g.randint(0, peak + 1, (2, shape[1]))                 # rows that have nothing in common with the rest
    plane = plane.astype(np.uint8 if depth == 8 else np.uint16)
    got = NL.nlmeans_plane_np(plane, depth, S, Pr, R)
    assert got.dtype == plane.dtype and np.array_equal(got, by_hand(plane, depth, S, Pr, R))
    if plane.size > 20:
        assert not np.array_equal(got, plane)


def test_the_table_by_hand_and_every_legal_table():
    t, g = NL.weight_table(8, 3, 2)
    assert g == 1 and t[:4].tolist() == [256, 254, 251, 249] and t[1023] == 0 and t.dtype == np.uint16 and t.shape == (1024,)
    assert NL.K == 1024 and NL.DEFAULTS == (3, 2, 5)
    for depth in y4m.DEPTHS:
        for S in range(1, NL.MAX_S + 1):
            for Pr in range(NL.MIN_P, NL.MAX_P + 1):
                t, g = NL.weight_table(depth, S, Pr)
                h2 = (2 * Pr + 1) ** 2 * 4 ** min(depth - 8, 4) * S * S
                assert 0 <= g <= 31 and (1023 << g) >= math.log(512) * h2 and (g == 0 or (1023 << (g - 1)) < math.log(512) * h2)   # minimal
                assert t[0] == 256 and t[1023] == 0 and not (np.diff(t.astype(np.int64)) > 0).any()
                assert NL.check_table(t, g)[1] == g
    with pytest.raises(ValueError):
        NL.weight_table(8, 0, 2)
    with pytest.raises(ValueError):
        NL.weight_table(9, 3, 2)
    for bad in (np.zeros(1024), np.full(1023, 256), np.r_[256, 257, np.zeros(1022)], np.r_[256, 0, 1, np.zeros(1021)]):
        with pytest.raises(ValueError):
            NL.check_table(bad, 0)


# ---- what follows from the rule ----------------------------------------------------------------------------------------------------------
def test_bounds_constant_planes_and_the_identity():
    g = np.random.RandomState(1)
    for depth, S, Pr, R in ((8, 3, 2, 5), (10, 16, 3, 7), (16, 8, 1, 3)):
        peak = (1 << depth) - 1
        plane = g.randint(0, peak + 1, (20, 26)).astype(np.uint8 if depth == 8 else np.uint16)
        plane[5:15, 5:20] = np.clip(peak // 2 + g.randint(-S << (depth - 8), (S << (depth - 8)) + 1, (10, 15)), 0, peak)
        out = NL.nlmeans_plane_np(plane, depth, S, Pr, R).astype(np.int64)
        pad = np.pad(plane.astype(np.int64), R, mode='edge')
        win = np.lib.stride_tricks.sliding_window_view(pad, (2 * R + 1, 2 * R + 1))
        assert (out >= win.min((2, 3))).all() and (out <= win.max((2, 3))).all() and out.max() <= peak      # a legal sample stays legal
        for level in (0, 1, peak // 3, peak):                             # a constant plane stays constant
            flat = np.full((9, 13), level, plane.dtype)
            assert np.array_equal(NL.nlmeans_plane_np(flat, depth, S, Pr, R), flat)
        same = NL.nlmeans_plane_np(plane, depth, 0, Pr, R)                 # S = 0 is the identity, out of place
        assert np.array_equal(same, plane) and same is not plane
        c = NL.plane_cases(plane, depth, S, Pr, R)
        assert (c['W'] >= 256).all() and (c['live'] >= 1).all()
    with pytest.raises(ValueError):
        NL.plane_cases(np.zeros((4, 4), np.uint8), 8, 0)
    with pytest.raises(ValueError):
        NL.nlmeans_plane_np(np.zeros(4, np.uint8), 8)


def test_an_output_depends_on_its_window_and_on_nothing_else():
    g = np.random.RandomState(2)
    for depth, S, Pr, R in ((8, 6, 2, 3), (10, 16, 3, 2), (8, 16, 1, 5)):
        H = R + Pr
        plane = np.clip((128 << (depth - 8)) + g.randint(-4 << (depth - 8), (4 << (depth - 8)) + 1, (31, 33)), 0, None).astype(np.uint16)
        ref = NL.nlmeans_plane_np(plane, depth, S, Pr, R)
        other = plane.copy()
        other[15, 16] ^= 3 << (depth - 8)
        out = NL.nlmeans_plane_np(other, depth, S, Pr, R)
        yy, xx = np.nonzero(out != ref)
        assert yy.size and np.abs(yy - 15).max() <= H and np.abs(xx - 16).max() <= H                  # nothing outside the reach changes
        far = np.ones(plane.shape, bool)
        far[15 - H:15 + H + 1, 16 - H:16 + H + 1] = False
        assert np.array_equal(out[far], ref[far])


def reach_plane(depth, seed=None):
    """48 x 64: a ramp of 2 codes a column plus a step of 80 codes between rows 24 and 25 (8-bit codes, scaled to ``depth``); ``seed``:
    with Gaussian noise of 3 codes of 8 bits.  Returns (the clean plane as floats, the plane)."""
    yy, xx = np.mgrid[0:48, 0:64]
    clean = (40 + 2 * xx + np.where(yy >= 25, 80, 0)).astype(np.float64) * (1 << (depth - 8))
    noise = np.random.RandomState(seed).normal(0, 3 * (1 << (depth - 8)), clean.shape) if seed is not None else 0
    return clean, np.clip(np.round(clean + noise), 0, (1 << depth) - 1).astype(np.uint8 if depth == 8 else np.uint16)


def test_a_step_of_80_codes_is_not_seen_across():
    """At 3:2:5 the table's reach is D < 2046 * 4^b; a candidate whose patch holds a sample of the other side where the sample's own patch
    has one of its own side differs there by 80 codes less the noise, above 60^2 * 4^b, and weighs nothing.  So whatever lies below the step
    (other noise, a step of 120) the rows whose own patches stay above it come back the same, and the other way round."""
    for depth in (8, 10):
        _, plane = reach_plane(depth, 5)
        _, other = reach_plane(depth, 6)
        out = NL.nlmeans_plane_np(plane, depth, 3, 2, 5)
        below = plane.copy()
        below[25:] = other[25:] + (40 << (depth - 8))
        assert np.array_equal(NL.nlmeans_plane_np(below, depth, 3, 2, 5)[:23], out[:23]) and not np.array_equal(below[25:], plane[25:])
        above = plane.copy()
        above[:25] = other[:25]
        assert np.array_equal(NL.nlmeans_plane_np(above, depth, 3, 2, 5)[27:], out[27:])
        c = NL.plane_cases(plane, depth, 3, 2, 5)
        assert c['live'][22].max() <= 11 * 8 and c['live'][20:23, 20:40].min() > 11     # rows 17 .. 24 at most; more than the row alone


def test_the_noise_figure_and_the_reach_on_the_clean_plane():
    """Measured with the module, six seeds, 3:2:5: rms error out / in 0.433 .. 0.467 at 8 bits and 0.422 .. 0.456 at 10 bits (asserted
    below 0.6: a margin, so that the seed is no condition).  The clean plane: exact more than 10 from a border and off rows 24 / 25, at
    most 1 code (8 bits) and 6 codes (10 bits) elsewhere; at 16:3:7 the clean 10-bit plane deviates by up to 31 codes."""
    for depth, lo, hi, worst in ((8, 0.43, 0.47, 1), (10, 0.42, 0.46, 6)):
        ratios = []
        for seed in range(6):
            clean, plane = reach_plane(depth, seed)
            out = NL.nlmeans_plane_np(plane, depth, *NL.DEFAULTS)
            ratios.append(float(np.sqrt(((out - clean) ** 2).mean()) / np.sqrt(((plane - clean) ** 2).mean())))
        print('nlmeans 3:2:5 at %d bits: rms out / in %s' % (depth, ' '.join('%.3f' % r for r in ratios)))
        assert max(ratios) < 0.6
        assert lo <= min(ratios) and max(ratios) <= hi                    # the recorded figures
        clean, plane = reach_plane(depth)
        dev = np.abs(NL.nlmeans_plane_np(plane, depth, *NL.DEFAULTS).astype(np.int64) - plane)
        inner = np.zeros(dev.shape, bool)
        inner[11:-11, 11:-11] = True
        inner[24:26] = False
        assert dev[inner].max() == 0 and dev.max() == worst
    clean, plane = reach_plane(10)
    assert np.abs(NL.nlmeans_plane_np(plane, 10, 16, 3, 7).astype(np.int64) - plane).max() == 31


def test_fields_are_planes_of_their_own():
    h, w = 24, 32
    pay = noisy_payload(h, w, '420', 10, 3)
    out = NL.nlmeans_payload_np(pay, h, w, 10, '420', 6, 1, 2, fields='t')
    table = DB.plane_table(h, w, '420', 't')
    assert len(table) == 6
    for entry in table:
        assert np.array_equal(plane_view(out, entry), NL.nlmeans_plane_np(plane_view(pay, entry), 10, 6, 1, 2))
    assert not np.array_equal(out, NL.nlmeans_payload_np(pay, h, w, 10, '420', 6, 1, 2)) and not np.array_equal(out, pay)
    assert np.array_equal(NL.nlmeans_payload_np(pay, h, w, 10, '420', 6, 1, 2, 't', (4, 28, 6, 38)), out)       # the phases are ignored
    assert all(np.array_equal(a, b) for a, b in zip(NL.nlmeans_stream_np([pay, pay[::-1].copy()], h, w, 10, '420', 6, 1, 2, 't'),
                                                    [out, NL.nlmeans_payload_np(pay[::-1].copy(), h, w, 10, '420', 6, 1, 2, 't')]))
    assert np.array_equal(NL.nlmeans_payload_np(pay, h, w, 10, '420', 0), pay)
    with pytest.raises(ValueError):
        NL.nlmeans_payload_np(pay[:-1], h, w, 10, '420')


# ---- accumulators and the quotient -------------------------------------------------------------------------------------------------------
BOX = (np.full(NL.K, 256, np.uint16), 0)                                  # a table the entry point takes: every candidate weighs 256


def test_the_accumulator_bounds_by_brute_force():
    """Adversarial planes at the widest window.  Under ANY legal table (the box reaches it): a centre of 0 among samples at the peak
    gives exactly the bound on the numerator, which fits int32 up to 14 bits and not at 16; sum(w v) reaches its bound on a plane at the
    peak and fits uint32 at every depth.  Under the rule's own tables a candidate's difference is part of its distance: a lone sample t
    below a flat plane, t swept about sqrt(h2 / 2), comes within a fifth of ``numerator_rule`` and never above it, and that bound fits
    int32 even at 16 bits."""
    for depth in y4m.DEPTHS:
        peak = (1 << depth) - 1
        b = NL.accumulator_bounds(depth)
        assert b['D_fits_int32'] and b['D'] < 2 ** 30 and b['W'] == 57600 and b['wv_fits_uint32']
        assert b['numerator_fits_int32'] == (depth <= 14) and b['numerator_rule_fits_int32'] and b['numerator_rule'] < b['numerator']
        plane = np.full((15, 15), peak, np.uint16)
        assert int(NL.plane_cases(plane, depth, 1, 3, 7, table=BOX)['wv'][7, 7]) == b['wv'] == 225 * 256 * peak
        plane[7, 7] = 0
        c = NL.plane_cases(plane, depth, 1, 3, 7, table=BOX)
        assert int(c['numerator'][7, 7]) == b['numerator'] == 2 * 224 * 256 * peak + 57600 and int(c['W'][7, 7]) == b['W']
        up = np.zeros((15, 15), np.uint16)
        up[7, 7] = peak
        assert int(NL.plane_cases(up, depth, 1, 3, 7, table=BOX)['numerator'][7, 7]) == 57600 - 2 * 224 * 256 * peak
        # the patch distance at its greatest: a checkerboard of 0 and the peak against itself displaced by one
        board = [[peak if (y + x) & 1 else 0 for x in range(9)] for y in range(9)]
        assert sum(min(abs(board[4 + e][4 + a] - board[4 + e][5 + a]) >> NL._scale(depth)[0], 4095) ** 2
                   for a in range(-3, 4) for e in range(-3, 4)) == b['D']
    assert 2 * 225 * 256 * 16383 + 57600 < 2 ** 31 < 2 * 224 * 256 * 65535
    for depth, S, Pr in ((16, 16, 3), (16, 3, 2), (10, 16, 3), (8, 16, 1)):
        b = NL.accumulator_bounds(depth, S, Pr, 7)
        h2 = (2 * Pr + 1) ** 2 * 4 ** min(depth - 8, 4) * S * S
        top, sh = 0, NL._scale(depth)[0]
        for t in sorted({min(int(f * math.sqrt(h2 / 2)) << sh, (1 << depth) - 1) for f in (0.5, 0.8, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0)}):
            plane = np.full((21, 21), (1 << depth) - 1, np.uint16)
            plane[10, 10] -= t
            top = max(top, int(NL.plane_cases(plane, depth, S, Pr, 7)['numerator'][10, 10]))
        assert 0.8 * b['numerator_rule'] <= top <= b['numerator_rule'] < 2 ** 31, (depth, S, Pr, top, b['numerator_rule'])


def test_the_kernels_quotient_against_the_floor():
    """Every W in 256 .. 57600; sum(w v) on both sides of the quotient boundaries at outputs 0, 1, 2, peak - 1 and peak of 16 bits and of
    8 bits, as far as the sums can reach them (wv <= 255 W: every weight 256 or less); the definition's form c + (2 sum(w (v - c)) + W)
    // (2 W) is taken with c below and above the mean, so its numerator has both signs."""
    W = np.arange(256, NL.MAX_W + 1, dtype=np.int64)
    n = 0
    for peak in (255, 65535):
        for m in (0, 1, 2, 3, peak // 2, peak - 1, peak):
            edge = (W * (2 * m - 1) + 1) // 2                             # the least wv with out >= m
            for d in (-2, -1, 0, 1, 2):
                wv = edge + d
                ok = (wv >= 0) & (wv <= W * peak)
                got = NL.kernel_quotient(wv[ok], W[ok])
                for c in (0, m, peak):                                    # sum(w (v - c)) = wv - W c
                    num = wv[ok] - W[ok] * c
                    assert np.array_equal(got, c + (2 * num + W[ok]) // (2 * W[ok]))
                    n += int((num < 0).any()) + 2 * int((num > 0).any())
                if d == 0:
                    assert (got[wv[ok] > 0] == m).all() if m else True
                if d == -1 and m:
                    assert (got == m - 1).all()
    assert n > 100
    g = np.random.RandomState(3)
    Wr = g.randint(256, NL.MAX_W + 1, 200000).astype(np.int64)
    wv = (g.randint(0, 65536, Wr.size).astype(np.int64) * Wr + g.randint(0, 256, Wr.size)).clip(0, Wr * 65535)
    assert np.array_equal(NL.kernel_quotient(wv, Wr), (2 * wv + Wr) // (2 * Wr))
    assert int(NL.kernel_quotient(225 * 256 * 65535, NL.MAX_W)) == 65535 and int(NL.kernel_quotient(0, 256)) == 0
    with pytest.raises(ValueError):
        NL.kernel_quotient(2 ** 32, 256)


# ---- the switch and the spec -------------------------------------------------------------------------------------------------------------
def test_parse_nlmeans_and_check_params():
    assert NL.parse_nlmeans('3') == (3, 2, 5) and NL.parse_nlmeans('4:1') == (4, 1, 5) and NL.parse_nlmeans(' 16:3:7 ') == (16, 3, 7)
    assert NL.parse_nlmeans('0') == (0, 2, 5) and NL.check_params() == (3, 2, 5) and NL.check_params(np.int64(5), 1, 1) == (5, 1, 1)
    for bad in ('', 'x', '3:', '3:2:5:1', '-1', '17', '3:0', '3:4', '3:2:0', '3:2:8', '3.5', '3:2.5'):
        with pytest.raises(ValueError):
            NL.parse_nlmeans(bad)
    for bad in ((-1,), (17,), (3, 0), (3, 4), (3, 2, 0), (3, 2, 8), (True,), (3.0,), (3, 2.0)):
        with pytest.raises(ValueError):
            NL.check_params(*bad)


def test_edge_spec_with_nlmeans_deblock_dering_and_deband():
    args = (True, True, False, 10, '422', None, 't', 'adaptive')
    plain = P.EdgeSpec(*args)
    nl = P.EdgeSpec(*args, nlmeans=(3, 2, 5))
    assert nl.nlmeans == (3, 2, 5) and plain.nlmeans is None and tuple(nl) == tuple(plain) and len(plain) == 8
    assert nl != plain and plain != nl and nl != tuple(nl) and plain == tuple(plain)
    assert hash(plain) == hash((tuple(plain), None))                      # as before there was the field
    assert nl == P.EdgeSpec(*args, nlmeans=[3, 2, 5]) and hash(nl) == hash(nl._replace())
    assert nl != nl._replace(nlmeans=(3, 2, 4)) and nl._replace(nlmeans=None) == plain and plain._replace(nlmeans=(3, 2, 5)) == nl
    assert 'nlmeans=(3, 2, 5)' in repr(nl) and 'nlmeans' not in repr(plain) and repr(plain) == repr(nl._replace(nlmeans=None))
    for none in ((0, 2, 5), (0, 1, 1), None):                             # S = 0: no stage
        assert P.EdgeSpec(True, nlmeans=none) == P.EdgeSpec(True) and P.EdgeSpec(True, nlmeans=none).nlmeans is None
        assert hash(P.EdgeSpec(True, nlmeans=none)) == hash(P.EdgeSpec(True)) and repr(P.EdgeSpec(True, nlmeans=none)) == repr(P.EdgeSpec(True))
    seen = set()
    for db in (None, (16, 4)):
        for dr in (None, (4, 2, 5)):
            for bd in (None, (2, 16)):
                for n in (None, (3, 2, 5)):
                    spec = P.EdgeSpec(*args, deblock=db, dering=dr, deband=bd, nlmeans=n)
                    assert (spec.deblock, spec.dering, spec.deband, spec.nlmeans) == (db, dr, bd, n)
                    assert spec == plain._replace(nlmeans=n)._replace(deband=bd)._replace(dering=dr)._replace(deblock=db)
                    assert spec._replace(depth=8).nlmeans == n and spec._replace(nlmeans=None) == P.EdgeSpec(*args, deblock=db, dering=dr, deband=bd)
                    assert ('nlmeans' in repr(spec)) == (n is not None) and ('deband' in repr(spec)) == (bd is not None)
                    if n is None:
                        same = P.EdgeSpec(*args, deblock=db, dering=dr, deband=bd)
                        assert repr(spec) == repr(same) and hash(spec) == hash(same)
                    seen.add(spec)
    assert len(seen) == 16
    assert nl.reach == plain.reach == 2 and P.EdgeSpec(True, nlmeans=(3, 2, 5)).reach == 0           # no look-ahead of its own
    edge = video.YuvEdge('bt601', False, '420jpeg', None, nlmeans=(4, 1, 3))
    assert edge.nlmeans == (4, 1, 3) and edge.deband is None and P.EdgeSpec.of(edge).nlmeans == (4, 1, 3)
    plain_edge = video.YuvEdge('bt601', False, '420jpeg', None)
    assert plain_edge.nlmeans is None and P.EdgeSpec.of(plain_edge) == P.EdgeSpec(True)
    assert video.YuvEdge('bt601', False, '420jpeg', None, nlmeans=(0, 1, 1)).nlmeans is None
    with pytest.raises(ValueError):
        video.YuvEdge('bt601', False, '420jpeg', None, nlmeans=(3, 2, 8))
    nl.check(True, True, True)                                            # nothing is refused
    P.EdgeSpec(True, True, True, 16, '444', (7, 5, 0, 4), 't', 'bob', dering=(4, 2, 5), deblock=(16, 4), deband=(8, 1),
               nlmeans=(16, 3, 7)).check(True, True, True)
    P.EdgeSpec(True, denoise=(5, 10, 2), nlmeans=(3, 2, 5), shutter=(2, 4), grain=(16, 1, 8, 'film', 0)).check(True, False, True)
    for spec, a, msg in ((P.EdgeSpec(True, nlmeans=(17, 2, 5)), (True, False, True), 'nlmeans must be'),
                         (P.EdgeSpec(True, nlmeans=(3, 4, 5)), (True, False, True), 'nlmeans must be'),
                         (P.EdgeSpec(True, nlmeans=(3, 2, 0)), (True, False, True), 'nlmeans must be'),
                         (P.EdgeSpec(True, nlmeans=(3, 2)), (True, False, True), 'nlmeans must be'),
                         (P.EdgeSpec(False, nlmeans=(3, 2, 5)), (False, False, True), 'Y4M edge')):
        with pytest.raises(ValueError, match=msg):
            spec.check(*a)


def test_runner_arguments_and_counter():
    vr = video.VideoRunner(None)
    assert vr.nlmeans is None and vr.last_nlm_filtered == 0
    assert video.VideoRunner(None, nlmeans=True).nlmeans == (3, 2, 5) and video.VideoRunner(None, nlmeans=False).nlmeans is None
    assert video.VideoRunner(None, nlmeans=4).nlmeans == (4, 2, 5) and video.VideoRunner(None, nlmeans='4:1').nlmeans == (4, 1, 5)
    assert video.VideoRunner(None, nlmeans=(1, 3, 7)).nlmeans == (1, 3, 7) and video.VideoRunner(None, nlmeans=(0, 1, 1)).nlmeans is None
    assert video.VideoRunner(None, nlmeans=0).nlmeans is None and video.VideoRunner(None, nlmeans='0').nlmeans is None
    assert video.check_nlmeans(None) is None and video.check_nlmeans((8, None, 3)) == (8, 2, 3) and video.check_nlmeans('1:1:1') == (1, 1, 1)
    assert video.check_nlmeans([2, 3]) == (2, 3, 5)
    vr = video.VideoRunner(None, nlmeans=True, dedup=True, deinterlace=True)
    assert vr.nlmeans == (3, 2, 5) and vr._behind('t') == 0               # no look-ahead
    vr = video.VideoRunner(None, nlmeans=True, deband=True, dering=True, deblock=True, deinterlace=True, deinterlace_mode='adaptive', tile='auto',
                           high_depth=True, tile_high_depth=True, layouts=True, work_depth=12)
    assert vr._behind('t') == 2 and (vr.deblock, vr.dering, vr.nlmeans, vr.deband) == ((16, 4), (4, 2, 5), (3, 2, 5), (2, 16))
    video.check_one_rank(4, nlmeans=(3, 2, 5))                            # any number of ranks
    assert 'nlmeans' not in video.ONE_RANK and 'nlmeans' not in video.ONE_RANK_EGRESS
    for kw, msg in ((dict(nlmeans=17), '0 .. 16'), (dict(nlmeans=(3, 4)), 'patch'), (dict(nlmeans=(3, 2, 8)), 'search'),
                    (dict(nlmeans=(1, 2, 3, 4)), 'nlmeans must be'), (dict(nlmeans=2.5), 'nlmeans must be'), (dict(nlmeans='x'), 'expected S')):
        with pytest.raises(ValueError, match=msg):
            video.VideoRunner(None, **kw)
    assert video.INGEST_COUNTERS['nlm_filtered'] == 'last_nlm_filtered' and video.INGEST_COUNTERS['debanded'] == 'last_debanded'
    vr = video.VideoRunner(None, mfi=2, nlmeans=True)
    vr._counted(types.SimpleNamespace(w=96, h=64, layout='420'), dict({name: 0 for name in video.COUNTERS}, nlm_filtered=9), [], 0)
    assert vr.last_nlm_filtered == 9 and vr.last_debanded == 0
    import inspect
    from demfi_amd.runner import WindowRunner
    assert 'self.nlm_filtered = 0' in inspect.getsource(WindowRunner.__init__)
    hdr = y4m.Header(96, 64, 25, 'p', None, '420jpeg', None, (), '420jpeg', 8, '420')
    edge = video.VideoRunner(None, mfi=2, nlmeans='4:1:3')._edge(hdr, None)
    assert edge.nlmeans == (4, 1, 3) and edge.deband is None and edge.crop_rect is None


def test_command_line(capsys):
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).nlmeans is None and p.parse_args(['-', '-', '--nlmeans']).nlmeans == (3, 2, 5)
    assert p.parse_args(['a', 'b', '--nlmeans', '4']).nlmeans == (4, 2, 5) and p.parse_args(['a', 'b', '--nlmeans', '4:1:3', '--dedup']).nlmeans == (4, 1, 3)
    assert p.parse_args(['a', 'b', '--nlmeans', '0']).nlmeans == (0, 2, 5)
    a = p.parse_args(['a', 'b', '--deblock', '--dering', '--nlmeans', '--deband'])
    assert (a.deblock, a.dering, a.nlmeans, a.deband) == ((16, 4), (4, 2, 5), (3, 2, 5), (2, 16))
    text = ' '.join(p.format_help().split())
    assert '--nlmeans' in text and 'S[:P[:R]]' in text and 'default 3:2:5 (not tuned against this network)' in text
    for argv, msg in ((['a.y4m', 'b.y4m', '--nlmeans', '17'], '0 .. 16'), (['a.y4m', 'b.y4m', '--nlmeans', '3:2:8'], 'search'),
                      (['a.y4m', 'b.y4m', '--nlmeans', 'x'], 'expected S')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
    from demfi_amd import clip
    with pytest.raises(SystemExit) as ex:                                 # the folder path has no such switch
        clip.parser().parse_args(['frames', '--nlmeans'])
    assert ex.value.code == 2
    for doc in (video.__doc__, video.VideoRunner.__doc__, NL.__doc__):
        assert 'nlmeans' in doc and 'tuned' in doc and '3:2:5' in doc


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
                               debanded=0, nlm_filtered=0)
    return Ingest(rn, P.FrameSlots(nslot, 2, 2, 'cpu'), spec, h, w), rn


STAGES = ('demfi_payload_dering', 'demfi_payload_nlmeans', 'demfi_payload_deband')


def test_the_ingest_order_the_scratch_copy_and_the_one_scratch(monkeypatch):
    import torch
    spec = P.EdgeSpec(True, depth=10, fields='t', denoise=(5, 10, 1), deblock=(16, 4), dering=(6, 3, 4), deband=(3, 5), nlmeans=(4, 1, 3),
                      depths=(8, 10, 10, None))
    seen = {}

    def on_call(name, args):                                              # at each launch the scratch already holds what the stage reads
        if name in STAGES:
            seen[name] = ing.nl_scratch[:6].clone()
            ing.yuv_in[:6] += 1                                           # "the stage": the next copy must pick this up
    ing, rn = _ingest(spec, monkeypatch, on_call=on_call)
    assert ing.nl_scratch is ing.dr_scratch and ing.bd_scratch is ing.dr_scratch          # one buffer serves all three
    ing.attach(types.SimpleNamespace(full_range=False, crop_rect=(4, 16, 6, 26)))
    ing.yuv_in.copy_(torch.arange(ing.yuv_in.numel(), dtype=torch.int64).reshape(ing.yuv_in.shape) % 199)
    start = ing.yuv_in[:6].clone()
    ing.nl_scratch.zero_()
    stream = types.SimpleNamespace(cuda_stream=0)
    near = ing.around({2, 3}, lambda g: g < 6)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2, 3})]
    assert [sl for _, sl in new] == list(range(6))
    done = ing.rebuilt(new, stream)
    names = [name for name, _ in rn.lib.calls]
    assert names == ['demfi_payload_promote', 'demfi_payload_deblock', 'demfi_payload_dering', 'demfi_payload_nlmeans', 'demfi_payload_deband',
                     'demfi_yuv_bob', 'demfi_payload_denoise']
    assert [f for f, _ in done] == [2, 3]
    assert (rn.depth_promoted, rn.deblocked, rn.deringed, rn.nlm_filtered, rn.debanded, rn.denoised) == (6, 6, 6, 6, 6, 2)
    for k, name in enumerate(STAGES):                                     # in order: each reads what the one before wrote
        assert bool((seen[name] == start + k).all())
    args = dict(rn.lib.calls)['demfi_payload_nlmeans']
    assert args[0] == ing.nl_scratch[0].data_ptr() and args[2] == ing.yuv_in[0].data_ptr() and args[1] == args[3] == ing.Pb == 2 * y4m.payload_size(12, 20)
    assert args[4] == 6 and ing.nl_scratch.shape == ing.yuv_in.shape and ing.nl_scratch.dtype == ing.yuv_in.dtype
    assert not bool((ing.nl_scratch[6:] != 0).any())
    tab = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int64 * (6 * args[6])).from_address(args[5])).reshape(-1, 6)
    assert tab.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))] and args[6] == 6
    assert args[7:11] == (2, 10, 1, 3) and len(args) == 14                # sample size, working depth, P, R; then the table, its shift, the stream
    t, g = NL.weight_table(10, 4, 1)
    weights = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint16 * NL.K).from_address(args[11]))
    assert np.array_equal(weights, t) and args[12] == g and ing.nl_table.dtype == np.uint16 and ing.nl_table.flags['C_CONTIGUOUS']
    # two runs of slots: two copies and two launches; nothing new: none
    rn.lib.calls.clear()
    ing.nlm_filtered([(8, 1), (9, 2), (11, 5)], stream)
    assert [(name, a[0] - ing.nl_scratch.data_ptr(), a[2] - ing.yuv_in.data_ptr(), a[4]) for name, a in rn.lib.calls] == [
        ('demfi_payload_nlmeans', ing.Pb, ing.Pb, 2), ('demfi_payload_nlmeans', 5 * ing.Pb, 5 * ing.Pb, 1)]
    rn.lib.calls.clear()
    ing.nlm_filtered([], stream)
    assert not rn.lib.calls and rn.nlm_filtered == 9


def test_alone_and_in_every_combination_the_scratch_is_one(monkeypatch):
    stream = types.SimpleNamespace(cuda_stream=0)
    for db in (None, (16, 4)):
        for dr in (None, (4, 2, 5)):
            for bd in (None, (2, 16)):
                for nl in (None, (3, 2, 5)):
                    ing, rn = _ingest(P.EdgeSpec(True, fields='b', deint_mode='adaptive', deblock=db, dering=dr, deband=bd, nlmeans=nl), monkeypatch)
                    near = ing.around({2}, lambda g: g < 8)
                    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2})]
                    ing.rebuilt(new, stream)
                    want = [n for n, on in (('demfi_payload_deblock', db), ('demfi_payload_dering', dr), ('demfi_payload_nlmeans', nl),
                                            ('demfi_payload_deband', bd)) if on is not None]
                    assert [name for name, _ in rn.lib.calls] == want + ['demfi_yuv_deint_adaptive']
                    assert (rn.deblocked, rn.deringed, rn.nlm_filtered, rn.debanded) == tuple(len(new) if on is not None else 0 for on in (db, dr, nl, bd))
                    # the names and the sharing the existing tests read stay: dr_scratch only with dering, bd_scratch only with deband
                    assert hasattr(ing, 'dr_scratch') == (dr is not None) and hasattr(ing, 'bd_scratch') == (bd is not None)
                    assert hasattr(ing, 'nl_scratch') == hasattr(ing, 'nl_planes') == hasattr(ing, 'nl_table') == (nl is not None)
                    if bd is not None and dr is not None:
                        assert ing.bd_scratch is ing.dr_scratch
                    if nl is not None:
                        assert ing.nl_scratch.shape == ing.yuv_in.shape and ing.nlmeans == (8, 2, 5) and ing.nl_shift == 1
                        assert (ing.nl_scratch is getattr(ing, 'dr_scratch', None)) == (dr is not None)
                        assert bd is None or ing.bd_scratch is ing.nl_scratch
                        assert ing.nl_planes.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 'b')]
                    else:
                        assert ing.nlmeans is None
                    bufs = {id(getattr(ing, n)) for n in ('dr_scratch', 'nl_scratch', 'bd_scratch') if hasattr(ing, n)}
                    assert len(bufs) == (1 if (dr or nl or bd) else 0)    # one scratch buffer serves every stage that needs one


def test_without_the_switch_the_ingest_is_what_it_was(monkeypatch):
    assert object.__new__(Ingest).nlmeans is None
    for spec in (P.EdgeSpec(True, fields='t'), P.EdgeSpec(True, nlmeans=(0, 2, 5), fields='t'), P.EdgeSpec(True, deband=(2, 16), fields='t')):
        ing, rn = _ingest(spec, monkeypatch)
        assert ing.nlmeans is None and not any(hasattr(ing, n) for n in ('nl_planes', 'nl_scratch', 'nl_table', 'nl_shift'))
        ing.attach(types.SimpleNamespace(full_range=True, crop_rect=(4, 16, 6, 26)))
        assert ing.full_range is True and not hasattr(ing, 'nl_planes')
        ing.rebuilt([(0, 0), (1, 1)], types.SimpleNamespace(cuda_stream=0))
        assert 'demfi_payload_nlmeans' not in [name for name, _ in rn.lib.calls] and rn.nlm_filtered == 0


# ---- the inputs of the GPU tests, and the proof that they cover the rule -----------------------------------------------------------------
CELL = 32


def noisy_plane(rows, cols, depth, seed, noise, shift=0, dtype=None):
    """Cells of 32 x 32 samples of eight kinds (8-bit codes, scaled to ``depth``): a ramp of 2 codes a column under noise of +-3; a flat
    cell; hard edges (bars of 40 and 200 every 5 samples) under noise of +-1; texture over the whole range; noise about a level whose
    amplitude grows across the cell from 0 to 12; a slow diagonal ramp without noise; noise of +-3 about a level; noise at the bottom and at
    the top of the range.  ``shift`` moves the pattern to the left; ``noise``: the generator of everything random, which does not move."""
    sh = depth - 8
    peak = (1 << depth) - 1
    kind = np.random.RandomState(seed).randint(0, 8, (64, 64))
    yy, xx = np.mgrid[0:rows, 0:cols]
    xx = xx + shift
    k = kind[(yy // CELL) % 64, (xx // CELL) % 64]
    n3 = noise.randint(-3 << sh, (3 << sh) + 1, (rows, cols))
    grow = (noise.uniform(-1, 1, (rows, cols)) * ((xx % CELL) * 12 // CELL << sh)).astype(np.int64)
    v = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6],
                  [((60 + 2 * (xx % CELL)) << sh) + n3, np.full((rows, cols), 180 << sh), (np.where((xx + yy // 2) % 10 < 5, 40, 200) << sh) + n3 // 3,
                   noise.randint(0, peak + 1, (rows, cols)), (128 << sh) + grow, ((120 << sh) + ((2 * xx + yy) << sh) // 40), (100 << sh) + n3],
                  np.where((yy // 4) % 2 == 0, np.abs(n3), peak - np.abs(n3)))
    return np.clip(v, 0, peak).astype(dtype or (np.uint8 if depth == 8 else np.uint16))


def plane_view(pay, entry):
    """The [rows, cols] view of one entry of a plane table into the flat payload ``pay``."""
    first, rows, cols, pitch = entry[:4]
    return np.lib.stride_tricks.as_strided(pay[first:], (rows, cols), (pitch * pay.itemsize, pay.itemsize))


def noisy_payload(h, w, layout, depth, seed, fields=None, rect=None, dtype=None, shift=0):
    """A payload every entry of whose plane table is a ``noisy_plane`` of its own."""
    g = np.random.RandomState(seed)
    out = np.zeros(y4m.payload_size(h, w, layout), dtype or (np.uint8 if depth == 8 else np.uint16))
    for n, entry in enumerate(DB.plane_table(h, w, layout, fields, rect)):
        plane_view(out, entry)[...] = noisy_plane(entry[1], entry[2], depth, 10 * seed + n, g, shift, out.dtype)
    return out


def noisy_clip(n, h, w, layout, d, seed=0, fps=b'24:1'):
    """A Y4M stream of ``noisy_payload`` frames whose pattern moves 3 samples a frame under noise that differs in every frame.  Returns
    (bytes, payloads as sample arrays); the header is that of the clips of tests/test_gpu_y4m_layouts.py."""
    from tests import test_gpu_y4m_layouts as Y
    data = Y._clip(1, h, w, layout, d, seed=seed, fps=fps)[0]
    pays = []
    for f in range(n):
        g = np.random.RandomState(4000 + 17 * seed + f)
        out = np.zeros(y4m.payload_size(h, w, layout), np.uint8 if d == 8 else np.uint16)
        for m, entry in enumerate(DB.plane_table(h, w, layout)):
            plane_view(out, entry)[...] = noisy_plane(entry[1], entry[2], d, 10 * seed + m, g, 3 * f, out.dtype)
        pays.append(out)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def stripes_payload(depth, dtype=None, h=20, w=34):
    """Columns of a and a + 1 in turn: at 16:1:1 every candidate weighs 256, and a sample of the first or the last column, off the corners,
    sees three of each: a tie, which rounds up: a + 1 in the first column (a) and in the last (a + 1)."""
    a = 77 << (depth - 8)
    return (a + (np.mgrid[0:h, 0:w][1] & 1)).astype(dtype or (np.uint8 if depth == 8 else np.uint16)).reshape(-1), h, w


def peaks_payload(h=40, w=72, seed=4):
    """16 bits: samples at 0 and at 65535 in patches and alone.  Under the box table (every weight 256, which the entry point takes) the
    definition's numerator leaves 32 bits; the kernel's sums do not."""
    g = np.random.RandomState(seed)
    v = np.where(g.randint(0, 4, (h, w)) > 0, 65535 - g.randint(0, 300, (h, w)), g.randint(0, 300, (h, w)))
    v[10:20, 20:50] = 65535
    v[12, 30] = 0
    v[25:35, 10:40] = 0
    v[30, 20] = 65535
    return v.astype(np.uint16).reshape(-1), h, w


# what tests/test_gpu_nlmeans.py::test_the_quotient_on_the_device runs: (depth, sample type, triple)
QUOTIENT_CASES = [(8, np.uint8, (3, 2, 5)), (8, np.uint16, (16, 3, 7)), (10, np.uint16, (3, 2, 5)), (10, np.uint16, (1, 1, 2)), (16, np.uint16, (6, 2, 4))]


@pytest.mark.parametrize('depth,dtype,spr', QUOTIENT_CASES, ids=['%d-%s-%d:%d:%d' % ((d, np.dtype(t).name) + s) for d, t, s in QUOTIENT_CASES])
def test_the_gpu_tests_payloads_cover_the_rule(depth, dtype, spr):
    S, Pr, R = spr
    h, w = 90, 150
    pay = noisy_payload(h, w, 'mono', depth, 21, dtype=dtype)
    c = NL.plane_cases(pay.reshape(h, w), depth, S, Pr, R)
    n = (2 * R + 1) ** 2
    assert (c['W'] == 256).any() and (c['live'] == 1).any()               # a sample whose only weight is the centre's
    assert (c['W'] == 256 * n).any()                                      # a sample where all (2R + 1)^2 candidates weigh 256
    assert c['indices'][0] and c['indices'][NL.K - 1] and c['indices'][1:NL.K - 1].sum() >= (NL.K - 2) // 2
    num = c['numerator'] - c['W']                                         # 2 sum(w (v - c))
    assert (num > 0).any() and (num < 0).any()
    H = R + Pr
    for bits in (1 | 4, 2 | 4, 1 | 8, 2 | 8, 1, 2, 4, 8, 0):              # clamped patches at the four corners, the four sides, and none
        assert (c['clamped'] == bits).any(), bits
    assert (c['clamped'][H:h - H, H:w - H] == 0).all() and (c['skipped'] > 0).any() and (c['skipped'][R:h - R, R:w - R] == 0).all()
    assert c['skipped'][0, 0] == n - (R + 1) ** 2 and c['changed'].mean() > 0.3
    assert np.array_equal(NL.kernel_quotient(c['wv'], c['W']), NL.nlmeans_plane_np(pay.reshape(h, w), depth, S, Pr, R))


def test_the_gpu_tests_ties_and_the_numerator_beyond_32_bits():
    for depth, dtype in ((8, np.uint8), (10, np.uint16), (16, np.uint16)):
        pay, h, w = stripes_payload(depth, dtype)
        c = NL.plane_cases(pay.reshape(h, w), depth, 16, 1, 1)
        tie = (c['numerator'] % (2 * c['W']) == 0) & (c['numerator'] != c['W'])          # the mean lies exactly between two codes
        assert tie[1:-1, 0].all() and tie[1:-1, -1].all() and (c['W'][1:-1, 0] == 6 * 256).all()
        out = NL.nlmeans_plane_np(pay.reshape(h, w), depth, 16, 1, 1)
        assert (out[1:-1, 0] == pay.reshape(h, w)[1:-1, 0] + 1).all() and (out[1:-1, -1] == pay.reshape(h, w)[1:-1, -1]).all()    # ties up
    pay, h, w = peaks_payload()
    c = NL.plane_cases(pay.reshape(h, w), 16, 1, 3, 7, table=BOX)
    assert int(c['numerator'].max()) >= 2 ** 31 and int(c['numerator'].min()) < -2 ** 31 and int(c['wv'].max()) < 2 ** 32
    assert np.array_equal(NL.kernel_quotient(c['wv'], c['W']), NL.nlmeans_plane_np(pay.reshape(h, w), 16, 1, 3, 7, table=BOX))
    # under the rule's own tables the numerator of the same plane stays within 32 bits (``accumulator_bounds``: numerator_rule)
    assert int(np.abs(NL.plane_cases(pay.reshape(h, w), 16, 16, 3, 7)['numerator']).max()) < 2 ** 31


@pytest.mark.parametrize('h,w,layout,d', [(64, 96, '420', 8), (48, 80, '420', 10), (48, 80, '444', 8)])
def test_the_gpu_tests_clip_moves_and_is_filtered(h, w, layout, d):
    data, pays = noisy_clip(4, h, w, layout, d, seed=3)
    assert data.startswith(b'YUV4MPEG2 W%d H%d ' % (w, h)) and len(pays) == 4 and data.count(b'FRAME\n') == 4
    assert all(not np.array_equal(a, b) for a, b in zip(pays, pays[1:]))
    outs = NL.nlmeans_stream_np(pays[:2], h, w, d, layout, *NL.DEFAULTS)
    assert all((o != p).mean() > 0.2 for o, p in zip(outs, pays))
