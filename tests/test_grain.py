"""Film grain (``--grain``, ``demfi_amd.grain``) on the host: the definition against values computed by hand in plain Python ints, the
moments of the field, the rule and its clip, the accumulator bound, the switches, the spec and the egress layout, and the stream form."""
import io
import itertools
import math

import numpy as np
import pytest

from demfi_amd import grain as G
from demfi_amd import interlace as IL
from demfi_amd import y4m
from demfi_amd.pipeline import EdgeSpec
from demfi_amd.y4m_edge import Buffer, LinearBuffer, egress_layout

M = 0xFFFFFFFF
P = (32, 1, 8, 'film', 0)                                                # S = 2, size 1, C = 0.5


# ---- the definition, in plain ints ---------------------------------------------------------------------------------------------
def _mix(x):
    x &= M
    x ^= x >> 16
    x = (x * 0x7feb352d) & M
    x ^= x >> 15
    x = (x * 0x846ca68b) & M
    return x ^ (x >> 16)


def _key(seed, n, p):
    return _mix((seed + 0x9E3779B9 * (4 * n + p + 1)) % (1 << 32))


def _white(key, X, Y):
    u = _mix(key ^ _mix((Y << 16) | X))
    return sum((u >> s) & 255 for s in (0, 8, 16, 24)) - 510


def test_hash_keys_and_white_cells_against_hand_computed_values():
    assert _mix(0) == 0 and G.mix32(0) == 0
    for x in (1, 0x9E3779B9, M, 0x12345678):
        assert G.mix32(x) == _mix(x) == int(G.mix32(np.array([x], np.uint32))[0])
    assert _key(0, 0, 0) == 0x01fce552 == G.plane_key(0, 0, 0)
    assert _key(1, 2, 1) == 0x11e0d632 == G.plane_key(1, 2, 1)
    key = 0x01fce552
    pinned = [[144, 282, 26, 184], [245, -133, -60, 213]]
    assert [[_white(key, X, Y) for X in range(4)] for Y in range(2)] == pinned
    assert G.white(key, np.arange(4)[None, :], np.arange(2)[:, None]).tolist() == pinned
    rng = np.random.default_rng(0)
    for k, X, Y in zip(rng.integers(0, 1 << 32, 50), rng.integers(0, 65536, 50), rng.integers(0, 65536, 50)):
        assert int(G.white(int(k), int(X), int(Y))) == _white(int(k), int(X), int(Y))
    assert _white(key, 65535, 65535) == int(G.white(key, 65535, 65535))
    with pytest.raises(ValueError):
        G.white(key, 65536, 0)


def test_field_is_the_binomial_sum_of_cells_two_to_the_right_and_down():
    key = G.plane_key(7, 3, 2)
    for r, c in enumerate(G.TAPS):
        F = G.field_np(key, 5, 6, r)
        for y, x in ((0, 0), (4, 5), (2, 3)):
            assert int(F[y, x]) == sum(c[i + r] * c[j + r] * _white(key, x + 2 + i, y + 2 + j) for i in range(-r, r + 1) for j in range(-r, r + 1))
        assert sum(t * t for t in c) == G.NORM[r]
    for bad in ((0, 4), (4, 0), (G.MAX_SIDE + 1, 4), (4, G.MAX_SIDE + 1)):
        with pytest.raises(ValueError, match='65531'):
            G.field_np(key, bad[0], bad[1], 1)


# ---- moments -----------------------------------------------------------------------------------------------------------------
def test_white_has_mean_zero_and_variance_21845_by_enumeration():
    counts = np.ones(1, np.int64)
    for _ in range(4):                                                   # the distribution of the sum of four bytes
        counts = np.convolve(counts, np.ones(256, np.int64))
    s = np.arange(counts.size) - 510
    total = int(counts.sum())
    assert total == 256 ** 4 and int((counts * s).sum()) == 0
    assert int((counts * s * s).sum()) == G.WHITE_VAR * total
    assert s[0] == -510 and s[-1] == 510


def _rho2(r):
    """The sum over all lags of the squared normalised autocorrelation of the 1-D taps."""
    c = np.array(G.TAPS[r], np.float64)
    a = np.convolve(c, c[::-1])
    return float(((a / a.max()) ** 2).sum())


@pytest.mark.parametrize('r', [0, 1, 2])
def test_variance_of_the_field_over_a_512_plane(r):
    N = 512 * 512
    F = G.field_np(G.plane_key(0, 0, 0), 512, 512, r).astype(np.float64)
    want = G.WHITE_VAR * G.NORM[r] ** 2
    se = math.sqrt(2.0 * _rho2(r) ** 2 / N)                              # of the variance estimate, relative (the field is separable)
    rel = F.var() / want - 1.0
    print('r=%d: variance off by %+.3f %%, one standard error %.3f %%' % (r, 100 * rel, 100 * se))
    assert abs(rel) <= 5 * se
    assert abs(F.mean()) <= 5 * math.sqrt(want / N) * sum(G.TAPS[r]) ** 2 / G.NORM[r]


def test_frames_and_planes_are_uncorrelated():
    N = 512 * 512
    for r in (0, 1, 2):
        a = G.field_np(G.plane_key(0, 0, 0), 512, 512, r).astype(np.float64)
        for other in (G.plane_key(0, 1, 0), G.plane_key(0, 0, 1)):
            b = G.field_np(other, 512, 512, r).astype(np.float64)
            rho = float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])
            print('r=%d: correlation %+.5f' % (r, rho))
            assert abs(rho) <= 5 / math.sqrt(N)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_flat_grain_of_two_on_mid_grey_has_a_deviation_of_two():
    for r in (0, 1, 2):
        g = int(G.gain_table(8, 32, r, 16, 'flat', False)[128])
        assert g == math.floor(65536 * 2 / (math.sqrt(21845) * G.NORM[r]) + 0.5)
        assert (G.gain_table(8, 32, r, 16, 'flat', False) == g).all()
        pay = np.full(512 * 512, 128, np.uint8)
        out = G.grain_payload_np(pay, 512, 512, 'mono', 8, False, 0, (32, r, 8, 'flat', 0)).astype(np.float64)
        want = G.WHITE_VAR * G.NORM[r] ** 2 * (g / 65536.0) ** 2 + 1.0 / 12.0       # the table's entry, and the rounding to integers
        se = math.sqrt(2.0 * _rho2(r) ** 2 / (512 * 512))
        print('r=%d: G=%d, deviation %.4f, expected %.4f' % (r, g, out.std(), math.sqrt(want)))
        assert abs(out.var() / want - 1.0) <= 5 * se
        assert abs(math.sqrt(want - 1.0 / 12.0) - 2.0) <= 2.0 * 0.5 / g    # the entry is rounded to an integer: half a step of g
        assert abs(out.mean() - 128.0) <= 5 * math.sqrt(want / (512 * 512)) * sum(G.TAPS[r]) ** 2 / G.NORM[r]
        assert out.min() >= 16 and out.max() <= 235


def test_gain_tables():
    for r, curve, full in itertools.product((0, 1, 2), G.CURVES, (False, True)):
        g8 = G.gain_table(8, 40, r, 16, curve, full)
        for d in (10, 12, 14, 16):
            k = 1 << (d - 8)
            assert (np.abs(G.gain_table(d, 40, r, 16, curve, full) - k * g8) <= k / 2 + 0.5).all()
        half = G.gain_table(8, 40, r, 8, curve, full)
        assert (np.abs(2 * half - g8) <= 1.5).all()
        assert (G.gain_table(8, 0, r, 16, curve, full) == 0).all() and (G.gain_table(8, 40, r, 0, curve, full) == 0).all()
    t = G.gain_tables(10, (24, 2, 4, 'film', 9), True)
    assert t.shape == (2, 256) and t.dtype == np.int32
    assert (t[0] == G.gain_table(10, 24, 2, 16, 'film', True)).all() and (t[1] == G.gain_table(10, 24, 2, 4, 'film', True)).all()


def test_the_film_curve_is_symmetric_and_a_quarter_at_both_ends():
    lim, full = G.curve8('film', False), G.curve8('film', True)
    assert (full == full[::-1]).all() and full[0] == full[255] == 64 and full.max() == 256
    assert (lim[16:236] == lim[16:236][::-1]).all() and (lim[:17] == 64).all() and (lim[235:] == 64).all() and lim.max() == 256
    assert lim[125] == lim[126] == 256 and abs(int(full[127]) - 256) <= 1
    assert all(int(lim[c]) == math.floor(256 * (0.25 + 3 * t * (1 - t)) + 0.5) for c in (40, 100, 200) for t in [(c - 16) / 219])
    assert (G.curve8('flat', False) == 256).all() and (G.curve8('flat', True) == 256).all()
    with pytest.raises(ValueError, match='film, flat'):
        G.curve8('log', False)


def test_clip_cases_by_hand():
    g, up, down = 65536, 7, -7                                           # delta = F exactly
    rule = lambda v, f: int(G.apply_rule(np.array([v]), np.array([f]), g, 16, 235)[0])      # noqa: E731
    assert rule(16, down) == 16 and rule(16, up) == 23                   # at lo
    assert rule(235, up) == 235 and rule(235, down) == 228               # at hi
    assert rule(5, down) == 5 and rule(5, up) == 12                      # below lo: not pulled in, not pushed further out
    assert rule(250, up) == 250 and rule(250, down) == 243               # above hi
    assert rule(230, 20) == 235 and rule(20, -20) == 16                  # a legal sample stays legal
    assert rule(5, 300) == 235 and rule(250, -300) == 16
    assert rule(100, 0) == 100 and rule(3, 0) == 3 and rule(255, 0) == 255
    # the shift floors: (F G + 2^15) >> 16 rounds halves up, also below zero
    assert [int(G.apply_rule(np.array([100]), np.array([f]), 1 << 15, 0, 255)[0]) for f in (1, -1, 3, -3)] == [101, 100, 102, 99]
    assert G.nominal_range(8, False, False) == (16, 235) and G.nominal_range(10, False, True) == (64, 960)
    assert G.nominal_range(16, False, False) == (4096, 60160) and G.nominal_range(12, True, True) == (0, 4095)


def _payload(rng, h, w, layout, depth):
    n = y4m.payload_size(h, w, layout)
    return rng.integers(0, 1 << min(depth + 1, 16) if depth > 8 else 256, n).astype(np.uint16 if depth > 8 else np.uint8)


def test_zero_strength_is_the_identity_and_the_output_is_a_pure_function():
    rng = np.random.default_rng(1)
    for layout, depth, full in itertools.product(y4m.LAYOUTS, (8, 10, 16), (False, True)):
        pay = _payload(rng, 9, 11, layout, depth)
        out = G.grain_payload_np(pay, 9, 11, layout, depth, full, 3, (0, 2, 16, 'flat', 5))
        assert out.dtype == pay.dtype and np.array_equal(out, pay)
        a = G.grain_payload_np(pay, 9, 11, layout, depth, full, 3, P)
        assert np.array_equal(a, G.grain_payload_np(pay.copy(), 9, 11, layout, depth, full, 3, P)) and not np.array_equal(a, pay)
        assert not np.array_equal(a, G.grain_payload_np(pay, 9, 11, layout, depth, full, 4, P))
        assert not np.array_equal(a, G.grain_payload_np(pay, 9, 11, layout, depth, full, 3, P[:4] + (1,)))
    with pytest.raises(ValueError, match='uint16 samples at 8 bits'):
        G.grain_payload_np(np.zeros(99, np.uint16), 9, 11, 'mono', 8, False, 0, P)
    with pytest.raises(ValueError, match='98 samples'):
        G.grain_payload_np(np.zeros(98, np.uint8), 9, 11, 'mono', 8, False, 0, P)


def test_mono_and_zero_chroma_strength_grain_luma_only():
    rng = np.random.default_rng(2)
    h, w = 10, 14
    pay = rng.integers(60, 200, y4m.payload_size(h, w, '420')).astype(np.uint8)
    out = G.grain_payload_np(pay, h, w, '420', 8, False, 0, (64, 1, 0, 'film', 0))
    assert np.array_equal(out[h * w:], pay[h * w:]) and not np.array_equal(out[:h * w], pay[:h * w])
    mono = G.grain_payload_np(pay[:h * w], h, w, 'mono', 8, False, 0, (64, 1, 0, 'film', 0))
    assert np.array_equal(mono, out[:h * w])                             # the luma plane does not know the layout
    both = G.grain_payload_np(pay, h, w, '420', 8, False, 0, (64, 1, 16, 'film', 0))
    assert np.array_equal(both[:h * w], out[:h * w]) and not np.array_equal(both[h * w:], pay[h * w:])


@pytest.mark.parametrize('layout', ['420', '422'])
def test_the_chroma_luma_index_at_the_right_and_bottom_edge_of_odd_planes(layout):
    h, w = 5, 7
    (_, _), (ch, cw), _ = IL.plane_shapes(h, w, layout)
    sy, sx = (2, 2) if layout == '420' else (1, 2)
    assert (ch, cw) == ((h + sy - 1) // sy, (w + sx - 1) // sx)
    luma = np.arange(h * w, dtype=np.int64).reshape(h, w)
    L = G.chroma_luma(luma, ch, cw)
    for y, x in itertools.product(range(ch), range(cw)):
        assert L[y, x] == luma[min(y * sy, h - 1), min(x * sx, w - 1)]
    # through the payload: the luma is black but for its last column and last row, which are mid-grey: under the film curve only the
    # chroma samples that read those get the full gain
    Y = np.full((h, w), 16, np.uint8)
    Y[:, w - 1], Y[h - 1, :] = 126, 126
    pay = np.concatenate([Y.reshape(-1), np.full(2 * ch * cw, 128, np.uint8)])
    params = (128, 0, 16, 'film', 3)
    out = G.grain_payload_np(pay, h, w, layout, 8, False, 2, params)
    tab = G.gain_tables(8, params, False)[1]
    for p in (1, 2):
        key = _key(3, 2, p)
        got = out[h * w + (p - 1) * ch * cw:h * w + p * ch * cw].reshape(ch, cw)
        for y, x in itertools.product(range(ch), range(cw)):
            c = int(Y[min(y * sy, h - 1), min(x * sx, w - 1)])
            assert c == (126 if x == cw - 1 or min(y * sy, h - 1) == h - 1 else 16)
            d = (_white(key, x + 2, y + 2) * int(tab[c]) + (1 << 15)) >> 16
            assert got[y, x] == min(max(128 + d, 16), 240), (p, y, x)
    assert abs(int(tab[126]) - 4 * int(tab[16])) <= 2                    # a quarter at black, up to the two roundings


# ---- bounds and switches ---------------------------------------------------------------------------------------------------------
def test_accumulator_bounds_against_brute_force_for_every_depth_and_size_at_the_cap():
    widest = 0
    for d, r in itertools.product(y4m.DEPTHS, (0, 1, 2)):
        lo, hi = G.accumulator_bounds(d, G.MAX_S16, r)
        fmax = 510 * sum(G.TAPS[r]) ** 2                                 # every cell at its extreme, every tap positive
        gains = [int(G.gain_table(d, G.MAX_S16, r, 16, curve, full).max()) for curve in G.CURVES for full in (False, True)]
        brute = [f * g + (1 << 15) for f in (-fmax, fmax) for g in gains + [0]]
        assert (lo, hi) == (min(brute), max(brute))
        assert -(1 << 31) <= lo and hi < (1 << 31), (d, r)               # the kernel's product is a 32-bit one everywhere
        widest = max(widest, hi)
        assert G.accumulator_bounds(d, G.MAX_S16, r, 8)[1] <= hi
    assert 1.68e9 < widest < 1.70e9 and widest == G.accumulator_bounds(16, 128, 2)[1]


def test_parse_and_check():
    assert [G.parse_strength(t) for t in ('0', '2', '1.5', ' 0.03 ', '0.04', '8', 2, 0.25)] == [0, 32, 24, 0, 1, 128, 32, 4]
    assert [G.parse_chroma(t) for t in ('0', '0.5', '1', '0.3')] == [0, 8, 16, 5]
    assert [G.parse_seed(t) for t in ('0', '0x10', '4294967295', 7)] == [0, 16, M, 7]
    for fn, bad in ((G.parse_strength, ('8.01', '-1', 'x', '', True)), (G.parse_chroma, ('1.1', '-0.1', 'half')),
                    (G.parse_seed, ('-1', '4294967296', '1.5', 'seed', True)), (G.check_size, (3, -1, '1', True, 1.0)),
                    (G.check_curve, ('log', 1))):
        for b in bad:
            with pytest.raises(ValueError):
                fn(b)
    assert G.check_size(None) == 1 and G.check_curve(None) == 'film' and [G.check_size(r) for r in (0, 1, 2)] == [0, 1, 2]
    assert G.check_params((32, 1, 8, 'film', 0)) == (32, 1, 8, 'film', 0)
    for bad in ((129, 1, 8, 'film', 0), (-1, 1, 8, 'film', 0), (32, 3, 8, 'film', 0), (32, 1, 17, 'film', 0), (32, 1, 8, 'log', 0),
                (32, 1, 8, 'film', -1), (32, 1, 8, 'film'), None, (1.5, 1, 8, 'film', 0)):
        with pytest.raises(ValueError):
            G.check_params(bad)
    assert G.check_grain() is None and G.check_grain('0') is None and G.check_grain('0', 2, '1', 'flat', 9) is None
    assert G.check_grain('2') == (32, 1, 8, 'film', 0) and G.check_grain('1.5', 2, '0.25', 'flat', '0xff') == (24, 2, 4, 'flat', 255)
    for kw in (dict(size=1), dict(chroma='0.5'), dict(curve='film'), dict(seed=0)):
        with pytest.raises(ValueError, match='give --grain S'):
            G.check_grain(None, **kw)
    for kw in (dict(grain='9'), dict(grain='2', size=3), dict(grain='2', chroma='2'), dict(grain='2', curve='x'), dict(grain='2', seed=-1)):
        with pytest.raises(ValueError):
            G.check_grain(**kw)
    with pytest.raises(ValueError, match='one rank'):
        G.check_grain('2', ranks=2)


def test_the_video_switches_and_the_one_rank_refusal(tmp_path):
    from demfi_amd import video
    assert video.check_grain('2', 0, '1', 'flat', 5) == (32, 0, 16, 'flat', 5) and video.check_grain() is None and video.check_grain(0) is None
    with pytest.raises(ValueError, match='grain with 2 ranks.*one rank'):
        video.check_grain('2', world=2)
    video.check_grain('0', world=2)                                      # no stage: nothing to refuse
    with pytest.raises(ValueError, match='--grain-seed.*give --grain S'):
        video.VideoRunner(None, mfi=2, grain_seed=4)
    for kw in (dict(grain='8.5'), dict(grain=1, grain_size=4), dict(grain=1, grain_chroma='1.5')):
        with pytest.raises(ValueError):
            video.VideoRunner(None, mfi=2, **kw)
    assert 'grain' in video.ONE_RANK_EGRESS and 'last_grain_payloads' in video.EGRESS_COUNTERS.values()
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n' + (b'FRAME\n' + bytes(96 * 64 * 3 // 2)) * 5)
    vr = video.VideoRunner(None, mfi=2, grain='1.5', grain_size=2)
    assert vr.grain == (24, 2, 8, 'film', 0) and vr.last_grain is None and vr.last_grain_payloads == 0
    with pytest.raises(ValueError, match='grain with 2 ranks'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'), world=2, rank=1)          # no model: nothing ran
    assert not (tmp_path / 'out.y4m').exists()
    assert video.VideoRunner(None, mfi=2, grain=0).grain is None
    a = video.parser().parse_args(['in', 'out', '--grain', '1.5', '--grain-size', '2', '--grain-chroma', '0.25', '--grain-curve', 'flat',
                                   '--grain-seed', '0x2a'])
    assert video.check_grain(a.grain, a.grain_size, a.grain_chroma, a.grain_curve, a.grain_seed) == (24, 2, 4, 'flat', 42)
    for argv in (['--grain', '9'], ['--grain', '1', '--grain-size', '3'], ['--grain', '1', '--grain-chroma', '2'], ['--grain', '1', '--grain-seed', '-1']):
        with pytest.raises(SystemExit):
            video.parser().parse_args(['in', 'out'] + argv)
    edge = video.YuvEdge('bt601', False, '420jpeg', lambda k: False, grain=(24, 2, 8, 'film', 0))
    assert edge.grain == (24, 2, 8, 'film', 0) and EdgeSpec.of(edge).grain == edge.grain
    assert video.YuvEdge('bt601', False, '420jpeg', lambda k: False, grain=(0, 2, 8, 'film', 0)).grain is None


# ---- the spec and the layout -------------------------------------------------------------------------------------------------------
def test_edge_spec_with_and_without_grain():
    plain, g = EdgeSpec(True, depth=10), EdgeSpec(True, depth=10, grain=P)
    assert plain.grain is None and g.grain == P and plain != g and g != plain and hash(plain) != hash(g)
    assert plain == EdgeSpec(True, depth=10, grain=None) == EdgeSpec(True, depth=10, grain=(0, 1, 8, 'film', 0))
    assert hash(plain) == hash(EdgeSpec(True, depth=10, grain=(0, 2, 16, 'flat', 9)))
    assert tuple(plain) == tuple(g) == (True, False, False, 10, '420', None, None, 'bob')
    assert g == EdgeSpec(True, depth=10, grain=list(P)) and g != EdgeSpec(True, depth=10, grain=P[:4] + (1,))
    assert 'grain' not in repr(plain) and repr(g).endswith(", grain=(32, 1, 8, 'film', 0))")
    assert g._replace(depth=8).grain == P and g._replace(grain=None) == plain and plain._replace(grain=P) == g
    assert g._replace(scale=(10, 10, 'bicubic')).grain == P and g._replace(scale=(10, 10, 'bicubic')) != g
    assert len({plain, g, EdgeSpec(True, depth=10, grain=P)}) == 2
    g.check(True, True, True)
    with pytest.raises(ValueError, match='film grain needs the Y4M edge'):
        EdgeSpec(False, grain=P).check(False, False, False)
    for bad in ((200, 1, 8, 'film', 0), (32, 5, 8, 'film', 0), (32, 1, 8, 'grey', 0)):
        with pytest.raises(ValueError, match='grain must be None or'):
            EdgeSpec(True, grain=bad).check(True, True, True)


def test_the_layout_without_grain_is_what_it_was():
    sp = EdgeSpec(True, depth=10, shutter=(2, 4), interlace=('t', 'linear'), depths=(8, 10, 8, 'bayer'))
    assert egress_layout(sp, 9, 2, 64, 96) == [Buffer('gather', 1, 9, 18432, 64, 96), Buffer('mix', 1, 6, 18432, 64, 96),
                                               Buffer('weave', 0, 4, 18432, 64, 96), Buffer('requant', 0, 4, 9216, 64, 96), (4, 9216)]
    assert egress_layout(EdgeSpec(True), 9, 2, 64, 96) == [Buffer('gather', 0, 9, 9216, 64, 96), (9, 9216)]
    assert egress_layout(EdgeSpec(True, grain=(0, 1, 8, 'film', 0)), 9, 2, 64, 96) == egress_layout(EdgeSpec(True), 9, 2, 64, 96)


def test_the_layout_with_grain_in_every_combination():
    order = ['gather', 'mix', 'scale', 'encode', 'grain', 'weave', 'requant']
    for mix, scale, lin, weave, requant in itertools.product((False, True), repeat=5):
        kw = dict(shutter=(3, 4) if mix else None, scale=(72, 48, 'bicubic') if scale else None, colour=('bt709', None, None) if lin else None,
                  interlace=('b', 'off') if weave else None, depths=(8, 10, 8, 'none') if requant else None)
        base = EdgeSpec(True, depth=10 if requant else 8, **kw)
        *b0, host0 = egress_layout(base, 13, 3, 64, 96)
        *b1, host1 = egress_layout(base._replace(grain=P), 13, 3, 64, 96)
        names = [b.name for b in b1]
        assert names == [n for n in order if n == 'grain' or n in [b.name for b in b0]] and host1 == host0
        at = names.index('grain')
        src, own = b1[at - 1], b1[at]
        assert src.name == [n for n in ('encode', 'scale', 'mix', 'gather') if n in names][0]
        assert not isinstance(src, LinearBuffer) and type(own) is Buffer         # the stage never sees linear light
        assert (own.rows, own.Pb, own.h, own.w) == (src.rows, src.Pb, src.h, src.w) and src.lead == 0
        assert own.lead == b0[at - 1].lead == (1 if weave else 0)        # the weave's carried frame now lies in front of the grained ones
        assert b1[:at - 1] == b0[:at - 1] and b1[at + 1:] == b0[at:] and src._replace(lead=own.lead) == b0[at - 1]
        assert own.Pb == y4m.payload_size(own.h, own.w, '420') * (2 if requant else 1) and (own.w, own.h) == ((72, 48) if scale else (96, 64))


# ---- streams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ctag,layout,depth', [(b'C420jpeg', '420', 8), (b'C422p10', '422', 10), (b'Cmono', 'mono', 8)])
def test_grain_stream_np(ctag, layout, depth):
    h, w, rng = 6, 10, np.random.default_rng(4)
    head = b'YUV4MPEG2 W10 H6 F25:1 Ip A1:1 ' + ctag + b' XCOLORRANGE=FULL\n'
    pays = [_payload(rng, h, w, layout, min(depth, 15)) for _ in range(3)]
    stream = head + b''.join(b'FRAME\n' + p.astype('<u2' if depth > 8 else np.uint8).tobytes() for p in pays)
    out = G.grain_stream_np(stream, P)
    assert len(out) == len(stream) and out.startswith(head) and out != stream
    es = 2 if depth > 8 else 1
    size = 6 + pays[0].size * es
    for n, p in enumerate(pays):
        body = out[len(head) + n * size + 6:len(head) + (n + 1) * size]
        assert out[len(head) + n * size:len(head) + n * size + 6] == b'FRAME\n'
        want = G.grain_payload_np(p, h, w, layout, depth, True, n, P)
        assert body == want.astype('<u2' if depth > 8 else np.uint8).tobytes()
    assert G.grain_stream_np(stream, None) == stream == G.grain_stream_np(stream, (0, 1, 8, 'film', 0))
    limited = G.grain_stream_np(stream.replace(b' XCOLORRANGE=FULL', b''), P)
    assert limited[len(head) - 17:] != out[len(head):]                   # the range written is the header's
    rd = y4m.Reader(io.BytesIO(out), y4m.DEPTHS, y4m.LAYOUTS)
    assert (rd.header.w, rd.header.h, rd.header.layout, rd.header.depth, rd.header.full_range) == (w, h, layout, depth, True)
