"""Weighted shutter windows (``--shutter-window``) on the host: the weight tables, ``shutter.mix_np`` with weights against exact rational
arithmetic, and ``shutter.magic_w``, the division of the weighted kernel, against floor division at every quotient boundary.  Nothing here
needs a GPU."""
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import shutter as SH


def test_the_weight_tables():
    assert SH.WINDOWS == ('box', 'triangle')
    assert SH.window_weights('triangle', 4) == [1, 2, 2, 1] and SH.window_weights('triangle', 5) == [1, 2, 3, 2, 1]
    for S in range(1, SH.MAX_SAMPLES + 1):
        box, tri = SH.window_weights('box', S), SH.window_weights('triangle', S)
        assert box == [1] * S == SH.window_weights(None, S)
        assert tri == [min(j + 1, S - j) for j in range(S)] == tri[::-1] and len(tri) == S
        assert all(isinstance(w, int) and w >= 1 for w in tri) and sum(tri) <= SH.MAX_WEIGHT_SUM
        assert (tri == box) == (S <= 2)
        assert max(tri) == (S + 1) // 2 and all(abs(a - b) <= 1 for a, b in zip(tri, tri[1:]))
    assert sum(SH.window_weights('triangle', 32)) == 272
    for bad in ('gaussian', 'Box', '', 3):
        with pytest.raises(ValueError, match='box, triangle'):
            SH.window_weights(bad, 4)
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match='samples'):
            SH.window_weights('triangle', bad)


def _half_up(q):
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


@pytest.mark.parametrize('es', [1, 2], ids=['bytes', '16-bit'])
def test_mix_np_with_weights_is_the_exact_weighted_mean_rounded_half_up(es):
    rng = np.random.default_rng(7 + es)
    P, peak = 23, 256 ** es - 1
    x = rng.integers(0, peak + 1, (40, P)).astype('<u2' if es == 2 else np.uint8)
    x[38], x[39] = 0, peak
    raw = x.view(np.uint8).reshape(40, P * es)
    for S in (1, 2, 3, 4, 5, 8, 32):
        w = SH.window_weights('triangle', S)
        groups = [list(range(c, c + k)) for c in (0, 3) for k in range(1, S + 1)] + [[39] * S, [38] * S]
        weights = [w[:len(g)] for g in groups]
        got = SH.mix_np(raw, groups, es, weights).view('<u2' if es == 2 else np.uint8)
        for c, (g, ws) in enumerate(zip(groups, weights)):
            want = [_half_up(Fraction(sum(wj * int(x[i, p]) for wj, i in zip(ws, g)), sum(ws))) for p in range(P)]
            assert got[c].tolist() == want, (S, c)
        assert (got[-2] == peak).all() and (got[-1] == 0).all()
    assert SH.group_weights([[8, 9, 10], [16]], 8, [1, 2, 2, 1]) == [[1, 2, 2], [1]]


def test_no_weights_and_unit_weights_give_todays_bytes():
    rng = np.random.default_rng(3)
    for es in (1, 2):
        raw = rng.integers(0, 256, (9, 34), dtype=np.uint8)
        groups = [[0, 1, 2, 3], [4, 5], [8], [2, 3, 4, 5, 6, 7, 8]]
        x = raw.view('<u2') if es == 2 else raw
        today = np.stack([(2 * x[g].sum(axis=0, dtype=np.int64) + len(g)) // (2 * len(g)) for g in groups]).astype(x.dtype).view(np.uint8)
        assert np.array_equal(SH.mix_np(raw, groups, es), today) and np.array_equal(SH.mix_np(raw, groups, es, None), today)
        assert np.array_equal(SH.mix_np(raw, groups, es, [[1] * len(g) for g in groups]), today)
    for bad in ([[1, 2]], [[1, 2, 0]], [[1, 2, -1]]):
        with pytest.raises(ValueError, match='weights'):
            SH.mix_np(raw, [[0, 1, 2]], 1, bad)


def test_a_constant_stays_constant_for_every_prefix():
    for es, values in ((1, (0, 1, 127, 128, 254, 255)), (2, (0, 1, 32767, 32768, 65534, 65535))):
        for v in values:
            x = np.full((32, 5), v, '<u2' if es == 2 else np.uint8).view(np.uint8).reshape(32, 5 * es)
            for S in range(1, 33):
                w = SH.window_weights('triangle', S)
                groups = [list(range(k)) for k in range(1, S + 1)]
                got = SH.mix_np(x, groups, es, [w[:k] for k in range(1, S + 1)]).view('<u2' if es == 2 else np.uint8)
                assert (got == v).all(), (es, v, S)


def _every_w():
    ws = {1023, 2047, 4095, 4096}
    for name in SH.WINDOWS:
        for S in range(1, SH.MAX_SAMPLES + 1):
            w = SH.window_weights(name, S)
            ws |= {sum(w[:k]) for k in range(1, S + 1)}
    return sorted(ws)


def test_magic_w_is_floor_division_at_every_quotient_boundary():
    for W in _every_w():
        mul, sh = SH.magic_w(W)
        assert 0 < mul < 1 << 32 and 0 <= sh < 32
        n_max = 2 * W * 65535 + W                                        # the largest numerator: every sample at the 16-bit peak
        assert n_max < 1 << 30
        q = np.arange(0, 65536 + 1, dtype=np.uint64)
        n = np.concatenate([2 * W * q - 1, 2 * W * q, 2 * W * q + 1, np.array([0, 1, W, n_max - 1, n_max], np.uint64)])
        n = n[(n <= n_max)]                                              # 2 W 0 - 1 wraps to 2^64 - 1 and drops out here
        got = ((n * np.uint64(mul)) >> np.uint64(32)) >> np.uint64(sh)  # n * mul < 2^62: exact in uint64
        assert np.array_equal(got, n // np.uint64(2 * W)), W
    rng = np.random.default_rng(0)
    for W in (1, 3, 272, 4096):                                          # and anywhere in between
        mul, sh = SH.magic_w(W)
        n = rng.integers(0, 2 * W * 65535 + W + 1, 200000).astype(np.uint64)
        assert np.array_equal(((n * np.uint64(mul)) >> np.uint64(32)) >> np.uint64(sh), n // np.uint64(2 * W))
    for bad in (0, 4097, -1, 2.0, True):
        with pytest.raises(ValueError, match='magic_w'):
            SH.magic_w(bad)
    assert SH.magic_w(1) == ((131073 << 14), 0)                          # s = 18 < 32: M = 2^18 / 2 + 1, pre-shifted
