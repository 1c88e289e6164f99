"""CPU tests of the retime schedule (``demfi_amd.retime``, ``python -m demfi_amd.video --fps``): frame rate parsing, the output
frames of every window for common conversions, the exact reduction to the x M stream for r = M, rank block offsets and the
default n_ctx choice."""
import math
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import video, y4m
from demfi_amd.dist import shard_windows
from demfi_amd.harness import t_schedule

HDR = y4m.parse_header(b'YUV4MPEG2 W98 H70 F24:1 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL')


# ---- --fps parsing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text,exp', [('60', Fraction(60)), ('60000/1001', Fraction(60000, 1001)), ('60000:1001', Fraction(60000, 1001)),
                                      ('120/2', Fraction(60)), (' 25 ', Fraction(25))])
def test_fps_accepted(text, exp):
    assert R.parse_fps(text) == exp


@pytest.mark.parametrize('text', ['0', '-1', 'abc', '', '60/0', '0/1001', '60/', '1e3', '60/1.001', '59.94'])
def test_fps_rejected(text):
    with pytest.raises(ValueError):
        R.parse_fps(text)


def test_decimal_fps_points_to_a_fraction():
    with pytest.raises(ValueError, match='N/D'):
        R.parse_fps('59.94')


def test_ratio_below_one_is_rejected():
    assert R.ratio(Fraction(24), Fraction(60)) == Fraction(5, 2)
    assert R.ratio(Fraction(30000, 1001), Fraction(30000, 1001)) == 1
    with pytest.raises(ValueError, match='below'):
        R.ratio(Fraction(60), Fraction(30))


@pytest.mark.parametrize('argv', [['-', '-', '--fps', '60', '--mfi', '2'], ['-', '-', '--fps', '59.94'], ['-', '-', '--fps', '0'],
                                  ['-', '-', '--fps', '-1'], ['-', '-', '--fps', 'abc']])
def test_cli_rejects(argv):
    with pytest.raises(SystemExit) as e:
        video.main(argv)
    assert e.value.code == 2


@pytest.mark.parametrize('fps', [59.94, 60.0, True])
def test_video_runner_refuses_inexact_fps(fps):
    with pytest.raises(TypeError, match='N/D'):
        video.VideoRunner(None, 1, fps=fps)


def test_ratio_is_bounded():
    assert R.ratio(1, R.MAX_RATIO) == R.MAX_RATIO
    with pytest.raises(ValueError, match='more than'):
        R.ratio(24, 24 * R.MAX_RATIO + 1)


def test_default_n_ctx_of_a_long_period_is_quick():
    """A Y4M rate with a period of 4e11 windows: the choice samples the first SCAN_WINDOWS of them."""
    r = R.ratio(Fraction(24000, 1001), Fraction(999999937, 16666667))
    assert r.denominator > 10 ** 11
    assert R.default_n_ctx(r, lambda d: True) in range(1, 9)


def test_video_runner_takes_mfi_or_fps():
    with pytest.raises(ValueError, match='not both'):
        video.VideoRunner(None, 1, 4, fps=Fraction(60))
    assert video.VideoRunner(None, 1).mfi == 8
    vr = video.VideoRunner(None, 1, fps='60000:1001')
    assert vr.fps == Fraction(60000, 1001) and vr.mfi is None


# ---- the schedule ---------------------------------------------------------------------------------------------------------
def _check_schedule(n, r):
    """The per-window lists tile 0 .. N_out-1 in order, and every output is the frame the definition says."""
    r = Fraction(r)
    nw = n - 3
    seen = []
    for k in range(nw):
        outs = R.window_outputs(k, r, last=k == nw - 1)
        assert outs and outs[0][0] == R.first_output(k, r)
        for i, kind, t in outs:
            tau = 1 + Fraction(i) / r
            assert tau <= n - 2
            if kind == R.S0:
                assert tau == k + 1
            elif kind == R.S1:
                assert tau == n - 2 and k == nw - 1
            else:
                assert math.floor(tau) - 1 == k and t == float(np.float32(t))
                assert abs(Fraction(t) - (tau - math.floor(tau))) <= Fraction(1, 2 ** 25)
        seen += [i for i, _, _ in outs]
        ts = R.instants(k, r)
        st = [t for _, kind, t in outs if kind == R.ST]
        assert ts == (sorted(set(st)) or [0.5])
    assert seen == list(range(R.n_output_frames(n, r)))
    assert all(1 + Fraction(i) / r > n - 2 for i in [len(seen)])          # the next frame would be past the last input
    return seen


def _windows(n, r):
    return [[(i, kind, None if t is None else round(t, 6)) for i, kind, t in R.window_outputs(k, r, last=k == n - 4)]
            for k in range(n - 3)]


def test_24_to_60():
    r = R.ratio(24, 60)
    assert R.n_output_frames(10, r) == 18
    w = _windows(10, r)
    assert w[0] == [(0, 'S0', None), (1, 'St', 0.4), (2, 'St', 0.8)]
    assert w[1] == [(3, 'St', 0.2), (4, 'St', 0.6)]
    assert w[2] == [(5, 'S0', None), (6, 'St', 0.4), (7, 'St', 0.8)]
    assert w[6] == [(15, 'S0', None), (16, 'St', 0.4), (17, 'St', 0.8)]   # (n-3) r = 17.5: no S1
    assert R.instants(0, r) == [np.float32(0.4), np.float32(0.8)]
    _check_schedule(10, r)


def test_25_to_60():
    r = R.ratio(25, 60)
    assert R.n_output_frames(10, r) == 17
    w = _windows(10, r)
    assert [kind for _, kind, _ in w[2]] == ['St'] * 3
    assert R.instants(2, r) == [float(np.float32(1 / 12)), 0.5, float(np.float32(11 / 12))]
    assert sum(max(1, len(R.instants(k, r))) for k in range(5)) == 11      # 2.2 per window
    _check_schedule(10, r)


def test_ntsc_x2_is_exact():
    r = R.ratio(Fraction(30000, 1001), Fraction(60000, 1001))
    assert r == 2
    assert R.n_output_frames(9, r) == y4m.n_output_frames(9, 2) == 13
    assert [R.instants(k, r) for k in range(3)] == [[0.5]] * 3
    _check_schedule(9, r)


def test_seven_thirds():
    r = Fraction(7, 3)
    assert R.n_output_frames(11, r) == math.floor(8 * r) + 1 == 19
    for n in range(4, 20):
        _check_schedule(n, r)


def test_r1_is_a_deblurrer():
    w = _windows(6, 1)
    assert w == [[(0, 'S0', None)], [(1, 'S0', None)], [(2, 'S0', None), (3, 'S1', None)]]
    assert R.n_output_frames(6, 1) == 4
    assert all(R.instants(k, 1) == [0.5] for k in range(3))
    assert R.window_plan(2, 1, last=True) == ([0.5], [(2, 'S0', 0), (3, 'S1', 0)])


def test_no_window_below_four_frames():
    for n in range(4):
        assert R.n_output_frames(n, Fraction(5, 2)) == 0


@pytest.mark.parametrize('m', range(2, 17))
def test_integer_ratio_is_the_x_m_stream(m):
    n = 9
    hdr = y4m.Header(98, 70, Fraction(30000, 1001), aspect='1:1', color_range='LIMITED')
    assert R.output_header(hdr, hdr.fps * m).encode() == y4m.output_header(hdr, m).encode()
    assert R.n_output_frames(n, m) == y4m.n_output_frames(n, m)
    for k in range(n - 3):
        outs = R.window_outputs(k, m, last=k == n - 4)
        exp = [(y4m.output_index(k, 0, m), 'S0')] + [(y4m.output_index(k, j, m), 'St') for j in range(1, m)]
        if k == n - 4:
            exp.append((y4m.output_index(k, m, m), 'S1'))
        assert [(i, kind) for i, kind, _ in outs] == exp
        ts = np.array(R.instants(k, m), np.float32)
        assert ts.tobytes() == t_schedule(m).tobytes()


def test_output_header_fields():
    h = R.output_header(HDR, Fraction(120, 2))
    assert h.encode() == b'YUV4MPEG2 W98 H70 F60:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n'
    assert R.output_header(HDR, Fraction(60000, 1001)).encode().split()[3] == b'F60000:1001'


def test_float32_rounding_is_exact():
    for num, den in [(1, 3), (2, 3), (1, 12), (11, 12), (1000, 1001), (1, 2 ** 30), (2 ** 24 + 1, 2 ** 25)]:
        x = Fraction(num, den)
        v = R.float32_of(x)
        lo, hi = np.nextafter(np.float32(v), np.float32(0)), np.nextafter(np.float32(v), np.float32(1))
        assert abs(Fraction(v) - x) <= abs(Fraction(float(lo)) - x) and abs(Fraction(v) - x) <= abs(Fraction(float(hi)) - x)
    assert R.float32_of(Fraction(2 ** 24 + 1, 2 ** 25)) == 0.5                                  # a tie goes to the even mantissa


@pytest.mark.parametrize('r', [Fraction(5, 2), Fraction(12, 5), Fraction(2500, 1001), Fraction(7, 3), Fraction(1), Fraction(6)])
@pytest.mark.parametrize('n', [4, 5, 9, 23, 60])
def test_every_window_has_an_output_and_counts_sum(r, n):
    counts = [len(R.window_outputs(k, r, last=k == n - 4)) for k in range(n - 3)]
    assert min(counts) >= 1 and max(counts) <= R.max_instants(r) + 1
    assert sum(counts) == R.n_output_frames(n, r)
    assert all(len(R.instants(k, r)) <= R.max_instants(r) for k in range(n - 3))


@pytest.mark.parametrize('r', [Fraction(5, 2), Fraction(12, 5), Fraction(7, 3), Fraction(1), Fraction(4)])
@pytest.mark.parametrize('world', [2, 3])
def test_rank_blocks_tile_the_file(r, world):
    n, hl, p = 17, 37, y4m.payload_size(70, 98)
    nw = n - 3
    seq = [i for k in range(nw) for i, _, _ in R.window_outputs(k, r, last=k == nw - 1)]
    pos = hl
    for rank in range(world):
        lo, hi = shard_windows(nw, world, rank)
        assert R.block_offset(hl, lo, r, p) == pos
        mine = [i for k in range(lo, hi) for i, _, _ in R.window_outputs(k, r, last=k == nw - 1)]
        assert mine == seq[R.first_output(lo, r):R.first_output(lo, r) + len(mine)]
        pos += len(mine) * (6 + p)
    assert pos == y4m.frame_offset(hl, R.n_output_frames(n, r), p)


def test_block_offset_of_integer_ratio_is_the_x_m_offset():
    for m in (2, 5, 8):
        for lo in range(6):
            assert R.block_offset(40, lo, m, 100) == y4m.frame_offset(40, y4m.output_index(lo, 0, m), 100)


# ---- default n_ctx ---------------------------------------------------------------------------------------------------------
def test_padded_slots():
    assert [R.padded_slots(Fraction(5, 2), d) for d in (1, 2, 3)] == [0, 0, 2]
    assert [R.padded_slots(Fraction(12, 5), d) for d in (1, 2, 3)] == [0, 1, 4]


@pytest.mark.parametrize('r,limit,exp', [
    (Fraction(5, 2), 8, 2),          # 2 instants per window: no padding at 2
    (Fraction(5, 2), 1, 1),          # only n_ctx = 1 fits
    (Fraction(12, 5), 8, 1),         # 2, 2, 3, 2, 2 instants: only 1 never pads
    (Fraction(8), 8, 7),             # x8: one chunk of 7
    (Fraction(8), 6, 1),             # 7 instants: 1 is the only size <= 6 without padding
    (Fraction(16), 8, 5),            # x16: 15 = 3 x 5
    (Fraction(4), 8, 3),
    (Fraction(1), 8, 1),
])
def test_default_n_ctx(r, limit, exp):
    assert R.default_n_ctx(r, lambda d: d <= limit) == exp
