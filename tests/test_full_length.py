"""CPU tests of the full-length timeline of the Y4M path (``python -m demfi_amd.video --full-length``): the window outputs tile
0 .. ceil(n r) - 1 for every short and long clip, the tuples clamp at both ends, the x M windows are the default ones shifted by
one input frame, rank blocks tile the file, the clip's ends work as scene cuts, the streaming reader hands out the windows, and
the command line."""
import io
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import video, y4m
from demfi_amd.clip import ClipRunner

RATIOS = [Fraction(1), Fraction(2), Fraction(8), Fraction(5, 2), Fraction(12, 5), Fraction(7, 3), Fraction(64)]


def _windows(n):
    k0 = R.first_window(n, True)
    return list(range(k0, k0 + R.n_windows(n, True)))


def _no_cuts(j):
    return False


# ---- the schedule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', RATIOS, ids=str)
@pytest.mark.parametrize('n', range(1, 13))
def test_windows_tile_the_whole_timeline(n, r):
    ks = _windows(n)
    assert ks[0] == (-1 if n >= 2 else -2) and ks[-1] == n - 3
    seen = []
    for k in ks:
        last = k == ks[-1]
        outs = R.window_outputs(k, r, last, full_length=True)
        assert outs and outs[0][0] == R.first_output(k, r, True)
        for i, kind, t in outs:
            tau = Fraction(i) / r
            assert 0 <= tau < n
            if kind == R.S0:
                assert tau == k + 1
            elif kind == R.ST:
                assert k + 1 < tau < k + 2 <= n - 1
                assert t == R.float32_of(tau - (k + 1)) and t == float(np.float32(t))
            else:
                assert last and n - 1 <= tau < n
        assert R.instants(k, r, True) == (sorted({t for _, kind, t in outs if kind == R.ST}) or [0.5])
        ts, plan = R.window_plan(k, r, last, full_length=True)
        assert [(i, kind) for i, kind, _ in plan] == [(i, kind) for i, kind, _ in outs]
        assert all(ts[j] == t for (_, kind, j), (_, _, t) in zip(plan, outs) if kind == R.ST)
        seen += [i for i, _, _ in outs]
    assert R.n_output_frames(n, r, True) == math.ceil(n * r)
    assert seen == list(range(math.ceil(n * r)))


def test_x_m_gives_n_m_frames_and_short_clips_have_output():
    for n in range(1, 10):
        assert R.n_output_frames(n, 8, True) == 8 * n
        assert R.n_output_frames(n, Fraction(5, 2), True) == math.ceil(n * Fraction(5, 2))
    assert R.n_output_frames(0, 8, True) == 0 and R.n_windows(0, True) == 0


def test_one_frame_clip_holds_frame_0():
    for r in RATIOS:
        ts, plan = R.window_plan(-2, r, True, full_length=True)
        assert ts == [0.5]
        assert plan == [(i, R.S1, 0) for i in range(math.ceil(r))]
    assert S.clip_tuple(-2, S.with_sentinels(_no_cuts, 1)) == (0, 0, 0, 0)


def test_24_to_60_full_length():
    r = Fraction(5, 2)
    w = {k: R.window_outputs(k, r, k == 1, True) for k in (-1, 0, 1)}                   # n = 4: windows -1, 0, 1
    assert [(i, kind, None if t is None else round(t, 6)) for i, kind, t in w[-1]] == [(0, 'S0', None), (1, 'St', 0.4), (2, 'St', 0.8)]
    assert [(i, kind) for i, kind, _ in w[0]] == [(3, 'St'), (4, 'St')]
    assert [(i, kind) for i, kind, _ in w[1]] == [(5, 'S0'), (6, 'St'), (7, 'St'), (8, 'S1'), (9, 'S1')]   # tau 3.2, 3.6 hold S1


@pytest.mark.parametrize('n', range(1, 13))
def test_tuples_clamp_at_both_ends(n):
    ends = S.with_sentinels(_no_cuts, n)
    for k in _windows(n):
        exp = tuple(min(max(x, 0), n - 1) for x in (k, k + 1, k + 2, k + 3))
        assert S.clip_tuple(k, ends) == exp
        runs, _ = S.window_runs(k, Fraction(5, 2), k == n - 3, ends, True)
        assert runs == [(exp, R.instants(k, Fraction(5, 2), True))]
    if n >= 4:
        assert S.clip_tuple(-1, ends) == (0, 0, 1, 2) and S.clip_tuple(n - 3, ends) == (n - 3, n - 2, n - 1, n - 1)


@pytest.mark.parametrize('m', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [4, 5, 9])
def test_integer_ratio_is_the_default_stream_shifted(n, m):
    """Windows 0 .. n-4 write what they write by default, m frames later; the default final S1 is the full-length last window's."""
    for k in range(n - 3):
        full = R.window_outputs(k, m, False, True)
        dflt = R.window_outputs(k, m, False)
        assert full == [(i + m, kind, t) for i, kind, t in dflt]
        assert R.window_plan(k, m, False, True)[0] == R.window_plan(k, m)[0]
    dflt_s1 = R.window_outputs(n - 4, m, True)[-1]
    assert dflt_s1[1] == R.S1 and (dflt_s1[0] + m, R.S0, None) == R.window_outputs(n - 3, m, True, True)[0]


def test_default_mode_is_unchanged():
    for r in RATIOS:
        for k in range(5):
            assert R.window_outputs(k, r, k == 4) == R.window_outputs(k, r, k == 4, False)
        assert R.n_output_frames(9, r) == math.floor(6 * r) + 1
        assert R.first_window(9) == 0 and R.n_windows(9) == 6


# ---- rank blocks ----------------------------------------------------------------------------------------------------------
def _my_windows(n, world, rank, full_length=True):
    return ClipRunner.my_windows(SimpleNamespace(world=world, rank=rank), n, full_length)


@pytest.mark.parametrize('r', [Fraction(8), Fraction(5, 2), Fraction(12, 5), Fraction(1)], ids=str)
@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 17])
def test_rank_blocks_tile_the_file(n, world, r):
    hl, p = 37, y4m.payload_size(70, 98)
    ends = S.with_sentinels(_no_cuts, n)
    ks = _windows(n)
    pos, got = hl, []
    for rank in range(world):
        lo, wins = _my_windows(n, world, rank)
        if not wins:
            continue
        assert wins == [S.runner_order(S.clip_tuple(k, ends)) for k in range(lo, lo + len(wins))]
        assert R.block_offset(hl, lo, r, p, True) == pos
        mine = [i for k in range(lo, lo + len(wins)) for i, _, _ in R.window_outputs(k, r, k == ks[-1], True)]
        got += list(range(lo, lo + len(wins)))
        pos += len(mine) * (6 + p)
    assert got == ks
    assert pos == y4m.frame_offset(hl, R.n_output_frames(n, r, True), p)


def test_default_rank_blocks_are_unchanged():
    for world in (1, 2, 3):
        for rank in range(world):
            lo, wins = _my_windows(11, world, rank, False)
            assert wins and lo == wins[0][2] and all(w == (k + 1, k + 2, k, k + 3) for k, w in enumerate(wins, lo))


# ---- the clip's ends as scene cuts ------------------------------------------------------------------------------------------
def test_sentinels_and_real_cuts_next_to_both_ends():
    """n = 8, real cuts before frames 1 and 7 = n-1: window -1 and window 5 = n-3 are cut windows; their neighbours clamp."""
    n, r = 8, Fraction(4)
    cut = S.with_sentinels(lambda j: j in (1, n - 1), n)
    runs = {k: S.window_runs(k, r, k == n - 3, cut, True) for k in _windows(n)}
    assert runs[-1][0] == [((0, 0, 0, 0), [0.5]), ((1, 1, 1, 2), [0.5])]
    assert runs[-1][1] == [(0, 0, R.S0, 0), (1, 0, R.S0, 0), (2, 1, R.S1, 0), (3, 1, R.S1, 0)]
    assert [tup for tup, _ in runs[0][0]] == [(1, 1, 2, 3)]
    assert [tup for tup, _ in runs[3][0]] == [(3, 4, 5, 6)]
    assert [tup for tup, _ in runs[4][0]] == [(4, 5, 6, 6)]
    assert runs[5][0] == [((5, 6, 6, 6), [0.5]), ((7, 7, 7, 7), [0.5])]
    assert runs[5][1] == [(24, 0, R.S0, 0), (25, 0, R.S0, 0)] + [(i, 1, R.S1, 0) for i in range(26, 32)]
    got = [i for k in _windows(n) for i, _, _, _ in runs[k][1]]
    assert got == list(range(R.n_output_frames(n, r, True)))


@pytest.mark.parametrize('n', [2, 3])
def test_short_clips_with_a_cut(n):
    cut = S.with_sentinels(lambda j: j == 1, n)
    runs, outs = S.window_runs(-1, Fraction(2), n == 2, cut, True)
    assert runs == [((0, 0, 0, 0), [0.5]), ((1, 1, 1, n - 1), [0.5])]
    assert [(i, run, kind) for i, run, kind, _ in outs][:2] == [(0, 0, R.S0), (1, 1, R.S1)]


def test_a_block_from_window_minus_1_reads_from_frame_0():
    assert S.first_frame(-1) == S.first_frame(-2) == S.first_frame(0) == 0 and S.first_frame(3) == 2


# ---- streaming reader -----------------------------------------------------------------------------------------------------
def _reader(n, h=4, w=6):
    p = y4m.payload_size(h, w)
    data = b'YUV4MPEG2 W%d H%d F24:1 Ip\n' % (w, h) + b''.join(b'FRAME\n' + bytes([j]) * p for j in range(n))
    return y4m.Reader(io.BytesIO(data))


@pytest.mark.parametrize('n', range(0, 12))
def test_frames_hand_out_the_clamped_windows(n):
    fr = y4m.Frames(_reader(n), pinned=False, full_length=True)
    got = []
    for win in fr.windows():
        k = fr.first_window + len(got)
        got.append((k, win, fr.is_last(k)))
        assert all(int(fr[j][0]) == j for j in win)
    ends = S.with_sentinels(_no_cuts, n)
    assert got == [(k, S.runner_order(S.clip_tuple(k, ends)), k == n - 3) for k in _windows(n)]
    assert fr.peak <= 5


def test_frames_default_windows_are_unchanged():
    fr = y4m.Frames(_reader(7), pinned=False)
    assert list(fr.windows()) == [(k + 1, k + 2, k, k + 3) for k in range(4)]
    assert fr.first_window == 0 and fr.is_last(3) and not fr.is_last(2)


# ---- VideoRunner and the command line --------------------------------------------------------------------------------------
def test_video_runner_full_length_counts():
    hdr = y4m.parse_header(b'YUV4MPEG2 W80 H48 F24:1 Ip')
    vr = video.VideoRunner(None, 1, 4, full_length=True)
    assert vr.full_length and vr._ratio(hdr) == 4 and vr._n_out(9, hdr) == 36 and vr._n_out(1, hdr) == 4
    assert vr._out_header(hdr).encode() == video.VideoRunner(None, 1, 4)._out_header(hdr).encode()
    vr = video.VideoRunner(None, 1, fps=Fraction(60), full_length=True)
    assert vr._n_out(9, hdr) == 23 and vr._n_out(0, hdr) == 0
    dflt = video.VideoRunner(None, 1, 4)
    assert not dflt.full_length and dflt._ratio(hdr) == 4 and dflt._n_out(9, hdr) == 25      # x M is r = M on every path


@pytest.mark.parametrize('argv', [['--mfi', '4'], ['--fps', '60000/1001'], ['--scene-cut'], ['--fps', '60', '--scene-cut', '20'], []])
def test_cli_full_length(argv):
    p = video.parser()
    assert p.parse_args(['-', '-'] + argv).full_length is False
    a = p.parse_args(['-', '-', '--full-length'] + argv)
    assert a.full_length is True
    assert p.parse_args(['-', '-'] + argv + ['--full-length']).full_length is True
