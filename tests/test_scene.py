"""CPU tests of scene-cut detection (``demfi_amd.scene``, ``python -m demfi_amd.video --scene-cut``): scores and cuts from the
SAD definition, the clamped tuples and the runs of cut windows for the layouts that stress them, the output mapping of cut
windows for x M and 24 -> 60, unchanged frame counts, the extra frame of a rank block and the command line."""
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import video


def _cuts(*js):
    c = set(js)
    return lambda j: j in c


# ---- scores and cuts -------------------------------------------------------------------------------------------------------
def test_sad_np_is_exact():
    a = np.array([0, 255, 10, 200, 7], np.uint8)
    b = np.array([255, 0, 20, 100, 7], np.uint8)
    assert S.sad_np(a, b) == 255 + 255 + 10 + 100 == S.sad_np(b, a)
    big = np.zeros(4096 * 4096 * 3 // 2, np.uint8)
    assert S.sad_np(big, big + 255) == 255 * big.size > 2 ** 32
    with pytest.raises(ValueError):
        S.sad_np(a, b[:4])


def test_scores_use_the_previous_mafd():
    """A steady change of 20 % per frame is motion, not a cut: only its first step (against mafd_0 = 0) scores 20, the next ones
    score |20 - 20| = 0.  Then every byte flips (mafd 100): score min(100, |100 - 20|) = 80."""
    P = 100
    fr = [np.where(np.arange(P) < 20 * j, 255, 0).astype(np.uint8) for j in range(5)]   # 20 more bytes flip per frame
    fr.append(255 - fr[-1])
    sads = [S.sad_np(fr[j], fr[j - 1]) for j in range(1, len(fr))]
    assert sads[:4] == [20 * 255] * 4
    m = [S.mafd(s, P) for s in sads]
    assert m[:4] == [20.0] * 4
    sc = S.scores(sads, P)
    assert sc[:4] == [20.0, 0.0, 0.0, 0.0]
    assert m[4] == 100.0 and sc[4] == 80.0
    assert S.cuts_of(sads, P, 10.0) == [1, 5]
    assert S.cuts_of(sads, P, 20.0) == [1, 5] and S.cuts_of(sads, P, 20.000001) == [5]


def test_detector_matches_the_whole_stream_definition():
    g = np.random.RandomState(3)
    P = 37
    sads = [int(x) for x in g.randint(0, 255 * P, 60)]
    sads[10] = sads[30] = 0
    for T in (5.0, 10.0, 30.0, 100.0):
        d = S.Detector(P, T)
        for j, s in enumerate(sads, 1):
            d.push(j, s)
        assert d.cuts == S.cuts_of(sads, P, T)
        assert all(d.is_cut(j) == (j in d.cuts) for j in range(1, 61))
    with pytest.raises(RuntimeError):
        d.is_cut(61)                                                  # not scored yet
    with pytest.raises(RuntimeError):
        S.Detector(P, 10.0).push(2, 0)                                # SADs arrive in frame order


def test_a_rank_block_needs_frame_lo_minus_1():
    """A block starting at window lo >= 1 reads from frame lo - 1: SAD_lo gives mafd_lo, on which score_{lo+1} depends; from there
    on its cuts are the one-rank cuts.  Without frame lo - 1 the cut at lo + 1 below would be missed."""
    P = 10
    sads = [0, 0, 255 * 3, 255 * 8, 255 * 8, 0, 0, 255 * 5, 0, 0, 0]          # SAD_1 .. SAD_11
    whole = S.cuts_of(sads, P, 10.0)
    assert whole == [3, 4, 8]                                                  # score_4 = min(80, 50) = 50
    for lo in range(0, 9):
        first = S.first_frame(lo)
        assert first == max(lo - 1, 0)
        d = S.Detector(P, 10.0, first=first)
        for j in range(first + 1, 12):
            d.push(j, sads[j - 1])
        assert [j for j in d.cuts if j >= lo + 1] == [j for j in whole if j >= lo + 1], lo
    late = S.Detector(P, 10.0, first=3)                                        # lo = 3 read from frame 3: mafd_3 unknown
    for j in range(4, 12):
        late.push(j, sads[j - 1])
    assert late.cuts == [8]                                                    # the cut before frame 4 is missed


# ---- clamped tuples and cut runs -------------------------------------------------------------------------------------------
def _layout(n, cuts):
    """(inner tuple or (left, right)) of every window of an n-frame stream."""
    is_cut = _cuts(*cuts)
    return [S.cut_runs(k, is_cut) if S.is_cut_window(k, is_cut) else S.inner_tuple(k, is_cut) for k in range(n - 3)]


def test_no_cut_gives_the_plain_tuples():
    assert _layout(8, []) == [(k, k + 1, k + 2, k + 3) for k in range(5)]


def test_cut_at_frame_1():
    assert _layout(8, [1]) == [(1, 1, 2, 3), (1, 2, 3, 4), (2, 3, 4, 5), (3, 4, 5, 6), (4, 5, 6, 7)]


def test_cut_at_the_last_frame():
    assert _layout(8, [7]) == [(0, 1, 2, 3), (1, 2, 3, 4), (2, 3, 4, 5), (3, 4, 5, 6), (4, 5, 6, 6)]


def test_cut_in_the_middle():
    lay = _layout(10, [5])
    assert lay[1] == (1, 2, 3, 4)
    assert lay[2] == (2, 3, 4, 4)                                      # B2 clamped
    assert lay[3] == ((3, 4, 4, 4), (5, 5, 5, 6))                      # the cut window: left, right
    assert lay[4] == (5, 5, 6, 7)                                      # B-1 clamped
    assert lay[5] == (5, 6, 7, 8)


def test_consecutive_cuts_one_frame_scene():
    lay = _layout(10, [4, 5])                                           # frame 4 is a scene of its own
    assert lay[0] == (0, 1, 2, 3)
    assert lay[1] == (1, 2, 3, 3)
    assert lay[2] == ((2, 3, 3, 3), (4, 4, 4, 4))
    assert lay[3] == ((4, 4, 4, 4), (5, 5, 5, 6))
    assert lay[4] == (5, 5, 6, 7)
    assert lay[5] == (5, 6, 7, 8)


def test_a_cut_before_every_frame():
    n = 9
    lay = _layout(n, range(1, n))
    for k, (left, right) in enumerate(lay):
        b = k + 1
        assert left == (b, b, b, b) and right == (b + 1,) * 4


def test_runner_order():
    assert S.runner_order((0, 1, 2, 3)) == (1, 2, 0, 3)


# ---- what a window runs and writes ------------------------------------------------------------------------------------------
def test_inner_windows_run_the_window_plan():
    for r in (Fraction(4), Fraction(5, 2), Fraction(1)):
        for k in range(6):
            runs, outs = S.window_runs(k, r, k == 5, _cuts(1, 20))
            ts, plan = R.window_plan(k, r, k == 5)
            assert [ts for _, ts in runs] == [ts]
            assert outs == [(i, 0, kind, j) for i, kind, j in plan]


def test_cut_window_x4_half_goes_right_and_last_s1():
    """x 4, cut before frame 4 (window 2 is the cut window): S0 and t = 1/4 hold B0 (left's S0); t = 1/2 and 3/4 hold B1 (right's
    S1), and so does S1 when the window is the last."""
    r = Fraction(4)
    runs, outs = S.window_runs(2, r, False, _cuts(4))
    assert runs == [((2, 3, 3, 3), [0.5]), ((4, 4, 4, 5), [0.5])]
    assert outs == [(8, 0, R.S0, 0), (9, 0, R.S0, 0), (10, 1, R.S1, 0), (11, 1, R.S1, 0)]
    runs, outs = S.window_runs(2, r, True, _cuts(4))
    assert runs[1] == ((4, 4, 4, 5), [0.5])
    assert outs[-1] == (12, 1, R.S1, 0) and len(outs) == 5


def test_cut_window_24_to_60():
    r = Fraction(5, 2)
    # window 0 owns i = 0 (S0), 1 (fraction 2/5), 2 (4/5); window 1: 3 (1/5), 4 (3/5); window 2: 5 (S0), 6 (2/5), 7 (4/5)
    assert S.window_runs(0, r, False, _cuts(2))[1] == [(0, 0, R.S0, 0), (1, 0, R.S0, 0), (2, 1, R.S1, 0)]
    assert S.window_runs(1, r, False, _cuts(3))[1] == [(3, 0, R.S0, 0), (4, 1, R.S1, 0)]
    runs, outs = S.window_runs(2, r, True, _cuts(4))
    assert outs == [(5, 0, R.S0, 0), (6, 0, R.S0, 0), (7, 1, R.S1, 0)]   # (k+1) r = 7.5: no S1 of its own
    runs, outs = S.window_runs(3, r, True, _cuts(5))
    assert outs == [(8, 0, R.S0, 0), (9, 1, R.S1, 0), (10, 1, R.S1, 0)]   # 1/5, 3/5, then the last S1


def test_half_is_decided_on_the_exact_fraction():
    """Output 16 of window 0 at r = (2^25 + 1) / 2^20 sits at 2^24 / (2^25 + 1), just below 1/2; its float32 t is 0.5.  It holds
    B0."""
    r = Fraction(2 ** 25 + 1, 2 ** 20)
    outs = R.window_outputs(0, r)
    assert outs[16] == (16, R.ST, 0.5) and Fraction(16) / r < Fraction(1, 2)
    assert outs[17][2] > 0.5
    got = S.window_runs(0, r, False, _cuts(2))[1]
    assert got[16] == (16, 0, R.S0, 0) and got[17] == (17, 1, R.S1, 0)


@pytest.mark.parametrize('r', [Fraction(4), Fraction(8), Fraction(5, 2), Fraction(60, 25), Fraction(1)])
@pytest.mark.parametrize('cuts', [(), (1,), (4, 5), (9,), tuple(range(1, 10))])
def test_frame_counts_and_positions_are_unchanged(r, cuts):
    n = 10
    is_cut = _cuts(*cuts)
    got = []
    for k in range(n - 3):
        runs, outs = S.window_runs(k, r, k == n - 4, is_cut)
        assert len(runs) == (2 if S.is_cut_window(k, is_cut) else 1)
        assert [i for i, _, _, _ in outs] == [i for i, _, _ in R.window_outputs(k, r, k == n - 4)]
        for _, run, kind, j in outs:
            assert run < len(runs) and j < len(runs[run][1])
        got += [i for i, _, _, _ in outs]
    assert got == list(range(R.n_output_frames(n, r)))


# ---- command line --------------------------------------------------------------------------------------------------------
def test_cli_scene_cut_parsing():
    p = video.parser()
    assert p.parse_args(['-', '-']).scene_cut is None
    assert p.parse_args(['-', '-', '--scene-cut']).scene_cut == 10.0
    assert p.parse_args(['-', '-', '--scene-cut', '25']).scene_cut == 25.0
    assert p.parse_args(['-', '-', '--scene-cut', '100', '--fps', '60']).scene_cut == 100.0
    assert p.parse_args(['-', '-', '--mfi', '4', '--scene-cut']).scene_cut == 10.0


@pytest.mark.parametrize('t', ['0', '-1', '100.5', '1000', 'nan', 'abc'])
def test_cli_scene_cut_refused(t):
    with pytest.raises(SystemExit) as e:
        video.main(['-', '-', '--scene-cut', t])
    assert e.value.code == 2


@pytest.mark.parametrize('t', [0, -5, 101, float('nan')])
def test_video_runner_refuses_a_bad_threshold(t):
    with pytest.raises(ValueError):
        video.VideoRunner(None, 1, scene_cut=t)
