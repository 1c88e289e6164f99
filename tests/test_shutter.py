"""The synthesized shutter without a GPU: ``demfi_amd.shutter`` (parameters, groups against a brute-force ``Fraction`` timeline, ``mix_np``
against exact rational rounding, ``filter_plan`` over the plans of ``retime`` and ``scene``, the multiplier of the kernel's division over
its whole input range), the rules of ``pipeline.EdgeSpec`` and of the command line."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import shutter as SH
from demfi_amd.pipeline import EdgeSpec
from demfi_amd.y4m_edge import plan_batch, plan_fine

RATIOS = [Fraction(1), Fraction(2), Fraction(5, 2), Fraction(8), Fraction(60000, 1001) / Fraction(24000, 1001)]
SD = [(1, 1), (2, 4), (4, 8), (3, 3)]


# ---- parameters --------------------------------------------------------------------------------------------------------------------
def test_check_params_accepts_and_refuses():
    assert SH.check_params(180, 4) == (4, 8) and SH.check_params(360) == (4, 4) and SH.check_params(90, 4) == (4, 16)
    assert SH.check_params('180', 2) == (2, 4) and SH.check_params('1/1', 1) == (1, 360) and SH.check_params(Fraction(360, 7), 1) == (1, 7)
    assert SH.check_params('1440/11', 4) == (4, 11) and SH.MAX_SAMPLES == 32 and SH.check_params(360, 32) == (32, 32)
    with pytest.raises(ValueError, match=r'sample counts up to 32 that work for this angle: none'):
        SH.check_params(172, 4)
    with pytest.raises(ValueError, match=r'not an integer; sample counts up to 32 that work for this angle: 3, 6, 9, .*30$'):
        SH.check_params(270, 4)
    assert SH.workable_samples(270) == list(range(3, 33, 3)) and SH.check_params(270, 3) == (3, 4)
    for angle in (0, 361, '0', '-5', '180.0', 'wide', '1/0', 180.0, True):
        with pytest.raises(ValueError, match='shutter angle'):
            SH.check_params(angle, 4)
    for s in (0, 33, 2.0, '4', True):
        with pytest.raises(ValueError, match='samples must be an integer in 1 .. 32'):
            SH.check_params(180, s)


def test_the_fine_ratio_is_refused_above_the_largest_ratio():
    assert SH.fine_ratio(Fraction(5, 2), 8) == 20 and SH.fine_ratio(8, 8) == R.MAX_RATIO
    with pytest.raises(ValueError, match='more than 64'):
        SH.fine_ratio(1, SH.check_params('1/1', 1)[1])
    with pytest.raises(ValueError, match='5/2 x 32 = 80 times'):
        SH.fine_ratio(Fraction(5, 2), 32)


# ---- groups ------------------------------------------------------------------------------------------------------------------------
def _times(n, r, full):
    """The exact times of the stream at ratio r over n input frames: tau_i = (0 | 1) + i / r while it lies on the timeline."""
    out, i = [], 0
    if full:
        while n >= 1 and Fraction(i) / r < n:
            out.append(Fraction(i) / r)
            i += 1
    else:
        while n >= 4 and 1 + Fraction(i) / r <= n - 2:
            out.append(1 + Fraction(i) / r)
            i += 1
    return out


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', RATIOS, ids=str)
def test_groups_against_a_brute_force_timeline(r, full):
    truncated = 0
    for n in range(1, 10):
        coarse = _times(n, r, full)
        assert len(coarse) == R.n_output_frames(n, r, full)
        for s, d in SD:
            fine = _times(n, r * d, full)
            assert len(fine) == R.n_output_frames(n, r * d, full)
            got = SH.groups(len(fine), len(coarse), s, d)
            assert len(got) == len(coarse)
            step = Fraction(1) / (r * d)                                 # the exposure is S steps of the fine stream from tau_c on
            for c, (tau, ks) in enumerate(zip(coarse, got)):
                want = [g for g, t in enumerate(fine) if tau <= t < tau + s * step]
                assert ks == want and ks[0] == c * d and fine[ks[0]] == tau, (n, s, d, c)
                truncated += len(ks) < s
            if coarse:
                assert got[-1] == list(range((len(coarse) - 1) * d, min((len(coarse) - 1) * d + s, len(fine))))
    # the tail groups lose samples: always on the reference timeline (the last written frame sits on the timeline's end), on the full-length
    # one when n r is not an integer (with an integer r the last group ends at n r D - D + S - 1 < n r D)
    assert (truncated > 0) == (not full or r.denominator > 1)


def test_groups_stop_at_a_scene_change():
    scene = lambda g: int(g >= 6)                                        # noqa: E731
    assert SH.groups(12, 3, 3, 4, scene) == [[0, 1, 2], [4, 5], [8, 9, 10]]
    assert SH.groups(12, 3, 3, 4) == [[0, 1, 2], [4, 5, 6], [8, 9, 10]]
    assert SH.groups(10, 3, 4, 4, lambda g: g == 5) == [[0, 1, 2, 3], [4, 6, 7], [8, 9]]      # only the scene of sample 0 counts
    with pytest.raises(ValueError, match='needs fine frame 8 of 8'):
        SH.groups(8, 3, 2, 4)


# ---- mix_np ------------------------------------------------------------------------------------------------------------------------
def _round_half_up(q):
    return math.floor(q + Fraction(1, 2))


@pytest.mark.parametrize('es', [1, 2], ids=['bytes', '16-bit'])
def test_mix_np_against_exact_rational_rounding(es):
    peak = 255 if es == 1 else 65535
    rng = np.random.default_rng(es)
    special = [0, 1, peak // 2, peak // 2 + 1, peak - 1, peak]
    for k in range(1, 33):
        cols = [[v] * k for v in special]                                # a constant group gives the constant back
        cols += [[0] * (k - j) + [1] * j for j in range(k + 1)]          # every sum 0 .. k over k: the ties of even k among them
        cols += [[peak] * (k - j) + [peak - 1] * j for j in range(k + 1)]
        cols += [list(rng.integers(0, peak + 1, k)) for _ in range(8)]
        x = np.array(cols, dtype='<u2' if es == 2 else np.uint8).T      # [k, P]
        pay = np.ascontiguousarray(x).view(np.uint8).reshape(k, -1)
        got = SH.mix_np(pay, [list(range(k))], es)
        assert got.dtype == np.uint8 and got.shape == (1, pay.shape[1])
        got = got.view('<u2' if es == 2 else np.uint8)[0]
        want = [_round_half_up(Fraction(sum(int(v) for v in col), k)) for col in cols]
        assert got.tolist() == want, k
        if k % 2 == 0:                                                   # k/2 ones among k samples: exactly one half, rounded up
            assert got[len(special) + k // 2] == 1 and got[len(special) + k // 2 - 1] == 0
    pay = rng.integers(0, 256, (5, 8), dtype=np.uint8)
    out = SH.mix_np(pay, [[0], [1, 3], [4, 2, 0]], 1)                    # groups pick rows; one row is itself
    assert out[0].tolist() == pay[0].tolist() and out[1].tolist() == ((pay[1].astype(int) + pay[3] + 1) // 2).tolist()
    with pytest.raises(ValueError):
        SH.mix_np(pay, [[]], 1)
    with pytest.raises(ValueError):
        SH.mix_np(pay, [[0]], 3)


def test_the_multiplier_of_the_kernel_is_exact_over_its_whole_range():
    """(n * magic(k)) >> 32 == n // (2 k) for n = 2 sum + k, every k in 1 .. 32 and every sum in 0 .. k * 65535."""
    for k in range(1, SH.MAX_SAMPLES + 1):
        m = SH.magic(k)
        assert 0 < m < 1 << 32 and m == (1 << 32) // (2 * k) + 1
        n = 2 * np.arange(k * 65535 + 1, dtype=np.uint64) + np.uint64(k)
        assert int(n[-1]) < 1 << 22
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(2 * k)), k


# ---- filter_plan -------------------------------------------------------------------------------------------------------------------
CUTS = {'none': [], 'start': [1], 'middle': [4], 'end': [7], 'adjacent': [3, 4], 'start and end': [1, 2, 7]}
N = 8


def _plans(r, d, full, cuts):
    """Per window of an N-frame clip at the fine ratio r d: (k, runs, outs) of ``scene.window_runs`` (no cuts: ``retime.window_plan``)."""
    k0, nw = R.first_window(N, full), R.n_windows(N, full)
    is_cut = S.with_sentinels(lambda j: j in cuts, N) if full else (lambda j: j in cuts)
    for k in range(k0, k0 + nw):
        last = k == k0 + nw - 1
        if cuts:
            yield (k,) + S.window_runs(k, r * d, last, is_cut, full)
        else:
            ts, o = R.window_plan(k, r * d, last, full)
            yield k, [(None, ts)], [(i, 0, kind, j) for i, kind, j in o]


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('cuts', sorted(CUTS))
@pytest.mark.parametrize('r', [Fraction(1), Fraction(2), Fraction(5, 2)], ids=str)
def test_filter_plan_keeps_what_the_written_frames_need(r, cuts, full):
    for s, d in [(1, 4), (2, 4), (4, 8), (3, 4), (1, 2)]:
        seen = []
        for k, runs, outs in _plans(r, d, full, CUTS[cuts]):
            before = ([(tup, list(ts)) for tup, ts in runs], list(outs))
            fr, fo = SH.filter_plan(runs, outs, s, d)
            assert (runs, outs) == before                                              # pure
            assert [i for i, _, _, _ in fo] == [i for i, _, _, _ in outs if i % d < s] and fo
            seen += [i for i, _, _, _ in fo]
            old = {i: (runs[run][0], kind, runs[run][1][j]) for i, run, kind, j in outs}
            for i, run, kind, j in fo:                                                 # the same tuple, kind and instant as before
                assert (fr[run][0], kind) == old[i][:2] and (kind != R.ST or fr[run][1][j] == old[i][2])
                assert kind == R.ST or j == 0
            assert sorted({run for _, run, _, _ in fo}) == list(range(len(fr)))       # dense, none without outputs
            for ri, (tup, ts) in enumerate(fr):
                st = {old[i][2] for i, run, kind, _ in fo if run == ri and kind == R.ST}
                first = [rts for rtup, rts in runs if rtup == tup and set(ts) <= set(rts)][0][0]
                keeps_first = any(run == ri and kind != R.ST for _, run, kind, _ in fo)
                assert ts == sorted(st | ({first} if keeps_first else set())), (k, ri)  # the distinct kept t, and the first for S0 / S1
                assert len(ts) == len(st) or (keeps_first and ts[0] == first)
        n_fine = R.n_output_frames(N, r * d, full)
        assert seen == [i for i in range(n_fine) if i % d < s]                         # exactly the existing i with i mod D < S


@pytest.mark.parametrize('cuts', sorted(CUTS))
def test_filter_plan_with_s_equal_d_returns_the_plan(cuts):
    for r, d in [(Fraction(1), 1), (Fraction(5, 2), 3), (Fraction(2), 4)]:
        for _, runs, outs in _plans(r, d, True, CUTS[cuts]):
            fr, fo = SH.filter_plan(runs, outs, d, d)
            assert fr is runs and fo is outs
    with pytest.raises(ValueError):
        SH.filter_plan([], [], 3, 2)


def test_a_window_is_never_left_empty_and_half_the_instants_go_at_180_degrees():
    for r in RATIOS:
        for s, d in [(2, 4), (4, 8), (1, 8)]:
            if r * d > R.MAX_RATIO:
                continue
            plain = kept = 0
            for k in range(0, 12):
                ts, o = R.window_plan(k, r * d)
                fr, fo = SH.filter_plan([(None, ts)], [(i, 0, kind, j) for i, kind, j in o], s, d)
                assert fo and len(fr) == 1
                plain, kept = plain + len(ts), kept + len(fr[0][1])
            assert kept <= plain * s / d + 12                               # at most the first instant of every window on top
            assert SH.period_counts(r, s, d)[:1] == [len(SH.filter_plan([(None, R.window_plan(0, r * d)[0])],
                                                                         [(i, 0, kind, j) for i, kind, j in R.window_plan(0, r * d)[1]], s, d)[0][0][1])]
    assert SH.period_counts(Fraction(5, 2), 4, 8)[:2] == [11, 8]             # 24 -> 60 at 180 degrees: r S = 10 instants per window


# ---- the stage's bookkeeping: any batch size closes the same groups ----------------------------------------------------------------
@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('cuts', ['none', 'middle', 'adjacent', 'end'])
def test_batches_of_any_size_close_the_groups_of_the_definition(cuts, full):
    for r, (s, d) in [(Fraction(2), (2, 4)), (Fraction(1), (3, 4)), (Fraction(5, 2), (4, 8)), (Fraction(5, 2), (3, 3)), (Fraction(2), (1, 4))]:
        fine_r, lead = r * d, s - 1
        k0, nw = R.first_window(N, full), R.n_windows(N, full)
        spec = EdgeSpec(y4m=True, cuts=bool(CUTS[cuts]), full=full, shutter=(s, d))
        det = SimpleNamespace(is_cut=lambda j: j in CUTS[cuts]) if CUTS[cuts] else None
        wins = [S.runner_order((k, k + 1, k + 2, k + 3)) for k in range(k0, k0 + nw)]
        slot = {f: f for f in range(-4, N + 4)}
        scene_of, sc = {}, 0                                             # the definition: the scene of every fine frame of the stream
        for k, runs, outs in _plans(r, d, full, CUTS[cuts]):
            for i, run, _, _ in outs:
                scene_of[i] = sc + (run if len(runs) > 1 else 0)
            sc += len(runs) - 1
        n_fine, n_out = R.n_output_frames(N, fine_r, full), R.n_output_frames(N, r, full)
        assert sorted(scene_of) == list(range(n_fine))
        want = SH.groups(n_fine, n_out, s, d, scene_of.get)
        for batch in (1, 2, 3, 4, nw):
            closed, per_window, still_open, scene, at = [], [], [], 0, {}
            for b0 in range(0, nw, batch):
                bw = wins[b0:b0 + batch]
                plan = plan_fine(spec, fine_r, bw, b0, lambda j: k0 + j, lambda j: j == nw - 1, det, None, [list(w) for w in bw], slot)
                fine, ends = plan[4], plan[5]
                m = len(still_open)                                      # the carry: the open samples move in front of the gather
                assert m <= lead and [rw for _, _, rw in still_open] == list(range(still_open[0][2], still_open[0][2] + m) if m else [])
                at = {lead - m + j: at[rw] for j, (_, _, rw) in enumerate(still_open)}
                still_open = [(g, c, lead - m + j) for j, (g, c, _) in enumerate(still_open)]
                for j, g in enumerate(g for _, e in fine for g, _ in e):
                    at[lead + j] = g
                assert len(at) <= lead + sum(len(o) for o in plan[1])
                table, counts, still_open, scene = SH.close_groups(still_open, fine, scene, ends, s, d, lead)
                assert ends == (b0 + batch >= nw) and len(counts) == len(bw)
                closed += [[at[rw] for rw in rows] for rows in table]
                per_window += counts
            assert closed == want and not still_open, (r, s, d, batch)
            assert sum(per_window) == n_out and len(per_window) == nw
            done = 0                                                     # a written frame is handed out once its last sample has run
            for w, c in enumerate(per_window):
                for grp in want[done:done + c]:
                    last = min(grp[0] + s, n_fine) - 1
                    assert R.first_output(k0 + w, fine_r, full) <= last or w == 0
                    assert w == nw - 1 or last < R.first_output(k0 + w + 1, fine_r, full)
                done += c
    with pytest.raises(RuntimeError, match='got the fine frames'):
        SH.close_groups([], [(False, [(0, False), (2, False)])], 0, False, 3, 4, 2)


def test_the_batched_plan_is_sized_by_the_instants_that_run():
    """24 -> 60 at 180 degrees runs 11 and 8 instants in alternate windows: nothing but 1 divides both, and an eighth of padding buys 4."""
    from demfi_amd.runner import choose_config
    fits = lambda d: True                                                # noqa: E731
    counts = SH.period_counts(Fraction(5, 2), 4, 8)
    assert counts[:2] == [11, 8] and R.default_n_ctx(Fraction(20), fits, counts=counts) == 1
    assert R.default_n_ctx(Fraction(20), fits, counts=counts, slack=Fraction(1, 8)) == 4
    assert R.default_n_ctx(Fraction(8), fits, counts=SH.period_counts(Fraction(2), 2, 4), slack=Fraction(1, 8)) == 3      # pads nothing
    for r in (Fraction(2), Fraction(5, 2), Fraction(8), Fraction(11), Fraction(5, 3)):      # one sample of the whole period: the plain choice
        assert R.default_n_ctx(r, fits, counts=SH.period_counts(r, 1, 1), slack=Fraction(1, 8)) == R.default_n_ctx(r, fits)
        assert R.default_n_ctx(r, fits, slack=0) == min(range(1, 9), key=lambda d: (R.padded_slots(r, d), -d))
    kw = dict(env={}, cached=None, total_memory=288 * 10 ** 9, free_memory=lambda: 0, workspace_bytes=lambda *a: 10 ** 9)
    cfg = choose_config(736, 1280, 3, 8, 0, True, None, None, False, Fraction(20), instant_counts=counts, **kw)
    assert (cfg['n_ctx'], cfg['n_trunk'], cfg['batched']) == (4, 3, True)
    assert choose_config(736, 1280, 3, 8, 0, True, None, None, False, Fraction(20), **kw)['n_ctx'] == R.default_n_ctx(Fraction(20), fits)


# ---- the edge's rules --------------------------------------------------------------------------------------------------------------
def _yuv(**kw):
    return SimpleNamespace(matrix=0, full_range=False, siting=0, with_s1=lambda k: False, **kw)


def test_edge_spec_defaults_are_unchanged_and_the_shutter_keys_the_pipeline():
    assert EdgeSpec() == (False, False, False, 8, '420', None, None, 'bob') and EdgeSpec().shutter is None
    assert EdgeSpec.of(_yuv()).shutter is None and EdgeSpec.of(_yuv()) == EdgeSpec(y4m=True) and EdgeSpec.of(None).shutter is None
    a = EdgeSpec.of(_yuv(shutter=(4, 8)))
    assert a.shutter == (4, 8) and a == EdgeSpec(y4m=True, shutter=[4, 8]) and hash(a) == hash(EdgeSpec(y4m=True, shutter=(4, 8)))
    assert a != EdgeSpec(y4m=True) and EdgeSpec(y4m=True) != a and a != EdgeSpec(y4m=True, shutter=(2, 4)) and a != tuple(a)
    assert len({(4, a), (4, EdgeSpec(y4m=True)), (4, EdgeSpec.of(_yuv(shutter=(4, 8))))}) == 2
    assert a._replace(cuts=True).shutter == (4, 8) and a._replace(shutter=None) == EdgeSpec(y4m=True)
    assert EdgeSpec(y4m=True)._replace(shutter=(2, 4)).shutter == (2, 4) and 'shutter=(4, 8)' in repr(a)


Y = EdgeSpec(y4m=True, shutter=(2, 4))
REFUSED = {
    'without a retimed runner': (Y, (False, False, True), 'a shutter needs the Y4M edge on a retimed runner'),
    'with repeated frames': (Y._replace(dedup=(768, 320, Fraction(33, 100), 3)), (True, True, True), 'a shutter does not go with repeated frames'),
    'more samples than steps': (Y._replace(shutter=(5, 4)), (True, False, True), 'shutter must be None or'),
    'too many samples': (Y._replace(shutter=(33, 66)), (True, False, True), 'shutter must be None or'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_check_refuses(case):
    spec, args, why = REFUSED[case]
    with pytest.raises(ValueError, match=why):
        spec.check(*args)


def test_check_accepts_a_shutter_with_everything_else():
    assert Y.check(True, False, True) is None and Y.check(True, False, False) is None
    assert Y._replace(cuts=True, full=True, depth=10, layout='mono', fields='t', deint_mode='adaptive').check(True, True, True) is None


def test_plan_fine_filters_both_paths_and_plan_batch_is_its_head():
    slot = {f: 100 + f for f in range(-1, 16)}
    wins = [(k + 1, k + 2, k, k + 3) for k in range(4)]
    frames = [[slot[x] for x in w] for w in wins]
    det = SimpleNamespace(is_cut=lambda j: j == 3)
    for spec, d in ((EdgeSpec(y4m=True, shutter=(2, 4)), None), (EdgeSpec(y4m=True, cuts=True, shutter=(2, 4)), det)):
        args = (Fraction(8), wins, 0, None, lambda j: j == 3, d, None, frames, slot)
        runs, outs, cw, st, fine, ends = plan_fine(spec, *args)
        assert plan_batch(spec, *args) == (runs, outs, cw, st) and ends and cw == (1 if d else 0)
        plain = plan_fine(spec._replace(shutter=None), *args)
        assert [i for _, e in fine for i, _ in e] == [i for _, e in plain[4] for i, _ in e if i % 4 < 2]
        assert sum(len(ts) for _, ts, _ in runs) < sum(len(ts) for _, ts, _ in plain[0])
        assert [c for c, _ in fine] == [c for c, _ in plain[4]] == ([False, True, False, False] if d else [False] * 4)
        if d:                                        # window 1 is the cut window: its second half belongs to the next scene
            assert [right for _, right in plain[4][1][1]] == [False] * 4 + [True] * 4
            assert [(i, right) for i, right in fine[1][1]] == [(8, False), (9, False), (12, True), (13, True)]
    assert plan_fine(EdgeSpec(y4m=True), Fraction(2), wins[:1], 0, None, lambda j: False, None, None, frames, slot)[5] is False


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_the_switches_of_the_command_line():
    from demfi_amd import video
    a = video.parser().parse_args(['in.y4m', 'out.y4m', '--shutter', '180', '--shutter-samples', '2'])
    assert (a.shutter, a.shutter_samples) == (180, 2) and video.check_shutter(a.shutter, a.shutter_samples) == (2, 4)
    a = video.parser().parse_args(['in.y4m', 'out.y4m', '--shutter', '1440/11'])
    assert a.shutter == Fraction(1440, 11) and a.shutter_samples is None and video.check_shutter(a.shutter, None) == (4, 11)
    assert video.parser().parse_args(['in.y4m', 'out.y4m']).shutter is None and video.check_shutter(None, None) is None
    with pytest.raises(SystemExit):
        video.parser().parse_args(['in.y4m', 'out.y4m', '--shutter', '400'])
    for given in (8, 4):                             # the default's own value too: the switch was given
        with pytest.raises(ValueError, match='--shutter-samples .* says how --shutter works'):
            video.check_shutter(None, given)
    with pytest.raises(SystemExit):
        video.main(['in.y4m', 'out.y4m', '--shutter-samples', '4'])
    with pytest.raises(ValueError, match='--shutter does not go with --dedup'):
        video.check_shutter(180, 4, dedup=True)
    with pytest.raises(ValueError, match='shutter with 2 ranks'):
        video.check_shutter(180, 4, world=2)
    with pytest.raises(SystemExit):                  # main refuses before anything is loaded
        video.main(['in.y4m', 'out.y4m', '--shutter-samples', '8'])
    with pytest.raises(SystemExit):
        video.main(['in.y4m', 'out.y4m', '--shutter', '180', '--dedup'])


def test_video_runner_refuses_before_a_library_is_loaded(tmp_path):
    from demfi_amd import video
    with pytest.raises(ValueError, match='does not go with --dedup'):
        video.VideoRunner(None, shutter=180, dedup=True)
    for given in (8, 4):
        with pytest.raises(ValueError, match='says how --shutter works'):
            video.VideoRunner(None, shutter_samples=given)
    with pytest.raises(ValueError, match='not an integer'):
        video.VideoRunner(None, shutter=172)
    vr = video.VideoRunner(None, mfi=2, shutter=180)
    assert vr.shutter == (4, 8) and vr.last_shutter is None and video.VideoRunner(None).shutter is None
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n' + (b'FRAME\n' + bytes(96 * 64 * 3 // 2)) * 5)
    with pytest.raises(ValueError, match='shutter with 2 ranks'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'), world=2, rank=0)
    far = video.VideoRunner(None, mfi=2, shutter='1/1', shutter_samples=1)             # D = 360: refused once the header is known
    with pytest.raises(ValueError, match='more than 64'):
        far.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert not (tmp_path / 'out.y4m').exists()
    import io
    with pytest.raises(ValueError, match='more than 64'):
        far.run_stream(io.BytesIO(src.read_bytes()), io.BytesIO())


def test_every_one_rank_switch_is_refused_with_two_ranks_before_anything_is_allocated(tmp_path):
    from demfi_amd import video
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n' + (b'FRAME\n' + bytes(96 * 64 * 3 // 2)) * 5)
    assert list(video.ONE_RANK) == ['dedup', 'ivtc', 'shutter', 'interlace']
    for kw, what in ((dict(dedup=True), 'dedup with 2 ranks.*one rank'), (dict(ivtc=True), 'ivtc with 2 ranks.*one rank'),
                     (dict(shutter=180), 'shutter with 2 ranks'), (dict(interlace='tff'), 'interlace with 2 ranks')):
        with pytest.raises(ValueError, match=what):
            video.VideoRunner(None, mfi=2, **kw).run_file(str(src), str(tmp_path / 'out.y4m'), world=2, rank=1)     # no model: nothing ran
        with pytest.raises(ValueError, match=what):
            video.check_one_rank(2, **kw)
        video.check_one_rank(1, **kw)
        video.check_one_rank(2, **{k: None for k in kw})
    video.check_one_rank(2, dedup=False, ivtc=False)
    assert not (tmp_path / 'out.y4m').exists()


def test_the_counter_table_names_counters_the_runner_has_and_attributes_the_video_runner_has():
    import ast
    import inspect
    import textwrap

    from demfi_amd import video
    from demfi_amd.runner import WindowRunner
    init = ast.parse(textwrap.dedent(inspect.getsource(WindowRunner.__init__)))
    zeroed = {t.attr for node in ast.walk(init) if isinstance(node, ast.Assign) and isinstance(node.value, ast.Constant) and node.value.value == 0
              for t in node.targets if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == 'self'}
    assert set(video.COUNTERS) <= zeroed and len(video.COUNTERS) == 9
    vr = video.VideoRunner(None)
    kept = [attr for attr in video.COUNTERS.values() if attr is not None]
    assert len(kept) == len(set(kept)) == 6 and all(attr.startswith('last_') and getattr(vr, attr) == 0 for attr in kept)
    assert vr.last_instants == (0, 0) and vr.last_st_frames == 0
    vr = video.VideoRunner(None, mfi=2, shutter=180, interlace='bff')
    vr._counted(SimpleNamespace(w=96, h=64, layout='420'), {name: i + 1 for i, name in enumerate(video.COUNTERS)}, [3], 7)
    assert vr.last_instants == (1, 2) and vr.last_st_frames == 3 and vr.last_cuts == [3] and vr.last_cut_windows == 4
    assert (vr.last_shutter_carried, vr.last_interlace_carried, vr.last_scale_payloads, vr.last_depth_promoted, vr.last_depth_requantised) == (5, 6, 7, 8, 9)
    assert (vr.last_shutter, vr.last_interlace, vr.last_scale) == ((4, 8), 'b', None)
