"""The host side of the clip edge without a GPU: ``pipeline.EdgeSpec`` (defaults, hashing, every refusal), ``y4m_edge.plan_batch``
against the three planners it composes, and ``pipeline.residency_order``."""
from fractions import Fraction
from types import SimpleNamespace

import pytest

from demfi_amd import cadence as K
from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd.pipeline import EdgeSpec, deint_conflict, residency_order
from demfi_amd.y4m_edge import egress_layout, plan_batch


# ---- EdgeSpec.of -----------------------------------------------------------------------------------------------------------------
def _yuv(**kw):
    return SimpleNamespace(matrix=0, full_range=False, siting=0, with_s1=lambda k: False, **kw)


def test_of_defaults_and_hashing():
    bgr = EdgeSpec.of(None)
    assert bgr == EdgeSpec() and not bgr.y4m and bgr == (False, False, False, 8, '420', None, None, 'bob')
    plain = EdgeSpec.of(_yuv())
    assert plain == EdgeSpec(y4m=True) and plain == (True, False, False, 8, '420', None, None, 'bob') and plain != bgr
    assert EdgeSpec.of(_yuv(deint_mode='adaptive')) == plain                        # no fields: the mode says nothing
    assert EdgeSpec.of(_yuv(fields=None, deint_mode='adaptive')).deint_mode == 'bob'
    assert EdgeSpec.of(_yuv(fields='t', deint_mode='adaptive')).deint_mode == 'adaptive'
    assert EdgeSpec.of(_yuv(fields='t')) == EdgeSpec.of(_yuv(fields='t', deint_mode='bob'))
    assert EdgeSpec.of(_yuv(scene_cut=None)) == plain and EdgeSpec.of(_yuv(scene_cut=10.0)).cuts is True
    assert EdgeSpec.of(_yuv(depth='10')).depth == 10 and EdgeSpec.of(_yuv(full_length=1)).full is True
    d = [768, 320, Fraction(33, 100), 3]
    a, b = EdgeSpec.of(_yuv(dedup=d)), EdgeSpec.of(_yuv(dedup=tuple(d)))
    assert a == b and hash(a) == hash(b) and isinstance(a.dedup, tuple)
    assert len({bgr, plain, a, b, EdgeSpec.of(_yuv())}) == 3
    assert {(4, plain): 1}[(4, EdgeSpec.of(_yuv()))] == 1 and (4, plain) != (2, plain)     # the pipeline's cache key


def test_every_field_changes_equality():
    base = EdgeSpec.of(_yuv(fields='t'))
    other = dict(y4m=False, cuts=True, full=True, depth=10, layout='444', dedup=(768, 320, Fraction(33, 100), 3), fields='b',
                 deint_mode='adaptive')
    assert set(other) == set(EdgeSpec._fields)
    for name, value in other.items():
        changed = base._replace(**{name: value})
        assert changed != base and hash((4, changed)) != hash((4, base)), name
    assert EdgeSpec.of(_yuv(dedup=(768, 320, Fraction(33, 100), 3))) != EdgeSpec.of(_yuv(dedup=(768, 320, Fraction(33, 100), 4)))


# ---- EdgeSpec.check --------------------------------------------------------------------------------------------------------------
DEDUP = (768, 320, Fraction(33, 100), 3)
Y = EdgeSpec(y4m=True)
REFUSED = {
    'depth without Y4M': (EdgeSpec(depth=10), (False, False, True), "Y4M edge .* only"),
    'dedup without Y4M': (EdgeSpec(dedup=DEDUP), (False, True, True), "Y4M edge .* only"),
    'fields without Y4M': (EdgeSpec(fields='t'), (False, False, True), "Y4M edge .* only"),
    'adaptive with dedup': (Y._replace(fields='t', deint_mode='adaptive', dedup=DEDUP), (True, True, True), "deint_mode 'adaptive' with fields='t', dedup=\\("),
    'adaptive without reuse_frames': (Y._replace(fields='t', deint_mode='adaptive'), (True, True, False), "needs reuse_frames"),
    'adaptive without fields': (Y._replace(deint_mode='adaptive'), (True, True, True), "deint_mode 'adaptive' with fields=None"),
    'an unknown mode': (Y._replace(fields='t', deint_mode='yadif'), (True, True, True), "deint_mode 'yadif' with"),
    'an unknown field order': (Y._replace(fields='x'), (True, True, True), "fields must be None, 't' or 'b'"),
    'dedup without a retimed runner': (Y._replace(dedup=DEDUP), (False, True, True), "repeated frames need"),
    'dedup without window_index': (Y._replace(dedup=DEDUP), (True, False, True), "repeated frames need"),
    'dedup without reuse_frames': (Y._replace(dedup=DEDUP), (True, True, False), "repeated frames need"),
    'cuts without a retimed runner': (Y._replace(cuts=True), (False, False, True), "scene cuts need"),
    'cuts without reuse_frames': (Y._replace(cuts=True), (True, False, False), "scene cuts need"),
    'full-length without a retimed runner': (Y._replace(full=True), (False, True, True), "full-length timeline needs"),
    'full-length without window_index': (Y._replace(full=True), (True, False, True), "full-length timeline needs"),
    'a retimed runner with the BGR spec': (EdgeSpec(), (True, False, True), "a retimed runner needs the Y4M edge"),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_check_refuses(case):
    spec, args, why = REFUSED[case]                                       # each rule on its own: nothing else refuses the case first
    with pytest.raises(ValueError, match=why):
        spec.check(*args)


def test_check_accepts_what_runs_today():
    for reuse in (True, False):                                          # the BGR edge, and the plain Y4M edge on either runner
        assert EdgeSpec().check(False, False, reuse) is None
        for retimed in (True, False):
            assert Y.check(retimed, False, reuse) is None and Y._replace(depth=10, layout='422').check(retimed, False, reuse) is None
            assert Y._replace(fields='b').check(retimed, False, reuse) is None
    assert Y._replace(cuts=True).check(True, False, True) is None
    assert Y._replace(full=True).check(True, True, False) is None
    assert Y._replace(dedup=DEDUP, cuts=True, full=True, fields='t').check(True, True, True) is None
    assert Y._replace(fields='t', deint_mode='adaptive', cuts=True, full=True, depth=10).check(True, True, True) is None


def test_deint_conflict_is_the_rule_of_the_command_line():
    from demfi_amd import video
    assert deint_conflict('adaptive', True, False) is None and deint_conflict('bob', False, True) is None
    for args, why, msg in (((True, 'yadif', None), 'mode', 'one of bob, adaptive'), ((False, 'adaptive', None), 'fields', 'needs --deinterlace'),
                           ((True, 'adaptive', True), 'dedup', '--deinterlace-mode bob')):
        deinterlace, mode, dedup = args
        assert deint_conflict(mode, deinterlace, bool(dedup)) == why
        with pytest.raises(ValueError, match='deint_mode'):
            Y._replace(fields='t' if deinterlace else None, deint_mode=mode, dedup=DEDUP if dedup else None).check(True, True, True)
        with pytest.raises(ValueError, match=msg):
            video.check_deinterlace_mode(*args)
    assert video.check_deinterlace_mode(True, 'adaptive', False) is None and video.check_deinterlace_mode(False, 'bob', True) is None


# ---- plan_batch ------------------------------------------------------------------------------------------------------------------
SLOT = {f: 100 + 3 * f for f in range(-1, 16)}                           # frame (or kept index) -> slot


def _wins(ks):
    return [(k + 1, k + 2, k, k + 3) for k in ks]                        # runner order (B0, B1, B-1, B2) of the unclamped tuples


def _check_plan(got, per_window, cut_windows, st_frames):
    """``got`` of plan_batch against ``per_window`` = the planner's (runs as (tuple in runner order, instants), outs as (run, kind,
    instant index)) of every window."""
    runs, outs, cw, st = got
    assert (cw, st) == (cut_windows, st_frames) and len(outs) == len(per_window)
    base = 0
    for w, (pr, po) in enumerate(per_window):
        mine = runs[base:base + len(pr)]
        assert [(fr, ts) for fr, ts, _ in mine] == [([SLOT[x] for x in tup], ts) for tup, ts in pr], w
        assert outs[w] == [(base + run, kind, j) for run, kind, j in po], w       # offset by the runs before this window
        base += len(pr)
    assert base == len(runs)
    for ri, (_, _, kinds) in enumerate(runs):                            # exactly the kinds the outputs name
        assert kinds == {kind for o in outs for run, kind, _ in o if run == ri}, ri


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', [Fraction(2), Fraction(5, 2)], ids=str)
def test_plan_batch_without_a_detector_is_retime(r, full):
    ks, n0 = [3, 4, 5], 7                                                # windows 3 .. 5 are windows 7 .. 9 of the sequence
    wins, spec = _wins(ks), EdgeSpec(y4m=True, full=full)
    frames = [[SLOT[x] for x in win] for win in wins]

    def with_s1(j):
        return j == n0 + 2
    per = []
    for wi, k in enumerate(ks):
        ts, o = R.window_plan(k, r, wi == 2, full)
        per.append(([(wins[wi], ts)], [(0, kind, j) for _, kind, j in o]))
    for index in (None, lambda j: j - n0 + ks[0]):
        got = plan_batch(spec, r, wins, n0, index, with_s1, None, None, frames, SLOT)
        _check_plan(got, per, 0, 0)
    assert len(got[0]) == 3 and (R.S1 in got[0][2][2]) == bool(full or (ks[2] + 1) * r % 1 == 0)


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', [Fraction(2), Fraction(5, 2)], ids=str)
def test_plan_batch_with_a_detector_is_scene(r, full):
    ks, cut = [2, 3, 4, 5], 6                                            # a cut before frame 6: window 4 is the cut window
    det = SimpleNamespace(is_cut=lambda j: j == cut)
    wins, spec = _wins(ks), EdgeSpec(y4m=True, cuts=True, full=full)
    per = []
    for wi, k in enumerate(ks):
        last = wi == 3
        is_cut = S.with_sentinels(det.is_cut, k + 3 if last else None) if full else det.is_cut
        sr, so = S.window_runs(k, r, last, is_cut, full)
        per.append(([(S.runner_order(tup), ts) for tup, ts in sr], [(run, kind, j) for _, run, kind, j in so]))
    assert [len(pr) for pr, _ in per] == [1, 1, 2, 1]                    # a cut window is two runs
    got = plan_batch(spec, r, wins, 0, None, lambda j: j == 3, det, None, None, SLOT)
    _check_plan(got, per, 1, 0)
    assert len(got[0]) == 5 and got[1][3][0][0] == 4                     # the window after the cut window starts at run 4


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', [Fraction(2), Fraction(5, 2)], ids=str)
def test_plan_batch_over_kept_frames_is_cadence(r, full):
    kept = SimpleNamespace(s=[0, 1, 2, 4, 5, 6, 7], n=8)                 # input frame 3 repeats frame 2: one hold
    ks = [0, 1, 2, 3]
    wins = [S.runner_order(K.window_tuple(k, kept.s, kept.n)) for k in ks]
    spec = EdgeSpec(y4m=True, full=full, dedup=DEDUP)
    for det, cuts in ((None, 0), (SimpleNamespace(is_cut=lambda j: j == 4), 1)):
        is_cut = det.is_cut if det is not None else None
        per, st = [], 0
        for k in ks:
            sr, so = K.window_runs(k, r, kept.s, kept.n, is_cut, full)
            per.append(([(S.runner_order(tup), ts) for tup, ts in sr], [(run, kind, j) for _, run, kind, j in so]))
            st += sum(kind == R.ST for _, _, kind, _ in so)
        got = plan_batch(spec._replace(cuts=det is not None), r, wins, 5, lambda j: j - 5, lambda j: False, det, kept, None, SLOT)
        _check_plan(got, per, cuts, st)
        assert st > 0
    held = K.window_runs(1, r, kept.s, kept.n, None, full)[0]            # the window over the hold spans two input frames
    assert len(held) == 2 and sum(len(ts) for _, ts in held) > R.max_instants(r)


# ---- residency_order -------------------------------------------------------------------------------------------------------------
def test_residency_order():
    wins = [(6, 7, 5, 8), (7, 8, 6, 9)]
    got = list(residency_order((4,), wins, [3, 10, 11]))
    assert [idx for _, idx in got] == [3, 4, 6, 7, 5, 8, 7, 8, 6, 9, 10, 11]
    assert [wi for wi, _ in got] == [None, None, 0, 0, 0, 0, 1, 1, 1, 1, None, None]
    assert list(residency_order((), wins, [])) == [(0, 6), (0, 7), (0, 5), (0, 8), (1, 7), (1, 8), (1, 6), (1, 9)]
    assert [idx for _, idx in residency_order((), wins, [3, 4, 10])] == [3, 4, 6, 7, 5, 8, 7, 8, 6, 9, 10]   # lookbehind, windows, lookahead


# ---- egress_layout: the buffer rule of the stages behind the gather ----------------------------------------------------------------
_G0, _G1 = ('gather', 0, 9, 10368, 48, 72), ('gather', 1, 9, 10368, 48, 72)
_LAYOUTS = {        # (shutter, scale, interlace, requant) -> the buffers as (producer, free rows in front, rows, payload bytes, h, w), then the host's
    (0, 0, 0, 0): [_G0, (9, 10368)],
    (0, 0, 0, 1): [_G0, ('requant', 0, 9, 5184, 48, 72), (9, 5184)],
    (0, 0, 1, 0): [_G1, ('weave', 0, 5, 10368, 48, 72), (5, 10368)],
    (0, 0, 1, 1): [_G1, ('weave', 0, 5, 10368, 48, 72), ('requant', 0, 5, 5184, 48, 72), (5, 5184)],
    (0, 1, 0, 0): [_G0, ('scale', 0, 9, 18432, 64, 96), (9, 18432)],
    (0, 1, 0, 1): [_G0, ('scale', 0, 9, 18432, 64, 96), ('requant', 0, 9, 9216, 64, 96), (9, 9216)],
    (0, 1, 1, 0): [_G0, ('scale', 1, 9, 18432, 64, 96), ('weave', 0, 5, 18432, 64, 96), (5, 18432)],
    (0, 1, 1, 1): [_G0, ('scale', 1, 9, 18432, 64, 96), ('weave', 0, 5, 18432, 64, 96), ('requant', 0, 5, 9216, 64, 96), (5, 9216)],
    (1, 0, 0, 0): [_G1, ('mix', 0, 8, 10368, 48, 72), (8, 10368)],
    (1, 0, 0, 1): [_G1, ('mix', 0, 8, 10368, 48, 72), ('requant', 0, 8, 5184, 48, 72), (8, 5184)],
    (1, 0, 1, 0): [_G1, ('mix', 1, 8, 10368, 48, 72), ('weave', 0, 5, 10368, 48, 72), (5, 10368)],
    (1, 0, 1, 1): [_G1, ('mix', 1, 8, 10368, 48, 72), ('weave', 0, 5, 10368, 48, 72), ('requant', 0, 5, 5184, 48, 72), (5, 5184)],
    (1, 1, 0, 0): [_G1, ('mix', 0, 8, 10368, 48, 72), ('scale', 0, 8, 18432, 64, 96), (8, 18432)],
    (1, 1, 0, 1): [_G1, ('mix', 0, 8, 10368, 48, 72), ('scale', 0, 8, 18432, 64, 96), ('requant', 0, 8, 9216, 64, 96), (8, 9216)],
    (1, 1, 1, 0): [_G1, ('mix', 0, 8, 10368, 48, 72), ('scale', 1, 8, 18432, 64, 96), ('weave', 0, 5, 18432, 64, 96), (5, 18432)],
    (1, 1, 1, 1): [_G1, ('mix', 0, 8, 10368, 48, 72), ('scale', 1, 8, 18432, 64, 96), ('weave', 0, 5, 18432, 64, 96),
                   ('requant', 0, 5, 9216, 64, 96), (5, 9216)],
}


def _egress_spec(sh, sc, il, rq, scale=(96, 64, 'lanczos3')):
    return EdgeSpec(y4m=True, depth=10, shutter=(2, 4) if sh else None, scale=scale if sc else None,
                    interlace=('t', 'linear') if il else None, depths=(10, 10, 8, 'bayer') if rq else None)


@pytest.mark.parametrize('which', sorted(_LAYOUTS))
def test_egress_layout_every_subset_of_the_stages(which):
    """9 payloads a batch of 4 windows, 72x48 4:2:0 at a working depth of 10: 10368 bytes a payload, 18432 resized to 96x64, 9216 of those at
    8 bits.  A buffer has its producer's rows plus its consumer's lead (shutter (2, 4): 1, weave: 1) in front; the host takes the last one's."""
    assert egress_layout(_egress_spec(*which), 9, 4, 48, 72) == _LAYOUTS[which]


def test_egress_layout_the_runs_own_size_builds_no_scaler():
    for which in sorted(_LAYOUTS):
        if which[1]:
            same = egress_layout(_egress_spec(*which, scale=(72, 48, 'bicubic')), 9, 4, 48, 72)
            assert same == _LAYOUTS[(which[0], 0) + which[2:]] and 'scale' not in [b[0] for b in same[:-1]]
