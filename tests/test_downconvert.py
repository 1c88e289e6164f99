"""An output rate below the input's (``--downconvert``, r = F_out / F_in < 1) on the host: the timeline of ``demfi_amd.retime`` for r < 1
against the same timeline at the ratio r D >= 1 (today's code, the reference: output i of r is output i D of r D), windows that own no
output, the schedules and buffer sizes that count them, scene cuts, the shutter's plan at a fine ratio below D, the refusals and the
headers.  Nothing here needs a GPU."""
import io
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import shutter as SH
from demfi_amd import video, y4m
from demfi_amd.pipeline import EdgeSpec
from demfi_amd.y4m_edge import egress_layout, plan_fine

RATIOS = [Fraction(5, 6), Fraction(5, 12), Fraction(1, 2), Fraction(1, 3), Fraction(1001, 1200), Fraction(1, 64)]
TIMELINES = pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])


def _windows(n, full):
    k0 = R.first_window(n, full)
    return list(range(k0, k0 + R.n_windows(n, full)))


def _stream(n, r, full):
    """[(window, kind, t)] of every output of an n-frame clip at the ratio r in stream order, and the outputs per window."""
    ks, out, per = _windows(n, full), [], {}
    for k in ks:
        outs = R.window_outputs(k, r, k == ks[-1], full)
        per[k] = outs
        assert [i for i, _, _ in outs] == list(range(len(out), len(out) + len(outs)))     # 0 .. N_out - 1 once each, in order
        out += [(k, kind, t) for _, kind, t in outs]
    assert len(out) == R.n_output_frames(n, r, full)
    return out, per


def _multipliers(r):
    return sorted({2, 3, math.ceil(1 / r)})           # and the smallest D with r D >= 1


@TIMELINES
@pytest.mark.parametrize('r', RATIOS, ids=str)
def test_the_timeline_is_the_decimated_timeline_of_a_ratio_that_runs_today(r, full):
    for n in range(1, 14):
        got, per = _stream(n, r, full)
        for D in _multipliers(r):
            ref, _ = _stream(n, r * D, full)
            assert len(ref) > (len(got) - 1) * D if got else True
            assert got == ref[::D][:len(got)], (n, D)  # by (window, kind, float32 t), exactly
        for k in _windows(n, full):
            last = k == _windows(n, full)[-1]
            ts, plan = R.window_plan(k, r, last, full)
            assert ts == R.instants(k, r, full, last) and len(ts) <= R.max_instants(r) == 1
            if not per[k]:
                assert ts == [] and plan == []         # a window that owns nothing has no instants
            elif all(kind != R.ST for _, kind, _ in per[k]):
                assert ts == [0.5]                     # S0 / S1 only: t = 1/2, as for r >= 1
            else:
                assert ts == sorted({t for _, kind, t in per[k] if kind == R.ST})
            assert [(i, kind) for i, kind, _ in plan] == [(i, kind) for i, kind, _ in per[k]] and all(j < len(ts) for _, _, j in plan)


def test_half_rate_runs_the_even_windows_only():
    for n in range(4, 14):
        got, per = _stream(n, Fraction(1, 2), False)
        ks = _windows(n, False)
        ran = [k for k in ks if R.instants(k, Fraction(1, 2), last=k == ks[-1])]
        s1 = (n - 3) % 2 == 0                         # tau = n - 2 is an output: the last window's S1
        assert ran == sorted({k for k in ks if k % 2 == 0} | ({ks[-1]} if s1 else set()))
        assert [kind for _, kind, _ in got] == [R.S0] * (len(got) - s1) + [R.S1] * s1
        assert all(R.instants(k, Fraction(1, 2), last=k == ks[-1]) == [0.5] for k in ran)


def test_ratio():
    with pytest.raises(ValueError, match='only F_out >= F_in'):
        R.ratio(60, 30)
    with pytest.raises(ValueError, match='only F_out >= F_in'):
        R.ratio(60, 30, down=False)
    assert R.ratio(60, 30, down=True) == Fraction(1, 2) and R.ratio(Fraction(60000, 1001), 50, True) == Fraction(1001, 1200)
    assert R.ratio(64, 1, True) == Fraction(1, 64) and R.ratio(24, 60, True) == Fraction(5, 2) == R.ratio(24, 60)
    for down in (False, True):
        with pytest.raises(ValueError):
            R.ratio(65, 1, down)
        with pytest.raises(ValueError, match='more than 64'):
            R.ratio(1, 65, down)
    with pytest.raises(ValueError, match='1/64'):
        R.ratio(Fraction(6401, 100), 1, True)


def test_schedules_count_zero_for_windows_that_own_nothing():
    assert R._period_counts(Fraction(1, 2)) == [1, 0] and R._period_counts(Fraction(1, 3)) == [1, 0, 0]
    assert R._period_counts(Fraction(5, 6)) == [1, 1, 1, 1, 1, 0] and sum(R._period_counts(Fraction(5, 12))) == 5
    assert R._period_counts(Fraction(5, 2)) == [2, 2] and R._period_counts(Fraction(1)) == [1]     # r >= 1: as before (S0 alone: t = 1/2)
    for r in RATIOS:
        counts = R._period_counts(r)
        assert set(counts) <= {0, 1} and sum(counts) == (r.numerator if r.denominator <= R.SCAN_WINDOWS else sum(counts))
        assert R.padded_slots(r, 1) == 0 and R.padded_slots(r, 4) == 3 * sum(counts)
        assert R.default_n_ctx(r, lambda d: True) == 1                   # nothing to batch: a window runs one instant at most
    # the shutter's filtered schedule: 60 -> 24 at 180 degrees (S, D) = (4, 8), R = 16/5; 60 -> 6 at 360 of two, R = 1/5
    counts = SH.period_counts(Fraction(2, 5), 4, 8)
    ref = []
    for k in range(len(counts)):
        kept = [(i, kind, t) for i, kind, t in R.window_outputs(k, Fraction(16, 5)) if i % 8 < 4]
        ref.append(len({t for _, kind, t in kept if kind == R.ST}) or (1 if kept else 0))
    assert counts == ref and 0 in counts and max(counts) >= 2
    counts = SH.period_counts(Fraction(1, 10), 2, 2)
    assert len(counts) == 10 and sum(counts) == 2 and set(counts) == {0, 1}
    assert R.default_n_ctx(Fraction(16, 5), lambda d: True, counts=SH.period_counts(Fraction(2, 5), 4, 8), slack=Fraction(1, 8)) >= 1


# ---- egress_layout -------------------------------------------------------------------------------------------------------------------
def _layout_by_the_rule(spec, nout, batch, h, w):
    """The buffer rule of ``y4m_edge`` written out again: rows of every producer, the lead of its consumer in front."""
    es = 2 if spec.depth > 8 else 1
    rows, chain = nout, [['gather', nout, y4m.payload_size(h, w, spec.layout) * es, h, w]]
    leads = []
    if spec.shutter is not None:
        leads.append(spec.shutter[0] - 1)
        rows = nout // spec.shutter[1] + batch + 2
        chain.append(['mix', rows, chain[-1][2], h, w])
    if spec.scale is not None and tuple(spec.scale[:2]) != (w, h):
        leads.append(0)
        w, h = spec.scale[:2]
        chain.append(['scale', rows, y4m.payload_size(h, w, spec.layout) * es, h, w])
    if spec.interlace is not None:
        leads.append(1)
        rows = rows // 2 + 1
        chain.append(['weave', rows, chain[-1][2], h, w])
    if spec.depths is not None and spec.depths[2] < spec.depths[1]:
        leads.append(0)
        chain.append(['requant', rows, y4m.payload_size(h, w, spec.layout) * (2 if spec.depths[2] > 8 else 1), h, w])
    leads.append(0)
    return [(c[0], lead, *c[1:]) for c, lead in zip(chain, leads)] + [tuple(chain[-1][1:3])]


def _spec(sh, sc, il, rq, shutter=(2, 4)):
    return EdgeSpec(y4m=True, depth=10, shutter=shutter if sh else None, scale=(96, 64, 'lanczos3') if sc else None,
                    interlace=('t', 'linear') if il else None, depths=(10, 10, 8, 'bayer') if rq else None)


def test_egress_layout_is_unchanged_for_ratios_of_one_and_above():
    for which in [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]:
        got = egress_layout(_spec(*which), 9, 4, 48, 72)                 # the case tests/test_edge_spec.py pins: J = 2, batch 4
        assert [tuple(b) for b in got] == _layout_by_the_rule(_spec(*which), 9, 4, 48, 72), which
    assert egress_layout(_spec(1, 0, 0, 0), 9, 4, 48, 72)[1][:3] == ('mix', 0, 8)


@TIMELINES
@pytest.mark.parametrize('r,shutter', [(Fraction(5, 12), None), (Fraction(1, 3), None), (Fraction(5, 6), None), (Fraction(2, 5), (4, 8)),
                                       (Fraction(1, 10), (2, 2)), (Fraction(5, 6), (2, 2))], ids=str)
def test_egress_layout_bounds_a_plan_walk_below_one(r, shutter, full):
    """Three periods of the schedule, in batches of 1, 3 and 4 windows: the gather's payloads fit ``nout`` and every stage's fit its rows."""
    from demfi_amd import interlace as IL
    fine = r * shutter[1] if shutter else r
    n = 3 * fine.denominator * (shutter[1] if shutter else 1) + 3
    n = min(n, 80)
    ks = _windows(n, full)
    wins = [S.runner_order((k, k + 1, k + 2, k + 3)) for k in ks]
    slot = {f: f for f in range(-4, n + 4)}
    for batch in (1, 3, 4):
        J = R.max_instants(fine)
        nout = (batch + 1) * J if full else batch * J + 1                # ``Y4mEdge``'s
        spec = EdgeSpec(y4m=True, full=full, shutter=shutter, interlace=('t', 'linear'))
        *bufs, host = egress_layout(spec, nout, batch, 48, 72)
        rows = {b.name: b.rows for b in bufs}
        still_open, scene, open_frame, written, skipped = [], 0, None, 0, 0
        for b0 in range(0, len(ks), batch):
            bw = wins[b0:b0 + batch]
            plan = plan_fine(spec, fine, bw, b0, lambda j: ks[j], lambda j: j == len(ks) - 1, None, None, [list(w) for w in bw], slot)
            counts = [len(o) for o in plan[1]]
            skipped += sum(not o for o in plan[1])
            assert sum(counts) <= rows['gather'] == nout and len(plan[0]) == sum(bool(o) for o in plan[1])
            if shutter:
                lead = shutter[0] - 1
                still_open = [(g, c, lead - len(still_open) + j) for j, (g, c, _) in enumerate(still_open)]
                table, counts, still_open, scene = SH.close_groups(still_open, plan[4], scene, plan[5], *shutter, lead)
                assert len(table) == sum(counts) <= rows['mix'] and len(still_open) <= lead
            pairs, woven, open_frame = IL.close_pairs(0 if open_frame is not None else None, counts, plan[5], 1)
            assert len(pairs) == sum(woven) <= rows['weave'] == host[0]
            written += len(pairs)
        assert written == IL.n_payloads(R.n_output_frames(n, r, full))
        assert skipped == sum(1 for k in ks if not _needed(k, fine, k == ks[-1], full, shutter))


def _needed(k, fine, last, full, shutter):
    outs = R.window_outputs(k, fine, last, full)
    return [o for o in outs if shutter is None or o[0] % shutter[1] < shutter[0]]


# ---- scene cuts ----------------------------------------------------------------------------------------------------------------------
@TIMELINES
@pytest.mark.parametrize('r', [Fraction(5, 6), Fraction(5, 12), Fraction(1, 2), Fraction(1, 3)], ids=str)
def test_window_runs_below_one_around_a_cut(r, full):
    n = 13
    for cut in range(2, n - 1):
        raw = lambda j: j == cut                                          # noqa: E731
        is_cut = S.with_sentinels(raw, n) if full else raw
        ks = _windows(n, full)
        seen, scene, scenes = [], 0, {}
        for k in ks:
            last = k == ks[-1]
            runs, outs = S.window_runs(k, r, last, is_cut, full)
            own = R.window_outputs(k, r, last, full)
            assert [i for i, _, _, _ in outs] == [i for i, _, _ in own]                  # the union of outputs is unchanged
            assert sorted({run for _, run, _, _ in outs}) == list(range(len(runs)))      # no run without an output
            assert bool(runs) == bool(own)
            is_cw = k >= -1 and S.is_cut_window(k, is_cut)
            if is_cw:
                left, right = S.cut_runs(k, is_cut)
                for i, run, kind, j in outs:
                    frac = Fraction(i) / r - k - (1 if full else 0)                      # tau_i - B0
                    on_left = frac < Fraction(1, 2) and dict((a, b) for a, b, _ in own)[i] != R.S1
                    assert runs[run] == ((left, [0.5]) if on_left else (right, [0.5])) and kind == (R.S0 if on_left else R.S1)
                    scenes[i] = scene + (0 if on_left else 1)
                scene += 1
            else:
                assert len(runs) <= 1
                for i, _, _, _ in outs:
                    scenes[i] = scene
            seen += [i for i, _, _, _ in outs]
        assert seen == list(range(R.n_output_frames(n, r, full)))
        # the scene of output i by a per-frame walk: tau_i lies in [B0, B0 + 1/2) of its window -> B0's scene, else B1's; S1 is B1's
        for i in seen:
            tau = Fraction(i) / r + (0 if full else 1)
            nearest = min(math.floor(tau + Fraction(1, 2)), n - 1)
            assert scenes[i] == int(nearest >= cut), (cut, i)
        # and what ``shutter.close_groups`` sees through ``plan_fine`` is the same walk (S = D = 1: every frame its own group)
        spec = EdgeSpec(y4m=True, cuts=True, full=full, shutter=(1, 1))
        wins = [S.runner_order((k, k + 1, k + 2, k + 3)) for k in ks]
        det = SimpleNamespace(is_cut=raw)
        slot = {f: f for f in range(-4, n + 4)}
        for batch in (1, 3, 4):
            sc, got, cut_windows = 0, {}, 0
            for b0 in range(0, len(ks), batch):
                bw = wins[b0:b0 + batch]
                plan = plan_fine(spec, r, bw, b0, lambda j: ks[j], lambda j: j == len(ks) - 1, det, None, None, slot)
                cut_windows += plan[2]
                for cw, entries in plan[4]:
                    for g, right in entries:
                        got[g] = sc + int(right)
                    sc += int(cw)
            assert got == scenes and sc == 1 and cut_windows <= 1


# ---- the shutter below the fine ratio D ------------------------------------------------------------------------------------------------
@TIMELINES
@pytest.mark.parametrize('r,S_,D', [(Fraction(2, 5), 4, 8), (Fraction(1, 10), 2, 2), (Fraction(5, 6), 3, 4), (Fraction(1, 2), 2, 4)], ids=str)
def test_filter_plan_and_close_groups_below_d_give_the_groups(r, S_, D, full):
    fine = SH.fine_ratio(r, D)
    assert fine < D
    for n in (5, 9, 16):
        ks = _windows(n, full)
        n_fine, n_out = R.n_output_frames(n, fine, full), R.n_output_frames(n, r, full)
        want = SH.groups(n_fine, n_out, S_, D)
        wins = [S.runner_order((k, k + 1, k + 2, k + 3)) for k in ks]
        slot = {f: f for f in range(-4, n + 4)}
        spec = EdgeSpec(y4m=True, full=full, shutter=(S_, D))
        for batch in (1, 2, 3, 4, 7):
            still_open, scene, got, rows_of, per_window = [], 0, [], {}, []
            for b0 in range(0, len(ks), batch):
                bw = wins[b0:b0 + batch]
                plan = plan_fine(spec, fine, bw, b0, lambda j: ks[j], lambda j: j == len(ks) - 1, None, None, [list(w) for w in bw], slot)
                lead = S_ - 1
                moved = {rw: lead - len(still_open) + j for j, (_, _, rw) in enumerate(still_open)}
                rows_of = {moved[rw]: g for rw, g in rows_of.items() if rw in moved}
                still_open = [(g, c, moved[rw]) for g, c, rw in still_open]
                row = lead
                for _, entries in plan[4]:
                    for g, _ in entries:
                        rows_of[row] = g
                        row += 1
                table, counts, still_open, scene = SH.close_groups(still_open, plan[4], scene, plan[5], S_, D, lead)
                got += [[rows_of[rw] for rw in t] for t in table]
                per_window += counts
            assert got == want and sum(per_window) == n_out and not still_open, (n, batch)


# ---- refusals and headers --------------------------------------------------------------------------------------------------------------
def _clip(n, fps=b'60:1', tag=b'Ip', h=48, w=80):
    P = y4m.payload_size(h, w, '420')
    rng = np.random.default_rng(n)
    return (b'YUV4MPEG2 W%d H%d F%s %s A1:1 C420jpeg\n' % (w, h, fps, tag)
            + b''.join(b'FRAME\n' + rng.integers(16, 235, P, dtype=np.uint8).tobytes() for _ in range(n)))


def test_refusals():
    with pytest.raises(ValueError, match='only F_out >= F_in'):
        video.VideoRunner(None, 1, fps=Fraction(30)).run_stream(io.BytesIO(_clip(6)), io.BytesIO())
    with pytest.raises(ValueError, match='--dedup does not go with an output rate below'):
        video.VideoRunner(None, 1, fps=Fraction(30), down=True, dedup=True).run_stream(io.BytesIO(_clip(6)), io.BytesIO())
    vr = video.VideoRunner(None, 1, fps=Fraction(120), down=True, dedup=True)     # r >= 1: the switch changes nothing, --dedup included
    assert vr._fine_ratio(y4m.parse_header(b'YUV4MPEG2 W80 H48 F60:1 Ip')) == 2
    with pytest.raises(ValueError, match='1/64'):
        video.VideoRunner(None, 1, fps=Fraction(1, 2), down=True).run_stream(io.BytesIO(_clip(6)), io.BytesIO())
    with pytest.raises(ValueError, match='--shutter ANGLE'):
        video.VideoRunner(None, 1, mfi=2, shutter_window='triangle')
    with pytest.raises(ValueError, match='--shutter ANGLE'):
        video.VideoRunner(None, 1, mfi=2, shutter_window='box')
    with pytest.raises(ValueError, match='box, triangle'):
        video.VideoRunner(None, 1, mfi=2, shutter=180, shutter_window='gaussian')
    with pytest.raises(SystemExit):
        video.parser().parse_args(['a', 'b', '--shutter', '180', '--shutter-window', 'gaussian'])
    a = video.parser().parse_args(['a', 'b', '--fps', '25', '--downconvert', '--shutter', '180', '--shutter-window', 'triangle'])
    assert a.downconvert and a.shutter_window == 'triangle' and not video.parser().parse_args(['a', 'b']).downconvert
    # below the field rate and below the film rate without the switch: as before
    fields = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 It', fields=True)
    with pytest.raises(ValueError, match='field rate 50'):
        video.VideoRunner(None, 1, fps=Fraction(30), deinterlace=True)._progressive(fields)
    assert video.VideoRunner(None, 1, fps=Fraction(30), deinterlace=True, down=True)._progressive(fields)[0].fps == 50
    tele = y4m.parse_header(b'YUV4MPEG2 W720 H480 F30000:1001 It', telecine=True)
    with pytest.raises(ValueError, match='film rate 24000/1001'):
        video.VideoRunner(None, 1, fps=Fraction(20), ivtc=True)._progressive(tele)
    assert video.VideoRunner(None, 1, fps=Fraction(20), ivtc=True, down=True)._progressive(tele)[0].fps == Fraction(24000, 1001)
    with pytest.raises(ValueError, match='shutter_window'):
        EdgeSpec(y4m=True, shutter_window='triangle').check(True, False, True)
    assert EdgeSpec(y4m=True, shutter=(4, 8), shutter_window='box') == EdgeSpec(y4m=True, shutter=(4, 8))
    assert EdgeSpec(y4m=True, shutter=(4, 8), shutter_window='triangle') != EdgeSpec(y4m=True, shutter=(4, 8))
    assert EdgeSpec(y4m=True, shutter=(4, 8), shutter_window='triangle')._replace(cuts=True).shutter_window == 'triangle'
    assert hash(EdgeSpec(y4m=True, shutter=(4, 8), shutter_window='box')) == hash(EdgeSpec(y4m=True, shutter=(4, 8)))


def test_headers():
    vr = video.VideoRunner(None, 1, fps=Fraction(25), down=True)
    hdr = y4m.parse_header(b'YUV4MPEG2 W80 H48 F60:1 Ip A1:1 C420jpeg')
    assert vr._ratio(hdr) == Fraction(5, 12) and vr._out_header(hdr).encode().startswith(b'YUV4MPEG2 W80 H48 F25:1 Ip')
    assert vr._n_out(16, hdr) == math.floor(13 * Fraction(5, 12)) + 1 == 6
    vr = video.VideoRunner(None, 1, fps=Fraction(50), down=True, deinterlace=True, interlace='tff')
    ph, order, per = vr._progressive(y4m.parse_header(b'YUV4MPEG2 W720 H480 F30000:1001 It A8:9 C420jpeg', fields=True))
    assert (ph.fps, order, per) == (Fraction(60000, 1001), 't', 2) and vr._ratio(ph) == Fraction(1001, 1200)
    assert vr._out_header(ph).encode().startswith(b'YUV4MPEG2 W720 H480 F25:1 It')
    assert vr.last_windows_skipped == 0 and vr.last_shutter_window is None
