"""``demfi_amd.cadence`` on the host: the block counts that define a repeated frame, the detector, and the timeline over the kept
frames -- its identities with ``retime`` / ``scene`` (no repeats: the same plans; every frame doubled at ratio r: the plans of the
undoubled clip at 2 r; every output owned once, in order) and the plan of a stream read with bounded look-ahead."""
import io
import itertools
import random
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import cadence as K
from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import y4m

RATIOS = [Fraction(1), Fraction(2), Fraction(5, 2), Fraction(8), Fraction(60000, 24024), Fraction(60000 * 1001, 1001 * 25000)]


# ---- block counts ----------------------------------------------------------------------------------------------------------
def _frame(h, w, seed=0, depth=8):
    rng = np.random.default_rng(seed)
    return rng.integers(16 << (depth - 8), 200 << (depth - 8), h * w + (h * w) // 2, dtype=np.int64).astype(np.uint8 if depth == 8 else np.uint16)


def _counts_slow(a, b, h, w, depth, hi, lo):
    """The definition, block by block in Python integers."""
    la, lb = (np.asarray(x).reshape(-1)[:h * w].reshape(h, w).astype(object) for x in (a, b))
    s, hot, warm = 1 << (depth - 8), 0, 0
    for y0 in range(0, h, 8):
        for x0 in range(0, w, 8):
            blk = abs(la[y0:y0 + 8, x0:x0 + 8] - lb[y0:y0 + 8, x0:x0 + 8])
            sad, area = int(blk.sum()), blk.size
            hot += 64 * sad > hi * s * area
            warm += 64 * sad > lo * s * area
    return hot, warm


def test_identical_frames_count_nothing():
    a = _frame(70, 70)
    assert K.block_counts_np(a, a.copy(), 70, 70) == (0, 0)
    assert K.is_repeat(0, 0, K.n_blocks(70, 70))


def test_one_lsb_of_noise_everywhere_is_a_repeat():
    a = _frame(72, 88, 1)
    rng = np.random.default_rng(2)
    b = (a.astype(np.int64) + rng.choice([-1, 1], a.size)).astype(np.uint8)
    hot, warm = K.block_counts_np(b, a, 72, 88)
    assert (hot, warm) == (0, 0)                        # 64 * SAD = 64 * 64 <= 320 * 64
    assert K.is_repeat(hot, warm, K.n_blocks(72, 88))


def test_a_small_moving_block_is_not_a_repeat_though_its_mafd_is_tiny():
    h, w = 240, 320
    a = np.full(h * w * 3 // 2, 60, np.uint8)
    b = a.copy()
    a[:h * w].reshape(h, w)[96:104, 160:168] = 220
    b[:h * w].reshape(h, w)[96:104, 164:172] = 220      # the same 8x8 block, 4 pixels to the right
    hot, warm = K.block_counts_np(b, a, h, w)
    assert hot == 2 and warm == 2                       # half a block changed by 160 in each of two blocks: 64 * 5120 > 768 * 64
    assert not K.is_repeat(hot, warm, K.n_blocks(h, w))
    assert S.mafd(S.sad_np(a, b), a.size) < 0.1         # far below any scene-cut threshold


@pytest.mark.parametrize('depth', [10, 16])
def test_deep_frames_count_like_the_8_bit_frames_scaled(depth):
    h, w, s = 38, 52, 1 << (depth - 8)
    a8, b8 = _frame(h, w, 3), _frame(h, w, 3)
    rng = np.random.default_rng(4)
    l = b8[:h * w].reshape(h, w)
    l[8:24, 8:40] += rng.integers(0, 30, (16, 32)).astype(np.uint8)      # about 15 per sample: hot
    l[24:38, 0:52] += rng.integers(5, 10, (14, 52)).astype(np.uint8)      # about 7 per sample: warm only
    a, b = (x.astype(np.uint16) * s for x in (a8, b8))
    exp = K.block_counts_np(a8, b8, h, w)
    assert exp[1] > exp[0] > 0
    assert K.block_counts_np(a, b, h, w, depth) == exp
    assert K.block_counts_np(a.view(np.uint8), b.view(np.uint8), h, w, depth) == exp     # the payload's bytes
    assert K.block_counts_np(a, b, h, w, depth) != K.block_counts_np(a, b, h, w, 16 if depth == 10 else 10)


@pytest.mark.parametrize('h,w', list(itertools.product([2, 7, 9, 70], repeat=2)))
def test_partial_blocks(h, w):
    rng = np.random.default_rng(h * 100 + w)
    a = rng.integers(0, 256, h * w, dtype=np.int64).astype(np.uint8)
    for amp in (3, 8, 14, 40):
        b = np.clip(a.astype(np.int64) + rng.integers(-amp, amp + 1, a.size), 0, 255).astype(np.uint8)
        assert K.block_counts_np(a, b, h, w) == _counts_slow(a, b, h, w, 8, K.DEFAULT_HI, K.DEFAULT_LO)
        assert K.block_counts_np(a, b, h, w, 8, 200, 100) == _counts_slow(a, b, h, w, 8, 200, 100)
    sads, area = K.block_sads_np(a, a, h, w)
    assert int(area.sum()) == h * w and area.shape == (-(-h // 8), -(-w // 8)) == sads.shape
    assert K.n_blocks(h, w) == area.size
    # a partial block is judged by its own area: 13 per sample is hot in every block, 12 in none
    assert K.block_counts_np(np.full(h * w, 13, np.uint8), np.zeros(h * w, np.uint8), h, w) == (area.size, area.size)
    assert K.block_counts_np(np.full(h * w, 12, np.uint8), np.zeros(h * w, np.uint8), h, w) == (0, area.size)


def test_the_repeat_test_is_an_integer_comparison():
    assert K.is_repeat(0, 33, 100) and not K.is_repeat(0, 34, 100) and not K.is_repeat(1, 0, 100)
    assert K.is_repeat(0, 1, 3, Fraction(1, 3)) and not K.is_repeat(0, 2, 3, Fraction(1, 3))
    assert K.is_repeat(0, 7, 7, 1) and not K.is_repeat(0, 1, 7, 0)


# ---- the detector -----------------------------------------------------------------------------------------------------------
def test_max_hold_caps_a_still_scene():
    a = _frame(16, 16)
    assert K.kept_of([a] * 11, 16, 16) == [0, 4, 8]
    assert K.kept_of([a] * 11, 16, 16, max_hold=1) == [0, 2, 4, 6, 8, 10]
    det = K.Detector(16, 16, max_hold=2)
    flags = []
    for i in range(7):
        flags.append(det.push(i, None if det.forced() else (0, 0)))
    assert flags == [True, False, False, True, False, False, True] and det.dups == [1, 2, 4, 5] and det.kept == [0, 3, 6]


def test_a_slow_drift_is_kept_in_the_end():
    """+1 LSB per frame: every frame is within 1 LSB of its predecessor, but the comparison is with the last KEPT frame."""
    base = np.full(32 * 32, 50, np.uint8)
    clip = [base + i for i in range(40)]
    kept = K.kept_of(clip, 32, 32, max_hold=1000)
    assert kept[0] == 0 and len(kept) > 1
    # the first frame whose blocks are warm (64 * 64 d > 320 * 64: d = 6) in more than a third of the plane
    assert kept[1] == 6 and kept[:4] == [0, 6, 12, 18]
    prev = [K.block_counts_np(clip[i], clip[i - 1], 32, 32) for i in range(1, 40)]
    assert all(c == (0, 0) for c in prev)


def test_detector_order_and_arguments():
    det = K.Detector(16, 16)
    with pytest.raises(RuntimeError):
        det.push(1, (0, 0))
    det.push(0)
    with pytest.raises(RuntimeError):
        det.push(1)                                     # not forced: the counts are needed
    for bad in (dict(hi=100, lo=200), dict(frac=Fraction(3, 2)), dict(frac=Fraction(-1, 3)), dict(max_hold=0), dict(lo=-1),
                dict(frac=0.33), dict(hi=7.5)):
        with pytest.raises(ValueError):
            K.check_params(**bad)
    assert K.check_params() == (768, 320, Fraction(33, 100), 3)
    assert K.check_params(10, 10, 1, 1) == (10, 10, Fraction(1), 1)
    with pytest.raises(ValueError):
        K.luma_np(np.zeros(10, np.uint8), 4, 4)


# ---- the timeline -----------------------------------------------------------------------------------------------------------
def _patterns(n, max_hold, rng, count):
    """Random keep / repeat patterns of n frames with at most max_hold repeats in a row -> lists of kept times."""
    out = []
    for _ in range(count):
        s, run = [0], 0
        for i in range(1, n):
            if run < max_hold and rng.random() < 0.5:
                run += 1
            else:
                s.append(i)
                run = 0
        out.append(s)
    return out


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', RATIOS, ids=str)
def test_no_repeats_is_retime(r, full):
    for n in range(1, 13):
        s = list(range(n))
        k0, nw = R.first_window(n, full), R.n_windows(n, full)
        assert K.windows(s, n, full, r) == list(range(k0, k0 + nw))
        for k in range(k0, k0 + nw):
            last = k == k0 + nw - 1
            assert K.window_plan(k, r, s, n, full) == R.window_plan(k, r, last, full)
            assert K.window_outputs(k, r, s, n, full) == R.window_outputs(k, r, last, full)
            for cuts in ([], [3], [2, 5]):
                is_cut = (lambda j, c=cuts: j in c)
                ref = S.window_runs(k, r, last, S.with_sentinels(is_cut, n) if full else is_cut, full)
                assert K.window_runs(k, r, s, n, is_cut, full) == ref


@pytest.mark.parametrize('r', RATIOS[:5], ids=str)
def test_doubled_frames_at_r_are_the_clip_at_2r(r):
    for n in range(1, 12):
        s2 = list(range(0, 2 * n, 2))
        ks = K.windows(s2, 2 * n, True, r)
        assert ks == list(range(R.first_window(n, True), R.first_window(n, True) + R.n_windows(n, True)))
        for k in ks:
            last = k == ks[-1]
            ts, outs = K.window_plan(k, r, s2, 2 * n, True)
            ts1, outs1 = R.window_plan(k, 2 * r, last, True)
            assert [np.float32(t).tobytes() for t in ts] == [np.float32(t).tobytes() for t in ts1] and outs == outs1
            assert K.window_tuple(k, s2, 2 * n) == S.clip_tuple(k, S.with_sentinels(lambda j: False, n))
            runs, ro = K.window_runs(k, r, s2, 2 * n, None, True)           # the same instants, in runs of at most ceil(r)
            J = R.max_instants(r)
            assert all(len(t) <= J for _, t in runs) and [t for _, tt in runs for t in tt] == ts
            assert [(i, kind, run * J + j) for i, run, kind, j in ro] == outs


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', RATIOS, ids=str)
def test_every_output_is_owned_once_in_order(r, full):
    rng = random.Random(int(r * 1000) + full)
    for n in range(1, 13):
        for max_hold in (1, 3):
            for s in _patterns(n, max_hold, rng, 6):
                total = R.n_output_frames(n, r, full)
                ks = K.windows(s, n, full, r)
                assert ks == list(range(ks[0], ks[0] + len(ks))) if ks else total == 0
                owned = []
                for k in ks:
                    outs = K.window_outputs(k, r, s, n, full)
                    assert outs
                    owned += [i for i, _, _ in outs]
                    runs, ro = K.window_runs(k, r, s, n, None, full)
                    Jw = K.max_window_instants(r, max_hold)             # the last window's hold is as many again at most
                    assert len(runs) <= K.max_window_runs(r, max_hold) and sum(len(ts) for _, ts in runs) <= Jw
                    assert len(outs) <= (2 * Jw if k == ks[-1] else Jw)
                    assert all(0 < len(ts) <= R.max_instants(r) for _, ts in runs)
                    assert all(0 <= x <= len(s) - 1 for tup, _ in runs for x in tup)
                    for (i, run, kind, j), (i1, kind1, t) in zip(ro, outs):
                        assert (i, kind) == (i1, kind1) and (kind != R.ST or runs[run][1][j] == t)
                assert owned == list(range(total)), (n, s, r, full)


def test_positions_on_a_three_two_cadence():
    """A B B C D D E, r = 2, full length: kept at 0 1 3 4 6; the gap of 2 is interpolated at quarters."""
    s, n, r = [0, 1, 3, 4, 6], 7, Fraction(2)
    assert K.windows(s, n, True, r) == [-1, 0, 1, 2]
    assert K.window_outputs(0, r, s, n, True) == [(2, R.S0, None), (3, R.ST, 0.25), (4, R.ST, 0.5), (5, R.ST, 0.75)]
    assert K.window_runs(0, r, s, n, None, True) == ([((0, 1, 2, 3), [0.25, 0.5]), ((0, 1, 2, 3), [0.75])],
                                                    [(2, 0, R.S0, 0), (3, 0, R.ST, 0), (4, 0, R.ST, 1), (5, 1, R.ST, 0)])
    assert K.window_outputs(2, r, s, n, True) == [(8, R.S0, None), (9, R.ST, 0.25), (10, R.ST, 0.5), (11, R.ST, 0.75),
                                                 (12, R.S1, None), (13, R.S1, None)]
    assert K.window_tuple(-1, s, n) == (0, 0, 1, 2) and K.window_tuple(2, s, n) == (2, 3, 4, 4)
    # the reference's timeline: tau = 1 + i / 2 <= 5; the last output sits inside the last gap
    assert K.windows(s, n, False, r) == [0, 1, 2]
    assert K.window_outputs(2, r, s, n, False) == [(6, R.S0, None), (7, R.ST, 0.25), (8, R.ST, 0.5)]
    # tau = 1 inside [s_0, s_1): window -1 exists and clamps
    s = [0, 2, 3, 4, 5]
    assert K.windows(s, 6, False, r) == [-1, 0, 1] and K.window_tuple(-1, s, 6) == (0, 0, 1, 2)
    assert K.window_outputs(-1, r, s, 6, False) == [(0, R.ST, 0.5), (1, R.ST, 0.75)]
    # tau = n - 2 on a kept frame: the S1 of the window that ends there
    assert K.window_outputs(1, r, s, 6, False) == [(4, R.S0, None), (5, R.ST, 0.5), (6, R.S1, None)]
    # one kept frame
    assert K.windows([0], 4, False, r) == [-2] and K.window_runs(-2, r, [0], 4) == ([((0, 0, 0, 0), [0.5])], [(i, 0, R.S1, 0) for i in range(3)])


def test_cuts_over_the_kept_sequence():
    """A A B B | C C D D with a cut between the kept frames 1 (B) and 2 (C): is_cut speaks of kept indices."""
    s, n, r = [0, 2, 4, 6], 8, Fraction(2)
    is_cut = lambda j: j == 2                           # noqa: E731
    runs, outs = K.window_runs(0, r, s, n, is_cut, True)                    # the cut window: between kept 1 and kept 2
    assert runs == [((0, 1, 1, 1), [0.5]), ((2, 2, 2, 3), [0.5])]
    assert outs == [(4, 0, R.S0, 0), (5, 0, R.S0, 0), (6, 1, R.S1, 0), (7, 1, R.S1, 0)]       # the nearer frame in input time
    assert K.window_runs(-1, r, s, n, is_cut, True)[0] == [((0, 0, 1, 1), [0.25, 0.5]), ((0, 0, 1, 1), [0.75])]
    assert K.window_runs(1, r, s, n, is_cut, True)[0][0][0] == (2, 2, 3, 3)
    assert K.is_cut_window(0, is_cut) and not K.is_cut_window(1, is_cut) and not K.is_cut_window(-2, is_cut)
    # scene scores see the kept frames only: a doubled clip's SAD series has no zeros in it
    a, b = np.zeros(64, np.uint8), np.full(64, 200, np.uint8)
    clip = [a, a, a + 1, a + 1, b, b, b + 1, b + 1]
    kept = K.kept_of(clip, 8, 8)
    assert kept == [0, 4]                               # +1 is a repeat; the cut is kept
    kept = K.kept_of(clip, 8, 8, hi=32, lo=16)
    assert kept == s
    sads = [S.sad_np(clip[kept[j]], clip[kept[j - 1]]) for j in range(1, len(kept))]
    assert S.cuts_of(sads, 64, 10.0) == [2] and S.cuts_of([S.sad_np(clip[j], clip[j - 1]) for j in range(1, 8)], 64, 10.0) == [4]


# ---- a stream: bounded look-ahead ---------------------------------------------------------------------------------------------
class _HostEdge:
    """What ``pipeline.KeptFrames`` asks of ``Y4mEdge``, on the host: slots are a dict, the counts are ``block_counts_np``."""

    def __init__(self, h, w, det):
        self.h, self.w, self.det, self.slots, self.staged, self.max_slots = h, w, det, {}, None, 0

    def stage(self, key, idx, f):
        self.slots[key] = f.numpy().copy()
        self.staged = key
        self.max_slots = max(self.max_slots, len(self.slots))
        return key

    def block_counts(self, sl, ref):
        return K.block_counts_np(self.slots[sl], self.slots[ref], self.h, self.w, 8, self.det.hi, self.det.lo)

    def keep(self, key, sl):
        assert key == sl == self.staged

    def discard(self, key):
        assert key == self.staged
        del self.slots[key]


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
@pytest.mark.parametrize('r', [Fraction(1), Fraction(2), Fraction(5, 2)], ids=str)
def test_a_stream_is_planned_as_the_whole_clip(r, full):
    """``KeptFrames`` over a pipe: the windows it hands out, planned with what is known when each is handed out, are the windows
    and plans of the whole clip; it reads at most a few frames ahead and a repeat never keeps a slot."""
    from demfi_amd.pipeline import KeptFrames
    h, w = 16, 24
    rng = random.Random(7)
    P = y4m.payload_size(h, w)
    for n in range(0, 12):
        for s in ([[]] if n == 0 else _patterns(n, 3, rng, 5)):
            pays, cur = [], None
            for i in range(n):
                if i in s:
                    cur = np.full(P, 40 + 17 * len(pays), np.uint8)
                pays.append(cur)
            data = b'YUV4MPEG2 W%d H%d F24:1 Ip C420jpeg\n' % (w, h) + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
            raw = y4m.Frames(y4m.Reader(_Pipe(data)), pinned=False)
            det = K.Detector(h, w)
            kf = KeptFrames(raw, det, r, full)
            kf.edge = edge = _HostEdge(h, w, det)
            got = []
            for j, tup in enumerate(kf.windows()):
                k = kf.index(j)
                assert K.ready(k, kf.s, raw.next, kf.n, full)
                got.append((k, tup, K.window_runs(k, r, list(kf.s), kf.n, None, full)))
                assert raw.next <= (kf.s[k + 2] if k >= -1 else 0) + 3 + det.max_hold + 1   # bounded look-ahead
            assert kf.n == n and det.kept == s and sorted(det.kept + det.dups) == list(range(n))
            exp = [(k, S.runner_order(K.window_tuple(k, s, n)), K.window_runs(k, r, s, n, None, full)) for k in K.windows(s, n, full, r)]
            assert got == exp, (n, s)
            assert sorted(edge.slots) == list(range(len(s))) and edge.max_slots <= len(s) + 1
            assert raw.peak <= 8


# ---- the interface, where it needs no GPU --------------------------------------------------------------------------------------
def test_video_runner_arguments(tmp_path):
    from demfi_amd.video import VideoRunner, parser
    assert VideoRunner(None, mfi=2).dedup is None and VideoRunner(None, mfi=2, dedup=False).dedup is None
    assert VideoRunner(None, mfi=2, dedup=True).dedup == (768, 320, Fraction(33, 100), 3)
    assert VideoRunner(None, mfi=2, dedup=(100, 50, Fraction(1, 2)), dedup_max_hold=5).dedup == (100, 50, Fraction(1, 2), 5)
    for bad in (dict(dedup=(100, 200, Fraction(1, 3))), dict(dedup=(768, 320, Fraction(3, 2))), dict(dedup=(768, 320, Fraction(-1, 2))),
                dict(dedup=True, dedup_max_hold=0), dict(dedup_max_hold=0)):
        with pytest.raises(ValueError):
            VideoRunner(None, mfi=2, **bad)
    with pytest.raises(ValueError, match='whole prefix'):         # before anything is opened
        VideoRunner(None, mfi=2, dedup=True).run_file(str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m'), world=2, rank=1)
    a = parser().parse_args(['in', 'out', '--dedup', '--dedup-max-hold', '2'])
    assert a.dedup is True and a.dedup_max_hold == 2
    a = parser().parse_args(['in', 'out'])
    assert a.dedup is False and a.dedup_max_hold == K.DEFAULT_MAX_HOLD
