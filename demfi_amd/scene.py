"""Scene cuts of the Y4M video path (``python -m demfi_amd.video --scene-cut [T]``): where they are, and what a window next to one
runs.  Pure Python; the one module that knows the policy.

Input frames are numbered 0 .. n-1 and window k reads frames k .. k+3, interpolating between B0 = k+1 and B1 = k+2 (``retime``).
p_j is the raw payload of frame j (all its payload samples: Y, Cb, Cr of a 4:2:0, 4:2:2 or 4:4:4 stream, Y of a mono one; P of
them, bytes at 8 bits).  For j = 1 .. n-1
  SAD_j   = sum |p_j - p_{j-1}| over the P payload samples (an exact integer; the GPU computes it, ``sad_np`` defines it),
  mafd_j  = 100 * SAD_j / (255 * P) in float64, mafd_0 = 0,
  score_j = min(mafd_j, |mafd_j - mafd_{j-1}|),
and a cut lies before frame j iff score_j >= T.  This has the shape of ffmpeg's ``scdet`` filter (the mean absolute frame
difference and how much it changed), so T is picked the same way; numeric equality with it is not claimed.
At bit depth d > 8 (``y4m``: 16-bit samples) everything counts samples, not bytes: SAD_j sums over the P samples and
mafd_j = 100 * SAD_j / (peak * P) with peak = 2^d - 1, so a threshold T means the same picture change at every depth.

scene(i) = number of cuts before frames 1 .. i.  Window k is
  * an inner window when scene(k+1) == scene(k+2): it runs its usual instants and outputs on the clamped tuple
    B-1 = k if scene(k) == scene(k+1) else k+1,  B2 = k+3 if scene(k+3) == scene(k+2) else k+2
    (a window that touches no cut runs exactly what it runs without cuts);
  * a cut window when scene(k+1) != scene(k+2), b = k+1: nothing is interpolated.  Two runs at the single instant t = 1/2,
    written (B-1, B0, B1, B2): left = (L, b, b, b) with L = b-1 if scene(b-1) == scene(b) else b, and right = (b+1, b+1, b+1, R)
    with R = b+2 if scene(b+2) == scene(b+1) else b+1.  Of the window's own outputs (``retime.window_outputs``), S0 and every
    St whose exact in-window fraction is below 1/2 are left's S0; every St at 1/2 or later, and S1 of the last window, are
    right's S1 (nearest-frame hold).
The output timing (header, frame count, the position of every frame) is that of the run without cuts.

On the full-length timeline (``retime``, ``full_length``) the clip's ends are cuts by another name: ``with_sentinels`` adds a
cut before frame 0 and one before frame n (frames -1 and n are scenes of their own), so the rules above clamp window -1 to
B-1 = 0 and the last window to B2 = n-1, and a real cut before frame 1 or n-1 makes window -1 or n-3 a cut window.  The one
window of a one-frame clip (k = -2) runs (0, 0, 0, 0).
"""
from fractions import Fraction

import numpy as np

from . import retime as R

DEFAULT_THRESHOLD = 10.0
HALF = Fraction(1, 2)


def check_threshold(t):
    """T as a float in (0, 100]; ValueError otherwise."""
    t = float(t)
    if not 0.0 < t <= 100.0:
        raise ValueError('scene-cut threshold %r outside (0, 100]' % t)
    return t


def sad_np(a, b):
    """SAD of two payloads (uint8 arrays of the same length, or uint16 arrays of samples): sum |a - b| as a Python int."""
    if all(isinstance(x, np.ndarray) and x.dtype == np.uint16 for x in (a, b)):
        a, b, wide = a.reshape(-1), b.reshape(-1), np.int32
    else:
        a, b, wide = np.asarray(a, np.uint8).reshape(-1), np.asarray(b, np.uint8).reshape(-1), np.int16
    if a.shape != b.shape:
        raise ValueError('sad_np: payloads of %d and %d samples' % (a.size, b.size))
    return int(np.abs(a.astype(wide) - b.astype(wide)).sum(dtype=np.int64))


def mafd(sad, payload, peak=255):
    """100 * SAD / (peak * payload): ``payload`` counts samples, ``peak`` is the largest sample value (2^d - 1)."""
    return 100.0 * int(sad) / (int(peak) * int(payload))


def scores(sads, payload, peak=255):
    """score_1 .. score_{n-1} from SAD_1 .. SAD_{n-1} of a whole stream."""
    out, prev = [], 0.0
    for s in sads:
        m = mafd(s, payload, peak)
        out.append(min(m, abs(m - prev)))
        prev = m
    return out


def cuts_of(sads, payload, threshold, peak=255):
    """Frame indices j that start a scene (a cut before j), from SAD_1 .. SAD_{n-1} of a whole stream."""
    return [j for j, s in enumerate(scores(sads, payload, peak), 1) if s >= threshold]


class Detector:
    """The cuts of a stream as its SADs arrive in frame order: ``push(j, SAD_j)`` for consecutive j.  ``first`` is the first frame
    read: mafd_0 = 0 is known when it is 0; otherwise the first SAD pushed (SAD_{first+1}) only supplies mafd_{first+1}, and cuts
    are decided from frame first + 2 on -- a rank whose block starts at window lo >= 1 reads from frame lo - 1, which decides every
    cut its windows look at (j >= lo + 1) as one rank over the whole stream would.  ``payload`` / ``peak``: as ``mafd``."""

    def __init__(self, payload, threshold, first=0, peak=255):
        self.payload, self.threshold, self.peak = int(payload), check_threshold(threshold), int(peak)
        self.next = first + 1
        self.prev = 0.0 if first == 0 else None
        self.cuts = []
        self._cut = set()

    def push(self, j, sad):
        if j != self.next:
            raise RuntimeError('scene.Detector: SAD of frame %d pushed where frame %d was due' % (j, self.next))
        m = mafd(sad, self.payload, self.peak)
        if self.prev is not None and min(m, abs(m - self.prev)) >= self.threshold:
            self.cuts.append(j)
            self._cut.add(j)
        self.prev = m
        self.next = j + 1

    def is_cut(self, j):
        """Is there a cut before frame j (j must have been pushed)?"""
        if j >= self.next:
            raise RuntimeError('scene.Detector: frame %d is not scored yet' % j)
        return j in self._cut


def first_frame(lo):
    """First input frame a block of windows starting at window lo must read: lo - 1 when lo >= 1 (score_{lo+1} needs mafd_lo),
    else frame 0 (full-length blocks start at window -1, or -2 for a one-frame clip)."""
    return max(lo - 1, 0)


def with_sentinels(is_cut, n=None):
    """``is_cut`` with the clip's ends as cuts (full-length timeline): a cut before frame 0 and, when the clip's length n is
    known, before frame n.  A reader that does not know n yet has read past every frame it asks about."""
    return lambda j: j <= 0 or (n is not None and j >= n) or is_cut(j)


def clip_tuple(k, is_cut):
    """(B-1, B0, B1, B2) of window k of the full-length timeline that is not a cut window under ``is_cut`` (with sentinels):
    its inner tuple, or (0, 0, 0, 0) for the one window (k = -2) of a one-frame clip."""
    return (0, 0, 0, 0) if k < -1 else inner_tuple(k, is_cut)


def _same(is_cut, i, j):
    """scene(i) == scene(j) for i < j: no cut before any of the frames i+1 .. j."""
    return not any(is_cut(x) for x in range(i + 1, j + 1))


def is_cut_window(k, is_cut):
    return is_cut(k + 2)


def inner_tuple(k, is_cut):
    """(B-1, B0, B1, B2) of inner window k, clamped at the cuts next to it."""
    bm1 = k if _same(is_cut, k, k + 1) else k + 1
    b2 = k + 3 if _same(is_cut, k + 2, k + 3) else k + 2
    return (bm1, k + 1, k + 2, b2)


def cut_runs(k, is_cut):
    """(left, right) runs of cut window k, each (B-1, B0, B1, B2)."""
    b = k + 1
    left = (b - 1 if _same(is_cut, b - 1, b) else b, b, b, b)
    right = (b + 1, b + 1, b + 1, b + 2 if _same(is_cut, b + 1, b + 2) else b + 1)
    return left, right


def window_runs(k, r, last, is_cut, full_length=False):
    """What window k runs for ratio r (``--mfi M`` is r = M): (runs, outs).  runs = [((B-1, B0, B1, B2), instants)];
    outs = [(output index, run, kind, instant index)] in stream order -- kind S0 / St / S1 of that run, as in
    ``retime.window_plan``.  The outputs are those of ``retime.window_outputs(k, r, last, full_length)``; on the full-length
    timeline ``is_cut`` must hold the sentinels (``with_sentinels``).  With r < 1 a window may own no output, or a cut window outputs
    on one side only: a run without an output is not returned (a cut window's right outputs keep the kind S1, whatever their run's
    number); with r >= 1 a cut window is always its two runs."""
    if k < -1 or not is_cut_window(k, is_cut):
        ts, outs = R.window_plan(k, r, last, full_length)
        return ([(clip_tuple(k, is_cut), ts)] if ts else []), [(i, 0, kind, j) for i, kind, j in outs]
    r = Fraction(r)
    left, right = cut_runs(k, is_cut)
    sh = 1 if full_length else 0
    outs = []
    for i, kind, _ in R.window_outputs(k, r, last, full_length):
        # exact in-window fraction of output i: tau_i - (k+1) = i / r - k (- 1 full-length); S0 is 0, S1 is 1
        if kind == R.S0 or (kind == R.ST and Fraction(i) / r - k - sh < HALF):
            outs.append((i, 0, R.S0, 0))
        else:
            outs.append((i, 1, R.S1, 0))
    runs = [(left, [0.5]), (right, [0.5])]
    if r < 1:                                        # the side without an output does not run
        used = sorted({run for _, run, _, _ in outs})
        runs, outs = [runs[run] for run in used], [(i, used.index(run), kind, j) for i, run, kind, j in outs]
    return runs, outs


def runner_order(tup):
    """(B-1, B0, B1, B2) -> the runner's (B0, B1, B-1, B2)."""
    bm1, b0, b1, b2 = tup
    return (b0, b1, bm1, b2)
