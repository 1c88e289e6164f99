"""Repeated frames of the Y4M video path (``python -m demfi_amd.video --dedup``): which input frames repeat the one before them,
and what the windows run once the repeats are left out.  Pure Python and numpy; the one module that knows the policy.

Which frames repeat.  Only the luma plane is read: the first h*w samples of a payload in every layout (bytes at 8 bits,
little-endian uint16 above, as in ``y4m``).  The plane is cut into 8x8 blocks from the top-left corner; blocks at the right and
bottom edges are partial, of area a < 64.  For a frame and the last KEPT frame before it a block's SAD is the sum of absolute
sample differences over the block; with s = 2^(depth-8) the block is hot when 64*SAD > hi*s*a and warm when 64*SAD > lo*s*a
(integers, nothing rounded).  The frame is a repeat when no block is hot and warm_blocks <= frac * n_blocks, frac a Fraction
and the test an integer comparison.  The defaults are those of ffmpeg's ``mpdecimate`` (hi = 768, lo = 320, frac = 33/100; its
blocks are 8x8 too).  Comparing with the last kept frame, not the previous one, keeps a slow drift from being dropped for ever.
Frame 0 is always kept, and after ``max_hold`` consecutive repeats the next frame is kept whatever it would score, so kept
frames are at most max_hold + 1 apart and a stream's look-ahead stays bounded.  ``block_counts_np`` defines the counts (the GPU
computes them: csrc/dedup.hip), ``Detector`` turns them into kept / repeat as frames arrive.

The timeline.  The n input frames sit at input times 0 .. n-1, the m kept frames d_0 .. d_{m-1} at s_0 = 0 < s_1 < ...  Output
frame i sits where it sits without --dedup (``retime``): tau_i = 1 + i / r, tau_i <= n - 2, or tau_i = i / r < n on the
full-length timeline, so the output's length and timing do not change.  Windows are numbered as in ``retime``, over the kept
sequence: window k is (B-1, B0, B1, B2) = kept frames (k, k+1, k+2, k+3) and interpolates between B0 at a = s_{k+1} and B1 at
b = s_{k+2}.  It owns the outputs with tau in [a, b): S0 when tau == a, else St at t = float32_of((tau - a) / (b - a)), rounded
once from the exact rational.  The last window (k = m - 3) also owns every tau >= s_{m-1}: its S1, held.  On the reference's
timeline the output at tau = n - 2, when a kept frame sits there, is the S1 of the window that ends there and not the S0 of the
one that starts there (the last input frame never starts a window, as in ``retime``).  A clip whose kept sequence is one frame
has the single window k = -2 on (0, 0, 0, 0): all its outputs are the S1 hold.  Tuples clamp at the ends of the kept sequence by
``scene.with_sentinels`` on both timelines; on the reference's timeline tau = 1 may lie inside [s_0, s_1), and window -1 then
runs on (0, 0, 1, 2).  A window that owns no output (window -1 when s_1 = 1, the windows past tau = n - 2) does not exist.
With no repeats all of this is ``retime.window_plan``.

``window_plan`` has the shape of ``retime.window_plan``; ``window_runs`` that of ``scene.window_runs``: a window whose gap makes
it own more than ``retime.max_instants(r)`` instants is several runs of at most that many on the same tuple, so no per-run
buffer grows with the gap.  Scene cuts are scored over the kept sequence (the SAD between consecutive kept frames), so is_cut
speaks of kept indices: a cut between d_j and d_{j+1} clamps tuples as ever, and the outputs in [s_j, s_{j+1}) hold the nearer
of the two frames in input time (fraction below 1/2: the left run's S0, else the right run's S1).

A stream is planned as it arrives: with n unknown (None) window k is planned once ``ready`` says enough is known, and the plan
is then the one the whole clip gives."""
import math
from fractions import Fraction

import numpy as np

from . import retime as R
from . import scene as S

BLOCK = 8
DEFAULT_HI, DEFAULT_LO, DEFAULT_FRAC, DEFAULT_MAX_HOLD = 768, 320, Fraction(33, 100), 3
DEFAULTS = (DEFAULT_HI, DEFAULT_LO, DEFAULT_FRAC)


def check_params(hi=DEFAULT_HI, lo=DEFAULT_LO, frac=DEFAULT_FRAC, max_hold=DEFAULT_MAX_HOLD):
    """(hi, lo, frac, max_hold) as (int, int, Fraction, int); ValueError for hi < lo, negative thresholds, frac outside [0, 1]
    or max_hold < 1.  frac is exact: a Fraction, an int or its text ('33/100'); a float is refused."""
    for name, v in (('hi', hi), ('lo', lo), ('max_hold', max_hold)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError('dedup: %s must be an integer, got %r' % (name, v))
    hi, lo, max_hold = int(hi), int(lo), int(max_hold)
    if isinstance(frac, float):
        raise ValueError('dedup: frac must be exact (a Fraction, an int or "N/D"), got the float %r' % frac)
    frac = Fraction(frac)
    if lo < 0 or hi < lo:
        raise ValueError('dedup: thresholds need 0 <= lo <= hi, got hi = %d, lo = %d' % (hi, lo))
    if hi >= 1 << 30:
        raise ValueError('dedup: hi = %d is beyond any block difference' % hi)
    if not 0 <= frac <= 1:
        raise ValueError('dedup: frac %s outside [0, 1]' % frac)
    if max_hold < 1:
        raise ValueError('dedup: max_hold %d below 1' % max_hold)
    return hi, lo, frac, max_hold


def n_blocks(h, w):
    """8x8 blocks of an h x w plane, partial ones included."""
    return -(-h // BLOCK) * -(-w // BLOCK)


def luma_np(payload, h, w, depth=8):
    """The luma plane [h, w] (int64) of a payload: a uint8 array of its bytes (little-endian pairs above 8 bits) or, above 8
    bits, a uint16 array of its samples."""
    a = np.asarray(payload)
    if depth > 8:
        a = a.reshape(-1).view('<u2') if a.dtype == np.uint8 else a.astype(np.uint16, copy=False).reshape(-1)
    elif a.dtype != np.uint8:
        raise ValueError('luma_np: an 8-bit payload is a uint8 array, got %s' % a.dtype)
    a = a.reshape(-1)
    if a.size < h * w:
        raise ValueError('luma_np: %d samples for a %dx%d plane' % (a.size, h, w))
    return a[:h * w].reshape(h, w).astype(np.int64)


def block_sads_np(a, b, h, w, depth=8):
    """(SAD, area) of every block, int64 arrays [ceil(h/8), ceil(w/8)]."""
    d = np.abs(luma_np(a, h, w, depth) - luma_np(b, h, w, depth))
    nby, nbx = -(-h // BLOCK), -(-w // BLOCK)
    pad = np.zeros((nby * BLOCK, nbx * BLOCK), np.int64)
    pad[:h, :w] = d
    sads = pad.reshape(nby, BLOCK, nbx, BLOCK).sum(axis=(1, 3))
    bh = np.minimum(BLOCK, h - BLOCK * np.arange(nby, dtype=np.int64))
    bw = np.minimum(BLOCK, w - BLOCK * np.arange(nbx, dtype=np.int64))
    return sads, bh[:, None] * bw[None, :]


def block_counts_np(a, b, h, w, depth=8, hi=DEFAULT_HI, lo=DEFAULT_LO):
    """(hot, warm): the blocks of payload a against payload b with 64*SAD > hi*s*area, and with 64*SAD > lo*s*area."""
    sads, area = block_sads_np(a, b, h, w, depth)
    s = 1 << (depth - 8)
    return int((64 * sads > hi * s * area).sum()), int((64 * sads > lo * s * area).sum())


def is_repeat(hot, warm, blocks, frac=DEFAULT_FRAC):
    """No hot block and warm <= frac * blocks, as an integer comparison."""
    frac = Fraction(frac)
    return hot == 0 and warm * frac.denominator <= frac.numerator * blocks


class Detector:
    """Kept or repeat, as the frames of a stream arrive in order.  ``forced()``: is the next frame kept whatever it scores
    (frame 0; the frame after ``max_hold`` repeats)?  ``push(i, counts)``: frame i = ``next`` scored (hot, warm) against the
    last kept frame (None when forced) -> was it kept.  ``kept``: the input indices (= times) of the kept frames, ``dups``:
    those of the repeats."""

    def __init__(self, h, w, hi=DEFAULT_HI, lo=DEFAULT_LO, frac=DEFAULT_FRAC, max_hold=DEFAULT_MAX_HOLD):
        self.hi, self.lo, self.frac, self.max_hold = check_params(hi, lo, frac, max_hold)
        self.blocks = n_blocks(h, w)
        self.kept, self.dups, self.next, self.run = [], [], 0, 0

    def forced(self):
        return self.next == 0 or self.run >= self.max_hold

    def push(self, i, counts=None):
        if i != self.next:
            raise RuntimeError('cadence.Detector: frame %d pushed where frame %d was due' % (i, self.next))
        if counts is None and not self.forced():
            raise RuntimeError('cadence.Detector: frame %d needs its block counts' % i)
        keep = self.forced() or not is_repeat(counts[0], counts[1], self.blocks, self.frac)
        if keep:
            self.kept.append(i)
            self.run = 0
        else:
            self.dups.append(i)
            self.run += 1
        self.next = i + 1
        return keep


def kept_of(payloads, h, w, depth=8, hi=DEFAULT_HI, lo=DEFAULT_LO, frac=DEFAULT_FRAC, max_hold=DEFAULT_MAX_HOLD):
    """The input indices of the kept frames of a whole clip (a list of payloads), on the host."""
    det = Detector(h, w, hi, lo, frac, max_hold)
    for i, p in enumerate(payloads):
        det.push(i, None if det.forced() else block_counts_np(p, payloads[det.kept[-1]], h, w, depth, det.hi, det.lo))
    return det.kept


# ---- the timeline ---------------------------------------------------------------------------------------------------
def _first_at(x, r, full_length):
    """Smallest output index i >= 0 with tau_i >= x."""
    return max(math.ceil((Fraction(x) - (0 if full_length else 1)) * r), 0)


def ready(k, s, seen, n=None, full_length=False):
    """Can window k be planned?  s: the times of the kept frames found so far, ``seen``: input frames known to exist, n: the
    input's length once its end was seen (s is then complete).  Before the end: B2 must be known, and on the reference's
    timeline input frame s_{k+2} + 2 must exist (then tau = s_{k+2} is not the stream's last output)."""
    if n is not None:
        return True
    return len(s) > k + 3 and (full_length or seen >= s[k + 2] + 3)


def _outputs(k, r, s, n, full_length):
    """[(output index, kind, exact fraction of the way from B0 to B1, None for S1)] of window k."""
    r, m = Fraction(r), len(s)
    total = R.n_output_frames(n, r, full_length) if n is not None else None
    if k == -2:
        if n is None or m != 1:
            raise ValueError('cadence: window -2 is the one window of a clip with one kept frame')
        return [(i, R.S1, None) for i in range(total)]
    j0, j1 = k + 1, k + 2
    if j0 < 0 or j1 >= m:
        raise IndexError('cadence: window %d of %d kept frames' % (k, m))
    a, b = s[j0], s[j1]
    base = 0 if full_length else 1
    lo, hi = _first_at(a, r, full_length), _first_at(b, r, full_length)
    if total is not None:
        hi = min(hi, total)
    out = []
    for i in range(lo, hi):
        x = Fraction(i) / r + base - a
        if x == 0 and not full_length and n is not None and a == n - 2:
            continue                                    # the S1 of the window that ends here
        out.append((i, R.S0 if x == 0 else R.ST, x / (b - a)))
    if n is not None:
        if j1 == m - 1:                                 # the last window holds its S1 to the end
            out += [(i, R.S1, None) for i in range(min(_first_at(b, r, full_length), total), total)]
        elif not full_length and b == n - 2 and ((n - 3) * r).denominator == 1 and (n - 3) * r < total:
            out.append((int((n - 3) * r), R.S1, None))
    return out


def window_outputs(k, r, s, n=None, full_length=False):
    """[(output index i, kind, t)] of window k in stream order, as ``retime.window_outputs``: t the float32 value (a Python
    float) for St, None for S0 / S1.  s, n: as ``ready``, which must hold.  Empty for a window that does not exist."""
    return [(i, kind, R.float32_of(x) if kind == R.ST else None) for i, kind, x in _outputs(k, r, s, n, full_length)]


def window_plan(k, r, s, n=None, full_length=False):
    """(T_k, [(output index, kind, instant index)]) as ``retime.window_plan``: the distinct t values in increasing order
    (t = 1/2 alone when the window has no St output); S0 / S1 come from instant 0."""
    outs = window_outputs(k, r, s, n, full_length)
    ts = sorted({t for _, kind, t in outs if kind == R.ST}) or [0.5]
    pos = {t: j for j, t in enumerate(ts)}
    return ts, [(i, kind, pos[t] if kind == R.ST else 0) for i, kind, t in outs]


def _cuts(is_cut, s, n):
    """is_cut over kept indices with the ends of the kept sequence as cuts (the end only once it is known)."""
    return S.with_sentinels(is_cut if is_cut is not None else (lambda j: False), len(s) if n is not None else None)


def window_tuple(k, s, n=None, is_cut=None):
    """(B-1, B0, B1, B2), kept indices, of window k when it is not a cut window."""
    return (0, 0, 0, 0) if k < -1 else S.inner_tuple(k, _cuts(is_cut, s, n))


def is_cut_window(k, is_cut):
    return k >= -1 and is_cut is not None and is_cut(k + 2)


def window_runs(k, r, s, n=None, is_cut=None, full_length=False):
    """What window k runs: (runs, outs) as ``scene.window_runs``.  runs = [((B-1, B0, B1, B2) kept indices, instants)], outs =
    [(output index, run, kind, instant index)] in stream order.  A window of more than ``retime.max_instants(r)`` instants
    is several runs of at most that many on one tuple (S0 and S1 come from the first); a cut window is the two runs of
    ``scene.cut_runs`` at t = 1/2."""
    if is_cut_window(k, is_cut):
        left, right = S.cut_runs(k, _cuts(is_cut, s, n))
        outs = [(i, 0, R.S0, 0) if kind == R.S0 or (kind == R.ST and x < S.HALF) else (i, 1, R.S1, 0)
                for i, kind, x in _outputs(k, r, s, n, full_length)]
        return [(left, [0.5]), (right, [0.5])], outs
    ts, plan = window_plan(k, r, s, n, full_length)
    J = R.max_instants(r)
    tup = window_tuple(k, s, n, is_cut)
    runs = [(tup, ts[c:c + J]) for c in range(0, len(ts), J)]
    return runs, [(i, p // J, kind, p % J) if kind == R.ST else (i, 0, kind, 0) for i, kind, p in plan]


def windows(s, n, full_length=False, r=1):
    """The windows of a whole clip (s complete, n its length), in order: those that own an output."""
    if not s:
        return []
    if len(s) == 1:
        return [-2] if R.n_output_frames(n, r, full_length) > 0 else []
    return [k for k in range(-1, len(s) - 2) if _outputs(k, r, s, n, full_length)]


def max_window_instants(r, max_hold):
    """Upper bound of the outputs (so of the instants) a window owns between its B0 and B1: kept frames are at most max_hold + 1
    apart.  The last window's hold (the last kept frame and the repeats after it) is at most as many again."""
    return math.ceil((max_hold + 1) * Fraction(r))


def max_window_runs(r, max_hold):
    """Upper bound of the runs ``window_runs`` gives one window that is not a cut window."""
    return -(-max_window_instants(r, max_hold) // R.max_instants(r))
