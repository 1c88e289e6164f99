"""Output frame rate F_out for any rational ratio r = F_out / F_in > 0 of the Y4M video path (``python -m demfi_amd.video --fps``;
r < 1, an output rate below the input's, with ``--downconvert``).

Pure Python over ``fractions.Fraction``.  Input frames are numbered 0 .. n-1 and window k is (B-1, B0, B1, B2) = (k, k+1, k+2,
k+3).  Output frame i sits at tau_i = 1 + i / r, in input frames; the output holds every i with tau_i <= n - 2, so
N_out = floor((n-3) r) + 1 for n >= 4.  Output frame i is
  * S0 (deblurred B0) of window m - 1 when tau_i is an integer m <= n - 3,
  * S1 of the last window when tau_i = n - 2,
  * otherwise St of window k = floor(tau_i) - 1 at t = float32(tau_i - floor(tau_i)) = float32((i q - k p) / p) for r = p / q,
    rounded once from the exact rational.
Window k owns the output indices ceil(k r) .. ceil((k+1) r) - 1 (at least one when r >= 1; possibly none when r < 1: at most
ceil(r) in any case), plus S1 when it is the last window and (n-3) r is an integer.  It runs the instants T_k: the distinct St t
values of its outputs in increasing order, or the single instant t = 1/2 when it has outputs but no St among them (S0 or S1
only).  S0 and S1 come from the window's first instant.  A window that owns no output runs nothing: T_k is empty.

For r = M this is exactly the x M stream of ``y4m``: ``n_output_frames`` / ``output_index`` / ``output_header`` and the t
values of ``harness.t_schedule(M)``.  Everything about window k follows from k and r alone, so a stream is scheduled as it
arrives; whether a window is the last one is the reader's business (``y4m.Frames.is_last``).

Full-length timeline (``full_length=True``, ``python -m demfi_amd.video --full-length``): the output covers the input's whole
timeline.  Output frame i sits at tau_i = i / r, so output 0 is input frame 0, and N_out = ceil(n r) (n M for x M).  Windows
are k = -1 .. n-3; window k interpolates between B0 = k+1 and B1 = k+2 and owns the outputs with tau in [k+1, k+2), i.e. the
indices ceil((k+1) r) .. ceil((k+2) r) - 1.  Output i is S0 when tau_i = k+1, else St at t = float32((i q - (k+1) p) / p).
The last window (k = n-3) also owns tau in [n-2, n): tau = n-1 is its S1 and every tau in (n-1, n) holds that S1.  A one-frame
clip has the single window k = n-3 = -2 (tuple (0, 0, 0, 0), t = 1/2): it owns [0, 1), all of it the S1 hold.  The tuples are
clamped at the clip's ends as if there were a scene cut before frame 0 and after frame n-1 (``scene.with_sentinels``).
"""
import math
import re
from fractions import Fraction

import numpy as np

from . import y4m

S0, ST, S1 = 'S0', 'St', 'S1'
_FPS = re.compile(r'([0-9]+)(?:[/:]([0-9]+))?')


def parse_fps(text):
    """``60`` / ``60000/1001`` / ``60000:1001`` -> Fraction > 0.  Decimals are refused: 59.94 is not 60000/1001."""
    s = str(text).strip()
    m = _FPS.fullmatch(s)
    if not m:
        if re.fullmatch(r'[0-9]*\.[0-9]*', s) and s != '.':
            raise ValueError('frame rate %r: give an exact fraction N/D (for example 60000/1001 for 59.94, 24000/1001 for '
                             '23.976); a decimal is not exact' % s)
        raise ValueError('frame rate %r: expected N or N/D (or N:D) with integers N, D > 0' % s)
    num, den = int(m.group(1)), int(m.group(2) or 1)
    if num == 0 or den == 0:
        raise ValueError('frame rate %r: N and D must be > 0' % s)
    return Fraction(num, den)


MAX_RATIO = 64


def ratio(fps_in, fps_out, down=False):
    """r = F_out / F_in (reduced); ValueError below 1 (unless ``down``: then below 1 / ``MAX_RATIO``) and above ``MAX_RATIO`` (a
    window keeps ceil(r) + 2 frame slots on the GPU)."""
    r = Fraction(fps_out) / Fraction(fps_in)
    if r < 1 and not down:
        raise ValueError('output frame rate %s is below the input rate %s: only F_out >= F_in is supported' % (fps_out, fps_in))
    if r * MAX_RATIO < 1:
        raise ValueError('output frame rate %s is less than 1/%d of the input rate %s' % (fps_out, MAX_RATIO, fps_in))
    if r > MAX_RATIO:
        raise ValueError('output frame rate %s is more than %d times the input rate %s' % (fps_out, MAX_RATIO, fps_in))
    return r


def float32_of(x):
    """The float32 nearest to the rational x in [0, 1) (ties to even), rounded ONCE from the exact value; as a Python float."""
    x = Fraction(x)
    if x == 0:
        return 0.0
    if not 0 < x < 1:
        raise ValueError('t = %s outside [0, 1)' % x)
    e = x.numerator.bit_length() - x.denominator.bit_length()     # 2^e <= x < 2^(e+1) after the fix-up below
    if Fraction(2) ** e > x:
        e -= 1
    s = 23 - max(e, -126)                                          # 24 significant bits (subnormals keep the -149 quantum)
    m, rem = divmod(x.numerator * 2 ** s, x.denominator)
    if 2 * rem > x.denominator or (2 * rem == x.denominator and m & 1):
        m += 1
    v = float(Fraction(m, 2 ** s))
    assert float(np.float32(v)) == v
    return v


def n_output_frames(n_in, r, full_length=False):
    """floor((n-3) r) + 1 for n >= 4 input frames, else 0.  ``full_length``: ceil(n r) for n >= 1."""
    if full_length:
        return math.ceil(n_in * Fraction(r)) if n_in >= 1 else 0
    return math.floor((n_in - 3) * Fraction(r)) + 1 if n_in >= 4 else 0


def first_window(n_in, full_length=False):
    """Index of the first window of an n-frame clip: 0; ``full_length``: -1, or -2 = n-3 for a one-frame clip."""
    return min(-1, n_in - 3) if full_length else 0


def n_windows(n_in, full_length=False):
    """Windows of an n-frame clip: n-3 (none below 4 frames); ``full_length``: n-1 for n >= 2, one for n = 1."""
    if full_length:
        return max(n_in - 1, 1) if n_in >= 1 else 0
    return max(n_in - 3, 0)


def first_output(k, r, full_length=False):
    """Stream index of the first output frame owned by window k: ceil(k r); ``full_length``: ceil((k+1) r), 0 for k = -2."""
    if full_length:
        return max(math.ceil((k + 1) * Fraction(r)), 0)
    return math.ceil(k * Fraction(r))


def window_outputs(k, r, last=False, full_length=False):
    """[(output index i, kind, t)] of window k in stream order: kind S0 / St / S1, t the float32 value (a Python float) for St
    and None for S0 / S1.  ``last``: window k is the clip's last one (its S1 is written when (k+1) r is an integer; in
    ``full_length`` mode it also owns tau in [k+2, k+3): S1 and its hold)."""
    r = Fraction(r)
    p, q = r.numerator, r.denominator
    sh = 1 if full_length else 0                                   # full-length: tau_i is one input frame earlier
    out = []
    for i in range(first_output(k, r, full_length), first_output(k + 1, r, full_length)):
        num = i * q - (k + sh) * p                                 # tau_i - (k+1) = num / p, 0 <= num < p
        out.append((i, S0, None) if num == 0 else (i, ST, float32_of(Fraction(num, p))))
    if full_length:
        if last:
            out += [(i, S1, None) for i in range(first_output(k + 1, r, True), first_output(k + 2, r, True))]
    elif last and (k + 1) * r == first_output(k + 1, r):
        out.append((first_output(k + 1, r), S1, None))
    return out


def instants(k, r, full_length=False, last=False):
    """T_k: the float32 t values window k runs, in increasing order: t = 1/2 alone when it has outputs but no St among them, none
    when it owns no output (r < 1 only; ``last``: the S1 and its hold count as the last window's)."""
    outs = window_outputs(k, r, last, full_length)
    ts = sorted({t for _, kind, t in outs if kind == ST})
    return ts or ([0.5] if outs or Fraction(r) >= 1 else [])


def window_plan(k, r, last=False, full_length=False):
    """(T_k, [(output index, kind, instant index)]): window k's instants and, per output in stream order, which instant's St
    it is (S0 / S1: instant 0, the window's first)."""
    outs = window_outputs(k, r, last, full_length)
    ts = instants(k, r, full_length, last)
    pos = {t: j for j, t in enumerate(ts)}
    return ts, [(i, kind, pos[t] if kind == ST else 0) for i, kind, t in outs]


def max_instants(r):
    """Upper bound of |T_k| over all windows: ceil(r) (a window owns at most ceil(r) outputs; 1 for r < 1)."""
    return math.ceil(Fraction(r))


def output_header(hdr, fps_out):
    """Header of the retimed stream: the input's W H, F = F_out (reduced), progressive, A copied, C420jpeg (C420pNN at the input's
    depth above 8 bits; the input's layout and depth for 4:2:2, 4:4:4 and mono), the input's XCOLORRANGE -- the fields of
    ``y4m.output_header``."""
    return y4m.Header(hdr.w, hdr.h, Fraction(fps_out), 'p', hdr.aspect, '420jpeg', hdr.color_range, (),
                      y4m.output_ctag(hdr.depth, hdr.layout), hdr.depth, hdr.layout)


def block_offset(hdr_len, first_window, r, payload, full_length=False):
    """Byte offset in the output file of the first frame of the block of windows starting at ``first_window``; ``payload``:
    the bytes of one payload (``Header.payload``)."""
    return y4m.frame_offset(hdr_len, first_output(first_window, r, full_length), payload)


SCAN_WINDOWS = 1000


def _period_counts(r):
    """|T_k| of the windows of one period (at most ``SCAN_WINDOWS`` of them); 0 for a window that owns no output (r < 1)."""
    r = Fraction(r)
    return [len(instants(k, r)) for k in range(min(r.denominator, SCAN_WINDOWS))]


def padded_slots(r, n_ctx, counts=None):
    """Padded per-t slots over one period (q windows for r = p/q, the schedule repeats after it) when the instants of a window
    run in chunks of n_ctx.  Unusual rates can have periods of millions of windows: at most the first ``SCAN_WINDOWS`` are
    counted, a sample of the same schedule."""
    return sum(-c % n_ctx for c in (counts if counts is not None else _period_counts(r)))


def default_n_ctx(r, fits, largest=8, counts=None, slack=0):
    """The batched plan's n_ctx for ratio r: among 1 .. ``largest`` where ``fits(n_ctx)`` (the workspace fits the GPU), the
    size with the fewest padded slots over one period of the schedule (``padded_slots``); ties go to the larger size.
    ``counts``: the instants per window of a schedule that runs only some of the ratio's instants (``shutter.period_counts``).
    ``slack``: the share of the period's instants that may be padded for the sake of a larger size: the largest size within it
    wins (0, the default: only sizes that pad nothing win that way, which is the rule above).  Window counts of 11 and 8 instants
    pad nothing only at 1, the non-batched plan; an eighth of slack takes 4, which pads one slot in 19.  That the largest size within the
    slack is the fastest, and the eighth a shutter's schedule is given, rest on ONE measurement (profiles/shutter.md: 24 -> 60 at 180
    degrees, 720p, 1.707 s at n_ctx = 1 against 1.324 s at 4), not on a model of what a padded slot and a larger batch cost."""
    counts = counts if counts is not None else _period_counts(r)
    ok = [d for d in range(1, largest + 1) if d == 1 or fits(d)]
    pads = {d: padded_slots(r, d, counts) for d in ok}
    within = [d for d in ok if pads[d] <= slack * sum(counts)]
    return max(within) if within else min(ok, key=lambda d: (pads[d], -d))
