"""Debanding of the Y4M video path in front of the network (``python -m demfi_amd.video --deband [T[:R]]``): low-bitrate 8-bit input carries
skies, walls and fades as plateaus one code apart.  The promotion to the working depth (``--work-depth``) is a pure shift and keeps the steps
(4 codes at 10 bits, 16 at 12), a deblurring network sharpens a contour of one code like any other edge, and the egress (``--grain``, the
ordered dither) can only bury what arrives.  ``--deblock`` handles block edges, ``--dering`` ringing; this stage handles the bands, directly
behind the deringing filter, at the working depth.  Pure Python / numpy; the one module that knows the rule.

The rule is a range-limited box mean (Lee's sigma filter with a hard threshold) in exact integers, on every plane as a plane in its own
right.  T (threshold, 0 .. 8) is in 8-bit steps, R (radius, 1 .. 16) in samples; one pair serves every plane; the default 2:16 has NOT been
tuned against this network; T alone means T:16; T = 0 is the identity.  For a sample c at column x, row y of a plane of rows x cols at the
working depth d:

    thr = T << (d - 8)
    rx = min(R, x, cols - 1 - x), ry = min(R, y, rows - 1 - y): the window is clipped SYMMETRICALLY about the sample; it never leaves the
        plane, nothing is clamped or mirrored
    N = the samples v of the plane as it was before the stage at (x + i, y + j), |i| <= rx, |j| <= ry, with |v - c| < thr (c itself is
        one of them: n = |N| >= 1)
    out = (2 sum(N) + n) // (2 n): the mean of the near samples, rounded to nearest, ties up

What follows: |out - c| < thr and out lies between the least and the greatest of N (no clip is needed, a legal sample stays legal); a
constant plane stays constant; every affine plane a x + b y + e comes back exactly, corners and borders included, because N is
point-symmetric about c (what the symmetric clipping buys; an edge-clamped window has no such property); a step of thr or more is an edge
that neither side sees across; rx = ry = 0 (the four corners, a plane with a side of 1) is the identity; an output depends on the
(2R + 1)^2 inputs around it and on nothing else.  Under ``--deinterlace`` each field of each plane is a plane of its own and R counts field
rows (``deblock.plane_table``; its two phase columns are carried and ignored: banding has no grid).

The reach of the filter.  An 8-bit ramp promoted to 10 bits with plateaus 16 to 32 samples wide comes back at 2:16 monotone with steps of at
most 1 code (the input's are 4), at the rounding floor of its true ramp; plateaus of 64 keep a flat middle.  At equal input and working
depth a band of one code rounds back to itself: the switch does its work only with ``--work-depth`` above the input's depth (10 or more on
8-bit input).  Bands narrower than about R / T come back unchanged: every band within the threshold then lies wholly inside the window and
the mean is c.  Fine detail within the threshold is averaged like a band: a higher T costs texture (``profiles/deband.md``).

``deband_payload_np`` is the definition the kernel (csrc/deband.hip, ``demfi_payload_deband``) is held to, byte for byte.  Not offered:
debanding behind ``--denoise`` (noise hides bands and denoising uncovers them, but that stage is deferred and has its own buffer);
randomly placed reference samples in the manner of ``f3kdb`` or ffmpeg's ``deband`` (a fixed random pattern that stands still over moving
content); dither or grain at this stage (``--grain`` is the place); per-plane pairs; a radius above 16; bands narrower than about R / T;
``demfi_amd.clip``; numeric equality with any ffmpeg filter.
"""
import re

import numpy as np

from . import y4m
from .deblock import plane_table

DEFAULT_T, DEFAULT_R = 2, 16
DEFAULTS = (DEFAULT_T, DEFAULT_R)
MAX_T, MIN_R, MAX_R = 8, 1, 16
MAX_N = (2 * MAX_R + 1) ** 2                      # 1089 samples in a window at most
_PAIR = re.compile(r'([0-9]+)(?::([0-9]+))?')


def check_params(t=DEFAULT_T, r=None):
    """(T, R) checked: integers with 0 <= T <= 8 and 1 <= R <= 16 (``r`` None: 16)."""
    for name, v in (('T', t), ('R', r)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError('deband: %s must be an integer, got %r' % (name, v))
    if not 0 <= t <= MAX_T:
        raise ValueError('deband: the threshold T = %d lies outside 0 .. %d (8-bit steps)' % (t, MAX_T))
    r = DEFAULT_R if r is None else r
    if not MIN_R <= r <= MAX_R:
        raise ValueError('deband: the radius R = %d lies outside %d .. %d (samples)' % (r, MIN_R, MAX_R))
    return int(t), int(r)


def parse_deband(text):
    """``2`` / ``2:16`` -> (T, R) of ``--deband`` (T alone: T:16); ValueError for anything else."""
    m = _PAIR.fullmatch(str(text).strip())
    if not m:
        raise ValueError('deband %r: expected T or T:R, integers with 0 <= T <= %d (8-bit steps) and %d <= R <= %d (samples)'
                         % (text, MAX_T, MIN_R, MAX_R))
    return check_params(int(m.group(1)), int(m.group(2)) if m.group(2) is not None else None)


def thresholds(depth, t=DEFAULT_T):
    """thr at ``depth`` bits: T << (depth - 8)."""
    if depth not in y4m.DEPTHS:
        raise ValueError('deband: depth %r' % (depth,))
    return check_params(t)[0] << (depth - 8)


def accumulator_bounds(depth=16, t=MAX_T, r=MAX_R):
    """(n, sum, |D|, numerator) at their greatest over every plane of samples of 16 stored bits at ``depth``, T = ``t`` and R = ``r``, as
    Python ints: n <= (2R + 1)^2 (1089); sum(N) <= n * 65535 (< 2^27); in the difference form out = c + (2 D + n) // (2 n) with
    D = sum(v - c), |D| <= n * (thr - 1) (1089 * 2047 < 2^22); the kernel's biased form sums e = v - c + thr - 1 in [0, 2 thr - 2], so its
    numerator 2 sum(e) + n <= n * (4 thr - 3) (< 2^24: exact in a float).  Everything is int32."""
    t, r = check_params(t, r)
    thr = thresholds(depth, t)
    n = (2 * r + 1) ** 2
    return n, n * 65535, n * max(thr - 1, 0), n * max(4 * thr - 3, 1)


def _filter(p, thr, R):
    """The plane ``p`` [rows, cols] (int64) debanded at thr >= 1, and what ``plane_cases`` tells."""
    rows, cols = p.shape
    ys, xs = np.arange(rows), np.arange(cols)
    ry, rx = np.minimum(R, np.minimum(ys, rows - 1 - ys)), np.minimum(R, np.minimum(xs, cols - 1 - xs))
    pad = np.pad(p, R)
    total, n = np.zeros_like(p), np.zeros_like(p)
    for j in range(-int(ry.max()), int(ry.max()) + 1):
        for i in range(-int(rx.max()), int(rx.max()) + 1):
            v = pad[R + j:R + j + rows, R + i:R + i + cols]
            near = (abs(j) <= ry)[:, None] & (abs(i) <= rx)[None, :] & (np.abs(v - p) < thr)
            total += np.where(near, v, 0)
            n += near
    out = (2 * total + n) // (2 * n)
    return out, dict(n=n, rx=np.broadcast_to(rx[None, :], p.shape), ry=np.broadcast_to(ry[:, None], p.shape), changed=out != p,
                     D=total - n * p)


def _plane(plane, name):
    src = np.asarray(plane)
    if src.ndim != 2 or not src.size:
        raise ValueError('%s: a [rows, cols] plane, got %s' % (name, src.shape,))
    return src


def deband_plane_np(plane, depth, t=DEFAULT_T, r=None):
    """The plane [rows, cols] of samples at ``depth`` debanded, out of place; ``t`` at the 8-bit scale, ``r`` in samples."""
    src = _plane(plane, 'deband_plane_np')
    t, r = check_params(t, r)
    if t == 0:
        return src.copy()
    return _filter(src.astype(np.int64), thresholds(depth, t), r)[0].astype(src.dtype)


def plane_cases(plane, depth, t=DEFAULT_T, r=None):
    """What the rule does on the plane, per sample: ``n`` (the near samples), ``rx``, ``ry`` (the clipped window), ``changed`` (out != c)
    and ``D`` (sum(v - c) over N).  T >= 1."""
    src = _plane(plane, 'plane_cases')
    t, r = check_params(t, r)
    if t == 0:
        raise ValueError('plane_cases: T = 0 has no window')
    return _filter(src.astype(np.int64), thresholds(depth, t), r)[1]


def deband_payload_np(payload, h, w, depth, layout, t=DEFAULT_T, r=None, fields=None, rect=None):
    """The payload (a 1-D uint8 / uint16 array of the samples of an h x w frame of ``layout``) debanded; ``t`` at the 8-bit scale, ``r`` in
    samples; ``fields``, ``rect``: as for ``deblock.plane_table`` (the phases ``rect`` gives are ignored).  The definition."""
    src = np.asarray(payload)
    if src.ndim != 1 or src.size != y4m.payload_size(h, w, layout):
        raise ValueError('deband_payload_np: a flat payload of %d samples for a %dx%d %s frame, got %s'
                         % (y4m.payload_size(h, w, layout), w, h, layout, src.shape))
    t, r = check_params(t, r)
    out = src.copy()
    for first, rows, cols, pitch, _, _ in plane_table(h, w, layout, fields, rect):
        view = np.lib.stride_tricks.as_strided(src[first:], (rows, cols), (pitch * src.itemsize, src.itemsize))
        dst = np.lib.stride_tricks.as_strided(out[first:], (rows, cols), (pitch * out.itemsize, out.itemsize))
        dst[...] = deband_plane_np(view, depth, t, r)
    return out


def deband_stream_np(pays, h, w, depth, layout, t=DEFAULT_T, r=None, fields=None, rect=None):
    """Every payload of the stream ``pays`` debanded; the stage keeps nothing from one payload to the next."""
    t, r = check_params(t, r)
    return [deband_payload_np(x, h, w, depth, layout, t, r, fields, rect) for x in pays]
