"""Spatial denoising of the Y4M video path in front of the network (``python -m demfi_amd.video --nlmeans [S[:P[:R]]]``): the ingest answers
block edges (``--deblock``), ringing (``--dering``), banding (``--deband``) and noise that stands still (``--denoise``, purely temporal: each
side of its walk stops at the first difference above A, so on a moving object, a pan or a zoom every sample keeps its grain).  Those are the
samples the flow estimator works on -- noise that differs from frame to frame is motion that is not there -- and the network sharpens that
noise with the rest.  This stage is the answer for noise on anything that moves: a non-local-means filter within the frame, directly behind
the deringing filter and in front of the debander (noise hides bands and denoising uncovers them, so ``--deband`` sees the cleaned samples).
Pure Python / numpy; the one module that knows the rule.

The rule is non-local means in exact integers, on every plane as a plane in its own right.  S (strength, 0 .. 16) is in 8-bit steps, P
(patch radius, 1 .. 3) and R (search radius, 1 .. 7) in samples; one triple serves every plane; the default 3:2:5 has NOT been tuned against
this network; S alone means S:2:5; S = 0 is the identity.  For a plane of rows x cols at depth d, with s = d - 8, b = min(s, 4),
np_ = (2P + 1)^2 and K = 1024, every read from the plane as it was before the stage:

    u(x, y) = the sample at column clamp(x, 0, cols - 1), row clamp(y, 0, rows - 1): patches replicate the edge
    q(t) = min(|t| >> (s - b), 4095): differences are taken at 12 bits of precision at most.  Legal samples never reach the min; it is
        there so that D < 2^30 holds for any 16 stored bits (49 * 4095^2)
    for the sample c = u(x, y) and every offset (i, j), |i|, |j| <= R, whose candidate position (x + i, y + j) lies INSIDE the plane
    (others are skipped, as in ``dering``):
        D = sum over |a|, |e| <= P of q(u(x + a, y + e) - u(x + i + a, y + j + e))^2
        w = T[min(D >> g, K - 1)], v = u(x + i, y + j)      (the centre is a candidate like any other: D = 0, w = 256)
    out = c + (2 sum(w (v - c)) + W) // (2 W), W = sum(w) >= 256: the weighted mean rounded to nearest, ties up

The table T and the shift g are ``weight_table(depth, S, P)``, built on the host: g is the least g >= 0 with (K - 1) << g >=
ln(512) np_ 4^b S^2 and T[k] = floor(256 exp(-(k << g) / (np_ 4^b S^2)) + 0.5), so T[0] = 256 and T[K - 1] = 0.  The kernel computes no
exponential: it receives the table and g, from the same function.

What follows: out lies between the least and the greatest candidate with w > 0 (no clip is needed, a legal sample stays legal); a constant
plane stays constant; a candidate whose patch differs by more than the table's reach contributes nothing, so a hard edge is not seen
across; an output depends on the (2 (R + P) + 1)^2 inputs around it and on nothing else.  Under ``--deinterlace`` each field of each plane
is a plane of its own (``deblock.plane_table``; its two phase columns are carried and ignored).

The kernel's arithmetic (csrc/nlmeans.hip).  out = (2 sum(w v) + W) // (2 W) is the same integer (c is one), and sum(w v) <= 225 * 256 *
65535 < 2^32 at every depth, so the kernel keeps W and sum(w v) as unsigned 32-bit sums and divides once: ``kernel_quotient`` is the host
restatement.  The signed numerator 2 sum(w (v - c)) + W fits int32 up to 14 bits and not at 16 for the tables the entry point takes (an
all-256 table reaches the bound); under ``weight_table``'s own tables it stays within int32 even at 16 bits, because a candidate's own
difference is part of its patch distance (``accumulator_bounds``).

The reach of the filter (``profiles/nlmeans.md``).  On a 48 x 64 plane, a ramp of 2 codes a column plus a step of 80 codes between rows 24
and 25, with Gaussian noise of 3 codes of 8 bits, 3:2:5 brings the rms error to 0.44 .. 0.47 of the input's at 8 bits and 0.42 .. 0.45 at
10.  On the clean plane every sample more than 10 from a border and not beside the step comes back exactly; the rest deviate by at most 1
code (8 bits) or 6 (10 bits): a window cut off by a border or an edge is lopsided, so a ramp next to one is biased.  At 16:3:7 the clean
10-bit plane deviates by up to 31 codes: a high S costs texture.

``nlmeans_payload_np`` is the definition the kernel (``demfi_payload_nlmeans``) is held to, byte for byte.  Not offered: separate luma /
chroma strengths; a noise estimate that sets S; temporal or motion-compensated search (that remains ``--denoise``'s side); P above 3 or R
above 7; subtraction of the noise variance from D; numeric equality with ffmpeg's ``nlmeans``; ``demfi_amd.clip``; decisions of ``--ivtc`` /
``--crop auto`` on filtered samples (they decide in front, on the input's own).
"""
import math
import re

import numpy as np

from . import y4m
from .deblock import plane_table

DEFAULT_S, DEFAULT_P, DEFAULT_R = 3, 2, 5
DEFAULTS = (DEFAULT_S, DEFAULT_P, DEFAULT_R)
MAX_S, MIN_P, MAX_P, MIN_R, MAX_R = 16, 1, 3, 1, 7
K = 1024                                             # entries of the weight table
UNIT = 256                                           # the weight of a patch that does not differ
MAX_Q = 4095                                         # a difference at 12 bits
MAX_W = (2 * MAX_R + 1) ** 2 * UNIT                  # 57600
_TRIPLE = re.compile(r'([0-9]+)(?::([0-9]+)(?::([0-9]+))?)?')


def check_params(s=DEFAULT_S, p=None, r=None):
    """(S, P, R) checked: integers with 0 <= S <= 16, 1 <= P <= 3 and 1 <= R <= 7 (``p`` None: 2, ``r`` None: 5)."""
    for name, v in (('S', s), ('P', p), ('R', r)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError('nlmeans: %s must be an integer, got %r' % (name, v))
    if not 0 <= s <= MAX_S:
        raise ValueError('nlmeans: the strength S = %d lies outside 0 .. %d (8-bit steps)' % (s, MAX_S))
    p, r = DEFAULT_P if p is None else p, DEFAULT_R if r is None else r
    if not MIN_P <= p <= MAX_P:
        raise ValueError('nlmeans: the patch radius P = %d lies outside %d .. %d (samples)' % (p, MIN_P, MAX_P))
    if not MIN_R <= r <= MAX_R:
        raise ValueError('nlmeans: the search radius R = %d lies outside %d .. %d (samples)' % (r, MIN_R, MAX_R))
    return int(s), int(p), int(r)


def parse_nlmeans(text):
    """``3`` / ``3:2`` / ``3:2:5`` -> (S, P, R) of ``--nlmeans`` (S alone: S:2:5); ValueError for anything else."""
    m = _TRIPLE.fullmatch(str(text).strip())
    if not m:
        raise ValueError('nlmeans %r: expected S, S:P or S:P:R, integers with 0 <= S <= %d (8-bit steps), %d <= P <= %d and %d <= R <= %d '
                         '(samples)' % (text, MAX_S, MIN_P, MAX_P, MIN_R, MAX_R))
    return check_params(int(m.group(1)), *(int(v) if v is not None else None for v in m.group(2, 3)))


def _scale(depth):
    """(s - b, 4^b) at ``depth``: the shift of a difference and the square of the step of 8 bits at the precision kept."""
    if depth not in y4m.DEPTHS:
        raise ValueError('nlmeans: depth %r' % (depth,))
    s = depth - 8
    b = min(s, 4)
    return s - b, 4 ** b


def weight_table(depth, s=DEFAULT_S, p=None):
    """(T, g): the K weights as uint16 and the shift of a patch distance D; w = T[min(D >> g, K - 1)].  S >= 1."""
    s, p, _ = check_params(s, p)
    if s == 0:
        raise ValueError('weight_table: S = 0 has no table')
    h2 = (2 * p + 1) ** 2 * _scale(depth)[1] * s * s
    g = 0
    while ((K - 1) << g) < math.log(512.0) * h2:
        g += 1
    t = np.floor(UNIT * np.exp(-(np.arange(K, dtype=np.float64) * float(1 << g)) / h2) + 0.5).astype(np.uint16)
    return t, g


def check_table(table, shift):
    """(T as int64 [K], g) of a weight table the entry point takes: K entries, T[0] = 256, none above 256, none above the one before,
    0 <= g <= 31.  ``weight_table`` gives such tables; an all-256 table is a box mean, one that is 0 behind T[0] the identity."""
    t = np.asarray(table).astype(np.int64).reshape(-1)
    if t.size != K or t[0] != UNIT or t.min() < 0 or t.max() > UNIT or (np.diff(t) > 0).any() or not 0 <= int(shift) <= 31:
        raise ValueError('nlmeans: a table of %d weights from 256 down, never increasing, and a shift of 0 .. 31' % K)
    return t, int(shift)


def accumulator_bounds(depth=16, s=MAX_S, p=MAX_P, r=MAX_R):
    """What the sums can reach over every plane of legal samples at ``depth``, as Python ints, and which of them fit 32 bits.
    ``D`` <= (2P + 1)^2 * 4095^2 (< 2^30 always).  ``W`` <= (2R + 1)^2 * 256.  ``wv`` = sum(w v) <= (2R + 1)^2 * 256 * peak, the kernel's
    sum: it fits uint32 at every depth.  ``numerator`` = |2 sum(w (v - c)) + W| <= 2 ((2R + 1)^2 - 1) * 256 * peak + W for ANY table the
    entry point takes (the centre adds nothing to the sum; an all-256 table reaches it): at the widest window it fits int32 up to 14 bits
    and not at 16, so the kernel never forms it.  ``numerator_rule``: the same under the tables of ``weight_table(depth, s, p)``, where a
    candidate's own difference t is part of its patch distance, D >= q(t)^2, so w |t| <= max over q of T[min(q^2 >> g, K - 1)] * (the
    greatest |t| with that q): far less, and within int32 even at 16 bits."""
    s, p, r = check_params(s, p, r)
    peak = (1 << depth) - 1
    sh = _scale(depth)[0]
    qmax = min(peak >> sh, MAX_Q)
    n = (2 * r + 1) ** 2
    d, w = (2 * p + 1) ** 2 * qmax * qmax, n * UNIT
    num, wv = 2 * (n - 1) * UNIT * peak + w, n * UNIT * peak
    out = dict(D=d, W=w, numerator=num, wv=wv, D_fits_int32=d < 2 ** 31, numerator_fits_int32=num < 2 ** 31, wv_fits_uint32=wv < 2 ** 32)
    if s:
        tab, g = weight_table(depth, s, p)
        each = max(int(tab[min((q * q) >> g, K - 1)]) * min(((q + 1) << sh) - 1, peak) for q in range(qmax + 1))
        out.update(numerator_rule=2 * (n - 1) * each + w, numerator_rule_fits_int32=2 * (n - 1) * each + w < 2 ** 31)
    return out


def kernel_quotient(wv, w):
    """The kernel's quotient restated on the host: out = (2 wv + W) // (2 W) from the unsigned 32-bit sums wv = sum(w v) and W, as one
    unsigned 32-bit division and a comparison of the remainder (no 33-bit numerator is ever formed): q = wv // W, r = wv - q W,
    out = q + (2 r >= W).  Arrays or ints; every intermediate is asserted to fit 32 bits."""
    wv, w = np.asarray(wv, dtype=np.uint64), np.asarray(w, dtype=np.uint64)
    if wv.size and (int(wv.max()) >= 2 ** 32 or int(w.max()) > MAX_W or int(w.min()) < 1):
        raise ValueError('kernel_quotient: sums outside 32 bits')
    q = wv // w
    r = wv - q * w                                       # < W <= 57600: 2 r fits
    return (q + (2 * r >= w)).astype(np.int64)


def _filter(p, depth, S, P, R, table=None):
    """The plane ``p`` [rows, cols] (int64) filtered at S >= 1 (``table``: (T, g) in place of ``weight_table``'s, whatever S), and what
    ``plane_cases`` tells."""
    rows, cols = p.shape
    tab, g = check_table(*(weight_table(depth, S, P) if table is None else table))
    sh, H, n = _scale(depth)[0], R + P, 2 * P + 1
    pad = np.pad(p, H, mode='edge')
    ys, xs = np.arange(rows), np.arange(cols)
    a = pad[R:R + rows + 2 * P, R:R + cols + 2 * P]
    W, num, wv, live, skipped = (np.zeros_like(p) for _ in range(5))
    met = np.zeros(K, dtype=bool)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            q = np.minimum(np.abs(a - pad[R + j:R + j + rows + 2 * P, R + i:R + i + cols + 2 * P]) >> sh, MAX_Q)
            ii = np.zeros((rows + 2 * P + 1, cols + 2 * P + 1), dtype=np.int64)
            ii[1:, 1:] = (q * q).cumsum(0).cumsum(1)
            D = ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]
            idx = np.minimum(D >> g, K - 1)
            inside = ((ys + j >= 0) & (ys + j < rows))[:, None] & ((xs + i >= 0) & (xs + i < cols))[None, :]
            w = np.where(inside, tab[idx], 0)
            v = pad[H + j:H + j + rows, H + i:H + i + cols]
            W += w
            num += w * (v - p)
            wv += w * v
            live += w > 0
            skipped += ~inside
            met[idx[inside]] = True
    out = p + (2 * num + W) // (2 * W)
    clamped = np.zeros(p.shape, dtype=np.uint8)          # bit 0: a patch column left of the plane, 1: right, 2: a row above, 3: below
    clamped |= np.where(xs - H < 0, 1, 0).astype(np.uint8)[None, :] | np.where(xs + H > cols - 1, 2, 0).astype(np.uint8)[None, :]
    clamped |= np.where(ys - H < 0, 4, 0).astype(np.uint8)[:, None] | np.where(ys + H > rows - 1, 8, 0).astype(np.uint8)[:, None]
    return out, dict(W=W, live=live, numerator=2 * num + W, wv=wv, indices=met, clamped=clamped, skipped=skipped, changed=out != p)


def _plane(plane, name):
    src = np.asarray(plane)
    if src.ndim != 2 or not src.size:
        raise ValueError('%s: a [rows, cols] plane, got %s' % (name, src.shape,))
    return src


def nlmeans_plane_np(plane, depth, s=DEFAULT_S, p=None, r=None, table=None):
    """The plane [rows, cols] of samples at ``depth`` filtered, out of place; ``s`` at the 8-bit scale, ``p`` and ``r`` in samples.
    ``table``: None, or (T, g) as the entry point takes them, used in place of ``weight_table(depth, s, p)``."""
    src = _plane(plane, 'nlmeans_plane_np')
    s, p, r = check_params(s, p, r)
    if s == 0 and table is None:
        return src.copy()
    _scale(depth)
    return _filter(src.astype(np.int64), depth, s, p, r, table)[0].astype(src.dtype)


def plane_cases(plane, depth, s=DEFAULT_S, p=None, r=None, table=None):
    """What the rule does on the plane.  Per sample: ``W`` (the sum of the weights), ``live`` (the candidates with w > 0), ``numerator``
    (2 sum(w (v - c)) + W), ``wv`` (sum(w v), the kernel's sum), ``skipped`` (the candidates outside the plane), ``clamped`` (bits: a patch
    of some candidate reaches left of / right of / above / below the plane: 1, 2, 4, 8) and ``changed`` (out != c); for the plane:
    ``indices``, a bool per table index met by a candidate inside the plane.  S >= 1, or a ``table`` (T, g) of its own."""
    src = _plane(plane, 'plane_cases')
    s, p, r = check_params(s, p, r)
    if s == 0 and table is None:
        raise ValueError('plane_cases: S = 0 has no window')
    return _filter(src.astype(np.int64), depth, s, p, r, table)[1]


def nlmeans_payload_np(payload, h, w, depth, layout, s=DEFAULT_S, p=None, r=None, fields=None, rect=None, table=None):
    """The payload (a 1-D uint8 / uint16 array of the samples of an h x w frame of ``layout``) filtered; ``s`` at the 8-bit scale, ``p`` and
    ``r`` in samples; ``fields``, ``rect``: as for ``deblock.plane_table`` (the phases ``rect`` gives are ignored).  The definition."""
    src = np.asarray(payload)
    if src.ndim != 1 or src.size != y4m.payload_size(h, w, layout):
        raise ValueError('nlmeans_payload_np: a flat payload of %d samples for a %dx%d %s frame, got %s'
                         % (y4m.payload_size(h, w, layout), w, h, layout, src.shape))
    s, p, r = check_params(s, p, r)
    out = src.copy()
    for first, rows, cols, pitch, _, _ in plane_table(h, w, layout, fields, rect):
        view = np.lib.stride_tricks.as_strided(src[first:], (rows, cols), (pitch * src.itemsize, src.itemsize))
        dst = np.lib.stride_tricks.as_strided(out[first:], (rows, cols), (pitch * out.itemsize, out.itemsize))
        dst[...] = nlmeans_plane_np(view, depth, s, p, r, table)
    return out


def nlmeans_stream_np(pays, h, w, depth, layout, s=DEFAULT_S, p=None, r=None, fields=None, rect=None):
    """Every payload of the stream ``pays`` filtered; the stage keeps nothing from one payload to the next."""
    s, p, r = check_params(s, p, r)
    return [nlmeans_payload_np(x, h, w, depth, layout, s, p, r, fields, rect) for x in pays]
