"""Temporal denoising of the Y4M video path in front of the network (``python -m demfi_amd.video --denoise [A[:B]] [--denoise-radius R]``):
DV, 576i / 480i captures and telecined broadcasts are noisy, a deblurring network sharpens whatever it is shown, and noise that differs
from frame to frame is motion that is not there.  Pure Python / numpy; the one module that knows the definition.

For every stored sample position p of a payload (all planes, one flat array of bytes, or of little-endian 16-bit samples), with c frame
f's sample:

    sum, n = c, 1
    for side in (-1, +1):
        acc = 0
        for j in 1 .. R:
            g = f + side * j * step
            if frame g is absent: break          # outside the input
            d = |x_g[p] - c| ; acc += d
            if d > A_d or acc > B_d: break
            sum += x_g[p] ; n += 1
    out[p] = (2 * sum + n) // (2 * n)

Serial adaptive temporal averaging, the idea of ffmpeg's ``atadenoise`` in its serial mode: each side walks outward on its own, stops for
good at the first sample that differs from the centre by more than A or brings the side's accumulated difference above B, and never skips
a frame.  A and B are given at the 8-bit scale (0 <= A <= B <= 255; defaults 5:10, atadenoise's 0.02 / 0.04 of the peak, rounded; A alone
means A:2A) and one pair serves every plane; at the working depth d, A_d = A << (d - 8) and B_d = B << (d - 8).  R, the frames on each
side, is 1 .. 3 (default 2), so n <= 7.  ``step`` is 1 for progressive frames; behind the bob of ``--deinterlace`` it is 2: frame f is
field f, its neighbours are the fields of the same parity f +- 2, f +- 4, ..., so kept rows are compared with kept rows and rebuilt rows
with rebuilt rows of the same parity.

What follows from the rule: A = 0 is the identity (only equal samples are averaged); a clip constant in time comes back byte for byte;
every output lies between the least and the greatest sample that went into it; a difference above A never bleeds in, so moving edges and
cuts are left alone; an output frame depends on the input frames f - R step .. f + R step only.

``denoise_payload_np`` is the definition the kernel (csrc/denoise.hip, ``demfi_payload_denoise``) is held to; the kernel divides by
multiplying with ``magic(n)``, exact over its whole input range (tests/test_denoise.py walks every n and every sum).  Not offered: spatial
filtering, separate chroma thresholds, motion-compensated averaging, stopping at detected cuts (the thresholds do that per sample),
numeric equality with ffmpeg's ``atadenoise``.
"""
import re

import numpy as np

DEFAULT_A, DEFAULT_B, DEFAULT_RADIUS, MAX_RADIUS = 5, 10, 2, 3
DEFAULTS = (DEFAULT_A, DEFAULT_B)
_PAIR = re.compile(r'([0-9]+)(?::([0-9]+))?')


def check_params(a=DEFAULT_A, b=None, radius=None):
    """(A, B, R) checked: integers with 0 <= A <= B <= 255 (``b`` None: min(2 A, 255)) and 1 <= R <= ``MAX_RADIUS`` (None: the default)."""
    radius = DEFAULT_RADIUS if radius is None else radius
    for name, v in (('A', a), ('B', b), ('radius', radius)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError('denoise: %s must be an integer, got %r' % (name, v))
    if not 0 <= a <= 255:
        raise ValueError('denoise: the threshold A = %d lies outside 0 .. 255 (8-bit steps)' % a)
    b = min(2 * a, 255) if b is None else b
    if not a <= b <= 255:
        raise ValueError('denoise: the thresholds need 0 <= A <= B <= 255 (8-bit steps), got A = %d, B = %d' % (a, b))
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError('denoise: the radius must be 1 .. %d frames on each side, got %d' % (MAX_RADIUS, radius))
    return int(a), int(b), int(radius)


def parse_denoise(text):
    """``5`` / ``5:10`` -> (A, B) of ``--denoise`` (A alone: A:2A, at most 255); ValueError for anything else."""
    m = _PAIR.fullmatch(str(text).strip())
    if not m:
        raise ValueError('denoise %r: expected A or A:B, integers in 8-bit steps with 0 <= A <= B <= 255' % (text,))
    return check_params(int(m.group(1)), int(m.group(2)) if m.group(2) is not None else None)[:2]


def thresholds(depth, a, b):
    """(A_d, B_d): the thresholds at ``depth`` bits, A << (depth - 8) and B << (depth - 8)."""
    if depth not in (8, 10, 12, 14, 16):
        raise ValueError('denoise: depth %r' % (depth,))
    a, b, _ = check_params(a, b)
    return a << (depth - 8), b << (depth - 8)


def reach(radius, fields=False):
    """R step: how far the frames a denoised frame reads lie from it; step = 2 over the fields of a bobbed stream (``fields``)."""
    return radius * (2 if fields else 1)


def neighbours(f, radius, step, has):
    """The 2 R + 1 frames f - R step, .., f, .., f + R step in that order, None for one the input does not have (``has(g)`` for g >= 0)
    and for every frame beyond such a one on its side: the walk ends there."""
    out = [f] * (2 * radius + 1)
    for side in (-1, 1):
        alive = True
        for j in range(1, radius + 1):
            g = f + side * j * step
            alive = alive and g >= 0 and bool(has(g))
            out[radius + side * j] = g if alive else None
    return out


def denoise_payload_np(cands, depth, a, b):
    """The denoised payload of the centre of ``cands``: 2 R + 1 payloads (1-D uint8 / uint16 arrays of samples) in frame order, None for
    an absent one, the centre present; ``a``, ``b`` at the 8-bit scale.  The definition."""
    if len(cands) not in (3, 5, 7) or cands[len(cands) // 2] is None:
        raise ValueError('denoise_payload_np: 3, 5 or 7 payloads with the centre present')
    r, (ad, bd) = len(cands) // 2, thresholds(depth, a, b)
    c = np.asarray(cands[r]).astype(np.int64)
    total, n = c.copy(), np.ones(c.shape, np.int64)
    for side in (-1, 1):
        acc, alive = np.zeros(c.shape, np.int64), np.ones(c.shape, bool)
        for j in range(1, r + 1):
            if cands[r + side * j] is None:
                break
            x = np.asarray(cands[r + side * j]).astype(np.int64)
            d = np.abs(x - c)
            acc += d
            alive &= (d <= ad) & (acc <= bd)
            total += np.where(alive, x, 0)
            n += alive
    return ((2 * total + n) // (2 * n)).astype(np.asarray(cands[r]).dtype)


def denoise_stream_np(pays, depth, a, b, radius, step=1):
    """Every payload of the stream ``pays`` denoised from the stream as it came in (never from denoised neighbours)."""
    a, b, radius = check_params(a, b, radius)
    return [denoise_payload_np([None if g is None else pays[g] for g in neighbours(f, radius, step, lambda g: g < len(pays))], depth, a, b)
            for f in range(len(pays))]


MAX_COUNT = 2 * MAX_RADIUS + 1


def magic(n):
    """The 32-bit multiplier M of the kernel's division by 2 n: (v * M) >> 32 == v // (2 n) for every v = 2 sum + n it meets, n <=
    ``MAX_COUNT`` and sum <= n * 65535 (v < 2^20).  M = 2^32 // (2 n) + 1: M * 2 n exceeds 2^32 by at most 2 n <= 14, so the product is off
    by less than v * 14 / 2^32 < 1 / (2 n) quotient steps; tests/test_denoise.py walks the whole range."""
    if not 1 <= n <= MAX_COUNT:
        raise ValueError('magic: n = %r outside 1 .. %d' % (n, MAX_COUNT))
    return (1 << 32) // (2 * n) + 1


MAGIC = tuple(magic(n) for n in range(1, MAX_COUNT + 1))     # csrc/denoise.hip carries the same seven constants
