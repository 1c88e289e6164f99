"""Film grain synthesis at the egress of the Y4M video path (``python -m demfi_amd.video --grain S [--grain-size 0|1|2] [--grain-chroma C]
[--grain-curve film|flat] [--grain-seed N]``): ``--denoise`` removes grain on purpose, the network, the shutter mix and the scaler smooth
what is left, so the written picture is cleaner than any camera original and its gradients band.  The stage behind the encode and in front
of the weave and the requantisation adds synthetic grain to every progressive payload.  Pure Python / numpy and integers; the one module
that knows the rule.

**Switches.**  S: the grain's standard deviation in 8-bit code values at the curve's peak, a decimal quantised to sixteenths (S16 =
round(16 S)), 0 <= S <= 8.  ``--grain-size`` r in {0, 1, 2} (default 1): how coarse.  C in [0, 1], sixteenths, default 0.5: the chroma
strength relative to luma, 0 is luma only.  The curve: ``film`` (default) or ``flat``.  The seed: a uint32, default 0.  ``params`` below
is the tuple (S16, r, C16, curve, seed).

**Hash.**  ``mix32(x)`` on uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.

**Key** of plane p (0 .. 2) of written progressive frame n (0-based, in the order the stage sees them over the whole run):
key = mix32((seed + 0x9E3779B9 (4 n + p + 1)) mod 2^32).

**White cell.**  white(key, X, Y) = b0 + b1 + b2 + b3 - 510 over the four bytes of u = mix32(key ^ mix32((Y << 16) | X)): mean exactly 0,
variance exactly 21845 = 4 (256^2 - 1) / 12.  Sample (x, y) of a plane sits at cell (x + 2, y + 2), so the neighbours a filter needs
always exist; planes wider or taller than ``MAX_SIDE`` = 65531 are refused.

**Grain field.**  F(x, y) = sum over i, j in -r .. r of c[i] c[j] white(key, x + 2 + i, y + 2 + j) with the binomial taps c = [1],
[1, 2, 1], [1, 4, 6, 4, 1]; Var F = 21845 N_r^2 with N_r = sum c^2 = 1, 6, 70.

**Gain tables**, luma and chroma, 256 entries each, built once on the host:
G[c] = floor(2^16 2^(d - 8) (S16 / 16) k curve8[c] / 256 / (sqrt(21845) N_r) + 1/2), d the working depth, k = 1 for luma and C16 / 16 for
chroma.  ``curve8`` is a Q8 integer table: 256 everywhere for ``flat``; round(256 (1/4 + 3 t (1 - t))) for ``film``, which peaks in the
midtones and falls to a quarter at black and white, t the position of the 8-bit luma code in the written range: clip((c - 16) / 219, 0, 1)
for limited range, c / 255 for full range.

**The rule**, for stored sample v of a plane:  delta = (F G[c] + 2^15) >> 16 (an arithmetic, flooring shift) with c = min(L >> (d - 8),
255), L the frame's own luma before any grain: v itself for luma, for the chroma sample (x, y) the luma sample at (min(x sx, w - 1),
min(y sy, h - 1)), sx, sy the layout's subsampling factors.  out = clip(v + delta, min(lo, v), max(hi, v)), lo and hi the nominal range
of the range written: limited 16 << (d - 8) .. 235 << (d - 8) for luma and .. 240 << (d - 8) for chroma, full 0 .. peak.  A zero delta
never moves a sample, super-whites and out-of-range 16-bit stored values are not pulled in, and grain never pushes a legal sample out
of the legal range.

What follows from the rule: S = 0 is the identity; the output depends on (seed, n, plane, x, y, v, L) only, so batch size never shows;
equal seeds give equal bytes; a mono layout gets luma grain only (and so does C = 0).

``grain_payload_np`` is the definition the kernel (csrc/grain.hip, ``demfi_payload_grain``) is held to, byte for byte.
``accumulator_bounds`` states how wide F G + 2^15 gets: the cap S <= 8 keeps it below 2^31 for every depth and size.

Not offered: measuring the grain that ``--denoise`` removed and matching it, grain that is correlated in time, AR-model grain as in AV1,
per-plane curves, grain in linear light, several ranks, ``demfi_amd.clip``.
"""
import io
import math
from fractions import Fraction

import numpy as np

from . import y4m
from .interlace import plane_shapes

CURVES = ('film', 'flat')
DEFAULT_SIZE, DEFAULT_CHROMA16, DEFAULT_CURVE, DEFAULT_SEED = 1, 8, 'film', 0
MAX_S16, MAX_SIDE = 8 * 16, 65531
TAPS = ((1,), (1, 2, 1), (1, 4, 6, 4, 1))
NORM = (1, 6, 70)                                    # N_r = sum of the squared taps
WHITE_VAR = 21845
GOLDEN = 0x9E3779B9
_M32 = 0xFFFFFFFF


# ---- switches --------------------------------------------------------------------------------------------------------------
def _sixteenths(text, name, top):
    try:
        if isinstance(text, bool):
            raise ValueError
        q = Fraction(str(text).strip()) if not isinstance(text, (int, float, Fraction)) else Fraction(text)
    except (ValueError, ZeroDivisionError, OverflowError):
        raise ValueError('%s takes a decimal number in 0 .. %d, got %r' % (name, top, text)) from None
    if not 0 <= q <= top:
        raise ValueError('%s: %s lies outside 0 .. %d' % (name, text, top))
    return int(math.floor(q * 16 + Fraction(1, 2)))


def parse_strength(text):
    """``'2'`` / ``'1.5'`` -> S16 = round(16 S) of ``--grain``; 0 <= S <= 8."""
    return _sixteenths(text, '--grain (grain)', 8)


def parse_chroma(text):
    """``'0.5'`` -> C16 = round(16 C) of ``--grain-chroma``; 0 <= C <= 1."""
    return _sixteenths(text, '--grain-chroma (grain_chroma)', 1)


def parse_seed(text):
    """A uint32 of ``--grain-seed``, decimal or 0x hexadecimal."""
    try:
        if isinstance(text, bool):
            raise ValueError
        v = int(text, 0) if isinstance(text, str) else int(text)
        if isinstance(text, float) and v != text:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError('--grain-seed (grain_seed) takes an integer in 0 .. 2^32 - 1, got %r' % (text,)) from None
    if not 0 <= v <= _M32:
        raise ValueError('--grain-seed (grain_seed): %d lies outside 0 .. 2^32 - 1' % v)
    return v


def check_size(r):
    """None (the default, 1) or 0, 1, 2."""
    if r is None:
        return DEFAULT_SIZE
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r not in (0, 1, 2):
        raise ValueError('--grain-size (grain_size) must be 0, 1 or 2, got %r' % (r,))
    return int(r)


def check_curve(name):
    """None (the default, ``film``) or one of ``CURVES``."""
    if name is None:
        return DEFAULT_CURVE
    if name not in CURVES:
        raise ValueError('--grain-curve (grain_curve) must be one of %s, got %r' % (', '.join(CURVES), name))
    return name


def check_params(params):
    """(S16, r, C16, curve, seed) checked, as ints and a curve name."""
    try:
        s16, r, c16, curve, seed = params
        ints = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (s16, r, c16, seed))
    except (TypeError, ValueError):
        ints = False
    if not ints:
        raise ValueError('grain must be (S16, r, C16, curve, seed), got %r' % (params,))
    if not 0 <= s16 <= MAX_S16:
        raise ValueError('grain: S16 = %d lies outside 0 .. %d (S in 0 .. 8)' % (s16, MAX_S16))
    if not 0 <= c16 <= 16:
        raise ValueError('grain: C16 = %d lies outside 0 .. 16 (C in 0 .. 1)' % c16)
    return int(s16), check_size(r), int(c16), check_curve(curve), parse_seed(seed)


def check_grain(grain=None, size=None, chroma=None, curve=None, seed=None, ranks=1):
    """The five switches as given (None: not given) -> None (no ``--grain``, or S = 0: no stage) or ``params``.  Refused: S outside
    [0, 8], a size outside {0, 1, 2}, C outside [0, 1], an unknown curve, a seed that is no uint32, a sub-switch without ``--grain``,
    more than one rank (frame n is a running count of the rank's written frames)."""
    given = [name for name, v in (('--grain-size', size), ('--grain-chroma', chroma), ('--grain-curve', curve), ('--grain-seed', seed))
             if v is not None]
    if grain is None:
        if given:
            raise ValueError('%s says how --grain works: give --grain S with it' % ', '.join(given))
        return None
    params = (parse_strength(grain), check_size(size), DEFAULT_CHROMA16 if chroma is None else parse_chroma(chroma), check_curve(curve),
              DEFAULT_SEED if seed is None else parse_seed(seed))
    if ranks != 1:
        raise ValueError('--grain runs on one rank: frame n of the grain is a running count of the frames a rank writes, and a second '
                         'rank would restart it (got %d ranks)' % ranks)
    return params if params[0] else None


# ---- the noise -------------------------------------------------------------------------------------------------------------
def mix32(x):
    """The hash, on uint32 values (an int or an array) -> uint32 of the same shape (an int for an int)."""
    if isinstance(x, (int, np.integer)) and not isinstance(x, np.ndarray):
        x = int(x) & _M32
        x ^= x >> 16
        x = (x * 0x7feb352d) & _M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & _M32
        return x ^ (x >> 16)
    x = np.asarray(x).astype(np.uint64) & np.uint64(_M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(_M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(_M32)
    return (x ^ (x >> np.uint64(16))).astype(np.uint32)


def plane_key(seed, n, p):
    """The key of plane p (0 .. 2) of written frame n."""
    if not 0 <= p <= 2 or n < 0:
        raise ValueError('plane_key: frame %r, plane %r' % (n, p))
    return mix32((int(seed) + GOLDEN * (4 * int(n) + p + 1)) & _M32)


def white(key, X, Y):
    """white(key, X, Y) for cell coordinates in 0 .. 65535 (ints or arrays that broadcast) -> int64."""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if X.size and Y.size and (X.min() < 0 or Y.min() < 0 or X.max() > 0xFFFF or Y.max() > 0xFFFF):
        raise ValueError('white: cell coordinates outside 0 .. 65535')
    u = np.asarray(mix32(np.uint64(int(key) & _M32) ^ np.asarray(mix32((Y << 16) | X), np.uint64)), np.int64)
    return (u & 255) + ((u >> 8) & 255) + ((u >> 16) & 255) + (u >> 24) - 510


def field_np(key, rows, cols, r):
    """F of a rows x cols plane -> int64 [rows, cols]."""
    r = check_size(r)
    if not (1 <= rows <= MAX_SIDE and 1 <= cols <= MAX_SIDE):
        raise ValueError('grain: a plane of %d x %d samples (1 .. %d a side)' % (cols, rows, MAX_SIDE))
    w = white(key, np.arange(2 - r, cols + 2 + r)[None, :], np.arange(2 - r, rows + 2 + r)[:, None])
    c = TAPS[r]
    hz = sum(c[i] * w[:, i:i + cols] for i in range(2 * r + 1))
    return sum(c[j] * hz[j:j + rows] for j in range(2 * r + 1))


# ---- the gain ----------------------------------------------------------------------------------------------------------------
def curve8(curve, full_range):
    """The Q8 curve over the 256 8-bit luma codes -> int64 [256]."""
    curve = check_curve(curve)
    if curve == 'flat':
        return np.full(256, 256, np.int64)
    c = np.arange(256, dtype=np.float64)
    t = c / 255.0 if full_range else np.clip((c - 16.0) / 219.0, 0.0, 1.0)
    return np.floor(256.0 * (0.25 + 3.0 * t * (1.0 - t)) + 0.5).astype(np.int64)


def gain_table(depth, s16, r, k16, curve, full_range):
    """G [256] int64 for the working depth, S16, the size r, k = k16 / 16 (16 for luma, C16 for chroma), the curve and the range."""
    y4m.check_depth(depth)
    r = check_size(r)
    scale = 65536.0 * (1 << (depth - 8)) * (s16 / 16.0) * (k16 / 16.0)
    return np.floor(scale * curve8(curve, full_range) / 256.0 / (math.sqrt(WHITE_VAR) * NORM[r]) + 0.5).astype(np.int64)


def gain_tables(depth, params, full_range):
    """The two tables the kernel reads, luma then chroma -> int32 [2, 256]."""
    s16, r, c16, curve, _ = check_params(params)
    return np.stack([gain_table(depth, s16, r, 16, curve, full_range), gain_table(depth, s16, r, c16, curve, full_range)]).astype(np.int32)


def nominal_range(depth, full_range, chroma):
    """(lo, hi) of the range written."""
    if full_range:
        return 0, (1 << depth) - 1
    return 16 << (depth - 8), (240 if chroma else 235) << (depth - 8)


def accumulator_bounds(d, s16, r, k16=16):
    """(lowest, highest) value of F G[c] + 2^15 over every white cell in [-510, 510] and every entry of the gain table of depth d, S16, size r
    and k = k16 / 16 (either curve peaks at 256), as Python ints.  The cap S <= 8 keeps both inside int32 for every (d, r): the widest is
    r = 2, d = 16, S = 8 at about 1.69e9, so the kernel's product is a 32-bit one everywhere."""
    f = 510 * sum(TAPS[check_size(r)]) ** 2
    g = int(gain_table(d, s16, r, k16, 'flat', False).max())
    return -f * g + (1 << 15), f * g + (1 << 15)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def apply_rule(v, f, g, lo, hi):
    """out of the rule for samples v, field values f and gains g = G[c] (int64 arrays that broadcast) -> int64."""
    v = np.asarray(v, np.int64)
    delta = (np.asarray(f, np.int64) * np.asarray(g, np.int64) + (1 << 15)) >> 16
    return np.clip(v + delta, np.minimum(lo, v), np.maximum(hi, v))


def grain_plane_np(plane, luma, key, r, gain, depth, lo, hi):
    """The plane [rows, cols] with grain: ``luma`` [rows, cols] is L of every sample (the plane itself for luma), ``gain`` the plane's table
    [256] -> int64 [rows, cols]."""
    v, L = np.asarray(plane).astype(np.int64), np.asarray(luma).astype(np.int64)
    if v.ndim != 2 or L.shape != v.shape:
        raise ValueError('grain_plane_np: a [rows, cols] plane and its luma, got %s and %s' % (v.shape, L.shape))
    c = np.minimum(L >> (depth - 8), 255)
    return apply_rule(v, field_np(key, v.shape[0], v.shape[1], r), np.asarray(gain, np.int64)[c], lo, hi)


def chroma_luma(luma, rows, cols):
    """L of the samples of a rows x cols chroma plane of the frame whose luma plane is ``luma`` [h, w]: the luma sample at
    (min(x sx, w - 1), min(y sy, h - 1))."""
    h, w = luma.shape
    sy, sx = (1 if rows == h else 2), (1 if cols == w else 2)
    return luma[np.minimum(np.arange(rows) * sy, h - 1)[:, None], np.minimum(np.arange(cols) * sx, w - 1)[None, :]]


def grain_payload_np(payload, h, w, layout, depth, full_range, n, params):
    """The payload (a 1-D array of samples: uint8 at 8 bits, uint16 above) of the h x w progressive frame n in ``layout`` with grain: every
    plane of ``interlace.plane_shapes`` by ``grain_plane_np``, plane p with ``plane_key(seed, n, p)``.  The definition."""
    s16, r, c16, curve, seed = check_params(params)
    p = np.asarray(payload).reshape(-1)
    if p.dtype != (np.uint16 if depth > 8 else np.uint8):
        raise ValueError('grain_payload_np: %s samples at %d bits' % (p.dtype, depth))
    shapes = plane_shapes(h, w, layout)
    if p.size != sum(a * b for a, b in shapes):
        raise ValueError('grain_payload_np: %d samples for a %dx%d %s frame' % (p.size, w, h, layout))
    tables = gain_tables(depth, params, full_range)
    luma, out, pos = p[:h * w].reshape(h, w), [], 0
    for i, (rows, cols) in enumerate(shapes):
        v = p[pos:pos + rows * cols].reshape(rows, cols)
        L = luma if i == 0 else chroma_luma(luma, rows, cols)
        out.append(grain_plane_np(v, L, plane_key(seed, n, i), r, tables[min(i, 1)], depth, *nominal_range(depth, full_range, i > 0)).reshape(-1))
        pos += rows * cols
    return np.concatenate(out).astype(p.dtype)


def grain_stream_np(stream, params):
    """A whole progressive Y4M byte string (every depth and layout) with grain: frame n gets key n, the header is unchanged -> bytes.  None
    and S16 = 0 give the stream back."""
    if params is None or check_params(params)[0] == 0:
        return bytes(stream)
    rd = y4m.Reader(io.BytesIO(bytes(stream)), y4m.DEPTHS, y4m.LAYOUTS)
    hdr, stream = rd.header, bytes(stream)
    out, buf, n = [stream[:stream.index(b'\n') + 1]], np.empty(hdr.payload, np.uint8), 0
    while rd.read_into(buf):
        p = buf.view('<u2').astype(np.uint16) if hdr.depth > 8 else buf
        q = grain_payload_np(p, hdr.h, hdr.w, hdr.layout, hdr.depth, hdr.full_range, n, params)
        out += [y4m.FRAME + b'\n', q.astype('<u2' if hdr.depth > 8 else np.uint8).tobytes()]
        n += 1
    return b''.join(out)
