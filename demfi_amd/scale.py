"""Resized Y4M output (``python -m demfi_amd.video --scale WxH [--scale-filter lanczos3|bicubic|bilinear]``): every progressive payload
the run would write is resampled to W x H by a separable polyphase filter.  Pure Python / numpy; the one module that knows the rule.

**Size.**  ``WxH``, width first, as in ffmpeg's ``-s`` (``--tile`` is rows first).  The header is the progressive one but for W, H and the
pixel aspect (``scaled_header``): with ``A = N:D``, both positive, A_out = N w_in h_out : D h_in w_out, reduced, so the display aspect
stays (720x576 at A16:15 -> 720x480 at A8:9); a missing A and A0:0 stay as they are.

**Tables** (``axis_table``).  One axis of n_in samples becomes n_out.  Output sample o has its centre at c = (2 o + 1) n_in / (2 n_out) - 1/2
(centre-aligned; floor(c) is computed in integers).  The kernel k has the support a: lanczos3 a = 3, sinc(x) sinc(x / 3); bicubic a = 2,
Catmull-Rom; bilinear a = 1, the triangle.  It is stretched by s = max(n_in / n_out, 1), so shrinking low-passes.  T = 2 ceil(a s) taps
start at first = floor(c) - T / 2 + 1; tap j weighs source sample first + j with k((first + j - c) / s).  The T weights are normalised in
float64, rounded half up to Q14 (``ONE`` = 1 << 14), and the rounding remainder goes to the first largest tap, so every row sums to exactly
``ONE``: a constant plane stays constant, and n_in == n_out gives the unit tap, an exact copy of the axis.  Source indices clamp to
[0, n_in - 1] where they are used (the table keeps ``first`` as it is).  T > ``MAX_TAPS`` = 32 is refused: a shrink beyond 16 / a to 1.

**Plane** (``resize_plane_np``).  Exact integers, ``>>`` a floor shift, F = ``FRAC`` = 6 bits kept between the passes:

    horizontal:  t = (sum_j cx[xo, j] src[y, clamp(fx[xo] + j)] + 2^(13 - F)) >> (14 - F)            signed, not clamped
    vertical:    v = clip((sum_j cy[yo, j] t[clamp(fy[yo] + j), xo] + 2^(13 + F)) >> (14 + F), 0, peak)

``accumulator_bounds`` gives the exact worst-case magnitude of both sums from the tables' rows: the horizontal sum fits int32 at every
depth and the vertical one at 8 bits; above 8 bits it does not provably fit, so the kernel (csrc/scale.hip, ``demfi_payload_scale``) keeps a
64-bit vertical sum for two-byte samples.  The kernel computes no weights: it reads these tables (``table_blob``) and is held to
``scale_payload_np`` byte for byte.

**Payload.**  Every plane of the payload (``interlace.plane_shapes``) is resampled as a plane in its own right, centre-aligned, to the
shape the output size gives it.

Not offered: scaling in front of the network (cheaper for a shrink), chroma siting offsets (the half-sample horizontal offset of
``420mpeg2`` and the quarter-row offset of interlaced 4:2:0 are not modelled, as in ``demfi_amd.deint`` and ``demfi_amd.interlace``),
``-1`` / keep-aspect sizes, linear-light resampling, ``demfi_amd.clip``, numeric equality with swscale or zimg.
"""
import io
import re
from fractions import Fraction

import numpy as np

from . import y4m
from .interlace import plane_shapes
from .letterbox import resized_header

FILTERS = ('lanczos3', 'bicubic', 'bilinear')
DEFAULT_FILTER = 'lanczos3'
SUPPORT = {'lanczos3': 3, 'bicubic': 2, 'bilinear': 1}
Q, ONE, FRAC, MAX_TAPS = 14, 1 << 14, 6, 32


def parse_size(text):
    """``'1280x720'`` -> (w, h): width first.  Each side in 2 .. ``y4m.MAX_SIDE``, what a Y4M header may name."""
    m = re.fullmatch(r'\s*(\d{1,9})[xX](\d{1,9})\s*', text) if isinstance(text, str) else None
    if not m:
        raise ValueError("--scale (scale) takes WxH, width first, for instance 1280x720; got %r" % (text,))
    return check_size((int(m.group(1)), int(m.group(2))))


def check_size(size):
    """(w, h) as two ints, each in 2 .. ``y4m.MAX_SIDE``."""
    try:
        w, h = size
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (w, h))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('--scale (scale) takes (w, h), two integers, width first; got %r' % (size,))
    if not (2 <= w <= y4m.MAX_SIDE and 2 <= h <= y4m.MAX_SIDE):
        raise ValueError('--scale (scale): %dx%d is outside 2..%d a side' % (w, h, y4m.MAX_SIDE))
    return int(w), int(h)


def check_filter(name):
    """None (the default, ``lanczos3``) or one of ``FILTERS``."""
    if name is None:
        return DEFAULT_FILTER
    if name not in FILTERS:
        raise ValueError('--scale-filter (scale_filter) must be one of %s, got %r' % (', '.join(FILTERS), name))
    return name


def kernel(filt, x):
    """k(x) of the filter, float64, zero outside its support."""
    x = np.abs(np.asarray(x, np.float64))
    if filt == 'lanczos3':
        return np.where(x < 3, np.sinc(x) * np.sinc(x / 3), 0.0)
    if filt == 'bicubic':                            # Catmull-Rom: the cubic convolution kernel with a = -1/2
        return np.where(x <= 1, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2, ((-0.5 * x + 2.5) * x - 4) * x + 2, 0.0))
    return np.where(x < 1, 1 - x, 0.0)


def n_taps(n_in, n_out, filt):
    """T = 2 ceil(a max(n_in / n_out, 1)), in integers."""
    a = SUPPORT[check_filter(filt)]
    return 2 * (a if n_in <= n_out else -(-a * n_in // n_out))


def _axis(n_in, n_out, filt):
    """(first [n_out] int64, the normalised float64 weights [n_out, T]) of one axis."""
    filt = check_filter(filt)
    if n_in < 1 or n_out < 1:
        raise ValueError('--scale: an axis of %r samples to one of %r' % (n_in, n_out))
    T = n_taps(n_in, n_out, filt)
    if T > MAX_TAPS:
        a = SUPPORT[filt]
        raise ValueError('--scale: %d -> %d samples with %s takes %d taps, more than %d: this filter shrinks an axis by %d:%d at most '
                         '(a plane of a subsampled layout counts for itself)' % (n_in, n_out, filt, T, MAX_TAPS, MAX_TAPS // 2, a))
    o = np.arange(n_out, dtype=np.int64)
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out             # c = num / den
    first = num // den - T // 2 + 1
    c = num.astype(np.float64) / den
    s = max(n_in / n_out, 1.0)
    w = kernel(filt, ((first[:, None] + np.arange(T)) - c[:, None]) / s)
    return first, w / w.sum(axis=1, keepdims=True)


def axis_table(n_in, n_out, filt=None):
    """(first [n_out] int32, coef [n_out, T] int16) of one axis (the module's docstring): every row of ``coef`` sums to ``ONE``."""
    first, w = _axis(n_in, n_out, filt)
    q = np.floor(w * ONE + 0.5).astype(np.int64)
    rows = np.arange(n_out)
    q[rows, np.argmax(q, axis=1)] += ONE - q.sum(axis=1)        # argmax: the first of the largest taps
    assert (q.sum(axis=1) == ONE).all() and np.abs(q).max() < 1 << 15
    return first.astype(np.int32), q.astype(np.int16)


def _taps(src, first, coef, axis):
    """sum_j coef[o, j] src[clamp(first[o] + j)] along ``axis`` of the int64 array ``src`` -> int64."""
    n = src.shape[axis]
    out = 0
    for j in range(coef.shape[1]):
        idx = np.clip(first.astype(np.int64) + j, 0, n - 1)
        c = coef[:, j].astype(np.int64)
        out = out + (np.take(src, idx, axis=axis) * (c[:, None] if axis == 0 else c[None, :]))
    return out


def resize_plane_np(plane, h_out, w_out, filt=None, peak=255):
    """The plane [rows, cols] resampled to [h_out, w_out] (the module's docstring); the dtype of ``plane``."""
    p = np.asarray(plane)
    if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError('resize_plane_np: a [rows, cols] plane, got %s' % (p.shape,))
    fx, cx = axis_table(p.shape[1], w_out, filt)
    fy, cy = axis_table(p.shape[0], h_out, filt)
    t = (_taps(p.astype(np.int64), fx, cx, 1) + (1 << (Q - 1 - FRAC))) >> (Q - FRAC)
    v = (_taps(t, fy, cy, 0) + (1 << (Q - 1 + FRAC))) >> (Q + FRAC)
    return np.clip(v, 0, peak).astype(p.dtype)


def accumulator_bounds(tables, peak):
    """``tables`` = ((fx, cx), (fy, cy)), the horizontal and the vertical ``axis_table`` of a plane: the exact worst-case magnitudes
    (|horizontal sum with its rounding term|, |vertical sum with its rounding term|) over samples in [0, peak], as Python ints."""
    (_, cx), (_, cy) = tables
    cx, cy = np.asarray(cx, np.int64), np.asarray(cy, np.int64)
    px, nx = int(np.clip(cx, 0, None).sum(axis=1).max()), int(np.clip(-cx, 0, None).sum(axis=1).max())
    rh = 1 << (Q - 1 - FRAC)
    h_hi, h_lo = peak * px + rh, -peak * nx + rh                 # the extremes of the horizontal sum
    t_hi, t_lo = h_hi >> (Q - FRAC), h_lo >> (Q - FRAC)          # and of t (t_lo <= 0 <= t_hi)
    py, ny = np.clip(cy, 0, None).sum(axis=1), np.clip(-cy, 0, None).sum(axis=1)
    rv = 1 << (Q - 1 + FRAC)
    v_hi, v_lo = int((py * t_hi - ny * t_lo).max()) + rv, int((py * t_lo - ny * t_hi).min()) + rv
    return max(abs(h_hi), abs(h_lo)), max(abs(v_hi), abs(v_lo))


def scale_payload_np(payload, h, w, h_out, w_out, depth, layout, filt=None):
    """The payload (a 1-D array of samples: uint8 at 8 bits, uint16 above) of an h x w frame resampled to h_out x w_out: every plane by
    ``resize_plane_np`` to the shape the output size gives it; ``y4m.payload_size(h_out, w_out, layout)`` samples."""
    p = np.asarray(payload).reshape(-1)
    if p.dtype != (np.uint16 if depth > 8 else np.uint8):
        raise ValueError('scale_payload_np: %s samples at %d bits' % (p.dtype, depth))
    planes = [a for a in y4m.split_planes_layout(p, h, w, layout) if a is not None]
    out = [resize_plane_np(a, ro, co, filt, (1 << depth) - 1).reshape(-1) for a, (ro, co) in zip(planes, plane_shapes(h_out, w_out, layout))]
    return np.concatenate(out)


def scaled_header(hdr, w, h):
    """The header of the resized stream: ``hdr`` with W, H = w, h and the pixel aspect that keeps the display aspect."""
    out = resized_header(hdr, h, w)
    m = re.fullmatch(r'(\d+):(\d+)', hdr.aspect) if hdr.aspect is not None else None
    if m and int(m.group(1)) > 0 and int(m.group(2)) > 0 and (w, h) != (hdr.w, hdr.h):
        a = Fraction(int(m.group(1)) * hdr.w * h, int(m.group(2)) * hdr.h * w)
        out.aspect = '%d:%d' % (a.numerator, a.denominator)
    return out


def scale_stream_np(stream, w, h, filt=None):
    """A whole progressive Y4M byte string resampled to w x h, header included -> bytes.  Every depth and layout; an interlaced stream
    is refused: a scaler must never see woven fields."""
    filt = check_filter(filt)
    rd = y4m.Reader(io.BytesIO(bytes(stream)), y4m.DEPTHS, y4m.LAYOUTS)
    hdr = rd.header
    ohdr = scaled_header(hdr, w, h)
    out, buf = [ohdr.encode()], np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        p = buf.view('<u2') if hdr.depth > 8 else buf
        q = scale_payload_np(p, hdr.h, hdr.w, h, w, hdr.depth, hdr.layout, filt)
        out += [y4m.FRAME + b'\n', q.astype('<u2' if hdr.depth > 8 else np.uint8).tobytes()]
    return b''.join(out)


def check_interlaced_rows(h, layout):
    """With interlaced output the resized frame must keep field parity in every plane: rows in units of 2, of 4 for 4:2:0."""
    unit = 4 if layout == '420' else 2
    if h % unit:
        raise ValueError('--scale with --interlace: H = %d is not a multiple of %d, the rows of an interlaced %s frame; the nearest are %d and %d'
                         % (h, unit, layout, h - h % unit, h - h % unit + unit))


# ---- the tables as the kernel reads them ------------------------------------------------------------------------------------
DESC_WORDS = 6          # per plane: byte offsets of fx and cx in the blob, Tx, byte offsets of fy and cy, Ty; one last word: the blob's bytes


def table_blob(shapes_in, shapes_out, filt=None):
    """The tables of the planes ``shapes_in`` [(rows, cols)] -> ``shapes_out`` as ``demfi_payload_scale`` takes them: (blob, a uint8
    array that holds the ``first`` (int32) and ``coef`` (int16, [n_out, T]) arrays of every distinct (n_in, n_out) axis, each on a 4-byte
    boundary; desc, int32 [planes * ``DESC_WORDS`` + 1]: per plane the byte offsets of fx and cx, Tx, those of fy and cy, Ty, and behind
    the last plane the bytes of the blob).  Planes of one shape share their tables."""
    parts, at, pos, desc = [], {}, 0, []

    def put(a):
        nonlocal pos
        off = pos
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        parts.append(b)
        pad = -b.size % 4
        if pad:
            parts.append(np.zeros(pad, np.uint8))
        pos += b.size + pad
        return off

    def axis(n_in, n_out):
        if (n_in, n_out) not in at:
            first, coef = axis_table(n_in, n_out, filt)
            at[n_in, n_out] = (put(first), put(coef), coef.shape[1])
        return at[n_in, n_out]
    for (ri, ci), (ro, co) in zip(shapes_in, shapes_out):
        desc.append(axis(ci, co) + axis(ri, ro))
    return np.concatenate(parts), np.ascontiguousarray([v for d in desc for v in d] + [pos], dtype=np.int32)


def float_resize_np(plane, h_out, w_out, filt=None):
    """The separable resample of ``plane`` with the unquantised float64 weights, no rounding: what the integer rule approximates."""
    p = np.asarray(plane, np.float64)
    out = p
    for axis, n_out in ((1, w_out), (0, h_out)):
        first, w = _axis(p.shape[axis], n_out, filt)
        acc = 0.0
        for j in range(w.shape[1]):
            idx = np.clip(first + j, 0, p.shape[axis] - 1)
            acc = acc + np.take(out, idx, axis=axis) * (w[:, j][:, None] if axis == 0 else w[:, j][None, :])
        out = acc
    return out


def float_error_bound(shape_in, h_out, w_out, filt, peak):
    """How far ``resize_plane_np`` may lie from ``float_resize_np`` on samples in [0, peak], from the tables alone: 1/2 for the final
    rounding, max_row sum|cy| 2^-(F+1) / 2^14 for the rounding of t (|t / 2^F - its exact value| <= 2^-(F+1), weighed by the vertical
    row), and peak times the summed coefficient-quantisation error max_row sum_j |c / 2^14 - w| of both axes."""
    (_, wx), (_, wy) = _axis(shape_in[1], w_out, filt), _axis(shape_in[0], h_out, filt)
    (_, cx), (_, cy) = axis_table(shape_in[1], w_out, filt), axis_table(shape_in[0], h_out, filt)
    ex = np.abs(cx / ONE - wx).sum(axis=1).max()
    ey = np.abs(cy / ONE - wy).sum(axis=1).max()
    ay = np.abs(cy.astype(np.float64)).sum(axis=1).max() / ONE
    return 0.5 + ay * 2.0 ** -(FRAC + 1) + peak * (ex + ey)
