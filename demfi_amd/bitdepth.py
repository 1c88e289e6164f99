"""Bit depth of the Y4M video path (``python -m demfi_amd.video --work-depth W --out-depth D [--dither bayer|none]``): payloads are promoted
to W bits right behind their H2D copy and requantised to D bits as the last device stage.  Pure Python / numpy and integers; the one
module that knows the rule.

**Which depths.**  ``resolve(in_depth, work, out)``: work = W if given, else max(input depth, D); out = D if given, else the INPUT's depth
(so ``--work-depth 12`` alone on an 8-bit stream is 8 -> 12 -> 8, dithered).  Refused: a depth outside ``y4m.DEPTHS``, W below the input's
depth, D above W, ``--dither`` where nothing is requantised.  work == out == the input's depth is no stage at all.

**The rule**, for one sample v of a plane taken from d_in to d_out bits, peak_d = 2^d - 1:

    out = clip(off_out + floor(((v - off_in) * num + T) / den), 0, peak_out)

Limited range, every plane: off = 0 and (num, den) = (2^(d_out - d_in), 1) going up, (1, 2^(d_in - d_out)) going down -- pure shifts, so
16 << 2 = 64 and 128 << 2 = 512 stay exact, the convention of ``y4m.to_bgr_coefs_depth`` and ``letterbox.black``.  Full range
(``XCOLORRANGE=FULL``): (num, den) = (peak_out, peak_in), off = 0 for luma and 2^(d - 1) for chroma on each side; the floor is the
mathematical one (numpy's ``//``), so neutral chroma maps to neutral and black to black under every threshold.  The threshold T lies in
[0, den): going up, and with ``--dither none``, den // 2 (round half up); with ``bayer``, going down, ((2 B + 1) * den) >> 7, where B in
0 .. 63 is the 8x8 ordered-dither index (``bayer_index``) of the sample's position (x, y) WITHIN ITS OWN PLANE:

    B = sum over i = 0 .. 2 of  (((x ^ y) >> i) & 1) << (5 - 2 i)  |  ((y >> i) & 1) << (4 - 2 i)

(first row 0 32 8 40 2 34 10 42).  For interlaced output (``field_rows``) y is the row within its field, payload row >> 1: otherwise a
field would see four of the eight matrix rows only and the two fields would differ in mean by 1/8 LSB.  The pattern is the same in every
frame.  v is the stored sample, whatever it is: a 16-bit sample above peak_in goes through the same formula and ends at the clip.

``promote_payload_np`` / ``requant_payload_np`` are the definitions the kernels (csrc/bitdepth.hip, ``demfi_payload_promote`` /
``demfi_payload_requant``) are held to, byte for byte.  ``accumulator_bounds`` states how wide (v - off_in) * num + T gets; ``reciprocal`` /
``div_np`` are the multiply-and-shift division by den that the kernel uses for full range, mirrored here so that a test can hold it to
the floor.

fp16 (``--dtype fp16``) resolves 10 bits fully and about 12 at best, so W >= 12 wants ``--dtype fp32``; it is not refused.

Not offered: error diffusion, random or blue-noise dither, patterns that change from frame to frame, ``demfi_amd.clip``, changing the
range or the matrix on the way.
"""
import io

import numpy as np

from . import y4m
from .interlace import plane_shapes

DITHERS = ('bayer', 'none')
DEFAULT_DITHER = 'bayer'


def check_dither(mode):
    """None (the default, ``bayer``) or one of ``DITHERS``."""
    if mode is None:
        return DEFAULT_DITHER
    if mode not in DITHERS:
        raise ValueError('dither must be one of %s, got %r' % (', '.join(DITHERS), mode))
    return mode


def check_switches(work=None, out=None, dither=None):
    """What can be said of the three switches before a header is known: the depths are ``y4m.DEPTHS``' (or None), D <= W when both are
    given, ``dither`` is one of ``DITHERS`` (or None) and says how a requantisation works, so it is an error where neither depth is given.
    Returns (work, out, dither) as given."""
    for name, d in (('--work-depth (work_depth)', work), ('--out-depth (out_depth)', out)):
        if d is not None and (isinstance(d, bool) or d not in y4m.DEPTHS):
            raise ValueError('%s must be one of %s, got %r' % (name, ', '.join(str(x) for x in y4m.DEPTHS), d))
    if work is not None and out is not None and out > work:
        raise ValueError('--out-depth %d is above --work-depth %d: the output is requantised DOWN from the working depth; give a working '
                         'depth of at least %d, or leave it out' % (out, work, out))
    if dither is not None:
        check_dither(dither)
        if work is None and out is None:
            raise ValueError('--dither (dither) says how --out-depth requantises: give --out-depth D (or --work-depth W) with it')
    return work, out, dither


def resolve(in_depth, work=None, out=None, dither=None):
    """(input depth, working depth, output depth, dither mode) of a stream of ``in_depth`` bits under the switches: work = W if given,
    else max(in_depth, D); out = D if given, else in_depth; the mode is one of ``DITHERS`` when out < work and None otherwise.  Refused:
    what ``check_switches`` refuses, W < in_depth, D > the working depth, a ``dither`` where nothing is requantised."""
    check_switches(work, out, dither)
    y4m.check_depth(in_depth)
    w = work if work is not None else max(in_depth, out if out is not None else in_depth)
    o = out if out is not None else in_depth
    if w < in_depth:
        raise ValueError('--work-depth %d is below the input\'s %d bits: the working depth is what every stage computes at, and samples are only '
                         'promoted on the way in; give --out-depth %d to deliver %d bits' % (w, in_depth, w, w))
    if o > w:
        raise ValueError('--out-depth %d is above the working depth %d' % (o, w))
    if o == w and dither is not None:
        raise ValueError('--dither %s without a requantisation: the output has the working depth (%d bits); it says how --out-depth below '
                         'the working depth rounds' % (dither, w))
    return in_depth, w, o, (check_dither(dither) if o < w else None)


def is_noop(depths):
    """True for None and for (in, work, out, ...) all equal: no stage, no buffer, no launch."""
    return depths is None or depths[0] == depths[1] == depths[2]


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def bayer_index(x, y):
    """B in 0 .. 63 of the position (x, y) (ints or arrays): the bit-reversed interleave of x ^ y and y, modulo 8 each."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    b = 0
    for i in range(3):
        b = b | ((((x ^ y) >> i) & 1) << (5 - 2 * i)) | (((y >> i) & 1) << (4 - 2 * i))
    return b


def plane_rule(d_in, d_out, full_range, chroma):
    """(off_in, off_out, num, den) of a plane (``chroma``: Cb or Cr) taken from d_in to d_out bits."""
    y4m.check_depth(d_in), y4m.check_depth(d_out)
    if not full_range:
        k = d_out - d_in
        return (0, 0, 1 << k, 1) if k >= 0 else (0, 0, 1, 1 << -k)
    off_in, off_out = (1 << (d_in - 1), 1 << (d_out - 1)) if chroma else (0, 0)
    return off_in, off_out, (1 << d_out) - 1, (1 << d_in) - 1


def threshold(den, bayer=None):
    """T of the rule: den // 2 (``bayer`` None), or ((2 B + 1) * den) >> 7 for the dither index / indices ``bayer``."""
    if bayer is None:
        return den // 2
    return ((2 * np.asarray(bayer, np.int64) + 1) * den) >> 7


def convert_plane_np(plane, d_in, d_out, full_range=False, chroma=False, dither=None, field_rows=False):
    """The plane [rows, cols] taken from d_in to d_out bits by the rule -> int64 [rows, cols].  ``dither``: None or 'none' (T = den // 2), or
    'bayer', which counts only going down; ``field_rows``: the dither's y is the row within its field."""
    p = np.asarray(plane).astype(np.int64)
    if p.ndim != 2:
        raise ValueError('convert_plane_np: a [rows, cols] plane, got %s' % (p.shape,))
    off_in, off_out, num, den = plane_rule(d_in, d_out, full_range, chroma)
    if dither == 'bayer' and d_out < d_in:
        ys, xs = np.arange(p.shape[0])[:, None], np.arange(p.shape[1])[None, :]
        t = threshold(den, bayer_index(xs, ys >> 1 if field_rows else ys))
    else:
        if dither not in (None, 'none', 'bayer'):
            check_dither(dither)
        t = threshold(den)
    return np.clip(off_out + ((p - off_in) * num + t) // den, 0, (1 << d_out) - 1)


def _dtype(depth):
    return np.uint16 if depth > 8 else np.uint8


def convert_payload_np(payload, h, w, layout, d_in, d_out, full_range=False, dither=None, field_rows=False):
    """The payload (a 1-D array of samples: uint8 at 8 bits, uint16 above) of an h x w frame in ``layout`` from d_in to d_out bits: every
    plane of ``interlace.plane_shapes`` by ``convert_plane_np``, the first as luma, the others as chroma; uint8 at 8 bits, uint16 above."""
    p = np.asarray(payload).reshape(-1)
    if p.dtype != _dtype(d_in):
        raise ValueError('convert_payload_np: %s samples at %d bits' % (p.dtype, d_in))
    shapes = plane_shapes(h, w, layout)
    if p.size != sum(r * c for r, c in shapes):
        raise ValueError('convert_payload_np: %d samples for a %dx%d %s frame' % (p.size, w, h, layout))
    out, pos = [], 0
    for i, (r, c) in enumerate(shapes):
        out.append(convert_plane_np(p[pos:pos + r * c].reshape(r, c), d_in, d_out, full_range, i > 0, dither, field_rows).reshape(-1))
        pos += r * c
    return np.concatenate(out).astype(_dtype(d_out))


def promote_payload_np(payload, h, w, layout, d_in, d_out, full_range=False):
    """``convert_payload_np`` going up (d_out > d_in): T = den // 2."""
    if d_out <= d_in:
        raise ValueError('promote_payload_np: %d -> %d bits does not go up' % (d_in, d_out))
    return convert_payload_np(payload, h, w, layout, d_in, d_out, full_range)


def requant_payload_np(payload, h, w, layout, d_in, d_out, full_range=False, dither=DEFAULT_DITHER, field_rows=False):
    """``convert_payload_np`` going down (d_out < d_in) with the rounding ``dither``."""
    if d_out >= d_in:
        raise ValueError('requant_payload_np: %d -> %d bits does not go down' % (d_in, d_out))
    return convert_payload_np(payload, h, w, layout, d_in, d_out, full_range, check_dither(dither), field_rows)


def depth_header(hdr, depth):
    """``hdr`` at another bit depth: the C tag of that depth in the header's layout (an 8-bit 4:2:0 stream keeps its siting tag when it stays
    at 8 bits) and everything else the same."""
    y4m.check_depth(depth)
    ctag = hdr.ctag if depth == hdr.depth else y4m.output_ctag(depth, hdr.layout)
    return y4m.Header(hdr.w, hdr.h, hdr.fps, hdr.interlace, hdr.aspect, hdr.chroma, hdr.color_range, hdr.xtags, ctag, depth, hdr.layout)


def _convert_stream(stream, depth, dither, field_rows, up):
    rd = y4m.Reader(io.BytesIO(bytes(stream)), y4m.DEPTHS, y4m.LAYOUTS, fields=True)
    hdr = rd.header
    if depth == hdr.depth:
        return bytes(stream)
    if (depth > hdr.depth) != up:
        raise ValueError('%s: a %d-bit stream to %d bits' % ('promote_stream_np' if up else 'requant_stream_np', hdr.depth, depth))
    field_rows = hdr.interlace in ('t', 'b') if field_rows is None else bool(field_rows)
    out, buf = [depth_header(hdr, depth).encode()], np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        p = buf.view('<u2') if hdr.depth > 8 else buf
        q = convert_payload_np(p.astype(_dtype(hdr.depth)), hdr.h, hdr.w, hdr.layout, hdr.depth, depth, hdr.full_range, dither, field_rows)
        out += [y4m.FRAME + b'\n', q.astype('<u2' if depth > 8 else np.uint8).tobytes()]
    return b''.join(out)


def promote_stream_np(stream, depth):
    """A whole Y4M byte string (every layout; progressive or ``It`` / ``Ib``) promoted to ``depth`` bits, the header's C tag rewritten ->
    bytes.  The stream's own depth gives the stream back."""
    return _convert_stream(stream, depth, None, False, True)


def requant_stream_np(stream, depth, dither=DEFAULT_DITHER, field_rows=None):
    """A whole Y4M byte string requantised to ``depth`` bits -> bytes.  ``field_rows``: None takes it from the header (an ``It`` / ``Ib``
    stream holds fields)."""
    return _convert_stream(stream, depth, check_dither(dither), field_rows, False)


# ---- widths, and the division the kernel makes ---------------------------------------------------------------------------------
def accumulator_bounds(d_in, d_out, full_range, chroma=False, stored_peak=None):
    """(lowest, highest) value of (v - off_in) * num + T over v in [0, stored_peak] (None: peak_in; 65535: whatever a 16-bit sample can
    hold) and T in [0, den), as Python ints.  Limited range stays below 2^24.  Full range reaches 65535 * 65535 + 65534 < 2^32 at its
    widest (16-bit samples at their stored peak towards 16 bits) and goes below zero for chroma, so a signed value needs 64 bits there
    and a bias that makes the floor unsigned does too; the kernel divides magnitudes instead (``floor_div_magnitudes``), which stay below
    2^32 for every pair."""
    off_in, _, num, den = plane_rule(d_in, d_out, full_range, chroma)
    top = (1 << d_in) - 1 if stored_peak is None else int(stored_peak)
    return (0 - off_in) * num, (top - off_in) * num + den - 1


def reciprocal(den):
    """(m, s) with floor(n / den) == (t + ((n - t) >> 1)) >> s, t = (m * n) >> 32, for EVERY n in [0, 2^32) (32-bit unsigned arithmetic
    throughout; the round-up method of Granlund and Montgomery): l = ceil(log2 den), m = floor(2^32 (2^l - den) / den) + 1, s = l - 1.
    den in [2, 2^32)."""
    den = int(den)
    if not 2 <= den < 1 << 32:
        raise ValueError('reciprocal: den=%r outside 2 .. 2^32 - 1' % (den,))
    l = (den - 1).bit_length()
    return ((1 << 32) * ((1 << l) - den)) // den + 1, l - 1


def div_np(n, den):
    """floor(n / den) of uint32 values by ``reciprocal``, as the kernel computes it (uint64 arrays that hold 32-bit values)."""
    m, s = reciprocal(den)
    n = np.asarray(n, np.uint64)
    if n.size and int(n.max()) >= 1 << 32:
        raise ValueError('div_np: values of 32 bits')
    t = (n * np.uint64(m)) >> np.uint64(32)
    return (t + ((n - t) >> np.uint64(1))) >> np.uint64(s)


def floor_div_magnitudes(a, num, t, den):
    """How the kernel gets floor((a * num + t) / den) for signed a without a signed or a 64-bit division: (negative?, the unsigned
    numerator n) with the quotient q = n // den giving  +q  where a >= 0 (n = a num + t)  and  -q  where a < 0 (n = |a| num + (den - 1 - t):
    floor(-m / den) = -floor((m + den - 1) / den) for m = |a| num - t > -den).  int64 arrays."""
    a, t = np.asarray(a, np.int64), np.asarray(t, np.int64)
    neg = a < 0
    return neg, np.where(neg, -a * num + (den - 1 - t), a * num + t)
