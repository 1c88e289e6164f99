"""Letterbox and pillarbox bars of Y4M video (``--crop``): where the picture is inside a payload, and the crop and pad around the
network (demfi_amd/video.py).  Pure host code, numpy only: the definitions and the policy; the GPU only counts
(csrc/crop.hip, ``demfi_luma_line_counts``, integer for integer with ``line_counts_np``).

A sample of the luma plane is *lit* when it is strictly greater than the limit (ffmpeg ``cropdetect``'s, 24 at 8 bits, times
2^(depth-8)).  ``line_counts_np`` DEFINES the lit samples of every row and every column.  A line of ``len`` samples is *picture*
when it has more than floor(len * noise) lit samples (noise = 1/256: a few hot pixels or specks of dust do not make a line, a line
of subtitle text does, so subtitles set in a bar keep that bar).  The extent of a frame is the half-open rectangle (top, bottom,
left, right) from its first picture row and column to one past its last; a frame without a picture line (black, a fade) has none
and contributes nothing.  ``Extent`` takes the union over the probed frames, ``align_rect`` grows it outward to the chroma grid
(and to whole row pairs of each field when the payloads are interlaced), ``check_rect`` decides whether it is worth a crop.

The crop works plane by plane on payloads: the chroma rectangle of (top, bottom, left, right) is (top/sv, ceil(bottom/sv), left/sh,
ceil(right/sh)) with the layout's subsampling factors sv, sh, so a cropped frame has the chroma shape ``y4m.chroma_shape`` gives
for its own size and the siting phase is unchanged.  ``pad_payload_np`` puts the active payload back into a frame of the stream's
black (Y 16 s limited range, 0 full range; chroma 2^(depth-1)): crop(pad(x)) == x always, pad(crop(p)) == p for a payload whose
outside is that black.  ``Cropper`` is the same two conversions over byte views, for the data path.

Not offered: bars that change within a stream (the union is taken, so the widest picture decides); ``--crop`` on
``demfi_amd.clip``; restoring the input's own bar samples (output bars are exact black, whatever noise or logo the input's held).
Scene-cut and repeated-frame decisions are made over the cropped payloads, so they can differ from those of an uncropped run."""
from fractions import Fraction

import numpy as np

from . import y4m

DEFAULT_LIMIT = 24                      # ffmpeg cropdetect's limit, at 8 bits
DEFAULT_NOISE = Fraction(1, 256)        # a line is picture above floor(len * noise) lit samples
DEFAULT_PROBE = 'all'
MIN_ACTIVE = 64                         # rows and columns a cropped frame keeps at least
OUTPUTS = ('pad', 'cropped')
_SUB = {'420': (2, 2), '422': (1, 2), '444': (1, 1), 'mono': (1, 1)}      # (sv, sh): luma samples per chroma sample


def check_params(limit=DEFAULT_LIMIT, noise=DEFAULT_NOISE, probe=DEFAULT_PROBE, output='pad'):
    """(limit 0..255, noise a Fraction in [0, 1), probe 'all' or an int >= 1, output) or ValueError."""
    if isinstance(limit, bool) or not isinstance(limit, int) or not 0 <= limit <= 255:
        raise ValueError('crop_limit must be an integer in 0..255 (8-bit steps), got %r' % (limit,))
    if isinstance(noise, float) or isinstance(noise, bool):
        raise ValueError('crop_noise must be a Fraction, an int or an "N/D" string, got %r' % (noise,))
    try:
        noise = Fraction(noise)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError('crop_noise must be a Fraction, an int or an "N/D" string, got %r' % (noise,))
    if not 0 <= noise < 1:
        raise ValueError('crop_noise must be in [0, 1), got %s' % noise)
    if probe != 'all' and (isinstance(probe, bool) or not isinstance(probe, int) or probe < 1):
        raise ValueError("crop_probe must be 'all' or an integer >= 1, got %r" % (probe,))
    if output not in OUTPUTS:
        raise ValueError('crop_output must be one of %s, got %r' % (', '.join(OUTPUTS), output))
    return limit, noise, probe, output


def parse_probe(text):
    """``--crop-probe``: 'all' or N."""
    if text == 'all':
        return text
    try:
        return check_params(probe=int(text))[2]
    except ValueError:
        raise ValueError("--crop-probe takes 'all' or an integer >= 1, got %r" % (text,))


def parse_crop(text):
    """``--crop``: 'auto', or T:B:L:R, the widths of the top, bottom, left and right bars in luma samples, all >= 0."""
    if text == 'auto':
        return text
    parts = str(text).split(':')
    if len(parts) != 4 or not all(p.isdigit() for p in parts):
        raise ValueError("--crop takes 'auto' or T:B:L:R (the widths of the top, bottom, left and right bars in luma samples, "
                         "all >= 0), got %r" % (text,))
    return tuple(int(p) for p in parts)


def check_crop(crop):
    """The ``crop`` argument of ``VideoRunner``: None, 'auto' or four bar widths (T, B, L, R) >= 0 (a T:B:L:R string is parsed)."""
    if crop is None or crop == 'auto':
        return crop
    if isinstance(crop, str):
        return parse_crop(crop)
    try:
        bars = tuple(crop)
    except TypeError:
        bars = ()
    if len(bars) != 4 or any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 0 for b in bars):
        raise ValueError("crop must be None, 'auto' or four bar widths (T, B, L, R) >= 0 in luma samples, got %r" % (crop,))
    return tuple(int(b) for b in bars)


# ---- detection ---------------------------------------------------------------------------------------------------------------
def line_counts_np(luma, h, w, thresh):
    """(rows [h], cols [w]) uint32: the samples strictly greater than ``thresh`` of every row and every column of the luma plane,
    the first h*w samples of ``luma`` (uint8 or uint16).  The definition ``demfi_luma_line_counts`` matches."""
    a = np.asarray(luma).reshape(-1)
    if a.dtype not in (np.uint8, np.uint16) or a.size < h * w:
        raise ValueError('line_counts_np: %d %s samples for a %dx%d luma plane (uint8 or uint16)' % (a.size, a.dtype, h, w))
    lit = a[:h * w].reshape(h, w) > thresh
    return lit.sum(1).astype(np.uint32), lit.sum(0).astype(np.uint32)


def allowance(length, noise=DEFAULT_NOISE):
    """floor(length * noise): the lit samples a line of ``length`` may have and still be a bar."""
    noise = Fraction(noise)
    return length * noise.numerator // noise.denominator


def frame_extent(rows, cols, noise=DEFAULT_NOISE):
    """(top, bottom, left, right), half-open, of a frame with the line counts ``rows`` [h], ``cols`` [w]; None without a picture
    row or a picture column."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    pr = np.flatnonzero(rows > allowance(cols.size, noise))              # a row has w samples
    pc = np.flatnonzero(cols > allowance(rows.size, noise))
    if pr.size == 0 or pc.size == 0:
        return None
    return int(pr[0]), int(pr[-1]) + 1, int(pc[0]), int(pc[-1]) + 1


class Extent:
    """The union of the extents of the frames pushed.  ``frames``: frames pushed, ``lit``: those that had picture."""

    def __init__(self, noise=DEFAULT_NOISE):
        self.noise, self.frames, self.lit, self._rect = Fraction(noise), 0, 0, None

    def push(self, rows, cols):
        self.frames += 1
        e = frame_extent(rows, cols, self.noise)
        if e is None:
            return
        self.lit += 1
        r = self._rect
        self._rect = e if r is None else (min(r[0], e[0]), max(r[1], e[1]), min(r[2], e[2]), max(r[3], e[3]))

    def rect(self):
        return self._rect


def units(layout, fields=1):
    """(vunit, hunit): what the top / left of a crop must be multiples of.  ``fields`` = 2: the payloads are interlaced
    (``y4m.Frames``' count), so the vertical unit doubles: field parity, and the field each chroma row belongs to, survive."""
    if fields not in (1, 2):
        raise ValueError('fields must be 1 or 2, got %r' % (fields,))
    sv, sh = _SUB[y4m.check_layout(layout)]
    return sv * fields, sh


def align_rect(rect, h, w, layout, fields=1):
    """``rect`` grown outward: top and left multiples of ``units``, bottom and right multiples of them too, or h, w."""
    vu, hu = units(layout, fields)
    t, b, l, r = rect
    return t // vu * vu, min(-(-b // vu) * vu, h), l // hu * hu, min(-(-r // hu) * hu, w)


def bars_rect(bars, h, w):
    """Bar widths (T, B, L, R) of an h x w frame -> the rectangle (top, bottom, left, right)."""
    t, b, l, r = bars
    return t, h - b, l, w - r


def check_rect(rect, h, w, layout, fields=1, explicit=False):
    """What a run does with ``rect`` = (top, bottom, left, right) or None on h x w payloads: (the rectangle to crop to or None for
    no crop stage, None or a line to report).  An ``explicit`` rectangle (the user's) that leaves the frame, keeps fewer than
    ``MIN_ACTIVE`` rows or columns or is not aligned (``align_rect``) is a ValueError that names the unit and the nearest aligned
    values; a detected one is aligned here, is dropped (and reported) below ``MIN_ACTIVE``, and is None when it is the whole frame:
    there is then no crop stage and the bytes are those of a run without the switch."""
    if rect is None:
        return None, ('crop: no probed frame has picture; the frame stays whole' if not explicit else None)
    t, b, l, r = rect
    if not explicit:
        t, b, l, r = align_rect(rect, h, w, layout, fields)
    if not (0 <= t < b <= h and 0 <= l < r <= w):
        raise ValueError('crop: the bars %d:%d:%d:%d (T:B:L:R) leave nothing of a %dx%d frame' % (t, h - b, l, w - r, w, h))
    if b - t < MIN_ACTIVE or r - l < MIN_ACTIVE:
        if explicit:
            raise ValueError('crop: %dx%d of a %dx%d frame is left, the crop keeps at least %dx%d'
                             % (r - l, b - t, w, h, MIN_ACTIVE, MIN_ACTIVE))
        return None, ('crop: the picture found is %dx%d, below %dx%d; the frame stays whole' % (r - l, b - t, MIN_ACTIVE, MIN_ACTIVE))
    if explicit and (t, b, l, r) != align_rect(rect, h, w, layout, fields):
        vu, hu = units(layout, fields)
        at, ab, al, ar = align_rect(rect, h, w, layout, fields)
        raise ValueError('crop: the picture edges of a %s%s stream lie on multiples of %d rows and %d columns (or on the frame\'s edge), '
                         '%d:%d:%d:%d (T:B:L:R) does not; the nearest that keeps all of it is %d:%d:%d:%d'
                         % (layout, ' interlaced' if fields == 2 else '', vu, hu, t, h - b, l, w - r, at, h - ab, al, w - ar))
    if (t, b, l, r) == (0, h, 0, w):
        return None, None
    return (t, b, l, r), None


def probe_indices(n, probe=DEFAULT_PROBE):
    """The payloads of an n-payload input the pre-pass looks at: all of them for 'all' or N >= n, else floor(i n / N), i < N."""
    probe = check_params(probe=probe)[2]
    if probe == 'all' or probe >= n:
        return list(range(n))
    return [i * n // probe for i in range(probe)]


# ---- the two conversions -----------------------------------------------------------------------------------------------------
def black(depth, full_range):
    """(Y, chroma) of black at ``depth`` in the stream's range."""
    return (0 if full_range else 16 << (depth - 8)), 1 << (depth - 1)


def plane_rects(h, w, layout, rect):
    """Per plane of an h x w payload (Y, then Cb and Cr unless mono): (first sample, rows, columns, (r0, r1, c0, c1)), the plane's
    place in the payload and the part of it inside ``rect``."""
    t, b, l, r = rect
    sv, sh = _SUB[y4m.check_layout(layout)]
    ch, cw = y4m.chroma_shape(h, w, layout)
    out = [(0, h, w, (t, b, l, r))]
    if layout != 'mono':
        cr = (t // sv, -(-b // sv), l // sh, -(-r // sh))
        out += [(h * w, ch, cw, cr), (h * w + ch * cw, ch, cw, cr)]
    return out


def _samples(payload, depth):
    a = np.asarray(payload).reshape(-1)
    if depth > 8:
        return y4m.as_samples16(a)
    if a.dtype != np.uint8:
        raise ValueError('a payload of 8-bit samples is a uint8 array, got %s' % a.dtype)
    return a


def _checked(rect, h, w):
    t, b, l, r = rect
    if not (0 <= t < b <= h and 0 <= l < r <= w):
        raise ValueError('rectangle %r outside a %dx%d frame' % (tuple(rect), w, h))
    return b - t, r - l


def crop_payload_np(payload, h, w, depth, layout, rect):
    """The payload of the h x w frame -> the payload of its part inside ``rect``, 1-D (uint8, or uint16 above 8 bits)."""
    ah, aw = _checked(rect, h, w)
    a = _samples(payload, depth)
    if a.size != y4m.payload_size(h, w, layout):
        raise ValueError('payload of %d samples for a %dx%d %s frame' % (a.size, h, w, layout))
    out = np.concatenate([a[o:o + ph * pw].reshape(ph, pw)[r0:r1, c0:c1].reshape(-1) for o, ph, pw, (r0, r1, c0, c1) in
                          plane_rects(h, w, layout, rect)])
    assert out.size == y4m.payload_size(ah, aw, layout)
    return out


def pad_payload_np(active, h, w, depth, layout, rect, full_range=False):
    """The payload of the frame inside ``rect`` -> the payload of the h x w frame, black of the stream's range around it."""
    ah, aw = _checked(rect, h, w)
    a = _samples(active, depth)
    if a.size != y4m.payload_size(ah, aw, layout):
        raise ValueError('payload of %d samples for a %dx%d %s frame' % (a.size, ah, aw, layout))
    yb, cb = black(depth, full_range)
    out = np.empty(y4m.payload_size(h, w, layout), a.dtype)
    pos = 0
    for i, (o, ph, pw, (r0, r1, c0, c1)) in enumerate(plane_rects(h, w, layout, rect)):
        out[o:o + ph * pw] = cb if i else yb
        k = (r1 - r0) * (c1 - c0)
        out[o:o + ph * pw].reshape(ph, pw)[r0:r1, c0:c1] = a[pos:pos + k].reshape(r1 - r0, c1 - c0)
        pos += k
    return out


def resized_header(hdr, h, w):
    """``hdr`` with another frame size and everything else the same (the A tag too: pixel aspect does not depend on the size)."""
    return y4m.Header(w, h, hdr.fps, hdr.interlace, hdr.aspect, hdr.chroma, hdr.color_range, hdr.xtags, hdr.ctag, hdr.depth, hdr.layout)


def cropped_header(hdr, rect):
    """The header of the stream cropped to ``rect``."""
    ah, aw = _checked(rect, hdr.h, hdr.w)
    return resized_header(hdr, ah, aw)


class Cropper:
    """``crop_payload_np`` / ``pad_payload_np`` on the data path, over bytes: ``hdr`` is the FULL stream's header.  The plane
    rectangles are worked out once, in bytes (samples of one or two), and one black full-size payload is kept as the template every
    pad starts from.  ``crop_into(full, active)``: one payload.  ``pad_into(active [c, Pa], full [c, Pf])``: c payloads at once.
    Buffers are writable byte buffers (numpy uint8 arrays, CPU tensors)."""

    def __init__(self, hdr, rect):
        self.rect, self.full, self.active = tuple(rect), hdr, cropped_header(hdr, rect)
        es = 2 if hdr.depth > 8 else 1
        self.Pf, self.Pa = hdr.payload, self.active.payload
        self.planes, pos = [], 0                 # (full offset, rows, row bytes, r0, r1, first byte, bytes of a row piece, active offset)
        for o, ph, pw, (r0, r1, c0, c1) in plane_rects(hdr.h, hdr.w, hdr.layout, rect):
            self.planes.append((o * es, ph, pw * es, r0, r1, c0 * es, (c1 - c0) * es, pos))
            pos += (r1 - r0) * (c1 - c0) * es
        assert pos == self.Pa
        dt = np.uint16 if es == 2 else np.uint8
        zero = np.zeros(y4m.payload_size(self.active.h, self.active.w, hdr.layout), dt)
        self.template = pad_payload_np(zero, hdr.h, hdr.w, hdr.depth, hdr.layout, rect, hdr.full_range).astype(dt).view(np.uint8)

    @staticmethod
    def _bytes(buf):
        a = buf.numpy() if hasattr(buf, 'numpy') else buf if isinstance(buf, np.ndarray) else np.frombuffer(memoryview(buf).cast('B'), np.uint8)
        return a.view(np.uint8)

    def crop_into(self, full_buf, active_buf):
        src, dst = self._bytes(full_buf).reshape(-1), self._bytes(active_buf).reshape(-1)
        if src.size != self.Pf or dst.size != self.Pa:
            raise ValueError('Cropper: buffers of %d and %d bytes for payloads of %d and %d' % (src.size, dst.size, self.Pf, self.Pa))
        for o, ph, rb, r0, r1, b0, nb, pos in self.planes:
            dst[pos:pos + (r1 - r0) * nb].reshape(r1 - r0, nb)[...] = src[o:o + ph * rb].reshape(ph, rb)[r0:r1, b0:b0 + nb]

    def pad_into(self, active, full):
        src, dst = self._bytes(active), self._bytes(full)
        src, dst = src.reshape(-1, self.Pa), dst.reshape(-1, self.Pf)
        c = src.shape[0]
        if dst.shape[0] != c:
            raise ValueError('Cropper: %d active payloads for %d full ones' % (c, dst.shape[0]))
        dst[...] = self.template
        for i in range(c):                       # row slices of one payload are views; those of [c, P] would be copies
            for o, ph, rb, r0, r1, b0, nb, pos in self.planes:
                dst[i, o:o + ph * rb].reshape(ph, rb)[r0:r1, b0:b0 + nb] = src[i, pos:pos + (r1 - r0) * nb].reshape(r1 - r0, nb)
