"""YUV4MPEG2 (Y4M) stream I/O and the definition of the YUV <-> BGR conversion of the video edge (demfi_amd/video.py).

Y4M is what video tools pass through pipes (``ffmpeg -f yuv4mpegpipe``, x264 / x265 / SVT-AV1 ``--input-y4m``, mpv): one text
header line, then per frame ``FRAME[ params]\\n`` and the raw payload.

``yuv_to_bgr16_np`` / ``bgr16_to_yuv_np`` DEFINE the colour conversion, for every chroma layout of ``LAYOUTS`` and every bit
depth d of ``DEPTHS``; the HIP kernels (csrc/yuv.hip: 8-bit 4:2:0; csrc/yuv_family.hip: the rest; csrc/yuv_common.h: what they
share) match them bit for bit.  Samples and frame values hold 0 .. peak = 2^d - 1.  Integer arithmetic only; with s = 2^(d-8):
  * Q(8+d) matrix coefficients rounded (half up) from the float64 BT.601 / BT.709 matrices, with limited (Y 16s .. 235s,
    C 16s .. 240s; scale factors peak / (219 s), peak / (224 s) and their inverses) or full range folded in; the Y offset is
    16s, the chroma centre 2^(d-1); int64 accumulators (at d = 8 every sum fits int32, which is what the 8-bit kernels use), ONE
    round-half-up, clamp to [0, peak];
  * upsampling keeps chroma in 1/16 units into the matrix.  4:2:0: 420jpeg (centred) 9/3/3/1 over 16, 420mpeg2 (co-sited
    horizontally, centred vertically) 1/2 + 1/2 at odd columns and 3/4 + 1/4 vertically; neighbours clamp to the edge.  4:2:2
    (co-sited horizontally): the horizontal rule of 420mpeg2 with no vertical filter.  4:4:4: the sample itself.  Mono: no chroma
    term, so B = G = R;
  * downsampling rounds once, from the full-resolution Q(8+d) Cb / Cr.  4:2:0 (output is always 420jpeg): a 2x2 box; at an odd
    edge the clamped neighbour repeats the pixel that exists, i.e. the 2 or 1 pixels there are averaged.  4:2:2: the co-sited
    [1,2,1]/4 with clamped edges.  4:4:4: the value itself.  Mono: Y only.
Frames are [h,w,3] in B, G, R order, the frame order of the whole pipeline (cv2's).  The other public conversions are instances:
``yuv_to_bgr_np`` / ``bgr_to_yuv_np`` are d = 8 on uint8 payloads and frames, and ``yuv420_to_bgr_np`` / ``bgr_to_yuv420_np`` /
``yuv420_to_bgr16_np`` / ``bgr16_to_yuv420_np`` are the '420' layout of the two pairs.

What a stream may carry: 8-bit 4:2:0 by default -- the Y plane [h,w] followed by the Cb and Cr planes [ceil(h/2), ceil(w/2)],
1.5 bytes per pixel.  High bit depth is opt-in (``depths=DEPTHS``, ``python -m demfi_amd.video --high-depth``): the tags C420p10 /
C420p12 / C420p14 / C420p16 carry unsigned 16-bit little-endian samples, so a payload has twice the bytes (``Header.payload``
counts bytes) and frames are uint16.  Other chroma layouts are opt-in too (``layouts=LAYOUTS``, ``--any-layout``): C422 (Cb, Cr
[h, ceil(w/2)]), C444 (three [h,w] planes) and Cmono (Y only), and with ``depths=DEPTHS`` their deep forms C422pNN / C444pNN /
CmonoNN.  The output keeps the input's layout and depth.

Two timelines: by default n input frames give (n-3)*M + 1 output frames and the first and last input frames have no output
(``n_output_frames``); on the full-length timeline (``Frames(full_length=True)``, ``retime``) output frame 0 is input frame 0
and n frames give n*M, windows running from k = -1 on tuples clamped at the clip's ends.
"""
import io
import math
import os
import re
from fractions import Fraction

import numpy as np

MAGIC = b'YUV4MPEG2'
FRAME = b'FRAME'
MAX_SIDE = 16384
FIX = "convert the input with ffmpeg's -pix_fmt yuv420p (progressive 8-bit 4:2:0), e.g. ffmpeg -i in.mp4 -pix_fmt yuv420p -f yuv4mpegpipe -"
MATRICES = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}       # (Kr, Kb)
SITINGS = ('420jpeg', '420mpeg2')
DEPTHS = (8, 10, 12, 14, 16)                                          # what ``depths=DEPTHS`` (--high-depth) accepts
HIGH_DEPTH_HINT = '; or keep the bit depth: --high-depth accepts 10- to 16-bit 4:2:0 (C420p10, C420p12, C420p14, C420p16)'
LAYOUTS = ('420', '422', '444', 'mono')                               # what ``layouts=LAYOUTS`` (--any-layout) accepts
ANY_LAYOUT_HINT = ('; or keep the chroma layout: --any-layout accepts 4:2:2, 4:4:4 and grey (C422, C444, Cmono; together with '
                   '--high-depth also C422pNN, C444pNN, CmonoNN for NN in 10, 12, 14, 16)')
DEINTERLACE_HINT = ('; or pass --deinterlace, which bobs the fields of an It (top field first) or Ib (bottom field first) stream '
                    'to progressive frames at twice the rate')
MIXED_HINT = ('; --deinterlace takes It and Ib only: a mixed-mode stream (Im) changes its field order from frame to frame and needs '
              'a field-order fix upstream (for example ffmpeg -vf fieldorder=tff); if it is film carried by 3:2 pulldown, --ivtc takes it '
              'as it is and gives the film frames back')
_CHROMA = {None: '420jpeg', '420jpeg': '420jpeg', '420': '420jpeg', '420mpeg2': '420mpeg2'}
_MAX_LINE = 4096


class Y4MError(ValueError):
    pass


# ---- the conversion definition ---------------------------------------------------------------------------------------------
def _kr_kb(matrix):
    if matrix not in MATRICES:
        raise ValueError('matrix must be one of %s, got %r' % (sorted(MATRICES), matrix))
    return MATRICES[matrix]


def check_depth(depth):
    if depth not in DEPTHS:
        raise ValueError('bit depth must be one of %s, got %r' % (DEPTHS, depth))
    return depth


def check_layout(layout):
    if layout not in LAYOUTS:
        raise ValueError('chroma layout must be one of %s, got %r' % (LAYOUTS, layout))
    return layout


def _fixq(c, q):
    return int(math.floor(c * float(1 << q) + 0.5))


def to_bgr_coefs_depth(matrix, full_range, depth):
    """Q(8+d) (cy, r_cr, g_cb, g_cr, b_cb), Y offset 16 s (s = 2^(d-8)): R = cy*Y' + r_cr*Cr', G = cy*Y' + g_cb*Cb' + g_cr*Cr',
    B = cy*Y' + b_cb*Cb'."""
    kr, kb = _kr_kb(matrix)
    kg = 1.0 - kr - kb
    q, s, peak = 8 + depth, 1 << (depth - 8), (1 << depth) - 1
    ys, cs = (1.0, 1.0) if full_range else (peak / (219.0 * s), peak / (224.0 * s))
    return (_fixq(ys, q), _fixq(cs * 2.0 * (1.0 - kr), q), _fixq(-(cs * 2.0 * kb * (1.0 - kb) / kg), q),
            _fixq(-(cs * 2.0 * kr * (1.0 - kr) / kg), q), _fixq(cs * 2.0 * (1.0 - kb), q)), (0 if full_range else 16 * s)


def to_yuv_coefs_depth(matrix, full_range, depth):
    """Q(8+d) rows (Y, Cb, Cr) x (R, G, B), Y offset 16 s (the chroma offset is 2^(d-1))."""
    kr, kb = _kr_kb(matrix)
    kg = 1.0 - kr - kb
    q, s, peak = 8 + depth, 1 << (depth - 8), (1 << depth) - 1
    ys, cs = (1.0, 1.0) if full_range else (219.0 * s / peak, 224.0 * s / peak)
    return ((_fixq(ys * kr, q), _fixq(ys * kg, q), _fixq(ys * kb, q)),
            (_fixq(-(cs * kr / (2.0 * (1.0 - kb))), q), _fixq(-(cs * kg / (2.0 * (1.0 - kb))), q), _fixq(cs * 0.5, q)),
            (_fixq(cs * 0.5, q), _fixq(-(cs * kg / (2.0 * (1.0 - kr))), q), _fixq(-(cs * kb / (2.0 * (1.0 - kr))), q))), \
        (0 if full_range else 16 * s)


def to_bgr_coefs(matrix, full_range):
    """The 8-bit coefficients: ``to_bgr_coefs_depth`` at d = 8 (Q16, Y offset 16)."""
    return to_bgr_coefs_depth(matrix, full_range, 8)


def to_yuv_coefs(matrix, full_range):
    """The 8-bit coefficients: ``to_yuv_coefs_depth`` at d = 8 (Q16, Y offset 16, chroma offset 128)."""
    return to_yuv_coefs_depth(matrix, full_range, 8)


def chroma_shape(h, w, layout='420'):
    """(rows, columns) of one chroma plane of an h x w frame; (0, 0) for mono."""
    check_layout(layout)
    return {'420': ((h + 1) // 2, (w + 1) // 2), '422': (h, (w + 1) // 2), '444': (h, w), 'mono': (0, 0)}[layout]


def payload_size(h, w, layout='420'):
    """Samples of one payload: Y [h,w], then Cb and Cr of ``chroma_shape`` (4:2:0 unless ``layout`` says otherwise)."""
    ch, cw = chroma_shape(h, w, layout)
    return h * w + 2 * ch * cw


def payload_bytes(h, w, depth=8, layout='420'):
    """Bytes of one payload: ``payload_size`` samples of one byte at depth 8, of two above."""
    return payload_size(h, w, layout) * (2 if depth > 8 else 1)


def as_samples16(payload):
    """A payload of 16-bit little-endian samples (bytes-like, a uint8 array or a uint16 array) -> 1-D uint16 view."""
    if isinstance(payload, np.ndarray) and payload.dtype == np.uint16:
        return payload.reshape(-1)
    a = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else payload.reshape(-1)
    if a.dtype != np.uint8 or a.size % 2:
        raise ValueError('a payload of 16-bit samples is an even number of bytes (uint8) or a uint16 array, got %s x %d' % (a.dtype, a.size))
    return a.view('<u2')


def _split(a, h, w, layout, unit, name):
    ch, cw = chroma_shape(h, w, layout)
    if a.size != payload_size(h, w, layout):
        raise ValueError('payload of %d %s for a %dx%d %s frame (%d expected)' % (a.size, unit, h, w, name, payload_size(h, w, layout)))
    if layout == 'mono':
        return a.reshape(h, w), None, None
    return a[:h * w].reshape(h, w), a[h * w:h * w + ch * cw].reshape(ch, cw), a[h * w + ch * cw:].reshape(ch, cw)


def split_planes_layout(payload, h, w, layout):
    """Payload of samples (a 1-D uint8 or uint16 array) -> (Y [h,w], Cb, Cr of ``chroma_shape``) views; mono: Cb = Cr = None."""
    return _split(payload.reshape(-1), h, w, layout, 'samples', layout)


def split_planes(payload, h, w):
    """8-bit 4:2:0 Y4M payload (bytes-like, 1-D uint8) -> (Y [h,w], Cb, Cr [ceil(h/2), ceil(w/2)]) views."""
    a = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else payload.reshape(-1)
    return _split(a, h, w, '420', 'bytes', '4:2:0')


def split_planes16(payload, h, w):
    """16-bit 4:2:0 Y4M payload -> (Y [h,w], Cb, Cr [ceil(h/2), ceil(w/2)]) uint16 views."""
    return _split(as_samples16(payload), h, w, '420', 'samples', '4:2:0')


def _upsample16(c, h, w, siting):
    """4:2:0 chroma [ch,cw] -> int32 [h,w] in 1/16 units (weights sum to 16)."""
    ch, cw = c.shape
    c = c.astype(np.int32)
    ys = np.arange(h)
    cy0 = ys >> 1
    cy1 = np.where(ys & 1, np.minimum(cy0 + 1, ch - 1), np.maximum(cy0 - 1, 0))
    v = 3 * c[cy0] + c[cy1]                                   # vertical 3/4 + 1/4, weight 4
    xs = np.arange(w)
    cx0 = xs >> 1
    if siting == '420jpeg':
        cx1 = np.where(xs & 1, np.minimum(cx0 + 1, cw - 1), np.maximum(cx0 - 1, 0))
        return 3 * v[:, cx0] + v[:, cx1]
    if siting == '420mpeg2':
        cx1 = np.where(xs & 1, np.minimum(cx0 + 1, cw - 1), cx0)
        return 2 * (v[:, cx0] + v[:, cx1])
    raise ValueError('chroma siting must be one of %s, got %r' % (SITINGS, siting))


def _upsample16_layout(c, h, w, layout):
    """chroma plane of a 4:2:2 / 4:4:4 frame -> int32 [h,w] in 1/16 units.  4:4:4: the sample.  4:2:2 (co-sited horizontally, no
    vertical filter): the sample at even x, 1/2 + 1/2 of it and its right neighbour (clamped to the edge) at odd x -- the
    horizontal rule of 420mpeg2."""
    c = c.astype(np.int32)
    if layout == '444':
        return 16 * c
    if layout == '422':
        xs = np.arange(w)
        cx0 = xs >> 1
        cx1 = np.where(xs & 1, np.minimum(cx0 + 1, c.shape[1] - 1), cx0)
        return 8 * (c[:, cx0] + c[:, cx1])
    raise ValueError('no chroma upsampling for layout %r' % (layout,))


def _matrix_to_bgr(yy, cbv, crv, depth, coefs):
    """The matrix step: int64 [h,w] luma and chroma in 1/16 units, offsets removed -> int64 B, G, R [h,w,3] in 0 .. peak."""
    cy, r_cr, g_cb, g_cr, b_cb = coefs
    sh = 8 + depth + 4
    rnd = np.int64(1 << (sh - 1))
    r = (cy * yy + r_cr * crv + rnd) >> sh
    g = (cy * yy + g_cb * cbv + g_cr * crv + rnd) >> sh
    b = (cy * yy + b_cb * cbv + rnd) >> sh
    return np.clip(np.stack([b, g, r], -1), 0, (1 << depth) - 1)


def _to_bgr(planes, h, w, depth, layout, matrix, full_range, siting):
    """(Y, Cb, Cr) sample planes of any of ``LAYOUTS`` at depth d -> int64 B, G, R [h,w,3] in 0 .. peak: the layout's upsampler,
    then the matrix step."""
    y, cb, cr = planes
    coefs, yoff = to_bgr_coefs_depth(matrix, full_range, depth)
    mid = (1 << (depth - 1)) * 16
    yy = (y.astype(np.int64) - yoff) * 16
    if layout == 'mono':
        cbv = crv = np.zeros((h, w), np.int64)
    else:
        up = (lambda c: _upsample16(c, h, w, siting)) if layout == '420' else (lambda c: _upsample16_layout(c, h, w, layout))
        cbv, crv = up(cb).astype(np.int64) - mid, up(cr).astype(np.int64) - mid
    return _matrix_to_bgr(yy, cbv, crv, depth, coefs)


def _luma_and_chroma(bgr, depth, coefs):
    """B, G, R [h,w,3] at depth d -> (Y [h,w] in 0 .. peak, (Cb, Cr) the full-resolution Q(8+d) chroma centred on 0), int64."""
    (ky, kcb, kcr), yoff = coefs
    q = 8 + depth
    b, g, r = (bgr[:, :, i].astype(np.int64) for i in range(3))
    y = np.clip((ky[0] * r + ky[1] * g + ky[2] * b + (yoff << q) + (1 << (q - 1))) >> q, 0, (1 << depth) - 1)
    return y, [k[0] * r + k[1] * g + k[2] * b for k in (kcb, kcr)]


def _to_yuv(bgr, dtype, depth, layout, matrix, full_range):
    """B, G, R [h,w,3] of ``dtype`` at depth d -> the samples of one payload in any of ``LAYOUTS``, 1-D int64."""
    bgr = np.asarray(bgr)
    if bgr.dtype != dtype or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError('%s [h,w,3] expected, got %s %s' % (np.dtype(dtype).name, bgr.dtype, bgr.shape))
    h, w = bgr.shape[:2]
    if h < 2 or w < 2:
        raise ValueError('frame of %dx%d: 2x2 at least' % (h, w))
    y, fs = _luma_and_chroma(bgr, depth, to_yuv_coefs_depth(matrix, full_range, depth))
    q, peak, mid = 8 + depth, (1 << depth) - 1, 1 << (depth - 1)

    def rounded(s, sh):                                       # a sum of weight 2^(sh-q) over f -> samples, rounded once
        return np.clip((s + (mid << sh) + (1 << (sh - 1))) >> sh, 0, peak)

    def down(f):
        if layout == '444':
            return rounded(f, q)
        if layout == '422':                                   # chroma column i is co-sited with luma column 2i: [1,2,1]/4
            ci = np.arange(0, w, 2)
            return rounded(f[:, np.maximum(ci - 1, 0)] + 2 * f[:, ci] + f[:, np.minimum(ci + 1, w - 1)], q + 2)
        r0, c0 = np.arange(0, h, 2), np.arange(0, w, 2)       # 4:2:0: the 2x2 box; at an odd edge the pixel that exists repeats
        r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
        return rounded(f[r0][:, c0] + f[r0][:, c1] + f[r1][:, c0] + f[r1][:, c1], q + 2)
    planes = [y] if layout == 'mono' else [y, down(fs[0]), down(fs[1])]
    return np.concatenate([p.reshape(-1) for p in planes])


def _as_u8(payload):
    a = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else payload.reshape(-1)
    if a.dtype != np.uint8:
        raise ValueError('a payload of 8-bit samples is a uint8 array, got %s' % a.dtype)
    return a


def yuv_to_bgr16_np(payload, h, w, depth, layout, matrix='bt601', full_range=False, siting='420jpeg'):
    """One payload of 16-bit samples at depth d in any of ``LAYOUTS`` -> uint16 BGR [h,w,3], values 0 .. peak (the definition
    the HIP kernels match); ``siting`` only matters to '420'.  ``depth`` = 8 (samples 0 .. 255 in the 16-bit container) gives the
    values of ``yuv_to_bgr_np``."""
    check_depth(depth)
    planes = split_planes_layout(as_samples16(payload), h, w, check_layout(layout))
    return _to_bgr(planes, h, w, depth, layout, matrix, full_range, siting).astype(np.uint16)


def yuv_to_bgr_np(payload, h, w, layout, matrix='bt601', full_range=False, siting='420jpeg'):
    """One 8-bit payload in any of ``LAYOUTS`` -> uint8 BGR [h,w,3]: the d = 8 instance (whose intermediates fit int32, as the
    8-bit kernels compute them)."""
    planes = split_planes_layout(_as_u8(payload), h, w, check_layout(layout))
    return _to_bgr(planes, h, w, 8, layout, matrix, full_range, siting).astype(np.uint8)


def yuv420_to_bgr16_np(payload, h, w, depth, matrix='bt601', full_range=False, siting='420jpeg'):
    """``yuv_to_bgr16_np`` of a 4:2:0 payload."""
    check_depth(depth)
    return _to_bgr(split_planes16(payload, h, w), h, w, depth, '420', matrix, full_range, siting).astype(np.uint16)


def yuv420_to_bgr_np(payload, h, w, matrix='bt601', full_range=False, siting='420jpeg'):
    """``yuv_to_bgr_np`` of a 4:2:0 payload: one 8-bit 4:2:0 Y4M payload -> uint8 BGR [h,w,3]."""
    return _to_bgr(split_planes(payload, h, w), h, w, 8, '420', matrix, full_range, siting).astype(np.uint8)


def bgr16_to_yuv_np(bgr16, depth, layout, matrix='bt601', full_range=False):
    """uint16 BGR [h,w,3] at depth d -> one payload of 16-bit samples in any of ``LAYOUTS``, 1-D uint16 (the definition the HIP
    kernels match); ``.view(np.uint8)`` / ``.tobytes()`` of it are the little-endian bytes of the stream."""
    check_depth(depth)
    return _to_yuv(bgr16, np.uint16, depth, check_layout(layout), matrix, full_range).astype(np.uint16).astype('<u2', copy=False)


def bgr_to_yuv_np(bgr, layout, matrix='bt601', full_range=False):
    """uint8 BGR [h,w,3] -> one 8-bit payload in any of ``LAYOUTS``, 1-D uint8: the d = 8 instance."""
    return _to_yuv(bgr, np.uint8, 8, check_layout(layout), matrix, full_range).astype(np.uint8)


def bgr16_to_yuv420_np(bgr16, depth, matrix='bt601', full_range=False):
    """``bgr16_to_yuv_np`` to a 4:2:0 (420jpeg) payload."""
    return bgr16_to_yuv_np(bgr16, depth, '420', matrix, full_range)


def bgr_to_yuv420_np(bgr, matrix='bt601', full_range=False):
    """``bgr_to_yuv_np`` to a 4:2:0 (420jpeg) payload."""
    return bgr_to_yuv_np(bgr, '420', matrix, full_range)


def auto_matrix(h):
    """--matrix auto: BT.709 for HD (H >= 720), BT.601 below (what encoders assume for untagged video)."""
    return 'bt709' if h >= 720 else 'bt601'


# ---- header ----------------------------------------------------------------------------------------------------------------
class Header:
    """Parsed stream header.  ``chroma``: '420jpeg' | '420mpeg2' (C420 / missing C = 420jpeg); ``full_range`` from
    XCOLORRANGE (default limited); ``fps`` a Fraction; ``aspect`` / ``color_range`` the raw A / XCOLORRANGE values or None;
    ``xtags`` the other X parameters in order.  ``depth``: bits per sample, 8 or (C420pNN) 10 / 12 / 14 / 16, the latter as
    16-bit little-endian samples; ``payload`` / ``frame_bytes`` are bytes.  ``layout``: one of ``LAYOUTS``; ``chroma`` is the
    siting of a 4:2:0 stream and stays '420jpeg' for the other layouts, which have one siting each."""

    def __init__(self, w, h, fps, interlace='p', aspect=None, chroma='420jpeg', color_range=None, xtags=(), ctag=None, depth=8,
                 layout='420'):
        self.w, self.h, self.fps = int(w), int(h), Fraction(fps)
        self.interlace, self.aspect, self.chroma = interlace, aspect, chroma
        self.color_range = color_range
        self.xtags = list(xtags)
        self.ctag = ctag
        self.depth = check_depth(depth)
        self.layout = check_layout(layout)

    @property
    def full_range(self):
        return self.color_range == 'FULL'

    @property
    def payload(self):
        return payload_bytes(self.h, self.w, self.depth, self.layout)

    @property
    def samples(self):
        """samples of one payload (what the scene-cut scores count)"""
        return payload_size(self.h, self.w, self.layout)

    @property
    def peak(self):
        return (1 << self.depth) - 1

    @property
    def frame_bytes(self):
        """bytes of one frame written by this module: 'FRAME\\n' + payload"""
        return len(FRAME) + 1 + self.payload

    def encode(self):
        p = [MAGIC, b'W%d' % self.w, b'H%d' % self.h, b'F%d:%d' % (self.fps.numerator, self.fps.denominator),
             b'I' + self.interlace.encode()]
        if self.aspect is not None:
            p.append(b'A' + self.aspect.encode())
        if self.ctag is not None:
            p.append(b'C' + self.ctag.encode())
        p += [b'X' + x.encode() for x in self.xtags]
        if self.color_range is not None:
            p.append(b'XCOLORRANGE=' + self.color_range.encode())
        return b' '.join(p) + b'\n'

    def __repr__(self):
        return 'Header(%r)' % self.encode()


def _reject(what, hint=''):
    raise Y4MError('Y4M: %s is not supported: %s%s' % (what, FIX, hint))


_DEEP = {'420p%d' % d: d for d in DEPTHS if d > 8}                    # 4:2:0 tags of 16-bit samples (420jpeg siting)
# tags of the other layouts -> (layout, depth): C422 / C444 / Cmono, and C422pNN / C444pNN / CmonoNN of 16-bit samples
_LAYOUT_TAGS = dict([(lay, (lay, 8)) for lay in LAYOUTS[1:]] +
                    [(('mono%d' if lay == 'mono' else lay + 'p%d') % d, (lay, d)) for lay in LAYOUTS[1:] for d in DEPTHS if d > 8])
_LAYOUT_NAMES = {'420': '4:2:0', '422': '4:2:2', '444': '4:4:4', 'mono': 'mono'}


def parse_header(line, depths=(8,), layouts=('420',), fields=False, telecine=False):
    """One header line (bytes, with or without the trailing newline) -> Header.  Raises Y4MError.  ``depths``: the bit depths
    taken; the default is 8-bit only, ``DEPTHS`` also takes C420p10 / C420p12 / C420p14 / C420p16.  ``layouts``: the chroma
    layouts taken; the default is 4:2:0 only, ``LAYOUTS`` also takes C422 / C444 / Cmono and, with ``depths=DEPTHS``, their deep
    forms C422pNN / C444pNN / CmonoNN.  ``fields``: also take interlaced streams of a fixed field order, ``It`` and ``Ib``
    (``Header.interlace`` is then 't' or 'b'; ``demfi_amd.deint`` makes frames of their fields); mixed-mode ``Im`` stays refused.
    ``telecine``: also take ``It``, ``Ib`` and ``Im`` (``Header.interlace`` 't', 'b' or 'm') for inverse telecine, which matches
    fields whatever their flagged order (``demfi_amd.telecine``)."""
    if isinstance(line, str):
        line = line.encode()
    line = line.rstrip(b'\n')
    toks = line.split(b' ')
    if toks[0] != MAGIC:
        raise Y4MError('not a YUV4MPEG2 stream (bad magic %r): %s' % (bytes(line[:16]), FIX))
    w = h = fps = None
    inter, aspect, ctag, crange, xt, depth, layout = 'p', None, None, None, [], 8, '420'
    for t in toks[1:]:
        if not t:
            continue
        tag, val = chr(t[0]), t[1:].decode('ascii', 'replace')
        if tag in 'WH':
            if not re.fullmatch(r'\d{1,9}', val):
                raise Y4MError('Y4M: bad %s%s' % (tag, val))
            if tag == 'W':
                w = int(val)
            else:
                h = int(val)
        elif tag == 'F':
            m = re.fullmatch(r'(\d{1,9}):(\d{1,9})', val)
            if not m or int(m.group(1)) == 0 or int(m.group(2)) == 0:
                raise Y4MError('Y4M: bad frame rate F%s' % val)
            fps = Fraction(int(m.group(1)), int(m.group(2)))
        elif tag == 'I':
            if val == 'm' and not telecine:
                _reject('mixed-mode interlaced video (Im)', MIXED_HINT)
            if val not in ('p', '?') and not ((fields or telecine) and val in ('t', 'b')) and not (telecine and val == 'm'):
                _reject('interlaced video (I%s)' % val, DEINTERLACE_HINT if val in ('t', 'b') else '')
            inter = val
        elif tag == 'A':
            aspect = val
        elif tag == 'C':
            names = ', '.join(_LAYOUT_NAMES[x] for x in layouts)
            only = '8-bit %s only' % names if tuple(depths) == (8,) else '%s only, %s bits' % (names, ', '.join(str(d) for d in depths))
            if val in _DEEP:
                if _DEEP[val] not in depths:
                    _reject('colour space C%s (8-bit 4:2:0 only)' % val, HIGH_DEPTH_HINT)
                depth, layout = _DEEP[val], '420'
            elif val in _LAYOUT_TAGS:
                lay, d = _LAYOUT_TAGS[val]
                if lay not in layouts:
                    _reject('colour space C%s (%s)' % (val, only), ANY_LAYOUT_HINT)
                if d not in depths:
                    _reject('colour space C%s (8-bit %s only)' % (val, names),
                            '; or keep the bit depth: --high-depth accepts 10- to 16-bit samples (C%s)' % val)
                depth, layout = d, lay
            elif val not in _CHROMA:
                _reject('colour space C%s (%s)' % (val, only))
            else:
                depth, layout = 8, '420'
            ctag = val
        elif tag == 'X':
            if val.startswith('COLORRANGE='):
                crange = val.split('=', 1)[1]
                if crange not in ('FULL', 'LIMITED'):
                    raise Y4MError('Y4M: bad XCOLORRANGE=%s (FULL or LIMITED)' % crange)
            else:
                xt.append(val)
        # other tags: ignored, as the format says
    if w is None or h is None:
        raise Y4MError('Y4M: header lacks W / H')
    if fps is None:
        raise Y4MError('Y4M: header lacks the frame rate F')
    for nm, v in (('width', w), ('height', h)):
        if not 2 <= v <= MAX_SIDE:
            raise Y4MError('Y4M: %s %d outside 2..%d' % (nm, v, MAX_SIDE))
    return Header(w, h, fps, inter, aspect, _CHROMA.get(ctag, '420jpeg'), crange, xt, ctag, depth, layout)


def output_ctag(depth, layout='420'):
    """C tag of an output stream: 420jpeg, or the input's 420pNN (420jpeg siting) above 8 bits; for the other layouts the
    input's own tag: 422 / 444 / mono, 422pNN / 444pNN / monoNN above 8 bits."""
    if check_layout(layout) == '420':
        return '420jpeg' if depth == 8 else '420p%d' % depth
    return layout if depth == 8 else ('mono%d' if layout == 'mono' else layout + 'p%d') % depth


def output_header(hdr, mfi):
    """Header of the x M stream: the input's W H, F x M (reduced), progressive, A copied, C420jpeg (C420pNN at the input's depth
    above 8 bits; the input's layout and depth for 4:2:2, 4:4:4 and mono), the input's XCOLORRANGE."""
    return Header(hdr.w, hdr.h, hdr.fps * mfi, 'p', hdr.aspect, '420jpeg', hdr.color_range, (), output_ctag(hdr.depth, hdr.layout),
                  hdr.depth, hdr.layout)


# ---- stream order of the x M output ----------------------------------------------------------------------------------------
def n_output_frames(n_in, mfi):
    """(n-3)*M + 1: per window S0 and the M-1 St, then the last window's S1; the first and last input frames have no output."""
    return (n_in - 3) * mfi + 1 if n_in >= 4 else 0


def output_index(k, j, mfi):
    """Stream position of frame j of window k: j = 0 is S0 (deblurred B0), j = 1 .. M-1 is St at t = j/M, j = M is S1 (only
    written for the last window)."""
    return k * mfi + j


def frame_offset(hdr_len, i, payload):
    """Byte offset of output frame i in a file written by this module ('FRAME\\n' before every payload of ``payload`` bytes)."""
    return hdr_len + i * (len(FRAME) + 1 + payload)


# ---- reading -------------------------------------------------------------------------------------------------------------
def _readline(f, what):
    line = f.readline(_MAX_LINE)
    if line and not line.endswith(b'\n'):
        raise Y4MError('Y4M: %s line longer than %d bytes or cut off' % (what, _MAX_LINE))
    return line


def _readinto_full(f, mv):
    """readinto until mv is full (a pipe returns short reads); returns the bytes read."""
    got = 0
    while got < len(mv):
        k = f.readinto(mv[got:])
        if not k:
            break
        got += k
    return got


def _frame_line(line, index):
    if not (line == FRAME + b'\n' or line.startswith(FRAME + b' ')):
        raise Y4MError('Y4M: frame %d does not start with FRAME (got %r)' % (index, bytes(line[:16])))


class Reader:
    """Sequential reader of a binary stream (a file, or stdin: nothing is seeked).  ``read_into(buf)`` fills one payload."""

    def __init__(self, f, depths=(8,), layouts=('420',), fields=False, telecine=False):
        self.f = f
        line = _readline(f, 'header')
        if not line:
            raise Y4MError('Y4M: empty input: %s' % FIX)
        self.header = parse_header(line, depths, layouts, fields, telecine)
        self.header_bytes = len(line)
        self.index = 0                                  # frames read so far

    def read_into(self, buf):
        """Next frame's payload into ``buf`` (writable, payload bytes).  False at a clean end of stream; a truncated frame raises."""
        line = _readline(self.f, 'FRAME')
        if not line:
            return False
        _frame_line(line, self.index)
        mv = memoryview(buf).cast('B')
        if len(mv) != self.header.payload:
            raise ValueError('buffer of %d bytes for a payload of %d' % (len(mv), self.header.payload))
        got = _readinto_full(self.f, mv)
        if got != len(mv):
            raise Y4MError('Y4M: truncated frame %d (%d of %d bytes)' % (self.index, got, len(mv)))
        self.index += 1
        return True


def scan(f, depths=(8,), layouts=('420',), fields=False, telecine=False):
    """One pass over the frame headers of a seekable file: (Header, header bytes, [file offset of every payload]).  The
    payloads are skipped, not read; a truncated last frame raises.  ``depths``, ``layouts``, ``fields``, ``telecine``: as ``parse_header``."""
    f.seek(0)
    rd = Reader(f, depths, layouts, fields, telecine)
    size = os.fstat(f.fileno()).st_size if hasattr(f, 'fileno') else None
    p = rd.header.payload
    offs = []
    while True:
        line = _readline(f, 'FRAME')
        if not line:
            break
        _frame_line(line, len(offs))
        off = f.tell()
        end = size if size is not None else f.seek(0, io.SEEK_END)
        if off + p > end:
            raise Y4MError('Y4M: truncated frame %d (%d of %d bytes)' % (len(offs), end - off, p))
        offs.append(off)
        f.seek(off + p)
    return rd.header, rd.header_bytes, offs


def file_fetch(f, offsets):
    """fetch(i, buf) over a scanned file (``scan``): payload i of the file into ``buf`` by seek + readinto."""
    def fetch(i, buf):
        f.seek(offsets[i])
        mv = memoryview(buf).cast('B')
        if _readinto_full(f, mv) != len(mv):
            raise Y4MError('Y4M: truncated frame %d' % i)
        return True
    return fetch


class Frames:
    """``host_frames`` of ``WindowRunner.run_clip_u8`` over a Y4M input: frame i is its payload (1-D uint8 tensor of the payload's bytes,
    pinned when a GPU is present), read with ``readinto`` when first needed and dropped once the windows have moved past it (windows come in
    increasing order and read frames k .. k+3).  ``peak`` = frames held at once: bounded by the runner's batch + 5, whatever
    the input's length.

    Frames(reader): the frames of a stream, read in order (stdin: nothing is seeked).
    Frames.from_file(f, offsets, first, stop): frames first .. stop-1 of a scanned file (``scan``), by seek + readinto (with
    ``behind`` = b: frames first-b .. stop+b-1, as far as the file has them).
    ``full_length``: ``windows`` / ``is_last`` follow the full-length timeline (``retime``).
    ``fields`` = 2 (an interlaced input, ``demfi_amd.deint``): index i is FIELD i, and both fields of payload i // 2 are the
    same tensor: the payload is read once and never copied.  ``first`` / ``stop``, ``n``, ``is_last``, ``windows`` and the
    dropping count fields; ``peak`` counts the payload tensors held.
    ``behind`` = b (default 0: nothing changes): for a consumer that also reads the b frames before every frame it names and the
    frames after it (the motion-adaptive deinterlacer, b = 2 fields; the temporal denoiser, b = R frames or 2 R fields): the input starts b frames earlier (at frame 0 at the
    earliest) and b more frames are kept behind, so ``peak`` grows by at most the payloads those b frames and the b frames read
    ahead by ``has`` add."""

    def __init__(self, reader=None, payload=None, fetch=None, first=0, stop=None, pinned=None, full_length=False, fields=1, behind=0):
        import torch
        if fields not in (1, 2):
            raise ValueError('Frames: fields must be 1 or 2, got %r' % (fields,))
        self.payload = reader.header.payload if reader is not None else payload
        self._fetch = fetch or (lambda i, buf: reader.read_into(buf))
        if int(behind) != behind or behind < 0:
            raise ValueError('Frames: behind must be an integer >= 0, got %r' % (behind,))
        self.fields, self.behind = fields, int(behind)
        first = max(first - self.behind, 0)
        self.next, self.stop = first - first % fields, stop
        self.pinned = torch.cuda.is_available() if pinned is None else pinned
        self.full_length = full_length
        self.buf = {}
        self.n = None                                   # index one past the last frame, once the end was seen
        self.first_window = None                        # global index of the first window handed out by ``windows``
        self.peak = 0

    @classmethod
    def from_file(cls, f, offsets, first, stop, payload, pinned=None, fields=1, behind=0):
        return cls(payload=payload, fetch=file_fetch(f, offsets), first=first, stop=min(stop + behind, fields * len(offsets)), pinned=pinned,
                   fields=fields, behind=behind)

    def has(self, i):
        """Reads through frame i; False when the input ends before it."""
        import torch
        while self.next <= i and self.n is None:
            t = torch.empty(self.payload, dtype=torch.uint8, pin_memory=self.pinned)
            if (self.stop is not None and self.next >= self.stop) or not self._fetch(self.next // self.fields, t.numpy()):
                self.n = self.next
                break
            for j in range(self.next, self.next + self.fields):          # the fields of a payload share its tensor
                self.buf[j] = t
            self.next += self.fields
            if self.stop is not None:
                self.next = min(self.next, self.stop)
            self.peak = max(self.peak, len({j // self.fields for j in self.buf}))
        return i < self.next

    def __getitem__(self, i):
        if not self.has(i):
            raise IndexError('Y4M frame %d: the input has %d frames' % (i, self.n))
        for j in [j for j in self.buf if j < i - 3 - self.behind]:
            del self.buf[j]
        if i not in self.buf:
            raise IndexError('Y4M frame %d was already dropped (frames are read in window order)' % i)
        return self.buf[i]

    def windows(self, first=0):
        """(B0, B1, B-1, B2) of window k = first, first+1, ... while the input has frame k+3; frame k+4 is read ahead, so
        ``is_last(k)`` is known when window k is handed out.
        ``full_length``: window k = -1, 0, ... while the input has frame k+2, on its tuple clamped at the clip's ends
        (``scene.clip_tuple``); frame k+3 is read ahead, and its absence makes window k the last.  A one-frame input has the
        single window -2 on frame 0.  ``first_window`` is set before the first window is handed out."""
        if not self.full_length:
            self.first_window = k = first
            while self.has(k + 3):
                self.has(k + 4)
                yield (k + 1, k + 2, k, k + 3)
                k += 1
            return
        from . import scene as S
        if not self.has(0):
            return
        self.first_window = k = -1 if self.has(1) else -2
        while k == -2 or self.has(k + 2):
            self.has(k + 3)
            yield S.runner_order(S.clip_tuple(k, S.with_sentinels(lambda j: False, self.n)))
            if k == -2:
                return
            k += 1

    def is_last(self, k):
        return self.n is not None and self.n == k + (3 if self.full_length else 4)


class Writer:
    """Writes the header (unless ``at`` is given: then the frames go at byte offset ``at`` of a file another rank sized),
    then frames ('FRAME\\n' + payload) in stream order."""

    def __init__(self, f, header, at=None):
        self.f = f
        self.header = header
        self.header_bytes = header.encode()
        if at is None:
            f.write(self.header_bytes)
        else:
            f.seek(at)
        self.frames = 0

    def write(self, payloads):
        """payloads: uint8 [n, payload bytes] (numpy array / CPU tensor; uint16 rows are written as they lie in memory) in
        stream order."""
        for p in payloads:
            self.f.write(FRAME + b'\n')
            self.f.write(memoryview(p.numpy() if hasattr(p, 'numpy') else np.asarray(p)).cast('B'))
            self.frames += 1
