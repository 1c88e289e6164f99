"""Linear light and the egress matrix / range of the Y4M edge (``demfi_amd.video --linear-light``, ``--out-matrix``, ``--out-range``): the
definitions, in numpy.  The module is the only source of the tables; the kernels of csrc/colour.hip compute no transfer function.

A shutter integrates light and a scaler should resample it, but the stored samples are gamma-encoded.  With ``--linear-light`` the gather
behind the network writes LINEAR payloads instead of Y'CbCr ones, the mix and the scaler work on those unchanged, and an encode stage
takes them back: gather-to-linear -> mix -> scale -> encode -> weave -> requant.

Transfers (``TRANSFERS``): 'bt709' is the OETF of BT.709 / BT.601 / BT.2020-SDR with its linear toe (V = 4.5 L below L = beta, else
alpha L^0.45 - (alpha - 1), with the unrounded alpha = 1.0993 and beta = 0.0181 at which the two segments meet) and 'srgb' the sRGB pair (V = 12.92 L below L = 0.0031308, else 1.055 L^(1/2.4) - 0.055).  Light is scene-linear
through the INVERSE OETF, not a display gamma, so its slope near black is finite and 16 bits of linear light are enough there.

Tables at working depth d (peak = 2^d - 1), d <= 12:
  ``forward_table``   fwd[c] = floor(65535 f^-1(c / peak) + 0.5), uint16 [peak + 1], float64 arithmetic; fwd[0] = 0, fwd[peak] = 65535.
  ``thresholds``      thr[c] = (fwd[c-1] + fwd[c] + 1) // 2 for c = 1 .. peak: the first linear value that is nearer to code c than to c-1
                      (a tie goes up).
  ``inverse_table``   inv[v] = the number of c in 1 .. peak with thr[c] <= v, uint16 [65536]: the code nearest in light.  Defined through
                      the thresholds, so indexing the table and a binary search over the thresholds are one function by construction.
At 8, 10 and 12 bits fwd increases strictly (its smallest step: bt709 57 / 14 / 3, srgb 19 / 4 / 1), so inv[fwd[c]] = c for every code:
a frame that is only linearised and encoded again keeps its codes.  At 14 and 16 bits fwd has ties and ``check_depth`` refuses.

A LINEAR PAYLOAD of an h x w frame is uint16 [3, h, w], planes B, G, R at full resolution, little-endian: 6 h w bytes whatever the working
depth and the chroma layout.  ``linearize_np`` makes one from a BGR frame of codes; ``encode_payload_np`` makes the Y'CbCr payload of the
run's depth and layout from one and defines nothing new behind the table: it is ``y4m.bgr16_to_yuv_np`` (``y4m.bgr_to_yuv_np`` at 8 bits)
of the codes inv[lin], with that function's rounding, 2x2 box and 4:2:2 [1,2,1].  Between the two the mix (``shutter.mix_np``) treats a
payload as a flat array of 16-bit samples and the scaler (``scale.scale_payload_np``) as three h x w planes at peak 65535.

``resolve`` gives the matrix and range a stream leaves with.  Every written sample is made from a BGR frame by the gather (or the encode
stage), which takes a matrix and a range: binding those to other values than the input's is all ``--out-matrix`` / ``--out-range`` do.
Not defined here: primaries / gamut conversion, PQ and HLG (``--lut`` applies a user's cube that holds them, ``demfi_amd.lut3d``), working
depths 14 and 16."""
import numpy as np

from . import scale as SC
from . import shutter as SH
from . import y4m

TRANSFERS = ('bt709', 'srgb')
MAX_DEPTH = 12
LIN_PEAK = 65535
OUT_MATRICES = ('auto',) + tuple(y4m.MATRICES)
OUT_RANGES = ('limited', 'full')
# BT.709's 1.099 and 0.018 are roundings of the pair that makes the toe and the power segment meet (BT.2020 gives them to more digits:
# 1.0993, 0.0181); with the rounded pair the curve jumps at the joint and the table's step there falls below the toe's
BT709_ALPHA, BT709_BETA = 1.09929682680944, 0.018053968510807


def check_transfer(name):
    """The transfer ``name``, one of ``TRANSFERS``; ValueError otherwise."""
    if name not in TRANSFERS:
        raise ValueError('linear-light transfer must be one of %s, got %r' % (', '.join(TRANSFERS), name))
    return name


def check_depth(depth):
    """Linear light at the working depth ``depth``: 8, 10 or 12.  Above, 16 bits of light no longer tell neighbouring codes apart."""
    if depth not in (8, 10, 12):
        raise ValueError('--linear-light needs a working depth of 8, 10 or 12 bits, got %r: above %d bits neighbouring codes share a '
                         '16-bit linear value and the way back is no longer exact; work at %d bits or below (--work-depth)'
                         % (depth, MAX_DEPTH, MAX_DEPTH))
    return depth


def to_linear(transfer, v):
    """f^-1: encoded values v in [0, 1] (float64 array) -> light in [0, 1]."""
    v = np.asarray(v, np.float64)
    if check_transfer(transfer) == 'bt709':
        return np.where(v < 4.5 * BT709_BETA, v / 4.5, ((v + (BT709_ALPHA - 1.0)) / BT709_ALPHA) ** (1.0 / 0.45))
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def forward_table(transfer, depth):
    """fwd[c], uint16 [peak + 1]: the linear value of code c at the working depth."""
    peak = (1 << check_depth(depth)) - 1
    fwd = np.floor(LIN_PEAK * to_linear(transfer, np.arange(peak + 1, dtype=np.float64) / peak) + 0.5)
    fwd = np.clip(fwd, 0, LIN_PEAK).astype(np.uint16)
    assert fwd[0] == 0 and fwd[peak] == LIN_PEAK and (np.diff(fwd.astype(np.int64)) > 0).all()
    return fwd


def thresholds(fwd):
    """thr[c] for c = 1 .. peak as index c - 1 of an int64 [peak] array."""
    f = np.asarray(fwd, np.int64)
    return (f[:-1] + f[1:] + 1) // 2


def inverse_table(fwd):
    """inv[v], uint16 [65536]: the code nearest in light to the linear value v."""
    return np.searchsorted(thresholds(fwd), np.arange(LIN_PEAK + 1, dtype=np.int64), side='right').astype(np.uint16)


def tables(transfer, depth):
    """(fwd, inv) of a transfer at a working depth."""
    fwd = forward_table(transfer, depth)
    return fwd, inverse_table(fwd)


def linearize_np(bgr, fwd):
    """BGR codes [h, w, 3] (uint8, or uint16 at the working depth) -> the linear payload, '<u2' [3, h, w]."""
    bgr = np.asarray(bgr)
    if bgr.dtype not in (np.uint8, np.uint16) or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError('linearize_np: uint8 or uint16 [h,w,3] expected, got %s %s' % (bgr.dtype, bgr.shape))
    if int(bgr.max(initial=0)) >= len(fwd):
        raise ValueError('linearize_np: code %d above the peak %d of the table' % (int(bgr.max()), len(fwd) - 1))
    return np.ascontiguousarray(np.asarray(fwd, np.uint16)[bgr].transpose(2, 0, 1)).astype('<u2', copy=False)


def delinearize_np(lin, inv, depth):
    """The linear payload [3, h, w] -> BGR codes [h, w, 3] at the working depth (uint8 at 8 bits, else uint16)."""
    lin = np.asarray(lin)
    if lin.dtype.itemsize != 2 or lin.dtype.kind != 'u' or lin.ndim != 3 or lin.shape[0] != 3:
        raise ValueError('a linear payload is uint16 [3,h,w], got %s %s' % (lin.dtype, lin.shape))
    codes = np.asarray(inv, np.uint16)[lin].transpose(1, 2, 0)
    return np.ascontiguousarray(codes.astype(np.uint8 if depth == 8 else np.uint16))


def encode_payload_np(lin, inv, depth, layout, matrix='bt601', full_range=False):
    """The linear payload [3, h, w] -> the Y'CbCr payload of ``depth`` and ``layout`` (1-D uint8 at 8 bits, else '<u2'): the existing
    definition of the gather over the codes inv[lin]."""
    bgr = delinearize_np(lin, inv, check_depth(depth))
    if depth == 8:
        return y4m.bgr_to_yuv_np(bgr, layout, matrix, full_range)
    return y4m.bgr16_to_yuv_np(bgr, depth, layout, matrix, full_range)


def linear_stream_np(frames, groups, transfer, depth, layout, matrix='bt601', full_range=False, scale=None, weights=None):
    """The written payloads of a linear-light run, as uint8 byte arrays: ``frames`` are the fine BGR frames [h, w, 3] of a timeline (codes
    at ``depth``), ``groups`` the fine indices each written frame mixes (``shutter.groups``; None: every frame is written as it is) with
    ``weights`` as ``shutter.mix_np`` takes them, ``scale`` None or (w, h, filter).  linearize -> mix over the flat linear payloads -> scale
    over three planes at peak 65535 -> encode."""
    fwd, inv = tables(transfer, depth)
    h, w = np.asarray(frames[0]).shape[:2]
    lin = np.stack([linearize_np(f, fwd).reshape(-1) for f in frames]).view(np.uint8)
    if groups is not None:
        lin = SH.mix_np(lin, groups, 2, weights)
    out = []
    for p in lin:
        p = np.ascontiguousarray(p).view('<u2')
        if scale is not None and tuple(scale[:2]) != (w, h):
            p = SC.scale_payload_np(p.astype(np.uint16), h, w, scale[1], scale[0], 16, '444', scale[2] if len(scale) > 2 else None)
            p = p.reshape(3, scale[1], scale[0])
        else:
            p = p.reshape(3, h, w)
        out.append(np.ascontiguousarray(encode_payload_np(p, inv, depth, layout, matrix, full_range)).view(np.uint8))
    return out


def check_switches(linear_light=None, out_matrix=None, out_range=None):
    """The three switches checked as far as they can be before a header is known: (transfer or None, out_matrix or None, out_range or
    None).  ``linear_light`` True means 'bt709'."""
    if linear_light is False:
        linear_light = None
    if linear_light is True:
        linear_light = TRANSFERS[0]
    if linear_light is not None:
        check_transfer(linear_light)
    if out_matrix is not None and out_matrix not in OUT_MATRICES:
        raise ValueError('out_matrix must be one of %s, got %r' % (', '.join(OUT_MATRICES), out_matrix))
    if out_range is not None and out_range not in OUT_RANGES:
        raise ValueError('out_range must be one of %s, got %r' % (', '.join(OUT_RANGES), out_range))
    return linear_light, out_matrix, out_range


def resolve(out_matrix, out_range, in_matrix, in_full, out_h):
    """The (matrix name, full_range) a stream leaves with: ``out_matrix`` None is the input's ``in_matrix``, 'auto' is
    ``y4m.auto_matrix(out_h)`` of the height actually written; ``out_range`` None is the input's ``in_full``."""
    _, out_matrix, out_range = check_switches(None, out_matrix, out_range)
    if in_matrix not in y4m.MATRICES:
        raise ValueError('resolve: the input matrix is one of %s, got %r' % (', '.join(y4m.MATRICES), in_matrix))
    matrix = in_matrix if out_matrix is None else y4m.auto_matrix(out_h) if out_matrix == 'auto' else out_matrix
    return matrix, bool(in_full) if out_range is None else out_range == 'full'


def range_tag(color_range, out_full):
    """The XCOLORRANGE value of the output header: ``color_range`` is the input's (None: no tag).  FULL / LIMITED is written when the
    range changes or the input carried the tag; an untagged stream that keeps its (limited) range stays untagged."""
    if bool(out_full) == (color_range == 'FULL'):
        return color_range
    return 'FULL' if out_full else 'LIMITED'


def range_header(hdr, out_full):
    """``hdr`` with the range tag of ``range_tag``.  Y4M has no matrix tag: the matrix does not show in the header."""
    return y4m.Header(hdr.w, hdr.h, hdr.fps, hdr.interlace, hdr.aspect, hdr.chroma, range_tag(hdr.color_range, out_full), hdr.xtags,
                      hdr.ctag, hdr.depth, hdr.layout)
