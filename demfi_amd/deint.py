"""Interlaced Y4M input (``python -m demfi_amd.video --deinterlace``): the definition of the bob and its timeline.

A payload of an interlaced stream (``It``: top field first, ``Ib``: bottom field first) holds two fields taken half a frame
period apart: the even rows of every plane are the top field, the odd rows the bottom field.  The bob makes one progressive
frame per field, at the field's own time instant: field f = 2p + s of payload p (s = 0 is the first field in time) is
progressive frame f, so n payloads at F frames/s are a progressive stream of 2n frames at 2F, and everything behind the bob
(retiming, scene cuts, repeated frames, tiles, the network, the egress) runs on that stream unchanged.

``bob_plane_np`` DEFINES the bob of one plane; the HIP kernel (csrc/deint.hip, ``demfi_yuv_bob``) matches it sample for sample.
The rows of the field are kept, the rows between them are rebuilt by the classic five-direction edge-directed line average:
with a = row y-1 and b = row y+1 (column indices clamped to the plane), score(j) = sum over k = -1, 0, 1 of
|a[x+k+j] - b[x+k-j]| measures how well the line through a[x+j] and b[x-j] continues an edge, and pred(j) =
(a[x+j] + b[x-j] + 1) >> 1 is the average along it.  The vertical average pred(0) is the start (best = score(0) - 1, so a
direction must beat it by more than a tie); j = -1 is taken when score(-1) < best and only then is j = -2 tried; then, whatever
happened on the left, j = +1 is tried against the running best and, if taken, j = +2.  Integers throughout, no state between
pixels; the result lies between two samples of the plane.  A missing row with one neighbour inside the plane copies it; a
plane without a kept row (one row, and the odd rows are kept) is returned as it is.

``bob_payload_np`` applies it to every plane of a payload: Y and, by their own shapes (``y4m.chroma_shape``), Cb and Cr.  In
interlaced 4:2:0 the chroma rows alternate between the fields as the luma rows do.  Known limit: a field's chroma rows are
taken to sit at the plane's own row positions; the quarter-row vertical offset that interlaced 4:2:0 chroma has per field is
not modelled.

Out of scope: motion-adaptive or temporal deinterlacing (it would need the neighbouring payloads resident at the bob), inverse
telecine, mixed-mode streams (``Im``) and interlaced output.
"""
import numpy as np

from . import y4m


def field_parity(order, f):
    """Parity q of the rows field f keeps (0: even rows, the top field; 1: odd rows): ``order`` 't' starts with the top field,
    'b' with the bottom field."""
    if order not in ('t', 'b'):
        raise ValueError("field order must be 't' or 'b', got %r" % (order,))
    return (int(f) & 1) ^ int(order == 'b')


def progressive_header(hdr):
    """Header of the bobbed stream: progressive (``Ip``) at twice the rate, everything else kept."""
    return y4m.Header(hdr.w, hdr.h, hdr.fps * 2, 'p', hdr.aspect, hdr.chroma, hdr.color_range, hdr.xtags, hdr.ctag, hdr.depth, hdr.layout)


def bob_plane_np(plane, q):
    """``plane`` [rows, cols] of integers with the rows of parity ``q`` kept (0: even, 1: odd) -> the plane with the other rows
    rebuilt from them (the module's docstring); same dtype."""
    p = np.asarray(plane)
    if p.ndim != 2 or q not in (0, 1):
        raise ValueError('bob_plane_np: a [rows, cols] plane and q in (0, 1), got %s and %r' % (p.shape, q))
    rows, cols = p.shape
    out = p.copy()
    if rows <= q or cols == 0:                                # no kept row
        return out
    for y in range(1 - q, rows, 2):                           # a missing row at an end of the plane has one neighbour
        if y == 0 or y == rows - 1:
            out[y] = p[y + 1] if y == 0 else p[y - 1]
    ys = np.arange(1 - q, rows, 2)
    ys = ys[(ys >= 1) & (ys + 1 < rows)]
    if ys.size == 0:
        return out
    a, b = p[ys - 1].astype(np.int64), p[ys + 1].astype(np.int64)
    xs = np.arange(cols)

    def at(r, off):
        return r[:, np.clip(xs + off, 0, cols - 1)]

    def score(j):
        return sum(np.abs(at(a, k + j) - at(b, k - j)) for k in (-1, 0, 1))

    def pred(j):
        return (at(a, j) + at(b, -j) + 1) >> 1
    best, res = score(0) - 1, pred(0)
    for side in (-1, 1):
        taken = np.ones(best.shape, bool)
        for j in (side, 2 * side):
            s = score(j)
            taken = taken & (s < best)
            best, res = np.where(taken, s, best), np.where(taken, pred(j), res)
    out[ys] = res.astype(p.dtype)
    return out


def bob_payload_np(payload, h, w, depth, layout, q):
    """One payload (depth 8: bytes-like or a uint8 array; above: 16-bit little-endian samples as bytes or a uint16 array) of an
    h x w frame in ``layout`` with the field of parity ``q`` kept -> the progressive payload, 1-D uint8 / uint16: ``bob_plane_np``
    of Y, Cb and Cr."""
    y4m.check_depth(depth)
    a = y4m.as_samples16(payload) if depth > 8 else (np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray)
                                                    else payload.reshape(-1))
    if depth == 8 and a.dtype != np.uint8:
        raise ValueError('a payload of 8-bit samples is a uint8 array, got %s' % a.dtype)
    planes = y4m.split_planes_layout(a, h, w, y4m.check_layout(layout))
    return np.concatenate([bob_plane_np(p, q).reshape(-1) for p in planes if p is not None])
