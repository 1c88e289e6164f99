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

``adaptive_plane_np`` DEFINES the motion-adaptive mode (``--deinterlace-mode adaptive``; csrc/deint.hip,
``demfi_yuv_deint_adaptive``): yadif's temporal rule (the ``filter_line`` of ffmpeg's filter with the spatial check on) around this
module's own spatial predictor.  Field f of parity q keeps its rows; a missing row y with both neighbours inside the plane is
rebuilt sample by sample from the fields around it in time, each read ONLY at rows of its own parity out of the payload that holds
it: P1 = field f-1 and N1 = field f+1 (parity 1-q: rows y, y-2, y+2), P2 = field f-2 and N2 = field f+2 (parity q: rows y-1, y+1).
With c = cur[y-1][x] and e = cur[y+1][x]:

    d  = (P1[y][x] + N1[y][x]) >> 1
    t0 = |P1[y][x] - N1[y][x]| >> 1
    t1 = (|P2[y-1][x] - c| + |P2[y+1][x] - e|) >> 1
    t2 = (|N2[y-1][x] - c| + |N2[y+1][x] - e|) >> 1
    diff = max(t0, t1, t2)

and, when y-2 >= 0 and y+2 < rows, the spatial check

    b  = (P1[y-2][x] + N1[y-2][x]) >> 1        g  = (P1[y+2][x] + N1[y+2][x]) >> 1
    mx = max(d-e, d-c, min(b-c, g-e))          mn = min(d-e, d-c, max(b-c, g-e))
    diff = max(diff, mn, -mx)

    out = clamp(sp, d - diff, d + diff),  sp = the bob's value at (y, x), exactly ``bob_plane_np``'s

Integers throughout, no state between samples.  A missing row with one neighbour copies it and a plane without a kept row is
returned as it is, as in the bob.  A field absent at an end of the stream is replaced by its partner on the other side in time (P1
by N1 or N1 by P1, P2 by N2 or N2 by P2); every payload has two fields, so one of P1 and N1 always exists in a stream, and the
function given neither returns the bob's value (the kernel does the same); with P2 and N2 both absent (a one-payload stream) t1 and
t2 are dropped.  So a static scene comes back at full vertical resolution (diff = 0, out = d = the source row) and where the
picture moves diff is large and out = sp, the bob.  Scene cuts need nothing special for the same reason: across a cut diff is large
and the result falls back to the spatial value.  Output field f depends on payloads p-1, p and p+1 of the input only.

Out of scope: ``--dedup`` together with the adaptive mode (repeated frames are staged and discarded one field at a time, the
adaptive mode needs two fields of lookahead; ``--deinterlace-mode bob`` is the way out), mixed-mode streams (``Im``).  Interlaced
output is ``demfi_amd.interlace`` (``--interlace``), which weaves by this module's field convention.  Film carried by 3:2 pulldown is not deinterlaced but put back together: ``demfi_amd.telecine`` (``--ivtc``).
"""
import numpy as np

from . import y4m

MODES = ('bob', 'adaptive')

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
    ys = _interior_rows(rows, q)
    if ys.size == 0:
        return out
    out[ys] = edge_average_np(p[ys - 1], p[ys + 1]).astype(p.dtype)
    return out


def _interior_rows(rows, q):
    """The missing rows (parity 1-q) of a plane of ``rows`` rows that have both neighbours inside it."""
    ys = np.arange(1 - q, rows, 2)
    return ys[(ys >= 1) & (ys + 1 < rows)]


def edge_average_np(a, b):
    """The bob's spatial value of the rows between rows ``a`` (above) and ``b`` (below), [m, cols] each -> int64 [m, cols]: the
    five-direction edge-directed line average of the module's docstring.  ``bob_plane_np`` and ``adaptive_plane_np`` share it."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    cols = a.shape[1]
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
    return res


def adaptive_bounds_np(planes, q):
    """(ys, d, diff) of ``adaptive_plane_np``: the interior missing rows and, int64 [len(ys), cols] each, the temporal average d and
    the half-width diff of the interval [d - diff, d + diff] the spatial value is clamped to.  None when P1 and N1 are both absent."""
    p2, p1, cur, n1, n2 = [None if p is None else np.asarray(p) for p in planes]
    if cur is None or cur.ndim != 2 or q not in (0, 1) or any(p is not None and p.shape != cur.shape for p in (p2, p1, n1, n2)):
        raise ValueError('adaptive_plane_np: (P2, P1, cur, N1, N2) planes of one [rows, cols] shape (None: absent) and q in (0, 1)')
    if p1 is None and n1 is None:
        return None
    p1, n1 = (n1 if p1 is None else p1), (p1 if n1 is None else n1)
    p2, n2 = (n2 if p2 is None else p2), (p2 if n2 is None else n2)
    rows = cur.shape[0]
    ys = _interior_rows(rows, q) if rows > q else np.arange(0)

    def at(p, r):
        return p[r].astype(np.int64)
    c, e = at(cur, ys - 1), at(cur, ys + 1)
    py, ny = at(p1, ys), at(n1, ys)
    d = (py + ny) >> 1
    diff = np.abs(py - ny) >> 1
    if p2 is not None:
        for t in (p2, n2):
            diff = np.maximum(diff, (np.abs(at(t, ys - 1) - c) + np.abs(at(t, ys + 1) - e)) >> 1)
    ok = (ys - 2 >= 0) & (ys + 2 < rows)                       # rows y-2 and y+2 exist: the spatial check
    up, dn = np.where(ok, ys - 2, ys), np.where(ok, ys + 2, ys)
    b, g = (at(p1, up) + at(n1, up)) >> 1, (at(p1, dn) + at(n1, dn)) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, g - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, g - e))
    diff = np.where(ok[:, None], np.maximum(diff, np.maximum(mn, -mx)), diff)
    return ys, d, diff


def adaptive_plane_np(planes, q):
    """``planes`` = (P2, P1, cur, N1, N2): the planes [rows, cols] that hold fields f-2 .. f+2 (None for a field the stream does not
    have), field f of parity ``q`` kept in ``cur`` -> ``cur`` with its other rows rebuilt by the motion-adaptive rule (the module's
    docstring); same dtype.  Of P1 and N1 only rows of parity 1-q are read, of P2 and N2 only rows of parity q, of ``cur`` only its
    kept rows: what the other rows of any of them hold does not matter."""
    cur = np.asarray(planes[2])
    out = bob_plane_np(cur, q)
    bounds = adaptive_bounds_np(planes, q)
    if bounds is None or bounds[0].size == 0:
        return out
    ys, d, diff = bounds
    out[ys] = np.clip(out[ys].astype(np.int64), d - diff, d + diff).astype(cur.dtype)
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


def _samples(payload, depth):
    a = y4m.as_samples16(payload) if depth > 8 else (np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray)
                                                    else payload.reshape(-1))
    if depth == 8 and a.dtype != np.uint8:
        raise ValueError('a payload of 8-bit samples is a uint8 array, got %s' % a.dtype)
    return a


def adaptive_payload_np(payloads, h, w, depth, layout, q):
    """``payloads`` = the five payloads (as ``bob_payload_np`` takes one; None for an absent field) that hold fields f-2, f-1, f, f+1
    and f+2 of an h x w stream in ``layout``, field f of parity ``q`` -> the progressive payload of field f, 1-D uint8 / uint16:
    ``adaptive_plane_np`` of Y, Cb and Cr by their own shapes."""
    y4m.check_depth(depth)
    if len(payloads) != 5 or payloads[2] is None:
        raise ValueError('adaptive_payload_np: five payloads (f-2 .. f+2), that of field f not None')
    split = [None if p is None else y4m.split_planes_layout(_samples(p, depth), h, w, y4m.check_layout(layout)) for p in payloads]
    return np.concatenate([adaptive_plane_np([None if s is None else s[i] for s in split], q).reshape(-1)
                           for i in range(3) if split[2][i] is not None])


def field_neighbours(f, n_fields):
    """Fields f-2, f-1, f, f+1, f+2 of a stream of ``n_fields`` fields, None for one the stream does not have."""
    return [g if 0 <= g < n_fields else None for g in range(f - 2, f + 3)]


def adaptive_stream_np(payloads, h, w, depth, layout, order):
    """The payloads of an interlaced stream of field order ``order`` -> the 2n progressive payloads of the adaptive mode: field
    f = 2p + s from the payloads that hold fields f-2 .. f+2."""
    n = 2 * len(payloads)
    return [adaptive_payload_np([None if g is None else payloads[g // 2] for g in field_neighbours(f, n)], h, w, depth, layout,
                                field_parity(order, f)) for f in range(n)]
