"""Deblocking of the Y4M video path in front of the network (``python -m demfi_amd.video --deblock [A[:B]]``): DV, 576i / 480i captures, NTSC
DVDs behind ``--ivtc`` and broadcast captures are 8x8-DCT coded and arrive with block edges, a deblurring network sharpens a block edge like
any other, and the flow sees a grid that never moves over content that does.  Pure Python / numpy; the one module that knows the rule.

The rule is H.264's intra-edge (bS = 4) luma filter, applied as a post filter on a fixed 8-sample grid to every plane as a plane in its own
right.  A and B are 8-bit steps (0 <= B <= A <= 255; default 16:4; A alone means A : (A + 3) // 4) and one pair serves every plane; at the
working depth d: a = A << (d - 8), b = B << (d - 8), s = (a >> 2) + (2 << (d - 8)).  A plane of ``cols`` samples a row whose left Lp columns
were removed by ``--crop`` (0 otherwise) has a vertical block edge at column x when (x + Lp) % 8 == 0 and 4 <= x <= cols - 4, that is when
all eight samples x-4 .. x+3 exist; rows likewise with the Tp rows removed at the top.  One line p3 p2 p1 p0 | q0 q1 q2 q3 across an edge,
every term taken from the line's values before the edge is filtered:

    unchanged unless |p0 - q0| < a and |p1 - p0| < b and |q1 - q0| < b
    p side, if |p0 - q0| < s and |p2 - p0| < b:
        p0' = (p2 + 2 p1 + 2 p0 + 2 q0 + q1 + 4) >> 3
        p1' = (p2 + p1 + p0 + q0 + 2) >> 2
        p2' = (2 p3 + 3 p2 + p1 + p0 + q0 + 4) >> 3
    p side, otherwise:
        p0' = (2 p1 + p0 + q1 + 2) >> 2                 (p1 and p2 stay)
    the q side is the mirror image; p3 and q3 never change

All vertical edges of the plane are filtered first, on every row; then all horizontal edges on that result, on every column.  Interlaced
input under ``--deinterlace`` (either mode): each field of each plane is a plane of its own -- rows of one parity, pitch two rows, horizontal
edges every 8 field rows with phase Tp / 2 --, nothing is averaged across two time instants, and both fields of a payload are filtered
whichever the slot keeps.

What follows from the rule: A = 0 is the identity; a constant plane stays constant; every output sample lies between the least and the
greatest of the eight samples of its line; the rule is mirror symmetric in both axes; only samples within 3 of an edge can change; every sum
stays below 2^20, so int32 suffices at 16 bits.  Edges are 8 apart, each reads +-4 and writes +-3: no edge reads what another edge of the
same pass writes, and both passes of the cell [x-4, x+4) x [y-4, y+4) around a grid crossing read and write only that cell and the
remainders of the plane in line with it, which is why the kernel may work in place.

``deblock_payload_np`` is the definition the kernel (csrc/deblock.hip, ``demfi_payload_deblock``) is held to, byte for byte; ``plane_table``
is what the two share.  Not offered: frame-DCT blocks of interlaced material, whose edges fall every 4 field rows; grids other than 8, and
material scaled after coding; strength from a quantiser, and per-plane thresholds; ``demfi_amd.clip``; numeric equality with ffmpeg's
``deblock`` / ``pp``.  Ringing is the business of ``--dering`` (``demfi_amd.dering``), which runs directly behind this stage.
"""
import re

import numpy as np

from . import y4m

DEFAULT_A, DEFAULT_B, GRID = 16, 4, 8
DEFAULTS = (DEFAULT_A, DEFAULT_B)
MAX_PLANES = 6                                   # 3 planes x 2 fields: the entries of a plane table at most
_PAIR = re.compile(r'([0-9]+)(?::([0-9]+))?')
_SUB = {'420': (2, 2), '422': (1, 2), '444': (1, 1), 'mono': (1, 1)}     # (vertical, horizontal) luma samples per chroma sample


def check_params(a=DEFAULT_A, b=None):
    """(A, B) checked: integers with 0 <= B <= A <= 255 (``b`` None: (A + 3) // 4)."""
    for name, v in (('A', a), ('B', b)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError('deblock: %s must be an integer, got %r' % (name, v))
    if not 0 <= a <= 255:
        raise ValueError('deblock: the threshold A = %d lies outside 0 .. 255 (8-bit steps)' % a)
    b = (a + 3) // 4 if b is None else b
    if not 0 <= b <= a:
        raise ValueError('deblock: the thresholds need 0 <= B <= A <= 255 (8-bit steps), got A = %d, B = %d' % (a, b))
    return int(a), int(b)


def parse_deblock(text):
    """``16`` / ``16:4`` -> (A, B) of ``--deblock`` (A alone: A : (A + 3) // 4); ValueError for anything else."""
    m = _PAIR.fullmatch(str(text).strip())
    if not m:
        raise ValueError('deblock %r: expected A or A:B, integers in 8-bit steps with 0 <= B <= A <= 255' % (text,))
    return check_params(int(m.group(1)), int(m.group(2)) if m.group(2) is not None else None)


def thresholds(depth, a=DEFAULT_A, b=None):
    """(a, b, s) at ``depth`` bits: A << (d - 8), B << (d - 8) and (a >> 2) + (2 << (d - 8))."""
    if depth not in y4m.DEPTHS:
        raise ValueError('deblock: depth %r' % (depth,))
    a, b = check_params(a, b)
    sh = depth - 8
    return a << sh, b << sh, ((a << sh) >> 2) + (2 << sh)


def edges(n, removed=0):
    """The block edges of a line of ``n`` samples in front of which ``removed`` samples were cut away: every x with (x + removed) % 8 == 0
    and 4 <= x <= n - 4."""
    if n < 0 or removed < 0:
        raise ValueError('edges: n = %r, removed = %r' % (n, removed))
    return [x for x in range(4, n - 3) if (x + removed) % GRID == 0]


def _filter(v, a, b, s):
    """Lines [..., 8] (int64) -> the filtered lines; the rule, vectorised over the leading axes."""
    p3, p2, p1, p0, q0, q1, q2, q3 = (v[..., i] for i in range(8))
    on = (np.abs(p0 - q0) < a) & (np.abs(p1 - p0) < b) & (np.abs(q1 - q0) < b)
    small = np.abs(p0 - q0) < s
    out = v.copy()
    for (r3, r2, r1, r0, o0, o1), (i2, i1, i0) in (((p3, p2, p1, p0, q0, q1), (1, 2, 3)), ((q3, q2, q1, q0, p0, p1), (6, 5, 4))):
        strong = on & small & (np.abs(r2 - r0) < b)
        weak = on & ~strong
        out[..., i0] = np.where(strong, (r2 + 2 * r1 + 2 * r0 + 2 * o0 + o1 + 4) >> 3, np.where(weak, (2 * r1 + r0 + o1 + 2) >> 2, r0))
        out[..., i1] = np.where(strong, (r2 + r1 + r0 + o0 + 2) >> 2, r1)
        out[..., i2] = np.where(strong, (2 * r3 + 3 * r2 + r1 + r0 + o0 + 4) >> 3, r2)
    return out


def line_cases(v, a, b, s):
    """Which branch each line of ``v`` [..., 8] takes: 0 unfiltered, else 1 + (p side strong) + 2 * (q side strong), so 1 is weak / weak and 4
    strong / strong."""
    v = np.asarray(v).astype(np.int64)
    p2, p1, p0, q0, q1, q2 = (v[..., i] for i in range(1, 7))
    on = (np.abs(p0 - q0) < a) & (np.abs(p1 - p0) < b) & (np.abs(q1 - q0) < b)
    small = np.abs(p0 - q0) < s
    return np.where(on, 1 + (small & (np.abs(p2 - p0) < b)) + 2 * (small & (np.abs(q2 - q0) < b)), 0)


def deblock_line_np(line, a, b, s):
    """One line p3 p2 p1 p0 q0 q1 q2 q3 across an edge -> the filtered line (a list of ints); ``a``, ``b``, ``s`` at the line's depth."""
    v = np.asarray(line).astype(np.int64)
    if v.shape != (8,):
        raise ValueError('deblock_line_np: eight samples, got %s' % (v.shape,))
    return _filter(v, a, b, s).tolist()


def _pass(p, xs, a, b, s):
    """The lines across the edges ``xs`` of every row of ``p`` [rows, cols] (int64) filtered in place."""
    if len(xs) and p.shape[0]:
        idx = np.asarray(xs)[:, None] + np.arange(-4, 4)[None, :]
        p[:, idx] = _filter(p[:, idx], a, b, s)


def deblock_plane_np(plane, a, b, s, left=0, top=0, order='vh'):
    """The plane [rows, cols] deblocked: all vertical edges on every row, then all horizontal edges on that result on every column (``order``
    'hv': the other way round, which the rule does NOT ask for; tests pin the difference).  ``left``, ``top``: the columns and rows removed
    in front of the plane; ``a``, ``b``, ``s`` at the plane's depth."""
    src = np.asarray(plane)
    if src.ndim != 2:
        raise ValueError('deblock_plane_np: a [rows, cols] plane, got %s' % (src.shape,))
    p = src.astype(np.int64)
    for axis in order:
        if axis == 'v':
            _pass(p, edges(p.shape[1], left), a, b, s)
        else:
            _pass(p.T, edges(p.shape[0], top), a, b, s)
    return p.astype(src.dtype)


def plane_table(h, w, layout, fields=None, rect=None):
    """What the kernel and the definition share: [(first sample, rows, cols, row pitch in samples, x phase, y phase)] of the planes of an
    h x w payload of ``layout`` that are filtered as planes in their own right, at most ``MAX_PLANES``.  ``fields`` (None: progressive; else
    the field order): each field of each plane is an entry, the rows of one parity at a pitch of two rows.  ``rect`` = (top, bottom, left,
    right): the crop rectangle that left this payload of its uncropped stream (None: nothing removed); the phases are its top and left in the
    plane's own samples mod 8, the top halved over fields."""
    top, _, left, _ = rect if rect is not None else (0, 0, 0, 0)
    sv, sh = _SUB[y4m.check_layout(layout)]
    ch, cw = y4m.chroma_shape(h, w, layout)
    planes = [(0, h, w, top, left)]
    if layout != 'mono':
        planes += [(h * w, ch, cw, top // sv, left // sh), (h * w + ch * cw, ch, cw, top // sv, left // sh)]
    out = []
    for first, rows, cols, tp, lp in planes:
        if fields is None:
            out.append((first, rows, cols, cols, lp % GRID, tp % GRID))
        else:
            out += [(first + q * cols, (rows - q + 1) // 2, cols, 2 * cols, lp % GRID, (tp // 2) % GRID) for q in (0, 1) if rows > q]
    return out


def deblock_payload_np(payload, h, w, depth, layout, a=DEFAULT_A, b=None, fields=None, rect=None):
    """The payload (a 1-D uint8 / uint16 array of the samples of an h x w frame of ``layout``) deblocked; ``a``, ``b`` at the 8-bit scale;
    ``fields``, ``rect``: as for ``plane_table``.  The definition."""
    src = np.asarray(payload)
    if src.ndim != 1 or src.size != y4m.payload_size(h, w, layout):
        raise ValueError('deblock_payload_np: a flat payload of %d samples for a %dx%d %s frame, got %s'
                         % (y4m.payload_size(h, w, layout), w, h, layout, src.shape))
    thr = thresholds(depth, a, b)
    out = src.copy()
    for first, rows, cols, pitch, xp, yp in plane_table(h, w, layout, fields, rect):
        view = np.lib.stride_tricks.as_strided(out[first:], (rows, cols), (pitch * out.itemsize, out.itemsize))
        view[...] = deblock_plane_np(view, *thr, left=xp, top=yp)
    return out


def deblock_stream_np(pays, h, w, depth, layout, a=DEFAULT_A, b=None, fields=None, rect=None):
    """Every payload of the stream ``pays`` deblocked; the stage keeps nothing from one payload to the next."""
    a, b = check_params(a, b)
    return [deblock_payload_np(p, h, w, depth, layout, a, b, fields, rect) for p in pays]
