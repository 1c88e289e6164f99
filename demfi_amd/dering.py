"""Deringing of the Y4M video path in front of the network (``python -m demfi_amd.video --dering [P[:S[:D]]]``): 8x8-DCT coded input (DV,
576i / 480i captures, NTSC DVDs behind ``--ivtc``, broadcast captures) rings beside strong edges, a deblurring network sharpens the ripples
like any other fine detail, and because they change with the coder's quantiser from frame to frame the flow sees motion that is not there.
``--denoise`` is purely temporal and stops at ringing beside a moving edge; ``--deblock`` touches only samples within 3 of a grid line.
Pure Python / numpy; the one module that knows the rule.

The rule is AV1's constrained directional enhancement filter (CDEF) in exact integers, on every plane as a plane in its own right.  P
(primary strength, 0 .. 15), S (secondary strength, 0 .. 4) and D (damping, 3 .. 6) are 8-bit steps and one triple serves every plane;
the default 4:2:5 is the middle of AV1's range and has NOT been tuned against this network; P alone means P : min((P + 1) // 2, 4) : 5;
P = S = 0 is the identity.  A plane of ``cols`` samples a row whose left Lp columns were removed by ``--crop`` (0 otherwise) has a block
starting at column x when (x + Lp) % 8 == 0, rows likewise with Tp: the coder's grid.  Blocks partition the plane; the first and the last
block of an axis may be partial.  At the working depth d, sh = d - 8:

direction of a block: its 64 positions (i, j), i the row, read at the position clamped into the plane, x = min(v >> sh, 255) - 128;
    direction k groups them into lines by i + j, i + j//2, i, 3 + i - j//2, 7 + i - j, 3 - i//2 + j, j, i//2 + j (k = 0 .. 7);
    cost[k] = sum over lines of (840 // n_line) * (sum of x on the line)^2; dir = the first k of the greatest cost;
    var = (cost[dir] - cost[(dir + 4) & 7]) >> 10.  Every cost is at most 64 * 840 * 128^2 < 2^31.
strengths of a block: t = 0 if var == 0, else (P * (4 + i) + 8) >> 4 with i = min(ilog2(var >> 6), 12) (0 when var >> 6 == 0);
    pri = t << sh, sec = S << sh, damp = D + sh.
taps: ``TAPS[k]`` = the offsets (dy, dx) of direction k at distances 1 and 2, each taken with both signs.  Primary: the 4 samples along
    dir, weights 4 and 2, threshold pri.  Secondary: the 8 samples along (dir + 2) & 7 and (dir + 6) & 7, weights 2 and 1, threshold sec.
    A tap outside the plane contributes nothing and does not enter the clamp; block borders do not stop taps; all taps read the plane
    as it was before the stage.
a sample c and a tap v, diff = v - c: constrain(diff, thr, damp) = 0 if thr == 0, else
    sign(diff) * min(|diff|, max(0, thr - (|diff| >> max(0, damp - ilog2(thr)))));
    s = the weighted sum; out = clip(c + ((8 + s - (s < 0)) >> 4), lo, hi), lo / hi the least and greatest of c and the taps in the plane.

What follows: 0:0 is the identity; a constant plane stays constant; every output lies between the extremes of the 13 samples it read; a
difference of thr << shift or more contributes nothing, so edges stay; the direction and the strengths of a block do not depend on the depth
when a plane is shifted up (the outputs then lie within 7 of the shifted result: the floor in |diff| >> shift and the rounding of s / 16 do
not commute with the shift); |s| <= 12 * (15 + 4) << 8.  Under ``--deinterlace`` each field of each plane is a plane of its own (``deblock.plane_table``).

``dering_payload_np`` is the definition the kernel (csrc/dering.hip, ``demfi_payload_dering``) is held to, byte for byte.  Not offered:
equality with libaom / dav1d output (the strengths are per stream and not per superblock, every plane searches its own direction, there is
no skip map); strength from a quantiser; per-plane strengths; 4x4 chroma blocks; frame-DCT blocks of interlaced material;
``demfi_amd.clip``.
"""
import re

import numpy as np

from . import y4m
from .deblock import GRID, plane_table

DEFAULT_P, DEFAULT_S, DEFAULT_D = 4, 2, 5
DEFAULTS = (DEFAULT_P, DEFAULT_S, DEFAULT_D)
MAX_P, MAX_S, MIN_D, MAX_D = 15, 4, 3, 6
COST_BOUND = 64 * 840 * 128 ** 2                  # 880 803 840 < 2^31
_TRIPLE = re.compile(r'([0-9]+)(?::([0-9]+)(?::([0-9]+))?)?')
# (dy, dx) of direction k at distances 1 and 2
TAPS = (((-1, 1), (-2, 2)), ((0, 1), (-1, 2)), ((0, 1), (0, 2)), ((0, 1), (1, 2)),
        ((1, 1), (2, 2)), ((1, 0), (2, 1)), ((1, 0), (2, 0)), ((1, 0), (2, -1)))
_DY = np.array([[t[0] for t in k] for k in TAPS])
_DX = np.array([[t[1] for t in k] for k in TAPS])
PRI_W, SEC_W = (4, 2), (2, 1)


def line_index(k, i, j):
    """The line of direction ``k`` that position (row i, column j) of a block lies on."""
    return (i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j)[k]


def _line_maps():
    """[8 directions, 15 lines, 64 positions] 0 / 1, and the weights 840 // n_line [8, 15] (0 for a line without samples)."""
    m = np.zeros((8, 15, 64), np.int64)
    for k in range(8):
        for i in range(8):
            for j in range(8):
                m[k, line_index(k, i, j), 8 * i + j] = 1
    n = m.sum(2)
    return m, np.where(n > 0, 840 // np.maximum(n, 1), 0)


_LINES, _WEIGHTS = _line_maps()


def check_params(p=DEFAULT_P, s=None, d=None):
    """(P, S, D) checked: integers with 0 <= P <= 15, 0 <= S <= 4, 3 <= D <= 6 (``s`` None: min((P + 1) // 2, 4); ``d`` None: 5)."""
    for name, v in (('P', p), ('S', s), ('D', d)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError('dering: %s must be an integer, got %r' % (name, v))
    if not 0 <= p <= MAX_P:
        raise ValueError('dering: the primary strength P = %d lies outside 0 .. %d (8-bit steps)' % (p, MAX_P))
    s = min((p + 1) // 2, MAX_S) if s is None else s
    d = DEFAULT_D if d is None else d
    if not 0 <= s <= MAX_S:
        raise ValueError('dering: the secondary strength S = %d lies outside 0 .. %d (8-bit steps)' % (s, MAX_S))
    if not MIN_D <= d <= MAX_D:
        raise ValueError('dering: the damping D = %d lies outside %d .. %d' % (d, MIN_D, MAX_D))
    return int(p), int(s), int(d)


def parse_dering(text):
    """``4`` / ``4:2`` / ``4:2:5`` -> (P, S, D) of ``--dering`` (P alone: P : min((P + 1) // 2, 4) : 5); ValueError for anything else."""
    m = _TRIPLE.fullmatch(str(text).strip())
    if not m:
        raise ValueError('dering %r: expected P, P:S or P:S:D, integers with 0 <= P <= %d, 0 <= S <= %d, %d <= D <= %d'
                         % (text, MAX_P, MAX_S, MIN_D, MAX_D))
    return check_params(*(int(g) if g is not None else None for g in m.groups()))


def ilog2(n):
    """floor(log2 n) of the positive integers ``n`` (0 for n <= 1), elementwise."""
    n = np.asarray(n, np.int64)
    out = np.zeros(n.shape, np.int64)
    for b in range(1, 40):
        out += (n >> b) > 0
    return out


def strengths(depth, p=DEFAULT_P, s=None, d=None):
    """(P, sec, damp, sh) at ``depth`` bits: the primary strength stays at the 8-bit scale until a block's variance has adjusted it;
    sec = S << sh, damp = D + sh, sh = depth - 8."""
    if depth not in y4m.DEPTHS:
        raise ValueError('dering: depth %r' % (depth,))
    p, s, d = check_params(p, s, d)
    sh = depth - 8
    return p, s << sh, d + sh, sh


def block_costs_np(blocks, depth):
    """Blocks [..., 8, 8] of samples at ``depth`` -> their costs [..., 8] (int64)."""
    v = np.asarray(blocks).astype(np.int64)
    x = np.minimum(v >> (depth - 8), 255) - 128
    sums = np.einsum('klp,...p->...kl', _LINES, x.reshape(x.shape[:-2] + (64,)))
    return (_WEIGHTS * sums * sums).sum(-1)


def block_direction_np(block8x8, depth):
    """One 8x8 block -> (dir, var, costs): the first direction of the greatest cost, (cost[dir] - cost[(dir + 4) & 7]) >> 10, the 8 costs."""
    b = np.asarray(block8x8)
    if b.shape != (8, 8):
        raise ValueError('block_direction_np: an 8x8 block, got %s' % (b.shape,))
    costs = block_costs_np(b, depth)
    k = int(np.argmax(costs))
    return k, int((costs[k] - costs[(k + 4) & 7]) >> 10), costs.tolist()


def adjust_np(p, var):
    """The primary strength of a block of variance ``var`` at the 8-bit scale: 0 if var == 0, else (P * (4 + i) + 8) >> 4 with
    i = min(ilog2(var >> 6), 12), 0 when var >> 6 == 0.  Elementwise over ``var``."""
    var = np.asarray(var, np.int64)
    i = np.where(var >> 6 > 0, np.minimum(ilog2(var >> 6), 12), 0)
    return np.where(var == 0, 0, (p * (4 + i) + 8) >> 4)


def constrain_np(diff, thr, damp):
    """0 where thr == 0, else sign(diff) * min(|diff|, max(0, thr - (|diff| >> max(0, damp - ilog2(thr))))).  Elementwise."""
    diff, thr = np.asarray(diff, np.int64), np.asarray(thr, np.int64)
    shift = np.maximum(0, damp - ilog2(thr))
    mag = np.minimum(np.abs(diff), np.maximum(0, thr - (np.abs(diff) >> shift)))
    return np.where(thr == 0, 0, np.sign(diff) * mag)


def round_np(s):
    """The weighted sum ``s`` / 16 rounded to nearest, ties away from zero: (8 + s - (s < 0)) >> 4.  Elementwise."""
    s = np.asarray(s, np.int64)
    return (8 + s - (s < 0)) >> 4


def _blocks(p, depth, left, top):
    """The plane ``p`` [rows, cols] (int64) -> (dir, var) of its blocks [nby, nbx] and the block index (by [rows], bx [cols]) of every
    row and column.  Positions of a partial block outside the plane read the plane at the clamped position."""
    rows, cols = p.shape
    nby, nbx = (rows + top + GRID - 1) // GRID, (cols + left + GRID - 1) // GRID
    ys, xs = np.clip(np.arange(nby * GRID) - top, 0, rows - 1), np.clip(np.arange(nbx * GRID) - left, 0, cols - 1)
    grid = p[ys][:, xs].reshape(nby, GRID, nbx, GRID).transpose(0, 2, 1, 3)
    costs = block_costs_np(grid, depth)
    k = np.argmax(costs, -1)
    best = np.take_along_axis(costs, k[..., None], -1)[..., 0]
    opp = np.take_along_axis(costs, ((k + 4) & 7)[..., None], -1)[..., 0]
    return k, (best - opp) >> 10, (np.arange(rows) + top) // GRID, (np.arange(cols) + left) // GRID


def _filter(p, depth, P, S, D, left, top):
    """The plane ``p`` [rows, cols] (int64) deringed, and what ``plane_cases`` tells."""
    rows, cols = p.shape
    _, sec, damp, sh = strengths(depth, P, S, D)
    bdir, var, by, bx = _blocks(p, depth, left, top)
    t = adjust_np(P, var)
    k = bdir[by][:, bx]
    pri = (t << sh)[by][:, bx]
    yy, xx = np.mgrid[0:rows, 0:cols]
    s, lo, hi = np.zeros_like(p), p.copy(), p.copy()
    outside = np.zeros(p.shape, bool)
    for kk, thr, weights in ((k, pri, PRI_W), ((k + 2) & 7, sec, SEC_W), ((k + 6) & 7, sec, SEC_W)):
        for dist in (0, 1):
            for sign in (1, -1):
                ty, tx = yy + sign * _DY[kk, dist], xx + sign * _DX[kk, dist]
                ok = (ty >= 0) & (ty < rows) & (tx >= 0) & (tx < cols)
                v = np.where(ok, p[np.clip(ty, 0, rows - 1), np.clip(tx, 0, cols - 1)], p)
                s += weights[dist] * constrain_np(v - p, thr, damp)
                lo, hi = np.minimum(lo, v), np.maximum(hi, v)
                outside |= ~ok
    raw = p + round_np(s)
    out = np.clip(raw, lo, hi)
    return out, dict(dir=bdir, flat=var == 0, t=t, clamped=raw != out, outside=outside)


def _plane(plane, name):
    src = np.asarray(plane)
    if src.ndim != 2 or not src.size:
        raise ValueError('%s: a [rows, cols] plane, got %s' % (name, src.shape,))
    return src


def dering_plane_np(plane, depth, p=DEFAULT_P, s=None, d=None, left=0, top=0):
    """The plane [rows, cols] of samples at ``depth`` deringed, out of place; ``p``, ``s``, ``d`` at the 8-bit scale; ``left``, ``top``:
    the columns and rows removed in front of the plane (their values mod 8 are the phases of the block grid)."""
    src = _plane(plane, 'dering_plane_np')
    p, s, d = check_params(p, s, d)
    if p == 0 and s == 0:
        return src.copy()
    return _filter(src.astype(np.int64), depth, p, s, d, left % GRID, top % GRID)[0].astype(src.dtype)


def plane_cases(plane, depth, p=DEFAULT_P, s=None, d=None, left=0, top=0):
    """What the rule does on the plane: per block ``dir`` [nby, nbx], ``flat`` (var == 0) and ``t`` (the adjusted primary strength at the
    8-bit scale); per sample ``clamped`` (the clamp to lo / hi acted) and ``outside`` (a tap fell outside the plane)."""
    src = _plane(plane, 'plane_cases')
    return _filter(src.astype(np.int64), depth, *check_params(p, s, d), left % GRID, top % GRID)[1]


def dering_payload_np(payload, h, w, depth, layout, p=DEFAULT_P, s=None, d=None, fields=None, rect=None):
    """The payload (a 1-D uint8 / uint16 array of the samples of an h x w frame of ``layout``) deringed; ``p``, ``s``, ``d`` at the 8-bit
    scale; ``fields``, ``rect``: as for ``deblock.plane_table``.  The definition."""
    src = np.asarray(payload)
    if src.ndim != 1 or src.size != y4m.payload_size(h, w, layout):
        raise ValueError('dering_payload_np: a flat payload of %d samples for a %dx%d %s frame, got %s'
                         % (y4m.payload_size(h, w, layout), w, h, layout, src.shape))
    p, s, d = check_params(p, s, d)
    out = src.copy()
    for first, rows, cols, pitch, xp, yp in plane_table(h, w, layout, fields, rect):
        view = np.lib.stride_tricks.as_strided(src[first:], (rows, cols), (pitch * src.itemsize, src.itemsize))
        dst = np.lib.stride_tricks.as_strided(out[first:], (rows, cols), (pitch * out.itemsize, out.itemsize))
        dst[...] = dering_plane_np(view, depth, p, s, d, left=xp, top=yp)
    return out


def dering_stream_np(pays, h, w, depth, layout, p=DEFAULT_P, s=None, d=None, fields=None, rect=None):
    """Every payload of the stream ``pays`` deringed; the stage keeps nothing from one payload to the next."""
    p, s, d = check_params(p, s, d)
    return [dering_payload_np(x, h, w, depth, layout, p, s, d, fields, rect) for x in pays]
