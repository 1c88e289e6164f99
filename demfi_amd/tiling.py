"""Tile plans for frames larger than one forward can hold: the counterpart of the reference's ``--test_patch`` / ``--patch_boundary``
(/root/reference/utils.py:1339-1477, ``get_HW_boundary`` 1757-1774, ``trim_patch_boundary`` 1777-1798; broken upstream for any grid but
(1,1)).  The frame is cut into a grid of overlapping tiles, the network runs per tile, and from every tile only its
kept rectangle is pasted into the output; the kept rectangles partition the frame, so nothing is blended.

Unlike the reference, all tiles of a plan have ONE size (one engine, one workspace, one set of captured graphs serves them all):
where the reference gives an edge patch a one-sided margin and so a smaller size, the edge tiles here are shifted inwards and start
at the frame's border.  The frame is not pre-padded to a multiple of the margin either.

Pure Python + numpy: no GPU, no torch.  ``crop_np`` / ``stitch_np`` are the definition csrc/tile.hip is tested against."""
from collections import namedtuple

import numpy as np

# 'auto' never picks a tile above the largest frame the GPU tests run untiled (configuration 5: 1088 x 1920)
MAX_TILE_H = 1088
MAX_TILE_W = 1920
DEFAULT_MARGIN = 32                    # the reference's patch_boundary (main.py:117)
ALIGN = 32                             # a split axis has tiles of a multiple of 32: they never need the reflect padding

Rect = namedtuple('Rect', 'y0 x0 y1 x1')                 # rows y0 .. y1-1, columns x0 .. x1-1, frame coordinates
Tile = namedtuple('Tile', 'src keep')                    # source rectangle (what the network sees), kept rectangle (what is pasted)


class Plan(namedtuple('Plan', 'h w tile margin grid tiles')):
    """h, w: the frame; tile: (th, tw) of every tile; grid: (tiles per column, tiles per row); tiles: Tile, row-major."""
    __slots__ = ()

    @property
    def n_tiles(self):
        return len(self.tiles)

    def rects(self):
        """[n_tiles, 6] ints as csrc/tile.hip takes them: source origin (y0, x0), then the kept rectangle (y0, x0, y1, x1)."""
        return [[t.src.y0, t.src.x0, t.keep.y0, t.keep.x0, t.keep.y1, t.keep.x1] for t in self.tiles]

    def label(self):
        """'768x1344', or None for the one-tile plan (untiled)."""
        return '%dx%d' % self.tile if self.n_tiles > 1 else None


def min_count(length, size, margin):
    """Fewest tiles of ``size`` that cover ``length`` > size when the two outer tiles keep size - margin and the others
    size - 2 margin: n size - 2 margin (n - 1) >= length."""
    return max(2, -(-(length - 2 * margin) // (size - 2 * margin)))


def _axis(length, size, margin, what):
    """[(source start, kept start, kept end)] of one axis, and the tile length on it."""
    if length <= size:
        return [(0, 0, length)], length
    if size % ALIGN:
        raise ValueError('plan_tiles: tile %s %d is not a multiple of %d (the frame\'s %s %d is split)' % (what, size, ALIGN, what, length))
    if 2 * margin >= size:
        raise ValueError('plan_tiles: margin %d leaves nothing of a tile %s of %d (2 * margin >= tile side)' % (margin, what, size))
    n = min_count(length, size, margin)
    # evenly spread, the outer tiles at the borders; neighbours overlap by size - step >= 2 margin, and the cut is mid-overlap
    starts = [i * (length - size) // (n - 1) for i in range(n)]
    cuts = [0] + [(starts[i] + starts[i - 1] + size) // 2 for i in range(1, n)] + [length]
    return [(starts[i], cuts[i], cuts[i + 1]) for i in range(n)], size


def _auto_side(length, cap, margin, what):
    if length <= cap:
        return length
    top = cap // ALIGN * ALIGN
    if 2 * margin >= top:
        raise ValueError('plan_tiles: margin %d leaves nothing of the largest tile %s %d' % (margin, what, top))
    n = min_count(length, top, margin)
    side = -(-(length + 2 * margin * (n - 1)) // n)              # n side - 2 margin (n - 1) >= length
    side = max(-(-side // ALIGN) * ALIGN, (2 * margin // ALIGN + 1) * ALIGN)
    return min(side, top)


def plan_tiles(h, w, tile, margin=DEFAULT_MARGIN):
    """The plan of an h x w frame.  tile: (th, tw), or 'auto': per axis the fewest tiles with th <= MAX_TILE_H, tw <= MAX_TILE_W,
    then the smallest multiple of 32 that still does with that count.  An axis that fits in one tile has one tile of its own
    length.  Every kept rectangle keeps ``margin`` pixels from each side of its source rectangle that is inside the frame."""
    if int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError('plan_tiles: frame size %rx%r' % (h, w))
    if int(margin) != margin or margin < 0:
        raise ValueError('plan_tiles: margin must be an integer >= 0, got %r' % (margin,))
    h, w, margin = int(h), int(w), int(margin)
    if isinstance(tile, str):
        if tile != 'auto':
            raise ValueError("plan_tiles: tile must be (th, tw) or 'auto', got %r" % (tile,))
        tile = (_auto_side(h, MAX_TILE_H, margin, 'height'), _auto_side(w, MAX_TILE_W, margin, 'width'))
    try:
        th, tw = tile
        ok = int(th) == th and int(tw) == tw and th >= 1 and tw >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("plan_tiles: tile must be (th, tw) or 'auto', got %r" % (tile,))
    ys, th = _axis(h, int(th), margin, 'height')
    xs, tw = _axis(w, int(tw), margin, 'width')
    tiles = tuple(Tile(Rect(sy, sx, sy + th, sx + tw), Rect(ky0, kx0, ky1, kx1)) for sy, ky0, ky1 in ys for sx, kx0, kx1 in xs)
    return Plan(h, w, (th, tw), margin, (len(ys), len(xs)), tiles)


def parse_tile(text):
    """Command-line value of --tile: 'auto' or 'THxTW' (both multiples of 32: a tile is given to split a frame)."""
    if text == 'auto':
        return text
    try:
        th, tw = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise ValueError("--tile: expected 'auto' or THxTW, got %r" % (text,))
    if th <= 0 or tw <= 0 or th % ALIGN or tw % ALIGN:
        raise ValueError('--tile: tile sides must be positive multiples of %d, got %dx%d' % (ALIGN, th, tw))
    return th, tw


def parse_margin(text):
    try:
        m = int(text)
    except ValueError:
        raise ValueError('--tile-margin: expected an integer, got %r' % (text,))
    if m < 0:
        raise ValueError('--tile-margin: must be >= 0, got %d' % m)
    return m


def add_arguments(ap):
    """--tile / --tile-margin of the command lines (demfi_amd.video, demfi_amd.clip)."""
    import argparse

    def arg(fn):
        def conv(text):
            try:
                return fn(text)
            except ValueError as e:
                raise argparse.ArgumentTypeError(str(e))
        return conv
    ap.add_argument('--tile', type=arg(parse_tile), default=None, metavar='auto|THxTW',
                    help='run every frame as a grid of overlapping THxTW tiles (multiples of 32) and paste their kept parts; auto: the '
                         'fewest tiles of at most %dx%d.  For frames larger than one forward holds.  Off by default' % (MAX_TILE_H, MAX_TILE_W))
    ap.add_argument('--tile-margin', type=arg(parse_margin), default=DEFAULT_MARGIN, metavar='N',
                    help='pixels of a tile next to a cut that are computed and thrown away (the reference\'s patch_boundary); default %d'
                         % DEFAULT_MARGIN)


def crop_np(frame, plan):
    """frame [h,w,3] -> the tiles' source rectangles [n_tiles, th, tw, 3]."""
    frame = np.asarray(frame)
    if frame.shape[:2] != (plan.h, plan.w):
        raise ValueError('crop_np: frame %s for a %dx%d plan' % (frame.shape, plan.h, plan.w))
    return np.stack([frame[t.src.y0:t.src.y1, t.src.x0:t.src.x1] for t in plan.tiles])


def stitch_np(tiles, plan, h=None, w=None):
    """tiles [n_tiles, th, tw, 3] -> frame [h,w,3]: every tile's kept rectangle, pasted."""
    tiles = np.asarray(tiles)
    h, w = plan.h if h is None else h, plan.w if w is None else w
    if (h, w) != (plan.h, plan.w) or tiles.shape[:3] != (plan.n_tiles,) + plan.tile:
        raise ValueError('stitch_np: tiles %s, frame %dx%d for a %dx%d plan of %d %dx%d tiles' %
                         ((tiles.shape, h, w, plan.h, plan.w, plan.n_tiles) + plan.tile))
    out = np.empty((h, w) + tiles.shape[3:], tiles.dtype)
    for t, a in zip(plan.tiles, tiles):
        k, s = t.keep, t.src
        out[k.y0:k.y1, k.x0:k.x1] = a[k.y0 - s.y0:k.y1 - s.y0, k.x0 - s.x0:k.x1 - s.x0]
    return out
