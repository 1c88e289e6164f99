"""CPU tests of the tile plans (demfi_amd/tiling.py): the invariants of ``plan_tiles`` over a sweep of sizes, the numpy crop /
stitch pair, and the --tile / --tile-margin command-line arguments.  No GPU, no kernel."""
import itertools

import numpy as np
import pytest

from demfi_amd import tiling as T

MARGINS = [0, 32, 64, 96]
# odd sizes, primes, L = T, L = T + 1 (T = 256 / 1088 / 1920), the UHD sizes
LENGTHS = [2, 31, 97, 131, 255, 256, 257, 509, 640, 1087, 1088, 1089, 1283, 1920, 1921, 2160, 3840, 4320, 7680, 16384]
TILES = [256, 320, 1088, 1920]


def _axis(plan, axis):
    """(source start, source end, kept start, kept end) of the tiles along one axis (the plan is a grid: taken from its first row /
    column), after checking that the plan IS that grid."""
    ny, nx = plan.grid
    assert len(plan.tiles) == ny * nx
    rows = [plan.tiles[i * nx] for i in range(ny)]
    cols = plan.tiles[:nx]
    for i, j in itertools.product(range(ny), range(nx)):
        t = plan.tiles[i * nx + j]
        assert (t.src.y0, t.src.y1, t.keep.y0, t.keep.y1) == (rows[i].src.y0, rows[i].src.y1, rows[i].keep.y0, rows[i].keep.y1)
        assert (t.src.x0, t.src.x1, t.keep.x0, t.keep.x1) == (cols[j].src.x0, cols[j].src.x1, cols[j].keep.x0, cols[j].keep.x1)
    if axis == 0:
        return [(t.src.y0, t.src.y1, t.keep.y0, t.keep.y1) for t in rows]
    return [(t.src.x0, t.src.x1, t.keep.x0, t.keep.x1) for t in cols]


def _feasible(n, length, size, margin):
    """Can n tiles of ``size`` (inside the frame) keep a partition of ``length`` with ``margin`` to every inner side?  The two
    outer tiles keep at most size - margin, the others size - 2 margin; one tile must be the whole axis."""
    if n == 1:
        return size >= length
    return 2 * (size - margin) + (n - 2) * (size - 2 * margin) >= length


def _check_axis(tiles, length, size, margin):
    assert tiles[0][2] == 0 and tiles[-1][3] == length                                   # 1: the kept intervals partition the axis
    for a, b in zip(tiles, tiles[1:]):
        assert a[3] == b[2]
    for s0, s1, k0, k1 in tiles:
        assert 0 <= s0 and s1 <= length and s1 - s0 == size                               # 2: inside the frame, the plan's size
        assert s0 <= k0 < k1 <= s1                                                        # 3: kept inside the source ...
        assert k0 - s0 >= (margin if s0 > 0 else 0) and s1 - k1 >= (margin if s1 < length else 0)    # ... margin off inner sides
    n = len(tiles)
    assert n == 1 or not _feasible(n - 1, length, size, margin)                           # 4: no fewer tiles would do


@pytest.mark.parametrize('margin', MARGINS)
def test_plan_invariants_over_the_sweep(margin):
    checked = 0
    for (h, w), (th, tw) in itertools.product(zip(LENGTHS, reversed(LENGTHS)), itertools.product(TILES, TILES)):
        if (h > th and 2 * margin >= th) or (w > tw and 2 * margin >= tw):
            continue
        p = T.plan_tiles(h, w, (th, tw), margin)
        eh, ew = min(h, th), min(w, tw)
        assert p.tile == (eh, ew) and (p.h, p.w, p.margin) == (h, w, margin)
        _check_axis(_axis(p, 0), h, eh, margin)
        _check_axis(_axis(p, 1), w, ew, margin)
        assert (p.grid[0] == 1) == (h <= th) and (p.grid[1] == 1) == (w <= tw)
        cover = np.zeros((h, w), np.uint8) if h * w <= 1 << 22 else None                  # 1 again, pixel by pixel where cheap
        if cover is not None:
            for t in p.tiles:
                cover[t.keep.y0:t.keep.y1, t.keep.x0:t.keep.x1] += 1
            assert (cover == 1).all()
        checked += 1
    assert checked >= 200


def _auto_rule(length, cap, margin):
    """The issue's rule, restated: the fewest tiles with a side <= cap, then the smallest multiple of 32 that still does."""
    if length <= cap:
        return 1, length
    n = next(n for n in range(2, 10000) if _feasible(n, length, cap // 32 * 32, margin))
    side = next(s for s in range(32, cap + 1, 32) if 2 * margin < s and _feasible(n, length, s, margin))
    return n, side


@pytest.mark.parametrize('margin', MARGINS)
@pytest.mark.parametrize('h,w', [(2160, 3840), (4320, 7680), (1088, 1920), (1089, 1921), (720, 1280), (1283, 4099), (16384, 16384)])
def test_auto_follows_the_rule(h, w, margin):
    p = T.plan_tiles(h, w, 'auto', margin)
    (ny, th), (nx, tw) = _auto_rule(h, T.MAX_TILE_H, margin), _auto_rule(w, T.MAX_TILE_W, margin)
    assert p.grid == (ny, nx) and p.tile == (th, tw)
    assert th <= T.MAX_TILE_H and tw <= T.MAX_TILE_W
    _check_axis(_axis(p, 0), h, th, margin)
    _check_axis(_axis(p, 1), w, tw, margin)


def test_auto_at_uhd_is_3x3_of_768x1344():
    assert (T.MAX_TILE_H, T.MAX_TILE_W, T.DEFAULT_MARGIN) == (1088, 1920, 32)
    p = T.plan_tiles(2160, 3840, 'auto')
    assert p.grid == (3, 3) and p.tile == (768, 1344) and p.n_tiles == 9 and p.label() == '768x1344'
    assert round(9 * 768 * 1344 / (2160 * 3840), 2) == 1.12
    assert T.plan_tiles(2160, 3840, (768, 1344)) == p


def test_a_frame_that_fits_is_the_one_tile_plan():
    for tile in ('auto', (64, 96), (1088, 1920), (100, 100)):
        p = T.plan_tiles(48, 80, tile)
        assert p.n_tiles == 1 and p.tile == (48, 80) and p.label() is None
        assert p.tiles[0] == T.Tile(T.Rect(0, 0, 48, 80), T.Rect(0, 0, 48, 80))
    p = T.plan_tiles(50, 160, (64, 96), 16)                   # one axis fits: any length there, the other is split
    assert p.grid == (1, 2) and p.tile == (50, 96)
    with pytest.raises(AttributeError):
        p.h = 1


@pytest.mark.parametrize('args', [(96, 160, (50, 96), 16), (96, 160, (64, 100), 16), (96, 160, (64, 96), 32), (96, 160, (64, 96), 48),
                                  (96, 160, (64, 96), -1), (96, 160, 'big', 16), (96, 160, (64,), 16), (96, 160, (0, 96), 16),
                                  (4000, 4000, 'auto', 544)])
def test_bad_plans_are_rejected(args):
    with pytest.raises(ValueError):
        T.plan_tiles(*args)


@pytest.mark.parametrize('h,w,tile,margin', [(96, 160, (64, 96), 16), (97, 131, (64, 96), 0), (61, 1283, (64, 320), 32), (131, 97, (96, 64), 8)])
def test_stitch_of_crop_is_the_frame(h, w, tile, margin):
    p = T.plan_tiles(h, w, tile, margin)
    f = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    tiles = T.crop_np(f, p)
    assert tiles.shape == (p.n_tiles,) + p.tile + (3,) and tiles.dtype == np.uint8
    for t, a in zip(p.tiles, tiles):
        assert (a == f[t.src.y0:t.src.y1, t.src.x0:t.src.x1]).all()
    assert (T.stitch_np(tiles, p, h, w) == f).all()
    labels = np.empty_like(tiles)
    for j in range(p.n_tiles):
        labels[j] = j
    exp = np.full((h, w, 3), 255, np.uint8)
    for j, t in enumerate(p.tiles):
        exp[t.keep.y0:t.keep.y1, t.keep.x0:t.keep.x1] = j
    assert (T.stitch_np(labels, p, h, w) == exp).all() and exp.max() == p.n_tiles - 1
    with pytest.raises(ValueError):
        T.stitch_np(tiles[1:], p, h, w)
    with pytest.raises(ValueError):
        T.crop_np(f[1:], p)


def test_rects_are_what_the_kernels_take():
    p = T.plan_tiles(96, 160, (64, 96), 16)
    r = p.rects()
    assert len(r) == 4 and r[0] == [0, 0, 0, 0, 48, 80] and r[3] == [32, 64, 48, 80, 96, 160]


def test_command_line_arguments():
    from demfi_amd import clip, video
    for ap, head in ((video.parser(), ['in.y4m', 'out.y4m']), (clip.parser(), ['frames'])):
        a = ap.parse_args(head)
        assert a.tile is None and a.tile_margin == 32
        assert ap.parse_args(head + ['--tile', 'auto']).tile == 'auto'
        a = ap.parse_args(head + ['--tile', '768x1344', '--tile-margin', '64'])
        assert a.tile == (768, 1344) and a.tile_margin == 64
        for bad in (['--tile', '100x100'], ['--tile', '768'], ['--tile', '0x32'], ['--tile-margin', '-1'], ['--tile-margin', 'x']):
            with pytest.raises(SystemExit):
                ap.parse_args(head + bad)
