"""Host side of ``--tile-high-depth`` (10- to 16-bit Y4M video as tiles): the command line, the constructor, the check that lets a deep
stream through to a tiled run, and the numpy definition the GPU path is tested against on 16-bit frames."""
import io

import numpy as np
import pytest

from demfi_amd import _lib as L
from demfi_amd import tiling as T
from demfi_amd import y4m
from demfi_amd.pipeline import TileGrid
from demfi_amd.video import VideoRunner, parser


def test_the_parser_takes_the_switch():
    a = parser().parse_args(['in.y4m', 'out.y4m', '--tile', 'auto', '--high-depth', '--tile-high-depth'])
    assert a.tile_high_depth is True and a.high_depth is True and a.tile == 'auto'
    a = parser().parse_args(['in.y4m', 'out.y4m', '--tile', '768x1344', '--high-depth'])
    assert a.tile_high_depth is False and a.tile == (768, 1344)                # off by default
    assert parser().parse_args(['-', '-', '--tile-high-depth']).tile_high_depth is True   # alone: accepted, changes nothing


def test_the_constructor_stores_the_switch():
    assert VideoRunner(None).tile_high_depth is False
    vr = VideoRunner(None, high_depth=True, tile='auto', tile_high_depth=1)
    assert vr.tile_high_depth is True and vr.runner_kw['tile'] == 'auto' and 'tile_high_depth' not in vr.runner_kw


def test_the_depth_check_follows_the_switch():
    hdr = y4m.parse_header(b'YUV4MPEG2 W3840 H2160 F24:1 Ip C420p10\n', y4m.DEPTHS)
    hdr8 = y4m.parse_header(b'YUV4MPEG2 W3840 H2160 F24:1 Ip C420jpeg\n', y4m.DEPTHS)
    with pytest.raises(ValueError) as e:
        VideoRunner(None, high_depth=True, tile='auto')._check_depth(hdr)
    assert 'tile' in str(e.value) and '10-bit' in str(e.value) and '--tile-high-depth' in str(e.value)
    for kw in ({'tile': 'auto', 'tile_high_depth': True}, {'tile': None}, {'tile': None, 'tile_high_depth': True}):
        vr = VideoRunner(None, high_depth=True, **kw)
        vr._check_depth(hdr)
        assert vr.last_depth == 10
    for thd in (False, True):                                                  # an 8-bit stream never was refused
        vr = VideoRunner(None, high_depth=True, tile='auto', tile_high_depth=thd)
        vr._check_depth(hdr8)
        assert vr.last_depth == 8
    # without --high-depth the reader refuses the stream before any of this, whatever the switch
    with pytest.raises(y4m.Y4MError):
        VideoRunner(None, tile='auto', tile_high_depth=True).run_stream(io.BytesIO(b'YUV4MPEG2 W64 H64 F24:1 Ip C420p10\n'), io.BytesIO())


@pytest.mark.parametrize('h,w,tile,margin', [(96, 160, (64, 96), 16), (97, 131, (64, 96), 0), (2160, 3840, 'auto', 32)])
def test_crop_and_stitch_round_trip_a_16_bit_frame(h, w, tile, margin):
    p = T.plan_tiles(h, w, tile, margin)
    assert p.n_tiles > 1
    f = np.random.default_rng(h + w).integers(0, 65536, (h, w, 3), dtype=np.uint16)
    tiles = T.crop_np(f, p)
    assert tiles.dtype == np.uint16 and tiles.shape == (p.n_tiles,) + p.tile + (3,)
    back = T.stitch_np(tiles, p)
    assert back.dtype == np.uint16 and np.array_equal(back, f)
    # the kept rectangles partition the frame: tiles that write only those fill it exactly once
    hits = np.zeros((h, w), np.int32)
    for t in p.tiles:
        hits[t.keep.y0:t.keep.y1, t.keep.x0:t.keep.x1] += 1
        assert t.src.y0 <= t.keep.y0 < t.keep.y1 <= t.src.y1 and t.src.x0 <= t.keep.x0 < t.keep.x1 <= t.src.x1
    assert (hits == 1).all()


def test_the_tile_grid_has_the_sizes_of_its_plan():
    p = T.plan_tiles(2160, 3840, 'auto', 32)
    g = TileGrid(p)
    assert (g.h, g.w, g.th, g.tw, g.nt, g.plan) == (2160, 3840, p.tile[0], p.tile[1], 9, p) and p.tile == (768, 1344)


def test_the_new_entry_points_are_bound():
    for name in ('demfi_u16_ingest_rect', 'demfi_frame_to_u16_rect', 'demfi_ingest_u16_rect'):
        assert name in L.EXPORTS
    assert L.ABI_VERSION == 8                                                  # the ABI is additive
