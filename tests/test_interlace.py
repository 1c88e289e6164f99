"""Interlaced output (``--interlace``) without a GPU: the definitions of ``demfi_amd.interlace`` against hand-computed columns and against
the deinterlacer's field convention, the pair bookkeeping of the stage, headers and counts, the refusals (each before a library is
loaded) and what ``pipeline.EdgeSpec`` does with the new attribute."""
import io
import itertools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from demfi_amd import deint as DI
from demfi_amd import interlace as IL
from demfi_amd import retime as R
from demfi_amd import y4m
from demfi_amd.pipeline import EdgeSpec

LAYOUTS = ('420', '422', '444', 'mono')


def _col(values, depth, lowpass, dtype=None):
    """The column ``values`` as a one-column plane woven with itself: every row filtered within its one source."""
    p = np.array(values, dtype or (np.uint16 if depth > 8 else np.uint8)).reshape(-1, 1)
    return IL.weave_plane_np(p, p, depth, 0, lowpass)[:, 0].tolist()


# ---- 1. the filters, by hand -------------------------------------------------------------------------------------------------------
def test_linear_columns_computed_by_hand():
    # (a + 2 c + b + 2) >> 2 with the rows above and below clamped to the plane
    assert _col([10, 20, 40, 80], 8, 'linear') == [(10 + 20 + 20 + 2) >> 2, (10 + 40 + 40 + 2) >> 2, (20 + 80 + 80 + 2) >> 2, (40 + 160 + 80 + 2) >> 2]
    assert _col([10, 20, 40, 80], 8, 'linear') == [13, 23, 45, 70]
    assert _col([7], 8, 'linear') == [7]                                 # one row: its own neighbours
    assert _col([0, 255], 8, 'linear') == [64, 191]                      # two rows: (0 + 0 + 255 + 2) >> 2, (0 + 510 + 255 + 2) >> 2
    assert _col([0, 255, 0], 8, 'linear') == [64, 128, 64]
    for depth in (8, 10, 16):
        peak = (1 << depth) - 1
        assert _col([peak] * 4, depth, 'linear') == [peak] * 4 and _col([0, peak], depth, 'linear') == [(peak + 2) >> 2, (3 * peak + 2) >> 2]


def test_complex_columns_computed_by_hand():
    # v = clip((4 + 6 c + 2 (a + b) - a2 - b2) >> 3, 0, peak); out = max(v, c) if a + b > 2 c else min(v, c)
    # row 0: (4 - 255) >> 3 = -32 (a floor shift) clips to 0; row 1: 514 >> 3 = 64, pulled up; row 2: 1534 >> 3 = 191, pulled down
    assert _col([0, 0, 255, 0, 0], 8, 'complex') == [0, 64, 191, 64, 0]
    # row 0: 264 >> 3 = 33; row 1: 1779 >> 3 = 222; row 2: 2524 >> 3 = 315 clips to the peak
    assert _col([0, 255, 250, 255, 0], 8, 'complex') == [33, 222, 255, 222, 33]
    # the guard, both branches: the far rows may not push the sample past itself, away from its neighbours' mean
    assert _col([255, 101, 100, 101, 255], 8, 'complex')[2] == 100       # a + b > 2 c and v = 498 >> 3 = 62 < c: max(v, c) = c
    assert _col([0, 99, 100, 99, 0], 8, 'complex')[2] == 100             # a + b < 2 c and v = 1000 >> 3 = 125 > c: min(v, c) = c
    assert _col([0, 101, 100, 101, 0], 8, 'complex')[2] == (4 + 600 + 404) >> 3 == 126      # towards the mean: the filter's value
    assert _col([255, 99, 100, 99, 255], 8, 'complex')[2] == (4 + 600 + 396 - 510) >> 3 == 61
    for depth in (8, 10, 16):                                            # the clip at 0 and at the peak
        peak = (1 << depth) - 1
        assert _col([0, peak, peak - 5, peak, 0], depth, 'complex')[2] == peak
        assert (4 + 6 * (peak - 5) + 4 * peak) >> 3 > peak
        assert _col([peak, 0, 5, 0, peak], depth, 'complex')[2] == 0
        assert (4 + 30 - 2 * peak) >> 3 < 0


def test_edge_rows_replicate_in_planes_of_one_to_four_rows():
    rng = np.random.default_rng(0)
    for rows in (1, 2, 3, 4):
        col = rng.integers(0, 256, rows).tolist()
        at = lambda y: col[min(max(y, 0), rows - 1)]                     # noqa: E731
        assert _col(col, 8, 'off') == col
        assert _col(col, 8, 'linear') == [(at(y - 1) + 2 * at(y) + at(y + 1) + 2) >> 2 for y in range(rows)]
        want = []
        for y in range(rows):
            c, a, b = at(y), at(y - 1), at(y + 1)
            v = min(max((4 + 6 * c + 2 * (a + b) - at(y - 2) - at(y + 2)) >> 3, 0), 255)
            want.append(max(v, c) if a + b > 2 * c else min(v, c))
        assert _col(col, 8, 'complex') == want


def test_a_row_is_filtered_within_the_frame_that_owns_it():
    rng = np.random.default_rng(1)
    f, s = rng.integers(0, 1024, (7, 5)).astype(np.uint16), rng.integers(0, 1024, (7, 5)).astype(np.uint16)
    for lowpass, q0 in itertools.product(IL.LOWPASS, (0, 1)):
        out = IL.weave_plane_np(f, s, 10, q0, lowpass)
        assert np.array_equal(out[q0::2], IL.weave_plane_np(f, f, 10, q0, lowpass)[q0::2])
        assert np.array_equal(out[1 - q0::2], IL.weave_plane_np(s, s, 10, q0, lowpass)[1 - q0::2])
        assert out.dtype == np.uint16 and out.max() <= 1023


# ---- 2. the field convention is the deinterlacer's ---------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['t', 'b'])
def test_weaving_the_bobs_of_a_plane_gives_the_plane_back(order):
    rng = np.random.default_rng(2)
    q0, q1 = DI.field_parity(order, 0), DI.field_parity(order, 1)
    for rows in range(1, 10):
        p = rng.integers(0, 256, (rows, 6)).astype(np.uint8)
        assert np.array_equal(IL.weave_plane_np(DI.bob_plane_np(p, q0), DI.bob_plane_np(p, q1), 8, q0, 'off'), p)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('order', ['tff', 'bff'])
def test_weaving_the_bobbed_payloads_gives_the_payload_back(order, layout):
    h, w = 10, 14
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, y4m.payload_size(h, w, layout)).astype(np.uint8)
    o = IL.parse_order(order)
    bobs = [np.concatenate([DI.bob_plane_np(pl, DI.field_parity(o, f)).reshape(-1) for pl in y4m.split_planes_layout(p, h, w, layout)
                            if pl is not None]) for f in (0, 1)]
    assert np.array_equal(IL.weave_payload_np(bobs[0], bobs[1], h, w, 8, layout, order, 'off'), p)
    planes = [pl for pl in y4m.split_planes_layout(IL.weave_payload_np(bobs[0], bobs[1], h, w, 8, layout, order, 'linear'), h, w, layout)
              if pl is not None]
    assert [pl.shape for pl in planes] == IL.plane_shapes(h, w, layout)  # chroma planes follow the rule on their own rows
    q0 = DI.field_parity(o, 0)
    for pl, a in zip(planes, y4m.split_planes_layout(bobs[0], h, w, layout)):
        assert np.array_equal(pl[q0::2], IL.weave_plane_np(a, a, 8, q0, 'linear')[q0::2])


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_constants_are_preserved_and_a_frame_woven_with_itself_comes_back(depth):
    peak, dt = (1 << depth) - 1, np.uint16 if depth > 8 else np.uint8
    rng = np.random.default_rng(depth)
    for layout, lowpass, order in itertools.product(LAYOUTS, IL.LOWPASS, ('t', 'b')):
        P = y4m.payload_size(9, 11, layout)
        for v in (0, 1, peak // 2, peak):
            c = np.full(P, v, dt)
            assert np.array_equal(IL.weave_payload_np(c, c, 9, 11, depth, layout, order, lowpass), c)
        x, z = rng.integers(0, peak + 1, P).astype(dt), rng.integers(0, peak + 1, P).astype(dt)
        out = IL.weave_payload_np(x, z, 9, 11, depth, layout, order, lowpass)
        assert out.dtype == dt and out.shape == (P,) and int(out.max()) <= peak
        if lowpass == 'off':
            assert np.array_equal(IL.weave_payload_np(x, x, 9, 11, depth, layout, order, 'off'), x)


def test_weave_stream_pairs_frames_and_weaves_an_odd_tail_with_itself():
    h, w = 6, 8
    rng = np.random.default_rng(4)
    pays = [rng.integers(0, 256, y4m.payload_size(h, w, '420')).astype(np.uint8) for _ in range(5)]
    out = IL.weave_stream_np([p.tobytes() for p in pays], h, w, 8, '420', 'tff', 'linear')
    assert len(out) == 3 and all(o.dtype == np.uint8 for o in out)
    for q, (a, b) in enumerate(((0, 1), (2, 3), (4, 4))):
        assert np.array_equal(out[q], IL.weave_payload_np(pays[a], pays[b], h, w, 8, '420', 't', 'linear'))
    assert IL.weave_stream_np([], h, w, 8, '420', 'tff') == []
    deep = [rng.integers(0, 1024, y4m.payload_size(h, w, '422')).astype('<u2') for _ in range(2)]
    out = IL.weave_stream_np([d.tobytes() for d in deep], h, w, 10, '422', 'b', 'complex')
    assert np.array_equal(out[0].view('<u2'), IL.weave_payload_np(deep[0], deep[1], h, w, 10, '422', 'bff', 'complex'))


# ---- 3. the pair bookkeeping -------------------------------------------------------------------------------------------------------
def _compositions(n):
    """Every way to cut n items into consecutive non-empty batches."""
    for cuts in itertools.product((False, True), repeat=max(n - 1, 0)):
        sizes, run = [], 1
        for c in cuts:
            if c:
                sizes.append(run)
                run = 1
            else:
                run += 1
        yield sizes + [run]


def _replay(counts, sizes):
    """The stage over ``counts`` (frames per window) in batches of ``sizes`` windows: (pairs as stream indices, payloads per window, frames
    carried).  A carried frame lies at row 0, a batch's frames from row 1 on."""
    pairs, woven, carried, still_open, index_open, w0, frame = [], [], 0, None, None, 0, 0
    for bi, size in enumerate(sizes):
        batch = counts[w0:w0 + size]
        if still_open is not None:
            carried, still_open = carried + 1, 0
        index = {0: index_open} if still_open is not None else {}
        index.update({1 + j: frame + j for j in range(sum(batch))})
        table, per_window, still_open = IL.close_pairs(still_open, batch, w0 + size == len(counts), 1)
        assert still_open is None or (still_open in index and still_open == sum(batch))      # at most one open frame: the batch's last
        pairs += [(index[a], index[b]) for a, b in table]
        woven += per_window
        index_open = index[still_open] if still_open is not None else None
        w0, frame = w0 + size, frame + sum(batch)
    assert still_open is None
    return pairs, woven, carried


def test_close_pairs_gives_the_one_batch_table_for_every_partition():
    seen_carry = False
    for n in range(0, 10):
        for counts in ([1] * n, [2] * ((n + 1) // 2) if n % 2 == 0 else None, [3, 0, 2, 1, 0, 3][:max(n - 3, 0)] if n > 3 else None):
            if counts is None or not counts:
                continue
            total = sum(counts)
            want = [(2 * q, min(2 * q + 1, total - 1)) for q in range(IL.n_payloads(total))]
            one = _replay(counts, [len(counts)])
            assert one[0] == want and one[2] == 0 and sum(one[1]) == IL.n_payloads(total)
            for sizes in _compositions(len(counts)):
                pairs, woven, carried = _replay(counts, sizes)
                assert pairs == want and woven == one[1], (counts, sizes)
                seen_carry = seen_carry or carried > 0
    assert seen_carry
    # N frames one per window, for every N up to 9 and every partition
    for n in range(1, 10):
        for sizes in _compositions(n):
            assert _replay([1] * n, sizes)[0] == [(2 * q, min(2 * q + 1, n - 1)) for q in range((n + 1) // 2)]


def test_close_pairs_counts_a_payload_to_the_window_that_completed_it():
    assert IL.close_pairs(None, [1, 1, 1], False) == ([(0, 1)], [0, 1, 0], 2)
    assert IL.close_pairs(None, [1, 1, 1], True) == ([(0, 1), (2, 2)], [0, 1, 1], None)
    assert IL.close_pairs(0, [0, 3], False, 1) == ([(0, 1), (2, 3)], [0, 2], None)
    assert IL.close_pairs(0, [0, 0], True, 1) == ([(0, 0)], [0, 1], None)
    assert IL.close_pairs(None, [], False) == ([], [], None) and IL.close_pairs(None, [0], True) == ([], [0], None)
    with pytest.raises(ValueError):
        IL.close_pairs(None, [-1], False)


# ---- 4. headers and counts ---------------------------------------------------------------------------------------------------------
def test_header_order_and_counts():
    hdr = y4m.parse_header(b'YUV4MPEG2 W96 H64 F60000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL\n', y4m.DEPTHS, y4m.LAYOUTS)
    out = R.output_header(hdr, hdr.fps)
    for order, tag in (('tff', b'It'), ('bff', b'Ib'), ('t', b'It'), ('b', b'Ib')):
        il = IL.interlaced_header(out, order)
        assert il.encode() == out.encode().replace(b' Ip ', b' ' + tag + b' ').replace(b'F60000:1001', b'F30000:1001')
        assert il.fps == Fraction(30000, 1001) and il.payload == out.payload
    assert [IL.n_payloads(n) for n in range(8)] == [0, 1, 1, 2, 2, 3, 3, 4]
    assert [IL.parse_order(t) for t in ('tff', 'bff', 't', 'b', ' TFF ')] == ['t', 'b', 't', 'b', 't']
    assert IL.check_lowpass(None) == 'linear' and [IL.check_lowpass(m) for m in IL.LOWPASS] == list(IL.LOWPASS)
    for bad in ('', 'p', 'top', None, 1, 'm'):
        with pytest.raises(ValueError, match='field order'):
            IL.parse_order(bad)
    for bad in ('', 'cubic', 1, True):
        with pytest.raises(ValueError, match='interlace_lowpass'):
            IL.check_lowpass(bad)
    with pytest.raises(ValueError):
        IL.n_payloads(-1)


@pytest.mark.parametrize('n_frames,n_in,full,rate', [(0, 0, True, {'mfi': 2}), (1, 1, True, {'fps': 24}), (2, 1, True, {'mfi': 2}),
                                                     (7, 6, False, {'mfi': 2})])
def test_file_size(n_frames, n_in, full, rate):
    """The runner sizes the output by ``n_payloads``: header + ceil(N / 2) frames, the length of the host-woven stream."""
    from demfi_amd import video
    vr, r = video.VideoRunner(None, full_length=full, interlace='bff', **rate), Fraction(rate.get('mfi', 1))
    hdr = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n')
    assert R.n_output_frames(n_in, r, full) == n_frames
    out_hdr = vr._out_header(hdr)
    assert out_hdr.interlace == 'b' and out_hdr.fps == 12 * r == vr.last_fps_out       # half of F_out = 24 r
    woven = IL.weave_stream_np([bytes(hdr.payload)] * n_frames, 64, 96, 8, '420', 'b')
    stream = out_hdr.encode() + b''.join(b'FRAME\n' + p.tobytes() for p in woven)
    assert vr._n_out(n_in, hdr) == IL.n_payloads(n_frames) == len(woven)
    assert y4m.frame_offset(len(out_hdr.encode()), vr._n_out(n_in, hdr), out_hdr.payload) == len(stream)
    assert video.VideoRunner(None, full_length=full, **rate)._n_out(n_in, hdr) == n_frames


# ---- 5. refusals, each before a library is loaded ----------------------------------------------------------------------------------
def _clip_file(tmp_path, h=96, w=96, n=5):
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W%d H%d F24:1 Ip C420jpeg\n' % (w, h) + (b'FRAME\n' + bytes(w * h * 3 // 2)) * n)
    return src


def test_video_runner_refuses_before_a_library_is_loaded(tmp_path):
    from demfi_amd import video
    for bad in ('p', 'top', 1, ''):
        with pytest.raises(ValueError, match='field order'):
            video.VideoRunner(None, interlace=bad)
    with pytest.raises(ValueError, match='interlace_lowpass must be one of'):
        video.VideoRunner(None, interlace='tff', interlace_lowpass='cubic')
    for given in ('off', 'linear'):                                      # the default's own value too: the argument was given
        with pytest.raises(ValueError, match='says how --interlace works'):
            video.VideoRunner(None, interlace_lowpass=given)
    vr = video.VideoRunner(None, mfi=2, interlace='tff')
    assert vr.interlace == ('t', 'linear') and vr.last_interlace is None and vr.last_interlace_carried == 0
    assert video.VideoRunner(None, mfi=2, interlace='b', interlace_lowpass='complex').interlace == ('b', 'complex')
    assert video.VideoRunner(None).interlace is None
    src = _clip_file(tmp_path)
    with pytest.raises(ValueError, match='interlace with 2 ranks'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'), world=2, rank=0)
    with pytest.raises(ValueError, match='interlace with 2 ranks'):
        video.check_interlace('tff', None, world=2)
    assert not (tmp_path / 'out.y4m').exists() and not vr._runners


@pytest.mark.parametrize('bars,why', [((1, 1, 0, 0), 'multiples of 4 rows'), ((2, 2, 0, 0), 'multiples of 4 rows')], ids=['odd top', 'top 2 mod 4'])
def test_a_crop_rectangle_must_keep_field_parity(bars, why, tmp_path):
    """With ``--interlace`` the rectangle lies on the interlaced grid: top and bottom even, units of 4 rows for 4:2:0."""
    from demfi_amd import letterbox as LB
    from demfi_amd import video
    src = _clip_file(tmp_path)
    vr = video.VideoRunner(None, mfi=2, interlace='tff', crop=bars)
    with pytest.raises(ValueError, match=why):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    with pytest.raises(ValueError, match=why):
        vr.run_stream(io.BytesIO(src.read_bytes()), io.BytesIO())
    assert not (tmp_path / 'out.y4m').exists() and not vr._runners
    if bars[0] % 2 == 0:                                                 # the same rectangle is fine for progressive output
        assert LB.check_rect(LB.bars_rect(bars, 96, 96), 96, 96, '420', 1, True)[0] == (2, 94, 0, 96)
    assert LB.check_rect((6, 90, 0, 96), 96, 96, '420', 2, False)[0] == (4, 92, 0, 96)
    assert LB.align_rect((6, 90, 0, 96), 96, 96, '420', 2) == (4, 92, 0, 96)          # auto grows to the grid
    assert LB.align_rect((6, 90, 0, 96), 96, 96, '444', 2) == (6, 90, 0, 96)          # rows in units of 2 without vertical subsampling


def test_the_switches_of_the_command_line():
    from demfi_amd import video
    a = video.parser().parse_args(['in.y4m', 'out.y4m', '--interlace', 'tff', '--interlace-lowpass', 'complex'])
    assert (a.interlace, a.interlace_lowpass) == ('t', 'complex') and video.check_interlace(a.interlace, a.interlace_lowpass) == ('t', 'complex')
    a = video.parser().parse_args(['in.y4m', 'out.y4m', '--interlace', 'bff'])
    assert (a.interlace, a.interlace_lowpass) == ('b', None) and video.check_interlace(a.interlace, None) == ('b', 'linear')
    a = video.parser().parse_args(['in.y4m', 'out.y4m'])
    assert a.interlace is None and a.interlace_lowpass is None and video.check_interlace(None, None) is None
    for argv in (['--interlace', 'progressive'], ['--interlace', 'tff', '--interlace-lowpass', 'cubic']):
        with pytest.raises(SystemExit):
            video.parser().parse_args(['in.y4m', 'out.y4m'] + argv)
    with pytest.raises(SystemExit):                  # main refuses before anything is loaded
        video.main(['in.y4m', 'out.y4m', '--interlace-lowpass', 'off'])


# ---- 6. the edge's record ----------------------------------------------------------------------------------------------------------
def _yuv(**kw):
    return SimpleNamespace(matrix=0, full_range=False, siting=0, with_s1=lambda k: False, **kw)


def test_edge_spec_defaults_are_unchanged_and_interlace_keys_the_pipeline():
    assert EdgeSpec() == (False, False, False, 8, '420', None, None, 'bob') and EdgeSpec().interlace is None
    assert EdgeSpec.of(_yuv()).interlace is None and EdgeSpec.of(_yuv()) == EdgeSpec(y4m=True) and EdgeSpec.of(None).interlace is None
    assert hash(EdgeSpec(y4m=True)) == hash((tuple(EdgeSpec(y4m=True)), None)) and 'interlace' not in repr(EdgeSpec(y4m=True))
    a = EdgeSpec.of(_yuv(interlace=('t', 'linear')))
    assert a.interlace == ('t', 'linear') and a == EdgeSpec(y4m=True, interlace=['t', 'linear'])
    assert hash(a) == hash(EdgeSpec(y4m=True, interlace=('t', 'linear')))
    assert a != EdgeSpec(y4m=True) and EdgeSpec(y4m=True) != a and a != tuple(a)
    assert a != EdgeSpec(y4m=True, interlace=('b', 'linear')) and a != EdgeSpec(y4m=True, interlace=('t', 'off'))
    assert len({(4, a), (4, EdgeSpec(y4m=True)), (4, EdgeSpec.of(_yuv(interlace=('t', 'linear'))))}) == 2
    assert a._replace(cuts=True).interlace == ('t', 'linear') and a._replace(interlace=None) == EdgeSpec(y4m=True)
    assert EdgeSpec(y4m=True)._replace(interlace=('b', 'off')).interlace == ('b', 'off') and "interlace=('t', 'linear')" in repr(a)
    both = EdgeSpec.of(_yuv(shutter=(2, 4), interlace=('b', 'complex')))
    assert (both.shutter, both.interlace) == ((2, 4), ('b', 'complex')) and both._replace(full=True).shutter == (2, 4)
    assert both != a and both != EdgeSpec(y4m=True, shutter=(2, 4)) and both._replace(shutter=None, interlace=('t', 'linear')) == a


def test_check_refuses_interlace_off_the_y4m_edge_and_accepts_it_with_everything_else():
    spec = EdgeSpec(y4m=True, interlace=('t', 'linear'))
    assert spec.check(True, False, True) is None and spec.check(True, False, False) is None
    assert spec._replace(cuts=True, full=True, depth=10, layout='mono', fields='t', deint_mode='adaptive', shutter=(2, 4)).check(True, True, True) is None
    assert spec._replace(dedup=(768, 320, Fraction(33, 100), 3)).check(True, True, True) is None
    with pytest.raises(ValueError, match='interlaced output needs the Y4M edge on a retimed runner'):
        spec.check(False, False, True)
    with pytest.raises(ValueError, match='needs the Y4M edge'):
        EdgeSpec(interlace=('t', 'linear')).check(True, False, True)
    for bad in (('p', 'linear'), ('t', 'cubic'), ('t',)):
        with pytest.raises(ValueError, match='interlace must be None or'):
            EdgeSpec(y4m=True, interlace=bad).check(True, False, True)


def test_the_yuv_edge_carries_the_switch_into_the_spec():
    from demfi_amd import video
    edge = video.YuvEdge('bt601', False, '420jpeg', lambda k: False, interlace='bff', interlace_lowpass='off')
    assert edge.interlace == ('b', 'off') and EdgeSpec.of(edge).interlace == ('b', 'off')
    assert EdgeSpec.of(video.YuvEdge('bt601', False, '420jpeg', lambda k: False)) == EdgeSpec(y4m=True)
    vr = video.VideoRunner(None, mfi=2, interlace='tff', interlace_lowpass='complex')
    hdr = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n')
    assert EdgeSpec.of(vr._edge(hdr, lambda k: False)).interlace == ('t', 'complex')
