"""``demfi_amd.bitdepth`` (``--work-depth`` / ``--out-depth`` / ``--dither``) on the CPU: the plane rule against exact rational arithmetic, the
Bayer index, the invariants that make the rule worth having, the field-row rule, ``resolve``'s table, the header rewrite, the accumulator
bounds, the reciprocal the kernel divides with, the stream helpers, and the parts of the plumbing that need no GPU (``EdgeSpec.depths``, the
switches of ``VideoRunner`` and of the command line)."""
import io
import itertools
from fractions import Fraction
from math import floor

import numpy as np
import pytest

from demfi_amd import bitdepth as BD
from demfi_amd import y4m
from demfi_amd.interlace import plane_shapes

PAIRS = [(a, b) for a in y4m.DEPTHS for b in y4m.DEPTHS if a != b]
ROW0 = [0, 32, 8, 40, 2, 34, 10, 42]
ROW1 = [48, 16, 56, 24, 50, 18, 58, 26]


def _values(d_in, seed):
    """Every v up to 10 bits; above, both ends, the values around neutral and a seeded sample."""
    peak = (1 << d_in) - 1
    if d_in <= 10:
        return np.arange(peak + 1)
    rng = np.random.default_rng(seed)
    mid = 1 << (d_in - 1)
    return np.unique(np.concatenate([[0, 1, 2, peak - 1, peak, mid - 1, mid, mid + 1], rng.integers(0, peak + 1, 300)]))


def _exact(v, d_in, d_out, full, chroma, T):
    """The rule in ``fractions.Fraction``: off_out + floor(((v - off_in) num + T) / den), clipped."""
    pi, po = (1 << d_in) - 1, (1 << d_out) - 1
    if full:
        num, den = po, pi
        oi, oo = ((1 << (d_in - 1)), (1 << (d_out - 1))) if chroma else (0, 0)
    else:
        num, den = (1 << (d_out - d_in), 1) if d_out > d_in else (1, 1 << (d_in - d_out))
        oi = oo = 0
    return min(max(oo + floor(Fraction((v - oi) * num + T, den)), 0), po)


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def test_bayer_index_is_the_quoted_matrix_and_a_permutation():
    ys, xs = np.mgrid[0:8, 0:8]
    b = BD.bayer_index(xs, ys)
    assert b[0].tolist() == ROW0 and b[1].tolist() == ROW1
    assert sorted(b.reshape(-1).tolist()) == list(range(64))
    big = BD.bayer_index(np.arange(40)[None, :] + 1000, np.arange(24)[:, None] + 72)        # period 8 both ways
    assert np.array_equal(big, np.tile(b, (3, 5)))
    for x, y in ((0, 0), (5, 1), (7, 7), (3, 6)):                        # the sum as the text writes it
        assert int(b[y, x]) == sum(((((x ^ y) >> i) & 1) << (5 - 2 * i)) | (((y >> i) & 1) << (4 - 2 * i)) for i in range(3))


@pytest.mark.parametrize('full', [False, True], ids=['limited', 'full'])
@pytest.mark.parametrize('d_in,d_out', PAIRS, ids=['%d-%d' % p for p in PAIRS])
def test_plane_rule_equals_fraction_floor_arithmetic(d_in, d_out, full):
    """Every pair of depths, luma and chroma, all v up to 10 bits (a seeded sample and both ends above); going down every one of the 64
    Bayer cells and ``none``, going up the one threshold.  The plane is laid out so that column x of row y has cell (x mod 8, y mod 8)."""
    vals = _values(d_in, d_in * 17 + d_out)
    for chroma in (False, True):
        _, _, num, den = BD.plane_rule(d_in, d_out, full, chroma)
        plane = np.tile(np.repeat(vals, 8), (8, 1))                      # [8, 8 n]: value j at columns 8 j .. 8 j + 7 of every row
        modes = [None] if d_out > d_in else ['none', 'bayer']
        exact = {}                                                       # threshold -> the exact results of all values (cells share thresholds)
        for mode in modes:
            got = BD.convert_plane_np(plane, d_in, d_out, full, chroma, mode)
            assert got.shape == plane.shape and got.min() >= 0 and got.max() <= (1 << d_out) - 1
            for y in range(8):
                for x in range(8):
                    T = den // 2 if mode != 'bayer' else ((2 * int(BD.bayer_index(x, y)) + 1) * den) >> 7
                    assert 0 <= T < den
                    if T not in exact:
                        exact[T] = np.array([_exact(int(v), d_in, d_out, full, chroma, T) for v in vals])
                    assert np.array_equal(got[y, x::8], exact[T]), (d_in, d_out, full, chroma, mode, x, y)


def test_limited_range_promotion_is_a_shift_and_the_round_trip_is_the_identity():
    rng = np.random.default_rng(1)
    for d_in, d_out in PAIRS:
        if d_out < d_in:
            continue
        v = rng.integers(0, 1 << d_in, (16, 24))
        up = BD.convert_plane_np(v, d_in, d_out)
        assert np.array_equal(up, v << (d_out - d_in))
        for mode in ('none', 'bayer'):
            for fr in (False, True):
                assert np.array_equal(BD.convert_plane_np(up, d_out, d_in, False, False, mode, fr), v)
    assert BD.convert_plane_np(np.array([[16, 128, 235, 240]]), 8, 10).tolist() == [[64, 512, 940, 960]]


def test_black_and_neutral_map_to_black_and_neutral_under_every_threshold():
    for (d_in, d_out), full in itertools.product(PAIRS, (False, True)):
        yb_in, cb_in = (0 if full else 16 << (d_in - 8)), 1 << (d_in - 1)
        yb_out, cb_out = (0 if full else 16 << (d_out - 8)), 1 << (d_out - 1)
        modes = (None,) if d_out > d_in else ('none', 'bayer')
        for mode in modes:
            for fr in (False, True):
                assert (BD.convert_plane_np(np.full((16, 16), yb_in), d_in, d_out, full, False, mode, fr) == yb_out).all()
                assert (BD.convert_plane_np(np.full((16, 16), cb_in), d_in, d_out, full, True, mode, fr) == cb_out).all()
    for d_in, d_out in PAIRS:                                            # the ends of full range map to the ends
        pi, po = (1 << d_in) - 1, (1 << d_out) - 1
        assert BD.convert_plane_np(np.array([[0, pi]]), d_in, d_out, True, False, 'none').tolist() == [[0, po]]


def test_block_means_of_constant_planes():
    """10 -> 8, limited: T = ((2 B + 1) 4) >> 7 = B >> 4 takes each of 0, 1, 2, 3 sixteen times in an 8x8 block, so a constant plane
    4 a + b comes out as a + [b + T >= 4], whose block mean is exactly a + b / 4.
    16 -> 8: T = ((2 B + 1) 256) >> 7 = 4 B + 2.  A constant 256 a + b (a < 255) comes out as a + 1 where b + 4 B + 2 >= 256, that is for
    B >= (254 - b) / 4: floor((b + 2) / 4) of the 64 cells.  The block mean is a + floor((b + 2) / 4) / 64 against the ideal a + b / 256: the
    error (4 floor((b + 2) / 4) - b) / 256 lies in [-1 / 256, 2 / 256], so |error| <= 1 / 128 of an output step."""
    for a, b in itertools.product((0, 16, 100, 254), range(4)):
        out = BD.convert_plane_np(np.full((16, 24), 4 * a + b), 10, 8, False, False, 'bayer')
        for y0, x0 in ((0, 0), (8, 8), (8, 16)):
            assert Fraction(int(out[y0:y0 + 8, x0:x0 + 8].sum()), 64) == a + Fraction(b, 4)
    worst = Fraction(0)
    for a, b in itertools.product((0, 77, 254), range(256)):
        out = BD.convert_plane_np(np.full((8, 8), 256 * a + b), 16, 8, False, False, 'bayer')
        mean = Fraction(int(out.sum()), 64)
        assert mean == a + Fraction((b + 2) // 4, 64)
        worst = max(worst, abs(mean - (a + Fraction(b, 256))))
    assert worst == Fraction(1, 128)
    assert (BD.convert_plane_np(np.full((8, 8), 65535), 16, 8, False, False, 'bayer') == 255).all()     # the clip at the peak


def test_field_rows_give_both_fields_the_same_pattern():
    rng = np.random.default_rng(3)
    for d_in, d_out, full in ((10, 8, False), (16, 10, True), (12, 10, False)):
        field = rng.integers(0, 1 << d_in, (9, 21))
        woven = np.repeat(field, 2, 0)                                   # both fields hold the same picture
        out = BD.convert_plane_np(woven, d_in, d_out, full, True, 'bayer', field_rows=True)
        assert np.array_equal(out[0::2], out[1::2])
        assert np.array_equal(out[0::2], BD.convert_plane_np(field, d_in, d_out, full, True, 'bayer'))
        plain = BD.convert_plane_np(woven, d_in, d_out, full, True, 'bayer')
        assert not np.array_equal(plain[0::2], plain[1::2])              # without the rule a field sees four of the eight rows
        assert np.array_equal(BD.convert_plane_np(woven, d_in, d_out, full, True, 'none', True), BD.convert_plane_np(woven, d_in, d_out, full, True, 'none'))


# ---- resolve ------------------------------------------------------------------------------------------------------------------------
def test_resolve_defaults_and_refusals():
    R = BD.resolve
    assert R(8) == (8, 8, 8, None) and R(10) == (10, 10, 10, None) and BD.is_noop(R(8)) and BD.is_noop(None)
    assert R(8, 8, 8) == (8, 8, 8, None) and R(10, None, 10) == (10, 10, 10, None) and BD.is_noop(R(10, 10, 10))
    assert R(8, 12) == (8, 12, 8, 'bayer')                               # --work-depth alone: the output keeps the INPUT's depth
    assert R(8, None, 10) == (8, 10, 10, None)                           # --out-depth alone, up: work = max(in, D)
    assert R(10, None, 8) == (10, 10, 8, 'bayer') and R(16, None, 8, 'none') == (16, 16, 8, 'none')
    assert R(8, 10, 8) == (8, 10, 8, 'bayer') and R(8, 16, 10, 'none') == (8, 16, 10, 'none') and R(10, 16, 16) == (10, 16, 16, None)
    assert not BD.is_noop(R(8, 10, 8)) and not BD.is_noop((8, 10, 10, None))
    for args, what in (((10, 8), 'below the input'), ((16, 12, 12), 'below the input'), ((8, 10, 12), 'above --work-depth'),
                       ((10, None, 12, None), None), ((8, 9), 'must be one of'), ((8, None, 11), 'must be one of'), ((8, 7), 'must be one of'),
                       ((8, True), 'must be one of'), ((8, None, None, 'bayer'), 'says how'), ((8, 10, 10, 'bayer'), 'without a requantisation'),
                       ((10, 10, None, 'none'), 'without a requantisation'), ((8, 10, 8, 'blue'), 'dither must be one of')):
        if what is None:
            assert R(*args) == (10, 12, 12, None)                        # D above the input alone is a promotion, not a refusal
            continue
        with pytest.raises(ValueError, match=what):
            R(*args)
    with pytest.raises(ValueError):
        R(9)
    assert BD.check_switches(12, 8, 'none') == (12, 8, 'none') and BD.check_switches() == (None, None, None)
    assert BD.DITHERS == ('bayer', 'none') and BD.check_dither(None) == 'bayer'


# ---- headers and streams ----------------------------------------------------------------------------------------------------------------
def _tag(layout, d):
    if layout == '420':
        return '420jpeg' if d == 8 else '420p%d' % d
    return layout if d == 8 else ('mono%d' if layout == 'mono' else layout + 'p%d') % d


def test_header_rewrite_for_every_layout_and_depth():
    for layout, d_in, d_out in itertools.product(y4m.LAYOUTS, y4m.DEPTHS, y4m.DEPTHS):
        line = b'YUV4MPEG2 W10 H6 F30000:1001 It A8:9 C%s XYSCSS=x XCOLORRANGE=FULL\n' % _tag(layout, d_in).encode()
        hdr = y4m.parse_header(line, y4m.DEPTHS, y4m.LAYOUTS, fields=True)
        out = BD.depth_header(hdr, d_out)
        assert out.encode() == line.replace(b'C' + _tag(layout, d_in).encode(), b'C' + _tag(layout, d_out).encode())
        back = y4m.parse_header(out.encode(), y4m.DEPTHS, y4m.LAYOUTS, fields=True)
        assert (back.depth, back.layout, back.w, back.h, back.fps, back.interlace, back.aspect, back.full_range, back.xtags) == \
            (d_out, layout, 10, 6, Fraction(30000, 1001), 't', '8:9', True, ['YSCSS=x'])
        assert back.payload == y4m.payload_bytes(6, 10, d_out, layout)
    keep = y4m.parse_header(b'YUV4MPEG2 W10 H6 F25:1 Ip C420mpeg2\n')
    assert BD.depth_header(keep, 8).encode() == keep.encode()           # the same depth keeps the siting tag
    with pytest.raises(ValueError):
        BD.depth_header(keep, 9)


def _clip(layout, d, n=3, h=6, w=10, full=False, inter='p', seed=0):
    rng = np.random.default_rng(seed + d)
    P = y4m.payload_size(h, w, layout)
    pays = [rng.integers(0, 1 << d, P).astype('<u2' if d > 8 else np.uint8) for _ in range(n)]
    head = b'YUV4MPEG2 W%d H%d F24:1 I%s C%s%s\n' % (w, h, inter.encode(), _tag(layout, d).encode(), b' XCOLORRANGE=FULL' if full else b'')
    return head + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


def _payloads(data):
    rd = y4m.Reader(io.BytesIO(data), y4m.DEPTHS, y4m.LAYOUTS, fields=True)
    buf, out = np.empty(rd.header.payload, np.uint8), []
    while rd.read_into(buf):
        out.append(buf.view('<u2').copy() if rd.header.depth > 8 else buf.copy())
    return rd.header, out


@pytest.mark.parametrize('layout', y4m.LAYOUTS)
def test_stream_helpers_on_a_small_clip_of_every_layout(layout):
    h, w = 6, 10
    shapes = plane_shapes(h, w, layout)
    for full in (False, True):
        data, pays = _clip(layout, 8, full=full)
        up = BD.promote_stream_np(data, 12)
        hdr, got = _payloads(up)
        assert (hdr.depth, hdr.layout, hdr.full_range, len(got)) == (12, layout, full, 3) and hdr.ctag == _tag(layout, 12)
        for p, q in zip(pays, got):
            pos = 0
            for i, (r, c) in enumerate(shapes):                          # plane by plane, the first luma and the others chroma
                exp = BD.convert_plane_np(p[pos:pos + r * c].reshape(r, c), 8, 12, full, i > 0)
                assert np.array_equal(q[pos:pos + r * c].reshape(r, c), exp)
                pos += r * c
            assert np.array_equal(q, BD.promote_payload_np(p, h, w, layout, 8, 12, full))
        assert BD.promote_stream_np(data, 8) == data
        for mode in BD.DITHERS:
            down = BD.requant_stream_np(up, 8, mode)
            assert _payloads(down)[0].encode() == _payloads(data)[0].encode() and len(down) == len(data)
            if not full:
                assert down == data                                      # limited range: promote, then requantise, is the identity
        with pytest.raises(ValueError):
            BD.promote_stream_np(up, 8)
        with pytest.raises(ValueError):
            BD.requant_stream_np(data, 10)
    deep, pays = _clip(layout, 16, full=True, inter='t', seed=5)           # an interlaced stream: field rows by the header
    down = BD.requant_stream_np(deep, 10)
    hdr, got = _payloads(down)
    assert (hdr.depth, hdr.interlace) == (10, 't')
    for p, q in zip(pays, got):
        assert np.array_equal(q, BD.requant_payload_np(p.astype(np.uint16), h, w, layout, 16, 10, True, 'bayer', field_rows=True))
    assert BD.requant_stream_np(deep, 10, 'bayer', field_rows=False) != down
    assert BD.requant_stream_np(deep, 10, 'none', field_rows=False) == BD.requant_stream_np(deep, 10, 'none')
    with pytest.raises(ValueError):
        BD.promote_payload_np(pays[0].astype(np.uint16), h, w, layout, 16, 10)
    with pytest.raises(ValueError):
        BD.requant_payload_np(pays[0].astype(np.uint8), h, w, layout, 16, 10)       # the wrong sample type


# ---- widths and the division -----------------------------------------------------------------------------------------------------------
def test_accumulator_bounds_against_a_brute_force_maximum():
    for (d_in, d_out), full, chroma in itertools.product(PAIRS, (False, True), (False, True)):
        off_in, _, num, den = BD.plane_rule(d_in, d_out, full, chroma)
        for top in (None, 65535 if d_in > 8 else 255):
            v = np.arange((top if top is not None else (1 << d_in) - 1) + 1, dtype=np.int64)
            acc = (v - off_in) * num
            lo, hi = BD.accumulator_bounds(d_in, d_out, full, chroma, top)
            assert (lo, hi) == (int(acc.min()), int(acc.max()) + den - 1)
            if not full:
                assert 0 <= lo and hi < 1 << 24
            # what the kernel divides: magnitudes, below 2^32 for every stored sample and every threshold
            for T in (0, den // 2, den - 1):
                neg, n = BD.floor_div_magnitudes(v - off_in, num, T, den)
                assert int(n.min()) >= 0 and int(n.max()) < 1 << 32
                q = n // den
                assert np.array_equal(np.where(neg, -q, q), ((v - off_in) * num + T) // den)
    assert BD.accumulator_bounds(14, 16, True, False, 65535)[1] == 65535 * 65535 + 16382 < 1 << 32
    assert BD.accumulator_bounds(16, 14, True, True)[0] == -32768 * 16383     # signed: a chroma sample below neutral
    widest = max(BD.accumulator_bounds(a, b, True, c, 65535 if a > 8 else 255)[1] for (a, b), c in itertools.product(PAIRS, (False, True)))
    assert widest < 1 << 32 and widest + (1 << 31) >= 1 << 32            # a bias of off_in * num on top of it needs more than 32 bits


def test_the_reciprocal_equals_the_floor():
    """``div_np`` is the kernel's division.  For every full-range pair: every numerator the rule can form from in-range samples under all 64
    Bayer thresholds and den // 2 (all of them up to 10 bits, a stride and both ends above), and values around every multiple of den near
    both ends of the 32-bit range."""
    rng = np.random.default_rng(7)
    for d_in in y4m.DEPTHS:
        den = (1 << d_in) - 1
        m, s = BD.reciprocal(den)
        assert 0 < m < 1 << 32 and s == d_in - 1
        edge = np.concatenate([np.arange(0, 4 * den), (1 << 32) - 1 - np.arange(0, 4 * den), rng.integers(0, 1 << 32, 200000),
                               (rng.integers(1, (1 << 32) // den, 50000)[:, None] * den + np.array([-1, 0, 1])).reshape(-1)]).astype(np.uint64)
        edge = edge[edge < (1 << 32)]
        assert np.array_equal(BD.div_np(edge, den), edge // np.uint64(den))
        for d_out in y4m.DEPTHS:
            if d_out == d_in:
                continue
            Ts = sorted({den // 2} | ({int(((2 * b + 1) * den) >> 7) for b in range(64)} if d_out < d_in else set()))
            step = 1 if d_in <= 10 else 13
            v = np.unique(np.concatenate([np.arange(0, 1 << d_in, step), [(1 << d_in) - 1, 65535 if d_in > 8 else 255]])).astype(np.int64)
            for chroma in (False, True):
                off_in, _, num, _ = BD.plane_rule(d_in, d_out, True, chroma)
                for T in Ts:
                    _, n = BD.floor_div_magnitudes(v - off_in, num, T, den)
                    assert np.array_equal(BD.div_np(n, den), n.astype(np.uint64) // np.uint64(den))
    for den in (2, 3, 7, 255, 256, 65535, (1 << 32) - 1):
        n = np.concatenate([np.arange(0, 1000), (1 << 32) - 1 - np.arange(0, 1000)]).astype(np.uint64)
        assert np.array_equal(BD.div_np(n, den), n // np.uint64(den))
    with pytest.raises(ValueError):
        BD.reciprocal(1)


# ---- the plumbing that needs no GPU --------------------------------------------------------------------------------------------------------
def test_edge_spec_keeps_depths_beside_the_tuple():
    from demfi_amd.pipeline import EdgeSpec
    plain = EdgeSpec(True, False, False, 10, '420')
    assert plain.depths is None and EdgeSpec(True, False, False, 10, '420', depths=(10, 10, 10, None)) == plain
    assert hash(EdgeSpec(True, False, False, 10, '420', depths=(10, 10, 10, None))) == hash(plain) and tuple(plain) == (True, False, False, 10, '420', None, None, 'bob')
    up = EdgeSpec(True, False, False, 10, '420', depths=(8, 10, 10, None))
    assert up.depths == (8, 10, 10, None) and up != plain and plain != up and hash(up) != hash(plain) and up.hi and tuple(up) == tuple(plain)
    assert up._replace(cuts=True).depths == up.depths and up._replace(depths=None) == plain and 'depths=(8, 10, 10, None)' in repr(up)
    assert 'depths' not in repr(plain)
    down = EdgeSpec(True, depth=10, depths=(10, 10, 8, 'bayer'), scale=(64, 48, 'bicubic'))
    assert down != up and down.scale == (64, 48, 'bicubic') and down == down._replace()
    up.check(True, False, True), down.check(True, False, True)
    for bad in ((8, 10, 10, 'bayer'), (10, 10, 8, None), (12, 10, 10, None), (8, 10, 12, None), (8, 12, 12, None)):
        with pytest.raises(ValueError, match='depths must be'):
            EdgeSpec(True, depth=10, depths=bad).check(True, False, True)
    with pytest.raises(ValueError, match='Y4M edge'):
        EdgeSpec(False, depth=10, depths=(8, 10, 10, None)).check(True, False, True)

    class Yuv:
        depth, depths, layout = 10, (8, 10, 8, 'none'), '420'
    assert EdgeSpec.of(Yuv()).depths == (8, 10, 8, 'none') and EdgeSpec.of(Yuv()).depth == 10


def test_the_switches_of_the_runner_and_the_command_line():
    from demfi_amd import video as V
    assert V.check_depths() == (None, None, None) and V.check_depths(12, 8, 'none') == (12, 8, 'none')
    for kw, what in (({'work_depth': 9}, 'must be one of'), ({'out_depth': 18}, 'must be one of'), ({'work_depth': 10, 'out_depth': 12}, 'above --work-depth'),
                     ({'dither': 'none'}, 'says how'), ({'out_depth': 8, 'dither': 'noise'}, 'dither must be one of')):
        with pytest.raises(ValueError, match=what):
            V.VideoRunner(None, **kw)
    vr = V.VideoRunner(None, mfi=2, work_depth=12)
    h8 = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip C420jpeg\n')
    h10 = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip C422p10 XCOLORRANGE=FULL\n', y4m.DEPTHS, y4m.LAYOUTS)
    assert vr._depths_of(h8) == (8, 12, 8, 'bayer') and vr._out_header(h8).encode() == b'YUV4MPEG2 W96 H64 F48:1 Ip C420jpeg\n'
    assert V.VideoRunner(None, mfi=2, out_depth=10)._out_header(h8).encode() == b'YUV4MPEG2 W96 H64 F48:1 Ip C420p10\n'
    assert V.VideoRunner(None, mfi=2, out_depth=8)._out_header(h10).encode() == b'YUV4MPEG2 W96 H64 F48:1 Ip C422 XCOLORRANGE=FULL\n'
    assert V.VideoRunner(None, mfi=2)._out_header(h10).encode() == b'YUV4MPEG2 W96 H64 F48:1 Ip C422p10 XCOLORRANGE=FULL\n'
    with pytest.raises(ValueError, match='below the input'):
        V.VideoRunner(None, mfi=2, work_depth=8)._depths_of(h10)
    with pytest.raises(ValueError, match='without a requantisation'):
        V.VideoRunner(None, mfi=2, out_depth=10, dither='none')._depths_of(h8)
    tiled = V.VideoRunner(None, mfi=2, out_depth=10, tile=(64, 64))
    with pytest.raises(ValueError, match='--tile-high-depth'):
        tiled._check_depth(h8)
    ok = V.VideoRunner(None, mfi=2, out_depth=10, tile=(64, 64), tile_high_depth=True)
    ok._check_depth(h8)
    assert ok.last_depth == 10 and ok.last_depths == (8, 10, 10, None)
    plain = V.VideoRunner(None, mfi=2, tile=(64, 64))
    plain._check_depth(h8)
    assert plain.last_depth == 8 and plain.last_depths is None
    edge = V.VideoRunner(None, mfi=2, out_depth=8, dither='none')._edge(h10, lambda k: False)
    assert (edge.depth, edge.depths, edge.full_range) == (10, (10, 10, 8, 'none'), True)
    assert V.VideoRunner(None, mfi=2, out_depth=10)._edge(h10, lambda k: False).depths is None
    a = V.parser().parse_args(['-', '-', '--work-depth', '12', '--out-depth', '10', '--dither', 'none'])
    assert (a.work_depth, a.out_depth, a.dither) == (12, 10, 'none')
    a = V.parser().parse_args(['-', '-'])
    assert (a.work_depth, a.out_depth, a.dither) == (None, None, None)
    for argv in (['--work-depth', '9'], ['--dither', 'blue']):
        with pytest.raises(SystemExit):
            V.parser().parse_args(['-', '-'] + argv)
    for argv in (['--dither', 'none'], ['--work-depth', '8', '--out-depth', '10']):      # refused by main before a GPU is asked for
        with pytest.raises(SystemExit):
            V.main(['-', '-'] + argv)
