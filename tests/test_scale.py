"""The definitions of resized output (``demfi_amd/scale.py``, ``--scale``) on the CPU: parsing and refusals, the tap tables, the integer
plane rule against hand-computed values and against a float64 resample with a tolerance derived from the tables, the accumulator
bounds the kernel's accumulator widths rest on, payload sizes, the header rule and the switches of ``demfi_amd.video``."""
import io
import itertools
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import scale as SC
from demfi_amd import video, y4m
from demfi_amd.interlace import plane_shapes
from demfi_amd.pipeline import EdgeSpec

RATIOS = [(4, 1), (3, 1), (2, 1), (6, 5), (1, 1), (5, 6), (1, 2), (1, 8)]          # n_in : n_out


# ---- parsing and refusals ------------------------------------------------------------------------------------------------------
def test_parse_size_is_width_first():
    assert SC.parse_size('1280x720') == (1280, 720) and SC.parse_size(' 720X480 ') == (720, 480)
    for bad in ('1280', '1280x', 'x720', '1280x720x3', '-1x720', '1280*720', '12.5x10', '', None, 1280):
        with pytest.raises(ValueError, match='--scale'):
            SC.parse_size(bad)
    for bad in ('1x720', '720x1', '0x0', '%dx16' % (y4m.MAX_SIDE + 1)):
        with pytest.raises(ValueError, match='--scale.*outside'):
            SC.parse_size(bad)
    assert SC.check_size((64, 48)) == (64, 48)
    for bad in ((64,), (64, 48, 3), (64.0, 48), (True, 48), 'ab', None):
        with pytest.raises(ValueError, match='--scale'):
            SC.check_size(bad)


def test_check_filter():
    assert SC.check_filter(None) == 'lanczos3' == SC.DEFAULT_FILTER
    assert [SC.check_filter(f) for f in SC.FILTERS] == ['lanczos3', 'bicubic', 'bilinear']
    with pytest.raises(ValueError, match='--scale-filter'):
        SC.check_filter('nearest')


def test_the_tap_limit_names_the_largest_shrink():
    assert SC.MAX_TAPS == 32
    for filt, most in (('lanczos3', Fraction(16, 3)), ('bicubic', Fraction(8)), ('bilinear', Fraction(16))):
        n_out = 30
        ok = int(most * n_out)
        assert SC.axis_table(ok, n_out, filt)[1].shape == (n_out, 32) and SC.n_taps(ok, n_out, filt) == 32
        with pytest.raises(ValueError, match=r'--scale.*more than 32.*%d:%d at most' % (16, SC.SUPPORT[filt])):
            SC.axis_table(ok + 1, n_out, filt)
    assert SC.n_taps(256, 64, 'lanczos3') == 24 and SC.n_taps(64, 512, 'lanczos3') == 6 and SC.n_taps(64, 64, 'bilinear') == 2
    with pytest.raises(ValueError):
        SC.axis_table(0, 4)
    with pytest.raises(ValueError):
        SC.axis_table(4, 0)


# ---- the header ----------------------------------------------------------------------------------------------------------------
def _hdr(w, h, aspect):
    return y4m.Header(w, h, Fraction(25), 'p', aspect, '420jpeg', 'FULL', ('YSCSS=420JPEG',), '420jpeg', 8, '420')


def test_the_pixel_aspect_keeps_the_display_aspect():
    out = SC.scaled_header(_hdr(720, 576, '16:15'), 720, 480)
    assert (out.w, out.h, out.aspect) == (720, 480, '8:9')
    assert out.encode() == b'YUV4MPEG2 W720 H480 F25:1 Ip A8:9 C420jpeg XYSCSS=420JPEG XCOLORRANGE=FULL\n'
    for w_in, h_in, (n, d), w, h in ((1920, 1080, (1, 1), 1280, 720), (1440, 1080, (4, 3), 1280, 720), (720, 480, (8, 9), 1920, 1080)):
        out = SC.scaled_header(_hdr(w_in, h_in, '%d:%d' % (n, d)), w, h)
        n2, d2 = (int(v) for v in out.aspect.split(':'))
        assert Fraction(w * n2, h * d2) == Fraction(w_in * n, h_in * d) and Fraction(n2, d2).numerator == n2


def test_a_missing_or_unknown_aspect_stays():
    assert SC.scaled_header(_hdr(720, 576, None), 720, 480).aspect is None
    assert b' A' not in SC.scaled_header(_hdr(720, 576, None), 720, 480).encode()
    assert SC.scaled_header(_hdr(720, 576, '0:0'), 720, 480).aspect == '0:0'
    assert SC.scaled_header(_hdr(720, 576, '16:15'), 720, 576).aspect == '16:15'          # the same size: nothing changes
    assert SC.scaled_header(_hdr(720, 576, '32:30'), 720, 576).encode() == _hdr(720, 576, '32:30').encode()


# ---- tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filt', SC.FILTERS)
def test_every_row_sums_to_one(filt):
    for n_in, n_out in [(64 * a, 64 * b) for a, b in RATIOS] + [(37, 35), (33, 40), (1, 1), (1, 9), (5, 1), (1080, 720), (576, 480)]:
        first, coef = SC.axis_table(n_in, n_out, filt)
        assert first.dtype == np.int32 and coef.dtype == np.int16 and first.shape == (n_out,)
        assert coef.shape == (n_out, SC.n_taps(n_in, n_out, filt))
        assert (coef.astype(np.int64).sum(axis=1) == 1 << 14).all()
        assert (np.diff(first) >= 0).all()                                   # what the kernel's row range rests on


@pytest.mark.parametrize('filt', SC.FILTERS)
def test_n_to_n_is_the_unit_tap(filt):
    for n in (1, 2, 7, 64):
        first, coef = SC.axis_table(n, n, filt)
        a = SC.SUPPORT[filt]
        assert coef.shape == (n, 2 * a) and (first == np.arange(n) - a + 1).all()
        unit = np.zeros(2 * a, np.int16)
        unit[a - 1] = 1 << 14
        assert (coef == unit).all()


def test_bilinear_tables():
    first, coef = SC.axis_table(32, 16, 'bilinear')
    assert (coef[1:-1] == (2048, 6144, 6144, 2048)).all() and (first == 2 * np.arange(16) - 1).all()
    assert (coef[0] == coef[1]).all() and first[0] == -1 and first[-1] + 3 == 32          # the edge rows clamp: index -1 and index 32
    first, coef = SC.axis_table(16, 32, 'bilinear')
    assert (coef[0::2] == (4096, 12288)).all() and (coef[1::2] == (12288, 4096)).all()
    assert first[0] == -1 and first[1] == 0 and first[-1] == 15 and (first[2::2] == first[1:-1:2]).all()


def test_edge_rows_clamp():
    for filt in SC.FILTERS:
        src = np.arange(10, dtype=np.int64)[None, :] * 100
        fx, cx = SC.axis_table(10, 10, filt)
        assert fx[0] <= 0 and fx[-1] + cx.shape[1] - 1 >= 10 - 1
        fx, cx = SC.axis_table(10, 23, filt)
        assert fx[0] < 0 and fx[-1] + cx.shape[1] - 1 > 9
        got = SC._taps(src, fx, cx, 1)
        want = np.array([[sum(int(cx[o, j]) * int(src[0, min(max(int(fx[o]) + j, 0), 9)]) for j in range(cx.shape[1])) for o in range(23)]])
        assert np.array_equal(got, want)
    up = SC.resize_plane_np(np.array([[7, 7, 7, 200]], np.uint8).repeat(3, 0), 3, 12, 'bilinear')
    assert (up[:, :4] == 7).all() and (up[:, -2:] == 200).all()             # half a sample beyond the edge repeats the edge


# ---- the plane rule ------------------------------------------------------------------------------------------------------------
def test_a_hand_computed_bilinear_case():
    """4x4 -> 2x2, bilinear: the weights of both axes are (1, 3, 3, 1) / 8, the first tap at index -1 and the last at 4 clamp to the
    edge, so a row of an output pair is (a + 3a + 3b + c) / 8 = (4a + 3b + c) / 8 and (b + 3c + 4d) / 8."""
    p = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120], [130, 140, 150, 255]], np.uint8)
    t = np.array([[(4 * a + 3 * b + c) * 8, (b + 3 * c + 4 * d) * 8] for a, b, c, d in p.tolist()])      # 6 fractional bits: x 64 / 8
    assert t.tolist() == [[1040, 2160], [3600, 4720], [6160, 7280], [8720, 12880]]
    v = [[(4 * t[0, x] + 3 * t[1, x] + t[2, x]) * 2048, (t[1, x] + 3 * t[2, x] + 4 * t[3, x]) * 2048] for x in range(2)]
    want = np.array([[(v[x][y] + (1 << 19)) >> 20 for x in range(2)] for y in range(2)])
    assert want.tolist() == [[41, 59], [111, 153]]                           # 41.25, 58.75, 111.25 and 152.5, which rounds up
    assert SC.resize_plane_np(p, 2, 2, 'bilinear').tolist() == want.tolist()
    assert SC.resize_plane_np(p.astype(np.uint16) * 4, 2, 2, 'bilinear', 1023).dtype == np.uint16


@pytest.mark.parametrize('filt', SC.FILTERS)
def test_a_constant_plane_stays_constant(filt):
    for (a, b), (peak, dt) in itertools.product([(4, 1), (6, 5), (5, 6), (1, 8)], [(255, np.uint8), (1023, np.uint16), (65535, np.uint16)]):
        n = 5 if (a, b) == (1, 8) else 6 * a
        for value in (0, 1, peak // 3, peak):
            out = SC.resize_plane_np(np.full((n * a, 2 * n * a), value, dt), n * b, 2 * n * b, filt, peak)
            assert out.shape == (n * b, 2 * n * b) and out.dtype == dt and (out == value).all()


@pytest.mark.parametrize('filt', SC.FILTERS)
def test_a_same_size_call_returns_the_input(filt):
    rng = np.random.default_rng(3)
    for peak, dt in ((255, np.uint8), (65535, np.uint16)):
        p = rng.integers(0, peak + 1, (13, 21)).astype(dt)
        assert np.array_equal(SC.resize_plane_np(p, 13, 21, filt, peak), p)
        only_rows = SC.resize_plane_np(p, 20, 21, filt, peak)               # one axis a copy: the other axis's rule alone
        fy, cy = SC.axis_table(13, 20, filt)
        want = np.clip((SC._taps(p.astype(np.int64) * 64, fy, cy, 0) + (1 << 19)) >> 20, 0, peak)
        assert np.array_equal(only_rows, want)


def test_alternating_rows_stay_in_range():
    """Rows of peak and 0 under lanczos3: the negative lobes push the sums past both ends, and the clip brings them back."""
    for peak, dt in ((255, np.uint8), (1023, np.uint16), (65535, np.uint16)):
        p = np.zeros((48, 40), dt)
        p[0::2] = peak
        hit = [False, False]
        for h_out in (40, 56, 47, 96):
            out = SC.resize_plane_np(p, h_out, 33, 'lanczos3', peak).astype(np.int64)
            assert out.min() >= 0 and out.max() <= peak
            fy, cy = SC.axis_table(48, h_out, 'lanczos3')
            raw = (SC._taps(p[:, :1].astype(np.int64) * 64, fy, cy, 0) + (1 << 19)) >> 20
            hit = [hit[0] or raw.min() < 0, hit[1] or raw.max() > peak]
        assert hit == [True, True]


# ---- against float64 -----------------------------------------------------------------------------------------------------------
FLOAT_CASES = [((64, 48), (16, 12)), ((37, 53), (35, 61)), ((33, 41), (40, 47)), ((60, 50), (50, 60)), ((8, 9), (64, 72)), ((48, 64), (24, 96))]


@pytest.mark.parametrize('depth', [8, 10, 16])
@pytest.mark.parametrize('filt', SC.FILTERS)
def test_against_a_float64_resample(filt, depth):
    """``float_resize_np`` resamples with the unquantised float64 weights w and rounds nothing.  With c the Q14 coefficients:
    the integer t / 2^F differs from sum (cx / 2^14) s by at most 2^-(F+1) (one rounding to F fractional bits), the vertical row weighs
    that by at most sum|cy| / 2^14, the final rounding adds 1/2, and replacing w by c / 2^14 moves a sum over samples in [0, peak] by at
    most peak * sum_j |c_j / 2^14 - w_j| on each axis.  So |integer - float| <= 1/2 + max_row sum|cy| 2^-(F+1) / 2^14 + peak (ex + ey),
    with ex, ey the largest summed coefficient-quantisation error of a row: ``scale.float_error_bound`` computes exactly that from the
    tables, per case.  Where the float value leaves [0, peak] the integer rule clips, so the float value is clipped too."""
    peak = (1 << depth) - 1
    rng = np.random.default_rng(depth)
    for (h, w), (ho, wo) in FLOAT_CASES:
        p = rng.integers(0, peak + 1, (h, w)).astype(np.uint16)
        got = SC.resize_plane_np(p, ho, wo, filt, peak).astype(np.float64)
        ref = np.clip(SC.float_resize_np(p, ho, wo, filt), 0, peak)
        bound = SC.float_error_bound((h, w), ho, wo, filt, peak)
        (_, wx), (_, cx) = SC._axis(w, wo, filt), SC.axis_table(w, wo, filt)
        (_, wy), (_, cy) = SC._axis(h, ho, filt), SC.axis_table(h, ho, filt)
        ex, ey = np.abs(cx / 16384 - wx).sum(axis=1).max(), np.abs(cy / 16384 - wy).sum(axis=1).max()
        assert bound == 0.5 + np.abs(cy.astype(np.float64)).sum(axis=1).max() / 16384 / 128 + peak * (ex + ey)
        worst = np.abs(got - ref).max()
        print('%s %d bits %dx%d -> %dx%d: %.4f LSB of %.4f allowed' % (filt, depth, w, h, wo, ho, worst, bound))
        assert worst <= bound, (filt, depth, (h, w), (ho, wo), worst, bound)


# ---- accumulator widths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filt', SC.FILTERS)
def test_accumulator_bounds(filt):
    """Both sums fit int32 at peak = 255 and the horizontal one at peak = 65535: what the kernel's int32 accumulators rest on.  The
    vertical sum at 16 bits does not (the kernel keeps it in 64 bits); the bound is exact: planes that reach it are built below."""
    top = 0
    for (ax, bx), (ay, by) in itertools.product(RATIOS, RATIOS):
        tables = (SC.axis_table(48 * ax, 48 * bx, filt), SC.axis_table(48 * ay, 48 * by, filt))
        h8, v8 = SC.accumulator_bounds(tables, 255)
        h16, v16 = SC.accumulator_bounds(tables, 65535)
        assert h8 < 2 ** 31 and v8 < 2 ** 31 and h16 < 2 ** 31 and v16 < 2 ** 63
        assert all(np.abs(c.astype(np.int64)).sum(axis=1).max() < 2 * (1 << 14) for _, c in tables)
        top = max(top, v16)
    assert (top >= 2 ** 31) == (filt != 'bilinear') or top >= 2 ** 31
    # the bound is reached: the source that drives one output sample's sums to their extremes
    (fx, cx), (fy, cy) = tables = (SC.axis_table(48, 40, filt), SC.axis_table(48, 40, filt))
    hb, vb = SC.accumulator_bounds(tables, 65535)
    xo = int(np.clip(cx, 0, None).sum(axis=1).argmax())
    row = np.zeros(48, np.int64)
    for j in range(cx.shape[1]):
        i = min(max(int(fx[xo]) + j, 0), 47)
        row[i] = 65535 if cx[xo, j] > 0 else row[i]
    got = int(SC._taps(row[None, :], fx, cx, 1)[0, xo]) + 128
    assert got <= hb and (filt == 'bilinear' or got > 0.98 * hb)


# ---- payloads and streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['420', '422', '444', 'mono'])
@pytest.mark.parametrize('depth', [8, 10, 16])
def test_payload_sizes(layout, depth):
    rng = np.random.default_rng(5)
    dt = np.uint16 if depth > 8 else np.uint8
    for (h, w), (ho, wo) in (((37, 53), (35, 61)), ((33, 41), (15, 23)), ((3, 5), (9, 7))):
        p = rng.integers(0, 1 << depth, y4m.payload_size(h, w, layout)).astype(dt)
        out = SC.scale_payload_np(p, h, w, ho, wo, depth, layout, 'bicubic')
        assert out.dtype == dt and out.shape == (y4m.payload_size(ho, wo, layout),) and int(out.max()) < 1 << depth
        planes_in = [a for a in y4m.split_planes_layout(p, h, w, layout) if a is not None]
        planes_out = [a for a in y4m.split_planes_layout(out, ho, wo, layout) if a is not None]
        assert [a.shape for a in planes_out] == plane_shapes(ho, wo, layout)
        for a, b in zip(planes_in, planes_out):                            # every plane on its own, chroma centre-aligned like luma
            assert np.array_equal(b, SC.resize_plane_np(a, b.shape[0], b.shape[1], 'bicubic', (1 << depth) - 1))
    with pytest.raises(ValueError, match='samples at'):
        SC.scale_payload_np(np.zeros(6, np.uint8 if depth > 8 else np.uint16), 2, 2, 4, 4, depth, '420')


def test_a_stream_is_scaled_header_and_all():
    rng = np.random.default_rng(8)
    for ctag, depth, layout in (('420jpeg', 8, '420'), ('422p10', 10, '422'), ('mono', 8, 'mono')):
        h, w, es = 18, 26, 2 if depth > 8 else 1
        P = y4m.payload_size(h, w, layout)
        pays = [rng.integers(0, 1 << depth, P).astype('<u2' if es == 2 else np.uint8) for _ in range(3)]
        head = b'YUV4MPEG2 W26 H18 F30000:1001 Ip A10:11 C%s XCOLORRANGE=FULL\n' % ctag.encode()
        data = head + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
        out = SC.scale_stream_np(data, 40, 12, 'bilinear')
        ohead = out[:out.index(b'\n') + 1]
        assert ohead == b'YUV4MPEG2 W40 H12 F30000:1001 Ip A13:33 C%s XCOLORRANGE=FULL\n' % ctag.encode()       # 10 * 26 * 12 : 11 * 18 * 40
        rd = y4m.Reader(io.BytesIO(out), y4m.DEPTHS, y4m.LAYOUTS)
        buf = np.empty(rd.header.payload, np.uint8)
        for p in pays:
            assert rd.read_into(buf)
            assert buf.tobytes() == SC.scale_payload_np(p, h, w, 12, 40, depth, layout, 'bilinear').tobytes()
        assert not rd.read_into(buf)
        assert SC.scale_stream_np(data, 26, 18) == data                     # the same size: every byte
        assert SC.scale_stream_np(head, 40, 12) == ohead                    # a header alone
    with pytest.raises(y4m.Y4MError):
        SC.scale_stream_np(b'YUV4MPEG2 W26 H18 F25:1 It C420jpeg\n', 40, 12)             # a scaler never sees woven fields


def test_table_blob_layout():
    shapes_in, shapes_out = plane_shapes(37, 53, '420'), plane_shapes(35, 61, '420')
    blob, desc = SC.table_blob(shapes_in, shapes_out, 'lanczos3')
    assert blob.dtype == np.uint8 and desc.dtype == np.int32 and desc.shape == (3 * SC.DESC_WORDS + 1,) and desc[-1] == blob.size
    assert (desc[6:12] == desc[12:18]).all() and blob.size % 4 == 0         # Cb and Cr share their tables
    for p, ((ri, ci), (ro, co)) in enumerate(zip(shapes_in, shapes_out)):
        fxo, cxo, tx, fyo, cyo, ty = desc[6 * p:6 * p + 6]
        for off, n_in, n_out, t, c_off in ((fxo, ci, co, tx, cxo), (fyo, ri, ro, ty, cyo)):
            first, coef = SC.axis_table(n_in, n_out, 'lanczos3')
            assert off % 4 == 0 and c_off % 4 == 0 and t == coef.shape[1]
            assert np.array_equal(blob[off:off + 4 * n_out].view(np.int32), first)
            assert np.array_equal(blob[c_off:c_off + 2 * n_out * t].view(np.int16).reshape(n_out, t), coef)


# ---- the switches --------------------------------------------------------------------------------------------------------------
def test_check_scale_and_the_runner_s_refusals():
    assert video.check_scale(None) is None
    assert video.check_scale('1280x720') == (1280, 720, 'lanczos3') == video.check_scale((1280, 720), None)
    assert video.check_scale((64, 48), 'bilinear', crop=(8, 8, 0, 0), crop_output='cropped') == (64, 48, 'bilinear')
    with pytest.raises(ValueError, match='--scale-filter.*--scale'):
        video.check_scale(None, 'bicubic')
    with pytest.raises(ValueError, match='--crop-output cropped'):
        video.check_scale((64, 48), None, crop=(8, 8, 0, 0))
    with pytest.raises(ValueError, match='--crop-output cropped'):
        video.VideoRunner(None, mfi=2, scale=(64, 48), crop='auto')
    with pytest.raises(ValueError, match='--scale-filter'):
        video.VideoRunner(None, mfi=2, scale_filter='bilinear')
    with pytest.raises(ValueError, match='--scale-filter'):
        video.VideoRunner(None, mfi=2, scale=(64, 48), scale_filter='cubic')
    vr = video.VideoRunner(None, mfi=2)
    assert vr.scale is None and vr.last_scale is None and vr.last_scale_payloads == 0


def test_the_output_header_and_the_edge_spec():
    hdr = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 Ip A16:15 C420jpeg')
    plain = video.VideoRunner(None, mfi=2)
    vr = video.VideoRunner(None, mfi=2, scale='720x480', scale_filter='bicubic')
    assert vr._out_header(hdr).encode() == b'YUV4MPEG2 W720 H480 F50:1 Ip A8:9 C420jpeg\n'
    assert EdgeSpec.of(vr._edge(hdr, lambda k: False)).scale == (720, 480, 'bicubic')
    il = video.VideoRunner(None, mfi=2, scale=(720, 480), interlace='tff')
    assert il._out_header(hdr).encode() == b'YUV4MPEG2 W720 H480 F25:1 It A8:9 C420jpeg\n'      # scaled first, then the fields' header
    # the run's own size: no stage, the header and the spec of a run without the switch
    same = video.VideoRunner(None, mfi=2, scale=(720, 576))
    assert same._scale_of(hdr) is None and same._out_header(hdr).encode() == plain._out_header(hdr).encode()
    assert EdgeSpec.of(same._edge(hdr, lambda k: False)) == EdgeSpec.of(plain._edge(hdr, lambda k: False))
    # before anything is allocated: the interlaced grid and the tap limit
    with pytest.raises(ValueError, match='--scale with --interlace.*multiple of 4'):
        video.VideoRunner(None, mfi=2, scale=(720, 482), interlace='tff')._out_header(hdr)
    h422 = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 Ip C422', layouts=y4m.LAYOUTS)
    assert video.VideoRunner(None, mfi=2, scale=(720, 482), interlace='tff', layouts=True)._out_header(h422).h == 482
    with pytest.raises(ValueError, match='multiple of 2'):
        video.VideoRunner(None, mfi=2, scale=(720, 481), interlace='bff', layouts=True)._out_header(h422)
    with pytest.raises(ValueError, match='more than 32'):
        video.VideoRunner(None, mfi=2, scale=(720, 100))._out_header(hdr)
    assert video.VideoRunner(None, mfi=2, scale=(720, 100), scale_filter='bilinear')._out_header(hdr).h == 100


def test_the_edge_spec_keeps_scale_beside_the_tuple():
    a, b = EdgeSpec(y4m=True), EdgeSpec(y4m=True, scale=(64, 48, 'lanczos3'))
    assert a.scale is None and a == tuple(a) and b != a and b != tuple(b) and hash(a) == hash(EdgeSpec(y4m=True))
    assert b == EdgeSpec(y4m=True, scale=[64, 48, 'lanczos3']) and hash(b) == hash(b._replace()) and b._replace(full=True).scale == b.scale
    assert b._replace(scale=None) == a and 'scale=' not in repr(a) and "scale=(64, 48, 'lanczos3')" in repr(b)
    assert b != EdgeSpec(y4m=True, scale=(64, 48, 'bicubic')) and len({a, b, b._replace(interlace=('t', 'off'))}) == 3
    b.check(True, False, False)
    with pytest.raises(ValueError, match='resized output needs the Y4M edge'):
        EdgeSpec(scale=(64, 48, 'lanczos3')).check(False, False, False)
    with pytest.raises(ValueError, match='scale must be'):
        EdgeSpec(y4m=True, scale=(64, 48, 'nearest')).check(True, False, False)


def test_the_command_line():
    a = video.parser().parse_args(['in', 'out', '--scale', '1280x720', '--scale-filter', 'bicubic'])
    assert a.scale == (1280, 720) and a.scale_filter == 'bicubic'
    a = video.parser().parse_args(['in', 'out'])
    assert a.scale is None and a.scale_filter is None
    text = video.parser().format_help()
    assert 'WIDTH FIRST' in text and '--scale-filter' in text
    for argv in (['in', 'out', '--scale', '1280'], ['in', 'out', '--scale', '64x48', '--scale-filter', 'nearest']):
        with pytest.raises(SystemExit):
            video.parser().parse_args(argv)
    for argv in (['in', 'out', '--scale-filter', 'bicubic'], ['in', 'out', '--scale', '64x48', '--crop', '8:8:0:0']):
        with pytest.raises(SystemExit):                                     # refused before a GPU is looked for
            video.main(argv)
