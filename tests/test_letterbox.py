"""Letterbox and pillarbox bars (``--crop``), the host side: ``demfi_amd.letterbox``'s definitions and policy against loops and
hand-made frames, the crop / pad round trips over every layout, ``Cropper`` against the numpy conversions, and the refusals of
``VideoRunner`` and the command line, none of which loads the HIP library."""
import io
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import _lib as L
from demfi_amd import letterbox as LB
from demfi_amd import video, y4m


# ---- detection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,thresh', [(np.uint8, 24), (np.uint8, 0), (np.uint16, 96), (np.uint16, 65535)])
@pytest.mark.parametrize('h,w', [(2, 2), (5, 9), (13, 7)])
def test_line_counts_equal_a_double_loop(h, w, dt, thresh):
    rng = np.random.default_rng(h * 17 + w)
    hi = min(thresh + 1, np.iinfo(dt).max)
    luma = rng.choice(np.array([0, max(thresh - 1, 0), thresh, hi, np.iinfo(dt).max], dt), h * w + 5)      # five samples of chroma behind
    rows, cols = np.zeros(h, np.uint32), np.zeros(w, np.uint32)
    for y in range(h):
        for x in range(w):
            if int(luma[y * w + x]) > thresh:
                rows[y] += 1
                cols[x] += 1
    got = LB.line_counts_np(luma, h, w, thresh)
    assert got[0].dtype == got[1].dtype == np.uint32
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols) and rows.sum() == cols.sum()
    if thresh == np.iinfo(dt).max:
        assert rows.sum() == 0
    elif h * w > 40:                                     # lit and dark samples both occur
        assert 0 < rows.sum() < h * w


def test_the_compare_is_strict():
    luma = np.array([24, 25, 24, 25, 25, 25], np.uint8)
    rows, cols = LB.line_counts_np(luma, 2, 3, 24)
    assert rows.tolist() == [1, 3] and cols.tolist() == [1, 2, 1]
    with pytest.raises(ValueError):
        LB.line_counts_np(luma, 3, 3, 24)
    with pytest.raises(ValueError):
        LB.line_counts_np(luma.astype(np.int32), 2, 3, 24)


def _boxed(h, w, rect, value=120, dt=np.uint8):
    y = np.full((h, w), 16, dt)
    t, b, l, r = rect
    y[t:b, l:r] = value
    return y


def _counts(y, thresh=24):
    return LB.line_counts_np(y.reshape(-1), y.shape[0], y.shape[1], thresh)


def test_frame_extent_and_the_noise_allowance():
    h, w, rect = 300, 520, (40, 260, 12, 500)
    y = _boxed(h, w, rect)
    assert LB.allowance(w) == 2 and LB.allowance(h) == 1 and LB.allowance(255) == 0 and LB.allowance(512, Fraction(1, 128)) == 4
    assert LB.frame_extent(*_counts(y)) == rect
    y[10, 100:102] = 255                                 # two hot pixels in a row of 520: within floor(520 / 256) = 2
    y[100:101, 5] = 255                                  # one in a column of 300: within floor(300 / 256) = 1
    assert LB.frame_extent(*_counts(y)) == rect
    y[10, 100:103] = 255                                 # three: a picture row
    assert LB.frame_extent(*_counts(y)) == (10, 260, 12, 500)
    y[10] = 16
    y[280:284, 200:320] = 235                            # a line of subtitle text set in the bottom bar keeps that bar
    assert LB.frame_extent(*_counts(y)) == (40, 284, 12, 500)
    assert LB.frame_extent(*_counts(np.full((h, w), 16, np.uint8))) is None
    assert LB.frame_extent(*_counts(_boxed(h, w, rect, 24))) is None                  # at the limit is not above it
    assert LB.frame_extent(*_counts(_boxed(h, w, rect), 0)) == (0, h, 0, w)           # limit 0: the bars' 16 is lit
    assert LB.frame_extent(*_counts(y), noise=0) == (40, 284, 5, 500)                 # no allowance: the speck counts


def test_extent_is_the_union_and_black_frames_contribute_nothing():
    h, w = 200, 300
    e = LB.Extent()
    assert e.rect() is None
    e.push(*_counts(np.full((h, w), 16, np.uint8)))      # a black frame
    assert e.rect() is None and (e.frames, e.lit) == (1, 0)
    e.push(*_counts(_boxed(h, w, (30, 170, 0, w))))
    e.push(*_counts(np.full((h, w), 3, np.uint8)))       # a fade-out's end
    e.push(*_counts(_boxed(h, w, (40, 180, 20, 280))))
    assert e.rect() == (30, 180, 0, w) and (e.frames, e.lit) == (4, 2)


# ---- alignment and policy ------------------------------------------------------------------------------------------------------
def test_align_rect_for_every_layout_and_both_field_counts():
    assert [LB.units(lay, f) for lay in y4m.LAYOUTS for f in (1, 2)] == [(2, 2), (4, 2), (1, 2), (2, 2), (1, 1), (2, 1), (1, 1), (2, 1)]
    h, w, rect = 101, 77, (5, 71, 7, 63)
    exp = {('420', 1): (4, 72, 6, 64), ('420', 2): (4, 72, 6, 64), ('422', 1): (5, 71, 6, 64), ('422', 2): (4, 72, 6, 64),
           ('444', 1): rect, ('444', 2): (4, 72, 7, 63), ('mono', 1): rect, ('mono', 2): (4, 72, 7, 63)}
    for (lay, f), e in exp.items():
        assert LB.align_rect(rect, h, w, lay, f) == e, (lay, f)
    assert LB.align_rect((6, 70, 7, 63), h, w, '420', 2) == (4, 72, 6, 64)
    # a rectangle that touches the odd frame's edge stays there: bottom = h and right = w are allowed as they are
    assert LB.align_rect((3, 101, 9, 77), h, w, '420', 1) == (2, 101, 8, 77)
    assert LB.align_rect((3, 99, 9, 77), h, w, '420', 2) == (0, 100, 8, 77)
    assert LB.align_rect((3, 100, 9, 77), h, w, '420', 2) == (0, 100, 8, 77) and LB.align_rect((3, 101, 9, 76), h, w, '420', 2) == (0, 101, 8, 76)
    for lay in y4m.LAYOUTS:                              # the cropped frame has the chroma shape of its own size
        for f in (1, 2):
            t, b, l, r = LB.align_rect(rect, h, w, lay, f)
            planes = LB.plane_rects(h, w, lay, (t, b, l, r))
            for _, _, _, (r0, r1, c0, c1) in planes[1:]:
                assert (r1 - r0, c1 - c0) == y4m.chroma_shape(b - t, r - l, lay)
    with pytest.raises(ValueError):
        LB.units('420', 3)


def test_parse_crop_check_rect_and_probe_indices():
    assert LB.parse_crop('auto') == 'auto' and LB.parse_crop('140:140:0:0') == (140, 140, 0, 0)
    for bad in ('', 'on', '1:2:3', '1:2:3:4:5', '-1:0:0:0', '1.5:0:0:0', 'a:b:c:d', '1:2:3:'):
        with pytest.raises(ValueError, match='T:B:L:R'):
            LB.parse_crop(bad)
    assert LB.check_crop(None) is None and LB.check_crop('2:2:0:0') == (2, 2, 0, 0) and LB.check_crop([1, 2, 3, 4]) == (1, 2, 3, 4)
    for bad in ((1, 2, 3), (1, 2, 3, -4), (1.0, 2, 3, 4), True, 7):
        with pytest.raises(ValueError):
            LB.check_crop(bad)
    h, w = 1080, 1920
    assert LB.bars_rect((140, 140, 0, 0), h, w) == (140, 940, 0, 1920)
    assert LB.check_rect((140, 940, 0, 1920), h, w, '420', 1, explicit=True) == ((140, 940, 0, 1920), None)
    assert LB.check_rect((0, h, 0, w), h, w, '420', 1, explicit=True) == (None, None)      # the whole frame: no crop stage
    assert LB.check_rect((0, h, 0, w), h, w, '420', 1) == (None, None)
    assert LB.check_rect((139, 941, 1, 1919), h, w, '420', 1) == ((138, 942, 0, 1920), None)            # a detected one is aligned
    with pytest.raises(ValueError) as e:                                                                 # an explicit one must be
        LB.check_rect((139, 941, 0, 1920), h, w, '420', 1, explicit=True)
    assert 'multiples of 2 rows' in str(e.value) and '138:138:0:0' in str(e.value)
    with pytest.raises(ValueError) as e:
        LB.check_rect((138, 942, 0, 1920), h, w, '420', 2, explicit=True)
    assert 'multiples of 4 rows' in str(e.value) and 'interlaced' in str(e.value) and '136:136:0:0' in str(e.value)
    assert LB.check_rect((138, 942, 0, 1920), h, w, '422', 1, explicit=True)[0] == (138, 942, 0, 1920)
    with pytest.raises(ValueError, match='at least 64x64'):
        LB.check_rect((500, 562, 0, 1920), h, w, '420', 1, explicit=True)
    with pytest.raises(ValueError, match='leave nothing'):
        LB.check_rect(LB.bars_rect((600, 600, 0, 0), h, w), h, w, '420', 1, explicit=True)
    rect, note = LB.check_rect((500, 562, 0, 1920), h, w, '420', 1)                     # auto below MIN_ACTIVE: whole, and reported
    assert rect is None and '62' in note and 'whole' in note
    assert LB.check_rect((500, 564, 100, 164), h, w, '420', 1)[0] == (500, 564, 100, 164)
    rect, note = LB.check_rect(None, h, w, '420', 1)
    assert rect is None and 'no probed frame' in note
    assert LB.probe_indices(7) == list(range(7)) and LB.probe_indices(7, 'all') == list(range(7)) and LB.probe_indices(0) == []
    assert LB.probe_indices(10, 4) == [0, 2, 5, 7] and LB.probe_indices(3, 5) == [0, 1, 2] and LB.probe_indices(5, 5) == [0, 1, 2, 3, 4]
    for bad in (0, -1, 'some', 2.0, True):
        with pytest.raises(ValueError):
            LB.probe_indices(10, bad)
    for bad in (dict(limit=-1), dict(limit=256), dict(limit=2.0), dict(noise=0.5), dict(noise=1), dict(noise=-1), dict(noise='x'),
                dict(output='both')):
        with pytest.raises(ValueError):
            LB.check_params(**bad)
    assert LB.check_params(noise='1/128')[1] == Fraction(1, 128) and LB.parse_probe('all') == 'all' and LB.parse_probe('12') == 12
    with pytest.raises(ValueError):
        LB.parse_probe('0')
    assert (LB.DEFAULT_LIMIT, LB.DEFAULT_NOISE, LB.MIN_ACTIVE) == (24, Fraction(1, 256), 64)


# ---- the two conversions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('h,w,rect,fields', [(24, 40, (4, 20, 6, 30), 1), (23, 37, (4, 23, 8, 37), 1), (23, 37, (8, 20, 0, 36), 2),
                                             (23, 37, (0, 23, 2, 34), 1)])
def test_crop_and_pad_round_trips_and_the_cropper(h, w, rect, fields, layout, depth):
    assert LB.align_rect(rect, h, w, layout, fields) == rect
    dt, peak = (np.uint8, 255) if depth == 8 else (np.uint16, 1023)
    rng = np.random.default_rng(h + w + depth)
    t, b, l, r = rect
    ah, aw = b - t, r - l
    full = rng.integers(0, peak + 1, y4m.payload_size(h, w, layout)).astype(dt)
    act = LB.crop_payload_np(full, h, w, depth, layout, rect)
    assert act.dtype == dt and act.size == y4m.payload_size(ah, aw, layout)
    planes, aplanes = y4m.split_planes_layout(full, h, w, layout), y4m.split_planes_layout(act, ah, aw, layout)
    assert np.array_equal(aplanes[0], planes[0][t:b, l:r])
    if layout != 'mono':
        sv, sh = {'420': (2, 2), '422': (1, 2), '444': (1, 1)}[layout]
        for p, a in zip(planes[1:], aplanes[1:]):
            assert np.array_equal(a, p[t // sv:-(-b // sv), l // sh:-(-r // sh)])
    for full_range in (False, True):
        x = rng.integers(0, peak + 1, act.size).astype(dt)
        padded = LB.pad_payload_np(x, h, w, depth, layout, rect, full_range)
        assert padded.dtype == dt and np.array_equal(LB.crop_payload_np(padded, h, w, depth, layout, rect), x)      # crop(pad(x)) == x
        yb, cb = (0 if full_range else 16 << (depth - 8)), 1 << (depth - 1)
        pp = y4m.split_planes_layout(padded, h, w, layout)
        outside = np.ones((h, w), bool)
        outside[t:b, l:r] = False
        assert (pp[0][outside] == yb).all() and outside.any()
        if layout != 'mono':
            inside = np.zeros(pp[1].shape, bool)
            inside[t // sv:-(-b // sv), l // sh:-(-r // sh)] = True
            assert (pp[1][~inside] == cb).all() and (pp[2][~inside] == cb).all()
        # pad(crop(p)) == p for a payload whose outside is that black
        assert np.array_equal(LB.pad_payload_np(LB.crop_payload_np(padded, h, w, depth, layout, rect), h, w, depth, layout, rect, full_range), padded)
        hdr = y4m.Header(w, h, 24, 'p', '1:1', color_range='FULL' if full_range else None, depth=depth, layout=layout)
        cr = LB.Cropper(hdr, rect)
        assert (cr.Pf, cr.Pa) == (hdr.payload, LB.cropped_header(hdr, rect).payload)
        buf = np.full(cr.Pa, 0xEE, np.uint8)
        cr.crop_into(full.view(np.uint8), buf)
        assert np.array_equal(buf, act.view(np.uint8))
        two = np.stack([x.view(np.uint8), act.view(np.uint8)])
        out = np.full((2, cr.Pf), 0xEE, np.uint8)
        cr.pad_into(two, out)
        assert np.array_equal(out[0], padded.view(np.uint8))
        assert np.array_equal(out[1], LB.pad_payload_np(act, h, w, depth, layout, rect, full_range).view(np.uint8))
        with pytest.raises(ValueError):
            cr.crop_into(full.view(np.uint8)[:-1], buf)
    with pytest.raises(ValueError):
        LB.crop_payload_np(full[:-1], h, w, depth, layout, rect)
    with pytest.raises(ValueError):
        LB.crop_payload_np(full, h, w, depth, layout, (t, h + 1, l, r))


def test_cropped_header_keeps_everything_but_the_size():
    hdr = y4m.parse_header(b'YUV4MPEG2 W1920 H1080 F24000:1001 Ip A1:1 C420p10 XCOLORRANGE=FULL XYSCSS=420P10', y4m.DEPTHS)
    c = LB.cropped_header(hdr, (140, 940, 0, 1920))
    assert c.encode() == hdr.encode().replace(b'H1080', b'H800') and (c.h, c.w, c.aspect, c.depth) == (800, 1920, '1:1', 10)
    assert c.payload == y4m.payload_bytes(800, 1920, 10) and hdr.h == 1080


# ---- VideoRunner and the command line: refused before a library is loaded ----------------------------------------------------------
def _stream(h=96, w=128, n=4, tags=b'Ip C420jpeg'):
    return b'YUV4MPEG2 W%d H%d F24:1 %s\n' % (w, h, tags) + (b'FRAME\n' + bytes(y4m.payload_size(h, w))) * n


def test_runner_refusals_happen_before_a_library_is_loaded(tmp_path):
    loaded = L._lib
    vr = video.VideoRunner(None, crop='auto')
    with pytest.raises(ValueError, match='cropdetect') as e:
        vr.run_stream(io.BytesIO(_stream()), io.BytesIO())
    assert 'T:B:L:R' in str(e.value)
    for crop, msg in (((1, 0, 0, 0), 'multiples of 2 rows'), ((0, 0, 3, 0), 'and 2 columns'), ((20, 20, 0, 0), 'at least 64x64'),
                      ((0, 0, 64, 64), 'leave nothing')):
        vr = video.VideoRunner(None, crop=crop)
        with pytest.raises(ValueError, match=msg):
            vr.run_stream(io.BytesIO(_stream()), io.BytesIO())
        src = tmp_path / 'in.y4m'
        src.write_bytes(_stream())
        with pytest.raises(ValueError, match=msg):
            vr.run_file(str(src), str(tmp_path / 'out.y4m'))
        assert not vr._runners
    vr = video.VideoRunner(None, crop=(2, 2, 0, 0), deinterlace=True)                  # interlaced payloads: rows in units of 4
    with pytest.raises(ValueError, match='multiples of 4 rows'):
        vr.run_stream(io.BytesIO(_stream(tags=b'It C420jpeg')), io.BytesIO())
    for kw in (dict(crop_limit=30), dict(crop_noise=Fraction(1, 128)), dict(crop_probe=8), dict(crop_output='cropped')):
        with pytest.raises(ValueError, match='--crop'):
            video.VideoRunner(None, **kw)
        video.VideoRunner(None, crop='auto', **kw)
    for kw in (dict(crop='sometimes'), dict(crop=(1, 2, 3)), dict(crop='auto', crop_limit=300), dict(crop='auto', crop_noise=0.01),
               dict(crop='auto', crop_probe=0), dict(crop='auto', crop_output='both')):
        with pytest.raises(ValueError):
            video.VideoRunner(None, **kw)
    vr = video.VideoRunner(None)
    assert (vr.crop, vr.last_crop, vr.last_crop_probed) == (None, None, 0)
    assert video.VideoRunner(None, crop='4:4:0:0').crop == (4, 4, 0, 0)
    assert L._lib is loaded                                                            # nothing above loaded the library


def test_command_line_has_the_switches(capsys):
    a = video.parser().parse_args(['in.y4m', 'out.y4m', '--crop', 'auto', '--crop-limit', '30', '--crop-noise', '1/128', '--crop-probe', '12',
                                   '--crop-output', 'cropped'])
    assert (a.crop, a.crop_limit, a.crop_noise, a.crop_probe, a.crop_output) == ('auto', 30, Fraction(1, 128), 12, 'cropped')
    a = video.parser().parse_args(['-', '-', '--crop', '140:140:0:0'])
    assert a.crop == (140, 140, 0, 0) and (a.crop_limit, a.crop_noise, a.crop_probe, a.crop_output) == (None, None, None, None)
    assert video.parser().parse_args(['-', '-']).crop is None
    for bad in (['--crop', 'yes'], ['--crop-probe', '0'], ['--crop-noise', '3/2'], ['--crop-output', 'both']):
        with pytest.raises(SystemExit):
            video.parser().parse_args(['-', '-'] + bad)
    for argv in (['-', '-', '--crop-limit', '30'], ['-', '-', '--crop-output', 'cropped'], ['-', '-', '--crop', 'auto']):
        with pytest.raises(SystemExit):                  # a secondary switch without --crop; auto on a pipe: both before any GPU work
            video.main(argv)
    err = capsys.readouterr().err
    assert 'say how --crop works' in err and 'cropdetect' in err
