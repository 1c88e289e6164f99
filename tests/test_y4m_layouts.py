"""4:2:2, 4:4:4 and mono Y4M (C422, C444, Cmono and their deep forms C422pNN / C444pNN / CmonoNN): the opt-in of the parser
(``layouts=y4m.LAYOUTS``), payload bytes through Reader / scan / Frames / Writer, the conversion definition per layout anchored
exactly to the 4:2:0 definition where the two must agree, its accuracy against a float64 matrix conversion, and the scene-cut
scores over a payload of another layout.

The accuracy bound 0.5 + 3 * 2^-9 LSB is the one derived in tests/test_y4m_depth.py and carries over because the form of the
definition is unchanged: ONE rounding of the result (0.5) plus at most three coefficient errors, each at most 2^-(9+d) (Q(8+d),
rounded half up) on an operand below 2^d.  The resampling adds nothing to it: upsampled chroma is exact in 1/16 units, and for
4:2:2 the float64 reference applies the same co-sited [1,2,1]/4 to the full-resolution chroma before the one rounding."""
import io

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import y4m

NEW = ('422', '444', 'mono')
HIGH = (10, 12, 14, 16)
BOUND = 0.5 + 3 * 2.0 ** -9
CONFIGS = [(m, f) for m in ('bt601', 'bt709') for f in (False, True)]


def _tag(layout, d):
    return layout if d == 8 else ('mono%d' if layout == 'mono' else layout + 'p%d') % d


def _samples(h, w, layout):
    cw = (w + 1) // 2
    return {'422': h * w + 2 * h * cw, '444': 3 * h * w, 'mono': h * w}[layout]


TAGS = [(lay, d) for lay in NEW for d in (8,) + HIGH]


# ---- headers ------------------------------------------------------------------------------------------------------------------
def test_layouts_constant_and_payload_sizes():
    assert y4m.LAYOUTS == ('420', '422', '444', 'mono')
    for h, w in ((3, 5), (53, 37), (2, 2), (64, 96)):
        assert y4m.payload_size(h, w) == y4m.payload_size(h, w, '420') == h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)
        for lay in NEW:
            assert y4m.payload_size(h, w, lay) == _samples(h, w, lay)
            assert y4m.payload_bytes(h, w, 8, lay) == _samples(h, w, lay) and y4m.payload_bytes(h, w, 10, lay) == 2 * _samples(h, w, lay)
    with pytest.raises(ValueError):
        y4m.payload_size(4, 4, '411')


@pytest.mark.parametrize('layout,d', TAGS)
@pytest.mark.parametrize('w,h', [(5, 3), (37, 53)])
def test_header_round_trip_and_payload_bytes(layout, d, w, h):
    tag = _tag(layout, d)
    line = b'YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C%s XCOLORRANGE=FULL\n' % (w, h, tag.encode())
    hdr = y4m.parse_header(line, depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    assert (hdr.w, hdr.h, hdr.depth, hdr.layout, hdr.ctag, hdr.full_range, hdr.peak) == (w, h, d, layout, tag, True, (1 << d) - 1)
    assert hdr.payload == _samples(h, w, layout) * (1 if d == 8 else 2)
    assert hdr.frame_bytes == 6 + hdr.payload
    assert hdr.encode() == line
    again = y4m.parse_header(hdr.encode(), depths=y4m.DEPTHS, layouts=y4m.LAYOUTS)
    assert (again.depth, again.layout, again.payload, again.encode()) == (d, layout, hdr.payload, line)
    for out in (y4m.output_header(hdr, 4), R.output_header(hdr, hdr.fps * 4)):
        assert (out.depth, out.layout, out.ctag, out.payload, out.color_range) == (d, layout, tag, hdr.payload, 'FULL')
        assert out.fps == hdr.fps * 4 and b' C%s ' % tag.encode() in out.encode()
    assert y4m.output_ctag(d, layout) == tag
    assert R.block_offset(40, 2, 4, hdr.payload) == y4m.frame_offset(40, 8, hdr.payload) == 40 + 8 * (6 + hdr.payload)
    if d == 8:                                                             # the 8-bit tags need no depths=
        assert y4m.parse_header(line, layouts=y4m.LAYOUTS).payload == hdr.payload


@pytest.mark.parametrize('layout,d', TAGS)
def test_new_tags_are_refused_without_the_opt_in(layout, d):
    line = b'YUV4MPEG2 W64 H48 F25:1 Ip C' + _tag(layout, d).encode()
    for kw in ({}, {'depths': y4m.DEPTHS}, {'layouts': ('420',)}, {'depths': y4m.DEPTHS, 'layouts': ('420',)}):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(line, **kw)
        assert y4m.FIX in str(e.value) and '--any-layout' in str(e.value)
    with pytest.raises(y4m.Y4MError):
        y4m.Reader(io.BytesIO(line + b'\n'))
    if d > 8:                                                              # a deep tag needs depths= as well
        for kw in ({'layouts': y4m.LAYOUTS}, {'layouts': y4m.LAYOUTS, 'depths': (8,)}):
            with pytest.raises(y4m.Y4MError) as e:
                y4m.parse_header(line, **kw)
            assert y4m.FIX in str(e.value) and '--high-depth' in str(e.value)


@pytest.mark.parametrize('tag', ['411', '420paldv', '444alpha', '420p9', '422p9', '444p11', 'mono9', 'mono8', '422p10le', '440'])
def test_other_tags_stay_refused_with_every_switch(tag):
    for kw in ({}, {'layouts': y4m.LAYOUTS}, {'layouts': y4m.LAYOUTS, 'depths': y4m.DEPTHS}):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C' + tag.encode(), **kw)
        assert y4m.FIX in str(e.value)


def test_420_headers_are_as_before_with_the_switch_on():
    for line, kw in ((b'YUV4MPEG2 W64 H48 F25:1 Ip C420mpeg2', {}), (b'YUV4MPEG2 W64 H48 F25:1', {}),
                     (b'YUV4MPEG2 W64 H48 F25:1 Ip C420p10', {'depths': y4m.DEPTHS})):
        a, b = y4m.parse_header(line, **kw), y4m.parse_header(line, layouts=y4m.LAYOUTS, **kw)
        assert (a.layout, b.layout) == ('420', '420') and a.encode() == b.encode() and a.payload == b.payload and a.chroma == b.chroma
        assert y4m.output_header(a, 2).encode() == y4m.output_header(b, 2).encode()
    with pytest.raises(y4m.Y4MError) as e:                                 # deep 4:2:0 keeps its own hint
        y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C420p10', layouts=y4m.LAYOUTS)
    assert '--high-depth' in str(e.value) and y4m.FIX in str(e.value)
    assert y4m.output_ctag(8) == '420jpeg' and y4m.output_ctag(12) == '420p12'
    with pytest.raises(ValueError):
        y4m.Header(64, 48, 25, layout='411')


# ---- stream I/O -----------------------------------------------------------------------------------------------------------------
def _stream(tag, n=3, h=5, w=7, seed=0):
    hdr = y4m.parse_header(b'YUV4MPEG2 W%d H%d F25:1 Ip C%s' % (w, h, tag.encode()), y4m.DEPTHS, y4m.LAYOUTS)
    g = np.random.RandomState(seed)
    header = hdr.encode()
    if hdr.depth == 8:
        pays = [g.randint(0, 256, hdr.samples).astype(np.uint8) for _ in range(n)]
    else:
        pays = [g.randint(0, hdr.peak + 1, hdr.samples).astype('<u2') for _ in range(n)]
    return header, pays, header + b''.join(b'FRAME\n' + p.tobytes() for p in pays)


@pytest.mark.parametrize('tag', ['422', '444p10'])
def test_reader_scan_frames_writer_round_trip(tag, tmp_path):
    header, pays, data = _stream(tag)
    kw = {'depths': y4m.DEPTHS, 'layouts': y4m.LAYOUTS}
    rd = y4m.Reader(io.BytesIO(data), **kw)
    hdr = rd.header
    assert hdr.payload == pays[0].nbytes and hdr.samples == pays[0].size
    buf = np.empty(hdr.payload, np.uint8)
    for p in pays:
        assert rd.read_into(buf)
        assert buf.tobytes() == p.tobytes()
    assert not rd.read_into(buf)
    with pytest.raises(ValueError):                                        # a 4:2:0-sized buffer is not this stream's payload
        y4m.Reader(io.BytesIO(data), **kw).read_into(np.empty(y4m.payload_bytes(hdr.h, hdr.w, hdr.depth), np.uint8))
    path = tmp_path / 'in.y4m'
    path.write_bytes(data)
    with open(path, 'rb') as f:
        with pytest.raises(y4m.Y4MError):
            y4m.scan(f)
        h2, hb, offs = y4m.scan(f, **kw)
        assert (h2.layout, h2.depth, hb, offs) == (hdr.layout, hdr.depth, len(header), [len(header) + 6 + i * (6 + hdr.payload) for i in range(3)])
        fr = y4m.Frames.from_file(f, offs, 0, 3, hdr.payload, pinned=False)
        for i, p in enumerate(pays):
            assert fr[i].numel() == hdr.payload and fr[i].numpy().tobytes() == p.tobytes()
    fr = y4m.Frames(y4m.Reader(io.BytesIO(data), **kw), pinned=False)
    assert fr.payload == hdr.payload and fr.has(2) and not fr.has(3)
    assert fr[1].numpy().tobytes() == pays[1].tobytes()
    out = io.BytesIO()
    wr = y4m.Writer(out, y4m.output_header(hdr, 1))
    wr.write(np.stack([p.view(np.uint8) for p in pays]))
    assert wr.frames == 3 and out.getvalue() == data


@pytest.mark.parametrize('tag', ['422', '444p10'])
def test_truncated_last_frame(tag, tmp_path):
    header, pays, data = _stream(tag)
    kw = {'depths': y4m.DEPTHS, 'layouts': y4m.LAYOUTS}
    cut = data[:-5]
    rd = y4m.Reader(io.BytesIO(cut), **kw)
    buf = np.empty(rd.header.payload, np.uint8)
    assert rd.read_into(buf) and rd.read_into(buf)
    with pytest.raises(y4m.Y4MError) as e:
        rd.read_into(buf)
    assert 'truncated frame 2 (%d of %d bytes)' % (rd.header.payload - 5, rd.header.payload) in str(e.value)
    path = tmp_path / 'cut.y4m'
    path.write_bytes(cut)
    with open(path, 'rb') as f, pytest.raises(y4m.Y4MError):
        y4m.scan(f, **kw)


# ---- exact anchors to the 4:2:0 definition ----------------------------------------------------------------------------------------
def _rand_pay(g, h, w, layout, d):
    return g.randint(0, (1 << d), y4m.payload_size(h, w, layout)).astype(np.uint16)


def _to_bgr(pay16, h, w, d, layout, matrix, full, siting='420jpeg'):
    """The definition at depth d; at 8 bits through the 8-bit function, checked against the 16-bit one."""
    got = y4m.yuv_to_bgr16_np(pay16, h, w, d, layout, matrix, full, siting)
    if d == 8:
        got8 = y4m.yuv_to_bgr_np(pay16.astype(np.uint8), h, w, layout, matrix, full, siting)
        assert got8.dtype == np.uint8 and np.array_equal(got8, got)
    return got


def _to_yuv(bgr16, d, layout, matrix, full):
    got = y4m.bgr16_to_yuv_np(bgr16, d, layout, matrix, full)
    assert got.dtype.itemsize == 2 and got.size == y4m.payload_size(bgr16.shape[0], bgr16.shape[1], layout)
    if d == 8:
        got8 = y4m.bgr_to_yuv_np(bgr16.astype(np.uint8), layout, matrix, full)
        assert got8.dtype == np.uint8 and np.array_equal(got8, got)
    return got


DEPTHS4 = (8, 10, 12, 16)


@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (37, 53), (64, 96)])
def test_layout_420_is_the_existing_pair(d, h, w):
    g = np.random.RandomState(d + h)
    pay, bgr = _rand_pay(g, h, w, '420', d), g.randint(0, 1 << d, (h, w, 3)).astype(np.uint16)
    for siting in y4m.SITINGS:
        assert np.array_equal(_to_bgr(pay, h, w, d, '420', 'bt709', False, siting), y4m.yuv420_to_bgr16_np(pay, h, w, d, 'bt709', False, siting))
    assert np.array_equal(_to_yuv(bgr, d, '420', 'bt601', True), y4m.bgr16_to_yuv420_np(bgr, d, 'bt601', True))


@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_mono_to_bgr_is_420_with_chroma_at_mid(d, matrix, full):
    g = np.random.RandomState(d)
    for h, w in ((2, 2), (3, 5), (37, 53)):
        y = _rand_pay(g, h, w, 'mono', d)
        c = np.full(2 * ((h + 1) // 2) * ((w + 1) // 2), 1 << (d - 1), np.uint16)
        got = _to_bgr(y, h, w, d, 'mono', matrix, full)
        for siting in y4m.SITINGS:
            assert np.array_equal(got, y4m.yuv420_to_bgr16_np(np.concatenate([y, c]), h, w, d, matrix, full, siting))
        if d == 8:
            assert np.array_equal(got, y4m.yuv420_to_bgr_np(np.concatenate([y, c]).astype(np.uint8), h, w, matrix, full))
        assert np.array_equal(got[:, :, 0], got[:, :, 1]) and np.array_equal(got[:, :, 1], got[:, :, 2])


@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_y_samples_of_every_layout_are_those_of_420(d, matrix, full):
    g = np.random.RandomState(d + 1)
    for h, w in ((2, 2), (5, 3), (37, 53)):
        bgr = g.randint(0, 1 << d, (h, w, 3)).astype(np.uint16)
        ref = y4m.bgr16_to_yuv420_np(bgr, d, matrix, full)[:h * w]
        if d == 8:
            assert np.array_equal(ref, y4m.bgr_to_yuv420_np(bgr.astype(np.uint8), matrix, full)[:h * w])
        for lay in NEW:
            assert np.array_equal(_to_yuv(bgr, d, lay, matrix, full)[:h * w], ref), lay


@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_422_with_columns_of_constant_chroma_is_420mpeg2(d, matrix, full):
    """Chroma constant down every column: the vertical 3/4 + 1/4 of 4:2:0 gives the sample back, so only the horizontal rule is
    left, and that of 4:2:2 is that of 420mpeg2."""
    g = np.random.RandomState(d + 2)
    for h, w in ((2, 2), (4, 5), (38, 53), (64, 96)):
        cw = (w + 1) // 2
        y = g.randint(0, 1 << d, h * w).astype(np.uint16)
        rows = [g.randint(0, 1 << d, cw).astype(np.uint16) for _ in range(2)]
        p422 = np.concatenate([y] + [np.tile(r, h) for r in rows])
        p420 = np.concatenate([y] + [np.tile(r, h // 2) for r in rows])
        assert np.array_equal(_to_bgr(p422, h, w, d, '422', matrix, full), y4m.yuv420_to_bgr16_np(p420, h, w, d, matrix, full, '420mpeg2'))


@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_444_with_constant_chroma_is_420_with_that_constant(d, matrix, full):
    g = np.random.RandomState(d + 3)
    for h, w in ((2, 2), (3, 5), (37, 53)):
        y = g.randint(0, 1 << d, h * w).astype(np.uint16)
        cb, cr = (int(v) for v in g.randint(0, 1 << d, 2))
        nc = ((h + 1) // 2) * ((w + 1) // 2)
        p444 = np.concatenate([y, np.full(h * w, cb, np.uint16), np.full(h * w, cr, np.uint16)])
        p420 = np.concatenate([y, np.full(nc, cb, np.uint16), np.full(nc, cr, np.uint16)])
        p422 = np.concatenate([y, np.full(h * ((w + 1) // 2), cb, np.uint16), np.full(h * ((w + 1) // 2), cr, np.uint16)])
        for siting in y4m.SITINGS:
            ref = y4m.yuv420_to_bgr16_np(p420, h, w, d, matrix, full, siting)
            assert np.array_equal(_to_bgr(p444, h, w, d, '444', matrix, full), ref)
            assert np.array_equal(_to_bgr(p422, h, w, d, '422', matrix, full), ref)


@pytest.mark.parametrize('d', DEPTHS4 + (14,))
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_grey_bgr_gives_chroma_at_mid_in_every_layout(d, matrix, full):
    g = np.random.RandomState(d + 4)
    for h, w in ((2, 2), (3, 5), (37, 53)):
        v = g.randint(0, 1 << d, (h, w, 1)).astype(np.uint16)
        v.reshape(-1)[:2] = [0, (1 << d) - 1]
        bgr = np.repeat(v, 3, axis=2)
        for lay in ('420', '422', '444'):
            pay = _to_yuv(bgr, d, lay, matrix, full)
            assert (pay[h * w:] == 1 << (d - 1)).all(), lay
        assert _to_yuv(bgr, d, 'mono', matrix, full).size == h * w


def test_definition_rejects_what_it_does_not_define():
    with pytest.raises(ValueError):
        y4m.yuv_to_bgr16_np(np.zeros(12, np.uint16), 2, 2, 10, '411')
    with pytest.raises(ValueError):
        y4m.yuv_to_bgr16_np(np.zeros(12, np.uint16), 2, 2, 9, '444')
    with pytest.raises(ValueError):
        y4m.yuv_to_bgr16_np(np.zeros(11, np.uint16), 2, 2, 10, '444')
    with pytest.raises(ValueError):
        y4m.yuv_to_bgr_np(np.zeros(8, np.uint16), 2, 2, '422')
    with pytest.raises(ValueError):
        y4m.bgr16_to_yuv_np(np.zeros((2, 2, 3), np.uint8), 10, '422')
    with pytest.raises(ValueError):
        y4m.bgr_to_yuv_np(np.zeros((2, 2, 3), np.uint16), 'mono')
    pay = np.arange(8, dtype='<u2')
    assert np.array_equal(y4m.yuv_to_bgr16_np(pay.tobytes(), 2, 2, 10, '422'), y4m.yuv_to_bgr16_np(pay, 2, 2, 10, '422'))


# ---- accuracy against float64 -----------------------------------------------------------------------------------------------------
def _ranges(d, full):
    s, peak = 1 << (d - 8), (1 << d) - 1
    return (0, 1.0, 1.0) if full else (16 * s, peak / (219.0 * s), peak / (224.0 * s))


def _up_f64(c, w, layout):
    c = c.astype(np.float64)
    if layout == '444':
        return c
    xs = np.arange(w)
    cx = xs >> 1
    nb = np.minimum(cx + 1, c.shape[1] - 1)
    return np.where(xs & 1, (c[:, cx] + c[:, nb]) / 2.0, c[:, cx])


def _to_bgr_f64(pay, h, w, d, layout, matrix, full):
    """The float64 matrix conversion of the layout's upsampled chroma, before rounding, clipped to the range."""
    y, cb, cr = y4m.split_planes_layout(pay, h, w, layout)
    kr, kb = y4m.MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, ys, cs = _ranges(d, full)
    mid = float(1 << (d - 1))
    Y = (y.astype(np.float64) - yoff) * ys
    if layout == 'mono':
        CB = CR = np.zeros((h, w))
    else:
        CB, CR = (_up_f64(cb, w, layout) - mid) * cs, (_up_f64(cr, w, layout) - mid) * cs
    r = Y + 2.0 * (1.0 - kr) * CR
    b = Y + 2.0 * (1.0 - kb) * CB
    g = Y - 2.0 * kb * (1.0 - kb) / kg * CB - 2.0 * kr * (1.0 - kr) / kg * CR
    return np.clip(np.stack([b, g, r], -1), 0.0, float((1 << d) - 1))


def _to_yuv_f64(bgr, d, layout, matrix, full):
    """The float64 matrix conversion and the layout's downsampling ([1,2,1]/4 with clamped edges for 4:2:2), before rounding."""
    h, w = bgr.shape[:2]
    kr, kb = y4m.MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, ys, cs = _ranges(d, full)
    b, g, r = (bgr[:, :, i].astype(np.float64) for i in range(3))
    yl = kr * r + kg * g + kb * b
    planes = [yoff + yl / ys]
    ci = np.arange(0, w, 2)

    def down(f):
        if layout == '444':
            return f
        return (f[:, np.maximum(ci - 1, 0)] + 2.0 * f[:, ci] + f[:, np.minimum(ci + 1, w - 1)]) / 4.0
    if layout != 'mono':
        mid = float(1 << (d - 1))
        planes += [mid + down((b - yl) / (2.0 * (1.0 - kb))) / cs, mid + down((r - yl) / (2.0 * (1.0 - kr))) / cs]
    return np.clip(np.concatenate([p.reshape(-1) for p in planes]), 0.0, float((1 << d) - 1))


def _corners(d):
    s = 1 << (d - 8)
    return np.array([0, 16 * s, 235 * s, 240 * s, 1 << (d - 1), (1 << d) - 1], np.uint16)


@pytest.mark.parametrize('layout', NEW)
@pytest.mark.parametrize('d', DEPTHS4)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_both_directions_within_the_derived_bound_of_float64(layout, d, matrix, full):
    peak = (1 << d) - 1
    g = np.random.RandomState(d)
    cor = _corners(d)
    worst = [0.0, 0.0]
    for h, w in ((37, 53), (64, 96)):
        P = y4m.payload_size(h, w, layout)
        for pay in (g.randint(0, peak + 1, P).astype(np.uint16), cor[g.randint(0, len(cor), P)]):
            got = _to_bgr(pay, h, w, d, layout, matrix, full)
            assert got.dtype == np.uint16 and got.max() <= peak
            worst[0] = max(worst[0], float(np.abs(got.astype(np.float64) - _to_bgr_f64(pay, h, w, d, layout, matrix, full)).max()))
        for bgr in (g.randint(0, peak + 1, (h, w, 3)).astype(np.uint16), cor[g.randint(0, len(cor), (h, w, 3))]):
            got = _to_yuv(bgr, d, layout, matrix, full)
            assert got.max() <= peak
            worst[1] = max(worst[1], float(np.abs(got.astype(np.float64) - _to_yuv_f64(bgr, d, layout, matrix, full)).max()))
    print('%s depth %d %s %s: max |definition - float64| = %.5f LSB to BGR, %.5f LSB to YUV (bound %.5f)'
          % (layout, d, matrix, 'full' if full else 'limited', worst[0], worst[1], BOUND))
    assert worst[0] <= BOUND and worst[1] <= BOUND, worst


# ---- scene-cut scores over a 4:4:4 payload ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [8, 10])
def test_scene_scores_over_a_444_payload(d):
    h, w = 6, 10
    hdr = y4m.parse_header(b'YUV4MPEG2 W%d H%d F25:1 Ip C%s' % (w, h, _tag('444', d).encode()), y4m.DEPTHS, y4m.LAYOUTS)
    P, peak = hdr.samples, hdr.peak
    assert P == 3 * h * w == y4m.payload_size(h, w, '444') and P != y4m.payload_size(h, w)
    g = np.random.RandomState(d)
    dt = np.uint8 if d == 8 else np.uint16
    a, b = g.randint(peak // 8, peak // 2, P), g.randint(peak // 2, peak, P)
    pays = [((a if i < 5 else b) + g.randint(-2, 3, P)).astype(dt) for i in range(10)]          # a hard cut before frame 5
    sads = [S.sad_np(pays[j], pays[j - 1]) for j in range(1, len(pays))]
    assert sads[4] == int(np.abs(pays[5].astype(np.int64) - pays[4].astype(np.int64)).sum())
    assert S.mafd(sads[4], P, peak) == 100.0 * sads[4] / (peak * P)
    assert S.cuts_of(sads, P, S.DEFAULT_THRESHOLD, peak=peak) == [5]
    det = S.Detector(P, S.DEFAULT_THRESHOLD, peak=peak)
    for j in range(1, len(pays)):
        det.push(j, sads[j - 1])
    assert det.cuts == [5]
    # scored with the 4:2:0 payload size the same SADs would be mis-scaled by 2: P is the layout's
    assert S.mafd(sads[4], y4m.payload_size(h, w), peak) == pytest.approx(2.0 * S.mafd(sads[4], P, peak))
