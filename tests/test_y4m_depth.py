"""10- to 16-bit 4:2:0 Y4M (C420p10 .. C420p16): the opt-in of the parser, byte payloads through Reader / scan / Frames / Writer,
the conversion definition at depth d (its d = 8 instance IS the 8-bit pair; within 0.5 + 3 * 2^-9 LSB of a float64 matrix
conversion in both directions; grey stays grey exactly) and the scene-cut scores over samples with ``peak``.

The bound 0.5 + 3 * 2^-9 LSB follows from the form of the definition: ONE rounding of the result (0.5) plus at most three
coefficient errors, each at most 2^-(9+d) (Q(8+d), rounded half up) on an operand below 2^d."""
import io

import numpy as np
import pytest

from demfi_amd import retime as R
from demfi_amd import scene as S
from demfi_amd import y4m

HIGH = (10, 12, 14, 16)
BOUND = 0.5 + 3 * 2.0 ** -9


# ---- header, payload bytes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', HIGH)
def test_header_round_trip_and_byte_payloads(d):
    line = b'YUV4MPEG2 W37 H53 F30000:1001 Ip A1:1 C420p%d XCOLORRANGE=FULL\n' % d
    hdr = y4m.parse_header(line, depths=y4m.DEPTHS)
    assert (hdr.w, hdr.h, hdr.depth, hdr.chroma, hdr.ctag, hdr.full_range, hdr.peak) == (37, 53, d, '420jpeg', '420p%d' % d, True, (1 << d) - 1)
    assert hdr.payload == 2 * y4m.payload_size(53, 37) == y4m.payload_bytes(53, 37, d)
    assert hdr.frame_bytes == 6 + hdr.payload
    assert hdr.encode() == line
    again = y4m.parse_header(hdr.encode(), depths=y4m.DEPTHS)
    assert (again.depth, again.payload, again.encode()) == (d, hdr.payload, line)
    for out in (y4m.output_header(hdr, 4), R.output_header(hdr, hdr.fps * 4)):
        assert (out.depth, out.ctag, out.chroma, out.payload, out.color_range) == (d, '420p%d' % d, '420jpeg', hdr.payload, 'FULL')
        assert out.fps == hdr.fps * 4 and b' C420p%d ' % d in out.encode()
    assert R.block_offset(40, 2, 4, hdr.payload) == y4m.frame_offset(40, 8, hdr.payload) == 40 + 8 * (6 + hdr.payload)


def test_eight_bit_headers_are_as_before():
    hdr = y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C420mpeg2', depths=y4m.DEPTHS)
    assert (hdr.depth, hdr.payload, hdr.chroma) == (8, y4m.payload_size(48, 64), '420mpeg2')
    assert y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1').depth == 8
    assert y4m.output_header(hdr, 2).encode() == b'YUV4MPEG2 W64 H48 F50:1 Ip C420jpeg\n'
    with pytest.raises(ValueError):
        y4m.Header(64, 48, 25, depth=9)


@pytest.mark.parametrize('d', HIGH)
def test_rejected_without_the_opt_in(d):
    for kw in ({}, {'depths': (8,)}):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C420p%d' % d, **kw)
        assert '-pix_fmt yuv420p' in str(e.value) and '--high-depth' in str(e.value) and y4m.FIX in str(e.value)
    with pytest.raises(y4m.Y4MError):
        y4m.Reader(io.BytesIO(b'YUV4MPEG2 W64 H48 F25:1 Ip C420p%d\n' % d))


@pytest.mark.parametrize('tag', ['420p9', '422p10', '444p10', 'mono16', '420p11', '420p10le', '422', 'mono'])
def test_other_tags_are_rejected_in_both_modes(tag):
    for kw in ({}, {'depths': y4m.DEPTHS}):
        with pytest.raises(y4m.Y4MError) as e:
            y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C' + tag.encode(), **kw)
        assert y4m.FIX in str(e.value)


# ---- stream I/O ------------------------------------------------------------------------------------------------------------
def _stream10(n=3, h=6, w=10, seed=0):
    g = np.random.RandomState(seed)
    header = b'YUV4MPEG2 W%d H%d F25:1 Ip C420p10\n' % (w, h)
    pays = [g.randint(0, 1024, y4m.payload_size(h, w)).astype('<u2') for _ in range(n)]
    return header, pays, header + b''.join(b'FRAME\n' + p.tobytes() for p in pays)


def test_reader_scan_frames_writer_round_trip(tmp_path):
    header, pays, data = _stream10()
    rd = y4m.Reader(io.BytesIO(data), depths=y4m.DEPTHS)
    hdr = rd.header
    assert hdr.depth == 10 and hdr.payload == 2 * pays[0].size
    buf = np.empty(hdr.payload, np.uint8)
    for p in pays:
        assert rd.read_into(buf)
        assert np.array_equal(y4m.as_samples16(buf), p)
    assert not rd.read_into(buf)
    with pytest.raises(ValueError):
        y4m.Reader(io.BytesIO(data), depths=y4m.DEPTHS).read_into(np.empty(hdr.payload // 2, np.uint8))     # a buffer of samples, not bytes

    path = tmp_path / 'in.y4m'
    path.write_bytes(data)
    with open(path, 'rb') as f:
        with pytest.raises(y4m.Y4MError):
            y4m.scan(f)
        h2, hb, offs = y4m.scan(f, depths=y4m.DEPTHS)
        assert (h2.depth, hb, offs) == (10, len(header), [len(header) + 6 + i * (6 + hdr.payload) for i in range(3)])
        fr = y4m.Frames.from_file(f, offs, 0, 3, hdr.payload, pinned=False)
        for i, p in enumerate(pays):
            assert fr[i].dtype.itemsize == 1 and fr[i].numel() == hdr.payload
            assert np.array_equal(y4m.as_samples16(fr[i].numpy()), p)
    fr = y4m.Frames(y4m.Reader(io.BytesIO(data), depths=y4m.DEPTHS), pinned=False)
    assert fr.payload == hdr.payload and fr.has(2) and not fr.has(3)
    assert np.array_equal(y4m.as_samples16(fr[1].numpy()), pays[1])

    out = io.BytesIO()
    wr = y4m.Writer(out, y4m.output_header(hdr, 1))
    wr.write(np.stack([p.view(np.uint8) for p in pays]))
    assert wr.frames == 3 and out.getvalue() == data
    out = io.BytesIO()
    y4m.Writer(out, y4m.output_header(hdr, 1)).write(np.stack(pays))                 # uint16 rows: written as they lie in memory
    assert out.getvalue() == data


def test_truncated_last_frame(tmp_path):
    header, pays, data = _stream10()
    cut = data[:-5]
    rd = y4m.Reader(io.BytesIO(cut), depths=y4m.DEPTHS)
    buf = np.empty(rd.header.payload, np.uint8)
    assert rd.read_into(buf) and rd.read_into(buf)
    with pytest.raises(y4m.Y4MError) as e:
        rd.read_into(buf)
    assert 'truncated frame 2 (%d of %d bytes)' % (rd.header.payload - 5, rd.header.payload) in str(e.value)
    path = tmp_path / 'cut.y4m'
    path.write_bytes(cut)
    with open(path, 'rb') as f, pytest.raises(y4m.Y4MError):
        y4m.scan(f, depths=y4m.DEPTHS)
    # a stream cut to the length its frames would have at 8 bits is truncated too: the payload counts bytes
    half = header + b''.join(b'FRAME\n' + p.tobytes()[:p.size] for p in pays)
    rd = y4m.Reader(io.BytesIO(half), depths=y4m.DEPTHS)
    with pytest.raises(y4m.Y4MError):
        while rd.read_into(buf):
            pass


# ---- the definition --------------------------------------------------------------------------------------------------------
SIZES = [(2, 2), (3, 5), (37, 53), (64, 96)]
CONFIGS = [(m, f) for m in ('bt601', 'bt709') for f in (False, True)]


@pytest.mark.parametrize('h,w', SIZES)
def test_depth_8_is_the_8_bit_pair(h, w):
    g = np.random.RandomState(h * 131 + w)
    for matrix, full in CONFIGS:
        pay = g.randint(0, 256, y4m.payload_size(h, w)).astype(np.uint8)
        for siting in y4m.SITINGS:
            got = y4m.yuv420_to_bgr16_np(pay.astype(np.uint16), h, w, 8, matrix, full, siting)
            assert got.dtype == np.uint16
            assert np.array_equal(got, y4m.yuv420_to_bgr_np(pay, h, w, matrix, full, siting)), (matrix, full, siting)
        bgr = g.randint(0, 256, (h, w, 3)).astype(np.uint8)
        got = y4m.bgr16_to_yuv420_np(bgr.astype(np.uint16), 8, matrix, full)
        assert got.dtype.itemsize == 2
        assert np.array_equal(got, y4m.bgr_to_yuv420_np(bgr, matrix, full)), (matrix, full)
        assert y4m.to_bgr_coefs_depth(matrix, full, 8) == y4m.to_bgr_coefs(matrix, full)
        assert y4m.to_yuv_coefs_depth(matrix, full, 8) == y4m.to_yuv_coefs(matrix, full)


def _ranges(d, full):
    """(Y offset, luma scale, chroma scale) of YUV -> RGB at depth d in float64."""
    s, peak = 1 << (d - 8), (1 << d) - 1
    return (0, 1.0, 1.0) if full else (16 * s, peak / (219.0 * s), peak / (224.0 * s))


def _to_bgr_f64(pay, h, w, d, matrix, full, siting):
    """The float64 matrix conversion of the same upsampled chroma, before rounding (clipped to the range like the definition)."""
    y, cb, cr = y4m.split_planes16(pay, h, w)
    kr, kb = y4m.MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, ys, cs = _ranges(d, full)
    mid = float(1 << (d - 1))
    Y = (y.astype(np.float64) - yoff) * ys
    CB = (y4m._upsample16(cb, h, w, siting) / 16.0 - mid) * cs
    CR = (y4m._upsample16(cr, h, w, siting) / 16.0 - mid) * cs
    r = Y + 2.0 * (1.0 - kr) * CR
    b = Y + 2.0 * (1.0 - kb) * CB
    g = Y - 2.0 * kb * (1.0 - kb) / kg * CB - 2.0 * kr * (1.0 - kr) / kg * CR
    return np.clip(np.stack([b, g, r], -1), 0.0, float((1 << d) - 1))


def _to_yuv_f64(bgr, d, matrix, full):
    """The float64 matrix conversion and 2x2 box (edges repeat the pixels that exist), before rounding, clipped to the range."""
    h, w = bgr.shape[:2]
    kr, kb = y4m.MATRICES[matrix]
    kg = 1.0 - kr - kb
    yoff, ys, cs = _ranges(d, full)
    b, g, r = (bgr[:, :, i].astype(np.float64) for i in range(3))
    yl = kr * r + kg * g + kb * b
    y = yoff + yl / ys
    r0 = np.arange(0, h, 2)
    r1 = np.minimum(r0 + 1, h - 1)
    c0 = np.arange(0, w, 2)
    c1 = np.minimum(c0 + 1, w - 1)

    def box(f):
        return (f[r0][:, c0] + f[r0][:, c1] + f[r1][:, c0] + f[r1][:, c1]) / 4.0
    mid = float(1 << (d - 1))
    cb = mid + box((b - yl) / (2.0 * (1.0 - kb))) / cs
    cr = mid + box((r - yl) / (2.0 * (1.0 - kr))) / cs
    return np.clip(np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)]), 0.0, float((1 << d) - 1))


def _corners(d):
    s = 1 << (d - 8)
    return np.array([0, 16 * s, 235 * s, 240 * s, 1 << (d - 1), (1 << d) - 1], np.uint16)


@pytest.mark.parametrize('d', HIGH)
@pytest.mark.parametrize('matrix,full', CONFIGS)
def test_both_directions_within_the_derived_bound_of_float64(d, matrix, full):
    peak = (1 << d) - 1
    g = np.random.RandomState(d)
    worst = [0.0, 0.0]
    for h, w in ((37, 53), (64, 96)):
        P = y4m.payload_size(h, w)
        cor = _corners(d)
        pays = [g.randint(0, peak + 1, P).astype(np.uint16), cor[g.randint(0, len(cor), P)]]
        # every triple of corner values as a flat frame (flat chroma upsamples to itself)
        tri = np.array([(a, b, c) for a in cor for b in cor for c in cor], np.uint16)
        for siting in y4m.SITINGS:
            for pay in pays:
                got = y4m.yuv420_to_bgr16_np(pay, h, w, d, matrix, full, siting)
                assert got.dtype == np.uint16 and got.max() <= peak
                worst[0] = max(worst[0], float(np.abs(got.astype(np.float64) - _to_bgr_f64(pay, h, w, d, matrix, full, siting)).max()))
            for yv, cbv, crv in tri:
                pay = np.concatenate([np.full(4, yv), [cbv], [crv]]).astype(np.uint16)
                got = y4m.yuv420_to_bgr16_np(pay, 2, 2, d, matrix, full, siting)
                worst[0] = max(worst[0], float(np.abs(got.astype(np.float64) - _to_bgr_f64(pay, 2, 2, d, matrix, full, siting)).max()))
        frames = [g.randint(0, peak + 1, (h, w, 3)).astype(np.uint16), cor[g.randint(0, len(cor), (h, w, 3))]]
        frames += [np.broadcast_to(t, (2, 2, 3)).copy() for t in tri]
        for bgr in frames:
            got = y4m.bgr16_to_yuv420_np(bgr, d, matrix, full)
            assert got.max() <= peak
            worst[1] = max(worst[1], float(np.abs(got.astype(np.float64) - _to_yuv_f64(bgr, d, matrix, full)).max()))
    print('depth %d %s %s: max |definition - float64| = %.5f LSB to BGR, %.5f LSB to YUV (bound %.5f)'
          % (d, matrix, 'full' if full else 'limited', worst[0], worst[1], BOUND))
    assert worst[0] <= BOUND and worst[1] <= BOUND, worst


@pytest.mark.parametrize('d', HIGH)
@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_grey_in_grey_out_exactly(d, matrix):
    s, mid = 1 << (d - 8), 1 << (d - 1)
    ks = np.arange(16 * s, 235 * s + 1, dtype=np.uint16)                  # every limited-range luma code k ...
    row = np.concatenate([ks, ks[-1:]]) if ks.size % 2 else ks
    h, w = 2, row.size
    y = np.stack([row, row[::-1]])                                        # ... next to every other one, over flat centred chroma
    pay = np.concatenate([y.reshape(-1), np.full(2 * (w // 2), mid, np.uint16)]).astype(np.uint16)
    for siting in y4m.SITINGS:
        bgr = y4m.yuv420_to_bgr16_np(pay, h, w, d, matrix, False, siting)
        assert np.array_equal(bgr[:, :, 0], bgr[:, :, 1]) and np.array_equal(bgr[:, :, 1], bgr[:, :, 2])
        assert bgr[y == 16 * s].max() == 0 and bgr[y == 235 * s].min() == (1 << d) - 1
        back = y4m.bgr16_to_yuv420_np(bgr, d, matrix, False)
        assert np.array_equal(back, pay)


def test_definition_rejects_what_it_does_not_define():
    with pytest.raises(ValueError):
        y4m.yuv420_to_bgr16_np(np.zeros(6, np.uint16), 2, 2, 9)
    with pytest.raises(ValueError):
        y4m.yuv420_to_bgr16_np(np.zeros(5, np.uint16), 2, 2, 10)
    with pytest.raises(ValueError):
        y4m.bgr16_to_yuv420_np(np.zeros((2, 2, 3), np.uint8), 10)
    with pytest.raises(ValueError):
        y4m.bgr16_to_yuv420_np(np.zeros((2, 2, 3), np.uint16), 17)
    pay = np.arange(6, dtype='<u2')
    assert np.array_equal(y4m.yuv420_to_bgr16_np(pay.tobytes(), 2, 2, 10), y4m.yuv420_to_bgr16_np(pay, 2, 2, 10))
    assert np.array_equal(y4m.yuv420_to_bgr16_np(pay.view(np.uint8), 2, 2, 10), y4m.yuv420_to_bgr16_np(pay, 2, 2, 10))


# ---- scene-cut scores over samples -----------------------------------------------------------------------------------------
def _scene_stream(n=12, P=600, seed=1):
    """8-bit payloads: slow drift, a hard cut before frame 5, a flash at frame 9."""
    g = np.random.RandomState(seed)
    a, b = g.randint(40, 200, P), g.randint(40, 200, P)
    out = []
    for i in range(n):
        base = a if i < 5 else b
        f = base + g.randint(-2, 3, P) + (50 if i == 9 else 0)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def test_scores_and_cuts_at_16_bits_equal_the_8_bit_stream():
    p8 = _scene_stream()
    p16 = [p.astype(np.uint16) * 257 for p in p8]                          # 65535 = 257 * 255: the scaling is exact
    P = p8[0].size
    s8 = [S.sad_np(p8[j], p8[j - 1]) for j in range(1, len(p8))]
    s16 = [S.sad_np(p16[j], p16[j - 1]) for j in range(1, len(p16))]
    assert s16 == [257 * s for s in s8]
    assert [S.mafd(s, P, 65535) for s in s16] == [S.mafd(s, P) for s in s8]
    assert S.scores(s16, P, 65535) == S.scores(s8, P)
    for thr in (5.0, 10.0, 20.0):
        cuts = S.cuts_of(s8, P, thr)
        assert S.cuts_of(s16, P, thr, 65535) == cuts
        d8, d16 = S.Detector(P, thr), S.Detector(P, thr, peak=65535)
        for j in range(1, len(p8)):
            d8.push(j, s8[j - 1])
            d16.push(j, s16[j - 1])
        assert d16.cuts == d8.cuts == cuts
    assert 5 in S.cuts_of(s8, P, 10.0)
    # a rank that starts later (first > 0) decides the same cuts from frame first + 2 on
    late = S.Detector(P, 10.0, first=3, peak=65535)
    for j in range(4, len(p16)):
        late.push(j, s16[j - 1])
    assert late.cuts == [j for j in S.cuts_of(s8, P, 10.0) if j >= 5]


@pytest.mark.parametrize('d', [10, 12, 14])
def test_score_formula_over_samples(d):
    peak = (1 << d) - 1
    g = np.random.RandomState(d)
    P = 777
    a, b = g.randint(0, peak + 1, P).astype(np.uint16), g.randint(0, peak + 1, P).astype(np.uint16)
    sad = S.sad_np(a, b)
    assert sad == int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum()) == S.sad_np(b, a)
    assert S.mafd(sad, P, peak) == 100.0 * sad / (peak * P)
    assert S.sad_np(np.full(P, peak, np.uint16), np.zeros(P, np.uint16)) == peak * P          # no int16 wrap
    assert S.mafd(peak * P, P, peak) == 100.0
    det = S.Detector(P, 10.0, peak=peak)
    det.push(1, sad)
    assert det.prev == 100.0 * sad / (peak * P)
    with pytest.raises(ValueError):
        S.sad_np(a, b[:-1])
