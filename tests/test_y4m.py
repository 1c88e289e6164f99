"""CPU tests of the Y4M stream edge: header parsing and rejections, the x M output header, stream order and per-rank byte
offsets, the numpy definition of the YUV 4:2:0 <-> BGR conversion (against the float64 textbook formulas and PIL, an
independent implementation) and the bounded read-ahead on a pipe."""
import io
import itertools

import numpy as np
import pytest

from demfi_amd import y4m
from demfi_amd.clip import deblurred_writes, output_names, window_list
from demfi_amd.dist import shard_windows


def _stream(hdr_line, payloads, frame_line=b'FRAME\n'):
    return io.BytesIO(hdr_line + b''.join(frame_line + bytes(p) for p in payloads))


# ---- header ----------------------------------------------------------------------------------------------------------------
def test_ffmpeg_header_parses_and_round_trips():
    line = b'YUV4MPEG2 W98 H70 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\n'
    h = y4m.parse_header(line)
    assert (h.w, h.h, h.fps, h.interlace, h.aspect, h.chroma, h.full_range) == (98, 70, y4m.Fraction(30000, 1001), 'p', '1:1',
                                                                                '420mpeg2', False)
    assert h.xtags == ['YSCSS=420MPEG2']
    assert h.payload == 98 * 70 + 2 * 35 * 49
    assert y4m.parse_header(h.encode()).encode() == h.encode()
    assert set(h.encode().split()) == set(line.split())


@pytest.mark.parametrize('c,siting', [(b'', '420jpeg'), (b' C420', '420jpeg'), (b' C420jpeg', '420jpeg'), (b' C420mpeg2', '420mpeg2')])
def test_accepted_chroma_and_odd_sizes(c, siting):
    h = y4m.parse_header(b'YUV4MPEG2 W5 H3 F25:1 I?' + c + b' XCOLORRANGE=FULL')
    assert (h.w, h.h, h.chroma, h.full_range, h.interlace) == (5, 3, siting, True, '?')
    assert h.payload == 15 + 2 * 2 * 3


@pytest.mark.parametrize('line', [
    b'YUV4MPEG2 W64 H48 F25:1 Ip C422',
    b'YUV4MPEG2 W64 H48 F25:1 Ip C444',
    b'YUV4MPEG2 W64 H48 F25:1 Ip Cmono',
    b'YUV4MPEG2 W64 H48 F25:1 Ip C420paldv',
    b'YUV4MPEG2 W64 H48 F25:1 Ip C420p10',
    b'YUV4MPEG2 W64 H48 F25:1 It C420jpeg',
    b'YUV4MPEG2 W64 H48 F25:1 Ib',
    b'YUV4MPEG2 W64 H48 F25:1 Im',
    b'YUV4MPEG2 W1 H48 F25:1',
    b'YUV4MPEG2 W64 H16385 F25:1',
    b'YUV4MPEG2 W64 F25:1',
    b'YUV4MPEG2 W64 H48 F25:0',
    b'YUV4MPEG2 W64 H48',
    b'YUV4MPEG2 W64 H48 F25:1 XCOLORRANGE=SOMETIMES',
    b'YUV4MPEG W64 H48 F25:1',
    b'\x89PNG\r\n\x1a\n',
])
def test_rejections(line):
    with pytest.raises(y4m.Y4MError):
        y4m.parse_header(line)


def test_rejection_names_the_ffmpeg_fix():
    with pytest.raises(y4m.Y4MError, match='-pix_fmt yuv420p'):
        y4m.parse_header(b'YUV4MPEG2 W64 H48 F25:1 Ip C422')


def test_reader_frames_params_and_truncation():
    hdr = b'YUV4MPEG2 W5 H3 F25:1 Ip\n'
    p = y4m.payload_size(3, 5)
    pay = [np.full(p, i, np.uint8) for i in range(3)]
    rd = y4m.Reader(_stream(hdr, pay, b'FRAME Ixyz XFOO=1\n'))
    buf = np.empty(p, np.uint8)
    for i in range(3):
        assert rd.read_into(buf) and (buf == i).all()
    assert not rd.read_into(buf)
    cut = io.BytesIO(hdr + b'FRAME\n' + bytes(p) + b'FRAME\n' + bytes(p - 1))
    rd = y4m.Reader(cut)
    assert rd.read_into(buf)
    with pytest.raises(y4m.Y4MError, match='truncated'):
        rd.read_into(buf)
    with pytest.raises(y4m.Y4MError, match='FRAME'):
        y4m.Reader(io.BytesIO(hdr + b'FRAMX\n' + bytes(p))).read_into(buf)


def test_scan_finds_offsets_and_rejects_a_truncated_file(tmp_path):
    hdr = b'YUV4MPEG2 W6 H4 F24:1 Ip\n'
    p = y4m.payload_size(4, 6)
    path = tmp_path / 'a.y4m'
    path.write_bytes(hdr + b'FRAME\n' + bytes(p) + b'FRAME Ix\n' + bytes(p))
    with open(path, 'rb') as f:
        h, hl, offs = y4m.scan(f)
    assert hl == len(hdr) and offs == [len(hdr) + 6, len(hdr) + 6 + p + 9]
    path.write_bytes(hdr + b'FRAME\n' + bytes(p) + b'FRAME\n' + bytes(p - 3))
    with open(path, 'rb') as f, pytest.raises(y4m.Y4MError, match='truncated'):
        y4m.scan(f)


# ---- output header, order, offsets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('fps,m,exp', [((30000, 1001), 8, (240000, 1001)), ((25, 1), 2, (50, 1)), ((24, 4), 8, (48, 1)),
                                       ((60000, 1001), 4, (240000, 1001))])
def test_output_header_rate(fps, m, exp):
    h = y4m.parse_header(b'YUV4MPEG2 W98 H70 F%d:%d I? A4:3 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL' % fps)
    o = y4m.output_header(h, m)
    assert o.encode() == b'YUV4MPEG2 W98 H70 F%d:%d Ip A4:3 C420jpeg XCOLORRANGE=FULL\n' % exp


@pytest.mark.parametrize('n,m', [(4, 8), (9, 8), (9, 2), (23, 4)])
def test_stream_order_is_the_sorted_reference_folder(n, m):
    names = ['%05d.png' % i for i in range(n)]
    onames = output_names(names, m)
    nw = len(window_list(n))
    order = [None] * y4m.n_output_frames(n, m)
    for k, (st, s0, s1) in enumerate(onames):
        w0, w1 = deblurred_writes(k, nw)
        assert w0
        order[y4m.output_index(k, 0, m)] = s0
        for j, nm in enumerate(st):
            order[y4m.output_index(k, 1 + j, m)] = nm
        if w1:
            order[y4m.output_index(k, m, m)] = s1
    assert None not in order
    assert order == sorted(order)
    assert len(order) == (n - 3) * m + 1


@pytest.mark.parametrize('n,m,world', [(9, 8, 2), (40, 2, 3), (7, 4, 8)])
def test_rank_offsets_tile_the_file(n, m, world):
    """Every rank's frames start at header + first*(6 + payload) and the ranks together cover (n-3)*M + 1 frames once."""
    p, hl = y4m.payload_size(70, 98), 57
    nw = n - 3
    spans = []
    for r in range(world):
        lo, hi = shard_windows(nw, world, r)
        if hi == lo:
            continue
        cnt = (hi - lo) * m + (1 if hi == nw else 0)
        spans.append((y4m.frame_offset(hl, y4m.output_index(lo, 0, m), p), cnt))
    pos = hl
    for off, cnt in spans:
        assert off == pos
        pos += cnt * (6 + p)
    assert pos == y4m.frame_offset(hl, y4m.n_output_frames(n, m), p) == hl + ((n - 3) * m + 1) * (6 + p)


# ---- the conversion definition ---------------------------------------------------------------------------------------------
def _float_yuv_to_rgb(y, cb, cr, matrix, full):
    kr, kb = y4m.MATRICES[matrix]
    kg = 1 - kr - kb
    if full:
        yy, u, v = y, cb - 128.0, cr - 128.0
    else:
        yy, u, v = (y - 16.0) * 255 / 219, (cb - 128.0) * 255 / 224, (cr - 128.0) * 255 / 224
    r = yy + 2 * (1 - kr) * v
    b = yy + 2 * (1 - kb) * u
    g = (yy - kr * r - kb * b) / kg
    return np.clip(np.round(np.stack([r, g, b], -1)), 0, 255)


def _float_rgb_to_yuv(rgb, matrix, full):
    kr, kb = y4m.MATRICES[matrix]
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    yp = kr * r + (1 - kr - kb) * g + kb * b
    u, v = (b - yp) / (2 * (1 - kb)), (r - yp) / (2 * (1 - kr))
    if full:
        return np.clip(np.round(np.stack([yp, u + 128, v + 128], -1)), 0, 255)
    return np.clip(np.round(np.stack([16 + yp * 219 / 255, 128 + u * 224 / 255, 128 + v * 224 / 255], -1)), 0, 255)


CASES = list(itertools.product(['bt601', 'bt709'], [False, True]))


@pytest.mark.parametrize('matrix,full', CASES)
@pytest.mark.parametrize('siting', y4m.SITINGS)
def test_yuv_to_bgr_within_1_of_float64_on_uniform_chroma_blocks(matrix, full, siting):
    """Every luma value against a grid of chroma values, one uniform chroma value per 2x2 block (uniform over the whole frame, so
    the upsampling filter sees the same value everywhere and only the matrix is tested)."""
    g = np.random.RandomState(1)
    for cb, cr in [(128, 128), (16, 240), (240, 16), (0, 255), (255, 0), (90, 170)] + [tuple(g.randint(0, 256, 2)) for _ in range(10)]:
        h, w = 16, 16
        yv = np.arange(256, dtype=np.uint8).reshape(h, w)
        pay = np.concatenate([yv.reshape(-1), np.full(64, cb, np.uint8), np.full(64, cr, np.uint8)])
        bgr = y4m.yuv420_to_bgr_np(pay, h, w, matrix, full, siting).astype(np.int32)
        ref = _float_yuv_to_rgb(yv.astype(np.float64), float(cb), float(cr), matrix, full)[..., ::-1]
        assert np.abs(bgr - ref).max() <= 1, (cb, cr)


@pytest.mark.parametrize('matrix,full', CASES)
def test_bgr_to_yuv_within_1_of_float64_on_uniform_2x2_blocks(matrix, full):
    g = np.random.RandomState(2)
    hb, wb = 13, 17
    rgb = g.randint(0, 256, (hb, wb, 3)).astype(np.uint8)
    rgb[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    big = np.repeat(np.repeat(rgb, 2, 0), 2, 1)[:2 * hb - 1, :2 * wb - 1]        # odd size: the edge blocks are 2x1 / 1x2 / 1x1
    h, w = big.shape[:2]
    y, cb, cr = y4m.split_planes(y4m.bgr_to_yuv420_np(big[..., ::-1], matrix, full), h, w)
    ref = _float_rgb_to_yuv(rgb, matrix, full)
    assert np.abs(y.astype(np.int32) - np.repeat(np.repeat(ref[..., 0], 2, 0), 2, 1)[:h, :w]).max() <= 1
    assert np.abs(cb.astype(np.int32) - ref[..., 1]).max() <= 1
    assert np.abs(cr.astype(np.int32) - ref[..., 2]).max() <= 1


def test_full_range_bt601_matches_pil():
    """PIL's YCbCr is full-range BT.601 (JPEG): 4:4:4 content -- uniform 2x2 blocks for BGR -> YUV, uniform chroma for
    YUV -> BGR -- agrees within 1."""
    Image = pytest.importorskip('PIL.Image')
    g = np.random.RandomState(4)
    rgb = g.randint(0, 256, (20, 24, 3)).astype(np.uint8)
    big = np.repeat(np.repeat(rgb, 2, 0), 2, 1)
    pil = np.asarray(Image.fromarray(big, 'RGB').convert('YCbCr')).astype(np.int32)
    h, w = big.shape[:2]
    y, cb, cr = y4m.split_planes(y4m.bgr_to_yuv420_np(big[..., ::-1], 'bt601', True), h, w)
    assert np.abs(y.astype(np.int32) - pil[..., 0]).max() <= 1
    assert np.abs(cb.astype(np.int32) - pil[::2, ::2, 1]).max() <= 1
    assert np.abs(cr.astype(np.int32) - pil[::2, ::2, 2]).max() <= 1
    for cbv, crv in [(128, 128), (30, 200), (220, 60), (0, 255)]:
        yv = g.randint(0, 256, (16, 16)).astype(np.uint8)
        ycc = np.stack([yv, np.full_like(yv, cbv), np.full_like(yv, crv)], -1)
        ref = np.asarray(Image.fromarray(ycc, 'YCbCr').convert('RGB')).astype(np.int32)
        pay = np.concatenate([yv.reshape(-1), np.full(64, cbv, np.uint8), np.full(64, crv, np.uint8)])
        bgr = y4m.yuv420_to_bgr_np(pay, 16, 16, 'bt601', True).astype(np.int32)
        assert np.abs(bgr[..., ::-1] - ref).max() <= 1


@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (7, 9), (70, 98)])
def test_round_trip_of_smooth_content_and_odd_sizes(h, w):
    """YUV -> BGR -> YUV of slowly varying content returns close to the input at every size, odd ones included."""
    yy, xx = np.mgrid[0:h, 0:w]
    bgr = np.stack([40 + 3 * xx % 160, 60 + 2 * yy % 150, 90 + (xx + yy) % 120], -1).astype(np.uint8)
    pay = y4m.bgr_to_yuv420_np(bgr, 'bt709', False)
    assert pay.size == y4m.payload_size(h, w)
    back = y4m.bgr_to_yuv420_np(y4m.yuv420_to_bgr_np(pay, h, w, 'bt709', False, '420jpeg'), 'bt709', False)
    assert np.abs(back[:h * w].astype(np.int32) - pay[:h * w]).max() <= 3


def test_auto_matrix():
    assert y4m.auto_matrix(720) == 'bt709' and y4m.auto_matrix(576) == 'bt601' and y4m.auto_matrix(1080) == 'bt709'


# ---- streaming ---------------------------------------------------------------------------------------------------------------
class _Pipe(io.RawIOBase):
    """A non-seekable stream that hands out at most 1000 bytes per read (what a pipe does)."""

    def __init__(self, data):
        self.data, self.pos, self.max_read = data, 0, 0

    def readable(self):
        return True

    def readinto(self, b):
        k = min(len(b), 1000, len(self.data) - self.pos)
        b[:k] = self.data[self.pos:self.pos + k]
        self.pos += k
        self.max_read = max(self.max_read, self.pos)
        return k


@pytest.mark.parametrize('batch', [1, 4])
def test_pipe_read_ahead_is_bounded_by_the_batch(batch):
    """The runner's access pattern (pull a batch of windows, then fetch their frames) over a 60-frame pipe: every frame is
    delivered intact, at most batch + 5 are held, and the stream is read no further than the windows need."""
    h, w, n = 6, 10, 60
    p = y4m.payload_size(h, w)
    data = b'YUV4MPEG2 W10 H6 F25:1 Ip\n' + b''.join(b'FRAME\n' + bytes([i]) * p for i in range(n))
    pipe = _Pipe(data)
    fr = y4m.Frames(y4m.Reader(io.BufferedReader(pipe, 64)), pinned=False)
    it = fr.windows()
    seen = []
    while True:
        wins = list(itertools.islice(it, batch))
        if not wins:
            break
        for win in wins:
            for i in win:
                assert (fr[i].numpy() == i).all()
        seen += wins
        assert len(fr.buf) <= batch + 5
    assert seen == window_list(n)
    assert fr.peak <= batch + 5
    assert fr.is_last(n - 4) and not fr.is_last(n - 5)


def test_stream_windows_know_the_last_one_before_it_is_handed_out():
    p = y4m.payload_size(4, 4)
    fr = y4m.Frames(y4m.Reader(_stream(b'YUV4MPEG2 W4 H4 F25:1\n', [bytes(p)] * 6)), pinned=False)
    flags = [(k, fr.is_last(k)) for k, _ in enumerate(fr.windows())]
    assert flags == [(0, False), (1, False), (2, True)]
    few = y4m.Frames(y4m.Reader(_stream(b'YUV4MPEG2 W4 H4 F25:1\n', [bytes(p)] * 3)), pinned=False)
    assert list(few.windows()) == []
