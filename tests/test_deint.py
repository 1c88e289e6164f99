"""Interlaced Y4M input (``--deinterlace``) without a GPU: the definition of the bob (``deint.bob_plane_np`` against a per-pixel scalar
loop written here, and the properties that pin down what the directional search does), ``bob_payload_np`` over every layout and
depth, the header (``It`` / ``Ib`` / ``Im``), the field timeline of ``y4m.Frames(fields=2)`` and the argument checks of
``VideoRunner(deinterlace=True)``."""
import io
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import deint as I
from demfi_amd import video, y4m


# ---- the definition, again, one sample at a time --------------------------------------------------------------------------------
def _bob_scalar(plane, q):
    rows, cols = plane.shape
    out = [[int(v) for v in row] for row in plane]
    if rows == 1 and q == 1:
        return np.array(out, plane.dtype)

    def cl(x):
        return min(max(x, 0), cols - 1)
    for y in range(rows):
        if y % 2 == q:
            continue
        if y - 1 < 0 or y + 1 >= rows:
            src = y + 1 if y - 1 < 0 else y - 1
            out[y] = [int(v) for v in plane[src]]
            continue
        a, b = [int(v) for v in plane[y - 1]], [int(v) for v in plane[y + 1]]
        for x in range(cols):
            def score(j):
                return sum(abs(a[cl(x + k + j)] - b[cl(x + k - j)]) for k in (-1, 0, 1))

            def pred(j):
                return (a[cl(x + j)] + b[cl(x - j)] + 1) >> 1
            best, o = score(0) - 1, pred(0)
            if score(-1) < best:
                best, o = score(-1), pred(-1)
                if score(-2) < best:
                    best, o = score(-2), pred(-2)
            if score(1) < best:
                best, o = score(1), pred(1)
                if score(2) < best:
                    best, o = score(2), pred(2)
            out[y][x] = o
    return np.array(out, plane.dtype)


def _planes(rows, cols, bits, seed):
    """Noise, a smooth-plus-edges picture (where directions other than 0 win) and the extremes 0 / peak."""
    dt, peak = (np.uint8, 255) if bits == 8 else (np.uint16, (1 << bits) - 1)
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    edges = np.where((xx + yy) % 7 < 3, peak, 0) ^ np.where((2 * xx - yy) % 11 < 4, peak // 3, 0)
    ends = g.choice([0, peak], (rows, cols))
    return [g.randint(0, peak + 1, (rows, cols)).astype(dt), edges.astype(dt), ends.astype(dt),
            np.zeros((rows, cols), dt), np.full((rows, cols), peak, dt)]


@pytest.mark.parametrize('bits', [8, 16])
@pytest.mark.parametrize('q', [0, 1])
@pytest.mark.parametrize('rows,cols', [(1, 1), (1, 5), (2, 2), (3, 2), (2, 7), (5, 9), (33, 47)])
def test_bob_plane_equals_the_scalar_loop(rows, cols, q, bits):
    took_a_direction = False
    for p in _planes(rows, cols, bits, rows * 100 + cols + q):
        before = p.copy()
        got = I.bob_plane_np(p, q)
        exp = _bob_scalar(p, q)
        assert got.dtype == p.dtype and got.shape == p.shape and np.array_equal(p, before)
        assert np.array_equal(got, exp)
        if rows > q:
            assert np.array_equal(got[q::2], p[q::2])                     # kept rows bit-identical
        if rows >= 3:
            ys = [y for y in range(1 - q, rows, 2) if 1 <= y < rows - 1]
            va = ((p[[y - 1 for y in ys]].astype(np.int64) + p[[y + 1 for y in ys]] + 1) >> 1)
            took_a_direction |= bool((got[ys] != va).any())
    if (rows, cols) == (33, 47):
        assert took_a_direction                                           # the planes exercise the search, not only pred(0)


def test_a_plane_linear_in_y_is_reproduced():
    for q in (0, 1):
        p = (np.arange(12, dtype=np.int64)[:, None] * 7 + 3 + np.zeros((1, 20), np.int64)).astype(np.uint8)
        got = I.bob_plane_np(p, q)
        ys = [y for y in range(1 - q, 12, 2) if 1 <= y < 11]
        assert np.array_equal(got[ys], p[ys])
        p16 = (np.arange(9, dtype=np.int64)[:, None] * 5000 + 11 + np.zeros((1, 5), np.int64)).astype(np.uint16)
        got = I.bob_plane_np(p16, q)
        ys = [y for y in range(1 - q, 9, 2) if 1 <= y < 8]
        assert np.array_equal(got[ys], p16[ys])


@pytest.mark.parametrize('slope', [1, -1])
def test_a_diagonal_step_edge_is_reproduced_where_the_vertical_average_is_not(slope):
    """A step edge that moves one sample per row: plane[y, x] = 200 where x >= c + slope * y, else 20.  Between rows y-1 and y+1 the
    vertical average blurs the two samples next to the edge to 110; the search follows the edge (for slope +1 the line through
    a[x-1] and b[x+1], j = -1) and gives the row of the progressive plane exactly."""
    rows, cols = 12, 32
    yy, xx = np.mgrid[0:rows, 0:cols]
    c = 10 if slope > 0 else 21
    p = np.where(xx >= c + slope * yy, 200, 20).astype(np.uint8)
    for q in (0, 1):
        got = I.bob_plane_np(p, q)
        ys = [y for y in range(1 - q, rows, 2) if 1 <= y < rows - 1]
        assert np.array_equal(got[ys], p[ys])
        va = ((p[[y - 1 for y in ys]].astype(np.int64) + p[[y + 1 for y in ys]] + 1) >> 1)
        assert (va != p[ys]).any(axis=1).all()                            # every such row: the plain average misses the edge
    # the direction: at the sample just right of the edge in row y the winner is j = -slope
    y, x = 5, c + slope * 5
    a, b = p[y - 1].astype(int), p[y + 1].astype(int)

    def score(j):
        return sum(abs(a[x + k + j] - b[x + k - j]) for k in (-1, 0, 1))
    assert score(-slope) == 0 and score(0) > 1 and score(slope) > score(0)


def test_single_neighbour_rows_copy_and_a_one_row_plane_stays():
    g = np.random.RandomState(3)
    p = g.randint(0, 256, (6, 9)).astype(np.uint8)
    assert np.array_equal(I.bob_plane_np(p, 1)[0], p[1])                   # the top row is missing: below only
    assert np.array_equal(I.bob_plane_np(p, 0)[5], p[4])                   # the bottom row is missing: above only
    p5 = p[:5]
    assert np.array_equal(I.bob_plane_np(p5, 1)[4], p5[3]) and np.array_equal(I.bob_plane_np(p5, 1)[0], p5[1])
    two = p[:2]
    assert np.array_equal(I.bob_plane_np(two, 0), np.stack([two[0], two[0]]))
    assert np.array_equal(I.bob_plane_np(two, 1), np.stack([two[1], two[1]]))
    one = p[:1]
    assert np.array_equal(I.bob_plane_np(one, 1), one) and np.array_equal(I.bob_plane_np(one, 0), one)
    with pytest.raises(ValueError):
        I.bob_plane_np(p, 2)
    with pytest.raises(ValueError):
        I.bob_plane_np(p.reshape(-1), 0)


@pytest.mark.parametrize('depth', [8, 10, 16])
@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('h,w', [(7, 5), (9, 7), (2, 2)])
def test_bob_payload_handles_every_plane_by_its_own_shape(h, w, layout, depth):
    g = np.random.RandomState(h * 10 + w + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    pay = g.randint(0, 1 << depth, y4m.payload_size(h, w, layout)).astype(dt)
    ch, cw = y4m.chroma_shape(h, w, layout)
    for q in (0, 1):
        got = I.bob_payload_np(pay, h, w, depth, layout, q)
        assert got.dtype == dt and got.shape == pay.shape
        exp = [_bob_scalar(pay[:h * w].reshape(h, w), q).reshape(-1)]
        for i in range(2 if layout != 'mono' else 0):
            exp.append(_bob_scalar(pay[h * w + i * ch * cw:h * w + (i + 1) * ch * cw].reshape(ch, cw), q).reshape(-1))
        assert np.array_equal(got, np.concatenate(exp))
        assert np.array_equal(I.bob_payload_np(pay.tobytes(), h, w, depth, layout, q), got)      # bytes in: the same samples
    if (h, layout) == (2, '420'):                     # one chroma row: the bottom field has none, so chroma stays
        assert np.array_equal(I.bob_payload_np(pay, h, w, depth, layout, 1)[h * w:], pay[h * w:])
    with pytest.raises(ValueError):
        I.bob_payload_np(pay[:-1], h, w, depth, layout, 0)


# ---- header and timeline -----------------------------------------------------------------------------------------------------
def test_header_takes_fixed_field_orders_only_when_asked():
    line = b'YUV4MPEG2 W720 H576 F25:1 I%s A16:15 C420mpeg2 XCOLORRANGE=LIMITED XFOO=1'
    for tag in (b't', b'b'):
        h = y4m.parse_header(line % tag, fields=True)
        assert h.interlace == tag.decode() and (h.w, h.h, h.fps) == (720, 576, 25)
        assert y4m.Reader(io.BytesIO(line % tag + b'\n'), fields=True).header.interlace == tag.decode()
    assert y4m.parse_header(line % b'p', fields=True).interlace == 'p'
    with pytest.raises(y4m.Y4MError, match='field-order fix upstream'):
        y4m.parse_header(line % b'm', fields=True)
    for tag in (b't', b'b', b'm'):
        for kw in ({}, {'fields': False}):
            with pytest.raises(y4m.Y4MError, match='--deinterlace') as e:
                y4m.parse_header(line % tag, **kw)
            assert y4m.FIX in str(e.value)
        with pytest.raises(y4m.Y4MError, match='--deinterlace'):
            y4m.Reader(io.BytesIO(line % tag + b'\n'))
    with pytest.raises(y4m.Y4MError):
        y4m.parse_header(line % b'x', fields=True)


def test_scan_takes_fields(tmp_path):
    p = y4m.payload_size(4, 6)
    path = tmp_path / 'i.y4m'
    path.write_bytes(b'YUV4MPEG2 W6 H4 F25:1 Ib\n' + b''.join(b'FRAME\n' + bytes([i]) * p for i in range(3)))
    with open(path, 'rb') as f:
        with pytest.raises(y4m.Y4MError, match='--deinterlace'):
            y4m.scan(f)
        hdr, hb, offs = y4m.scan(f, fields=True)
        assert hdr.interlace == 'b' and len(offs) == 3
        fr = y4m.Frames.from_file(f, offs, 1, 5, hdr.payload, pinned=False, fields=2)     # fields 1 .. 4: payloads 0, 1, 2
        assert [int(fr[i][0]) for i in range(1, 5)] == [0, 1, 1, 2] and not fr.has(5) and fr.n == 5
        fr = y4m.Frames.from_file(f, offs, 0, 99, hdr.payload, pinned=False, fields=2)
        assert fr.has(5) and not fr.has(6) and fr.n == 6


def test_progressive_header_and_field_parity():
    h = y4m.parse_header(b'YUV4MPEG2 W1920 H1080 F30000:1001 It A1:1 C422p10 XCOLORRANGE=FULL XYSCSS=422P10', y4m.DEPTHS, y4m.LAYOUTS,
                         fields=True)
    p = I.progressive_header(h)
    assert p.encode() == b'YUV4MPEG2 W1920 H1080 F60000:1001 Ip A1:1 C422p10 XYSCSS=422P10 XCOLORRANGE=FULL\n'
    assert (p.depth, p.layout, p.payload, p.full_range) == (10, '422', h.payload, True) and h.interlace == 't' and h.fps == Fraction(30000, 1001)
    assert [I.field_parity('t', f) for f in range(4)] == [0, 1, 0, 1]
    assert [I.field_parity('b', f) for f in range(4)] == [1, 0, 1, 0]
    with pytest.raises(ValueError):
        I.field_parity('p', 0)


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')

    def seekable(self):
        return False


def _interlaced(n, order=b't', h=4, w=6):
    p = y4m.payload_size(h, w)
    return b'YUV4MPEG2 W%d H%d F25:1 I%s\n' % (w, h, order) + b''.join(b'FRAME\n' + bytes([i + 1]) * p for i in range(n))


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
def test_frames_of_fields_share_the_payload_and_read_it_once(full):
    n = 9
    src = _Pipe(_interlaced(n))
    rd = y4m.Reader(src, fields=True)
    reads = []
    fetch = rd.read_into
    rd.read_into = lambda buf: (reads.append(rd.index), fetch(buf))[1]
    fr = y4m.Frames(rd, pinned=False, full_length=full, fields=2)
    wins, last = [], []
    for win in fr.windows():
        k = fr.first_window + len(wins)
        wins.append(win)
        last.append(fr.is_last(k))
        held = {i: fr[i] for i in sorted(set(win))}
        for i, t in held.items():
            assert int(t[0]) == i // 2 + 1 and t.shape == (rd.header.payload,)
            assert (i ^ 1) not in held or held[i ^ 1] is t                 # both fields of a payload: ONE tensor
    assert fr.n == 2 * n and reads == list(range(n + 1))                   # 2n fields; every payload read once, in order (+ the end)
    ref = y4m.Frames(y4m.Reader(io.BytesIO(_interlaced(2 * n).replace(b' It', b' Ip'))), pinned=False, full_length=full)
    ref_wins = list(ref.windows())
    assert wins == ref_wins and ref.n == 2 * n                             # the windows of a progressive stream of 2n frames
    assert last == [False] * (len(wins) - 1) + [True]
    assert fr.peak <= ref.peak and fr.peak <= 1 + 5                        # payload tensors held: bounded as for progressive input
    assert not src.read()                                                  # the pipe was consumed to its end


def test_frames_of_fields_drop_by_field_index():
    rd = y4m.Reader(io.BytesIO(_interlaced(8)), fields=True)
    fr = y4m.Frames(rd, pinned=False, fields=2)
    a, b = fr[0], fr[1]
    assert a is b and fr[2] is fr[3] and fr[2] is not a
    fr[9]
    assert sorted(fr.buf) == [6, 7, 8, 9] and fr.peak == 5
    with pytest.raises(IndexError, match='dropped'):
        fr[5]
    with pytest.raises(IndexError, match='16 frames'):
        fr[16]
    with pytest.raises(ValueError):
        y4m.Frames(rd, pinned=False, fields=3)


# ---- the runner's checks that need no GPU ---------------------------------------------------------------------------------------
def test_runner_arguments_and_rates():
    assert video.VideoRunner(None).deinterlace is False and video.VideoRunner(None).last_fields is None
    hdr = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 It', fields=True)
    vr = video.VideoRunner(None, 1, 4, deinterlace=True)
    ph, order, per = vr._progressive(hdr)
    assert (ph.fps, ph.interlace, order, per, vr.last_fields) == (50, 'p', 't', 2, 'tff')
    assert vr._out_header(ph).encode().startswith(b'YUV4MPEG2 W720 H576 F200:1 Ip')          # --mfi M gives 2 M F
    assert vr._n_out(2 * 10, ph) == (20 - 3) * 4 + 1
    vr = video.VideoRunner(None, 1, fps=Fraction(120), deinterlace=True)
    ph, order, per = vr._progressive(y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 Ib', fields=True))
    assert vr._ratio(ph) == Fraction(12, 5) and order == 'b' and vr.last_fields == 'bff'
    assert video.VideoRunner(None, 1, fps=Fraction(50), deinterlace=True)._progressive(hdr)[0].fps == 50   # the field rate itself
    prog = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 Ip')
    vr = video.VideoRunner(None, 1, fps=Fraction(30), deinterlace=True)
    assert vr._progressive(prog) == (prog, None, 1) and vr.last_fields is None                 # progressive input: nothing changes
    for fps in (Fraction(30), Fraction(25), Fraction(49)):                                    # fine for 25p, below the field rate of 25i
        vr = video.VideoRunner(None, 1, fps=fps, deinterlace=True)
        with pytest.raises(ValueError, match='field rate 50'):
            vr.run_stream(io.BytesIO(_interlaced(6)), io.BytesIO())
        assert vr._runners == {}
    with pytest.raises(y4m.Y4MError, match='--deinterlace'):                                  # without the switch: refused at the header
        video.VideoRunner(None, 1, 4).run_stream(io.BytesIO(_interlaced(6)), io.BytesIO())


def test_the_file_path_refuses_before_anything_is_built(tmp_path):
    src = tmp_path / 'in.y4m'
    src.write_bytes(_interlaced(6, b'b'))
    vr = video.VideoRunner(None, 1, 4)
    with pytest.raises(y4m.Y4MError, match='--deinterlace'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    vr = video.VideoRunner(None, 1, fps=Fraction(40), deinterlace=True)
    with pytest.raises(ValueError, match='field rate 50'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert vr._runners == {} and not (tmp_path / 'out.y4m').exists()


def test_command_line_has_the_switch():
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).deinterlace is False
    a = p.parse_args(['-', '-', '--deinterlace', '--mfi', '2', '--scene-cut', '--full-length'])
    assert a.deinterlace is True and a.mfi == 2
    assert '--deinterlace' in p.format_help() and 'It, Ib' in p.format_help()
