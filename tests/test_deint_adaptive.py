"""Motion-adaptive deinterlacing (``--deinterlace-mode adaptive``) without a GPU: ``deint.adaptive_plane_np`` against hand-computed
samples and a scalar loop, its end rules, the rows it may read, its properties on still and on fast-moving pictures,
``y4m.Frames(behind=2)`` and the argument checks of ``VideoRunner`` and the command line."""
import io
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import deint as I
from demfi_amd import pipeline as P
from demfi_amd import video, y4m
from demfi_amd.y4m_edge import Ingest


# ---- hand-computed samples ------------------------------------------------------------------------------------------------------
def _flat(rows, cols=6, dtype=np.uint8):
    """A plane of constant rows: every direction of the bob scores 0, so its value between rows c and e is (c + e + 1) >> 1."""
    return np.repeat(np.asarray(rows, dtype)[:, None], cols, 1)


# five rows, odd rows kept (q = 1): row 2 is the one missing row with rows y-2 and y+2.  cur has c = 100 above, e = 110 below: sp = 105.
CUR = [7, 100, 7, 110, 7]
HAND = {
    # P1 = 100, N1 = 112 at row 2: d = 106, t0 = 6; P2 = N2 = cur: t1 = t2 = 0; b = 100, g = 110: mx = max(-4, 6, 0) = 6,
    # mn = min(-4, 6, 0) = -4, diff = max(6, -4, -6) = 6: 105 lies in [100, 112]
    'clamp-not-active': (([100, 9, 100, 9, 110], [100, 9, 112, 9, 110], CUR, CUR), 105),
    # P1 = N1 = 90: d = 90, t0 = 0; P2 has 106 at row 1: t1 = (6 + 0) >> 1 = 3; b = 120, g = 130: mx = max(-20, -10, 20) = 20,
    # mn = min(-20, -10, 20) = -20, diff = 3: 105 comes down to 93
    'clamped-high': (([120, 9, 90, 9, 130], [120, 9, 90, 9, 130], [7, 106, 7, 110, 7], CUR), 93),
    # P1 = N1 = 120: d = 120; t1 = 3; b = 80, g = 90: mx = max(10, 20, -20) = 20, mn = min(10, 20, -20) = -20, diff = 3: up to 117
    'clamped-low': (([80, 9, 120, 9, 90], [80, 9, 120, 9, 90], [7, 106, 7, 110, 7], CUR), 117),
    # as clamped-high but b = 80, g = 90: mx = max(-20, -10, -20) = -10, mn = -20, diff = max(3, -20, 10) = 10: 105 comes down to 100
    'raised-by-the-spatial-check': (([80, 9, 90, 9, 90], [80, 9, 90, 9, 90], [7, 106, 7, 110, 7], CUR), 100),
}


@pytest.mark.parametrize('case', sorted(HAND))
def test_hand_computed_interior_sample(case):
    (p1, n1, p2, n2), want = HAND[case]
    cur = _flat(CUR)
    assert (I.bob_plane_np(cur, 1)[2] == 105).all()
    out = I.adaptive_plane_np((_flat(p2), _flat(p1), cur, _flat(n1), _flat(n2)), 1)
    assert (out[2] == want).all(), out[2]
    assert (out[0] == 100).all() and (out[4] == 110).all()              # one neighbour: copied, as the bob does
    assert np.array_equal(out[1::2], cur[1::2]) and out.dtype == np.uint8


# ---- a scalar loop of the rule, written from the definition's text ------------------------------------------------------------------
def _scalar(planes, q):
    p2, p1, cur, n1, n2 = planes
    out = I.bob_plane_np(cur, q)
    if p1 is None and n1 is None:
        return out
    p1, n1 = (n1 if p1 is None else p1), (p1 if n1 is None else n1)
    p2, n2 = (n2 if p2 is None else p2), (p2 if n2 is None else n2)
    rows, cols = cur.shape
    for y in range(1 - q, rows, 2):
        if y < 1 or y + 1 >= rows:
            continue
        for x in range(cols):
            c, e = int(cur[y - 1, x]), int(cur[y + 1, x])
            a, b = int(p1[y, x]), int(n1[y, x])
            d, diff = (a + b) >> 1, abs(a - b) >> 1
            if p2 is not None:
                for t in (p2, n2):
                    diff = max(diff, (abs(int(t[y - 1, x]) - c) + abs(int(t[y + 1, x]) - e)) >> 1)
            if y - 2 >= 0 and y + 2 < rows:
                bb = (int(p1[y - 2, x]) + int(n1[y - 2, x])) >> 1
                gg = (int(p1[y + 2, x]) + int(n1[y + 2, x])) >> 1
                mx = max(d - e, d - c, min(bb - c, gg - e))
                mn = min(d - e, d - c, max(bb - c, gg - e))
                diff = max(diff, mn, -mx)
            out[y, x] = min(max(int(out[y, x]), d - diff), d + diff)
    return out


def _five(rows, cols, bits, seed, near=True):
    """Five seeded planes; ``near``: the neighbours are the centre plane plus small noise, so that the clamp is active at some
    samples and idle at others."""
    g = np.random.RandomState(seed)
    peak = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    cur = g.randint(0, peak + 1, (rows, cols))
    if not near:
        return [g.randint(0, peak + 1, (rows, cols)).astype(dt) for _ in range(2)] + [cur.astype(dt)] + \
               [g.randint(0, peak + 1, (rows, cols)).astype(dt) for _ in range(2)]
    s = max(peak >> 4, 1)
    return [np.clip(cur + g.randint(-s, s + 1, (rows, cols)), 0, peak).astype(dt) if i != 2 else cur.astype(dt) for i in range(5)]


PATTERNS = {'all': (1, 1, 1, 1, 1), 'first-field': (0, 0, 1, 1, 1), 'second-field': (0, 1, 1, 1, 1), 'last-field': (1, 1, 1, 0, 0),
            'next-to-last': (1, 1, 1, 1, 0), 'one-payload-first': (0, 0, 1, 1, 0), 'one-payload-second': (0, 1, 1, 0, 0)}


def _mask(planes, pattern):
    return [p if on else None for p, on in zip(planes, pattern)]


@pytest.mark.parametrize('bits', [8, 10, 16])
@pytest.mark.parametrize('q', [0, 1])
@pytest.mark.parametrize('rows,cols', [(1, 4), (2, 2), (3, 5), (4, 7), (5, 8), (6, 9), (11, 19)])
def test_equals_the_scalar_loop_with_every_end_rule(rows, cols, q, bits):
    """Planes of 1 to 5 rows have no rows y-2 / y+2 (or no interior row at all); f = 0, f = last and a one-payload stream."""
    for near in (True, False):
        planes = _five(rows, cols, bits, rows * 100 + cols + q + bits, near)
        for name, pat in PATTERNS.items():
            got, exp = I.adaptive_plane_np(_mask(planes, pat), q), _scalar(_mask(planes, pat), q)
            assert got.dtype == planes[2].dtype and np.array_equal(got, exp), (name, near)
            assert np.array_equal(got[q::2], planes[2][q::2])            # kept rows untouched
            if rows <= q:
                assert np.array_equal(got, planes[2])                    # no kept row: the plane is returned as it is
    assert np.array_equal(I.adaptive_plane_np(_mask(planes, (1, 0, 1, 0, 1)), q), I.bob_plane_np(planes[2], q))   # neither P1 nor N1


def test_end_rules_substitute_the_partner_in_time():
    planes = _five(9, 12, 8, 5)
    p2, p1, cur, n1, n2 = planes
    assert np.array_equal(I.adaptive_plane_np((None, None, cur, n1, n2), 0), I.adaptive_plane_np((n2, n1, cur, n1, n2), 0))
    assert np.array_equal(I.adaptive_plane_np((p2, p1, cur, None, None), 1), I.adaptive_plane_np((p2, p1, cur, p1, p2), 1))
    assert np.array_equal(I.adaptive_plane_np((None, p1, cur, n1, n2), 0), I.adaptive_plane_np((n2, p1, cur, n1, n2), 0))
    one = I.adaptive_plane_np((None, None, cur, n1, None), 0)            # a one-payload stream: t1 and t2 are dropped
    assert np.array_equal(one, _scalar((None, None, cur, n1, None), 0))
    with pytest.raises(ValueError):
        I.adaptive_plane_np((p2, p1, cur, n1[:4], n2), 0)
    with pytest.raises(ValueError):
        I.adaptive_plane_np((p2, p1, cur, n1, n2), 2)


@pytest.mark.parametrize('q', [0, 1])
@pytest.mark.parametrize('bits', [8, 16])
def test_only_rows_of_the_stated_parity_are_read(q, bits):
    """Garbage in the rows a neighbour does not own (and in the missing rows of the plane itself) changes nothing: this is what
    lets the GPU side read neighbouring slots whose other rows were already rewritten."""
    planes = _five(10, 13, bits, 17 + q)
    for pat in PATTERNS.values():
        exp = I.adaptive_plane_np(_mask(planes, pat), q)
        g = np.random.RandomState(3)
        dirty = [p.copy() for p in planes]
        for i, own in enumerate((q, 1 - q, q, 1 - q, q)):                # P2, cur, N2 own parity q; P1, N1 parity 1-q
            dirty[i][1 - own::2] = g.randint(0, 1 << bits, dirty[i][1 - own::2].shape)
        got = I.adaptive_plane_np(_mask(dirty, pat), q)
        assert np.array_equal(got, exp)


# ---- properties ------------------------------------------------------------------------------------------------------------------
def _weave_fields(src):
    """A still scene: every payload is the progressive frame itself, so every field of every payload shows ``src``."""
    return [src] * 5


@pytest.mark.parametrize('order', ['t', 'b'])
@pytest.mark.parametrize('bits', [8, 10])
def test_a_static_scene_comes_back_at_full_vertical_resolution(order, bits):
    """A frame monotone down every column (a rounded quadratic plus a column-dependent offset) woven into fields and repeated over
    three payloads: every missing row with both neighbours equals the source row; the bob does not give it back."""
    h, w = 16, 12
    yy, xx = np.mgrid[0:h, 0:w]
    peak = (1 << bits) - 1
    src = ((yy * yy * (peak - 40)) // ((h - 1) * (h - 1)) + (xx * 7) % 37).astype(np.uint8 if bits == 8 else np.uint16)
    assert (np.diff(src.astype(np.int64), axis=0) >= 0).all() and src.max() <= peak
    pays = [src.reshape(-1)] * 3                                          # mono payloads: the plane alone
    outs = I.adaptive_stream_np(pays, h, w, bits, 'mono', order)
    assert len(outs) == 6
    for f, out in enumerate(outs):
        q = I.field_parity(order, f)
        ys = np.arange(1 - q, h, 2)
        ys = ys[(ys >= 1) & (ys + 1 < h)]
        got = out.reshape(h, w)
        assert np.array_equal(got[ys], src[ys]), f
        assert not np.array_equal(I.bob_plane_np(src, q)[ys], src[ys])    # the test discriminates
    assert I.field_parity('t', 0) != I.field_parity('b', 0)


@pytest.mark.parametrize('bits', [8, 10, 16])
def test_far_motion_gives_the_bob(bits):
    """Neighbouring fields differ by more than peak / 2 everywhere: diff > peak / 4 ... in fact |P1 - N1| >> 1 and the P2 / N2 terms
    exceed any distance between sp and d, so the clamp is idle."""
    peak = (1 << bits) - 1
    g = np.random.RandomState(bits)
    dt = np.uint8 if bits == 8 else np.uint16
    lo = lambda: g.randint(0, peak // 8, (12, 15)).astype(dt)            # noqa: E731
    hi = lambda: (peak - g.randint(0, peak // 8, (12, 15))).astype(dt)   # noqa: E731
    for q in (0, 1):
        planes = (hi(), lo(), lo(), hi(), hi())                           # cur dark; P1 dark, N1 bright; P2, N2 bright
        assert np.array_equal(I.adaptive_plane_np(planes, q), I.bob_plane_np(planes[2], q))


@pytest.mark.parametrize('bits', [8, 10, 16])
def test_result_lies_in_the_interval_and_in_range(bits):
    peak = (1 << bits) - 1
    for seed, near in ((1, True), (2, False)):
        planes = _five(14, 21, bits, seed, near)
        for q in (0, 1):
            out = I.adaptive_plane_np(planes, q).astype(np.int64)
            ys, d, diff = I.adaptive_bounds_np(planes, q)
            assert ((out[ys] >= d - diff) & (out[ys] <= d + diff)).all() and (diff >= 0).all()
            assert out.min() >= 0 and out.max() <= peak
    assert I.adaptive_bounds_np(_mask(planes, (1, 0, 1, 0, 1)), 0) is None


@pytest.mark.parametrize('h,w,layout,depth', [(6, 9, '420', 8), (7, 17, '422', 10), (5, 8, '444', 16), (9, 7, 'mono', 8)])
def test_payload_handles_every_plane_by_its_own_shape(h, w, layout, depth):
    g = np.random.RandomState(h + w)
    dt = np.uint8 if depth == 8 else np.uint16
    pays = [g.randint(0, 1 << depth, y4m.payload_size(h, w, layout)).astype(dt) for _ in range(5)]
    for pat in ((1, 1, 1, 1, 1), (0, 0, 1, 1, 0)):
        for q in (0, 1):
            got = I.adaptive_payload_np(_mask(pays, pat), h, w, depth, layout, q)
            split = [None if p is None else y4m.split_planes_layout(p, h, w, layout) for p in _mask(pays, pat)]
            exp = np.concatenate([I.adaptive_plane_np([None if s is None else s[i] for s in split], q).reshape(-1)
                                  for i in range(3) if split[2][i] is not None])
            assert got.dtype == dt and np.array_equal(got, exp)
            assert np.array_equal(I.adaptive_payload_np([None if p is None else p.tobytes() for p in _mask(pays, pat)], h, w, depth, layout, q), got)
    with pytest.raises(ValueError):
        I.adaptive_payload_np([pays[0], pays[1], None, pays[3], pays[4]], h, w, depth, layout, 0)
    assert I.field_neighbours(0, 6) == [None, None, 0, 1, 2] and I.field_neighbours(5, 6) == [3, 4, 5, None, None]
    assert I.field_neighbours(1, 2) == [None, 0, 1, None, None]


def test_the_bob_is_unchanged_by_the_shared_spatial_value():
    g = np.random.RandomState(0)
    p = g.randint(0, 256, (9, 20)).astype(np.uint8)
    assert int(I.bob_plane_np(p, 0).astype(np.int64).sum()) == 21342     # the value the function gave before the factoring
    ys = np.arange(1, 8, 2)
    assert np.array_equal(I.bob_plane_np(p, 0)[ys], I.edge_average_np(p[ys - 1], p[ys + 1]))


# ---- y4m.Frames(behind=...) ---------------------------------------------------------------------------------------------------------
def _interlaced(n, order=b't', h=4, w=6):
    p = y4m.payload_size(h, w)
    return b'YUV4MPEG2 W%d H%d F25:1 I%s\n' % (w, h, order) + b''.join(b'FRAME\n' + bytes([i + 1]) * p for i in range(n))


def _record(**kw):
    rd = y4m.Reader(io.BytesIO(_interlaced(5)), fields=True)
    log, fetch = [], rd.read_into
    rd.read_into = lambda buf: (log.append(('read', rd.index)), fetch(buf))[1]
    fr = y4m.Frames(rd, pinned=False, fields=2, **kw)
    for win in fr.windows():
        for i in win:
            fr[i]
            log.append(('held', i, tuple(sorted(fr.buf))))
    return log, fr.peak


# what the class gave before the keyword existed, on five payloads of two fields: reads of the input and the fields held after each access
RECORDED = ([('read', 0), ('read', 1), ('read', 2), ('held', 1, (0, 1, 2, 3, 4, 5)), ('held', 2, (0, 1, 2, 3, 4, 5)), ('held', 0, (0, 1, 2, 3, 4, 5)),
             ('held', 3, (0, 1, 2, 3, 4, 5)), ('held', 2, (0, 1, 2, 3, 4, 5)), ('held', 3, (0, 1, 2, 3, 4, 5)), ('held', 1, (0, 1, 2, 3, 4, 5)),
             ('held', 4, (1, 2, 3, 4, 5)), ('read', 3), ('held', 3, (1, 2, 3, 4, 5, 6, 7)), ('held', 4, (1, 2, 3, 4, 5, 6, 7)),
             ('held', 2, (1, 2, 3, 4, 5, 6, 7)), ('held', 5, (2, 3, 4, 5, 6, 7)), ('held', 4, (2, 3, 4, 5, 6, 7)), ('held', 5, (2, 3, 4, 5, 6, 7)),
             ('held', 3, (2, 3, 4, 5, 6, 7)), ('held', 6, (3, 4, 5, 6, 7)), ('read', 4), ('held', 5, (3, 4, 5, 6, 7, 8, 9)),
             ('held', 6, (3, 4, 5, 6, 7, 8, 9)), ('held', 4, (3, 4, 5, 6, 7, 8, 9)), ('held', 7, (4, 5, 6, 7, 8, 9)), ('held', 6, (4, 5, 6, 7, 8, 9)),
             ('held', 7, (4, 5, 6, 7, 8, 9)), ('held', 5, (4, 5, 6, 7, 8, 9)), ('held', 8, (5, 6, 7, 8, 9)), ('read', 5), ('held', 7, (5, 6, 7, 8, 9)),
             ('held', 8, (5, 6, 7, 8, 9)), ('held', 6, (5, 6, 7, 8, 9)), ('held', 9, (6, 7, 8, 9))], 4)


def test_frames_default_reads_and_drops_as_before():
    assert _record() == RECORDED and _record(behind=0) == RECORDED


def test_frames_behind_keeps_two_more_fields_and_starts_two_earlier(tmp_path):
    rd = y4m.Reader(io.BytesIO(_interlaced(8)), fields=True)
    fr = y4m.Frames(rd, pinned=False, fields=2, behind=2)
    fr[0]
    fr[9]
    assert sorted(fr.buf) == [4, 5, 6, 7, 8, 9] and fr.peak == 5          # fields 4 and 5 stay: two more than without
    fr[4]
    with pytest.raises(IndexError, match='dropped'):
        fr[3]
    log, peak = _record(behind=2)
    assert [x for x in log if x[0] == 'read'] == [x for x in RECORDED[0] if x[0] == 'read'] and peak <= RECORDED[1] + 1
    # a block of a file that starts at field 5 and ends before field 11: fields 3 .. 12 are there, no more
    src = tmp_path / 'in.y4m'
    src.write_bytes(_interlaced(8))
    with open(src, 'rb') as f:
        hdr, _, offs = y4m.scan(f, fields=True)
        fr = y4m.Frames.from_file(f, offs, 5, 11, hdr.payload, pinned=False, fields=2, behind=2)
        assert fr.has(3) and int(fr[3][0]) == 2 and int(fr[4][0]) == 3 and 2 in fr.buf   # payload 1 holds fields 2 and 3
        assert fr.has(12) and not fr.has(13) and fr.n == 13 and int(fr[12][0]) == 7
        old = y4m.Frames.from_file(f, offs, 5, 11, hdr.payload, pinned=False, fields=2)
        assert old.has(5) and 3 not in old.buf and not old.has(11) and old.n == 11
        end = y4m.Frames.from_file(f, offs, 1, 15, hdr.payload, pinned=False, fields=2, behind=2)     # clamped at both ends of the file
        assert end.has(0) and end.has(15) and not end.has(16)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            y4m.Frames(rd, pinned=False, fields=2, behind=bad)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_runner_arguments():
    assert video.VideoRunner(None).deinterlace_mode == 'bob'
    assert video.VideoRunner(None, deinterlace=True, deinterlace_mode='bob').deinterlace_mode == 'bob'
    vr = video.VideoRunner(None, 1, 2, deinterlace=True, deinterlace_mode='adaptive')
    assert vr.deinterlace_mode == 'adaptive' and vr._behind('t') == 2 and vr._behind(None) == 0
    assert video.VideoRunner(None, deinterlace=True)._behind('t') == 0
    with pytest.raises(ValueError, match='needs --deinterlace'):
        video.VideoRunner(None, deinterlace_mode='adaptive')
    with pytest.raises(ValueError, match='--deinterlace-mode bob'):      # refused at construction: nothing is allocated yet
        video.VideoRunner(None, deinterlace=True, deinterlace_mode='adaptive', dedup=True)
    with pytest.raises(ValueError, match='--deinterlace-mode bob'):
        video.VideoRunner(None, deinterlace=True, deinterlace_mode='adaptive', dedup=(5, 3, Fraction(1, 3)))
    with pytest.raises(ValueError, match='one of bob, adaptive'):
        video.VideoRunner(None, deinterlace=True, deinterlace_mode='yadif')
    assert video.VideoRunner(None, deinterlace=True, deinterlace_mode='bob', dedup=True).dedup is not None
    e = video.YuvEdge('bt601', False, '420jpeg', None, fields='t', deint_mode='adaptive')
    assert e.deint_mode == 'adaptive' and video.YuvEdge('bt601', False, '420jpeg', None).deint_mode == 'bob'
    assert P.EdgeSpec(True, False, False, fields='t') == P.EdgeSpec(True, False, False, fields='t', deint_mode='bob')
    assert P.EdgeSpec(True, False, False, fields='t', deint_mode='adaptive') != P.EdgeSpec(True, False, False, fields='t')


def test_command_line(capsys):
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).deinterlace_mode == 'bob'
    assert p.parse_args(['-', '-', '--deinterlace', '--deinterlace-mode', 'adaptive']).deinterlace_mode == 'adaptive'
    assert '--deinterlace-mode' in p.format_help()
    for argv, msg in ((['a.y4m', 'b.y4m', '--deinterlace-mode', 'adaptive'], 'needs --deinterlace'),
                      (['a.y4m', 'b.y4m', '--deinterlace', '--deinterlace-mode', 'adaptive', '--dedup'], '--deinterlace-mode bob')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err


# ---- residency: the edge's bookkeeping, driven as the batch loop drives it, without a GPU ----------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def demfi_yuv_deint_adaptive(self, base, size, offs_host, offs_dev, n, h, w, layout, es, mask, stream):
        import ctypes
        self.calls.append((list((ctypes.c_int64 * (5 * n)).from_address(offs_host)), n, mask))
        return 0


def _fake_edge(nslot, order='t', pb=36):
    import types

    import torch
    slots = P.FrameSlots(nslot, 2, 2, 'cpu')
    e = object.__new__(Ingest)
    e.slots, e.adaptive, e.raw, e.fields, e.Pb, e.es, e.fh, e.fw, e.layout = slots, True, {}, order, pb, 1, 4, 6, '420'
    e.rn = types.SimpleNamespace(lib=_FakeLib())
    e.yuv_in = torch.empty((nslot, pb), dtype=torch.uint8)
    e.dei_offs = torch.empty(5 * nslot, dtype=torch.int64)
    return e


def _drive(frames, windows, batch, n_fields, extra=(), order='t', monkeypatch=None):
    """The uploads and rebuilds of a run of ``windows`` over ``frames`` in batches of ``batch``, in the order of ``ClipPipeline.run``.
    Returns the uploads (field indices in order) and the fields rebuilt per batch."""
    import itertools
    import types

    import torch
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    e = _fake_edge(max(2 * batch + 12, 8 * batch), order)
    stream = types.SimpleNamespace(cuda_stream=0)
    it = iter(windows)
    wins = list(itertools.islice(it, batch))
    ups, rebuilt, finished = [], [], set()
    while wins:
        new = []

        def resident(idx):
            sl, fresh = e.slots.acquire(idx, None)
            if fresh:
                frames[idx]                                               # must still be held by the host side
                ups.append(idx)
                new.append((idx, sl))
        named = set(extra).union(*wins)
        for _, idx in P.residency_order(extra, wins, e.around(named, frames.has)):
            resident(idx)
        calls0 = len(e.rn.lib.calls)
        done = e._adaptive(new, stream)
        fs = [f for f, _ in done]
        assert not finished & set(fs) and fs == sorted(fs)                # a field is rebuilt once
        offs = [o for c in e.rn.lib.calls[calls0:] for o in c[0]]
        assert len(offs) == 5 * len(fs)
        for i, f in enumerate(fs):                                        # the offsets name the slots of f-2 .. f+2, -1 only beyond the stream's ends
            want = [e.slots.slot_of[g] * e.Pb if 0 <= g < n_fields else -1 for g in range(f - 2, f + 3)]
            assert offs[5 * i:5 * i + 5] == want, (f, offs[5 * i:5 * i + 5], want)
        masks = [c[2] for c in e.rn.lib.calls[calls0:]]
        assert masks == ([sum(I.field_parity(order, f) << i for i, f in enumerate(fs))] if fs else [])   # one launch per batch
        finished |= set(fs)
        assert named <= finished                                          # what the batch converts and runs is progressive
        rebuilt.append(fs)
        extra = ()
        wins = list(itertools.islice(it, batch))
    return ups, rebuilt


@pytest.mark.parametrize('batch', [1, 2, 4])
@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
def test_residency_of_a_stream(batch, full, monkeypatch):
    n = 7
    rd = y4m.Reader(io.BytesIO(_interlaced(n)), fields=True)
    fr = y4m.Frames(rd, pinned=False, full_length=full, fields=2, behind=2)
    ups, rebuilt = _drive(fr, fr.windows(), batch, 2 * n, monkeypatch=monkeypatch)
    assert sorted(ups) == list(range(2 * n)) and len(set(ups)) == len(ups)        # every field uploaded once: as the bob does
    assert sorted(f for fs in rebuilt for f in fs) == list(range(2 * n))
    assert fr.peak <= batch // 2 + 6                                      # payload tensors held: bounded by the batch, not the input


@pytest.mark.parametrize('lo,count,cuts', [(5, 4, False), (5, 4, True), (0, 5, False), (9, 2, True)])
def test_residency_of_a_block_of_a_file(lo, count, cuts, tmp_path, monkeypatch):
    """A rank's block of windows lo .. lo+count-1 of 7 payloads (14 fields): the two fields before its first frame and the two after
    its last are uploaded raw and never rebuilt; with scene cuts the block also rebuilds the field before its first window."""
    n = 7
    src = tmp_path / 'in.y4m'
    src.write_bytes(_interlaced(n))
    with open(src, 'rb') as f:
        hdr, _, offs = y4m.scan(f, fields=True)
        first = max(lo - 1, 0) if cuts else lo
        fr = y4m.Frames.from_file(f, offs, first, lo + count + 3, hdr.payload, pinned=False, fields=2, behind=2)
        wins = [(k + 1, k + 2, k, k + 3) for k in range(lo, lo + count)]
        ups, rebuilt = _drive(fr, wins, 2, 2 * n, extra=(first,) if cuts and first < lo else (), monkeypatch=monkeypatch)
    named = list(range(first, lo + count + 3))
    assert sorted(f for fs in rebuilt for f in fs) == named
    assert sorted(ups) == list(range(max(first - 2, 0), min(lo + count + 5, 2 * n))) and len(set(ups)) == len(ups)
