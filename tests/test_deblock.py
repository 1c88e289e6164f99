"""The deblocking filter in front of the network (``--deblock``, ``demfi_amd.deblock``) without a GPU: the rule by hand and at every boundary
value, what follows from it by brute force, the grid, the order of the passes, fields, the plane table, the switch from the command line to
the ``EdgeSpec``, and the place of the stage in the ingest."""
import types

import numpy as np
import pytest

from demfi_amd import deblock as DB
from demfi_amd import interlace as IL
from demfi_amd import pipeline as P
from demfi_amd import video
from demfi_amd import y4m
from demfi_amd.y4m_edge import Ingest


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def test_the_four_lines_of_the_definition_by_hand():
    a, b, s = DB.thresholds(8, 16, 4)
    assert (a, b, s) == (16, 4, 6)
    # a step of 4: below a and below s, both sides flat: strong on both sides
    assert DB.deblock_line_np([10, 10, 10, 10, 14, 14, 14, 14], a, b, s) == [10, (2 * 10 + 3 * 10 + 10 + 10 + 14 + 4) >> 3, (10 + 10 + 10 + 14 + 2) >> 2,
                                                                             (10 + 20 + 20 + 28 + 14 + 4) >> 3, (14 + 28 + 28 + 20 + 10 + 4) >> 3,
                                                                             (14 + 14 + 14 + 10 + 2) >> 2, (2 * 14 + 3 * 14 + 14 + 14 + 10 + 4) >> 3, 14]
    assert DB.deblock_line_np([10, 10, 10, 10, 14, 14, 14, 14], a, b, s) == [10, 11, 11, 12, 13, 13, 14, 14]
    # a step of 12: below a, not below s: the weak form, p0 and q0 only
    assert DB.deblock_line_np([10, 10, 10, 10, 22, 22, 22, 22], a, b, s) == [10, 10, 10, (20 + 10 + 22 + 2) >> 2, (44 + 22 + 10 + 2) >> 2, 22, 22, 22]
    assert DB.deblock_line_np([10, 10, 10, 10, 22, 22, 22, 22], a, b, s) == [10, 10, 10, 13, 19, 22, 22, 22]
    # a step of 16 = a: a real edge, left alone
    assert DB.deblock_line_np([10, 10, 10, 10, 26, 26, 26, 26], a, b, s) == [10, 10, 10, 10, 26, 26, 26, 26]
    # |p2 - p0| = 10 >= b: the p side weak, the q side strong
    assert DB.deblock_line_np([0, 20, 12, 10, 14, 14, 14, 14], a, b, s) == [0, 20, 12, (24 + 10 + 14 + 2) >> 2, (14 + 28 + 28 + 20 + 12 + 4) >> 3, 13, 14, 14]
    assert DB.deblock_line_np([0, 20, 12, 10, 14, 14, 14, 14], a, b, s) == [0, 20, 12, 12, 13, 13, 14, 14]


def _by_hand(v, a, b, s):
    """The rule, written out a second time and one line at a time."""
    p3, p2, p1, p0, q0, q1, q2, q3 = (int(x) for x in v)
    if not (abs(p0 - q0) < a and abs(p1 - p0) < b and abs(q1 - q0) < b):
        return [p3, p2, p1, p0, q0, q1, q2, q3]
    out = [p3, p2, p1, p0, q0, q1, q2, q3]
    if abs(p0 - q0) < s and abs(p2 - p0) < b:
        out[3], out[2], out[1] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (p2 + p1 + p0 + q0 + 2) >> 2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
    else:
        out[3] = (2 * p1 + p0 + q1 + 2) >> 2
    if abs(p0 - q0) < s and abs(q2 - q0) < b:
        out[4], out[5], out[6] = (q2 + 2 * q1 + 2 * q0 + 2 * p0 + p1 + 4) >> 3, (q2 + q1 + q0 + p0 + 2) >> 2, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
    else:
        out[4] = (2 * q1 + q0 + p1 + 2) >> 2
    return out


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_every_branch_at_its_boundary_values(depth):
    """|p0-q0| in {a-1, a, s-1, s}, |p1-p0| and |p2-p0| in {b-1, b}, on each side, in both directions: which samples change is what the
    thresholds say, and the values are those of the rule written out a second time."""
    a, b, s = DB.thresholds(depth, 16, 4)
    base, seen = 100 << (depth - 8), set()
    for step in (a - 1, a, s - 1, s):
        for d1 in (b - 1, b):
            for d2 in (b - 1, b):
                for e1 in (b - 1, b):
                    for e2 in (b - 1, b):
                        for sign in (1, -1):
                            p0, q0 = base, base + sign * step
                            line = [p0 + 1, p0 - sign * d2, p0 - sign * d1, p0, q0, q0 + sign * e1, q0 + sign * e2, q0 - 1]
                            out = DB.deblock_line_np(line, a, b, s)
                            assert out == _by_hand(line, a, b, s), line
                            on = step < a and d1 < b and e1 < b
                            ps, qs = on and step < s and d2 < b, on and step < s and e2 < b
                            assert out[0] == line[0] and out[7] == line[7]
                            if not on:
                                assert out == line
                            if not ps:
                                assert out[1:3] == line[1:3]
                            if not qs:
                                assert out[5:7] == line[5:7]
                            assert int(DB.line_cases(line, a, b, s)) == (1 + ps + 2 * qs if on else 0)
                            seen.add((on, ps, qs))
    assert seen == {(False, False, False), (True, False, False), (True, True, False), (True, False, True), (True, True, True)}


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_what_follows_from_the_rule_by_brute_force(depth):
    g = np.random.RandomState(depth)
    peak, sh = (1 << depth) - 1, depth - 8
    a, b, s = DB.thresholds(depth, 16, 4)
    level = g.randint(0, peak + 1, (20000, 1))
    lines = np.clip(level + np.concatenate([np.zeros((20000, 4), np.int64), g.randint(-20, 21, (20000, 1)).repeat(4, 1) << sh], 1)
                    + (g.randint(-3, 4, (20000, 8)) << sh), 0, peak)
    lines = np.concatenate([lines, g.randint(0, peak + 1, (2000, 8)), np.full((1, 8), peak), np.zeros((1, 8), np.int64)])
    out = DB._filter(lines, a, b, s)
    cases = DB.line_cases(lines, a, b, s)
    assert set(np.unique(cases)) == {0, 1, 2, 3, 4}                       # every branch is met
    for i in range(0, len(lines), 97):                                    # the vectorised rule is the rule
        assert out[i].tolist() == _by_hand(lines[i], a, b, s)
    assert (out >= lines.min(1, keepdims=True)).all() and (out <= lines.max(1, keepdims=True)).all()      # between the line's extremes
    assert (out[:, 0] == lines[:, 0]).all() and (out[:, 7] == lines[:, 7]).all()                          # p3 and q3 never change
    assert np.array_equal(DB._filter(lines[:, ::-1], a, b, s)[:, ::-1], out)                              # mirror symmetric
    assert np.array_equal(DB._filter(lines, *DB.thresholds(depth, 0, 0)), lines)                          # A = 0 is the identity
    flat = np.repeat(g.randint(0, peak + 1, (100, 1)), 8, 1)
    assert np.array_equal(DB._filter(flat, a, b, s), flat)                                                # a constant stays constant
    worst = np.full((1, 8), peak)
    assert 2 * peak + 3 * peak + 3 * peak + 4 < 1 << 20 and np.array_equal(DB._filter(worst, a, b, s), worst)      # sums below 2^20


def test_identity_constant_mirror_and_reach_on_planes():
    g = np.random.RandomState(5)
    a, b, s = DB.thresholds(8)
    p = (g.randint(40, 60, (3, 5)).repeat(8, 0).repeat(8, 1)[:22, :37] + g.randint(-2, 3, (22, 37))).astype(np.uint8)
    for left, top in ((0, 0), (3, 6)):
        out = DB.deblock_plane_np(p, a, b, s, left, top)
        assert out.dtype == p.dtype and (out != p).any()
        assert np.array_equal(DB.deblock_plane_np(p, 0, 0, 2, left, top), p)
        # mirrored in x: the edges of the mirrored plane lie at cols - x, so its phase is the one that puts them there
        xs, ys = DB.edges(p.shape[1], left), DB.edges(p.shape[0], top)
        ml, mt = (-(p.shape[1] - xs[0])) % 8, (-(p.shape[0] - ys[0])) % 8
        assert np.array_equal(DB.deblock_plane_np(p[:, ::-1], a, b, s, ml, top)[:, ::-1], out)
        assert np.array_equal(DB.deblock_plane_np(p[::-1], a, b, s, left, mt)[::-1], out)
        near_x = np.zeros(p.shape[1], bool)
        near_y = np.zeros(p.shape[0], bool)
        for x in xs:
            near_x[x - 3:x + 3] = True
        for y in ys:
            near_y[y - 3:y + 3] = True
        assert not (out != p)[~near_y][:, ~near_x].any()                  # only samples within 3 of an edge change
    const = np.full((19, 23), 77, np.uint8)
    assert np.array_equal(DB.deblock_plane_np(const, a, b, s, 2, 5), const)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def test_edges_for_every_length_and_every_removed_count():
    for n in range(4, 25):
        for removed in range(8):
            want = [x for x in range(n) if (x + removed) % 8 == 0 and x - 4 >= 0 and x + 3 <= n - 1]
            assert DB.edges(n, removed) == want, (n, removed)
    assert DB.edges(8) == [] and DB.edges(12) == [8] and DB.edges(16) == [8] and DB.edges(20) == [8, 16] and DB.edges(9, 4) == [4]
    assert DB.edges(3, 5) == [] and DB.edges(24, 2) == [6, 14] and DB.edges(16, 8) == [8]


def test_vertical_edges_first_then_horizontal_ones():
    """Around a grid crossing the two orders differ: the pinned values are those of the defined order."""
    a, b, s = DB.thresholds(8)
    p = np.array([[10] * 8 + [14] * 8] * 8 + [[14] * 8 + [22] * 8] * 8, np.uint8)
    p[7, 7], p[8, 8] = 12, 18
    vh, hv = DB.deblock_plane_np(p, a, b, s), DB.deblock_plane_np(p, a, b, s, order='hv')
    assert (vh != hv).any()
    rows = p.astype(np.int64)
    for r in range(16):                                                   # by hand: every row across x = 8, then every column across y = 8
        rows[r, 4:12] = _by_hand(rows[r, 4:12], a, b, s)
    for c in range(16):
        rows[4:12, c] = _by_hand(rows[4:12, c], a, b, s)
    assert np.array_equal(vh, rows)
    assert vh[6:10, 6:10].tolist() == [[12, 13, 14, 13], [12, 13, 15, 16], [13, 14, 17, 20], [14, 15, 18, 22]]
    assert hv[6:10, 6:10].tolist() == [[12, 12, 13, 14], [13, 13, 14, 15], [14, 15, 17, 18], [13, 16, 20, 22]]       # what the other order would give


def test_fields_are_planes_of_their_own():
    g = np.random.RandomState(9)
    h, w = 36, 40
    for layout in y4m.LAYOUTS:
        for depth in (8, 10):
            pay = np.concatenate([(g.randint(60, 90, (-(-r // 4), -(-c // 8))).repeat(4, 0).repeat(8, 1)[:r, :c] + g.randint(-2, 3, (r, c))).reshape(-1)
                                  for r, c in IL.plane_shapes(h, w, layout)]).astype(np.uint8 if depth == 8 else np.uint16) << (depth - 8)
            rect = (8, 8 + h, 6, 6 + w)
            got = DB.deblock_payload_np(pay, h, w, depth, layout, fields='t', rect=rect)
            assert np.array_equal(got, DB.deblock_payload_np(pay, h, w, depth, layout, fields='b', rect=rect))     # the order does not matter
            thr, pos, exp = DB.thresholds(depth), 0, pay.copy()
            sv, sh = DB._SUB[layout]
            for i, (r, c) in enumerate(IL.plane_shapes(h, w, layout)):
                plane = pay[pos:pos + r * c].reshape(r, c)
                tp, lp = (8 // sv, 6 // sh) if i else (8, 6)
                woven = plane.copy()
                for q in (0, 1):                                          # de-woven, filtered with the phase Tp / 2, woven again
                    woven[q::2] = DB.deblock_plane_np(plane[q::2], *thr, left=lp, top=tp // 2)
                exp[pos:pos + r * c] = woven.reshape(-1)
                pos += r * c
            assert np.array_equal(got, exp) and (got != pay).any()
            assert (got != DB.deblock_payload_np(pay, h, w, depth, layout, rect=rect)).any()       # and not as one woven plane


def test_plane_table():
    T = DB.plane_table
    assert T(12, 20, 'mono') == [(0, 12, 20, 20, 0, 0)]
    assert T(12, 20, '444') == [(0, 12, 20, 20, 0, 0), (240, 12, 20, 20, 0, 0), (480, 12, 20, 20, 0, 0)]
    assert T(12, 20, '422') == [(0, 12, 20, 20, 0, 0), (240, 12, 10, 10, 0, 0), (360, 12, 10, 10, 0, 0)]
    assert T(12, 20, '420') == [(0, 12, 20, 20, 0, 0), (240, 6, 10, 10, 0, 0), (300, 6, 10, 10, 0, 0)]
    assert T(13, 21, '420') == [(0, 13, 21, 21, 0, 0), (273, 7, 11, 11, 0, 0), (350, 7, 11, 11, 0, 0)]
    rect = (4, 16, 6, 26)                                                 # 12 x 20 cut out with 4 rows above and 6 columns to the left
    assert T(12, 20, '420', None, rect) == [(0, 12, 20, 20, 6, 4), (240, 6, 10, 10, 3, 2), (300, 6, 10, 10, 3, 2)]
    assert T(12, 20, '422', None, rect) == [(0, 12, 20, 20, 6, 4), (240, 12, 10, 10, 3, 4), (360, 12, 10, 10, 3, 4)]
    assert T(12, 20, '444', None, (12, 24, 10, 30))[1] == (240, 12, 20, 20, 2, 4)
    assert T(12, 20, '420', 't', rect) == [(0, 6, 20, 40, 6, 2), (20, 6, 20, 40, 6, 2), (240, 3, 10, 20, 3, 1), (250, 3, 10, 20, 3, 1),
                                           (300, 3, 10, 20, 3, 1), (310, 3, 10, 20, 3, 1)]
    assert T(12, 20, '420', 'b', rect) == T(12, 20, '420', 't', rect)
    assert T(13, 20, 'mono', 't') == [(0, 7, 20, 40, 0, 0), (20, 6, 20, 40, 0, 0)]
    assert T(2, 20, '420', 't') == [(0, 1, 20, 40, 0, 0), (20, 1, 20, 40, 0, 0), (40, 1, 10, 20, 0, 0), (50, 1, 10, 20, 0, 0)]      # a one-row plane has one field
    for layout in y4m.LAYOUTS:
        for fields in (None, 't'):
            tab = T(37, 45, layout, fields, (4, 41, 2, 47))
            assert 1 <= len(tab) <= DB.MAX_PLANES
            seen = np.zeros(y4m.payload_size(37, 45, layout), int)        # the entries tile the payload: every sample once
            for first, rows, cols, pitch, xp, yp in tab:
                assert 0 <= xp < 8 and 0 <= yp < 8 and pitch >= cols
                seen[(first + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :]).reshape(-1)] += 1
            assert (seen == 1).all()


def test_payload_and_stream():
    g = np.random.RandomState(2)
    h, w = 24, 40
    pays = [(g.randint(50, 80, y4m.payload_size(h, w, '420') // 16 + 1).repeat(16)[:y4m.payload_size(h, w, '420')] + g.randint(-2, 3, 1440)).astype(np.uint8)
            for _ in range(3)]
    outs = DB.deblock_stream_np(pays, h, w, 8, '420')
    assert len(outs) == 3 and all(o.dtype == np.uint8 and (o != p).any() for o, p in zip(outs, pays))
    assert all(np.array_equal(o, DB.deblock_payload_np(p, h, w, 8, '420', 16, 4)) for o, p in zip(outs, pays))
    luma = DB.deblock_plane_np(pays[0][:h * w].reshape(h, w), *DB.thresholds(8))
    assert np.array_equal(outs[0][:h * w].reshape(h, w), luma)
    assert all(np.array_equal(o, p) for o, p in zip(DB.deblock_stream_np(pays, h, w, 8, '420', 0), pays))
    with pytest.raises(ValueError, match='flat payload'):
        DB.deblock_payload_np(pays[0][:-1], h, w, 8, '420')


# ---- the switch --------------------------------------------------------------------------------------------------------------------------
def test_parse_deblock_check_params_and_thresholds():
    assert DB.DEFAULTS == (16, 4) and DB.parse_deblock('16:4') == (16, 4) and DB.parse_deblock(' 20 ') == (20, 5) and DB.parse_deblock('17') == (17, 5)
    assert DB.parse_deblock('0') == (0, 0) and DB.parse_deblock('255:255') == (255, 255) and DB.parse_deblock('9:0') == (9, 0)
    assert DB.check_params() == (16, 4) and DB.check_params(1) == (1, 1) and DB.check_params(np.int64(8), np.int32(2)) == (8, 2)
    for bad in ('', 'x', '4:', ':4', '4:5', '256', '300:2', '-1', '4:2:1', '1.5'):
        with pytest.raises(ValueError):
            DB.parse_deblock(bad)
    for bad in ((-1,), (256,), (4, 5), (4, -1), (True,), (4.0,), (4, 2.0)):
        with pytest.raises(ValueError):
            DB.check_params(*bad)
    assert DB.thresholds(8, 16, 4) == (16, 4, 6) and DB.thresholds(10, 16, 4) == (64, 16, 24) and DB.thresholds(16, 16, 4) == (4096, 1024, 1536)
    assert DB.thresholds(10, 17) == (68, 20, 25) and DB.thresholds(8, 255, 255) == (255, 255, 65) and DB.thresholds(12, 0, 0) == (0, 0, 32)
    with pytest.raises(ValueError):
        DB.thresholds(9, 16, 4)


def test_edge_spec_with_deblock():
    plain = P.EdgeSpec(True, True, False, 10, '422', None, 't', 'adaptive')
    db = P.EdgeSpec(True, True, False, 10, '422', None, 't', 'adaptive', deblock=(16, 4))
    assert db.deblock == (16, 4) and plain.deblock is None and tuple(db) == tuple(plain) and len(plain) == 8
    assert db != plain and plain != db and db != tuple(db) and plain == tuple(plain)
    assert hash(plain) == hash((tuple(plain), None))                      # as before there was the field
    assert db == P.EdgeSpec(True, True, False, 10, '422', None, 't', 'adaptive', deblock=[16, 4]) and hash(db) == hash(db._replace())
    assert db != db._replace(deblock=(16, 5)) and db._replace(deblock=None) == plain and plain._replace(deblock=(16, 4)) == db
    assert db._replace(depth=8).deblock == (16, 4) and db._replace(denoise=(5, 10, 2)).deblock == (16, 4)
    assert db._replace(denoise=(5, 10, 2))._replace(deblock=None).denoise == (5, 10, 2)
    assert len({plain, db, db._replace(deblock=(12, 4))}) == 3
    assert 'deblock=(16, 4)' in repr(db) and 'deblock' not in repr(plain) and repr(plain) == repr(db._replace(deblock=None))
    assert P.EdgeSpec(True, deblock=(0, 0)) == P.EdgeSpec(True) and P.EdgeSpec(True, deblock=(0, 0)).deblock is None     # A = 0: no stage
    assert db.reach == plain.reach == 2 and P.EdgeSpec(True, deblock=(16, 4)).reach == 0       # no look-ahead of its own
    edge = video.YuvEdge('bt601', False, '420jpeg', None, deblock=(20, 5), crop_rect=(4, 60, 6, 90))
    assert edge.deblock == (20, 5) and edge.crop_rect == (4, 60, 6, 90) and P.EdgeSpec.of(edge).deblock == (20, 5)
    plain_edge = video.YuvEdge('bt601', False, '420jpeg', None)
    assert plain_edge.deblock is None and plain_edge.crop_rect is None and P.EdgeSpec.of(plain_edge) == P.EdgeSpec(True)
    assert video.YuvEdge('bt601', False, '420jpeg', None, deblock=0).deblock is None
    with pytest.raises(ValueError):
        video.YuvEdge('bt601', False, '420jpeg', None, deblock=(4, 5))
    # nothing is refused: repeated frames, the adaptive mode, the denoiser, deep streams, layouts
    db.check(True, True, True)
    P.EdgeSpec(True, True, True, 16, '444', (7, 5, 0, 4), 't', 'bob', deblock=(16, 4)).check(True, True, True)
    P.EdgeSpec(True, denoise=(5, 10, 2), deblock=(16, 4), shutter=(2, 4), grain=(16, 1, 8, 'film', 0)).check(True, False, True)
    for spec, args, msg in ((P.EdgeSpec(True, deblock=(4, 5)), (True, False, True), 'deblock must be'),
                            (P.EdgeSpec(True, deblock=(256, 4)), (True, False, True), 'deblock must be'),
                            (P.EdgeSpec(True, deblock=(16, 4, 2)), (True, False, True), 'deblock must be'),
                            (P.EdgeSpec(False, deblock=(16, 4)), (False, False, True), 'Y4M edge')):
        with pytest.raises(ValueError, match=msg):
            spec.check(*args)


def test_runner_arguments_counter_and_tables():
    vr = video.VideoRunner(None)
    assert vr.deblock is None and vr.last_deblocked == 0
    assert video.VideoRunner(None, deblock=True).deblock == (16, 4) and video.VideoRunner(None, deblock=False).deblock is None
    assert video.VideoRunner(None, deblock=20).deblock == (20, 5) and video.VideoRunner(None, deblock='12:3').deblock == (12, 3)
    assert video.VideoRunner(None, deblock=(9, 0)).deblock == (9, 0) and video.VideoRunner(None, deblock=0).deblock is None
    assert video.check_deblock('0') is None and video.check_deblock(None) is None and video.check_deblock((16, None)) == (16, 4)
    # it goes with what the denoiser refuses, and with everything else
    vr = video.VideoRunner(None, deblock=True, dedup=True, deinterlace=True)
    assert vr.deblock == (16, 4) and vr._behind('t') == 0
    vr = video.VideoRunner(None, deblock=True, deinterlace=True, deinterlace_mode='adaptive', tile='auto', high_depth=True, tile_high_depth=True, layouts=True)
    assert vr._behind('t') == 2
    assert video.VideoRunner(None, deblock=True, denoise=True, denoise_radius=3)._behind(None) == 3
    video.check_one_rank(4, deblock=(16, 4))                              # any number of ranks
    assert 'deblock' not in video.ONE_RANK and 'deblock' not in video.ONE_RANK_EGRESS
    for kw, msg in ((dict(deblock=(4, 5)), 'B <= A'), (dict(deblock=300), '0 .. 255'), (dict(deblock=(1, 2, 3)), 'deblock must be'),
                    (dict(deblock=2.5), 'deblock must be'), (dict(deblock='x'), 'expected A or A:B')):
        with pytest.raises(ValueError, match=msg):
            video.VideoRunner(None, **kw)
    assert video.INGEST_COUNTERS['deblocked'] == 'last_deblocked' and video.INGEST_COUNTERS['denoised'] == 'last_denoised'
    vr = video.VideoRunner(None, mfi=2, deblock=True)
    vr._counted(types.SimpleNamespace(w=96, h=64, layout='420'), dict({name: 0 for name in video.COUNTERS}, deblocked=9), [], 0)
    assert vr.last_deblocked == 9 and vr.last_denoised == 0
    import inspect
    from demfi_amd.runner import WindowRunner
    assert 'self.deblocked = 0' in inspect.getsource(WindowRunner.__init__)
    # the rectangle reaches the edge only with the switch
    hdr = y4m.Header(96, 64, 25, 'p', None, '420jpeg', None, (), '420jpeg', 8, '420')
    vr = video.VideoRunner(None, mfi=2, deblock=True, crop=(4, 4, 6, 2))
    vr.last_crop = (4, 60, 6, 94)
    edge = vr._edge(hdr, None)
    assert edge.deblock == (16, 4) and edge.crop_rect == (4, 60, 6, 94)
    vr = video.VideoRunner(None, mfi=2, crop=(4, 4, 6, 2))
    vr.last_crop = (4, 60, 6, 94)
    assert vr._edge(hdr, None).crop_rect is None and vr._edge(hdr, None).deblock is None


def test_command_line(capsys):
    p = video.parser()
    assert p.parse_args(['in.y4m', 'out.y4m']).deblock is None and p.parse_args(['-', '-', '--deblock']).deblock == (16, 4)
    assert p.parse_args(['a', 'b', '--deblock', '20']).deblock == (20, 5) and p.parse_args(['a', 'b', '--deblock', '12:3', '--dedup']).deblock == (12, 3)
    assert p.parse_args(['a', 'b', '--deblock', '0']).deblock == (0, 0) and '--deblock' in p.format_help()
    for argv, msg in ((['a.y4m', 'b.y4m', '--deblock', '3:9'], 'B <= A'), (['a.y4m', 'b.y4m', '--deblock', '256'], '0 .. 255'),
                      (['a.y4m', 'b.y4m', '--deblock', 'x'], 'expected A or A:B')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
    from demfi_amd import clip
    with pytest.raises(SystemExit) as ex:                                 # the folder path has no such switch
        clip.parser().parse_args(['frames', '--deblock'])
    assert ex.value.code == 2
    for doc in (video.__doc__, video.VideoRunner.__doc__):
        assert 'deblock' in doc


# ---- the place of the stage in the ingest ----------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _ingest(spec, h=12, w=20, nslot=8, monkeypatch=None):
    import torch
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    rn = types.SimpleNamespace(lib=_FakeLib(), engine=types.SimpleNamespace(device='cpu'), depth_promoted=0, denoised=0, deblocked=0)
    ing = Ingest(rn, P.FrameSlots(nslot, 2, 2, 'cpu'), spec, h, w)
    return ing, rn


def test_the_ingest_order_with_promote_bob_and_denoise_present(monkeypatch):
    spec = P.EdgeSpec(True, depth=10, fields='t', denoise=(5, 10, 1), deblock=(16, 4), depths=(8, 10, 10, None))
    ing, rn = _ingest(spec, monkeypatch=monkeypatch)
    ing.attach(types.SimpleNamespace(full_range=False, crop_rect=(4, 16, 6, 26)))
    stream = types.SimpleNamespace(cuda_stream=0)
    has = lambda g: g < 6                                                 # noqa: E731
    near = ing.around({2, 3}, has)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2, 3})]
    assert [sl for _, sl in new] == list(range(len(new))) and len(new) == 6
    done = ing.rebuilt(new, stream)
    names = [name for name, _ in rn.lib.calls]
    assert names == ['demfi_payload_promote', 'demfi_payload_deblock', 'demfi_yuv_bob', 'demfi_payload_denoise']    # one launch each: one run of slots
    assert [f for f, _ in done] == [2, 3] and (rn.depth_promoted, rn.deblocked, rn.denoised) == (6, 6, 2)
    args = dict(rn.lib.calls)['demfi_payload_deblock']
    assert args[0] == ing.yuv_in[0].data_ptr() and args[1] == ing.Pb == 2 * y4m.payload_size(12, 20) and args[2] == 6       # in place in yuv_in
    tab = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int64 * (6 * args[4])).from_address(args[3])).reshape(-1, 6)
    assert tab.tolist() == [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))] and args[4] == 6
    assert args[5:9] == (2,) + DB.thresholds(10, 16, 4)                   # the working depth's sample size and thresholds
    # two runs of slots: two launches; nothing new: none
    rn.lib.calls.clear()
    ing.deblocked([(8, 1), (9, 2), (11, 5)], stream)
    assert [(name, a[0] - ing.yuv_in.data_ptr(), a[2]) for name, a in rn.lib.calls] == [('demfi_payload_deblock', ing.Pb, 2), ('demfi_payload_deblock', 5 * ing.Pb, 1)]
    rn.lib.calls.clear()
    ing.deblocked([], stream)
    assert not rn.lib.calls and rn.deblocked == 9


def test_the_adaptive_mode_and_the_probe_of_repeated_frames_get_deblocked_payloads(monkeypatch):
    spec = P.EdgeSpec(True, fields='b', deint_mode='adaptive', deblock=(16, 4))
    ing, rn = _ingest(spec, monkeypatch=monkeypatch)
    stream = types.SimpleNamespace(cuda_stream=0)
    near = ing.around({2}, lambda g: g < 8)
    new = [(f, ing.slots.acquire(f, None)[0]) for f in sorted(set(near) | {2})]
    ing.rebuilt(new, stream)
    assert [name for name, _ in rn.lib.calls] == ['demfi_payload_deblock', 'demfi_yuv_deint_adaptive'] and rn.deblocked == len(new) == 5
    # a frame staged by the probe is one new slot: promoted, deblocked, bobbed there
    ing, rn = _ingest(P.EdgeSpec(True, dedup=(7, 5, 0, 4), fields='t', deblock=(16, 4)), monkeypatch=monkeypatch)
    ing.rebuilt([(0, 3)], stream)
    assert [name for name, _ in rn.lib.calls] == ['demfi_payload_deblock', 'demfi_yuv_bob'] and rn.deblocked == 1


def test_without_the_switch_the_ingest_is_what_it_was(monkeypatch):
    e = object.__new__(Ingest)
    assert e.deblock is None
    for spec in (P.EdgeSpec(True, fields='t'), P.EdgeSpec(True, deblock=(0, 0), fields='t')):
        ing, rn = _ingest(spec, monkeypatch=monkeypatch)
        assert ing.deblock is None and not hasattr(ing, 'db_planes')
        ing.attach(types.SimpleNamespace(full_range=True, crop_rect=(4, 16, 6, 26)))
        assert ing.full_range is True and not hasattr(ing, 'db_planes')
        ing.rebuilt([(0, 0), (1, 1)], types.SimpleNamespace(cuda_stream=0))
        assert [name for name, _ in rn.lib.calls] == ['demfi_yuv_bob'] and rn.deblocked == 0


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
def plane_view(pay, entry):
    """The [rows, cols] view of one entry of a plane table into the flat payload ``pay``."""
    first, rows, cols, pitch = entry[:4]
    return np.lib.stride_tricks.as_strided(pay[first:], (rows, cols), (pitch * pay.itemsize, pay.itemsize))


def blocky_payload(h, w, layout, depth, seed, fields=None, rect=None, dtype=None):
    """A payload that exercises every branch: in every entry of its plane table 8x8 blocks on the entry's own grid, of levels up to +-10
    steps around a random base (so jumps of up to +-20 steps from block to block), plus noise of +-3 steps; 8-bit steps at ``depth``."""
    g = np.random.RandomState(seed)
    sh, peak = depth - 8, (1 << depth) - 1
    out = np.zeros(y4m.payload_size(h, w, layout), dtype or (np.uint8 if depth == 8 else np.uint16))
    for entry in DB.plane_table(h, w, layout, fields, rect):
        _, rows, cols, _, xp, yp = entry
        lev = g.randint(30, 220) + g.randint(-10, 11, ((rows + yp) // 8 + 1, (cols + xp) // 8 + 1))
        pl = lev.repeat(8, 0).repeat(8, 1)[yp:yp + rows, xp:xp + cols] + g.randint(-3, 4, (rows, cols))
        plane_view(out, entry)[...] = np.clip(pl << sh, 0, peak)
    return out


def edge_lines(pay, h, w, layout, fields=None, rect=None):
    """Every line [n, 8] across an edge of the payload as it comes in: rows across the vertical edges, columns across the horizontal ones."""
    ls = [np.zeros((0, 8), np.int64)]
    for entry in DB.plane_table(h, w, layout, fields, rect):
        p = plane_view(pay, entry).astype(np.int64)
        ls += [p[:, x - 4:x + 4] for x in DB.edges(entry[2], entry[4])] + [p[y - 4:y + 4].T for y in DB.edges(entry[1], entry[5])]
    return np.concatenate(ls)


def coverage(lines, depth, a=DB.DEFAULT_A, b=DB.DEFAULT_B):
    """The share of ``lines`` in each of the five cases: unfiltered, weak / weak, strong p only, strong q only, strong / strong."""
    return np.bincount(DB.line_cases(lines, *DB.thresholds(depth, a, b)), minlength=5) / max(len(lines), 1)


def blocky_clip(n, h, w, layout, d, seed=0, fps=b'24:1'):
    """A Y4M stream of coded-looking material: the moving pattern of tests/test_gpu_y4m_layouts.py with every 8x8 block of every plane
    flattened to its mean (quantised to 4 steps) plus noise of +-2 steps.  Returns (bytes, payloads as sample arrays)."""
    from tests import test_gpu_y4m_layouts as Y
    data, moving, _ = Y._clip(n, h, w, layout, d, seed=seed, fps=fps)
    g = np.random.RandomState(2000 + seed)
    sh, peak, pays = d - 8, (1 << d) - 1, []
    for m in moving:
        m = np.asarray(m).reshape(-1)
        out, pos = m.copy(), 0
        for r, c in IL.plane_shapes(h, w, layout):
            p = m[pos:pos + r * c].reshape(r, c).astype(np.int64)
            ys, xs = np.arange(0, r, 8), np.arange(0, c, 8)
            mean = np.add.reduceat(np.add.reduceat(p, ys, 0), xs, 1) // (np.diff(np.append(ys, r))[:, None] * np.diff(np.append(xs, c))[None, :])
            q = (mean >> (sh + 2) << (sh + 2)).repeat(8, 0).repeat(8, 1)[:r, :c] + (g.randint(-2, 3, (r, c)) << sh)
            out[pos:pos + r * c] = np.clip(q, 0, peak).reshape(-1)
            pos += r * c
        pays.append(out)
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_the_gpu_tests_payloads_exercise_every_branch(depth):
    """Over 200,000 edge lines of ``blocky_payload`` at 16:4 every case occurs, none below 2 %."""
    lines = np.concatenate([edge_lines(blocky_payload(96, 160, '444', depth, s), 96, 160, '444') for s in range(20)])
    share = coverage(lines, depth)
    print(len(lines), share)
    assert len(lines) >= 200000 and (share >= 0.02).all() and share[0] > 0.3
    flat = np.full((100, 8), 50 << (depth - 8))
    assert coverage(flat, depth).tolist() == [0, 0, 0, 0, 1]              # an input of one branch fails any floor on the others


@pytest.mark.parametrize('h,w,layout,d', [(64, 96, '420', 8), (48, 80, '420', 8), (48, 80, '422', 10), (96, 160, '420', 10), (48, 80, '444', 8),
                                          (48, 80, 'mono', 8)])
def test_the_gpu_tests_clip_exercises_the_filter(h, w, layout, d):
    data, pays = blocky_clip(6, h, w, layout, d, seed=3)
    assert len(pays) == 6 and pays[0].size == y4m.payload_size(h, w, layout)
    share = coverage(np.concatenate([edge_lines(p, h, w, layout) for p in pays]), d)
    changed = np.mean([(o != p).mean() for o, p in zip(DB.deblock_stream_np(pays, h, w, d, layout), pays)])
    moved = np.mean([(x != y).mean() for x, y in zip(pays, pays[1:])])
    print(share, changed, moved)
    assert (share >= 0.01).all() and changed > 0.2 and moved > 0.5
