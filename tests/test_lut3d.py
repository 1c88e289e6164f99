"""The 3D colour LUT of the Y4M egress (``--lut``) without a GPU: the ``.cube`` parser, the quantisation, the ``Cube`` object, the tables, the
tetrahedral rule of ``demfi_amd.lut3d`` against a scalar reading and against exact rational arithmetic, what follows from the rule, the
kernel's division, the spec, the layout and the switch -- and a proof that the inputs of tests/test_gpu_lut3d.py (tests/lut3d_cases.py)
reach every branch the kernel has."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import colour as CL
from demfi_amd import lut3d as LU
from demfi_amd import video
from demfi_amd.pipeline import EdgeSpec
from demfi_amd.y4m_edge import Buffer, LinearBuffer, STAGES, egress_layout, rgb_domain, rgb_tables
from tests import lut3d_cases as K

PEAK = 65535
CUBE2 = """LUT_3D_SIZE 2
0 0 0
1 0 0
0 1 0
1 1 0
0 0 1
1 0 1
0 1 1
1 1 1
"""


# ---- the file ----------------------------------------------------------------------------------------------------------------------
def test_parse_a_hand_written_cube_with_and_without_comments():
    n, t = LU.parse_cube(CUBE2)
    assert n == 2 and t.shape == (2, 2, 2, 3) and t.dtype == np.float64
    assert np.array_equal(t, LU.identity_table(2))
    dressed = ('# a comment\n\nTITLE "an identity # with a hash"\n  \nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1.0 1.0 1.0\nLUT_3D_SIZE 2  # the size\n'
               + CUBE2.split('\n', 1)[1].replace('1 0 0\n', '1 0 0   # a row\n\n', 1))
    n2, t2 = LU.parse_cube(dressed)
    assert n2 == 2 and np.array_equal(t2, t)
    assert LU.Cube.of_text(dressed) == LU.Cube.of_text(CUBE2)
    assert LU.parse_cube(LU.cube_text(t, 'x'))[1].tobytes() == t.tobytes()


def test_the_r_coordinate_changes_fastest():
    """A cube whose channels encode their own indices: row r + N g + N^2 b holds (r, g, b) / 100, and the table is indexed [b, g, r]."""
    n = 3
    rows = ['%g %g %g' % (r / 100, g / 100, b / 100) for b in range(n) for g in range(n) for r in range(n)]
    _, t = LU.parse_cube('LUT_3D_SIZE 3\n' + '\n'.join(rows))
    for b, g, r in itertools.product(range(n), repeat=3):
        assert tuple(t[b, g, r]) == (r / 100, g / 100, b / 100)
    q = LU.Cube.of_table(t)
    assert np.array_equal(LU.cube_words(q)[1 + 3 * 2 + 9 * 0], [655, 1311, 0, 0])    # r = 1, g = 2, b = 0: floor(655.35 + .5), floor(1310.7 + .5)


def _rows(n, bad=None):
    rows = ['0.5 0.5 0.5'] * n ** 3
    if bad is not None:
        rows[bad[0]] = bad[1]
    return '\n'.join(rows) + '\n'


@pytest.mark.parametrize('text,line,word', [
    ('LUT_1D_SIZE 4\n' + _rows(2), 1, 'LUT_1D_SIZE'),
    ('TITLE "t"\nLUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 2 2 2\n' + _rows(2), 4, 'DOMAIN_MAX'),
    ('LUT_3D_SIZE 2\nDOMAIN_MIN -1 0 0\n' + _rows(2), 2, 'DOMAIN_MIN'),
    ('# c\nLUT_3D_SIZE 1\n0 0 0\n', 2, 'LUT_3D_SIZE'),
    ('LUT_3D_SIZE 66\n', 1, 'LUT_3D_SIZE'),
    ('LUT_3D_SIZE 2.5\n' + _rows(2), 1, 'LUT_3D_SIZE'),
    ('LUT_3D_SIZE 2\n' + _rows(2)[:-12], 8, '7 data rows'),
    ('LUT_3D_SIZE 2\n' + _rows(2) + '0 0 0\n', 10, 'more than the 8 rows'),
    ('LUT_3D_SIZE 2\n' + _rows(2, (3, '0.5 nan 0.5')), 5, 'not finite'),
    ('LUT_3D_SIZE 2\n' + _rows(2, (0, 'inf 0 0')), 2, 'not finite'),
    ('LUT_3D_SIZE 2\n' + _rows(2, (7, '-inf 0 0')), 9, 'not finite'),
    ('LUT_3D_SIZE 2\n' + _rows(2, (1, '0.5 0.5')), 3, 'three numbers'),
    ('LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n' + _rows(2), 2, 'unknown keyword'),
    ('LUT_3D_SIZE 2\n' + _rows(2, (2, '0.5 0.5 x')), 4, 'unknown keyword'),
    ('0 0 0\nLUT_3D_SIZE 2\n', 1, 'before LUT_3D_SIZE'),
    ('LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n' + _rows(2), 2, 'twice'),
    ('# nothing\n\n', 2, 'no LUT_3D_SIZE'),
])
def test_the_parser_refuses_with_the_line(text, line, word):
    with pytest.raises(ValueError, match=r'line %d: .*%s' % (line, word)):
        LU.parse_cube(text)


def test_load_cube_names_the_file(tmp_path):
    p = tmp_path / 'a.cube'
    p.write_text(CUBE2)
    assert LU.load_cube(str(p)) == LU.Cube.of_text(CUBE2)
    p.write_text('LUT_1D_SIZE 2\n')
    with pytest.raises(ValueError, match=r'a\.cube: line 1: LUT_1D_SIZE'):
        LU.load_cube(str(p))
    with pytest.raises(ValueError, match=r'missing\.cube'):
        LU.load_cube(str(tmp_path / 'missing.cube'))


# ---- the numbers -------------------------------------------------------------------------------------------------------------------
def test_quantise_by_hand():
    x = [0.0, 1.0, 0.5, 1 / 65535, 0.5 / 65535, 0.49 / 65535, 1.5 / 65535, -0.25, 1.25, 1e9, -1e9, 65534.5 / 65535, 65534.4 / 65535]
    #    0    65535 32767.5 -> 32768, 1, .5 -> 1, .49 -> 0, 1.5 -> 2, clipped low, high, high, low, 65535, 65534
    assert LU.quantise(x).tolist() == [0, 65535, 32768, 1, 1, 0, 2, 0, 65535, 65535, 0, 65535, 65534]
    assert LU.quantise(x).dtype == np.uint16


def test_a_cube_is_immutable_hashable_and_equal_by_its_numbers():
    t = np.random.default_rng(0).random((3, 3, 3, 3))
    a, b = LU.Cube.of_table(t), LU.Cube.of_text(LU.cube_text(t, 'another title'))
    assert a == b and hash(a) == hash(b) and not a != b and len({a, b}) == 1
    t2 = t.copy()
    t2[1, 2, 0, 1] += 1 / 65535
    c = LU.Cube.of_table(t2)
    assert a != c and len({a, c}) == 2 and a != LU.Cube.of_table(LU.identity_table(3)) and a != (3, a.q.tobytes()) and a != None  # noqa: E711
    # another size with the same bytes in front is another cube
    assert LU.Cube(2, np.zeros((2, 2, 2, 3))) != LU.Cube(3, np.zeros((3, 3, 3, 3)))
    with pytest.raises(AttributeError):
        a.n = 4
    with pytest.raises(AttributeError):
        del a.q
    with pytest.raises(ValueError):
        a.q[0, 0, 0, 0] = 1
    src = np.zeros((2, 2, 2, 3), np.uint16)
    held = LU.Cube(2, src)
    src[:] = 7                                                           # the cube holds a copy
    assert held == LU.Cube(2, np.zeros((2, 2, 2, 3)))
    for n, shape in ((1, (1, 1, 1, 3)), (66, (66, 66, 66, 3)), (3, (3, 3, 3)), (3, (2, 2, 2, 3))):
        with pytest.raises(ValueError):
            LU.Cube(n, np.zeros(shape, np.uint16))


@pytest.mark.parametrize('depth', K.DEPTHS)
def test_the_code_table_and_its_inverse(depth):
    peak = (1 << depth) - 1
    e = LU.code_table(depth)
    assert e.dtype == np.uint16 and len(e) == peak + 1 and e[0] == 0 and e[peak] == PEAK
    assert [int(e[c]) for c in (1, peak // 2, peak - 1)] == [int(Fraction(PEAK * c, peak) + Fraction(1, 2)) for c in (1, peak // 2, peak - 1)]
    gaps = np.diff(e.astype(np.int64))
    assert gaps.min() == {8: 257, 10: 64, 12: 16}[depth]                 # strictly increasing; half the smallest gap is at least 8
    inv = CL.inverse_table(e)
    assert np.array_equal(inv[e], np.arange(peak + 1))
    v = np.arange(PEAK + 1)
    near = np.abs(v[:, None] - e[None, :].astype(np.int64)).argmin(axis=1) if depth == 8 else None
    if near is not None:                                                 # the nearest code; a tie goes up, which argmin does not say
        d = np.abs(v - e[inv].astype(np.int64))
        assert (d == np.abs(v - e[near].astype(np.int64))).all()
    for off in (-7, 7):                                                  # within 7 of e[c] the code is c: the identity cube moves a value by 1
        assert np.array_equal(inv[np.clip(e.astype(np.int64) + off, 0, PEAK)], np.arange(peak + 1))
    with pytest.raises(ValueError, match='--work-depth'):
        LU.code_table(14)


@pytest.mark.parametrize('n', [2, 17, 33, 65])
def test_axis_at_the_ends_and_on_both_sides_of_every_lattice_point(n):
    assert LU.axis(0, n) == (0, 0) and LU.axis(PEAK, n) == (n - 2, PEAK)
    for j in range(1, n - 1):                                            # lattice point j lies at u = 65535 j / (n - 1), where that is whole
        lo = (PEAK * j) // (n - 1)                                       # the last u at or below it
        for u in (lo - 1, lo, lo + 1):
            idx, frac = (int(x) for x in LU.axis(u, n))
            p = u * (n - 1)
            assert idx == p // PEAK and frac == p % PEAK and 0 <= frac < PEAK and idx * PEAK + frac == p
        if PEAK * j % (n - 1) == 0:
            assert tuple(int(x) for x in LU.axis(lo, n)) == (j, 0) and int(LU.axis(lo - 1, n)[0]) == j - 1
    u = np.arange(PEAK + 1)
    idx, frac = LU.axis(u, n)
    assert idx.min() == 0 and idx.max() == n - 2 and frac.min() == 0 and np.flatnonzero(frac == PEAK).tolist() == [PEAK]
    assert (idx * PEAK + frac == u * (n - 1)).all() and (np.diff(idx) >= 0).all()
    for depth in K.DEPTHS:
        words = LU.axis_table(depth, n)
        i2, f2 = LU.axis(LU.code_table(depth), n)
        assert words.dtype == np.uint32 and np.array_equal(words >> 16, i2) and np.array_equal(words & 0xffff, f2)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def _exact_pixel(v, inv_in, depth, cube):
    """The rule in rational arithmetic: barycentric weights of the tetrahedron, the mix as a fraction, rounded half up."""
    n, e = cube.n, LU.code_table(depth)
    pos, fr = [], []
    for x in v[::-1]:                                                    # R, G, B
        u = Fraction(int(e[int(inv_in[int(x)])]), PEAK) * (n - 1)
        i = min(int(u), n - 2)
        pos.append(i)
        fr.append(u - i)
    order = sorted(range(3), key=lambda a: -fr[a])
    f = [fr[a] for a in order] + [Fraction(0)]
    verts, p = [tuple(pos)], list(pos)
    for a in order:
        p[a] += 1
        verts.append(tuple(p))
    ws = [1 - f[0], f[0] - f[1], f[1] - f[2], f[2]]
    assert sum(ws) == 1 and all(w >= 0 for w in ws)
    out = [int(sum(int(cube.q[b, g, r, c]) * w for (r, g, b), w in zip(verts, ws)) + Fraction(32767, PEAK)) for c in range(3)]
    return out[2], out[1], out[0]


@pytest.mark.parametrize('depth', K.DEPTHS)
def test_the_rule_equals_the_scalar_and_the_rational_reading(depth):
    rng = np.random.default_rng(depth)
    for n in (2, 5, 33):
        cube = K.cubes(n)['random']
        for name, (fwd, inv) in K.table_pairs(depth).items():
            rgb = rng.integers(0, PEAK + 1, (3, 6, 10)).astype(np.uint16)
            rgb[:, 0, :4] = np.asarray(fwd, np.uint16)[[0, len(fwd) - 1, len(fwd) // 2, 1]]      # black, white, ties
            out = LU.lut_payload_np(rgb, inv, depth, cube)
            assert out.dtype == np.dtype('<u2') and out.shape == rgb.shape
            for y, x in itertools.product(range(6), range(10)):
                px = rgb[:, y, x]
                assert tuple(out[:, y, x]) == LU.lut_pixel(px, inv, depth, cube) == _exact_pixel(px, inv, depth, cube), (n, name, y, x)
    with pytest.raises(ValueError):
        LU.lut_payload_np(np.zeros((6, 10, 3), np.uint16), inv, depth, cube)
    with pytest.raises(ValueError):
        LU.lut_payload_np(np.zeros((3, 6, 10), np.uint8), inv, depth, cube)


def test_ties_do_not_depend_on_their_order():
    """Every kind of tie, both vertex orders evaluated explicitly.  The proof: with f_a = f_b adjacent in the sorted order the vertex between
    them has the weight f_a - f_b = 0, and it is the only vertex the order changes; the vertices before and after the pair are the same
    points either way (v0 plus the same set of steps)."""
    depth, n = 10, 5
    fwd, inv = LU.tables(depth)
    cube = K.cubes(n)['random']
    peak = (1 << depth) - 1
    seen = set()
    for c in range(peak + 1):
        for other in (0, 300, peak):
            for v in ((c, c, other), (c, other, c), (other, c, c), (c, c, c)):
                px = fwd[list(v)]
                a, b = LU.lut_pixel(px, inv, depth, cube, False), LU.lut_pixel(px, inv, depth, cube, True)
                assert a == b
                seen.add(len(set(v)))
    assert seen == {1, 2}
    # and the two orders do name different middle vertices, so the assertion above is not empty
    e = LU.code_table(depth)
    c = 300
    idx, frac = LU.axis(int(e[c]), n)
    assert 0 < frac < PEAK
    q = cube.q
    i = int(idx)
    assert not np.array_equal(q[i, i, i + 1], q[i, i + 1, i])


@pytest.mark.parametrize('n', K.NS)
def test_what_follows_from_the_rule(n):
    depth = 10
    fwd, inv = LU.tables(depth)
    rng = np.random.default_rng(n)
    rgb = rng.integers(0, PEAK + 1, (3, 40, 50)).astype(np.uint16)
    cs = K.cubes(n)
    # a cube of constant colour gives that colour
    colour = (1234, 65535, 7)
    const = LU.Cube(n, np.broadcast_to(np.array(colour, np.uint16), (n, n, n, 3)))
    out = LU.lut_payload_np(rgb, inv, depth, const)
    assert (out[2] == colour[0]).all() and (out[1] == colour[1]).all() and (out[0] == colour[2]).all()
    assert (LU.lut_payload_np(rgb, inv, depth, cs['zero']) == 0).all() and (LU.lut_payload_np(rgb, inv, depth, cs['full']) == PEAK).all()
    # every output lies between the smallest and the largest of the four Q it mixes (a fortiori of the cell's eight)
    cube = cs['random']
    out = LU.lut_payload_np(rgb, inv, depth, cube).astype(np.int64)
    idx, frac = LU.cell_coords(rgb, inv, depth, n)
    q = cube.q.astype(np.int64)
    order = np.argsort(-frac, axis=0, kind='stable')
    axes = np.arange(3)[:, None, None]
    p1 = idx + (order[0][None] == axes)
    p2 = p1 + (order[1][None] == axes)
    four = np.stack([q[p[2], p[1], p[0]] for p in (idx, p1, p2, idx + 1)])      # [4, h, w, 3] in R, G, B
    lo, hi = four.min(axis=0), four.max(axis=0)
    got = out[::-1].transpose(1, 2, 0)
    assert (lo <= got).all() and (got <= hi).all()


@pytest.mark.parametrize('n', [2, 4, 6, 16, 18])
def test_a_lattice_point_maps_to_its_q_exactly(n):
    """Where n - 1 divides 255 the code 255 j / (n - 1) has e = 65535 j / (n - 1), lattice point j with the fraction 0 (the top one: cell
    n - 2 with the fraction 65535): every lattice point of such a cube is met by an 8-bit code and comes back as its Q.  The sizes 17, 33
    and 65 have no such codes (16, 32 and 64 do not divide 65535); their cells are covered by the bounds below."""
    assert 255 % (n - 1) == 0
    fwd, inv = LU.tables(8)
    c = np.arange(n) * (255 // (n - 1))
    b, g, r = np.meshgrid(c, c, c, indexing='ij')
    cube = K.cubes(n)['random']
    got = LU.lut_payload_np(fwd[np.stack([b, g, r]).reshape(3, n * n, n)], inv, 8, cube)
    want = cube.q.reshape(n * n, n, 3)
    assert np.array_equal(got[2], want[..., 0]) and np.array_equal(got[1], want[..., 1]) and np.array_equal(got[0], want[..., 2])


@pytest.mark.parametrize('depth', K.DEPTHS)
@pytest.mark.parametrize('n', K.NS)
def test_the_identity_cube_keeps_every_code(n, depth):
    """It moves a value by at most 1 of 65535 (a rounding of at most 1/2 an entry, a convex mix, one final rounding), and half the gap of
    e is at least 8: every code on every axis and diagonal, the corners and random pixels, with e and with each transfer's tables."""
    ident = K.cubes(n)['identity']
    e = LU.code_table(depth)
    inv_e = CL.inverse_table(e)
    peak = (1 << depth) - 1
    corners = np.array(list(itertools.product((0, peak), repeat=3))).T.reshape(3, 1, 8)
    rng = np.random.default_rng(n * 100 + depth)
    codes = np.concatenate([np.concatenate([f.reshape(3, 1, -1) for f in K.enum_codes(depth)], axis=2), corners,
                            rng.integers(0, peak + 1, (3, 1, 20000))], axis=2)
    for name, (fwd, inv_in) in K.table_pairs(depth).items():
        out = LU.lut_payload_np(fwd[codes].astype(np.uint16), inv_in, depth, ident)
        assert np.abs(out.astype(np.int64) - e[codes].astype(np.int64)).max() <= 1, name
        assert np.array_equal(inv_e[out], codes), name


def test_the_numerator_bound_by_its_extreme_case():
    """The weights are 65535 - f1, f1 - f2, f2 - f3, f3 >= 0 and sum to 65535, so the numerator is at most 65535 * max Q + 32767, reached
    by any pixel of the all-65535 cube, and at least 32767, reached by the all-zero cube."""
    top = PEAK * PEAK + 32767
    assert top == 4294868992 < 1 << 32 and top + (top >> 16) + 1 < 1 << 32
    for f1, f2, f3 in ((PEAK, PEAK, PEAK), (PEAK, 0, 0), (0, 0, 0), (40000, 40000, 3), (PEAK, 30000, 1)):
        ws = (PEAK - f1, f1 - f2, f2 - f3, f3)
        assert sum(ws) == PEAK and min(ws) >= 0
        assert sum(PEAK * w for w in ws) + 32767 == top and (sum(PEAK * w for w in ws) + 32767) // PEAK == PEAK
        assert (sum(0 * w for w in ws) + 32767) // PEAK == 0


def test_the_kernels_division_is_the_floor():
    """(n + (n >> 16) + 1) >> 16 against n // 65535 on both sides of every quotient boundary and at the largest numerator."""
    k = np.arange(0, 65537, dtype=np.uint64)
    top = np.uint64(PEAK * PEAK + 32767)
    n = np.concatenate([k * np.uint64(PEAK), k[1:] * np.uint64(PEAK) - np.uint64(1), [top, top - np.uint64(1)]])
    n = n[n <= top]
    assert len(n) > 131000 and n.max() == top
    assert np.array_equal(LU.div65535(n), (n // np.uint64(PEAK)).astype(np.int64))
    rnd = np.random.default_rng(5).integers(0, int(top) + 1, 1 << 20).astype(np.uint64)
    assert np.array_equal(LU.div65535(rnd), (rnd // np.uint64(PEAK)).astype(np.int64))
    for x in (0, 65534, 65535, 65536, int(top)):                         # and in Python integers, inside 32 bits
        t = x + (x >> 16) + 1
        assert t < 1 << 32 and t >> 16 == x // PEAK


def test_the_stream_reference_with_the_identity_is_the_linear_stream():
    """``lut_stream_np`` is ``colour.linear_stream_np`` with the LUT in between: with an identity cube and a transfer the two agree, with a
    mix and a scale in front; without a transfer the RGB payloads are made with ``code_table``."""
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (12, 16, 3)).astype(np.uint8) for _ in range(6)]
    groups = [[0, 1], [2, 3, 4], [5]]
    ident = K.cubes(17)['identity']
    for scale in (None, (24, 10, 'bicubic')):
        a = LU.lut_stream_np(frames, groups, ident, 8, '420', 'bt709', False, transfer='srgb', scale=scale)
        b = CL.linear_stream_np(frames, groups, 'srgb', 8, '420', 'bt709', False, scale=scale)
        assert len(a) == len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    from demfi_amd import y4m
    plain = LU.lut_stream_np(frames, None, ident, 8, '422', 'bt601', True)
    assert all(np.array_equal(p, y4m.bgr_to_yuv_np(f, '422', 'bt601', True)) for p, f in zip(plain, frames))
    other = LU.lut_stream_np(frames, None, K.cubes(17)['random'], 8, '422', 'bt601', True)
    assert not any(np.array_equal(p, o) for p, o in zip(plain, other))


# ---- spec, layout, switch ----------------------------------------------------------------------------------------------------------
def test_the_spec_with_a_lut():
    t = np.random.default_rng(1).random((3, 3, 3, 3))
    a, b, other = LU.Cube.of_table(t), LU.Cube.of_table(t.copy()), LU.Cube.of_table(LU.identity_table(3))
    plain = EdgeSpec(True, depth=10)
    sa, sb, so = EdgeSpec(True, depth=10, lut=a), EdgeSpec(True, depth=10, lut=b), EdgeSpec(True, depth=10, lut=other)
    assert sa == sb and hash(sa) == hash(sb) and sa != so and sa != plain and plain != sa and len({sa, sb, so, plain}) == 3
    assert plain.lut is None and plain == (True, False, False, 10, '420', None, None, 'bob') and hash(plain) == hash(EdgeSpec(True, depth=10, lut=None))
    assert tuple(sa) == tuple(plain) and sa != tuple(plain)              # item for item today's record; with the field it equals no plain tuple
    assert sa._replace(lut=None) == plain and plain._replace(lut=a) == sa and sa._replace(depth=8).lut is a
    assert sa._replace(grain=(16, 1, 8, 'film', 0)).lut is a and 'lut=Cube(n=3' in repr(sa) and 'lut' not in repr(plain)

    class Y:
        lut = a
    assert EdgeSpec.of(Y()).lut is a and EdgeSpec.of(object()).lut is None
    sa._replace(y4m=True).check(True, False, False)
    for spec, word in ((EdgeSpec(True, lut=(3, t)), 'lut3d.Cube'), (EdgeSpec(False, lut=a), 'Y4M edge'), (EdgeSpec(True, depth=14, lut=a), '12 bits')):
        with pytest.raises(ValueError, match=word):
            spec.check(True, False, False)
    with pytest.raises(ValueError, match='retimed'):
        EdgeSpec(True, lut=a).check(False, False, False)


def test_the_layout_without_a_lut_is_what_it_was():
    sp = EdgeSpec(True, depth=10, shutter=(2, 4), interlace=('t', 'linear'), depths=(8, 10, 8, 'bayer'))
    assert egress_layout(sp, 9, 2, 64, 96) == [Buffer('gather', 1, 9, 18432, 64, 96), Buffer('mix', 1, 6, 18432, 64, 96),
                                               Buffer('weave', 0, 4, 18432, 64, 96), Buffer('requant', 0, 4, 9216, 64, 96), (4, 9216)]
    assert egress_layout(EdgeSpec(True), 9, 2, 64, 96) == [Buffer('gather', 0, 9, 9216, 64, 96), (9, 9216)]
    assert not rgb_domain(EdgeSpec(True, colour=('bt709', None, None)), 64, 96) and 'lut' in STAGES


def test_the_layout_with_a_lut_in_every_combination():
    cube = K.cubes(3)['random']
    order = ['gather', 'mix', 'scale', 'lut', 'encode', 'grain', 'weave', 'requant']
    for mix, scale, lin, grain, weave, requant in itertools.product((False, True), repeat=6):
        kw = dict(shutter=(3, 4) if mix else None, scale=(72, 48, 'bicubic') if scale else None, colour=('bt709', None, None) if lin else None,
                  grain=(16, 1, 8, 'film', 0) if grain else None, interlace=('b', 'off') if weave else None,
                  depths=(8, 10, 8, 'none') if requant else None)
        base = EdgeSpec(True, depth=10 if requant else 8, **kw)
        *b0, host0 = egress_layout(base, 13, 3, 64, 96)
        *b1, host1 = egress_layout(base._replace(lut=cube), 13, 3, 64, 96)
        names = [b.name for b in b1]
        assert names == [n for n in order if n in ('lut', 'encode') or n in [b.name for b in b0]] and host1 == host0
        at = names.index('lut')
        h, w = (48, 72) if scale else (64, 96)
        # everything up to the LUT holds RGB payloads, at the size behind the scaler from there on; the encode writes the run's payloads
        assert all(isinstance(b, LinearBuffer) for b in b1[:at + 1]) and not any(isinstance(b, LinearBuffer) for b in b1[at + 1:])
        assert b1[at] == LinearBuffer('lut', 0, b1[at - 1].rows, 6 * h * w, h, w) and b1[at - 1].lead == 0
        assert b1[at + 1].name == 'encode' and b1[at + 1].rows == b1[at].rows and b1[0].Pb == 6 * 64 * 96
        # behind the encode the chain is the one without the LUT, buffer for buffer
        tail0 = [b for b in b0 if b.name in ('grain', 'weave', 'requant')]
        assert [tuple(b) for b in b1[at + 2:]] == [tuple(b) for b in tail0]
        # rows and leads in front are those of the run without it
        front0 = [b for b in b0 if b.name in ('gather', 'mix', 'scale')]
        assert [(b.name, b.rows) for b in b1[:at]] == [(b.name, b.rows) for b in front0]
        assert [b.lead for b in b1[:at - 1]] == [b.lead for b in front0[:-1]]               # the last one's consumer is the LUT: lead 0, above
        # the tables: the gather's is the transfer's only where the run is in linear light; the encode's inverts code_table
        fwd, inv_in, inv_enc = rgb_tables(base._replace(lut=cube), 64, 96)
        want = CL.forward_table('bt709', base.depth) if lin and (mix or scale) else LU.code_table(base.depth)
        assert np.array_equal(fwd, want) and np.array_equal(inv_in, CL.inverse_table(want))
        assert np.array_equal(inv_enc, CL.inverse_table(LU.code_table(base.depth)))
    f0, i0, e0 = rgb_tables(EdgeSpec(True, shutter=(3, 4), colour=('srgb', None, None)), 64, 96)       # without a LUT: linear light as before
    assert np.array_equal(f0, CL.forward_table('srgb', 8)) and e0 is i0


def test_the_switch_and_its_refusals(tmp_path):
    good, bad = tmp_path / 'good.cube', tmp_path / 'bad.cube'
    good.write_text('TITLE "t"\n' + CUBE2)
    bad.write_text('LUT_3D_SIZE 2\n0 0 0\n')
    cube = LU.Cube.of_text(CUBE2)
    assert video.check_lut(None) is None and video.check_lut(None, 16) is None
    assert video.check_lut(str(good)) == cube and video.check_lut(good, 12) == cube and video.check_lut(cube, 8) is cube
    with pytest.raises(ValueError, match=r'bad\.cube: line 2: 1 data rows'):
        video.check_lut(str(bad))
    for depth in (14, 16):
        with pytest.raises(ValueError, match=r'--lut needs a working depth of 8, 10 or 12 bits.*--work-depth'):
            video.check_lut(str(good), depth)
    a = video.parser().parse_args(['in', 'out', '--lut', str(good)])
    assert a.lut == str(good) and video.parser().parse_args(['in', 'out']).lut is None
    vr = video.VideoRunner(None, mfi=2, lut=str(good))
    assert vr.lut == cube and vr.last_lut is None and vr.last_lut_payloads == 0
    assert video.VideoRunner(None, mfi=2, lut=cube).lut is cube and video.VideoRunner(None, mfi=2).lut is None
    with pytest.raises(ValueError, match=r'bad\.cube'):
        video.VideoRunner(None, mfi=2, lut=str(bad))
    with pytest.raises(ValueError, match='--work-depth'):
        video.VideoRunner(None, mfi=2, lut=cube, work_depth=14, high_depth=True)
    assert video.EGRESS_COUNTERS['lut_payloads'] == 'last_lut_payloads' and 'lut' not in video.ONE_RANK and 'lut' not in video.ONE_RANK_EGRESS
    video.check_one_rank(2, lut=cube)                                    # several ranks are fine
    edge = video.YuvEdge('bt601', False, '420jpeg', lambda j: False, lut=cube)
    assert edge.lut is cube and EdgeSpec.of(edge).lut is cube and video.YuvEdge('bt601', False, '420jpeg', lambda j: False).lut is None
    # the command line refuses before a GPU or the input is touched
    for argv, word in ((['in', 'out', '--lut', str(bad)], 'bad.cube'), (['in', 'out', '--lut', str(good), '--work-depth', '14', '--high-depth'], '--work-depth')):
        with pytest.raises(SystemExit) as ex:
            video.main(argv)
        assert ex.value.code == 2
    # a 14-bit input under a LUT is refused once the header is known, before anything is allocated
    src = tmp_path / 'in.y4m'
    src.write_bytes(b'YUV4MPEG2 W96 H64 F24:1 Ip C420p14\n' + (b'FRAME\n' + bytes(96 * 64 * 3)) * 5)
    vr = video.VideoRunner(None, mfi=2, lut=cube, high_depth=True)
    with pytest.raises(ValueError, match='--lut needs a working depth'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert vr._runners == {} and vr.last_lut_payloads == 0


# ---- what the GPU tests' inputs reach ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', K.DEPTHS)
@pytest.mark.parametrize('n', K.NS)
def test_the_gpu_inputs_reach_every_branch(n, depth):
    """Over the launches of tests/lut3d_cases.py at this size and depth, with the e tables: all six orderings of the fractions; two equal
    fractions, three equal, fractions of zero; idx = N - 2 with frac = 65535; a cell at every face of the lattice; and, with the all-zero
    and the all-65535 cube among ``cubes``, both extremes of the numerator at every pixel."""
    fwd, inv = LU.tables(depth)
    idx = np.concatenate([LU.cell_coords(K.payloads(c, fwd)[i], inv, depth, n)[0].reshape(3, -1) for _, _, c in K.launches(depth) for i in range(len(c))], axis=1)
    frac = np.concatenate([LU.cell_coords(K.payloads(c, fwd)[i], inv, depth, n)[1].reshape(3, -1) for _, _, c in K.launches(depth) for i in range(len(c))], axis=1)
    fr, fg, fb = frac
    strict = {tuple(o) for o in np.unique(np.argsort(-frac[:, (fr != fg) & (fg != fb) & (fr != fb)], axis=0), axis=1).T.tolist()}
    assert len(strict) == 6
    two = ((fr == fg) ^ (fg == fb) ^ (fr == fb)) & ~((fr == fg) & (fg == fb))
    assert (two & (frac.max(axis=0) > 0)).any() and ((fr == fg) & (fg == fb) & (fr > 0) & (fr < PEAK)).any()
    assert (frac.max(axis=0) == 0).any() and ((frac == 0).sum(axis=0) == 1).any() and ((frac == 0).sum(axis=0) == 2).any()
    for a in range(3):
        assert ((idx[a] == n - 2) & (frac[a] == PEAK)).any() and (idx[a] == 0).any() and (idx[a] == n - 2).any()
    assert ((idx == n - 2) & (frac == PEAK)).all(axis=0).any()           # the white corner
    cs = K.cubes(n)
    assert set(cs) == {'identity', 'random', 'zero', 'full', 'checker'} and cs['zero'].q.max() == 0 and cs['full'].q.min() == PEAK
    assert set(np.unique(cs['checker'].q)) == {0, PEAK} and cs['checker'].q[0, 0, 0, 0] != cs['checker'].q[0, 0, 1, 0]
    assert [(h, w) for h, w, _ in K.launches(depth)[1:]] == [(6, 10), (17, 33), (33, 70)]
    assert all(w % 8 for _, w in K.SIZES[1:]) and 33 * ((70 + 7) // 8) > 256                  # off the strip; more than one block
