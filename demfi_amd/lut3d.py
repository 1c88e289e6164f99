"""A user's 3D colour LUT at the egress of the Y4M edge (``demfi_amd.video --lut FILE.cube``): the definitions, in numpy with exact integers.
The module is the only one that knows the rule; the kernel of csrc/lut3d.hip (``demfi_rgb_lut3d``) matches ``lut_payload_np`` byte for byte
and computes no curve and no gamut arithmetic: HDR10 or HLG to SDR, BT.2020 to BT.709, camera log to display, a legaliser or a look all
arrive as data.

The file.  ``parse_cube`` reads the Adobe / Resolve ``.cube`` text: ``#`` comments, blank lines, an optional ``TITLE``, ``LUT_3D_SIZE N``
(2 .. 65), optional ``DOMAIN_MIN 0 0 0`` / ``DOMAIN_MAX 1 1 1``, then N^3 lines of three floats (R, G, B of the output) with the R
coordinate of the input changing fastest.  The table is float64 [N, N, N, 3] indexed [b, g, r]: the row for the input lattice point
(r, g, b) is line r + N g + N^2 b.  Refused, with the line: ``LUT_1D_SIZE``, another domain, N out of range, a wrong number of rows, a
value that is not finite, an unknown keyword.

The numbers.  ``quantise``: Q = clip(floor(65535 x + 0.5), 0, 65535), uint16; values outside [0, 1], which many shipped LUTs have, are
clipped.  A ``Cube`` holds N and Q, immutable and hashable: equal to exactly the cubes of the same N and Q bytes, so two files with the
same numbers key one cached pipeline.

The coordinates.  ``code_table(depth)``: e[c] = (2 * 65535 * c + peak) // (2 * peak), the 16-bit value of the working-depth code c; it
plays the role of ``colour.forward_table`` in a run that is not in linear light, increases strictly at 8, 10 and 12 bits (its smallest
step: 257 / 64 / 16), and ``colour.inverse_table(e)`` is its nearest-code inverse.  ``axis(u, N)``: p = u (N - 1), idx = min(p // 65535,
N - 2), frac = p - 65535 idx in 0 .. 65535, 65535 only at u = 65535.

The rule, ``lut_payload_np(rgb, inv_in, depth, cube)``.  The input is an RGB payload, uint16 [3, h, w] with planes B, G, R
(``demfi_amd.colour``).  Per pixel and channel code = inv_in[v], the working-depth code the encode stage would have written, u = e[code],
(idx, frac) = axis(u, N).  Tetrahedral interpolation: with the three fractions sorted f1 >= f2 >= f3, v0 the cell's low corner, v1 = v0
plus one step along the axis of f1, v2 = v1 plus one step along the axis of f2, v3 the high corner, per output channel
    out = (Q[v0] (65535 - f1) + Q[v1] (f1 - f2) + Q[v2] (f2 - f3) + Q[v3] f3 + 32767) // 65535.
The weights sum to 65535, so the numerator is at most 65535^2 + 32767 < 2^32; a tie between fractions gives the disputed vertex the weight
0, so the order of tied fractions never shows.  The output is an RGB payload of 16-bit ENCODED values, which the encode stage reads
through ``colour.inverse_table(e)``.  An identity cube of any size moves a value by at most 1 of 65535 (a rounding of at most 1/2 an
entry, a convex mix, one final rounding) and half the gap of e is at least 8, so it returns every code.

``div65535`` is the kernel's form of the division, (n + (n >> 16) + 1) >> 16, which stays below 2^32 and equals the floor over the whole
range of the numerator.  ``axis_table`` and ``cube_words`` are the two device tables of the kernel: per code the word idx << 16 | frac
of axis(e[code], N), so the kernel divides nothing by N - 1, and the cube as [N^3][4] uint16 (R, G, B, 0), one lattice point an 8-byte
word.

Not offered: a LUT in front of the network, 1D and shaper LUTs, domains other than 0 .. 1, trilinear interpolation, other file formats,
a transfer or primaries tag in the header (Y4M has none), working depths 14 and 16, ``demfi_amd.clip``, numeric equality with ffmpeg's
``lut3d`` or OCIO."""
import math

import numpy as np

from . import colour as CL
from . import scale as SC
from . import shutter as SH

MIN_N, MAX_N = 2, 65
PEAK = 65535
MAX_DEPTH = CL.MAX_DEPTH
KEYWORDS = ('TITLE', 'LUT_3D_SIZE', 'DOMAIN_MIN', 'DOMAIN_MAX')


def _floats(tokens):
    try:
        return [float(t) for t in tokens]
    except ValueError:
        return None


def parse_cube(text):
    """The ``.cube`` text -> (N, float64 [N, N, N, 3] indexed [b, g, r]).  ValueError, naming the line, for what the module does not read."""
    n, rows, first_row = None, [], None
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.split('#', 1)[0].strip()
        if not line:
            continue
        tok = line.split()
        vals = _floats(tok)
        if vals is not None:                         # a data line (float() reads nan and inf: they get here and are refused)
            if n is None:
                raise ValueError('line %d: data before LUT_3D_SIZE' % no)
            if len(vals) != 3:
                raise ValueError('line %d: a data line holds three numbers, got %d' % (no, len(vals)))
            if not all(math.isfinite(v) for v in vals):
                raise ValueError('line %d: a value that is not finite: %s' % (no, line))
            if len(rows) == n ** 3:
                raise ValueError('line %d: more than the %d rows of LUT_3D_SIZE %d' % (no, n ** 3, n))
            first_row = first_row or no
            rows.append(vals)
            continue
        key = tok[0]
        if key == 'TITLE':
            continue
        if key not in KEYWORDS + ('LUT_1D_SIZE',):
            raise ValueError('line %d: unknown keyword %r (known: %s)' % (no, key, ', '.join(KEYWORDS)))
        if rows:
            raise ValueError('line %d: %s behind the first data line (line %d)' % (no, key, first_row))
        if key == 'LUT_1D_SIZE':
            raise ValueError('line %d: LUT_1D_SIZE: 1D and shaper LUTs are not offered, only LUT_3D_SIZE' % no)
        if key == 'LUT_3D_SIZE':
            if n is not None:
                raise ValueError('line %d: LUT_3D_SIZE given twice' % no)
            if len(tok) != 2 or not tok[1].isdigit() or not MIN_N <= int(tok[1]) <= MAX_N:
                raise ValueError('line %d: LUT_3D_SIZE must be one integer in %d..%d, got %r' % (no, MIN_N, MAX_N, ' '.join(tok[1:])))
            n = int(tok[1])
        else:
            want = [0.0] * 3 if key == 'DOMAIN_MIN' else [1.0] * 3
            if _floats(tok[1:]) != want:
                raise ValueError('line %d: %s must be %s: other domains are not offered, got %r'
                                 % (no, key, ' '.join('%d' % v for v in want), ' '.join(tok[1:])))
    if n is None:
        raise ValueError('line %d: no LUT_3D_SIZE in the file' % (len(text.splitlines()) or 1))
    if len(rows) != n ** 3:
        raise ValueError('line %d: %d data rows for LUT_3D_SIZE %d, which needs %d' % (len(text.splitlines()), len(rows), n, n ** 3))
    return n, np.asarray(rows, np.float64).reshape(n, n, n, 3)


def quantise(table):
    """Q = clip(floor(65535 x + 0.5), 0, 65535) as uint16; values outside [0, 1] are clipped."""
    return np.clip(np.floor(PEAK * np.asarray(table, np.float64) + 0.5), 0, PEAK).astype(np.uint16)


class Cube:
    """N and Q (uint16 [N, N, N, 3] indexed [b, g, r], channels R, G, B), immutable and hashable: equal to, and hashing with, exactly the
    cubes of the same N and the same Q bytes."""
    __slots__ = ('n', 'q', '_key')

    def __init__(self, n, q):
        n, q = int(n), np.array(q, dtype=np.uint16, order='C')           # a copy of its own
        if not MIN_N <= n <= MAX_N or q.shape != (n, n, n, 3):
            raise ValueError('Cube: N in %d..%d and Q uint16 [N, N, N, 3] expected, got N=%r and %s' % (MIN_N, MAX_N, n, q.shape))
        q.setflags(write=False)
        object.__setattr__(self, 'n', n)
        object.__setattr__(self, 'q', q)
        object.__setattr__(self, '_key', (n, q.astype('<u2').tobytes()))

    def __setattr__(self, name, value=None):
        raise AttributeError('a Cube is immutable')

    __delattr__ = __setattr__

    def __eq__(self, other):
        return isinstance(other, Cube) and self._key == other._key

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return 'Cube(n=%d, q=<%08x>)' % (self.n, hash(self._key) & 0xffffffff)

    @classmethod
    def of_table(cls, table):
        """The cube of a float table [N, N, N, 3] (``parse_cube``'s)."""
        return cls(len(table), quantise(table))

    @classmethod
    def of_text(cls, text):
        n, table = parse_cube(text)
        return cls(n, quantise(table))


def identity_table(n):
    """The float table of the identity cube of size n: the lattice point (r, g, b) maps to (r, g, b) / (n - 1)."""
    b, g, r = np.meshgrid(*[np.arange(n, dtype=np.float64) / (n - 1)] * 3, indexing='ij')
    return np.stack([r, g, b], axis=-1)


def cube_text(table, title=None):
    """The ``.cube`` text of a float table [N, N, N, 3], 17 significant digits: ``parse_cube`` reads the same float64 values back."""
    table = np.asarray(table, np.float64)
    head = (['TITLE "%s"' % title] if title else []) + ['LUT_3D_SIZE %d' % len(table)]
    return '\n'.join(head + ['%.17g %.17g %.17g' % tuple(row) for row in table.reshape(-1, 3)]) + '\n'


def load_cube(path):
    """The ``Cube`` of the file ``path``; ValueError with the file's name for one that cannot be read or does not parse."""
    try:
        with open(path, 'r', encoding='utf-8', errors='replace') as f:
            text = f.read()
    except OSError as e:
        raise ValueError('--lut %s: %s' % (path, e.strerror or e))
    try:
        return Cube.of_text(text)
    except ValueError as e:
        raise ValueError('--lut %s: %s' % (path, e))


def check_depth(depth):
    """The LUT at the working depth ``depth``: 8, 10 or 12, the limit of ``--linear-light`` and for its reason: the reused gather keeps its
    table of at most 4096 entries in LDS."""
    if depth not in (8, 10, 12):
        raise ValueError('--lut needs a working depth of 8, 10 or 12 bits, got %r: the gather in front of it keeps its table of at most '
                         '%d entries in LDS, as for --linear-light; work at %d bits or below (--work-depth)'
                         % (depth, 1 << MAX_DEPTH, MAX_DEPTH))
    return depth


def code_table(depth):
    """e[c] = (2 * 65535 * c + peak) // (2 * peak), uint16 [peak + 1]: the 16-bit value of code c, rounded half up."""
    peak = (1 << check_depth(depth)) - 1
    c = np.arange(peak + 1, dtype=np.int64)
    e = (2 * PEAK * c + peak) // (2 * peak)
    assert e[0] == 0 and e[peak] == PEAK and (np.diff(e) > 0).all()
    return e.astype(np.uint16)


def axis(u, n):
    """The 16-bit coordinate(s) u -> (idx, frac) on an axis of n lattice points, int64."""
    p = np.asarray(u, np.int64) * (n - 1)
    idx = np.minimum(p // PEAK, n - 2)
    return idx, p - PEAK * idx


def axis_table(depth, n):
    """Per working-depth code c the word idx << 16 | frac of axis(e[c], n), uint32 [peak + 1]: the kernel divides nothing by n - 1."""
    idx, frac = axis(code_table(depth), n)
    return ((idx << 16) | frac).astype(np.uint32)


def cube_words(cube):
    """The cube as the kernel reads it: uint16 [N^3, 4] = (R, G, B, 0) of lattice point r + N g + N^2 b, one 8-byte word a point."""
    out = np.zeros((cube.n ** 3, 4), np.uint16)
    out[:, :3] = cube.q.reshape(-1, 3)
    return out


def div65535(n):
    """floor(n / 65535) for 0 <= n <= 65535^2 + 32767 in the kernel's form: uint32 shifts and adds that never leave 32 bits."""
    n = np.asarray(n, np.uint64)
    t = n + (n >> np.uint64(16)) + np.uint64(1)
    assert (t < (1 << 32)).all()
    return (t >> np.uint64(16)).astype(np.int64)


def _payload(rgb):
    rgb = np.asarray(rgb)
    if rgb.dtype.itemsize != 2 or rgb.dtype.kind != 'u' or rgb.ndim != 3 or rgb.shape[0] != 3:
        raise ValueError('an RGB payload is uint16 [3,h,w], got %s %s' % (rgb.dtype, rgb.shape))
    return rgb


def cell_coords(rgb, inv_in, depth, n):
    """(idx [3, h, w], frac [3, h, w]) in the order R, G, B of the pixels of the RGB payload ``rgb`` (planes B, G, R)."""
    e = code_table(depth).astype(np.int64)
    code = np.asarray(inv_in, np.int64)[_payload(rgb)[::-1]]
    if int(code.max(initial=0)) >= len(e):
        raise ValueError('lut: inv_in holds the code %d above the peak %d' % (int(code.max()), len(e) - 1))
    return axis(e[code], n)


def lut_payload_np(rgb, inv_in, depth, cube):
    """The plane rule: the RGB payload [3, h, w] (planes B, G, R; values of the table ``inv_in`` inverts) through ``cube`` -> the RGB
    payload of 16-bit encoded values, '<u2' [3, h, w]."""
    n, q = cube.n, cube.q.astype(np.int64)
    idx, frac = cell_coords(rgb, inv_in, depth, n)                       # [3, h, w], axes R, G, B
    order = np.argsort(-frac, axis=0, kind='stable')                     # the axes by falling fraction
    f = np.take_along_axis(frac, order, axis=0)
    axes = np.arange(3)[:, None, None]
    p1 = idx + (order[0][None] == axes)
    p2 = p1 + (order[1][None] == axes)

    def at(p):                                                           # Q of the lattice points p = (r, g, b): [h, w, 3]
        return q[p[2], p[1], p[0]]
    num = (at(idx) * (PEAK - f[0])[..., None] + at(p1) * (f[0] - f[1])[..., None] + at(p2) * (f[1] - f[2])[..., None]
           + at(idx + 1) * f[2][..., None] + 32767)
    assert int(num.max(initial=0)) < 1 << 32
    out = num // PEAK                                                    # [h, w, 3] in R, G, B
    return np.ascontiguousarray(out[..., ::-1].transpose(2, 0, 1)).astype('<u2')


def lut_pixel(v, inv_in, depth, cube, swap_ties=False):
    """The scalar reading of the rule in Python integers: v = (B, G, R) values of one pixel -> (B, G, R) out.  ``swap_ties``: tied
    fractions are taken in the other order, which must not show."""
    n, e = cube.n, code_table(depth)
    fr = []
    for ch, x in zip((2, 1, 0), v):                                      # B, G, R -> axis 2, 1, 0
        u = int(e[int(inv_in[int(x)])])
        p = u * (n - 1)
        i = min(p // PEAK, n - 2)
        fr.append((p - PEAK * i, ch, i))
    fr.sort(key=lambda t: (-t[0], -t[1] if swap_ties else t[1]))
    pos = [0, 0, 0]
    for _, ch, i in fr:
        pos[ch] = i
    verts = [tuple(pos)]
    for _, ch, _ in fr[:2]:
        pos[ch] += 1
        verts.append(tuple(pos))
    verts.append(tuple(i + 1 for i in verts[0]))
    f1, f2, f3 = (t[0] for t in fr)
    ws = (PEAK - f1, f1 - f2, f2 - f3, f3)
    out = [(sum(int(cube.q[p[2], p[1], p[0], c]) * w for p, w in zip(verts, ws)) + 32767) // PEAK for c in range(3)]
    return out[2], out[1], out[0]


def tables(depth, transfer=None):
    """(gather table, inv_in) of a LUT run: ``colour.forward_table`` of the transfer in linear light, else ``code_table``, and the inverse
    of that same table."""
    fwd = code_table(depth) if transfer is None else CL.forward_table(transfer, depth)
    return fwd, CL.inverse_table(fwd)


def lut_stream_np(frames, groups, cube, depth, layout, matrix='bt601', full_range=False, transfer=None, scale=None, weights=None):
    """The written payloads of a LUT run, as uint8 byte arrays: the counterpart of ``colour.linear_stream_np`` with the LUT between the
    scale and the encode.  ``transfer`` None: the RGB payloads are made with ``code_table`` (the run is not in linear light); a transfer:
    with ``colour.forward_table``.  The encode reads the LUT's output through ``colour.inverse_table(code_table(depth))``."""
    fwd, inv_in = tables(depth, transfer)
    inv_e = CL.inverse_table(code_table(depth))
    h, w = np.asarray(frames[0]).shape[:2]
    lin = np.stack([CL.linearize_np(f, fwd).reshape(-1) for f in frames]).view(np.uint8)
    if groups is not None:
        lin = SH.mix_np(lin, groups, 2, weights)
    out = []
    for p in lin:
        p = np.ascontiguousarray(p).view('<u2')
        if scale is not None and tuple(scale[:2]) != (w, h):
            p = SC.scale_payload_np(p.astype(np.uint16), h, w, scale[1], scale[0], 16, '444', scale[2] if len(scale) > 2 else None)
            p = p.reshape(3, scale[1], scale[0])
        else:
            p = p.reshape(3, h, w)
        p = lut_payload_np(p.astype(np.uint16), inv_in, depth, cube)
        out.append(np.ascontiguousarray(CL.encode_payload_np(p, inv_e, depth, layout, matrix, full_range)).view(np.uint8))
    return out
