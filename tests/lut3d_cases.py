"""The cubes and the inputs of the 3D LUT's kernel tests, shared by tests/test_gpu_lut3d.py, which runs them on the GPU, and
tests/test_lut3d.py, which proves on the CPU what they reach (every ordering of the fractions, every tie, the top of every axis, every
face of the lattice).  Everything here is numpy; nothing needs a GPU."""
import numpy as np

from demfi_amd import colour as CL
from demfi_amd import lut3d as LU

SIZES = [(6, 10), (17, 33), (33, 70)]                # one strip and a cut one; widths off the 8-pixel strip, more than one block at 33x70
NS = [2, 3, 17, 33, 65]
DEPTHS = [8, 10, 12]
ENUM_SHAPE = {8: (16, 16), 10: (32, 32), 12: (64, 64)}      # peak + 1 pixels


def cubes(n):
    """name -> ``Cube`` of size n: the identity, a seeded random one, all zero, all 65535, a checkerboard of 0 and 65535."""
    r = np.arange(n)
    checker = ((r[:, None, None] + r[None, :, None] + r[None, None, :]) & 1) * 65535
    return {'identity': LU.Cube.of_table(LU.identity_table(n)),
            'random': LU.Cube(n, np.random.default_rng(1000 + n).integers(0, 65536, (n, n, n, 3))),
            'zero': LU.Cube(n, np.zeros((n, n, n, 3), np.uint16)),
            'full': LU.Cube(n, np.full((n, n, n, 3), 65535, np.uint16)),
            'checker': LU.Cube(n, np.repeat(checker[..., None], 3, axis=-1))}


def table_pairs(depth):
    """name -> (the table the payloads are made with, its inverse = the LUT's inv_in): ``code_table`` and each transfer's."""
    return {'e': LU.tables(depth), **{t: LU.tables(depth, t) for t in CL.TRANSFERS}}


def enum_codes(depth):
    """Seven frames of codes [3, hh, ww] (planes B, G, R) that hold peak + 1 pixels each: every code on each axis against fixed other axes
    (the fixed ones: the peak, which is the top of its axis, and a third of it), then every code on the diagonal of each pair of axes
    against a fixed third (two fractions tie) and on the main diagonal (all three tie)."""
    peak = (1 << depth) - 1
    c, shape = np.arange(peak + 1), ENUM_SHAPE[depth]
    fixed = [np.full(peak + 1, peak), np.full(peak + 1, peak // 3), np.full(peak + 1, 0)]
    out = []
    for a in range(3):                               # axis a runs, the two others stay
        planes = [fixed[(a + 1 + j) % 3] for j in range(3)]
        planes[a] = c
        out.append(np.stack(planes))
    for a in range(3):                               # the pair without axis a runs together
        planes = [c, c, c]
        planes[a] = fixed[(a + 1) % 3]
        out.append(np.stack(planes))
    out.append(np.stack([c, c, c]))
    return [f.reshape((3,) + shape) for f in out]


def random_codes(depth, h, w, m=3):
    """m random frames of codes [3, h, w]; the last holds only 0 and the peak, so every corner of the cube is met."""
    peak = (1 << depth) - 1
    rng = np.random.default_rng(depth * 1000 + h * 31 + w)
    f = rng.integers(0, peak + 1, (m, 3, h, w))
    f[m - 1] = rng.integers(0, 2, (3, h, w)) * peak
    return list(f)


def payloads(codes, fwd):
    """Frames of codes -> RGB payloads uint16 [m, 3, h, w] through the table ``fwd``."""
    return np.asarray(fwd, np.uint16)[np.stack(codes)]


def launches(depth):
    """[(h, w, codes of the launch's payloads)] of one depth: the enumerations in one launch, the random frames of each size in one."""
    hh, ww = ENUM_SHAPE[depth]
    return [(hh, ww, enum_codes(depth))] + [(h, w, random_codes(depth, h, w)) for h, w in SIZES]
