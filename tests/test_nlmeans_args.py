"""What ``demfi_payload_nlmeans`` refuses, without a GPU, in the manner of tests/test_deband_args.py: the entry point checks its arguments
before its first HIP call, so the statuses below come back on any machine.  One hand-written good tuple (never called as it stands: it
would launch) and a table of changes to it; the "device" pointers are aligned integers nobody dereferences, the plane table and the weight
table real arrays.  No tuple here reaches a launch: each is refused, or has n == 0, which is checked last and so also proves the tuple
acceptable."""
import numpy as np

from demfi_amd import deblock as DB
from demfi_amd import nlmeans as NL
from tests.test_payload_args import DST, ERR_ARG, KEEP, OK, SRC, i64, nulls, run

TABLE = [list(e) for e in DB.plane_table(12, 20, '420')]              # 360 samples: luma 12 x 20, two chroma planes 6 x 10
FIELDS = [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))]
WEIGHTS, SHIFT = NL.weight_table(8, 3, 2)


def u16(x):
    KEEP.append(np.ascontiguousarray(x, np.uint16))
    return KEEP[-1].ctypes.data


def t(p, c, v, table=TABLE):
    x = [list(e) for e in table]
    x[p][c] = v
    return i64(x)


def wt(k, v):
    x = WEIGHTS.copy()
    x[k] = v
    return u16(x)


def test_payload_nlmeans():
    #       src, src_stride, dst, dst_stride, n, planes, n_planes, sample_bytes, depth, patch, search, table, shift, stream
    good = (SRC, 360, DST, 360, 2, i64(TABLE), 3, 1, 8, 2, 5, u16(WEIGHTS), SHIFT, None)
    wide16 = {1: 720, 3: 720, 7: 2, 8: 10}
    run('demfi_payload_nlmeans', good, nulls((0, 2, 5, 11)) + [
        ('n -1', {4: -1}, ERR_ARG),
        ('0 bytes a sample', {7: 0}, ERR_ARG, b'bytes per sample'), ('3 bytes a sample', {7: 3}, ERR_ARG, b'bytes per sample'),
        ('9 bits', {**wide16, 8: 9}, ERR_ARG, b'depth'), ('7 bits', {8: 7}, ERR_ARG, b'depth'), ('18 bits', {**wide16, 8: 18}, ERR_ARG, b'depth'),
        ('10 bits in bytes', {8: 10}, ERR_ARG, b'depth'), ('16 bits in bytes', {8: 16}, ERR_ARG, b'depth'),
        ('P 0', {9: 0}, ERR_ARG, b'window'), ('P -1', {9: -1}, ERR_ARG, b'window'), ('P 4', {9: 4}, ERR_ARG, b'window'),
        ('R 0', {10: 0}, ERR_ARG, b'window'), ('R -1', {10: -1}, ERR_ARG, b'window'), ('R 8', {10: 8}, ERR_ARG, b'window'),
        ('shift -1', {12: -1}, ERR_ARG, b'window'), ('shift 32', {12: 32}, ERR_ARG, b'window'),
        ('a table that starts at 255', {11: wt(0, 255)}, ERR_ARG, b'table[0]'), ('a table that starts at 257', {11: wt(0, 257)}, ERR_ARG, b'table[0]'),
        ('a table that starts at 0', {11: u16(np.zeros(1024))}, ERR_ARG, b'table[0]'),
        ('an entry above 256', {11: u16(np.r_[256, 300, np.zeros(1022)])}, ERR_ARG, b'table[1]'),
        ('an entry that increases', {11: wt(700, int(WEIGHTS[699]) + 1)}, ERR_ARG, b'table[700]'),
        ('a last entry that increases', {11: wt(1023, 1)}, ERR_ARG, b'table[1023]'),
        ('no plane', {6: 0}, ERR_ARG, b'planes'), ('seven planes', {6: 7, 5: i64(FIELDS + [FIELDS[0]])}, ERR_ARG, b'planes'),
        ('a plane of no rows', {5: t(1, 1, 0)}, ERR_ARG, b'plane 1'), ('a plane of no columns', {5: t(2, 2, 0)}, ERR_ARG, b'plane 2'),
        ('16385 rows', {5: t(0, 1, 16385), 1: 1 << 30, 3: 1 << 30}, ERR_ARG, b'plane 0'),
        ('16385 columns', {5: t(0, 2, 16385), 1: 1 << 30, 3: 1 << 30}, ERR_ARG, b'plane 0'),
        ('a side at the limit', {4: 0, 5: i64([[0, 16384, 16384, 16384, 7, 7]]), 6: 1, 1: 1 << 28, 3: 1 << 28}, OK),
        ('a pitch below cols', {5: t(0, 3, 19)}, ERR_ARG, b'pitch'), ('a pitch below cols in a chroma plane', {5: t(2, 3, 9)}, ERR_ARG, b'pitch'),
        ('an x phase of 8', {5: t(0, 4, 8)}, ERR_ARG, b'phases'), ('an x phase of -1', {5: t(1, 4, -1)}, ERR_ARG, b'phases'),
        ('a y phase of 8', {5: t(2, 5, 8)}, ERR_ARG, b'phases'), ('a y phase of -1', {5: t(0, 5, -1)}, ERR_ARG, b'phases'),
        ('a plane that starts below the payload', {5: t(0, 0, -1)}, ERR_ARG, b'starts'),
        ('a src stride one byte short', {1: 359}, ERR_ARG, b'src_stride'), ('a dst stride one byte short', {3: 359}, ERR_ARG, b'dst_stride'),
        ('a stride one byte short of 16-bit payloads', {**wide16, 3: 718}, ERR_ARG, b'stride'),
        ('a plane that ends behind the stride', {5: t(2, 0, 301)}, ERR_ARG, b'stride'),
        ('a pitch that carries the last row behind the stride', {5: t(2, 3, 11)}, ERR_ARG, b'stride'),
        ('16 bits, odd src', {**wide16, 0: SRC + 1}, ERR_ARG, b'odd'), ('16 bits, odd dst', {**wide16, 2: DST + 1}, ERR_ARG, b'odd'),
        ('16 bits, odd src stride', {**wide16, 1: 721}, ERR_ARG, b'odd'), ('16 bits, odd dst stride', {**wide16, 3: 721}, ERR_ARG, b'odd'),
        ('in place', {2: SRC}, ERR_ARG, b'overlap'), ('dst inside the last source payload', {2: SRC + 360 + 359}, ERR_ARG, b'overlap'),
        ('src inside the last destination payload', {0: DST + 719}, ERR_ARG, b'overlap'),
        ('dst between two source payloads', {1: 2000, 2: SRC + 400, 3: 400}, ERR_ARG, b'overlap'),
        ('in place, the identity table', {2: SRC, 11: u16(np.r_[256, np.zeros(1023)])}, ERR_ARG, b'overlap'),
        ('strides that leave the address space', {1: 1 << 62, 3: 1 << 62, 4: 8}, ERR_ARG, b'address space'),
        ('n 0', {4: 0}, OK), ('n 0, 16 bits', {**wide16, 4: 0}, OK), ('n 0, 8 bits in 16', {**wide16, 8: 8, 4: 0}, OK),
        ('n 0, fields and phases', {4: 0, 5: i64(FIELDS), 6: 6}, OK),
        ('n 0, the corners of the window', {4: 0, 9: 1, 10: 7}, OK), ('n 0, the other corners', {4: 0, 9: 3, 10: 1}, OK),
        ('n 0, the widest window and shift', {4: 0, 9: 3, 10: 7, 12: 31}, OK), ('n 0, no shift', {4: 0, 12: 0}, OK),
        ('n 0, the identity table', {4: 0, 11: u16(np.r_[256, np.zeros(1023)])}, OK), ('n 0, the box table', {4: 0, 11: u16(np.full(1024, 256))}, OK),
        ('n 0, 16 bits at 16:3', {**wide16, 8: 16, 4: 0, 9: 3, 11: u16(NL.weight_table(16, 16, 3)[0]), 12: NL.weight_table(16, 16, 3)[1]}, OK),
        ('n 0, wider strides', {4: 0, 1: 1000, 3: 377}, OK), ('n 0, odd bases of bytes', {4: 0, 0: SRC + 3, 2: DST + 5, 1: 361}, OK),
        ('n 0, dst directly behind src', {4: 0, 2: SRC + 720}, OK),
        ('n 0 after the checks', {4: 0, 7: 3}, ERR_ARG), ('n 0 after the plane table', {4: 0, 5: t(0, 4, 9)}, ERR_ARG),
        ('n 0 after the patch', {4: 0, 9: 4}, ERR_ARG), ('n 0 after the search', {4: 0, 10: 8}, ERR_ARG),
        ('n 0 after the weights', {4: 0, 11: wt(5, 257)}, ERR_ARG),
    ])
