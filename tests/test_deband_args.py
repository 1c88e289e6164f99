"""What ``demfi_payload_deband`` refuses, without a GPU, in the manner of tests/test_dering_args.py: the entry point checks its arguments
before its first HIP call, so the statuses below come back on any machine.  One hand-written good tuple (never called as it stands: it
would launch) and a table of changes to it; the "device" pointers are aligned integers nobody dereferences, the plane table a real array.
No tuple here reaches a launch: each is refused, or has n == 0, which is checked last and so also proves the tuple acceptable."""
from demfi_amd import deblock as DB
from tests.test_payload_args import DST, ERR_ARG, OK, SRC, i64, nulls, run

TABLE = [list(e) for e in DB.plane_table(12, 20, '420')]              # 360 samples: luma 12 x 20, two chroma planes 6 x 10
FIELDS = [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))]


def t(p, c, v, table=TABLE):
    x = [list(e) for e in table]
    x[p][c] = v
    return i64(x)


def test_payload_deband():
    #       src, src_stride, dst, dst_stride, n, planes, n_planes, sample_bytes, depth, thr8, radius, stream
    good = (SRC, 360, DST, 360, 2, i64(TABLE), 3, 1, 8, 2, 16, None)
    wide16 = {1: 720, 3: 720, 7: 2, 8: 10}
    run('demfi_payload_deband', good, nulls((0, 2, 5)) + [
        ('n -1', {4: -1}, ERR_ARG),
        ('0 bytes a sample', {7: 0}, ERR_ARG, b'bytes per sample'), ('3 bytes a sample', {7: 3}, ERR_ARG, b'bytes per sample'),
        ('9 bits', {**wide16, 8: 9}, ERR_ARG, b'depth'), ('7 bits', {8: 7}, ERR_ARG, b'depth'), ('18 bits', {**wide16, 8: 18}, ERR_ARG, b'depth'),
        ('10 bits in bytes', {8: 10}, ERR_ARG, b'depth'), ('16 bits in bytes', {8: 16}, ERR_ARG, b'depth'),
        ('T -1', {9: -1}, ERR_ARG, b'window'), ('T 9', {9: 9}, ERR_ARG, b'window'), ('R 0', {10: 0}, ERR_ARG, b'window'),
        ('R -1', {10: -1}, ERR_ARG, b'window'), ('R 17', {10: 17}, ERR_ARG, b'window'),
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
        ('in place, the identity', {2: SRC, 9: 0}, ERR_ARG, b'overlap'),
        ('strides that leave the address space', {1: 1 << 62, 3: 1 << 62, 4: 8}, ERR_ARG, b'address space'),
        ('n 0', {4: 0}, OK), ('n 0, 16 bits', {**wide16, 4: 0}, OK), ('n 0, 8 bits in 16', {**wide16, 8: 8, 4: 0}, OK),
        ('n 0, fields and phases', {4: 0, 5: i64(FIELDS), 6: 6}, OK),
        ('n 0, the corners of the window', {4: 0, 9: 8, 10: 1}, OK), ('n 0, the other corners', {4: 0, 9: 1, 10: 16}, OK),
        ('n 0, the identity', {4: 0, 9: 0, 10: 16}, OK), ('n 0, 16 bits at T 8', {**wide16, 8: 16, 4: 0, 9: 8}, OK),
        ('n 0, wider strides', {4: 0, 1: 1000, 3: 377}, OK), ('n 0, odd bases of bytes', {4: 0, 0: SRC + 3, 2: DST + 5, 1: 361}, OK),
        ('n 0, dst directly behind src', {4: 0, 2: SRC + 720}, OK),
        ('n 0 after the checks', {4: 0, 7: 3}, ERR_ARG), ('n 0 after the table', {4: 0, 5: t(0, 4, 9)}, ERR_ARG),
        ('n 0 after the window', {4: 0, 9: 9}, ERR_ARG), ('n 0 after the radius', {4: 0, 10: 17}, ERR_ARG),
    ])
