"""What ``demfi_payload_deblock`` refuses, without a GPU, in the manner of tests/test_payload_args.py: the entry point checks its arguments
before its first HIP call, so the statuses below come back on any machine.  One hand-written good tuple (never called as it stands: it
would launch) and a table of changes to it; the "device" pointer is an aligned integer nobody dereferences, the plane table a real array.
No tuple here reaches a launch: each is refused, or has n == 0, which is checked last and so also proves the tuple acceptable."""
from demfi_amd import deblock as DB
from tests.test_payload_args import ERR_ARG, OK, SRC, i64, nulls, run

TABLE = [list(e) for e in DB.plane_table(12, 20, '420')]              # 360 samples: luma 12 x 20, two chroma planes 6 x 10
FIELDS = [list(e) for e in DB.plane_table(12, 20, '420', 't', (4, 16, 6, 26))]


def t(p, c, v, table=TABLE):
    x = [list(e) for e in table]
    x[p][c] = v
    return i64(x)


def test_payload_deblock():
    #       payloads, stride, n, planes, n_planes, sample_bytes, a, b, s, stream
    good = (SRC, 360, 2, i64(TABLE), 3, 1, 16, 4, 6, None)
    wide16 = {1: 720, 5: 2, 6: 64, 7: 16, 8: 24}
    run('demfi_payload_deblock', good, nulls((0, 3)) + [
        ('n -1', {2: -1}, ERR_ARG),
        ('0 bytes a sample', {5: 0}, ERR_ARG, b'bytes per sample'), ('3 bytes a sample', {5: 3}, ERR_ARG, b'bytes per sample'),
        ('no plane', {4: 0}, ERR_ARG, b'planes'), ('seven planes', {4: 7, 3: i64(FIELDS + [FIELDS[0]])}, ERR_ARG, b'planes'),
        ('a plane of no rows', {3: t(1, 1, 0)}, ERR_ARG, b'plane 1'), ('a plane of no columns', {3: t(2, 2, 0)}, ERR_ARG, b'plane 2'),
        ('16385 rows', {3: t(0, 1, 16385), 1: 1 << 30}, ERR_ARG, b'plane 0'), ('16385 columns', {3: t(0, 2, 16385), 1: 1 << 30}, ERR_ARG, b'plane 0'),
        ('a side at the limit', {2: 0, 3: i64([[0, 16384, 16384, 16384, 7, 7]]), 4: 1, 1: 1 << 28}, OK),
        ('a pitch below cols', {3: t(0, 3, 19)}, ERR_ARG, b'pitch'), ('a pitch below cols in a chroma plane', {3: t(2, 3, 9)}, ERR_ARG, b'pitch'),
        ('an x phase of 8', {3: t(0, 4, 8)}, ERR_ARG, b'phases'), ('an x phase of -1', {3: t(1, 4, -1)}, ERR_ARG, b'phases'),
        ('a y phase of 8', {3: t(2, 5, 8)}, ERR_ARG, b'phases'), ('a y phase of -1', {3: t(0, 5, -1)}, ERR_ARG, b'phases'),
        ('a plane that starts below the payload', {3: t(0, 0, -1)}, ERR_ARG, b'starts'),
        ('a stride one byte short', {1: 359}, ERR_ARG, b'stride'), ('a stride one byte short of 16-bit payloads', {**wide16, 1: 718}, ERR_ARG, b'stride'),
        ('a plane that ends behind the stride', {3: t(2, 0, 301)}, ERR_ARG, b'stride'),
        ('a pitch that carries the last row behind the stride', {3: t(2, 3, 11)}, ERR_ARG, b'stride'),
        ('16 bits, odd base', {**wide16, 0: SRC + 1}, ERR_ARG, b'odd'), ('16 bits, odd stride', {**wide16, 1: 721}, ERR_ARG, b'odd'),
        ('a below 0', {6: -1, 7: -1}, ERR_ARG, b'thresholds'), ('b below 0', {7: -1}, ERR_ARG, b'thresholds'), ('b above a', {7: 17}, ERR_ARG, b'thresholds'),
        ('a above the peak of a byte', {6: 256}, ERR_ARG, b'thresholds'), ('a above the peak of 16 bits', {**wide16, 6: 65536}, ERR_ARG, b'thresholds'),
        ('s below 0', {8: -1}, ERR_ARG, b'thresholds'), ('s above the peak of a byte', {8: 256}, ERR_ARG, b'thresholds'),
        ('n 0', {2: 0}, OK), ('n 0, 16 bits', {**wide16, 2: 0}, OK), ('n 0, fields and phases', {2: 0, 3: i64(FIELDS), 4: 6}, OK),
        ('n 0, a = 0', {2: 0, 6: 0, 7: 0, 8: 2}, OK), ('n 0, a wider stride', {2: 0, 1: 1000}, OK), ('n 0, an odd base of bytes', {2: 0, 0: SRC + 3, 1: 361}, OK),
        ('n 0 after the checks', {2: 0, 5: 3}, ERR_ARG), ('n 0 after the table', {2: 0, 3: t(0, 4, 9)}, ERR_ARG),
    ])
