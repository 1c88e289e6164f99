"""What ``demfi_rgb_lut3d`` refuses, without a GPU, in the manner of tests/test_payload_args.py: the entry point checks its arguments before
its first HIP call, so the statuses below come back on any machine.  One hand-written good tuple (never called as it stands: it would
launch) and a table of changes to it; the "device" pointers are aligned integers nobody dereferences, the offset table a real array.  No
tuple here reaches a launch: each is refused, or has n == 0, which is checked last and so also proves the tuple acceptable."""
from tests.test_payload_args import AUX, DST, ERR_ARG, OK, SRC, TAB, i64, nulls, run

INV, CUBE, AXT = AUX, AUX + 0x1000, AUX + 0x2000                     # 16-byte aligned; 4 x 4 frames: payloads of 96 bytes


def test_rgb_lut3d():
    #       src, offsets, offsets_dev, n, h, w, depth, inv_in, cube_n, cube, axis_table, cube_in_lds, dst, dst_stride, stream
    good = (SRC, i64([0, 96]), TAB, 2, 4, 4, 8, INV, 17, CUBE, AXT, 0, DST, 96, None)
    run('demfi_rgb_lut3d', good, nulls((0, 1, 2, 7, 9, 10, 12)) + [
        ('n -1', {3: -1}, ERR_ARG),
        ('one row', {4: 1}, ERR_ARG, b'frame size'), ('one column', {5: 1}, ERR_ARG, b'frame size'),
        ('16385 rows', {4: 16385, 13: 1 << 30}, ERR_ARG, b'frame size'), ('16385 columns', {5: 16385, 13: 1 << 30}, ERR_ARG, b'frame size'),
        ('9 bits', {6: 9}, ERR_ARG, b'depth'), ('14 bits', {6: 14}, ERR_ARG, b'depth'), ('16 bits', {6: 16}, ERR_ARG, b'depth'),
        ('0 bits', {6: 0}, ERR_ARG, b'depth'),
        ('a cube of 1', {8: 1}, ERR_ARG, b'cube size'), ('a cube of 66', {8: 66}, ERR_ARG, b'cube size'), ('a cube of -3', {8: -3}, ERR_ARG, b'cube size'),
        ('cube_in_lds 2', {11: 2}, ERR_ARG, b'cube_in_lds'), ('cube_in_lds -1', {11: -1}, ERR_ARG, b'cube_in_lds'),
        ('a cube of 18 in LDS', {8: 18, 11: 1}, ERR_ARG, b'cube_in_lds'), ('a cube of 65 in LDS', {8: 65, 11: 1}, ERR_ARG, b'cube_in_lds'),
        ('axis_table off a word', {10: AXT + 2}, ERR_ARG, b'boundary'), ('cube off 8 bytes', {9: CUBE + 4}, ERR_ARG, b'boundary'),
        ('dst_stride one sample short', {13: 94}, ERR_ARG, b'dst_stride'),
        ('a negative offset', {1: i64([0, -2])}, ERR_ARG), ('an absent payload', {1: i64([-1, 96])}, ERR_ARG),
        ('an odd src', {0: SRC + 1}, ERR_ARG, b'odd'), ('an odd offset', {1: i64([0, 97])}, ERR_ARG, b'odd'),
        ('an odd inv_in', {7: INV + 1}, ERR_ARG, b'odd'), ('an odd dst', {12: DST + 1}, ERR_ARG, b'odd'),
        ('an odd stride', {13: 97}, ERR_ARG, b'odd'),
        ('in place', {12: SRC}, ERR_ARG, b'overlap'), ('dst inside the last source payload', {12: SRC + 96 + 94}, ERR_ARG, b'overlap'),
        ('src inside the last destination payload', {0: DST + 190}, ERR_ARG, b'overlap'),
        ('dst between two source payloads', {1: i64([0, 1000]), 12: SRC + 400}, ERR_ARG, b'overlap'),
        ('a stride that leaves the address space', {13: 1 << 62}, ERR_ARG, b'address space'),
        ('an offset that leaves the address space', {1: i64([0, (1 << 63) - 2])}, ERR_ARG, b'address space'),
        ('n 0', {3: 0}, OK), ('n 0, 12 bits, the largest cube', {3: 0, 6: 12, 8: 65}, OK), ('n 0, the smallest cube in LDS', {3: 0, 8: 2, 11: 1}, OK),
        ('n 0, a cube of 17 in LDS at 10 bits', {3: 0, 6: 10, 11: 1}, OK), ('n 0, a wider stride', {3: 0, 13: 1000}, OK),
        ('n 0, dst directly behind src', {3: 0, 12: SRC + 192}, OK), ('n 0, in place: nothing is written', {3: 0, 12: SRC}, OK),
        ('n 0, the largest frame', {3: 0, 4: 16384, 5: 16384, 13: 6 << 28}, OK),
        ('n 0 after the checks', {3: 0, 6: 9}, ERR_ARG), ('n 0 after the cube', {3: 0, 8: 66}, ERR_ARG), ('n 0 after the stride', {3: 0, 13: 94}, ERR_ARG),
        ('n 0 after the offsets', {3: 0, 12: DST + 1}, ERR_ARG),
    ])
