"""What the entry points of the Y4M stages refuse, without a GPU: every ``demfi_payload_*`` entry point, the two deinterlacers and the
four luma statistics check their arguments before their first HIP call, so the statuses below come back on any machine.  Each entry
has one hand-written good tuple (never called as it stands: it would launch) and a table of changes to it with the status the entry
specifies.  "Device" pointers are aligned integers nobody dereferences; the offset tables, plane lists and weights are real arrays.
No tuple here reaches a launch: each is refused, or has n <= 0 (where n == 0 is checked last, it also proves the tuple acceptable)."""
import numpy as np

from demfi_amd import _lib as L

OK, ERR_ARG = 0, -1
SRC, DST, TAB, AUX = 0x10000, 0x20000, 0x30000, 0x40000              # "device" addresses, 16-byte aligned
KEEP = []                                                            # the arrays the tuples point into


def i64(x):
    KEEP.append(np.ascontiguousarray(x, np.int64))
    return KEEP[-1].ctypes.data


def i32(x):
    KEEP.append(np.ascontiguousarray(x, np.int32))
    return KEEP[-1].ctypes.data


def u32(x):
    KEEP.append(np.ascontiguousarray(x, np.uint32))
    return KEEP[-1].ctypes.data


def run(name, good, cases):
    """cases: (what, {argument index: value}, status[, a word the message must hold])"""
    lib = L.load()
    fn = getattr(lib, name)
    for what, changes, want, *word in cases:
        a = list(good)
        for i, v in changes.items():
            a[i] = v
        got = fn(*a)
        msg = lib.demfi_last_error()
        assert got == want, (name, what, got, msg)
        if want == ERR_ARG:
            assert name.encode() in msg, (name, what, msg)
            assert all(w in msg for w in word), (name, what, msg)


def nulls(idx):
    return [('argument %d NULL' % i, {i: None}, ERR_ARG) for i in idx]


PLANES = [[4, 16], [2, 8], [2, 8]]                                   # 4:2:0, 96 samples a payload


# ---- shutter -----------------------------------------------------------------------------------------------------------------------
def mix_cases(n, smax, P, sb, dst, stride, tab):
    return [
        ('smax 0', {smax: 0}, ERR_ARG), ('smax 33', {smax: 33}, ERR_ARG), ('P 0', {P: 0}, ERR_ARG),
        ('0 bytes a sample', {sb: 0}, ERR_ARG), ('3 bytes a sample', {sb: 3}, ERR_ARG),
        ('dst_stride one byte short', {stride: 15}, ERR_ARG),
        ('a row that keeps nothing', {tab: i64([[0, 32, -1], [-1, -1, -1]])}, ERR_ARG),
        ('a kept offset behind a -1', {tab: i64([[0, -1, 32], [64, -1, -1]])}, ERR_ARG),
        ('a negative offset', {tab: i64([[0, 32, -2], [64, -1, -1]])}, ERR_ARG),
        ('16 bits, odd base', {0: SRC + 1, P: 8, sb: 2}, ERR_ARG),
        ('16 bits, odd offset', {tab: i64([[0, 33, -1], [64, -1, -1]]), P: 8, sb: 2}, ERR_ARG),
        ('16 bits, odd dst', {dst: DST + 1, P: 8, sb: 2}, ERR_ARG),
        ('16 bits, odd stride', {stride: 17, P: 8, sb: 2}, ERR_ARG),
        ('n 0', {n: 0}, OK), ('n 0 before every check', {n: 0, 0: None, sb: 7}, OK), ('n -1', {n: -1, 0: None}, OK),
    ]


def test_payload_mix():
    good = (SRC, i64([[0, 32, -1], [64, -1, -1]]), TAB, 2, 3, 16, 1, DST, 32, None)
    run('demfi_payload_mix', good, nulls((0, 1, 2, 7)) + mix_cases(3, 4, 5, 6, 7, 8, 1))


def test_payload_mix_w():
    good = (SRC, i64([[0, 32, -1], [64, -1, -1]]), TAB, 2, 3, 16, 1, DST, 32, i32([1, 2, 1]), None)
    run('demfi_payload_mix_w', good, nulls((0, 1, 2, 7, 9)) + mix_cases(3, 4, 5, 6, 7, 8, 1) + [
        ('weight 0', {9: i32([1, 0, 1])}, ERR_ARG), ('weight 4097', {9: i32([4097, 1, 1])}, ERR_ARG),
        ('weights summing to 4097', {9: i32([2000, 2000, 97])}, ERR_ARG)])


# ---- interlace ---------------------------------------------------------------------------------------------------------------------
def test_payload_weave():
    good = (SRC, i64([[0, 96], [192, 288]]), TAB, 2, i32(PLANES), 3, 1, 255, 0, 1, DST, 96, None)
    big = 32768 * 16 + 2 * 2 * 8
    run('demfi_payload_weave', good, nulls((0, 1, 2, 4, 10)) + [
        ('0 bytes a sample', {6: 0}, ERR_ARG), ('3 bytes a sample', {6: 3}, ERR_ARG),
        ('peak 0', {7: 0}, ERR_ARG), ('peak 256 in bytes', {7: 256}, ERR_ARG), ('peak 65536', {6: 2, 7: 65536, 11: 192}, ERR_ARG),
        ('no plane', {5: 0}, ERR_ARG), ('four planes', {5: 4, 4: i32(PLANES + [[2, 8]])}, ERR_ARG),
        ('a side above the limit', {4: i32([[32769, 16], [2, 8], [2, 8]]), 11: big + 16}, ERR_ARG, b'plane'),
        ('a side at the limit passes the plane check', {4: i32([[32768, 16], [2, 8], [2, 8]]), 11: big - 1}, ERR_ARG, b'dst_stride'),
        ('a side of 0', {4: i32([[4, 0], [2, 8], [2, 8]])}, ERR_ARG),
        ('a negative offset', {1: i64([[0, 96], [192, -2]])}, ERR_ARG), ('an absent payload', {1: i64([[0, 96], [-1, 288]])}, ERR_ARG),
        ('dst_stride one byte short', {11: 95}, ERR_ARG), ('q0 2', {8: 2}, ERR_ARG), ('low-pass 3', {9: 3}, ERR_ARG),
        ('low-pass -1', {9: -1}, ERR_ARG),
        ('16 bits, odd base', {0: SRC + 1, 6: 2, 7: 1023, 11: 192}, ERR_ARG),
        ('16 bits, odd offset', {1: i64([[0, 97], [192, 288]]), 6: 2, 7: 1023, 11: 192}, ERR_ARG),
        ('16 bits, odd dst', {10: DST + 1, 6: 2, 7: 1023, 11: 192}, ERR_ARG),
        ('16 bits, odd stride', {6: 2, 7: 1023, 11: 193}, ERR_ARG),
        ('n 0', {3: 0}, OK), ('n 0 before every check', {3: 0, 0: None, 6: 7}, OK), ('n -1', {3: -1, 4: None}, OK),
    ])


# ---- bit depth ---------------------------------------------------------------------------------------------------------------------
def depth_cases(dst, stride, up):
    d_in, d_out, b_in, b_out = (8, 10, 1, 2) if up else (10, 8, 2, 1)
    wide16 = {6: 2, 7: 2, 8: 10 if up else 12, 9: 12 if up else 10, stride: 192}
    return [
        ('bytes that do not fit the depth, in', {6: 3 - b_in}, ERR_ARG), ('and out', {7: 3 - b_out}, ERR_ARG),
        ('0 bytes a sample', {6: 0}, ERR_ARG), ('3 bytes a sample', {7: 3}, ERR_ARG),
        ('9 bits', {8 if up else 9: 9}, ERR_ARG), ('the wrong way', {6: b_out, 7: b_in, 8: d_out, 9: d_in}, ERR_ARG),
        ('the same depth', {7: b_in, 9: d_in}, ERR_ARG),
        ('no plane', {5: 0}, ERR_ARG), ('four planes', {5: 4, 4: i32(PLANES + [[2, 8]])}, ERR_ARG),
        ('a side above the limit', {4: i32([[(1 << 20) + 1, 1]]), 5: 1, stride: 1 << 22}, ERR_ARG),
        ('a side at the limit', {3: 0, 4: i32([[1 << 20, 1]]), 5: 1, stride: 1 << 22}, OK),
        ('a plane above 2^30 samples', {4: i32([[(1 << 15) + 1, 1 << 15]]), 5: 1, stride: 1 << 32}, ERR_ARG),
        ('a plane of 2^30 samples', {3: 0, 4: i32([[1 << 15, 1 << 15]]), 5: 1, stride: 1 << 32}, OK),
        ('a negative offset', {1: i64([0, -2])}, ERR_ARG), ('an absent payload', {1: i64([-1, 96])}, ERR_ARG),
        ('dst_stride one byte short', {stride: 96 * b_out - 1}, ERR_ARG), ('full_range 2', {10: 2}, ERR_ARG),
        ('16 bits in, odd base', {**wide16, 0: SRC + 1}, ERR_ARG),
        ('16 bits in, odd offset', {**wide16, 1: i64([0, 193])}, ERR_ARG),
        ('16 bits out, odd dst', {**wide16, dst: DST + 1}, ERR_ARG),
        ('16 bits out, odd stride', {**wide16, stride: 193}, ERR_ARG),
        ('n 0', {3: 0}, OK), ('n 0 after the checks', {3: 0, 10: 2}, ERR_ARG), ('n -1', {3: -1}, ERR_ARG),
    ]


def test_payload_promote():
    good = (SRC, i64([0, 96]), TAB, 2, i32(PLANES), 3, 1, 2, 8, 10, 0, DST, 192, None)
    run('demfi_payload_promote', good, nulls((0, 1, 2, 4, 11)) + depth_cases(11, 12, True))


def test_payload_requant():
    good = (SRC, i64([0, 192]), TAB, 2, i32(PLANES), 3, 2, 1, 10, 8, 0, 1, 0, DST, 96, None)
    run('demfi_payload_requant', good, nulls((0, 1, 2, 4, 13)) + depth_cases(13, 14, False) + [
        ('dither 2', {11: 2}, ERR_ARG), ('field_rows 2', {12: 2}, ERR_ARG), ('16 bits in, odd offset at 10 -> 8', {1: i64([0, 193])}, ERR_ARG)])


# ---- grain -------------------------------------------------------------------------------------------------------------------------
def test_payload_grain():
    gains = np.zeros(512, np.int32)
    good = (SRC, i64([0, 96]), TAB, u32(np.arange(6)), AUX, 2, i32(PLANES), 3, 1, 8, 0, 1, i32(gains), AUX + 64, DST, 96, None)
    wide16 = {8: 2, 9: 10, 15: 192}
    bad_gain = gains.copy()
    bad_gain[300] = -1
    run('demfi_payload_grain', good, nulls((0, 1, 2, 3, 4, 6, 12, 13, 14)) + [
        ('0 bytes a sample', {8: 0}, ERR_ARG), ('3 bytes a sample', {8: 3}, ERR_ARG), ('8 bits in two bytes', {8: 2}, ERR_ARG),
        ('9 bits', {9: 9}, ERR_ARG),
        ('no plane', {7: 0}, ERR_ARG), ('two planes', {7: 2}, ERR_ARG), ('four planes', {7: 4, 6: i32(PLANES + [[2, 8]])}, ERR_ARG),
        ('a side above the limit', {6: i32([[65532, 1]]), 7: 1, 15: 65532}, ERR_ARG),
        ('a side at the limit', {5: 0, 6: i32([[1, 65531]]), 7: 1, 15: 65531}, OK),
        ('chroma planes of two shapes', {6: i32([[4, 16], [2, 8], [2, 7]])}, ERR_ARG),
        ('chroma planes that fit no subsampling', {6: i32([[4, 16], [3, 8], [3, 8]])}, ERR_ARG),
        ('a negative offset', {1: i64([0, -2])}, ERR_ARG), ('an absent payload', {1: i64([-1, 96])}, ERR_ARG),
        ('dst_stride one byte short', {15: 95}, ERR_ARG), ('full_range 2', {10: 2}, ERR_ARG), ('size 3', {11: 3}, ERR_ARG),
        ('size -1', {11: -1}, ERR_ARG), ('gains_dev off a word', {13: AUX + 66}, ERR_ARG), ('keys_dev off a word', {4: AUX + 2}, ERR_ARG),
        ('a negative gain', {12: i32(bad_gain)}, ERR_ARG),
        ('16 bits, odd base', {**wide16, 0: SRC + 1}, ERR_ARG), ('16 bits, odd offset', {**wide16, 1: i64([0, 193])}, ERR_ARG),
        ('16 bits, odd dst', {**wide16, 14: DST + 1}, ERR_ARG), ('16 bits, odd stride', {**wide16, 15: 193}, ERR_ARG),
        ('n 0', {5: 0}, OK), ('n 0 after the checks', {5: 0, 11: 3}, ERR_ARG), ('n -1', {5: -1}, ERR_ARG),
    ])


# ---- scale -------------------------------------------------------------------------------------------------------------------------
def test_payload_scale():
    # one 4 x 4 plane to 4 x 4, one tap each way: first x [4] int32 at 0, coef x [4][1] int16 at 16, first y at 24, coef y at 40; 48 bytes
    desc = [0, 16, 1, 24, 40, 1, 48]
    good = (SRC, i64([0, 16]), TAB, 2, i32([[4, 4]]), i32([[4, 4]]), 1, 1, 255, AUX, i32(desc), DST, 16, None)
    wide16 = {7: 2, 8: 1023, 12: 32}
    run('demfi_payload_scale', good, nulls((0, 1, 2, 4, 5, 9, 10, 11)) + [
        ('0 bytes a sample', {7: 0}, ERR_ARG), ('3 bytes a sample', {7: 3}, ERR_ARG),
        ('peak 0', {8: 0}, ERR_ARG), ('peak 256 in bytes', {8: 256}, ERR_ARG), ('peak 65536', {7: 2, 8: 65536, 12: 32}, ERR_ARG),
        ('no plane', {6: 0}, ERR_ARG), ('four planes', {6: 4, 4: i32([[4, 4]] * 4), 5: i32([[4, 4]] * 4), 10: i32(desc[:6] * 4 + [48])}, ERR_ARG),
        ('a source side above the limit', {4: i32([[32769, 4]])}, ERR_ARG), ('a source side at the limit', {3: 0, 4: i32([[32768, 4]])}, OK),
        ('an output side above the limit', {5: i32([[4, 32769]]), 12: 1 << 20, 10: i32([0, 1 << 18, 1, 1 << 19, 1 << 19, 1, 1 << 20])}, ERR_ARG),
        ('a source side of 0', {4: i32([[0, 4]])}, ERR_ARG),
        ('no tap', {10: i32([0, 16, 0, 24, 40, 1, 48])}, ERR_ARG), ('33 taps', {10: i32([0, 16, 1, 24, 40, 33, 4096])}, ERR_ARG),
        ('a table behind the blob', {10: i32(desc[:6] + [47])}, ERR_ARG), ('a table off a word', {10: i32([2, 16, 1, 24, 40, 1, 48])}, ERR_ARG),
        ('a negative offset', {1: i64([0, -2])}, ERR_ARG), ('an absent payload', {1: i64([-1, 16])}, ERR_ARG),
        ('dst_stride one byte short', {12: 15}, ERR_ARG), ('tables_dev off a word', {9: AUX + 2}, ERR_ARG),
        ('16 bits, odd base', {**wide16, 0: SRC + 1}, ERR_ARG), ('16 bits, odd offset', {**wide16, 1: i64([0, 33])}, ERR_ARG),
        ('16 bits, odd dst', {**wide16, 11: DST + 1}, ERR_ARG), ('16 bits, odd stride', {**wide16, 12: 33}, ERR_ARG),
        ('n 0', {3: 0}, OK), ('n 0 after the checks', {3: 0, 8: 0}, ERR_ARG), ('n -1', {3: -1}, ERR_ARG),
    ])


# ---- denoise -----------------------------------------------------------------------------------------------------------------------
def test_payload_denoise():
    tab = [[-1, 0, 16, 0], [0, 16, 32, 16]]                          # three taps and the destination; 16-byte payloads
    good = (SRC, 64, i64(tab), TAB, 2, 3, 16, 1, 5, 10, DST, 32, None)
    wide16 = {6: 8, 7: 2}

    def t(r, c, v):
        x = np.array(tab, np.int64)
        x[r, c] = v
        return i64(x)
    run('demfi_payload_denoise', good, nulls((0, 2, 3, 10)) + [
        ('n -1', {4: -1}, ERR_ARG), ('n 65', {4: 65}, ERR_ARG), ('4 taps', {5: 4}, ERR_ARG), ('9 taps', {5: 9}, ERR_ARG),
        ('0 bytes a sample', {7: 0}, ERR_ARG), ('3 bytes a sample', {7: 3}, ERR_ARG),
        ('A below 0', {8: -1}, ERR_ARG), ('B below A', {9: 4}, ERR_ARG), ('B above the peak of a byte', {9: 256}, ERR_ARG),
        ('B above the peak of 16 bits', {**wide16, 9: 65536}, ERR_ARG), ('P 0', {6: 0}, ERR_ARG),
        ('a source buffer below a payload', {1: 15}, ERR_ARG), ('a destination buffer below a payload', {11: 15}, ERR_ARG),
        ('dst inside src', {10: SRC + 32}, ERR_ARG),
        ('the centre absent', {2: t(0, 1, -1)}, ERR_ARG), ('a negative offset', {2: t(1, 0, -2)}, ERR_ARG),
        ('a payload that leaves src', {2: t(1, 2, 49)}, ERR_ARG), ('a destination that leaves dst', {2: t(1, 3, 17)}, ERR_ARG),
        ('a negative destination', {2: t(0, 3, -1)}, ERR_ARG), ('two frames, one destination', {2: t(1, 3, 0)}, ERR_ARG),
        ('two destinations that overlap', {2: t(1, 3, 8)}, ERR_ARG),
        ('16 bits, odd src', {**wide16, 0: SRC + 1}, ERR_ARG), ('16 bits, odd dst', {**wide16, 10: DST + 1}, ERR_ARG),
        ('16 bits, odd offset', {**wide16, 2: t(1, 0, 1)}, ERR_ARG), ('16 bits, odd destination', {**wide16, 2: t(1, 3, 15)}, ERR_ARG),
        ('n 0', {4: 0}, OK), ('n 0 after the checks', {4: 0, 5: 4}, ERR_ARG),
    ])


# ---- the deinterlacers -------------------------------------------------------------------------------------------------------------
def test_yuv_bob():
    good = (SRC, 24, 2, 4, 4, 0, 1, 1, None)                         # 4 x 4 4:2:0: 24 samples
    run('demfi_yuv_bob', good, nulls((0,)) + [
        ('n -1', {2: -1}, ERR_ARG), ('n 65', {2: 65}, ERR_ARG), ('one row', {3: 1}, ERR_ARG), ('16385 columns', {4: 16385, 1: 1 << 20}, ERR_ARG),
        ('layout 4', {5: 4}, ERR_ARG), ('0 bytes a sample', {6: 0}, ERR_ARG), ('3 bytes a sample', {6: 3}, ERR_ARG),
        ('a stride one byte short', {1: 23}, ERR_ARG),
        ('16 bits, odd base', {0: SRC + 1, 1: 48, 6: 2}, ERR_ARG), ('16 bits, odd stride', {1: 49, 6: 2}, ERR_ARG),
        ('n 0', {2: 0}, OK), ('n 0 after the checks', {2: 0, 5: 4}, ERR_ARG),
    ])


def test_yuv_deint_adaptive():
    tab = [[-1, 0, 24, 48, 72], [0, 24, 48, 72, -1]]                 # fields f-2 .. f+2 of two fields; 24-byte payloads
    good = (SRC, 96, i64(tab), TAB, 2, 4, 4, 0, 1, 1, None)

    def t(r, c, v):
        x = np.array(tab, np.int64)
        x[r, c] = v
        return i64(x)
    run('demfi_yuv_deint_adaptive', good, nulls((0, 2, 3)) + [
        ('n -1', {4: -1}, ERR_ARG), ('n 65', {4: 65}, ERR_ARG), ('one row', {5: 1}, ERR_ARG), ('16385 columns', {6: 16385}, ERR_ARG),
        ('layout 4', {7: 4}, ERR_ARG), ('0 bytes a sample', {8: 0}, ERR_ARG), ('3 bytes a sample', {8: 3}, ERR_ARG),
        ('the field itself absent', {2: t(0, 2, -1)}, ERR_ARG), ('a negative offset', {2: t(0, 1, -2)}, ERR_ARG),
        ('a payload that leaves the buffer', {2: t(1, 3, 73)}, ERR_ARG), ('a buffer below a payload', {1: 23}, ERR_ARG),
        ('neither neighbour', {2: i64([[-1, -1, 24, -1, 72], [0, 24, 48, 72, -1]])}, ERR_ARG),
        ('two fields, one payload', {2: t(1, 2, 24)}, ERR_ARG),
        ('16 bits, odd base', {0: SRC + 1, 1: 192, 8: 2}, ERR_ARG), ('16 bits, odd offset', {1: 192, 8: 2, 2: t(0, 3, 49)}, ERR_ARG),
        ('n 0', {4: 0}, OK), ('n 0 after the checks', {4: 0, 7: 4}, ERR_ARG),
    ])


# ---- the luma statistics: their offsets are device arrays, so only the scalars and the addresses can be refused -------------------
def luma_cases(n, h, w, sb):
    return [
        ('n -1', {n: -1}, ERR_ARG), ('one row', {h: 1}, ERR_ARG), ('one column', {w: 1}, ERR_ARG), ('16385 rows', {h: 16385}, ERR_ARG),
        ('16385 columns', {w: 16385}, ERR_ARG), ('0 bytes a sample', {sb: 0}, ERR_ARG), ('3 bytes a sample', {sb: 3}, ERR_ARG),
        ('16 bits, odd base', {0: SRC + 1, sb: 2}, ERR_ARG), ('n 0', {n: 0}, OK), ('n 0 after the checks', {n: 0, sb: 3}, ERR_ARG),
    ]


def test_luma_block_counts():
    good = (SRC, TAB, TAB + 64, 2, 16, 16, 1, 100, 50, DST, None)
    run('demfi_luma_block_counts', good, nulls((0, 1, 2, 9)) + luma_cases(3, 4, 5, 6) + [
        ('hi below 0', {7: -1}, ERR_ARG), ('lo below 0', {8: -1}, ERR_ARG), ('hi above 2^40', {7: (1 << 40) + 1}, ERR_ARG)])


def test_luma_comb_counts():
    good = (SRC, TAB, TAB + 64, 2, 16, 16, 1, 7, DST, None)
    run('demfi_luma_comb_counts', good, nulls((0, 1, 2, 8)) + luma_cases(3, 4, 5, 6) + [
        ('threshold below 0', {7: -1}, ERR_ARG), ('threshold above 2^20', {7: (1 << 20) + 1}, ERR_ARG)])


def test_luma_woven_sad():
    good = (SRC, TAB, 2, 16, 16, 1, DST, None)
    run('demfi_luma_woven_sad', good, nulls((0, 1, 6)) + luma_cases(2, 3, 4, 5))


def test_luma_line_counts():
    good = (SRC, TAB, 2, 16, 16, 1, 16, DST, DST + 256, None)
    run('demfi_luma_line_counts', good, nulls((0, 1, 7, 8)) + luma_cases(2, 3, 4, 5) + [
        ('threshold below 0', {6: -1}, ERR_ARG), ('threshold above 65535', {6: 65536}, ERR_ARG)])
