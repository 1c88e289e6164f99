"""``demfi_amd.colour`` on the host: the tables and their round trip, what mixing in light does, the encode as the existing definition
behind the table, the switch resolution and header rule, ``EdgeSpec.colour``, the sizes ``egress_layout`` gives a linear-light chain, and
the refusals."""
import numpy as np
import pytest

from demfi_amd import colour as CL
from demfi_amd import scale as SC
from demfi_amd import shutter as SH
from demfi_amd import y4m
from demfi_amd.pipeline import EdgeSpec
from demfi_amd.y4m_edge import Buffer, LinearBuffer, egress_layout, linear_light, sample_format

DEPTHS = (8, 10, 12)
SMALLEST_STEP = {('bt709', 8): 57, ('bt709', 10): 14, ('bt709', 12): 3, ('srgb', 8): 19, ('srgb', 10): 4, ('srgb', 12): 1}


# ---- tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', DEPTHS)
@pytest.mark.parametrize('transfer', CL.TRANSFERS)
def test_tables_are_monotone_and_round_trip(transfer, depth):
    peak = (1 << depth) - 1
    fwd, inv = CL.tables(transfer, depth)
    assert fwd.dtype == np.uint16 and fwd.shape == (peak + 1,) and inv.dtype == np.uint16 and inv.shape == (65536,)
    assert fwd[0] == 0 and fwd[peak] == 65535
    steps = np.diff(fwd.astype(np.int64))
    assert steps.min() == SMALLEST_STEP[transfer, depth] > 0
    assert (np.diff(inv.astype(np.int64)) >= 0).all() and inv[0] == 0 and inv[65535] == peak
    assert np.array_equal(inv[fwd], np.arange(peak + 1))                 # every code comes back


@pytest.mark.parametrize('depth', DEPTHS)
@pytest.mark.parametrize('transfer', CL.TRANSFERS)
def test_inverse_is_the_nearest_code_in_light(transfer, depth):
    """Brute force: of all codes the one whose linear value is nearest to v; of two equally near ones the larger (the threshold rounds up)."""
    fwd, inv = CL.tables(transfer, depth)
    f = fwd.astype(np.int64)
    for v0 in range(0, 65536, 4096):
        v = np.arange(v0, v0 + 4096, dtype=np.int64)
        dist = np.abs(v[:, None] - f[None, :])
        best = dist.shape[1] - 1 - np.argmin(dist[:, ::-1], axis=1)      # the last of the nearest
        assert np.array_equal(inv[v0:v0 + 4096], best)
    thr = CL.thresholds(fwd)
    assert thr.shape == (len(fwd) - 1,) and thr[0] == (f[0] + f[1] + 1) // 2
    v = np.array([0, 1, 77, 4095, 30000, 65534, 65535])
    assert np.array_equal(inv[v], [(thr <= x).sum() for x in v])         # the binary search over the thresholds is the same function


def test_transfers_are_the_standards():
    assert CL.TRANSFERS == ('bt709', 'srgb')
    assert CL.to_linear('bt709', 0.0812) == pytest.approx(0.018, rel=5e-3) and CL.to_linear('bt709', 0.0405) == pytest.approx(0.009)
    assert CL.to_linear('srgb', 0.04045) == pytest.approx(0.04045 / 12.92) and CL.to_linear('srgb', 0.5) == pytest.approx(0.21404, rel=1e-4)
    assert float(CL.to_linear('bt709', 1.0)) == pytest.approx(1.0) and float(CL.to_linear('srgb', 1.0)) == pytest.approx(1.0)
    with pytest.raises(ValueError):
        CL.forward_table('pq', 8)


@pytest.mark.parametrize('depth', [14, 16, 9, 0])
def test_depths_above_12_are_refused(depth):
    with pytest.raises(ValueError, match='8, 10 or 12'):
        CL.forward_table('bt709', depth)
    with pytest.raises(ValueError):
        CL.check_depth(depth)


# ---- what the mix does in light --------------------------------------------------------------------------------------------------
def _mix_codes(a, b, transfer, depth):
    """Codes a and b over a 2x2 frame each, mixed 1:1 in light: the code that comes back."""
    fwd, inv = CL.tables(transfer, depth)
    dt = np.uint8 if depth == 8 else np.uint16
    lin = np.stack([CL.linearize_np(np.full((2, 2, 3), c, dt), fwd).reshape(-1) for c in (a, b)]).view(np.uint8)
    mixed = SH.mix_np(lin, [[0, 1]], 2).view('<u2').reshape(3, 2, 2)
    codes = CL.delinearize_np(mixed, inv, depth)
    assert len(set(codes.reshape(-1).tolist())) == 1
    return int(codes[0, 0, 0])


def test_16_and_235_mix_above_their_mean_by_hand():
    """bt709 with a = 1.09929682680944 (BT.709's 1.099 before rounding): fwd[16] = floor(65535 (16/255)/4.5 + .5) = 914 (the toe),
    fwd[235] = floor(65535 ((235/255 + a - 1)/a)^(1/.45) + .5) = 55595; their mean (2 (914 + 55595) + 2) // 4 = 28255 lies between
    fwd[166] = 28043 and fwd[167] = 28370, nearer the latter (115 against 212): code 167, where the code-value mean is 126."""
    fwd, inv = CL.tables('bt709', 8)
    a = 1.09929682680944
    v16 = int(np.floor(65535 * (16 / 255) / 4.5 + 0.5))
    v235 = int(np.floor(65535 * ((235 / 255 + a - 1) / a) ** (1 / 0.45) + 0.5))
    assert (fwd[16], fwd[235]) == (v16, v235) == (914, 55595)
    mean = (2 * (v16 + v235) + 2) // 4
    assert mean == 28255 and fwd[166] == 28043 and fwd[167] == 28370 and inv[mean] == 167
    assert _mix_codes(16, 235, 'bt709', 8) == 167 > (16 + 235 + 1) // 2
    assert _mix_codes(16, 235, 'srgb', 8) > 167                          # the steeper curve lifts the mix further


@pytest.mark.parametrize('depth', DEPTHS)
@pytest.mark.parametrize('transfer', CL.TRANSFERS)
def test_constants_are_kept_and_mixes_lie_above_the_code_mean(transfer, depth):
    peak, s = (1 << depth) - 1, 1 << (depth - 8)
    for c in (0, 1, 16 * s, 100 * s + 1, 235 * s, peak):
        assert _mix_codes(c, c, transfer, depth) == c
    # f^-1 is convex above the toe, so the mean of two lights lies above the light of the mean code: by about (b - a)^2 / 8 times
    # f^-1'' / f^-1' ~ 1.2 / c codes, more than the half code of the rounding for pairs 20 eight-bit steps and more apart
    for a, b in ((40 * s, 60 * s), (30 * s, peak), (100 * s, 140 * s), (128 * s, 250 * s)):
        assert _mix_codes(a, b, transfer, depth) > (a + b + 1) // 2


# ---- the encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('depth', DEPTHS)
def test_encode_of_a_linearised_frame_is_the_existing_gather(depth, layout):
    rng = np.random.default_rng(depth)
    peak = (1 << depth) - 1
    bgr = rng.integers(0, peak + 1, (7, 9, 3)).astype(np.uint8 if depth == 8 else np.uint16)
    for transfer, matrix, full in (('bt709', 'bt601', False), ('srgb', 'bt709', True)):
        fwd, inv = CL.tables(transfer, depth)
        lin = CL.linearize_np(bgr, fwd)
        assert lin.dtype == np.dtype('<u2') and lin.shape == (3, 7, 9) and np.array_equal(lin[2], fwd[bgr[:, :, 2]])
        got = CL.encode_payload_np(lin, inv, depth, layout, matrix, full)
        want = y4m.bgr_to_yuv_np(bgr, layout, matrix, full) if depth == 8 else y4m.bgr16_to_yuv_np(bgr, depth, layout, matrix, full)
        assert got.dtype == want.dtype and np.array_equal(got, want)


def test_linear_stream_composes_the_definitions():
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (6, 10, 3)).astype(np.uint8) for _ in range(5)]
    fwd, inv = CL.tables('bt709', 8)
    groups = SH.groups(5, 2, 3, 4)
    assert groups == [[0, 1, 2], [4]]
    out = CL.linear_stream_np(frames, groups, 'bt709', 8, '420', 'bt709', True, scale=(14, 4, 'bilinear'))
    lin = np.stack([CL.linearize_np(f, fwd).reshape(-1) for f in frames]).astype(np.int64)
    m0 = ((2 * lin[:3].sum(axis=0) + 3) // 6).astype(np.uint16)
    want = [CL.encode_payload_np(SC.scale_payload_np(m, 6, 10, 4, 14, 16, '444', 'bilinear').reshape(3, 4, 14), inv, 8, '420', 'bt709', True)
            for m in (m0, lin[4].astype(np.uint16))]
    assert len(out) == 2 and all(np.array_equal(a, b) for a, b in zip(out, want))
    same = CL.linear_stream_np(frames, None, 'srgb', 8, '444', scale=(10, 6, 'lanczos3'))         # the run's own size: no resampling
    assert all(np.array_equal(a, y4m.bgr_to_yuv_np(f, '444')) for a, f in zip(same, frames))


# ---- the switches ----------------------------------------------------------------------------------------------------------------
def test_resolve_and_the_header_rule():
    assert CL.resolve(None, None, 'bt601', False, 480) == ('bt601', False)
    assert CL.resolve(None, None, 'bt709', True, 480) == ('bt709', True)
    assert CL.resolve('auto', None, 'bt601', False, 720) == ('bt709', False) and CL.resolve('auto', None, 'bt601', False, 719) == ('bt601', False)
    assert CL.resolve('auto', 'full', 'bt709', False, 576) == ('bt601', True)
    assert CL.resolve('bt709', 'limited', 'bt601', True, 64) == ('bt709', False)
    for bad in (('bt2020', None), (None, 'pc'), ('AUTO', None)):
        with pytest.raises(ValueError):
            CL.resolve(*bad, 'bt601', False, 480)
    # XCOLORRANGE: written when the range changes or the input carried the tag
    assert CL.range_tag(None, False) is None and CL.range_tag(None, True) == 'FULL'
    assert CL.range_tag('FULL', True) == 'FULL' and CL.range_tag('FULL', False) == 'LIMITED'
    assert CL.range_tag('LIMITED', False) == 'LIMITED' and CL.range_tag('LIMITED', True) == 'FULL'
    hdr = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip A1:1 C420jpeg XFOO=1\n')
    assert CL.range_header(hdr, False).encode() == hdr.encode()
    assert CL.range_header(hdr, True).encode() == hdr.encode()[:-1] + b' XCOLORRANGE=FULL\n'
    assert CL.check_switches(True, 'auto', 'full') == ('bt709', 'auto', 'full') and CL.check_switches() == (None, None, None)


def test_video_switches_and_refusals():
    from demfi_amd import clip, video as V
    a = V.parser().parse_args(['in', 'out', '--linear-light', '--out-matrix', 'auto', '--out-range', 'full'])
    assert (a.linear_light, a.out_matrix, a.out_range) == ('bt709', 'auto', 'full')
    assert V.parser().parse_args(['in', 'out', '--linear-light', 'srgb']).linear_light == 'srgb'
    assert V.parser().parse_args(['in', 'out']).linear_light is None
    for bad in (['--linear-light', 'pq'], ['--out-matrix', 'bt2020'], ['--out-range', 'tv']):
        with pytest.raises(SystemExit):
            V.parser().parse_args(['in', 'out'] + bad)
    for switch in (['--linear-light'], ['--out-matrix', 'bt709'], ['--out-range', 'full']):       # not offered on the folder tool
        with pytest.raises(SystemExit):
            clip.parser().parse_args(['frames'] + switch)
    assert V.check_colour() is None and V.check_colour('srgb', None, 'full') == ('srgb', None, True)
    assert V.check_colour(None, 'auto', None, auto=True) == (None, 'auto', None)
    with pytest.raises(ValueError):
        V.check_colour(None, 'auto', None)
    edge = V.YuvEdge('bt601', False, '420jpeg', None, linear_light=True, out_matrix='bt709')
    assert edge.colour == ('bt709', 'bt709', None) and V.YuvEdge('bt601', False, '420jpeg', None).colour is None
    vr = V.VideoRunner(None, linear_light='bt709', out_matrix='auto', high_depth=True)
    hdr = y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip C420p14\n', y4m.DEPTHS)
    with pytest.raises(ValueError, match='8, 10 or 12'):              # before anything is allocated: the header alone refuses
        vr._check_depth(hdr)
    with pytest.raises(ValueError, match='8, 10 or 12'):
        V.VideoRunner(None, linear_light=True, work_depth=16, high_depth=True)._check_depth(y4m.parse_header(b'YUV4MPEG2 W96 H64 F24:1 Ip\n'))
    sd = y4m.parse_header(b'YUV4MPEG2 W720 H576 F25:1 Ip\n')
    assert V.VideoRunner(None, out_matrix='auto', scale='1920x1080')._colour_of(sd) == (None, 'bt709', False)
    assert V.VideoRunner(None, out_matrix='auto')._colour_of(sd) == (None, 'bt601', False)
    assert V.VideoRunner(None, out_range='full')._out_header(sd).color_range == 'FULL'
    assert V.VideoRunner(None)._out_header(sd).color_range is None


# ---- EdgeSpec --------------------------------------------------------------------------------------------------------------------
def test_edge_spec_with_and_without_colour():
    plain = EdgeSpec(True, depth=10, shutter=(4, 8))
    same = EdgeSpec(True, depth=10, shutter=(4, 8), colour=(None, None, None))
    assert same.colour is None and plain == same and hash(plain) == hash(same) and repr(plain) == repr(same)
    assert 'colour' not in repr(plain) and tuple(plain) == tuple(same)
    lin = plain._replace(colour=('bt709', None, None))
    assert lin != plain and plain != lin and lin.colour == ('bt709', None, None) and lin.shutter == (4, 8)
    assert repr(lin).endswith(", colour=('bt709', None, None))") and hash(lin) == hash(plain._replace(colour=('bt709', None, None)))
    assert lin._replace(depth=8).colour == lin.colour and lin._replace(colour=None) == plain
    assert lin != tuple(lin) and EdgeSpec(True, colour=(None, 'bt709', 1)).colour == (None, 'bt709', True)
    assert len({plain, same, lin, lin._replace(colour=('srgb', None, None)), lin._replace(colour=('bt709', 'bt601', None))}) == 4

    class Yuv:
        depth, layout, shutter, colour = 8, '420', (4, 8), ('srgb', 'bt709', True)
    assert EdgeSpec.of(Yuv).colour == ('srgb', 'bt709', True) and EdgeSpec.of(None).colour is None
    lin._replace(depth=12).check(True, False, True)
    for bad, why in ((lin._replace(depth=14), '12 bits'), (lin._replace(depth=16), '12 bits'), (lin._replace(colour=('pq', None, None)), 'colour'),
                     (lin._replace(colour=(None, 'auto', None)), 'colour'), (lin._replace(y4m=False, shutter=None), 'Y4M edge')):
        with pytest.raises(ValueError, match=why):
            bad.check(True, False, True)
    with pytest.raises(ValueError, match='retimed'):
        EdgeSpec(True, colour=(None, 'bt709', None)).check(False, False, True)
    EdgeSpec(True, depth=16, colour=(None, 'bt709', True)).check(True, False, True)       # matrix and range alone: every depth


# ---- egress_layout ---------------------------------------------------------------------------------------------------------------
H, W, NOUT, BATCH = 64, 96, 33, 4
P420 = y4m.payload_size(H, W)
LIN = ('bt709', None, None)


def test_layout_linear_mix():
    spec = EdgeSpec(True, shutter=(4, 8), colour=LIN)
    got = egress_layout(spec, NOUT, BATCH, H, W)
    rows = NOUT // 8 + BATCH + 2
    assert got == [('gather', 3, NOUT, 6 * H * W, H, W), ('mix', 0, rows, 6 * H * W, H, W), ('encode', 0, rows, P420, H, W), (rows, P420)]
    assert [type(b) for b in got[:3]] == [LinearBuffer, LinearBuffer, Buffer] and Buffer._fields == ('name', 'lead', 'rows', 'Pb', 'h', 'w')
    assert sample_format(spec, got[0]) == (2, [(H, W)] * 3, 65535) and sample_format(spec, got[2]) == (1, [(H, W), (32, 48), (32, 48)], 255)
    plain = egress_layout(spec._replace(colour=None), NOUT, BATCH, H, W)
    assert plain == [('gather', 3, NOUT, P420, H, W), ('mix', 0, rows, P420, H, W), (rows, P420)]


def test_layout_linear_scale():
    spec = EdgeSpec(True, depth=10, layout='422', scale=(72, 48, 'bicubic'), colour=('srgb', 'bt709', True))
    got = egress_layout(spec, NOUT, BATCH, H, W)
    P = y4m.payload_size(48, 72, '422') * 2
    assert got == [('gather', 0, NOUT, 6 * H * W, H, W), ('scale', 0, NOUT, 6 * 48 * 72, 48, 72), ('encode', 0, NOUT, P, 48, 72), (NOUT, P)]
    assert sample_format(spec, got[1]) == (2, [(48, 72)] * 3, 65535)      # 2-byte samples whatever the depth


def test_layout_linear_both_weave_requant():
    spec = EdgeSpec(True, depth=10, shutter=(2, 4), interlace=('t', 'linear'), scale=(128, 80, 'lanczos3'), depths=(8, 10, 8, 'bayer'), colour=LIN)
    got = egress_layout(spec, NOUT, BATCH, H, W)
    rows, P10, P8 = NOUT // 4 + BATCH + 2, y4m.payload_size(80, 128) * 2, y4m.payload_size(80, 128)
    assert got == [('gather', 1, NOUT, 6 * H * W, H, W), ('mix', 0, rows, 6 * H * W, H, W), ('scale', 0, rows, 6 * 80 * 128, 80, 128),
                   ('encode', 1, rows, P10, 80, 128), ('weave', 0, rows // 2 + 1, P10, 80, 128), ('requant', 0, rows // 2 + 1, P8, 80, 128),
                   (rows // 2 + 1, P8)]
    assert [type(b) is LinearBuffer for b in got[:-1]] == [True, True, True, False, False, False]
    plain = egress_layout(spec._replace(colour=(None, 'bt709', True)), NOUT, BATCH, H, W)     # matrix and range alone: no buffer, no stage
    assert plain == egress_layout(spec._replace(colour=None), NOUT, BATCH, H, W) and [b.name for b in plain[:-1]] == ['gather', 'mix', 'scale', 'weave', 'requant']


def test_layout_linear_alone_builds_nothing():
    for spec in (EdgeSpec(True, colour=LIN), EdgeSpec(True, scale=(W, H, 'lanczos3'), colour=LIN),       # the run's own size: no scale stage
                 EdgeSpec(True, interlace=('b', 'none'), colour=LIN)):
        assert not linear_light(spec, H, W)
        got = egress_layout(spec, NOUT, BATCH, H, W)
        assert got == egress_layout(spec._replace(colour=None), NOUT, BATCH, H, W) and not any(isinstance(b, LinearBuffer) for b in got)
    assert linear_light(EdgeSpec(True, scale=(W, H + 2, 'lanczos3'), colour=LIN), H, W)
    assert not linear_light(EdgeSpec(True, shutter=(4, 8), colour=(None, 'bt709', None)), H, W)
