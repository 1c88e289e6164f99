"""The 3D colour LUT of the Y4M egress (``--lut``) on a real MI355X: ``demfi_rgb_lut3d`` equal to ``lut3d.lut_payload_np`` byte for byte inside
poisoned memory over the cubes and inputs of tests/lut3d_cases.py (tests/test_lut3d.py proves on the CPU what those reach), and
``VideoRunner(lut=...)`` byte-identical to expectations that never run the new code: the fine BGR frames of the timeline, from
``ClipRunner.run_frames`` (8-bit 4:2:0) or the composed expectation of tests/test_gpu_y4m_layouts.py (other depths, layouts, tiles), taken
through ``lut3d.lut_stream_np`` on the host.  The clips, the model and the stream helpers are those of tests/test_gpu_colour.py."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import bitdepth as BD                                                 # noqa: E402
from demfi_amd import grain as GR                                                    # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import lut3d as LU                                                    # noqa: E402
from demfi_amd import shutter as SH                                                  # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from demfi_amd.y4m_edge import Encoder, Lut                                          # noqa: E402
from tests import lut3d_cases as K                                                   # noqa: E402
from tests import test_gpu_colour as TC                                              # noqa: E402
from tests import test_gpu_interlace as TI                                           # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
POISON = 0xC3


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
class Tables:
    """The device tables of one (cube, depth, inv_in): uploaded once and shared by the launches that use them."""

    def __init__(self, cube, depth, inv_in):
        self.cube, self.depth, self.n = cube, depth, cube.n
        self.inv = torch.from_numpy(np.ascontiguousarray(inv_in, np.uint16).view(np.int16)).to(DEV)
        self.axt = torch.from_numpy(LU.axis_table(depth, cube.n).view(np.int32)).to(DEV)
        self.words = torch.from_numpy(LU.cube_words(cube).view(np.int64).reshape(-1)).to(DEV)


def _lut_gpu(pays, order, tab, shift=0, gap=0, in_lds=0):
    """RGB payloads ``pays`` [m, 3, h, w] uint16 placed ``shift`` BYTES behind a 16-byte boundary each; payload order[i] -> written
    payload i, rows ``gap`` bytes apart in a poisoned dst.  The poison outside the payloads and the sources come back untouched."""
    m, _, h, w = pays.shape
    Pb = 6 * h * w
    pitch = -(-Pb // 16) * 16 + 16
    buf = np.full(m * pitch + 16, 0xEE, np.uint8)
    at = [i * pitch + shift for i in range(m)]
    for o, p in zip(at, pays):
        buf[o:o + Pb] = np.ascontiguousarray(p, '<u2').reshape(-1).view(np.uint8)
    n, stride = len(order), Pb + gap
    table = np.array([at[a] for a in order], np.int64)
    src, od = torch.from_numpy(buf).to(DEV), torch.from_numpy(table).to(DEV)
    dst = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    L.check(L.load().demfi_rgb_lut3d(src.data_ptr(), table.ctypes.data, od.data_ptr(), n, h, w, tab.depth, tab.inv.data_ptr(), tab.n,
                                     tab.words.data_ptr(), tab.axt.data_ptr(), in_lds, dst.data_ptr(), stride, _stream()), 'rgb_lut3d')
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    body = out[:n * stride].reshape(n, stride)
    assert (body[:, Pb:] == POISON).all() and (out[n * stride:] == POISON).all(), 'write outside the payloads'
    assert np.array_equal(src.cpu().numpy(), buf), 'a source was written'
    return np.ascontiguousarray(body[:, :Pb]).view('<u2').reshape(n, 3, h, w)


def _combos(n, depth):
    """(cube name, table pair name): every cube with the e tables, the random cube with each transfer's tables."""
    pairs = K.table_pairs(depth)
    return [(c, 'e') for c in K.cubes(n)] + [('random', t) for t in pairs if t != 'e'], pairs


@pytest.mark.parametrize('depth', K.DEPTHS)
@pytest.mark.parametrize('n', K.NS)
def test_kernel_equals_the_numpy_definition(n, depth):
    """Every cube size and depth: the enumerations of every code on each axis and diagonal in one launch, the random frames of 6x10,
    17x33 and 33x70 in one each; scattered and repeated offsets; an aligned placement and one two bytes off the 16-byte boundary with a
    stride that keeps no row of dst aligned."""
    cubes = K.cubes(n)
    combos, pairs = _combos(n, depth)
    launches = K.launches(depth)
    for j, (cname, tname) in enumerate(combos):
        fwd, inv_in = pairs[tname]
        tab = Tables(cubes[cname], depth, inv_in)
        for k, (h, w, codes) in enumerate(launches):
            pays = K.payloads(codes, fwd)
            m = len(pays)
            order = [(3 * i + 1) % m for i in range(m + 2)]
            shift, gap = ((0, 32 + -(6 * h * w) % 16), (2, 6))[(j + k) % 2]
            got = _lut_gpu(pays, order, tab, shift, gap)
            ref = [LU.lut_payload_np(p, inv_in, depth, cubes[cname]) for p in pays]
            for i, a in enumerate(order):
                assert np.array_equal(got[i], ref[a]), (cname, tname, h, w, shift, i)


@pytest.mark.parametrize('n', [2, 3, 17])
def test_the_cube_in_lds_writes_the_same_bytes(n):
    """cube_in_lds = 1, up to 17^3: another schedule (a workgroup walks several chunks of lanes and all payloads), the same bytes."""
    depth = 10
    fwd, inv_in = LU.tables(depth)
    for cname in ('random', 'checker'):
        cube = K.cubes(n)[cname]
        tab = Tables(cube, depth, inv_in)
        for k, (h, w, codes) in enumerate(K.launches(depth)):
            pays = K.payloads(codes, fwd)
            order = list(range(len(pays))) + [0]
            got = _lut_gpu(pays, order, tab, 2 * (k % 2), 6 * (k % 2), in_lds=1)
            for i, a in enumerate(order):
                assert np.array_equal(got[i], LU.lut_payload_np(pays[a], inv_in, depth, cube)), (cname, h, w, i)


def test_more_payloads_than_the_grid_has_rows():
    depth, (h, w) = 12, K.SIZES[0]
    fwd, inv_in = LU.tables(depth, 'srgb')
    cube = K.cubes(3)['random']
    pays = K.payloads(K.random_codes(depth, h, w), fwd)
    n = 4096 + 5                                                         # the grid's payload dimension is 4096
    order = [(i * 5) % 3 for i in range(n)]
    got = _lut_gpu(pays, order, Tables(cube, depth, inv_in), 2, 2)
    ref = np.stack([LU.lut_payload_np(p, inv_in, depth, cube) for p in pays])
    assert np.array_equal(got, ref[order])


def test_values_off_the_table_read_the_peaks_entry_and_bad_arguments_launch_nothing():
    """inv_in may hold anything: a code above the peak is read as the peak, so no load leaves the tables."""
    depth, (h, w) = 8, K.SIZES[0]
    cube = K.cubes(5)['random']
    wild = np.random.default_rng(3).integers(0, 65536, 65536).astype(np.uint16)
    pays = np.random.default_rng(4).integers(0, 65536, (2, 3, h, w)).astype(np.uint16)
    got = _lut_gpu(pays, [0, 1], Tables(cube, depth, wild))
    ref = [LU.lut_payload_np(p, np.minimum(wild, 255), depth, cube) for p in pays]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    lib, tab = L.load(), Tables(cube, depth, wild)
    src = torch.full((1024,), 0x11, dtype=torch.uint8, device=DEV)
    dst = torch.full((1024,), POISON, dtype=torch.uint8, device=DEV)
    offs, host = torch.zeros(2, dtype=torch.int64, device=DEV), np.array([0, 96], np.int64)
    ok = [src.data_ptr(), host.ctypes.data, offs.data_ptr(), 2, 4, 4, depth, tab.inv.data_ptr(), 5, tab.words.data_ptr(), tab.axt.data_ptr(), 0,
          dst.data_ptr(), 96, _stream()]
    for i, v in ((0, None), (3, -1), (4, 1), (6, 14), (8, 66), (11, 2), (13, 94), (12, src.data_ptr())):
        a = list(ok)
        a[i] = v
        assert lib.demfi_rgb_lut3d(*a) == -1 and b'demfi_rgb_lut3d' in lib.demfi_last_error(), i
    a = list(ok)
    a[3] = 0
    assert lib.demfi_rgb_lut3d(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0x11).all())
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
H, W, N = TC.H, TC.W, TC.N
_run, _payloads, _same_payloads = TC._run, TC._payloads, TC._same_payloads
CUBE = LU.Cube(17, np.random.default_rng(17).integers(0, 65536, (17, 17, 17, 3)))
LIFT = LU.Cube.of_table(0.25 + 0.5 * LU.identity_table(5))               # lifts black to a quarter


@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


@pytest.fixture(scope='module')
def clip7():
    return Y._clip(N, H, W, '420', 8, seed=3)[0]


@pytest.fixture(scope='module')
def fine2(model16, clip7):
    return TC._fine_frames(model16, clip7, 2)


@pytest.fixture(scope='module')
def fine8(model16, clip7):
    return TC._fine_frames(model16, clip7, 8)


def _fine_bgr(model, data, r, plan=None):
    """The fine BGR frames of the x r timeline of any depth and layout, in stream order: the composed expectation of
    tests/test_gpu_y4m_layouts.py, stopped in front of its conversion back to Y'CbCr."""
    got = []
    with pytest.MonkeyPatch.context() as m:
        m.setattr(Y, '_to_yuv_np', lambda f, d, lay, matrix, full: (got.append(np.array(f)), np.zeros(0, np.uint8))[1])
        Y._expected(model, data, 2, Fraction(r), 'bt601', plan=plan)
    return got


def _edge(vr):
    (cr,) = vr._runners.values()
    return cr.runner, cr.runner._pipeline.edge


def test_the_lut_alone_equals_the_reference(model16, clip7, fine2, tmp_path):
    """8-bit 4:2:0 through a stream, a pipe and a file at batches of 1, 2 and 4 windows."""
    exp = LU.lut_stream_np(fine2, None, CUBE, 8, '420', 'bt601', False)
    plain = _run(model16, clip7, mfi=2)[3]
    for batch, how in ((1, 'stream'), (2, 'pipe'), (4, 'file')):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, how=how, tmp_path=tmp_path, mfi=2, lut=CUBE)
        head, pays = _payloads(got)
        _same_payloads(pays, exp)
        rn, edge = _edge(vr)
        assert nf == len(exp) == len(fine2) and vr.last_lut_payloads == nf == rn.lut_payloads and vr.last_colour_encoded == nf
        assert [type(st) for st in edge.stages] == [Lut, Encoder] and edge.fwd is not None and vr.last_lut == CUBE
        assert head == plain[:len(head)] and len(got) == len(plain) and got != plain


@pytest.mark.parametrize('case', ['10-bit-422', 'work-depth-12', 'tiled'])
def test_the_lut_alone_on_the_other_frame_paths(case, model16, clip7):
    if case == '10-bit-422':
        data, kw, depth, layout = Y._clip(5, H, W, '422', 10, seed=4)[0], {'high_depth': True, 'layouts': True}, 10, '422'
        fine = _fine_bgr(model16, data, 2)
    elif case == 'work-depth-12':                                        # the network sees the stream promoted to 12 bits
        data, kw, depth, layout = Y._clip(5, H, W, '422', 8, seed=4)[0], {'work_depth': 12, 'out_depth': 12, 'layouts': True}, 12, '422'
        fine = _fine_bgr(model16, BD.promote_stream_np(data, 12), 2)
    else:
        data, kw, depth, layout = Y._clip(5, 96, 128, '420', 8, seed=4)[0], {'tile': (64, 64), 'tile_margin': 16}, 8, '420'
        plan = _run(model16, data, batch=2, mfi=2, **kw)[0].last_plan
        assert plan.n_tiles > 1
        fine = _fine_bgr(model16, data, 2, plan)
    exp = LU.lut_stream_np(fine, None, CUBE, depth, layout, 'bt601', False)
    vr, nw, nf, got = _run(model16, data, batch=2, mfi=2, lut=CUBE, **kw)
    _same_payloads(_payloads(got)[1], exp)
    assert vr.last_lut_payloads == nf == len(exp) > 0 and vr.last_depth == depth


@pytest.mark.parametrize('n', [17, 33])
def test_an_identity_cube_writes_the_bytes_of_the_run_without(n, model16, clip7):
    ident = LU.Cube.of_table(LU.identity_table(n))
    for kw in ({'mfi': 2}, {'linear_light': 'bt709', **TC.SHUTTER}, {'mfi': 2, 'linear_light': 'srgb', 'scale': (72, 48)}):
        plain = _run(model16, clip7, batch=2, **kw)[3]
        vr, nw, nf, got = _run(model16, clip7, batch=2, lut=ident, **kw)
        Y._same(got, plain)
        assert vr.last_lut_payloads == nf == vr.last_colour_encoded > 0


def test_behind_the_shutter_and_the_scaler_with_and_without_linear_light(model16, clip7, fine2, fine8):
    groups = SH.groups(len(fine8), N - 3 + 1, 4, 8)
    for transfer in (None, 'bt709'):
        lin = {} if transfer is None else {'linear_light': transfer}
        vr, nw, nf, got = _run(model16, clip7, batch=2, lut=CUBE, **lin, **TC.SHUTTER)
        _same_payloads(_payloads(got)[1], LU.lut_stream_np(fine8, groups, CUBE, 8, '420', 'bt601', False, transfer=transfer))
        assert vr.last_lut_payloads == nf == len(groups)
        vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, lut=CUBE, scale=(72, 48), **lin)
        _same_payloads(_payloads(got)[1], LU.lut_stream_np(fine2, None, CUBE, 8, '420', 'bt601', False, transfer=transfer, scale=(72, 48, 'lanczos3')))
        assert vr.last_lut_payloads == vr.last_scale_payloads == nf == len(fine2)
        rn, edge = _edge(vr)
        assert [type(st).__name__ for st in edge.stages] == ['Scaler', 'Lut', 'Encoder'] and (edge.stages[1].h, edge.stages[1].w) == (48, 72)
    # both, at half the input rate with a 360-degree shutter of 16 samples: a written frame mixes the fine frames of two windows, so its
    # first samples carry over from one batch to the next as RGB payloads
    groups = SH.groups(len(fine8), 3, 16, 16)
    for transfer in (None, 'bt709'):
        lin = {} if transfer is None else {'linear_light': transfer}
        exp = LU.lut_stream_np(fine8, groups, CUBE, 8, '420', 'bt601', False, transfer=transfer, scale=(72, 48, 'bicubic'))
        for batch in (1, 2):
            vr, nw, nf, got = _run(model16, clip7, batch=batch, lut=CUBE, scale=(72, 48), scale_filter='bicubic', fps='12/1', down=True,
                                   shutter='360', shutter_samples=16, **lin)
            _same_payloads(_payloads(got)[1], exp)
            assert (vr.last_shutter_carried > 0) == (batch == 1) and vr.last_lut_payloads == nf == 3


def test_the_stages_behind_are_unchanged(model16, clip7, fine2):
    """Grain, weave, requantisation, output matrix and range applied on the host to the LUT run's reference give the run with them."""
    kw = dict(batch=2, mfi=2, lut=CUBE)
    prog = _run(model16, clip7, **kw)[3]
    head, pays = _payloads(prog)
    _same_payloads(pays, LU.lut_stream_np(fine2, None, CUBE, 8, '420', 'bt601', False))
    vr, _, nf, got = _run(model16, clip7, grain='3', grain_seed=11, **kw)
    Y._same(got, GR.grain_stream_np(prog, (48, 1, 8, 'film', 11)))
    assert vr.last_grain_payloads == vr.last_lut_payloads == nf
    woven, n_woven = TI._woven(prog, 't')
    vr, _, nf, got = _run(model16, clip7, interlace='tff', **kw)
    Y._same(got, woven)
    assert nf == n_woven
    prog10 = _run(model16, clip7, work_depth=10, out_depth=10, **kw)[3]
    Y._same(_run(model16, clip7, work_depth=10, out_depth=8, **kw)[3], BD.requant_stream_np(prog10, 8))
    vr, _, nf, got = _run(model16, clip7, out_matrix='bt709', out_range='full', **kw)
    ghead, gpays = _payloads(got)
    _same_payloads(gpays, LU.lut_stream_np(fine2, None, CUBE, 8, '420', 'bt709', True))
    assert ghead == head[:-1] + b' XCOLORRANGE=FULL\n' and vr.last_colour == (None, 'bt709', True)


def test_two_ranks(model16, clip7, fine2, tmp_path):
    tot, got = Y._two_ranks(model16, clip7, 2, tmp_path, mfi=2, matrix='bt601', lut=CUBE)
    _same_payloads(_payloads(got)[1], LU.lut_stream_np(fine2, None, CUBE, 8, '420', 'bt601', False))
    assert tot == [N - 3, len(fine2)]


def test_with_a_crop_the_bars_stay_exact_black(model16):
    """The cube lifts black to a quarter; the bars are padded behind D2H and stay at 16 / 128."""
    big, bars = Y._clip(5, 96, 128, '420', 8, seed=4)[0], dict(batch=2, mfi=2, lut=LIFT, crop=(16, 16, 32, 32))      # a 64x64 picture
    pic = _payloads(_run(model16, big, crop_output='cropped', **bars)[3])[1]
    rect = LB.bars_rect((16, 16, 32, 32), 96, 128)
    padded = _payloads(_run(model16, big, **bars)[3])[1]
    _same_payloads(padded, [LB.pad_payload_np(p, 96, 128, 8, '420', rect, False) for p in pic])
    assert min(int(p[:64 * 64].min()) for p in pic) > 40                 # the picture's black was lifted
    assert all((p[:16 * 128] == 16).all() and (p[80 * 128:96 * 128] == 16).all() and (p[96 * 128:96 * 128 + 8 * 64] == 128).all() for p in padded)


def test_a_refused_depth_fires_first_and_the_switch_absent_adds_nothing(model16, clip7):
    deep = Y._clip(5, H, W, '420', 14, seed=4)[0]
    out = io.BytesIO()
    vr = VideoRunner(model16, 2, batch=2, mfi=2, high_depth=True, lut=CUBE)
    with pytest.raises(ValueError, match='--lut needs a working depth of 8, 10 or 12'):
        vr.run_stream(io.BytesIO(deep), out)
    assert out.getvalue() == b'' and vr._runners == {} and vr.last_lut_payloads == 0     # before anything ran or was allocated
    with pytest.raises(ValueError, match='--work-depth'):
        VideoRunner(model16, 2, mfi=2, work_depth=16, high_depth=True, lut=CUBE)
    vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2)
    rn, edge = _edge(vr)
    assert edge.stages == [] and edge.fwd is None and edge.written is edge.yuv_out and edge.spec.lut is None
    assert rn.lut_payloads == 0 and vr.last_lut_payloads == 0 and vr.last_lut is None and vr.last_colour_encoded == 0
