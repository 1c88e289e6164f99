"""Linear light and the egress matrix / range (``--linear-light``, ``--out-matrix``, ``--out-range``) on a real MI355X: the two kernels of
csrc/colour.hip equal to ``colour.linearize_np`` / ``colour.encode_payload_np`` byte for byte inside poisoned memory, and
``VideoRunner`` byte-identical to an expectation that never runs the new code: the input payloads converted on the host, run through
``ClipRunner.run_frames`` at the fine ratio, assembled in stream order and taken through ``colour.linear_stream_np``.  The clips, the model
and the stream helpers are those of tests/test_gpu_y4m_layouts.py and tests/test_gpu_dedup.py."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import bitdepth as BD                                                 # noqa: E402
from demfi_amd import colour as CL                                                   # noqa: E402
from demfi_amd import letterbox as LB                                                # noqa: E402
from demfi_amd import scale as SC                                                    # noqa: E402
from demfi_amd import shutter as SH                                                  # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_interlace as TI                                           # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
POISON = 0xC3
SIZES = [(5, 13), (37, 53), (70, 98)]                # odd: rows fall off the vector boundary, strips and 4:2:0 row pairs are cut
TABLES = {(t, d): CL.tables(t, d) for t in CL.TRANSFERS for d in (8, 10, 12)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------
def _linear_gather_gpu(frames, order, depth, fwd, shift=0, gap=0):
    """``frames`` [m, h, w, 3] (uint8 or uint16) placed ``shift`` samples behind a 16-byte boundary each; frame order[i] -> linear payload
    i, rows ``gap`` samples apart in a poisoned dst.  The poison outside the payloads and the sources come back untouched."""
    m, h, w = frames.shape[:3]
    es, F, P = frames.dtype.itemsize, h * w * 3, 3 * h * w
    pitch = -(-F * es // 16) * 16 // es + 16 // es
    buf = np.full(m * pitch + 16, 0xEEEE if es == 2 else 0xEE, frames.dtype)
    at = [i * pitch + shift for i in range(m)]
    for o, f in zip(at, frames):
        buf[o:o + F] = f.reshape(-1)
    n, stride = len(order), P + gap
    src = torch.from_numpy(buf.view(np.int16 if es == 2 else np.uint8)).to(DEV)
    offs = torch.tensor([at[a] for a in order], dtype=torch.int64, device=DEV)
    dst = torch.from_numpy(np.full(n * stride + 32, POISON * 257, np.uint16).view(np.int16)).to(DEV)
    table = _table_dev(fwd)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    L.check(L.load().demfi_bgr_to_linear_gather(src.data_ptr(), offs.data_ptr(), dst.data_ptr(), stride, n, h, w, es, depth, table.data_ptr(),
                                                _stream()), 'bgr_to_linear_gather')
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    body = out[:n * stride].reshape(n, stride)
    assert (body[:, P:] == POISON * 257).all() and (out[n * stride:] == POISON * 257).all(), 'write outside the payloads'
    assert np.array_equal(src.cpu().numpy().view(frames.dtype), buf), 'a source was written'
    return body[:, :P].reshape(n, 3, h, w)


def _frames(m, h, w, depth, seed):
    """m random frames over the whole range of the depth; the last two are all zero and all peak."""
    peak = (1 << depth) - 1
    f = np.random.default_rng(seed).integers(0, peak + 1, (m, h, w, 3)).astype(np.uint8 if depth == 8 else np.uint16)
    f[m - 2], f[m - 1] = 0, peak
    return f


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('kind', ['u8', 'u16-10', 'u16-12', 'u16-8'])
def test_linear_gather_equals_linearize_np(kind, h, w):
    """uint8 frames and uint16 frames at 10 and 12 bits (and at 8, value for value with the bytes); non-consecutive and repeated offsets;
    an aligned placement (16-byte stores where the rows allow) and one a sample off with a stride that keeps no row aligned."""
    depth = 8 if kind == 'u8' else int(kind.split('-')[1])
    frames = _frames(5, h, w, depth, h * 31 + w + depth)
    if kind == 'u16-8':
        frames = frames.astype(np.uint16)
    order = [3, 0, 0, 4, 2, 0, 3]
    for transfer in CL.TRANSFERS:
        fwd = TABLES[transfer, depth][0]
        ref = [CL.linearize_np(f, fwd) for f in frames]
        for shift, gap in ((0, -(3 * h * w) % 8), (1, 3)):
            got = _linear_gather_gpu(frames, order, depth, fwd, shift, gap)
            for i, a in enumerate(order):
                assert np.array_equal(got[i], ref[a]), (transfer, shift, i)


def test_linear_gather_of_more_frames_than_the_grid_has_rows_and_of_every_code():
    fwd = TABLES['srgb', 12][0]
    frames = _frames(3, 5, 13, 12, 1)
    n = 4096 + 7                                                         # the grid's frame dimension is 4096
    order = [(i * 5) % 3 for i in range(n)]
    got = _linear_gather_gpu(frames, order, 12, fwd, 1, 1)
    ref = np.stack([CL.linearize_np(f, fwd) for f in frames])
    assert np.array_equal(got, ref[order])
    for depth in (8, 10, 12):                                            # one frame that holds every code once per channel
        peak = (1 << depth) - 1
        hw = {8: (16, 16), 10: (32, 32), 12: (64, 64)}[depth]
        codes = np.arange(peak + 1, dtype=np.uint16)
        frame = np.stack([codes, codes[::-1], np.roll(codes, 7)], axis=-1).reshape(hw + (3,)).astype(np.uint8 if depth == 8 else np.uint16)
        for transfer in CL.TRANSFERS:
            fwd = TABLES[transfer, depth][0]
            got = _linear_gather_gpu(frame[None], [0], depth, fwd)[0]
            assert np.array_equal(got, CL.linearize_np(frame, fwd)) and np.array_equal(np.sort(got[1].reshape(-1)), fwd)


def _encode_gpu(lin, order, h, w, depth, layout, matrix, full, inv, shift=0, gap=0):
    """Linear payloads ``lin`` [m, 3 h w] uint16 placed ``shift`` BYTES behind a 16-byte boundary each; payload order[i] -> Y'CbCr payload
    i, rows ``gap`` bytes apart in a poisoned dst."""
    m, Pb_in = lin.shape[0], lin.shape[1] * 2
    es = 2 if depth > 8 else 1
    Pb = y4m.payload_size(h, w, layout) * es
    pitch = -(-Pb_in // 16) * 16 + 16
    buf = np.full(m * pitch + 16, 0xEE, np.uint8)
    at = [i * pitch + shift for i in range(m)]
    for o, p in zip(at, lin):
        buf[o:o + Pb_in] = p.astype('<u2').view(np.uint8)
    n, stride = len(order), Pb + gap
    table = np.array([at[a] for a in order], np.int64)
    src, od = torch.from_numpy(buf).to(DEV), torch.from_numpy(table).to(DEV)
    dst = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    tab = _table_dev(inv)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    L.check(L.load().demfi_linear_to_yuv(src.data_ptr(), table.ctypes.data, od.data_ptr(), n, h, w, depth, L.YUV_LAYOUT[layout], Y.MCODE[matrix],
                                         int(full), tab.data_ptr(), dst.data_ptr(), stride, _stream()), 'linear_to_yuv')
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    body = out[:n * stride].reshape(n, stride)
    assert (body[:, Pb:] == POISON).all() and (out[n * stride:] == POISON).all(), 'write outside the payloads'
    assert np.array_equal(src.cpu().numpy(), buf), 'a source was written'
    return body[:, :Pb]


def _lin_payloads(m, h, w, seed):
    x = np.random.default_rng(seed).integers(0, 65536, (m, 3 * h * w)).astype(np.uint16)
    x[m - 2], x[m - 1] = 0, 65535
    return x


@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('depth', [8, 10, 12])
def test_encode_equals_encode_payload_np(depth, layout):
    """Every layout and depth, both matrices, both ranges and both transfers over the three odd sizes; scattered and repeated offsets; an
    aligned placement and one two bytes off with a stride that keeps no row of dst aligned."""
    es = 2 if depth > 8 else 1
    order = [2, 0, 3, 3, 1]
    for k, (h, w) in enumerate(SIZES):
        lin = _lin_payloads(4, h, w, depth * 100 + k)
        for j, (transfer, matrix, full) in enumerate((('bt709', 'bt601', False), ('srgb', 'bt709', True), ('bt709', 'bt709', False),
                                                      ('srgb', 'bt601', True))):
            inv = TABLES[transfer, depth][1]
            ref = [np.ascontiguousarray(CL.encode_payload_np(p.reshape(3, h, w), inv, depth, layout, matrix, full)).view(np.uint8) for p in lin]
            Pb = len(ref[0])
            shift, gap = ((0, 32 + -Pb % 16), (2, 3 * es))[(j + k) % 2]
            got = _encode_gpu(lin, order, h, w, depth, layout, matrix, full, inv, shift, gap)
            for i, a in enumerate(order):
                assert np.array_equal(got[i], ref[a]), (h, w, transfer, matrix, full, shift, i)


@pytest.mark.parametrize('depth', [8, 10, 12])
def test_encode_of_every_linear_value(depth):
    """One 256x256 payload that holds all 65536 linear values in each plane, in three different orders."""
    v = np.arange(65536, dtype=np.uint16)
    lin = np.stack([v, v[::-1], np.roll(v, 12345)]).reshape(1, -1)
    for transfer, layout in (('bt709', '420'), ('srgb', '444')):
        inv = TABLES[transfer, depth][1]
        ref = np.ascontiguousarray(CL.encode_payload_np(lin.reshape(3, 256, 256), inv, depth, layout, 'bt709', False)).view(np.uint8)
        got = _encode_gpu(lin, [0], 256, 256, depth, layout, 'bt709', False, inv)
        assert np.array_equal(got[0], ref)
    n = 4096 + 3                                                         # and more payloads than the grid has rows
    small = _lin_payloads(3, 5, 13, depth)
    order = [(i * 7) % 3 for i in range(n)]
    inv = TABLES['bt709', depth][1]
    ref = np.stack([np.ascontiguousarray(CL.encode_payload_np(p.reshape(3, 5, 13), inv, depth, '422', 'bt601', True)).view(np.uint8) for p in small])
    assert np.array_equal(_encode_gpu(small, order, 5, 13, depth, '422', 'bt601', True, inv, 2, 2), ref[order])


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), _stream()
    src = torch.full((512,), 0x11, dtype=torch.uint8, device=DEV)
    dst = torch.full((512,), POISON, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(2, dtype=torch.int64, device=DEV)
    fwd, inv = _table_dev(TABLES['bt709', 8][0]), _table_dev(TABLES['bt709', 8][1])
    host = np.array([0, 0], np.int64)
    g_ok = (src.data_ptr(), offs.data_ptr(), dst.data_ptr(), 48, 2, 4, 4, 1, 8, fwd.data_ptr(), st)              # 4x4 frames: 48 samples
    e_ok = (src.data_ptr(), host.ctypes.data, offs.data_ptr(), 2, 4, 4, 8, 0, 0, 0, inv.data_ptr(), dst.data_ptr(), 24, st)

    def bad(fn, ok, i, v, **kw):
        a = list(ok)
        a[i] = v
        for k, x in kw.items():
            a[int(k[1:])] = x
        return fn(*a) == ERR_ARG
    g, e = lib.demfi_bgr_to_linear_gather, lib.demfi_linear_to_yuv
    assert all(bad(g, g_ok, i, None) for i in (0, 1, 2, 9)) and all(bad(e, e_ok, i, None) for i in (0, 1, 2, 10, 11))
    assert bad(g, g_ok, 4, -1) and bad(e, e_ok, 3, -1)                                       # n < 0
    assert all(bad(g, g_ok, 5, v) for v in (1, 16385)) and all(bad(e, e_ok, 5, v) for v in (1, 16385))       # frame size
    assert all(bad(g, g_ok, 8, v, a7=2) for v in (9, 14, 16, 0)) and all(bad(e, e_ok, 6, v, a12=48) for v in (9, 14, 16, 0))     # depth
    assert all(bad(g, g_ok, 7, v) for v in (0, 3, 4)) and bad(g, g_ok, 8, 10)               # sample bytes; 10-bit codes in bytes
    assert bad(g, g_ok, 3, 47) and bad(e, e_ok, 12, 23)                                      # dst_stride below the payload
    assert bad(g, g_ok, 2, dst.data_ptr() + 1) and bad(g, g_ok, 0, src.data_ptr() + 1, a7=2)   # 16-bit samples at an odd address
    assert b'demfi_bgr_to_linear_gather' in lib.demfi_last_error()
    assert all(bad(e, e_ok, 7, v) for v in (4, -1)) and all(bad(e, e_ok, 8, v) for v in (2, -1)) and all(bad(e, e_ok, 9, v) for v in (2, -1))
    for tab in ([0, -2], [1, 0]):
        assert bad(e, e_ok, 1, np.array(tab, np.int64).ctypes.data)                          # a negative or odd offset
    assert bad(e, e_ok, 0, src.data_ptr() + 1) and bad(e, e_ok, 11, dst.data_ptr() + 1, a6=10, a12=48) and bad(e, e_ok, 12, 49, a6=10)
    assert b'demfi_linear_to_yuv' in lib.demfi_last_error()
    for fn, ok, i in ((g, g_ok, 4), (e, e_ok, 3)):                                           # no payload: nothing to do
        a = list(ok)
        a[i] = 0
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0x11).all())
    assert L.ABI_VERSION == 8                                                                # the ABI only grows


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
H, W, N = 64, 96, 7


@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


@pytest.fixture(scope='module')
def clip7():
    return Y._clip(N, H, W, '420', 8, seed=3)[0]


def _run(model, data, batch=4, how='stream', tmp_path=None, **kw):
    vr = VideoRunner(model, 2, batch=batch, matrix='bt601', **kw)
    if how == 'file':
        src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
        src.write_bytes(data)
        nw, nf = vr.run_file(str(src), str(dst))
        return vr, nw, nf, dst.read_bytes()
    out = io.BytesIO()
    nw, nf = vr.run_stream(D._Pipe(data) if how == 'pipe' else io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _fine_frames(model, data, mfi):
    """The fine BGR frames of the x ``mfi`` timeline, in stream order: the input payloads converted on the host, run through
    ``ClipRunner.run_frames``, [S0, St.., S1] assembled as tests/test_gpu_y4m.py does."""
    hdr, pays = Y._read(data)
    frames = [y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, 'bt601', hdr.full_range, hdr.chroma) for p in pays]
    got = {}
    nw = ClipRunner(model, hdr.h, hdr.w, 2, mfi, batch=4).run_frames(frames, lambda k, st, s01: got.__setitem__(k, (st.numpy().copy(), s01.numpy().copy())))
    out = []
    for k in range(nw):
        st, s01 = got[k]
        out += [s01[0]] + list(st) + ([s01[1]] if k == nw - 1 else [])
    return out


@pytest.fixture(scope='module')
def fine8(model16, clip7):
    return _fine_frames(model16, clip7, 8)               # --fps at the input rate with --shutter 180: S = 4 of D = 8


@pytest.fixture(scope='module')
def fine2(model16, clip7):
    return _fine_frames(model16, clip7, 2)


def _payloads(got):
    head, pays = D._split(got)
    return head, [np.frombuffer(p, np.uint8) for p in pays]


def _same_payloads(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if not np.array_equal(a, b)]
    assert not bad, 'payloads differ: %s' % bad[:10]


SHUTTER = {'fps': '24/1', 'shutter': '180'}


@pytest.fixture(scope='module')
def shutter_ref(fine8):
    groups = SH.groups(len(fine8), N - 3 + 1, 4, 8)
    return groups, CL.linear_stream_np(fine8, groups, 'bt709', 8, '420', 'bt601', False)


def test_shutter_in_linear_light_equals_the_reference(model16, clip7, fine8, shutter_ref, tmp_path):
    groups, exp = shutter_ref
    plain = _run(model16, clip7, **SHUTTER)[3]
    head = None
    for batch, how in ((1, 'stream'), (2, 'pipe'), (4, 'file'), (2, 'stream'), (4, 'stream')):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, how=how, tmp_path=tmp_path, linear_light='bt709', **SHUTTER)
        h, pays = _payloads(got)
        _same_payloads(pays, exp)
        assert nf == len(exp) == N - 2 and (head is None or h == head)
        head = h
        assert vr.last_colour == ('bt709', 'bt601', False) and vr.last_colour_encoded == nf and vr.last_st_frames == sum(len(g) for g in groups)
    assert head == plain[:len(head)] and len(got) == len(plain) and got != plain      # the same header; light and code values mix differently
    _, pp = _payloads(plain)
    assert sum(int((a != b).sum()) for a, b in zip(pays, pp)) > 100
    srgb = _payloads(_run(model16, clip7, batch=2, linear_light='srgb', **SHUTTER)[3])[1]
    _same_payloads(srgb, CL.linear_stream_np(fine8, groups, 'srgb', 8, '420', 'bt601', False))


def test_scale_in_linear_light_and_both_with_carry_over(model16, clip7, fine2, fine8, shutter_ref):
    for size in ((72, 48), (128, 80)):                                   # a shrink and an enlargement
        vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, linear_light='bt709', scale=size)
        head, pays = _payloads(got)
        _same_payloads(pays, CL.linear_stream_np(fine2, None, 'bt709', 8, '420', 'bt601', False, scale=size + ('lanczos3',)))
        plain = _run(model16, clip7, batch=2, mfi=2, scale=size)[3]
        assert plain[:len(head)] == head and plain != got and vr.last_colour_encoded == vr.last_scale_payloads == nf == len(fine2)
    # both, at half the input rate with a 360-degree shutter of 16 samples: a written frame mixes the fine frames of two windows, so its
    # first samples carry over from one batch to the next as linear payloads
    groups = SH.groups(len(fine8), 3, 16, 16)
    exp = CL.linear_stream_np(fine8, groups, 'bt709', 8, '420', 'bt601', False, scale=(72, 48, 'bicubic'))
    for batch in (1, 2):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, linear_light='bt709', scale=(72, 48), scale_filter='bicubic', fps='12/1', down=True,
                               shutter='360', shutter_samples=16)
        _same_payloads(_payloads(got)[1], exp)
        assert (vr.last_shutter_carried > 0) == (batch == 1) and vr.last_scale_payloads == vr.last_colour_encoded == nf == 3


def test_out_matrix_and_range(model16, clip7, fine2):
    vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, out_matrix='bt709', out_range='full')
    head, pays = _payloads(got)
    _same_payloads(pays, [y4m.bgr_to_yuv_np(f, '420', 'bt709', True) for f in fine2])
    plain = _run(model16, clip7, batch=2, mfi=2)[3]
    assert head == plain[:plain.index(b'\n')] + b' XCOLORRANGE=FULL\n' and vr.last_colour == (None, 'bt709', True) and vr.last_colour_encoded == 0
    # auto goes by the height written: 720 rows behind the scaler are BT.709, the 64 of the input BT.601
    vr, _, _, auto = _run(model16, clip7, batch=2, mfi=2, out_matrix='auto', scale=(96, 720), scale_filter='bilinear')
    assert vr.last_colour == (None, 'bt709', False)
    hd = _run(model16, clip7, batch=2, mfi=2, out_matrix='bt709')[3]
    assert auto == SC.scale_stream_np(hd, 96, 720, 'bilinear') and hd != plain
    vr, _, _, same = _run(model16, clip7, batch=2, mfi=2, out_matrix='auto')
    assert vr.last_colour == (None, 'bt601', False) and same == plain


IDENTITY = {'shutter': '360', 'shutter_samples': 1, 'mfi': 2}


@pytest.mark.parametrize('case', ['8-bit', '10-bit-422', 'tiled', 'work-depth-12'])
def test_one_sample_shutter_in_linear_light_writes_the_plain_bytes(case, model16, clip7):
    """S = 1: every mix is its one sample, and inv[fwd[c]] = c, so the linear chain must hand every frame through unchanged on every frame
    path: 8-bit and 16-bit storage, tiled, and a working depth above the input's."""
    data, kw = clip7, {}
    if case == '10-bit-422':
        data, kw = Y._clip(5, H, W, '422', 10, seed=4)[0], {'high_depth': True, 'layouts': True}
    elif case == 'tiled':
        data, kw = Y._clip(5, 96, 128, '420', 8, seed=4)[0], {'tile': (64, 64), 'tile_margin': 16}
    elif case == 'work-depth-12':
        kw = {'work_depth': 12, 'out_depth': 8, 'dither': 'none'}
    plain = _run(model16, data, batch=2, **IDENTITY, **kw)[3]
    for transfer in CL.TRANSFERS:
        vr, nw, nf, got = _run(model16, data, batch=2, linear_light=transfer, **IDENTITY, **kw)
        Y._same(got, plain)
        assert vr.last_colour_encoded == nf > 0 and vr.last_colour[0] == transfer


def test_the_stages_behind_are_unchanged(model16, clip7, shutter_ref, tmp_path):
    """Interlace, requantisation and padding compose with the linear-light progressive stream exactly as with any other."""
    lin = {'linear_light': 'bt709', 'batch': 2, **SHUTTER}
    prog = _run(model16, clip7, **lin)[3]
    woven, n_woven = TI._woven(prog, 't')
    vr, _, nf, got = _run(model16, clip7, interlace='tff', **lin)
    Y._same(got, woven)
    assert nf == n_woven
    # 10-bit working depth, 8 bits out, full range out of a limited stream: the requantisation goes by the egress range
    deep = dict(lin, work_depth=10, out_range='full')
    prog10 = _run(model16, clip7, out_depth=10, **deep)[3]
    assert b'XCOLORRANGE=FULL' in prog10[:prog10.index(b'\n')] and b'C420p10' in prog10[:prog10.index(b'\n')]
    vr, _, _, got = _run(model16, clip7, out_depth=8, **deep)
    Y._same(got, BD.requant_stream_np(prog10, 8))
    # crop with pad: the black of the egress range
    big, bars = Y._clip(5, 96, 128, '420', 8, seed=4)[0], dict(lin, crop=(16, 16, 32, 32), out_range='full')     # a 64x64 picture
    head, pic = _payloads(_run(model16, big, crop_output='cropped', **bars)[3])
    rect = LB.bars_rect((16, 16, 32, 32), 96, 128)
    padded = _payloads(_run(model16, big, **bars)[3])[1]
    _same_payloads(padded, [LB.pad_payload_np(p, 96, 128, 8, '420', rect, True) for p in pic])
    assert padded[0][0] == 0                                             # full-range black, not 16


def test_scale_in_linear_light_on_two_ranks(model16, clip7, fine2, tmp_path):
    tot, got = Y._two_ranks(model16, clip7, 2, tmp_path, mfi=2, matrix='bt601', linear_light='bt709', scale=(72, 48))
    _same_payloads(_payloads(got)[1], CL.linear_stream_np(fine2, None, 'bt709', 8, '420', 'bt601', False, scale=(72, 48, 'lanczos3')))
    assert tot == [N - 3, len(fine2)]


def test_linear_light_alone_builds_nothing_and_the_refusals_fire_first(model16, clip7):
    plain = _run(model16, clip7, batch=2, mfi=2)[3]
    vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, linear_light='bt709')
    assert got == plain and vr.last_colour_encoded == 0
    edge = vr._runners[next(iter(vr._runners))].runner._pipeline.edge
    assert edge.stages == [] and edge.fwd is None and edge.written is edge.yuv_out
    deep = Y._clip(5, H, W, '420', 14, seed=4)[0]
    out = io.BytesIO()
    vr = VideoRunner(model16, 2, batch=2, mfi=2, high_depth=True, linear_light='bt709', shutter='180')
    with pytest.raises(ValueError, match='8, 10 or 12'):
        vr.run_stream(io.BytesIO(deep), out)
    assert out.getvalue() == b'' and vr._runners == {}                   # before anything ran or was allocated
    with pytest.raises(ValueError, match='8, 10 or 12'):
        VideoRunner(model16, 2, mfi=2, work_depth=16, high_depth=True, linear_light='srgb', scale=(72, 48)).run_stream(io.BytesIO(clip7), out)
    for kw in ({'linear_light': 'pq'}, {'out_matrix': 'bt2020'}, {'out_range': 'tv'}):
        with pytest.raises(ValueError):
            VideoRunner(model16, 2, mfi=2, **kw)
