"""Y4M stream edge on a real MI355X: the colour conversion kernels bit-exact against their numpy definition, and the video
pipeline (in-process, two ranks writing one file, and ``python -m demfi_amd.video - -`` through pipes) byte-identical to the
expectation built from the numpy definition and the existing clip pipeline."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict, synthetic_window   # noqa: E402
from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCODE = {'bt601': L.BT601, 'bt709': L.BT709}
SCODE = {'420jpeg': L.SITING_420JPEG, '420mpeg2': L.SITING_420MPEG2}
GUARD = 0xA5


def _yuv_to_bgr_gpu(pays, h, w, matrix, full, siting, src_pad=0, dst_pad=0):
    """pays [n, P] numpy -> [n, h, w, 3] through demfi_yuv420_to_bgr with padded strides; the padding must stay untouched."""
    n, P = pays.shape
    F = h * w * 3
    src = torch.zeros((n, P + src_pad), dtype=torch.uint8)
    src[:, :P] = torch.from_numpy(pays)
    src = src.to(DEV)
    dst = torch.full((n, F + dst_pad), GUARD, dtype=torch.uint8, device=DEV)
    L.check(L.load().demfi_yuv420_to_bgr(src.data_ptr(), P + src_pad, dst.data_ptr(), F + dst_pad, n, h, w, MCODE[matrix], int(full),
                                         SCODE[siting], torch.cuda.current_stream().cuda_stream), 'yuv420_to_bgr')
    out = dst.cpu().numpy()
    assert (out[:, F:] == GUARD).all(), 'write outside the frames'
    return out[:, :F].reshape(n, h, w, 3)


def _bgr_to_yuv_gpu(frames, matrix, full, group=0, gap=0, dst_pad=0):
    """frames [n, h, w, 3] numpy -> [n, P] through demfi_bgr_to_yuv420; with group > 0 the source holds `group` frames per
    block and `gap` spare frames between blocks (the two-level addressing of the egress)."""
    n, h, w = frames.shape[:3]
    F, P = h * w * 3, y4m.payload_size(h, w)
    g = group or n
    nblk = (n + g - 1) // g
    src = torch.zeros((nblk, g + gap, F), dtype=torch.uint8)
    for i in range(n):
        src[i // g, i % g] = torch.from_numpy(frames[i].reshape(-1))
    src = src.to(DEV)
    dst = torch.full((n, P + dst_pad), GUARD, dtype=torch.uint8, device=DEV)
    L.check(L.load().demfi_bgr_to_yuv420(src.data_ptr(), F, group, (g + gap) * F, dst.data_ptr(), P + dst_pad, n, h, w, MCODE[matrix],
                                         int(full), torch.cuda.current_stream().cuda_stream), 'bgr_to_yuv420')
    out = dst.cpu().numpy()
    assert (out[:, P:] == GUARD).all(), 'write outside the payloads'
    return out[:, :P]


SIZES = [(2, 2), (3, 5), (5, 3), (37, 53), (70, 98), (64, 128), (720, 1280)]


@pytest.mark.parametrize('h,w', SIZES)
@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
@pytest.mark.parametrize('full', [False, True])
def test_kernels_bit_exact_against_numpy(h, w, matrix, full):
    g = np.random.RandomState(h * 7 + w)
    pays = g.randint(0, 256, (2, y4m.payload_size(h, w))).astype(np.uint8)
    for siting in y4m.SITINGS:
        got = _yuv_to_bgr_gpu(pays, h, w, matrix, full, siting)
        for i in range(2):
            assert np.array_equal(got[i], y4m.yuv420_to_bgr_np(pays[i], h, w, matrix, full, siting)), (siting, i)
    bgr = g.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    got = _bgr_to_yuv_gpu(bgr, matrix, full)
    for i in range(2):
        assert np.array_equal(got[i], y4m.bgr_to_yuv420_np(bgr[i], matrix, full)), i


@pytest.mark.parametrize('h,w', [(37, 53), (64, 128), (70, 98)])
@pytest.mark.parametrize('pad', [0, 8, 13])
def test_strided_batches(h, w, pad):
    """Several frames per launch at strides larger than a frame (aligned and not), and the grouped source addressing."""
    g = np.random.RandomState(pad)
    pays = g.randint(0, 256, (5, y4m.payload_size(h, w))).astype(np.uint8)
    got = _yuv_to_bgr_gpu(pays, h, w, 'bt709', False, '420mpeg2', src_pad=pad, dst_pad=2 * pad)
    for i in range(5):
        assert np.array_equal(got[i], y4m.yuv420_to_bgr_np(pays[i], h, w, 'bt709', False, '420mpeg2')), i
    bgr = g.randint(0, 256, (7, h, w, 3)).astype(np.uint8)
    got = _bgr_to_yuv_gpu(bgr, 'bt601', True, group=3, gap=1, dst_pad=pad)
    for i in range(7):
        assert np.array_equal(got[i], y4m.bgr_to_yuv420_np(bgr[i], 'bt601', True)), i


def test_bad_arguments_are_rejected():
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.demfi_yuv420_to_bgr(buf.data_ptr(), 6, buf.data_ptr(), 12, 1, 1, 2, 0, 0, 0, st) < 0       # h < 2
    assert lib.demfi_yuv420_to_bgr(buf.data_ptr(), 6, buf.data_ptr(), 12, 1, 2, 2, 2, 0, 0, st) < 0       # matrix
    assert lib.demfi_yuv420_to_bgr(buf.data_ptr(), 6, buf.data_ptr(), 12, 1, 2, 2, 0, 0, 5, st) < 0       # siting
    assert lib.demfi_yuv420_to_bgr(buf.data_ptr(), 5, buf.data_ptr(), 12, 2, 2, 2, 0, 0, 0, st) < 0       # stride < payload
    assert lib.demfi_bgr_to_yuv420(buf.data_ptr(), 12, 0, 0, buf.data_ptr(), 5, 2, 2, 2, 0, 0, st) < 0    # stride < payload
    assert lib.demfi_bgr_to_yuv420(None, 12, 0, 0, buf.data_ptr(), 6, 1, 2, 2, 0, 0, st) < 0


# ---- end to end ------------------------------------------------------------------------------------------------------------
H, W = 70, 98


def _model(dtype):
    m = DeMFInet(HyperParams(), dtype=dtype)
    m.load_state_dict(synthetic_state_dict(0))
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def model16():
    return _model(torch.float16)


@pytest.fixture(scope='module')
def model32():
    return _model(torch.float32)


def _clip_y4m(n, header, matrix, full, seed=0):
    """A seeded clip of n frames of a moving pattern as a Y4M stream (bytes)."""
    base = synthetic_window(H + 2 * n, W + 2 * n, seed)[0, :, 0]
    out = [header]
    for i in range(n):
        f = base[:, i:i + H, 2 * i:2 * i + W]
        bgr = ((f.permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        out += [b'FRAME\n', y4m.bgr_to_yuv420_np(bgr, matrix, full).tobytes()]
    return b''.join(out)


def _expected(model, data, n_tst, mfi, matrix, batch=4):
    """numpy YUV -> BGR, ClipRunner.run_frames, frames in stream order, numpy BGR -> YUV."""
    rd = y4m.Reader(io.BytesIO(data))
    hdr = rd.header
    pays = []
    buf = np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    frames = [y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma) for p in pays]
    got = {}
    cr = ClipRunner(model, hdr.h, hdr.w, n_tst, mfi, batch=batch)
    nw = cr.run_frames(frames, lambda k, st, s01: got.__setitem__(k, (st.numpy().copy(), s01.numpy().copy())))
    assert nw == len(frames) - 3
    out = [y4m.output_header(hdr, mfi).encode()]
    for k in range(nw):
        st, s01 = got[k]
        seq = [s01[0]] + list(st) + ([s01[1]] if k == nw - 1 else [])
        for f in seq:
            out += [b'FRAME\n', y4m.bgr_to_yuv420_np(f, matrix, hdr.full_range).tobytes()]
    return b''.join(out)


CASES = [  # (dtype, n_tst, mfi, header, matrix, full range)
    ('fp16', 3, 8, b'YUV4MPEG2 W98 H70 F25:1 Ip A1:1 C420jpeg\n', 'bt601', False),
    ('fp32', 3, 2, b'YUV4MPEG2 W98 H70 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n', 'bt601', True),
]


@pytest.mark.parametrize('case', CASES, ids=['x8_fp16', 'x2_fp32'])
def test_video_stream_and_ranks_equal_the_frame_pipeline(case, model16, model32, tmp_path):
    dtype, n_tst, mfi, header, matrix, full = case
    model = model16 if dtype == 'fp16' else model32
    data = _clip_y4m(9, header, matrix, full, seed=3)
    exp = _expected(model, data, n_tst, mfi, matrix)
    assert len(exp) == len(y4m.output_header(y4m.parse_header(header), mfi).encode()) + (6 * mfi + 1) * (6 + y4m.payload_size(H, W))
    vr = VideoRunner(model, n_tst, mfi, batch=4)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    assert (nw, nf) == (6, 6 * mfi + 1)
    assert out.getvalue() == exp
    assert vr.last_decode_peak <= 4 + 5
    # two ranks of one file, run one after the other in this process (rank 0 sizes the file first)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tot = [0, 0]
    for r in range(2):
        nw_r, nf_r = VideoRunner(model, n_tst, mfi, batch=2).run_file(str(src), str(dst), world=2, rank=r)
        tot[0] += nw_r
        tot[1] += nf_r
    assert tot == [6, 6 * mfi + 1]
    assert dst.read_bytes() == exp


def test_cli_through_pipes(model16):
    data = _clip_y4m(7, b'YUV4MPEG2 W98 H70 F24:1 Ip\n', 'bt601', False, seed=5)
    out = io.BytesIO()
    VideoRunner(model16, 1, 4, batch=4).run_stream(io.BytesIO(data), out)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '4', '--n-tst', '1'], input=data,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == out.getvalue()
    last = p.stderr.decode().strip().splitlines()[-1]
    assert '"windows": 4' in last and '"frames_written": 17' in last
