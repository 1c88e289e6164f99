"""Retimed Y4M streams (``python -m demfi_amd.video --fps``) on a real MI355X: the gather egress kernel bit-exact against its numpy
definition, ``--fps M*F_in`` byte-identical to ``--mfi M``, every frame of 24 -> 60, 25 -> 60 and r = 1 byte-identical to the
module path at that frame's t, the padded-chunk and non-batched plans, and the CLI through pipes."""
import io
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict, synthetic_window   # noqa: E402
from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.harness import module_window_ts_u8                                    # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCODE = {'bt601': L.BT601, 'bt709': L.BT709}
GUARD = 0x5A


# ---- gather egress kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(48, 80), (64, 96), (37, 53), (5, 3)])
@pytest.mark.parametrize('matrix,full', [('bt601', False), ('bt709', True)])
@pytest.mark.parametrize('pad', [0, 13])
def test_gather_bit_exact_against_numpy(h, w, matrix, full, pad):
    g = np.random.RandomState(h * 31 + w + pad)
    F, P = h * w * 3, y4m.payload_size(h, w)
    nb = 6
    frames = g.randint(0, 256, (nb, h, w, 3)).astype(np.uint8)
    fstride = F + pad                                                  # source frames at a padded stride
    base = torch.zeros(nb * fstride + 64, dtype=torch.uint8)
    for i in range(nb):
        base[i * fstride:i * fstride + F] = torch.from_numpy(frames[i].reshape(-1))
    base = base.to(DEV)
    order = [4, 0, 0, 5, 2, 2, 1, 3, 4]                                # out of order and repeated
    offs = torch.tensor([i * fstride for i in order], dtype=torch.int64, device=DEV)
    dstride = P + 2 * pad + 3
    dst = torch.full((len(order) * dstride,), GUARD, dtype=torch.uint8, device=DEV)
    before = base.clone()
    L.check(L.load().demfi_bgr_to_yuv420_gather(base.data_ptr(), offs.data_ptr(), dst.data_ptr(), dstride, len(order), h, w,
                                                MCODE[matrix], int(full), torch.cuda.current_stream().cuda_stream), 'gather')
    out = dst.cpu().numpy().reshape(len(order), dstride)
    for f, i in enumerate(order):
        assert np.array_equal(out[f, :P], y4m.bgr_to_yuv420_np(frames[i], matrix, full)), (f, i)
    assert (out[:, P:] == GUARD).all(), 'write outside the payloads'
    assert torch.equal(base, before)


def test_gather_bad_arguments_are_rejected():
    lib = L.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = y4m.payload_size(2, 2)
    ok = (buf.data_ptr(), offs.data_ptr(), buf.data_ptr(), p, 2, 2, 2, 0, 0, st)
    assert lib.demfi_bgr_to_yuv420_gather(*ok) == 0
    torch.cuda.synchronize()

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return lib.demfi_bgr_to_yuv420_gather(*a) < 0
    assert bad(0, None) and bad(1, None) and bad(2, None)              # NULL buffers
    assert bad(3, p - 1)                                               # dst_stride < payload
    assert bad(4, -1)                                                  # n < 0
    assert bad(5, 1) and bad(6, 1) and bad(5, 16385) and bad(6, 16385)  # h, w outside 2..16384
    assert bad(7, 2) and bad(8, 2)                                     # matrix, full_range


# ---- end to end ------------------------------------------------------------------------------------------------------------
H, W = 48, 80


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


def _clip_y4m(n, header, matrix='bt601', full=False, seed=0):
    base = synthetic_window(H + 2 * n, W + 2 * n, seed)[0, :, 0]
    out = [header]
    for i in range(n):
        f = base[:, i:i + H, 2 * i:2 * i + W]
        bgr = ((f.permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        out += [b'FRAME\n', y4m.bgr_to_yuv420_np(bgr, matrix, full).tobytes()]
    return b''.join(out)


def _stream(model, data, n_tst, batch=4, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _ranks(model, data, n_tst, tmp_path, world=2, **kw):
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    nf = 0
    for r in range(world):
        nf += VideoRunner(model, n_tst, batch=2, **kw).run_file(str(src), str(dst), world=world, rank=r)[1]
    return nf, dst.read_bytes()


@pytest.mark.parametrize('m', [2, 4])
def test_fps_m_times_input_equals_mfi_m(m, model16, tmp_path):
    data = _clip_y4m(10, b'YUV4MPEG2 W80 H48 F24000:1001 Ip A1:1 C420jpeg\n', seed=m)
    _, nw, nf, exp = _stream(model16, data, 3, mfi=m)
    vr, nw2, nf2, got = _stream(model16, data, 3, fps=Fraction(24000, 1001) * m)
    assert (nw2, nf2) == (nw, nf) == (7, 7 * m + 1)
    assert got == exp
    assert vr.last_instants[0] == 7 * max(1, m - 1) and vr.last_st_frames == 7 * (m - 1)
    nfr, got = _ranks(model16, data, 3, tmp_path, fps=Fraction(24000, 1001) * m)
    assert nfr == nf and got == exp


def _module_expected(model, data, n_tst, fps):
    """numpy YUV -> BGR, one module forward per instant of every window (``module_window_ts_u8``), each output frame picked by
    the schedule, numpy BGR -> YUV."""
    rd = y4m.Reader(io.BytesIO(data))
    hdr = rd.header
    pays = []
    buf = np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    matrix = y4m.auto_matrix(hdr.h)
    frames = [torch.from_numpy(y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma)) for p in pays]
    r = R.ratio(hdr.fps, fps)
    n = len(frames)
    out = [R.output_header(hdr, fps).encode()]
    for k in range(n - 3):
        ts, outs = R.window_plan(k, r, last=k == n - 4)
        st, s01 = (a.cpu().numpy() for a in module_window_ts_u8(model, [frames[k + 1], frames[k + 2], frames[k], frames[k + 3]], n_tst, ts))
        for _, kind, j in outs:
            f = s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[j]
            out += [b'FRAME\n', y4m.bgr_to_yuv420_np(f, matrix, hdr.full_range).tobytes()]
    return b''.join(out)


RETIMES = [  # (input header, F_out, expected frames for 9 input frames)
    (b'YUV4MPEG2 W80 H48 F24:1 Ip C420jpeg\n', Fraction(60), 16),
    (b'YUV4MPEG2 W80 H48 F25:1 Ip C420mpeg2 XCOLORRANGE=FULL\n', Fraction(60), 15),
    (b'YUV4MPEG2 W80 H48 F30000:1001 Ip\n', Fraction(30000, 1001), 7),
]


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
@pytest.mark.parametrize('case', RETIMES, ids=['24to60', '25to60', 'r1'])
def test_retimed_frames_equal_the_module_path(case, dtype, model16, model32):
    """On the module's shared models, after the other tests' runners have come and gone on the same engines."""
    header, fps, nf_exp = case
    model = model16 if dtype == 'fp16' else model32
    full = b'FULL' in header
    data = _clip_y4m(9, header, 'bt601', full, seed=11)
    exp = _module_expected(model, data, 3, fps)
    vr, nw, nf, got = _stream(model, data, 3, fps=fps)
    assert (nw, nf) == (6, nf_exp)
    assert len(got) == len(exp)
    assert got == exp
    r = R.ratio(y4m.parse_header(header).fps, fps)
    assert vr.last_instants[0] == sum(max(1, len(R.instants(k, r))) for k in range(6))


def test_one_runner_two_input_rates_fp32(model32):
    """One VideoRunner(fps=60) on one fp32 model: a 24 fps input (batched plan, n_ctx 2) and then a 25 fps input (non-batched
    plan, n_ctx 1, a second runner on the same model), each against the module path."""
    vr = VideoRunner(model32, 3, batch=4, fps=Fraction(60))
    for header, nf_exp in [(b'YUV4MPEG2 W80 H48 F24:1 Ip\n', 16), (b'YUV4MPEG2 W80 H48 F25:1 Ip C420mpeg2 XCOLORRANGE=FULL\n', 15)]:
        data = _clip_y4m(9, header, 'bt601', b'FULL' in header, seed=13)
        exp = _module_expected(model32, data, 3, Fraction(60))
        out = io.BytesIO()
        assert vr.run_stream(io.BytesIO(data), out) == (6, nf_exp)
        assert out.getvalue() == exp, header
    assert sorted(cr.runner.n_ctx for cr in vr._runners.values()) == [1, 2]


def test_a_new_runner_on_a_used_engine_writes_nothing_before_its_run(model16):
    """A runner takes over the model's cached engine, whose uint8 sink records may still point at the output buffers of a runner
    that is gone (and at memory that now belongs to someone else).  Its warm-up must not fire them: every record is aimed at a
    guard buffer here, and the next runner on the same engines leaves the guard untouched and writes the right bytes."""
    data = _clip_y4m(8, b'YUV4MPEG2 W80 H48 F24:1 Ip\n', seed=17)
    for fps in (Fraction(60), Fraction(24)):                           # batched (n_ctx 2) and non-batched (n_ctx 1) plans
        exp = _stream(model16, data, 3, fps=fps)[3]
        guard = torch.full((3, H, W, 3), GUARD, dtype=torch.uint8, device=DEV)
        rec = torch.zeros(32, dtype=torch.int64)
        rec[0], rec[1], rec[2] = guard[0].data_ptr(), guard[1].data_ptr(), guard[2].data_ptr()
        rec[8], rec[9] = H | (W << 32), 3 - 1
        rec = rec.to(DEV)
        for eng in model16._engines.values():
            for row in eng._ctxs:
                for ctx in row:
                    ctx['sink'][:32].copy_(rec)
        got = _stream(model16, data, 3, fps=fps)[3]
        torch.cuda.synchronize()
        assert (guard == GUARD).all(), 'a stale sink record fired (fps %s)' % fps
        assert got == exp


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_at_a_non_integer_ratio(world, model16, tmp_path):
    """24 -> 60 over ranks: blocks start at windows with and without S0, and the file equals the one-rank stream."""
    data = _clip_y4m(10, b'YUV4MPEG2 W80 H48 F24:1 Ip\n', seed=19)
    _, nw, nf, exp = _stream(model16, data, 2, fps=Fraction(60))
    assert (nw, nf) == (7, 18)
    nfr, got = _ranks(model16, data, 2, tmp_path, world=world, fps=Fraction(60))
    assert nfr == nf and got == exp


def test_n_ctx_variants_give_the_same_bytes(model16):
    """24 -> 60 and 25 -> 60 with n_ctx 1 (non-batched), 2 and 3 (padded chunks): the same bytes; the instant counters follow
    the chunking."""
    for header, fps in [(b'YUV4MPEG2 W80 H48 F24:1 Ip\n', Fraction(60)), (b'YUV4MPEG2 W80 H48 F25:1 Ip\n', Fraction(60))]:
        data = _clip_y4m(11, header, seed=7)
        r = R.ratio(y4m.parse_header(header).fps, fps)
        counts = [max(1, len(R.instants(k, r))) for k in range(8)]
        ref = None
        for n_ctx in (1, 2, 3):
            vr, nw, nf, got = _stream(model16, data, 2, batch=3, fps=fps, n_ctx=n_ctx)
            assert nw == 8 and nf == R.n_output_frames(11, r)
            ref = got if ref is None else ref
            assert got == ref, (header, n_ctx)
            assert vr.last_instants == (sum(counts), sum(-c % n_ctx for c in counts) if n_ctx > 1 else 0), (header, n_ctx)


def test_cli_through_pipes(model16):
    data = _clip_y4m(8, b'YUV4MPEG2 W80 H48 F24:1 Ip\n', seed=5)
    _, nw, nf, exp = _stream(model16, data, 1, fps=Fraction(60))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--fps', '60', '--n-tst', '1'],
                       input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert nf == R.n_output_frames(8, Fraction(5, 2)) == 13
    assert p.stdout.split(b'\n', 1)[0].split()[3] == b'F60:1'
    assert p.stdout == exp
    last = p.stderr.decode().strip().splitlines()[-1]
    assert '"windows": 5' in last and '"frames_written": 13' in last and '"fps_out": "60"' in last
    assert '"instants_run": 10' in last
