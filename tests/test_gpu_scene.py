"""Scene cuts of Y4M streams (``python -m demfi_amd.video --scene-cut``) on a real MI355X: the SAD kernel bit-exact against
``scene.sad_np``, every frame of a clip with a flash between two scenes byte-identical to the module path on the clamped tuples
and the cut windows' runs, a clip without cuts unchanged by the flag, ranks with a cut at a block boundary, and the CLI."""
import io
import json
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
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.harness import module_window_ts_u8                                    # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A5A5A5A5A


# ---- SAD kernel ------------------------------------------------------------------------------------------------------------
def _sad(base, a_offs, b_offs, payload):
    n = len(a_offs)
    offs = torch.tensor(list(a_offs) + list(b_offs), dtype=torch.int64, device=DEV)
    out = torch.full((n + 1,), GUARD, dtype=torch.int64, device=DEV)
    L.check(L.load().demfi_yuv420_sad(base.data_ptr(), offs.data_ptr(), offs[n:].data_ptr(), n, payload, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), 'yuv420_sad')
    got = out.cpu().tolist()
    assert got[n] == GUARD, 'write past the n SADs'
    return got[:n]


@pytest.mark.parametrize('payload', [1, 3, 15, 16, 17, 31, 33, 255, y4m.payload_size(5, 3), y4m.payload_size(37, 53),
                                     y4m.payload_size(48, 80), 70001])
def test_sad_bit_exact_against_numpy(payload):
    g = np.random.RandomState(payload)
    host = g.randint(0, 256, 3 * payload + 67).astype(np.uint8)
    base = torch.from_numpy(host).to(DEV)
    hi = host.size - payload
    a = [0, 1, 5, hi, 3, 16, 7, 7] + [int(x) for x in g.randint(0, hi + 1, 6)]      # odd, unaligned, repeated, out of order
    b = [hi, 2, 5, 0, 16, 3, 9, 9] + [int(x) for x in g.randint(0, hi + 1, 6)]
    got = _sad(base, a, b, payload)
    assert got == [S.sad_np(host[x:x + payload], host[y:y + payload]) for x, y in zip(a, b)]


def test_sad_of_a_payload_slot_table():
    """Payloads at the slot stride the runner uses (odd sizes put the slots at every alignment)."""
    P = y4m.payload_size(37, 53)
    g = np.random.RandomState(1)
    host = g.randint(0, 256, (9, P)).astype(np.uint8)
    base = torch.from_numpy(host.reshape(-1)).to(DEV)
    pairs = [(s - 1, s) for s in range(1, 9)] + [(8, 0), (4, 4)]
    got = _sad(base, [a * P for a, _ in pairs], [b * P for _, b in pairs], P)
    assert got == [S.sad_np(host[a], host[b]) for a, b in pairs]
    assert got[-1] == 0


def test_sad_past_2_to_the_32():
    P = y4m.payload_size(4096, 4096)
    base = torch.zeros(2 * P + 5, dtype=torch.uint8, device=DEV)
    base[P + 5:] = 255
    got = _sad(base, [0, P + 5, 1], [P + 5, 0, P + 4], P)
    assert got[0] == got[1] == 255 * P > 2 ** 32
    assert got[2] == 255 * (P - 1)


def test_sad_bad_arguments_are_rejected():
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ok = (buf.data_ptr(), offs.data_ptr(), offs.data_ptr(), 2, 16, out.data_ptr(), st)
    assert lib.demfi_yuv420_sad(*ok) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return lib.demfi_yuv420_sad(*a) < 0
    assert bad(0, None) and bad(1, None) and bad(2, None) and bad(5, None)      # NULL buffers
    assert bad(3, -1)                                                           # n < 0
    assert bad(4, 0) and bad(4, -16)                                            # payload <= 0
    a = list(ok)
    a[3] = 0
    assert lib.demfi_yuv420_sad(*a) == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------
H, W = 48, 80
HDR24 = b'YUV4MPEG2 W80 H48 F24:1 Ip C420jpeg\n'
CUTS = [5, 6]                                    # frames 0-4 scene A, frame 5 a flash, frames 6-11 scene B


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


def _scene(seed, n, look):
    """n payloads of a moving crop of ``synthetic_window(seed)`` (as ``test_gpu_retime._clip_y4m``), colours mapped by look."""
    base = synthetic_window(H + 2 * n, W + 2 * n, seed)[0, :, 0]
    out = []
    for i in range(n):
        bgr = ((base[:, i:i + H, 2 * i:2 * i + W].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        out.append(y4m.bgr_to_yuv420_np(look(bgr), 'bt601', False))
    return out


def _y4m(payloads, header=HDR24):
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in payloads)


def _cut_clip():
    fr = _scene(0, 5, lambda x: x) + _scene(2, 1, lambda x: x // 4 + 190) + _scene(1, 6, lambda x: (255 - x) // 3)
    sc = S.scores([S.sad_np(fr[j], fr[j - 1]) for j in range(1, len(fr))], fr[0].size)
    for j, s in enumerate(sc, 1):
        assert (s >= S.DEFAULT_THRESHOLD) == (j in CUTS), (j, s)
    return _y4m(fr)


def _plain_clip(n=10):
    fr = _scene(0, n, lambda x: x)
    assert max(S.scores([S.sad_np(fr[j], fr[j - 1]) for j in range(1, n)], fr[0].size)) < S.DEFAULT_THRESHOLD
    return _y4m(fr)


def _stream(model, data, n_tst, batch=4, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _expected(model, data, n_tst, r, cuts, ohdr):
    """numpy YUV -> BGR, one module forward per instant of every run of ``scene.window_runs`` (the clamped tuple of an inner
    window, the left and right runs of a cut window), each output picked by the window's outputs, numpy BGR -> YUV."""
    rd = y4m.Reader(io.BytesIO(data))
    hdr = rd.header
    pays = []
    buf = np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    frames = [torch.from_numpy(y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, 'bt601', hdr.full_range, hdr.chroma)) for p in pays]
    n = len(frames)
    out = [ohdr]
    n_cut = 0
    for k in range(n - 3):
        runs, outs = S.window_runs(k, r, k == n - 4, lambda j: j in cuts)
        n_cut += len(runs) - 1
        res = [[a.cpu().numpy() for a in module_window_ts_u8(model, [frames[x] for x in S.runner_order(tup)], n_tst, ts)]
               for tup, ts in runs]
        for _, run, kind, j in outs:
            st, s01 = res[run]
            f = s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[j]
            out += [b'FRAME\n', y4m.bgr_to_yuv420_np(f, 'bt601', hdr.full_range).tobytes()]
    return b''.join(out), n_cut


@pytest.mark.parametrize('dtype,rate', [('fp16', 'mfi4'), ('fp16', 'fps60'), ('fp32', 'mfi4')])
def test_cut_clip_equals_the_module_path(dtype, rate, model16, model32):
    model = model16 if dtype == 'fp16' else model32
    data = _cut_clip()
    kw = {'mfi': 4} if rate == 'mfi4' else {'fps': Fraction(60)}
    r = Fraction(4) if rate == 'mfi4' else Fraction(5, 2)
    plain = _stream(model, data, 3, **kw)
    hdr_bytes = plain[3][:plain[3].index(b'FRAME')]
    exp, n_cut = _expected(model, data, 3, r, CUTS, hdr_bytes)
    vr, nw, nf, got = _stream(model, data, 3, scene_cut=S.DEFAULT_THRESHOLD, **kw)
    assert (nw, nf) == plain[1:3] == (9, R.n_output_frames(12, r))            # timing unchanged
    assert len(got) == len(exp) == len(plain[3])
    assert got == exp
    assert got != plain[3]
    assert vr.last_cuts == CUTS
    assert vr.last_cut_windows == n_cut == 2                                   # windows 3 (cut before 5) and 4 (before 6)


def test_no_cut_is_unchanged_by_the_flag(model16):
    data = _plain_clip()
    for kw in ({'mfi': 4}, {'fps': Fraction(60)}):
        vr0, nw0, nf0, exp = _stream(model16, data, 2, **kw)
        vr1, nw1, nf1, got = _stream(model16, data, 2, scene_cut=S.DEFAULT_THRESHOLD, **kw)
        assert (nw1, nf1) == (nw0, nf0)
        assert got == exp, kw
        assert vr1.last_instants[0] == vr0.last_instants[0], kw
        assert vr1.last_cuts == [] and vr1.last_cut_windows == 0


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_with_a_cut_at_a_block_boundary(world, model16, tmp_path):
    """9 windows: world 2 starts rank 1 at window 5, whose first cut decision (frame 6) needs the SAD of frame 5 against frame 4;
    world 3 starts blocks at windows 3 (the first cut window) and 6 (frame 6 starts scene B)."""
    data = _cut_clip()
    _, nw, nf, exp = _stream(model16, data, 2, mfi=4, scene_cut=S.DEFAULT_THRESHOLD)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    total, cut_windows = 0, 0
    for rank in range(world):
        vr = VideoRunner(model16, 2, mfi=4, batch=2, scene_cut=S.DEFAULT_THRESHOLD)
        total += vr.run_file(str(src), str(dst), world=world, rank=rank)[1]
        cut_windows += vr.last_cut_windows
    assert total == nf and cut_windows == 2
    assert dst.read_bytes() == exp


def test_cli_through_pipes(model16):
    data = _cut_clip()
    vr, nw, nf, exp = _stream(model16, data, 1, mfi=4, scene_cut=S.DEFAULT_THRESHOLD)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '4', '--n-tst', '1',
                        '--scene-cut'], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['windows'] == nw == 9 and last['frames_written'] == nf == 37 and last['cut_windows'] == 2
