"""Full-length Y4M streams (``python -m demfi_amd.video --full-length``) on a real MI355X: every frame byte-identical to the
module path on the window's clamped tuple (x 8, 24 -> 60, scene cuts next to both ends, clips of 1, 2, 3, 5 and 9 frames), the
x M windows equal to the default stream shifted by one input frame, ranks writing one file, and the CLI through pipes."""
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
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.harness import module_window_ts_u8                                    # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 80
HDR24 = b'YUV4MPEG2 W80 H48 F24:1 Ip C420jpeg\n'


@pytest.fixture(scope='module')
def model16():
    m = DeMFInet(HyperParams(), dtype=torch.float16)
    m.load_state_dict(synthetic_state_dict(0))
    return m.to(DEV).eval()


def _scene(seed, n, look=lambda x: x):
    """n payloads of a moving crop of ``synthetic_window(seed)``, colours mapped by look."""
    base = synthetic_window(H + 2 * n, W + 2 * n, seed)[0, :, 0]
    out = []
    for i in range(n):
        bgr = ((base[:, i:i + H, 2 * i:2 * i + W].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        out.append(y4m.bgr_to_yuv420_np(look(bgr), 'bt601', False))
    return out


def _y4m(payloads, header=HDR24):
    return header + b''.join(b'FRAME\n' + p.tobytes() for p in payloads)


def _stream(model, data, n_tst, batch=4, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, full_length=True, **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _frames_of(stream):
    return stream.split(b'FRAME\n')


def _same(got, exp):
    g, e = _frames_of(got), _frames_of(exp)
    assert len(g) == len(e), (len(g), len(e))
    bad = [i for i, (a, b) in enumerate(zip(g, e)) if a != b]
    assert not bad, 'frames differ (0 = header): %s' % bad[:10]


def _expected(model, data, n_tst, r, cuts=()):
    """numpy YUV -> BGR, one module forward per instant of every run of every full-length window (``scene.window_runs`` with
    the clip's ends as cuts: the clamped tuple, or the two runs of a cut window), each output picked by the window's plan --
    holds repeat their S1 -- and numpy BGR -> YUV.  Returns (stream, windows, cut windows)."""
    rd = y4m.Reader(io.BytesIO(data))
    hdr = rd.header
    pays = []
    buf = np.empty(hdr.payload, np.uint8)
    while rd.read_into(buf):
        pays.append(buf.copy())
    matrix = y4m.auto_matrix(hdr.h)
    frames = [torch.from_numpy(y4m.yuv420_to_bgr_np(p, hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma)) for p in pays]
    n = len(frames)
    is_cut = S.with_sentinels(lambda j: j in cuts, n)
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    k0, nw = R.first_window(n, True), R.n_windows(n, True)
    n_cut = 0
    for k in range(k0, k0 + nw):
        runs, outs = S.window_runs(k, r, k == k0 + nw - 1, is_cut, True)
        n_cut += len(runs) - 1
        res = [[a.cpu().numpy() for a in module_window_ts_u8(model, [frames[x] for x in S.runner_order(tup)], n_tst, ts)]
               for tup, ts in runs]
        for _, run, kind, j in outs:
            st, s01 = res[run]
            f = s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[j]
            out += [b'FRAME\n', y4m.bgr_to_yuv420_np(f, matrix, hdr.full_range).tobytes()]
    return b''.join(out), nw, n_cut


def test_x8_equals_the_module_path(model16):
    data = _y4m(_scene(3, 9))
    exp, nw_exp, _ = _expected(model16, data, 3, Fraction(8))
    vr, nw, nf, got = _stream(model16, data, 3, mfi=8)
    assert (nw, nf) == (nw_exp, 72) == (8, 9 * 8)
    _same(got, exp)
    assert vr.last_st_frames == 8 * 7 and vr.last_instants[0] == 8 * 7


def test_24_to_60_equals_the_module_path(model16):
    data = _y4m(_scene(5, 9))
    exp, nw_exp, _ = _expected(model16, data, 2, Fraction(5, 2))
    vr, nw, nf, got = _stream(model16, data, 2, batch=3, fps=Fraction(60))
    assert (nw, nf) == (nw_exp, 23) == (8, R.n_output_frames(9, Fraction(5, 2), True))
    assert got.split(b'\n', 1)[0].split()[3] == b'F60:1'
    _same(got, exp)


def _edge_cut_clip(n=8):
    """Frame 0 scene A, frames 1 .. n-2 scene B, frame n-1 scene C: cuts before frames 1 and n-1."""
    fr = _scene(0, 1) + _scene(1, n - 2, lambda x: (255 - x) // 3) + _scene(2, 1, lambda x: x // 4 + 190)
    sc = S.scores([S.sad_np(fr[j], fr[j - 1]) for j in range(1, n)], fr[0].size)
    for j, s in enumerate(sc, 1):
        assert (s >= S.DEFAULT_THRESHOLD) == (j in (1, n - 1)), (j, s)
    return _y4m(fr)


@pytest.mark.parametrize('rate', ['mfi4', 'fps60'])
def test_scene_cuts_next_to_both_ends(rate, model16):
    n = 8
    data = _edge_cut_clip(n)
    kw, r = ({'mfi': 4}, Fraction(4)) if rate == 'mfi4' else ({'fps': Fraction(60)}, Fraction(5, 2))
    exp, nw_exp, n_cut = _expected(model16, data, 2, r, cuts=(1, n - 1))
    vr, nw, nf, got = _stream(model16, data, 2, scene_cut=S.DEFAULT_THRESHOLD, **kw)
    assert (nw, nf) == (nw_exp, R.n_output_frames(n, r, True))
    _same(got, exp)
    assert vr.last_cuts == [1, n - 1]
    assert vr.last_cut_windows == n_cut == 2                       # windows -1 and n-3
    plain = _stream(model16, data, 2, **kw)[3]
    assert len(plain) == len(got) and plain != got


@pytest.mark.parametrize('n', [1, 2, 3, 5, 9])
def test_short_and_long_clips(n, model16):
    data = _y4m(_scene(7, n))
    exp, nw_exp, _ = _expected(model16, data, 1, Fraction(4))
    vr, nw, nf, got = _stream(model16, data, 1, batch=2, mfi=4)
    assert (nw, nf) == (nw_exp, 4 * n)
    _same(got, exp)
    assert vr.last_decode_peak <= 2 + 5


def test_empty_input_writes_the_header(model16):
    vr, nw, nf, got = _stream(model16, HDR24, 1, mfi=4)
    assert (nw, nf) == (0, 0)
    assert got == VideoRunner(model16, 1, 4)._out_header(y4m.parse_header(HDR24)).encode()


@pytest.mark.parametrize('m', [2, 4])
def test_x_m_is_the_default_stream_shifted_by_one_input_frame(m, model16):
    n = 9
    data = _y4m(_scene(11, n))
    full = _frames_of(_stream(model16, data, 2, mfi=m)[3])
    out = io.BytesIO()
    VideoRunner(model16, 2, m).run_stream(io.BytesIO(data), out)
    dflt = _frames_of(out.getvalue())
    assert full[0] == dflt[0]                                      # the header
    assert len(full) - 1 == n * m and len(dflt) - 1 == (n - 3) * m + 1
    assert full[1 + m:1 + m + (n - 3) * m] == dflt[1:1 + (n - 3) * m]


@pytest.mark.parametrize('kw', [{'mfi': 4}, {'fps': Fraction(60)}, {'mfi': 4, 'scene_cut': S.DEFAULT_THRESHOLD}],
                         ids=['mfi4', 'fps60', 'mfi4-cuts'])
@pytest.mark.parametrize('world', [2, 3])
def test_ranks_equal_the_stream(world, kw, model16, tmp_path):
    data = _edge_cut_clip(8) if 'scene_cut' in kw else _y4m(_scene(13, 8))
    _, nw, nf, exp = _stream(model16, data, 1, **kw)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    tw = tf = 0
    for rank in range(world):
        w, f = VideoRunner(model16, 1, batch=2, full_length=True, **kw).run_file(str(src), str(dst), world=world, rank=rank)
        tw, tf = tw + w, tf + f
    assert (tw, tf) == (nw, nf)
    _same(dst.read_bytes(), exp)


def test_cli_through_pipes(model16):
    data = _edge_cut_clip(8)
    vr, nw, nf, exp = _stream(model16, data, 1, fps=Fraction(60), scene_cut=S.DEFAULT_THRESHOLD)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--fps', '60', '--n-tst', '1',
                        '--scene-cut', '--full-length'], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env,
                       timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['windows'] == nw == 7 and last['frames_written'] == nf == 20 and last['cut_windows'] == 2
