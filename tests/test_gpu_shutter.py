"""The synthesized shutter (``--shutter``) on a real MI355X: ``demfi_payload_mix`` (csrc/shutter.hip) equal to ``shutter.mix_np`` bit for
bit, and ``VideoRunner(shutter=...)`` byte-identical to an expectation that never runs the new code: the fine stream a run WITHOUT the
switch writes at the ratio r D from the same input, mixed on the host by ``mix_np`` over ``shutter.groups``.  The clips, the model and the
stream helpers are those of tests/test_gpu_y4m_layouts.py and tests/test_gpu_dedup.py."""
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

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import shutter as SH                                                  # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
POISON = 0xC3


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _sources(m, P, es, seed):
    """m source payloads of P samples: random ones over the whole range, then an all-zero and an all-peak one."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256 ** es, (m, P)).astype('<u2' if es == 2 else np.uint8)
    x[m - 2], x[m - 1] = 0, 256 ** es - 1
    return x.view(np.uint8).reshape(m, P * es)


def _rows(n, smax, m):
    """n rows of kept sources: full rows (smax kept), truncated ones (down to one) and rows of the all-peak source alone."""
    rng = np.random.default_rng(n * 131 + smax)
    rows = []
    for i in range(n):
        k = smax if i % 3 == 0 else 1 + (i * 7) % smax
        rows.append([m - 1] * k if i % 5 == 4 else list(rng.integers(0, m, k)))
    return rows


def _mix_gpu(src, rows, smax, P, es, shift, gap):
    """``src`` [m, P es] placed ``shift`` bytes behind a 16-byte boundary each, rows of indices into it -> the mixed rows [n, P es]; the
    poisoned bytes between the rows of dst and behind the last one come back untouched, and so do the sources."""
    lib, n, Pb = L.load(), len(rows), P * es
    pitch = -(-Pb // 16) * 16 + 16
    buf = np.full(len(src) * pitch + 16, 0xEE, np.uint8)
    offs_src = [i * pitch + shift for i in range(len(src))]
    for o, p in zip(offs_src, src):
        buf[o:o + Pb] = p
    stride = Pb + gap
    table = np.full((n, smax), -1, np.int64)
    for r, ks in enumerate(rows):
        table[r, :len(ks)] = [offs_src[j] for j in ks]
    dev = torch.from_numpy(buf).to(DEV)
    assert dev.data_ptr() % 16 == 0
    od = torch.from_numpy(table).to(DEV)
    dst = torch.full((n * stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    L.check(lib.demfi_payload_mix(dev.data_ptr(), table.ctypes.data, od.data_ptr(), n, smax, P, es, dst.data_ptr(), stride,
                                  torch.cuda.current_stream().cuda_stream), 'payload_mix')
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    body = out[:n * stride].reshape(n, stride)
    assert (body[:, Pb:] == POISON).all() and (out[n * stride:] == POISON).all(), 'write outside the payloads'
    assert np.array_equal(dev.cpu().numpy(), buf)
    return body[:, :Pb]


def _check_kernel(P, es, smax, n, shift, gap, seed=0):
    m = smax + 3
    src = _sources(m, P, es, seed + P + smax)
    rows = _rows(n, smax, m)
    got = _mix_gpu(src, rows, smax, P, es, shift, gap)
    want = SH.mix_np(src, rows, es)
    diff = int((got != want).sum())
    print('P=%d es=%d smax=%d n=%d shift=%d gap=%d: %d of %d bytes differ' % (P, es, smax, n, shift, gap, diff, want.size))
    assert np.array_equal(got, want)
    peak_rows = [r for r, ks in enumerate(rows) if set(ks) == {m - 1}]
    assert all((got[r] == 0xFF).all() for r in peak_rows) and (peak_rows or n < 5)      # k peaks average to the peak, up to 32 x 65535


@pytest.mark.parametrize('es', [1, 2], ids=['bytes', '16-bit'])
@pytest.mark.parametrize('P', [1, 15, 16, 17, 33, 4099, 64 * 96 * 3 // 2])
def test_kernel_equals_the_numpy_definition(P, es):
    """Aligned sources, dst and stride take the 16-byte path (with its sample-by-sample tail when P es is no multiple of 16); sources at odd
    byte offsets (2 mod 16 for 16-bit samples) and an odd stride take the sample-by-sample path."""
    for smax in (1, 2, 5, 32):
        for n in (1, 37):
            _check_kernel(P, es, smax, n, 0, 32 + -(P * es) % 16)        # the vector path: the gap makes the stride a multiple of 16
            _check_kernel(P, es, smax, n, 1 if es == 1 else 2, 3 if es == 1 else 6)
    _check_kernel(P, es, 5, 3, 0, 8)                                     # aligned sources, a stride that is not: sample by sample


def test_rows_and_chunks_beyond_one_grid():
    _check_kernel(1, 1, 1, 4099, 0, 16)                                  # more rows than the grid has: rows are strided over
    _check_kernel(4096 * 256 * 16 + 4099, 1, 2, 2, 0, 13 + 16)           # more 4 KiB chunks than the grid has: chunks are strided over
    _check_kernel(4096 * 256 + 77, 1, 2, 2, 1, 3)                        # and on the sample-by-sample path, whose chunks are 256 samples


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((64,), POISON, dtype=torch.uint8, device=DEV)
    table = np.array([[0, 32, -1], [64, -1, -1]], np.int64)
    od = torch.from_numpy(table).to(DEV)
    fn = lib.demfi_payload_mix
    ok = (src.data_ptr(), table.ctypes.data, od.data_ptr(), 2, 3, 16, 1, dst.data_ptr(), 32, st)

    def bad(i, v, tab=None):
        a = list(ok)
        a[i] = v
        if tab is not None:
            a[1] = tab.ctypes.data
        return fn(*a) == ERR_ARG
    assert all(bad(i, None) for i in (0, 1, 2, 7))
    assert all(bad(4, v) for v in (0, 33, -1)) and all(bad(6, v) for v in (0, 3, 4)) and bad(5, 0) and bad(8, 15)
    for tab in ([[0, 32, -1], [-1, -1, -1]], [[0, -1, 32], [64, -1, -1]], [[0, 32, -2], [64, -1, -1]]):
        assert bad(3, 2, np.array(tab, np.int64))                        # a row that keeps nothing; a kept offset behind a -1; a bad offset
    assert b'demfi_payload_mix' in lib.demfi_last_error()
    odd = np.array([[1, -1, -1], [64, -1, -1]], np.int64)
    a = list(ok)
    a[1], a[5], a[6] = odd.ctypes.data, 8, 2                             # 16-bit samples at an odd address
    assert fn(*a) == ERR_ARG
    a = list(ok)
    a[5], a[6], a[8] = 8, 2, 17                                          # and at an odd stride
    assert fn(*a) == ERR_ARG
    for n in (0, -3):                                                    # no row: nothing to do, nothing written
        a = list(ok)
        a[3] = n
        assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((dst == POISON).all()) and bool((src == 0xA5).all())
    assert fn(*ok) == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:16] == 0xA5).all() and (out[32:48] == 0xA5).all() and (out[16:32] == POISON).all() and (out[48:] == POISON).all()
    assert L.ABI_VERSION == 8                                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _run(model, data, batch=4, pipe=False, **kw):
    vr = VideoRunner(model, 2, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(D._Pipe(data) if pipe else io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _run_file(model, data, tmp_path, **kw):
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    vr = VideoRunner(model, 2, batch=kw.pop('batch', 4), matrix='bt601', **kw)
    nw, nf = vr.run_file(str(src), str(dst))
    return vr, nw, nf, dst.read_bytes()


def _ratios(data, rate):
    hdr = y4m.parse_header(data[:data.index(b'FRAME\n')], y4m.DEPTHS, y4m.LAYOUTS)
    return hdr, (Fraction(rate['mfi']) if 'mfi' in rate else R.ratio(hdr.fps, rate['fps']))


def _fine_rate(data, rate, d):
    hdr, r = _ratios(data, rate)
    return {'mfi': int(r * d)} if 'mfi' in rate else {'fps': hdr.fps * r * d}


def _scenes(n, r, full, cuts):
    """The scene of every frame of the stream at ratio r over n input frames with cuts before the frames ``cuts`` (``scene.window_runs``)."""
    is_cut = S.with_sentinels(lambda j: j in cuts, n) if full else (lambda j: j in cuts)
    k0, nw, scene_of, sc = R.first_window(n, full), R.n_windows(n, full), {}, 0
    for k in range(k0, k0 + nw):
        runs, outs = S.window_runs(k, r, k == k0 + nw - 1, is_cut, full)
        for i, run, _, _ in outs:
            scene_of[i] = sc + (run if len(runs) > 1 else 0)
        sc += len(runs) - 1
    return scene_of


def _mixed(fine, data, rate, s, d, full=False, cuts=None):
    """The expectation: the fine stream's payloads mixed on the host; the header of the stream at the ratio r.  Returns (bytes, groups)."""
    hdr, r = _ratios(data, rate)
    n = data.count(b'FRAME\n')
    head, pays = D._split(fine)
    n_out = R.n_output_frames(n, r, full)
    assert len(pays) == R.n_output_frames(n, r * d, full)
    scene_of = _scenes(n, r * d, full, cuts).get if cuts else None
    groups = SH.groups(len(pays), n_out, s, d, scene_of)
    x = np.stack([np.frombuffer(p, np.uint8) for p in pays]) if pays else np.zeros((0, hdr.payload), np.uint8)
    out = SH.mix_np(x, groups, 2 if hdr.depth > 8 else 1) if groups else x[:0]
    return R.output_header(hdr, hdr.fps * r).encode() + b''.join(b'FRAME\n' + p.tobytes() for p in out), groups


def _instants(n, r, s, d, full=False):
    """The instants ``filter_plan`` leaves of the windows of an n-frame clip without cuts at the fine ratio r d."""
    k0, nw = R.first_window(n, full), R.n_windows(n, full)
    total = 0
    for k in range(k0, k0 + nw):
        ts, o = R.window_plan(k, r * d, k == k0 + nw - 1, full)
        total += len(SH.filter_plan([(None, ts)], [(i, 0, kind, j) for i, kind, j in o], s, d)[0][0][1])
    return total


@pytest.fixture(scope='module')
def clip7():
    return Y._clip(7, 64, 96, '420', 8, seed=3)[0]


@pytest.fixture(scope='module')
def fine7(model16, clip7):
    """The stream ``--mfi 8`` writes of the seven-frame clip: the fine stream of ``--mfi 2 --shutter 180 --shutter-samples 2``."""
    vr, nw, nf, out = _run(model16, clip7, mfi=8)
    return vr, out


def test_a_stream_equals_the_mix_of_the_fine_stream_at_every_batch_size(model16, clip7, fine7):
    """The test that needs the feature.  At x2 with S/D = 2/4 every window starts on a multiple of D, so no group is open at a batch's end
    and nothing is carried, whatever the batch size (``test_groups_that_straddle_windows_are_carried_between_batches`` is the case that
    carries); pipes take the same way."""
    fvr, fine = fine7
    exp, groups = _mixed(fine, clip7, {'mfi': 2}, 2, 4)
    plain = _run(model16, clip7, mfi=2)[3]
    assert exp[:exp.index(b'FRAME\n')] == plain[:plain.index(b'FRAME\n')] and len(exp) == len(plain) and exp != plain
    assert [len(g) for g in groups] == [2] * 8 + [1]                     # the last written frame sits on the timeline's end
    for batch, pipe in ((4, False), (1, False), (2, True)):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, pipe=pipe, mfi=2, shutter=180, shutter_samples=2)
        Y._same(got, exp)
        assert (nw, nf) == (4, 9) and vr.last_shutter == (2, 4) and vr.last_st_frames == sum(map(len, groups)) == 17
        assert vr.last_shutter_carried == 0
        assert vr.last_instants[0] == _instants(7, Fraction(2), 2, 4) == 12 and vr.last_instants[0] < fvr.last_instants[0] == 28
    assert _run(model16, clip7, mfi=2)[0].last_shutter is None


def _carried(n, r, s, d, batch, full=False):
    """The samples a run of an n-frame clip without cuts carries between its batches: the bookkeeping of the stage replayed on the host."""
    from demfi_amd.pipeline import EdgeSpec
    from demfi_amd.y4m_edge import plan_fine
    k0, nw = R.first_window(n, full), R.n_windows(n, full)
    spec, wins = EdgeSpec(y4m=True, full=full, shutter=(s, d)), [S.runner_order((k, k + 1, k + 2, k + 3)) for k in range(k0, k0 + nw)]
    slot, still_open, scene, total = {f: f for f in range(-4, n + 4)}, [], 0, 0
    for b0 in range(0, nw, batch):
        bw = wins[b0:b0 + batch]
        plan = plan_fine(spec, r * d, bw, b0, lambda j: k0 + j, lambda j: j == nw - 1, None, None, [list(w) for w in bw], slot)
        total += len(still_open)
        still_open = [(g, c, s - 1 - len(still_open) + j) for j, (g, c, _) in enumerate(still_open)]
        _, _, still_open, scene = SH.close_groups(still_open, plan[4], scene, plan[5], s, d, s - 1)
    return total


@pytest.mark.parametrize('angle,s', [(360, 4), (270, 3)], ids=['360 of 4', '270 of 3'])
def test_groups_that_straddle_windows_are_carried_between_batches(angle, s, model16, clip7, tmp_path):
    """24 -> 60 (r = 5/2) with D = 4: the fine stream is x10, a window owns ten fine frames and the groups start every four, so the groups
    from 8 and from 28 lie across the windows 0 | 1 and 2 | 3.  With batches of 1 and of 3 windows they lie across batches too: their first
    two samples are carried on the device, in front of the next batch's gather, and the mix reads them there.  One batch of 4 carries nothing;
    all three give the bytes of the host mix of the x10 stream."""
    rate, d = {'fps': Fraction(60)}, 4
    assert SH.check_params(angle, s) == (s, d)
    fine = _run(model16, clip7, **_fine_rate(clip7, rate, d))[3]
    exp, groups = _mixed(fine, clip7, rate, s, d)
    assert groups[2] == list(range(8, 8 + s)) and groups[7] == list(range(28, 28 + s)) and len(groups) == 11
    for batch, carried in ((1, 4), (3, 2), (4, 0)):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, shutter=angle, shutter_samples=s, **rate)
        Y._same(got, exp)
        assert vr.last_shutter_carried == carried == _carried(7, Fraction(5, 2), s, d, batch), batch
        assert nf == 11 and vr.last_st_frames == sum(map(len, groups))
    vr, nw, nf, got = _run_file(model16, clip7, tmp_path, batch=1, shutter=angle, shutter_samples=s, **rate)
    Y._same(got, exp)
    assert vr.last_shutter_carried == 4
    full = _run(model16, clip7, full_length=True, **_fine_rate(clip7, rate, d))[3]         # and on the full-length timeline, S1 hold included
    exp, groups = _mixed(full, clip7, rate, s, d, full=True)
    vr, nw, nf, got = _run(model16, clip7, batch=3, full_length=True, shutter=angle, shutter_samples=s, **rate)
    Y._same(got, exp)
    assert vr.last_shutter_carried == _carried(7, Fraction(5, 2), s, d, 3, True) > 0


def test_a_file_equals_the_mix_of_the_fine_stream(model16, clip7, fine7, tmp_path):
    exp, _ = _mixed(fine7[1], clip7, {'mfi': 2}, 2, 4)
    vr, nw, nf, got = _run_file(model16, clip7, tmp_path, batch=2, mfi=2, shutter='180', shutter_samples=2)
    Y._same(got, exp)
    assert (nw, nf) == (4, 9) and vr.last_shutter == (2, 4)


@pytest.mark.parametrize('n', [1, 2, 7])
def test_full_length(n, model16, clip7, tmp_path):
    data = clip7[:clip7.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p for p in D._split(clip7)[1][:n])
    fine = _run(model16, data, mfi=8, full_length=True)[3]
    exp, groups = _mixed(fine, data, {'mfi': 2}, 2, 4, full=True)
    vr, nw, nf, got = _run(model16, data, batch=2, mfi=2, full_length=True, shutter=180, shutter_samples=2)
    Y._same(got, exp)
    assert nf == 2 * n == len(groups) and vr.last_instants[0] == _instants(n, Fraction(2), 2, 4, True)
    Y._same(_run_file(model16, data, tmp_path, mfi=2, full_length=True, shutter=180, shutter_samples=2)[3], exp)


def test_a_non_integer_ratio(model16, clip7):
    rate = {'fps': Fraction(60)}                                         # 24 -> 60: r = 5/2; 180 degrees with two samples: the fine stream is 240
    fine = _run(model16, clip7, **_fine_rate(clip7, rate, 4))[3]
    exp, groups = _mixed(fine, clip7, rate, 2, 4)
    for batch in (4, 1):
        vr, nw, nf, got = _run(model16, clip7, batch=batch, shutter=180, shutter_samples=2, **rate)
        Y._same(got, exp)
        assert nf == R.n_output_frames(7, Fraction(5, 2)) == len(groups) == 11 and vr.last_fps_out == 60
        assert vr.last_instants[0] == _instants(7, Fraction(5, 2), 2, 4)


def test_high_depth(model16):
    data = Y._clip(7, 64, 96, '420', 10, seed=3)[0]
    fine = _run(model16, data, mfi=8, high_depth=True)[3]
    exp, _ = _mixed(fine, data, {'mfi': 2}, 2, 4)
    vr, nw, nf, got = _run(model16, data, batch=2, mfi=2, high_depth=True, shutter=180, shutter_samples=2)
    Y._same(got, exp)
    assert vr.last_depth == 10 and b' C420p10' in got[:80]


def test_mono_with_an_odd_payload(model16):
    h, w = 65, 97                                                        # P = 6305 samples: rows of the payload buffers at odd addresses
    data = Y._clip(6, h, w, 'mono', 8, seed=5)[0]
    assert y4m.payload_size(h, w, 'mono') % 2 == 1
    fine = _run(model16, data, mfi=8, layouts=True)[3]
    exp, _ = _mixed(fine, data, {'mfi': 2}, 2, 4)
    vr, nw, nf, got = _run(model16, data, batch=1, mfi=2, layouts=True, shutter=180, shutter_samples=2)
    Y._same(got, exp)
    assert vr.last_layout == 'mono'


def test_tiles(model16):
    data = Y._clip(5, 96, 128, '420', 8, seed=4)[0]
    kw = dict(tile=(64, 64), tile_margin=16)
    fine = _run(model16, data, mfi=8, **kw)[3]
    exp, _ = _mixed(fine, data, {'mfi': 2}, 2, 4)
    vr, nw, nf, got = _run(model16, data, batch=1, mfi=2, shutter=180, shutter_samples=2, **kw)
    Y._same(got, exp)
    assert vr.last_plan is not None and vr.last_plan.n_tiles > 1


def _cut_clip():
    def look(i, bgr, peak):                                              # a hard cut before frame 3: another scene's colours
        return bgr if i < 3 else ((peak - bgr) // 3).astype(bgr.dtype)
    return Y._clip(7, 64, 96, '420', 8, seed=1, look=look)[0]


def test_scene_cut_keeps_the_samples_of_the_own_scene(model16):
    """x3 with a 360 degree shutter of four samples (D = 4, the fine stream is x12): window 1 is the cut window, its fine frames 12 .. 17 hold
    frame 2 and 18 .. 23 frame 3, so written frame 4 = fine 16 .. 19 straddles the cut and keeps 16 and 17 only."""
    data = _cut_clip()
    fvr, _, _, fine = _run(model16, data, mfi=12, scene_cut=S.DEFAULT_THRESHOLD)
    assert fvr.last_cuts == [3]
    exp, groups = _mixed(fine, data, {'mfi': 3}, 4, 4, cuts=[3])
    across, plain_groups = _mixed(fine, data, {'mfi': 3}, 4, 4)
    cut_frames = [c for c, (a, b) in enumerate(zip(groups, plain_groups)) if a != b]
    assert cut_frames == [4] and groups[4] == [16, 17] and plain_groups[4] == [16, 17, 18, 19]
    for batch in (4, 1):
        vr, nw, nf, got = _run(model16, data, batch=batch, mfi=3, scene_cut=S.DEFAULT_THRESHOLD, shutter=360)
        Y._same(got, exp)
        assert vr.last_cuts == [3] and vr.last_cut_windows == 1 and nf == len(groups) == 13
    step = 6 + len(D._split(data)[1][0])
    at = got.index(b'FRAME\n') + 4 * step
    assert got[at:at + step] != across[at:at + step]                     # no written payload is the plain average across the cut
    # and the case of the plain streams above, with cuts: no group straddles there, the bytes are still those of the fine stream with cuts
    fine = _run(model16, data, mfi=8, scene_cut=S.DEFAULT_THRESHOLD)[3]
    exp, _ = _mixed(fine, data, {'mfi': 2}, 2, 4, cuts=[3])
    Y._same(_run(model16, data, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD, shutter=180, shutter_samples=2)[3], exp)


def _composed(model, data, **kw):
    """``data`` with the switches ``kw`` at x2 and a 180 degree shutter of two samples == the x8 stream of the same switches mixed on the
    host, under the header of their x2 stream: the stage sits behind whole payloads, whatever made the frames."""
    fine, plain = _run(model, data, mfi=8, **kw)[3], _run(model, data, mfi=2, **kw)[3]
    head, pays = D._split(fine)
    phead, ppays = D._split(plain)
    groups = SH.groups(len(pays), len(ppays), 2, 4)
    out = SH.mix_np(np.stack([np.frombuffer(p, np.uint8) for p in pays]), groups, 1)
    vr, nw, nf, got = _run(model, data, batch=2, mfi=2, shutter=180, shutter_samples=2, **kw)
    Y._same(got, phead + b''.join(b'FRAME\n' + p.tobytes() for p in out))
    assert nf == len(ppays) > 0 and got != plain
    return vr


def test_behind_the_deinterlacer_the_inverse_telecine_and_the_crop(model16):
    from demfi_amd import telecine as TC
    from tests import test_gpu_deint as DI
    fields = DI._interlaced(Y._clip(4, 64, 96, '420', 8, seed=6, fps=b'25:1')[0], 't')
    assert _composed(model16, fields, deinterlace=True).last_fields == 'tff'
    assert _composed(model16, fields, deinterlace=True, deinterlace_mode='adaptive').last_fields == 'tff'
    boxed = Y._clip(6, 80, 96, '420', 8, seed=2)[0]
    assert _composed(model16, boxed, crop=(8, 8, 0, 0)).last_crop == (8, 72, 0, 96)
    assert _composed(model16, boxed, crop=(8, 8, 0, 0), crop_output='cropped').last_crop == (8, 72, 0, 96)
    h, w = 64, 80
    head, pays = D._split(Y._clip(8, h, w, '420', 8, seed=5, fps=b'24000:1001')[0])
    tele = [t.view(np.uint8) for t in TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], h, w, 8, '420', 't', 0)]
    thead = b' '.join(b'F30000:1001' if f.startswith(b'F') else b'It' if f.startswith(b'I') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    vr = _composed(model16, thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele), ivtc=True)
    assert len(vr.last_dropped) == 2 and vr.last_fps_out == Fraction(48000, 1001)


def test_one_sample_of_the_whole_period_is_the_run_without_the_switch(model16, clip7):
    plain = _run(model16, clip7, mfi=2)
    vr, nw, nf, got = _run(model16, clip7, batch=2, mfi=2, shutter=360, shutter_samples=1)
    assert got == plain[3] and vr.last_shutter == (1, 1) and vr.last_instants == plain[0].last_instants


def test_what_does_not_go_together_is_refused_before_anything_runs(model16, clip7, tmp_path):
    with pytest.raises(ValueError, match='more than 64'):
        VideoRunner(model16, 2, mfi=16, shutter=90).run_stream(io.BytesIO(clip7), io.BytesIO())
    vr = VideoRunner(model16, 2, mfi=2, shutter=180)
    (tmp_path / 'in.y4m').write_bytes(clip7)
    with pytest.raises(ValueError, match='shutter with 2 ranks'):
        vr.run_file(str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m'), world=2, rank=1)
    assert not vr._runners and not (tmp_path / 'out.y4m').exists()


def test_cli_through_pipes(model16, clip7):
    """The command line is what this test is about: the two switches reach the runner, the stream owns stdout, the JSON line gains ``shutter``."""
    exp = _run(model16, clip7, mfi=2, shutter=180, shutter_samples=2)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '2', '--matrix',
                        'bt601', '--shutter', '180', '--shutter-samples', '2'],
                       input=clip7, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['shutter'] == {'angle': '180', 'samples': 2, 'fine_per_written': 4}
    assert (last['windows'], last['frames_written'], last['instants_run'], last['fps_out']) == (4, 9, 12, '48')
