"""The temporal denoiser in front of the network (``--denoise``) on a real MI355X: ``demfi_payload_denoise`` (csrc/denoise.hip) equal to
``denoise.denoise_payload_np`` byte for byte inside guard bytes, and ``VideoRunner(denoise=...)`` byte-identical to an expectation that
never runs the new kernel or the deferred launches: the same runner WITHOUT ``denoise`` on the stream denoised on the host with
``denoise_stream_np``.  The clip is ``noisy_clip`` of tests/test_denoise.py, which checks there that it exercises the filter; model and
helpers are those of the neighbouring files."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fractions import Fraction                                                       # noqa: E402

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import bitdepth as BD                                                 # noqa: E402
from demfi_amd import denoise as DN                                                  # noqa: E402
from demfi_amd import pipeline as P                                                  # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_telecine as TC                                            # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402
from tests.test_denoise import exercised, noisy_clip                                 # noqa: E402

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD = 0xC7


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _cands(p, depth, radius, seed, far):
    """2 R + 1 payloads of p samples: a seeded centre and neighbours near it (noise of +-A_d: both thresholds bite at some samples and
    pass at others) or unrelated to it (``far``); some centre samples at 0 and at the peak."""
    g = np.random.RandomState(seed)
    peak, (ad, _) = (1 << depth) - 1, DN.thresholds(depth, 5, 10)
    c = g.randint(0, peak + 1, p)
    c[::7] = peak
    c[3::11] = 0
    out = [np.clip(c + g.randint(-ad, ad + 1, p), 0, peak) if not far else g.randint(0, peak + 1, p) for _ in range(2 * radius + 1)]
    out[radius] = c
    return [a.astype(_dtype(depth)) for a in out]


def _launch(srcs, rows, depth, a=5, b=10, lead=0, gap=0):
    """``srcs``: payloads (1-D sample arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes; ``rows``: per frame
    the 2 R + 1 source numbers (None: absent) -> the denoised payloads after ONE demfi_payload_denoise launch into a second buffer laid out
    the same way.  Every byte before, between and after the written payloads is intact and the sources are untouched."""
    es, pb, n, taps = srcs[0].itemsize, srcs[0].nbytes, len(rows), len(rows[0])
    stride = pb + gap
    src = np.full(lead + len(srcs) * stride + 64, GUARD, np.uint8)
    for i, p in enumerate(srcs):
        src[lead + i * stride:lead + i * stride + pb] = p.view(np.uint8)
    dst = np.full(lead + n * stride + 64, GUARD, np.uint8)
    offs = np.array([[-1 if s is None else lead + s * stride for s in row] + [lead + i * stride] for i, row in enumerate(rows)], np.int64).reshape(-1)
    d_src, d_dst, d_offs = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), torch.from_numpy(offs).to(DEV)
    ad, bd = DN.thresholds(depth, a, b)
    L.check(L.load().demfi_payload_denoise(d_src.data_ptr(), d_src.numel(), offs.ctypes.data, d_offs.data_ptr(), n, taps, srcs[0].size, es, ad, bd,
                                           d_dst.data_ptr(), d_dst.numel(), torch.cuda.current_stream().cuda_stream), 'payload_denoise')
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src), 'a source was written'
    assert (out[:lead] == GUARD).all() and (out[lead + (n - 1) * stride + pb:] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(srcs[0].dtype) for i in range(n)]


def _check_patterns(p, depth, radius, seed, lead, gap):
    """Every pattern of absent neighbours -- 0 .. R present frames on each side: the start of a stream, its end, a one-frame stream --
    with near and unrelated neighbours alternating, in ONE launch; frame i owns sources (2 R + 1) i .. (2 R + 1) i + 2 R."""
    taps = 2 * radius + 1
    cases = [(nb, na, (nb + na + k) & 1) for k, (nb, na) in enumerate((x, y) for x in range(radius + 1) for y in range(radius + 1))]
    cases += [(radius, radius, 1 - cases[-1][2])]                         # all present: near and far
    srcs, rows = [], []
    for i, (nb, na, far) in enumerate(cases):
        srcs += _cands(p, depth, radius, seed + 13 * i, far)
        rows.append([taps * i + j if radius - nb <= j <= radius + na else None for j in range(taps)])
    got = _launch(srcs, rows, depth, lead=lead, gap=gap)
    changed = 0
    for i, (row, (nb, na, far)) in enumerate(zip(rows, cases)):
        exp = DN.denoise_payload_np([None if s is None else srcs[s] for s in row], depth, 5, 10)
        bad = np.flatnonzero(got[i] != exp)
        assert bad.size == 0, ('p=%d before=%d after=%d far=%d: %d of %d samples differ' % (p, nb, na, far, bad.size, exp.size), bad[:10])
        changed += int((exp != srcs[row[radius]]).sum())
    return changed


SIZES = [(2, 2), (7, 17), (37, 61), (70, 9)]


@pytest.mark.parametrize('depth', [8, 10, 16], ids=['bytes', '10-bit', '16-bit'])
@pytest.mark.parametrize('radius', [1, 2, 3])
def test_kernel_equals_the_numpy_definition(radius, depth):
    """Sample counts around the 16-byte word and the payloads of four frame sizes in every layout; each at aligned offsets (the vector
    path and its tail) and at odd leads and gaps for bytes, even but unaligned ones for 16-bit samples (sample by sample)."""
    counts = [1, 15, 16, 17, 31, 33] + [y4m.payload_size(h, w, layout) for h, w in SIZES for layout in y4m.LAYOUTS]
    changed = 0
    for k, p in enumerate(counts):
        changed += _check_patterns(p, depth, radius, 100 * radius + depth + k, 0, (-p * (1 if depth == 8 else 2)) % 16)      # every payload on a 16-byte boundary
        changed += _check_patterns(p, depth, radius, 100 * radius + depth + k, *((3, 5) if depth == 8 else (6, 10)))
    assert changed > 0                                                    # the data exercises the filter


@pytest.mark.parametrize('depth', [8, 10], ids=['bytes', '10-bit'])
def test_a_stream_of_64_frames_in_one_launch(depth):
    """The frames of a stream as the edge holds them: frame f reads the slots of f-2 .. f+2, which other frames of the launch read too."""
    n, radius, p = 64, 2, y4m.payload_size(37, 61, '420')
    g = np.random.RandomState(depth)
    peak, sh = (1 << depth) - 1, depth - 8
    still = g.randint(0, peak + 1, p)
    pays = [np.clip(still + (g.randint(-3, 4, p) << sh), 0, peak).astype(_dtype(depth)) for _ in range(n)]
    rows = [DN.neighbours(f, radius, 1, lambda g_: g_ < n) for f in range(n)]
    got = _launch(pays, rows, depth, lead=3 if depth == 8 else 6, gap=5 if depth == 8 else 10)
    for f, exp in enumerate(DN.denoise_stream_np(pays, depth, 5, 10, radius)):
        assert np.array_equal(got[f], exp), f
    got = _launch(pays, rows, depth, lead=16, gap=(-pays[0].nbytes) % 16)
    for f, exp in enumerate(DN.denoise_stream_np(pays, depth, 5, 10, radius)):
        assert np.array_equal(got[f], exp), f


@pytest.mark.parametrize('depth,centre,jitter', [(8, 100, 0), (8, 3, 0), (8, 252, 0), (16, 65535 - 700, 0), (16, 65535 - 700, 1), (16, 600, 0), (16, 600, 1)],
                         ids=['bytes', 'bytes-near-0', 'bytes-near-255', '16-bit-near-the-peak', '16-bit-near-the-peak-A+1', '16-bit-near-0', '16-bit-near-0-A+1'])
def test_every_combination_of_differences_around_the_thresholds(depth, centre, jitter):
    """R = 2, the centre fixed, the four neighbours taking every difference k << (depth - 8), k in -(A+2) .. A+2, independently: 15^4
    samples laid out as one payload.  ``jitter`` moves every difference one step further from the centre, so that A_d + 1 and B_d + 1 are
    met as well as A_d and B_d.  Neighbours that would leave the sample range are clipped into it; the definition sees the same values."""
    a, b, sh, peak = 5, 10, depth - 8, (1 << depth) - 1
    ks = np.arange(-(a + 2), a + 3)
    grid = np.stack(np.meshgrid(ks, ks, ks, ks, indexing='ij')).reshape(4, -1)            # f-2, f-1, f+1, f+2
    assert grid.shape == (4, 15 ** 4)
    diffs = (grid << sh) + jitter * np.sign(grid)
    c = np.full(grid.shape[1], centre)
    srcs = [np.clip(c + diffs[0], 0, peak), np.clip(c + diffs[1], 0, peak), c, np.clip(c + diffs[2], 0, peak), np.clip(c + diffs[3], 0, peak)]
    srcs = [s.astype(_dtype(depth)) for s in srcs]
    got = _launch(srcs, [[0, 1, 2, 3, 4]], depth, a, b)[0]
    exp = DN.denoise_payload_np(srcs, depth, a, b)
    assert np.array_equal(got, exp)
    ad, bd = DN.thresholds(depth, a, b)
    for first, second in ((1, 0), (3, 4)):                                # on each side: stopped at once, averaged once, averaged twice
        d1, d2 = np.abs(srcs[first].astype(np.int64) - centre), np.abs(srcs[second].astype(np.int64) - centre)
        assert (d1 > ad).any() and ((d1 <= ad) & (d1 + d2 > bd)).any() and ((d1 <= ad) & (d2 <= ad) & (d1 + d2 <= bd)).any()
        if depth == 8 or not jitter:
            assert (d1 == ad).any() and (d1 + d2 == bd).any()
        else:
            assert (d1 == ad + 1).any() and (d1 + d2 == bd + 2).any()
    assert (exp != centre).any() and (exp == centre).any()


def test_full_size_point():
    h, w, radius = 1088, 1920, 2
    srcs = _cands(y4m.payload_size(h, w, '420'), 8, radius, 11, False)
    got = _launch(srcs, [[0, 1, 2, 3, 4]], 8)[0]
    exp = DN.denoise_payload_np(srcs, 8, 5, 10)
    assert np.array_equal(got, exp) and (exp != srcs[2]).mean() > 0.25


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    src = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = torch.full((256,), 0x5A, dtype=torch.uint8, device=DEV)
    fn = lib.demfi_payload_denoise
    good = np.array([0, 24, 48, 0, -1, 96, 120, 24], np.int64)             # 24-byte payloads, R = 1; frame 1 is the first of a stream
    good_dev = torch.from_numpy(good).to(DEV)
    ok = [src.data_ptr(), 256, good.ctypes.data, good_dev.data_ptr(), 2, 3, 24, 1, 5, 10, dst.data_ptr(), 256, st]

    def bad(i, v, offs=None, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        if offs is not None:
            o = np.array(offs, np.int64)
            a[2] = o.ctypes.data
        return fn(*a) == ERR_ARG
    assert bad(0, None) and bad(2, None) and bad(3, None) and bad(10, None)                                # NULL pointers
    assert bad(4, -1) and bad(4, 65)                                      # n outside 0 .. 64
    assert bad(5, 1) and bad(5, 2) and bad(5, 4) and bad(5, 9)            # taps not 3, 5 or 7
    assert bad(7, 0) and bad(7, 3) and bad(7, 4)                          # sample size not 1 or 2
    assert bad(6, 0) and bad(6, -5)                                       # no samples
    assert bad(8, -1) and bad(8, 11) and bad(9, 256) and bad(9, 65536, _7=2, _6=12)                       # thresholds out of range
    assert bad(0, src.data_ptr() + 1, _7=2, _6=12) and bad(10, dst.data_ptr() + 1, _7=2, _6=12)             # 16-bit samples at an odd address
    assert bad(4, 2, offs=[0, 25, 48, 0, -1, 96, 120, 24], _7=2, _6=12)   # ... at an odd source offset
    assert bad(4, 2, offs=[0, 24, 48, 1, -1, 96, 120, 24], _7=2, _6=12)   # ... at an odd destination offset
    assert bad(4, 2, offs=[0, 24, -2, 0, -1, 96, 120, 24])                # an offset below -1
    assert bad(4, 2, offs=[0, -1, 48, 0, -1, 96, 120, 24])                # an absent centre
    assert bad(4, 2, offs=[0, 24, 233, 0, -1, 96, 120, 24])               # a source payload that leaves its buffer
    assert bad(4, 2, offs=[0, 24, 48, 233, -1, 96, 120, 24])              # a destination payload that leaves its buffer
    assert bad(4, 2, offs=[0, 24, 48, -1, -1, 96, 120, 24])               # no destination
    assert bad(1, 143) and bad(11, 47)                                    # the buffers end inside payloads 120 .. 143 and 24 .. 47
    assert bad(4, 2, offs=[0, 24, 48, 24, -1, 96, 120, 24])               # two frames with one destination
    assert bad(4, 2, offs=[0, 24, 48, 30, -1, 96, 120, 24])               # ... or overlapping ones
    assert bad(10, src.data_ptr() + 128, _11=128) and bad(10, src.data_ptr())                              # destination inside the source
    assert b'demfi_payload_denoise' in lib.demfi_last_error()
    torch.cuda.synchronize()
    assert bool((src == 0xA5).all()) and bool((dst == 0x5A).all())
    a = list(ok)
    a[4] = 0
    assert fn(*a) == 0                                                    # n = 0: a no-op success
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    assert fn(*ok) == 0                                                   # flat payloads stay flat, and only the two payloads are written
    torch.cuda.synchronize()
    assert bool((src == 0xA5).all()) and bool((dst[:48] == 0xA5).all()) and bool((dst[48:] == 0x5A).all())
    assert L.ABI_VERSION == 8                                             # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _denoised(data, a=5, b=10, radius=2, step=1):
    """The stream ``data`` denoised on the host, payload by payload, header untouched."""
    hdr, pays = D._parse(data)
    smp = [np.frombuffer(p, _dtype(hdr.depth)) for p in pays]
    return data[:data.index(b'FRAME\n')] + b''.join(b'FRAME\n' + o.tobytes() for o in DN.denoise_stream_np(smp, hdr.depth, a, b, radius, step))


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')

    def seekable(self):
        return False


def _run(model, data, batch=4, pipe=False, **kw):
    vr = VideoRunner(model, 1, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(_Pipe(data) if pipe else io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


ON = dict(denoise=True)


def _check(model, data, batch=4, pipe=False, host=None, on=ON, **kw):
    """``VideoRunner(..., denoise=..., **kw)`` on ``data`` == the same runner WITHOUT ``denoise`` on the stream denoised on the host
    (``host``: that stream and the switches it runs with, where they differ), header, counts, cuts and instants included."""
    prog, hkw = (_denoised(data), kw) if host is None else host
    ve, nwe, nfe, exp = _run(model, prog, batch, **hkw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **on, **kw)
    assert (nw, nf) == (nwe, nfe) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_cut_windows) == (ve.last_instants, ve.last_st_frames, ve.last_cuts, ve.last_cut_windows)
    assert vr.last_denoised > 0 and ve.last_denoised == 0
    return vr, got


@pytest.fixture(scope='module')
def clip8():
    data, pays, left = noisy_clip(7, 64, 96, '420', 8, seed=3)
    changed, alone = exercised(pays, left, 8)
    assert changed > 0.25 and alone > 0.5                                 # the filter works on one half and keeps off the other
    return data


def test_x2_uploads_every_frame_once_and_the_switch_matters(model16, clip8, monkeypatch):
    n = 7
    ups = []
    up = P.Y4mEdge.upload
    monkeypatch.setattr(P.Y4mEdge, 'upload', lambda self, sl, idx, f: (ups.append(idx), up(self, sl, idx, f))[1])
    vr, got = _check(model16, clip8, mfi=2)
    assert sorted(ups[n:]) == list(range(n)) and vr.last_denoised == n      # after the expectation's n: every frame once
    assert vr.denoise == (5, 10, 2) and (len(D._parse(got)[1]) == R.n_output_frames(n, 2))
    plain = _run(model16, clip8, mfi=2)[3]
    assert len(plain) == len(got) and plain != got
    for radius in (1, 3):
        _check(model16, clip8, mfi=2, on=dict(denoise=(4, 9), denoise_radius=radius), host=(_denoised(clip8, 4, 9, radius), dict(mfi=2)))


def test_fps_12_5(model16):
    data = noisy_clip(6, 48, 80, '420', 8, seed=4, fps=b'25:1')[0]
    vr, got = _check(model16, data, fps=Fraction(60))
    assert vr.last_fps_out == 60


def test_scene_cut_is_found_at_the_same_frame(model16):
    h, w, n, cut = 64, 96, 8, 4
    head, a, left = noisy_clip(n, h, w, '420', 8, seed=1)
    b = noisy_clip(n, h, w, '420', 8, seed=2)[1]
    pays = [a[f] if f < cut else 255 - b[f] for f in range(n)]
    data = head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays)
    vr, got = _check(model16, data, batch=2, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [cut] and vr.last_cut_windows >= 1


def test_full_length_and_batch_sizes(model16, clip8):
    vr, exp = _check(model16, clip8, batch=2, mfi=2, full_length=True)
    assert len(D._parse(exp)[1]) == 7 * 2
    for batch in (1, 4):
        assert _run(model16, clip8, batch, mfi=2, full_length=True, **ON)[3] == exp
    exp = _check(model16, clip8, batch=1, mfi=2)[1]
    assert _run(model16, clip8, 4, mfi=2, **ON)[3] == exp


def test_a_pipe(model16, clip8):
    vr, got = _check(model16, clip8, batch=2, pipe=True, mfi=2)
    assert vr.last_decode_peak <= 2 + 5 + 2 * 2


def test_files_one_rank_and_two_ranks_of_two(model16, tmp_path):
    """Output frame f depends on input frames f-2 .. f+2 of the whole input, not on batches or blocks: ``run_file`` on one rank and
    ranks 0 and 1 of two, whose blocks meet mid-stream and read two frames of each other's, give the bytes of the stream run."""
    n = 10
    data = noisy_clip(n, 48, 80, '420', 8, seed=8)[0]
    vr, exp = _check(model16, data, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (n - 3, R.n_output_frames(n, 2)) and one.last_denoised == n
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot = [0, 0]
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        assert 0 < v.last_denoised < n
    assert tot == [nw, nf]
    Y._same(dst.read_bytes(), exp)
    kw = dict(mfi=2, full_length=True, scene_cut=S.DEFAULT_THRESHOLD)     # where a block also denoises the frame before its first window
    exp = _run(model16, _denoised(data), batch=2, **kw)[3]
    dst.unlink()
    for rank in range(2):
        VideoRunner(model16, 1, batch=2, matrix='bt601', **ON, **kw).run_file(str(src), str(dst), world=2, rank=rank)
    Y._same(dst.read_bytes(), exp)


def test_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    data = noisy_clip(6, h, w, '420', 8, seed=4)[0]
    vr, got = _check(model16, data, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def test_422p10_with_high_depth_and_any_layout(model16):
    data = noisy_clip(6, 48, 80, '422', 10, seed=5)[0]
    vr, got = _check(model16, data, mfi=2, high_depth=True, layouts=True)
    assert (vr.last_depth, vr.last_layout) == (10, '422') and b' C422p10' in got[:80]


def test_tiled_420p10_with_tile_high_depth(model16):
    data = noisy_clip(6, 96, 160, '420', 10, seed=7)[0]
    vr, got = _check(model16, data, batch=2, mfi=2, tile=(64, 96), tile_margin=16, high_depth=True, tile_high_depth=True)
    assert vr.last_depth == 10 and vr.last_plan.n_tiles == 4


def test_work_depth_10_on_an_8_bit_input_takes_the_thresholds_at_10_bits(model16, clip8):
    """Host promote, then host denoise at 10 bits (thresholds 20 and 40), then the ``high_depth`` run: the pattern of tests/test_gpu_bitdepth.py."""
    host = _denoised(BD.promote_stream_np(clip8, 10))
    vr, got = _check(model16, clip8, batch=2, mfi=2, work_depth=10, out_depth=10, host=(host, dict(mfi=2, high_depth=True)))
    assert vr.last_depths == (8, 10, 10, None) and vr.last_depth_promoted == vr.last_denoised == 7 and b' C420p10' in got[:80]


@pytest.mark.parametrize('order', ['t', 'b'])
def test_behind_the_bob_the_neighbours_are_the_fields_of_the_same_parity(order, model16):
    """``D._bobbed``, then ``denoise_stream_np(step=2)``, then the progressive run."""
    n = 6
    data = D._interlaced(noisy_clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], order)
    host = _denoised(D._bobbed(data), step=2)
    vr, got = _check(model16, data, mfi=2, deinterlace=True, host=(host, dict(mfi=2)))
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_denoised == 2 * n
    assert got != _run(model16, data, mfi=2, deinterlace=True)[3]
    assert got != _run(model16, _denoised(D._bobbed(data), step=1), mfi=2)[3]      # the step matters


def test_behind_the_inverse_telecine(model16):
    film, tele, st = TC._clips()
    vr, got = _check(model16, tele, mfi=2, ivtc=True, host=(_denoised(film), dict(mfi=2)))
    assert vr.last_matches == st.matches and vr.last_dropped == st.dropped and vr.last_denoised == 12


def test_behind_an_explicit_crop(model16):
    """The crop is a host stage in front and the filter works sample by sample: cropping the denoised stream is denoising the cropped one."""
    data = noisy_clip(6, 80, 112, '420', 8, seed=6)[0]
    vr, got = _check(model16, data, mfi=2, crop=(8, 8, 16, 32))
    assert vr.last_crop is not None and got.startswith(b'YUV4MPEG2 W112 H80 ')


def test_in_front_of_the_shutter_the_scaler_and_the_weave(model16, clip8):
    vr, got = _check(model16, clip8, batch=2, mfi=4, shutter=180, shutter_samples=2, scale=(80, 48), interlace='tff')
    assert b' W80 H48 ' in got[:40] and b' It ' in got[:80] and vr.last_shutter == (2, 4)


def test_a_threshold_of_zero_gives_the_bytes_of_a_run_without_the_switch(model16, clip8):
    plain = _run(model16, clip8, mfi=2)[3]
    vr, nw, nf, got = _run(model16, clip8, mfi=2, denoise=(0, 0))
    assert got == plain and vr.last_denoised == 7


def test_cli_through_pipes(model16, clip8):
    """The command line is what this test is about: the two switches reach the runner, the stream owns stdout, the JSON line says what
    the stage did."""
    exp = _run(model16, _denoised(clip8, 4, 9, 1), mfi=2)[3]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run(['timeout', '-k', '10', '600', sys.executable, '-m', 'demfi_amd.video', '-', '-', '--mfi', '2', '--n-tst', '1', '--matrix',
                        'bt601', '--denoise', '4:9', '--denoise-radius', '1'],
                       input=clip8, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, env=env, timeout=660)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-2000:]
    assert p.stdout == exp
    last = json.loads(p.stderr.decode().strip().splitlines()[-1])
    assert last['denoise'] == {'a': 4, 'b': 9, 'radius': 1, 'frames': 7} and (last['windows'], last['frames_written']) == (4, 9)


def test_refusals_come_before_anything_is_allocated(model16):
    free0 = torch.cuda.mem_get_info()[0]
    for kw, msg in ((dict(dedup=True), '--dedup'), (dict(deinterlace=True, deinterlace_mode='adaptive'), '--deinterlace-mode bob'),
                    (dict(denoise_radius=4), 'radius'), (dict(denoise=(9, 3)), 'A <= B')):
        with pytest.raises(ValueError, match=msg):
            VideoRunner(model16, 1, mfi=2, matrix='bt601', **dict(ON, **kw))
    with pytest.raises(ValueError, match='give --denoise'):
        VideoRunner(model16, 1, mfi=2, matrix='bt601', denoise_radius=2)
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
