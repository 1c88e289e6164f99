"""Repeated frames (``--dedup``) on a real MI355X: ``demfi_luma_block_counts`` (csrc/dedup.hip) equal to ``cadence.block_counts_np``
integer for integer, and ``VideoRunner(dedup=...)`` byte-identical to expectations that do not run the new code: the undoubled
clip at twice the ratio, the run without ``dedup`` when nothing repeats, and compositions on the host from the plans of
``demfi_amd.cadence`` and per-window forwards, in the way tests/test_gpu_y4m_layouts.py composes its streams (whose clip and
conversion helpers are used here)."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import cadence as K                                                   # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.clip import ClipRunner                                                # noqa: E402
from demfi_amd.harness import module_window_ts_u8                                    # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
GUARD = 0x5A5A5A5A


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _pair(h, w, sb, seed, top=30):
    """Two luma planes (uint8 / uint16 samples at 10 bits) whose difference grows from nothing on the left to ``top`` (far above
    ``hi``) on the right, so that cold, warm and hot blocks all occur, partial ones included."""
    rng = np.random.default_rng(seed)
    s = 1 if sb == 1 else 4
    a = rng.integers(40 * s, 180 * s, (h, w), dtype=np.int64)
    amp = (np.arange(w, dtype=np.int64) * top * s) // max(w - 1, 1) + (np.arange(h, dtype=np.int64)[:, None] % 3)
    b = a + rng.integers(-1, 2, (h, w)) * amp
    dt = np.uint8 if sb == 1 else np.uint16
    return a.astype(dt).reshape(-1), np.clip(b, 0, 255 * s + (3 if sb == 2 else 0)).astype(dt).reshape(-1)


def _counts_gpu(buf, a_offs, b_offs, h, w, sb, hi_s, lo_s):
    """buf: the bytes of a device buffer; pairs at byte offsets -> [(hot, warm)], and the guards around the counts hold."""
    lib, n = L.load(), len(a_offs)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    offs = torch.tensor(list(a_offs) + list(b_offs), dtype=torch.int64, device=DEV)
    cnt = torch.from_numpy(np.full(2 * n + 2, GUARD, np.uint32).view(np.int32)).to(DEV)
    L.check(lib.demfi_luma_block_counts(dev.data_ptr(), offs.data_ptr(), offs[n:].data_ptr(), n, h, w, sb, hi_s, lo_s,
                                        cnt[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), 'luma_block_counts')
    torch.cuda.synchronize()
    out = cnt.cpu().numpy().view(np.uint32)
    assert out[0] == GUARD and out[-1] == GUARD
    assert bytes(dev.cpu().numpy()) == bytes(np.ascontiguousarray(buf))
    return [(int(out[1 + 2 * i]), int(out[2 + 2 * i])) for i in range(n)]


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
@pytest.mark.parametrize('h,w', [(2, 2), (2, 7), (7, 5), (9, 70), (33, 47), (70, 9), (64, 128), (1088, 1920)])
def test_counts_equal_the_numpy_definition(h, w, sb):
    a, b = _pair(h, w, sb, h * 31 + w)
    depth = 8 if sb == 1 else 10
    buf = np.concatenate([a, b]).view(np.uint8)
    for hi, lo in ((K.DEFAULT_HI, K.DEFAULT_LO), (200, 64), (0, 0)):
        s = 1 << (depth - 8)
        exp = K.block_counts_np(a, b, h, w, depth, hi, lo)
        got = _counts_gpu(buf, [0], [a.nbytes], h, w, sb, hi * s, lo * s)
        print('%dx%d, %d bytes per sample, hi %d lo %d: kernel %s numpy %s of %d blocks' % (h, w, sb, hi, lo, got[0], exp, K.n_blocks(h, w)))
        assert got == [exp]
    if w >= 47:
        hot, warm = K.block_counts_np(a, b, h, w, depth)
        assert 0 < hot < warm < K.n_blocks(h, w)        # the pair exercises all three kinds of block
    assert _counts_gpu(buf, [0], [0], h, w, sb, 0, 0) == [(0, 0)]


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
def test_a_batch_of_pairs_at_unaligned_offsets(sb):
    h, w = 37, 61                                        # rows start at every alignment
    depth = 8 if sb == 1 else 10
    planes = [p for seed, top in enumerate((30, 12, 50)) for p in _pair(h, w, sb, 50 + seed, top)]
    gaps = [3, 5, 1, 7, 9, 11] if sb == 1 else [2, 6, 10, 14, 18, 22]          # byte offsets: odd for bytes, even and unaligned for samples
    chunks, offs, pos = [], [], 0
    for p, g in zip(planes, gaps):
        chunks.append(np.full(g, 0xEE, np.uint8))
        pos += g
        offs.append(pos)
        chunks.append(p.view(np.uint8))
        pos += p.nbytes
    buf = np.concatenate(chunks + [np.full(64, 0xEE, np.uint8)])
    pairs = [(0, 1), (2, 3), (4, 5), (0, 3), (5, 5), (4, 1), (2, 0)]
    s = 1 << (depth - 8)
    got = _counts_gpu(buf, [offs[i] for i, _ in pairs], [offs[j] for _, j in pairs], h, w, sb, K.DEFAULT_HI * s, K.DEFAULT_LO * s)
    exp = [K.block_counts_np(planes[i], planes[j], h, w, depth) for i, j in pairs]
    print(got, exp)
    assert got == exp and exp[4] == (0, 0) and len(set(exp)) >= 4


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(2, dtype=torch.int64, device=DEV)
    cnt = torch.full((2,), 0x5A5A, dtype=torch.int32, device=DEV)
    ok = (buf.data_ptr(), offs.data_ptr(), offs.data_ptr(), 1, 2, 2, 1, 768, 320, cnt.data_ptr(), st)
    fn = lib.demfi_luma_block_counts

    def bad(i, v):
        a = list(ok)
        a[i] = v
        return fn(*a) == ERR_ARG
    assert bad(0, None) and bad(1, None) and bad(2, None) and bad(9, None) and bad(3, -1)
    assert bad(4, 1) and bad(5, 1) and bad(4, 16385) and bad(5, 16385) and bad(6, 0) and bad(6, 3) and bad(6, 4)
    assert bad(7, -1) and bad(8, -1) and bad(7, (1 << 40) + 1) and bad(8, (1 << 40) + 1)
    a = list(ok)
    a[0], a[6] = buf.data_ptr() + 1, 2                   # 16-bit samples at an odd address
    assert fn(*a) == ERR_ARG
    assert b'demfi_luma_block_counts' in lib.demfi_last_error()
    a = list(ok)
    a[3] = 0                                             # no pair: nothing to do, nothing written
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((cnt == 0x5A5A).all()) and bool((buf == 0xA5).all())
    assert fn(*ok) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0]
    assert L.ABI_VERSION == 8                            # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _split(data):
    """(header line, [payload bytes])."""
    at = data.index(b'FRAME\n')
    hdr = y4m.Reader(io.BytesIO(data), **Y.ANY).header
    body = data[at:]
    step = 6 + hdr.payload
    assert len(body) % step == 0
    return data[:at], [body[i + 6:i + step] for i in range(0, len(body), step)]


def _join(head, pays, fps=None):
    if fps is not None:
        head = b' '.join(b'F' + fps if f.startswith(b'F') else f for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    return head + b''.join(b'FRAME\n' + p for p in pays)


def _repeat(data, times, fps=None):
    """The clip with frame i shown times[i] times in a row."""
    head, pays = _split(data)
    return _join(head, [p for p, c in zip(pays, times) for _ in range(c)], fps)


def _kept(data, **kw):
    """The host detector over a whole stream: (kept input indices, header, payloads as numpy bytes)."""
    hdr, pays = Y._read(data)
    return K.kept_of(pays, hdr.h, hdr.w, hdr.depth, **kw), hdr, pays


def _expected(model, data, n_tst, r, matrix, kept, full_length=False, cuts=None, plan=None):
    """Composed on the host: numpy payload -> BGR of the KEPT frames; every run of every window of ``cadence.window_runs`` on its own
    instants through the BGR window path (as tests/test_gpu_y4m_layouts.py ``_expected``: one module forward per instant, per tile
    and stitched with ``plan``; ONE ``run_windows_u16`` above 8 bits); each output picked by the window's outputs; numpy BGR ->
    payload.  ``cuts``: kept indices that start a scene.  Returns (bytes, cut windows, runs)."""
    hdr, pays = Y._read(data)
    d, lay, n = hdr.depth, hdr.layout, len(pays)
    frames = [Y._to_bgr_np(pays[i] if d == 8 else y4m.as_samples16(pays[i]), hdr.h, hdr.w, d, lay, matrix, hdr.full_range) if lay != '420'
              else (y4m.yuv420_to_bgr_np(pays[i], hdr.h, hdr.w, matrix, hdr.full_range, hdr.chroma) if d == 8 else
                    y4m.yuv420_to_bgr16_np(y4m.as_samples16(pays[i]), hdr.h, hdr.w, d, matrix, hdr.full_range, hdr.chroma)) for i in kept]
    is_cut = (lambda j: j in cuts) if cuts else None
    runs, outs, n_cut = [], [], 0
    for k in K.windows(kept, n, full_length, r):
        wr, wo = K.window_runs(k, r, kept, n, is_cut, full_length)
        n_cut += K.is_cut_window(k, is_cut)
        outs += [(len(runs) + run, kind, j) for _, run, kind, j in wo]
        runs += wr
    if d > 8:
        dev = [Y._dev(f, d) for f in frames]
        rn = ClipRunner(model, hdr.h, hdr.w, n_tst, 8, retime=r).runner
        st, s01 = rn.run_windows_u16([[dev[x] for x in S.runner_order(tup)] for tup, _ in runs], d, ts=[ts for _, ts in runs])
        torch.cuda.synchronize()
        st, s01 = Y._host(st, d), Y._host(s01, d)
        res = [(st[i], s01[i]) for i in range(len(runs))]
    elif plan is None:
        tf = [torch.from_numpy(f) for f in frames]
        res = [[a.cpu().numpy() for a in module_window_ts_u8(model, [tf[x] for x in S.runner_order(tup)], n_tst, ts)] for tup, ts in runs]
    else:
        tiles = [torch.from_numpy(T.crop_np(f, plan)) for f in frames]
        res = []
        for tup, ts in runs:
            per = [[a.cpu().numpy() for a in module_window_ts_u8(model, [tiles[x][j] for x in S.runner_order(tup)], n_tst, ts)]
                   for j in range(plan.n_tiles)]
            res.append(tuple(np.stack([T.stitch_np(np.stack([per[j][part][i] for j in range(plan.n_tiles)]), plan, hdr.h, hdr.w)
                                       for i in range(per[0][part].shape[0])]) for part in range(2)))
    out = [R.output_header(hdr, hdr.fps * r).encode()]
    for run, kind, j in outs:
        st, s01 = res[run]
        f = s01[0] if kind == R.S0 else s01[1] if kind == R.S1 else st[j]
        if lay != '420':
            p = Y._to_yuv_np(np.ascontiguousarray(f), d, lay, matrix, hdr.full_range)
        elif d == 8:
            p = y4m.bgr_to_yuv420_np(np.ascontiguousarray(f), matrix, hdr.full_range)
        else:
            p = y4m.bgr16_to_yuv420_np(np.ascontiguousarray(f), d, matrix, hdr.full_range)
        out += [b'FRAME\n', p.tobytes()]
    assert len(outs) == R.n_output_frames(n, r, full_length)
    return b''.join(out), n_cut, runs


def _run(model, data, n_tst, batch=4, **kw):
    vr = VideoRunner(model, n_tst, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def test_doubled_frames_give_the_undoubled_clip_at_twice_the_ratio(model16):
    """The test that needs the feature: A A B B C C ... with dedup at x M is, byte for byte, A B C ... at x 2M."""
    n, M = 6, 2
    plain, _, _ = Y._clip(n, 48, 80, '420', 8, seed=5, fps=b'12:1')
    doubled = _repeat(plain, [2] * n, fps=b'24:1')
    kept, _, _ = _kept(doubled)
    assert kept == list(range(0, 2 * n, 2))
    exp = _run(model16, plain, 2, mfi=2 * M, full_length=True)[3]
    vr, nw, nf, got = _run(model16, doubled, 2, mfi=M, full_length=True, dedup=True)
    assert (nw, nf) == (n - 1, 2 * n * M) and vr.last_dups == list(range(1, 2 * n, 2))
    Y._same(got, exp)
    vr0, nw0, nf0, stutter = _run(model16, doubled, 2, mfi=M, full_length=True)
    assert nf0 == nf and len(stutter) == len(got) and stutter != got and vr0.last_dups == []
    # and a small batch, which splits the kept sequence differently
    Y._same(_run(model16, doubled, 2, batch=1, mfi=M, full_length=True, dedup=True)[3], exp)


@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
def test_a_clip_without_repeats_is_unchanged(full, model16):
    data, _, _ = Y._clip(7, 48, 80, '420', 8, seed=3)
    assert _kept(data)[0] == list(range(7))
    vr0, nw0, nf0, exp = _run(model16, data, 2, fps=Fraction(60), full_length=full)
    vr, nw, nf, got = _run(model16, data, 2, fps=Fraction(60), full_length=full, dedup=True)
    assert (nw, nf) == (nw0, nf0) and vr.last_dups == [] and vr.last_st_frames == vr0.last_st_frames
    assert vr.last_instants == vr0.last_instants
    Y._same(got, exp)


def test_three_two_cadence_against_the_host_composition(model16):
    """One frame in five repeats (A B C D D E F G H H I): x3 on the reference's timeline; a gap of 2 owns 6 outputs, which
    is two runs of at most 3 instants."""
    base, _, _ = Y._clip(9, 48, 80, '420', 8, seed=6)
    data = _repeat(base, [1, 1, 1, 2, 1, 1, 1, 2, 1])
    kept, hdr, pays = _kept(data)
    assert kept == [0, 1, 2, 3, 5, 6, 7, 8, 10] and len(pays) == 11
    r = Fraction(3)
    exp, _, runs = _expected(model16, data, 2, r, 'bt601', kept)
    # the gap 3 -> 5 owns S0 and 5 St: two runs; the gap 8 -> 10 ends at tau = n - 2 = 9 after S0 and 3 St: one run
    assert len(runs) == len(K.windows(kept, 11, False, r)) + 1
    assert [len(ts) for tup, ts in runs if tup == (2, 3, 4, 5)] == [3, 2] and [len(ts) for tup, ts in runs if tup == (6, 7, 8, 8)] == [3]
    vr, nw, nf, got = _run(model16, data, 2, mfi=3, dedup=True)
    assert (nw, nf) == (len(K.windows(kept, 11, False, r)), R.n_output_frames(11, 3)) and vr.last_dups == [4, 9]
    Y._same(got, exp)
    assert _run(model16, data, 2, mfi=3)[3] != got


def test_with_scene_cut(model16):
    """A doubled clip with a hard cut: the cut is scored between KEPT frames (the doubled stream's own SAD series has a zero
    before and after the cut, which halves its score) and the frames around it hold the nearer kept frame."""
    cut = 3

    def look(i, bgr, peak):
        return bgr if i < cut else (bgr // 2 + peak // 2).astype(bgr.dtype)     # another scene: brighter, half the contrast
    base, _, _ = Y._clip(7, 48, 80, '420', 8, seed=1, look=look)
    data = _repeat(base, [2] * 7)
    params = (256, 107, Fraction(1, 3))                  # thresholds of its own, through the tuple form
    kept, hdr, pays = _kept(data, hi=params[0], lo=params[1], frac=params[2])
    assert kept == list(range(0, 14, 2))
    P = y4m.payload_size(48, 80)
    cuts = S.cuts_of([S.sad_np(pays[kept[j]], pays[kept[j - 1]]) for j in range(1, len(kept))], P, S.DEFAULT_THRESHOLD)
    assert cuts == [cut]
    exp, n_cut, _ = _expected(model16, data, 2, Fraction(2), 'bt601', kept, full_length=True, cuts=cuts)
    vr, nw, nf, got = _run(model16, data, 2, mfi=2, full_length=True, dedup=params, scene_cut=S.DEFAULT_THRESHOLD)
    assert (nw, nf) == (6, 28) and vr.last_cuts == [kept[cut]] and vr.last_cut_windows == n_cut == 1
    Y._same(got, exp)
    assert _run(model16, data, 2, mfi=2, full_length=True, dedup=params)[3] != got


def test_with_tiles(model16):
    h, w, tile, margin = 96, 160, (64, 96), 16
    base, _, _ = Y._clip(4, h, w, '420', 8, seed=4)
    data = _repeat(base, [1, 2, 1, 2])
    kept = _kept(data)[0]
    assert kept == [0, 1, 3, 4]
    p = T.plan_tiles(h, w, tile, margin)
    assert p.n_tiles == 4 and p.grid == (2, 2)
    exp, _, _ = _expected(model16, data, 2, Fraction(2), 'bt601', kept, full_length=True, plan=p)
    vr, nw, nf, got = _run(model16, data, 2, batch=2, mfi=2, full_length=True, dedup=True, tile=tile, tile_margin=margin)
    assert (nw, nf) == (3, 12) and vr.last_plan == p and vr.last_dups == [2, 5]
    Y._same(got, exp)


def test_with_high_depth(model16):
    base, _, _ = Y._clip(5, 48, 80, '420', 10, seed=2)
    data = _repeat(base, [2, 1, 2, 1, 1])
    kept = _kept(data)[0]
    assert kept == [0, 2, 3, 5, 6]
    exp, _, _ = _expected(model16, data, 2, Fraction(2), 'bt601', kept)
    vr, nw, nf, got = _run(model16, data, 2, mfi=2, dedup=True, high_depth=True)
    assert nf == R.n_output_frames(7, 2) and vr.last_dups == [1, 4] and vr.last_depth == 10
    Y._same(got, exp)


def test_with_a_422_stream(model16):
    base, _, _ = Y._clip(5, 48, 80, '422', 8, seed=7)
    data = _repeat(base, [1, 3, 1, 1, 2])
    kept = _kept(data)[0]
    assert kept == [0, 1, 4, 5, 6]
    exp, _, _ = _expected(model16, data, 2, Fraction(2), 'bt601', kept, full_length=True)
    vr, nw, nf, got = _run(model16, data, 2, mfi=2, full_length=True, dedup=True, layouts=True)
    assert nf == 16 and vr.last_dups == [2, 3, 7] and vr.last_layout == '422'
    Y._same(got, exp)


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')

    def seekable(self):
        return False


def test_a_pipe_is_never_seeked_and_ranks_are_refused(model16, tmp_path):
    base, _, _ = Y._clip(5, 48, 80, '420', 8, seed=8)
    data = _repeat(base, [1, 2, 2, 1, 1])
    exp = _run(model16, data, 2, batch=2, mfi=2, dedup=True)[3]
    vr = VideoRunner(model16, 2, batch=2, mfi=2, matrix='bt601', dedup=True)
    chunks = []

    class Out(io.RawIOBase):
        def writable(self):
            return True

        def write(self, b):
            chunks.append(bytes(b))
            return len(b)
    nw, nf = vr.run_stream(_Pipe(data), Out())
    assert b''.join(chunks) == exp and nf == R.n_output_frames(7, 2) and vr.last_dups == [2, 4]
    assert vr.last_decode_peak <= 2 + 5 + K.DEFAULT_MAX_HOLD
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    with pytest.raises(ValueError, match='prefix'):
        vr.run_file(str(src), str(dst), world=2, rank=0)
    assert vr.run_file(str(src), str(dst)) == (nw, nf) and dst.read_bytes() == exp and vr.last_dups == [2, 4]
    for bad in (dict(dedup=(100, 200, Fraction(1, 3))), dict(dedup=(768, 320, Fraction(3, 2))), dict(dedup=True, dedup_max_hold=0)):
        with pytest.raises(ValueError):
            VideoRunner(model16, 2, mfi=2, **bad)


def test_repeats_off_by_one_lsb_are_found(model16):
    """The repeats carry +-1 LSB of noise on every sample, as a lossy encoder leaves it."""
    base, _, _ = Y._clip(5, 48, 80, '420', 8, seed=9)
    head, pays = _split(base)
    rng = np.random.default_rng(1)

    def noisy(p):
        a = np.frombuffer(p, np.uint8).astype(np.int64)
        return np.clip(a + rng.choice([-1, 1], a.size), 0, 255).astype(np.uint8).tobytes()
    seq = [pays[0], noisy(pays[0]), pays[1], pays[2], noisy(pays[2]), noisy(pays[2]), pays[3], pays[4], noisy(pays[4])]
    data = _join(head, seq)
    kept = _kept(data)[0]
    assert kept == [0, 2, 3, 6, 7]
    exp, _, _ = _expected(model16, data, 2, Fraction(2), 'bt601', kept, full_length=True)
    vr, nw, nf, got = _run(model16, data, 2, mfi=2, full_length=True, dedup=True)
    assert vr.last_dups == [1, 4, 5, 8] and nf == 18
    Y._same(got, exp)
