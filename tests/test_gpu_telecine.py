"""Inverse telecine (``--ivtc``) on a real MI355X: ``demfi_luma_comb_counts`` and ``demfi_luma_woven_sad`` (csrc/ivtc.hip) equal to
``telecine.comb_counts_np`` / ``woven_sad_np`` integer for integer, and ``VideoRunner(ivtc=True)`` on a telecined clip byte-identical
to ``VideoRunner()`` on the film clip it was made from, with a header at 4/5 of the rate: an expectation that runs no new code.
The clip, the model and the stream helpers are those of tests/test_gpu_dedup.py."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import telecine as TC                                                 # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
GUARD = 0x5A5A5A5A
BIG = 255                                                # a threshold nothing reaches: samples stay below 255 s


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------
def _planes(h, w, sb, seed):
    """Four luma planes (uint8, or uint16 samples at 10 bits): a top payload and three candidates for its bottom field, cut from
    vertical bars that move 3 samples per instant under a gentle vertical ramp and +-1 of noise.  c is the top's own instant on the
    left half and the next instant on the right half (clean and combed blocks), p the instant before, n the one two after."""
    rng = np.random.default_rng(seed)
    s = 1 if sb == 1 else 4
    bars = np.repeat(rng.integers(30, 220, (w + 16) // 4 + 1), 4)

    def at(t):
        return bars[3 * t:3 * t + w][None, :] + (np.arange(h) % 4)[:, None] + rng.integers(-1, 2, (h, w))
    top = at(1)
    c = np.where(np.arange(w)[None, :] < w // 2, top, at(2))
    dt = np.uint8 if sb == 1 else np.uint16
    return [(p * s).astype(dt).reshape(-1) for p in (top, c, at(0), at(3))]


def _pack(planes, gaps, fill=0xEE):
    """The planes behind gaps of ``gaps`` bytes in one buffer: (bytes, byte offsets)."""
    chunks, offs, pos = [], [], 0
    for p, g in zip(planes, gaps):
        chunks.append(np.full(g, fill, np.uint8))
        pos += g
        offs.append(pos)
        chunks.append(p.view(np.uint8))
        pos += p.nbytes
    return np.concatenate(chunks + [np.full(64, fill, np.uint8)]), offs


def _comb_gpu(buf, tops, bots, h, w, sb, thresh_s):
    """buf: the bytes of a device buffer; entries at byte offsets (bots: three per entry, -1 absent) -> [[(max_block, total)] * 3];
    the guards around the output hold and the buffer is unchanged."""
    lib, n = L.load(), len(tops)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    offs = torch.tensor(list(tops) + [b for e in bots for b in e], dtype=torch.int64, device=DEV)
    out = torch.from_numpy(np.full(6 * n + 2, GUARD, np.uint32).view(np.int32)).to(DEV)
    L.check(lib.demfi_luma_comb_counts(dev.data_ptr(), offs.data_ptr(), offs[n:].data_ptr(), n, h, w, sb, thresh_s, out[1:].data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), 'luma_comb_counts')
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    assert o[0] == GUARD and o[-1] == GUARD
    assert bytes(dev.cpu().numpy()) == bytes(np.ascontiguousarray(buf))
    return [[(int(o[1 + 6 * i + 2 * k]), int(o[2 + 6 * i + 2 * k])) for k in range(3)] for i in range(n)]


def _sad_gpu(buf, quads, h, w, sb):
    lib, n = L.load(), len(quads)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    offs = torch.tensor([o for q in quads for o in q], dtype=torch.int64, device=DEV)
    out = torch.full((n + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    L.check(lib.demfi_luma_woven_sad(dev.data_ptr(), offs.data_ptr(), n, h, w, sb, out[1:].data_ptr(), torch.cuda.current_stream().cuda_stream),
            'luma_woven_sad')
    torch.cuda.synchronize()
    o = out.tolist()
    assert o[0] == o[-1] == 0x5A5A5A5A5A5A5A5A
    assert bytes(dev.cpu().numpy()) == bytes(np.ascontiguousarray(buf))
    return o[1:-1]


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
@pytest.mark.parametrize('h,w', [(5, 2), (6, 7), (7, 5), (18, 70), (33, 47), (70, 9), (64, 128), (1088, 1920)])
def test_kernels_equal_the_numpy_definitions(h, w, sb):
    planes = _planes(h, w, sb, h * 31 + w)
    depth = 8 if sb == 1 else 10
    buf, offs = _pack(planes, [0, 0, 0, 0])
    top, cands = planes[0], planes[1:]
    for cthresh in (TC.DEFAULT_CTHRESH, 0, BIG):
        exp = [TC.comb_counts_np(top, b, h, w, depth, cthresh) for b in cands]
        got = _comb_gpu(buf, [offs[0]], [offs[1:]], h, w, sb, cthresh << (depth - 8))
        print('%dx%d, %d bytes per sample, cthresh %d: kernel %s numpy %s' % (h, w, sb, cthresh, got[0], exp))
        assert got == [exp]
        if cthresh == BIG:
            assert exp == [(0, 0)] * 3
    if w >= 47:                                          # the candidates differ, and c has clean blocks and combed ones
        exp = [TC.comb_counts_np(top, b, h, w, depth) for b in cands]
        assert len(set(exp)) == 3 and all(e[0] > 0 for e in exp)
        sums = TC.block_sums_np(TC.combed_np(TC.woven_luma_np(top, cands[0], h, w, depth), TC.DEFAULT_CTHRESH << (depth - 8)))
        assert (sums == 0).any() and (sums > 0).any()
    assert _comb_gpu(buf, [offs[0]], [[offs[0], -1, offs[0]]], h, w, sb, 0)[0][1] == (0, 0)          # absent: its words stay 0
    quads = [(offs[0], offs[1], offs[2], offs[3]), (offs[0], offs[0], offs[0], offs[2]), (offs[1], offs[2], offs[1], offs[2])]
    exp = [TC.woven_sad_np(*(planes[offs.index(o)] for o in q), h, w, depth) for q in quads]
    got = _sad_gpu(buf, quads, h, w, sb)
    print('%dx%d, %d bytes per sample: woven SADs kernel %s numpy %s' % (h, w, sb, got, exp))
    assert got == exp and exp[0] > 0 and exp[1] > 0 and exp[2] == 0


@pytest.mark.parametrize('sb', [1, 2], ids=['bytes', '16-bit'])
def test_a_batch_of_entries_at_unaligned_offsets(sb):
    h, w = 37, 61                                        # rows start at every alignment
    depth = 8 if sb == 1 else 10
    planes = _planes(h, w, sb, 11) + _planes(h, w, sb, 12)
    gaps = [3, 5, 1, 7, 9, 11, 13, 3] if sb == 1 else [2, 6, 10, 14, 18, 22, 26, 2]      # byte offsets: odd for bytes, 2 mod 4 for samples
    buf, offs = _pack(planes, gaps)
    assert all(o % 2 == 1 for o in offs) if sb == 1 else all(o % 4 == 2 for o in offs)
    entries = [(0, (1, 2, 3)), (4, (5, 6, 7)), (0, (0, None, 3)), (4, (4, 5, None)), (3, (2, 1, 0)), (7, (None, None, 6)), (1, (1, 1, 1))]
    got = _comb_gpu(buf, [offs[t] for t, _ in entries], [[-1 if b is None else offs[b] for b in bots] for _, bots in entries], h, w, sb,
                    TC.DEFAULT_CTHRESH << (depth - 8))
    exp = [[(0, 0) if b is None else TC.comb_counts_np(planes[t], planes[b], h, w, depth) for b in bots] for t, bots in entries]
    print(got, exp)
    assert got == exp and len({e for row in exp for e in row}) >= 8 and exp[2][0] == (0, 0) and exp[6] == [exp[6][0]] * 3
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (7, 0, 3, 4), (2, 2, 2, 2), (5, 1, 5, 0)]
    assert _sad_gpu(buf, [tuple(offs[i] for i in q) for q in quads], h, w, sb) == \
        [TC.woven_sad_np(*(planes[i] for i in q), h, w, depth) for q in quads]


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.full((6,), 0x5A5A, dtype=torch.int32, device=DEV)
    sad = torch.full((1,), 0x5A5A, dtype=torch.int64, device=DEV)
    for fn, ok, ptrs, sizes, sbi, extra in (
            (lib.demfi_luma_comb_counts, (buf.data_ptr(), offs.data_ptr(), offs.data_ptr(), 1, 5, 2, 1, 9, out.data_ptr(), st), (0, 1, 2, 8),
             (4, 5), 6, ((7, -1), (7, (1 << 20) + 1))),
            (lib.demfi_luma_woven_sad, (buf.data_ptr(), offs.data_ptr(), 1, 5, 2, 1, sad.data_ptr(), st), (0, 1, 6), (3, 4), 5, ())):
        def bad(i, v):
            a = list(ok)
            a[i] = v
            return fn(*a) == ERR_ARG
        nn = sizes[0] - 1
        assert all(bad(i, None) for i in ptrs) and bad(nn, -1)
        assert all(bad(i, v) for i in sizes for v in (1, 16385)) and all(bad(sbi, v) for v in (0, 3, 4)) and all(bad(i, v) for i, v in extra)
        a = list(ok)
        a[0], a[sbi] = buf.data_ptr() + 1, 2                 # 16-bit samples at an odd address
        assert fn(*a) == ERR_ARG
        assert fn.__name__.encode() in lib.demfi_last_error()
        a = list(ok)
        a[nn] = 0                                            # no entry: nothing to do, nothing written
        assert fn(*a) == 0
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A).all()) and bool((sad == 0x5A5A).all()) and bool((buf == 0xA5).all())
    assert lib.demfi_luma_comb_counts(buf.data_ptr(), offs.data_ptr(), offs.data_ptr(), 1, 5, 2, 1, 9, out.data_ptr(), st) == 0
    assert lib.demfi_luma_woven_sad(buf.data_ptr(), offs.data_ptr(), 1, 5, 2, 1, sad.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0] * 6 and sad.tolist() == [0] and bool((buf == 0xA5).all())
    assert L.ABI_VERSION == 8                                # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


FILM_FPS, TELE_FPS = b'24000:1001', b'30000:1001'


def _clips(d=8, order='t', phase=0, tag=None, n=12, seed=5):
    """(the film clip at 24000/1001, the same clip telecined to 30000/1001 with the I tag ``tag``, the CPU stage's counters)."""
    film, _, _ = Y._clip(n, 48, 80, '420', d, seed=seed, fps=FILM_FPS)
    head, pays = D._split(film)
    tele = TC.pulldown_payloads_np([np.frombuffer(p, np.uint8) for p in pays], 48, 80, d, '420', order, phase)
    tele = [t.view(np.uint8) for t in tele]
    out, st = TC.film_of(tele, 48, 80, d, '420')
    assert [o.tobytes() for o in out] == pays              # the host stage gives the film back: what follows compares streams
    tag = tag or b'I' + order.encode()
    thead = b' '.join(b'F' + TELE_FPS if f.startswith(b'F') else tag if f.startswith(b'I') else f
                      for f in head.rstrip(b'\n').split(b' ')) + b'\n'
    return film, thead + b''.join(b'FRAME\n' + t.tobytes() for t in tele), st


def _run(model, data, batch=4, **kw):
    vr = VideoRunner(model, 2, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _counters(vr, st):
    assert vr.last_matches == st.matches and vr.last_dropped == st.dropped and vr.last_combed == st.combed == []
    assert len(vr.last_dropped) == 3 and vr.last_matches['c'] == 9


@pytest.mark.parametrize('order,phase', [('t', 0), ('b', 1)])
def test_a_telecined_clip_gives_the_film_clip(order, phase, model16):
    """The test that needs the feature: 15 telecined payloads at 30000/1001 with --ivtc are, byte for byte, the 12 film frames at
    24000/1001 without it."""
    film, tele, st = _clips(order=order, phase=phase)
    vr0, nw0, nf0, exp = _run(model16, film, mfi=2)
    vr, nw, nf, got = _run(model16, tele, mfi=2, ivtc=True)
    assert (nw, nf) == (nw0, nf0) == (9, 19) and vr.last_fps_out == vr0.last_fps_out == Fraction(48000, 1001)
    _counters(vr, st)
    Y._same(got, exp)
    assert vr0.last_matches == {'c': 0, 'p': 0, 'n': 0} and vr0.last_dropped == []
    for batch in (1, 3):                                 # the stage does not depend on how the windows are batched
        Y._same(_run(model16, tele, batch=batch, mfi=2, ivtc=True)[3], exp)


def test_true_film_rate_to_59_94_through_a_pipe_and_a_file(model16, tmp_path):
    film, tele, st = _clips(order='b', phase=0, tag=b'Im')   # a mixed-mode header is taken as it is
    fps = Fraction(60000, 1001)
    exp = _run(model16, film, fps=fps)[3]
    vr = VideoRunner(model16, 2, matrix='bt601', fps=fps, ivtc=True)
    chunks = []

    class Out(io.RawIOBase):
        def writable(self):
            return True

        def write(self, b):
            chunks.append(bytes(b))
            return len(b)
    nw, nf = vr.run_stream(D._Pipe(tele), Out())
    Y._same(b''.join(chunks), exp)
    _counters(vr, st)
    assert vr.last_fps_out == fps and nf == (12 - 3) * 5 // 2 + 1
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(tele)
    assert vr.run_file(str(src), str(dst)) == (nw, nf)
    Y._same(dst.read_bytes(), exp)
    _counters(vr, st)
    with pytest.raises(ValueError, match='one rank'):
        vr.run_file(str(src), str(dst), world=2, rank=0)


@pytest.mark.parametrize('kw', [dict(scene_cut=S.DEFAULT_THRESHOLD), dict(dedup=True), dict(full_length=True)],
                         ids=['scene_cut', 'dedup', 'full_length'])
def test_with_the_other_switches(kw, model16, tmp_path):
    film, tele, st = _clips(order='t', phase=1, tag=b'Ip')   # wrongly flagged progressive
    vr0, nw0, nf0, exp = _run(model16, film, mfi=2, **kw)
    vr, nw, nf, got = _run(model16, tele, mfi=2, ivtc=True, **kw)
    assert (nw, nf) == (nw0, nf0) and vr.last_cuts == vr0.last_cuts and vr.last_dups == vr0.last_dups
    _counters(vr, st)
    Y._same(got, exp)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'    # and sized and written as a file
    src.write_bytes(tele)
    assert vr.run_file(str(src), str(dst)) == (nw, nf)
    Y._same(dst.read_bytes(), exp)


def test_with_high_depth(model16):
    film, tele, st = _clips(d=10, order='b', phase=1)
    exp = _run(model16, film, mfi=2, high_depth=True)[3]
    vr, nw, nf, got = _run(model16, tele, mfi=2, ivtc=True, high_depth=True)
    assert vr.last_depth == 10 and nf == 19
    _counters(vr, st)
    Y._same(got, exp)
