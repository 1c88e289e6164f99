"""Motion-adaptive deinterlacing (``--deinterlace --deinterlace-mode adaptive``) on a real MI355X: ``demfi_yuv_deint_adaptive``
(csrc/deint.hip) equal to ``deint.adaptive_payload_np`` byte for byte, in place, and ``VideoRunner`` over ``It`` / ``Ib`` streams
byte-identical to an expectation that never runs the new kernel or the deferred launches: the progressive stream of 2n frames at 2F
built on the host with ``adaptive_payload_np`` and run through the same runner WITHOUT ``deinterlace``.  Clips, model and helpers are
those of tests/test_gpu_deint.py."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fractions import Fraction                                                       # noqa: E402

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import deint as I                                                     # noqa: E402
from demfi_amd import pipeline as P                                                  # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_deint as D                                                # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
GUARD = 0xC7
# (P2, P1, cur, N1, N2) present: all five, the first field of a stream, the last, and both fields of a one-payload stream
PATTERNS = [(1, 1, 1, 1, 1), (0, 0, 1, 1, 1), (1, 1, 1, 0, 0), (0, 0, 1, 1, 0), (0, 1, 1, 0, 0)]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _five(h, w, layout, depth, seed, far):
    """Five payloads: the edges-over-noise payload of tests/test_gpu_deint.py and four neighbours, near it (small noise: the clamp
    is active at some samples, idle at others) or unrelated to it (``far``)."""
    g = np.random.RandomState(seed)
    peak = (1 << depth) - 1
    cur = D._payload(h, w, layout, depth, seed)
    if far:
        return [D._payload(h, w, layout, depth, seed + 1 + i) if i != 2 else cur for i in range(5)]
    s = max(peak >> 4, 1)
    return [np.clip(cur.astype(np.int64) + g.randint(-s, s + 1, cur.shape), 0, peak).astype(cur.dtype) if i != 2 else cur for i in range(5)]


def _launch(slots, fields, h, w, layout, lead=0, gap=0):
    """``slots``: payloads (1-D uint8 / uint16 arrays) laid out at a stride of their bytes + ``gap`` behind ``lead`` guard bytes;
    ``fields``: (five slot numbers or None, q) per field -> every slot after ONE demfi_yuv_deint_adaptive launch; every byte before,
    between and after the slots is intact."""
    sb, n, pb = slots[0].itemsize, len(slots), slots[0].nbytes
    stride = pb + gap
    buf = np.full(lead + n * stride + 64, GUARD, np.uint8)
    for i, p in enumerate(slots):
        buf[lead + i * stride:lead + i * stride + pb] = p.view(np.uint8)
    dev = torch.from_numpy(buf).to(DEV)
    offs = np.array([[-1 if s is None else lead + s * stride for s in five] for five, _ in fields], np.int64).reshape(-1)
    offs_dev = torch.from_numpy(offs).to(DEV)
    mask = sum(int(q) << i for i, (_, q) in enumerate(fields))
    L.check(L.load().demfi_yuv_deint_adaptive(dev.data_ptr(), dev.numel(), offs.ctypes.data, offs_dev.data_ptr(), len(fields), h, w,
                                              L.YUV_LAYOUT[layout], sb, mask, torch.cuda.current_stream().cuda_stream), 'yuv_deint_adaptive')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert (out[:lead] == GUARD).all() and (out[lead + (n - 1) * stride + pb:] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(slots[0].dtype) for i in range(n)]


def _check_fields(h, w, layout, depth, seed):
    """Both parities x every neighbour pattern, near and far neighbours alternating, in ONE launch: field i owns slots 5i .. 5i+4."""
    cases = [(q, pat, (k + q) & 1) for q in (0, 1) for k, pat in enumerate(PATTERNS)]
    slots, fields = [], []
    for i, (q, pat, far) in enumerate(cases):
        slots += _five(h, w, layout, depth, seed + 7 * i, far)
        fields.append(([5 * i + j if on else None for j, on in enumerate(pat)], q))
    got = _launch(slots, fields, h, w, layout)
    for i, (q, pat, far) in enumerate(cases):
        five = slots[5 * i:5 * i + 5]
        exp = I.adaptive_payload_np([p if on else None for p, on in zip(five, pat)], h, w, depth, layout, q)
        bad = np.flatnonzero(got[5 * i + 2] != exp)
        assert bad.size == 0, ('q=%d pattern=%s far=%d: %d of %d samples differ' % (q, pat, far, bad.size, exp.size), bad[:10])
        D._kept_rows_same(got[5 * i + 2], five[2], h, w, layout, q)
        for j in (0, 1, 3, 4):                                            # a neighbour is only read
            assert np.array_equal(got[5 * i + j], five[j]), (i, j)
    return slots, cases


@pytest.mark.parametrize('depth', [8, 10, 16], ids=['bytes', '10-bit', '16-bit'])
@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('h,w', [(2, 2), (3, 2), (4, 7), (5, 8), (6, 9), (7, 17), (9, 70), (33, 47), (70, 9)])
def test_kernel_equals_the_numpy_definition(h, w, layout, depth):
    slots, cases = _check_fields(h, w, layout, depth, h * 31 + w + depth)
    if h >= 9 and w >= 9:                                                 # the data exercises the clamp and leaves it idle elsewhere
        five = slots[:5]
        a, b = I.adaptive_payload_np(five, h, w, depth, layout, 0), I.bob_payload_np(five[2], h, w, depth, layout, 0)
        assert (a != b).any() and (a == b).mean() > 0.5


def test_full_size_point():
    h, w = 1088, 1920
    five = _five(h, w, '420', 8, 11, False)
    got = _launch(five, [([0, 1, 2, 3, 4], 0)], h, w, '420')
    exp = I.adaptive_payload_np(five, h, w, 8, '420', 0)
    assert np.array_equal(got[2], exp) and (exp != I.bob_payload_np(five[2], h, w, 8, '420', 0)).any()
    for j in (0, 1, 3, 4):
        assert np.array_equal(got[j], five[j])


@pytest.mark.parametrize('depth', [8, 10], ids=['bytes', '10-bit'])
@pytest.mark.parametrize('n', [3, 64])
def test_a_stream_in_one_launch_at_padded_strides_and_unaligned_offsets(n, depth):
    """The slots of a stream as the edge holds them -- slot f is the copy of payload f // 2 that belongs to field f -- and fields
    0 .. n-1 rebuilt by ONE launch: every neighbour a lane reads is rewritten by the same launch, which the hazard rule allows.
    n = 3 of 4 fields leaves field 3 raw.  Odd byte offsets for bytes, even but unaligned ones for 16-bit samples."""
    h, w, layout, order = 37, 61, '420', 'b'
    nf = n + (n & 1)
    pays = [D._payload(h, w, layout, depth, 100 + p) if p % 3 else _five(h, w, layout, depth, 99 + p, False)[0] for p in range(nf // 2)]
    slots = [pays[f // 2] for f in range(nf)]
    fields = [([g for g in I.field_neighbours(f, nf)], I.field_parity(order, f)) for f in range(n)]
    lead, gap = (3, 5) if depth == 8 else (6, 10)
    got = _launch(slots, fields, h, w, layout, lead=lead, gap=gap)
    exp = I.adaptive_stream_np(pays, h, w, depth, layout, order)
    for f in range(n):
        assert np.array_equal(got[f], exp[f]), f
        D._kept_rows_same(got[f], slots[f], h, w, layout, I.field_parity(order, f))
    for f in range(n, nf):
        assert np.array_equal(got[f], slots[f])


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    fn = lib.demfi_yuv_deint_adaptive
    good = np.array([0, 24, 48, 72, 96, -1, -1, 120, 144, -1], np.int64)   # 4x4 4:2:0 payloads of 24 bytes; field 1 is a first field
    good_dev = torch.from_numpy(good).to(DEV)
    ok = [buf.data_ptr(), 256, good.ctypes.data, good_dev.data_ptr(), 2, 4, 4, L.YUV_LAYOUT['420'], 1, 1, st]

    def bad(i, v, offs=None, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        if offs is not None:
            o = np.array(offs, np.int64)
            a[2] = o.ctypes.data
        return fn(*a) == ERR_ARG
    assert bad(0, None) and bad(2, None) and bad(3, None) and bad(4, -1) and bad(4, 65)
    assert bad(5, 1) and bad(6, 1) and bad(5, 16385) and bad(6, 16385)
    assert bad(7, -1) and bad(7, 4) and bad(8, 0) and bad(8, 3)
    assert bad(0, buf.data_ptr() + 1, _8=2)                               # 16-bit samples at an odd address
    assert bad(4, 2, offs=[0, 24, -1, 72, 96, -1, -1, 120, 144, -1])      # the field's own payload is absent
    assert bad(4, 2, offs=[0, -1, 48, -1, 96, -1, -1, 120, 144, -1])      # neither the field before nor the one after
    assert bad(4, 2, offs=[0, 24, 48, 72, 96, -1, -1, 233, 144, -1])      # a payload that leaves the buffer
    assert bad(4, 2, offs=[0, 24, 48, 72, -2, -1, -1, 120, 144, -1])      # an offset below -1
    assert bad(4, 2, offs=[0, 24, 48, 72, 96, -1, -1, 48, 144, -1])       # two fields rebuild one payload
    assert bad(1, 167)                                                    # the buffer ends inside payload 144 .. 167
    assert bad(4, 2, offs=[0, 24, 49, 72, 96, -1, -1, 120, 144, -1], _8=2, _5=2, _6=4)   # 16-bit samples at an odd offset
    assert b'demfi_yuv_deint_adaptive' in lib.demfi_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    a = list(ok)
    a[4] = 0
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert fn(*ok) == 0                                                   # flat planes stay flat
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    assert L.ABI_VERSION == 8                                             # the ABI is additive


# ---- 2. streams ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


def _adaptive(data):
    """The progressive stream of 2n frames at 2F, on the host: frame f from the payloads that hold fields f-2 .. f+2."""
    hdr, pays = D._parse(data)
    outs = I.adaptive_stream_np(pays, hdr.h, hdr.w, hdr.depth, hdr.layout, hdr.interlace)
    return I.progressive_header(hdr).encode() + b''.join(b'FRAME\n' + o.tobytes() for o in outs)


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


ON = dict(deinterlace=True, deinterlace_mode='adaptive')


def _check(model, data, n_fields, batch=4, pipe=False, **kw):
    """``data`` (It / Ib) in adaptive mode == its host-deinterlaced progressive stream without ``deinterlace``."""
    prog = _adaptive(data)
    ve, nwe, nfe, exp = _run(model, prog, batch, **kw)
    vr, nw, nf, got = _run(model, data, batch, pipe, **ON, **kw)
    r = vr._ratio(I.progressive_header(D._parse(data)[0]))
    assert (nw, nf) == (nwe, nfe) and nf == R.n_output_frames(n_fields, r, kw.get('full_length', False)) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')] and b' Ip ' in got[:80]
    Y._same(got, exp)
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts) == (ve.last_instants, ve.last_st_frames, ve.last_cuts)
    return vr, got


def _today(model, data, **kw):
    """``--deinterlace`` alone and ``--deinterlace-mode bob`` give the bytes of the host-bobbed stream, as before."""
    exp = _run(model, D._bobbed(data), **kw)[3]
    for mode in ({}, {'deinterlace_mode': 'bob'}):
        Y._same(_run(model, data, deinterlace=True, **mode, **kw)[3], exp)
    return exp


@pytest.mark.parametrize('order', ['t', 'b'])
def test_both_field_orders_at_x2(order, model16, monkeypatch):
    n = 6
    data = D._interlaced(Y._clip(n, 64, 96, '420', 8, seed=3, fps=b'25:1')[0], order)
    ups = []
    up = P.Y4mEdge.upload
    monkeypatch.setattr(P.Y4mEdge, 'upload', lambda self, sl, idx, f: (ups.append(idx), up(self, sl, idx, f))[1])
    vr, got = _check(model16, data, 2 * n, mfi=2)
    assert got.startswith(b'YUV4MPEG2 W96 H64 F100:1 Ip ') and vr.last_fps_out == 100
    assert sorted(ups[2 * n:]) == list(range(2 * n))                      # after the progressive run's 2n: every field once, as the bob does
    assert vr.last_decode_peak <= 4 + 5 + 2
    bob = _today(model16, data, mfi=2)
    assert len(bob) == len(got) and bob != got                            # the mode matters
    other = _run(model16, D._retag(data, order.encode(), b'b' if order == 't' else b't'), mfi=2, **ON)[3]
    assert len(other) == len(got) and other != got                        # and so does the field order


@pytest.mark.parametrize('fps', [Fraction(50), Fraction(120)], ids=['field-rate', '12/5'])
def test_fps_counts_from_the_field_rate(fps, model16):
    n = 6
    data = D._interlaced(Y._clip(n, 48, 80, '420', 8, seed=4, fps=b'25:1')[0], 't')
    vr, got = _check(model16, data, 2 * n, fps=fps)
    assert vr.last_fps_out == fps
    _today(model16, data, fps=fps)


@pytest.mark.parametrize('cut', [6, 7], ids=['between-payloads', 'between-the-fields-of-a-payload'])
def test_scene_cut(cut, model16):
    """Fields 0 .. cut-1 show one scene, the rest another.  Nothing special happens at the cut: diff is large there and the
    fields next to it get the bob's value."""
    h, w, n, order = 64, 96, 7, 't'
    head, a, _ = Y._clip(n, h, w, '420', 8, seed=1, fps=b'25:1')
    _, b, _ = Y._clip(n, h, w, '420', 8, seed=1, fps=b'25:1', look=lambda i, bgr, peak: ((peak - bgr) // 3).astype(bgr.dtype))
    pays = [D._weave(*[(a if f < cut else b)[p] for f in (2 * p, 2 * p + 1)], h, w, I.field_parity(order, 2 * p)) for p in range(n)]
    data = D._interlaced(head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), order)
    vr, got = _check(model16, data, 2 * n, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [cut] and vr.last_cut_windows >= 1


def test_full_length(model16):
    n = 6
    data = D._interlaced(Y._clip(n, 48, 80, '420', 8, seed=2, fps=b'30000:1001')[0], 'b')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, full_length=True)
    assert got.startswith(b'YUV4MPEG2 W80 H48 F120000:1001 Ip ') and len(D._parse(got)[1]) == 2 * n * 2
    _today(model16, data, batch=2, mfi=2, full_length=True)


def test_tiles(model16):
    h, w, tile, margin, n = 96, 160, (64, 96), 16, 6
    data = D._interlaced(Y._clip(n, h, w, '420', 8, seed=4)[0], 't')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def test_422p10_with_high_depth_and_any_layout(model16):
    n = 6
    data = D._interlaced(Y._clip(n, 48, 80, '422', 10, seed=5)[0], 'b')
    vr, got = _check(model16, data, 2 * n, mfi=2, high_depth=True, layouts=True)
    assert (vr.last_depth, vr.last_layout) == (10, '422') and b' C422p10' in got[:80]


def test_tiled_420p10_with_tile_high_depth(model16):
    h, w, tile, margin, n = 96, 160, (64, 96), 16, 6
    data = D._interlaced(Y._clip(n, h, w, '420', 10, seed=7)[0], 't')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, tile=tile, tile_margin=margin, high_depth=True, tile_high_depth=True)
    assert vr.last_depth == 10 and vr.last_plan.n_tiles == 4


def test_files_two_ranks_and_batch_sizes(model16, tmp_path):
    """Output field f depends on payloads p-1, p, p+1 of the whole input, not on batches or blocks: ``run_file`` on one rank,
    ranks 0 and 1 of two (their blocks meet mid-stream, rank 1's starts at field 5 inside payload 2, so each block reads the two
    fields beyond its end of the other's) and batch sizes 1 and 4 all give the bytes of the stream run."""
    n = 6
    data = D._interlaced(Y._clip(n, 48, 80, '420', 8, seed=8)[0], 't')
    vr, exp = _check(model16, data, 2 * n, mfi=2)
    for batch in (1, 4):
        assert _run(model16, data, batch, mfi=2, **ON)[3] == exp
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', **ON)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (2 * n - 3, R.n_output_frames(2 * n, 2))
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot, firsts = [0, 0], []
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', **ON)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        firsts.append(a)
    assert tot == [nw, nf] and firsts == [5, 4]
    Y._same(dst.read_bytes(), exp)
    # and with the full-length timeline and scene cuts, where a block also rebuilds the field before its first window
    kw = dict(mfi=2, full_length=True, scene_cut=S.DEFAULT_THRESHOLD)
    exp = _run(model16, _adaptive(data), batch=2, **kw)[3]
    dst.unlink()
    for rank in range(2):
        VideoRunner(model16, 1, batch=2, matrix='bt601', **ON, **kw).run_file(str(src), str(dst), world=2, rank=rank)
    Y._same(dst.read_bytes(), exp)


def test_a_pipe(model16):
    n = 5
    data = D._interlaced(Y._clip(n, 48, 80, '420', 8, seed=9, fps=b'25:1')[0], 't')
    _check(model16, data, 2 * n, batch=2, pipe=True, mfi=2)


def test_dedup_is_refused_before_anything_is_allocated(model16):
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError, match='--deinterlace-mode bob'):
        VideoRunner(model16, 1, mfi=2, matrix='bt601', dedup=True, **ON)
    with pytest.raises(ValueError, match='needs --deinterlace'):
        VideoRunner(model16, 1, mfi=2, matrix='bt601', deinterlace_mode='adaptive')
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
