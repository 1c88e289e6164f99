"""Interlaced input (``--deinterlace``) on a real MI355X: ``demfi_yuv_bob`` (csrc/deint.hip) equal to ``deint.bob_payload_np`` byte for
byte, in place, and ``VideoRunner(deinterlace=True)`` over ``It`` / ``Ib`` streams byte-identical to an expectation that never runs
the new kernel: the progressive stream of 2n frames at 2F built on the host with ``bob_payload_np`` and run through ``VideoRunner``
WITHOUT the switch, a path this change leaves as it was.  The clips and the model are those of tests/test_gpu_y4m_layouts.py."""
import io
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                                                      # noqa: E402
from demfi_amd import cadence as K                                                   # noqa: E402
from demfi_amd import deint as I                                                     # noqa: E402
from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd import tiling as T                                                    # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

DEV = 'cuda:0'
ERR_ARG = -1
GUARD = 0xC7


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
def _payload(h, w, layout, depth, seed):
    """One payload whose planes hold diagonal edges of both slopes over noise, with 0 and the peak among the values: every
    direction of the search wins somewhere."""
    g = np.random.RandomState(seed)
    peak = (1 << depth) - 1
    ch, cw = y4m.chroma_shape(h, w, layout)
    planes = []
    for i, (r, c) in enumerate([(h, w)] + ([(ch, cw)] * 2 if layout != 'mono' else [])):
        yy, xx = np.mgrid[0:r, 0:c]
        p = np.where((xx + yy + i) % 9 < 4, peak, 0) ^ np.where((2 * xx - yy) % 13 < 5, peak // 3, 0)
        p = np.where(g.randint(0, 4, (r, c)) == 0, g.randint(0, peak + 1, (r, c)), p)
        planes.append(p.reshape(-1))
    return np.concatenate(planes).astype(np.uint8 if depth == 8 else np.uint16)


def _bob_gpu(pays, h, w, layout, qs, lead=0, gap=0):
    """The payloads (1-D uint8 / uint16 arrays) at a stride of their bytes + ``gap`` behind ``lead`` guard bytes -> the payloads
    after ONE demfi_yuv_bob launch; every byte before, between and after them is intact."""
    sb, n, pb = pays[0].itemsize, len(pays), pays[0].nbytes
    stride = pb + gap
    buf = np.full(lead + n * stride + 64, GUARD, np.uint8)
    for i, p in enumerate(pays):
        buf[lead + i * stride:lead + i * stride + pb] = p.view(np.uint8)
    dev = torch.from_numpy(buf).to(DEV)
    mask = sum(int(q) << i for i, q in enumerate(qs))
    L.check(L.load().demfi_yuv_bob(dev.data_ptr() + lead, stride, n, h, w, L.YUV_LAYOUT[layout], sb, mask,
                                   torch.cuda.current_stream().cuda_stream), 'yuv_bob')
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    assert (out[:lead] == GUARD).all() and (out[lead + (n - 1) * stride + pb:] == GUARD).all(), 'write outside the payloads'
    for i in range(n - 1):
        assert (out[lead + i * stride + pb:lead + (i + 1) * stride] == GUARD).all(), 'write between payloads %d and %d' % (i, i + 1)
    return [out[lead + i * stride:lead + i * stride + pb].copy().view(pays[0].dtype) for i in range(n)]


def _kept_rows_same(got, pay, h, w, layout, q):
    for a, b in zip(y4m.split_planes_layout(got, h, w, layout), y4m.split_planes_layout(pay, h, w, layout)):
        if a is not None:
            assert np.array_equal(a[q::2], b[q::2])


@pytest.mark.parametrize('depth', [8, 10, 16], ids=['bytes', '10-bit', '16-bit'])
@pytest.mark.parametrize('layout', y4m.LAYOUTS)
@pytest.mark.parametrize('h,w', [(2, 2), (3, 2), (2, 7), (7, 5), (9, 70), (33, 47), (70, 9), (64, 128), (1088, 1920)])
def test_kernel_equals_the_numpy_definition(h, w, layout, depth):
    pay = _payload(h, w, layout, depth, h * 31 + w + depth)
    got = _bob_gpu([pay, pay], h, w, layout, [0, 1])                      # both parities in one launch
    for q in (0, 1):
        exp = I.bob_payload_np(pay, h, w, depth, layout, q)
        bad = np.flatnonzero(got[q] != exp)
        print('%dx%d %s %d-bit q=%d: %d of %d samples differ' % (h, w, layout, depth, q, bad.size, exp.size))
        assert bad.size == 0, bad[:10]
        _kept_rows_same(got[q], pay, h, w, layout, q)
    if h >= 9 and w >= 9:                                                 # the payload exercises the search, not only pred(0)
        y = y4m.split_planes_layout(pay, h, w, layout)[0].astype(np.int64)
        e = y4m.split_planes_layout(I.bob_payload_np(pay, h, w, depth, layout, 0), h, w, layout)[0]
        ys = np.arange(1, h - 1, 2)
        assert (e[ys] != ((y[ys - 1] + y[ys + 1] + 1) >> 1)).any()


@pytest.mark.parametrize('depth', [8, 10], ids=['bytes', '10-bit'])
@pytest.mark.parametrize('n', [1, 3, 64])
def test_batches_at_padded_strides_and_unaligned_offsets(n, depth):
    """Odd byte offsets for bytes, even but unaligned ones for 16-bit samples; a stride larger than the payload whose gap
    survives; a mixed odd_mask up to bit 63."""
    h, w, layout = 37, 61, '420'                                          # odd widths: rows start at every alignment
    pays = [_payload(h, w, layout, depth, 100 + i % 5) for i in range(n)]
    qs = [(i + (i >> 2) + (i >> 4)) & 1 for i in range(n)]             # 0 1 0 1 | 1 0 1 0 | ...: mixed from n = 2 on
    if n == 64:
        qs[63] = 1
    assert n == 1 or len(set(qs)) == 2
    lead, gap = (3, 5) if depth == 8 else (6, 10)
    got = _bob_gpu(pays, h, w, layout, qs, lead=lead, gap=gap)
    exp = {(i % 5, q): I.bob_payload_np(pays[i], h, w, depth, layout, q) for i, q in enumerate(qs)}
    for i, q in enumerate(qs):
        assert np.array_equal(got[i], exp[(i % 5, q)]), i
        _kept_rows_same(got[i], pays[i], h, w, layout, q)
    for lay in ('422', '444', 'mono'):                                    # the other layouts at an aligned base and no gap
        p = _payload(h, w, lay, depth, 7)
        g2 = _bob_gpu([p] * min(n, 3), h, w, lay, [1, 0, 1][:min(n, 3)])
        for i, q in enumerate([1, 0, 1][:min(n, 3)]):
            assert np.array_equal(g2[i], I.bob_payload_np(p, h, w, depth, lay, q)), (lay, i)


def test_bad_arguments_are_rejected_and_nothing_is_launched():
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=DEV)
    fn = lib.demfi_yuv_bob
    ok = (buf.data_ptr(), 64, 2, 4, 4, L.YUV_LAYOUT['420'], 1, 1, st)      # two 4x4 4:2:0 payloads of 24 bytes

    def bad(i, v, **kw):
        a = list(ok)
        a[i] = v
        for j, x in kw.items():
            a[int(j[1:])] = x
        return fn(*a) == ERR_ARG
    assert bad(0, None) and bad(2, -1) and bad(2, 65)
    assert bad(3, 1) and bad(4, 1) and bad(3, 16385) and bad(4, 16385)
    assert bad(5, -1) and bad(5, 4) and bad(6, 0) and bad(6, 3) and bad(6, 4)
    assert bad(0, buf.data_ptr() + 1, _6=2) and bad(1, 65, _6=2)          # 16-bit samples: odd address, odd stride
    assert bad(1, 23) and bad(1, 46, _6=2) and bad(1, -64)                # a stride below the payload's bytes
    assert b'demfi_yuv_bob' in lib.demfi_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    a = list(ok)
    a[2] = 0                                                              # no payload: nothing to do, nothing written
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


def _interlaced(data, order):
    """The clip's payloads tagged as interlaced: each is now two fields."""
    return _retag(data, b'p', order.encode())


def _retag(data, old, new):
    """The stream with the header's interlace tag ``I<old>`` replaced by ``I<new>``; the frames are not looked at."""
    at = data.index(b'\n')
    assert data[:at].count(b' I' + old + b' ') == 1
    return data[:at].replace(b' I' + old + b' ', b' I' + new + b' ') + data[at:]


def _parse(data):
    at = data.index(b'FRAME\n')
    hdr = y4m.parse_header(data[:at], y4m.DEPTHS, y4m.LAYOUTS, fields=True)
    step = 6 + hdr.payload
    assert (len(data) - at) % step == 0
    return hdr, [data[i + 6:i + step] for i in range(at, len(data), step)]


def _bobbed(data):
    """The progressive stream of 2n frames at 2F, on the host: frame 2p + s is payload p with the field of
    ``field_parity(order, 2p + s)`` kept and the other rebuilt by ``bob_payload_np``."""
    hdr, pays = _parse(data)
    out = [I.progressive_header(hdr).encode()]
    for p, pay in enumerate(pays):
        for s in (0, 1):
            out += [b'FRAME\n', I.bob_payload_np(pay, hdr.h, hdr.w, hdr.depth, hdr.layout, I.field_parity(hdr.interlace, 2 * p + s)).tobytes()]
    return b''.join(out)


def _run(model, data, batch=4, **kw):
    vr = VideoRunner(model, 1, batch=batch, matrix='bt601', **kw)
    out = io.BytesIO()
    nw, nf = vr.run_stream(io.BytesIO(data), out)
    return vr, nw, nf, out.getvalue()


def _check(model, data, n_fields, batch=4, **kw):
    """``data`` (It / Ib) with the switch == its host-bobbed progressive stream without it, header and payloads."""
    prog = _bobbed(data)
    assert y4m.Reader(io.BytesIO(prog), **Y.ANY).header.interlace == 'p'
    ve, nwe, nfe, exp = _run(model, prog, batch, **kw)
    vr, nw, nf, got = _run(model, data, batch, deinterlace=True, **kw)
    r = vr._ratio(I.progressive_header(_parse(data)[0]))
    assert (nw, nf) == (nwe, nfe) and nf == R.n_output_frames(n_fields, r, kw.get('full_length', False)) and nf > 0
    assert got[:got.index(b'FRAME\n')] == exp[:exp.index(b'FRAME\n')] and b' Ip ' in got[:80]
    Y._same(got, exp)
    assert vr.last_fields == {'t': 'tff', 'b': 'bff'}[_parse(data)[0].interlace] and ve.last_fields is None
    assert (vr.last_instants, vr.last_st_frames, vr.last_cuts, vr.last_dups) == (ve.last_instants, ve.last_st_frames, ve.last_cuts, ve.last_dups)
    return vr, got


@pytest.mark.parametrize('order', ['t', 'b'])
def test_both_field_orders_at_x2(order, model16):
    n = 6
    data = _interlaced(Y._clip(n, 70, 98, '420', 8, seed=3, fps=b'25:1')[0], order)
    vr, got = _check(model16, data, 2 * n, mfi=2)
    assert got.startswith(b'YUV4MPEG2 W98 H70 F100:1 Ip ') and vr.last_fps_out == 100            # 50i in, 100p out
    assert vr.last_decode_peak <= 4 + 5
    other = _run(model16, _retag(data, order.encode(), b'b' if order == 't' else b't'), mfi=2, deinterlace=True)[3]
    assert len(other) == len(got) and other != got                                                # the field order matters


@pytest.mark.parametrize('fps', [Fraction(50), Fraction(120)], ids=['field-rate', '12/5'])
def test_fps_counts_from_the_field_rate(fps, model16):
    n = 6
    data = _interlaced(Y._clip(n, 48, 80, '420', 8, seed=4, fps=b'25:1')[0], 't')
    vr, got = _check(model16, data, 2 * n, fps=fps)
    assert vr.last_fps_out == fps and vr._ratio(I.progressive_header(_parse(data)[0])) == fps / 50


def _weave(pa, pb, h, w, q):
    """Rows of parity q of every plane from payload pa, the others from pb."""
    out = []
    for x, y in zip(y4m.split_planes(pa, h, w), y4m.split_planes(pb, h, w)):
        z = y.copy()
        z[q::2] = x[q::2]
        out.append(z.reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize('cut', [6, 7], ids=['between-payloads', 'between-the-fields-of-a-payload'])
def test_scene_cut_between_fields(cut, model16):
    """Fields 0 .. cut-1 show one scene, the rest another: cut = 7 puts the hard cut between the two fields of payload 3."""
    h, w, n, order = 70, 98, 7, 't'
    head, a, _ = Y._clip(n, h, w, '420', 8, seed=1, fps=b'25:1')
    _, b, _ = Y._clip(n, h, w, '420', 8, seed=1, fps=b'25:1', look=lambda i, bgr, peak: ((peak - bgr) // 3).astype(bgr.dtype))
    pays = [_weave(*[(a if f < cut else b)[p] for f in (2 * p, 2 * p + 1)], h, w, I.field_parity(order, 2 * p)) for p in range(n)]
    data = _interlaced(head[:head.index(b'FRAME\n')] + b''.join(b'FRAME\n' + p.tobytes() for p in pays), order)
    vr, got = _check(model16, data, 2 * n, mfi=2, scene_cut=S.DEFAULT_THRESHOLD)
    assert vr.last_cuts == [cut] and vr.last_cut_windows >= 1
    plain = _run(model16, data, mfi=2, deinterlace=True)[3]
    assert len(plain) == len(got) and plain != got


def test_full_length(model16):
    n = 6
    data = _interlaced(Y._clip(n, 48, 80, '420', 8, seed=2, fps=b'30000:1001')[0], 'b')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, full_length=True)
    assert got.startswith(b'YUV4MPEG2 W80 H48 F120000:1001 Ip ') and len(_parse(got)[1]) == 2 * n * 2


def test_dedup_over_repeated_payloads(model16):
    """A A B C C D: the two fields of a payload, bobbed, differ by what the interpolation misses -- little against the motion from
    one payload to the next -- so with thresholds above that the repeats AND the second field of every payload are dropped, on
    both paths alike."""
    pays = Y._clip(12, 48, 80, '420', 8, seed=6, fps=b'25:1')
    head = pays[0][:pays[0].index(b'FRAME\n')]
    a, b, c, d = pays[1][::3]
    data = _interlaced(head + b''.join(b'FRAME\n' + p.tobytes() for p in (a, a, b, c, c, d)), 't')
    params = (2000, 1200, Fraction(1, 3))
    hdr, fields = Y._read(_bobbed(data))
    assert K.kept_of(fields, 48, 80, 8, hi=params[0], lo=params[1], frac=params[2]) == [0, 4, 6, 10]
    vr, got = _check(model16, data, 12, mfi=2, full_length=True, dedup=params)
    assert vr.last_dups == [1, 2, 3, 5, 7, 8, 9, 11]


def test_tiles(model16):
    h, w, tile, margin, n = 96, 160, (64, 96), 16, 6
    data = _interlaced(Y._clip(n, h, w, '420', 8, seed=4)[0], 't')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, tile=tile, tile_margin=margin)
    assert vr.last_plan == T.plan_tiles(h, w, tile, margin) and vr.last_plan.n_tiles == 4


def test_422p10_with_high_depth_and_any_layout(model16):
    n = 6
    data = _interlaced(Y._clip(n, 48, 80, '422', 10, seed=5)[0], 'b')
    vr, got = _check(model16, data, 2 * n, mfi=2, high_depth=True, layouts=True)
    assert (vr.last_depth, vr.last_layout) == (10, '422') and b' C422p10' in got[:80]


def test_tiled_420p10_with_tile_high_depth(model16):
    h, w, tile, margin, n = 96, 160, (64, 96), 16, 6
    data = _interlaced(Y._clip(n, h, w, '420', 10, seed=7)[0], 't')
    vr, got = _check(model16, data, 2 * n, batch=2, mfi=2, tile=tile, tile_margin=margin, high_depth=True, tile_high_depth=True)
    assert vr.last_depth == 10 and vr.last_plan.n_tiles == 4


def test_files_and_two_ranks(model16, tmp_path):
    """``run_file`` on one rank equals ``run_stream``; ranks 0 and 1 of two, run one after the other into one file (as
    tests/test_gpu_y4m_layouts.py does), equal it too -- rank 1's block starts at an odd field."""
    n = 6
    data = _interlaced(Y._clip(n, 48, 80, '420', 8, seed=8)[0], 't')
    vr, exp = _check(model16, data, 2 * n, mfi=2)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(data)
    one = VideoRunner(model16, 1, mfi=2, batch=4, matrix='bt601', deinterlace=True)
    nw, nf = one.run_file(str(src), str(dst))
    assert (nw, nf) == (2 * n - 3, R.n_output_frames(2 * n, 2)) and one.last_fields == 'tff'
    Y._same(dst.read_bytes(), exp)
    dst.unlink()
    tot, firsts = [0, 0], []
    for rank in range(2):
        v = VideoRunner(model16, 1, mfi=2, batch=2, matrix='bt601', deinterlace=True)
        a, b = v.run_file(str(src), str(dst), world=2, rank=rank)
        tot[0] += a
        tot[1] += b
        firsts.append(a)
    assert tot == [nw, nf] and firsts == [5, 4]                            # rank 1's block starts at field 5, inside payload 2
    Y._same(dst.read_bytes(), exp)
    # and with the full-length timeline and scene cuts, where a block also reads the field before its first window
    kw = dict(mfi=2, full_length=True, scene_cut=S.DEFAULT_THRESHOLD)
    exp = _run(model16, _bobbed(data), batch=2, **kw)[3]
    dst.unlink()
    for rank in range(2):
        VideoRunner(model16, 1, batch=2, matrix='bt601', deinterlace=True, **kw).run_file(str(src), str(dst), world=2, rank=rank)
    Y._same(dst.read_bytes(), exp)


def test_the_switch_changes_nothing_for_progressive_input_and_is_needed_for_interlaced(model16, tmp_path):
    data = Y._clip(6, 48, 80, '420', 8, seed=5)[0]
    outs = [_run(model16, _retag(data, b'p', tag), mfi=2, deinterlace=on)[3] for on in (False, True) for tag in (b'p', b'?')]
    assert outs[0] == outs[1] == outs[2] == outs[3] and len(_parse(outs[0])[1]) == R.n_output_frames(6, 2)
    vr = VideoRunner(model16, 1, mfi=2, matrix='bt601')
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(y4m.Y4MError, match='--deinterlace'):
        vr.run_stream(io.BytesIO(_interlaced(data, 't')), io.BytesIO())
    src = tmp_path / 'in.y4m'
    src.write_bytes(_interlaced(data, 'b'))
    with pytest.raises(y4m.Y4MError, match='--deinterlace'):
        vr.run_file(str(src), str(tmp_path / 'out.y4m'))
    assert vr._runners == {} and torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
    on = VideoRunner(model16, 1, mfi=2, matrix='bt601', deinterlace=True)
    with pytest.raises(y4m.Y4MError, match='field-order fix upstream'):
        on.run_stream(io.BytesIO(_retag(data, b'p', b'm')), io.BytesIO())
    assert on._runners == {}
