"""The temporal denoiser in front of the network (``--denoise``, ``demfi_amd.denoise``) without a GPU: the rule against hand-computed
columns, its identities, the noise it removes, the stream form and its dependency window, the kernel's divisor constants over their whole
range, the switches and their refusals, and the edge's look-ahead bookkeeping driven as the batch loop drives it.  ``noisy_clip`` is the
clip the GPU tests (tests/test_gpu_denoise.py) run: its construction is checked here."""
import ctypes
import io
import itertools
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from demfi_amd import denoise as DN
from demfi_amd import interlace as IL
from demfi_amd import pipeline as P
from demfi_amd import video, y4m
from demfi_amd.y4m_edge import Ingest


def _col(c, before, after, depth=8, a=5, b=10):
    """One sample position: the centre c, the samples of f-1, f-2, .. (``before``) and of f+1, f+2, .. (``after``); None = absent."""
    r = max(len(before), len(after))
    before, after = list(before) + [None] * (r - len(before)), list(after) + [None] * (r - len(after))
    dt = np.uint8 if depth == 8 else np.uint16
    arr = lambda v: None if v is None else np.array([v], dt)             # noqa: E731
    out = DN.denoise_payload_np([arr(v) for v in reversed(before)] + [arr(c)] + [arr(v) for v in after], depth, a, b)
    assert out.dtype == dt and out.shape == (1,)
    return int(out[0])


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_each_side_stops_on_its_own_and_for_good():
    # before: 102 is taken, 120 stops the side, the 101 behind it is never looked at; after: all three are taken
    assert _col(100, [102, 120, 101], [99, 100, 101]) == (2 * (100 + 102 + 99 + 100 + 101) + 5) // 10 == 100
    assert _col(100, [120, 100, 100], [103, 103, 103]) == (2 * (100 + 3 * 103) + 4) // 8 == 102      # the first sample stops its side
    assert _col(100, [120], [120]) == 100 and _col(100, [100, 100, 100], [100, 100, 100]) == 100


def test_the_two_thresholds_at_their_edges():
    assert _col(100, [105], [106]) == (2 * 205 + 2) // 4 == 103           # d == A passes, d == A + 1 stops
    assert _col(100, [95], [94]) == (2 * 195 + 2) // 4 == 98
    # acc == B passes (4 + 4 + 2), acc == B + 1 stops (4 + 4 + 3) though every d <= A
    assert _col(100, [104, 104, 102], [104, 104, 103]) == (2 * (100 + 104 * 4 + 102) + 6) // 12 == 103
    assert _col(100, [104, 96, 102], [100, 100, 100]) == (2 * (100 + 104 + 96 + 102 + 300) + 7) // 14   # |d| adds up: 4 + 4 + 2
    assert _col(100, [104, 96, 103], [100, 100, 100]) == (2 * (100 + 104 + 96 + 300) + 6) // 12
    assert _col(100, [105, 105], [105, 105], a=5, b=5) == (2 * 310 + 3) // 6          # B == A: one sample a side


def test_an_absent_neighbour_ends_its_side():
    assert _col(100, [None, 102], [102]) == 101                           # f-2 is there, f-1 is not: nothing before f is used
    assert _col(100, [None], [None]) == 100 and _col(100, [102, None, 102], [None, 102, 102]) == 101
    with pytest.raises(ValueError):
        DN.denoise_payload_np([np.zeros(1, np.uint8), None, np.zeros(1, np.uint8)], 8, 5, 10)
    with pytest.raises(ValueError):
        DN.denoise_payload_np([np.zeros(1, np.uint8)] * 4, 8, 5, 10)


@pytest.mark.parametrize('n', range(1, 8))
def test_rounding_half_up_for_every_count(n):
    taken = n - 1                                                        # neighbours taken: the first ones of each side, the rest far away
    for ones in range(taken + 1):                                        # ``ones`` of them are c + 1, the others c
        vals = [11] * ones + [10] * (taken - ones)
        before, after = vals[:3] + [99] * (3 - len(vals[:3])), vals[3:] + [99] * (3 - len(vals[3:]))
        exact = Fraction(10 * n + ones, n)
        assert _col(10, before, after) == int(exact + Fraction(1, 2)) == (10 if 2 * ones < n else 11)
    if n % 2 == 0:                                                       # a tie goes up
        assert _col(10, ([11] * (n // 2) + [10] * (n // 2 - 1) + [99] * 3)[:3], ([11] * (n // 2) + [10] * (n // 2 - 1) + [99] * 6)[3:6]) == 11


@pytest.mark.parametrize('depth', [8, 10, 16])
def test_the_thresholds_shift_with_the_depth(depth):
    ad, bd = DN.thresholds(depth, 5, 10)
    assert (ad, bd) == (5 << (depth - 8), 10 << (depth - 8))
    peak = (1 << depth) - 1
    assert _col(peak, [peak - ad], [peak - ad - 1], depth) == (2 * (2 * peak - ad) + 2) // 4      # at the peak: no wrap, no clip
    assert _col(0, [ad], [ad + 1], depth) == (2 * ad + 2) // 4
    assert _col(peak, [peak - ad, peak - ad], [peak - ad, peak - ad - 1], depth) == (2 * (4 * peak - 3 * ad) + 4) // 8    # acc == B_d, B_d + 1
    assert _col(peak, [peak] * 3, [peak] * 3, depth) == peak
    with pytest.raises(ValueError):
        DN.thresholds(9, 5, 10)


# ---- the identities ------------------------------------------------------------------------------------------------------------------
def _random_stream(n, p, depth, seed, spread=None):
    g = np.random.RandomState(seed)
    peak = (1 << depth) - 1
    base = g.randint(0, peak + 1, p)
    spread = (8 << (depth - 8)) if spread is None else spread
    return [np.clip(base + g.randint(-spread, spread + 1, p), 0, peak).astype(np.uint8 if depth == 8 else np.uint16) for _ in range(n)]


@pytest.mark.parametrize('depth', [8, 10, 16])
@pytest.mark.parametrize('radius', [1, 2, 3])
def test_identities(depth, radius):
    pays = _random_stream(9, 500, depth, depth + radius)
    for got, pay in zip(DN.denoise_stream_np(pays, depth, 0, 0, radius), pays):      # A = 0: only equal samples are averaged
        assert np.array_equal(got, pay)
    for got in DN.denoise_stream_np([pays[0]] * 6, depth, 5, 10, radius):             # constant in time
        assert np.array_equal(got, pays[0])
    ad, _ = DN.thresholds(depth, 5, 10)
    outs = DN.denoise_stream_np(pays, depth, 5, 10, radius)
    changed = 0
    for f, out in enumerate(outs):                                       # inside the range of what can have gone into it
        c = pays[f].astype(np.int64)
        near = [np.where(np.abs(pays[g].astype(np.int64) - c) <= ad, pays[g], c) for g in range(max(f - radius, 0), min(f + radius + 1, len(pays)))]
        assert (out >= np.min(near, axis=0)).all() and (out <= np.max(near, axis=0)).all() and (np.abs(out.astype(np.int64) - c) <= ad).all()
        changed += int((out != pays[f]).sum())
    assert changed > 0


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_a_moving_edge_higher_than_a_is_left_alone(radius):
    n, p = 9, 40
    pays = [np.where(np.arange(p) < 10 + f, 50, 56).astype(np.uint8) for f in range(n)]      # the step moves one sample a frame
    for got, pay in zip(DN.denoise_stream_np(pays, 8, 5, 10, radius), pays):
        assert np.array_equal(got, pay)
    soft = [np.where(np.arange(p) < 10 + f, 50, 55).astype(np.uint8) for f in range(n)]      # a step of A is noise to it: it does bleed
    assert any(not np.array_equal(g, s) for g, s in zip(DN.denoise_stream_np(soft, 8, 5, 10, radius), soft))


def test_noise_on_a_static_picture_loses_more_than_half_its_variance():
    g = np.random.RandomState(7)
    clean = g.randint(16, 236, 64 * 96)
    pays = [(clean + g.randint(-3, 4, clean.size)).astype(np.uint8) for _ in range(9)]
    var_in = float(np.mean([(p.astype(np.int64) - clean) ** 2 for p in pays]))
    got = {r: float(np.mean([(o.astype(np.int64) - clean) ** 2 for o in DN.denoise_stream_np(pays, 8, *DN.DEFAULTS, r)])) for r in (1, 2, 3)}
    print('error variance: input %.3f, output R=1 %.3f, R=2 %.3f, R=3 %.3f' % (var_in, got[1], got[2], got[3]))
    assert 3.5 < var_in < 4.5                                            # uniform on -3 .. 3: (7^2 - 1) / 12 = 4
    assert got[DN.DEFAULT_RADIUS] < var_in / 2 and DN.DEFAULT_RADIUS == 2


# ---- streams -------------------------------------------------------------------------------------------------------------------------
def test_stream_ends_parity_and_dependency_window():
    pays = _random_stream(10, 300, 8, 1, spread=3)
    for radius, step in ((1, 1), (2, 1), (3, 1), (1, 2), (2, 2)):
        reach = DN.reach(radius, step == 2)
        assert reach == radius * step
        outs = DN.denoise_stream_np(pays, 8, 5, 10, radius, step)
        for f in range(len(pays)):
            nb = DN.neighbours(f, radius, step, lambda g: g < len(pays))
            assert nb[radius] == f and [g for g in nb if g is not None] == [g for g in range(f - reach, f + reach + 1, step) if 0 <= g < len(pays)]
            assert np.array_equal(outs[f], DN.denoise_payload_np([None if g is None else pays[g] for g in nb], 8, 5, 10))
        assert not np.array_equal(outs[0], pays[0]) and not np.array_equal(outs[-1], pays[-1])      # the ends still average inward
        for f in (0, 4, 9):                                              # frames beyond the reach do not matter, the one at its rim does
            for g in (f - reach - 1, f + reach + 1):
                if 0 <= g < len(pays):
                    other = list(pays)
                    other[g] = np.zeros_like(pays[g])
                    assert np.array_equal(DN.denoise_stream_np(other, 8, 5, 10, radius, step)[f], outs[f])
        if step == 2:                                                    # the other parity is never read
            other = [np.zeros_like(p) if i % 2 else p for i, p in enumerate(pays)]
            for f in range(0, len(pays), 2):
                assert np.array_equal(DN.denoise_stream_np(other, 8, 5, 10, radius, step)[f], outs[f])
    assert DN.neighbours(0, 2, 1, lambda g: g < 2) == [None, None, 0, 1, None]
    assert DN.neighbours(5, 3, 2, lambda g: g < 9) == [None, 1, 3, 5, 7, None, None]
    assert len(DN.denoise_stream_np(pays[:1], 8, 5, 10, 2)) == 1 and np.array_equal(DN.denoise_stream_np(pays[:1], 8, 5, 10, 2)[0], pays[0])


# ---- the divisor constants ---------------------------------------------------------------------------------------------------------
def test_the_kernels_constants_are_exact_over_the_whole_range():
    src = open(os.path.join(os.path.dirname(DN.__file__), 'csrc', 'denoise.hip')).read()
    m = re.search(r'MAGIC\[7\] = \{([0-9u, ]+)\};', src)
    assert tuple(int(t.strip().rstrip('u')) for t in m.group(1).split(',')) == DN.MAGIC and DN.MAX_COUNT == 7
    v = np.arange(2 * 7 * 65535 + 7 + 1, dtype=np.uint64)
    for n in range(1, 8):
        assert DN.MAGIC[n - 1] == DN.magic(n) < 1 << 32
        assert np.array_equal((v * np.uint64(DN.magic(n))) >> np.uint64(32), v // np.uint64(2 * n)), n
    for bad in (0, 8):
        with pytest.raises(ValueError):
            DN.magic(bad)


# ---- the switches ------------------------------------------------------------------------------------------------------------------
def test_parse_denoise_and_check_params():
    assert DN.parse_denoise('5:10') == (5, 10) == DN.DEFAULTS and DN.parse_denoise('5') == (5, 10) and DN.parse_denoise(' 0 ') == (0, 0)
    assert DN.parse_denoise('200') == (200, 255) and DN.parse_denoise('0:255') == (0, 255) and DN.parse_denoise('255:255') == (255, 255)
    for bad in ('', 'a', '5:', ':5', '5:4', '256', '5:256', '-1', '5.0', '5:10:2', '5/10'):
        with pytest.raises(ValueError):
            DN.parse_denoise(bad)
    assert DN.check_params() == (5, 10, 2) and DN.check_params(3, None, 1) == (3, 6, 1) and DN.check_params(3, 3, 3) == (3, 3, 3)
    for bad in ((5, 10, 0), (5, 10, 4), (5, 4, 2), (-1, 3, 2), (5, 256, 2), (5.0, 10, 2), (True, 10, 2), (5, 10, 2.0)):
        with pytest.raises(ValueError):
            DN.check_params(*bad)


def test_edge_spec_with_denoise():
    plain = P.EdgeSpec(True, True, False, 10, '422', None, 't', 'bob')
    dn = P.EdgeSpec(True, True, False, 10, '422', None, 't', 'bob', denoise=(5, 10, 2))
    assert dn.denoise == (5, 10, 2) and plain.denoise is None and tuple(dn) == tuple(plain) and len(plain) == 8
    assert dn != plain and plain != dn and dn != tuple(dn) and plain == tuple(plain)
    assert hash(plain) == hash(P.EdgeSpec(True, True, False, 10, '422', None, 't')) == hash((tuple(plain), None))     # as before there was the field
    assert dn == P.EdgeSpec(True, True, False, 10, '422', None, 't', 'bob', denoise=[5, 10, 2]) and hash(dn) == hash(dn._replace())
    assert dn != dn._replace(denoise=(5, 10, 3)) and dn._replace(denoise=None) == plain and plain._replace(denoise=(5, 10, 2)) == dn
    assert dn._replace(depth=8).denoise == (5, 10, 2) and dn._replace(shutter=(4, 8)).denoise == (5, 10, 2)
    assert len({plain, dn, dn._replace(denoise=(4, 10, 2))}) == 3
    assert 'denoise=(5, 10, 2)' in repr(dn) and 'denoise' not in repr(plain)
    assert repr(plain) == repr(dn._replace(denoise=None))
    # the reach of the ingest: the adaptive deinterlacer's two fields, the denoiser's R frames or 2 R fields
    assert (plain.reach, dn.reach, dn._replace(fields=None).reach, dn._replace(denoise=(5, 10, 3)).reach) == (0, 4, 2, 6)
    assert plain._replace(deint_mode='adaptive').reach == 2
    edge = video.YuvEdge('bt601', False, '420jpeg', None, denoise=(5, 10, 3))
    assert edge.denoise == (5, 10, 3) and P.EdgeSpec.of(edge).denoise == (5, 10, 3)
    assert video.YuvEdge('bt601', False, '420jpeg', None).denoise is None
    assert P.EdgeSpec.of(video.YuvEdge('bt601', False, '420jpeg', None)) == P.EdgeSpec(True)
    with pytest.raises(ValueError):
        video.YuvEdge('bt601', False, '420jpeg', None, denoise=(5, 4, 2))


def test_check_refuses_what_does_not_go_together():
    ok = P.EdgeSpec(True, denoise=(5, 10, 2))
    ok.check(True, False, True)
    ok._replace(fields='t', cuts=True, full=True).check(True, True, True)
    for spec, args, msg in ((ok._replace(denoise=(5, 4, 2)), (True, False, True), 'denoise must be'),
                            (ok._replace(denoise=(5, 10, 4)), (True, False, True), 'denoise must be'),
                            (ok._replace(denoise=(5, 10, 0)), (True, False, True), 'denoise must be'),
                            (ok._replace(denoise=(5, 256, 1)), (True, False, True), 'denoise must be'),
                            (ok, (True, False, False), 'reuse_frames'),
                            (ok._replace(y4m=False), (False, False, True), 'Y4M edge'),
                            (ok._replace(dedup=(7, 5, Fraction(1, 3), 4)), (True, True, True), 'dedup'),
                            (ok._replace(fields='t', deint_mode='adaptive'), (True, False, True), "deint_mode 'adaptive'")):
        with pytest.raises(ValueError, match=msg):
            spec.check(*args)


def test_runner_arguments_and_refusals():
    vr = video.VideoRunner(None)
    assert vr.denoise is None and vr.last_denoised == 0 and vr._behind(None) == 0 and vr._behind('t') == 0
    assert video.VideoRunner(None, denoise=True).denoise == (5, 10, 2) and video.VideoRunner(None, denoise=False).denoise is None
    assert video.VideoRunner(None, denoise=4).denoise == (4, 8, 2) and video.VideoRunner(None, denoise='3:9', denoise_radius=1).denoise == (3, 9, 1)
    vr = video.VideoRunner(None, 1, 2, denoise=(0, 0), denoise_radius=3, deinterlace=True)
    assert vr.denoise == (0, 0, 3) and vr._behind(None) == 3 and vr._behind('b') == 6
    assert video.VideoRunner(None, deinterlace=True, deinterlace_mode='adaptive')._behind('t') == 2
    for kw, msg in ((dict(denoise_radius=2), '--denoise-radius'), (dict(denoise=True, dedup=True), '--dedup'),
                    (dict(denoise=True, deinterlace=True, deinterlace_mode='adaptive'), '--deinterlace-mode adaptive'),
                    (dict(denoise=True, denoise_radius=4), 'radius'), (dict(denoise=True, denoise_radius=0), 'radius'),
                    (dict(denoise=(5, 4)), 'A <= B'), (dict(denoise=300), '0 .. 255'), (dict(denoise=(1, 2, 3)), 'denoise must be'),
                    (dict(denoise=2.5), 'denoise must be'), (dict(denoise='x'), 'expected A or A:B')):
        with pytest.raises(ValueError, match=msg):
            video.VideoRunner(None, **kw)
    # the counter goes the way of the others
    vr = video.VideoRunner(None, mfi=2, denoise=True)
    added = dict({name: 0 for name in video.COUNTERS}, denoised=11)
    vr._counted(types.SimpleNamespace(w=96, h=64, layout='420'), added, [], 0)
    assert vr.last_denoised == 11
    from demfi_amd.runner import WindowRunner
    import inspect
    assert 'self.denoised = 0' in inspect.getsource(WindowRunner.__init__)


def test_command_line(capsys):
    p = video.parser()
    a = p.parse_args(['in.y4m', 'out.y4m'])
    assert a.denoise is None and a.denoise_radius is None
    assert p.parse_args(['-', '-', '--denoise']).denoise == (5, 10)
    a = p.parse_args(['in.y4m', 'out.y4m', '--denoise', '3:7', '--denoise-radius', '3'])
    assert a.denoise == (3, 7) and a.denoise_radius == 3 and p.parse_args(['a', 'b', '--denoise', '4']).denoise == (4, 8)
    assert '--denoise' in p.format_help() and '--denoise-radius' in p.format_help()
    for argv, msg in ((['a.y4m', 'b.y4m', '--denoise-radius', '2'], 'give --denoise'),
                      (['a.y4m', 'b.y4m', '--denoise', '--dedup'], '--dedup'),
                      (['a.y4m', 'b.y4m', '--denoise', '--deinterlace', '--deinterlace-mode', 'adaptive'], '--deinterlace-mode bob'),
                      (['a.y4m', 'b.y4m', '--denoise', '--denoise-radius', '4'], 'radius'),
                      (['a.y4m', 'b.y4m', '--denoise', '9:3'], 'A <= B')):
        with pytest.raises(SystemExit) as ex:                             # an argument error, before a GPU or a file is touched
            video.main(argv)
        assert ex.value.code == 2 and msg in capsys.readouterr().err
    from demfi_amd import clip
    with pytest.raises(SystemExit) as ex:                                 # the folder path has no such switch
        clip.parser().parse_args(['frames', '--denoise'])
    assert ex.value.code == 2


# ---- the clip of the GPU tests ---------------------------------------------------------------------------------------------------------
def noisy_clip(n, h, w, layout, d, seed=0, fps=b'24:1'):
    """A Y4M stream that exercises the filter: in the left half of every plane a static seeded picture with independent noise of +-3
    (8-bit steps) per frame, in the right half the moving pattern of tests/test_gpu_y4m_layouts.py.  Returns (bytes, payloads as sample
    arrays, the mask of the left halves over a payload)."""
    from tests import test_gpu_y4m_layouts as Y
    data, moving, _ = Y._clip(n, h, w, layout, d, seed=seed, fps=fps)
    g = np.random.RandomState(1000 + seed)
    peak, sh = (1 << d) - 1, d - 8
    left = np.concatenate([(np.arange(c)[None, :] < c // 2).repeat(r, 0).reshape(-1) for r, c in IL.plane_shapes(h, w, layout)])
    still = g.randint(32 << sh, 224 << sh, left.size)
    pays = []
    for m in moving:
        m = np.asarray(m).reshape(-1)
        noisy = np.clip(still + (g.randint(-3, 4, left.size) << sh), 0, peak)
        pays.append(np.where(left, noisy, m).astype(m.dtype))
    head = data[:data.index(b'FRAME\n')]
    return head + b''.join(b'FRAME\n' + p.tobytes() for p in pays), pays, left


def exercised(pays, left, d, radius=DN.DEFAULT_RADIUS):
    """(share of the noisy half's samples the host filter changes, share of the moving half's it leaves alone) at the defaults."""
    outs = DN.denoise_stream_np(pays, d, *DN.DEFAULTS, radius)
    diff = np.stack([o != p for o, p in zip(outs, pays)])
    return float(diff[:, left].mean()), float(1 - diff[:, ~left].mean())


@pytest.mark.parametrize('h,w,layout,d', [(64, 96, '420', 8), (48, 80, '420', 8), (48, 80, '422', 10), (96, 160, '420', 10), (96, 160, '420', 8)])
def test_the_gpu_tests_clip_exercises_the_filter(h, w, layout, d):
    data, pays, left = noisy_clip(7, h, w, layout, d, seed=3)
    assert len(pays) == 7 and pays[0].size == y4m.payload_size(h, w, layout) and 0.4 < left.mean() <= 0.5
    rd = y4m.Reader(io.BytesIO(data), y4m.DEPTHS, y4m.LAYOUTS)
    assert (rd.header.h, rd.header.w, rd.header.depth, rd.header.layout) == (h, w, d, layout)
    changed, alone = exercised(pays, left, d)
    print('noisy half changed %.3f, moving half left alone %.3f' % (changed, alone))
    assert changed > 0.25 and alone > 0.5


# ---- residency: the edge's bookkeeping, driven as the batch loop drives it, without a GPU ----------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def demfi_payload_denoise(self, src, src_bytes, offs_host, offs_dev, n, taps, p, es, a, b, dst, dst_bytes, stream):
        self.calls.append((list((ctypes.c_int64 * ((taps + 1) * n)).from_address(offs_host)), n, taps, (a, b)))
        return 0


def _fake_ingest(nslot, radius, order, pb=36):
    e = object.__new__(Ingest)
    e.slots, e.adaptive, e.raw, e.fields, e.Pb, e.P, e.es, e.fh, e.fw, e.layout = P.FrameSlots(nslot, 2, 2, 'cpu'), False, {}, order, pb, pb, 1, 4, 6, '420'
    e.rn = types.SimpleNamespace(lib=_FakeLib(), denoised=0)
    e.yuv_in, e.clean = torch.empty((nslot, pb), dtype=torch.uint8), torch.empty((nslot, pb), dtype=torch.uint8)
    e.denoise, e.radius, e.step = (5, 10), radius, 2 if order is not None else 1
    e.dn_offs = torch.empty((2 * radius + 2) * nslot, dtype=torch.int64)
    return e


def _drive(frames, windows, batch, n_frames, radius, order=None, extra=(), monkeypatch=None):
    """The uploads and launches of a run of ``windows`` over ``frames`` in batches of ``batch``, in the order of ``ClipPipeline.run``.
    Returns the uploads (frame indices in order) and the frames denoised per batch."""
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    step = 2 if order is not None else 1
    spec = P.EdgeSpec(True, fields=order, denoise=(5, 10, radius))
    reach = spec.reach
    e = _fake_ingest(max(2 * batch + 8 + 2 * reach, 8 * batch), radius, order)   # the slot count of ``ClipPipeline``
    assert e.reach == reach == radius * step
    stream = types.SimpleNamespace(cuda_stream=0)
    it = iter(windows)
    wins = list(itertools.islice(it, batch))
    ups, denoised, finished, width = [], [], set(), 2 * radius + 2
    while wins:
        new = []
        named = set(extra).union(*wins)
        for _, idx in P.residency_order(extra, wins, e.around(named, frames.has)):
            sl, fresh = e.slots.acquire(idx, None)
            if fresh:
                frames[idx]                                               # must still be held by the host side
                ups.append(idx)
                new.append((idx, sl))
        calls0 = len(e.rn.lib.calls)
        done = e._denoise(new, stream)
        fs = [f for f, _ in done]
        assert not finished & set(fs) and fs == sorted(fs)                # a frame is denoised once
        calls = e.rn.lib.calls[calls0:]
        assert len(calls) == (1 if fs else 0) and all(c[2] == 2 * radius + 1 and c[3] == (5, 10) for c in calls)      # one launch per batch
        offs = [o for c in calls for o in c[0]]
        assert len(offs) == width * len(fs)
        for i, f in enumerate(fs):                                        # the slots of f - R step .. f + R step, -1 only beyond the stream's ends
            want = [e.slots.slot_of[g] * e.Pb if 0 <= g < n_frames else -1 for g in range(f - reach, f + reach + 1, step)]
            assert offs[width * i:width * (i + 1)] == want + [e.slots.slot_of[f] * e.Pb], (f, offs[width * i:width * (i + 1)], want)
        finished |= set(fs)
        assert named <= finished                                          # what the batch converts and runs is denoised
        denoised.append(fs)
        extra = ()
        wins = list(itertools.islice(it, batch))
    assert e.rn.denoised == len(finished)
    return ups, denoised


def _stream(n, interlaced=None, h=4, w=6):
    p = y4m.payload_size(h, w)
    return b'YUV4MPEG2 W%d H%d F25:1 I%s\n' % (w, h, interlaced or b'p') + b''.join(b'FRAME\n' + bytes([i + 1]) * p for i in range(n))


class _Pipe(io.BytesIO):
    def seek(self, *a):
        raise AssertionError('a pipe does not seek')

    def tell(self):
        raise AssertionError('a pipe does not tell')


@pytest.mark.parametrize('batch', [1, 2, 4])
@pytest.mark.parametrize('radius', [1, 2, 3])
@pytest.mark.parametrize('full', [False, True], ids=['reference', 'full-length'])
def test_residency_of_a_progressive_pipe(batch, radius, full, monkeypatch):
    n = 12
    fr = y4m.Frames(y4m.Reader(_Pipe(_stream(n))), pinned=False, full_length=full, behind=radius)
    ups, denoised = _drive(fr, fr.windows(), batch, n, radius, monkeypatch=monkeypatch)
    assert sorted(ups) == list(range(n)) and len(set(ups)) == len(ups)   # every frame uploaded once; the pipe was read in order, never seeked
    assert sorted(f for fs in denoised for f in fs) == list(range(n))
    # payload tensors held at once: the batch's + 5 of a run without the switch, the R frames kept behind and the R read ahead
    assert fr.peak <= batch + 5 + 2 * radius


@pytest.mark.parametrize('batch', [1, 4])
@pytest.mark.parametrize('radius', [1, 3])
def test_residency_of_a_bobbed_stream(batch, radius, monkeypatch):
    n = 9                                                                # payloads: 18 fields, neighbours two fields apart
    fr = y4m.Frames(y4m.Reader(_Pipe(_stream(n, b't')), fields=True), pinned=False, fields=2, behind=2 * radius)
    ups, denoised = _drive(fr, fr.windows(), batch, 2 * n, radius, order='t', monkeypatch=monkeypatch)
    assert sorted(ups) == list(range(2 * n)) and len(set(ups)) == len(ups) and sorted(f for fs in denoised for f in fs) == list(range(2 * n))
    assert fr.peak <= (batch + 5 + 4 * radius) // 2 + 1


@pytest.mark.parametrize('lo,count,cuts', [(5, 4, False), (5, 4, True), (0, 5, False), (9, 2, True)])
def test_residency_of_a_block_of_a_file(lo, count, cuts, tmp_path, monkeypatch):
    """A rank's block of windows lo .. lo+count-1 of 14 frames: the R frames before its first frame and the R after its last are uploaded
    and never denoised; with scene cuts the block also denoises the frame before its first window."""
    n, radius = 14, 2
    src = tmp_path / 'in.y4m'
    src.write_bytes(_stream(n))
    with open(src, 'rb') as f:
        hdr, _, offs = y4m.scan(f)
        first = max(lo - 1, 0) if cuts else lo
        fr = y4m.Frames.from_file(f, offs, first, lo + count + 3, hdr.payload, pinned=False, behind=radius)
        wins = [(k + 1, k + 2, k, k + 3) for k in range(lo, lo + count)]
        ups, denoised = _drive(fr, wins, 2, n, radius, extra=(first,) if cuts and first < lo else (), monkeypatch=monkeypatch)
    assert sorted(f for fs in denoised for f in fs) == list(range(first, lo + count + 3))
    assert sorted(ups) == list(range(max(first - radius, 0), min(lo + count + 3 + radius, n))) and len(set(ups)) == len(ups)


def test_a_frame_that_left_the_ring_is_not_taken_for_an_absent_one(monkeypatch):
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    e = _fake_ingest(16, 2, None)
    e.around({3}, lambda g: g < 10)
    new = [(g, e.slots.acquire(g, None)[0]) for g in (2, 3, 4, 5)]        # frame 1 exists and was never uploaded
    with pytest.raises(RuntimeError, match='frame 3 needs frame 1'):
        e._denoise(new, types.SimpleNamespace(cuda_stream=0))
    assert not e.rn.lib.calls


def test_without_the_switch_the_ingest_is_what_it_was():
    e = object.__new__(Ingest)
    e.adaptive, e.yuv_in = False, torch.empty((4, 8), dtype=torch.uint8)
    assert e.denoise is None and e.clean is None and e.payloads is e.yuv_in and e.reach == 0 and e.around({1, 2}, None) == []
    assert P.EdgeSpec(True, fields='t', deint_mode='adaptive').reach == 2 and P.EdgeSpec(True, fields='t').reach == 0
