"""Inverse telecine (``--ivtc``) on the host: the numpy definitions of ``demfi_amd.telecine`` against direct per-sample loops, the
matching and decimation policy, the stage ``FilmFrames`` with the numpy scorer over telecined clips of every field order, phase,
layout and depth, the header keyword and every refusal of ``VideoRunner``.  No kernel is launched here."""
import io
from fractions import Fraction

import numpy as np
import pytest

from demfi_amd import deint as I
from demfi_amd import telecine as TC
from demfi_amd import video, y4m


# ---- clips -------------------------------------------------------------------------------------------------------------------
def _film(n, h, w, layout='420', depth=8, speed=3, noise=0, seed=0):
    """n progressive payloads (uint8 arrays of their bytes) of vertical bars, 4 samples wide, that move ``speed`` samples per
    frame, with a gentle vertical ramp (rows differ by at most 3 s, s = 2^(depth-8)) and ``noise`` * s of per-frame noise: a frame
    has no combed sample of its own (3 s + 2 * 2 s < T = 9 s), a weave of two different frames is combed wherever the bars differ."""
    rng = np.random.default_rng(seed)
    s = 1 << (depth - 8)
    ch, cw = y4m.chroma_shape(h, w, layout)
    bars = [np.repeat(rng.integers(30, 220, (wd + speed * n + 7) // 4 + 1), 4) for wd in (w, cw, cw)]
    out = []
    for i in range(n):
        planes = []
        for (rows, cols), b in zip(((h, w), (ch, cw), (ch, cw)), bars):
            if rows == 0:
                continue
            p = b[speed * i:speed * i + cols][None, :] + (np.arange(rows) % 4)[:, None]
            if noise:
                p = p + rng.integers(-noise, noise + 1, (rows, cols))
            planes.append((p * s).reshape(-1))
        a = np.concatenate(planes).astype(np.uint8 if depth == 8 else '<u2')
        out.append(a.view(np.uint8).copy())
    return out


def _telecined(film, h, w, layout, depth, order, phase):
    return [t.view(np.uint8) for t in TC.pulldown_payloads_np(film, h, w, depth, layout, order, phase)]


def _same(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a.tobytes() != b.tobytes()]
    assert not bad, 'frames differ: %s' % bad


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def _comb_loop(plane, t):
    """(max_block, total) by the words of the module's docstring, sample by sample."""
    h, w = plane.shape
    p = plane.astype(int).tolist()
    blocks = {}
    for y in range(2, h - 2):
        for x in range(w):
            d1, d2 = p[y][x] - p[y - 1][x], p[y][x] - p[y + 1][x]
            if ((d1 > t and d2 > t) or (d1 < -t and d2 < -t)) and \
                    abs(p[y - 2][x] + 4 * p[y][x] + p[y + 2][x] - 3 * (p[y - 1][x] + p[y + 1][x])) > 6 * t:
                blocks[(y // 16, x // 16)] = blocks.get((y // 16, x // 16), 0) + 1
    return max(blocks.values(), default=0), sum(blocks.values())


@pytest.mark.parametrize('h,w', [(5, 2), (6, 7), (7, 5), (18, 35), (33, 17), (16, 16)])
def test_comb_counts_equal_a_per_sample_loop(h, w):
    rng = np.random.default_rng(h * 100 + w)
    top = rng.integers(0, 256, h * w + 5).astype(np.uint8)               # a payload: luma first, then something else
    bot = rng.integers(0, 256, h * w + 5).astype(np.uint8)
    woven = top[:h * w].reshape(h, w).copy()
    woven[1::2] = bot[:h * w].reshape(h, w)[1::2]
    assert (TC.woven_luma_np(top, bot, h, w) == woven).all()
    some = 0
    for cthresh in (0, 9, 60, 255):
        exp = _comb_loop(woven, cthresh)
        assert TC.comb_counts_np(top, bot, h, w, 8, cthresh) == exp
        some += exp[1]
        top10, bot10 = (top.astype('<u2') * 4).view(np.uint8), (bot.astype('<u2') * 4).view(np.uint8)
        assert TC.comb_counts_np(top10, bot10, h, w, 10, cthresh) == exp     # the same picture at 10 bits: T scales with it
    assert some > 0 and TC.comb_counts_np(top, bot, h, w, 8, 255) == (0, 0)


def test_edge_rows_never_comb_and_short_planes_score_nothing():
    h, w = 12, 20
    a = np.where(np.arange(h)[:, None] % 2 == 0, 200, 20) * np.ones((1, w), int)       # every row differs from both neighbours by 180
    m = TC.combed_np(a, 9)
    assert m[2:h - 2].all() and not m[:2].any() and not m[h - 2:].any()
    top, bot = np.full(h * w, 200, np.uint8), np.full(h * w, 20, np.uint8)
    assert TC.comb_counts_np(top, bot, h, w) == (16 * 8, 20 * 8) and TC.comb_counts_np(top, top, h, w) == (0, 0)
    for hh in (2, 3, 4):
        assert TC.comb_counts_np(top, bot, hh, w) == (0, 0)
    assert TC.comb_counts_np(top, bot, 5, w) == (16, 20)                   # one row, two blocks (16 and 4 columns)
    # a spike in one direction only is not combing: a ramp
    ramp = (np.arange(h)[:, None] * 20 * np.ones((1, w), int)).astype(np.uint8)
    assert not TC.combed_np(ramp, 9).any()


def test_partial_blocks():
    h, w = 35, 21                                                            # blocks of 16 and 5 columns, 16, 16 and 3 rows
    top, bot = np.full(h * w, 200, np.uint8), np.full(h * w, 20, np.uint8)
    sums = TC.block_sums_np(TC.combed_np(TC.woven_luma_np(top, bot, h, w), 9))
    assert sums.tolist() == [[14 * 16, 14 * 5], [16 * 16, 16 * 5], [16, 5]]
    assert TC.comb_counts_np(top, bot, h, w) == (256, 31 * 21)


def test_woven_sad():
    h, w = 7, 9
    rng = np.random.default_rng(3)
    a, b, c, d = (rng.integers(0, 256, h * w).astype(np.uint8) for _ in range(4))
    wa, wb = a.reshape(h, w).astype(int), c.reshape(h, w).astype(int)
    wa[1::2], wb[1::2] = b.reshape(h, w)[1::2], d.reshape(h, w)[1::2]
    assert TC.woven_sad_np(a, b, c, d, h, w) == int(np.abs(wa - wb).sum()) > 0
    assert TC.woven_sad_np(a, b, a, b, h, w) == 0


# ---- the policy ---------------------------------------------------------------------------------------------------------------
def test_ties_go_c_then_p_then_n():
    m = TC.Matcher()
    assert m.push(0, [(3, 9), None, (3, 9)]) == 0
    assert m.push(1, [(3, 9), (3, 9), (3, 9)]) == 0
    assert m.push(2, [(3, 9), (3, 8), (3, 8)]) == -1
    assert m.push(3, [(3, 9), (3, 9), (2, 99)]) == 1
    assert m.push(4, [(81, 90), (81, 90), None]) == 0
    assert m.matches == list('ccpnc') and m.combed == [4]                   # max_block > combpel = 80
    assert TC.Matcher(combpel=81).push(0, [(81, 90), None, None]) == 0
    with pytest.raises(RuntimeError):
        m.push(6, [(0, 0), None, None])
    with pytest.raises(RuntimeError):
        m.push(5, [None, (0, 0), None])


def test_decimator_drops_the_closest_repeat_of_every_full_cycle():
    d = TC.Decimator()
    out = [d.push(i, m) for i, m in enumerate([None, 5, 7, 5, 9, 4, 4, 8, 1])]
    assert out == [[], [], [], [], [0, 2, 3, 4], [], [], [], []] and d.dropped == [1]       # ties: the lowest index; frame 0 has no metric
    assert d.push(9, 1) == [5, 6, 7, 9] and d.dropped == [1, 8]
    assert d.push(10, 0) == [] and d.finish() == [10] and d.finish() == [] and d.dropped == [1, 8]
    with pytest.raises(RuntimeError):
        d.push(11)
    with pytest.raises(RuntimeError):
        TC.Decimator().push(0, 3)


@pytest.mark.parametrize('n', range(13))
def test_n_payloads_give_n_minus_n_over_5_frames(n):
    h, w = 16, 16
    pays = _film(n, h, w, speed=3, seed=n)
    out, film = TC.film_of(pays, h, w)
    assert len(out) == TC.n_film_frames(n) == n - n // 5 and len(film.dropped) == n // 5
    assert sum(film.matches.values()) == n and film.combed == []
    assert all(5 * c <= d < 5 * c + 5 and d > 0 for c, d in enumerate(film.dropped))


def test_a_progressive_clip_comes_back_byte_for_byte():
    h, w = 32, 48
    pays = _film(10, h, w, speed=6, noise=2, seed=1)
    out, film = TC.film_of(pays, h, w)
    assert film.matches == {'c': 10, 'p': 0, 'n': 0} and film.combed == [] and len(film.dropped) == 2
    _same(out, [p for i, p in enumerate(pays) if i not in film.dropped])
    still = [pays[0]] * 7                                                    # a still: everything ties, c everywhere, the first ties drop
    out, film = TC.film_of(still, h, w)
    assert film.matches['c'] == 7 and film.dropped == [1] and all(o.tobytes() == pays[0].tobytes() for o in out) and len(out) == 6


@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('layout', ['420', '422', '444', 'mono'])
@pytest.mark.parametrize('phase', [0, 1])
@pytest.mark.parametrize('order', ['t', 'b'])
def test_pulldown_is_undone_exactly(order, phase, layout, depth):
    h, w = 32, 48
    film = _film(12, h, w, layout, depth, speed=3, noise=2, seed=7)
    tele = _telecined(film, h, w, layout, depth, order, phase)
    assert len(tele) == 15 and sum(a.tobytes() != b.tobytes() for a, b in zip(tele, [film[0]] * 15)) >= 14
    mixed = [j for j, t in enumerate(tele) if all(t.tobytes() != f.tobytes() for f in film)]
    assert len(mixed) == 6                                                   # two payloads in five weave two film frames
    out, st = TC.film_of(tele, h, w, depth, layout)
    _same(out, film)
    assert st.combed == [] and len(st.dropped) == 3 and st.matches['c'] == 9 and st.matches['p' if order == 't' else 'n'] == 6


@pytest.mark.parametrize('h,w,speed,noise', [(16, 16, 3, 0), (16, 16, 6, 2), (64, 96, 3, 2), (64, 96, 6, 0)])
def test_other_sizes_and_speeds(h, w, speed, noise):
    film = _film(12, h, w, speed=speed, noise=noise, seed=h + speed)
    for order in 'tb':
        for phase in (0, 1):
            _same(TC.film_of(_telecined(film, h, w, '420', 8, order, phase), h, w)[0], film)


def test_pulldown_np_field_pattern():
    frames = [[np.full((4, 2), i)] for i in range(4)]
    def tb(out):
        return [(int(f[0][0, 0]), int(f[0][1, 0])) for f in out]
    assert tb(TC.pulldown_np(frames, 't', 0)) == [(0, 0), (1, 1), (1, 2), (2, 3), (3, 3)]
    assert tb(TC.pulldown_np(frames, 'b', 0)) == [(0, 0), (1, 1), (2, 1), (3, 2), (3, 3)]
    assert tb(TC.pulldown_np(frames, 't', 1)) == [(0, 0), (0, 1), (1, 2), (2, 2), (3, 3)]
    assert tb(TC.pulldown_np(frames[:3], 't', 0)) == [(0, 0), (1, 1), (1, 2), (2, 2)]     # a field left over: its own frame's other field
    with pytest.raises(ValueError):
        TC.pulldown_np(frames, 'x', 0)
    with pytest.raises(ValueError):
        TC.pulldown_np(frames, 't', 2)


@pytest.mark.parametrize('mode', ['bob', 'keep'])
def test_a_clip_that_starts_mid_cycle_reports_a_combed_frame(mode):
    h, w = 32, 48
    film = _film(12, h, w, '422', 8, speed=3, seed=2)
    tele = _telecined(film, h, w, '422', 8, 't', 0)[2:]                       # starts at the payload that weaves film frames 1 and 2
    out, st = TC.film_of(tele, h, w, 8, '422', combed=mode)
    assert st.combed == [0] and st.matcher.combed == [0] and len(out) == 13 - 2
    exp0 = I.bob_payload_np(tele[0], h, w, 8, '422', 0) if mode == 'bob' else tele[0]
    assert out[0].tobytes() == exp0.tobytes() and out[0].tobytes() != film[1].tobytes()
    # every frame behind the first is a clean film frame again, in order; which ones the fixed cycles of five drop or repeat once
    # the cadence is out of step with them is the decimator's policy (13 payloads: two full cycles, two dropped)
    index = {f.tobytes(): i for i, f in enumerate(film)}
    later = [index[o.tobytes()] for o in out[1:]]
    assert later == sorted(later) and later[0] in (2, 3) and later[-1] == 11 and set(later) >= set(range(2, 12)) - {st.dropped[0] + 1}
    assert st.dropped[0] in (1, 2, 3, 4) and 5 <= st.dropped[1] <= 9
    assert TC.film_of(tele, h, w, 8, '422', combpel=256)[1].combed == []     # a block has 256 samples


def test_matcher_and_decimator_fed_one_payload_at_a_time():
    h, w = 32, 48
    film = _film(8, h, w, speed=3, seed=4)
    tele = _telecined(film, h, w, '420', 8, 'b', 1)
    n = len(tele)
    whole = TC.film_of(tele, h, w)[1]
    m, d, bot, kept = TC.Matcher(), TC.Decimator(), {}, []
    for p in range(n):                                                        # payload p is scored once p + 1 is there (or the end is)
        cands = (p, p - 1 if p else None, p + 1 if p + 1 < n else None)
        bot[p] = p + m.push(p, [None if b is None else TC.comb_counts_np(tele[p], tele[b], h, w) for b in cands])
        kept += d.push(p, None if p == 0 else TC.woven_sad_np(tele[p], tele[bot[p]], tele[p - 1], tele[bot[p - 1]], h, w))
    kept += d.finish()
    assert m.matches == whole.matcher.matches and d.dropped == whole.dropped and len(kept) == n - n // 5
    _same([TC.weave_np(tele[p], tele[bot[p]], h, w, 8, '420').view(np.uint8) for p in kept], film)


def test_film_frames_are_asked_for_in_order():
    h, w = 16, 16
    pays = _film(3, h, w)
    hdr = y4m.Header(w, h, 30)
    film = TC.FilmFrames(lambda j, buf: j < 3 and (buf.__setitem__(slice(None), pays[j]) or True), hdr, TC.NumpyScorer(h, w))
    buf = np.empty(hdr.payload, np.uint8)
    with pytest.raises(RuntimeError, match='due'):
        film(1, buf)
    assert [film(i, buf) for i in range(4)] == [True, True, True, False] and not film(3, buf)


# ---- headers --------------------------------------------------------------------------------------------------------------------
def test_film_header():
    hdr = y4m.parse_header(b'YUV4MPEG2 W720 H480 F30000:1001 Im A10:11 C420mpeg2 XCOLORRANGE=LIMITED XFOO=1', telecine=True)
    f = TC.film_header(hdr)
    assert (f.fps, f.interlace, f.w, f.h, f.chroma, f.aspect, f.xtags, f.color_range) == (Fraction(24000, 1001), 'p', 720, 480, '420mpeg2',
                                                                                         '10:11', ['FOO=1'], 'LIMITED')
    assert f.encode() == hdr.encode().replace(b'F30000:1001', b'F24000:1001').replace(b' Im', b' Ip')
    assert TC.film_header(y4m.Header(8, 8, 25)).fps == 20


def test_the_header_keyword_admits_every_field_flag():
    line = b'YUV4MPEG2 W720 H480 F30000:1001 I%s'
    for tag in (b't', b'b', b'm', b'p', b'?'):
        assert y4m.parse_header(line % tag, telecine=True).interlace == tag.decode()
        assert y4m.Reader(io.BytesIO(line % tag + b'\n'), telecine=True).header.interlace == tag.decode()
    with pytest.raises(y4m.Y4MError):
        y4m.parse_header(line % b'x', telecine=True)
    for tag in (b't', b'b', b'm'):                                            # off by default, and the refusals keep their words
        with pytest.raises(y4m.Y4MError, match='--deinterlace'):
            y4m.parse_header(line % tag)
    with pytest.raises(y4m.Y4MError, match='--ivtc'):
        y4m.parse_header(line % b'm', fields=True)


def test_scan_takes_the_keyword(tmp_path):
    p = y4m.payload_size(4, 6)
    path = tmp_path / 'm.y4m'
    path.write_bytes(b'YUV4MPEG2 W6 H4 F30:1 Im\n' + b''.join(b'FRAME\n' + bytes([i]) * p for i in range(3)))
    with open(path, 'rb') as f:
        with pytest.raises(y4m.Y4MError):
            y4m.scan(f, fields=True)
        hdr, _, offs = y4m.scan(f, telecine=True)
        assert hdr.interlace == 'm' and len(offs) == 3
        fetch, buf = y4m.file_fetch(f, offs), np.empty(p, np.uint8)
        assert fetch(2, buf) and (buf == 2).all()
        with pytest.raises(IndexError):                                       # the caller bounds it, as ``Frames.from_file`` does with ``stop``
            fetch(3, buf)


# ---- the runner's checks that need no GPU --------------------------------------------------------------------------------------
def _stream(n=6, tag=b'm', fps=b'30000:1001'):
    p = y4m.payload_size(16, 16)
    return b'YUV4MPEG2 W16 H16 F%s I%s\n' % (fps, tag) + b''.join(b'FRAME\n' + bytes(p) for _ in range(n))


def test_runner_arguments_rates_and_refusals(tmp_path):
    vr = video.VideoRunner(None)
    assert vr.ivtc is False and vr.last_matches == {'c': 0, 'p': 0, 'n': 0} and vr.last_dropped == [] and vr.last_combed == []
    with pytest.raises(y4m.Y4MError, match='--ivtc'):                        # without the switch Im stays refused, and the hint names it
        vr.run_stream(io.BytesIO(_stream()), io.BytesIO())
    vr = video.VideoRunner(None, 1, fps=Fraction(60000, 1001), ivtc=True)
    fh, order, per = vr._progressive(y4m.parse_header(_stream(0).rstrip(b'\n'), telecine=True))
    assert (fh.fps, fh.interlace, order, per, vr.last_fields) == (Fraction(24000, 1001), 'p', None, 1, None)
    assert vr._ratio(fh) == Fraction(5, 2) and vr._out_header(fh).fps == Fraction(60000, 1001)
    assert video.VideoRunner(None, 1, fps=Fraction(24000, 1001), ivtc=True)._progressive(fh)[0].fps == Fraction(96000, 5005)
    with pytest.raises(ValueError, match='--deinterlace'):
        video.VideoRunner(None, ivtc=True, deinterlace=True)
    for bad in (dict(ivtc_cthresh=-1), dict(ivtc_cthresh=256), dict(ivtc_cthresh=9.5), dict(ivtc_combpel=-1), dict(ivtc_combpel=257),
                dict(ivtc_combed='blend'), dict(ivtc_cthresh=True)):
        with pytest.raises(ValueError, match='ivtc'):
            video.VideoRunner(None, ivtc=True, **bad)
        with pytest.raises(ValueError, match='ivtc'):
            video.VideoRunner(None, **bad)                                    # bad values are refused whether the switch is on or not
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(_stream())
    for fps in (Fraction(24000, 1001) - Fraction(1, 1000), Fraction(20)):   # below the film rate 4F/5
        vr = video.VideoRunner(None, 1, fps=fps, ivtc=True)
        with pytest.raises(ValueError, match='film rate 24000/1001'):
            vr.run_stream(io.BytesIO(_stream()), io.BytesIO())
        with pytest.raises(ValueError, match='film rate 24000/1001'):
            vr.run_file(str(src), str(dst))
        assert vr._runners == {} and not dst.exists()
    vr = video.VideoRunner(None, 1, 2, ivtc=True)
    with pytest.raises(ValueError, match='one rank'):
        vr.run_file(str(src), str(dst), world=2, rank=0)
    assert vr._runners == {} and not dst.exists()


def test_command_line_has_the_switches():
    p = video.parser()
    a = p.parse_args(['in.y4m', 'out.y4m'])
    assert (a.ivtc, a.ivtc_cthresh, a.ivtc_combpel, a.ivtc_combed) == (False, 9, 80, 'bob')
    a = p.parse_args(['-', '-', '--ivtc', '--fps', '60000/1001', '--ivtc-cthresh', '12', '--ivtc-combpel', '100', '--ivtc-combed', 'keep'])
    assert (a.ivtc, a.fps, a.ivtc_cthresh, a.ivtc_combpel, a.ivtc_combed) == (True, Fraction(60000, 1001), 12, 100, 'keep')
    with pytest.raises(SystemExit):
        p.parse_args(['-', '-', '--ivtc-combed', 'blend'])
    with pytest.raises(SystemExit):
        video.main(['-', '-', '--ivtc', '--deinterlace'])
