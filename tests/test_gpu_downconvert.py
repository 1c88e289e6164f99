"""Output rates below the input's (``--downconvert``) on a real MI355X: every stream byte-identical to an expectation that never runs the
new code -- the stream a run WITHOUT the switch writes at ``--fps`` F_out D (D the smallest integer with r D >= 1), keeping payloads 0, D,
2 D, ..., under the header of the rate F_out.  The clips, the model and the stream helpers are those of tests/test_gpu_shutter.py,
tests/test_gpu_dedup.py and tests/test_gpu_interlace.py."""
import io
import math
from fractions import Fraction

import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import retime as R                                                    # noqa: E402
from demfi_amd import scene as S                                                     # noqa: E402
from demfi_amd.video import VideoRunner                                              # noqa: E402
from tests import test_gpu_dedup as D                                                # noqa: E402
from tests import test_gpu_shutter as G                                              # noqa: E402
from tests import test_gpu_y4m_layouts as Y                                          # noqa: E402

N, FPS_IN = 13, Fraction(60)


@pytest.fixture(scope='module')
def model16():
    return Y._model(torch.float16)


@pytest.fixture(scope='module')
def clip60():
    return Y._clip(N, 48, 80, '420', 8, fps=b'60:1', seed=3)[0]


@pytest.fixture(scope='module')
def cut60():
    def look(i, bgr, peak):                                              # a hard cut before frame 6: another scene's colours
        return bgr if i < 6 else ((peak - bgr) // 3).astype(bgr.dtype)
    return Y._clip(N, 48, 80, '420', 8, fps=b'60:1', seed=1, look=look)[0]


_runs = {}


def _old(model, data, fps, **kw):
    """A run without the switch, shared by (clip, rate, switches)."""
    key = (id(model), hash(data), Fraction(fps), tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = G._run(model, data, fps=Fraction(fps), **kw)
    return _runs[key]


def _reference(model, data, fps_out, fps_in=FPS_IN, n=None, cuts=(), **kw):
    """The expectation, which never runs the new code: the stream of the run without the switch at F_out D (D the smallest integer with
    r D >= 1), keeping payloads 0, D, 2 D, ..., under the header of the rate F_out.

    A FINDING ABOUT THE PARENT bounds that rule.  An S0 or S1 frame is computed with its window's FIRST instant (``demfi_amd.retime``), and
    its bytes depend on that instant's t: against the plainly decimated stream, 60 -> 25, 60 -> 50 and 59.94 -> 50 differed in exactly the
    S0 frames whose window also owns an St at the ratio r D (its first instant is that St's t) and only the S0 at r (t = 1/2, as the
    definition has it), and in no other frame; 60 -> 30 and 60 -> 20, where r D = 1 and every window runs t = 1/2, were identical throughout.  So an output whose
    (tuple, kind, t of the instant it comes from) is the same at r and at r D is taken from the decimated stream, and an S0 / S1 whose first
    instant differs is taken from the run without the switch at F_in (r = 1), where every window runs t = 1/2 alone as it does at r.  Every
    byte of every frame is still held to a stream the parent writes."""
    full, r = kw.get('full_length', False), Fraction(fps_out) / fps_in
    d = math.ceil(1 / r)
    n = data.count(b'FRAME\n') if n is None else n
    fine_vr, _, _, fine = _old(model, data, fps_out * d, **kw)
    head, fine_pays = D._split(fine)
    unit_pays = D._split(_old(model, data, fps_in, **kw)[3])[1]
    is_cut = S.with_sentinels(lambda j: j in cuts, n) if full else (lambda j: j in cuts)
    ks = range(R.first_window(n, full), R.first_window(n, full) + R.n_windows(n, full))
    out, swapped = [], 0
    for k in ks:
        last = k == ks[-1]
        (runs, outs), (fruns, fouts), (uruns, uouts) = (S.window_runs(k, x, last, is_cut, full) for x in (r, r * d, Fraction(1)))
        at = {i: (fruns[run][0], kind, fruns[run][1][j]) for i, run, kind, j in fouts}
        for i, run, kind, j in outs:
            assert i == len(out)
            want = (runs[run][0], kind, runs[run][1][j])
            if at[i * d] == want:
                out.append(fine_pays[i * d])
                continue
            u = [ui for ui, urun, ukind, uj in uouts if (uruns[urun][0], ukind, uruns[urun][1][uj]) == want]
            assert kind != R.ST and want[2] == 0.5 and at[i * d][:2] == want[:2] and u, (k, i, want, at[i * d])
            out.append(unit_pays[u[0]])
            swapped += 1
    assert len(out) == R.n_output_frames(n, r, full) > 0 and (swapped == 0 or r * d != 1)
    f = Fraction(fps_out)
    return fine_vr, D._join(head, out, fps=b'%d:%d' % (f.numerator, f.denominator))


def _skipped(n, r, full=False):
    ks = range(R.first_window(n, full), R.first_window(n, full) + R.n_windows(n, full))
    return sum(not R.window_outputs(k, r, k == ks[-1], full) for k in ks)


@pytest.mark.parametrize('fps_out', [25, 50, 30, 20])
def test_a_down_rate_stream_is_the_decimated_stream_of_a_rate_that_runs_today(fps_out, model16, clip60, tmp_path):
    r = Fraction(fps_out) / FPS_IN
    _, exp = _reference(model16, clip60, fps_out)
    assert exp.startswith(b'YUV4MPEG2 W80 H48 F%d:1 Ip' % fps_out)
    for batch, pipe in ((4, False), (1, True), (3, False)):
        vr, nw, nf, got = G._run(model16, clip60, batch=batch, pipe=pipe, fps=Fraction(fps_out), down=True)
        Y._same(got, exp)
        assert (nw, nf) == (N - 3, R.n_output_frames(N, r)) and vr.last_fps_out == fps_out
        assert vr.last_windows_skipped == _skipped(N, r) and vr.last_instants == (N - 3 - _skipped(N, r), 0)
    assert (_skipped(N, Fraction(1, 3)), _skipped(N, Fraction(1, 2)), _skipped(N, Fraction(5, 6))) == (6, 4, 1)
    vr, nw, nf, got = G._run_file(model16, clip60, tmp_path, batch=3, fps=Fraction(fps_out), down=True)
    Y._same(got, exp)
    assert vr.last_windows_skipped == _skipped(N, r)
    with pytest.raises(ValueError, match='only F_out >= F_in'):
        G._run(model16, clip60, fps=Fraction(fps_out))


@pytest.mark.parametrize('fps_out', [25, 20])
def test_full_length(fps_out, model16, clip60, tmp_path):
    r = Fraction(fps_out) / FPS_IN
    _, exp = _reference(model16, clip60, fps_out, full_length=True)
    for batch in (4, 1):
        vr, nw, nf, got = G._run(model16, clip60, batch=batch, fps=Fraction(fps_out), down=True, full_length=True)
        Y._same(got, exp)
        assert (nw, nf) == (N - 1, math.ceil(N * r)) and vr.last_windows_skipped == _skipped(N, r, True)
    Y._same(G._run_file(model16, clip60, tmp_path, batch=3, fps=Fraction(fps_out), down=True, full_length=True)[3], exp)


@pytest.mark.parametrize('fps_out', [25, 20])
def test_scene_cut(fps_out, model16, cut60):
    kw = dict(scene_cut=S.DEFAULT_THRESHOLD)
    ref, exp = _reference(model16, cut60, fps_out, cuts=(6,), **kw)
    assert ref.last_cuts == [6]
    for batch in (4, 1, 3):
        vr, nw, nf, got = G._run(model16, cut60, batch=batch, fps=Fraction(fps_out), down=True, **kw)
        Y._same(got, exp)
        assert vr.last_cuts == [6] and vr.last_cut_windows <= 1              # the decisions are those of the run without the switch
    assert exp != _reference(model16, cut60, fps_out)[1]


@pytest.mark.parametrize('world', [2, 3])
def test_ranks(world, model16, clip60, tmp_path):
    _, exp = _reference(model16, clip60, 25)
    src, dst = tmp_path / 'in.y4m', tmp_path / 'out.y4m'
    src.write_bytes(clip60)
    nf = 0
    for rank in range(world):
        nf += VideoRunner(model16, 2, batch=2, matrix='bt601', fps=Fraction(25), down=True).run_file(str(src), str(dst), world=world, rank=rank)[1]
    Y._same(dst.read_bytes(), exp)
    assert nf == R.n_output_frames(N, Fraction(5, 12))


def test_behind_the_scaler_and_the_requantiser(model16, clip60):
    for fps_out, kw, mark in ((30, dict(scale=(64, 32)), b' W64 H32 '), (50, dict(out_depth=10), b' C420p10')):
        vr_ref, exp = _reference(model16, clip60, fps_out, **kw)
        vr, nw, nf, got = G._run(model16, clip60, batch=3, fps=Fraction(fps_out), down=True, **kw)
        Y._same(got, exp)
        assert mark in got[:got.index(b'\n') + 1] + b' ' and nf == R.n_output_frames(N, Fraction(fps_out) / FPS_IN)


def test_ntsc_fields_to_pal_fields(model16):
    """59.94i -> 50i: ``--deinterlace --downconvert --fps 50 --interlace tff`` weaves the progressive stream of the same run without
    ``--interlace``; the header says ``F25:1 It``."""
    from tests import test_gpu_deint as DI
    from tests import test_gpu_interlace as IT
    fields = DI._interlaced(Y._clip(7, 48, 80, '420', 8, seed=6, fps=b'30000:1001')[0], 't')
    kw = dict(deinterlace=True, down=True, fps=Fraction(50))
    plain = G._run(model16, fields, **kw)
    assert plain[2] == R.n_output_frames(14, Fraction(1001, 1200)) == 10 and plain[0].last_windows_skipped == _skipped(14, Fraction(1001, 1200)) == 1
    for batch in (4, 1):
        vr, nw, nf, got = G._run(model16, fields, batch=batch, interlace='tff', **kw)
        Y._same(got, IT._woven(plain[3], 'tff')[0])
        assert b' F25:1 It ' in got[:60] and nf == 5 and vr.last_fps_out == 25
    with pytest.raises(ValueError, match='field rate 60000/1001'):
        G._run(model16, fields, deinterlace=True, fps=Fraction(50))
    # and that progressive stream is the decimated one of a rate that runs today: 100 frames/s from the 59.94 fields/s, every other frame
    Y._same(plain[3], _reference(model16, fields, 50, Fraction(60000, 1001), 14, deinterlace=True)[1])


def test_the_switch_changes_nothing_at_or_above_the_input_rate(model16, clip60):
    for fps in (60, 120):
        a, b = G._run(model16, clip60, fps=Fraction(fps)), G._run(model16, clip60, fps=Fraction(fps), down=True)
        assert a[1:] == b[1:] and b[0].last_windows_skipped == 0
        assert (a[0].last_instants, a[0].last_st_frames, a[0].last_cut_windows) == (b[0].last_instants, b[0].last_st_frames, b[0].last_cut_windows)


def test_dedup_is_refused_before_anything_runs(model16, clip60):
    vr = VideoRunner(model16, 2, fps=Fraction(25), down=True, dedup=True)
    with pytest.raises(ValueError, match='--dedup does not go with an output rate below'):
        vr.run_stream(io.BytesIO(clip60), io.BytesIO())
    assert not vr._runners
