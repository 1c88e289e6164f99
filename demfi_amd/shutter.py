"""Synthesized motion blur of the Y4M video path (``python -m demfi_amd.video --shutter ANGLE [--shutter-samples S]``): the network's
frames are sharp, as if shot with a near-zero shutter angle; a written frame becomes the average of S finer frames spread over its
exposure instead.  Pure Python / numpy; the one module that knows the definition.

The exposure is e = ANGLE / 360 of the written stream's frame period (0 < ANGLE <= 360: 180 degrees is the film look).  With S samples
per written frame the sub-frames are e / S of a frame period apart, so the fine stream they come from runs D = S / e times as fast as
the written one; D must be an integer (180 degrees with S = 4: D = 8; 360 with S = 4: D = 4; 90 with S = 4: D = 16).  With the stream's
ratio r = F_out / F_in (M for ``--mfi M``; below 1 with ``--downconvert``) the fine stream is the ordinary timeline of
``demfi_amd.retime`` at the ratio R = r D, on either timeline; R may not exceed ``retime.MAX_RATIO``, and with r < 1 it may lie below D
and below 1, so that a window owns fewer than D fine frames or none.

Written ("coarse") frame c exposes from its own time tau_c on: its samples are the fine frames g = c D + j, j = 0 .. S-1.  The written
stream has the header, the length (``retime.n_output_frames(n, r, full)``) and the timing of a run without the switch.  Fine frame c D
always exists (non-full: (N_out - 1) D = floor((n-3) r) D <= floor((n-3) r D); full: (ceil(n r) - 1) D < n r D); later samples of the
last groups may not.  A group keeps a sample when it exists and lies in the same scene as sample 0: with scene cuts
(``demfi_amd.scene``) the scene changes inside a cut window only, between the outputs of its left run and those of its right run.

With K the kept samples (|K| >= 1; always a prefix j = 0 .. |K| - 1 of the group's S samples: a sample exists when all before it do, and
a scene ends once) every payload sample position p gives

    out[p] = (2 * sum_{g in K} x_g[p] + |K|) // (2 * |K|)

(``--shutter-window box``, the default), or with the positive integer weights w_j of ``window_weights`` (``--shutter-window triangle``:
w_j = min(j + 1, S - j), a tent over the exposure) and W = sum_{j < |K|} w_j

    out[p] = (2 * sum_{j < |K|} w_j x_{cD+j}[p] + W) // (2 W)

so a truncated group renormalises by its own W and a constant payload stays constant.  Both run over the stored samples (uint8 at 8
bits, little-endian uint16 above), the payload taken as one flat array of P samples, so layout, depth, matrix and range never matter: an
average, rounded half up, in gamma light (not linear light) -- what ffmpeg's ``tmix``
computes on the fine stream, minus the samples across a cut.  ``mix_np`` is the definition the kernel (csrc/shutter.hip,
``demfi_payload_mix``, and ``demfi_payload_mix_w`` for weighted windows) is held to; the kernels divide by multiplying with
``magic(|K|)`` / ``magic_w(W)``, which are exact over their whole input range.  Not offered: gaussian or free weights, an exposure centred
on the frame time, linear-light mixing.

Only the instants the written frames need are run: ``filter_plan`` takes the plan of a window at the ratio R and keeps the outputs
whose fine index i has i mod D < S, and the instants those name.
"""
import re
from fractions import Fraction

import numpy as np

from .retime import MAX_RATIO, ST

MAX_SAMPLES = 32
DEFAULT_SAMPLES = 4
_ANGLE = re.compile(r'([0-9]+)(?:/([0-9]+))?')


def parse_shutter(text):
    """``180`` / ``1440/11`` -> the shutter angle in degrees as a Fraction, 0 < angle <= 360.  Decimals are refused: they are not exact."""
    if isinstance(text, bool) or isinstance(text, float):
        raise ValueError('shutter angle %r: give degrees as an integer N or an exact fraction N/D' % (text,))
    if isinstance(text, (int, Fraction)):
        angle = Fraction(text)
    else:
        m = _ANGLE.fullmatch(str(text).strip())
        if not m or int(m.group(2) or 1) == 0:
            raise ValueError('shutter angle %r: expected degrees as N or N/D with integers N, D > 0 (a decimal is not exact)' % (text,))
        angle = Fraction(int(m.group(1)), int(m.group(2) or 1))
    if not 0 < angle <= 360:
        raise ValueError('shutter angle %s outside (0, 360] degrees' % angle)
    return angle


def workable_samples(angle):
    """The sample counts S <= MAX_SAMPLES for which D = 360 S / angle is an integer."""
    angle = parse_shutter(angle)
    return [s for s in range(1, MAX_SAMPLES + 1) if (360 * s / angle).denominator == 1]


def check_params(angle, samples=DEFAULT_SAMPLES):
    """(S, D) of the shutter ``angle`` (degrees: int, Fraction or "N/D") with ``samples`` sub-frames: D = S / (angle / 360), which must be
    an integer.  ValueError otherwise; the message names the sample counts that work for the angle."""
    angle = parse_shutter(angle)
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
        raise ValueError('shutter samples must be an integer in 1 .. %d, got %r' % (MAX_SAMPLES, samples))
    d = 360 * samples / angle
    if d.denominator != 1:
        ok = workable_samples(angle)
        raise ValueError('shutter angle %s with %d samples: the fine stream would run 360 * %d / %s = %s times as fast as the written one, which '
                         'is not an integer; sample counts up to %d that work for this angle: %s'
                         % (angle, samples, samples, angle, d, MAX_SAMPLES, ', '.join(map(str, ok)) if ok else 'none'))
    return samples, int(d)


def fine_ratio(r, D):
    """R = r D, the ratio of the fine stream; ValueError above ``retime.MAX_RATIO``."""
    R = Fraction(r) * D
    if R > MAX_RATIO:
        raise ValueError('shutter: the fine stream would run %s x %d = %s times the input rate, more than %d; use fewer samples, a wider '
                         'shutter angle or a lower output rate' % (Fraction(r), D, R, MAX_RATIO))
    return R


def groups(n_fine, n_out, S, D, scene_of=None):
    """[[g, ...]] per written frame c = 0 .. n_out-1: the fine frames c D + j, j < S, that exist (g < n_fine) and lie in the scene of
    sample 0 (``scene_of(g)``: any value that differs between scenes; None: one scene)."""
    out = []
    for c in range(n_out):
        g0 = c * D
        if g0 >= n_fine:
            raise ValueError('shutter: written frame %d needs fine frame %d of %d' % (c, g0, n_fine))
        out.append([g for g in range(g0, min(g0 + S, n_fine)) if scene_of is None or scene_of(g) == scene_of(g0)])
    return out


WINDOWS = ('box', 'triangle')
MAX_WEIGHT_SUM = 4096


def check_window(name):
    """The shutter window ``name`` (None: 'box'), one of ``WINDOWS``; ValueError otherwise."""
    name = 'box' if name is None else name
    if name not in WINDOWS:
        raise ValueError('shutter window must be one of %s, got %r' % (', '.join(WINDOWS), name))
    return name


def window_weights(name, S):
    """The positive integer weights w_0 .. w_(S-1) of the samples of a written frame under the window ``name``: box 1 each; triangle
    w_j = min(j + 1, S - j) (S = 4: 1, 2, 2, 1; S = 5: 1, 2, 3, 2, 1; up to S = 2 the box).  Their sum is at most ``MAX_WEIGHT_SUM``
    (S = 32 triangle: 272)."""
    name = check_window(name)
    if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= MAX_SAMPLES:
        raise ValueError('shutter samples must be an integer in 1 .. %d, got %r' % (MAX_SAMPLES, S))
    w = [1] * S if name == 'box' else [min(j + 1, S - j) for j in range(S)]
    assert min(w) >= 1 and sum(w) <= MAX_WEIGHT_SUM
    return w


def mix_np(payloads, groups, sample_bytes, weights=None):
    """The written payloads [len(groups), Pb] uint8 of the fine ``payloads`` [n_fine, Pb] uint8 (``sample_bytes`` 1, or 2: little-endian
    16-bit samples): per group K, (2 sum + |K|) // (2 |K|) of every sample, accumulated in int64.  ``weights``[c] parallel to
    ``groups``[c] (None: all 1): (2 sum_j w_j x_j + W) // (2 W) with W the sum of the group's weights."""
    if sample_bytes not in (1, 2):
        raise ValueError('mix_np: %r bytes per sample (1 or 2)' % (sample_bytes,))
    x = np.ascontiguousarray(payloads, dtype=np.uint8)
    x = x.reshape(x.shape[0], -1)
    x = x.view('<u2') if sample_bytes == 2 else x
    out = np.empty((len(groups), x.shape[1]), x.dtype)
    for c, ks in enumerate(groups):
        if not ks:
            raise ValueError('mix_np: group %d keeps no sample' % c)
        if weights is None:
            out[c] = (2 * x[list(ks)].sum(axis=0, dtype=np.int64) + len(ks)) // (2 * len(ks))
            continue
        w = np.asarray(weights[c], np.int64)
        if w.shape != (len(ks),) or (w < 1).any():
            raise ValueError('mix_np: group %d of %d samples has the weights %r' % (c, len(ks), weights[c]))
        W = int(w.sum())
        out[c] = (2 * (x[list(ks)].astype(np.int64) * w[:, None]).sum(axis=0) + W) // (2 * W)
    return out.view(np.uint8)


def group_weights(groups, D, w):
    """``mix_np``'s ``weights`` for ``groups`` of fine indices (``groups``) under the window weights w: sample c D + j has weight w[j]."""
    return [[w[g % D] for g in ks] for ks in groups]


def magic_w(W):
    """(mul, sh) of the weighted kernel's division by 2 W: ((n * mul) >> 32) >> sh == n // (2 W) for every n = 2 sum + W it meets, W <=
    ``MAX_WEIGHT_SUM`` and sum <= W * 65535.  With n_max = 2 W 65535 + W (< 2^30), s = bit_length(n_max * 2 W) and M = 2^s // (2 W) + 1
    (< 2^30), M * 2 W exceeds 2^s by at most 2 W, so n M / 2^s is off by less than n_max * 2 W / (2 W * 2^s) < 1 / (2 W) quotient
    steps: exact.  Folded to one 32-bit multiply-high: s < 32 pre-shifts M (mul = M << (32 - s), sh = 0), else mul = M, sh = s - 32.
    The entry point ``demfi_payload_mix_w`` computes the same constants on the host; the kernel computes none."""
    if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= MAX_WEIGHT_SUM:
        raise ValueError('magic_w: W = %r outside 1 .. %d' % (W, MAX_WEIGHT_SUM))
    s = ((2 * W * 65535 + W) * 2 * W).bit_length()
    M = (1 << s) // (2 * W) + 1
    mul, sh = (M << (32 - s), 0) if s < 32 else (M, s - 32)
    assert mul < 1 << 32
    return mul, sh


def magic(k):
    """The 32-bit multiplier M of the kernel's division by 2 k: (n * M) >> 32 == n // (2 k) for every n = 2 sum + k it meets,
    k <= MAX_SAMPLES and sum <= k * 65535 (n < 2^22).  M = 2^32 // (2 k) + 1: M * 2 k exceeds 2^32 by at most 2 k <= 64, so the product
    is off by less than n * 64 / 2^32 < 1 / (2 k) quotient steps; tests/test_shutter.py walks the whole range."""
    return (1 << 32) // (2 * k) + 1


def filter_plan(runs, outs, S, D):
    """The plan of one window at the fine ratio (``scene.window_runs``: runs = [(tuple, instants)], outs = [(fine index i, run, kind,
    instant index)] in stream order; ``retime.window_plan`` is the one-run case) -> what the written frames need of it.  Keeps the outputs
    with i mod D < S; of every run the instants a kept St names, and its first instant when a kept S0 / S1 of it is written (those come
    from the run's first instant); drops the runs left without outputs and renumbers ``run``.  A window that owns at least D consecutive
    fine indices (every window when r >= 1) always keeps some output; one that owns fewer (r < 1, ``--downconvert``) may be left nothing:
    no run, no output.  S == D keeps everything: the plan is returned as it is.  Pure."""
    if not 1 <= S <= D:
        raise ValueError('filter_plan: S = %r, D = %r' % (S, D))
    if S == D:
        return runs, outs
    kept = [o for o in outs if o[0] % D < S]
    assert kept or len(outs) < D, 'a window that owns at least D consecutive fine frames keeps one'
    new_runs, new_index, maps = [], {}, {}
    for ri, (tup, ts) in enumerate(runs):
        mine = [o for o in kept if o[1] == ri]
        if not mine:
            continue
        js = sorted({j for _, _, kind, j in mine if kind == ST} | ({0} if any(kind != ST for _, _, kind, _ in mine) else set()))
        new_index[ri], maps[ri] = len(new_runs), {j: n for n, j in enumerate(js)}
        new_runs.append((tup, [ts[j] for j in js]))
    return new_runs, [(i, new_index[ri], kind, maps[ri][j]) for i, ri, kind, j in kept]


def close_groups(still_open, fine, scene, ends, S, D, first_row):
    """One batch of the shutter stage, pure.  ``still_open``: [(fine index, scene, row)] of the samples of the group left open by the batch
    before, at the rows they were carried to; ``fine``[w] = (is window w a cut window, [(fine index, from the right run of the cut window)])
    of the batch's windows, whose payloads lie at the rows first_row, first_row + 1, ...; ``scene``: the scene number so far (a cut window
    raises it between its left and its right outputs); ``ends``: the batch holds the clip's last window, so every group is closed.  A group
    closes when its sample S - 1 has arrived.  Returns (the rows of the kept samples of every closed group in order, the written frames per
    window -- a frame counts to the window that brought its last sample --, the samples still open, the scene number)."""
    counts = [0] * len(fine)
    arrived, row = [(g, sc, rw, 0) for g, sc, rw in still_open], first_row
    for wi, (cut, entries) in enumerate(fine):
        for g, right in entries:
            arrived.append((g, scene + int(right), row, wi))
            row += 1
        scene += int(cut)
    grouped = []                                     # consecutive samples of one written frame
    for smp in arrived:
        if not grouped or grouped[-1][0][0] // D != smp[0] // D:
            grouped.append([])
        grouped[-1].append(smp)
    table, left = [], []
    for gi, grp in enumerate(grouped):
        c = grp[0][0] // D
        if [g for g, _, _, _ in grp] != list(range(c * D, c * D + len(grp))) or len(grp) > S:
            raise RuntimeError('shutter: written frame %d got the fine frames %s' % (c, [g for g, _, _, _ in grp]))
        if len(grp) < S and not ends:                # its next sample is still to come
            if gi != len(grouped) - 1:
                raise RuntimeError('shutter: written frame %d is left open behind a later one' % c)
            left = [(g, sc, rw) for g, sc, rw, _ in grp]
            break
        table.append([rw for _, sc, rw, _ in grp if sc == grp[0][1]])
        counts[grp[-1][3]] += 1
    return table, counts, left, scene


def period_counts(r, S, D, scan=1000):
    """The instants per window of the filtered schedule at the ratio r with (S, D), over one period (at most ``scan`` windows): what
    ``retime.default_n_ctx`` sizes the batched plan by."""
    from . import retime as R
    fine = Fraction(r) * D
    out = []
    for k in range(min(fine.denominator * D, scan)):
        ts, o = R.window_plan(k, fine)
        runs = filter_plan([(None, ts)] if ts else [], [(i, 0, kind, j) for i, kind, j in o], S, D)[0]
        out.append(len(runs[0][1]) if runs else 0)           # a window left nothing (r < 1) runs no instant
    return out
