"""Synthesized motion blur of the Y4M video path (``python -m demfi_amd.video --shutter ANGLE [--shutter-samples S]``): the network's
frames are sharp, as if shot with a near-zero shutter angle; a written frame becomes the average of S finer frames spread over its
exposure instead.  Pure Python / numpy; the one module that knows the definition.

The exposure is e = ANGLE / 360 of the written stream's frame period (0 < ANGLE <= 360: 180 degrees is the film look).  With S samples
per written frame the sub-frames are e / S of a frame period apart, so the fine stream they come from runs D = S / e times as fast as
the written one; D must be an integer (180 degrees with S = 4: D = 8; 360 with S = 4: D = 4; 90 with S = 4: D = 16).  With the stream's
ratio r = F_out / F_in (M for ``--mfi M``) the fine stream is the ordinary timeline of ``demfi_amd.retime`` at the ratio R = r D, on
either timeline, and R may not exceed ``retime.MAX_RATIO``.

Written ("coarse") frame c exposes from its own time tau_c on: its samples are the fine frames g = c D + j, j = 0 .. S-1.  The written
stream has the header, the length (``retime.n_output_frames(n, r, full)``) and the timing of a run without the switch.  Fine frame c D
always exists (non-full: (N_out - 1) D = floor((n-3) r) D <= floor((n-3) r D); full: (ceil(n r) - 1) D < n r D); later samples of the
last groups may not.  A group keeps a sample when it exists and lies in the same scene as sample 0: with scene cuts
(``demfi_amd.scene``) the scene changes inside a cut window only, between the outputs of its left run and those of its right run.

With K the kept samples (|K| >= 1) every payload sample position p gives

    out[p] = (2 * sum_{g in K} x_g[p] + |K|) // (2 * |K|)

over the stored samples (uint8 at 8 bits, little-endian uint16 above), the payload taken as one flat array of P samples, so layout,
depth, matrix and range never matter: a box average, rounded half up, in gamma light (not linear light) -- what ffmpeg's ``tmix``
computes on the fine stream, minus the samples across a cut.  ``mix_np`` is the definition the kernel (csrc/shutter.hip,
``demfi_payload_mix``) is held to; the kernel divides by multiplying with ``magic(|K|)``, which is exact over its whole input range.

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


def mix_np(payloads, groups, sample_bytes):
    """The written payloads [len(groups), Pb] uint8 of the fine ``payloads`` [n_fine, Pb] uint8 (``sample_bytes`` 1, or 2: little-endian
    16-bit samples): per group K, (2 sum + |K|) // (2 |K|) of every sample, accumulated in int64."""
    if sample_bytes not in (1, 2):
        raise ValueError('mix_np: %r bytes per sample (1 or 2)' % (sample_bytes,))
    x = np.ascontiguousarray(payloads, dtype=np.uint8)
    x = x.reshape(x.shape[0], -1)
    x = x.view('<u2') if sample_bytes == 2 else x
    out = np.empty((len(groups), x.shape[1]), x.dtype)
    for c, ks in enumerate(groups):
        if not ks:
            raise ValueError('mix_np: group %d keeps no sample' % c)
        out[c] = (2 * x[list(ks)].sum(axis=0, dtype=np.int64) + len(ks)) // (2 * len(ks))
    return out.view(np.uint8)


def magic(k):
    """The 32-bit multiplier M of the kernel's division by 2 k: (n * M) >> 32 == n // (2 k) for every n = 2 sum + k it meets,
    k <= MAX_SAMPLES and sum <= k * 65535 (n < 2^22).  M = 2^32 // (2 k) + 1: M * 2 k exceeds 2^32 by at most 2 k <= 64, so the product
    is off by less than n * 64 / 2^32 < 1 / (2 k) quotient steps; tests/test_shutter.py walks the whole range."""
    return (1 << 32) // (2 * k) + 1


def filter_plan(runs, outs, S, D):
    """The plan of one window at the fine ratio (``scene.window_runs``: runs = [(tuple, instants)], outs = [(fine index i, run, kind,
    instant index)] in stream order; ``retime.window_plan`` is the one-run case) -> what the written frames need of it.  Keeps the outputs
    with i mod D < S; of every run the instants a kept St names, and its first instant when a kept S0 / S1 of it is written (those come
    from the run's first instant); drops the runs left without outputs and renumbers ``run``.  A window owns at least D consecutive fine
    indices (r >= 1), so some output is always kept.  S == D keeps everything: the plan is returned as it is.  Pure."""
    if not 1 <= S <= D:
        raise ValueError('filter_plan: S = %r, D = %r' % (S, D))
    if S == D:
        return runs, outs
    kept = [o for o in outs if o[0] % D < S]
    assert kept, 'a window owns at least D consecutive fine frames'
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
        out.append(len(filter_plan([(None, ts)], [(i, 0, kind, j) for i, kind, j in o], S, D)[0][0][1]))
    return out
