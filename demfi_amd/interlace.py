"""Interlaced Y4M output (``python -m demfi_amd.video --interlace tff|bff [--interlace-lowpass off|linear|complex]``): consecutive frames
of the progressive output become the two fields of one payload.  Pure Python / numpy; the one module that knows the rule.

**Pairing.**  With the switch, the progressive stream a run without it would write (with ``--shutter``: its mixed frames) is frames
c = 0 .. N-1 at the rate F_out.  The run writes ``n_payloads(N)`` = ceil(N / 2) payloads: payload q weaves frame 2q, the first field in
time, and frame 2q + 1, the second; when N is odd the last payload weaves frame N-1 with itself.  The header is the progressive one but
for two items (``interlaced_header``): the I tag is ``It`` (tff) or ``Ib`` (bff) and the rate is F_out / 2.  So ``--fps`` and ``--mfi``
name the FIELD rate, as they do behind ``--deinterlace``: ``--deinterlace --fps 60000/1001 --interlace tff`` turns 50i into 59.94i.

**Weave.**  Per plane of the payload (``y4m.split_planes_layout``; the chroma planes of every layout follow the rule on their own rows):
with q0 = ``deint.field_parity(order, 0)``, output row y comes from the first frame when y mod 2 == q0, else from the second.  This is
the convention of ``demfi_amd.deint``: bobbing the woven payload gives the two frames' own rows back.

**Low-pass** (default ``linear``) damps interline twitter.  An output row is computed from rows of the ONE frame that owns it, never from
both; row indices are clamped to [0, rows - 1]; signed integers, ``>>`` a floor shift.  With c = src[y], a = src[y-1], b = src[y+1],
a2 = src[y-2], b2 = src[y+2]:

    off:      out = c
    linear:   out = (a + 2 c + b + 2) >> 2
    complex:  v = clip((4 + 6 c + 2 (a + b) - a2 - b2) >> 3, 0, peak),  peak = 2^depth - 1
              out = max(v, c) if a + b > 2 c else min(v, c)

The guard of ``complex`` keeps the filter from pushing a sample past itself, away from its neighbours' mean.  These have the shape of
the vertical filters of ffmpeg's ``interlace`` / ``tinterlace``; numeric equality with them is not claimed (``demfi_amd.scene`` takes the
same stance towards ``scdet``).  ``weave_payload_np`` is the definition the kernel (csrc/interlace.hip, ``demfi_payload_weave``) is held
to, byte for byte.

Not offered: the quarter-row chroma offset that interlaced 4:2:0 fields have (as in ``demfi_amd.deint``), fusing the weave into the
gather so that unused rows are never converted, ``Im`` output, several ranks, ``demfi_amd.clip``.
"""
from fractions import Fraction

import numpy as np

from . import deint as I
from . import y4m

LOWPASS = ('off', 'linear', 'complex')
DEFAULT_LOWPASS = 'linear'
_ORDERS = {'tff': 't', 'bff': 'b', 't': 't', 'b': 'b'}


def parse_order(text):
    """``tff`` / ``bff`` / ``t`` / ``b`` -> the field order 't' or 'b' of the written stream."""
    if not isinstance(text, str) or text.strip().lower() not in _ORDERS:
        raise ValueError("interlace: the field order must be 'tff' or 'bff' (or 't', 'b'), got %r" % (text,))
    return _ORDERS[text.strip().lower()]


def check_lowpass(mode):
    """None (the default, ``linear``) or one of ``LOWPASS``."""
    if mode is None:
        return DEFAULT_LOWPASS
    if mode not in LOWPASS:
        raise ValueError('interlace_lowpass must be one of %s, got %r' % (', '.join(LOWPASS), mode))
    return mode


def n_payloads(n):
    """Payloads written for n progressive frames: ceil(n / 2)."""
    if n < 0:
        raise ValueError('n_payloads: %r frames' % (n,))
    return (int(n) + 1) // 2


def interlaced_header(hdr, order):
    """The header of the woven stream: ``hdr`` (the progressive output header) with the I tag of ``order`` and half the rate."""
    return y4m.Header(hdr.w, hdr.h, Fraction(hdr.fps) / 2, parse_order(order), hdr.aspect, hdr.chroma, hdr.color_range, hdr.xtags,
                      hdr.ctag, hdr.depth, hdr.layout)


def plane_shapes(h, w, layout):
    """[(rows, cols)] of the planes of an h x w payload, in payload order: Y, then Cb and Cr unless mono."""
    ch, cw = y4m.chroma_shape(h, w, layout)
    return [(h, w)] + ([(ch, cw)] * 2 if layout != 'mono' else [])


def lowpass_plane_np(src, depth, lowpass):
    """Every row of the plane ``src`` [rows, cols] filtered vertically within ``src`` (the module's docstring) -> int64 [rows, cols]."""
    lowpass = check_lowpass(lowpass)
    s = np.asarray(src).astype(np.int64)
    if s.ndim != 2:
        raise ValueError('lowpass_plane_np: a [rows, cols] plane, got %s' % (s.shape,))
    rows = s.shape[0]
    if lowpass == 'off' or rows == 0:
        return s
    ys = np.arange(rows)
    a, b, c = s[np.clip(ys - 1, 0, rows - 1)], s[np.clip(ys + 1, 0, rows - 1)], s
    if lowpass == 'linear':
        return (a + 2 * c + b + 2) >> 2
    a2, b2 = s[np.clip(ys - 2, 0, rows - 1)], s[np.clip(ys + 2, 0, rows - 1)]
    v = np.clip((4 + 6 * c + 2 * (a + b) - a2 - b2) >> 3, 0, (1 << depth) - 1)
    return np.where(a + b > 2 * c, np.maximum(v, c), np.minimum(v, c))


def weave_plane_np(first, second, depth, q0, lowpass=DEFAULT_LOWPASS):
    """One plane woven: rows of parity ``q0`` from ``first``, the others from ``second``, each low-passed within its own frame; the
    dtype of ``first``."""
    f, s = np.asarray(first), np.asarray(second)
    if f.ndim != 2 or f.shape != s.shape or q0 not in (0, 1):
        raise ValueError('weave_plane_np: two [rows, cols] planes of one shape and q0 in (0, 1), got %s, %s and %r' % (f.shape, s.shape, q0))
    out = lowpass_plane_np(s, depth, lowpass)
    out[q0::2] = lowpass_plane_np(f, depth, lowpass)[q0::2]
    return out.astype(f.dtype)


def weave_payload_np(first, second, h, w, depth, layout, order, lowpass=DEFAULT_LOWPASS):
    """The woven payload (a 1-D array of samples: uint8 at 8 bits, uint16 above) of the payloads ``first`` and ``second`` of h x w frames:
    every plane by ``weave_plane_np`` with q0 = ``deint.field_parity(order, 0)``."""
    q0 = I.field_parity(parse_order(order), 0)
    f, s = np.asarray(first).reshape(-1), np.asarray(second).reshape(-1)
    if f.dtype != s.dtype or f.dtype != (np.uint16 if depth > 8 else np.uint8):
        raise ValueError('weave_payload_np: %s and %s samples at %d bits' % (f.dtype, s.dtype, depth))
    planes = zip(y4m.split_planes_layout(f, h, w, layout), y4m.split_planes_layout(s, h, w, layout))
    return np.concatenate([weave_plane_np(a, b, depth, q0, lowpass).reshape(-1) for a, b in planes if a is not None])


def weave_stream_np(payloads, h, w, depth, layout, order, lowpass=DEFAULT_LOWPASS):
    """The ``n_payloads(N)`` woven payloads of the N progressive ``payloads`` (bytes-like or uint8 arrays, in stream order) as uint8
    arrays: payload q weaves frames 2q and 2q + 1, an odd last frame with itself."""
    def samples(p):
        a = np.frombuffer(p, np.uint8) if not isinstance(p, np.ndarray) else p.reshape(-1).view(np.uint8)
        return a.view('<u2') if depth > 8 else a
    n = len(payloads)
    return [weave_payload_np(samples(payloads[2 * q]), samples(payloads[min(2 * q + 1, n - 1)]), h, w, depth, layout, order,
                             lowpass).view(np.uint8) for q in range(n_payloads(n))]


def close_pairs(still_open, counts, ends, first_row=0):
    """One batch of the weave stage, pure.  ``still_open``: None, or the row of the one frame left open by the batch before, where it was
    carried to; ``counts``[w]: the progressive frames window w of the batch brings, which lie in stream order at the rows first_row,
    first_row + 1, ...; ``ends``: the batch holds the clip's last window, so an odd last frame is closed with itself.  A pair closes when
    its second frame has arrived.  Returns (the (row of the first field's frame, row of the second's) of every closed pair in order, the
    woven payloads per window -- a payload counts to the window that completed it, the odd tail to the batch's last window --, the row of
    the frame still open or None)."""
    woven, pairs, row = [0] * len(counts), [], first_row
    for wi, c in enumerate(counts):
        if c < 0:
            raise ValueError('close_pairs: window %d brings %r frames' % (wi, c))
        for _ in range(c):
            if still_open is None:
                still_open = row
            else:
                pairs.append((still_open, row))
                woven[wi] += 1
                still_open = None
            row += 1
    if ends and still_open is not None:
        if not counts:
            raise ValueError('close_pairs: a batch without windows cannot end the clip')
        pairs.append((still_open, still_open))
        woven[-1] += 1
        still_open = None
    return pairs, woven, still_open
