"""Inverse telecine of Y4M input (``python -m demfi_amd.video --ivtc``): field matching and decimation, what ffmpeg's
``fieldmatch,decimate`` does for 24p film carried as 29.97 frames/s by 3:2 pulldown.  Pure Python and numpy; the one module that
knows the policy.  n payloads at F frames/s become n - floor(n/5) progressive frames at 4F/5, and everything behind this stage
(retiming, scene cuts, repeated frames, depths, layouts, tiles, the network, the egress) runs on that stream unchanged.

Virtual woven frame.  W(a, b) has the even rows of every plane from payload a (its top field) and the odd rows from payload b
(its bottom field); every plane uses its own row parity, with the shapes of ``y4m.chroma_shape``.  Only luma is scored: the first
h*w samples of a payload, as ``cadence.luma_np`` reads them.

Candidates for input payload p.  The top field of p is always kept: c = W(p, p), p = W(p, p-1), n = W(p, p+1); p is absent for the
first payload and n for the last.  Keeping the top field and trying the bottom field of three payloads recovers every film frame
of a 3:2 cadence in either field order and any phase, so ``It``, ``Ib``, ``Im`` and a wrongly flagged ``Ip`` are treated alike.

Comb score of a candidate.  Integers throughout; T = cthresh * 2^(depth-8), cthresh = 9 by default (ffmpeg fieldmatch's).  For
rows 2 <= y <= h-3 and every x, with d1 = W[y] - W[y-1] and d2 = W[y] - W[y+1], the sample is combed when both hold:
(d1 > T and d2 > T) or (d1 < -T and d2 < -T); and |W[y-2] + 4 W[y] + W[y+2] - 3 (W[y-1] + W[y+1])| > 6 T.  Rows 0, 1, h-2 and h-1
are never combed, and a plane with h < 5 scores (0, 0).  The plane is cut into 16x16 blocks from the top-left corner, partial at
the right and bottom; the score is (max_block, total): the largest number of combed samples in one block, and the number in the
plane.  ``comb_counts_np`` DEFINES it (the GPU computes it: csrc/ivtc.hip, ``demfi_luma_comb_counts``, integer for integer).

Match.  The present candidate with the smallest (max_block, total) wins; ties go in the order c, p, n, so a static or progressive
stream chooses c everywhere and comes back byte for byte.  The matched frame of payload p is W(p, chosen).

Residual combing.  A matched frame with max_block > combpel (80 by default, ffmpeg's) is COMBED: video-origin inserts, bad edits,
or a stream that starts mid-cycle.  ``combed='bob'`` (the default) rebuilds it with ``deint.bob_payload_np(..., q=0)``: the kept
top field, every plane; ``combed='keep'`` passes it through.  Either way its index is reported.

Decimation.  Matched frames are taken in cycles of five (5c .. 5c+4).  Each frame's metric is the luma SAD of the matched frame
against the matched frame before it (``woven_sad_np``; residual bobbing is not applied for this comparison); frame 0 has none and
is never dropped.  The frame with the smallest metric of the cycle is dropped, ties go to the lowest index, and a last cycle of
fewer than five drops nothing.  So n payloads give n - floor(n/5) frames whatever they show: the output is constant-rate at
exactly 4F/5, and ``film_header(hdr)`` is ``hdr`` at fps * 4/5, progressive.

Streaming.  ``Matcher`` and ``Decimator`` take scores as payloads arrive, as ``cadence.Detector`` does; the state is one payload of
look-ahead (for n) plus the open cycle.  ``FilmFrames`` is the stage: film frame i into a host buffer, strictly in order, in the
shape of the ``fetch(i, buf)`` that ``y4m.Frames`` takes.  Its scorer is an argument: ``NumpyScorer`` (the definitions, on the
host) or the two launches of csrc/ivtc.hip (``y4m_edge.IvtcScorer``).  ``pulldown_np`` makes a 3:2 telecined payload list from
progressive payloads, for tests and documents.

Known limit: combing weaker than T scores (0, 0), so a slow-moving mixed frame can tie with its clean candidate and keep c.

Out of scope: hybrid material (true 30i sections are decimated like the rest), cadences other than cycle 5 / drop 1, a scene-change
guard for the decimator, more than one rank (which frames are dropped depends on the whole prefix of the input,
as with ``--dedup``), and ``--ivtc`` together with ``--deinterlace``.  Interlaced output is ``--interlace`` (``demfi_amd.interlace``).
"""
from collections import deque
from fractions import Fraction

import numpy as np

from . import cadence as K
from . import deint as I
from . import y4m

BLOCK = 16
CYCLE = 5
DEFAULT_CTHRESH, DEFAULT_COMBPEL, DEFAULT_COMBED = 9, 80, 'bob'
COMBED_MODES = ('bob', 'keep')
CANDIDATES = 'cpn'
FILM_RATIO = Fraction(CYCLE - 1, CYCLE)


def check_params(cthresh=DEFAULT_CTHRESH, combpel=DEFAULT_COMBPEL, combed=DEFAULT_COMBED):
    """(cthresh, combpel, combed) as (int, int, str); ValueError for cthresh outside 0..255, combpel outside 0..256 (a block has
    256 samples) or a mode that is not 'bob' or 'keep'."""
    for name, v, top in (('cthresh', cthresh, 255), ('combpel', combpel, BLOCK * BLOCK)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= top:
            raise ValueError('ivtc: %s must be an integer in 0..%d, got %r' % (name, top, v))
    if combed not in COMBED_MODES:
        raise ValueError('ivtc: combed must be one of %s, got %r' % (', '.join(COMBED_MODES), combed))
    return int(cthresh), int(combpel), combed


def n_film_frames(n):
    """Frames n payloads give: one of every full cycle of five is dropped."""
    return n - n // CYCLE


def film_header(hdr):
    """Header of the film stream: ``hdr`` at 4/5 of its rate, progressive (``Ip``), everything else kept."""
    return y4m.Header(hdr.w, hdr.h, hdr.fps * FILM_RATIO, 'p', hdr.aspect, hdr.chroma, hdr.color_range, hdr.xtags, hdr.ctag, hdr.depth,
                      hdr.layout)


# ---- the definitions --------------------------------------------------------------------------------------------------------
def woven_luma_np(top, bot, h, w, depth=8):
    """Luma [h, w] (int64) of W(top, bot): even rows from payload ``top``, odd rows from payload ``bot``."""
    a = K.luma_np(top, h, w, depth)
    if bot is not top:
        a[1::2] = K.luma_np(bot, h, w, depth)[1::2]
    return a


def combed_np(plane, thresh):
    """bool [h, w]: the combed samples of an integer plane at the threshold T = ``thresh`` (the module's docstring)."""
    p = np.asarray(plane).astype(np.int64)
    h, w = p.shape
    out = np.zeros((h, w), bool)
    if h < 5:
        return out
    c, up, dn, up2, dn2 = p[2:h - 2], p[1:h - 3], p[3:h - 1], p[0:h - 4], p[4:h]
    d1, d2 = c - up, c - dn
    out[2:h - 2] = (((d1 > thresh) & (d2 > thresh)) | ((d1 < -thresh) & (d2 < -thresh))) & \
        (np.abs(up2 + 4 * c + dn2 - 3 * (up + dn)) > 6 * thresh)
    return out


def block_sums_np(mask):
    """Combed samples of every 16x16 block, int64 [ceil(h/16), ceil(w/16)]."""
    h, w = mask.shape
    nby, nbx = -(-h // BLOCK), -(-w // BLOCK)
    pad = np.zeros((nby * BLOCK, nbx * BLOCK), np.int64)
    pad[:h, :w] = mask
    return pad.reshape(nby, BLOCK, nbx, BLOCK).sum(axis=(1, 3))


def comb_counts_np(top, bot, h, w, depth=8, cthresh=DEFAULT_CTHRESH):
    """(max_block, total) of W(top, bot): the comb score of the module's docstring."""
    sums = block_sums_np(combed_np(woven_luma_np(top, bot, h, w, depth), cthresh << (depth - 8)))
    return int(sums.max()), int(sums.sum())


def woven_sad_np(a_top, a_bot, b_top, b_bot, h, w, depth=8):
    """Luma SAD of W(a_top, a_bot) against W(b_top, b_bot)."""
    return int(np.abs(woven_luma_np(a_top, a_bot, h, w, depth) - woven_luma_np(b_top, b_bot, h, w, depth)).sum())


def _samples(payload, depth):
    a = y4m.as_samples16(payload) if depth > 8 else (np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray)
                                                    else payload.reshape(-1))
    if depth == 8 and a.dtype != np.uint8:
        raise ValueError('a payload of 8-bit samples is a uint8 array, got %s' % a.dtype)
    return a


def weave_np(top, bot, h, w, depth, layout):
    """W(top, bot) over every plane: the payload (1-D uint8 / uint16, a copy) with the even rows of Y, Cb and Cr from ``top`` and
    their odd rows from ``bot``."""
    y4m.check_depth(depth)
    out = _samples(top, depth).copy()
    if bot is not top:
        src = y4m.split_planes_layout(_samples(bot, depth), h, w, y4m.check_layout(layout))
        for d, s in zip(y4m.split_planes_layout(out, h, w, layout), src):
            if d is not None:
                d[1::2] = s[1::2]
    return out


def pulldown_np(frames, order='t', phase=0):
    """3:2 pulldown of progressive frames, ``frames[i]`` = the list of 2-D planes of film frame i (every plane's rows alternate
    between the fields by its own parity) -> the telecined frames in the same form.  Film frame i is shown for
    2 fields when i + phase is even and for 3 when it is odd (phase 0: 2 3 2 3 ..., phase 1: 3 2 3 2 ...); the fields alternate in
    parity from the first, which is the top field for order 't' and the bottom field for 'b'; payload j holds fields 2j and 2j+1.
    A field left over at the end is paired with the other field of its own frame.  Four film frames give five payloads."""
    if order not in ('t', 'b') or phase not in (0, 1):
        raise ValueError("pulldown_np: order 't' or 'b' and phase 0 or 1, got %r and %r" % (order, phase))
    fields = [i for i in range(len(frames)) for _ in range(2 + ((i + phase) & 1))]
    if len(fields) & 1:
        fields.append(fields[-1])
    out = []
    for j in range(0, len(fields), 2):
        top, bot = (fields[j], fields[j + 1]) if order == 't' else (fields[j + 1], fields[j])
        planes = []
        for pt, pb in zip(frames[top], frames[bot]):
            p = np.array(pt, copy=True)
            p[1::2] = np.asarray(pb)[1::2]
            planes.append(p)
        out.append(planes)
    return out


def pulldown_payloads_np(payloads, h, w, depth, layout, order='t', phase=0):
    """``pulldown_np`` of whole payloads (as ``weave_np`` takes them) -> the telecined payloads, 1-D uint8 / uint16."""
    planes = [[p for p in y4m.split_planes_layout(_samples(f, depth), h, w, y4m.check_layout(layout)) if p is not None] for f in payloads]
    return [np.concatenate([p.reshape(-1) for p in f]) for f in pulldown_np(planes, order, phase)]


# ---- matching and decimation as payloads arrive -------------------------------------------------------------------------------
class Matcher:
    """Which bottom field each payload takes, as the payloads of a stream arrive in order.  ``push(p, scores)``: payload p =
    ``next`` with the (max_block, total) of its candidates in the order c, p, n (None: absent) -> the offset -1, 0 or +1 of the
    payload whose bottom field it takes.  ``matches``: the letter chosen for every payload, ``combed``: the payloads whose matched
    frame has max_block > combpel."""

    def __init__(self, combpel=DEFAULT_COMBPEL):
        self.combpel = check_params(combpel=combpel)[1]
        self.matches, self.combed, self.next = [], [], 0

    def push(self, p, scores):
        if p != self.next:
            raise RuntimeError('telecine.Matcher: payload %d pushed where payload %d was due' % (p, self.next))
        if len(scores) != 3 or scores[0] is None:
            raise RuntimeError('telecine.Matcher: payload %d needs the scores of c, p and n, that of c present' % p)
        best = min((tuple(int(v) for v in s), k) for k, s in enumerate(scores) if s is not None)     # ties: the lowest k
        k = best[1]
        self.matches.append(CANDIDATES[k])
        if best[0][0] > self.combpel:
            self.combed.append(p)
        self.next = p + 1
        return (0, -1, 1)[k]


class Decimator:
    """Which matched frames are dropped, as they arrive in order.  ``push(i, metric)``: frame i = ``next`` with its luma SAD
    against the matched frame before it (None for frame 0) -> the frames released as kept, in order: none while a cycle of five
    is open, four when it closes.  ``finish()``: the end of the stream -> the frames of the open cycle, all kept.  ``dropped``:
    the frames dropped so far."""

    def __init__(self):
        self.dropped, self.open, self.next = [], [], 0

    def push(self, i, metric=None):
        if i != self.next:
            raise RuntimeError('telecine.Decimator: frame %d pushed where frame %d was due' % (i, self.next))
        if (metric is None) != (i == 0):
            raise RuntimeError('telecine.Decimator: frame %d %s' % (i, 'has no frame before it' if i == 0 else 'needs its metric'))
        self.open.append((i, None if metric is None else int(metric)))
        self.next = i + 1
        if len(self.open) < CYCLE:
            return []
        drop = min((m, j) for j, m in self.open if m is not None)[1]          # ties: the lowest index; frame 0 is never dropped
        self.dropped.append(drop)
        kept, self.open = [j for j, _ in self.open if j != drop], []
        return kept

    def finish(self):
        kept, self.open = [j for j, _ in self.open], []
        return kept


class NumpyScorer:
    """The scorer of ``FilmFrames`` on the host: the numpy definitions.  ``put(i, payload)``: payload i arrived; ``forget(i)``: it
    is not read again; ``comb(entries)``: entries of (top, (c, p, n)) payload indices, None for an absent candidate -> per entry
    the three (max_block, total), None where absent; ``sad(quads)``: (a_top, a_bot, b_top, b_bot) -> the woven SADs."""

    def __init__(self, h, w, depth=8, cthresh=DEFAULT_CTHRESH):
        self.h, self.w, self.depth, self.cthresh, self.pay = h, w, depth, check_params(cthresh=cthresh)[0], {}

    def put(self, i, payload):
        self.pay[i] = payload

    def forget(self, i):
        self.pay.pop(i, None)

    def comb(self, entries):
        return [[None if b is None else comb_counts_np(self.pay[t], self.pay[b], self.h, self.w, self.depth, self.cthresh) for b in bots]
                for t, bots in entries]

    def sad(self, quads):
        return [woven_sad_np(*(self.pay[i] for i in q), self.h, self.w, self.depth) for q in quads]


class FilmFrames:
    """The stage: ``film(i, buf)`` writes film frame i of the input into ``buf`` (a writable buffer of the payload's bytes) and
    returns True, or False when the input has no such frame -- the ``fetch`` of ``y4m.Frames(payload=..., fetch=...)``; frames are
    asked for strictly in order.  ``read(j, buf)``: input payload j into ``buf``, False at the end (a ``y4m.Reader``'s
    ``read_into`` or a seeking reader), called in order.  ``hdr``: the INPUT's header.  ``scorer``: ``NumpyScorer`` or
    ``y4m_edge.IvtcScorer``.

    Per cycle of five payloads, plus one of look-ahead: the payloads are read and handed to the scorer, ONE ``comb`` call scores
    the three candidates of the five, the host matches, ONE ``sad`` call gives the decimation metrics, the host decimates, weaves
    the four kept frames with numpy row slices over every plane and bobs the combed ones if asked.  Payloads 5c-2 .. 5c+5 are
    held during cycle c.  ``matches``: {'c': , 'p': , 'n': } counts; ``dropped``: input indices; ``combed``: film-frame indices."""

    def __init__(self, read, hdr, scorer, combpel=DEFAULT_COMBPEL, combed=DEFAULT_COMBED):
        self.read, self.hdr, self.scorer = read, hdr, scorer
        _, combpel, self.mode = check_params(combpel=combpel, combed=combed)
        self.matcher, self.decimator = Matcher(combpel), Decimator()
        self.raw, self.bot = {}, {}             # payloads held; the payload whose bottom field payload p takes
        self.n = None                           # the input's length, once its end was seen
        self.got, self.cycle, self.done = 0, 0, False
        self.ready, self.next, self.combed = deque(), 0, []

    @property
    def matches(self):
        return {c: self.matcher.matches.count(c) for c in CANDIDATES}

    @property
    def dropped(self):
        return list(self.decimator.dropped)

    def _read_through(self, j):
        while self.n is None and self.got <= j:
            buf = np.empty(self.hdr.payload, np.uint8)
            if not self.read(self.got, buf):
                self.n = self.got
                break
            self.raw[self.got] = buf
            self.scorer.put(self.got, buf)
            self.got += 1

    def _emit(self, p):
        h = self.hdr
        top, bot = self.raw[p], self.raw[self.bot[p]]
        if p in self.matcher.combed:
            self.combed.append(self.next + len(self.ready))
            if self.mode == 'bob':
                return I.bob_payload_np(top, h.h, h.w, h.depth, h.layout, 0)
        return top if bot is top else weave_np(top, bot, h.h, h.w, h.depth, h.layout)

    def _cycle(self):
        lo = CYCLE * self.cycle
        self._read_through(lo + CYCLE)
        hi = min(lo + CYCLE, self.got)
        ps = list(range(lo, hi))
        if ps:
            scores = self.scorer.comb([(p, (p, p - 1 if p > 0 else None, p + 1 if p + 1 < self.got else None)) for p in ps])
            for p, s in zip(ps, scores):
                self.bot[p] = p + self.matcher.push(p, s)
            moving = [p for p in ps if p > 0]
            sads = dict(zip(moving, self.scorer.sad([(p, self.bot[p], p - 1, self.bot[p - 1]) for p in moving])))
            kept = [q for p in ps for q in self.decimator.push(p, sads.get(p))]
        else:
            kept = []
        if self.n is not None and hi == self.n:
            kept += self.decimator.finish()
            self.done = True
        for p in kept:
            self.ready.append(self._emit(p))
        self.cycle += 1
        for j in [j for j in self.raw if j < CYCLE * self.cycle - 2]:
            del self.raw[j]
            self.bot.pop(j, None)
            self.scorer.forget(j)

    def __call__(self, i, buf):
        if i != self.next:
            raise RuntimeError('telecine.FilmFrames: film frame %d asked for where frame %d was due' % (i, self.next))
        while not self.ready and not self.done:
            self._cycle()
        if not self.ready:
            return False
        f = self.ready.popleft()
        np.copyto(np.frombuffer(memoryview(buf).cast('B'), np.uint8), f.reshape(-1).view(np.uint8))
        self.next += 1
        return True


def film_of(payloads, h, w, depth=8, layout='420', cthresh=DEFAULT_CTHRESH, combpel=DEFAULT_COMBPEL, combed=DEFAULT_COMBED):
    """The whole-clip answer on the host: a list of payloads (uint8 arrays of their bytes) -> (film payloads, the ``FilmFrames``
    that made them, for its counters)."""
    hdr = y4m.Header(w, h, 30, 'p', depth=depth, layout=layout)
    pays = [np.frombuffer(memoryview(np.ascontiguousarray(p)).cast('B'), np.uint8) for p in payloads]

    def read(j, buf):
        if j >= len(pays):
            return False
        buf[:] = pays[j]
        return True
    film = FilmFrames(read, hdr, NumpyScorer(h, w, depth, cthresh), combpel, combed)
    out, buf = [], np.empty(hdr.payload, np.uint8)
    while film(len(out), buf):
        out.append(buf.copy())
    return out, film
