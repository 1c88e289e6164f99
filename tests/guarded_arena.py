"""Hostile memory for kernels that take views and bare pointers  --  TEST INFRASTRUCTURE (not shipped).

``Arena`` is the slab of ``tests/guarded_plan.py`` without the ``engine.Plan`` around it: ONE uint8 tensor that starts out as 0xFF
bytes (0xFFFF is a NaN as fp16, 0xFFFFFFFF a NaN as fp32, 0xFF the one uint8 value ``randint(0, 255)`` never draws), out of which
every argument of a launch is cut:

  * ``fat(B, h, w, C, dtype)``: the interior of a poisoned [B, h+2G, w+2G, C] block (G = 4 pixels) -- every NHWC ``demfi_view``.  Rows -1
    and h, columns -1 and w and the space between two images are guard memory; sy != w * sx and sb != h * sy.
  * ``thin(C, h, w)`` (``n=`` for n copies at one stride): the interior of fp32 [C, h+2G, w+2G] -- every planar ``demfi_view``, and the
    strided ``pred`` / ``gt`` of demfi_eval_frame.  sy != w and sc != h * w.
  * ``flat(n, shape, dtype)``: n TIGHT items at a constant stride of their size rounded up to 256 bytes plus GAP -- every bare-pointer
    argument, which the ABI declares contiguous.  Poison lies before, between and behind the items; ``zero=True`` zero-fills the items
    (a CFR workspace: the poison starts at byte workspace_bytes).  A batched launch gets ``bstride(t)``, never the tight size.
  * at least GAP = 256 poisoned bytes lie between any two blocks.

Interiors are poisoned until ``fill`` (or a kernel) writes them.  ``snapshot()`` before a launch, ``check(written)`` after it: every byte
of the slab outside the tensors listed in ``written`` (views of the slab: whole blocks, channel slices, single items) must be what it
was, and ``assert_finite(written)`` finds a consumed guard value or an element nobody wrote inside them.  ``GuardError`` names the block
and the coordinates.

The contract this makes testable: a kernel touches the frame of the views it is given and the exact byte count of its workspaces, and
nothing else.  One caveat is out of reach on purpose: gather4 and the fat-warp records load out-of-frame corners from a clamped
IN-FRAME address with weight 0, which "contributes exactly 0 for finite data" -- a non-finite border pixel of a frame would leak into
out-of-frame samples.  The arena never poisons frame interiors, so that documented behaviour stays as it is.

``Plain`` hands out ordinary contiguous tensors (NaN / 0xFF filled) behind the same interface, so that one test body runs on either.
"""
import numpy as np
import torch

G = 4                 # guard pixels on every side of a frame
GAP = 256             # poisoned bytes between two blocks and between two flat items (at least)
POISON = 0xFF


class GuardError(AssertionError):
    pass


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _ints(dtype):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[_esz(dtype)]


def bstride(t):
    """Byte stride between the items / images / copies of a tensor an allocator returned (dimension 0)."""
    return t.stride(0) * t.element_size()


def bits(t):
    """The bytes of a tensor as a contiguous CPU integer tensor."""
    return t.contiguous().view(_ints(t.dtype)).cpu()


class _Block:
    __slots__ = ('name', 'kind', 'off', 'nbytes', 'full', 'dtype', 'item', 'stride')

    def __init__(self, name, kind, off, nbytes, full, dtype, item=0, stride=0):
        self.name, self.kind, self.off, self.nbytes, self.full, self.dtype = name, kind, off, nbytes, full, dtype
        self.item, self.stride = item, stride


class Arena:
    guarded = True

    def __init__(self, device='cpu', capacity=32 << 20):
        self.device = torch.device(device)
        self.slab = torch.full((capacity,), POISON, dtype=torch.uint8, device=self.device)
        self._cur = (-self.slab.data_ptr()) % 256 + GAP
        self._blocks = []                 # in address order
        self._snap = None
        self.recording = True
        self.bits = []                    # the bytes of every written region, launch by launch (record())

    # ---- memory --------------------------------------------------------------------------------------------------------------
    def _alloc(self, nbytes):
        off = self._cur
        self._cur = ((off + nbytes + 255) & ~255) + GAP
        if self._cur > self.slab.numel():
            raise MemoryError('Arena: the slab of %d bytes is full (pass a larger capacity)' % self.slab.numel())
        return off

    def _view(self, slab, off, shape, strides, dtype):
        e = _esz(dtype)
        assert off % e == 0
        return torch.as_strided(slab.view(dtype), tuple(shape), tuple(strides), off // e)

    def _add(self, kind, label, name, nbytes, full, dtype, item=0, stride=0):
        off = self._alloc(nbytes)
        name = 'block %d%s (%s %s)' % (len(self._blocks), ' "%s"' % name if name else '', kind, label)
        blk = _Block(name, kind, off, nbytes, tuple(full), dtype, item, stride)
        self._blocks.append(blk)
        return blk

    def fat(self, B, h, w, C, dtype, name=None):
        """[B,h,w,C]: the frames of a poisoned [B,h+2G,w+2G,C] block."""
        FH, FW = h + 2 * G, w + 2 * G
        blk = self._add('fat', [B, h, w, C], name, B * FH * FW * C * _esz(dtype), (B, FH, FW, C), dtype)
        return self._view(self.slab, blk.off + (G * FW + G) * C * _esz(dtype), (B, h, w, C), (FH * FW * C, FW * C, C, 1), dtype)

    def thin(self, C, h, w, n=None, name=None):
        """fp32 [C,h,w] (n given: [n,C,h,w], the copies one behind the other): the frames of a poisoned [n*C,h+2G,w+2G] block."""
        FH, FW = h + 2 * G, w + 2 * G
        planes = C * (n or 1)
        blk = self._add('thin', [planes, h, w], name, planes * FH * FW * 4, (planes, FH, FW), torch.float32)
        t = self._view(self.slab, blk.off + (G * FW + G) * 4, (n or 1, C, h, w), (C * FH * FW, FH * FW, FW, 1), torch.float32)
        return t if n is not None else t[0]

    def flat(self, n, shape, dtype, zero=False, name=None):
        """[n, *shape]: n tight items, item k at byte k * stride, stride = the item's size rounded up to 256 + GAP."""
        shape = tuple(int(s) for s in shape)
        e = _esz(dtype)
        item = int(np.prod(shape)) * e
        stride = ((item + 255) & ~255) + GAP
        blk = self._add('flat', [n] + list(shape), name, (n - 1) * stride + item, (n,) + shape, dtype, item, stride)
        tight = [int(np.prod(shape[i + 1:])) for i in range(len(shape))]
        t = self._view(self.slab, blk.off, (n,) + shape, [stride // e] + tight, dtype)
        if zero:
            t.zero_()
        return t

    def fill(self, t, values):
        """Write a tensor of the arena (its guards stay poisoned); returns it."""
        self._off(t)
        t.copy_(torch.as_tensor(values).to(self.device))
        return t

    def poison(self, t):
        """Back to 0xFF bytes: a destination before a second launch writes it."""
        self._off(t)
        t.view(_ints(t.dtype)).fill_(-1 if t.element_size() > 1 else POISON)

    def _off(self, t):
        o = t.data_ptr() - self.slab.data_ptr()
        assert t.device == self.slab.device and 0 <= o < self.slab.numel(), 'not a tensor of this arena'
        return o

    def _like(self, slab, t):
        """The bytes of ``slab`` (the live one or a snapshot) that ``t`` covers, as a tensor of t's shape."""
        return self._view(slab, self._off(t), t.shape, t.stride(), t.dtype)

    # ---- the checks ------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        self._snap = self.slab.clone()

    def check(self, written=()):
        """Every byte of the slab outside the tensors in ``written`` is bit-identical to the last snapshot: guards, sources,
        workspaces beyond their contract, scratch, the other channels of a destination record."""
        assert self._snap is not None, 'check() without snapshot()'
        now = self.slab.clone()
        for t in written:
            self._like(now, t).view(_ints(t.dtype)).copy_(self._like(self._snap, t).view(_ints(t.dtype)))
        if torch.equal(now, self._snap):
            return
        o = int((now != self._snap).nonzero()[0])
        raise GuardError(self._where(o, written) + ' (byte %d of the slab: 0x%02x -> 0x%02x)' % (o, int(self._snap[o]), int(now[o])))

    def _block_at(self, o):
        prev = None
        for blk in self._blocks:
            if blk.off <= o < blk.off + blk.nbytes:
                return blk, prev
            if blk.off < o:
                prev = blk
        return None, prev

    def _is_dest(self, blk, written):
        return any(self._block_at(self._off(t))[0] is blk for t in written)

    def _where(self, o, written):
        blk, prev = self._block_at(o)
        if blk is None:
            return 'guard bytes between two blocks written, %s' % ('%d bytes behind %s' % (o - prev.off - prev.nbytes, prev.name)
                                                                   if prev is not None else 'in front of the first block')
        rel = o - blk.off
        if blk.kind == 'flat':
            k, b = rel // blk.stride, rel % blk.stride
            if b < blk.item:
                at = '(item %d, byte %d, element %d)' % (k, b, b // _esz(blk.dtype))
                if self._is_dest(blk, written):
                    return '%s: a part of a destination that the launch does not own written at %s' % (blk.name, at)
                return '%s: source interior written at %s' % (blk.name, at)
            return '%s: byte %d behind item %d written (the gap between item %d and item %d)' % (blk.name, b - blk.item, k, k, k + 1)
        e = rel // _esz(blk.dtype)
        if blk.kind == 'fat':
            B, FH, FW, Cc = blk.full
            ch, x, y, b = e % Cc, e // Cc % FW, e // (Cc * FW) % FH, e // (Cc * FW * FH)
            img = 'image'
        else:
            Cc, FH, FW = blk.full
            ch, x, y, b = 0, e % FW, e // FW % FH, e // (FW * FH)
            img = 'plane'
        y, x, h, w = y - G, x - G, FH - 2 * G, FW - 2 * G
        at = '(%s %d, row %d, column %d, channel %d)' % (img, b, y, x, ch)
        if 0 <= y < h and 0 <= x < w:
            if self._is_dest(blk, written):
                return '%s: a part of a destination that the launch does not own written at %s' % (blk.name, at)
            return '%s: source interior written at %s' % (blk.name, at)
        rows = 'row %d%s' % (y, ' (= H)' if y == h else '')
        cols = 'column %d%s' % (x, ' (= W)' if x == w else '')
        return '%s: %s of %s %d written, at %s' % (blk.name, rows if not 0 <= y < h else cols, img, b, at)

    def assert_finite(self, written):
        """No NaN / inf in the written tensors: no poisoned value was consumed, no output element was left unwritten.  Integer
        tensors are left to the comparison with the reference (0xFF is a value the inputs never hold)."""
        for t in written:
            if not t.is_floating_point():
                continue
            bad = ~torch.isfinite(t)
            if bool(bad.any()):
                i = [int(v) for v in bad.nonzero()[0]]
                blk = self._block_at(self._off(t))[0]
                raise GuardError('%s: %s at index %s of the written region %s -- a poisoned value was consumed or the element was never '
                                 'written (%d of %d elements)' % (blk.name if blk else 'a tensor', float(t[tuple(i)]), i, list(t.shape),
                                                                  int(bad.sum()), t.numel()))

    def record(self, written):
        self.bits += [bits(t) for t in written]


class Plain:
    """The same interface on ordinary tensors: contiguous, an allocation each, NaN (floats) or 0xFF bytes (integers) until written."""
    guarded = False

    def __init__(self, device='cpu', recording=False):
        self.device = torch.device(device)
        self.recording = recording        # launch() keeps the bytes of what was written (the expectation of a guarded run's (e))
        self.bits = []

    def _new(self, shape, dtype, zero=False):
        if zero:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        if dtype.is_floating_point:
            return torch.full(shape, float('nan'), dtype=dtype, device=self.device)
        return torch.full(shape, POISON if dtype == torch.uint8 else -1, dtype=dtype, device=self.device)

    def fat(self, B, h, w, C, dtype, name=None):
        return self._new((B, h, w, C), dtype)

    def thin(self, C, h, w, n=None, name=None):
        return self._new((C, h, w) if n is None else (n, C, h, w), torch.float32)

    def flat(self, n, shape, dtype, zero=False, name=None):
        return self._new((n,) + tuple(int(s) for s in shape), dtype, zero)

    def fill(self, t, values):
        t.copy_(torch.as_tensor(values).to(self.device))
        return t

    def poison(self, t):
        t.view(_ints(t.dtype)).fill_(-1 if t.element_size() > 1 else POISON)

    def snapshot(self):
        pass

    def check(self, written=()):
        pass

    def assert_finite(self, written):
        for t in written:
            if t.is_floating_point():
                assert bool(torch.isfinite(t).all()), 'NaN / inf in a written tensor: an element was never written'

    def record(self, written):
        self.bits += [bits(t) for t in written]


def launch(al, call, written, what='', finite=None):
    """Run ``call`` (which returns a demfi status) between snapshot() and, in this order: (b) nothing but ``written`` changed,
    (c) ``written`` holds no NaN / inf; then the bytes of ``written`` are recorded for (e).  (d), the comparison with the reference,
    is the body's.  finite: the tensors of ``written`` that the launch must fill completely (default: all; a scratch buffer of which a
    launch may use a part is listed in ``written`` only, and then not recorded)."""
    from demfi_amd import _lib as L
    al.snapshot()
    L.check(call(), what)
    if al.device.type == 'cuda':
        torch.cuda.synchronize()
    al.check(written)
    al.assert_finite(written if finite is None else finite)
    if al.recording:
        al.record(written if finite is None else finite)


def assert_bit_identical(guarded, plain):
    """(e) nothing depends on addresses or pitches: the guarded run stored the bytes the run on contiguous tensors stored."""
    assert len(guarded.bits) == len(plain.bits) > 0
    for i, (a, b) in enumerate(zip(guarded.bits, plain.bits)):
        if not torch.equal(a, b):
            at = [int(v) for v in (a != b).nonzero()[0]]
            raise GuardError('written region %d differs from the plain run at %s (%d of %d elements)' % (i, at, int((a != b).sum()), a.numel()))
