"""A ``Plan`` whose memory is hostile  --  TEST INFRASTRUCTURE (not shipped).

``engine.Plan`` gives every buffer, the zero page and the weight blob a zero-filled allocation of its own: a kernel that reads row -1
or row H finds zeros (the padding value) and one that stores past the frame writes where nobody looks.  ``GuardedPlan`` puts all of
them into ONE uint8 slab that starts out as 0xFF bytes (0xFFFF is a NaN as fp16, 0xFFFFFFFF a NaN as fp32):

  * a fat buffer [B,h,w,C] is the interior crop of a poisoned [B,h+2G,w+2G,C] block (G = 4 pixels: the largest halo of the project is
    3), a thin buffer [C,h,w] the interior crop of [C,h+2G,w+2G]: rows -1 and h, columns -1 and w and the gap between two images are
    guard memory, and the row pitch differs from the row length;
  * the zero page is 256 zero bytes with poison directly behind it, the weight blob is followed by poison, and at least 256 poisoned
    bytes lie between any two blocks;
  * interiors are poisoned until ``fill`` (or a kernel) writes them, so an output pixel nobody wrote is a NaN;
  * ``snapshot()`` before a launch, ``check(written=[...])`` after it: every byte outside the listed destination interiors and channel
    ranges must be what it was, and ``assert_finite(written)`` finds a consumed guard value or an unwritten pixel inside them.

The contract this makes testable: a kernel touches only [0,H) x [0,W) of the views it is given, plus the first 256 bytes of the zero page.
"""
import ctypes as C

import numpy as np
import torch

from demfi_amd import _lib as L
from demfi_amd.engine import Plan, _Src, _view
from tests.guarded_arena import G, GAP, POISON, GuardError    # one error type and one guard geometry for both harnesses


class _Block:
    __slots__ = ('name', 'fat', 'off', 'nbytes', 'full', 'dtype', 'key')

    def __init__(self, name, fat, off, nbytes, full, dtype, key):
        self.name, self.fat, self.off, self.nbytes, self.full, self.dtype, self.key = name, fat, off, nbytes, full, dtype, key

    def of(self, slab):
        """This block of ``slab`` (the live one or a snapshot) with its guard frame: [B,h+2G,w+2G,C] or [C,h+2G,w+2G]."""
        return slab[self.off:self.off + self.nbytes].view(self.dtype).view(self.full)

    def region(self, slab, c0=0, c1=None):
        """The frame (no guards), channels / planes [c0, c1)."""
        t = self.of(slab)
        if self.fat:
            return t[:, G:t.shape[1] - G, G:t.shape[2] - G, c0:c1]
        return t[c0:c1, G:t.shape[1] - G, G:t.shape[2] - G]


class GuardedPlan(Plan):
    def __init__(self, H, W, dtype=torch.float16, device='cuda:0', state_dict=None, capacity=32 << 20, slab=None):
        """slab: a uint8 tensor to build the plan in (tests/far_memory.py: one multi-GiB slab for every case); it is poisoned here."""
        super().__init__(H, W, dtype, device, state_dict)
        self.slab = torch.full((capacity,), POISON, dtype=torch.uint8, device=self.device) if slab is None else slab.fill_(POISON)
        self._cur = (-self.slab.data_ptr()) % 256 + GAP
        self._blocks = []                 # in address order
        self._by_key = {}                 # data_ptr of the interior -> block
        self._spans = []                  # (off, nbytes, what) of the zero page and the weight blob
        self._snap = None

    # ---- memory ------------------------------------------------------------------------------------------------
    def _alloc(self, nbytes):
        off = self._cur
        self._cur = ((off + nbytes + 255) & ~255) + GAP
        if self._cur > self.slab.numel():
            raise MemoryError('GuardedPlan: the slab of %d bytes is full (pass a larger capacity)' % self.slab.numel())
        return off

    def _block(self, fat, full, dtype, inner):
        esz = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(full)) * esz
        off = self._alloc(nbytes)
        name = 'buffer %d (%s %s)' % (len(self._blocks), 'fat' if fat else 'thin', list(inner))
        blk = _Block(name, fat, off, nbytes, tuple(full), dtype, None)
        t = blk.region(self.slab)
        blk.key = t.data_ptr()
        self._blocks.append(blk)
        self._by_key[blk.key] = blk
        return t

    def _fat(self, h, w, c, batch=1):
        return self._block(True, (batch, h + 2 * G, w + 2 * G, c), self.dtype, (batch, h, w, c))

    def _thin(self, c, h=None, w=None):
        h, w = h or self.H, w or self.W
        return self._block(False, (c, h + 2 * G, w + 2 * G), torch.float32, (c, h, w))

    def regions(self):
        return [self.slab]

    def block_of(self, buf):
        return self._by_key[buf.data_ptr()]

    def fill(self, buf, values):
        """Write the interior of a buffer (its guards stay poisoned)."""
        self.block_of(buf)
        buf.copy_(values)

    def poison(self, t):
        """Back to 0xFF bytes: a buffer made by _fat / _thin, or a slice of one (the channel range a launch writes)."""
        t.view(torch.int16 if t.element_size() == 2 else torch.int32).fill_(-1)

    # ---- views: strides from the tensors themselves ------------------------------------------------------------------
    def fsrc(self, buf, cin0, c0=0, nch=None, b=None, up=0):
        B, h, w, Ct = buf.shape
        sb, sy, sx, sc = buf.stride()
        nch = Ct - c0 if nch is None else nch
        ptr = buf.data_ptr() + (c0 * sc + (0 if b is None else b * sb)) * self.esz
        return _Src(True, ptr, sx, sy, sc, sb if b is None else 0, self.f32, range(cin0, cin0 + nch), up)

    def fsrc_map(self, buf, cin, b=0):
        B, h, w, Ct = buf.shape
        sb, sy, sx, sc = buf.stride()
        assert len(cin) == Ct
        ptr = buf.data_ptr() + (0 if b is None else b) * sb * self.esz
        return _Src(True, ptr, sx, sy, sc, sb if b is None else 0, self.f32, cin, 0)

    def tsrc(self, buf, cin, c0=0, nch=None):
        Ct, h, w = buf.shape
        sc, sy, sx = buf.stride()
        nch = Ct - c0 if nch is None else nch
        cin = list(cin)
        assert len(cin) == nch
        return _Src(False, buf.data_ptr() + c0 * sc * 4, sx, sy, sc, 0, True, cin)

    def fview(self, buf, c0=0, b=None):
        B, h, w, Ct = buf.shape
        sb, sy, sx, sc = buf.stride()
        ptr = buf.data_ptr() + (c0 * sc + (0 if b is None else b * sb)) * self.esz
        return _view(ptr, sx, sy, sc, sb if b is None else 0, self.f32)

    def tview(self, buf, c0=0, sb=0):
        """sb: the batch stride in elements of a CONTIGUOUS [C,h,w] tensor (a whole number of planes), as Plan.tview takes it."""
        Ct, h, w = buf.shape
        sc, sy, sx = buf.stride()
        assert sb % (h * w) == 0
        return _view(buf.data_ptr() + c0 * sc * 4, sx, sy, sc, sb // (h * w) * sc, True)

    # ---- weights, zero page, descriptors -------------------------------------------------------------------------------
    def _upload(self):
        host = np.zeros(max(self._wbytes, 256), np.uint8)
        for off, a in self._wblobs:
            host[off:off + a.nbytes] = a.reshape(-1)
        self._wblobs = None
        zoff = self._alloc(256)
        self.zero_page = self.slab[zoff:zoff + 256]
        self.zero_page.zero_()
        boff = self._alloc(host.size)
        self.weight_blob = self.slab[boff:boff + host.size]
        self.weight_blob.copy_(torch.from_numpy(host))
        self._spans = [(zoff, 256, 'the zero page'), (boff, host.size, 'the weight blob')]
        base = self.weight_blob.data_ptr()
        for d in self._descs:
            d.wpack = base + (d.wpack or 0)
            d.bias = base + (d.bias or 0)
            d.zero_page = self.zero_page.data_ptr()
        sz = C.sizeof(L.Conv)
        raw = bytearray(len(self._descs) * sz)
        for i, d in enumerate(self._descs):
            raw[i * sz:(i + 1) * sz] = bytes(d)
        self.desc_dev = torch.frombuffer(raw, dtype=torch.uint8).clone().to(self.device)
        self._desc_sz = sz

    # ---- the checks ----------------------------------------------------------------------------------------------------
    def snapshot(self):
        self._snap = self.slab.clone()

    @staticmethod
    def _norm(written):
        out = []
        for w in written:
            if isinstance(w, torch.Tensor):
                out.append((w, 0, None))
            else:
                out.append((w[0], w[1], w[2]))
        return out

    def check(self, written=()):
        """Everything but the frames (and channel / plane ranges) listed in ``written`` -- buffers, or (buffer, c0, c1) -- is
        bit-identical to the last snapshot: guards, sources, the zero page, the weights, the other channels of a destination."""
        assert self._snap is not None, 'check() without snapshot()'
        written = self._norm(written)
        now = self.slab.clone()
        for buf, c0, c1 in written:
            blk = self.block_of(buf)
            blk.region(now, c0, c1).copy_(blk.region(self._snap, c0, c1))
        if torch.equal(now, self._snap):
            return
        o = int((now != self._snap).nonzero()[0])
        raise GuardError(self._where(o, written) + ' (byte %d of the slab: 0x%02x -> 0x%02x)' % (o, int(self._snap[o]), int(now[o])))

    def _coords(self, blk, o):
        """Byte o of the slab inside blk -> (image or plane, row, column, channel) relative to the frame."""
        e = (o - blk.off) // torch.empty((), dtype=blk.dtype).element_size()
        if blk.fat:
            B, FH, FW, Cc = blk.full
            ch = e % Cc
            x = e // Cc % FW
            y = e // (Cc * FW) % FH
            b = e // (Cc * FW * FH)
        else:
            Cc, FH, FW = blk.full
            ch = 0
            x = e % FW
            y = e // FW % FH
            b = e // (FW * FH)
        return b, y - G, x - G, ch, FH - 2 * G, FW - 2 * G

    def _where(self, o, written):
        for off, nb, what in self._spans:
            if off <= o < off + nb:
                return '%s written at byte %d' % (what, o - off)
            if what == 'the zero page' and off + nb <= o < off + nb + GAP:
                return 'byte %d behind the zero page written' % (o - off - nb)
            if what == 'the weight blob' and off + nb <= o:
                return 'byte %d behind the weight blob written' % (o - off - nb)
        prev = None
        for blk in self._blocks:
            if blk.off <= o < blk.off + blk.nbytes:
                b, y, x, ch, h, w = self._coords(blk, o)
                img = 'image' if blk.fat else 'plane'
                at = '(%s %d, row %d, column %d, channel %d)' % (img, b, y, x, ch)
                if 0 <= y < h and 0 <= x < w:
                    if any(self.block_of(buf) is blk for buf, _, _ in written):
                        return '%s: unwritten channel %d of a destination written at %s' % (blk.name, b if not blk.fat else ch, at)
                    return '%s: source interior written at %s' % (blk.name, at)
                rows = 'row %d%s' % (y, ' (= H)' if y == h else '')
                cols = 'column %d%s' % (x, ' (= W)' if x == w else '')
                edge = rows if not 0 <= y < h else cols
                return '%s: %s of %s %d written, at %s' % (blk.name, edge, img, b, at)
            if blk.off < o:
                prev = blk
        return 'guard bytes between two blocks written, %s' % ('%d bytes behind %s' % (o - prev.off - prev.nbytes, prev.name)
                                                               if prev is not None else 'in front of the first block')

    def assert_finite(self, written):
        """No NaN / inf anywhere in the written regions: no poisoned value was consumed, no output pixel was left unwritten."""
        for buf, c0, c1 in self._norm(written):
            blk = self.block_of(buf)
            r = blk.region(self.slab, c0, c1)
            bad = ~torch.isfinite(r)
            if bool(bad.any()):
                i = [int(v) for v in bad.nonzero()[0]]
                if blk.fat:
                    at = '(image %d, row %d, column %d, channel %d)' % (i[0], i[1], i[2], i[3] + c0)
                else:
                    at = '(plane %d, row %d, column %d)' % (i[0] + c0, i[1], i[2])
                raise GuardError('%s: %s at %s of the written region -- a poisoned value was consumed or the pixel was never written '
                                 '(%d of %d elements)' % (blk.name, float(r[tuple(i)]), at, int(bad.sum()), r.numel()))


# ---- running a test body on either kind of plan -----------------------------------------------------------------------------------
class Record:
    """What the launches of one run of a kernel-test body did: the owner of every launch (demfi_conv_owner, or the *_eligible answer of a
    fused launch) and the bits of every written region.  ``expect``: the record of the plain-Plan run of the same case and seed."""

    def __init__(self, expect=None, launch_only=False):
        self.owners, self.bits = [], []
        self.expect, self.launch_only = expect, launch_only

    def assert_bit_identical(self):
        """(e) the tile walk depends on H, W, batch, never on addresses or pitches: the guarded run stored what the plain run stored."""
        e = self.expect
        assert self.owners == e.owners and len(self.bits) == len(e.bits) > 0
        for i, (a, b) in enumerate(zip(self.bits, e.bits)):
            if not torch.equal(a, b):
                at = [int(v) for v in (a != b).nonzero()[0]]
                raise GuardError('written region %d differs from the plain run at %s (%d of %d elements)' % (i, at, int((a != b).sum()), a.numel()))


def region(buf, c0=0, c1=None):
    return buf[..., c0:c1] if buf.dim() == 4 else buf[c0:c1]


def _bits(written):
    out = []
    for buf, c0, c1 in GuardedPlan._norm(written):
        r = region(buf, c0, c1).contiguous()
        out.append(r.view(torch.int16 if r.element_size() == 2 else torch.int32).cpu())
    return out


def owner(pl, kind, idx):
    d = [C.byref(pl._descs[i]) for i in idx]
    if kind == 'conv':
        return pl.lib.demfi_conv_owner(d[0])
    return getattr(pl.lib, 'demfi_%s_eligible' % kind)(*d)


def prefill(pl, t, value=None):
    """What a destination holds before its launch: ``value`` on a plain Plan (None: whatever it holds); poison on a guarded one."""
    if isinstance(pl, GuardedPlan):
        pl.poison(t)
    elif value is not None:
        t.fill_(value)


def launch(pl, rec, kind, idx, written, stream):
    """pl.launch_<kind>(*idx, stream).  On a guarded plan, in this order: (a) the launch has the owner it has on a plain Plan, (b) nothing
    but ``written`` changed, (c) ``written`` holds no NaN / inf.  The body goes on with (d), its comparison with the reference."""
    guarded = isinstance(pl, GuardedPlan)
    if rec is not None or guarded:
        own = (kind, owner(pl, kind, idx))
        if rec is not None:
            if rec.expect is not None:
                want = rec.expect.owners[len(rec.owners)]
                assert own == want, 'launch %d: %s on pitched views, %s on contiguous ones' % (len(rec.owners), own, want)
            rec.owners.append(own)
    if guarded:
        pl.snapshot()
    getattr(pl, 'launch_' + kind)(*idx, stream)
    if guarded:
        torch.cuda.synchronize()
        pl.check(written)
        pl.assert_finite(written)
    if rec is not None:
        torch.cuda.synchronize()
        rec.bits += _bits(written)
