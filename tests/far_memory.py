"""Hostile ADDRESSES for the kernels  --  TEST INFRASTRUCTURE (not shipped).

``tests/guarded_plan.py`` and ``tests/guarded_arena.py`` vary what lies around a frame; every block of theirs still sits in a few MB.  The engine runs inside one
workspace of tens of GB, and ``demfi_view`` carries int64 strides, while the hot kernels address with "uniform base + one 32-bit lane
offset".  ``FarPlan`` is a ``GuardedPlan``, ``FarArena`` an ``Arena``, inside ONE slab of a little over 10 GiB in which one chosen block
lies FAR:

  * ``cross``: a 2^32-aligned virtual address lies strictly inside the block's frame, in the middle of a middle row (for the zero page and
    the weight blob: in their middle);
  * ``batch``: image k of the block lies k * (2^32 + 4096) bytes behind image 0, and the view's batch stride says so;
  * ``pitch``: the block's row stride (``sy``), record stride (``sx``: the rows then interleave between two records) or, for planar
    blocks, plane stride (``sc``) is a parameter far above the row / record / plane; everything in between is guard memory.

Every other block, the zero page and the weights keep the ordinary guarded layout, directly in front of the far block.  No defect may
fault: a lane offset cut to 32 bits, or sign-extended from 32 bits, still lands inside the slab, because at least 2 GiB of slab lie in
front of the far block and the slab reaches at least 4 GiB past its base (``Space``).

The checks never clone the slab.  ``snapshot()`` copies the frames (small); ``check(written)`` copies them again, compares, poisons every
frame IN PLACE, scans the whole slab for a byte that is not POISON (chunked, a few ms for 10 GiB), and puts the frames back.

Placement is integer arithmetic on a base address, kept in pure functions (``Space``, ``layout``, ``pitch_strides``, ``locate``):
tests/test_far_memory.py checks them with synthetic base pointers and runs the checks on the CPU in a slab with a small period.
"""
import ctypes as C

import torch

from tests import guarded_arena as GA
from tests.guarded_arena import G, GAP, POISON, GuardError
from tests.guarded_plan import GuardedPlan, _Block


class Refused(Exception):
    """A launch answered with an error status (and, checked before this is raised, touched nothing)."""


def _up(v, a):
    return (v + a - 1) // a * a


class Space:
    """The geometry of the slab in units of the boundary period: 2^32 on the GPU, a small power of two in CPU stand-ins."""

    def __init__(self, period=1 << 32):
        assert period & (period - 1) == 0 and period >= 1 << 20
        self.period = period
        self.front = period // 2                      # slab in front of everything: a sign-extended 32-bit offset reaches back this far
        self.near = period // 32                      # room for the ordinary blocks; the far block starts within ``near`` of its anchor
        self.batch_stride = period + 4096
        self.room = 2 * period + self.near            # slab from the anchor of a batch / pitch block on (three items a batch stride apart)
        self.slab_bytes = self.front + 2 * self.near + self.room

    def boundary(self, base):
        """The period-aligned address ``cross`` uses: at least a period (+ the ordinary blocks) of slab in front of it -- an address whose
        carry into the upper half was lost is still inside -- and at least half a period behind it."""
        return _up(base + self.period + 2 * self.near, self.period)

    def anchor(self, base, kind):
        """Where the far block goes (cross: the boundary, the block is laid around it; batch, pitch: its first byte)."""
        return self.boundary(base) if kind == 'cross' else _up(base + self.front + 2 * self.near, 256)

    def near_range(self, base, kind):
        """[start, end) of the ordinary blocks: directly in front of the region the far block may begin in."""
        a = self.anchor(base, kind)
        return _up(a - 2 * self.near, 256), a - self.near - GAP


def contiguous_strides(full, esz):
    out, s = [], esz
    for n in reversed(full):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def span(full, strides, esz):
    return sum((n - 1) * s for n, s in zip(full, strides)) + esz


def layout(space, base, kind, fat, full, esz, param=None):
    """A far block with its guard frame, ``full`` = (B, h+2G, w+2G, C) or (C, h+2G, w+2G): -> (address of its element 0, byte strides).
    param of ``pitch``: (axis, bytes), axis 'sy' / 'sx' (fat) or 'sy' / 'sc' (thin)."""
    st = list(contiguous_strides(full, esz))
    a = space.anchor(base, kind)
    if kind == 'cross':
        FH, FW = (full[1], full[2])
        mid = ((FH // 2) * st[-3] + (FW // 2) * st[-2]) if fat else ((FH // 2) * st[1] + (FW // 2) * st[2])     # image / plane 0
        assert mid < space.near
        return a - _up(mid, 16), tuple(st)            # the boundary falls into the first 16 bytes of pixel (h/2, w/2)
    if kind == 'batch' and fat:
        assert full[0] > 1, 'batch: a block with more than one image'
        st[0] = space.batch_stride
    elif kind == 'batch':
        # a planar block of B images of n = param planes: a [B * n, h, w] tensor has ONE plane stride, so the planes go
        # ceil(batch stride / n) apart and the images n of those: at least the batch stride (GuardedPlan.tview: sb = n planes)
        n = param
        assert n and full[0] % n == 0 and full[0] > n, 'batch: a planar block of several images of n planes'
        st[0] = _up(-(-space.batch_stride // n), 256)
    elif kind == 'pitch':
        axis, S = param
        assert S % 256 == 0
        if fat:
            B, FH, FW, Cc = full
            if axis == 'sy':
                assert S >= FW * Cc * esz + GAP
                st = [FH * S, S, Cc * esz, esz]
            else:
                assert axis == 'sx'
                slot = _up(Cc * esz, 256) + GAP       # the records of one column, row after row and image after image, poison between them
                assert B * FH * slot + GAP <= S
                st = [FH * slot, slot, S, esz]
        else:
            Cc, FH, FW = full
            if axis == 'sy':
                slot = _up(FW * esz, 256) + GAP        # row y of every plane, plane after plane, poison between them; then row y + 1
                assert Cc * slot + GAP <= S
                st = [slot, S, esz]
            else:
                assert axis == 'sc' and S >= FH * FW * esz + GAP
                st = [S, FW * esz, esz]
    else:
        raise ValueError(kind)
    assert span(full, st, esz) <= space.room, 'the far block of %d bytes does not fit' % span(full, st, esz)
    return a, tuple(st)


def pitch_strides(extent, period=1 << 32):
    """Three strides in bytes (multiples of 256) for a kernel whose largest lane offset inside one tile is ``extent`` strides: the offset
    lies below period / 2 (at three quarters of it: the family's own kernel still owns the view, at a wide stride), in [period / 2,
    period), and at or above period."""
    lo = (period // 8 * 3) // extent // 256 * 256
    mid = _up(-(-(period // 2) // extent), 256)
    hi = _up(-(-period // extent), 256)
    return lo, mid, hi


def offset_class(nbytes, period=1 << 32):
    return 'lt31' if nbytes < period // 2 else ('31to32' if nbytes < period else 'ge32')


def locate(full, strides, esz, rel):
    """Byte ``rel`` of a block -> (index per dimension, None) if it belongs to an element (frame or guard), or (indices so far, the
    dimension in whose gap it lies).  Greedy from the largest stride down: strides need not be ordered like the dimensions."""
    idx, r = [0] * len(full), rel
    for d in sorted(range(len(full)), key=lambda k: -strides[k]):
        idx[d], r = r // strides[d], r % strides[d]
        if idx[d] >= full[d]:
            return idx, d
    return (idx, None) if r < esz else (idx, len(full))


def inside(lo, hi):
    """The byte of [lo, hi) -- a row of a frame, an item -- that goes to the boundary: the multiple of 16 nearest to the middle that lies
    strictly inside (pointers keep their alignment); a range too short to hold one starts at the boundary."""
    c = [v for v in range(_up(lo + 1, 16), hi - 1, 16)]
    return min(c, key=lambda v: abs(v - (lo + hi) // 2)) if c else (_up(lo, 16) if _up(lo, 16) < hi else lo // 16 * 16)


def first_nonpoison(slab, chunk=256 << 20):
    """Offset of the first byte of a uint8 tensor that is not POISON, or None.  One reduction per chunk, one synchronisation."""
    n = slab.numel()
    assert slab.data_ptr() % 8 == 0 and n % 8 == 0 and chunk % 8 == 0
    words = slab.view(torch.int64)
    parts = [(o, min(chunk // 8, n // 8 - o)) for o in range(0, n // 8, chunk // 8)]
    flags = torch.stack([(words[o:o + m] != -1).any() for o, m in parts]).cpu()
    for (o, m), f in zip(parts, flags):
        if bool(f):
            j = o + int((words[o:o + m] != -1).nonzero()[0])
            return j * 8 + int((slab[j * 8:j * 8 + 8] != POISON).nonzero()[0])
    return None


class _FarBlock(_Block):
    __slots__ = ('strides', 'far')

    def __init__(self, name, fat, off, full, dtype, strides, far):
        esz = torch.empty((), dtype=dtype).element_size()
        super().__init__(name, fat, off, span(full, strides, esz), tuple(full), dtype, None)
        self.strides, self.far = tuple(strides), far

    def of(self, slab):
        esz = torch.empty((), dtype=self.dtype).element_size()
        return torch.as_strided(slab.view(self.dtype), self.full, [s // esz for s in self.strides], self.off // esz)


class FarPlan(GuardedPlan):
    """far: None (every block ordinary) or (kind, which, param): which = the index of the _fat / _thin call, 'zero page' or 'weights'
    (cross only)."""

    def __init__(self, H, W, dtype=torch.float16, device='cuda:0', state_dict=None, slab=None, space=None, far=None):
        self.space = space or Space()
        assert slab is not None and slab.numel() >= self.space.slab_bytes and slab.data_ptr() % 8 == 0
        super().__init__(H, W, dtype, device, state_dict, slab=slab)
        self.far = far
        self.gate_agnostic = bool(far) and far[0] == 'pitch'       # the owner is whatever the gates say at that stride
        self.base = slab.data_ptr()
        kind = far[0] if far else 'cross'
        lo, hi = self.space.near_range(self.base, kind)
        self._cur, self._near_end = lo - self.base + GAP, hi - self.base
        self._n_spans = 0
        self.far_block = None
        self.boundary = self.space.boundary(self.base)

    # ---- memory ------------------------------------------------------------------------------------------------------------------
    def _near(self, nbytes):
        off = self._cur
        self._cur = ((off + nbytes + 255) & ~255) + GAP
        if self._cur > self._near_end:
            raise MemoryError('FarPlan: the ordinary blocks do not fit in front of the far block')
        return off

    def _alloc(self, nbytes):
        # GuardedPlan._upload allocates the zero page (256 bytes), then the weight blob, and nothing else goes through _alloc here (blocks
        # go through _block): told apart by order, which the assertions pin
        assert self._n_spans < 2, 'GuardedPlan allocates something FarPlan does not know'
        what = ('zero page', 'weights')[self._n_spans]
        assert what != 'zero page' or nbytes == 256
        self._n_spans += 1
        if self.far and self.far[1] == what:
            assert self.far[0] == 'cross'
            self.far_block = what
            return self.boundary - self.base - _up(nbytes // 2, 16)
        return self._near(nbytes)

    def _block(self, fat, full, dtype, inner):
        esz = torch.empty((), dtype=dtype).element_size()
        k = len(self._blocks)
        far = bool(self.far) and self.far[1] == k
        if far:
            addr, st = layout(self.space, self.base, self.far[0], fat, tuple(full), esz, self.far[2])
            off = addr - self.base
        else:
            st = contiguous_strides(full, esz)
            off = self._near(span(full, st, esz))
        name = 'buffer %d (%s%s %s)' % (k, 'FAR ' if far else '', 'fat' if fat else 'thin', list(inner))
        blk = _FarBlock(name, fat, off, full, dtype, st, (self.far[2][0] if self.far[0] == 'pitch' else self.far[0]) if far else False)
        assert 0 <= blk.off and blk.off + blk.nbytes <= self.slab.numel()
        t = blk.region(self.slab)
        blk.key = t.data_ptr()
        self._blocks.append(blk)
        self._by_key[blk.key] = blk
        if far:
            self.far_block = blk
        return t

    def assert_crosses(self):
        """cross: the boundary is a multiple of the period with the margins of ``Space`` and lies strictly inside the far frame, inside a
        middle row -- from data_ptr() arithmetic on the tensors the kernels get."""
        A, sp = self.boundary, self.space
        assert A % sp.period == 0 and A - self.base >= sp.period and self.base + self.slab.numel() - A >= sp.front
        blk = self.far_block
        if isinstance(blk, str):
            t = self.zero_page if blk == 'zero page' else self.weight_blob
            assert t.data_ptr() < A < t.data_ptr() + t.numel() - 1
            return
        r = blk.region(self.slab)
        r = r[0]                                      # image / plane 0: [h, w, C] or [h, w]
        h, w = r.shape[0], r.shape[1]
        row = r[h // 2]
        first, last = row[0].data_ptr(), row[w - 1].data_ptr() + row[w - 1].numel() * r.element_size() - 1
        assert 0 < h // 2 < h - 1 or h < 3
        assert first < A < last, (first, A, last)

    # ---- launches: an error status is a refusal, and a refusal touches nothing ---------------------------------------------------------------
    def _status(self, st, what):
        if st < 0:
            if self.device.type == 'cuda':
                torch.cuda.synchronize()
            self.check(())
            raise Refused(what)

    def launch_conv(self, i, stream, what='conv'):
        self._status(self.lib.demfi_conv2d(C.byref(self._descs[i]), self.desc_dev.data_ptr() + i * self._desc_sz, stream), what)

    def launch_resblock(self, i1, i2, stream, what='resblock'):
        self._status(self.lib.demfi_resblock3x3_c64(C.byref(self._descs[i1]), C.byref(self._descs[i2]), stream), what)

    def launch_gru_r(self, i, stream, what='gru_r'):
        self._status(self.lib.demfi_gru_r(C.byref(self._descs[i]), stream), what)

    def launch_gru_zq(self, iz, iq, stream, what='gru_zq'):
        self._status(self.lib.demfi_gru_zq(C.byref(self._descs[iz]), C.byref(self._descs[iq]), stream), what)

    # ---- who reads and writes which block ------------------------------------------------------------------------------------------------
    def operands(self):
        """{block index: roles} over every descriptor: 'src' (a piece), 'dst', 'res', 'aux', 'pack'; {index: True if batched}."""
        roles, batched = {}, {}                     # batched: False, True (NHWC images) or n (a planar block of images of n planes)

        def hit(v, role):
            if not v.ptr:
                return
            for k, blk in enumerate(self._blocks):
                if self.base + blk.off <= v.ptr < self.base + blk.off + blk.nbytes:
                    roles.setdefault(k, set()).add(role)
                    if v.sb != 0 and blk.fat and blk.full[0] > 1:
                        batched[k] = True
                    elif v.sb != 0 and not blk.fat and v.sc and 0 < v.sb // v.sc < blk.full[0]:
                        batched[k] = int(v.sb // v.sc)
                    else:
                        batched.setdefault(k, False)
                    return
            raise AssertionError('a %s view points at no block' % role)

        for d in self._descs:
            for i in range(d.n_pieces):
                hit(d.pieces[i].v, 'src')
            for i in range(d.n_segs):
                hit(d.segs[i].dst, 'dst')
                hit(d.segs[i].res, 'res')
                hit(d.segs[i].aux, 'aux')
            hit(d.pack, 'pack')
        return roles, batched

    # ---- the checks ------------------------------------------------------------------------------------------------------------------------
    def _frames(self):
        return [blk.region(self.slab) for blk in self._blocks] + [self.slab[o:o + n] for o, n, _ in self._spans]

    def snapshot(self):
        self._snap = [f.clone(memory_format=torch.contiguous_format) for f in self._frames()]

    def check(self, written=()):
        """Outside the frames every byte of the slab is POISON; every frame (and span) but the channel / plane ranges in ``written`` holds
        what it held at the last snapshot."""
        assert self._snap is not None, 'check() without snapshot()'
        written = self._norm(written)
        frames = self._frames()
        assert len(frames) == len(self._snap), 'blocks were added after snapshot()'
        now = [f.clone(memory_format=torch.contiguous_format) for f in frames]
        for f in frames:
            _ints(f).fill_(-1 if f.element_size() > 1 else POISON)
        o = first_nonpoison(self.slab)
        for f, n in zip(frames, now):
            f.copy_(n)
        if o is not None:
            raise GuardError(self._where(o, written) + ' (byte %d of the slab)' % o)
        for i, (n, s) in enumerate(zip(now, self._snap)):
            blk = self._blocks[i] if i < len(self._blocks) else None
            mine = [(c0, c1) for buf, c0, c1 in written if blk is not None and self.block_of(buf) is blk]
            for c0, c1 in mine:
                (n[..., c0:c1] if blk.fat else n[c0:c1]).copy_(s[..., c0:c1] if blk.fat else s[c0:c1])
            diff = _ints(n) != _ints(s)
            if not bool(diff.any()):
                continue
            at = [int(v) for v in diff.nonzero()[0]]
            if blk is None:
                raise GuardError('%s written at byte %d' % (self._spans[i - len(self._blocks)][2], at[0]))
            if blk.fat:
                where = '(image %d, row %d, column %d, channel %d)' % tuple(at)
                what = 'unwritten channel %d of a destination' % at[3] if mine else 'source interior'
            else:
                where = '(plane %d, row %d, column %d, channel 0)' % tuple(at)
                what = 'unwritten channel %d of a destination' % at[0] if mine else 'source interior'
            raise GuardError('%s: %s written at %s' % (blk.name, what, where))

    def _where(self, o, written):
        """A byte outside every frame."""
        for off, nb, what in self._spans:
            if off + nb <= o < off + nb + GAP:
                return 'byte %d behind %s written' % (o - off - nb, what)
        prev = None
        for blk in self._blocks:
            if blk.off <= o < blk.off + blk.nbytes:
                esz = torch.empty((), dtype=blk.dtype).element_size()
                idx, gap = locate(blk.full, blk.strides, esz, o - blk.off)
                names = ('image', 'row', 'column', 'channel') if blk.fat else ('plane', 'row', 'column')
                FH, FW = (blk.full[1], blk.full[2])
                h, w = FH - 2 * G, FW - 2 * G
                rel = list(idx)
                rel[1], rel[2] = idx[1] - G, idx[2] - G
                at = '(%s)' % ', '.join('%s %d' % (nm, v) for nm, v in zip(names, rel))
                if gap is not None:
                    unit = {'sx': 'far records', 'sc': 'far planes', 'batch': 'far images'}.get(blk.far, 'far rows') if blk.far else 'elements'
                    return '%s: a store between %s, behind %s' % (blk.name, unit, at)
                y, x = rel[1], rel[2]
                rows = 'row %d%s' % (y, ' (= H)' if y == h else '')
                cols = 'column %d%s' % (x, ' (= W)' if x == w else '')
                edge = rows if not 0 <= y < h else cols
                return '%s: %s of %s %d written (guard %s), at %s' % (blk.name, edge, names[0], idx[0], 'rows' if not 0 <= y < h else 'columns', at)
            if blk.off < o and not blk.far:
                prev = blk
        return 'guard bytes between two blocks written, %s' % ('%d bytes behind %s' % (o - prev.off - prev.nbytes, prev.name)
                                                               if prev is not None and o - prev.off - prev.nbytes < (1 << 20)
                                                               else 'far from every block')


def plan_factory(slab, space=None, far=None, made=None):
    """What a test body takes for its plan class: FarPlan in ``slab`` with one far block.  made: a list that collects the plans."""
    def make(H, W, dtype=torch.float16, device='cuda:0', state_dict=None):
        pl = FarPlan(H, W, dtype, device, state_dict, slab=slab, space=space, far=far)
        if made is not None:
            made.append(pl)
        return pl
    return make


# ---- the pitch cases ----------------------------------------------------------------------------------------------------------------------
# family -> src: (rows, columns) = the largest multiples of sy and sx that one tile / window adds to its base address when it reads a
# source; out: the same for the destination and residual tile; sy_hw / sx_hw: the frame of the row-stride and of the record-stride cases.
# c64: conv_c64.hip, P_LH x P_LW = (TH + 2) x (TW + 2) window read from pixel (-2, -2) (NCO 2) or (-1, -1) (NCO 1), TH x TW outputs.  The
# others: the multipliers of the family's own eligibility bound in bytes (conv.hip, conv_sep.hip, conv_wstream.hip, wsconv.hip: an upper
# bound of what a tile reaches; wsconv.hip multiplies a lane's column of the whole padded row by the destination's sx), and for the
# general kernel the whole image, which is what its 32-bit fast path of interior tiles measures (19x75 has an interior 5x5 tile).
PITCH_FAMILIES = {
    'c64_nco2': dict(src=(10, 34), out=(7, 31), sy_hw=(11, 45), sx_hw=(13, 45)),
    'c64_nco1': dict(src=(9, 33), out=(7, 31), sy_hw=(9, 45), sx_hw=(13, 45)),
    'general_f32': dict(src=(19, 75), out=(7, 31), sy_hw=(19, 75), sx_hw=(19, 75)),
    'narrow_nhwc': dict(src=(16, 64), out=(7, 31), sy_hw=(19, 75), sx_hw=(19, 75)),
    'sep_1x5': dict(src=(40, 40), out=(7, 31), sy_hw=(37, 45), sx_hw=(37, 45)),
    'sep_5x1': dict(src=(40, 40), out=(7, 31), sy_hw=(37, 45), sx_hw=(37, 45)),
    'wstream7': dict(src=(40, 48), out=(15, 31), sy_hw=(16, 45), sx_hw=(16, 45)),
    'ws2_units': dict(src=(80, 80), out=(7, 63), sy_hw=(16, 46), sx_hw=(16, 46)),
    # the fused launches: the multipliers of resblock.hip's and gru.hip's own bounds (source window and destination alike)
    'fused_resblock': dict(src=(20, 40), out=(20, 40), sy_hw=(16, 30), sx_hw=(16, 30)),
    'gru_1x5': dict(src=(24, 40), out=(24, 40), sy_hw=(8, 32), sx_hw=(8, 32)),
    'gru_5x1': dict(src=(24, 40), out=(24, 40), sy_hw=(8, 32), sx_hw=(8, 32)),
    # planar fp32 destinations and residuals (three planes each): their row stride and, in place of sx, their PLANE stride (sc)
    'narrow_thin': dict(src=(16, 64), out=(7, 31), sy_hw=(11, 75), sx_hw=(19, 75)),
    'thin_packed_copy': dict(src=(16, 64), out=(7, 31), sy_hw=(11, 75), sx_hw=(19, 75)),      # + the packed NHWC record (no gate looks at it)
    'narrow_7x7': dict(src=(16, 64), out=(7, 31), sy_hw=(19, 75), sx_hw=(19, 75)),            # 14 x 38 window under the 16 / 64 bound
    # wsconv.hip's 32-cout form and, where it declines, the 3x3 streamed-weight kernel (40 / 48): two pieces of different record strides
    'rdb_growth': dict(src=(80, 80), out=(7, 63), sy_hw=(16, 46), sx_hw=(16, 46)),
    'ws2_stride2': dict(src=(80, 80), out=(7, 63), sy_hw=(8, 40), sx_hw=(8, 40)),             # the sources are 2H x 2W
    'ws2_two_piece_tail': dict(src=(80, 80), out=(7, 63), sy_hw=(16, 46), sx_hw=(16, 46)),    # + the second piece's own bound
    # planar and upsampled pieces, PixelShuffle and GRU routing on the general kernel (fp32) / its owners (fp16): the whole 16x32 image
    'routing_f32': dict(src=(16, 32), out=(16, 32), sy_hw=(16, 32), sx_hw=(16, 32)),
    'routing_f16': dict(src=(16, 32), out=(16, 32), sy_hw=(16, 32), sx_hw=(16, 32)),
}


def thin_pitch_cases(family, axis, planes, space=None, full=None):
    """The same for a planar block of ``planes`` planes: [(axis, stride, 'out', class)].  axis 'sy': the output tile's rows; axis 'sx'
    stands for the plane stride 'sc', of which the last plane lies planes - 1 away from the view's pointer."""
    space = space or Space()
    fam = PITCH_FAMILIES[family]
    h, w = fam[axis + '_hw'] if full is None else (full[1] - 2 * G, full[2] - 2 * G)
    if axis != 'sy' and planes < 2:
        return []                                     # one plane has no plane stride
    ext = fam['out'][0] if axis == 'sy' else planes - 1
    reach = (h + 2 * G) if axis == 'sy' else planes - 1
    return [('sy' if axis == 'sy' else 'sc', S, 'out', offset_class(ext * S, space.period))
            for S in pitch_strides(ext, space.period) if reach * S + (h + 2 * G) * (w + 2 * G) * 4 <= space.room]


def pitch_cases(family, axis, space=None, full=None):
    """[(stride in bytes, operand kind whose extent chose it, class of that operand's largest lane offset)]: three classes from the source
    extent, and those of the output extent whose block still fits into the slab (an 8-row tile reaches 2^32 only at strides of which
    H + 2G rows are more than the slab)."""
    space = space or Space()
    fam = PITCH_FAMILIES[family]
    h, w = fam[axis + '_hw']
    lines = (h if axis == 'sy' else w) + 2 * G
    if full is not None:                              # the block's own frame with guards (a 2H x 2W source, an H/2 x W/2 piece)
        lines = full[1] if axis == 'sy' else full[2]
    out = []
    for kind in ('src', 'out'):
        ext = fam[kind][0 if axis == 'sy' else 1]
        for S in pitch_strides(ext, space.period):
            if lines * S <= space.room and S not in [s for s, _, _ in out]:
                out.append((S, kind, offset_class(ext * S, space.period)))
    return out


class FarArena(GA.Arena):
    """``Arena`` in the far slab.  far: None or (kind, k): allocation k (in the order of the fat / thin / flat calls) is laid across the
    boundary ('cross': a middle row of image / plane / item 0) or has its images / copies / items a batch stride apart ('batch')."""

    def __init__(self, device, slab, space=None, far=None):
        # Arena.__init__ is NOT called: it would allocate a slab of its own.  Every field it sets is set here; the assertion below fails
        # when Arena gains one.
        self.space = space or Space()
        assert slab.numel() >= self.space.slab_bytes and slab.data_ptr() % 8 == 0
        self.device = torch.device(device)
        self.slab = slab.fill_(POISON)
        self.base = slab.data_ptr()
        self.far = far
        lo, hi = self.space.near_range(self.base, far[0] if far else 'cross')
        self._cur, self._near_end = lo - self.base + GAP, hi - self.base
        self._blocks, self._frames, self._snap = [], [], None
        self.counts = []                              # per allocation: its images / copies (planes) / items -- what 'batch' can spread
        self.recording, self.bits = True, []
        self.boundary = self.space.boundary(self.base)
        self.far_block = self.far_frame = None
        assert set(vars(GA.Arena('cpu', 4096))) <= set(vars(self)), 'Arena has a field FarArena does not set'

    def _alloc(self, nbytes):
        off = self._cur
        self._cur = ((off + nbytes + 255) & ~255) + GAP
        if self._cur > self._near_end:
            raise MemoryError('FarArena: the ordinary blocks do not fit in front of the far block')
        return off

    def _far_block(self, kind, label, name, full, dtype, mid, dim):
        """The far allocation: -> (block, byte strides of ``full``).  mid: byte of image / plane / item 0 the boundary goes to;
        dim: the dimension of ``full`` that counts images / copies (planar block without copies: planes) / items: what 'batch' spreads."""
        esz = GA._esz(dtype)
        st = list(contiguous_strides(full, esz))
        a = self.space.anchor(self.base, self.far[0])
        if self.far[0] == 'cross':
            a -= mid
        else:
            assert self.far[0] == 'batch' and full[dim] > 1, 'batch: a block of several images / copies / planes / items'
            st[dim] = self.space.batch_stride
            for d in range(dim - 1, -1, -1):
                st[d] = st[d + 1] * full[d + 1]
        nbytes = span(full, st, esz)
        assert nbytes <= self.space.room and a - self.base + nbytes <= self.slab.numel()
        blk = GA._Block('block %d%s (FAR %s %s)' % (len(self._blocks), ' "%s"' % name if name else '', kind, label), kind, a - self.base, nbytes,
                        tuple(full), dtype)
        self.far_strides = tuple(st)
        self._blocks.append(blk)
        self.far_block = blk
        return blk, [v // esz for v in st]

    def _is_far(self):
        return bool(self.far) and self.far[1] == len(self._blocks)

    def fat(self, B, h, w, C, dtype, name=None):
        if not self._is_far():
            t = super().fat(B, h, w, C, dtype, name)
        else:
            FH, FW, esz = h + 2 * G, w + 2 * G, GA._esz(dtype)
            row = ((G + h // 2) * FW + G) * C * esz
            blk, st = self._far_block('fat', [B, h, w, C], name, (B, FH, FW, C), dtype, inside(row, row + w * C * esz), 0)
            t = self._view(self.slab, blk.off + (G * FW + G) * C * esz, (B, h, w, C), st, dtype)
            self.far_frame = t
        self._frames.append(t)
        self.counts.append(B)
        return t

    def thin(self, C, h, w, n=None, name=None):
        if not self._is_far():
            t = super().thin(C, h, w, n, name)
        else:
            FH, FW = h + 2 * G, w + 2 * G
            row = ((G + h // 2) * FW + G) * 4
            blk, st = self._far_block('thin', [C * (n or 1), h, w], name, (n or 1, C, FH, FW), torch.float32, inside(row, row + w * 4),
                                      0 if n is not None else 1)
            if self.far[0] == 'cross':
                blk.full = (C * (n or 1), FH, FW)     # contiguous: Arena._where reads it like any thin block
            t = self._view(self.slab, blk.off + (G * FW + G) * 4, (n or 1, C, h, w), st, torch.float32)
            self.far_frame = t
            t = t if n is not None else t[0]
        self._frames.append(t)
        self.counts.append(n if n is not None else C)
        return t

    def flat(self, n, shape, dtype, zero=False, name=None):
        if not self._is_far():
            t = super().flat(n, shape, dtype, zero, name)
        else:
            shape = tuple(int(v) for v in shape)
            full = (n,) + shape
            item = span(shape, contiguous_strides(shape, GA._esz(dtype)), GA._esz(dtype)) if shape else GA._esz(dtype)
            blk, st = self._far_block('flat', list(full), name, full, dtype, inside(0, item), 0)
            if self.far[0] == 'cross':                # the items keep the stride of an ordinary flat block: poison between them
                st[0] = (((item + 255) & ~255) + GAP) // GA._esz(dtype)
                blk.nbytes = (n - 1) * st[0] * GA._esz(dtype) + item
            blk.item, blk.stride = item, st[0] * GA._esz(dtype)
            t = self._view(self.slab, blk.off, full, st, dtype)
            if zero:
                t.zero_()
            self.far_frame = t
        self._frames.append(t)
        self.counts.append(n)
        return t

    def assert_far(self):
        """cross: the boundary lies strictly inside image / plane / item 0 of the far tensor, for views inside a middle row; batch: item k
        lies k * (period + 4096) bytes behind item 0.  From data_ptr() arithmetic on the tensor the kernels get."""
        t, blk = self.far_frame, self.far_block
        assert t is not None, 'no allocation %r' % (self.far[1],)
        if self.far[0] == 'batch':
            if blk.kind == 'thin' and t.shape[0] == 1:
                t = t[0]                               # a planar block without copies: its planes
            assert t.shape[0] > 1 and all(t[k].data_ptr() - t[0].data_ptr() == k * self.space.batch_stride for k in range(t.shape[0]))
            return
        A = self.boundary
        assert A % self.space.period == 0 and A - self.base >= self.space.period and self.base + self.slab.numel() - A >= self.space.front
        if blk.kind == 'flat':
            first, last = t[0].data_ptr(), t[0].data_ptr() + blk.item - 1
        else:
            r = t[0] if blk.kind == 'fat' else t[0, 0]     # [h, w, C] or [h, w]
            h, w = r.shape[0], r.shape[1]
            row = r[h // 2]
            first, last = row[0].data_ptr(), row[w - 1].data_ptr() + row[w - 1].numel() * r.element_size() - 1
        assert first < A < last or (last - first < 32 and first - 16 < A <= last), (first, A, last)       # (32 bytes may hold no multiple of 16)

    # ---- the checks: frames are copied, the slab is scanned in place --------------------------------------------------------------------------
    def snapshot(self):
        self._snap = [f.clone(memory_format=torch.contiguous_format) for f in self._frames]

    def check(self, written=()):
        assert self._snap is not None and len(self._snap) == len(self._frames), 'check() without snapshot()'
        frames = self._frames
        mine = [t.clone(memory_format=torch.contiguous_format) for t in written]
        now = [f.clone(memory_format=torch.contiguous_format) for f in frames]
        for f in frames:
            _ints(f).fill_(-1 if f.element_size() > 1 else POISON)
        o = first_nonpoison(self.slab)
        if o is None:
            for f, s in zip(frames, self._snap):       # the state of the snapshot ...
                _ints(f).copy_(_ints(s))
            for t, m in zip(written, mine):            # ... plus what the launch may write: that is what the frames must hold now
                _ints(t).copy_(_ints(m))
            bad = [(i, _ints(f) != _ints(n)) for i, (f, n) in enumerate(zip(frames, now))]
            bad = [(i, d) for i, d in bad if bool(d.any())]
        for f, n in zip(frames, now):
            _ints(f).copy_(_ints(n))
        if o is not None:
            raise GuardError(self._where(o, written) + ' (byte %d of the slab)' % o)
        if bad:
            i, d = bad[0]
            blk = self._blocks[i]
            what = 'a part of a destination that the launch does not own' if self._is_dest(blk, written) else 'source interior'
            raise GuardError('%s: %s written at index %s' % (blk.name, what, [int(v) for v in d.nonzero()[0]]))

    def _where(self, o, written):
        blk = self.far_block
        if blk is not None and blk.off <= o < blk.off + blk.nbytes and self.far[0] == 'batch':
            idx, gap = locate(blk.full, self.far_strides, GA._esz(blk.dtype), o - blk.off)
            return '%s: %s index %s' % (blk.name, 'a store between far items, behind' if gap is not None else 'a guard element written at', idx)
        if blk is not None and o >= blk.off + blk.nbytes:
            return 'guard bytes written %d bytes behind %s' % (o - blk.off - blk.nbytes, blk.name)
        return super()._where(o, written)


_INT_VIEWS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _ints(t):                                         # (also 8-byte elements: the arena's int64 / float64 items)
    return t.view(_INT_VIEWS[t.element_size()])
