"""CPU interpreter of a launch plan  --  TEST INFRASTRUCTURE (not shipped, not a fallback).

Builds nothing itself: it takes an ``Engine`` whose context was bound to HOST memory (``device='cpu'``: same descriptors,
same packed weight blob the GPU would get, built by the C++ planner in demfi_amd/csrc/plan.cpp) or a ``Plan`` on CPU
tensors, and *interprets* every ``demfi_conv`` descriptor and pointwise op with torch CPU ops, following the semantics
documented in include/demfi_hip.h.  Purpose: check the host logic (channel maps, chunking, weight repack, output
routing, buffer wiring) against the oracle without a GPU, so that a mismatch on the GPU box isolates the HIP kernels.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from demfi_amd import _lib as L
from demfi_amd.engine import SEG_TRUNK, SEG_HEAD, SEG_ITER
from oracle import demfi_oracle as O


class Out:
    """One stored tensor of an op as precise mode returns it.  off: byte offset of every element from the workspace base (int64 array
    of the value's shape); dtype: the type it is stored in; kind says which attributes carry the value:
      'epi'     v, S (and res, z, vz, Sz), act, mode -- the ingredients of the epilogue_ref references; widen for a fused residual block
      'motion'  ref, bound (units of 2^-23, tests/motion_ref.py), k, optionally exact_zero
      'sum'     ref, terms (sum of |term|), n (number of fp32 roundings)
      'exact'   ref: the stored value itself
      'mirror'  src, src_dtype: the element must be the value the op stored at byte offset src, rounded to dtype."""

    def __init__(self, name, kind, off, dtype, **kw):
        self.name, self.kind, self.off, self.dtype = name, kind, off, dtype
        self.__dict__.update(kw)


class PlanSim:
    """precise=False: every op is interpreted in fp32 with torch CPU ops and its result STORED, as the path dtype would store it.

    precise=True (tests/plan_replay.py): every op is evaluated in float64 from the bytes currently in the workspace -- operands read
    as stored (fp16 or fp32), nothing rounded except where the kernel's semantics round (fp16 staging of planar fp32 pieces, the fp16
    intermediate of a fused residual block; the z of gru_zq is NOT rounded, epilogue_ref.ref_zq) -- and the result is RETURNED by
    ``run`` as a list of ``Out`` records instead of being stored: the float64 ingredients per output element and, for
    convolution-type ops, S = conv(|x|, |w|) + |b| for epilogue_ref.bound.

    Either way the interpreter records every byte of the engine's workspace it reads and every byte it writes (``begin_record`` /
    ``end_record``): the read set and the write set of an op as the reference interpreter sees them, not a hand-written table."""

    def __init__(self, eng, precise=False, z_on_chip=False, round_mid=True):
        """z_on_chip: default mode keeps the z of gru_zq in fp32, as the kernel does (the default rounds it to fp16, as the two-launch
        form stored it).  round_mid=False: the intermediate of a fused residual block is NOT rounded to fp16 -- a wrong kernel, for the
        harness's own tests."""
        self.e = eng
        self.precise, self.z_on_chip, self.round_mid = precise, z_on_chip, round_mid
        self.reg = []
        for t in eng.regions():
            self.reg.append((t.data_ptr(), t.numel() * t.element_size(), t))
        self._rec = None
        self._wcache = {}
        self._raw_piece = None                                   # round_mid=False: the piece that is NOT rounded when it is staged

    # ---- access record ---------------------------------------------------------------------------------------------
    def begin_record(self, lo=0):
        """Start recording accesses to the engine's workspace as two byte masks over [lo, nbytes) from the workspace base (lo a multiple
        of 4; accesses in front of lo -- weights, zero page -- are not recorded)."""
        n = self.e.workspace.numel() - 256
        assert n % 4 == 0 and lo % 4 == 0
        self._rec_base = self.e._base + lo
        self._rec = (np.zeros(n - lo, np.uint8), np.zeros(n - lo, np.uint8))

    def end_record(self):
        """(read mask, write mask): bool arrays, one entry per byte of [lo, nbytes)."""
        r, w = self._rec
        self._rec = None
        return r.view(np.bool_), w.view(np.bool_)

    def _note(self, write, ptr, esz, shape, strides):
        """Record one strided access: elements of esz bytes at ptr + esz * sum(i_k * strides_k), i_k < shape_k."""
        if self._rec is None:
            return
        lo = ptr - self._rec_base
        m = self._rec[1 if write else 0]
        if not 0 <= lo < m.size:
            return                                               # in front of the record, or private memory of the interpreter (a fused op's intermediate)
        assert lo % esz == 0
        idx = np.full((1,) * len(shape), lo // esz, np.int64)
        for k, (n, st) in enumerate(zip(shape, strides)):
            sh = [1] * len(shape)
            sh[k] = n
            idx = idx + (np.arange(n, dtype=np.int64) * st).reshape(sh)
        assert idx.min() >= 0 and (int(idx.max()) + 1) * esz <= m.size, 'access outside the workspace'
        m.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[esz])[idx.ravel()] = {1: 1, 2: 0x0101, 4: 0x01010101}[esz]

    def note_read(self, ptr, nbytes):
        self._note(False, ptr, 1, (nbytes,), (1,))

    def note_write(self, ptr, nbytes):
        self._note(True, ptr, 1, (nbytes,), (1,))

    def offsets(self, v, nch, H, W, b=0):
        """Byte offsets from the workspace base of the elements of a view, int64 [nch,H,W]."""
        esz = 4 if v.is_f32 else 2
        lo = v.ptr - self.e._base + b * v.sb * esz
        return lo + esz * (np.arange(nch, dtype=np.int64)[:, None, None] * v.sc + np.arange(H, dtype=np.int64)[None, :, None] * v.sy
                           + np.arange(W, dtype=np.int64)[None, None, :] * v.sx)

    # ---- raw memory access through device-pointer arithmetic ----------------------------------------
    def _flat(self, ptr, is_f32):
        for base, nb, t in self.reg:
            if base <= ptr < base + nb:
                dt = torch.float32 if is_f32 else torch.float16
                assert t.dtype == dt or t.dtype == torch.uint8, (t.dtype, dt)
                flat = t.view(-1)
                if t.dtype == torch.uint8:
                    flat = flat.view(dt)
                esz = 4 if is_f32 else 2
                assert (ptr - base) % esz == 0
                return flat, (ptr - base) // esz
        raise KeyError('pointer %x not inside any engine buffer' % ptr)

    def strided(self, v, nch, H, W, b=0, write=False):
        """A [nch,H,W] view of memory; the access is recorded as a read, or as a write with write=True (``written``)."""
        flat, off = self._flat(v.ptr, v.is_f32)
        esz = 4 if v.is_f32 else 2
        self._note(write, v.ptr + b * v.sb * esz, esz, (nch, H, W), (v.sc, v.sy, v.sx))
        return torch.as_strided(flat, (nch, H, W), (v.sc, v.sy, v.sx), off + b * v.sb)

    def written(self, v, nch, H, W, b=0):
        return self.strided(v, nch, H, W, b, write=True)

    # ---- one convolution descriptor ---------------------------------------------------------------------
    def unpack_weights(self, d):
        """[cout_pad, K, kh, kw] fp32 from the packed blob; kept per blob address (the weights of a bound plan never change)."""
        key = (d.wpack, d.cout_pad, d.n_chunks, d.kh, d.kw, d.nco)
        if key not in self._wcache:
            self._wcache[key] = self._unpack_weights(d)
        return self._wcache[key]

    def _unpack_weights(self, d):
        f32 = d.dtype == L.F32
        cpk, half = (8, 4) if f32 else (16, 8)
        taps = d.kh * d.kw
        nks = [d.chunks[c].nks for c in range(d.n_chunks)]
        n_k = sum(nks) * cpk
        nblk = d.cout_pad // (32 * d.nco)
        flat, off = self._flat(d.wpack, f32)
        per16 = 4 if f32 else 8
        Wp = torch.zeros(d.cout_pad, n_k, taps)
        lanes = torch.arange(64)
        for blk in range(nblk):
            kbase = 0
            for c in range(d.n_chunks):
                vb = blk * d.w_blk_stride + d.chunks[c].w_off
                n = nks[c] * taps * d.nco * 64
                self.note_read(d.wpack + vb * 16, n * 16)
                blk_w = flat[off + vb * per16: off + (vb + n) * per16].float().view(taps, nks[c], d.nco, 64, half)
                for s in range(d.nco):
                    co = (blk * d.nco + s) * 32 + (lanes & 31)                      # [64]
                    for ks in range(nks[c]):
                        kp = kbase + ks * cpk + (lanes >> 5)[:, None] * half + torch.arange(half)[None]   # [64,half]
                        Wp[co[:, None].expand(64, half), kp, :] = blk_w[:, ks, s].permute(1, 2, 0)
                kbase += nks[c] * cpk
        return Wp.view(d.cout_pad, n_k, d.kh, d.kw)

    def conv(self, d):
        f32 = d.dtype == L.F32
        esz = 4 if f32 else 2
        cpk = 32 // esz
        outs = []
        for b in range(d.batch):
            xs = []
            for c in range(d.n_chunks):
                ch = d.chunks[c]
                fill = 0
                for pi in range(ch.first_piece, ch.first_piece + ch.n_pieces):
                    p = d.pieces[pi]
                    assert p.lds_ch == fill, 'piece not contiguous'
                    if p.v.ptr is None:
                        xs.append(torch.zeros(p.nch, d.inH, d.inW))
                    else:
                        u = p.up_shift
                        t = self.strided(p.v, p.nch, d.inH >> u, d.inW >> u, b).float()
                        if u:
                            t = t.repeat_interleave(2, 1).repeat_interleave(2, 2)
                        if not f32 and p.v.ptr != self._raw_piece:
                            t = t.half().float()       # staged in LDS as fp16
                        xs.append(t)
                    fill += p.nch
                assert fill == ch.nks * cpk
            X = torch.cat(xs, 0)[None]
            Wt = self.unpack_weights(d)
            # explicit zero padding: pad_y / pad_x on the top / left, whatever the output size needs on the bottom / right (the
            # kernels zero-fill every out-of-range tap: 2x2 phase filters use pad 1 or 0)
            need_h = (d.H - 1) * d.stride + d.kh - d.inH - d.pad_y
            need_w = (d.W - 1) * d.stride + d.kw - d.inW - d.pad_x
            Xp = F.pad(X, [d.pad_x, max(need_w, 0), d.pad_y, max(need_h, 0)])
            y = F.conv2d(Xp, Wt, None, stride=d.stride)[0][:, :d.H, :d.W]
            assert y.shape[1:] == (d.H, d.W), (y.shape, d.H, d.W)
            bflat, boff = self._flat(d.bias, True)
            self.note_read(d.bias, d.cout_pad * 4)
            y = y + bflat[boff:boff + d.cout_pad].view(-1, 1, 1)
            if d.cout_perm:
                # layers of the persistent kernels: MFMA row r of a 32-cout subtile holds channel
                # (r>>4)*16 + ((r>>2)&1)*8 + ((r>>3)&1)*4 + (r&3) (include/demfi_hip.h); the octet tables describe the channel order
                r = torch.arange(d.cout_pad)
                q = r % 32
                chan = (r // 32) * 32 + (q >> 4) * 16 + ((q >> 2) & 1) * 8 + ((q >> 3) & 1) * 4 + (q & 3)
                yc = torch.empty_like(y)
                yc[chan] = y
                y = yc
            outs.append(y)
        for b, y in enumerate(outs):
            for o in range(d.cout_pad // 8):
                n = d.oct_n[o]
                if n == 0:
                    continue
                sg = d.segs[d.oct_seg[o]]
                c0 = d.oct_ch[o]
                v = y[o * 8:o * 8 + n]

                def sub(view, cc=c0):
                    w = L.View(view.ptr + cc * view.sc * (4 if view.is_f32 else 2), view.sx, view.sy, view.sc, view.sb,
                               view.is_f32, 0)
                    return w
                if sg.res.ptr is not None:
                    r = self.strided(sub(sg.res), n, d.H, d.W, b).float()
                    if sg.mode == L.MODE_STORE:
                        v = _act(v + r, sg.act)
                    elif sg.mode == L.MODE_MUL:
                        v = torch.sigmoid(v) * r
                    else:
                        z = self.strided(sub(sg.aux), n, d.H, d.W, b).float()
                        v = (1 - z) * r + z * torch.tanh(v)
                else:
                    assert sg.mode == L.MODE_STORE
                    v = _act(v, sg.act)
                sc = sg.scale
                dv = sub(sg.dst)
                dst = L.View(dv.ptr + (sg.dy * dv.sy + sg.dx * dv.sx) * (4 if dv.is_f32 else 2), dv.sx * sc, dv.sy * sc,
                             dv.sc, dv.sb, dv.is_f32, 0)
                out = self.written(dst, n, d.H, d.W, b)
                out.copy_(v.to(out.dtype))
                if d.pack.ptr is not None and o < 4 and d.pack_oct_ch[o] >= 0:
                    # packed copy (demfi_conv.pack): the octet's channels + zeros up to the next multiple of 4, path dtype, NHWC
                    n4 = (n + 3) // 4 * 4
                    pv = L.View(d.pack.ptr + d.pack_oct_ch[o] * 2, d.pack.sx, d.pack.sy, d.pack.sc, d.pack.sb, 0, 0)
                    pk = self.written(pv, n4, d.H, d.W, b)
                    pk.copy_(torch.cat([v, torch.zeros(n4 - n, d.H, d.W)], 0).to(pk.dtype))

    # ---- whole segments ---------------------------------------------------------------------------------
    def planes(self, ptr, n, H, W, write=False):
        return self.strided(L.View(ptr, 1, W, H * W, 0, 1, 0), n, H, W, write=write)

    @staticmethod
    def expand(op):
        """A batched point-wise op (demfi_op.bt.nb > 1: one launch for all per-t contexts) as its nb per-context ops."""
        nb = int(op.bt.nb)
        if nb <= 1:
            return [op]
        out = []
        for q in range(nb):
            o = L.Op.from_buffer_copy(bytes(op))
            o.bt.nb = 1
            for name, st in (('a', op.bt.a), ('b', op.bt.b), ('o', op.bt.o)):
                v = getattr(o, name)
                if v.ptr:
                    v.ptr = v.ptr + q * st
            if o.t:
                o.t = o.t + q * op.bt.t
            for i in range(32):
                if o.p[i]:
                    o.p[i] = o.p[i] + q * op.bt.p[i]
            out.append(o)
        return out

    def run(self, ops):
        e = self.e
        H, W = e.H, e.W
        f32 = e.f32
        outs = []
        for op in [x for big in ops for x in self.expand(big)]:
            k = op.kind
            if self.precise:
                outs.extend(self.precise_op(op))
            elif k == 0:
                self.conv(e.conv_desc(op.conv))
            elif k == 10:
                # fused residual block == its two convolutions in turn, with the intermediate in PRIVATE memory: the fused kernel
                # keeps it in LDS and never touches the plan's scratch buffer, whose memory the workspace arena (round 5) may have
                # handed to a buffer that is alive right now
                d1 = L.Conv.from_buffer_copy(bytes(e.conv_desc(op.conv)))
                d2 = L.Conv.from_buffer_copy(bytes(e.conv_desc(op.nch)))
                sg = d1.segs[d1.sub_seg[0]]
                assert d2.pieces[0].v.ptr == sg.dst.ptr and sg.dst.sx == 64 and sg.dst.sy == d1.W * 64
                wide = d1.dtype == L.F32 or not self.round_mid
                tmp = torch.zeros(d1.batch * d1.H * d1.W * 64 + 64, dtype=torch.float32 if wide else torch.float16)
                self.reg.append((tmp.data_ptr(), tmp.numel() * tmp.element_size(), tmp))
                for v in (sg.dst, d2.pieces[0].v):
                    v.ptr = tmp.data_ptr()
                    v.sb = d1.H * d1.W * 64
                    v.is_f32 = 1 if wide else 0
                self._raw_piece = None if self.round_mid else tmp.data_ptr()
                self.conv(d1)
                self.conv(d2)
                self._raw_piece = None
                self.reg.pop()
            elif k == 11:                                                  # round 6: reset gate of a GRU half-step == its convolution
                self.conv(e.conv_desc(op.conv))
            elif k == 12:
                # z + q + blend in one launch == convz (sigmoid) then convq (GRU epilogue) with z in PRIVATE memory: the fused kernel
                # hands z over through LDS and never touches the plan's z buffer, which has no memory of its own under the arena
                dz = L.Conv.from_buffer_copy(bytes(e.conv_desc(op.conv)))
                dq = L.Conv.from_buffer_copy(bytes(e.conv_desc(op.nch)))
                sz, sq = dz.segs[dz.sub_seg[0]], dq.segs[dq.sub_seg[0]]
                assert sq.aux.ptr == sz.dst.ptr and sz.dst.sx == 64 and sz.dst.sy == dz.W * 64
                wide = dz.dtype == L.F32 or self.z_on_chip
                tmp = torch.zeros(dz.batch * dz.H * dz.W * 64 + 64, dtype=torch.float32 if wide else torch.float16)
                self.reg.append((tmp.data_ptr(), tmp.numel() * tmp.element_size(), tmp))
                for v in (sz.dst, sq.aux):
                    v.ptr = tmp.data_ptr()
                    v.sb = dz.H * dz.W * 64
                    v.is_f32 = 1 if wide else 0
                self.conv(dz)
                self.conv(dq)
                self.reg.pop()
            elif k == 13:                                                  # visualisation extras (DEMFI_HP_EXTRAS)
                if op.conv == 0:
                    a = self.strided(op.a, op.nch, H, W).float()
                    if op.b.ptr:
                        a = a - self.strided(op.b, op.nch, H, W).float()
                    self.planes(op.p[0], 1, H, W, write=True).copy_(a.abs().mean(0, keepdim=True))
                elif op.conv == 1:
                    self.planes(op.p[0], 1, H, W)
                    pl = self.planes(op.p[0], 1, H, W, write=True)
                    pl -= pl.min()
                    pl /= pl.max()
                else:
                    self.planes(op.p[0], 1, H, W, write=True).copy_(1 - self.planes(op.p[1], 1, H, W))
            elif k == 1:                                                   # pack planar fp32 planes -> NHWC slice
                dst = self.written(op.o, op.nch, H, W)
                for c in range(op.nch):
                    if op.p[c] is None:
                        dst[c] = 0
                    else:
                        dst[c] = self.planes(op.p[c], 1, H, W)[0].to(dst.dtype)
            elif k == 2:                                                   # s2d: x [3,4,H,W] -> [H/2,W/2,48]
                x = self.planes(op.p[0], 12, H, W).view(3, 4, H, W)
                cat = x.permute(1, 0, 2, 3).reshape(1, 12, H, W)
                out = self.strided(L.View(op.p[1], 48, (W // 2) * 48, 1, 0, 1 if f32 else 0, 0), 48, H // 2, W // 2, write=True)
                out.copy_(O.space_to_depth(cat, 2)[0].to(out.dtype))
            elif k == 3:                                                   # overlay
                x = self.planes(op.p[0], 12, H, W).view(3, 4, H, W)
                self.planes(op.p[1], 3, H, W, write=True).copy_(torch.mean(x[:, 0:2], dim=1))
            elif k == 4:                                                   # fgac gather
                rk = self.strided(op.a, op.nch, H, W).float()[None]
                fl = self.planes(op.p[0], 2, H, W)
                out = self.written(op.o, op.nch, H, W)
                out.copy_(O.fgac_sample(rk, fl[None])[0].to(out.dtype))
            elif k == 8:                                                   # generalised FGAC window (rr = op.conv, map = op._pad)
                rk = self.strided(op.a, op.nch, H, W).float()[None]
                sk = self.strided(op.b, op.nch, H, W).float()[None]
                fl = self.planes(op.p[0], 2, H, W)
                out = self.written(op.o, op.nch, H, W)
                out.copy_(O.fgac_window(rk, sk, fl[None], op.conv, 0, op._pad)[0][0].to(out.dtype))
            elif k == 9:                                                   # avg_pool (sr = op.conv)
                a = self.strided(op.a, op.nch, H, W).float()[None]
                out = self.written(op.o, op.nch, H, W)
                out.copy_(F.avg_pool2d(a, 2 * op.conv + 1, 1, op.conv)[0].to(out.dtype))
            elif k == 5:                                                   # gate blend
                g = self.planes(op.p[0], 1, H, W)
                s_, e_ = self.strided(op.a, op.nch, H, W).float(), self.strided(op.b, op.nch, H, W).float()
                out = self.written(op.o, op.nch, H, W)
                out.copy_((g * s_ + (1 - g) * e_).to(out.dtype))
            elif k == 6:                                                   # CFR
                t = self.planes(op.t, 1, 1, 1).view(1, 1, 1, 1)
                a, bb = O.cfr_flow_align(self.planes(op.p[0], 2, H, W)[None], self.planes(op.p[1], 2, H, W)[None], t)
                out = self.planes(op.p[3], 4, H, W, write=True)
                out[0:2].copy_(a[0])
                out[2:4].copy_(bb[0])
                if op.p[5] is not None:                                    # round 6: the packed record [ft | flow_01, flow_10, logit | 0] for enc1
                    pk = self.strided(L.View(op.p[5], 16, W * 16, 1, 0, 1 if f32 else 0, 0), 16, H, W, write=True)
                    pk.copy_(torch.cat([out, self.planes(op.p[0], 2, H, W), self.planes(op.p[1], 2, H, W), self.planes(op.p[4], 1, H, W),
                                        torch.zeros(7, H, W)], 0).to(pk.dtype))
            elif k == 7:                                                   # warp + blend
                t = self.planes(op.t, 1, 1, 1).view(1, 1, 1, 1)
                A = self.strided(op.a, op.nch, H, W).float()[None]
                B = self.strided(op.b, op.nch, H, W).float()[None]
                lg = self.planes(op.p[2], 1, H, W)
                r = O.warp_blend(A, self.planes(op.p[0], 2, H, W)[None], B, self.planes(op.p[1], 2, H, W)[None], lg[None], t)
                out = self.written(op.o, op.nch, H, W)
                out.copy_(r[0].to(out.dtype))
                if op.p[3] is not None:
                    self.planes(op.p[3], 1, H, W, write=True).copy_(torch.sigmoid(lg))
                if op.p[4] is not None:                                    # packed NHWC record [out | fa | fb | occ] for the next conv
                    pk = self.strided(L.View(op.p[4], 8, W * 8, 1, 0, 1 if f32 else 0, 0), 8, H, W, write=True)
                    pk.copy_(torch.cat([r[0], self.planes(op.p[0], 2, H, W), self.planes(op.p[1], 2, H, W), torch.sigmoid(lg)], 0).to(pk.dtype))
            else:
                raise AssertionError(k)
        return outs if self.precise else None

    # ---- precise mode: float64, results returned ----------------------------------------------------------------------
    def _pre64(self, d, X=None):
        """Pre-activations of descriptor d in float64, per image: [(v, S)] with v, S [cout_pad,H,W] in CHANNEL order (cout_perm
        undone) and S = conv(|x|, |w|) + |b|.  X: the input [batch,C,inH,inW] instead of the descriptor's pieces (a fused op)."""
        f32 = d.dtype == L.F32
        cpk = 8 if f32 else 16
        Wt = self.unpack_weights(d).double()
        bflat, boff = self._flat(d.bias, True)
        self.note_read(d.bias, d.cout_pad * 4)
        bias = bflat[boff:boff + d.cout_pad].double()
        out = []
        for b in range(d.batch):
            if X is None:
                xs = []
                for c in range(d.n_chunks):
                    ch = d.chunks[c]
                    fill = 0
                    for pi in range(ch.first_piece, ch.first_piece + ch.n_pieces):
                        p = d.pieces[pi]
                        assert p.lds_ch == fill, 'piece not contiguous'
                        if p.v.ptr is None:
                            xs.append(torch.zeros(p.nch, d.inH, d.inW, dtype=torch.float64))
                        else:
                            u = p.up_shift
                            t = self.strided(p.v, p.nch, d.inH >> u, d.inW >> u, b)
                            if u:
                                t = t.repeat_interleave(2, 1).repeat_interleave(2, 2)
                            if not f32:
                                t = t.half()                 # staged in LDS as fp16: the kernel's own rounding of a planar fp32 piece
                            xs.append(t.double())
                        fill += p.nch
                    assert fill == ch.nks * cpk
                x = torch.cat(xs, 0)[None]
            else:
                x = X[b][None]
            need_h = (d.H - 1) * d.stride + d.kh - d.inH - d.pad_y
            need_w = (d.W - 1) * d.stride + d.kw - d.inW - d.pad_x
            xp = F.pad(x, [d.pad_x, max(need_w, 0), d.pad_y, max(need_h, 0)])
            v = F.conv2d(xp, Wt, bias, stride=d.stride)[0][:, :d.H, :d.W]
            S = F.conv2d(xp.abs(), Wt.abs(), bias.abs(), stride=d.stride)[0][:, :d.H, :d.W]
            assert v.shape[1:] == (d.H, d.W)
            if d.cout_perm:
                r = torch.arange(d.cout_pad)
                q = r % 32
                chan = (r // 32) * 32 + (q >> 4) * 16 + ((q >> 2) & 1) * 8 + ((q >> 3) & 1) * 4 + (q & 3)
                vc, Sc = torch.empty_like(v), torch.empty_like(S)
                vc[chan], Sc[chan] = v, S
                v, S = vc, Sc
            out.append((v, S))
        return out, Wt

    @staticmethod
    def _sub(view, cc):
        return L.View(view.ptr + cc * view.sc * (4 if view.is_f32 else 2), view.sx, view.sy, view.sc, view.sb, view.is_f32, 0)

    def _octets(self, d):
        """(octet, count, segment, first destination channel) of the octets a descriptor stores."""
        return [(o, d.oct_n[o], d.segs[d.oct_seg[o]], d.oct_ch[o]) for o in range(d.cout_pad // 8) if d.oct_n[o]]

    def _dst_view(self, sg, c0):
        dv = self._sub(sg.dst, c0)
        sc = sg.scale
        return L.View(dv.ptr + (sg.dy * dv.sy + sg.dx * dv.sx) * (4 if dv.is_f32 else 2), dv.sx * sc, dv.sy * sc, dv.sc, dv.sb, dv.is_f32, 0)

    def _emit(self, name, d, b, o, n, sg, c0, **kw):
        """The Out records of one stored octet: the destination and, where the descriptor asks for it, the packed fp16 copy."""
        dst = self._dst_view(sg, c0)
        self.written(dst, n, d.H, d.W, b)
        outs = [Out(name, 'epi', self.offsets(dst, n, d.H, d.W, b), torch.float32 if dst.is_f32 else torch.float16, **kw)]
        if d.pack.ptr is not None and o < 4 and d.pack_oct_ch[o] >= 0:
            n4 = (n + 3) // 4 * 4
            pv = L.View(d.pack.ptr + d.pack_oct_ch[o] * 2, d.pack.sx, d.pack.sy, d.pack.sc, d.pack.sb, 0, 0)
            self.written(pv, n4, d.H, d.W, b)
            off = self.offsets(pv, n4, d.H, d.W, b)
            outs.append(Out(name + ' (packed copy)', 'epi', off[:n], torch.float16, **kw))
            if n4 > n:
                outs.append(Out(name + ' (packed copy, padding)', 'exact', off[n:], torch.float16, ref=torch.zeros(n4 - n, d.H, d.W, dtype=torch.float64)))
        return outs

    def conv64(self, d, name):
        outs = []
        pre, _ = self._pre64(d)
        for b, (v, S) in enumerate(pre):
            for o, n, sg, c0 in self._octets(d):
                kw = dict(v=v[o * 8:o * 8 + n], S=S[o * 8:o * 8 + n], act=sg.act, mode=sg.mode)
                if sg.res.ptr is not None:
                    kw['res'] = self.strided(self._sub(sg.res, c0), n, d.H, d.W, b).double()
                    if sg.mode == L.MODE_GRU:
                        kw['z'] = self.strided(self._sub(sg.aux, c0), n, d.H, d.W, b).double()
                else:
                    assert sg.mode == L.MODE_STORE
                outs += self._emit(name, d, b, o, n, sg, c0, **kw)
        return outs

    def _by_channel(self, d, t):
        """[cout_pad,H,W] in octet order -> [64,H,W] by destination channel of the (single) 64-channel segment."""
        out = torch.zeros(64, d.H, d.W, dtype=torch.float64)
        seen = 0
        for o, n, sg, c0 in self._octets(d):
            out[c0:c0 + n] = t[o * 8:o * 8 + n]
            seen += n
        assert seen == 64 and d.n_segs == 1
        return out

    def resblock64(self, d1, d2, name):
        """y = x + conv2(relu(conv1(x))): the intermediate m is rounded to the path dtype (it is staged in LDS in that type), everything
        else stays float64.  Besides (v2, S2) every record carries ``widen``: what conv2 may legitimately differ by because the
        kernel's fp32 pre-activation of conv1, off by at most d1 = C_ACC u S1, rounds to the OTHER neighbour where the float64 one lies
        within d1 of a rounding midpoint:  widen = conv(dm, |w2|),  dm = mask (ulp(m) + [d1 > ulp / 2] 2 d1)  (below the normal range
        d1 may exceed the spacing: the value then moves by up to 2 d1 before it is rounded).  fp32 path: no fp16 rounding hides the
        accumulation error of conv1, dm = d1 + ulp32(m) on every element where relu can be non-zero."""
        from tests import epilogue_ref as E
        f32 = d1.dtype == L.F32
        dt = torch.float32 if f32 else torch.float16
        s1 = d1.segs[d1.sub_seg[0]]
        assert s1.act == L.ACT_RELU and s1.mode == L.MODE_STORE and s1.res.ptr is None and d2.n_pieces == 1 and d2.pieces[0].nch == 64
        pre1, _ = self._pre64(d1)
        M, DM = [], []
        for v1, S1 in pre1:
            v1, S1 = self._by_channel(d1, v1), self._by_channel(d1, S1)
            m64 = torch.relu(v1)
            m = m64.to(dt).double()
            dl = E.C_ACC * E.U * S1
            ulp = E.spacing(m, dt)
            if f32:
                dm = torch.where(v1 > -dl, dl + ulp, torch.zeros_like(dl))
            else:
                pow2 = (m > 2.0 ** -14) & (torch.log2(torch.clamp(m, min=2.0 ** -24)) % 1.0 == 0.0)
                up = m + 0.5 * ulp                                        # the two rounding midpoints next to m
                dn = m - 0.5 * torch.where(pow2, 0.5 * ulp, ulp)
                mask = ((up - m64).abs() <= dl) | ((m64 - dn).abs() <= dl) | ((v1.abs() <= dl) & (dl > 0.5 * ulp))
                dm = mask * (ulp + torch.where(dl > 0.5 * ulp, 2.0 * dl, torch.zeros_like(dl)))
            M.append(m)
            DM.append(dm)
        pre2, W2 = self._pre64(d2, X=M)
        outs = []
        for b, (v, S) in enumerate(pre2):
            need_h = (d2.H - 1) * d2.stride + d2.kh - d2.inH - d2.pad_y
            need_w = (d2.W - 1) * d2.stride + d2.kw - d2.inW - d2.pad_x
            wd = F.conv2d(F.pad(DM[b][None], [d2.pad_x, max(need_w, 0), d2.pad_y, max(need_h, 0)]), W2.abs())[0][:, :d2.H, :d2.W]
            if d2.cout_perm:
                r = torch.arange(d2.cout_pad)
                q = r % 32
                chan = (r // 32) * 32 + (q >> 4) * 16 + ((q >> 2) & 1) * 8 + ((q >> 3) & 1) * 4 + (q & 3)
                wc = torch.empty_like(wd)
                wc[chan] = wd
                wd = wc
            for o, n, sg, c0 in self._octets(d2):
                assert sg.mode == L.MODE_STORE and sg.act in (L.ACT_NONE, L.ACT_RELU)
                kw = dict(v=v[o * 8:o * 8 + n], S=S[o * 8:o * 8 + n], act=sg.act, mode=sg.mode, widen=wd[o * 8:o * 8 + n])
                if sg.res.ptr is not None:
                    kw['res'] = self.strided(self._sub(sg.res, c0), n, d2.H, d2.W, b).double()
                outs += self._emit(name, d2, b, o, n, sg, c0, **kw)
        return outs

    def zq64(self, dz, dq, name):
        """z = sigmoid(convz) kept in float64 (the kernel keeps it in fp32 on chip: epilogue_ref.ref_zq), h' = (1 - z) h + z tanh(convq)."""
        sz = dz.segs[dz.sub_seg[0]]
        assert sz.act == L.ACT_SIGMOID and sz.mode == L.MODE_STORE and sz.res.ptr is None
        prez, _ = self._pre64(dz)
        preq, _ = self._pre64(dq)
        outs = []
        for b, ((vz, Sz), (vq, Sq)) in enumerate(zip(prez, preq)):
            vz, Sz = self._by_channel(dz, vz), self._by_channel(dz, Sz)
            for o, n, sg, c0 in self._octets(dq):
                assert sg.mode == L.MODE_GRU
                h = self.strided(self._sub(sg.res, c0), n, dq.H, dq.W, b).double()
                outs += self._emit(name, dq, b, o, n, sg, c0, vz=vz[c0:c0 + n], Sz=Sz[c0:c0 + n], v=vq[o * 8:o * 8 + n], S=Sq[o * 8:o * 8 + n],
                                   res=h, act=sg.act, mode='zq')
        return outs

    def precise_op(self, op):
        from tests import motion_ref as R
        e = self.e
        H, W = e.H, e.W
        f32 = e.f32
        pdt = torch.float32 if f32 else torch.float16
        k = op.kind
        name = op.name.decode()
        hwc = lambda t: t.permute(1, 2, 0).numpy()
        chw = lambda a: torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 0)))
        odt = lambda v: torch.float32 if v.is_f32 else torch.float16
        if k in (0, 11):
            return self.conv64(e.conv_desc(op.conv), name)
        if k == 10:
            return self.resblock64(e.conv_desc(op.conv), e.conv_desc(op.nch), name)
        if k == 12:
            return self.zq64(e.conv_desc(op.conv), e.conv_desc(op.nch), name)
        if k == 1:                                                         # pack: exact rounding of fp32 planes to the record's type
            self.written(op.o, op.nch, H, W)
            ref = torch.stack([torch.zeros(H, W) if op.p[c] is None else self.planes(op.p[c], 1, H, W)[0] for c in range(op.nch)])
            return [Out(name, 'exact', self.offsets(op.o, op.nch, H, W), odt(op.o), ref=ref.to(odt(op.o)).double())]
        if k == 2:
            x = self.planes(op.p[0], 12, H, W).view(3, 4, H, W)
            cat = x.permute(1, 0, 2, 3).reshape(1, 12, H, W)
            ov = L.View(op.p[1], 48, (W // 2) * 48, 1, 0, 1 if f32 else 0, 0)
            self.written(ov, 48, H // 2, W // 2)
            return [Out(name, 'exact', self.offsets(ov, 48, H // 2, W // 2), pdt, ref=O.space_to_depth(cat, 2)[0].to(pdt).double())]
        if k == 3:                                                         # overlay: mean of two fp32 values, one rounded sum
            x = self.planes(op.p[0], 12, H, W).view(3, 4, H, W).double()
            ov = L.View(op.p[1], 1, W, H * W, 0, 1, 0)
            self.written(ov, 3, H, W)
            return [Out(name, 'sum', self.offsets(ov, 3, H, W), torch.float32, ref=x[:, 0:2].mean(1), terms=x[:, 0:2].abs().mean(1), n=2)]
        if k == 9:
            a = self.strided(op.a, op.nch, H, W).double()[None]
            self.written(op.o, op.nch, H, W)
            ks = 2 * op.conv + 1
            return [Out(name, 'sum', self.offsets(op.o, op.nch, H, W), odt(op.o), ref=F.avg_pool2d(a, ks, 1, op.conv)[0],
                        terms=F.avg_pool2d(a.abs(), ks, 1, op.conv)[0], n=ks * ks + 1)]
        if k == 4:
            S = hwc(self.strided(op.a, op.nch, H, W))
            v, a = R.fgac_gather(S, self.planes(op.p[0], 2, H, W).numpy())
            self.written(op.o, op.nch, H, W)
            return [Out(name, 'motion', self.offsets(op.o, op.nch, H, W), odt(op.o), ref=chw(v), bound=chw(a), k=8)]
        if k == 5:
            g = self.planes(op.p[0], 1, H, W)[0].numpy()
            v, a = R.gate_blend(g, hwc(self.strided(op.a, op.nch, H, W)), hwc(self.strided(op.b, op.nch, H, W)))
            self.written(op.o, op.nch, H, W)
            return [Out(name, 'motion', self.offsets(op.o, op.nch, H, W), odt(op.o), ref=chw(v), bound=chw(a), k=8)]
        if k == 6:
            t = float(self.planes(op.t, 1, 1, 1).view(-1)[0])
            f01, f10 = self.planes(op.p[0], 2, H, W), self.planes(op.p[1], 2, H, W)
            r = R.cfr(f01.numpy(), f10.numpy(), t)
            ov = L.View(op.p[3], 1, W, H * W, 0, 1, 0)
            self.written(ov, 4, H, W)
            ft_off = self.offsets(ov, 4, H, W)
            zero = torch.from_numpy(np.broadcast_to(~r['hit'], r['ft'].shape).copy())
            outs = [Out(name, 'motion', ft_off, torch.float32, ref=torch.from_numpy(r['ft']), bound=torch.from_numpy(r['bound']), k=16, exact_zero=zero)]
            if op.p[5] is not None:      # the packed record [ft | flow_01, flow_10, logit | 0]: the planar values, rounded to the record's type
                pv = L.View(op.p[5], 16, W * 16, 1, 0, 1 if f32 else 0, 0)
                self.written(pv, 16, H, W)
                po = self.offsets(pv, 16, H, W)
                self.planes(op.p[4], 1, H, W)
                src = np.concatenate([ft_off, self.offsets(L.View(op.p[0], 1, W, H * W, 0, 1, 0), 2, H, W),
                                      self.offsets(L.View(op.p[1], 1, W, H * W, 0, 1, 0), 2, H, W),
                                      self.offsets(L.View(op.p[4], 1, W, H * W, 0, 1, 0), 1, H, W)], 0)
                outs.append(Out(name + ' (packed record)', 'mirror', po[:9], pdt, src=src, src_dtype=torch.float32))
                outs.append(Out(name + ' (packed record, padding)', 'exact', po[9:], pdt, ref=torch.zeros(7, H, W, dtype=torch.float64)))
            return outs
        if k == 7:
            t = float(self.planes(op.t, 1, 1, 1).view(-1)[0])
            fa, fb, lg = self.planes(op.p[0], 2, H, W), self.planes(op.p[1], 2, H, W), self.planes(op.p[2], 1, H, W)
            r = R.warp_blend(hwc(self.strided(op.a, op.nch, H, W)), fa.numpy(), hwc(self.strided(op.b, op.nch, H, W)), fb.numpy(), lg[0].numpy(), t)
            self.written(op.o, op.nch, H, W)
            o_off = self.offsets(op.o, op.nch, H, W)
            outs = [Out(name, 'motion', o_off, odt(op.o), ref=chw(r['out']), bound=chw(r['bound']), k=16)]
            occ_off = None
            if op.p[3] is not None:
                ov = L.View(op.p[3], 1, W, H * W, 0, 1, 0)
                self.written(ov, 1, H, W)
                occ_off = self.offsets(ov, 1, H, W)
                occ = torch.from_numpy(r['occ'])[None]
                outs.append(Out(name + ' (occlusion)', 'motion', occ_off, torch.float32, ref=occ, bound=occ + 2.0 ** -100, k=4))
            if op.p[4] is not None:      # the packed record [out | fa | fb | occ]: the planar values, rounded to the record's type
                assert op.nch == 3 and occ_off is not None and op.o.is_f32
                pv = L.View(op.p[4], 8, W * 8, 1, 0, 1 if f32 else 0, 0)
                self.written(pv, 8, H, W)
                src = np.concatenate([o_off, self.offsets(L.View(op.p[0], 1, W, H * W, 0, 1, 0), 2, H, W),
                                      self.offsets(L.View(op.p[1], 1, W, H * W, 0, 1, 0), 2, H, W), occ_off], 0)
                outs.append(Out(name + ' (packed record)', 'mirror', self.offsets(pv, 8, H, W), pdt, src=src, src_dtype=torch.float32))
            return outs
        raise NotImplementedError('precise mode does not cover op kind %d (%s): the generalised FGAC and the visualisation extras are '
                                  'outside the replay' % (k, name))

    def forward(self, x, t, n):
        e = self.e
        e.x.copy_(x[0])
        e.t_dev.fill_(float(t))
        self.run(e.ops(SEG_TRUNK))
        self.run(e.ops(SEG_HEAD))
        for it in range(n):
            self.run(e.ops(SEG_ITER, it))


    def forward_tb(self, x, ts, n):
        """The batched per-t plan (demfi_forward_tb): context c gets time instant ts[c]; one op list for all contexts."""
        from demfi_amd.engine import SEG_TB_HEAD, SEG_TB_ITER
        e = self.e
        e.x.copy_(x[0])
        for c, t in enumerate(ts):
            e._ctxs[e.trunk][c]['t_dev'].fill_(float(t))
        self.run(e.ops(SEG_TRUNK))
        self.run(e.ops(SEG_TB_HEAD))
        for it in range(n):
            self.run(e.ops(SEG_TB_ITER, it))


def _act(v, act):
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_TANH:
        return torch.tanh(v)
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v
