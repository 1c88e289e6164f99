"""Replay of a real launch plan one launch at a time  --  TEST INFRASTRUCTURE (not shipped); imports nothing GPU-specific.

Given a HOST-bound engine ``ref`` (its workspace is the reference image) and an executor ``run(op, image) -> image`` (``Replay.index``
tells it the op's position in the plan: its own engine's op there is the one to run), every op of the plan, in plan order, is

  1. evaluated in float64 from the reference image (``PlanSim(ref, precise=True)``), which also records the bytes the reference
     interpreter reads and writes for it: the op's read set and write set;
  2. launched on an image that is the reference image with every byte of the REPLAY SPAN outside the read set overwritten by poison
     (0xFF 0x7F repeated: a NaN as fp16 and as fp32), bytes of the write set that are not read included (0xFE 0x7F there, so that
     an element that was never stored can be told from one computed from poison);
  3. checked: outside the write set the returned image equals the launch image byte for byte (a stray write otherwise; the scratch
     buffer of a fused block and the z buffer of gru_zq stay poison); inside it every element is held to the float64 value with the
     per-element bounds of tests/epilogue_ref.py and tests/motion_ref.py; a NaN there is poison that was read, or poison that survived;
  4. advanced: the default-mode ``PlanSim`` stores the op's result into the reference image, so the next op sees what a correct plan
     would have stored, rounded as stored.  Errors cannot accumulate, and the forward's chaos around floor() decisions has no say.

The recorded sets must also lie inside the buffers the arena planner is told about (``declared``: a restatement of op_accesses() of
demfi_amd/csrc/layout.cpp from the descriptor fields).

The replay span begins behind the weight blob, the zero page and the descriptor table (compute_layout places them first); the device
twin keeps its own copy of those.  Inside the span two kinds of record are never poisoned: the per-context ``sink`` records (pointers;
zero = disabled: asserted all-zero before every launch) and ``cfr_acc`` (the device keeps its own bytes: an executor that runs on a
device does not upload them, ``upload_ranges``; after a launch they must be what they were)."""
import ctypes as C

import numpy as np
import torch

from demfi_amd import _lib as L
from demfi_amd.engine import KIND_NAME
from tests import epilogue_ref as E
from tests import motion_ref as R
from tests.plan_sim import PlanSim

TRUNK_BUFFERS = ('x', 's2d', 'f1', 'x0', 'grow', 'gffcat', 'g0', 'g1', 'up', 'F01', 'ffo', 'enc_a', 'enc_t', 'enc_b', 'rk', 'skk', 'rkp', 'skp',
                 'smp', 'E', 'wg', 'gate', 'aF', 'overlay', 'viz', 'vizs', 'u1a', 'xff16', 're1w', 'g_pw')
T_BUFFERS = ('t', 'sink', 'cfr_acc', 'ft', 'Ft', 'u1', 'u2', 'u3', 'd0', 'd1', 'd2', 'rF', 'delta', 'occ', 'dec_a', 'dec_t', 'dec_b', 'sharp1',
             'frec0', 'frec1', 're1', 'rd64', 'de1', 'bl1', 'xb', 'zb', 'rh', 'h1', 'fo1', 'stnew', 'misc16', 'ref16', 'ref32', 'agg3s', 'agg3d',
             'delta16', 'g_a', 'g_t', 'g_b', 'g_p2', 'finals')
NP_OF = {torch.float16: (np.uint16, np.float16, 0x7FFE), torch.float32: (np.uint32, np.float32, 0x7FFE7FFE)}      # [2]: the UNWRITTEN pattern


class ReplayError(AssertionError):
    pass


def poison(n, unwritten=False):
    """n bytes of the poison pattern (n even, placed at an even offset): every aligned half is the fp16 NaN 0x7FFF, every aligned word
    the fp32 NaN 0x7FFF7FFF.  unwritten: the second pattern, 0x7FFE / 0x7FFE7FFE, for bytes the op must write and does not read -- a
    NaN with this payload in the result was never stored; any other NaN was computed from poison the launch read."""
    p = np.empty(n, np.uint8)
    p[0::2] = 0xFE if unwritten else 0xFF
    p[1::2] = 0x7F
    return p


def declared(eng, op):
    """[(pointer, is_write)] of one op: op_accesses() of layout.cpp, from the descriptor fields."""
    out = []
    rd = lambda p: out.append((p, False)) if p else None
    wr = lambda p: out.append((p, True)) if p else None

    def conv_in(d):
        for i in range(d.n_pieces):
            rd(d.pieces[i].v.ptr)

    def conv_out(d):
        for i in range(d.n_segs):
            rd(d.segs[i].res.ptr), rd(d.segs[i].aux.ptr), wr(d.segs[i].dst.ptr)
        wr(d.pack.ptr)
    for o in PlanSim.expand(op):
        k = KIND_NAME[o.kind]
        if k in ('conv', 'gru_r'):
            conv_in(eng.conv_desc(o.conv)), conv_out(eng.conv_desc(o.conv))
        elif k == 'resblock':
            conv_in(eng.conv_desc(o.conv)), conv_out(eng.conv_desc(o.nch))
        elif k == 'gru_zq':
            dq = eng.conv_desc(o.nch)
            conv_in(eng.conv_desc(o.conv)), conv_in(dq)
            for i in range(dq.n_segs):
                rd(dq.segs[i].res.ptr), wr(dq.segs[i].dst.ptr)
        elif k == 'pack':
            for i in range(32):
                rd(o.p[i])
            wr(o.o.ptr)
        elif k in ('s2d', 'overlay'):
            rd(o.p[0]), wr(o.p[1])
        elif k == 'fgac':
            rd(o.a.ptr), rd(o.p[0]), wr(o.o.ptr)
        elif k == 'fgac_window':
            rd(o.a.ptr), rd(o.b.ptr), rd(o.p[0]), wr(o.o.ptr)
        elif k == 'avg_pool':
            rd(o.a.ptr), wr(o.o.ptr)
        elif k == 'gate':
            rd(o.p[0]), rd(o.a.ptr), rd(o.b.ptr), wr(o.o.ptr)
        elif k == 'cfr':
            rd(o.p[0]), rd(o.p[1]), rd(o.p[2]), rd(o.p[4]), wr(o.p[2]), wr(o.p[3]), wr(o.p[5]), rd(o.t)
        elif k == 'warp':
            rd(o.a.ptr), rd(o.b.ptr), rd(o.p[0]), rd(o.p[1]), rd(o.p[2]), rd(o.t), wr(o.o.ptr), wr(o.p[3]), wr(o.p[4])
        else:
            raise NotImplementedError('op kind %d is outside the replay' % o.kind)
    return out


class Replay:
    def __init__(self, ref, run):
        assert ref.device.type == 'cpu', 'the reference engine is bound to host memory'
        self.ref, self.run = ref, run
        self.nbytes = ref.workspace.numel() - 256
        self.img = ref.workspace[ref._ws_off:ref._ws_off + self.nbytes].numpy()       # shares memory with the engine
        self.buffers = []                                                              # (name, trunk, context, lo, hi)
        for k in range(ref.n_trunk):
            for c, names in [(-1, TRUNK_BUFFERS)] + [(q, T_BUFFERS) for q in range(ref.n_ctx)]:
                for n in names:
                    try:
                        t = ref.buffer(n, k, c)
                    except L.DemfiError:
                        continue
                    lo = t.data_ptr() - ref._base
                    self.buffers.append((n, k, c, lo, lo + t.numel() * t.element_size()))
        self.sinks = [(lo, hi) for n, _, _, lo, hi in self.buffers if n == 'sink']
        self.accs = [(lo, hi) for n, _, _, lo, hi in self.buffers if n == 'cfr_acc']
        self.span_lo = self._span_lo()
        self.poison, self.unwritten = poison(self.nbytes), poison(self.nbytes, unwritten=True)
        self.sim, self.sim64 = PlanSim(ref), PlanSim(ref, precise=True)
        self._launch = np.empty_like(self.img)
        self.n_ops = 0
        self.index = 0           # position in the plan of the op being replayed: an executor finds its twin of the op by it
        self.worst = {}          # (op kind, stored dtype) -> (largest |got - ref| / bound, op name)
        self.widening = {}       # resblock op name -> [mean widening / unwidened bound of each stored octet]
        self.cond = []           # (op name, largest accumulation term, scale) of the ops whose inputs were scaled to keep the bound valid

    # ---- the span ------------------------------------------------------------------------------------------------
    def _span_lo(self):
        """First byte behind weight blob | zero page | descriptor table, asserted from what the library reports."""
        ref = self.ref
        off, nb = C.c_int64(0), C.c_int64(0)
        L.check(ref.lib.demfi_ctx_weight_region(ref._ctx, C.byref(off), C.byref(nb)))
        w_end = off.value + ((nb.value + 255) & ~255)
        sz = C.sizeof(L.Conv)
        desc_off = w_end + 256
        lo = (desc_off + ref.n_convs * sz + 255) & ~255
        assert off.value == 0 and not self.img[w_end:w_end + 256].any(), 'zero page not where compute_layout puts it'
        for i in (0, ref.n_convs - 1):                 # the host-bound engine holds the table the device twin gets: it IS where we think
            assert bytes(self.img[desc_off + i * sz:desc_off + (i + 1) * sz]) == bytes(ref.conv_desc(i)), 'descriptor table not at %d' % desc_off
        for i in range(ref.n_convs):
            d = ref.conv_desc(i)
            assert d.zero_page == ref._base + w_end
            assert 0 <= d.wpack - ref._base < w_end and 0 <= d.bias - ref._base < w_end
        first = min(b[3] for b in self.buffers)
        assert first == lo, ('first buffer at %d, descriptor table ends at %d' % (first, lo))
        assert max(b[4] for b in self.buffers) <= self.nbytes
        return lo

    def upload_ranges(self):
        """Byte ranges of the image an executor on a device copies into its twin before a launch: the span without cfr_acc."""
        out, lo = [], self.span_lo
        for a, b in sorted(self.accs):
            out.append((lo, a))
            lo = b
        out.append((lo, self.nbytes))
        return [(a, b) for a, b in out if b > a]

    def where(self, byte):
        names = ['%s[trunk %d%s]+%d' % (n, k, '' if c < 0 else ', ctx %d' % c, byte - lo) for n, k, c, lo, hi in self.buffers if lo <= byte < hi]
        if byte < self.span_lo:
            names.append('weights / zero page / descriptors')
        return ' = '.join(names) or 'no buffer (padding between buffers)'

    # ---- one op --------------------------------------------------------------------------------------------------
    def _declared_masks(self, op):
        """(declared reads, declared writes) as byte masks over the span."""
        s0 = self.span_lo
        rd, wr = np.zeros(self.nbytes - s0, np.bool_), np.zeros(self.nbytes - s0, np.bool_)
        for p, w in declared(self.ref, op):
            a = p - self.ref._base
            if a < s0:
                continue                                   # zero page standing in for an absent piece
            named = {(n, k) for n, k, c, lo, hi in self.buffers if lo <= a < hi}
            assert named, 'declared pointer outside every buffer'
            # under the arena one address may name several buffers: all of them count; and a per-t buffer counts with the copies of
            # all contexts, as plan_arena() sizes it (a batched launch walks them with one batch stride from the first)
            for lo, hi in [(lo, hi) for n, k, c, lo, hi in self.buffers if (n, k) in named]:
                (wr if w else rd)[lo - s0:hi - s0] = True
        return rd, wr

    def _evaluate(self, op):
        self.sim64.begin_record(self.span_lo)
        outs = self.sim64.run([op])
        rmask, wmask = self.sim64.end_record()
        return outs, rmask, wmask

    def check_declared(self, name, op, rmask, wmask):
        """What the reference interpreter touches (masks over the span) is what the arena planner is told."""
        s0 = self.span_lo
        drd, dwr = self._declared_masks(op)
        for what, m, dm in (('reads', rmask, drd), ('writes', wmask, dwr)):
            bad = m & ~dm
            if bad.any():
                at = s0 + int(np.argmax(bad))
                raise ReplayError('%s: %s byte %d (%s), which op_accesses() does not declare' % (name, what, at, self.where(at)))

    def advance(self, op, check=True):
        """Advance the reference image over one op WITHOUT launching it (the default-mode interpreter stores its result); with check, the
        accesses it records are held to the declaration."""
        if not check:
            self.sim.run([op])
            return
        self.sim.begin_record(self.span_lo)
        self.sim.run([op])
        rmask, wmask = self.sim.end_record()
        self.check_declared('%s %s' % (KIND_NAME[op.kind], op.name.decode()), op, rmask, wmask)

    def step(self, op):
        name = '%s %s' % (KIND_NAME[op.kind], op.name.decode())
        s0 = self.span_lo
        outs, rmask, wmask = self._evaluate(op)
        # the bound's own validity condition (epilogue_ref: QUARTER_ULP).  An op of the real plan that violates it with these weights
        # gets its inputs scaled down by a power of two in the reference image, for this launch only; the bound stays what it is
        saved = None
        acc = max([float(self._ref_of(o).acc.max()) for o in outs if o.kind == 'epi'], default=0.0)
        if acc >= E.QUARTER_ULP:
            scale = 2.0 ** -(int(np.ceil(np.log2(acc / E.QUARTER_ULP))) + 1)
            saved = self.img[s0:].copy()
            self._scale_inputs(rmask & ~wmask, scale)
            self.cond.append((name, acc, scale))
            outs, r2, w2 = self._evaluate(op)
            assert np.array_equal(r2, rmask) and np.array_equal(w2, wmask)
        self.check_declared(name, op, rmask, wmask)
        assert wmask.any(), name + ': writes nothing'
        launch = self._launch
        np.copyto(launch, self.img)
        pz = ~rmask
        for lo, hi in self.sinks + self.accs:
            pz[lo - s0:hi - s0] = False
        np.copyto(launch[s0:], self.poison[s0:], where=pz)
        np.copyto(launch[s0:], self.unwritten[s0:], where=pz & wmask)
        for lo, hi in self.sinks:
            assert not launch[lo:hi].any(), name + ': a sink record is not all-zero'
        want = launch[s0:].copy()                          # the executor may work in place: what the span held at launch
        try:
            self._check(op, name, outs, want, self.run(op, launch), wmask)
        finally:
            if saved is not None:
                self.img[s0:] = saved
        self.sim.run([op])                                 # advance the reference image
        self.n_ops += 1

    def _check(self, op, name, outs, want, after, wmask):
        """want: the span of the launch image."""
        s0 = self.span_lo
        if after.shape != self.img.shape or after.dtype != np.uint8:
            raise ReplayError(name + ': the executor returned no image')
        if not torch.equal(torch.from_numpy(after[:s0]), torch.from_numpy(self.img[:s0])):
            raise ReplayError(name + ': stray write in front of the span (weights / zero page / descriptors)')
        stray = (after[s0:] != want) & ~wmask
        if stray.any():
            at = int(np.argmax(stray))
            was, at = int(want[at]), at + s0
            if any(lo <= at < hi for lo, hi in self.accs):
                raise ReplayError('%s: cfr_acc left dirty: byte %d (%s) is %d, was %d' % (name, at, self.where(at), after[at], was))
            raise ReplayError('%s: stray write: %d bytes outside the write set changed, first at %d (%s): %d -> %d'
                              % (name, int(stray.sum()), at, self.where(at), was, after[at]))
        for o in outs:
            self._compare(op, name, o, after)

    def _scale_inputs(self, mask, scale):
        """Multiply the activation elements of the reference image inside mask by scale (a power of two).  Planar buffers are fp32, every
        other buffer has the path dtype (the arena only aliases buffers of the path dtype)."""
        mask = mask.copy()                                 # over the span
        s0 = self.span_lo
        for n, k, c, lo, hi in self.buffers:
            if not mask[lo - s0:hi - s0].any():
                continue
            t = self.ref.buffer(n, k, c)
            assert t.dtype in (torch.float16, torch.float32), n
            el = torch.from_numpy(mask[lo - s0:hi - s0].copy()).view(torch.uint8)[::t.element_size()].bool()
            flat = t.view(-1)
            flat[el] = flat[el] * scale
            mask[lo - s0:hi - s0] = False
        assert not mask.any()

    def replay(self, ops):
        """Every op in turn.  An op that fails a check does not stop the replay (the reference image advances regardless, so the ops
        behind it are judged on their own): all findings are raised together at the end."""
        found = []
        for i, op in enumerate(ops):
            self.index = i
            try:
                self.step(op)
            except ReplayError as e:
                found.append(str(e))
                self.sim.run([op])
                self.n_ops += 1
        if found:
            raise ReplayError('%d of %d ops failed:\n' % (len(found), len(ops)) + '\n'.join(found))

    # ---- comparison ----------------------------------------------------------------------------------------------
    def _note(self, op, dtype, ratio, name):
        key = (KIND_NAME[op.kind], 'fp32' if dtype == torch.float32 else 'fp16')
        if ratio >= self.worst.get(key, (-1.0, ''))[0]:
            self.worst[key] = (ratio, name)

    def _compare(self, op, opname, o, after):
        name = opname if o.name == op.name.decode() else '%s [%s]' % (opname, o.name)
        ut, ft, pbits = NP_OF[o.dtype]
        esz = np.dtype(ut).itemsize
        assert not (o.off % esz).any()
        raw = after.view(ut)[o.off // esz]
        got = torch.from_numpy(raw.view(ft).astype(np.float64))
        nan = torch.isnan(got)
        if nan.any():
            at = tuple(torch.nonzero(nan)[0].tolist())
            byte = int(o.off[at])
            if raw[at] == pbits:
                raise ReplayError('%s: store skipped: the poison survived in %d elements of the write set, first at (c, y, x) = %s, byte %d (%s)'
                                  % (name, int(nan.sum()), at, byte, self.where(byte)))
            raise ReplayError('%s: NaN in %d elements, first at (c, y, x) = %s, byte %d (%s): the launch read poisoned memory, i.e. bytes '
                              'outside its read set (which buffer they belong to cannot be told from the result)'
                              % (name, int(nan.sum()), at, byte, self.where(byte)))
        if o.kind == 'epi':
            ratio, at, ref = self._epi(op, name, o, got)
        elif o.kind == 'motion':
            ref = o.ref
            tol = o.k * R.EPS32 * o.bound
            if o.dtype == torch.float16:
                tol = tol + 0.5 * torch.from_numpy(R.fp16_ulp((ref.abs() + tol).numpy()))
            err = (got - ref).abs()
            zero = getattr(o, 'exact_zero', None)
            if zero is not None and bool((got[zero] != 0).any()):
                raise ReplayError('%s: %d elements that receive no source are not exactly 0' % (name, int((got[zero] != 0).sum())))
            ratio, at = _worst(err, tol)
        elif o.kind == 'sum':
            ref = o.ref
            t = o.n * E.U * o.terms
            ratio, at = _worst((got - ref).abs(), 0.5 * E.spacing(ref.abs() + t, o.dtype) + t)
        elif o.kind == 'exact':
            ref = o.ref
            ratio, at = _worst((got - ref).abs(), torch.zeros_like(ref))
        else:                                                     # mirror: bit for bit the stored planar value, rounded to this type
            sut, sft, _ = NP_OF[o.src_dtype]
            src = torch.from_numpy(after.view(sut)[o.src // np.dtype(sut).itemsize].view(sft).copy())
            want = src.to(o.dtype)
            ref = want.double()
            same = torch.from_numpy(raw.copy().view(np.int16 if esz == 2 else np.int32)) == want.view(torch.int16 if esz == 2 else torch.int32)
            ratio, at = (0.0, (0, 0, 0)) if bool(same.all()) else (float('inf'), tuple(torch.nonzero(~same)[0].tolist()))
        self._note(op, o.dtype, ratio, name)
        if not ratio <= 1.0:
            byte = int(o.off[at])
            raise ReplayError('%s: |got - ref| = %.3g x its bound at (c, y, x) = %s, byte %d (%s): got %r, ref %r'
                              % (name, ratio, at, byte, self.where(byte), float(got[at]), float(ref[at])))

    @staticmethod
    def _ref_of(o):
        if getattr(o, 'R', None) is None:
            res = getattr(o, 'res', None)
            if o.mode == 'zq':
                o.R = E.ref_zq(o.vz, o.Sz, o.v, o.S, res, o.dtype)
            elif o.mode == L.MODE_MUL:
                o.R = E.ref_mul(o.v, o.S, res, o.dtype)
            elif o.mode == L.MODE_GRU:
                o.R = E.ref_gru(o.v, o.S, res, o.z, o.dtype)
            else:
                o.R = E.ref_store(o.v, o.S, o.act, o.dtype, res)
        return o.R

    def _epi(self, op, name, o, got):
        Rf = self._ref_of(o)
        if not float(Rf.acc.max()) < E.QUARTER_ULP:
            raise ReplayError('%s: accumulation term %.3g of the bound is above 2^-12: the bound would be vacuous for this op (scale its inputs)'
                              % (name, float(Rf.acc.max())))
        bound = Rf.bound(o.dtype)
        widen = getattr(o, 'widen', None)
        if widen is not None:
            self.widening.setdefault(name, []).append(float((widen / bound).mean()))
            Rf.acc = Rf.acc + widen
            bound = Rf.bound(o.dtype)
        bad = got[Rf.sat] != Rf.sat_val[Rf.sat]
        if bool(bad.any()):
            raise ReplayError('%s: %d saturated elements are not exact: got %r, must be %r'
                              % (name, int(bad.sum()), got[Rf.sat][bad][:4].tolist(), Rf.sat_val[Rf.sat][bad][:4].tolist()))
        ratio, at = _worst((got - Rf.ref).abs(), bound)
        return ratio, at, Rf.ref


def _worst(err, tol):
    """Largest err / tol (0 / 0 = 0, x / 0 = inf) and its index."""
    r = torch.where(err <= tol, err / torch.clamp(tol, min=1e-300), torch.where(tol > 0, err / torch.clamp(tol, min=1e-300), torch.full_like(err, float('inf'))))
    r = torch.where((err == 0), torch.zeros_like(r), r)
    i = int(torch.argmax(r))
    return float(r.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
