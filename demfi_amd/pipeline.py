"""Host-to-host clip pipeline behind ``WindowRunner.run_clip_u8``: a ring of device frame slots (``FrameSlots``), one edge object
per output format (``BgrEdge``: BGR frames in and out; ``Y4mEdge``: Y4M payloads in and out, every window on its own plan)
and the double-buffered batch loop that drives them (``ClipPipeline``).  An edge has the same few methods whatever its format:
``upload`` one frame into a slot and ``uploaded`` after a batch's copies (h2d stream), ``run`` a batch (compute stream), ``d2h``
its outputs to pinned memory (d2h stream) and ``drain`` them to the sink; what ``run`` returns is handed back to ``d2h`` / ``drain``.

A runner of tiles (``WindowRunner(tiles=plan)``, ``demfi_amd.tiling``) has the tile's size while the slots, the outputs and
everything after them keep the frame's: ``Tiler`` crops every uploaded frame into its tiles once, each (run, tile) pair is one run
of the runner, and one stitch launch per batch pastes the kept rectangles into the full-size output buffers.  The 16-bit frames
of a high-depth Y4M stream are not cropped or stitched (``TileGrid``): the 16-bit ingest and egress kernels address a tile inside
the full frames, so every (run, tile) pair reads the frame slots and writes the output frames directly."""
import ctypes as C
import itertools
import weakref
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from . import cadence as K
from . import deint as I
from . import retime as R
from . import scene as S
from .y4m import payload_size

# int64 word positions in a demfi_u8_sink record (256 bytes: the context's "sink" buffer)
_FRAME, _HW, _ITER = L.U8Sink.frame.offset // 8, L.U8Sink.h.offset // 8, L.U8Sink.iter.offset // 8
assert (L.U8Sink.h.offset, L.U8Sink.w.offset, L.U8Sink.iter.offset) == (8 * _HW, 8 * _HW + 4, 8 * _ITER) and C.sizeof(L.U8Sink) <= 256


def fill_sink_records(a, st, s0, s1, h, w, n_tst):
    """demfi_u8_sink records into the int64 array a [..., 32]: segments 0 / 1 / 2 of the last layer = S0 / S1 / St are written to
    the device pointers s0 / s1 / st (int64 arrays that broadcast to a.shape[:-1]; 0 = not written).  A record without St
    stays all zero: disabled, its time instant writes nothing."""
    live = np.broadcast_to(st, a.shape[:-1]) != 0
    a[...] = 0
    a[..., _FRAME], a[..., _FRAME + 1], a[..., _FRAME + 2] = s0, s1, st
    a[..., _HW] = np.where(live, h | (w << 32), 0)           # int32 h, w
    a[..., _ITER] = np.where(live, n_tst - 1, 0)              # int32 iter, pad
    return a


class FrameSlots:
    """Device ring of input frame slots ``frames`` [n,h,w,3] uint8 (``dtype`` int16: the 16-bit frames of a high-depth Y4M
    stream).  ``slot_of``: frame key -> slot; ``busy[s]``: event of the compute of the batch that last read slot s."""

    def __init__(self, n, h, w, dev, dtype=torch.uint8):
        self.frames = torch.empty((n, h, w, 3), dtype=dtype, device=dev)
        self.reset()

    def reset(self):
        self.slot_of, self.key_of, self.busy, self.next = {}, [None] * len(self.frames), [None] * len(self.frames), 0

    def acquire(self, key, stream):
        """(slot of frame ``key``, must it be uploaded).  A new frame takes the ring's next slot: the frame held there is
        forgotten, and ``stream`` (the one that uploads) waits for the compute that last read it."""
        sl = self.slot_of.get(key)
        if sl is not None:
            return sl, False
        sl = self.next
        self.next = (sl + 1) % len(self.busy)
        if self.key_of[sl] is not None:
            del self.slot_of[self.key_of[sl]]
        if self.busy[sl] is not None:
            stream.wait_event(self.busy[sl])
        self.slot_of[key], self.key_of[sl] = sl, key
        return sl, True

    def release(self, key):
        """Give back the slot of frame ``key``, the one acquired last: the ring's next frame takes it."""
        sl = self.slot_of.pop(key)
        if (sl + 1) % len(self.busy) != self.next:
            raise RuntimeError('FrameSlots.release: frame %r was not the last one acquired' % (key,))
        self.key_of[sl], self.next = None, sl

    def mark_busy(self, read, ev):
        """The slots a batch read (lists of slots) stay busy until ``ev``."""
        for fr in read:
            for sl in fr:
                self.busy[sl] = ev


def consecutive(sls):
    """(first, count) of every run of consecutive slots in the list ``sls``."""
    r = 0
    while r < len(sls):
        e = r + 1
        while e < len(sls) and sls[e] == sls[e - 1] + 1:
            e += 1
        yield sls[r], e - r
        r = e


class Tiler:
    """Device side of a multi-tile plan (``demfi_amd.tiling``).  ``tin`` [nslot, n_tiles, th, tw, 3]: the tiles of every frame
    slot, cropped when the frame is uploaded (``crop``: one ``demfi_u8_tile_crop`` launch per run of consecutive new slots, on the
    upload stream), so a frame is cropped once however many windows read it, and a slot's ``busy`` event covers its tiles too.
    ``stitch``: ONE ``demfi_u8_tile_stitch`` launch pastes the tile outputs of a batch into full frames."""

    def __init__(self, plan, slots, lib, dev, max_frames):
        self.plan, self.nt, self.lib, self.slots = plan, plan.n_tiles, lib, slots
        (self.h, self.w), (self.th, self.tw) = (plan.h, plan.w), plan.tile
        self.rects = np.ascontiguousarray(plan.rects(), dtype=np.int32)
        self.rects_dev = torch.from_numpy(self.rects).to(dev)
        self.tin = torch.empty((len(slots.frames), self.nt, self.th, self.tw, 3), dtype=torch.uint8, device=dev)
        self.offs = torch.empty(max_frames * (self.nt + 1), dtype=torch.int64, device=dev)    # reused in stream order

    def crop(self, sls, stream):
        fr = self.slots.frames
        for s0, cnt in consecutive(sls):
            L.check(self.lib.demfi_u8_tile_crop(fr[s0].data_ptr(), fr.stride(0), self.tin[s0].data_ptr(), cnt, self.h, self.w, self.th,
                                                self.tw, self.nt, self.rects.ctypes.data, self.rects_dev.data_ptr(), stream.cuda_stream),
                    'u8_tile_crop')

    def stitch(self, src, src_offs, dst, dst_offs, stream):
        """Frame f = the tiles at src + src_offs[f, j] -> the frame at dst + dst_offs[f] (numpy int64 byte offsets)."""
        n = len(dst_offs)
        if n == 0:
            return
        od = self.offs[:n * (self.nt + 1)]
        od.copy_(torch.from_numpy(np.concatenate([np.asarray(src_offs, np.int64).reshape(-1), np.asarray(dst_offs, np.int64)])).pin_memory(),
                 non_blocking=True)
        L.check(self.lib.demfi_u8_tile_stitch(src.data_ptr(), od.data_ptr(), dst.data_ptr(), od[n * self.nt:].data_ptr(), n, self.h, self.w,
                                              self.th, self.tw, self.nt, self.rects.ctypes.data, self.rects_dev.data_ptr(),
                                              stream.cuda_stream), 'u8_tile_stitch')


class TileGrid:
    """A multi-tile plan for the 16-bit frames of the Y4M edge: the sizes ``Tiler`` gives, and no device side.  The ingest of a
    (run, tile) pair reads its source rectangle out of the full frame slots and its egress writes its kept rectangle into the full
    output frames (``WindowRunner._u16_tile_io``), so there is nothing to crop into and nothing to stitch from."""

    def __init__(self, plan):
        self.plan, self.nt = plan, plan.n_tiles
        (self.h, self.w), (self.th, self.tw) = (plan.h, plan.w), plan.tile


class BgrEdge:
    """uint8 BGR [h,w,3] frames in; sink(k, St [M-1,h,w,3], S0S1 [2,h,w,3]) out (views of pinned staging buffers).  Tiled: window w
    is the n_tiles runs w * n_tiles + j into ``tout`` / ``ts01``; out and s01 are then halves of one buffer (one stitch launch)."""

    def __init__(self, runner, batch, slots, tiler=None):
        self.rn, self.slots, self.tiler = runner, slots, tiler
        self.fh, self.fw = (tiler.h, tiler.w) if tiler else (runner.h, runner.w)
        dev, shape, m1 = runner.engine.device, (self.fh, self.fw, 3), runner.mfi - 1
        if tiler:
            def halves(n, sh):                       # [n, M-1] + sh and [n, 2] + sh in one allocation
                buf, cut = torch.empty((n * (m1 + 2),) + sh, dtype=torch.uint8, device=dev), n * m1
                return buf, buf[:cut].view((n, m1) + sh), buf[cut:].view((n, 2) + sh)
            self.buf, self.out, self.s01 = zip(*[halves(batch, shape) for _ in range(2)])
            self.tbuf, self.tout, self.ts01 = halves(batch * tiler.nt, (tiler.th, tiler.tw, 3))
            self._stitch_offs = {}
        else:
            self.out = [torch.empty((batch, m1) + shape, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.s01 = [torch.empty((batch, 2) + shape, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.h_out = [torch.empty((batch, runner.mfi - 1) + shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.h_s01 = [torch.empty((batch, 2) + shape, dtype=torch.uint8).pin_memory() for _ in range(2)]

    def begin(self, yuv, window_index, first_win):
        return ()

    def upload(self, sl, idx, f):
        if tuple(f.shape) != (self.fh, self.fw, 3) or f.dtype != torch.uint8:
            raise ValueError('frame %d: expected uint8 [%d,%d,3], got %s %s' % (idx, self.fh, self.fw, f.dtype, tuple(f.shape)))
        self.slots.frames[sl].copy_(f, non_blocking=True)

    def uploaded(self, new, h2d):
        if self.tiler:
            self.tiler.crop([sl for _, sl in new], h2d)

    def run(self, i, n, wins, frames, cur):
        cnt, tl = len(wins), self.tiler
        if not tl:
            self.rn.run_windows_u8([[self.slots.frames[sl] for sl in fr] for fr in frames], out=self.out[i][:cnt], s01=self.s01[i][:cnt])
            return cnt, frames
        nt = tl.nt
        self.rn.run_windows_u8([[tl.tin[sl, j] for sl in fr] for fr in frames for j in range(nt)], out=self.tout[:cnt * nt],
                               s01=self.ts01[:cnt * nt])
        offs = self._stitch_offs.get(cnt)
        if offs is None:                             # frame (w, p) of out, then of s01: its tiles are rows w * nt + j of tout / ts01
            m1, fsz, tsz = self.rn.mfi - 1, self.out[i][0, 0].numel(), self.tout[0, 0].numel()
            w, j = np.arange(cnt, dtype=np.int64)[:, None, None], np.arange(nt, dtype=np.int64)[None, None, :]
            src, dst = [], []
            for k, d0, s0 in ((m1, 0, 0), (2, self.out[i].numel(), self.tout.numel())):
                p = np.arange(k, dtype=np.int64)[None, :, None]
                src.append((s0 + ((w * nt + j) * k + p) * tsz).reshape(-1, nt))
                dst.append((d0 + (w * k + p) * fsz)[:, :, 0].reshape(-1))
            offs = self._stitch_offs[cnt] = (np.concatenate(src), np.concatenate(dst))
        tl.stitch(self.tbuf, offs[0], self.buf[i], offs[1], cur)
        return cnt, frames

    def d2h(self, i, cnt):
        self.h_out[i][:cnt].copy_(self.out[i][:cnt], non_blocking=True)
        self.h_s01[i][:cnt].copy_(self.s01[i][:cnt], non_blocking=True)

    def drain(self, i, k0, cnt, sink):
        for j in range(cnt):
            sink(k0 + j, self.h_out[i][j], self.h_s01[i][j])


class Y4mEdge:
    """Y4M payloads in; sink(k, payloads [c, P]) out, the c output frames window k owns in stream order.  Window k runs the
    instants of ``retime.window_plan`` for the runner's ratio (x M is r = M), with ``cuts`` those of ``scene.window_runs`` (a
    cut window is two runs); run w of a batch writes its frames to comb[i][w] = [S0, St x J, S1], J = ceil(r), and one gather
    launch per batch puts the outputs in stream order.  ``full``: the full-length timeline of ``retime``.
    ``depth`` > 8: payloads of 16-bit samples at that bit depth.  The payload buffers stay uint8 tensors sized in bytes (what the
    host hands over and gets back); the frame slots and ``comb`` are int16 storage of the uint16 frames, the three launches
    are the 16-bit ones (strides and offsets in samples), the egress is the emit path and the SADs count samples.
    ``layout``: the payloads' chroma layout (``y4m.LAYOUTS``): it sets P, and for 4:2:2, 4:4:4 and mono the two conversion
    launches are those of the layouts family; everything between them sees BGR frames.  ``yuv_calls`` picks the launches.
    ``tiler``: a ``Tiler`` (8-bit frames: crop, run into ``tcomb``, stitch) or a ``TileGrid`` (16-bit frames: every tile run reads
    the slots and writes comb[i] in place).
    ``fields``: None, or the field order 't' / 'b' of an interlaced input (``demfi_amd.deint``): frame index f is then field f, its
    payload is uploaded as it is, and ONE ``demfi_yuv_bob`` launch per run of consecutive slots rebuilds the rows of the other field
    in place (upload stream) before anything reads yuv_in: the conversion, the scene SADs and the block counts see progressive
    payloads.
    ``deint_mode`` 'adaptive' (with ``fields``; 'bob' is the above): field f is rebuilt by ONE ``demfi_yuv_deint_adaptive`` launch per
    batch (at most 64 fields each) that also reads the kept rows of fields f-2, f-1, f+1 and f+2 out of THEIR slots, so those
    must have been uploaded (``around`` names them to the batch loop, which makes them resident: two fields of lookahead, and at
    the start of a block the two fields before it) but need not have been rebuilt, nor stay raw: a launch reads only kept rows and
    writes only missing ones (the hazard rule of csrc/deint.hip).  A field is rebuilt in the batch that first names it in a window
    (or as the scene detector's predecessor frame); until then it is ``raw``, and the conversion, the scene SADs and the tile crops
    are run for the fields just rebuilt, not for those just uploaded.  No payload is uploaded more often than by the bob: once per
    field."""

    def __init__(self, runner, batch, slots, cuts, full, tiler=None, depth=8, layout='420', dedup=None, h2d=None, fields=None,
                 deint_mode='bob'):
        self.rn, self.slots, self.cuts, self.full, self.tiler = runner, slots, cuts, full, tiler
        if fields not in (None, 't', 'b'):
            raise ValueError("Y4mEdge: fields must be None, 't' or 'b', got %r" % (fields,))
        if deint_mode not in I.MODES or (deint_mode != 'bob' and (fields is None or dedup is not None)):
            raise ValueError('Y4mEdge: deint_mode %r with fields=%r, dedup=%r' % (deint_mode, fields, dedup))
        self.fields, self.adaptive, self.raw = fields, deint_mode == 'adaptive', {}
        self.dedup, self.h2d, self.kept, self._pending = dedup, h2d, None, []
        self.depth, self.hi = depth, depth > 8
        self.layout = layout
        if tiler is not None and self.hi != isinstance(tiler, TileGrid):
            raise ValueError('Y4mEdge: %d-bit frames with a %s' % (depth, type(tiler).__name__))
        self.in_place = self.hi and tiler is not None                    # tiles addressed inside the full frames
        es, fdt = (2, torch.int16) if self.hi else (1, torch.uint8)      # bytes per sample; storage of a frame value
        self.es = es
        self.r = runner.retime if runner.retime is not None else Fraction(runner.mfi)
        h, w = self.fh, self.fw = (tiler.h, tiler.w) if tiler else (runner.h, runner.w)
        dev, nsl = runner.engine.device, len(slots.frames)
        P, J = self.P, self.J = payload_size(h, w, layout), R.max_instants(self.r)
        nJ = -(-J // runner.n_ctx) * runner.n_ctx if runner.tb else J    # instants incl. the padding of a short chunk
        runs_max = batch * max_runs(self.r, cuts, dedup)                 # a cut window is two runs
        # payloads of a batch: at most J per window, plus the last window's S1 (full-length: its [n-2, n) span, 2 J)
        nout = (batch + 1) * J if full else batch * J + 1
        if dedup is not None:                        # a window spans up to max_hold + 1 input frames, and so does the last one's hold
            nout = (batch + 1) * K.max_window_instants(self.r, dedup[3]) + 1
        Pb = self.Pb = P * es                                            # bytes of a payload of P samples
        self.yuv_in = torch.empty((nsl, Pb), dtype=torch.uint8, device=dev)
        self.comb = [torch.empty((runs_max, J + 2, h, w, 3), dtype=fdt, device=dev) for _ in range(2)]
        nt = tiler.nt if tiler else 1                                    # tiled: run w is the runs w * nt + j of the tile runner
        if tiler and not self.in_place:   # their frames; one buffer serves both sets: the stitch has read it before the next batch's runs start
            self.tcomb = torch.empty((runs_max * nt, J + 2, tiler.th, tiler.tw, 3), dtype=torch.uint8, device=dev)
        self.t = [torch.empty((runs_max * nt, nJ), dtype=torch.float32, device=dev) for _ in range(2)]
        self.sinks = [torch.empty((runs_max * nt, nJ, 32), dtype=torch.int64, device=dev) for _ in range(2)]
        self.offs = [torch.empty(nout, dtype=torch.int64, device=dev) for _ in range(2)]
        self.yuv_out = [torch.empty((nout, Pb), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.h_yuv = [torch.empty((nout, Pb), dtype=torch.uint8).pin_memory() for _ in range(2)]
        if self.adaptive:                            # five payload offsets per field rebuilt in a batch (at most nsl); reused in stream order
            self.dei_offs = torch.empty(5 * nsl, dtype=torch.int64, device=dev)
        if cuts:                                     # SADs of a batch's new frames (at most nsl) against their predecessors
            self.d_sad = torch.empty(nsl, dtype=torch.int64, device=dev)
            self.sad_offs = torch.empty(2 * nsl, dtype=torch.int64, device=dev)
            self.h_sad = torch.empty(nsl, dtype=torch.int64).pin_memory()
        if dedup is not None:                        # block counts of one (frame, last kept frame) pair; pinned buffers are reused:
            self.cnt = torch.empty(2, dtype=torch.int32, device=dev)         # every probe ends with a wait for its answer
            self.cnt_offs = torch.empty(2, dtype=torch.int64, device=dev)
            self.h_cnt = torch.empty(2, dtype=torch.int32).pin_memory()
            self.h_cnt_offs = torch.empty(2, dtype=torch.int64).pin_memory()
        self.yuv = self.window_index = self.det = self.to_bgr = self.gather = self.sad = None

    # ---- repeated frames (``cadence``): the windows generator (``KeptFrames``) stages, scores and keeps frames through these ----
    def attach(self, kept):
        """A --dedup run starts, before its first window is asked for: ``kept`` (``KeptFrames``) will stage frames here."""
        self.kept, self._pending = kept, []
        kept.edge = self

    def stage(self, key, idx, f):
        """Input frame idx, the candidate for kept index ``key``, is copied into the ring's next slot (upload stream)."""
        with torch.cuda.stream(self.h2d):
            sl, _ = self.slots.acquire(key, self.h2d)
            self.upload(sl, idx, f)
            self._bob([(idx, sl)], self.h2d)
        return sl

    def block_counts(self, sl, ref):
        """(hot, warm) of the payload in slot sl against the one in slot ref: ONE ``demfi_luma_block_counts`` launch on the
        upload stream behind the copy, read back with one event wait (the next frame is compared with whichever of the two
        is kept, so frames are scored one by one)."""
        hi, lo = self.dedup[0] << (self.depth - 8), self.dedup[1] << (self.depth - 8)
        with torch.cuda.stream(self.h2d):
            self.h_cnt_offs[0], self.h_cnt_offs[1] = sl * self.Pb, ref * self.Pb
            self.cnt_offs.copy_(self.h_cnt_offs, non_blocking=True)
            L.check(self.rn.lib.demfi_luma_block_counts(self.yuv_in.data_ptr(), self.cnt_offs.data_ptr(), self.cnt_offs[1:].data_ptr(), 1,
                                                        self.fh, self.fw, 2 if self.hi else 1, hi, lo, self.cnt.data_ptr(),
                                                        self.h2d.cuda_stream), 'luma_block_counts')
            self.h_cnt.copy_(self.cnt, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.h2d)
        ev.synchronize()
        hot, warm = self.h_cnt.tolist()
        return hot, warm

    def keep(self, key, sl):
        """The staged frame is kept: it is converted with the next batch's uploads."""
        self._pending.append((key, sl))

    def discard(self, key):
        """The staged frame repeats the last kept one: its slot is recycled at once."""
        self.slots.release(key)

    def begin(self, yuv, window_index, first_win):
        """A run starts; returns the frames to make resident before its first batch.  Scene cuts: the block's first window
        k0 >= 1 also needs frame k0 - 1, the predecessor SAD_k0 is taken against."""
        self.yuv, self.window_index, self.det = yuv, window_index, None
        self.raw = {}
        self.to_bgr, self.gather, self.sad = yuv_calls(self.rn.lib, self.depth, self.layout, self.fh, self.fw, yuv)
        if not self.cuts:
            return ()
        det = self.det = S.Detector(self.P, yuv.scene_cut, first=S.first_frame(window_index(0) if window_index is not None else first_win[2]),
                                    peak=(1 << self.depth) - 1)
        self.rn.last_cuts = det.cuts
        return (det.next - 1,) if det.next - 1 < first_win[2] else ()

    def upload(self, sl, idx, f):
        if tuple(f.shape) != (self.Pb,) or f.dtype != torch.uint8:
            raise ValueError('frame %d: expected a uint8 [%d] %s payload, got %s %s' % (idx, self.Pb, self.layout, f.dtype, tuple(f.shape)))
        self.yuv_in[sl].copy_(f, non_blocking=True)

    def _bob(self, new, stream):
        """Interlaced input: the payloads just copied to yuv_in[slot] for the (field index, slot) pairs ``new`` become progressive
        frames in place, one ``demfi_yuv_bob`` launch per run of consecutive slots (at most 64 payloads each) on ``stream``."""
        if self.fields is None or not new:
            return
        q = {sl: I.field_parity(self.fields, idx) for idx, sl in new}
        for s0, cnt in consecutive([sl for _, sl in new]):
            for c0 in range(s0, s0 + cnt, 64):
                c = min(64, s0 + cnt - c0)
                L.check(self.rn.lib.demfi_yuv_bob(self.yuv_in[c0].data_ptr(), self.Pb, c, self.fh, self.fw, L.YUV_LAYOUT[self.layout], self.es,
                                                  sum(q[c0 + j] << j for j in range(c)), stream.cuda_stream), 'yuv_bob')

    def around(self, needed, has):
        """Adaptive mode: the fields a batch that names the fields ``needed`` must find uploaded besides them, in order: fields
        f-2 .. f+2 of every field f of ``needed`` that is not rebuilt yet, as far as the input has them (``has``)."""
        if not self.adaptive:
            return []
        self._needed, self._has = sorted(set(needed)), has
        todo = [f for f in self._needed if f in self.raw or f not in self.slots.slot_of]
        return sorted({g for f in todo for g in range(max(f - 2, 0), f + 3) if g not in needed and (g < f or has(g))})

    def _adaptive(self, new, stream):
        """The fields of this batch that are still raw become progressive frames in place; returns them as (field, slot) pairs."""
        slot_of = self.slots.slot_of
        self.raw.update(new)
        self.raw = {f: sl for f, sl in self.raw.items() if slot_of.get(f) == sl}     # a slot the ring took back is forgotten
        todo = [f for f in self._needed if f in self.raw]
        done = 0
        for c0 in range(0, len(todo), 64):
            fs = todo[c0:c0 + 64]
            for f in fs:                             # a field of the input that is not resident must not pass for an absent one
                gone = [g for g in range(max(f - 2, 0), f + 3) if g not in slot_of and (g < f or self._has(g))]
                if gone:
                    raise RuntimeError('adaptive deinterlacing: field %d needs field %d, which is not resident' % (f, gone[0]))
            offs = [slot_of[g] * self.Pb if g in slot_of else -1 for f in fs for g in range(f - 2, f + 3)]
            host = torch.tensor(offs, dtype=torch.int64).pin_memory()
            od = self.dei_offs[5 * done:5 * (done + len(fs))]
            od.copy_(host, non_blocking=True)
            L.check(self.rn.lib.demfi_yuv_deint_adaptive(self.yuv_in.data_ptr(), self.yuv_in.numel(), host.data_ptr(), od.data_ptr(), len(fs),
                                                         self.fh, self.fw, L.YUV_LAYOUT[self.layout], self.es,
                                                         sum(I.field_parity(self.fields, f) << j for j, f in enumerate(fs)),
                                                         stream.cuda_stream), 'yuv_deint_adaptive')
            done += len(fs)
        return [(f, self.raw.pop(f)) for f in todo]

    def uploaded(self, new, h2d):
        """Payloads copied to yuv_in[slot] (interlaced input: bobbed there first, or in adaptive mode the batch's fields rebuilt
        there, which then take the place of ``new``) -> BGR frame slots, one launch per run of consecutive slots; then the SADs."""
        if self.adaptive:
            new = self._adaptive(new, h2d)
        else:
            self._bob(new, h2d)                      # the frames staged by --dedup were bobbed when they were staged
        if self._pending:                            # --dedup: the kept frames staged since the last batch
            new, self._pending = self._pending + list(new), []
        sls = [sl for _, sl in new]
        for s0, cnt in consecutive(sls):
            self.to_bgr(self.yuv_in[s0].data_ptr(), self.slots.frames[s0].data_ptr(), cnt, h2d.cuda_stream)
        if self.tiler and not self.in_place:
            self.tiler.crop(sls, h2d)
        if self.det is not None:
            self._scene_sads([idx for idx, _ in new], h2d)

    def _scene_sads(self, new_frames, h2d):
        """SAD_j of every frame j just uploaded against frame j-1 (``demfi_yuv420_sad``, ONE launch on the h2d stream after the
        copies), read back with one event wait and handed to the detector in frame order.  Call under the h2d stream.
        Frame j-1 is resident: it was uploaded in this batch or in the previous one (windows are consecutive), and a slot is
        reused only after all nslot >= 2 * batch + 8 slots have been (adaptive deinterlacing: nslot >= 2 * batch + 12, and batch b
        uploads up to frame k + 2 * batch + 4, its two fields of lookahead included, so it takes back the slots of frames up to
        k - 8 at most, while batch b-1 reads frames from k - 1 on and its rebuild launches, queued on h2d before, from k - 3 on).
        The wait does not wait on the compute stream: the
        ``busy`` waits queued on h2d before this batch's copies are on the compute of the batch that last read a reused
        slot, and that batch is at least two back (batch b-1 reads frames k .. k + batch + 2 of its first window k, batch b
        uploads frames up to k + 2 * batch + 2 only), so the host already waited for it when it drained that batch's D2H."""
        det, slot_of, P = self.det, self.slots.slot_of, self.P
        js = sorted(j for j in new_frames if j >= det.next)
        if not js:
            return
        if any(j - 1 not in slot_of for j in js):
            raise RuntimeError('scene cuts: the predecessor of frame %d is not resident' % min(j for j in js if j - 1 not in slot_of))
        m = len(js)
        offs = [slot_of[j - 1] * P for j in js] + [slot_of[j] * P for j in js]
        od = self.sad_offs[:2 * m]
        od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
        self.sad(self.yuv_in.data_ptr(), od.data_ptr(), od[m:].data_ptr(), m, self.d_sad.data_ptr(), h2d.cuda_stream)
        self.h_sad[:m].copy_(self.d_sad[:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(h2d)
        ev.synchronize()
        for j, sad in zip(js, self.h_sad[:m].tolist()):
            det.push(j, sad)

    def run(self, i, n, wins, frames, cur):
        """Plans the batch's windows (window n + wi of the sequence is window ``window_index(n + wi)``, else B-1 of its unclamped
        tuple), runs them and gathers their outputs into yuv_out[i].  Returns (payloads per window, slots read)."""
        rn, yuv, det, slot_of = self.rn, self.yuv, self.det, self.slots.slot_of
        runs, outs = [], []                          # runs: (slots, instants, kinds kept); outs[w]: (run, kind, instant index)
        for wi, win in enumerate(wins):
            k = self.window_index(n + wi) if self.window_index is not None else win[2]
            last = yuv.with_s1(n + wi)
            if self.kept is not None:                # --dedup: the plans of ``cadence`` over the kept frames; slots by kept index
                kf = self.kept
                sr, so = K.window_runs(k, self.r, kf.s, kf.n, det.is_cut if det is not None else None, self.full)
                wr = [([slot_of[x] for x in S.runner_order(tup)], ts) for tup, ts in sr]
                o = [(run, kind, j) for _, run, kind, j in so]
                rn.cut_windows += int(K.is_cut_window(k, det.is_cut if det is not None else None))
                kf.st_frames += sum(kind == R.ST for _, kind, _ in o)
            elif det is None:
                ts, o = R.window_plan(k, self.r, last, self.full)
                wr, o = [(frames[wi], ts)], [(0, kind, j) for _, kind, j in o]
            else:
                is_cut = S.with_sentinels(det.is_cut, k + 3 if last else None) if self.full else det.is_cut
                sr, so = S.window_runs(k, self.r, last, is_cut, self.full)
                wr = [([slot_of[x] for x in S.runner_order(tup)], ts) for tup, ts in sr]
                o = [(run, kind, j) for _, run, kind, j in so]
                rn.cut_windows += len(sr) - 1
            outs.append([(len(runs) + run, kind, j) for run, kind, j in o])
            runs += [(fr, ts, {kind for run, kind, _ in o if run == ri}) for ri, (fr, ts) in enumerate(wr)]
        self._run_windows(i, runs)
        return self._gather(i, outs, cur), [fr for fr, _, _ in runs]

    def _run_windows(self, i, runs):
        """Run w = (4 slots, instants, kinds) runs its instants into comb[i][w].  The t values (padded slots repeat the last t)
        and the uint8 sink records (one per (run, instant); S0 / S1 only in the row of the run's first instant and only when
        ``kinds`` holds that frame; rows past a run's instants disabled) are uploaded on the current stream.
        Tiled: every run is one run per tile, on that tile of its slots into tcomb, and the frames written are then stitched
        into comb[i] in one launch.  Tiled 16-bit frames: run w is the tile runs w * nt + j, each from the full slots into its
        kept rectangle of comb[i][w]; the rectangles of a frame are disjoint, so the runs need no order among themselves."""
        rn, J, tl = self.rn, self.J, self.tiler
        if self.in_place:
            comb = self.comb[i]
            runs = [([self.slots.frames[sl] for sl in fr], ts, kinds) for fr, ts, kinds in runs for _ in range(tl.nt)]
        elif tl:
            full, comb = runs, self.tcomb
            runs = [([tl.tin[sl, j] for sl in fr], ts, kinds) for fr, ts, kinds in full for j in range(tl.nt)]
        else:
            comb, runs = self.comb[i], [([self.slots.frames[sl] for sl in fr], ts, kinds) for fr, ts, kinds in runs]
        nw, nJ = len(runs), self.t[i].shape[1]
        tt = np.empty((nw, nJ), np.float32)
        st = np.zeros((nw, nJ), np.int64)
        s01 = np.zeros((2, nw, nJ), np.int64)
        base, (c0, c1) = comb.data_ptr(), comb.stride()[:2]              # uint8: element strides are bytes
        for w, (_, ts, kinds) in enumerate(runs):
            tt[w, :len(ts)] = ts
            tt[w, len(ts):] = ts[-1]
            if self.hi:                              # no sink records: every 16-bit frame leaves through the emit path
                continue
            st[w, :len(ts)] = base + w * c0 + c1 * np.arange(1, len(ts) + 1)
            s01[0, w, 0] = base + w * c0 if R.S0 in kinds else 0
            s01[1, w, 0] = base + w * c0 + (J + 1) * c1 if R.S1 in kinds else 0
        t_dev = self.t[i][:nw]
        t_dev.copy_(torch.from_numpy(tt).pin_memory(), non_blocking=True)
        rows = None
        if rn.engine.supports_u8_sink and not self.hi:
            a = fill_sink_records(np.empty((nw, nJ, 32), np.int64), st, s01[0], s01[1], rn.h, rn.w, rn.n_tst)
            rows = self.sinks[i][:nw]
            rows.copy_(torch.from_numpy(a).pin_memory(), non_blocking=True)
        if self.in_place:
            nt, tiles = tl.nt, tl.plan.tiles
            io = [rn._u16_tile_io(fr, tiles[w % nt], comb[w // nt, 1:J + 1], comb[w // nt, 0::J + 1], self.depth) for w, (fr, _, _) in enumerate(runs)]
        elif self.hi:
            io = [rn._u16_io(fr, comb[w, 1:J + 1], comb[w, 0::J + 1], self.depth) for w, (fr, _, _) in enumerate(runs)]
        else:
            io = [rn._u8_io(fr, comb[w, 1:J + 1], comb[w, 0::J + 1], None if rows is None else rows[w]) for w, (fr, _, _) in enumerate(runs)]
        cur = rn._begin()
        for w, (load, emit, pre) in enumerate(io):
            rn._window(load, emit, body_only=True, pre=pre, t_dev=t_dev[w], nt=len(runs[w][1]))
        rn._end(cur)
        if tl and not self.in_place:
            (c0, c1), (t0, t1), j = self.comb[i].stride()[:2], comb.stride()[:2], np.arange(tl.nt, dtype=np.int64)
            pos = [(w, p) for w, (_, ts, kinds) in enumerate(full)
                   for p in ([0] if R.S0 in kinds else []) + list(range(1, len(ts) + 1)) + ([J + 1] if R.S1 in kinds else [])]
            tl.stitch(comb, [(w * tl.nt + j) * t0 + p * t1 for w, p in pos], self.comb[i], [w * c0 + p * c1 for w, p in pos], cur)

    def _gather(self, i, outs, cur):
        """Outputs of a batch (comb[i]) -> yuv_out[i] in stream order: ONE gather launch on the compute stream.  outs[w]:
        window w's outputs as (run, kind, instant index).  Returns the number of payloads per window."""
        comb, dst, J = self.comb[i], self.yuv_out[i], self.J
        c0, c1 = comb.stride()[:2]
        offs = [run * c0 + (0 if kind == R.S0 else J + 1 if kind == R.S1 else 1 + j) * c1 for o in outs for run, kind, j in o]
        nf = len(offs)
        if nf > dst.shape[0]:
            raise RuntimeError('retime: %d outputs for %d payload slots' % (nf, dst.shape[0]))
        od = self.offs[i][:nf]
        od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
        self.gather(comb.data_ptr(), od.data_ptr(), dst.data_ptr(), nf, cur.cuda_stream)
        return [len(o) for o in outs]

    def d2h(self, i, counts):
        nf = sum(counts)
        self.h_yuv[i][:nf].copy_(self.yuv_out[i][:nf], non_blocking=True)

    def drain(self, i, k0, counts, sink):
        pos = 0
        for j, c in enumerate(counts):
            sink(k0 + j, self.h_yuv[i][pos:pos + c])
            pos += c


def yuv_calls(lib, depth, layout, h, w, yuv):
    """The three launches of the Y4M edge for h x w frames of (depth, layout), bound to the stream's matrix, range and siting
    (``yuv``): to_bgr(src, dst, cnt, stream) converts cnt consecutive payloads to BGR frames, gather(base, offs, dst, n, stream)
    converts the n frames at base + offs[] to consecutive payloads, sad(base, a, b, m, out, stream) scores m payload pairs.
    Pointers are addresses; every stride and offset counts samples, which are bytes at depth 8.  4:2:0 has C functions of its own
    (8-bit: csrc/yuv.hip), 4:2:2, 4:4:4 and mono those of the layouts family, which take the layout code; the 16-bit functions
    take the depth; only 4:2:0 has a siting."""
    hi, lc, P, F = depth > 8, L.YUV_LAYOUT[layout], payload_size(h, w, layout), h * w * 3
    if lc:
        names = ('yuvl16_to_bgr16', 'bgr16_to_yuvl16_gather') if hi else ('yuvl_to_bgr', 'bgr_to_yuvl_gather')
    else:
        names = ('yuv420p16_to_bgr16', 'bgr16_to_yuv420p16_gather') if hi else ('yuv420_to_bgr', 'bgr_to_yuv420_gather')
    names += ('yuv420p16_sad' if hi else 'yuv420_sad',)
    c_bgr, c_gather, c_sad = (getattr(lib, 'demfi_' + nm) for nm in names)
    fmt = ((depth,) if hi else ()) + ((lc,) if lc else ()) + (yuv.matrix, int(yuv.full_range))
    site = () if lc else (yuv.siting,)

    def to_bgr(src, dst, cnt, stream):
        L.check(c_bgr(src, P, dst, F, cnt, h, w, *fmt, *site, stream), names[0])

    def gather(base, offs, dst, n, stream):
        L.check(c_gather(base, offs, dst, P, n, h, w, *fmt, stream), names[1])

    def sad(base, a, b, m, out, stream):
        L.check(c_sad(base, a, b, m, P, out, stream), names[2])
    return to_bgr, gather, sad


def max_runs(r, cuts, dedup):
    """Upper bound of the runs of one window of the Y4M edge: a cut window is two; with ``dedup`` = (hi, lo, frac, max_hold) a
    window that spans several input frames is split into runs of at most ``retime.max_instants(r)`` instants."""
    return max(2 if cuts else 1, K.max_window_runs(r, dedup[3]) if dedup is not None else 1)


def pipeline_key(batch, y4m, cuts, full, depth=8, layout='420', dedup=None, fields=None, deint_mode='bob'):
    """What a cached ``ClipPipeline`` can be reused for."""
    return ((batch, y4m, cuts, full, depth, layout) + ((tuple(dedup),) if dedup is not None else ()) + (('fields', fields) if fields else ())
            + (('deint', deint_mode) if fields and deint_mode != 'bob' else ()))


class KeptFrames:
    """``host_frames`` and ``windows`` of a --dedup run: the kept frames of an input (``y4m.Frames`` ``raw``), indexed by kept
    index.  Pulling ``windows()`` reads the input: every frame is staged in a device slot and scored there against the last
    kept frame (``Y4mEdge.stage`` / ``block_counts``), a repeat's slot is recycled at once, and window k is handed out when
    ``cadence.ready`` says it can be planned -- B2 or the end of the input is known.  So the pipeline finds every frame a
    window names already resident, and only kept frames occupy slots.  ``det``: the ``cadence.Detector``; ``s`` its kept
    times, ``n`` the input's length once its end was seen, ``first_window`` the first window handed out, ``st_frames`` the St
    frames planned."""

    def __init__(self, raw, det, r, full_length=False):
        self.raw, self.det, self.r, self.full = raw, det, Fraction(r), bool(full_length)
        self.s, self.n, self.first_window, self.edge, self.ref, self.st_frames = det.kept, None, None, None, None, 0

    def __getitem__(self, j):
        raise IndexError('kept frame %d is not resident: --dedup stages every frame before a window names it' % j)

    def index(self, j):
        """Window index of the j-th window handed out."""
        return self.first_window + j

    def _probe(self):
        """Examines the next input frame; False at the end of the input."""
        det, i = self.det, self.det.next
        if not self.raw.has(i):
            self.n = i
            return False
        key = len(det.kept)
        sl = self.edge.stage(key, i, self.raw[i])
        if det.push(i, None if det.forced() else self.edge.block_counts(sl, self.ref)):
            self.ref = sl
            self.edge.keep(key, sl)
        else:
            self.edge.discard(key)
        return True

    def _know(self, k):
        """Reads on until window k can be planned."""
        while self.n is None:
            if len(self.s) > k + 2 and not self.full:
                self.raw.has(self.s[k + 2] + 2)      # read ahead only: is tau = s_{k+2} the last output?
            if K.ready(k, self.s, self.raw.next, None, self.full) or not self._probe():
                return

    def windows(self):
        """(B0, B1, B-1, B2), kept indices clamped at the ends of the kept sequence, of every window in order."""
        while self.n is None and len(self.s) < 2:
            self._probe()
        if not self.s:
            return
        if len(self.s) == 1:                         # the end was seen: one kept frame, held
            if R.n_output_frames(self.n, self.r, self.full) > 0:
                self.first_window = -2
                yield (0, 0, 0, 0)
            return
        k = -1
        while True:
            self._know(k)
            if self.n is not None and k + 2 > len(self.s) - 1:
                return
            if K.window_outputs(k, self.r, self.s, self.n, self.full):
                if self.first_window is None:
                    self.first_window = k
                yield S.runner_order(K.window_tuple(k, self.s, self.n))
            elif self.first_window is not None:
                return                               # past the last output
            k += 1


class ClipPipeline:
    """The batch loop of ``WindowRunner.run_clip_u8`` for one batch size and one edge (BGR, or Y4M with or without scene
    cuts / the full-length timeline, which size its buffers): H2D of a batch's new frames, its compute, the drain of the
    previous batch and its D2H, on three streams over two sets of output buffers."""

    def __init__(self, runner, batch, y4m, cuts, full, depth=8, layout='420', dedup=None, fields=None, deint_mode='bob'):
        dev = self.dev = runner.engine.device
        runner = weakref.proxy(runner)               # the runner owns this pipeline: no reference cycle keeps its buffers alive
        self.batch, self.key = batch, pipeline_key(batch, y4m, cuts, full, depth, layout, dedup, fields, deint_mode)
        if depth > 8 and not y4m:
            raise ValueError('ClipPipeline: 16-bit frames are those of the Y4M edge only')
        if dedup is not None and not y4m:
            raise ValueError('ClipPipeline: repeated frames are found by the Y4M edge only')
        if fields is not None and not y4m:
            raise ValueError('ClipPipeline: fields are bobbed by the Y4M edge only')
        self.h2d, self.d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        plan = runner.tiles
        fh, fw = (plan.h, plan.w) if plan is not None else (runner.h, runner.w)
        look = 4 if fields is not None and deint_mode == 'adaptive' else 0      # two fields behind a batch's frames and two ahead
        self.slots = FrameSlots(max(2 * batch + 8 + look, 8 * batch), fh, fw, dev, torch.int16 if depth > 8 else torch.uint8)
        tiler = None
        if plan is not None and depth > 8:           # 16-bit frames: tiles are read and written inside the full frames
            tiler = TileGrid(plan)
        elif plan is not None:                       # frames stitched per batch: a run's J + 2 (a cut window is two runs), or M + 1
            J2 = (R.max_instants(runner.retime if runner.retime is not None else Fraction(runner.mfi)) + 2) if y4m else runner.mfi + 1
            rr = (runner.retime if runner.retime is not None else Fraction(runner.mfi)) if y4m else None
            tiler = Tiler(plan, self.slots, runner.lib, dev, batch * (max_runs(rr, cuts, dedup) if y4m else 1) * J2)
        self.edge = (Y4mEdge(runner, batch, self.slots, cuts, full, tiler, depth, layout, dedup, self.h2d, fields, deint_mode) if y4m
                     else BgrEdge(runner, batch, self.slots, tiler))

    def run(self, host_frames, windows, sink, reuse_frames, yuv, window_index):
        edge, slots, h2d, cur = self.edge, self.slots, self.h2d, torch.cuda.current_stream(self.dev)
        slots.reset()
        if getattr(edge, 'dedup', None) is not None:  # --dedup: ``windows`` stages and scores frames as it is pulled
            edge.attach(host_frames)
        it = iter(windows)
        wins = list(itertools.islice(it, self.batch))
        if not wins:
            return 0
        extra = edge.begin(yuv, window_index, wins[0])
        around = edge.around if getattr(edge, 'adaptive', False) else None
        if around is not None and not reuse_frames:
            raise ValueError('ClipPipeline: adaptive deinterlacing needs reuse_frames (slots are keyed by field)')
        has = getattr(host_frames, 'has', lambda i: 0 <= i < len(host_frames))
        ev_d2h = [None, None]             # D2H of the batch that last wrote output buffer i
        pending = None                    # (buffer, first window, what edge.run returned) of the batch whose D2H is in flight
        n = b = 0
        while wins:
            i = b & 1
            # ---- H2D of the frames this batch needs (copy stream) -------------------------------------------------
            new = []                      # (frame, slot) uploaded for this batch

            def resident(idx, key):
                sl, fresh = slots.acquire(key, h2d)
                if fresh:
                    edge.upload(sl, idx, host_frames[idx])
                    new.append((idx, sl))
                return sl
            with torch.cuda.stream(h2d):
                if around is not None:    # raw fields next to this batch's in time: those before them first (frames are read in order)
                    named = set(extra).union(*wins)
                    near = around(named, has)
                    for idx in near:
                        if idx < min(named):
                            resident(idx, idx)
                for idx in extra:
                    resident(idx, idx)
                frames = [[resident(idx, idx if reuse_frames else (b, wi, idx)) for idx in win] for wi, win in enumerate(wins)]
                if around is not None:
                    for idx in near:
                        if idx > min(named):
                            resident(idx, idx)
                edge.uploaded(new, h2d)
                ev_up = torch.cuda.Event()
                ev_up.record(h2d)
            # ---- compute (pipelined windows) ---------------------------------------------------------------------
            cur.wait_event(ev_up)
            if ev_d2h[i] is not None:
                cur.wait_event(ev_d2h[i])                     # the D2H of batch b-2 has read this output buffer
            res, read = edge.run(i, n, wins, frames, cur)
            ev = torch.cuda.Event()
            ev.record(cur)
            slots.mark_busy(read, ev)
            # ---- hand the previous batch to the sink while this one computes ------------------------------------------
            if pending is not None:
                self._drain(pending, ev_d2h, sink)
            # ---- D2H of this batch (copy stream), into pinned staging ------------------------------------------------
            with torch.cuda.stream(self.d2h):
                self.d2h.wait_event(ev)
                edge.d2h(i, res)
                ev_d2h[i] = torch.cuda.Event()
                ev_d2h[i].record(self.d2h)
            pending = (i, n, res)
            n, b, extra = n + len(wins), b + 1, ()
            wins = list(itertools.islice(it, self.batch))
        self._drain(pending, ev_d2h, sink)
        return n

    def _drain(self, pending, ev_d2h, sink):
        i, k0, res = pending
        ev_d2h[i].synchronize()
        if sink is not None:
            self.edge.drain(i, k0, res, sink)
