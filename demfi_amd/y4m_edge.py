"""The Y4M edge of the clip pipeline (``demfi_amd.pipeline``): Y4M payloads in and out, every window on its own plan, all options in
one ``pipeline.EdgeSpec``.  One stage per job, each with its own buffers: ``Ingest``, ``SceneScores``, ``DedupProbe``, the pure function
``plan_batch`` (``plan_fine``), a ``FrameIO`` chosen once and, behind the gather, the ``Stage`` chain that ``egress_layout`` sizes: ``Shutter``,
``Scaler``, ``Lut`` (a 3D colour LUT over RGB payloads, ``demfi_amd.lut3d``), ``Encoder`` (linear light or a LUT: the gather then writes RGB
payloads, ``demfi_amd.colour``), ``Grain``, ``Interlacer`` and ``Requantizer``, in
that order, each only when ``spec`` asks for it; ``Y4mEdge`` loops over them and keeps the
payloads' way out.

The buffer rule of the chain: a stage reads its payloads from row ``lead`` of its source buffer on (the ``lead`` rows in front are where it
carries what it holds open from one batch to the next), so a buffer has as many rows as its producer can write, plus the ``lead`` of its consumer
in front.  The gather is producer number zero, the pinned host buffers are the last consumer and read from row 0."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import cadence as K
from . import colour as CL
from . import deband as BA
from . import deblock as DB
from . import deint as I
from . import denoise as DN
from . import dering as DR
from . import grain as GR
from . import interlace as IL
from . import lut3d as LU
from . import nlmeans as NL
from . import retime as R
from . import scale as SC
from . import scene as S
from . import shutter as SH
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


def consecutive(sls):
    """(first, count) of every run of consecutive slots in the list ``sls``."""
    r = 0
    while r < len(sls):
        e = r + 1
        while e < len(sls) and sls[e] == sls[e - 1] + 1:
            e += 1
        yield sls[r], e - r
        r = e


def egress_colour(spec, yuv):
    """(matrix code, full range 0 / 1) of the payloads written: those of ``spec.colour`` = (transfer, out matrix, out full range) where it names
    them (``--out-matrix`` / ``--out-range``), else the stream's (``yuv``).  Everything behind the gather that knows the range uses these;
    everything in front of the network keeps the input's."""
    _, matrix, full = spec.colour or (None, None, None)
    return ({'bt601': L.BT601, 'bt709': L.BT709}[matrix] if matrix is not None else yuv.matrix,
            int(yuv.full_range if full is None else full))


def yuv_calls(lib, spec, h, w, yuv):
    """The three launches of the Y4M edge for h x w frames of ``spec``'s depth and layout, bound to the stream's matrix, range and siting (``yuv``;
    the gather, which makes every written sample, to ``egress_colour``: without ``spec.colour`` the same):
    to_bgr(src, dst, cnt, stream) converts cnt consecutive payloads to BGR frames, gather(base, offs, dst, n, stream) converts the n frames at base +
    offs[] to consecutive payloads, sad(base, a, b, m, out, stream) scores m payload pairs. Pointers are addresses; every stride and offset counts
    samples, which are bytes at depth 8.  4:2:0 has C functions of its own (8-bit: csrc/yuv.hip), 4:2:2, 4:4:4 and mono those of the layouts family,
    which take the layout code; the 16-bit functions take the depth; only 4:2:0 has a siting."""
    hi, lc, P, F = spec.hi, L.YUV_LAYOUT[spec.layout], payload_size(h, w, spec.layout), h * w * 3
    if lc:
        names = ('yuvl16_to_bgr16', 'bgr16_to_yuvl16_gather') if hi else ('yuvl_to_bgr', 'bgr_to_yuvl_gather')
    else:
        names = ('yuv420p16_to_bgr16', 'bgr16_to_yuv420p16_gather') if hi else ('yuv420_to_bgr', 'bgr_to_yuv420_gather')
    names += ('yuv420p16_sad' if hi else 'yuv420_sad',)
    c_bgr, c_gather, c_sad = (getattr(lib, 'demfi_' + nm) for nm in names)
    fmt = ((spec.depth,) if hi else ()) + ((lc,) if lc else ()) + (yuv.matrix, int(yuv.full_range))
    site, out = () if lc else (yuv.siting,), fmt[:-2] + egress_colour(spec, yuv)

    def to_bgr(src, dst, cnt, stream):
        L.check(c_bgr(src, P, dst, F, cnt, h, w, *fmt, *site, stream), names[0])

    def gather(base, offs, dst, n, stream):
        L.check(c_gather(base, offs, dst, P, n, h, w, *out, stream), names[1])

    def sad(base, a, b, m, out, stream):
        L.check(c_sad(base, a, b, m, P, out, stream), names[2])
    return to_bgr, gather, sad


def max_runs(r, cuts, dedup):
    """Upper bound of the runs of one window of the Y4M edge: a cut window is two; with ``dedup`` = (hi, lo, frac, max_hold) a
    window that spans several input frames is split into runs of at most ``retime.max_instants(r)`` instants."""
    return max(2 if cuts else 1, K.max_window_runs(r, dedup[3]) if dedup is not None else 1)


class Ingest:
    """Payload copied -> BGR frame slot ready.  ``yuv_in`` [nslot, Pb]: the payload of every frame slot (uint8, sized in bytes: P samples of ``es``
    bytes); ``to_frames`` converts new ones into their slots, one launch per run of consecutive slots, and crops them into their tiles (``tiler``: the
    ``pipeline.Tiler`` of an 8-bit tiled run, else None).  Interlaced input (``fields`` 't' / 'b': frame f is field f, its payload uploaded as it is)
    is first made progressive in place.  ``bob``: ONE ``demfi_yuv_bob`` launch per run of consecutive slots.  ``adaptive``: ONE
    ``demfi_yuv_deint_adaptive`` launch per batch (at most 64 fields each) that also reads the kept rows of fields f-2, f-1, f+1 and f+2 out of THEIR
    slots, so those must have been uploaded (``around`` names them to the batch loop) but need not have been rebuilt, nor stay raw: a launch reads
    only kept rows and writes only missing ones (the hazard rule of csrc/deint.hip).  A field is rebuilt in the batch that first names it in a window
    (or as the scene detector's predecessor frame); until then it is ``raw``.  No payload is uploaded more often than by the bob: once per field.
    ``spec.denoise`` = (A, B, R) (``demfi_amd.denoise``): behind the promotion and the bob ONE ``demfi_payload_denoise`` launch per batch (at most 64
    frames each) writes the denoised payload of every frame the batch names for the first time into ``clean`` [nslot, Pb], slot for slot beside
    ``yuv_in``, from the frames f - R step .. f + R step in yuv_in (step 2 over bobbed fields), which the denoiser alone reads from then on:
    ``payloads`` is the buffer everything behind it reads.  The bookkeeping is the adaptive deinterlacer's with ``reach`` = R step in place of 2:
    ``around`` names the frames to upload, a frame uploaded ahead of its window waits in ``raw``, ``rebuilt`` returns the frames just denoised.
    ``spec.deblock`` = (A, B) (``demfi_amd.deblock``): behind the promotion and in front of everything else that reads yuv_in ONE
    ``demfi_payload_deblock`` launch per run of consecutive newly uploaded slots smooths the block edges of their payloads in place, every plane
    (interlaced input: every field of every plane) as ``deblock.plane_table`` lays them out; the phases of the grid are those of the crop
    rectangle that left the payloads of their uncropped stream (``crop_rect`` of the run's ``yuv``, taken by ``attach``).  The stage keeps
    nothing between payloads, so it needs no look-ahead and no bookkeeping; the runner counts ``deblocked``.
    ``spec.dering`` = (P, S, D) (``demfi_amd.dering``): behind the deblocker and in front of everything else that reads yuv_in.  The filter
    reads a halo of unfiltered samples and cannot work in place: per run of consecutive newly uploaded slots ONE device copy takes the run's
    payloads into ``dr_scratch`` (shaped like yuv_in) and ONE ``demfi_payload_dering`` launch writes them back into yuv_in deringed, every plane
    (every field of every plane) of ``deblock.plane_table`` on the same grid.  Nothing is kept between payloads; the runner counts ``deringed``.
    ``spec.deband`` = (T, R) (``demfi_amd.deband``): directly behind the deringing filter, in the same manner: per run of consecutive newly
    uploaded slots ONE device copy into ``bd_scratch`` and ONE ``demfi_payload_deband`` launch back into yuv_in.  With both switches
    ``bd_scratch`` IS ``dr_scratch``: the two stages run in order on the ingest stream, so one buffer serves both.  The phases of the plane
    table are carried and ignored.  Nothing is kept between payloads; the runner counts ``debanded``.
    ``spec.nlmeans`` = (S, P, R) (``demfi_amd.nlmeans``): the spatial denoiser, behind the deringing filter and IN FRONT of the debander
    (noise hides bands and denoising uncovers them), in the same manner: per run of consecutive newly uploaded slots ONE device copy into
    ``nl_scratch`` and ONE ``demfi_payload_nlmeans`` launch back into yuv_in.  ``nl_scratch`` IS ``dr_scratch`` where there is one;
    otherwise it is the buffer ``bd_scratch`` would be, and then ``bd_scratch`` IS ``nl_scratch``: one scratch buffer serves every stage
    that needs one.  The weight table and its shift are ``nlmeans.weight_table`` at the working depth, a host array the entry point reads.
    Nothing is kept between payloads; the runner counts ``nlm_filtered``."""
    denoise = clean = None                           # without --denoise: no buffer, table or launch
    nlmeans = None                                   # without --nlmeans: no buffer, table, launch, copy or counter
    deblock = None                                   # without --deblock: no table, launch or counter
    dering = None                                    # without --dering: no buffer, table, launch, copy or counter
    deband = None                                    # without --deband: no buffer, table, launch, copy or counter

    def __init__(self, runner, slots, spec, h, w, tiler=None):
        self.rn, self.slots, self.tiler, self.fh, self.fw = runner, slots, tiler, h, w
        self.fields, self.raw, self.layout, self.to_bgr = spec.fields, {}, spec.layout, None
        self.adaptive = spec.fields is not None and spec.deint_mode == 'adaptive'
        self.es, self.P = 2 if spec.hi else 1, payload_size(h, w, spec.layout)       # bytes per sample; samples of a payload
        self.Pb = self.P * self.es                                       # bytes of a payload
        dev, nsl = runner.engine.device, len(slots.frames)
        self.yuv_in = torch.empty((nsl, self.Pb), dtype=torch.uint8, device=dev)
        if self.adaptive:                            # five payload offsets per field rebuilt in a batch (at most nsl); reused in stream order
            self.dei_offs = torch.empty(5 * nsl, dtype=torch.int64, device=dev)
        if spec.denoise is not None:                 # 2 R + 1 source offsets and one destination offset per frame denoised in a batch
            a, b, self.radius = spec.denoise
            self.denoise, self.step = DN.thresholds(spec.depth, a, b), 2 if spec.fields is not None else 1
            self.clean = torch.empty((nsl, self.Pb), dtype=torch.uint8, device=dev)
            self.dn_offs = torch.empty((2 * self.radius + 2) * nsl, dtype=torch.int64, device=dev)
        if spec.deblock is not None:                 # the thresholds at the working depth; the plane table is a host array the entry point reads
            self.deblock = DB.thresholds(spec.depth, *spec.deblock)
        if spec.dering is not None:                  # the strengths at the 8-bit scale and the depth; the scratch the launch reads
            self.dering = (spec.depth,) + DR.check_params(*spec.dering)
            self.dr_scratch = torch.empty((nsl, self.Pb), dtype=torch.uint8, device=dev)
        if getattr(spec, 'nlmeans', None) is not None:       # depth, P, R; the weights and their shift; the scratch is the deringing filter's where there is one
            s, p, r = NL.check_params(*spec.nlmeans)
            self.nlmeans = (spec.depth, p, r)
            self.nl_table, self.nl_shift = NL.weight_table(spec.depth, s, p)
            self.nl_table = np.ascontiguousarray(self.nl_table, dtype=np.uint16)
            self.nl_scratch = self.dr_scratch if self.dering is not None else torch.empty((nsl, self.Pb), dtype=torch.uint8, device=dev)
        if spec.deband is not None:                  # depth, T at the 8-bit scale, R; the scratch is the deringing filter's where there is one
            self.deband = (spec.depth,) + BA.check_params(*spec.deband)
            self.bd_scratch = (self.dr_scratch if self.dering is not None else self.nl_scratch if self.nlmeans is not None
                               else torch.empty((nsl, self.Pb), dtype=torch.uint8, device=dev))
        if self.deblock is not None or self.dering is not None or self.deband is not None or self.nlmeans is not None:
            self.attach(None)
        # a working depth above the input's (``spec.depths``, ``demfi_amd.bitdepth``): payloads are copied into ``staged`` at the input's sample
        # size, so H2D carries the input's bytes, and ``promote`` writes them into yuv_in at the working depth before anything else reads them
        self.staged, self.up, self.full_range = None, self.yuv_in, False     # full_range: the stream's, set by ``Y4mEdge.attach``
        if spec.depths is not None and spec.depths[1] > spec.depths[0]:
            self.d_in, self.d_work = spec.depths[:2]
            self.es_in = 2 if self.d_in > 8 else 1
            self.staged = self.up = torch.empty((nsl, self.P * self.es_in), dtype=torch.uint8, device=dev)
            self.planes = np.ascontiguousarray(IL.plane_shapes(h, w, spec.layout), dtype=np.int32)
            self.pro_host = np.arange(nsl, dtype=np.int64) * (self.P * self.es_in)       # slot -> its byte offset in ``staged``, host and device
            self.pro_offs = torch.from_numpy(self.pro_host).to(dev)

    def upload(self, sl, idx, f):
        if tuple(f.shape) != (self.up.shape[1],) or f.dtype != torch.uint8:
            raise ValueError('frame %d: expected a uint8 [%d] %s payload, got %s %s' % (idx, self.up.shape[1], self.layout, f.dtype, tuple(f.shape)))
        self.up[sl].copy_(f, non_blocking=True)

    def attach(self, yuv):
        """A run on the stream ``yuv`` starts: its range, for the promotion, and the crop rectangle its payloads were cut out with
        (``crop_rect``; None: none), for the phases of the block grid of the deblocker and the deringing filter."""
        self.full_range = bool(getattr(yuv, 'full_range', False))
        if self.deblock is not None:
            self.db_planes = np.ascontiguousarray(DB.plane_table(self.fh, self.fw, self.layout, self.fields, getattr(yuv, 'crop_rect', None)),
                                                  dtype=np.int64)
        if self.dering is not None:
            self.dr_planes = np.ascontiguousarray(DB.plane_table(self.fh, self.fw, self.layout, self.fields, getattr(yuv, 'crop_rect', None)),
                                                  dtype=np.int64)
        if self.deband is not None:
            self.bd_planes = np.ascontiguousarray(DB.plane_table(self.fh, self.fw, self.layout, self.fields, getattr(yuv, 'crop_rect', None)),
                                                  dtype=np.int64)
        if self.nlmeans is not None:
            self.nl_planes = np.ascontiguousarray(DB.plane_table(self.fh, self.fw, self.layout, self.fields, getattr(yuv, 'crop_rect', None)),
                                                  dtype=np.int64)

    def deblocked(self, new, stream):
        """The payloads just copied (and promoted) for the (frame, slot) pairs ``new`` are deblocked in place: ONE ``demfi_payload_deblock``
        launch per run of consecutive slots, in front of everything else that reads yuv_in."""
        if self.deblock is None or not new:
            return
        for s0, cnt in consecutive([sl for _, sl in new]):
            L.check(self.rn.lib.demfi_payload_deblock(self.yuv_in[s0].data_ptr(), self.Pb, cnt, self.db_planes.ctypes.data, len(self.db_planes),
                                                      self.es, *self.deblock, stream.cuda_stream), 'payload_deblock')
        self.rn.deblocked += len(new)

    def deringed(self, new, stream):
        """The payloads just copied (promoted, deblocked) for the (frame, slot) pairs ``new`` are deringed: per run of consecutive slots ONE
        device copy into the scratch on the ingest stream, then ONE ``demfi_payload_dering`` launch from the scratch back into yuv_in."""
        if self.dering is None or not new:
            return
        for s0, cnt in consecutive([sl for _, sl in new]):
            self.dr_scratch[s0:s0 + cnt].copy_(self.yuv_in[s0:s0 + cnt], non_blocking=True)
            L.check(self.rn.lib.demfi_payload_dering(self.dr_scratch[s0].data_ptr(), self.Pb, self.yuv_in[s0].data_ptr(), self.Pb, cnt,
                                                     self.dr_planes.ctypes.data, len(self.dr_planes), self.es, *self.dering,
                                                     stream.cuda_stream), 'payload_dering')
        self.rn.deringed += len(new)

    def nlm_filtered(self, new, stream):
        """The payloads just copied (promoted, deblocked, deringed) for the (frame, slot) pairs ``new`` are denoised within the frame: per run
        of consecutive slots ONE device copy into the scratch on the ingest stream, then ONE ``demfi_payload_nlmeans`` launch from the
        scratch back into yuv_in."""
        if self.nlmeans is None or not new:
            return
        for s0, cnt in consecutive([sl for _, sl in new]):
            self.nl_scratch[s0:s0 + cnt].copy_(self.yuv_in[s0:s0 + cnt], non_blocking=True)
            L.check(self.rn.lib.demfi_payload_nlmeans(self.nl_scratch[s0].data_ptr(), self.Pb, self.yuv_in[s0].data_ptr(), self.Pb, cnt,
                                                      self.nl_planes.ctypes.data, len(self.nl_planes), self.es, *self.nlmeans,
                                                      self.nl_table.ctypes.data, self.nl_shift, stream.cuda_stream), 'payload_nlmeans')
        self.rn.nlm_filtered += len(new)

    def debanded(self, new, stream):
        """The payloads just copied (promoted, deblocked, deringed) for the (frame, slot) pairs ``new`` are debanded: per run of consecutive
        slots ONE device copy into the scratch on the ingest stream, then ONE ``demfi_payload_deband`` launch from the scratch back into
        yuv_in."""
        if self.deband is None or not new:
            return
        for s0, cnt in consecutive([sl for _, sl in new]):
            self.bd_scratch[s0:s0 + cnt].copy_(self.yuv_in[s0:s0 + cnt], non_blocking=True)
            L.check(self.rn.lib.demfi_payload_deband(self.bd_scratch[s0].data_ptr(), self.Pb, self.yuv_in[s0].data_ptr(), self.Pb, cnt,
                                                     self.bd_planes.ctypes.data, len(self.bd_planes), self.es, *self.deband,
                                                     stream.cuda_stream), 'payload_deband')
        self.rn.debanded += len(new)

    def promote(self, new, stream):
        """The payloads just copied for the (frame, slot) pairs ``new`` go from ``staged`` to yuv_in at the working depth: ONE
        ``demfi_payload_promote`` launch per run of consecutive slots, in front of everything that reads yuv_in."""
        if self.staged is None or not new:
            return
        for s0, cnt in consecutive([sl for _, sl in new]):
            L.check(self.rn.lib.demfi_payload_promote(self.staged.data_ptr(), self.pro_host[s0:].ctypes.data, self.pro_offs[s0:].data_ptr(), cnt,
                                                      self.planes.ctypes.data, len(self.planes), self.es_in, self.es, self.d_in, self.d_work,
                                                      int(self.full_range), self.yuv_in[s0].data_ptr(), self.Pb, stream.cuda_stream), 'payload_promote')
        self.rn.depth_promoted += len(new)

    def bob(self, new, stream):
        """The payloads just copied for the (field, slot) pairs ``new`` become progressive in place (at most 64 per launch)."""
        if self.fields is None or not new:
            return new
        q = {sl: I.field_parity(self.fields, idx) for idx, sl in new}
        for s0, cnt in consecutive([sl for _, sl in new]):
            for c0 in range(s0, s0 + cnt, 64):
                c = min(64, s0 + cnt - c0)
                L.check(self.rn.lib.demfi_yuv_bob(self.yuv_in[c0].data_ptr(), self.Pb, c, self.fh, self.fw, L.YUV_LAYOUT[self.layout], self.es,
                                                  sum(q[c0 + j] << j for j in range(c)), stream.cuda_stream), 'yuv_bob')
        return new

    def rebuilt(self, new, stream):
        """The payloads just copied for the (frame, slot) pairs ``new`` become progressive payloads at the working depth: promoted first of
        all, deblocked (``spec.deblock``), deringed (``spec.dering``), denoised within the frame (``spec.nlmeans``), debanded (``spec.deband``), then made progressive.  Returns the pairs that now are (adaptive: the fields just rebuilt, not those
        uploaded)."""
        self.promote(new, stream)
        self.deblocked(new, stream)
        self.deringed(new, stream)
        self.nlm_filtered(new, stream)
        self.debanded(new, stream)
        new = self._adaptive(new, stream) if self.adaptive else self.bob(new, stream)
        return self._denoise(new, stream) if self.denoise is not None else new

    payloads = property(lambda self: self.yuv_in if self.clean is None else self.clean, doc='the payloads everything behind the ingest reads')
    reach = property(lambda self: DN.reach(self.radius, self.step == 2) if self.denoise is not None else 2 if self.adaptive else 0,
                     doc='how far the frames a deferred launch reads lie from the frame it writes')

    def around(self, needed, has):
        """Adaptive, denoise: the frames f-reach .. f+reach of every frame f of ``needed`` not rebuilt / denoised yet, as far as the input has
        them (``has``)."""
        reach = self.reach
        if not reach:
            return []
        needed = set(needed)
        self._needed, self._has = sorted(needed), has
        todo = [f for f in self._needed if f in self.raw or f not in self.slots.slot_of]
        return sorted({g for f in todo for g in range(max(f - reach, 0), f + reach + 1) if g not in needed and (g < f or has(g))})

    def _denoise(self, new, stream):
        """The frames of this batch that still wait get their denoised payloads in ``clean``; returns them as (frame, slot) pairs."""
        slot_of, taps = self.slots.slot_of, 2 * self.radius + 1
        self.raw.update(new)
        self.raw = {f: sl for f, sl in self.raw.items() if slot_of.get(f) == sl}     # a slot the ring took back is forgotten
        todo = [f for f in self._needed if f in self.raw]
        done = 0
        for c0 in range(0, len(todo), 64):
            fs = todo[c0:c0 + 64]
            offs = []
            for f in fs:                             # a frame of the input that is not resident must not pass for an absent one
                nb = DN.neighbours(f, self.radius, self.step, lambda g: g < f or self._has(g))
                gone = [g for g in nb if g is not None and g not in slot_of]
                if gone:
                    raise RuntimeError('denoise: frame %d needs frame %d, which is not resident' % (f, gone[0]))
                offs += [-1 if g is None else slot_of[g] * self.Pb for g in nb] + [slot_of[f] * self.Pb]
            host = torch.tensor(offs, dtype=torch.int64).pin_memory()
            od = self.dn_offs[(taps + 1) * done:(taps + 1) * (done + len(fs))]
            od.copy_(host, non_blocking=True)
            L.check(self.rn.lib.demfi_payload_denoise(self.yuv_in.data_ptr(), self.yuv_in.numel(), host.data_ptr(), od.data_ptr(), len(fs), taps,
                                                      self.P, self.es, *self.denoise, self.clean.data_ptr(), self.clean.numel(),
                                                      stream.cuda_stream), 'payload_denoise')
            done += len(fs)
        self.rn.denoised += len(todo)
        return [(f, self.raw.pop(f)) for f in todo]

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

    def to_frames(self, new, stream):
        """The progressive payloads of the (frame, slot) pairs ``new`` -> their BGR frame slots (and tiles)."""
        sls = [sl for _, sl in new]
        for s0, cnt in consecutive(sls):
            self.to_bgr(self.payloads[s0].data_ptr(), self.slots.frames[s0].data_ptr(), cnt, stream.cuda_stream)
        if self.tiler is not None:
            self.tiler.crop(sls, stream)


class SceneScores:
    """SAD_j of every new frame j against frame j-1 over the payloads of ``ingest``, for the run's ``scene.Detector`` (``det``).
    d_sad / sad_offs / h_sad: the SADs of a batch's new frames (at most nslot), their offset pairs, the pinned copy the host reads."""

    def __init__(self, slots, ingest):
        self.slots, self.ingest, self.det, self.sad = slots, ingest, None, None
        dev, nsl = ingest.yuv_in.device, len(slots.frames)
        self.d_sad, self.sad_offs = torch.empty(nsl, dtype=torch.int64, device=dev), torch.empty(2 * nsl, dtype=torch.int64, device=dev)
        self.h_sad = torch.empty(nsl, dtype=torch.int64).pin_memory()

    def score(self, new_frames, h2d):
        """SAD_j of every frame j just uploaded against frame j-1 (``demfi_yuv420_sad``, ONE launch on the h2d stream after the
        copies), read back with one event wait and handed to the detector in frame order.  Call under the h2d stream.
        Frame j-1 is resident: it was uploaded in this batch or in the previous one (windows are consecutive), and a slot is
        reused only after all nslot >= 2 * batch + 8 slots have been (adaptive deinterlacing: nslot >= 2 * batch + 12, and batch b
        uploads up to frame k + 2 * batch + 4, its two fields of lookahead included, so it takes back the slots of frames up to
        k - 8 at most, while batch b-1 reads frames from k - 1 on and its rebuild launches, queued on h2d before, from k - 3 on;
        denoising: the same with its reach in place of 2, nslot >= 2 * batch + 8 + 2 * reach; the SADs are those of the denoised payloads).
        The wait does not wait on the compute stream: the
        ``busy`` waits queued on h2d before this batch's copies are on the compute of the batch that last read a reused
        slot, and that batch is at least two back (batch b-1 reads frames k .. k + batch + 2 of its first window k, batch b
        uploads frames up to k + 2 * batch + 2 only), so the host already waited for it when it drained that batch's D2H."""
        det, slot_of, P, yuv_in = self.det, self.slots.slot_of, self.ingest.P, self.ingest.payloads
        js = sorted(j for j in new_frames if j >= det.next)
        if not js:
            return
        if any(j - 1 not in slot_of for j in js):
            raise RuntimeError('scene cuts: the predecessor of frame %d is not resident' % min(j for j in js if j - 1 not in slot_of))
        m = len(js)
        offs = [slot_of[j - 1] * P for j in js] + [slot_of[j] * P for j in js]
        od = self.sad_offs[:2 * m]
        od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
        self.sad(yuv_in.data_ptr(), od.data_ptr(), od[m:].data_ptr(), m, self.d_sad.data_ptr(), h2d.cuda_stream)
        self.h_sad[:m].copy_(self.d_sad[:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(h2d)
        ev.synchronize()
        for j, sad in zip(js, self.h_sad[:m].tolist()):
            det.push(j, sad)


class DedupProbe:
    """Repeated frames (``cadence``): ``pipeline.KeptFrames`` stages, scores and keeps or discards input frames through this object, one
    at a time, on the upload stream ``h2d``.  cnt / cnt_offs: the block counts of one (frame, last kept frame) pair and their offsets;
    the pinned twins are reused: every probe ends with a wait for its answer.  ``thresholds``: (hi, lo) at the bit depth."""

    def __init__(self, runner, slots, ingest, spec, h2d):
        self.rn, self.slots, self.ingest, self.h2d, self.kept, self.pending = runner, slots, ingest, h2d, None, []
        self.thresholds = spec.dedup[0] << (spec.depth - 8), spec.dedup[1] << (spec.depth - 8)
        dev = ingest.yuv_in.device
        self.cnt, self.cnt_offs = torch.empty(2, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
        self.h_cnt, self.h_cnt_offs = torch.empty(2, dtype=torch.int32).pin_memory(), torch.empty(2, dtype=torch.int64).pin_memory()

    def attach(self, kept):
        """A --dedup run starts, before its first window is asked for: ``kept`` (``KeptFrames``) will stage frames here."""
        self.kept, self.pending, kept.edge = kept, [], self
        return kept

    def stage(self, key, idx, f):
        """Input frame idx, the candidate for kept index ``key``, is copied into the ring's next slot and (a field) bobbed there."""
        with torch.cuda.stream(self.h2d):
            sl, _ = self.slots.acquire(key, self.h2d)
            self.ingest.upload(sl, idx, f)
            self.ingest.rebuilt([(idx, sl)], self.h2d)
        return sl

    def block_counts(self, sl, ref):
        """(hot, warm) of the payload in slot sl against the one in slot ref: ONE ``demfi_luma_block_counts`` launch on the upload stream behind the
        copy, read back with one event wait (the next frame is compared with whichever of the two is kept, so frames are scored one by one)."""
        ing, (hi, lo) = self.ingest, self.thresholds
        with torch.cuda.stream(self.h2d):
            self.h_cnt_offs[0], self.h_cnt_offs[1] = sl * ing.Pb, ref * ing.Pb
            self.cnt_offs.copy_(self.h_cnt_offs, non_blocking=True)
            L.check(self.rn.lib.demfi_luma_block_counts(ing.yuv_in.data_ptr(), self.cnt_offs.data_ptr(), self.cnt_offs[1:].data_ptr(), 1,
                                                        ing.fh, ing.fw, ing.es, hi, lo, self.cnt.data_ptr(), self.h2d.cuda_stream),
                    'luma_block_counts')
            self.h_cnt.copy_(self.cnt, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.h2d)
        ev.synchronize()
        return tuple(self.h_cnt.tolist())

    def keep(self, key, sl):
        """The staged frame is kept: it is converted with the next batch's uploads."""
        self.pending.append((key, sl))

    def discard(self, key):
        """The staged frame repeats the last kept one: its slot is recycled at once."""
        self.slots.release(key)


def plan_batch(spec, r, wins, n, window_index, with_s1, det, kept, frames, slot_of):
    """The plan of a batch of windows n, n+1, ... of the sequence (window n + wi is window ``window_index(n + wi)``, else B-1 of its unclamped tuple)
    at the ratio r; ``frames``: the slots of their tuples, ``slot_of``: those of all resident frames.  The planner is ``retime.window_plan``, with a
    scene detector ``det`` ``scene.window_runs`` (a cut window is two runs), with the ``kept`` frames of a --dedup run ``cadence.window_runs`` over
    kept indices.  Returns (runs as (slots, instants, kinds kept), outs[w] as (run of the batch, kind, instant index) in stream order, the cut windows
    among them, the St frames planned over kept frames).  Pure."""
    return plan_fine(spec, r, wins, n, window_index, with_s1, det, kept, frames, slot_of)[:4]


def plan_fine(spec, r, wins, n, window_index, with_s1, det, kept, frames, slot_of):
    """``plan_batch`` and, behind its four values, what a shutter needs to know of the batch: fine[w] = (is window w a cut window, [(stream index i,
    does it come from the right run of the cut window)] of its outputs in stream order), and whether the batch holds the clip's last window.  With
    ``spec.shutter`` = (S, D) the ratio r is that of the fine stream and every window's plan goes through ``shutter.filter_plan``: only the outputs
    the written frames need, and the instants those name, are left.  With r < 1 (``--downconvert``) a window may own no output, or be left
    none by the filter: it gets no run and no output, and its entry of ``fine`` still says whether it is a cut window, since the scene
    changes on it.  Pure."""
    runs, outs, cut_windows, st_frames, fine, ends = [], [], 0, 0, [], False
    for wi, win in enumerate(wins):
        k = window_index(n + wi) if window_index is not None else win[2]
        last = with_s1(n + wi)
        ends, cut = ends or bool(last), False
        if kept is not None:                         # the plans of ``cadence`` over the kept frames; slots by kept index
            is_cut = det.is_cut if det is not None else None
            sr, so = K.window_runs(k, r, kept.s, kept.n, is_cut, spec.full)
            cut_windows += int(K.is_cut_window(k, is_cut))
            st_frames += sum(kind == R.ST for _, _, kind, _ in so)
        elif det is None:
            ts, o = R.window_plan(k, r, last, spec.full)
            sr, so = ([(None, ts)] if ts else []), [(i, 0, kind, j) for i, kind, j in o]
        else:
            is_cut = S.with_sentinels(det.is_cut, k + 3 if last else None) if spec.full else det.is_cut
            sr, so = S.window_runs(k, r, last, is_cut, spec.full)
            cut = k >= -1 and S.is_cut_window(k, is_cut)     # two runs; with r < 1 those of the two that have an output
            cut_windows += int(cut and bool(sr))
        right = {i for i, _, kind, _ in so if cut and kind == R.S1}      # a cut window's right run gives its frame as S1
        if spec.shutter is not None:
            sr, so = SH.filter_plan(sr, so, *spec.shutter)
        wr = [(frames[wi] if tup is None else [slot_of[x] for x in S.runner_order(tup)], ts) for tup, ts in sr]
        outs.append([(len(runs) + run, kind, j) for _, run, kind, j in so])
        fine.append((cut, [(i, i in right) for i, _, _, _ in so]))
        runs += [(fr, ts, {kind for _, run, kind, _ in so if run == ri}) for ri, (fr, ts) in enumerate(wr)]
    return runs, outs, cut_windows, st_frames, fine, ends


Buffer = namedtuple('Buffer', 'name lead rows Pb h w')


class LinearBuffer(Buffer):
    """A ``Buffer`` of LINEAR payloads (``demfi_amd.colour``): uint16 [3, h, w], ``Pb`` = 6 h w whatever the run's depth and layout.  The six
    fields and nothing else; what differs is how ``sample_format`` reads it."""
    __slots__ = ()


def linear_light(spec, h, w):
    """Does a run of ``spec`` on h x w frames work in linear light?  With a transfer (``spec.colour[0]``) and a mix or a scale stage: a
    transfer alone has nothing to do its work for, builds nothing and gives the bytes of a run without it."""
    return (spec.colour is not None and spec.colour[0] is not None
            and (spec.shutter is not None or (spec.scale is not None and tuple(spec.scale[:2]) != (w, h))))


def rgb_domain(spec, h, w):
    """Does the egress of a run of ``spec`` work on RGB payloads (``LinearBuffer``s) with an encode stage behind them?  In linear light, and
    with a LUT (``spec.lut``) whether or not the run is in linear light."""
    return linear_light(spec, h, w) or spec.lut is not None


def rgb_tables(spec, h, w):
    """(the gather's table, its inverse, the encode's table) of a run of ``spec`` in the RGB domain: the gather writes through
    ``colour.forward_table`` in linear light and ``lut3d.code_table`` otherwise; the inverse of that same table is the LUT's ``inv_in``;
    the encode reads through it too, or behind a LUT, whose output is encoded, through the inverse of ``code_table``."""
    fwd, inv = LU.tables(spec.depth, spec.colour[0] if linear_light(spec, h, w) else None)
    return fwd, inv, inv if spec.lut is None else CL.inverse_table(LU.code_table(spec.depth))


def sample_format(spec, buf):
    """(bytes per sample, [(rows, cols)] of the planes, peak) of the payloads in ``buf``: what a stage that reads it goes by."""
    if isinstance(buf, LinearBuffer):
        return 2, [(buf.h, buf.w)] * 3, CL.LIN_PEAK
    return 2 if spec.hi else 1, IL.plane_shapes(buf.h, buf.w, spec.layout), (1 << spec.depth) - 1


def egress_layout(spec, nout, batch, h, w):
    """The buffers behind the gather of ``nout`` h x w payloads a batch (of ``batch`` windows) by the module's buffer rule, for the stages
    ``spec`` asks for, in their order mix -> scale -> lut -> encode -> grain -> weave -> requant: a ``Buffer`` (name of its producer, free rows in front = the ``lead`` of
    its consumer, the most payloads its producer writes per batch, bytes of a payload, frame size) for the gather and every stage built, then
    (rows, payload bytes) of the pinned host buffers.  In linear light (``linear_light``) the gather, the mix and the scale buffers are
    ``LinearBuffer``s and an ``encode`` stage behind them writes the Y'CbCr payloads.  With a LUT (``spec.lut``) the chain runs on RGB payloads
    in the same way whether or not it is in linear light (``rgb_domain``), and a ``lut`` stage with a ``LinearBuffer`` of its own sits in
    front of the encode.  Pure: allocates nothing."""
    es, chain, lin = 2 if spec.hi else 1, [], rgb_domain(spec, h, w)

    def add(name, lead, rows, es=es, lin=False):     # lead: what the stage itself needs in front of its source's payloads
        chain.append((LinearBuffer if lin else Buffer, name, lead, rows, 6 * h * w if lin else payload_size(h, w, spec.layout) * es, h, w))
    add('gather', 0, nout, lin=lin)
    if spec.shutter is not None:
        # written frames of a batch: the multiples of D among the fine indices of its windows (each owns up to J, the last one of the full-length
        # timeline 2 J, nout in all), and the group carried into it; the open group's samples carry in front of the gather
        add('mix', spec.shutter[0] - 1, nout // spec.shutter[1] + batch + 2, lin=lin)
    if spec.scale is not None and tuple(spec.scale[:2]) != (w, h):       # the run's own size: no stage, the bytes of a run without
        w, h = spec.scale[:2]
        add('scale', 0, chain[-1][3], lin=lin)
    if spec.lut is not None:                         # stateless and pointwise: its source's rows, at the size behind the scaler
        add('lut', 0, chain[-1][3], lin=True)
    if lin:                                          # linear payloads -> the run's Y'CbCr payloads, in front of everything that reads those
        add('encode', 0, chain[-1][3])
    if spec.grain is not None:                       # every progressive payload of its source, in place of it: the same rows and size
        add('grain', 0, chain[-1][3])
    if spec.interlace is not None:                  # pairs of the carried frame and a batch's frames, the odd tail among them
        add('weave', 1, chain[-1][3] // 2 + 1)
    if spec.depths is not None and spec.depths[2] < spec.depths[1]:
        add('requant', 0, chain[-1][3], 2 if spec.depths[2] > 8 else 1)
    leads = [c[2] for c in chain[1:]] + [0]
    return [c[0](c[1], lead, *c[3:]) for c, lead in zip(chain, leads)] + [chain[-1][3:5]]


class Stage:
    """One device stage behind the gather: after a batch's payloads lie in ``src[i]`` from row ``lead`` on, ``run`` writes its own into
    ``out[i]`` from row ``front`` on (the ``lead`` of the stage behind) with ONE launch on the compute stream, and returns the payloads per
    window.  ``src`` / ``own``: the ``Buffer`` it reads and the one it writes (``egress_layout``); ``rows``, ``Pb``, ``h``, ``w``: of ``own``.
    ``begin(yuv)`` resets what a stage keeps within a run, ``carry(i, src)`` runs before the batch's gather, ``flush(i, src, stream)`` after
    the last batch and returns the payloads it still wrote (0 or 1).  ``regroups``: a window may complete no payload of the stage.
    ``offs`` / ``h_offs``: the offset tables of the launch, ``width`` offsets a payload written (0: the stage has a table of its own), on the
    device and pinned, one per buffer set; table i is written again two batches later, when the host has drained the batch that last copied
    from it (``ClipPipeline._drain`` waits for that batch's D2H, which waited for its compute, where the copy of the table ran)."""
    regroups, width = False, 1

    def __init__(self, runner, spec, src, own, dev):
        self.rn, self.lib, self.spec, self.es = runner, runner.lib, spec, sample_format(spec, src)[0]    # es: bytes of a sample it reads
        self.lead, self.front, self.rows, self.Pb, self.h, self.w = src.lead, own.lead, own.rows, own.Pb, own.h, own.w
        self.out = [torch.empty((own.lead + own.rows, own.Pb), dtype=torch.uint8, device=dev) for _ in range(2)]
        if self.width:
            self.offs = [torch.empty(self.rows * self.width, dtype=torch.int64, device=dev) for _ in range(2)]
            self.h_offs = [torch.empty((self.rows, self.width), dtype=torch.int64).pin_memory() for _ in range(2)]

    def begin(self, yuv):
        pass

    def carry(self, i, src):
        pass

    def flush(self, i, src, stream):
        return 0

    def _table(self, i, offsets):
        host = self.h_offs[i][:len(offsets)]
        host.numpy()[:] = offsets
        od = self.offs[i][:host.numel()]
        od.copy_(host.view(-1), non_blocking=True)
        return host.data_ptr(), od.data_ptr()

    def _launch(self, i, offsets, src, stream, counted=None):
        """The payloads of the byte offsets ``offsets`` [n, width] into src[i] are written into out[i]; the runner's ``counter`` goes up by
        ``counted`` (None: n)."""
        n = len(offsets)
        if n > self.rows:
            raise RuntimeError(self.too_many % (n, self.rows))
        setattr(self.rn, self.counter, getattr(self.rn, self.counter) + (n if counted is None else counted))
        if n:
            self._call(src[i].data_ptr(), *self._table(i, offsets), n, self.out[i][self.front:].data_ptr(), stream.cuda_stream)


class Shutter(Stage):
    """Fine payloads gathered -> written payloads mixed (``demfi_amd.shutter``, ``spec.shutter`` = (S, D)).  Written frame c averages the
    fine frames c D .. c D + S - 1 of its scene that exist.  After a batch's gather ``run`` closes every group whose last sample has arrived
    (all open groups when the batch holds the clip's last window) and ``demfi_payload_mix`` writes them (``spec.shutter_window`` 'triangle':
    ``demfi_payload_mix_w`` with the weights of ``shutter.window_weights``); a written frame counts to the window
    that completed it.  The samples of the one group still open (at most ``lead`` = S - 1 of them, consecutive rows at the end of the gather)
    carry over on the device: ``carry`` copies them into the ``lead`` rows in front of the next batch's gather, so which batch a sample came
    with never shows.  The runner counts for it, as it counts cut windows: ``shutter_mixed`` the fine frames that went into the mixes,
    ``shutter_carried`` the samples carried from one batch to the next."""
    regroups, counter, too_many = True, 'shutter_mixed', 'shutter: %d written frames for %d payload rows'

    def __init__(self, runner, spec, src, own, dev):
        self.S, self.D = spec.shutter
        self.width = self.S
        super().__init__(runner, spec, src, own, dev)
        w = SH.window_weights(spec.shutter_window, self.S)               # a weighted window: the kept samples are a prefix, one vector serves
        self.weights = None if set(w) == {1} else np.ascontiguousarray(w, dtype=np.int32)
        self.begin(None)

    def begin(self, yuv):
        self.open, self.scene = [], 0                # open: (fine index, scene, row) of the samples of the open group

    def carry(self, i, yuv_out):
        """Before batch i's gather (compute stream): the open group's samples move from the end of the other buffer's gather in front of this one's."""
        m = len(self.open)
        if not m:
            return
        a = self.open[0][2]
        if m > self.lead or [row for _, _, row in self.open] != list(range(a, a + m)):
            raise RuntimeError('shutter: %d open samples at rows %s for %d carry rows' % (m, [row for _, _, row in self.open], self.lead))
        yuv_out[i][self.lead - m:self.lead].copy_(yuv_out[1 - i][a:a + m])
        self.rn.shutter_carried += m
        self.open = [(g, sc, self.lead - m + j) for j, (g, sc, _) in enumerate(self.open)]

    def run(self, i, counts, batch, yuv_out, stream):
        """batch = (fine, ends) of ``plan_fine``: fine[w] for window w, gathered into yuv_out[i] from row ``lead`` on."""
        fine, ends = batch
        table, counts, self.open, self.scene = SH.close_groups(self.open, fine, self.scene, ends, self.S, self.D, self.lead)
        self._launch(i, [[rw * self.Pb for rw in t] + [-1] * (self.S - len(t)) for t in table], yuv_out, stream, sum(len(t) for t in table))
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        if self.weights is None:                     # the box, and a triangle of up to two samples, which is one
            L.check(self.lib.demfi_payload_mix(src, host, offs, n, self.S, self.Pb // self.es, self.es, dst, self.Pb, stream), 'payload_mix')
        else:
            L.check(self.lib.demfi_payload_mix_w(src, host, offs, n, self.S, self.Pb // self.es, self.es, dst, self.Pb, self.weights.ctypes.data,
                                                 stream), 'payload_mix_w')


class Scaler(Stage):
    """Progressive payloads -> resized ones (``demfi_amd.scale``, ``spec.scale`` = (w, h, filter)): behind the gather or the mix and in front
    of the weave, so the scaler never sees woven fields.  ``demfi_payload_scale`` resamples all of a batch's payloads.  Stateless per payload:
    no sample carries over from one batch to the next, so which batch a frame came with never shows, and the stage works on every rank.  The
    tables of ``scale.table_blob`` are the only source of the weights; they are uploaded once, here.  The runner counts ``scale_payloads``."""
    counter, too_many = 'scale_payloads', 'scale: %d payloads for %d payload rows'

    def __init__(self, runner, spec, src, own, dev):
        super().__init__(runner, spec, src, own, dev)
        self.filter, self.Pb_in = spec.scale[2], src.Pb
        (_, shapes_in, self.peak), shapes_out = sample_format(spec, src), sample_format(spec, own)[1]
        self.planes_in, self.planes_out = (np.ascontiguousarray(a, dtype=np.int32) for a in (shapes_in, shapes_out))
        blob, self.desc = SC.table_blob(shapes_in, shapes_out, self.filter)
        self.tables = torch.from_numpy(blob).to(dev)

    def run(self, i, counts, batch, src, stream):
        self._launch(i, np.arange(sum(counts), dtype=np.int64)[:, None] * self.Pb_in, src, stream)
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_payload_scale(src, host, offs, n, self.planes_in.ctypes.data, self.planes_out.ctypes.data, len(self.planes_in),
                                             self.es, self.peak, self.tables.data_ptr(), self.desc.ctypes.data, dst, self.Pb, stream),
                'payload_scale')


class Interlacer(Stage):
    """Progressive payloads -> woven ones (``demfi_amd.interlace``, ``spec.interlace`` = (field order, low-pass mode)).  Written payload q
    weaves frames 2q (the first field in time) and 2q + 1 of the progressive stream.  After a batch's frames are written into ``src[i]``
    ``run`` closes every pair whose second frame has arrived (``interlace.close_pairs``; the odd tail too when the batch holds the clip's last
    window) and ``demfi_payload_weave`` writes them; a woven payload counts to the window that completed it.  The one frame still open
    carries over on the device: ``carry`` copies it into row 0 of the next batch's source buffer (``lead`` = 1 row in front of its frames),
    so which batch a frame came with never shows.  A run whose edge never learns which window is the last (``--dedup``) ends with ``flush``,
    which weaves the open frame with itself.  The runner counts: ``interlace_woven`` the payloads woven, ``interlace_carried`` the frames
    carried from one batch to the next."""
    regroups, width, counter, too_many = True, 2, 'interlace_woven', 'interlace: %d woven payloads for %d payload rows'

    def __init__(self, runner, spec, src, own, dev):
        super().__init__(runner, spec, src, own, dev)
        self.order, self.lowpass = spec.interlace
        self.q0, self.mode, self.peak = I.field_parity(self.order, 0), IL.LOWPASS.index(self.lowpass), (1 << spec.depth) - 1
        self.planes = np.ascontiguousarray(IL.plane_shapes(self.h, self.w, spec.layout), dtype=np.int32)
        self.begin(None)

    def begin(self, yuv):
        self.open = None                             # (buffer set, row) of the one open frame

    def carry(self, i, src):
        """Before batch i's frames are written (compute stream): the open frame moves from the other buffer set in front of this one's."""
        if self.open is None:
            return
        j, row = self.open
        if j != i:
            src[i][0].copy_(src[j][row])
            self.rn.interlace_carried += 1
        elif row != 0:
            raise RuntimeError('interlace: the open frame lies at row %d of the buffer set about to be written' % row)
        self.open = (i, 0)

    def run(self, i, counts, batch, src, stream):
        """counts[w]: the progressive frames of window w, written into src[i] from row ``lead`` on; batch[1]: it holds the clip's last window."""
        pairs, woven, left = IL.close_pairs(0 if self.open is not None else None, counts, batch[1], self.lead)
        self.open = (i, left) if left is not None else None
        self._launch(i, [[a * self.Pb, b * self.Pb] for a, b in pairs], src, stream)
        return woven

    def flush(self, i, src, stream):
        if self.open is None:
            return 0
        self.carry(i, src)
        self.open = None
        self._launch(i, [[0, 0]], src, stream)
        return 1

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_payload_weave(src, host, offs, n, self.planes.ctypes.data, len(self.planes), self.es, self.peak, self.q0,
                                             self.mode, dst, self.Pb, stream), 'payload_weave')


class Requantizer(Stage):
    """Written payloads at the working depth -> the output's (``demfi_amd.bitdepth``, ``spec.depths`` = (input, working, output depth, dither
    mode) with output < working).  The last device stage: ``demfi_payload_requant`` takes all of a batch's payloads down into buffers of the
    output's payload size, which are what crosses D2H: 16 -> 8 sends half the bytes.  ``field_rows``: the payloads hold two fields
    (``spec.interlace``), so the dither's row is the row within its field.  Stateless per payload: which batch a payload came with never
    shows, and the stage works on every rank.  The runner counts ``depth_requantised``.  The offsets are those of consecutive rows, the same
    in every batch: one table, uploaded once, that no batch rewrites."""
    width, counter, too_many = 0, 'depth_requantised', 'requant: %d payloads for %d payload rows'

    def __init__(self, runner, spec, src, own, dev):
        super().__init__(runner, spec, src, own, dev)
        _, self.d_work, self.d_out, dither = spec.depths
        self.es_in, self.es = 2 if self.d_work > 8 else 1, 2 if self.d_out > 8 else 1
        self.dither, self.field_rows = int(dither == 'bayer'), int(spec.interlace is not None)
        self.planes = np.ascontiguousarray(IL.plane_shapes(self.h, self.w, spec.layout), dtype=np.int32)
        self.h_offs = np.arange(self.rows, dtype=np.int64) * src.Pb
        self.offs = torch.from_numpy(self.h_offs).to(dev)

    def begin(self, yuv):
        self.full_range = egress_colour(self.spec, yuv)[1]

    def _table(self, i, offsets):
        return self.h_offs.ctypes.data, self.offs.data_ptr()

    def run(self, i, counts, batch, src, stream):
        self._launch(i, range(sum(counts)), src, stream)
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_payload_requant(src, host, offs, n, self.planes.ctypes.data, len(self.planes), self.es_in, self.es, self.d_work,
                                               self.d_out, self.full_range, self.dither, self.field_rows, dst, self.Pb, stream), 'payload_requant')


class Encoder(Stage):
    """Linear payloads -> the run's Y'CbCr payloads (``demfi_amd.colour``, ``spec.colour`` = (transfer, out matrix, out full range)): behind
    the mix and the scaler, which worked in light, and in front of the weave and the requantisation, which see the payloads they always
    saw.  ``demfi_linear_to_yuv`` takes all of a batch's payloads through the inverse table of ``colour.inverse_table``, uploaded once,
    here, and then through the gather's own arithmetic with the egress matrix and range.  Stateless per payload, like the scaler: the stage
    works on every rank.  The runner counts ``colour_encoded``."""
    counter, too_many = 'colour_encoded', 'encode: %d payloads for %d payload rows'

    def __init__(self, runner, spec, src, own, dev, tables=None):
        super().__init__(runner, spec, src, own, dev)
        self.Pb_in, self.depth, self.layout = src.Pb, spec.depth, L.YUV_LAYOUT[spec.layout]
        inv = CL.tables(spec.colour[0], spec.depth)[1] if tables is None else tables[2]      # tables: ``rgb_tables`` at the gather's size
        self.inv = torch.from_numpy(inv.view(np.int16)).to(dev)

    def begin(self, yuv):
        self.matrix, self.full_range = egress_colour(self.spec, yuv)

    def run(self, i, counts, batch, src, stream):
        self._launch(i, np.arange(sum(counts), dtype=np.int64)[:, None] * self.Pb_in, src, stream)
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_linear_to_yuv(src, host, offs, n, self.h, self.w, self.depth, self.layout, self.matrix, self.full_range,
                                             self.inv.data_ptr(), dst, self.Pb, stream), 'linear_to_yuv')


class Lut(Stage):
    """RGB payloads -> RGB payloads through a user's 3D colour LUT (``demfi_amd.lut3d``, ``spec.lut`` = a ``lut3d.Cube``): behind the mix and
    the scaler, at full chroma resolution and the working depth, and in front of the encode, which reads its 16-bit encoded output through
    ``colour.inverse_table(lut3d.code_table)``.  ``demfi_rgb_lut3d`` takes all of a batch's payloads through the cube with ONE launch.  The
    three tables are the only source of the numbers and are uploaded once, here: ``inv_in``, the inverse of the table the gather wrote
    with (``rgb_tables``), ``lut3d.axis_table`` and ``lut3d.cube_words``.  Stateless per payload, like the scaler: the stage works on every
    rank.  A cube of up to ``LDS_N`` = 17 lattice points is kept in LDS (``cube_in_lds``: 9 to 35 % faster than reading it through L2,
    profiles/lut3d.md), a larger one is read through L2.  The runner counts ``lut_payloads``."""
    counter, too_many, LDS_N = 'lut_payloads', 'lut: %d payloads for %d payload rows', 17

    def __init__(self, runner, spec, src, own, dev, tables=None):
        super().__init__(runner, spec, src, own, dev)
        cube = spec.lut
        self.Pb_in, self.depth, self.n, self.in_lds = src.Pb, spec.depth, cube.n, int(cube.n <= self.LDS_N)
        inv_in = LU.tables(spec.depth)[1] if tables is None else tables[1]                   # tables: ``rgb_tables`` at the gather's size
        self.inv_in = torch.from_numpy(inv_in.view(np.int16)).to(dev)
        self.axt = torch.from_numpy(LU.axis_table(spec.depth, cube.n).view(np.int32)).to(dev)
        self.cube = torch.from_numpy(LU.cube_words(cube).view(np.int64).reshape(-1)).to(dev)

    def run(self, i, counts, batch, src, stream):
        self._launch(i, np.arange(sum(counts), dtype=np.int64)[:, None] * self.Pb_in, src, stream)
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_rgb_lut3d(src, host, offs, n, self.h, self.w, self.depth, self.inv_in.data_ptr(), self.n, self.cube.data_ptr(),
                                         self.axt.data_ptr(), self.in_lds, dst, self.Pb, stream), 'rgb_lut3d')


class Grain(Stage):
    """Progressive payloads -> the same payloads with film grain (``demfi_amd.grain``, ``spec.grain`` = (S16, r, C16, curve, seed)): behind
    the mix, the scaler and the encode, which would average grain away, and in front of the weave and the requantisation, so both fields
    of a woven payload get independent grain and the dither sees it.  ``demfi_payload_grain`` grains all of a batch's payloads.  Stateless
    per payload except for ``n``, the running count of the progressive frames the stage has seen in this run: payload j of a batch is
    frame n + j, whose three keys (``grain.plane_key``) go up beside its offset, so which batch a frame came with never shows.  ``begin``
    resets n and takes the range written from ``egress_colour``; the two gain tables of ``grain.gain_tables`` are the only source of the
    strength and the curve and are uploaded once per range, there.  The count restarts on every rank, so the stage runs on one
    (``video.ONE_RANK_EGRESS``); the field is a pure function of n, so handing each rank its first n is all several would take.  The
    runner counts ``grain_payloads``."""
    counter, too_many = 'grain_payloads', 'grain: %d payloads for %d payload rows'

    def __init__(self, runner, spec, src, own, dev):
        super().__init__(runner, spec, src, own, dev)
        self.params, self.depth, self.dev = GR.check_params(spec.grain), spec.depth, dev
        self.planes = np.ascontiguousarray(IL.plane_shapes(self.h, self.w, spec.layout), dtype=np.int32)
        self.keys = [torch.empty(self.rows * 3, dtype=torch.int32, device=dev) for _ in range(2)]
        self.h_keys = [torch.empty((self.rows, 3), dtype=torch.int32).pin_memory() for _ in range(2)]
        self.n, self.full_range, self.h_gains, self.gains = 0, None, None, None

    def begin(self, yuv):
        full = egress_colour(self.spec, yuv)[1]
        if full != self.full_range:                  # the curve's t goes by the range written
            self.full_range = full
            self.h_gains = np.ascontiguousarray(GR.gain_tables(self.depth, self.params, full), dtype=np.int32)
            self.gains = torch.from_numpy(self.h_gains).to(self.dev)
        self.n = 0

    def run(self, i, counts, batch, src, stream):
        m, seed = sum(counts), self.params[4]
        if m > self.rows:
            raise RuntimeError(self.too_many % (m, self.rows))
        if m:
            self.h_keys[i].numpy().view(np.uint32)[:m] = [[GR.plane_key(seed, self.n + j, p) for p in range(3)] for j in range(m)]
            self.keys[i][:3 * m].copy_(self.h_keys[i][:m].view(-1), non_blocking=True)
        self._i = i
        self._launch(i, np.arange(m, dtype=np.int64)[:, None] * self.Pb, src, stream)
        self.n += m
        return counts

    def _call(self, src, host, offs, n, dst, stream):
        L.check(self.lib.demfi_payload_grain(src, host, offs, self.h_keys[self._i].data_ptr(), self.keys[self._i].data_ptr(), n,
                                             self.planes.ctypes.data, len(self.planes), self.es, self.depth, self.full_range, self.params[1],
                                             self.h_gains.ctypes.data, self.gains.data_ptr(), dst, self.Pb, stream), 'payload_grain')


STAGES = {'mix': Shutter, 'scale': Scaler, 'lut': Lut, 'encode': Encoder, 'grain': Grain, 'weave': Interlacer, 'requant': Requantizer}


class TileGrid:
    """A multi-tile plan for the 16-bit frames of the Y4M edge: the sizes ``pipeline.Tiler`` gives, and no device side.  The ingest of
    a (run, tile) pair reads its source rectangle out of the full frame slots and its egress writes its kept rectangle into the full
    output frames (``WindowRunner._u16_tile_io``), so there is nothing to crop into and nothing to stitch from."""

    def __init__(self, plan):
        self.plan, self.nt = plan, plan.n_tiles
        (self.h, self.w), (self.th, self.tw) = (plan.h, plan.w), plan.tile


class FrameIO:
    """How the runs of a batch read and write frames, chosen once from (16-bit frames, tiled): each planned run is ``nt`` runner runs, ``reads(fr)``
    gives the four tensors each reads, ``dst[i]`` the buffer they write, ``window(w, frames, buf, rows)`` the (load, emit, pre) of runner run w, and
    ``after(i, runs, cur)`` follows the windows.  comb[i][w] = [S0, St x J, S1] of planned run w; 16-bit frames are int16 storage and leave through the
    emit path (``sinks`` False: the fused sink writes uint8 only).  8-bit tiles (``crops``: the ``pipeline.Tiler`` that cropped the slots at upload)
    run into ``tcomb`` and ONE stitch launch per batch pastes them into comb[i]; one tcomb serves both buffer sets: the stitch has read it before the
    next batch's runs start.  16-bit tiles are ``in_place``: their kept rectangles of comb[i][w] are disjoint, so the runs need no order among
    themselves."""

    def __init__(self, runner, slots, tiler, runs_max, J, h, w, depth):
        hi, tiled, dev, frames = depth > 8, tiler is not None, runner.engine.device, slots.frames
        if tiled and hi != isinstance(tiler, TileGrid):
            raise ValueError('Y4mEdge: %d-bit frames with a %s' % (depth, type(tiler).__name__))
        nt = self.nt = tiler.nt if tiled else 1
        self.J, self.tiler, self.sinks, self.in_place, self.crops = J, tiler, not hi, hi and tiled, None
        self.comb = self.dst = [torch.empty((runs_max, J + 2, h, w, 3), dtype=torch.int16 if hi else torch.uint8, device=dev) for _ in range(2)]
        self.reads, self.after = lambda fr: [[frames[sl] for sl in fr]] * nt, lambda i, runs, cur: None
        out = lambda buf, w: (buf[w, 1:J + 1], buf[w, 0::J + 1])          # noqa: E731  (St x J, [S0, S1]) of run w
        self.window = ((lambda w, fr, buf, rows: runner._u16_tile_io(fr, tiler.plan.tiles[w % nt], *out(buf, w // nt), depth)) if self.in_place
                       else (lambda w, fr, buf, rows: runner._u16_io(fr, *out(buf, w), depth)) if hi
                       else (lambda w, fr, buf, rows: runner._u8_io(fr, *out(buf, w), None if rows is None else rows[w])))
        if tiled and not hi:
            self.crops, self.after, self.reads = tiler, self._stitch, lambda fr: [[tiler.tin[sl, j] for sl in fr] for j in range(nt)]
            self.tcomb = torch.empty((runs_max * nt, J + 2, tiler.th, tiler.tw, 3), dtype=torch.uint8, device=dev)
            self.dst = [self.tcomb, self.tcomb]

    def _stitch(self, i, runs, cur):
        J, nt, comb, tcomb = self.J, self.nt, self.comb[i], self.tcomb
        (c0, c1), (t0, t1), j = comb.stride()[:2], tcomb.stride()[:2], np.arange(nt, dtype=np.int64)
        pos = [(w, p) for w, (_, ts, kinds) in enumerate(runs)
               for p in ([0] if R.S0 in kinds else []) + list(range(1, len(ts) + 1)) + ([J + 1] if R.S1 in kinds else [])]
        self.tiler.stitch(tcomb, [(w * nt + j) * t0 + p * t1 for w, p in pos], comb, [w * c0 + p * c1 for w, p in pos], cur)


class Y4mEdge:
    """Y4M payloads in; sink(k, payloads [c, P]) out, the c output frames window k owns in stream order.  ``spec``: the run's
    ``pipeline.EdgeSpec``; ``tiler``: None, a ``pipeline.Tiler`` (8-bit frames) or a ``TileGrid`` (16-bit).  ONE gather launch per batch
    converts the outputs in comb[i] into yuv_out[i] in stream order; the payload buffers are uint8 tensors sized in bytes.  ``stages``: the
    ``Stage`` objects behind the gather in their order, sized by ``egress_layout`` and run one after the other on the compute stream, each on the
    buffers of the one before it (``sources``); ``written``: the buffers of the last of them, or yuv_out, which ``d2h`` copies into the pinned
    ``h_yuv``.  Without a stage no buffer, table or launch is added."""

    def __init__(self, runner, batch, slots, spec, tiler, h2d):
        self.rn, self.slots, self.spec = runner, slots, spec
        r = self.r = runner.ratio
        h, w = (tiler.h, tiler.w) if tiler else (runner.h, runner.w)
        dev, J = runner.engine.device, R.max_instants(r)
        nJ = -(-J // runner.n_ctx) * runner.n_ctx if runner.tb else J    # instants incl. the padding of a short chunk
        runs_max = batch * max_runs(r, spec.cuts, spec.dedup)            # a cut window is two runs
        # payloads of a batch: at most J per window, plus the last window's S1 (full-length: its [n-2, n) span, 2 J)
        nout = (batch + 1) * J if spec.full else batch * J + 1
        if spec.dedup is not None:                   # a window spans up to max_hold + 1 input frames, and so does the last one's hold
            nout = (batch + 1) * K.max_window_instants(r, spec.dedup[3]) + 1
        io = self.io = FrameIO(runner, slots, tiler, runs_max, J, h, w, spec.depth)
        ing = self.ingest = Ingest(runner, slots, spec, h, w, io.crops)
        self.around = ing.around                     # the frames a batch must find uploaded besides those it names
        self.scores = SceneScores(slots, ing) if spec.cuts else None
        self.probe = DedupProbe(runner, slots, ing, spec, h2d) if spec.dedup is not None else None
        self.t = [torch.empty((runs_max * io.nt, nJ), dtype=torch.float32, device=dev) for _ in range(2)]
        self.sinks = [torch.empty((runs_max * io.nt, nJ, 32), dtype=torch.int64, device=dev) for _ in range(2)]
        self.offs = [torch.empty(nout, dtype=torch.int64, device=dev) for _ in range(2)]
        # the last buffer of the chain is what crosses D2H: only mixed, resized, woven payloads of the output's sample size leave the device
        *bufs, host = egress_layout(spec, nout, batch, h, w)
        self.lead = bufs[0].lead                     # the free rows in front of the gather
        self.yuv_out = [torch.empty((self.lead + nout, bufs[0].Pb), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.fwd, tables = None, None                # linear light, a LUT: the gather writes RGB payloads through this table, uploaded once
        if isinstance(bufs[0], LinearBuffer):        # the gather's frame size decides whether the run is in linear light
            tables = rgb_tables(spec, h, w)
            self.fwd = torch.from_numpy(tables[0].view(np.int16)).to(dev)
        self.stages, self.sources, self.written = [], [], self.yuv_out       # sources[j]: the buffers stages[j] reads
        for src, own in zip(bufs, bufs[1:]):
            st = STAGES[own.name](runner, spec, src, own, dev, **({'tables': tables} if own.name in ('lut', 'encode') else {}))
            self.stages.append(st)
            self.sources.append(self.written)
            self.written = st.out
        self.h_yuv = [torch.empty(host, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.yuv = self.window_index = self.det = self.kept = self.gather = None

    def __getattr__(self, name):                     # J, tiler, in_place and, on a crop-run-stitch edge only, tcomb: the frame IO's
        return getattr(self.__dict__['io'], name)

    def attach(self, host_frames, yuv=None):
        """Before a run's first window is asked for.  --dedup: ``host_frames`` is the ``KeptFrames`` that stages frames through ``probe``, and
        a frame staged is promoted there (``spec.depths``), which needs the range of the stream ``yuv``."""
        self.ingest.attach(yuv)
        if self.probe is not None:
            self.kept = self.probe.attach(host_frames)

    def begin(self, yuv, window_index, first_win):
        """A run starts; returns the frames to make resident first: with scene cuts, frame k0 - 1 of a first window k0 >= 1."""
        ing, sc = self.ingest, self.scores
        self.yuv, self.window_index, self.det, ing.raw = yuv, window_index, None, {}
        for st in self.stages:
            st.begin(yuv)
        ing.to_bgr, self.gather, sad = yuv_calls(self.rn.lib, self.spec, ing.fh, ing.fw, yuv)
        if self.fwd is not None:
            self.gather = self._linear_gather
        if sc is None:
            return ()
        sc.sad, det = sad, S.Detector(ing.P, yuv.scene_cut, first=S.first_frame(window_index(0) if window_index is not None else first_win[2]),
                                      peak=(1 << self.spec.depth) - 1)
        sc.det = self.det = det
        self.rn.last_cuts = det.cuts
        return (det.next - 1,) if det.next - 1 < first_win[2] else ()

    def _linear_gather(self, base, offs, dst, n, stream):
        """The gather of a linear-light run: the same frames of ``comb`` at the same offsets (in samples), written as linear payloads."""
        ing = self.ingest
        L.check(self.rn.lib.demfi_bgr_to_linear_gather(base, offs, dst, 3 * ing.fh * ing.fw, n, ing.fh, ing.fw, ing.es, self.spec.depth,
                                                       self.fwd.data_ptr(), stream), 'bgr_to_linear_gather')

    def upload(self, sl, idx, f):
        self.ingest.upload(sl, idx, f)

    def uploaded(self, new, h2d):
        """After a batch's copies (h2d stream): its (frame, slot) pairs and the kept frames staged since become frame slots; then the SADs."""
        ing, probe = self.ingest, self.probe
        new = ing.rebuilt(new, h2d)
        if probe is not None:                        # the frames kept since the last batch were bobbed when they were staged
            new, probe.pending = probe.pending + list(new), []
        ing.to_frames(new, h2d)
        if self.det is not None:
            self.scores.score([idx for idx, _ in new], h2d)

    def run(self, i, n, wins, frames, cur):
        """Plans the batch's windows, runs them and gathers their outputs into yuv_out[i].  Returns (payloads per window, slots read)."""
        runs, outs, cut_windows, st_frames, fine, ends = plan_fine(self.spec, self.r, wins, n, self.window_index, self.yuv.with_s1, self.det,
                                                                   self.kept, frames, self.slots.slot_of)
        self.rn.cut_windows += cut_windows
        if self.kept is not None:
            self.kept.st_frames += st_frames
        self.rn.windows_skipped += sum(not o for o in outs)               # r < 1: windows that own no output (or none a shutter needs)
        if runs:
            self._run_windows(i, runs)
        for st, src in zip(reversed(self.stages), reversed(self.sources)):   # the carries are independent copies: the last stage's goes first
            st.carry(i, src)
        counts = self._gather(i, outs, cur, self.lead)
        for st, src in zip(self.stages, self.sources):
            counts = st.run(i, counts, (fine, ends), src, cur)
        return counts, [fr for fr, _, _ in runs]

    def flush(self, i, cur):
        """After the last batch's ``run``: what is still to be written into buffer set i (None: nothing), for ``d2h`` and ``drain``.  Once a
        stage has flushed a payload, the stages behind it run on it (no plan goes with it: no stage that regroups may follow one that flushes)."""
        counts = None
        for st, src in zip(self.stages, self.sources):
            if counts is not None:
                counts = st.run(i, counts, None, src, cur)
            elif st.flush(i, src, cur):
                counts = [1]
        return counts

    def _run_windows(self, i, runs):
        """Planned run w = (4 slots, instants, kinds) becomes the ``io.nt`` runner runs w * nt + j, which run its instants into ``io.dst[i]``;
        ``io.after`` follows them.  The t values (padded slots repeat the last t) are uploaded on the current stream, and so are the uint8 sink records
        of a frame IO of ``sinks``, the one mode switch left here: one per (run, instant), S0 / S1 only in the row of the run's first instant and only
        when ``kinds`` holds that frame, rows past a run's instants disabled."""
        rn, J, io, buf = self.rn, self.J, self.io, self.io.dst[i]
        subs = [(frames, ts, kinds) for fr, ts, kinds in runs for frames in io.reads(fr)]
        nw, nJ = len(subs), self.t[i].shape[1]
        tt = np.empty((nw, nJ), np.float32)
        for w, (_, ts, _) in enumerate(subs):
            tt[w, :len(ts)] = ts
            tt[w, len(ts):] = ts[-1]
        t_dev = self.t[i][:nw]
        t_dev.copy_(torch.from_numpy(tt).pin_memory(), non_blocking=True)
        rows = None
        if io.sinks and rn.engine.supports_u8_sink:
            st = np.zeros((nw, nJ), np.int64)
            s01 = np.zeros((2, nw, nJ), np.int64)
            base, (c0, c1) = buf.data_ptr(), buf.stride()[:2]            # uint8: element strides are bytes
            for w, (_, ts, kinds) in enumerate(subs):
                st[w, :len(ts)] = base + w * c0 + c1 * np.arange(1, len(ts) + 1)
                s01[0, w, 0] = base + w * c0 if R.S0 in kinds else 0
                s01[1, w, 0] = base + w * c0 + (J + 1) * c1 if R.S1 in kinds else 0
            a = fill_sink_records(np.empty((nw, nJ, 32), np.int64), st, s01[0], s01[1], rn.h, rn.w, rn.n_tst)
            rows = self.sinks[i][:nw]
            rows.copy_(torch.from_numpy(a).pin_memory(), non_blocking=True)
        wio = [io.window(w, frames, buf, rows) for w, (frames, _, _) in enumerate(subs)]
        cur = rn._begin()
        for w, (load, emit, pre) in enumerate(wio):
            rn._window(load, emit, body_only=True, pre=pre, t_dev=t_dev[w], nt=len(subs[w][1]))
        rn._end(cur)
        io.after(i, runs, cur)

    def _gather(self, i, outs, cur, lead=0):
        """outs[w] = window w's outputs as (run, kind, instant index), from comb[i] -> yuv_out[i] from row ``lead`` on; returns the payloads per
        window."""
        comb, dst, J = self.io.comb[i], self.yuv_out[i][lead:], self.J
        c0, c1 = comb.stride()[:2]
        offs = [run * c0 + (0 if kind == R.S0 else J + 1 if kind == R.S1 else 1 + j) * c1 for o in outs for run, kind, j in o]
        nf = len(offs)
        if nf > dst.shape[0]:
            raise RuntimeError('retime: %d outputs for %d payload slots' % (nf, dst.shape[0]))
        if nf:                                       # r < 1: a batch may own no output
            od = self.offs[i][:nf]
            od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
            self.gather(comb.data_ptr(), od.data_ptr(), dst.data_ptr(), nf, cur.cuda_stream)
        return [len(o) for o in outs]

    def d2h(self, i, counts):
        self.h_yuv[i][:sum(counts)].copy_(self.written[i][:sum(counts)], non_blocking=True)

    def drain(self, i, k0, counts, sink):
        pos = 0
        for j, c in enumerate(counts):
            if c or not any(st.regroups for st in self.stages):          # a window that completed no written payload has nothing to hand out
                sink(k0 + j, self.h_yuv[i][pos:pos + c])
            pos += c


class IvtcScorer:
    """The scorer of ``telecine.FilmFrames`` on the GPU (``--ivtc``): the two launches of csrc/ivtc.hip over a device ring of luma
    planes of its own, on a stream of its own.  ``put`` copies the luma of a new payload (its first h*w samples) into the ring
    slot i mod RING through a pinned twin; ``comb`` and ``sad`` are ONE launch each, read back with one event wait; neither waits
    on the compute stream.  RING = 8: cycle c reads payloads 5c-2 .. 5c+5 (``FilmFrames``), and a slot is taken back 8 payloads
    later, after the waits of the cycle that read it.  MAX = the entries of one call: a cycle has five."""
    RING, MAX = 8, 8

    def __init__(self, lib, h, w, depth, cthresh, device):
        self.lib, self.h, self.w, self.es = lib, h, w, 2 if depth > 8 else 1
        self.thresh = cthresh << (depth - 8)
        self.Lb = h * w * self.es                            # bytes of a luma plane
        self.stream = torch.cuda.Stream(device)
        with torch.cuda.stream(self.stream):                 # the device buffers belong to the stream that alone touches them
            self.ring = torch.empty((self.RING, self.Lb), dtype=torch.uint8, device=device)
            self.offs = torch.empty(4 * self.MAX, dtype=torch.int64, device=device)
            self.cnt = torch.empty(6 * self.MAX, dtype=torch.int32, device=device)
            self.sads = torch.empty(self.MAX, dtype=torch.int64, device=device)
        self.h_ring = torch.empty((self.RING, self.Lb), dtype=torch.uint8).pin_memory()
        self.h_offs = torch.empty(4 * self.MAX, dtype=torch.int64).pin_memory()
        self.h_cnt = torch.empty(6 * self.MAX, dtype=torch.int32).pin_memory()
        self.h_sads = torch.empty(self.MAX, dtype=torch.int64).pin_memory()
        self.held = {}                                       # payload index -> ring slot

    def put(self, i, payload):
        sl = i % self.RING
        if sl in self.held.values():
            raise RuntimeError('ivtc: payload %d needs the ring slot of a payload still in use' % i)
        self.held[i] = sl
        self.h_ring[sl].numpy()[:] = np.frombuffer(memoryview(payload).cast('B'), np.uint8)[:self.Lb]
        with torch.cuda.stream(self.stream):
            self.ring[sl].copy_(self.h_ring[sl], non_blocking=True)

    def forget(self, i):
        self.held.pop(i, None)

    def _off(self, i):
        return -1 if i is None else self.held[i] * self.Lb

    def _call(self, offs, launch, dev, host, words):
        """The offsets go up, ``launch`` runs behind them on the stream, ``words`` results come back; one event wait."""
        m = len(offs)
        self.h_offs[:m] = torch.tensor(offs, dtype=torch.int64)
        with torch.cuda.stream(self.stream):
            self.offs[:m].copy_(self.h_offs[:m], non_blocking=True)
            launch(self.stream.cuda_stream)
            host[:words].copy_(dev[:words], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        ev.synchronize()
        return host[:words].tolist()

    def comb(self, entries):
        n = len(entries)
        if n > self.MAX:
            raise RuntimeError('ivtc: %d entries in one call, %d at most' % (n, self.MAX))
        if n == 0:
            return []
        offs = [self._off(t) for t, _ in entries] + [self._off(b) for _, bots in entries for b in bots]
        out = self._call(offs, lambda st: L.check(self.lib.demfi_luma_comb_counts(
            self.ring.data_ptr(), self.offs.data_ptr(), self.offs[n:].data_ptr(), n, self.h, self.w, self.es, self.thresh,
            self.cnt.data_ptr(), st), 'luma_comb_counts'), self.cnt, self.h_cnt, 6 * n)
        return [[None if b is None else (out[6 * i + 2 * k], out[6 * i + 2 * k + 1]) for k, b in enumerate(bots)]
                for i, (_, bots) in enumerate(entries)]

    def sad(self, quads):
        n = len(quads)
        if n > self.MAX:
            raise RuntimeError('ivtc: %d entries in one call, %d at most' % (n, self.MAX))
        if n == 0:
            return []
        return self._call([self._off(i) for q in quads for i in q], lambda st: L.check(self.lib.demfi_luma_woven_sad(
            self.ring.data_ptr(), self.offs.data_ptr(), n, self.h, self.w, self.es, self.sads.data_ptr(), st), 'luma_woven_sad'),
            self.sads, self.h_sads, n)


class LineScorer:
    """The pre-pass of ``--crop auto`` on the GPU (``demfi_amd.letterbox``): the lit samples of every row and column of the luma
    planes of the probed payloads, ``demfi_luma_line_counts`` of csrc/crop.hip, on a stream of its own over device buffers that
    only that stream touches.  ``counts(f, offsets, indices)`` reads only the luma of each probed payload (its first h*w samples,
    by seek) straight into a pinned ring, and per batch of up to MAX planes makes the copies, ONE launch and the copies back, read
    with one event wait; it never waits on the compute stream.  ``probed``: the payloads looked at so far."""
    MAX = 16

    def __init__(self, lib, h, w, depth, limit, device):
        self.lib, self.h, self.w, self.es = lib, h, w, 2 if depth > 8 else 1
        self.thresh = limit << (depth - 8)
        self.Lb = h * w * self.es                            # bytes of a luma plane
        self.stream = torch.cuda.Stream(device)
        with torch.cuda.stream(self.stream):
            self.ring = torch.empty((self.MAX, self.Lb), dtype=torch.uint8, device=device)
            self.offs = torch.arange(self.MAX, dtype=torch.int64, device=device) * self.Lb
            self.rows = torch.empty((self.MAX, h), dtype=torch.int32, device=device)
            self.cols = torch.empty((self.MAX, w), dtype=torch.int32, device=device)
        self.h_ring = torch.empty((self.MAX, self.Lb), dtype=torch.uint8).pin_memory()
        self.h_rows = torch.empty((self.MAX, h), dtype=torch.int32).pin_memory()
        self.h_cols = torch.empty((self.MAX, w), dtype=torch.int32).pin_memory()
        self.probed = 0

    def counts(self, f, offsets, indices):
        """(rows [h], cols [w]) uint32 of payload i of the scanned file ``f`` (``y4m.scan``'s offsets) for every i of ``indices``."""
        from .y4m import file_fetch
        fetch = file_fetch(f, offsets)
        for b0 in range(0, len(indices), self.MAX):
            batch = indices[b0:b0 + self.MAX]
            m = len(batch)
            for j, i in enumerate(batch):
                fetch(i, self.h_ring[j].numpy())
            with torch.cuda.stream(self.stream):
                self.ring[:m].copy_(self.h_ring[:m], non_blocking=True)
                L.check(self.lib.demfi_luma_line_counts(self.ring.data_ptr(), self.offs.data_ptr(), m, self.h, self.w, self.es, self.thresh,
                                                        self.rows.data_ptr(), self.cols.data_ptr(), self.stream.cuda_stream),
                        'luma_line_counts')
                self.h_rows[:m].copy_(self.rows[:m], non_blocking=True)
                self.h_cols[:m].copy_(self.cols[:m], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
            ev.synchronize()
            self.probed += m
            rows, cols = self.h_rows[:m].numpy().view(np.uint32).copy(), self.h_cols[:m].numpy().view(np.uint32).copy()
            for j in range(m):
                yield rows[j], cols[j]
