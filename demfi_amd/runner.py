"""Window scheduler: runs x M interpolation of 4-frame windows on one GPU.

Counterpart of the inner loop of test_custom (/root/reference/main.py:1121-1178) without the PNG codec: the
unpadded window is reflect-padded straight into the engine's input buffer, the t-independent trunk runs once,
then the per-t segment runs for t = k/M.  Launch sequences are captured once into hipGraphs through the C ABI and
replayed (t lives in device memory, so one graph serves every t).

Scheduling (all on ONE GPU, results bit-identical to one forward per (window, t)):
  * the time instants of a window only share the trunk's outputs.  Default: they run as ONE launch sequence over ``n_ctx``
    per-t contexts (``demfi_forward_tb``): every convolution once with batch x n_ctx, the point-wise kernels once per
    context -- the small per-t grids stop paying launch tails / pipeline fill / weight loads once per time instant.
    ``DEMFI_TB=0``: one graph per time instant, consecutive t on ``n_ctx`` separate streams;
  * ``run_windows`` pipelines windows over ``n_trunk`` = 2 trunk contexts: the trunk of window w+1 is queued beside the
    time instants of window w;
  * ``run_clip_u8`` is the host-to-host loop over a whole clip (``demfi_amd.pipeline``): BGR frames in and out, or the Y4M
    edge, where every window runs the instants of its own plan (``retime``; x M is r = M)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from . import retime as R
from .harness import t_schedule
from .pipeline import ClipPipeline, EdgeSpec, fill_sink_records

U16_DTYPES = tuple(d for d in (torch.int16, getattr(torch, 'uint16', None)) if d is not None)   # plain storage of 16-bit frames


def choose_config(H, W, n_tst, mfi, dtype_code, use_graph, n_ctx, n_trunk, auto, retime, env, cached, total_memory, free_memory,
                  workspace_bytes, final_only=False, instant_counts=None):
    """The launch configuration of a WindowRunner at the padded size H x W: {'n_ctx', 'n_trunk', 'batched', 'final_only',
    'chosen_by'}.  Touches neither torch nor the GPU.  env: mapping (the environment); cached: (n_ctx, n_trunk) of an engine the
    model already holds for this frame size, or None; total_memory: bytes of the device; free_memory(): its free bytes (called
    for ``auto`` only); workspace_bytes: ``demfi_workspace_bytes``.
    Explicit n_ctx / n_trunk are taken as given.  Otherwise env DEMFI_NCTX / DEMFI_NTRUNK, else the shape of the cached engine
    (batched x M plan only, when its n_ctx > 1 divides M-1), else FIXED values that depend on the arguments and the part only
    (7 / 3 at 720p x8, fp16 N_tst=3 as well as fp32 N_tst=5; 5 / 3 at 1080p x16 fp16); ``auto`` (or env DEMFI_AUTO=1) opts into a
    probe of the free memory instead.  DEMFI_TB=0: the non-batched plan.  retime (a Fraction): ``retime.default_n_ctx``, over
    ``instant_counts`` (the instants per window over a period) when the edge runs only some of the ratio's instants (a shutter); such a
    schedule may pad an eighth of its instants for a larger n_ctx, since its window counts are seldom multiples of anything."""
    def ws(trunks, ctxs):
        return workspace_bytes(H, W, max(n_tst, 3), dtype_code, trunks, ctxs)
    auto = bool(auto or env.get('DEMFI_AUTO') == '1')
    env_trunk, env_ctx = env.get('DEMFI_NTRUNK'), env.get('DEMFI_NCTX')
    # batched (default): the time instants of a window run as ONE launch sequence over n_ctx per-t contexts (demfi_forward_tb)
    tb = bool(use_graph and (retime is not None or mfi > 2) and env.get('DEMFI_TB', '1') != '0')
    # a cached engine is taken over (batched mode) instead of probing the memory again -- a second runner (bench.py's
    # final_only one) must not force a second multi-GB engine; a plain forward()'s engine (n_ctx 1) says nothing
    if not (tb and retime is None and cached is not None and cached[0] > 1):
        cached = None
    how = 'explicit' if (n_ctx is not None or n_trunk is not None) else None
    if n_trunk is None and env_trunk:
        n_trunk, how = int(env_trunk), 'env'
    if n_trunk is None and cached is not None:
        n_trunk, how = cached[1], 'cached engine'
    if tb:
        if n_ctx is None and env_ctx:
            n_ctx, how = int(env_ctx), 'env'
        if n_ctx is None and retime is not None:
            # fewest padded per-t slots over one period of the schedule, among the sizes whose workspace fits the GPU
            how = how or 'retime schedule'
            n_ctx = R.default_n_ctx(retime, lambda d: 0 < ws(n_trunk or 2, d) <= total_memory, counts=instant_counts,
                                    slack=Fraction(1, 8) if instant_counts is not None else 0)
            if n_trunk is None and n_ctx > 1:    # n_ctx = 1 falls back to the non-batched plan and its two trunk sets
                n_trunk = 3 if 0 < ws(3, n_ctx) <= total_memory // 2 else 2
        if n_ctx is None and cached is not None and (mfi - 1) % cached[0] == 0:
            n_ctx, how = cached[0], 'cached engine'
        if n_ctx is None and auto:
            # opt-in probe: the largest divisor of M-1 (<= 8) whose workspace fits 85 % of the free memory.  The launch plan
            # (and the throughput) then depends on co-tenants of the GPU -- never the default
            how = 'memory probe'
            free = free_memory()
            n_ctx = 1
            for d in range(min(8, mfi - 1), 1, -1):
                if (mfi - 1) % d == 0 and 0 < ws(n_trunk or 2, d) < 0.85 * free:
                    n_ctx = d
                    break
            if n_ctx > 1 and n_trunk is None and 0 < ws(3, n_ctx) < 0.5 * free:
                n_trunk = 3
        if n_ctx is None:
            # FIXED default: all time instants of a window in one launch sequence when M-1 <= 8 (7 at x8), else the largest
            # divisor of M-1 that is <= 8 (5 at x16); three trunk sets (a third window in flight: +0.7 % at 720p) when their workspace
            # stays below half of the device's memory (a function of the part, not of co-tenants), two otherwise
            how = how or 'fixed default'
            n_ctx = max(d for d in range(1, min(8, mfi - 1) + 1) if (mfi - 1) % d == 0)
            if n_trunk is None:
                n_trunk = 3 if 0 < ws(3, n_ctx) <= total_memory // 2 else 2
        elif n_ctx > 1 and (mfi - 1) % n_ctx and retime is None:
            raise ValueError('WindowRunner: n_ctx=%d must divide M-1=%d for the batched per-t plan' % (n_ctx, mfi - 1))
        n_ctx = int(n_ctx)
        tb = n_ctx > 1
    n_trunk = (n_trunk or 2) if use_graph else 1
    if not tb:
        if n_ctx is None:
            how = 'env' if env_ctx else how
        most = R.max_instants(retime) if retime is not None else max(1, mfi - 1)
        n_ctx = (int(n_ctx) if n_ctx else min(int(env_ctx or 5), most)) if (use_graph and (retime is not None or mfi > 2)) else 1
        final_only = False                           # a mode of the batched plan
    need = ws(n_trunk, n_ctx)
    if need > total_memory:
        raise RuntimeError('WindowRunner: workspace of %.1f GB for n_ctx=%d, n_trunk=%d at %dx%d exceeds the GPU memory; pass smaller '
                           'n_ctx / n_trunk (or auto=True to probe)' % (need / 1e9, n_ctx, n_trunk, H, W))
    return {'n_ctx': n_ctx, 'n_trunk': n_trunk, 'batched': tb, 'final_only': bool(final_only), 'chosen_by': how or 'fixed default'}


class WindowRunner:
    def __init__(self, model, height, width, n_tst=3, mfi=8, use_graph=True, final_only=False, n_ctx=None, n_trunk=None, auto=False,
                 retime=None, tiles=None, instant_counts=None):
        """final_only: produce the frames of the LAST recursion only (what test / test_custom consume, utils.py:1430-1434):
        the warp + D2 tail of the earlier recursions feeds nothing else and is skipped (batched plan only); the delivered
        frames are bit-identical.
        n_ctx / n_trunk: per-t contexts batched into one launch sequence / trunk buffer sets pipelined over windows.  Explicit
        values are taken as given (n_ctx must divide M-1 for the batched plan; the workspace must fit or engine creation
        fails loudly).  None = default: ``choose_config``.  The chosen values and how they were chosen are exposed as
        ``self.n_ctx`` / ``self.n_trunk`` / ``self.config`` and printed by bench.py.
        retime: output / input frame rate ratio r in 1/64 .. 64 (a Fraction) of the Y4M edge of ``run_clip_u8`` in place of x M: window k
        runs the instants of ``retime.window_plan`` (``mfi`` is not used).  An explicit n_ctx is taken as given; the default is
        ``retime.default_n_ctx`` over the sizes whose workspace fits the GPU.  ``instants_run`` / ``instants_padded`` count the
        time instants run and the padded per-t slots of short batched chunks.  instant_counts: the instants per window, over one period,
        of an edge that runs only some of the ratio's instants (``shutter.period_counts``); the default n_ctx is then sized by them.
        tiles: a multi-tile ``tiling.Plan`` whose tile size is height x width: ``run_clip_u8`` then takes and gives frames of the
        plan's size and runs every window once per tile (``demfi_amd.pipeline``); every other entry point stays at the tile's size."""
        if tiles is not None and (tiles.n_tiles < 2 or tuple(tiles.tile) != (height, width)):
            raise ValueError('WindowRunner: tiles must be a plan of several %dx%d tiles, got %d of %dx%d' %
                             ((height, width, tiles.n_tiles) + tuple(tiles.tile)))
        self.tiles = tiles
        self._g_trunk = self._g_t = self._g_body = self._g_tb = None
        self._out_u8 = self._s01_u8 = self.out_d1 = self.s01_d1 = self._pipeline = None
        self._sink_tabs = {}                         # every attribute exists from here on, for __del__ and the lazy allocations
        self.h, self.w = height, width
        H = (height + 31) // 32 * 32
        W = (width + 31) // 32 * 32
        if retime is not None and not isinstance(retime, (int, Fraction)):
            raise TypeError('WindowRunner: retime must be an int or a Fraction, got %r' % (retime,))
        self.retime = Fraction(retime) if retime is not None else None
        if self.retime is not None and not Fraction(1, R.MAX_RATIO) <= self.retime <= R.MAX_RATIO:
            raise ValueError('WindowRunner: retime ratio %s outside 1/%d .. %d' % (self.retime, R.MAX_RATIO, R.MAX_RATIO))
        self.lib = L.load()
        eng = model._engines.get((H, W, model.path_dtype))     # the plain slot only: never forward()'s batch engine
        self.config = choose_config(
            H, W, n_tst, mfi, L.F32 if model.path_dtype == torch.float32 else L.F16, use_graph, n_ctx, n_trunk, auto, self.retime,
            env=os.environ, cached=(eng.n_ctx, eng.n_trunk) if eng is not None else None, final_only=final_only,
            total_memory=torch.cuda.get_device_properties(model.device).total_memory if torch.cuda.is_available() else 288 * 10 ** 9,
            free_memory=lambda: torch.cuda.mem_get_info(model.device)[0], workspace_bytes=self.lib.demfi_workspace_bytes,
            instant_counts=instant_counts)
        self.n_ctx, self.n_trunk, self.tb, self.final_only = (self.config[k] for k in ('n_ctx', 'n_trunk', 'batched', 'final_only'))
        self.model = model
        self._HW = (H, W)
        self.engine = model.engine(H, W, n_tst, n_ctx=self.n_ctx, n_trunk=self.n_trunk, exact_ctx=self.tb)
        self._weights_version = model._weights_version
        self.n_tst, self.mfi = n_tst, mfi
        self.ratio = self.retime if self.retime is not None else Fraction(mfi)     # r of the Y4M edge of run_clip_u8: x M is r = M
        dev = self.engine.device
        self.stream = torch.cuda.Stream(dev)                                   # trunk stream
        self.t_streams = [torch.cuda.Stream(dev) for _ in range(self.n_ctx)]   # one per per-t context
        if self.retime is None:
            self.ts = [float(t) for t in t_schedule(mfi)]
            self.out = torch.zeros((mfi - 1, 3, height, width), dtype=torch.float32, device=dev)   # St per t (run_window)
            self.s01 = torch.zeros((2, 3, height, width), dtype=torch.float32, device=dev)          # S0, S1 (first t)
            self.t_all = torch.tensor(self.ts, dtype=torch.float32, device=dev)
        else:                                        # a retimed runner serves run_clip_u8's Y4M edge only: no x M buffers
            self.ts = self.out = self.s01 = self.t_all = None
        self.use_graph = use_graph
        self._next_ctx = self._next_trunk = 0
        self._t_done = [None] * self.n_trunk        # events: the per-t work that last read trunk context k
        self.instants_run = 0                        # time instants run (padded slots not counted)
        self.instants_padded = 0                     # per-t slots of short batched chunks that ran a repeated t and wrote nothing
        self.cut_windows = 0                         # windows run as scene-cut windows (two runs, no interpolation)
        self.windows_skipped = 0                     # r < 1: windows of the Y4M edge that own no output and ran nothing
        self.shutter_mixed = self.shutter_carried = 0    # a shutter's fine frames mixed / samples carried between batches (``y4m_edge.Shutter``)
        self.interlace_woven = self.interlace_carried = 0    # interlaced output: payloads woven / frames carried between batches (``y4m_edge.Interlacer``)
        self.scale_payloads = 0                      # resized output: payloads resampled (``y4m_edge.Scaler``)
        self.depth_promoted = self.depth_requantised = 0     # bit depth: payloads promoted at ingest / requantised at egress (``demfi_amd.bitdepth``)
        self.denoised = 0                            # temporal denoiser: frames denoised at ingest (``demfi_amd.denoise``)
        self.deblocked = 0                           # deblocking: payloads deblocked at ingest (``demfi_amd.deblock``)
        self.deringed = 0                            # deringing: payloads deringed at ingest (``demfi_amd.dering``)
        self.debanded = 0                            # debanding: payloads debanded at ingest (``demfi_amd.deband``)
        self.nlm_filtered = 0                        # spatial denoising: payloads filtered at ingest (``demfi_amd.nlmeans``)
        self.grain_payloads = 0                     # film grain: payloads grained at egress (``y4m_edge.Grain``)
        self.lut_payloads = 0                       # 3D colour LUT: payloads taken through the cube at egress (``y4m_edge.Lut``)
        self.colour_encoded = 0                      # linear light: payloads taken back to Y'CbCr (``y4m_edge.Encoder``)
        self.last_cuts = []                          # frames that start a scene, as the last run_clip_u8 with scene cuts found them

    # ---------------------------------------------------------------------------------------------------------
    def _check_device(self, t, what):
        """Raw device pointers go straight to the kernels: a host tensor or one on another GPU must fail in Python."""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.engine.device):
            raise ValueError('demfi_amd.WindowRunner: %s must be a tensor on %s (got %s)' %
                             (what, self.engine.device, getattr(t, 'device', type(t))))

    def _check_u8_frames(self, frames_u8):
        if len(frames_u8) != 4:
            raise ValueError('expected 4 uint8 frames (B0,B1,B-1,B2), got %d' % len(frames_u8))
        for f in frames_u8:
            self._check_device(f, 'uint8 frame')
            if f.dtype != torch.uint8 or tuple(f.shape) != (self.h, self.w, 3) or not f.is_contiguous():
                raise ValueError('uint8 frames must be contiguous [%d,%d,3] uint8 tensors, got %s %s' %
                                 (self.h, self.w, f.dtype, tuple(f.shape)))

    def _capture(self, fn, stream):
        h = stream.cuda_stream
        L.check(self.lib.demfi_graph_begin(h), 'graph_begin')
        try:
            fn(h)
        finally:
            g = C.c_void_p()
            L.check(self.lib.demfi_graph_end(h, C.byref(g)), 'graph_end')
        return g

    def _prepare_graphs(self):
        e = self.engine
        if self._g_trunk is not None or not self.use_graph:
            return
        h = self.stream.cuda_stream
        # the engine may come from the model's cache, used before by another runner whose uint8 sink records still point at
        # that runner's (possibly freed) output buffers: the warm-up below must write nothing, so every record is disabled first
        with torch.cuda.stream(self.stream):
            for row in e._ctxs:
                for ctx in row:
                    ctx['sink'].zero_()
        for k in range(self.n_trunk):                # warm every context (module load, attributes) before capture
            e.use_ctx(0, trunk=k)
            e.run_trunk(h)
            if self.tb:
                e.run_tb(h, self.n_tst, self.final_only)
            else:
                for c in range(self.n_ctx):
                    e.use_ctx(c)
                    e.run_t(h, self.n_tst)
        self.stream.synchronize()
        self._g_trunk, self._g_t, self._g_body, self._g_tb = [], [], [], []
        for k in range(self.n_trunk):
            e.use_ctx(0, trunk=k)
            self._g_trunk.append(self._capture(e.run_trunk, self.stream))
            self._g_body.append(self._capture(e.run_trunk_body, self.stream))     # trunk after the fused uint8 ingest
            if self.tb:
                self._g_tb.append(self._capture(lambda s: e.run_tb(s, self.n_tst, self.final_only), self.t_streams[0]))
                continue
            gs = []
            for c in range(self.n_ctx):
                e.use_ctx(c)
                gs.append(self._capture(lambda s: e.run_t(s, self.n_tst), self.t_streams[c]))
            self._g_t.append(gs)
        for s in self.t_streams:
            s.synchronize()
        e.use_ctx(0, trunk=0)

    def _window(self, load, emit, body_only=False, pre=None, t_dev=None, nt=None):
        """One window: load(engine, stream_handle) fills the bound trunk context's input on the trunk stream;
        emit(j, ctx, stream_handle) copies the outputs of time instant j out of the per-t context ``ctx`` (the last recursion's
        frames are ctx['finals'][n_tst - 1], Stage I's ctx['sharp1']) on that context's stream.
        body_only: load() already did the trunk's prologue (fused uint8 ingest).  pre(j, ctx): runs on the per-t stream before
        the per-t segment of time instant j (sets the uint8 sink record).
        t_dev / nt: the window's own nt instants (device fp32, padded to a multiple of n_ctx with the last t) in place of the
        x M schedule.  A short last batched chunk runs its padded slots with an all-zero (disabled) sink record: they compute
        and write nothing, and neither pre nor emit is called for them."""
        e = self.engine
        if t_dev is None:
            if self.retime is not None:
                raise ValueError('WindowRunner: a retimed runner runs the Y4M edge of run_clip_u8 only, not the x M entry points')
            t_dev, nt = self.t_all, self.mfi - 1
        self.instants_run += nt
        k = self._next_trunk
        self._next_trunk = (k + 1) % self.n_trunk
        if self._t_done[k] is not None:              # the time instants that last read trunk context k must be done
            for ev in self._t_done[k]:
                self.stream.wait_event(ev)
        e.use_ctx(0, trunk=k)
        with torch.cuda.stream(self.stream):
            h = self.stream.cuda_stream
            load(e, h)
            if self.use_graph:
                L.check(self.lib.demfi_graph_launch((self._g_body if body_only else self._g_trunk)[k], h), 'graph_launch')
            elif body_only:
                e.run_trunk_body(h)
            else:
                e.run_trunk(h)
            ev_trunk = torch.cuda.Event()
            ev_trunk.record(self.stream)
        if self.tb:
            # batched: chunks of n_ctx consecutive time instants, each ONE graph replay over all per-t contexts of trunk set k.
            # One stream per trunk set: consecutive windows own disjoint buffer sets, so their sequences may overlap (the tail
            # of one launch fills with the head of the other window's: +2-4 % like two processes sharing the GPU)
            st = self.t_streams[k % len(self.t_streams)]
            st.wait_event(ev_trunk)
            with torch.cuda.stream(st):
                for j0 in range(0, nt, self.n_ctx):
                    cnt = min(self.n_ctx, nt - j0)
                    self.instants_padded += self.n_ctx - cnt
                    e._tb[k]['t_col'].copy_(t_dev[j0:j0 + self.n_ctx], non_blocking=True)
                    if pre is not None:
                        for c in range(cnt):
                            pre(j0 + c, e._ctxs[k][c])
                        if cnt < self.n_ctx:
                            e._tb[k]['sink_all'][cnt:].zero_()
                    else:
                        e._tb[k]['sink_all'].zero_()  # float path: a sink left by an earlier uint8 run must not fire
                    L.check(self.lib.demfi_graph_launch(self._g_tb[k], st.cuda_stream), 'graph_launch')
                    for c in range(cnt):
                        emit(j0 + c, e._ctxs[k][c], st.cuda_stream)
                ev = torch.cuda.Event()
                ev.record(st)
            self._t_done[k] = [ev]
            return
        used = set()
        for j in range(nt):
            c = self._next_ctx
            self._next_ctx = (c + 1) % self.n_ctx
            st = self.t_streams[c]
            ctx = e._ctxs[k][c]
            if c not in used:
                st.wait_event(ev_trunk)
                used.add(c)
            with torch.cuda.stream(st):
                ctx['t_dev'].copy_(t_dev[j:j + 1], non_blocking=True)
                if pre is not None:
                    pre(j, ctx)
                else:
                    ctx['sink'].zero_()              # float path: a sink left by an earlier uint8 run must not fire
                if self.use_graph:
                    L.check(self.lib.demfi_graph_launch(self._g_t[k][c], st.cuda_stream), 'graph_launch')
                else:
                    e.use_ctx(c)
                    e.run_t(st.cuda_stream, self.n_tst)
                emit(j, ctx, st.cuda_stream)
        evs = []
        for c in used:
            ev = torch.cuda.Event()
            ev.record(self.t_streams[c])
            evs.append(ev)
        self._t_done[k] = evs

    def _destroy_graphs(self):
        gs = list(self._g_trunk or []) + list(self._g_body or []) + list(self._g_tb or [])
        for row in (self._g_t or []):
            gs += list(row)
        self._g_trunk = self._g_t = self._g_body = self._g_tb = None
        for g in gs:
            if g is not None:
                self.lib.demfi_graph_destroy(g)

    def _begin(self):
        if self.model._weights_version != self._weights_version:
            # the model's weights were reloaded: the old engine's blob (and the graphs pointing at it) are stale
            torch.cuda.synchronize(self.engine.device)
            self._destroy_graphs()
            self.engine = self.model.engine(self._HW[0], self._HW[1], self.n_tst, n_ctx=self.n_ctx, n_trunk=self.n_trunk, exact_ctx=self.tb)
            self._weights_version = self.model._weights_version
            self._t_done = [None] * self.n_trunk
        cur = torch.cuda.current_stream(self.engine.device)
        self.stream.wait_stream(cur)                 # inputs produced on the caller's stream
        for s in self.t_streams:
            s.wait_stream(cur)                       # output buffers may still be read there
        self._prepare_graphs()
        return cur

    def _end(self, cur):
        cur.wait_stream(self.stream)
        for s in self.t_streams:
            cur.wait_stream(s)
        self.engine.use_ctx(0, trunk=0)

    def _emitter(self, put, out, s01, s0_at=0, s1_at=0, frames=None):
        """emit(j, ctx, sh) of ``_window``: put(frame, dst, sh) writes St of instant j to out[j] and S0 / S1 of instants s0_at / s1_at to
        s01[0] / s01[1].  frames(ctx): the per-t context's [S0, S1, St]; default: those of the last recursion."""
        last = self.n_tst - 1

        def emit(j, ctx, sh):
            fin = ctx['finals'][last] if frames is None else frames(ctx)
            put(fin[2], out[j], sh)
            if j == s0_at:
                put(fin[0], s01[0], sh)
            if j == s1_at:
                put(fin[1], s01[1], sh)
        return emit

    def _crop(self, frame, dst, sh):                 # ``put`` of the fp32 entry points: the padded [3,H,W] frame without its padding
        dst.copy_(frame[:, :self.h, :self.w], non_blocking=True)

    def _loader(self, x):
        if tuple(x.shape) != (1, 3, 4, self.h, self.w):
            raise ValueError('expected a [1,3,4,%d,%d] window, got %s' % (self.h, self.w, tuple(x.shape)))
        self._check_device(x, 'window')
        x = x.contiguous().float()                   # the pad kernel reads raw [3,4,h,w] memory

        def load(e, h):
            if (self.h, self.w) != (e.H, e.W):
                L.check(self.lib.demfi_reflect_pad(x.data_ptr(), e.x.data_ptr(), 12, self.h, self.w, e.H, e.W, h), 'pad')
            else:
                e.x.copy_(x[0], non_blocking=True)
        return load

    # ---------------------------------------------------------------------------------------------------------
    def run_window(self, x, with_d1=False, s0_at=0, s1_at=0):
        """x: [1,3,4,h,w] fp32 on the GPU.  Returns (St [M-1,3,h,w], S0S1 [2,3,h,w]) -- views of reused buffers.
        with_d1: also the Stage-I frames ``Sharps_prime`` (DeMFInet.py:95-103): (St, S0S1, St' [M-1,3,h,w], S0'S1' [2,3,h,w]).
        s0_at / s1_at: index of the time instant whose S0 / S1 are kept (Stage I's S0' / S1' depend on t through the refinement
        module, DeMFInet.py:75-103; the reference's test() keeps S0 at t = 0.5 and S1 at the last t, main.py:918-955, 633-645)."""
        load = self._loader(x)
        cur = self._begin()
        if with_d1 and self.out_d1 is None:
            self.out_d1 = torch.zeros_like(self.out)
            self.s01_d1 = torch.zeros_like(self.s01)

        emit = self._emitter(self._crop, self.out, self.s01, s0_at, s1_at)
        if with_d1:                                  # then Stage I's frames, sharp1 [9,H,W]: S0', S1', St'
            both = emit, self._emitter(self._crop, self.out_d1, self.s01_d1, s0_at, s1_at, lambda ctx: ctx['sharp1'].unflatten(0, (3, 3)))
            emit = lambda j, ctx, sh: [e(j, ctx, sh) for e in both]   # noqa: E731
        self._window(load, emit)
        self._end(cur)
        if with_d1:
            return self.out, self.s01, self.out_d1, self.s01_d1
        return self.out, self.s01

    def run_windows(self, xs, out=None, s01=None):
        """Pipelined run of several windows (list of [1,3,4,h,w] fp32 GPU tensors, all ready on the current stream).
        Returns (St [n,M-1,3,h,w], S0S1 [n,2,3,h,w]); pass preallocated ``out`` / ``s01`` to reuse memory."""
        n = len(xs)
        dev = self.engine.device
        if out is None:
            out = torch.empty((n, self.mfi - 1, 3, self.h, self.w), dtype=torch.float32, device=dev)
        if s01 is None:
            s01 = torch.empty((n, 2, 3, self.h, self.w), dtype=torch.float32, device=dev)
        loads = [self._loader(x) for x in xs]
        cur = self._begin()
        for w in range(n):
            self._window(loads[w], self._emitter(self._crop, out[w], s01[w]))
        self._end(cur)
        return out, s01

    def _sink_table(self, out, s01):
        """Device table of demfi_u8_sink records, one per (window, time instant) of the output buffers out [n,M-1,h,w,3] /
        s01 [n,2,h,w,3]: segment 0 / 1 / 2 of the last layer = S0 / S1 / St (S0, S1 are kept from the first time instant
        only, main.py:1165-1172).  Cached per output buffer."""
        key = (out.data_ptr(), s01.data_ptr(), out.shape[0], out.stride()[:2], s01.stride()[:2])
        tab = self._sink_tabs.get(key)
        if tab is None:
            n, m1 = out.shape[0], self.mfi - 1
            (so0, so1), (ss0, ss1) = out.stride()[:2], s01.stride()[:2]              # uint8: element strides are bytes
            first = np.arange(m1)[None, :] == 0
            s0 = (s01.data_ptr() + ss0 * np.arange(n, dtype=np.int64))[:, None]
            st = out.data_ptr() + so0 * np.arange(n, dtype=np.int64)[:, None] + so1 * np.arange(m1, dtype=np.int64)[None, :]
            a = fill_sink_records(np.empty((n, m1, 32), np.int64), st, np.where(first, s0, 0), np.where(first, s0 + ss1, 0),
                                  self.h, self.w, self.n_tst)
            tab = torch.from_numpy(a).to(self.engine.device)
            if len(self._sink_tabs) > 8:
                self._sink_tabs.clear()
            self._sink_tabs[key] = tab
        return tab

    def _u8_io(self, frames_u8, out_u8, s01_u8, sink_rows=None):
        """(load, emit, pre) of one uint8 window: 4 BGR uint8 [h,w,3] GPU frames in -> out_u8 [M-1,h,w,3], s01_u8 [2,h,w,3].
        Ingest: ONE kernel (normalise + reflect pad + pixel reshuffle + overlay) straight into the trunk context.  Egress:
        with ``sink_rows`` (rows of _sink_table) the last layer's epilogue writes the uint8 frames itself; otherwise one
        crop + denorm + truncate kernel per frame (fp32 path)."""
        e = self.engine
        self._check_u8_frames(frames_u8)
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in frames_u8])

        def load(eng, h):
            eng.ingest_u8(ptrs, self.h, self.w, h)

        if sink_rows is not None:
            def pre(j, ctx):
                ctx['sink'][:32].copy_(sink_rows[j], non_blocking=True)
            return load, (lambda j, ctx, sh: None), pre

        def put(frame, dst, sh):
            L.check(self.lib.demfi_frame_to_u8(frame.data_ptr(), dst.data_ptr(), self.h, self.w, e.H, e.W, sh), 'to_u8')
        return load, self._emitter(put, out_u8, s01_u8), None

    def run_window_u8(self, frames_u8):
        """uint8 in / uint8 out: frames_u8 = 4 BGR uint8 [h,w,3] GPU tensors in the order (B0,B1,B-1,B2).  Returns
        (St uint8 [M-1,h,w,3], S0S1 uint8 [2,h,w,3]).  Normalisation + reflect padding are fused into ONE kernel writing
        the engine input; crop + denorm + uint8 truncation into one kernel per output frame."""
        e = self.engine
        if self._out_u8 is None:
            self._out_u8 = torch.zeros((self.mfi - 1, self.h, self.w, 3), dtype=torch.uint8, device=e.device)
            self._s01_u8 = torch.zeros((2, self.h, self.w, 3), dtype=torch.uint8, device=e.device)
        rows = self._sink_table(self._out_u8[None], self._s01_u8[None])[0] if e.supports_u8_sink else None
        load, emit, pre = self._u8_io(frames_u8, self._out_u8, self._s01_u8, rows)
        cur = self._begin()
        self._window(load, emit, body_only=True, pre=pre)
        self._end(cur)
        return self._out_u8, self._s01_u8

    def run_windows_u8(self, windows_u8, out=None, s01=None):
        """Pipelined uint8 run of several windows (list of 4-tuples of BGR uint8 [h,w,3] GPU frames, ready on the current
        stream): the scheduling of run_windows with the uint8 ingest / egress kernels of run_window_u8.
        Returns (St uint8 [n,M-1,h,w,3], S0S1 uint8 [n,2,h,w,3])."""
        n = len(windows_u8)
        dev = self.engine.device
        if out is None:
            out = torch.empty((n, self.mfi - 1, self.h, self.w, 3), dtype=torch.uint8, device=dev)
        if s01 is None:
            s01 = torch.empty((n, 2, self.h, self.w, 3), dtype=torch.uint8, device=dev)
        tab = self._sink_table(out, s01) if self.engine.supports_u8_sink else None
        io = [self._u8_io(windows_u8[i], out[i], s01[i], None if tab is None else tab[i]) for i in range(n)]
        cur = self._begin()
        for load, emit, pre in io:
            self._window(load, emit, body_only=True, pre=pre)
        self._end(cur)
        return out, s01

    # ---- 16-bit frames (bit depth 10 .. 16 of the Y4M edge; 8 to compare with the uint8 path) -------------------------------
    def _check_u16_frames(self, frames_u16, depth, shape, also=()):
        # the 4 frames a 16-bit window reads, and the frames ``also`` it writes: device tensors of ``shape`` in 16-bit storage
        if depth not in (8, 10, 12, 14, 16):
            raise ValueError('bit depth must be 8, 10, 12, 14 or 16, got %r' % (depth,))
        if len(frames_u16) != 4:
            raise ValueError('expected 4 16-bit frames (B0,B1,B-1,B2), got %d' % len(frames_u16))
        for f in list(frames_u16) + list(also):
            self._check_device(f, '16-bit frame')
            if f.dtype not in U16_DTYPES or tuple(f.shape) != shape or not f.is_contiguous():
                raise ValueError('16-bit frames must be contiguous [%d,%d,3] int16 / uint16 tensors (the bits of uint16 values), got %s %s' %
                                 (shape[0], shape[1], f.dtype, tuple(f.shape)))

    def _u16_io(self, frames_u16, out_u16, s01_u16, depth):
        """(load, emit, pre) of one 16-bit window, the counterpart of ``_u8_io``: 4 BGR [h,w,3] GPU frames of 16-bit storage
        (``torch.int16`` holding the bits of uint16 values 0 .. 2^depth - 1; only pointers reach the library) in ->
        out_u16 [J,h,w,3], s01_u16 [2,h,w,3] of the same storage.  Ingest: ONE kernel (``demfi_u16_ingest``).  Egress: always
        the emit path, one ``demfi_frame_to_u16`` per frame (the fused sink of the fp16 engine writes uint8 only)."""
        e = self.engine
        self._check_u16_frames(frames_u16, depth, (self.h, self.w, 3))
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in frames_u16])

        def load(eng, h):
            eng.ingest_u16(ptrs, self.h, self.w, depth, h)

        def put(frame, dst, sh):
            L.check(self.lib.demfi_frame_to_u16(frame.data_ptr(), dst.data_ptr(), self.h, self.w, e.H, e.W, depth, sh), 'to_u16')
        return load, self._emitter(put, out_u16, s01_u16), None      # no pre: _window then disables every uint8 sink record

    def _u16_tile_io(self, slots4, tile, out_full, s01_full, depth):
        """(load, emit, pre) of one (run, tile) pair of a runner of ``tiles``, the counterpart of ``_u16_io``: ``slots4`` are 4 BGR
        frames of the PLAN's size [fh,fw,3] (16-bit storage), ``tile`` one ``tiling.Tile`` of the plan; out_full [J,fh,fw,3] and
        s01_full [2,fh,fw,3] are full output frames.  Ingest: ONE kernel reads the tile's source rectangle in place
        (``demfi_u16_ingest_rect``).  Egress: one ``demfi_frame_to_u16_rect`` per frame writes the tile's kept rectangle only; the
        kept rectangles of a plan partition the frame, so its tiles fill a frame between them in any order."""
        e, plan = self.engine, self.tiles
        if plan is None or tile not in plan.tiles:
            raise ValueError('_u16_tile_io: a runner of tiles and one tile of its plan')
        fh, fw = plan.h, plan.w
        self._check_u16_frames(slots4, depth, (fh, fw, 3), also=list(out_full) + list(s01_full))
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in slots4])
        (y0, x0, _, _), k = tile.src, tile.keep

        def load(eng, h):
            eng.ingest_u16_rect(ptrs, fh, fw, y0, x0, self.h, self.w, depth, h)

        def put(frame, dst, sh):
            L.check(self.lib.demfi_frame_to_u16_rect(frame.data_ptr(), dst.data_ptr(), fh, fw, y0, x0, k.y0, k.x0, k.y1, k.x1, e.H, e.W,
                                                     depth, sh), 'to_u16_rect')

        return load, self._emitter(put, out_full, s01_full), None

    def run_windows_u16(self, windows_u16, depth, out=None, s01=None, ts=None):
        """``run_windows_u8`` for 16-bit frames at bit depth ``depth`` (list of 4-tuples of BGR [h,w,3] ``torch.int16`` GPU
        frames, ready on the current stream), with the same scheduling.  Returns (St [n,M-1,h,w,3], S0S1 [n,2,h,w,3]) as
        ``torch.int16`` storage of uint16 values (``.cpu().numpy().view(numpy.uint16)``).
        ts: per window, the float32 instants it runs in place of the x M schedule (what a retimed runner needs: the instants
        of ``retime.window_plan``); St is then [n, max len(ts), h, w, 3] and the rows past a window's instants are not written."""
        n = len(windows_u16)
        dev = self.engine.device
        if ts is not None and len(ts) != n:
            raise ValueError('run_windows_u16: %d lists of instants for %d windows' % (len(ts), n))
        nj = self.mfi - 1 if ts is None else max([len(t) for t in ts] or [0])
        if out is None:
            out = torch.empty((n, nj, self.h, self.w, 3), dtype=torch.int16, device=dev)
        if s01 is None:
            s01 = torch.empty((n, 2, self.h, self.w, 3), dtype=torch.int16, device=dev)
        for t in (out, s01):
            self._check_device(t, 'output buffer')
            if t.dtype not in U16_DTYPES:
                raise ValueError('run_windows_u16: the output buffers hold 16-bit values (torch.int16), got %s' % t.dtype)
        io = [self._u16_io(windows_u16[i], out[i], s01[i], depth) for i in range(n)]
        t_dev = None
        if ts is not None:                           # padded to whole chunks of n_ctx with the window's last t, as the Y4M edge does
            njp = -(-nj // self.n_ctx) * self.n_ctx if self.tb else nj
            tt = np.empty((n, max(njp, 1)), np.float32)
            for w, t in enumerate(ts):
                tt[w, :len(t)] = t
                tt[w, len(t):] = t[-1]
            t_dev = torch.from_numpy(tt).to(dev)
        cur = self._begin()
        for w, (load, emit, pre) in enumerate(io):
            if t_dev is None:
                self._window(load, emit, body_only=True, pre=pre)
            else:
                self._window(load, emit, body_only=True, pre=pre, t_dev=t_dev[w], nt=len(ts[w]))
        self._end(cur)
        return out, s01

    # ---------------------------------------------------------------------------------------------------------
    def run_clip_u8(self, host_frames, windows, sink=None, batch=4, reuse_frames=True, yuv=None, window_index=None):
        """Host-to-host run of a list of windows: the counterpart of the test_custom loop (/root/reference/main.py:
        1121-1178) between cv2.imread and cv2.imwrite.

        host_frames: sequence of uint8 [h,w,3] CPU tensors (BGR, as cv2.imread returns them; pinned memory makes the
        copies asynchronous); windows: list of (B0, B1, B-1, B2) index 4-tuples into it; sink(k, St, S0S1): called in
        window order with uint8 CPU tensors St [M-1,h,w,3], S0S1 [2,h,w,3] (views of pinned staging buffers, valid until
        the sink returns).  Windows are processed in batches of ``batch``: the H2D of a batch's frames (own stream), the
        pipelined compute and the D2H of the previous batch's uint8 frames (own stream) overlap; a frame is uploaded
        once when ``reuse_frames`` (consecutive windows share three frames), else once per window it appears in.
        ``windows`` may also be an iterator of unknown length (a stream): it is pulled one batch at a time.

        yuv: Y4M stream edge (``demfi_amd.video.YuvEdge``: matrix, full_range, siting, with_s1(k)).  host_frames[i] is then
        a 4:2:0 payload (1-D uint8 CPU tensor), converted once on the GPU after its H2D copy.  Window k (its global index is
        ``window_index(j)`` for the j-th window of ``windows`` when given, else B-1 of its 4-tuple) runs the instants of
        ``retime.window_plan`` for the ratio r = ``retime`` (constructor), or r = M on a runner built without it: S0, then St for
        t = 1/M .. (M-1)/M; plus S1 when ``with_s1(k)`` says window k is the clip's last.  ONE ``demfi_bgr_to_yuv420_gather``
        launch per batch puts its outputs in stream order, and sink(k, payloads) gets uint8 [c, payload], the c payloads
        window k owns (``pipeline.Y4mEdge``).
        ``yuv.full_length`` (retimed runners only, with ``window_index``): the full-length timeline of ``retime``; ``windows``
        are then the tuples clamped at the clip's ends, and the last window's S1 hold repeats its S1 slot in the gather.
        ``yuv.scene_cut`` = T (retimed runners only; ``--mfi M`` is r = M): scene cuts (``demfi_amd.scene``).  ``windows`` must
        then be the consecutive unclamped tuples, and host_frames must also hold frame k0 - 1 when the first window k0 >= 1.
        Each batch's new payloads are scored by ONE ``demfi_yuv420_sad`` launch before its windows are planned: window k runs
        ``scene.window_runs``, a cut window as two runs.  The cuts found are in ``last_cuts``; ``cut_windows`` counts the cut
        windows.
        A runner of ``tiles``: the frames (and payloads) have the plan's size, every run is one run per tile, and
        ``instants_run`` / ``instants_padded`` count those.
        ``yuv.depth`` > 8 (10, 12, 14, 16): the payloads hold 16-bit little-endian samples (host_frames[i] is still a 1-D
        uint8 tensor, of twice the bytes, and so are the payloads the sink gets); the frame slots and everything between the
        two conversions are 16-bit (csrc/yuv_family.hip, ``_u16_io``).  On a runner of ``tiles`` every (run, tile) pair reads its
        tile out of the full 16-bit frame slots and writes its kept rectangle into the full output frames (``_u16_tile_io``):
        nothing is cropped or stitched.
        ``yuv.layout`` ('420' when absent; ``y4m.LAYOUTS``): the payloads' chroma layout; 4:2:2, 4:4:4 and mono payloads are
        converted by csrc/yuv_family.hip and the outputs keep the layout.
        ``yuv.dedup`` = (hi, lo, frac, max_hold) (None when absent; retimed runners only, with ``window_index``): repeated
        frames are left out (``demfi_amd.cadence``).  host_frames is then a ``pipeline.KeptFrames`` over the input and ``windows``
        its ``windows()``: frames and windows are named by kept index, every input frame is scored on the GPU as it is
        uploaded (ONE ``demfi_luma_block_counts`` launch each), and window k runs ``cadence.window_runs``.
        ``yuv.fields`` = 't' / 'b' (None when absent): the input is interlaced with that field order (``demfi_amd.deint``).
        host_frames[f] is then the payload that holds FIELD f (``y4m.Frames(fields=2)``); every uploaded payload is bobbed in place
        on the GPU (``demfi_yuv_bob``) before it is converted or scored, and everything else runs as on the progressive stream of
        those frames.  ``yuv.deint_mode`` = 'adaptive' ('bob' when absent): every field is rebuilt by the motion-adaptive rule instead
        (``demfi_yuv_deint_adaptive``), which reads fields f-2 .. f+2: host_frames must then also hold the two fields before the first
        one named and answer ``has(f)`` for the fields after the last (``y4m.Frames(behind=2)``); not together with ``yuv.dedup``.
        ``yuv.depths`` = (input depth, working depth, output depth, dither mode or None) (None when absent; ``demfi_amd.bitdepth``):
        ``yuv.depth`` is the working depth, host_frames[i] holds samples of the input's depth, which are promoted on the GPU behind
        their upload (``demfi_payload_promote``), and the payloads the sink gets have the output's depth, requantised on the GPU as the
        last stage (``demfi_payload_requant``).
        ``yuv.denoise`` = (A, B, R) (None when absent; ``demfi_amd.denoise``): every frame is denoised on the GPU from the frames up to R
        before and after it (over the fields of ``yuv.fields``: 2 R, those of its parity) behind the promotion and the bob
        (``demfi_payload_denoise``) and everything else runs on the denoised stream; host_frames must then also hold that many frames before
        the first one named and answer ``has(f)`` for those after the last (``y4m.Frames(behind=reach)``); not together with ``yuv.dedup``
        or the adaptive ``yuv.deint_mode``.
        ``yuv.deblock`` = (A, B) (None when absent; ``demfi_amd.deblock``): every uploaded payload is deblocked in place on the GPU behind
        the promotion and in front of everything else (``demfi_payload_deblock``), on the grid of 8 shifted by ``yuv.crop_rect`` (the
        rectangle the payloads were cropped to, None when absent); goes with everything.
        ``yuv.dering`` = (P, S, D) (None when absent; ``demfi_amd.dering``): every uploaded payload is deringed on the GPU behind the
        deblocker and in front of everything else (one device copy into a scratch buffer, then ``demfi_payload_dering`` back into place),
        on the same grid; goes with everything.
        ``yuv.deband`` = (T, R) (None when absent; ``demfi_amd.deband``): every uploaded payload is debanded on the GPU behind the deringing
        filter and in front of everything else (one device copy into the scratch buffer the deringing filter uses, then
        ``demfi_payload_deband`` back into place); goes with everything.
        ``yuv.nlmeans`` = (S, P, R) (None when absent; ``demfi_amd.nlmeans``): every uploaded payload is denoised within the frame on the GPU
        behind the deringing filter and in front of the debander (one device copy into the same scratch buffer, then
        ``demfi_payload_nlmeans`` back into place); goes with everything.
        Returns the number of windows run."""
        spec = EdgeSpec.of(yuv)
        spec.check(self.retime is not None, window_index is not None, reuse_frames)
        if self._pipeline is None or self._pipeline.key != (batch, spec):
            self._pipeline = None                        # release the old buffers before the new ones are allocated
            self._pipeline = ClipPipeline(self, batch, spec)
        return self._pipeline.run(host_frames, windows, sink, reuse_frames, yuv, window_index)

    def __del__(self):
        try:
            self._destroy_graphs()
        except Exception:
            pass
