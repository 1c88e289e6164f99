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
    time instants of window w."""
import ctypes as C
import itertools
import os

import torch

from fractions import Fraction

from . import _lib as L
from . import retime as R
from . import scene as S
from .harness import t_schedule
from .y4m import payload_size


class WindowRunner:
    def __init__(self, model, height, width, n_tst=3, mfi=8, use_graph=True, final_only=False, n_ctx=None, n_trunk=None, auto=False,
                 retime=None):
        """final_only: produce the frames of the LAST recursion only (what test / test_custom consume, utils.py:1430-1434):
        the warp + D2 tail of the earlier recursions feeds nothing else and is skipped (batched plan only); the delivered
        frames are bit-identical.
        n_ctx / n_trunk: per-t contexts batched into one launch sequence / trunk buffer sets pipelined over windows.  Explicit
        values are taken as given (n_ctx must divide M-1 for the batched plan; the workspace must fit or engine creation
        fails loudly).  None = default: env DEMFI_NCTX / DEMFI_NTRUNK, else the configuration of an engine the model
        already holds for this frame size, else FIXED values that depend on the arguments only (7 / 3 at 720p x8 fp16, 7 / 2 at
        720p fp32 N_tst=5, 5 / 3 at 1080p x16); ``auto=True`` (or env DEMFI_AUTO=1) opts into a probe of the free memory instead.  The chosen values and
        how they were chosen are exposed as ``self.n_ctx`` / ``self.n_trunk`` / ``self.config`` and printed by bench.py.
        retime: output / input frame rate ratio r >= 1 (a Fraction) of the Y4M edge of ``run_clip_u8`` in place of x M: window k
        runs the instants of ``retime.window_plan`` (``mfi`` is not used).  An explicit n_ctx is taken as given; the default is
        ``retime.default_n_ctx`` over the sizes whose workspace fits the GPU.  ``instants_run`` / ``instants_padded`` count the
        time instants run and the padded per-t slots of short batched chunks."""
        auto = bool(auto or os.environ.get('DEMFI_AUTO') == '1')
        self.final_only = bool(final_only)
        self.h, self.w = height, width
        H = (height + 31) // 32 * 32
        W = (width + 31) // 32 * 32
        env_trunk = os.environ.get('DEMFI_NTRUNK')
        env_ctx = os.environ.get('DEMFI_NCTX')
        # batched mode (default): the time instants of a window run as ONE launch sequence whose convolutions are batched
        # over n_ctx per-t contexts (demfi_forward_tb).  DEMFI_TB=0: one graph per time instant on n_ctx streams (round-2a).
        if retime is not None and not isinstance(retime, (int, Fraction)):
            raise TypeError('WindowRunner: retime must be an int or a Fraction, got %r' % (retime,))
        self.retime = Fraction(retime) if retime is not None else None
        if self.retime is not None and not 1 <= self.retime <= R.MAX_RATIO:
            raise ValueError('WindowRunner: retime ratio %s outside 1 .. %d' % (self.retime, R.MAX_RATIO))
        if self.retime is not None:
            self.tb = bool(use_graph and os.environ.get('DEMFI_TB', '1') != '0')
        else:
            self.tb = bool(use_graph and mfi > 2 and os.environ.get('DEMFI_TB', '1') != '0')
        # a runner built earlier on this model for the same frame size fixed the engine's shape: take it over (batched mode) instead
        # of probing the memory again -- a second runner (bench.py's final_only one) must not force a second multi-GB engine
        cached = getattr(model, '_engines', {}).get((H, W, model.path_dtype)) if (self.tb and self.retime is None) else None     # the plain slot only: never forward()'s batch engine
        if cached is not None and cached.n_ctx <= 1:     # a plain forward()'s engine says nothing about a runner's configuration
            cached = None
        how = 'explicit' if (n_ctx is not None or n_trunk is not None) else None
        if n_trunk is None and env_trunk:
            n_trunk, how = int(env_trunk), 'env'
        if n_trunk is None and cached is not None:
            n_trunk, how = cached.n_trunk, 'cached engine'
        lib = L.load()
        dt = L.F32 if model.path_dtype == torch.float32 else L.F16
        if self.tb:
            if n_ctx is None and env_ctx:
                n_ctx, how = int(env_ctx), 'env'
            if n_ctx is None and self.retime is not None:
                # fewest padded per-t slots over one period of the schedule, among the sizes whose workspace fits the GPU
                how = how or 'retime schedule'
                total = torch.cuda.get_device_properties(model.device).total_memory if torch.cuda.is_available() else 288 * 10 ** 9
                n_ctx = R.default_n_ctx(self.retime, lambda d: 0 < lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, n_trunk or 2, d) <= total)
                if n_trunk is None and n_ctx > 1:    # n_ctx = 1 falls back to the non-batched plan and its two trunk sets
                    n_trunk = 3 if 0 < lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, 3, n_ctx) <= total // 2 else 2
            if n_ctx is None and cached is not None and (mfi - 1) % cached.n_ctx == 0:
                n_ctx, how = cached.n_ctx, 'cached engine'
            if n_ctx is None and auto:
                # opt-in probe: the largest divisor of M-1 (<= 8) whose workspace fits 85 % of the free memory.  The launch plan
                # (and the throughput) then depends on co-tenants of the GPU -- never the default
                how = 'memory probe'
                free = torch.cuda.mem_get_info(model.device)[0]
                n_ctx = 1
                for d in range(min(8, mfi - 1), 1, -1):
                    if (mfi - 1) % d == 0 and 0 < lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, n_trunk or 2, d) < 0.85 * free:
                        n_ctx = d
                        break
                if n_ctx > 1 and n_trunk is None and 0 < lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, 3, n_ctx) < 0.5 * free:
                    n_trunk = 3
            if n_ctx is None:
                # FIXED default, a function of the arguments only: all time instants of a window in one launch sequence when
                # M-1 <= 8 (7 at x8), else the largest divisor of M-1 that is <= 8 (5 at x16); three trunk sets (a third window in
                # flight: +0.7 % at 720p) when their workspace stays below half of the device's memory (144 GB on an MI355X), two otherwise.  Engine creation fails loudly when the
                # workspace does not fit the GPU -- nothing is silently scaled down.
                how = how or 'fixed default'
                n_ctx = max(d for d in range(1, min(8, mfi - 1) + 1) if (mfi - 1) % d == 0)
                if n_trunk is None:
                    # half of THIS device's memory (144 GB on an MI355X): a function of the arguments and the part, not of co-tenants
                    half = (torch.cuda.get_device_properties(model.device).total_memory // 2) if torch.cuda.is_available() else 144 * 10 ** 9
                    n_trunk = 3 if 0 < lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, 3, n_ctx) <= half else 2
            elif n_ctx > 1 and (mfi - 1) % n_ctx and self.retime is None:
                raise ValueError('WindowRunner: n_ctx=%d must divide M-1=%d for the batched per-t plan' % (n_ctx, mfi - 1))
            self.n_ctx = int(n_ctx)
            self.tb = self.n_ctx > 1
        self.n_trunk = (n_trunk or 2) if use_graph else 1
        if not self.tb:
            if n_ctx is None:
                how = 'env' if env_ctx else (how or 'fixed default')
            if self.retime is not None:
                self.n_ctx = (int(n_ctx) if n_ctx else min(int(env_ctx or 5), R.max_instants(self.retime))) if use_graph else 1
            else:
                self.n_ctx = (int(n_ctx) if n_ctx else min(int(env_ctx or 5), max(1, mfi - 1))) if (use_graph and mfi > 2) else 1
            self.final_only = False                  # a mode of the batched plan
        how = how or 'fixed default'
        need = lib.demfi_workspace_bytes(H, W, max(n_tst, 3), dt, self.n_trunk, self.n_ctx)
        if torch.cuda.is_available() and need > torch.cuda.get_device_properties(model.device).total_memory:
            raise RuntimeError('WindowRunner: workspace of %.1f GB for n_ctx=%d, n_trunk=%d at %dx%d exceeds the GPU memory; pass smaller '
                               'n_ctx / n_trunk (or auto=True to probe)' % (need / 1e9, self.n_ctx, self.n_trunk, H, W))
        self.config = {'n_ctx': self.n_ctx, 'n_trunk': self.n_trunk, 'batched': self.tb, 'final_only': self.final_only, 'chosen_by': how}
        self.model = model
        self._HW = (H, W)
        self.engine = model.engine(H, W, n_tst, n_ctx=self.n_ctx, n_trunk=self.n_trunk, exact_ctx=self.tb)
        self._weights_version = model._weights_version
        self.n_tst, self.mfi = n_tst, mfi
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
        self.lib = L.load()
        self.use_graph = use_graph
        self._g_trunk = None
        self._g_t = None
        self._next_ctx = 0
        self._next_trunk = 0
        self._t_done = [None] * self.n_trunk        # events: the per-t work that last read trunk context k
        self.instants_run = 0                        # time instants run (padded slots not counted)
        self.instants_padded = 0                     # per-t slots of short batched chunks that ran a repeated t and wrote nothing
        self.cut_windows = 0                         # windows run as scene-cut windows (two runs, no interpolation)
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

    def _window(self, load, emit, body_only=False, pre=None, emit_ctx=False, t_dev=None, nt=None):
        """One window: load(engine, stream_handle) fills the bound trunk context's input on the trunk stream;
        emit(j, finals, stream_handle) copies the outputs of time instant j out of a per-t context on that context's stream.
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
                        if emit_ctx:
                            emit(j0 + c, e._ctxs[k][c]['finals'][self.n_tst - 1], st.cuda_stream, e._ctxs[k][c])
                        else:
                            emit(j0 + c, e._ctxs[k][c]['finals'][self.n_tst - 1], st.cuda_stream)
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
                if emit_ctx:
                    emit(j, ctx['finals'][self.n_tst - 1], st.cuda_stream, ctx)
                else:
                    emit(j, ctx['finals'][self.n_tst - 1], st.cuda_stream)
        evs = []
        for c in used:
            ev = torch.cuda.Event()
            ev.record(self.t_streams[c])
            evs.append(ev)
        self._t_done[k] = evs

    def _destroy_graphs(self):
        gs = list(self._g_trunk or []) + list(getattr(self, '_g_body', None) or [])
        self._g_body = None
        for row in (self._g_t or []):
            gs += list(row)
        gs += list(getattr(self, '_g_tb', None) or [])
        self._g_tb = None
        for g in gs:
            if g is not None:
                self.lib.demfi_graph_destroy(g)
        self._g_trunk = self._g_t = None

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
        if with_d1 and getattr(self, 'out_d1', None) is None:
            self.out_d1 = torch.zeros_like(self.out)
            self.s01_d1 = torch.zeros_like(self.s01)

        def emit(j, fin, sh, ctx=None):
            self.out[j].copy_(fin[2, :, :self.h, :self.w], non_blocking=True)
            if j == s0_at:
                self.s01[0].copy_(fin[0, :, :self.h, :self.w], non_blocking=True)
            if j == s1_at:
                self.s01[1].copy_(fin[1, :, :self.h, :self.w], non_blocking=True)
            if with_d1:
                d1 = ctx['sharp1']                   # [9,H,W]: S0', S1', St'
                self.out_d1[j].copy_(d1[6:9, :self.h, :self.w], non_blocking=True)
                if j == s0_at:
                    self.s01_d1[0].copy_(d1[0:3, :self.h, :self.w], non_blocking=True)
                if j == s1_at:
                    self.s01_d1[1].copy_(d1[3:6, :self.h, :self.w], non_blocking=True)
        self._window(load, emit, emit_ctx=with_d1)
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
            def emit(j, fin, sh, w=w):
                out[w, j].copy_(fin[2, :, :self.h, :self.w], non_blocking=True)
                if j == 0:
                    s01[w, 0].copy_(fin[0, :, :self.h, :self.w], non_blocking=True)
                    s01[w, 1].copy_(fin[1, :, :self.h, :self.w], non_blocking=True)
            self._window(loads[w], emit)
        self._end(cur)
        return out, s01

    def _sink_table(self, out, s01):
        """Device table of demfi_u8_sink records, one per (window, time instant) of the output buffers out [n,M-1,h,w,3] /
        s01 [n,2,h,w,3]: segment 0 / 1 / 2 of the last layer = S0 / S1 / St (S0, S1 are kept from the first time instant
        only, main.py:1165-1172).  Cached per output buffer."""
        key = (out.data_ptr(), s01.data_ptr(), out.shape[0], out.stride()[:2], s01.stride()[:2])
        tab = self._sink_tabs.get(key) if hasattr(self, '_sink_tabs') else None
        if tab is None:
            import numpy as np
            n, m1 = out.shape[0], self.mfi - 1
            a = np.zeros((n, m1, 32), np.int64)                  # 256-byte records (the context's "sink" buffer)
            (so0, so1), (ss0, ss1) = out.stride()[:2], s01.stride()[:2]          # uint8: element strides are bytes
            for i in range(n):
                for j in range(m1):
                    a[i, j, 2] = out.data_ptr() + i * so0 + j * so1                  # frame[2] = St
                    if j == 0:
                        a[i, j, 0] = s01.data_ptr() + i * ss0                         # frame[0] = S0
                        a[i, j, 1] = s01.data_ptr() + i * ss0 + ss1                   # frame[1] = S1
                    a[i, j, 8] = self.h | (self.w << 32)                              # int32 h, w
                    a[i, j, 9] = self.n_tst - 1                                        # int32 iter, pad
            tab = torch.from_numpy(a).to(self.engine.device)
            if not hasattr(self, '_sink_tabs'):
                self._sink_tabs = {}
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
            return load, (lambda j, fin, sh: None), pre

        def emit(j, fin, sh):
            L.check(self.lib.demfi_frame_to_u8(fin[2].data_ptr(), out_u8[j].data_ptr(), self.h, self.w, e.H, e.W, sh), 'to_u8')
            if j == 0:
                for i in range(2):
                    L.check(self.lib.demfi_frame_to_u8(fin[i].data_ptr(), s01_u8[i].data_ptr(), self.h, self.w, e.H, e.W, sh),
                            'to_u8')
        return load, emit, None

    def run_window_u8(self, frames_u8):
        """uint8 in / uint8 out: frames_u8 = 4 BGR uint8 [h,w,3] GPU tensors in the order (B0,B1,B-1,B2).  Returns
        (St uint8 [M-1,h,w,3], S0S1 uint8 [2,h,w,3]).  Normalisation + reflect padding are fused into ONE kernel writing
        the engine input; crop + denorm + uint8 truncation into one kernel per output frame."""
        e = self.engine
        if getattr(self, '_out_u8', None) is None:
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
        a 4:2:0 payload (1-D uint8 CPU tensor): its H2D copy is followed by ONE ``demfi_yuv420_to_bgr`` launch per run of
        consecutive slots, so each frame is converted once.  After the sink's buffers of a batch are written, one
        ``demfi_bgr_to_yuv420`` launch puts its frames in stream order (per window S0, then St for t = 1/M .. (M-1)/M; plus
        S1 when ``with_s1(k)`` says window k is the clip's last) into a device buffer that is copied to pinned memory, and
        sink(k, payloads) gets uint8 [M or M+1, payload] per window.
        With ``retime`` (constructor) the Y4M edge follows ``retime.window_plan`` instead: window k (its global index is
        ``window_index(j)`` for the j-th window of ``windows`` when given, else B-1 of its 4-tuple) runs its own instants, its
        frames sit in [S0, St x ceil(r), S1] slots, and ONE ``demfi_bgr_to_yuv420_gather`` launch per batch puts its outputs in
        stream order; sink(k, payloads) gets as many payloads as window k owns.
        ``yuv.full_length`` (retimed runners only, with ``window_index``): the full-length timeline of ``retime``; ``windows``
        are then the tuples clamped at the clip's ends, and the last window's S1 hold repeats its S1 slot in the gather.
        ``yuv.scene_cut`` = T (retimed runners only; ``--mfi M`` is r = M): scene cuts (``demfi_amd.scene``).  ``windows`` must
        then be the consecutive unclamped tuples, and host_frames must also hold frame k0 - 1 when the first window k0 >= 1.
        Each batch's new payloads are scored by ONE ``demfi_yuv420_sad`` launch on the h2d stream, read back with one event wait,
        before its windows are planned: window k runs ``scene.window_runs``, a cut window as two runs.  The cuts found are in
        ``last_cuts``; ``cut_windows`` counts the cut windows.  Returns the number of windows run."""
        dev = self.engine.device
        it = iter(windows)
        wins = list(itertools.islice(it, batch))
        if not wins:
            return 0
        M1 = self.mfi - 1
        threshold = getattr(yuv, 'scene_cut', None)
        full = bool(getattr(yuv, 'full_length', False))
        mode = ('bgr' if yuv is None else 'yuv' if threshold is None else 'yuv+cuts') + ('+full' if full else '')
        if self.retime is not None and yuv is None:
            raise ValueError('WindowRunner.run_clip_u8: a retimed runner needs the Y4M edge (yuv=...)')
        if threshold is not None and (self.retime is None or not reuse_frames):
            raise ValueError('WindowRunner.run_clip_u8: scene cuts need a retimed runner (r = M for x M) and reuse_frames')
        if full and (self.retime is None or window_index is None):
            raise ValueError('WindowRunner.run_clip_u8: the full-length timeline needs a retimed runner and window_index')
        runs_max = 2 * batch if threshold is not None else batch        # a cut window is two runs
        if getattr(self, '_clip', None) is None or self._clip['batch'] != batch or self._clip['mode'] != mode:
            self._clip = None
            nslot = 4 * batch + 4 if not reuse_frames else 2 * batch + 8
            cl = {'batch': batch, 'mode': mode, 'h2d': torch.cuda.Stream(dev), 'd2h': torch.cuda.Stream(dev),
                  'slots': torch.empty((max(nslot, 4 * batch * 2), self.h, self.w, 3), dtype=torch.uint8, device=dev)}
            if yuv is None:
                cl.update({
                    'out': [torch.empty((batch, M1, self.h, self.w, 3), dtype=torch.uint8, device=dev) for _ in range(2)],
                    's01': [torch.empty((batch, 2, self.h, self.w, 3), dtype=torch.uint8, device=dev) for _ in range(2)],
                    'h_out': [torch.empty((batch, M1, self.h, self.w, 3), dtype=torch.uint8).pin_memory() for _ in range(2)],
                    'h_s01': [torch.empty((batch, 2, self.h, self.w, 3), dtype=torch.uint8).pin_memory() for _ in range(2)],
                })
            elif self.retime is not None:
                # per window [S0, St x J, S1] with J = ceil(r) >= |T_k|; the outputs of a batch are gathered into stream order
                P = payload_size(self.h, self.w)
                J = R.max_instants(self.retime)
                nJ = -(-J // self.n_ctx) * self.n_ctx if self.tb else J      # instants incl. the padding of a short chunk
                nsl = cl['slots'].shape[0]
                # payloads of a batch: at most J per window, plus the last window's S1 (full-length: its [n-2, n) span, 2 J)
                nout = (batch + 1) * J if full else batch * J + 1
                comb = [torch.empty((runs_max, J + 2, self.h, self.w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
                cl.update({
                    'J': J, 'comb': comb, 'yuv_in': torch.empty((nsl, P), dtype=torch.uint8, device=dev),
                    't': [torch.empty((runs_max, nJ), dtype=torch.float32, device=dev) for _ in range(2)],
                    'sinks': [torch.empty((runs_max, nJ, 32), dtype=torch.int64, device=dev) for _ in range(2)],
                    'offs': [torch.empty(nout, dtype=torch.int64, device=dev) for _ in range(2)],
                    'yuv_out': [torch.empty((nout, P), dtype=torch.uint8, device=dev) for _ in range(2)],
                    'h_yuv': [torch.empty((nout, P), dtype=torch.uint8).pin_memory() for _ in range(2)],
                })
                if threshold is not None:                # SADs of a batch's new frames (at most nsl) against their predecessors
                    cl.update({'sad': torch.empty(nsl, dtype=torch.int64, device=dev),
                               'sad_offs': torch.empty(2 * nsl, dtype=torch.int64, device=dev),
                               'h_sad': torch.empty(nsl, dtype=torch.int64).pin_memory()})
            else:
                # per window [S0, St x (M-1), S1]: the frames of a batch in stream order are M per window at a fixed stride
                P = payload_size(self.h, self.w)
                comb = [torch.empty((batch, self.mfi + 1, self.h, self.w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
                cl.update({
                    'comb': comb, 'out': [c[:, 1:self.mfi] for c in comb], 's01': [c[:, 0::self.mfi] for c in comb],
                    'yuv_in': torch.empty((cl['slots'].shape[0], P), dtype=torch.uint8, device=dev),
                    'yuv_out': [torch.empty((batch * self.mfi + 1, P), dtype=torch.uint8, device=dev) for _ in range(2)],
                    'h_yuv': [torch.empty((batch * self.mfi + 1, P), dtype=torch.uint8).pin_memory() for _ in range(2)],
                })
            self._clip = cl
        cl = self._clip
        slots = cl['slots']
        nslot = slots.shape[0]
        cur = torch.cuda.current_stream(dev)
        slot_of = {}                      # frame key -> slot
        slot_busy = [None] * nslot        # event: compute of the batch that last read the slot
        next_slot = 0
        ev_done = [None, None]            # compute of the batch that last wrote device output buffer i
        ev_d2h = [None, None]             # D2H of that batch
        pending = None                    # (first window, count, buffer[, frames per window]) whose D2H is in flight
        n = 0
        b = 0
        det = None
        if threshold is not None:
            det = S.Detector(cl['yuv_in'].shape[1], threshold,
                             first=S.first_frame(window_index(0) if window_index is not None else wins[0][2]))
            self.last_cuts = det.cuts
        while wins:
            i = b & 1
            # ---- H2D of the frames this batch needs (copy stream) -------------------------------------------------
            dev_wins = []
            new_slots = []
            new_frames = []
            with torch.cuda.stream(cl['h2d']):
                # scene cuts: the block's first window k0 >= 1 also needs frame k0 - 1, the predecessor SAD_k0 is taken against
                first = [(-1, [det.next - 1])] if det is not None and b == 0 and det.next - 1 < wins[0][2] else []
                for wi, win in first + list(enumerate(wins)):
                    fr = []
                    for idx in win:
                        key = idx if reuse_frames else (b, wi, idx)
                        sl = slot_of.get(key)
                        if sl is None:
                            sl = next_slot
                            next_slot = (next_slot + 1) % nslot
                            for k_old, s_old in list(slot_of.items()):
                                if s_old == sl:
                                    del slot_of[k_old]
                            if slot_busy[sl] is not None:
                                cl['h2d'].wait_event(slot_busy[sl])
                            new_frames.append(idx)
                            f = host_frames[idx]
                            if yuv is not None:
                                if tuple(f.shape) != tuple(cl['yuv_in'].shape[1:]) or f.dtype != torch.uint8:
                                    raise ValueError('frame %d: expected a uint8 [%d] 4:2:0 payload, got %s %s' %
                                                     (idx, cl['yuv_in'].shape[1], f.dtype, tuple(f.shape)))
                                cl['yuv_in'][sl].copy_(f, non_blocking=True)
                                new_slots.append(sl)
                            else:
                                if tuple(f.shape) != (self.h, self.w, 3) or f.dtype != torch.uint8:
                                    raise ValueError('frame %d: expected uint8 [%d,%d,3], got %s %s' % (idx, self.h, self.w, f.dtype, tuple(f.shape)))
                                slots[sl].copy_(f, non_blocking=True)
                            slot_of[key] = sl
                        fr.append(slots[sl])
                    if wi >= 0:
                        dev_wins.append(fr)
                if yuv is not None:
                    self._yuv_ingest(new_slots, yuv)
                if det is not None:
                    self._scene_sads(det, new_frames, slot_of)
                ev_up = torch.cuda.Event()
                ev_up.record(cl['h2d'])
            # ---- compute (pipelined windows) ---------------------------------------------------------------------
            cur.wait_event(ev_up)
            if ev_d2h[i] is not None:
                cur.wait_event(ev_d2h[i])                     # the D2H of batch b-2 has read this output buffer
            if self.retime is not None:
                runs, outs = [], []                      # runs: (frames, instants, kinds kept); outs[w]: (run, kind, instant index)
                for wi, win in enumerate(wins):
                    # window k's unclamped tuple is (k+1, k+2, k, k+3); clamped tuples come with their index
                    k = window_index(n + wi) if window_index is not None else win[2]
                    last = yuv.with_s1(n + wi)
                    if det is None:
                        ts, o = R.window_plan(k, self.retime, last, full)
                        wr, o = [(dev_wins[wi], ts)], [(0, kind, j) for _, kind, j in o]
                    else:
                        is_cut = S.with_sentinels(det.is_cut, k + 3 if last else None) if full else det.is_cut
                        sr, so = S.window_runs(k, self.retime, last, is_cut, full)
                        wr = [([slots[slot_of[x]] for x in S.runner_order(tup)], ts) for tup, ts in sr]
                        o = [(run, kind, j) for _, run, kind, j in so]
                        self.cut_windows += len(sr) - 1
                    outs.append([(len(runs) + run, kind, j) for run, kind, j in o])
                    runs += [(fr, ts, {kind for run, kind, _ in o if run == ri}) for ri, (fr, ts) in enumerate(wr)]
                self._run_windows_rt(i, runs)
                nf = self._yuv_egress_rt(i, outs, yuv, cur)
                dev_wins = [fr for fr, _, _ in runs]     # the frames the compute reads (slot_busy below)
            else:
                self.run_windows_u8(dev_wins, out=cl['out'][i][:len(wins)], s01=cl['s01'][i][:len(wins)])
                nf = self._yuv_egress(i, n, len(wins), yuv, cur) if yuv is not None else None
            ev = torch.cuda.Event()
            ev.record(cur)
            ev_done[i] = ev
            for fr in dev_wins:
                for t in fr:
                    slot_busy[(t.data_ptr() - slots.data_ptr()) // t.numel()] = ev
            # ---- hand the previous batch to the sink while this one computes ------------------------------------------
            if pending is not None:
                self._drain(pending, ev_d2h, sink)
            # ---- D2H of this batch (copy stream), into pinned staging ------------------------------------------------
            with torch.cuda.stream(cl['d2h']):
                cl['d2h'].wait_event(ev)
                if yuv is not None:
                    nt = sum(nf) if isinstance(nf, list) else nf
                    cl['h_yuv'][i][:nt].copy_(cl['yuv_out'][i][:nt], non_blocking=True)
                else:
                    cl['h_out'][i][:len(wins)].copy_(cl['out'][i][:len(wins)], non_blocking=True)
                    cl['h_s01'][i][:len(wins)].copy_(cl['s01'][i][:len(wins)], non_blocking=True)
                e2 = torch.cuda.Event()
                e2.record(cl['d2h'])
                ev_d2h[i] = e2
            pending = (n, len(wins), i, nf)
            n += len(wins)
            b += 1
            wins = list(itertools.islice(it, batch))
        self._drain(pending, ev_d2h, sink)
        return n

    def _drain(self, pending, ev_d2h, sink):
        k0, cnt, i, nf = pending
        ev_d2h[i].synchronize()
        if sink is None:
            return
        if isinstance(nf, list):                         # retimed Y4M: nf[j] payloads of window k0 + j, in stream order
            hy, pos = self._clip['h_yuv'][i], 0
            for j, c in enumerate(nf):
                sink(k0 + j, hy[pos:pos + c])
                pos += c
            return
        if nf is not None:                               # Y4M: M payloads per window, the last one's S1 after them
            hy = self._clip['h_yuv'][i]
            for j in range(cnt):
                sink(k0 + j, hy[j * self.mfi:(j + 1) * self.mfi + (1 if j == cnt - 1 and nf > cnt * self.mfi else 0)])
            return
        for j in range(cnt):
            sink(k0 + j, self._clip['h_out'][i][j], self._clip['h_s01'][i][j])

    def _yuv_ingest(self, slots, yuv):
        """4:2:0 payloads already copied to yuv_in[slot] -> BGR slots[slot], one launch per run of consecutive slots (h2d stream)."""
        cl = self._clip
        h2d = cl['h2d'].cuda_stream
        P = cl['yuv_in'].shape[1]
        fsz = self.h * self.w * 3
        r = 0
        while r < len(slots):
            e = r + 1
            while e < len(slots) and slots[e] == slots[e - 1] + 1:
                e += 1
            L.check(self.lib.demfi_yuv420_to_bgr(cl['yuv_in'][slots[r]].data_ptr(), P, cl['slots'][slots[r]].data_ptr(), fsz, e - r,
                                                 self.h, self.w, yuv.matrix, int(yuv.full_range), yuv.siting, h2d), 'yuv420_to_bgr')
            r = e

    def _yuv_egress(self, i, k0, cnt, yuv, cur):
        """Frames of a computed batch (comb[i]: per window S0, St..., S1) -> yuv_out[i] in stream order on the compute stream;
        returns the number of payloads."""
        cl = self._clip
        comb, dst = cl['comb'][i], cl['yuv_out'][i]
        P = dst.shape[1]
        fsz = self.h * self.w * 3
        nf = cnt * self.mfi
        L.check(self.lib.demfi_bgr_to_yuv420(comb.data_ptr(), fsz, self.mfi, comb.stride(0), dst.data_ptr(), P, nf, self.h, self.w,
                                             yuv.matrix, int(yuv.full_range), cur.cuda_stream), 'bgr_to_yuv420')
        if yuv.with_s1(k0 + cnt - 1):                    # the clip's last window: its S1 closes the stream
            L.check(self.lib.demfi_bgr_to_yuv420(comb[cnt - 1, self.mfi].data_ptr(), fsz, 1, 0, dst[nf].data_ptr(), P, 1, self.h,
                                                 self.w, yuv.matrix, int(yuv.full_range), cur.cuda_stream), 'bgr_to_yuv420')
            nf += 1
        return nf

    def _run_windows_rt(self, i, runs):
        """Retimed batch: run w = (4 frames, instants, kinds) runs its instants (``retime.window_plan``, or a run of a scene-cut
        window); its frames go to comb[i][w] = [S0, St x J, S1].  The t values and the uint8 sink records (one per (run, instant);
        S0 / S1 only in the row of the run's first instant and only when ``kinds`` holds that frame) are uploaded on the current
        stream."""
        import numpy as np
        cl = self._clip
        comb, J = cl['comb'][i], cl['J']
        nw, nJ = len(runs), cl['t'][i].shape[1]
        tt = np.empty((nw, nJ), np.float32)
        for w, (_, ts, _) in enumerate(runs):
            tt[w, :len(ts)] = ts
            tt[w, len(ts):] = ts[-1]                     # padded slots repeat the last t
        t_dev = cl['t'][i][:nw]
        t_dev.copy_(torch.from_numpy(tt).pin_memory(), non_blocking=True)
        rows = None
        if self.engine.supports_u8_sink:
            a = np.zeros((nw, nJ, 32), np.int64)         # rows past a window's instants stay zero (disabled)
            base, (c0, c1) = comb.data_ptr(), comb.stride()[:2]      # uint8: element strides are bytes
            for w, (_, ts, kinds) in enumerate(runs):
                for j in range(len(ts)):
                    a[w, j, 2] = base + w * c0 + (1 + j) * c1                          # frame[2] = St
                    a[w, j, 8] = self.h | (self.w << 32)                                # int32 h, w
                    a[w, j, 9] = self.n_tst - 1                                         # int32 iter, pad
                if R.S0 in kinds:
                    a[w, 0, 0] = base + w * c0                                          # frame[0] = S0
                if R.S1 in kinds:
                    a[w, 0, 1] = base + w * c0 + (J + 1) * c1                           # frame[1] = S1
            rows = cl['sinks'][i][:nw]
            rows.copy_(torch.from_numpy(a).pin_memory(), non_blocking=True)
        io = [self._u8_io(fr, comb[w, 1:J + 1], comb[w, 0::J + 1], None if rows is None else rows[w]) for w, (fr, _, _) in enumerate(runs)]
        cur = self._begin()
        for w, (load, emit, pre) in enumerate(io):
            self._window(load, emit, body_only=True, pre=pre, t_dev=t_dev[w], nt=len(runs[w][1]))
        self._end(cur)

    def _yuv_egress_rt(self, i, outs, yuv, cur):
        """Outputs of a retimed batch (comb[i]) -> yuv_out[i] in stream order: ONE gather launch on the compute stream.
        outs[w]: window w's outputs as (run, kind, instant index).  Returns the number of payloads per window."""
        cl = self._clip
        comb, dst, J = cl['comb'][i], cl['yuv_out'][i], cl['J']
        c0, c1 = comb.stride()[:2]
        offs, counts = [], []
        for o in outs:
            for run, kind, j in o:
                offs.append(run * c0 + (0 if kind == R.S0 else J + 1 if kind == R.S1 else 1 + j) * c1)
            counts.append(len(o))
        nf = len(offs)
        if nf > dst.shape[0]:
            raise RuntimeError('retime: %d outputs for %d payload slots' % (nf, dst.shape[0]))
        od = cl['offs'][i][:nf]
        od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
        L.check(self.lib.demfi_bgr_to_yuv420_gather(comb.data_ptr(), od.data_ptr(), dst.data_ptr(), dst.shape[1], nf, self.h, self.w,
                                                    yuv.matrix, int(yuv.full_range), cur.cuda_stream), 'bgr_to_yuv420_gather')
        return counts

    def _scene_sads(self, det, new_frames, slot_of):
        """SAD_j of every frame j just uploaded against frame j-1 (``demfi_yuv420_sad``, ONE launch on the h2d stream after the
        copies), read back with one event wait and handed to ``det`` in frame order.  Call under the h2d stream.
        Frame j-1 is resident: it was uploaded in this batch or in the previous one (windows are consecutive), and a slot is
        reused only after all nslot >= 2 * batch + 8 slots have been.  The wait does not wait on the compute stream: the
        ``slot_busy`` waits queued on h2d before this batch's copies are on the compute of the batch that last read a reused
        slot, and that batch is at least two back (batch b-1 reads frames k .. k + batch + 2 of its first window k, batch b
        uploads frames up to k + 2 * batch + 2 only), so the host already waited for it when it drained that batch's D2H."""
        cl = self._clip
        P = cl['yuv_in'].shape[1]
        js = sorted(j for j in new_frames if j >= det.next)
        if not js:
            return
        if any(j - 1 not in slot_of for j in js):
            raise RuntimeError('scene cuts: the predecessor of frame %d is not resident' % min(j for j in js if j - 1 not in slot_of))
        m = len(js)
        offs = [slot_of[j - 1] * P for j in js] + [slot_of[j] * P for j in js]
        od = cl['sad_offs'][:2 * m]
        od.copy_(torch.tensor(offs, dtype=torch.int64).pin_memory(), non_blocking=True)
        L.check(self.lib.demfi_yuv420_sad(cl['yuv_in'].data_ptr(), od.data_ptr(), od[m:].data_ptr(), m, P, cl['sad'].data_ptr(),
                                          cl['h2d'].cuda_stream), 'yuv420_sad')
        cl['h_sad'][:m].copy_(cl['sad'][:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cl['h2d'])
        ev.synchronize()
        for j, sad in zip(js, cl['h_sad'][:m].tolist()):
            det.push(j, sad)

    def __del__(self):
        try:
            self._destroy_graphs()
        except Exception:
            pass
