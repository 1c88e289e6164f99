#!/usr/bin/env python3
"""SHA-256 of a bound launch plan: the safety net of refactors of the host code that builds it.  CPU only.

A context is bound to host memory and hashed, in this order: the workspace size (int64), every demfi_op of every segment (trunk; head per
context; iter per context and recursion; batched head; batched iters), every demfi_conv descriptor in index order, the bytes of the weight
region.  Pointers are rebased first: every aligned 8-byte word of an op / descriptor whose value lies inside
[base, base + workspace bytes) becomes its offset with bit 63 set, so two engines at different addresses give one digest.

    python tools/plan_digest.py                       # the small configurations
    python tools/plan_digest.py --big                 # + 736x1280 fp16 N=3 n_ctx=7 (the benchmark plan: ~12 GB of host memory)
    python tools/plan_digest.py --config 64x96:f16:N3:c2:k2
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demfi_amd import _lib as L                                  # noqa: E402
from demfi_amd.engine import SEG_HEAD, SEG_ITER, SEG_TB_HEAD, SEG_TB_ITER, SEG_TRUNK, Engine   # noqa: E402
from demfi_amd.spec import HyperParams                           # noqa: E402
from demfi_amd.weights import synthetic_state_dict               # noqa: E402


def rebased(struct, base, nbytes):
    """The struct's bytes with every aligned 8-byte word that points into the workspace replaced by (offset | 1 << 63)."""
    w = np.frombuffer(bytes(struct), dtype=np.uint64).copy()
    inside = (w >= np.uint64(base)) & (w < np.uint64(base + nbytes))
    w[inside] = (w[inside] - np.uint64(base)) | np.uint64(1 << 63)
    return w.tobytes()


class Bound:
    """What the digest needs of a bound context: the library handle, the workspace and the segment walk."""

    def __init__(self, lib, ctx, workspace, base, nbytes, n_ctx, N, n_trunk=1, owner=None):
        self.lib, self.ctx, self.workspace, self.base, self.nbytes, self.n_ctx, self.N = lib, ctx, workspace, base, nbytes, n_ctx, N
        self.n_trunk, self.owner = n_trunk, owner                # owner: whatever keeps ctx alive (an Engine), None = destroy() frees it

    def destroy(self):
        if self.owner is None and self.ctx:
            self.lib.demfi_ctx_destroy(self.ctx)
        self.ctx = self.owner = None

    def segments(self, trunk):
        yield SEG_TRUNK, 0, 0
        if self.N == 0:                                          # operator context: the trunk segment is the operator
            return
        for c in range(self.n_ctx):
            yield SEG_HEAD, c, 0
        for c in range(self.n_ctx):
            for it in range(self.N):
                yield SEG_ITER, c, it
        if self.n_ctx > 1:
            yield SEG_TB_HEAD, 0, 0
            for it in range(self.N):
                yield SEG_TB_ITER, 0, it

    def ops(self):
        for k in range(self.n_trunk):
            for seg, c, it in self.segments(k):
                n = L.check(self.lib.demfi_ctx_num_ops(self.ctx, seg, k, c, it), 'num_ops')
                for i in range(n):
                    op = L.Op()
                    L.check(self.lib.demfi_ctx_get_op(self.ctx, seg, k, c, it, i, C.byref(op)), 'get_op')
                    yield op

    def descs(self):
        for i in range(self.lib.demfi_ctx_num_convs(self.ctx)):
            yield self.lib.demfi_ctx_conv_desc(self.ctx, i).contents


def digest(b):
    """(sha256 hex, number of ops, number of descriptors) of a Bound context."""
    h = hashlib.sha256()
    h.update(np.int64(b.nbytes).tobytes())
    n_ops = n_descs = 0
    for op in b.ops():
        h.update(rebased(op, b.base, b.nbytes))
        n_ops += 1
    for d in b.descs():
        h.update(rebased(d, b.base, b.nbytes))
        n_descs += 1
    off, nb = C.c_int64(0), C.c_int64(0)
    L.check(b.lib.demfi_ctx_weight_region(b.ctx, C.byref(off), C.byref(nb)))
    lo = b.base - b.workspace.data_ptr() + off.value
    h.update(b.workspace[lo:lo + nb.value].numpy().tobytes())
    return h.hexdigest(), n_ops, n_descs


def bound_engine(eng):
    return Bound(eng.lib, eng._ctx, eng.workspace, eng._base, eng.lib.demfi_ctx_workspace_bytes(eng._ctx), eng.n_ctx, eng.N,
                 eng.n_trunk, owner=eng)


def engine_bound(H, W, dtype, N, n_ctx=1, n_trunk=1, hp=None, sd=None):
    return bound_engine(Engine(sd or synthetic_state_dict(0, hp), H, W, dtype, 'cpu', max_updates=N, hp=hp, n_ctx=n_ctx, n_trunk=n_trunk))


def operator_bound(kind, batch, H, W, dt, sd):
    """A SepConvGRU ('gru') / FGAC ('fgac') operator context through the library, bound to host memory."""
    lib = L.load()
    ctx = C.c_void_p()
    create, prefix = ((lib.demfi_gru_sep_create, 'Booster_Module.GB.') if kind == 'gru'
                      else (lib.demfi_fgac_create, 'FAC_FB_Module.shared_FGAC.'))
    L.check(create(batch, H, W, dt, C.byref(ctx)), kind + '_create')
    for key, val in sd.items():
        if key.startswith(prefix):
            a = np.ascontiguousarray(val.detach().float().numpy())
            if a.ndim == 5:
                a = np.ascontiguousarray(a[:, :, 0])
            shp = (C.c_int64 * a.ndim)(*a.shape)
            L.check(lib.demfi_load_weight(ctx, key[len(prefix):].encode(), a.ctypes.data, shp, a.ndim), 'load_weight ' + key)
    nbytes = lib.demfi_ctx_workspace_bytes(ctx)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    L.check(lib.demfi_ctx_bind(ctx, base, nbytes, 1, 0), 'ctx_bind')
    return Bound(lib, ctx, ws, base, nbytes, 1, 0)


def small_configs():
    """(name, function returning the Bound context) per configuration."""
    f16, f32 = torch.float16, torch.float32
    yield '32x64 fp16 N=2 n_ctx=1', lambda: engine_bound(32, 64, f16, 2)
    yield '32x64 fp32 N=2 n_ctx=1', lambda: engine_bound(32, 64, f32, 2)
    yield '32x64 fp16 N=2 n_ctx=3', lambda: engine_bound(32, 64, f16, 2, 3)
    yield '32x64 fp32 N=2 n_ctx=3', lambda: engine_bound(32, 64, f32, 2, 3)
    yield '64x96 fp16 N=3 n_ctx=2 n_trunk=2', lambda: engine_bound(64, 96, f16, 3, 2, 2)
    yield '32x64 fp16 N=2 non-shared FGAC', lambda: engine_bound(32, 64, f16, 2, hp=HyperParams(shared_FGAC_flag=False))
    for rr, sr, fmap in ((1, 0, 0), (2, 2, 1)):
        yield ('32x64 fp16 N=2 FGAC rr=%d sr=%d map=%d' % (rr, sr, fmap),
               lambda rr=rr, sr=sr, fmap=fmap: engine_bound(32, 64, f16, 2, hp=HyperParams(fgac_rr=rr, fgac_sr=sr, fgac_map=fmap)))
    yield '32x64 fp16 N=2 extras', lambda: engine_bound(32, 64, f16, 2, hp=HyperParams(visualization_flag=True))
    sd = synthetic_state_dict(0)
    for kind in ('gru', 'fgac'):
        for name, dt in (('fp16', L.F16), ('fp32', L.F32)):
            yield '%s operator batch 2 16x32 %s' % (kind, name), lambda kind=kind, dt=dt: operator_bound(kind, 2, 16, 32, dt, sd)


def big_configs(more):
    yield '736x1280 fp16 N=3 n_ctx=7', lambda: engine_bound(736, 1280, torch.float16, 3, 7)
    if more:
        yield '736x1280 fp32 N=5 n_ctx=1', lambda: engine_bound(736, 1280, torch.float32, 5)
        yield '1088x1920 fp16 N=3 n_ctx=1', lambda: engine_bound(1088, 1920, torch.float16, 3)


def parse_config(s):
    """'HxW:f16|f32:N<n>[:c<n_ctx>][:k<n_trunk>]'"""
    parts = s.split(':')
    H, W = (int(v) for v in parts[0].split('x'))
    dtype = {'f16': torch.float16, 'f32': torch.float32}[parts[1]]
    kw = {'N': 1, 'c': 1, 'k': 1}
    for p in parts[2:]:
        kw[p[0]] = int(p[1:])
    return lambda: engine_bound(H, W, dtype, kw['N'], kw['c'], kw['k'])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--big', action='store_true', help='also the benchmark plan (736x1280 fp16 N=3 n_ctx=7)')
    ap.add_argument('--more', action='store_true', help='with --big: also 736x1280 fp32 N=5 and 1088x1920 fp16')
    ap.add_argument('--config', action='append', help='only these: HxW:f16|f32:N<n>[:c<n_ctx>][:k<n_trunk>]')
    a = ap.parse_args()
    if a.config:
        todo = [(s, parse_config(s)) for s in a.config]
    else:
        todo = list(small_configs()) + (list(big_configs(a.more)) if a.big else [])
    for name, fn in todo:
        b = fn()
        hexd, n_ops, n_descs = digest(b)
        b.destroy()
        print('%s  %4d ops %4d descs  %s' % (hexd, n_ops, n_descs, name), flush=True)


if __name__ == '__main__':
    main()
