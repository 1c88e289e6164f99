"""Every launch of the real plans on the GPU, one at a time, against float64, inside poisoned memory (tests/plan_replay.py).

The plan is the one ``Engine`` builds: the hoisted partial convolutions, the packed records of CFR and the warp, rd64 as two halves of
one buffer, batch-2 trunk layers, batch-stride-0 pieces of the batched per-t plan, resblock / gru_r / gru_zq at the planner's own
descriptors.  Before each launch the device workspace gets the reference image -- the inputs a correct plan would have stored -- with
every byte the op must not read overwritten by NaNs; after it, every byte outside the op's write set must be what it was, and every
element inside it must lie within the bound tests/epilogue_ref.py / tests/motion_ref.py derive for it.  No tolerance here was tuned on
GPU output, no element is exempt, and no op is skipped: the count of replayed ops is asserted.

40x72: 30-column resblock strips, 16-row steps, a ragged last strip and last step at full, half, quarter and eighth resolution.
32x64: the aligned case.  A few hundred launches over a workspace of a few MB per test.

Out of scope: the visualisation extras (DEMFI_HP_EXTRAS, op kind 13) and the generalised FGAC (fgac_rr > 0: op kinds 8 and 9 in the
plan); the float64 interpreter refuses them.

Run with -s for the table per op kind and dtype (profiles/plan_replay.md records one)."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd.engine import Engine, SEG_TRUNK, SEG_HEAD, SEG_ITER, SEG_TB_HEAD, SEG_TB_ITER   # noqa: E402
from demfi_amd.weights import synthetic_state_dict, synthetic_window                          # noqa: E402
from tests.plan_replay import Replay                                                          # noqa: E402

DEV = 'cuda:0'


def plan_ops(eng, n, batched):
    head, it = (SEG_TB_HEAD, SEG_TB_ITER) if batched else (SEG_HEAD, SEG_ITER)
    return eng.ops(SEG_TRUNK) + eng.ops(head) + [op for i in range(n) for op in eng.ops(it, i)]


class DeviceExecutor:
    """run(op, image) -> image on the device twin: the span of the image (without cfr_acc: the device keeps its own) is copied into the
    twin's workspace, ``Engine.run_op`` launches the twin's op at the same position of the plan, the span is copied back.  Weights, zero
    page and descriptor table are the twin's own and never overwritten; they are compared with their first state at the end."""

    def __init__(self, eng, ops, rp):
        self.eng, self.ops, self.rp = eng, ops, rp
        self.calls = 0
        self.ws = eng.workspace[eng._ws_off:eng._ws_off + rp.nbytes]
        assert eng.workspace.numel() - 256 == rp.nbytes
        self.front = self.ws[:rp.span_lo].cpu()
        self.stream = torch.cuda.current_stream(eng.device)

    def __call__(self, op, image):
        twin = self.ops[self.rp.index]
        self.calls += 1
        assert twin.name == op.name and twin.kind == op.kind and twin.conv == op.conv and twin.nch == op.nch
        for a, b in ((twin.o.ptr, op.o.ptr), (twin.a.ptr, op.a.ptr), (twin.p[0], op.p[0]), (twin.t, op.t)):
            assert (a or self.eng._base) - self.eng._base == (b or self.rp.ref._base) - self.rp.ref._base, 'the two engines lay the workspace out differently'
        src = torch.from_numpy(image)
        for lo, hi in self.rp.upload_ranges():
            self.ws[lo:hi].copy_(src[lo:hi])
        self.eng.run_op(twin, self.stream.cuda_stream)
        self.stream.synchronize()
        s0 = self.rp.span_lo
        src[s0:] = self.ws[s0:].cpu()
        return image

    def front_untouched(self):
        return torch.equal(self.ws[:self.rp.span_lo].cpu(), self.front)


def _table(rp, wall):
    rows = ['%-9s %-5s %8.4f  %s' % (k, dt, r, name) for (k, dt), (r, name) in sorted(rp.worst.items())]
    wid = ['%-48s %6.2f' % (n, float(np.mean(v))) for n, v in rp.widening.items()]
    cond = ['%-48s acc %.3g  inputs x %g' % c for c in rp.cond]
    return '\n'.join(['largest |got - ref| / bound per op kind and stored type:'] + rows + ['resblock widening / unwidened bound (mean):'] + wid
                     + ['ops whose inputs were scaled to keep the accumulation term below 2^-12:'] + cond + ['%d ops replayed, wall %.1f s' % (rp.n_ops, wall)])


CASES = [('fp16-40x72', torch.float16, 40, 72, 2, 1, False, None), ('fp16-32x64', torch.float16, 32, 64, 2, 1, False, None),
         ('fp16-40x72-batched', torch.float16, 40, 72, 2, 2, True, None), ('fp32-40x72', torch.float32, 40, 72, 1, 1, False, None),
         ('fp16-40x72-flow_gain', torch.float16, 40, 72, 2, 1, False, 0.3)]


@pytest.mark.parametrize('case,dtype,H,W,N,n_ctx,batched,flow_gain', CASES, ids=[c[0] for c in CASES])
def test_every_launch_of_the_plan_against_fp64_inside_poison(case, dtype, H, W, N, n_ctx, batched, flow_gain):
    t0 = time.time()
    sd = synthetic_state_dict(0) if flow_gain is None else synthetic_state_dict(0, flow_gain=flow_gain)
    ref = Engine(sd, H, W, dtype, 'cpu', max_updates=N, n_ctx=n_ctx)
    dev = Engine(sd, H, W, dtype, DEV, max_updates=N, n_ctx=n_ctx)
    ts = (0.375,) if n_ctx == 1 else (0.25, 0.75)
    x = synthetic_window(H, W, 4)[0]
    for eng in (ref, dev):                                  # x, t / t_col are inputs: both engines get them
        eng.x.copy_(x)
        for c, t in enumerate(ts):
            eng._ctxs[0][c]['t_dev'].fill_(t)
    ops = plan_ops(ref, N, batched)
    rp = Replay(ref, None)
    ex = DeviceExecutor(dev, plan_ops(dev, N, batched), rp)
    rp.run = ex
    try:
        rp.replay(ops)
    finally:
        print('\n%s\n%s' % (case, _table(rp, time.time() - t0)))
    assert ex.front_untouched(), 'weights, zero page or descriptor table changed on the device'
    want = len(ops) if batched else sum(ref.n_launches(N))
    assert rp.n_ops == ex.calls == len(ops) == want
    assert all(r <= 1.0 for r, _ in rp.worst.values())
