"""Every convolution kernel family inside poisoned guard bands, on a real MI355X.

The kernels decide for themselves which taps fall outside the frame and which rows and columns of a ragged tile are not stored.  On
``engine.Plan`` an off-by-one there reads zeros from a neighbouring allocation (the padding value) or stores where nobody looks.  Here
the bodies of tests/test_gpu_kernels.py run on ``GuardedPlan`` (tests/guarded_plan.py): every buffer is the interior crop of a block of
0xFF bytes (a NaN in fp16 and fp32) four pixels larger on every side, so the row pitch is not the row length and the image pitch is not
the image; the zero page and the weights sit in the same slab with poison behind them.

Every case asserts, in this order:
  (a) the launch has the same owner (demfi_conv_owner, or the *_eligible answer of a fused launch) on pitched views as on contiguous ones;
  (b) nothing outside the destination frames / channel ranges changed (guards, sources, zero page, weights, scratch buffers);
  (c) no NaN / inf in what was written: no poisoned value was consumed, no output pixel was left unwritten;
  (d) the fp64 comparison of the body, with its tolerance;
  (e) the written regions are bit-identical to the plain-Plan run of the same case and seed (no atomics; the tile walk depends on
      H, W, batch, not on addresses).

Every family runs EMBEDDED (pitched rows, guards around every image): none of the eligibility functions (conv.hip demfi_conv_owner and the
*_eligible functions it calls, resblock.hip demfi_resblock_eligible, gru.hip demfi_gru_r_eligible / demfi_gru_zq_eligible) compares sy with
W * sx or sb with H * sy; they only bound the strides by 32-bit lane offsets.  The shapes are the smallest of tests/test_gpu_kernels.py at
which a family's border logic has every branch live.

The last test is the GPU counterpart of tests/test_host.py::test_workspace_arena_shrinks_the_workspace_and_changes_no_result."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from demfi_amd.engine import Plan                    # noqa: E402
from tests import test_gpu_kernels as K              # noqa: E402
from tests.guarded_plan import GuardedPlan, Record   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWNER = {name: i for i, name in enumerate(L.OWNERS)}


def _guarded(body, *args, owners=None, **kw):
    """The body on a plain Plan (launches only: owners and stored bits), then on a GuardedPlan with (a) - (d), then (e).
    owners: the demfi_conv_owner names the FIRST launch may have on the plain plan -- the family the case is here for."""
    plain = Record(launch_only=True)
    body(Plan, *args, rec=plain, **kw)
    if owners is not None:
        assert plain.owners[0] in [('conv', OWNER[o]) for o in owners], (plain.owners[0], owners)
    assert all(own == 1 for kind, own in plain.owners if kind != 'conv')
    g = Record(expect=plain)
    body(GuardedPlan, *args, rec=g, **kw)
    g.assert_bit_identical()


# ---- the general kernel (and whoever owns the fp16 forms of its shapes) ---------------------------------------------------------------------
GENERAL_CASES = [c for c in K.CONV_CASES if c[5] * c[6] < 2000]          # every CONV_CASE at 16x32, 8x32, 8x40, 9x33, 13x45, 16x64


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('case', GENERAL_CASES)
def test_guarded_conv(case, dtype):
    """fp32: all of them run on the general kernel (48 -> 96 5x5, 64 -> 133 3x3 with a ragged cout block, 64 -> 128 4x4 stride 2 read from a
    2H x 2W block, 224 -> 96 1x1 + residual, ...); fp16: each on the kernel that owns it."""
    _guarded(K._conv_vs_torch, case, dtype, owners=['general'] if dtype == torch.float32 else None)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_guarded_conv_general_batch2(dtype):
    """The guard rows between the two images of a batch: 48 -> 96 5x5 at 13x45 (halo 2, ragged in both directions)."""
    _guarded(K._conv_vs_torch, (48, 96, 5, 5, 1, 13, 45, L.ACT_NONE, False), dtype, batch=2, owners=['general'])


# ---- 3x3 over one 64-channel piece -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,batch', [(13, 45, 1), (37, 75, 2), (16, 64, 1)])       # 16x64: no ragged edge, the `interior` branch
@pytest.mark.parametrize('cout,act,res', [(64, L.ACT_RELU, True), (32, L.ACT_NONE, False)])
def test_guarded_c64(cout, act, res, H, W, batch):
    _guarded(K._conv_vs_torch, (64, cout, 3, 3, 1, H, W, act, res), torch.float16, batch=batch, owners=['c64'])


# ---- the narrow kernel: NHWC and thin epilogues, 7x7, packed copy ------------------------------------------------------------------------------
NARROW_SHAPES = [(8, 32, 1), (37, 75, 2), (19, 130, 1)]


@pytest.mark.parametrize('case', K.NARROW_CASES)
@pytest.mark.parametrize('H,W,batch', NARROW_SHAPES)
def test_guarded_narrow_cases(case, H, W, batch):
    """NARROW_CASES: the narrow kernel's NHWC epilogue; two 32-channel pieces are two units of wsconv.hip, and the 48 + 16 record is not a
    shape of either (the general kernel)."""
    _guarded(K._narrow_persistent_conv, case, H, W, batch, owners=['narrow_nhwc', 'ws2', 'general'])


@pytest.mark.parametrize('H,W', [(8, 32), (37, 75), (19, 130)])
def test_guarded_narrow_7x7(H, W):
    _guarded(K._narrow_persistent_conv_7x7, H, W, owners=['narrow_nhwc'])


@pytest.mark.parametrize('case', K.THIN_CASES)
@pytest.mark.parametrize('H,W', [(8, 32), (37, 75), (19, 130)])
def test_guarded_narrow_thin(case, H, W):
    """Planar fp32 destinations and residuals, each plane inside its own guard frame (the plane pitch is not H * W either)."""
    _guarded(K._narrow_thin_outputs, case, H, W, owners=['narrow_thin'])


@pytest.mark.parametrize('dsts,pack_ch', [([(5, True)], [0]), ([(4, True), (1, True)], [0, 4]), ([(3, False), (5, True)], [-1, 8])])
@pytest.mark.parametrize('H,W,batch', NARROW_SHAPES)
def test_guarded_thin_packed_copy(dsts, pack_ch, H, W, batch):
    """The packed record is written in the channel ranges of the packed octets only: the others keep their poison."""
    _guarded(K._thin_outputs_with_packed_copy, dsts, pack_ch, H, W, batch, owners=['narrow_thin'])


# ---- SepConvGRU: the persistent 1x5 / 5x1 kernel and the fused half-step -----------------------------------------------------------------------
@pytest.mark.parametrize('kh,kw', [(1, 5), (5, 1)])
@pytest.mark.parametrize('H,W,batch', [(37, 75, 2), (33, 8, 3)])
def test_guarded_sep(kh, kw, H, W, batch):
    _guarded(K._sep_gru_persistent, kh, kw, H, W, batch, owners=['sep'])


@pytest.mark.parametrize('kh,kw', [(1, 5), (5, 1)])
@pytest.mark.parametrize('H,W,batch', [(8, 32, 1), (37, 75, 2), (33, 8, 3), (16, 160, 1)])
def test_guarded_gru_r_then_zq(kh, kw, H, W, batch):
    """demfi_gru_r / demfi_gru_zq: the z buffer and the state h are in the untouched set of the fused launches."""
    _guarded(K._gru_half_step, kh, kw, H, W, batch)


# ---- streamed weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,batch,act', [(16, 32, 1, L.ACT_TANH), (37, 75, 2, L.ACT_NONE)])
def test_guarded_wstream7(H, W, batch, act):
    """Three 64-channel slices of ONE guarded 192-channel buffer."""
    _guarded(K._streamed_weight_conv_7x7, H, W, batch, act, owners=['wstream7'])


@pytest.mark.parametrize('q', [0, 2, 3])
@pytest.mark.parametrize('H,W', [(16, 32), (37, 75)])
def test_guarded_rdb_growth_conv(H, W, q):
    """Reads channels [0, 32 q) of the growth buffer and writes [32 q, 32 q + 32) of it: poison in the written range only, and the
    channels in front of and behind it must be bit-identical after the launch."""
    _guarded(K._rdb_growth_conv, H, W, q, owners=['ws2', 'wstream3'])


@pytest.mark.parametrize('case', K.WS2_S2_CASES)
@pytest.mark.parametrize('H,W,batch', [(16, 32, 1), (37, 75, 2), (23, 40, 1)])
def test_guarded_ws2_stride2(case, H, W, batch):
    """The sources are 2H x 2W: their guard blocks are sized from their own height and width."""
    _guarded(K._stride2_4x4_conv, case, H, W, batch, owners=['ws2'])


@pytest.mark.parametrize('case', K.WS2_S1_CASES)
@pytest.mark.parametrize('H,W,batch', [(16, 32, 1), (38, 76, 2)])
def test_guarded_ws2_3x3_units(case, H, W, batch):
    """Pieces read through the x2 upsample are H/2 x W/2 blocks with guards of their own."""
    _guarded(K._conv3x3_over_units, case, H, W, batch, owners=['ws2'])


@pytest.mark.parametrize('H,W,batch', [(16, 32, 1), (37, 75, 2)])
def test_guarded_ws2_two_piece_tail(H, W, batch):
    _guarded(K._conv3x3_two_piece_tail, H, W, batch, owners=['ws2'])


# ---- fused residual block ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(16, 30, 1), (16, 32, 1), (37, 75, 2), (48, 64, 3)])
def test_guarded_fused_resblock(case):
    """The scratch buffer t of the two-launch form is in the untouched set of the fused launch."""
    _guarded(K._fused_resblock, case)


# ---- upsample / PixelShuffle / planar + residual routing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_guarded_multi_piece_routing_upsample_shuffle(dtype):
    _guarded(K._conv_multi_piece_routing, dtype)


# ---- arena on / off --------------------------------------------------------------------------------------------------------------------------------
_ARENA_CHILD = r'''
import hashlib, json, torch
from demfi_amd.engine import Engine
from demfi_amd.weights import synthetic_state_dict, synthetic_window
eng = Engine(synthetic_state_dict(0), 64, 96, torch.float16, 'cuda:0', max_updates=2, n_ctx=2)
x = synthetic_window(64, 96, 4)
st = torch.cuda.current_stream().cuda_stream
digests = []
for rep in range(2):
    eng.x.copy_(x[0].to('cuda:0'))
    eng._tb[0]['t_col'].copy_(torch.tensor([0.25, 0.75], device='cuda:0'))
    eng.run_trunk(st)
    eng.run_tb(st, 2)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for c in range(2):
        for k in ('finals', 'delta', 'occ', 'sharp1'):
            t = eng._ctxs[0][c][k]
            assert torch.isfinite(t).all(), (c, k)
            h.update(t.contiguous().cpu().numpy().tobytes())
    digests.append(h.hexdigest())
print(json.dumps({'digests': digests, 'workspace': int(eng.workspace.numel())}))
'''


def _arena_child(arena):
    env = dict(os.environ)
    env['DEMFI_ARENA'] = arena
    r = subprocess.run([sys.executable, '-c', _ARENA_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_workspace_arena_changes_no_result_on_the_gpu():
    """One fp16 engine at 64x96, two recursions, two per-t contexts (the batched per-t plan), fixed weights and window: with the arena on,
    the neighbour of every buffer and of the zero page is another tenant's live data; with DEMFI_ARENA=0 it is zeros.  The SHA-256 over
    finals / delta / occ / sharp1 of both contexts must not depend on it, nor on the workspace being dirty from a previous forward.  The
    switch is read once per process: one fresh child each, one after the other; a child that fails fails the test before the next starts."""
    on = _arena_child('1')
    assert on['digests'][0] == on['digests'][1]                 # the second forward ran on the dirty workspace
    off = _arena_child('0')
    assert off['digests'][0] == off['digests'][1]
    assert on['workspace'] < off['workspace']                    # the switch did switch
    assert on['digests'][0] == off['digests'][0]
