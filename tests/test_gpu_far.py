"""Every convolution family and motion entry point at far addresses, on a real MI355X: 4 GiB crossings, 4 GiB batch strides, wide row and record strides.

tests/test_gpu_guarded.py varies what lies around a frame, never WHERE the frame lies or how far apart its rows are; every block of it
sits in a few MB.  The hot kernels address with a uniform base plus one 32-bit lane offset, which is right only as far as the
eligibility functions bound the strides.  Here the bodies of tests/test_gpu_kernels.py run on ``FarPlan`` (tests/far_memory.py): one
slab of a little over 10 GiB, in which ONE operand at a time

  (a) straddles a 2^32-aligned address in the middle of a middle row (every source, destination, residual, the zero page, the weights);
  (b) has its images 2^32 + 4096 bytes apart (every batched operand of every family, at batch 2; the planes of a planar operand go
      ceil((2^32 + 4096) / n) apart for images of n planes, so its images at least that);
  (c) has a row stride or a record stride such that the largest lane offset of one tile lies below 2^31, in [2^31, 2^32), or at or above
      2^32 (``far_memory.PITCH_FAMILIES``: every family that demfi_conv2d dispatches, the fused residual block and GRU half-step; planar
      operands with a wide row stride and a wide PLANE stride, the packed copy's record as an operand of its own).

The motion, gather, frame-I/O, visualisation and metric entry points of tests/test_gpu_guarded_motion.py run on ``FarArena`` in the same
slab: every argument across the boundary in turn (a), and every batched argument -- images, per-context copies, per-item flat buffers, the
strided pred / gt of demfi_eval_frame -- with its items 2^32 + 4096 bytes apart (b).

Every launch asserts, in this order: the guard check (outside the frames the whole slab is still poison, every other frame is
unchanged), no NaN / inf in what was written, the body's own fp64 comparison at its own tolerance, and -- whenever the launch has the owner
it has on contiguous memory -- bit-identity with the contiguous run of the same seed.  In (c) the contract is gate-agnostic: whatever owner
demfi_conv_owner names at that stride must be right; a refusal (error status, nothing launched, slab untouched) is acceptable too.

With DEMFI_FAR_REPORT=<path> every run appends one JSON line (family, placement, operand, stride, owners, outcome): the source of
profiles/far_addresses.md.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import _lib as L                      # noqa: E402
from demfi_amd.engine import Plan                    # noqa: E402
from tests import far_memory as FM                   # noqa: E402
from tests import guarded_arena as GA                # noqa: E402
from tests import test_gpu_guarded_motion as GM      # noqa: E402
from tests import test_gpu_kernels as K              # noqa: E402
from tests.guarded_plan import GuardError, Record    # noqa: E402

F16, F32 = torch.float16, torch.float32
SPACE = FM.Space()


@pytest.fixture(scope='module')
def slab():
    """ONE allocation for every case of this module; FarPlan poisons it per case (a fill of 10 GiB takes milliseconds)."""
    s = torch.empty(SPACE.slab_bytes, dtype=torch.uint8, device=K.DEV)
    yield s
    del s
    torch.cuda.empty_cache()


# name -> (body, args, keywords): one shape per family, the smallest of tests/test_gpu_guarded.py with a ragged edge and an interior tile
FAMILIES = {
    'general_f32': (K._conv_vs_torch, ((48, 96, 5, 5, 1, 13, 45, L.ACT_NONE, False), F32), dict(batch=2)),
    'general_f16': (K._conv_vs_torch, ((48, 96, 5, 5, 1, 13, 45, L.ACT_NONE, False), F16), dict(batch=2)),
    'general_1x1_res_f32': (K._conv_vs_torch, ((224, 96, 1, 1, 1, 8, 40, L.ACT_NONE, True), F32), {}),
    'c64_nco2': (K._conv_vs_torch, ((64, 64, 3, 3, 1, 37, 75, L.ACT_RELU, True), F16), dict(batch=2)),
    'c64_nco1': (K._conv_vs_torch, ((64, 32, 3, 3, 1, 37, 75, L.ACT_NONE, False), F16), dict(batch=2)),
    'c64_interior': (K._conv_vs_torch, ((64, 64, 3, 3, 1, 16, 64, L.ACT_RELU, True), F16), {}),
    'narrow_nhwc': (K._narrow_persistent_conv, (K.NARROW_CASES[1], 37, 75, 2), {}),
    'narrow_two_pieces': (K._narrow_persistent_conv, (K.NARROW_CASES[2], 37, 75, 2), {}),
    'narrow_7x7': (K._narrow_persistent_conv_7x7, (37, 75), {}),
    'narrow_thin': (K._narrow_thin_outputs, (K.THIN_CASES[0], 37, 75), {}),
    'narrow_thin_batch3': (K._narrow_thin_outputs, (K.THIN_CASES[1], 37, 75), {}),
    'narrow_thin_batch2': (K._narrow_thin_outputs, ((64, [(3, False)], L.ACT_NONE, 2), 37, 75), {}),      # THIN_CASES[1] at batch 2: (b)
    'thin_packed_copy': (K._thin_outputs_with_packed_copy, ([(4, True), (1, True)], [0, 4], 37, 75, 2), {}),
    'sep_1x5': (K._sep_gru_persistent, (1, 5, 37, 75, 2), {}),
    'sep_5x1': (K._sep_gru_persistent, (5, 1, 37, 75, 2), {}),
    'gru_1x5': (K._gru_half_step, (1, 5, 37, 75, 2), {}),
    'gru_5x1': (K._gru_half_step, (5, 1, 37, 75, 2), {}),
    'wstream7': (K._streamed_weight_conv_7x7, (16, 32, 2, L.ACT_TANH), {}),
    'rdb_growth': (K._rdb_growth_conv, (37, 75, 2), {}),
    'ws2_stride2': (K._stride2_4x4_conv, (K.WS2_S2_CASES[0], 23, 40, 2), {}),
    'ws2_units': (K._conv3x3_over_units, (K.WS2_S1_CASES[4], 38, 76, 2), {}),
    'ws2_units_upsampled': (K._conv3x3_over_units, (K.WS2_S1_CASES[0], 38, 76, 2), {}),
    'ws2_two_piece_tail': (K._conv3x3_two_piece_tail, (37, 75, 2), {}),
    'fused_resblock': (K._fused_resblock, ((37, 75, 2),), {}),
    'routing_f32': (K._conv_multi_piece_routing, (F32,), {}),
    'routing_f16': (K._conv_multi_piece_routing, (F16,), {}),
}

# the pitch cases: the body at the frame far_memory.PITCH_FAMILIES gives it, batch 1
PITCH = {
    'c64_nco2': lambda H, W: (K._conv_vs_torch, ((64, 64, 3, 3, 1, H, W, L.ACT_RELU, True), F16), {}),
    'c64_nco1': lambda H, W: (K._conv_vs_torch, ((64, 32, 3, 3, 1, H, W, L.ACT_NONE, True), F16), {}),
    'general_f32': lambda H, W: (K._conv_vs_torch, ((48, 96, 5, 5, 1, H, W, L.ACT_NONE, True), F32), {}),
    'narrow_nhwc': lambda H, W: (K._narrow_persistent_conv, (K.NARROW_CASES[1], H, W, 1), {}),
    'sep_1x5': lambda H, W: (K._sep_gru_persistent, (1, 5, H, W, 1), {}),
    'sep_5x1': lambda H, W: (K._sep_gru_persistent, (5, 1, H, W, 1), {}),
    'wstream7': lambda H, W: (K._streamed_weight_conv_7x7, (H, W, 1, L.ACT_NONE), {}),
    'ws2_units': lambda H, W: (K._conv3x3_over_units, (K.WS2_S1_CASES[4], H, W, 1), {}),
    'fused_resblock': lambda H, W: (K._fused_resblock, ((H, W, 1),), {}),
    'gru_1x5': lambda H, W: (K._gru_half_step, (1, 5, H, W, 1), {}),
    'gru_5x1': lambda H, W: (K._gru_half_step, (5, 1, H, W, 1), {}),
    'narrow_thin': lambda H, W: (K._narrow_thin_outputs, (K.THIN_CASES[0], H, W), {}),
    'thin_packed_copy': lambda H, W: (K._thin_outputs_with_packed_copy, ([(4, True), (1, True)], [0, 4], H, W, 1), {}),
    'narrow_7x7': lambda H, W: (K._narrow_persistent_conv_7x7, (H, W), {}),
    'rdb_growth': lambda H, W: (K._rdb_growth_conv, (H, W, 2), {}),
    'ws2_stride2': lambda H, W: (K._stride2_4x4_conv, (K.WS2_S2_CASES[0], H, W, 1), {}),
    'ws2_two_piece_tail': lambda H, W: (K._conv3x3_two_piece_tail, (H, W, 1), {}),
    'routing_f32': lambda H, W: (K._conv_multi_piece_routing, (F32,), {}),
    'routing_f16': lambda H, W: (K._conv_multi_piece_routing, (F16,), {}),
}
assert set(PITCH) == set(FM.PITCH_FAMILIES)

_PROBE = {}


def _probe(slab, key, case):
    """Once per case: the launches on a plain Plan (owners and stored bits: the contiguous run of the same seed), and who reads and writes
    which block (from the descriptors of a FarPlan without a far block)."""
    if key not in _PROBE:
        body, args, kw = case
        plain = Record(launch_only=True)
        body(Plan, *args, rec=plain, **kw)
        made = []
        body(FM.plan_factory(slab, made=made), *args, rec=Record(launch_only=True), **kw)
        roles, batched = made[0].operands()
        _PROBE[key] = (plain, roles, batched, {k: (0 if b.fat else b.full[0]) for k, b in enumerate(made[0]._blocks)},
                       {k: b.full for k, b in enumerate(made[0]._blocks)})
    return _PROBE[key][:3]


def _report(**kw):
    path = os.environ.get('DEMFI_FAR_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(kw) + '\n')


def _names(owners):
    return [L.OWNERS[o] if kind == 'conv' else '%s:%d' % (kind, o) for kind, o in owners]


def _run(slab, case, plain, far, refusal_ok=False):
    """The body on a FarPlan with one far operand -> (owner names or 'refused', the plan).  The guard check, the finiteness of what was
    written and the reference comparison are the body's and launch()'s; bit-identity here, when the owners are those of the plain run."""
    body, args, kw = case
    rec, made = Record(), []
    try:
        body(FM.plan_factory(slab, far=far, made=made), *args, rec=rec, **kw)
    except FM.Refused:
        assert refusal_ok, 'the launch was refused'
        return 'refused', made[0]
    pl = made[0]
    assert pl.far_block is not None, 'no block %r' % (far[1],)
    if rec.owners == plain.owners:
        rec.expect = plain
        rec.assert_bit_identical()
    return _names(rec.owners), pl


def _sweep(runs):
    """Run every (label, thunk): all of them, so that one report holds every outcome; then fail with the list of those that failed."""
    failed = []
    for label, thunk in runs:
        try:
            thunk()
        except (AssertionError, GuardError) as e:
            failed.append('%s: %s: %s' % (label, type(e).__name__, str(e)[:300]))
            _report(label=label, outcome='FAILED', error='%s: %s' % (type(e).__name__, str(e)[:300]))
    assert not failed, '\n'.join(failed)


# ---- (a) every operand across a 2^32-aligned address --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_far_crossing(slab, name):
    case = FAMILIES[name]
    plain, roles, batched = _probe(slab, name, case)

    def one(which):
        owners, pl = _run(slab, case, plain, ('cross', which, None))
        pl.assert_crosses()
        assert owners == _names(plain.owners), (owners, _names(plain.owners))          # an address changes no owner
        _report(label='%s cross %s' % (name, which), outcome='ok', owners=owners)

    _sweep([('%s cross %s %s' % (name, w, sorted(roles.get(w, []))), (lambda w=w: one(w))) for w in sorted(roles) + ['zero page', 'weights']])


# ---- (b) images 2^32 + 4096 bytes apart --------------------------------------------------------------------------------------------------------
# narrow_thin_batch3: three images of three planes a batch stride apart are more than the slab; narrow_thin_batch2 is the same layer at batch 2
BATCHED = [n for n in sorted(FAMILIES) if n not in ('general_1x1_res_f32', 'c64_interior', 'narrow_7x7', 'narrow_thin', 'narrow_thin_batch3',
                                                    'rdb_growth', 'routing_f32', 'routing_f16')]


@pytest.mark.parametrize('name', BATCHED)
def test_far_batch_stride(slab, name):
    case = FAMILIES[name]
    plain, roles, batched = _probe(slab, name, case)
    which = [k for k in sorted(roles) if batched[k]]
    assert which, 'no batched operand'
    if name in ('narrow_thin_batch2', 'thin_packed_copy'):
        assert any(batched[k] is not True for k in which), 'no batched planar operand'

    def one(k):
        n = None if batched[k] is True else batched[k]              # a planar block: n planes per image
        owners, pl = _run(slab, case, plain, ('batch', k, n))
        r = pl.far_block.region(pl.slab)
        if n is None:
            assert r[1].data_ptr() - r[0].data_ptr() == (1 << 32) + 4096
        else:                                                       # image 1 = plane n: at least the batch stride behind image 0, and the views say so
            assert r[n].data_ptr() - r[0].data_ptr() >= (1 << 32) + 4096
            sbs = [v.sb * 4 for d in pl._descs for sg in list(d.segs)[:d.n_segs] for v in (sg.dst, sg.res)
                   if v.ptr and r[0].data_ptr() <= v.ptr < r[n].data_ptr()]
            assert sbs and all(b == r[n].data_ptr() - r[0].data_ptr() for b in sbs), sbs
        assert owners == _names(plain.owners), (owners, _names(plain.owners))
        _report(label='%s batch %s' % (name, k), outcome='ok', owners=owners)

    _sweep([('%s batch %d %s' % (name, k, sorted(roles[k])), (lambda k=k: one(k))) for k in which])


# ---- (c) wide row and record strides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', ['sy', 'sx'])
@pytest.mark.parametrize('name', sorted(PITCH))
def test_far_pitch(slab, name, axis):
    H, W = FM.PITCH_FAMILIES[name][axis + '_hw']
    case = PITCH[name](H, W)
    plain, roles, batched = _probe(slab, (name, axis), case)
    assert {'src', 'dst'} <= set().union(*roles.values())
    planar, fulls = _PROBE[(name, axis)][3:5]            # {block: its planes, 0 for an NHWC block}, {block: its frame with guards}

    def one(k, ax, S, kind, cls):
        owners, pl = _run(slab, case, plain, ('pitch', k, (ax, S)), refusal_ok=True)
        _report(label='%s pitch %s' % (name, ax), family=name, axis=ax, operand=k, roles=sorted(roles[k]), stride=S, chosen_for=kind, klass=cls,
                outcome='ok', owners=owners, plain=_names(plain.owners))

    runs = []
    for k in sorted(roles):
        full = fulls[k]                                   # the block's own frame: a 2H x 2W source and an H/2 x W/2 piece fit other strides
        if planar[k]:
            cases = FM.thin_pitch_cases(name, axis, planar[k], full=full)
        else:
            cases = [(axis, S, kind, cls) for S, kind, cls in FM.pitch_cases(name, axis, full=full)]
        for ax, S, kind, cls in cases:
            runs.append(('%s %s block %d %s stride %d (%s %s)' % (name, ax, k, sorted(roles[k]), S, kind, cls),
                         (lambda k=k, ax=ax, S=S, kind=kind, cls=cls: one(k, ax, S, kind, cls))))
    assert len(runs) >= 2 * len(roles), 'fewer than two stride classes per operand'
    _sweep(runs)


# ---- the motion, gather, frame-I/O, visualisation and metric entry points: (a) and (b) on FarArena ----------------------------------------------
# one case each of tests/test_gpu_guarded_motion.py; its body is whatever that test hands to _both()
MOTION = {
    'cfr_batched': (GM.test_cfr, (37, 130, 'edges', None)),
    'cfr_pack16': (GM.test_cfr, (16, 64, 'outward', F16)),
    'cfr_pack32': (GM.test_cfr, (37, 130, 'spikes', F32)),
    'fat_warp_f16': (GM.test_fat_warp, (37, 130, F16, 64, True)),
    'fat_warp_f32': (GM.test_fat_warp, (5, 65, F32, 4, False)),
    'thin_warp_pack16': (GM.test_thin_warp_pack, (37, 130, F16, True)),
    'thin_warp_pack32': (GM.test_thin_warp_pack, (9, 2, F32, False)),
    'thin_warp_nhwc': (GM.test_thin_warp_on_an_nhwc_view_takes_the_element_path, (37, 130)),
    'fgac_gather_gate': (GM.test_fgac_gather_and_gate_blend, (F16,)),
    'fgac_window': (GM.test_fgac_window, (13, 19, 2, F16, 1)),
    'avg_pool_fat': (GM.test_avg_pool_fat, (13, 19, F16, 2)),
    'pack_planes': (GM.test_pack_planes, (8, F16)),
    'frame_io': (GM.test_frame_io, (17, 33, 32, 64)),
    'absmean_map': (GM.test_absmean_map, (F16, 8, True)),
    'minmax_normalize': (GM.test_one_minus_and_minmax_normalize_bit_equal_numpy, (257,)),
    'eval_frame': (GM.test_eval_frame, (17, 33, 0)),
}


def _motion(slab, monkeypatch, name, kind):
    """The test of tests/test_gpu_guarded_motion.py with its _both() replaced: the body on plain tensors (the expectation of the
    bit-identity), on a FarArena without a far block (how many allocations, which of them have several items), then once per far block."""
    fn, args = MOTION[name]
    ran = []

    def both(body, capacity=None):
        plain = GA.Plain(K.DEV, recording=True)
        body(plain)
        probe = FM.FarArena(K.DEV, slab, SPACE)
        body(probe)
        which = range(len(probe._blocks)) if kind == 'cross' else [k for k, c in enumerate(probe.counts) if 2 <= c <= 3]

        def one(k):
            al = FM.FarArena(K.DEV, slab, SPACE, (kind, k))
            body(al)
            al.assert_far()
            GA.assert_bit_identical(al, plain)
            _report(label='%s %s %d' % (name, kind, k), outcome='ok', block=al.far_block.name)

        ran.append(len(which))
        _sweep([('%s %s allocation %d (%s)' % (name, kind, k, probe._blocks[k].name), (lambda k=k: one(k))) for k in which])

    monkeypatch.setattr(GM, '_both', both)
    fn(*args)
    return ran


@pytest.mark.parametrize('name', sorted(MOTION))
def test_far_motion_crossing(slab, monkeypatch, name):
    assert sum(_motion(slab, monkeypatch, name, 'cross')) > 0


@pytest.mark.parametrize('name', sorted(MOTION))
def test_far_motion_batch_stride(slab, monkeypatch, name):
    """Every allocation with two or three images, copies or items, those a batch stride apart: the batched launches get the stride through
    bstride(), demfi_eval_frame through the strides of its pred / gt views."""
    n = sum(_motion(slab, monkeypatch, name, 'batch'))
    assert n > 0 or name in ('fgac_gather_gate', 'fgac_window', 'avg_pool_fat', 'frame_io', 'absmean_map', 'minmax_normalize'), 'nothing batched'
