"""The plan digest (tools/plan_digest.py) is a function of the plan, not of where the workspace lies; and the kernel that owns a
descriptor (demfi_conv_owner) is the one its weights were packed for.  CPU only; no digest value is frozen here: a frozen digest would
fail on every honest change of the plan."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

from demfi_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('plan_digest', os.path.join(ROOT, 'tools', 'plan_digest.py'))
plan_digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_digest)

CONFIGS = {'fp16_nctx3': (torch.float16, 3), 'fp32_nctx1': (torch.float32, 1)}       # the batched fp16 plan; the fp32 plan


@pytest.fixture(scope='module', params=sorted(CONFIGS))
def two_bound(request, synthetic_sd):
    """Two engines of one 32x64 configuration alive at once, hence at different bases."""
    dtype, n_ctx = CONFIGS[request.param]
    return [plan_digest.engine_bound(32, 64, dtype, 2, n_ctx, sd=synthetic_sd) for _ in range(2)]


def test_digest_does_not_depend_on_the_base(two_bound):
    a, b = two_bound
    assert a.base != b.base
    da, db = plan_digest.digest(a), plan_digest.digest(b)
    assert da[1] > 100 and da[2] > 100                                                 # ops and descriptors were hashed
    assert da == db


def test_cout_perm_exactly_for_the_owners_that_want_it(two_bound):
    lib = L.load()
    seen = set()
    for d in two_bound[0].descs():
        owner = lib.demfi_conv_owner(C.byref(d))
        assert 0 <= owner < len(L.OWNERS)
        assert (d.cout_perm != 0) == (owner in L.OWNERS_COUT_PERM), L.OWNERS[owner]
        seen.add(L.OWNERS[owner])
    assert 'general' in seen                                                           # both plans keep layers on the general kernel
