"""The cached clip pipeline of ``WindowRunner.run_clip_u8`` on a real MI355X: it is keyed by (batch, ``EdgeSpec``), so a run whose
spec differs rebuilds it, a run whose spec is the same reuses it, and neither changes a byte of the output."""
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict, synthetic_window   # noqa: E402
from demfi_amd import y4m                                                            # noqa: E402
from demfi_amd.pipeline import EdgeSpec                                              # noqa: E402
from demfi_amd.runner import WindowRunner                                            # noqa: E402
from demfi_amd.video import YuvEdge                                                  # noqa: E402

DEV = 'cuda:0'
H, W, N, CUT = 48, 80, 6, 3


def _payloads():
    """Six 4:2:0 payloads of a moving pattern; frames CUT .. are another scene (the pattern inverted and darkened)."""
    base = synthetic_window(H + 2 * N, W + 2 * N, 5)[0, :, 0]
    out = []
    for i in range(N):
        bgr = ((base[:, i:i + H, 2 * i:2 * i + W].permute(1, 2, 0).numpy() + 1) * 127.5).clip(0, 255).astype(np.uint8)
        if i >= CUT:
            bgr = (255 - bgr) // 3
        out.append(torch.from_numpy(y4m.bgr_to_yuv420_np(bgr, 'bt601', False)).pin_memory())
    return out


def _run(rn, pays, yuv):
    got = {}
    wins = [(k + 1, k + 2, k, k + 3) for k in range(N - 3)]
    assert rn.run_clip_u8(pays, wins, lambda k, p: got.__setitem__(k, p.clone()), batch=2, yuv=yuv) == N - 3
    return torch.cat([got[k] for k in range(N - 3)])


def test_the_pipeline_is_rebuilt_for_another_spec_and_reused_for_the_same():
    model = DeMFInet(HyperParams(), dtype=torch.float16)
    model.load_state_dict(synthetic_state_dict(0))
    model = model.to(DEV).eval()
    pays = _payloads()

    def edge(**kw):                                                       # a new object every time: the key is its content
        return YuvEdge('bt601', False, '420jpeg', lambda k: k == N - 4, **kw)
    rn = WindowRunner(model, H, W, n_tst=1, mfi=2, retime=Fraction(2))
    first = _run(rn, pays, edge())
    p_a = rn._pipeline
    assert p_a.key == (2, EdgeSpec(y4m=True)) and first.shape == (2 * (N - 3) + 1, y4m.payload_size(H, W))
    with_cuts = _run(rn, pays, edge(scene_cut=10.0))
    p_b = rn._pipeline
    assert p_b is not p_a and p_b.key == (2, EdgeSpec(y4m=True, cuts=True)) and p_b.key != p_a.key
    assert rn.last_cuts == [CUT] and rn.cut_windows == 1 and not torch.equal(with_cuts, first)        # B is another computation
    third = _run(rn, pays, edge())
    p_c = rn._pipeline
    assert p_c is not p_b and p_c is not p_a and p_c.key == p_a.key
    assert torch.equal(third, first)
    fourth = _run(rn, pays, edge())
    assert rn._pipeline is p_c and torch.equal(fourth, first)
    fresh = WindowRunner(model, H, W, n_tst=1, mfi=2, retime=Fraction(2))
    assert torch.equal(_run(fresh, pays, edge(scene_cut=10.0)), with_cuts) and fresh._pipeline.key == p_b.key
