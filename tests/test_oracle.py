"""The oracle restatement against the fixtures frozen from the upstream reference (tools/make_goldens.py)."""
import os

import numpy as np
import pytest
import torch

from demfi_amd.weights import synthetic_window
from oracle import demfi_oracle as O

E2E = ['e2e_64x96_t0500_n3', 'e2e_64x96_t0125_n1', 'e2e_64x96_t0875_n2', 'e2e_32x64_t0375_n5']


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


@pytest.fixture(autouse=True)
def _fixture_thread_count():
    """oneDNN's CPU convolutions sum in an order that depends on the thread count; the fixtures are checked at 8 threads, whatever
    the host has (at 16 or more on a 64-core EPYC the FGAC extras drift past their 5e-6 tolerance)."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def test_e2e_matches_reference_goldens(golden_dir, synthetic_sd):
    for name in E2E:
        g = _load(golden_dir, name)
        x = synthetic_window(int(g['H']), int(g['W']), int(g['seed']))
        with torch.no_grad():
            d1, fin, flows, occs, ov = O.forward(synthetic_sd, x, torch.tensor([[float(g['t'])]]), int(g['N']))
        tol = 5e-5
        for i in range(3):
            assert np.abs(d1[i][0].numpy() - g['d1'][i]).max() < tol
        for it in range(int(g['N'])):
            for i in range(3):
                assert np.abs(fin[it][i][0].numpy() - g['finals'][it, i]).max() < tol
                # acceptance metric of the north star: |dPSNR| <= 1e-3 dB against a fixed pseudo ground truth
                gt = x[0, :, 0].numpy()
                assert abs(O.psnr(fin[it][i][0].numpy(), gt) - O.psnr(g['finals'][it, i], gt)) <= 1e-3
        for i in range(int(g['N']) + 1):
            assert np.abs(flows[i][0].numpy() - g['flows'][i]).max() < tol
            assert np.abs(occs[i][0].numpy() - g['occs'][i]).max() < tol
        assert np.array_equal(ov[0].numpy(), g['overlay'])


def test_harness_pad_forward_crop(golden_dir, synthetic_sd):
    g = _load(golden_dir, 'harness_50x70_t0625_n1')
    x = synthetic_window(50, 70, 5)
    with torch.no_grad():
        d1, fin, flows, occs, ov = O.pad_forward_crop(synthetic_sd, x, torch.tensor([[0.625]]), 1)
    assert fin[0][2].shape[-2:] == (50, 70)
    for i in range(3):
        assert np.abs(fin[0][i][0].numpy() - g['finals'][0, i]).max() < 5e-5
    assert np.abs(flows[1][0].numpy() - g['flows'][1]).max() < 5e-5


FAMS = ['zeros', 'ints', 'halves', 'smooth', 'large', 'edges', 'collide']


def test_backward_warp_and_maps(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    img3 = torch.from_numpy(g['img3'])[None]
    img8 = torch.from_numpy(g['img8'])[None]
    for f in FAMS:
        flo = torch.from_numpy(g['flo_' + f])[None]
        assert np.abs(O.backward_warp(img3, flo)[0].numpy() - g['bwarp3_' + f]).max() < 1e-6
        assert np.abs(O.backward_warp_explicit(img3, flo)[0].numpy() - g['bwarp3_' + f]).max() < 1e-6
        assert np.abs(O.backward_warp_explicit(img8, flo)[0].numpy() - g['bwarp8_' + f]).max() < 1e-6
        # the validity map of the step-by-step fp32 emulation == where the reference output is non-zero
        m = O.backward_warp_maps(g['flo_' + f])
        ref_nonzero = np.abs(g['bwarp8_' + f]).max(0) > 0
        assert not (ref_nonzero & ~m['valid']).any()


def test_forward_splat_bit_exact(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    for f in FAMS:
        flo = torch.from_numpy(g['flo_' + f])[None]
        iw, io = O.forward_splat(flo, 0.375 * flo)
        assert np.array_equal(iw[0].numpy(), g['fwarp_img_' + f])
        assert np.array_equal(io[0].numpy(), g['fwarp_one_' + f])


def test_cfr_bit_exact(golden_dir):
    g = _load(golden_dir, 'warps_24x40')
    for i in range(4):
        t = torch.tensor(float(g['cfr%d_t' % i])).view(1, 1, 1, 1)
        a, b = O.cfr_flow_align(torch.from_numpy(g['cfr%d_f01' % i])[None], torch.from_numpy(g['cfr%d_f10' % i])[None], t)
        assert np.array_equal(a[0].numpy(), g['cfr%d_ft0' % i])
        assert np.array_equal(b[0].numpy(), g['cfr%d_ft1' % i])


def test_fgac_and_space_to_depth(golden_dir, synthetic_sd):
    g = _load(golden_dir, 'fgac_16x24')
    ref = torch.from_numpy(g['ref'])[None]
    src = torch.from_numpy(g['src'])[None]
    for name in ('inrange', 'mixed', 'beyond'):
        fl = torch.from_numpy(g['flow_' + name])[None]
        with torch.no_grad():
            out, w = O.fgac(synthetic_sd, 'FAC_FB_Module.shared_FGAC', ref, src, fl)
        assert np.abs(out[0].numpy() - g['out_' + name]).max() < 1e-6
        assert np.abs(w[0].numpy() - g['gate_' + name]).max() < 1e-6
        # explicit-gather twin == grid_sample path
        rk = O.conv(synthetic_sd, 'FAC_FB_Module.shared_FGAC.conv_ref_k', ref)
        assert (O.fgac_sample_explicit(rk, fl)[0] - O.fgac_sample(rk, fl)).abs().max() < 1e-5
    assert np.array_equal(O.space_to_depth(torch.from_numpy(g['s2d_in'])[None], 2)[0].numpy(), g['s2d_out'])


def test_fgac_ignores_conv_source_k(synthetic_sd):
    """conv_source_k has no effect on the output (softmax over a singleton)."""
    sd = dict(synthetic_sd)
    x = synthetic_window(32, 32, 9)
    with torch.no_grad():
        a = O.forward(sd, x, torch.tensor([[0.5]]), 1)
        sd['FAC_FB_Module.shared_FGAC.conv_source_k.weight'] = sd['FAC_FB_Module.shared_FGAC.conv_source_k.weight'] * 100
        b = O.forward(sd, x, torch.tensor([[0.5]]), 1)
    assert torch.equal(a[1][0][2], b[1][0][2])


def test_config1_fixture_256(golden_dir, synthetic_sd):
    """BASELINE.json configs[0]: N_tst=1, x2 (t=0.5), 256x256, CPU fp32 -- the reference's own CPU-runnable case."""
    g = _load(golden_dir, 'cfg1_256x256_t0500_n1')
    x = synthetic_window(int(g['H']), int(g['W']), int(g['seed']))
    with torch.no_grad():
        d1, fin, flows, occs, ov = O.forward(synthetic_sd, x, torch.tensor([[float(g['t'])]]), int(g['N']))
    assert (fin[0][2][0].numpy() - g['St']).__abs__().max() < 5e-5
    assert np.abs(flows[-1][0].numpy() - g['flows_last']).max() < 5e-4
    assert np.abs(occs[-1][0].numpy() - g['occ_last']).max() < 5e-5
    gt = x[0, :, 0].numpy()
    p_or = O.psnr(fin[0][2][0].numpy(), gt)
    assert abs(p_or - float(g['psnr_St_vs_B0'])) <= 1e-3                       # the north-star tolerance
    for i in range(3):                                                          # rounded 8-bit frames: off by <= 1 level, rarely
        d = np.abs(np.around(O.denorm255(fin[0][i][0].numpy())).astype(np.int32) - g['finals_u8'][i].astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3


def test_uint8_loader_and_writer_fixture(golden_dir):
    """RGBframes_np2Tensor (utils.py:224-238) and the writer's denorm255_np + astype(uint8) truncation
    (utils.py:718-721, main.py:1165-1178): oracle helpers bit-identical to the frozen reference outputs."""
    g = _load(golden_dir, 'u8io_20x28')
    assert np.array_equal(O.frames_u8_to_tensor(list(g['frames'])).numpy(), g['tensor'])
    assert np.array_equal(O.frame_to_u8(g['pred']), g['out_u8'])


def test_psnr_ssim_fixture(golden_dir):
    """psnr (utils.py:652-660) and ssim / ssim_matlab_func (utils.py:663-705) against values computed by the reference
    code (cv2.getGaussianKernel / filter2D stubbed with their documented formulas, tools/make_goldens.py)."""
    g = _load(golden_dir, 'metrics_96x128')
    ia = np.around(O.denorm255(np.transpose(g['a'].astype(np.float64), [1, 2, 0])))
    ib = np.around(O.denorm255(np.transpose(g['b'].astype(np.float64), [1, 2, 0])))
    assert abs(O.psnr255(ia, ib) - float(g['psnr'])) < 1e-9
    assert abs(O.ssim_matlab(ia, ib) - float(g['ssim'])) < 1e-9
    assert O.psnr255(ia, ia) == float('inf') and abs(O.ssim_matlab(ia, ia) - 1.0) < 1e-12
    p, s = O.eval_frame(g['a'], g['b'], round_gt=True)
    assert abs(p - float(g['psnr'])) < 1e-9 and abs(s - float(g['ssim'])) < 1e-9


def test_generalised_fgac_matches_patched_reference(golden_dir, synthetic_sd):
    """FGAC with radii rr, sr > 0 (DeMFInet.py:401-445): the reference never executes it (its radii are function-local
    constants 0), so the pin is a PATCHED in-memory copy of the reference function (tools/make_goldens.py::patched_fgac) --
    parity pinned to a patched reference, said so here and in DESIGN.md."""
    g = _load(golden_dir, 'fgac_window_16x24')
    ref, src = torch.from_numpy(g['ref'])[None], torch.from_numpy(g['src'])[None]
    for rr, sr in ((1, 0), (2, 0), (1, 1)):
        for name in ('inrange', 'mixed'):
            fl = torch.from_numpy(g['flow_' + name])[None]
            with torch.no_grad():
                out, w, fac, att = O.fgac_general(synthetic_sd, 'FAC_FB_Module.shared_FGAC', ref, src, fl, rr, sr, 0)
            tag = 'rr%d_sr%d_%s' % (rr, sr, name)
            assert np.abs(fac[0].numpy() - g['fac_' + tag]).max() < 5e-6, tag
            assert np.abs(out[0].numpy() - g['out_' + tag]).max() < 5e-6, tag
            assert np.abs(w[0].numpy() - g['gate_' + tag]).max() < 5e-6, tag
            assert abs(float(att.sum(0).mean()) - 1.0) < 1e-6
    # rr = 0 collapses to the point-wise form whatever the mode (softmax over one element)
    fl = torch.from_numpy(g['flow_mixed'])[None]
    with torch.no_grad():
        rk = O.conv(synthetic_sd, 'FAC_FB_Module.shared_FGAC.conv_ref_k', ref)
        sk = O.conv(synthetic_sd, 'FAC_FB_Module.shared_FGAC.conv_source_k', src)
    for mode in (0, 1):
        fac0, att0 = O.fgac_window(rk, sk, fl, 0, 0, mode)
        assert torch.equal(att0, torch.ones_like(att0))
        assert (fac0 - O.fgac_sample_explicit(rk, fl)[0]).abs().max() < 1e-6


def test_extras_of_the_visualisation_and_training_tuples(golden_dir, synthetic_sd):
    """Round 6: FGAC's extra returns (DeMFInet.py:454-496) and DeMFInet.forward's longer tuples (167-176), fixture from the UNPATCHED
    reference with args.visualization_flag = True / is_training = True."""
    g = _load(golden_dir, 'extras_64x96_t0500_n1')
    x = synthetic_window(int(g['H']), int(g['W']), int(g['seed']))
    with torch.no_grad():
        bw, diffs = O.forward_extras(synthetic_sd, x)
    assert len(bw) == 5 and len(diffs) == 4
    for b in range(2):
        for k in range(6):
            assert np.abs(bw[b][k][0, 0].numpy() - g['bw'][b, k]).max() < 5e-6, (b, k)
        assert np.abs(diffs[b][0, 0].numpy() - g['diff'][b]).max() < 5e-6
        assert np.array_equal(g['diff'][b], g['train_diff'][b])                 # the training tuple carries the same maps
        assert g['bw'][b, 2:].min() == 0.0 and g['bw'][b, 2:].max() == 1.0      # min-max normalised
    assert np.abs(bw[4][0][0].numpy() - g['flow_01']).max() < 5e-5 and np.abs(bw[4][1][0].numpy() - g['flow_10']).max() < 5e-5


def test_second_weight_regime_small_flows_unsaturated_occlusion(golden_dir):
    """Round 6: every other fixture uses xavier weights whose flows reach +-6..20 px and whose occlusion maps
    saturate.  flow_gain = 0.3 on the flow / occlusion rows gives sub-pixel .. 3 px motions and occlusion spread over (0, 1)."""
    from demfi_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(0, flow_gain=0.3)
    for name in ('e2e_smallflow_64x96_t0500_n3', 'e2e_smallflow_64x96_t0125_n2'):
        g = _load(golden_dir, name)
        N = int(g['N'])
        x = synthetic_window(int(g['H']), int(g['W']), int(g['seed']))
        with torch.no_grad():
            d1, fin, flows, occs, ov = O.forward(sd, x, torch.tensor([[float(g['t'])]]), N)
        gt = x[0, :, 0].numpy()
        for it in range(N):
            for i in range(3):
                assert np.abs(fin[it][i][0].numpy() - g['finals'][it, i]).max() < 5e-5
                assert abs(O.psnr(fin[it][i][0].numpy(), gt) - O.psnr(g['finals'][it, i], gt)) <= 1e-3
        for i in range(N + 1):
            assert np.abs(flows[i][0].numpy() - g['flows'][i]).max() < 5e-5
            assert np.abs(occs[i][0].numpy() - g['occs'][i]).max() < 5e-5
        sat = ((g['occs'][-1] < 0.02) | (g['occs'][-1] > 0.98)).mean()
        assert np.abs(g['flows'][-1]).max() < 4.0 and sat < 0.05                # the regime the fixture claims
