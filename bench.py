#!/usr/bin/env python
"""Headline benchmark: interpolated frames/sec @720p x8 MFI, N_tst=3 (BASELINE.json metric, configs[1]).

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

One "step" = one input window of a synthetic 720p clip: 4 blurry uint8 frames in pinned host memory -> H2D ->
normalise + reflect-pad to 736x1280 -> t-independent trunk once -> 7 time instants t = k/8, each with N_tst = 3
recursive boosts -> 7 interpolated frames St (+ S0/S1) -> crop + denorm + uint8 -> D2H (the metric
includes H2D of the window and D2H of the outputs, excludes the PNG codec).  Each rank owns its own windows
(clip-parallel, no data-path collective; the state_dict is broadcast once over RCCL); value = all ranks' St frames /
max-over-ranks time.  Rank 0 prints ONE
JSON line.  A plain run does only what that headline needs: set up, warm up, time the K steps, dump the outputs if asked.
--full adds everything else after the timed region: the byte-for-byte check against the module path, the per-kernel rooflines
(runs of their own over the launch plan), the final-frames-only figure and the CPU baseline (oracle, bounded sample).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TF = {'fp16': 2500.0, 'fp32': 157.3}      # /opt/skills/guides/MI355X_MICROARCH.md:41-42 (dense)
HBM_PEAK_GBS = 8000.0                                # MI355X_MICROARCH.md:35


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--n-tst', type=int, default=3)
    ap.add_argument('--mfi', type=int, default=8)
    ap.add_argument('--dtype', default='fp16', choices=['fp16', 'fp32'])
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also run the checks and side figures: verification against the module path, per-kernel '
                         'rooflines, final-frames-only, CPU baseline')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without the CPU baseline')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--batch', type=int, default=4, help='windows per copy/compute batch of the uint8 pipeline')
    ap.add_argument('--profile-ops', default='', help='write the per-launch timing table of --full to this file')
    ap.add_argument('--n-ctx', type=int, default=None, help='per-t contexts batched per launch sequence (default: runner decides, printed in config)')
    ap.add_argument('--n-trunk', type=int, default=None, help='trunk buffer sets pipelined over windows')
    ap.add_argument('--no-verify', action='store_true', help='--full without the byte-for-byte check of one sunk window against the module path')
    ap.add_argument('--checkpoint', default='', help="reference checkpoint (.pt with 'state_dict_Model', main.py:316,351) to load instead of the random-init weights")
    ap.add_argument('--auto', action='store_true', help='let the runner probe the free memory for n_ctx / n_trunk (default: fixed values)')
    ap.add_argument('--with-png', action='store_true', help='side figure: PNG folder -> PNG folder frames/s of this rank (codec + threads inside)')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='after the timed steps, write the frames the last timed step delivered as DIR/<name>.npy (float32, at most 64 MB in all)')
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')
    if a.profile_ops and not a.full:
        ap.error('--profile-ops writes the per-launch table that --full measures: add --full')
    return a


def cpu_baseline(n_tst, full_px, model=None, dev=None):
    """Oracle (CPU restatement, reference semantics: one FULL forward per t, no trunk caching) on a bounded sample:
    the full padded 736x1280 frame of the workload, ONE of the 7 t (about 30 s on 32 threads).  The same window / t is
    then pushed through the HIP path to report the metric's second half: PSNR against the fp32 reference semantics."""
    from demfi_amd import synthetic_state_dict, synthetic_window
    from oracle import demfi_oracle as O
    torch.set_num_threads(min(os.cpu_count() or 1, 32))       # beyond ~32 threads MKLDNN convs of this size slow down
    sd = synthetic_state_dict(0)
    h, w = 736, 1280
    x = synthetic_window(h, w, 1)
    t = torch.tensor([[0.5]])
    with torch.no_grad():
        O.forward(sd, synthetic_window(64, 64, 2), t, 1)          # warm-up
        t0 = time.time()
        ref = O.forward(sd, x, t, n_tst)
        dt = time.time() - t0
    frac = (h * w) / float(full_px)
    out = {'value': round(frac / dt, 5), 'unit': 'frames/s (720p-equivalent)', 'cores': torch.get_num_threads(),
           'kind': 'port', 'seconds_for_sample': round(dt, 2),
           'sample': 'oracle/demfi_oracle.forward fp32, one t, N_tst=%d, on a %dx%d window (%.3f of the padded 736x1280 '
                     'pixels); reference semantics = full forward per frame' % (n_tst, h, w, frac)}
    psnr = None
    if model is not None:
        got = model(x.to(dev), t.to(dev), n_tst)
        st = got[1][n_tst - 1][2][0].float().cpu().numpy()
        st_ref = ref[1][n_tst - 1][2][0].numpy()
        gt = x[0, :, 0].numpy()                                 # fixed pseudo ground truth
        psnr = {'St_vs_oracle_fp32_dB': round(float(O.psnr(st, st_ref)), 2),
                'dPSNR_vs_pseudoGT_dB': round(float(O.psnr(st, gt) - O.psnr(st_ref, gt)), 4),
                'note': 'same window, t=0.5, N_tst=%d; oracle = CPU fp32 restatement pinned to the reference' % n_tst}
    return out, psnr


def synthetic_clip_u8(h, w, n_frames, seed):
    """n_frames uint8 BGR frames of a moving textured pattern with an 11-tap temporal box blur (SURVEY.md section 8d, config
    2; the reference's inputs are 11-frame averages, README.md:71) -- host tensors in pinned memory."""
    import numpy as np
    from demfi_amd import synthetic_window
    taps = 11
    base = synthetic_window(h + 2 * (n_frames + taps), w + 4 * (n_frames + taps), seed)[0, :, 0]      # [3,H',W'] in [-1,1]
    out = []
    for i in range(n_frames):
        acc = torch.zeros(3, h, w)
        for k in range(taps):                                   # sub-frame motion: 1 px down, 2 px right per sharp frame
            s = i * 2 + k // 4
            acc += base[:, s:s + h, 2 * s:2 * s + w]
        f = ((acc / taps).permute(1, 2, 0) + 1) * 127.5
        out.append(f.clamp(0, 255).to(torch.uint8).contiguous().pin_memory())
    return out


DUMP_BYTES = 64 * 10 ** 6                               # --dump-outputs: .npy payload of all arrays together
DUMP_SEED = 0


def dump_outputs(d, arrays):
    """--dump-outputs: the uint8 frames the timed path delivered for its last window, as float32 ``d/<name>.npy``, so that two builds
    can be compared output for output.  When all of them together exceed DUMP_BYTES, each array is cut to a fixed sample of its
    flat elements (sorted indices drawn by numpy.random.default_rng(DUMP_SEED), a share of the budget proportional to its size):
    the same elements in every run with the same arguments."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    total = sum(int(v.numel()) for v in arrays.values())
    cap = DUMP_BYTES // 4 - 1024                                    # float32 elements, headroom for the .npy headers
    info = {}
    for name, v in arrays.items():
        x = v.cpu().numpy()
        if total > cap:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(x.size, x.size * cap // total, replace=False))
            x = x.reshape(-1)[idx]
        np.save(os.path.join(d, name + '.npy'), x.astype(np.float32))
        info[name] = {'shape': list(v.shape), 'dtype': str(v.dtype).replace('torch.', ''), 'elements_written': int(x.size),
                      'sample': 'flat elements at sorted default_rng(%d) indices' % DUMP_SEED if total > cap else None}
    return {'dir': os.path.abspath(d), 'arrays': info}


def png_side_figure(a, model, runner):
    """Side figure (--with-png; NOT the headline, SURVEY.md section 8d excludes the codec): one scene folder of PNG frames ->
    folder of PNG frames through ClipRunner.run_folder (streamed decode ahead of the GPU, bounded encode queue behind it), so that
    the host side of an 8-GPU node is a number: frames/s of this GPU with the codec inside, host threads used, and the
    single-core codec times that say how many cores a GPU needs to stay busy."""
    import shutil
    import tempfile
    from demfi_amd import clipio
    from demfi_amd.clip import ClipRunner
    d = tempfile.mkdtemp(prefix='demfi_png_')
    try:
        scene = os.path.join(d, 'scene')
        os.makedirs(scene)
        clip = synthetic_clip_u8(a.height, a.width, 19, seed=77)           # 19 frames -> 16 windows
        t0 = time.perf_counter()
        for i, f in enumerate(clip):
            clipio.write_frame(os.path.join(scene, '%05d.png' % i), f.numpy())
        enc_ms = 1e3 * (time.perf_counter() - t0) / len(clip)
        t0 = time.perf_counter()
        for i in range(len(clip)):
            clipio.read_frame(os.path.join(scene, '%05d.png' % i))
        dec_ms = 1e3 * (time.perf_counter() - t0) / len(clip)
        threads = int(os.environ.get('DEMFI_IO_THREADS', 0)) or min(32, os.cpu_count() or 4)
        pool = clipio.FramePool(threads)
        cr = ClipRunner(model, a.height, a.width, a.n_tst, a.mfi, batch=a.batch, final_only=False, n_ctx=runner.n_ctx, n_trunk=runner.n_trunk)
        cr.run_folder(scene, os.path.join(d, 'warm'), pool=pool)
        t0 = time.perf_counter()
        nw, nf = cr.run_folder(scene, os.path.join(d, 'out'), pool=pool)
        dt = time.perf_counter() - t0
        pool.close()
        fps = nw * (a.mfi - 1) / dt
        per_st = (nf / float(nw * (a.mfi - 1)))                             # PNGs written per St frame (St + deblurred)
        return {'value': round(fps, 2), 'unit': 'St frames/s, PNG folder -> PNG folder, 1 GPU', 'windows': nw, 'png_written': nf,
                'png_read': len(clip), 'host_threads': threads, 'host_cores': os.cpu_count(),
                'encode_ms_per_frame_one_core': round(enc_ms, 1), 'decode_ms_per_frame_one_core': round(dec_ms, 1),
                'cores_to_feed_one_gpu_at_headline_rate': None,                 # filled by main() once the headline is known
                'png_per_St_frame': round(per_st, 3),
                'note': 'NOT the headline (the metric excludes the codec); zlib level 1 / Sub filter / Z_RLE = OpenCV defaults'}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def box_id(dev):
    """Which box / GPU produced the line (boxes differ by +-3 %, profiles/r03_notes.md section 11): host name, device name, PCI bus, the
    device's maximum shader clock and (when the sysfs node exists) the sclk level table of the first AMD card."""
    import socket
    pr = torch.cuda.get_device_properties(dev)
    out = {'host': socket.gethostname(), 'gpu': pr.name, 'arch': getattr(pr, 'gcnArchName', ''), 'cus': pr.multi_processor_count,
           'hbm_gb': round(pr.total_memory / 1e9, 1), 'max_sclk_mhz': round(getattr(pr, 'clock_rate', 0) / 1e3, 0),
           'pci_bus_id': getattr(pr, 'pci_bus_id', None)}
    try:
        import glob
        for f in sorted(glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk')):
            out['pp_dpm_sclk'] = ' | '.join(l.strip() for l in open(f).read().splitlines())
            break
    except OSError:
        pass
    return out


def load_rocprof_frac():
    """roofline.frac of the same ten launches from the committed rocprofv3 kernel trace of a sequential bench run
    (profiles/r04_seq_trace_roofline.json, written by tools/trace_by_op.py on the GPU box) so that the two timings -- HIP events
    measured live in this run, rocprofv3 kernel durations measured on the box that produced the committed trace -- sit side by side."""
    for r in ('r06', 'r05', 'r04', 'r03'):
        path = os.path.join(ROOT, 'profiles', r + '_seq_trace_roofline.json')
        if os.path.exists(path):
            with open(path) as f:
                return json.load(f)
    return None


def load_pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary (profiles/r02_pmc_traffic.json,
    written by tools/pmc_traffic.py on the GPU box: separate --pmc passes, 2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction)."""
    path = None
    for r in ('r06', 'r05', 'r04', 'r03', 'r02'):
        path = os.path.join(ROOT, 'profiles', r + '_pmc_traffic.json')
        if os.path.exists(path):
            break
    if not path or not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def load_pmc_innet():
    """Per-kernel HBM bytes / L2 hit rate / texture-addresser duty of the BATCHED launch plan in the network (profiles/r06_pmc_innet.json,
    written by tools/pmc_innet.py on a GPU box: rocprofv3 --pmc passes over this bench); the two fat warps of a window told apart."""
    path = os.path.join(ROOT, 'profiles', 'r06_pmc_innet.json')
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def by_op_table(prof, nb, peak_tf, window_ms):
    """Machine-readable per-op table: every launch of a window's plan grouped by call site -- launches, ms per
    window, achieved TFLOP/s and algorithmic GB/s with their fractions of the dense MFMA peak and of the 8 TB/s HBM peak.  A launch of the
    batched plan covers the nb time instants of a window; the trunk runs once per window."""
    import collections
    g = collections.OrderedDict()
    for seg, kind, name, ms, macs, ctx, by in prof:
        key = name if kind in ('conv', 'resblock', 'gru_r', 'gru_zq') else kind
        if seg == 'trunk':
            key = 'trunk:' + key
        e = g.setdefault(key, {'kind': kind, 'launches': 0, 'ms': 0.0, 'flop': 0.0, 'bytes': 0.0})
        e['launches'] += 1
        e['ms'] += ms
        e['flop'] += 2.0 * macs
        e['bytes'] += by
    tot = sum(e['ms'] for e in g.values())
    rows = []
    for key, e in sorted(g.items(), key=lambda kv: -kv[1]['ms']):
        tf = e['flop'] / (e['ms'] * 1e-3) / 1e12 if e['ms'] > 0 else 0.0
        gb = e['bytes'] / (e['ms'] * 1e-3) / 1e9 if e['ms'] > 0 else 0.0
        rows.append({'op': key, 'kind': e['kind'], 'launches': e['launches'], 'ms': round(e['ms'], 4), 'share': round(e['ms'] / tot, 4),
                     'TFLOPs': round(tf, 1), 'frac_mfma': round(tf / peak_tf, 4), 'algorithmic_GBs': round(gb, 1), 'frac_hbm': round(gb / HBM_PEAK_GBS, 4)})
    return {'note': 'sum of per-launch HIP-event times of ONE window: trunk once + the batched per-t plan (%d time instants per launch); '
                    'frac_mfma against the dense peak of the path dtype, frac_hbm = algorithmic bytes (every tensor once) against 8 TB/s; '
                    'sorted by time; window_ms_pipelined is the headline ms_per_step (trunk of the next window overlaps)' % nb,
            'sum_ms': round(tot, 3), 'window_ms_pipelined': window_ms, 'rows': rows}


def self_launch_argv(n, argv=None, port=None):
    """The command a bare ``python bench.py --gpus N`` (N > 1, no WORLD_SIZE in the environment) re-executes itself as: one rank per
    GPU under torch.distributed.run on 127.0.0.1 with a free port, the caller's own flags passed through unchanged."""
    import socket
    if port is None:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
    argv = list(sys.argv[1:] if argv is None else argv)
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
            '--master-port', str(port), os.path.abspath(__file__)] + argv


def self_launch(n):
    """Runs the N-rank job as a child process; rank 0's JSON line goes to this process's stdout, the return code is non-zero when
    any rank failed (torch.distributed.run's own exit status)."""
    import subprocess
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')        # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 8) // n)))
    return subprocess.call(self_launch_argv(n), env=env)


def main():
    a = parse()
    rank = int(os.environ.get('RANK', 0))
    local = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if 'WORLD_SIZE' not in os.environ and a.gpus > 1:
        raise SystemExit(self_launch(a.gpus))                 # bare `python bench.py --gpus N`: one rank per GPU under torch.distributed.run
    if world != a.gpus:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run)' % (a.gpus, world))
    from demfi_amd import DeMFInet, HyperParams, synthetic_state_dict
    from demfi_amd.clip import window_list
    from demfi_amd.runner import WindowRunner
    from demfi_amd import dist as D
    # test hook: DEMFI_BENCH_BACKEND=gloo runs all ranks of a multi-process launch on the GPUs that exist (rank % count),
    # so the N>1 control flow can be exercised on a 1-GPU box; the driver's 8-GPU run uses the default nccl (= RCCL)
    backend = os.environ.get('DEMFI_BENCH_BACKEND') or None
    local = local % torch.cuda.device_count() if backend == 'gloo' else local
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    D.init(world, rank, local, backend=backend)
    dtype = torch.float16 if a.dtype == 'fp16' else torch.float32
    model = DeMFInet(HyperParams(gpu=local), dtype=dtype)
    if rank == 0:
        if a.checkpoint:
            from demfi_amd.weights import load_checkpoint
            model.load_state_dict(load_checkpoint(a.checkpoint))         # the reference's .pt (main.py:316,351); other ranks get it by broadcast
        else:
            model.load_state_dict(synthetic_state_dict(0))   # random-init weights of the architecture (no checkpoint offline)
    model = model.to(dev).eval()
    # ONE flat broadcast of the 7.4 M parameters (RCCL over xGMI): every rank then owns the real state_dict and packs its
    # own engine, so later engine rebuilds (other frame sizes) are correct on every rank
    D.broadcast_state_dict(model, world, device=dev if backend != 'gloo' else 'cpu')
    runner = WindowRunner(model, a.height, a.width, a.n_tst, a.mfi, use_graph=not a.no_graph, n_ctx=a.n_ctx, n_trunk=a.n_trunk, auto=a.auto)
    # synthetic clip: each rank gets its own 11-frame clip = 8 distinct windows (weak scaling), uint8 frames in PINNED HOST
    # memory: the timed region contains the H2D of every window's 4 frames, the forward, and the D2H of its uint8 outputs
    frames = synthetic_clip_u8(a.height, a.width, 11, seed=1000 * rank + 1)
    wins = window_list(len(frames))
    pick = lambda first, n: [wins[(first + i) % len(wins)] for i in range(n)]
    sunk = [0]
    kept = {}                                                 # the LAST timed window's delivered bytes (verified after the timed region)
    keep_k = [-1]

    def sink(k, st, s01):                                     # the host consumer: touches every delivered window
        sunk[0] += int(st.shape[0])
        if k == keep_k[0]:
            kept['st'], kept['s01'] = st.clone(), s01.clone()
    if a.warmup:
        runner.run_clip_u8(frames, pick(0, a.warmup), sink, batch=a.batch, reuse_frames=False)
    torch.cuda.synchronize()
    sunk[0] = 0
    D.barrier()
    t0 = time.perf_counter()
    # a step = one window: H2D (4 uint8 frames, 11 MB) -> reflect pad + normalise -> trunk once -> 7 time instants x N_tst
    # boosts -> crop + denorm + uint8 -> D2H (7 St + S0/S1, 25 MB); the K steps are handed to the scheduler together so that
    # copies, the trunk of window w+1 and the time instants of window w overlap (WindowRunner.run_clip_u8)
    timed = pick(a.warmup, a.steps)
    keep_k[0] = a.steps - 1
    runner.run_clip_u8(frames, timed, sink, batch=a.batch, reuse_frames=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dt_rank = dt
    cdev = dev if backend != 'gloo' else 'cpu'
    dt = D.max_over_ranks(dt, cdev)
    # self-check of a multi-rank line: how many ranks took part (all-reduced count) and the spread of their own clocks
    seen = D.sum_over_ranks([1.0, dt_rank], cdev)
    dt_min = -D.max_over_ranks(-dt_rank, cdev)
    D.barrier()
    assert sunk[0] == (a.mfi - 1) * a.steps, 'frames delivered to the host: %d' % sunk[0]
    verify = None
    if a.full and not a.no_verify:
        # Self-verification of the measured path: the bytes the timed run delivered for its last window (fused uint8 ingest ->
        # batched per-t plan -> uint8 sink epilogue -> D2H) against the REFERENCE-shaped path on the same frames: one
        # DeMFInet.forward per t through pad_forward_crop, separate normalise / denorm kernels.  Any difference fails the run.
        from demfi_amd.harness import module_window_u8
        st_ref, s01_ref = module_window_u8(model, [frames[i] for i in timed[-1]], a.n_tst, a.mfi)
        bad = int((kept['st'] != st_ref.cpu()).sum()) + int((kept['s01'] != s01_ref.cpu()).sum())
        verify = {'window': list(timed[-1]), 'frames_compared': a.mfi + 1, 'bytes_compared': int(kept['st'].numel() + kept['s01'].numel()),
                  'mismatching_bytes': bad, 'against': 'DeMFInet.forward per t via harness.pad_forward_crop + demfi_frame_to_u8 (module path)'}
        if bad:
            raise SystemExit('bench.py: the timed path delivered %d bytes that differ from the module path: %s' % (bad, json.dumps(verify)))
    dumped = dump_outputs(a.dump_outputs, {'st': kept['st'], 's01': kept['s01']}) if a.dump_outputs and rank == 0 else None
    frames_out = (a.mfi - 1) * a.steps * world
    eng = runner.engine
    if rank == 0:
        out = {
            # BASELINE.json's metric on its configuration; other --height/--mfi/--n-tst values label themselves
            'metric': 'interpolated frames/sec @%dp x%d MFI (N_tst=%d)' % (a.height, a.mfi, a.n_tst),
            'value': round(frames_out / dt, 3), 'unit': 'frames/s',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': round(1e3 * dt / a.steps, 2),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f16' if a.dtype == 'fp16' else 'f32',
            'data': 'synthetic' if not a.checkpoint else 'synthetic frames, checkpoint weights (%s)' % os.path.basename(a.checkpoint),
            'ranks_seen': int(round(float(seen[0]))),
            'per_rank_fps': {'min': round((a.mfi - 1) * a.steps / dt, 3), 'max': round((a.mfi - 1) * a.steps / dt_min, 3),
                             'mean_s': round(float(seen[1]) / max(1.0, float(seen[0])), 4)},
            'box': box_id(dev),
            'config': {'workload': 'DeMFI-Net_rb N_tst=%d, x%d MFI, %dx%d (padded %dx%d), %s, clip-parallel windows, '
                                   'random-init weights; uint8 frames host->HBM->host inside the timed region (PNG codec '
                                   'excluded), %d distinct windows' % (a.n_tst, a.mfi, a.height, a.width, eng.H, eng.W, a.dtype,
                                                                         min(len(wins), a.steps)),
                       'frames_per_step': a.mfi - 1, 'graph': not a.no_graph, 'parallelism': 'clip%d' % world,
                       'n_ctx': runner.n_ctx, 'n_trunk': runner.n_trunk, 'runner': runner.config,
                       'h2d_bytes_per_step': 4 * a.height * a.width * 3, 'd2h_bytes_per_step': (a.mfi + 1) * a.height * a.width * 3},
        }
        if verify is not None:
            out['verified'] = verify
        if dumped is not None:
            out['dumped_outputs'] = dumped
        if a.full:
            out.update(kernel_figures(a, runner, out['ms_per_step']))
        if a.full and world == 1 and runner.tb:
            # the same K steps for a consumer of the LAST recursion's frames only (what the reference's test / test_custom write,
            # utils.py:1430-1434): the warp + D2 tail of recursions 0..N-2 feeds nothing else and is not run.  Reported beside
            # the headline, which computes every Sharps_final entry like the reference module does.
            fo = WindowRunner(model, a.height, a.width, a.n_tst, a.mfi, use_graph=not a.no_graph, final_only=True)
            fo.run_clip_u8(frames, pick(0, max(a.warmup, 1)), sink, batch=a.batch, reuse_frames=False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fo.run_clip_u8(frames, pick(a.warmup, a.steps), sink, batch=a.batch, reuse_frames=False)
            torch.cuda.synchronize()
            dt_fo = time.perf_counter() - t1
            out['final_frames_only'] = {'value': round((a.mfi - 1) * a.steps / dt_fo, 3), 'unit': 'frames/s',
                                        'ms_per_step': round(1e3 * dt_fo / a.steps, 2),
                                        'note': 'NOT the headline: D2 of recursions 0..N-2 skipped (outputs-only work); delivered uint8 '
                                                'frames bit-identical (tests/test_gpu_e2e.py::test_final_only_runner_delivers_the_same_frames)'}
            del fo
        if a.with_png and world == 1:
            pp = png_side_figure(a, model, runner)
            # cores one GPU needs at the headline rate: (encode of the St + deblurred frames + decode of ~1 input frame per window) per second
            pp['cores_to_feed_one_gpu_at_headline_rate'] = round(out['value'] * (pp['png_per_St_frame'] * pp['encode_ms_per_frame_one_core'] +
                                                                                 pp['decode_ms_per_frame_one_core'] / (a.mfi - 1)) / 1e3, 1)
            out['png_pipeline'] = pp
        if a.full and world == 1 and not a.no_cpu_baseline:
            out['cpu_baseline'], out['psnr'] = cpu_baseline(a.n_tst, eng.H * eng.W, model, dev)
        print(json.dumps(out))
    D.finalize()


def kernel_figures(a, runner, window_ms):
    """--full: the per-kernel objects of the line (roofline, roofline_hbm, breakdown_ms, by_op, gru) from in-sequence passes of
    the launch plan of their own after the timed region; --profile-ops also writes their per-launch table."""
    eng = runner.engine
    out = {}
    # ---- roofline of the dominant kernel, measured live with HIP events on the launch stream, IN SEQUENCE: the whole launch plan
    # runs op after op with an event between consecutive launches (mean of 5 passes), so every kernel sees the clock and cache
    # state the pipeline leaves it -- an isolated repeat loop lets the clock recover and read 4-5 % faster ----
    # batched runner: every convolution launch covers the nb per-t contexts of a trunk set (batch x nb), point-wise
    # kernels run once per context
    nb = eng.n_ctx if runner.tb else 1
    prof = eng.profile(a.n_tst, isolated=False, batched=runner.tb)
    per_t = sum(p[3] for p in prof if p[0] != 'trunk') / nb
    trunk = sum(p[3] for p in prof if p[0] == 'trunk')
    convs = [p for p in prof if p[1] in ('conv', 'resblock', 'gru_r', 'gru_zq')]              # resblock (round 5): conv1 -> ReLU -> conv2 + identity in ONE launch
    dom = max(convs, key=lambda p: p[3])
    grp = [p for p in convs if p[2].startswith('Decoder_res.')]          # D1 residual blocks: 3x3 64->64, batch 3
    fused = bool(grp) and all(p[1] == 'resblock' for p in grp)
    g_ms = sum(p[3] for p in grp) / len(grp)
    g_fl = 2.0 * sum(p[4] for p in grp) / len(grp)
    tot_conv_ms = sum(p[3] for p in convs)
    tot_conv_fl = 2.0 * sum(p[4] for p in convs)
    peak = MFMA_PEAK_TF[a.dtype]
    ach = g_fl / (g_ms * 1e-3) / 1e12
    pmc = load_pmc_traffic() if a.dtype == 'fp16' and (eng.H, eng.W) == (736, 1280) else None
    kname = 'resblock3x3_c64_kernel' if fused else ('conv3x3_c64_stg_kernel' if a.dtype == 'fp16' else 'conv_kernel<float,2>')
    # The kernel is co-bound: arithmetic intensity 288 (no residual) / 192 flop/B (residual) sits below the chip balance
    # point of 312, so both ceilings are reported per variant.  Algorithmic bytes (every tensor once):
    # input + output (+ residual) = 2 (3) x H x W x 64 ch x 2 B per image.
    img_bytes = eng.H * eng.W * 64 * 2
    variants = {}
    # fused residual block: the intermediate stays in LDS and the identity comes from the input tile, so the algorithmic bytes of a
    # launch are input + output only (2 tensors for 2 convolutions: 576 flop/B -- MFMA-bound, well above the chip balance of 312)
    for key, sel, ntens in ((('fused_block', '', 2),) if fused else (('no_residual', '.conv1', 2), ('residual', '.conv2', 3))):
        g2 = [p for p in grp if p[2].endswith(sel)]
        v_ms = sum(p[3] for p in g2) / len(g2)
        v_fl = 2.0 * sum(p[4] for p in g2) / len(g2)
        v_by = float(ntens * img_bytes * 3 * nb)
        variants[key] = {'launches': len(g2), 'avg_launch_ms': round(v_ms, 4), 'TFLOPs': round(v_fl / v_ms / 1e9, 1),
                         'frac_mfma': round(v_fl / v_ms / 1e9 / peak, 4), 'algorithmic_bytes': v_by,
                         'GBs': round(v_by / v_ms / 1e6, 1), 'frac_hbm': round(v_by / v_ms / 1e6 / HBM_PEAK_GBS, 4)}
    out['roofline'] = {'kernel': '%s: D1 residual blocks%s, 3x3 64->64, batch 3 x %d time instants per launch (%d launches per %d frames)' %
                                 (kname, ' (conv1 -> ReLU -> conv2 + identity fused: 2 convolutions per launch)' if fused else '', nb, len(grp), nb),
                       'bound': 'mfma', 'co_bound': None if fused else 'mfma+hbm', 'achieved': round(ach, 2), 'peak': peak,
                       'unit': 'TFLOP/s', 'frac': round(ach / peak, 4),
                       'variants': variants,
                       # HBM bytes per launch from rocprofv3 PMC (2*FETCH_SIZE + WRITE_SIZE, gfx950 correction), read from
                       # the committed summary (profiles/r02_pmc_traffic.json; per batch-3 image group: x nb for a launch of the batched plan)
                       'traffic': ((pmc.get('resblock_traffic_bytes_b21') if nb == 7 else None) if fused else
                                   (pmc.get('dominant_traffic_bytes_b21') if nb == 7 and pmc.get('dominant_traffic_bytes_b21')
                                    else pmc.get('dominant_traffic_bytes') * nb)) if pmc else None,
                       'algorithmic_bytes': (2.0 * img_bytes * 3 * nb) if fused else (pmc.get('dominant_algorithmic_bytes') * nb if pmc else None),
                       'traffic_source': pmc.get('source') if pmc else None,
                       'avg_launch_ms': round(g_ms, 4), 'flop_per_launch': g_fl,
                       'frac_rocprof': None, 'rocprof': None,
                       'timing': 'IN SEQUENCE: mean over 5 passes of the whole launch plan, HIP events on the launch stream between consecutive '
                                 'launches (includes the 5-8 us launch gap; reproduces the rocprofv3 in-sequence kernel durations of profiles/ within ~1 %)',
                       'sustained_clock_note': 'in-kernel s_memtime traces in the network (profiles/r04_notes.md sections 11-12): the clock falls as the matrix pipe fills -- 1.87 GHz at 0.47 busy '
                                               '(this kernel with residual), 1.65 GHz at 0.68 busy (without), 1.57 GHz at 0.83 busy (Ch_Reducer); '
                                               'back-to-back MFMAs from registers sustain 1460 TFLOP/s on random fp16 operands (tools/microbench/mfma_peak.hip, 2190 on zeros); '
                                               'frac is quoted against the 2.4 GHz datasheet peak as required',
                       'frac_of_sustained_random_operand_peak': round(ach / 1460.0, 4) if a.dtype == 'fp16' else None,
                       'all_convs_TFLOPs': round(tot_conv_fl / (tot_conv_ms * 1e-3) / 1e12, 2),
                       'slowest_conv': '%s %.3f ms' % (dom[2], dom[3])}
    rp = load_rocprof_frac() if a.dtype == 'fp16' and (eng.H, eng.W) == (736, 1280) and nb == 7 else None
    if rp and bool(rp.get('fused')) != fused:               # a committed trace of the other kernel says nothing about this run
        rp = None
    if rp:
        out['roofline']['frac_rocprof'] = round(g_fl / (rp['avg_launch_ms'] * 1e-3) / 1e12 / peak, 4)
        out['roofline']['rocprof'] = rp
    chr_ = [p for p in convs if p[2] == 'Ch_Reducer']
    if chr_ and a.dtype == 'fp16':
        c_ms, c_fl = chr_[0][3], 2.0 * chr_[0][4]
        out['roofline']['second_kernel'] = {'kernel': 'conv_wstream_c64_kernel<7>: Ch_Reducer, 7x7 192->64, %d time instants per launch (round 3: A fragments from L2 '
                                                      'into a register ring, 8 accumulators per wave)' % nb,
                                            'avg_launch_ms': round(c_ms, 4), 'TFLOPs': round(c_fl / c_ms / 1e9, 1), 'frac_mfma': round(c_fl / c_ms / 1e9 / peak, 4)}
    wb = [p for p in prof if p[1] == 'warp_fat']
    # round 5: ONE launch covers the nb time instants (one grid slice per context): per-time-instant figures = launch / contexts
    esz = 2 if a.dtype == 'fp16' else 4
    px = eng.H * eng.W
    innet = load_pmc_innet() if a.dtype == 'fp16' and (eng.H, eng.W) == (736, 1280) and nb == 7 else None
    # FAC + warp kernel of the north star: Eq.(2) blend of two backward-warped feature maps.  The window's two call sites differ:
    #   Ft: sources = trunk features F0 / F1, SHARED by the nb time instants of a window: algorithmic bytes per launch =
    #       sources once + nb x (output + flows + logit) -- and they are largely cache-resident (round 5 priced them once per time
    #       instant: 404 B/px, which flattered this half -- VERDICT r5 weak #5);
    #   rF: sources = the refined features of each time instant, fresh from HBM: 3 C e + 20 = 404 B/px per time instant.
    # The headline figure of this block is the rF half (a real HBM stream); both halves carry the PMC bytes of the batched launch
    # in the network beside the algorithmic ones, with the L2 hit rate and the texture-addresser duty the counters give.
    halves = {}
    for i, p_ in enumerate(wb[:2]):
        key = 'Ft' if i == 0 else 'rF'
        ctxs = p_[5]
        alg = p_[6] / ctxs                                   # algorithmic bytes per time instant (Engine.op_algorithmic_bytes)
        ms_t = p_[3] / ctxs
        h = {'what': ('sources: trunk features F0 / F1, shared by the %d time instants of a window (fetched once)' % ctxs) if i == 0 else
                     'sources: the refined features of this time instant, fresh from HBM',
             'ms_per_time_instant': round(ms_t, 4), 'algorithmic_bytes_per_time_instant': round(alg),
             'achieved_GBs': round(alg / (ms_t * 1e-3) / 1e9, 1), 'frac': round(alg / (ms_t * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
             'frac_at_404_B_per_px': round((3 * 64 * esz + 20) * px / (ms_t * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        pm = ((innet or {}).get('warp_blend_fat') or {}).get(key)
        if pm:
            tr = pm['hbm_bytes_per_launch'] / ((innet['warp_blend_fat'].get('time_instants_per_launch') or ctxs))
            # bytes through the L2s' fabric port: HBM + what the Infinity Cache serves (the shared sources of the Ft half are re-read per time instant from there)
            h.update({'pmc_bytes_per_time_instant': round(tr), 'frac_by_pmc_traffic': round(tr / (ms_t * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                      'l2_hit': round(pm['l2_hit'], 3), 'ta_busy_frac': round(pm['ta_busy_frac'], 3)})
        halves[key] = h
    rf = halves.get('rF') or halves.get('Ft')
    ta = rf.get('ta_busy_frac')
    out['roofline_hbm'] = {'kernel': 'warp_blend_fat C=64 (bwarp x2 + Eq.2 blend), in-network flows, the rF call site (sources fresh from HBM); per TIME INSTANT '
                                     '(%d per launch: one grid slice each)' % wb[0][5],
                           # what the counters say limits it: the texture addresser when it is busier than the HBM stream is full
                           'bound': 'ta' if (ta is not None and ta > rf.get('frac_by_pmc_traffic', rf['frac'])) else 'hbm',
                           'bound_note': 'texture addresser busy %.2f of the kernel vs %.2f of the 8 TB/s HBM peak by PMC bytes: 8 distinct 128-byte lines per pixel '
                                         '(two bilinear gathers) keep the TA busier than the HBM stream; priced against HBM as the north star asks' %
                                         (ta, rf.get('frac_by_pmc_traffic', rf['frac'])) if ta is not None else None,
                           'achieved': rf['achieved_GBs'], 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': rf['frac'],
                           'traffic': rf.get('pmc_bytes_per_time_instant'), 'frac_by_pmc_traffic': rf.get('frac_by_pmc_traffic'),
                           'avg_launch_ms': rf['ms_per_time_instant'], 'bytes_per_launch': rf['algorithmic_bytes_per_time_instant'],
                           'launches': len(wb), 'time_instants_per_launch': wb[0][5],
                           'halves': halves,
                           'traffic_source': innet.get('source') if innet else None,
                           'streaming_ceiling_note': 'tools/microbench/hbm_mix (profiles/r03_hbm_mix.txt): a plain streaming kernel with this read : write mix '
                                                     '(3 : 1) reaches 4.7 TB/s at 2 048 workgroups and 5.9 TB/s at its best grid (512, non-temporal, 4 lines in '
                                                     'flight per thread); read-only 7.1, write-only 6.6: 0.60 of 8 TB/s is above what most grids of a COPY reach'}
    fg = [p for p in prof if p[1] == 'fgac']
    if fg:
        # second gather kernel of the north star (FGAC sampling, DeMFInet.py:413-419, 499-508): input feature map read through the
        # bilinear gather + output + the 2-plane offset map, every tensor once
        fg_ms = sum(p[3] for p in fg) / len(fg)
        fg_bytes = (2 * 64 * esz + 8) * eng.H * eng.W
        out['roofline_hbm']['fgac_gather'] = {'avg_launch_ms': round(fg_ms, 4), 'bytes_per_launch': fg_bytes,
                                              'achieved': round(fg_bytes / (fg_ms * 1e-3) / 1e9, 1), 'frac': round(fg_bytes / (fg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                              'traffic': next((v.get('hbm_bytes_per_launch') for k, v in ((innet or {}).get('kernels') or (pmc or {}).get('in_network', {})).items()
                                                               if 'fgac_gather' in k), None)}
        # the source of this gather is cache-resident: by the PMC bytes the launch is a write stream, far below the
        # write-only ceiling -- the honest figure beside the upper-bound one
        tr = out['roofline_hbm']['fgac_gather']['traffic']
        if tr:
            out['roofline_hbm']['fgac_gather']['frac_by_pmc_traffic'] = round(tr / (fg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    cfr = [p for p in prof if p[1] == 'cfr']
    out['breakdown_ms'] = {'trunk_once_per_window': round(trunk, 2), 'per_t': round(per_t, 2),
                           'time_instants_per_launch_sequence': nb,
                           'launches_per_sequence': len([p for p in prof if p[0] != 'trunk']),
                           'conv_share_of_per_t': round(sum(p[3] for p in convs if p[0] != 'trunk') / nb / per_t, 3),
                           'cfr_flow_align': round(cfr[0][3], 4) if cfr else None}
    out['by_op'] = by_op_table(prof, nb, peak, window_ms)
    gr = [p for p in prof if p[1] in ('gru_r', 'gru_zq') or (p[1] == 'conv' and '.GB.conv' in p[2])]
    if gr:
        # SepConvGRU (DeMFInet.py:838-857), 2 half-steps x n_tst recursions per window.  Round 6: r*h, then z + q + blend in one launch
        g_ms = sum(p[3] for p in gr)
        g_fl = 2.0 * sum(p[4] for p in gr)
        g_by = sum(p[6] for p in gr)
        out['gru'] = {'kernel': 'gru_sep5_kernel<R> + gru_sep5_kernel<ZQS> (gru.hip, round 6: z stays on chip; both gates of a cout block in one wave)' if any(p[1] == 'gru_zq' for p in gr)
                                else 'conv_sep5_c128_persist_kernel: z|r launch + q launch (round 5)',
                      'launches_per_window': len(gr), 'ms_per_window': round(g_ms, 3), 'TFLOPs': round(g_fl / g_ms / 1e9, 1),
                      'frac_mfma': round(g_fl / g_ms / 1e9 / peak, 4), 'algorithmic_bytes_per_px_per_half_step': round(g_by / (px * nb * 2 * a.n_tst), 1),
                      'algorithmic_GBs': round(g_by / g_ms / 1e6, 1), 'frac_hbm': round(g_by / g_ms / 1e6 / HBM_PEAK_GBS, 4),
                      'pmc': {k: {'hbm_bytes_per_launch': round(v['hbm_bytes_per_launch']), 'bytes_per_px': round(v['hbm_bytes_per_launch'] / (px * nb), 1),
                                  'l2_hit': round(v['l2_hit'], 3)} for k, v in ((innet or {}).get('gru') or {}).items()} or None}
    if a.profile_ops:
        with open(a.profile_ops, 'w') as f:
            for p in prof:
                tf = 2.0 * p[4] / (p[3] * 1e-3) / 1e12 if p[4] else 0.0
                f.write('%-7s %-10s %-48s %9.4f ms %8.1f TFLOP/s nb=%d\n' % (p[0], p[1], p[2], p[3], tf, p[5]))
    return out


if __name__ == '__main__':
    main()
