#!/usr/bin/env python3
"""FGN inference throughput on MI355X: query-images / s for full ``FGN.simple_test``.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One step = one pass of the hot path over one synthetic episode per GPU (cfg3 of
BASELINE.json: COCO2VOC 3-way 3-shot, query 3x800x1333, 9 supports 3x256x256, seeded
random-init ResNet-50-C4 FGN weights), measured the way the reference's ``simple_test``
works (fgn.py:187-303): a step starts from HOST tensors (pinned; ``modify_input``'s
host->device copies, fgn.py:92-99, run on an upload stream and overlap the previous
episode) and ends with the numpy result dicts, including the COCO RLE of the detected masks
AND of the query's ground-truth masks (``qry_isegmaps_rle``, fgn.py:298).
Episodes are independent, so N GPUs run N episodes per step (weak scaling) and the per-step
detections (boxes, scores, labels, 14x14 mask probabilities) are gathered to every rank with
one RCCL all-gather of fixed-size padded buffers.  Rank 0 prints ONE JSON line.

``python bench.py --gpus N`` without a torch.distributed environment starts the N ranks itself
(a child ``torch.distributed.run``, before this process touches a GPU).

A plain run sets up, warms up, times K steps of the replayed pipeline and prints the line (``--dump-outputs DIR``:
plus the results of the last timed step as .npy files).  ``--full`` adds what needs more than that: the conv roofline
from event-stamped steps, the CPU baseline, and the accuracy and trained-heads legs against the CPU oracle.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DATASET = {'cfg1': 'MNISTISEG', 'cfg2': 'OMNIISEG', 'cfg3': 'COCO2VOC', 'cfg4': 'COCO2VOC', 'cfg5': 'COCO2VOC'}
PEAK_FP32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0     # the same table, "Peak BF16/FP16 MFMA" (dense): 16x the f32-input MFMA
X3_TERMS = 6                       # bf16 MFMA products conv_pw_x3_kernel issues per f32 product (csrc/conv_pw_x3.h)
H2_TERMS = 3                       # f16 MFMA products conv_pw_h2_kernel issues per f32 product (csrc/conv_pw_h2.h)
# options of the legs a plain run leaves out (argparse dests)
FULL_ONLY = ('no_cpu_baseline', 'cpu_episodes', 'accuracy_episodes', 'train_heads_steps', 'trained_eval_episodes',
             'isolated_steps', 'launch_records')
DUMP_MAX_BYTES = 64 << 20
DUMP_MASK_SAMPLES = 8192           # pixels of every RLE mask written by --dump-outputs (fixed seeded positions)


def mfma_terms(kernel: str):
    """(16-bit MFMA products per f32 product, peak of the pipe the kernel runs on in TFLOP/s)."""
    if kernel.startswith('conv_pw_x3_kernel'):
        return X3_TERMS, PEAK_BF16_MFMA_TFLOPS
    if kernel.startswith('conv_pw_h2_kernel'):
        return H2_TERMS, PEAK_BF16_MFMA_TFLOPS
    return 1, PEAK_FP32_MFMA_TFLOPS


def algorithmic_gflop(cfg, H, W, S, R, D):
    """Reference-formulation FLOPs per episode, 2 x MAC."""
    N, K = cfg['n_ways'], cfg['k_shots']

    def c4(h, w):
        mac = 0
        ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
        mac += ho * wo * 64 * 3 * 49
        ho, wo = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
        cin = 64
        for nblk, planes, stride in zip((3, 4, 6), (64, 128, 256), (1, 2, 2)):
            for b in range(nblk):
                s = stride if b == 0 else 1
                mac += ho * wo * cin * planes
                ho2, wo2 = (ho - 1) // s + 1, (wo - 1) // s + 1
                mac += ho2 * wo2 * planes * planes * 9 + ho2 * wo2 * planes * planes * 4
                if b == 0:
                    mac += ho2 * wo2 * cin * planes * 4
                ho, wo, cin = ho2, wo2, planes * 4
        return mac, ho, wo
    cq, h, w = c4(H, W)
    cs, _, _ = c4(S, S)
    sh = 3 * (2 * 1024 * 512 + 9 * 512 * 512) * 49
    mh = 49 * 9 * (1024 * 256 + 3 * 256 * 256) + 49 * 4 * 256 * 256 + 196 * 256
    mac = cq + N * K * cs + N * h * w * (9 * 1024 * 1024 + 75 * 1024) + (N * K + R + D) * sh + \
        R * N * 49 * 2048 * 1024 + R * N * 6 * 1024 + D * mh
    return 2 * mac / 1e9


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workload', default='cfg3')
    ap.add_argument('--full', action='store_true',
                    help='everything besides the headline: the conv roofline of event-stamped steps (an eagerly launched '
                         'isolated timed step, an overlapped warm-up step), the CPU baseline, the accuracy and trained-heads '
                         'legs against the CPU oracle, and the multi-rank check of the gathered results.  Without it a run '
                         'sets up, warms up, times --steps replayed steps and prints the line')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write the result dicts of the last one as DIR/<name>.npy (float32 / '
                         'float64): the same arguments give the same inputs, so two builds compare output for output')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-episodes', type=int, default=5, help='timed episodes of the CPU baseline (after 2 warm-up episodes)')
    ap.add_argument('--accuracy-episodes', type=int, default=0,
                    help='off the timed path: compare this many episodes HIP vs the CPU oracle (matched-pair maxima, '
                         'agreement AP at IoU 0.5 / 0.75 / 0.95); 0 = reuse the CPU-baseline episodes')
    ap.add_argument('--train-heads-steps', type=int, default=300,
                    help='off the timed path: overfit the heads on the accuracy episodes for this many Trainer steps '
                         '(frozen backbone, like the reference) so that AP against the synthetic ground truth is not '
                         '0 vs 0, then score HIP and the CPU oracle with those weights; 0 = skip')
    ap.add_argument('--trained-eval-episodes', type=int, default=3, help='episodes scored by both paths with the trained heads')
    ap.add_argument('--inflight', type=int, default=None, help='episodes queued ahead of result packing per GPU '
                    '(default: 3 with hipGraph replay, 1 without).  Measured on one box (r03, cfg3, two caller streams; '
                    'tools/micro/ab_inflight.sh): with 2 in flight the GPU holds a single episode while the host packs one '
                    'and replays the next - 177.7 img/s over 20 steps, 3 in flight 184.3, 4: 178.5, 6: 176.8 (filling '
                    'and draining a deeper queue weighs on a 20-step run); over 300 steps 186.5 / 191.6 / 193.7 / 193.1')
    ap.add_argument('--streams', type=int, default=None,
                    help='caller streams the steps alternate between: with 2, the low-occupancy phases of one episode '
                         '(selection kernels, small-grid launches, transforms) run beside the GEMMs of the next.  Measured '
                         '(r03, cfg3): 1 stream / 1 in flight 6.13 ms, 2 / 2 with graphs 5.76 ms; without graphs the host '
                         'cannot keep two streams fed (6.10 ms)')
    ap.add_argument('--graphs', dest='graphs', action='store_true', default=None,
                    help='replay one captured hipGraph per step instead of launching from Python (same kernels, same '
                         'bytes; host enqueue 0.2-0.8 ms instead of ~2.9 ms).  Default: on, at every batch.  Measured r04 on '
                         'one box, cfg4 shapes (tools/micro/sweep_batch.sh, profiles/r04_sweep_batch.txt): replay on two caller '
                         'streams with three steps in flight beats eager launches at every batch - B = 2 201 vs 181-188 '
                         'img/s, B = 4 (the reference evaluates with batch 4, fgn_test.py:49) 210-211 vs 193-196, B = 8 '
                         '212-213 vs 203-205; replay on ONE stream loses 2-5 % to eager (its kernels take the same time one by '
                         'one - rocprofv3, tools/micro/graph_vs_eager.sh - but the branches of one graph overlap less than '
                         'streams do).  A step holds 2.5 GiB (B = 4) / 4.6 GiB (B = 8) of the 288: pinned intermediates '
                         'are not a constraint')
    ap.add_argument('--no-graphs', dest='graphs', action='store_false')
    ap.add_argument('--batch', type=int, default=1, help='episodes per step per GPU (the reference evaluates with '
                    'batch 4, fgn_test.py:49; cfg4 of BASELINE.json is 8 per GPU); default 1 = cfg3 as surveyed')
    ap.add_argument('--no-winograd', action='store_true', help='direct implicit-GEMM form for every 3x3 convolution')
    ap.add_argument('--winograd', type=int, default=None, choices=(2, 4),
                    help='output tile edge of the Winograd form: 4 = F(4x4,3x3) (default), 2 = F(2x2,3x3)')
    ap.add_argument('--resident-inputs', action='store_true',
                    help='not the headline: park the inputs in HBM before timing (no host->device copy in the step)')
    ap.add_argument('--isolated-steps', default='last',
                    help="timed steps whose convolution launches are stamped with HIP events while they have the GPU to "
                         "themselves (queued behind the episodes in flight ON THE GPU, no host drain, the following steps "
                         "wait for them): 'last' (default: the final step, whose tail runs alone anyway), 'none', or a "
                         "comma list such as 5,20,35 (profiles/: three spread steps of a 60-step run; each costs the window "
                         "~1.5 ms of lost overlap)")
    ap.add_argument('--launch-records', action='store_true',
                    help='arm the launch records of the dominant kernel inside the captured graphs (roofline.timed_window: '
                         'every launch of every timed step on the in-kernel 100 MHz clock).  Off by default: a recorded launch '
                         'pays a returning atomic per workgroup at its exit, ~1 us per launch (measured r05: a first form '
                         'with all 1024 workgroups on one counter cost the step 4-7 %)')
    ap.add_argument('--cache-supports', action='store_true',
                    help='not the headline: encode each support set once (SURVEY 8f row 3) and time query passes only')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    full_only = ['--' + d.replace('_', '-') for d in FULL_ONLY if getattr(args, d) != ap.get_default(d)]
    if full_only and not args.full:
        ap.error(f'{", ".join(full_only)}: only with --full')
    if args.graphs is None:
        args.graphs = True
    if args.streams is None:
        args.streams = 2 if args.graphs else 1
    if args.inflight is None:
        args.inflight = 3 if args.graphs else 1
    return args


def under_profiler() -> bool:
    """rocprofv3 preloads its tool library into the profiled process (and, with --pmc, initialises the GPU before
    main()): starting a launcher from such a process is the exec-after-GPU-init hop this pool forbids."""
    blob = ' '.join(os.environ.get(k, '') for k in ('LD_PRELOAD', 'ROCP_TOOL_LIBRARIES', 'ROCPROFILER_REGISTER_LIBRARY'))
    return 'rocprof' in blob.lower() or any(k.startswith('ROCPROF') for k in os.environ)


# ---- host placement of the ranks: each rank pins itself to the cores next to its GPU BEFORE any GPU call -----------
def _cpulist(text: str) -> list:
    out = []
    for part in text.strip().split(','):
        if not part:
            continue
        a, _, b = part.partition('-')
        out.extend(range(int(a), int(b or a) + 1))
    return out


def gpu_local_cpus(sysfs: str = '/sys') -> list:
    """Per HIP device (KFD topology order, filtered by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES when those hold plain
    indices): the CPU list local to that GPU's PCIe root (sysfs ``local_cpulist`` of its DRM render node; NUMA node
    beside it).  Empty list for a device whose locality the kernel does not report.  Pure sysfs reads: no HIP call."""
    base = f'{sysfs}/class/kfd/kfd/topology/nodes'
    gpus = []
    try:
        nodes = sorted(os.listdir(base), key=int)
    except (OSError, ValueError):
        return []
    for n in nodes:
        try:
            props = dict(line.split() for line in open(f'{base}/{n}/properties') if len(line.split()) == 2)
        except OSError:
            continue
        if int(props.get('simd_count', 0)) <= 0:
            continue
        cpus, numa = [], -1
        try:
            dev = f"{sysfs}/class/drm/renderD{int(props['drm_render_minor'])}/device"
            cpus = _cpulist(open(dev + '/local_cpulist').read())
            numa = int(open(dev + '/numa_node').read())
        except (OSError, KeyError, ValueError):
            pass
        gpus.append(dict(kfd_node=int(n), cpus=cpus, numa=numa))
    for var in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES'):
        v = os.environ.get(var)
        if v and all(t.strip().isdigit() for t in v.split(',')):
            gpus = [gpus[int(t)] for t in v.split(',') if int(t) < len(gpus)]
    return gpus


def pin_rank(local_rank: int, local_world: int, sysfs: str = '/sys', apply: bool = True) -> dict:
    """Restrict this rank to its share of the host: the cores local to GPU ``local_rank``, split evenly among the
    ranks whose GPUs share those cores (all ranks of one socket see the same ``local_cpulist``); when the kernel
    reports no locality, an even contiguous split of the cores this process may use.  Also sizes the intra-op thread
    pools to the share (<= 8).  Called before torch touches the GPU."""
    allowed = sorted(os.sched_getaffinity(0))
    info = dict(policy='none', cpus=len(allowed))
    if local_world <= 1 or os.environ.get('FGN_BENCH_NO_PIN'):
        return info
    gpus = gpu_local_cpus(sysfs)
    mine = None
    if gpus:
        # rank -> GPU: one GPU per rank when there are enough, otherwise (a rehearsal of several ranks on one card, or
        # HIP_VISIBLE_DEVICES per rank) ranks wrap around; the cores of a cpulist are split among ALL ranks whose GPU
        # reports that list, so no two ranks ever get overlapping sets
        gpu_of = [r % len(gpus) for r in range(local_world)]
        g = gpus[gpu_of[local_rank]]
        if g['cpus']:
            local = [c for c in g['cpus'] if c in set(allowed)]
            sharers = [r for r in range(local_world) if gpus[gpu_of[r]]['cpus'] == g['cpus']]
            if local and len(local) >= len(sharers):
                k, n = sharers.index(local_rank), len(sharers)
                per = len(local) // n
                mine = local[k * per:(k + 1) * per]
                info = dict(policy='gpu-local', numa=g['numa'], sharers=n, gpu=gpu_of[local_rank])
    if mine is None:
        per = max(1, len(allowed) // local_world)
        mine = allowed[local_rank * per:(local_rank + 1) * per] or allowed
        info = dict(policy='even-split')
    info.update(cpus=len(mine), first_cpu=mine[0])
    if not apply:                 # tests: report the choice without changing this process
        info['cpu_list'] = mine
        return info
    try:
        os.sched_setaffinity(0, mine)
    except OSError as e:
        return dict(policy='failed', error=str(e), cpus=len(allowed))
    os.environ['OMP_NUM_THREADS'] = str(min(8, len(mine)))
    return info


def self_launch(args) -> int:
    """``python bench.py --gpus N`` (N > 1) outside torch.distributed.run: start the N ranks as a child job.  This
    process has not initialised the GPU (no HIP call so far), and it never does: it waits for the child and
    returns its exit code."""
    if under_profiler():
        raise SystemExit('bench.py --gpus N under rocprofv3 would start the launcher from the profiled process; '
                         'profile one rank: rocprofv3 ... -- python3 bench.py --gpus 1 ...')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '8')
    return subprocess.call(cmd, env=env)


def cpu_model() -> str:
    try:
        with open('/proc/cpuinfo') as fh:
            for line in fh:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def dump_outputs(results: list, out_dir: str) -> None:
    """--dump-outputs: the result dicts of one step, as ``FGN.pack_results`` hands them to its caller, written as
    ``out_dir/ep<i>_<key>.npy``.  Float arrays keep their dtype, integer arrays become float64 (exact).  A list of COCO
    RLE masks becomes ``<key>_area`` (pixels per mask) and ``<key>_sample`` (every mask at the same DUMP_MASK_SAMPLES
    seeded pixel positions, 0 / 1): a dense float32 800x1333 mask per detection would take 4 MB."""
    import numpy as np
    from fgn_amd import rle
    arrays = {}
    for i, res in enumerate(results):
        for key, val in res.items():
            if key.endswith('_rle'):
                masks = [rle.decode(r) for r in val]
                sample = np.zeros((0, DUMP_MASK_SAMPLES), np.float32)
                if masks:
                    h, w = masks[0].shape
                    pos = np.sort(np.random.default_rng(0).choice(h * w, DUMP_MASK_SAMPLES, replace=False))
                    sample = np.stack([m[pos // w, pos % w] for m in masks]).astype(np.float32)
                base = f'ep{i}_{key[:-len("_rle")]}'
                arrays[base + '_area'] = np.array([m.sum() for m in masks], np.float64)
                arrays[base + '_sample'] = sample
            elif val is not None:
                a = np.asarray(val)
                if a.dtype.kind in 'biuf':
                    arrays[f'ep{i}_{key}'] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f'--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte budget')
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)


def main():
    args = parse_args()
    if 'RANK' not in os.environ and 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))

    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    placement = pin_rank(local_rank, int(os.environ.get('LOCAL_WORLD_SIZE', world)))   # before any GPU call
    import torch
    if placement.get('policy') in ('gpu-local', 'even-split'):
        torch.set_num_threads(min(8, placement['cpus']))
    if world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks')
    # FGN_BENCH_BACKEND=gloo is a rehearsal mode for boxes with fewer GPUs than ranks (ranks share cuda:0 and
    # the collectives go through gloo): it checks the multi-rank control flow, not the scaling
    backend = os.environ.get('FGN_BENCH_BACKEND', 'nccl')
    n_vis = max(torch.cuda.device_count(), 1)      # (a launcher may restrict every rank to its own GPU)
    dev_index = local_rank if (backend == 'nccl' and local_rank < n_vis) else local_rank % n_vis
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        # a bounded collective timeout: a rank that died (or never arrived) must end the job with an error, not leave the
        # others inside an all-gather for the default 10-30 minutes (tests/test_host_cpu.py::test_a_failing_rank_...)
        import datetime
        pg_timeout = datetime.timedelta(seconds=int(os.environ.get('FGN_BENCH_PG_TIMEOUT', '300')))
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev, timeout=pg_timeout)
        else:
            dist.init_process_group(backend, timeout=pg_timeout)

    from fgn_amd import dist as fdist
    from fgn_amd import ops
    from fgn_amd.config import fgn_r50_c4_config, with_caps
    from fgn_amd.detector import FGN
    from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch
    from fgn_amd.weights import init_state_dict

    shape = CONFIGS[args.workload]
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    sd = init_state_dict(cfg, 0)
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=sd)
    model.use_graphs = bool(args.graphs)
    model.use_winograd = False if args.no_winograd else (args.winograd or True)
    if os.environ.get('FGN_MERGED_BACKBONE'):        # A/B knobs
        model.use_merged_backbone = os.environ['FGN_MERGED_BACKBONE'] != '0'
    if os.environ.get('FGN_MERGED_SUPPORT_HEAD'):
        model.use_merged_support_head = os.environ['FGN_MERGED_SUPPORT_HEAD'] != '0'
    if os.environ.get('FGN_SIDE_STREAM'):
        model.use_side_stream = os.environ['FGN_SIDE_STREAM'] != '0'
    if os.environ.get('FGN_PACKED_TRANSFERS'):
        model.use_packed_transfers = os.environ['FGN_PACKED_TRANSFERS'] != '0'

    # distinct seeded episodes per rank in PINNED host memory (what a DataLoader with pin_memory hands over);
    # every step copies its episode to the device (--resident-inputs: parked in HBM instead, not the headline)
    n_distinct = 4
    episodes = []
    for j in range(n_distinct):
        b = make_batch((rank * n_distinct + j) * args.batch, args.batch, **shape)
        place = (lambda t: t.to(dev)) if args.resident_inputs else (lambda t: t.pin_memory())
        e = {k: (place(v) if isinstance(v, torch.Tensor) else [place(t) for t in v] if isinstance(v, list) else v)
             for k, v in b.items()}
        e['img_shape'] = b['img_shape']            # shape metadata is host data in the reference too
        e['code'] = None
        if args.cache_supports:
            e['code'] = model.encode_supports(b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'])
        episodes.append(e)

    max_det = cfg['test_cfg']['rcnn']['max_per_img']
    # Hardware-queue budget: HIP maps streams onto four hardware queues (GPU_MAX_HW_QUEUES) in stream-creation
    # order, work of streams that share a queue runs in order, and a stream that waits for another queue's event blocks
    # whatever shares its queue.  More queues are NOT better: 2 / 3 / 4 / 5 / 6 / 8 queues give 170 / 172 / 190 / 114 /
    # 142 / 138 img/s, transfer streams in the high-priority pool 140 (profiles/r04_hw_queues.txt).  The fewer streams an
    # episode touches, the fewer cross-queue waits it pays:
    # (graph mode only: an eager episode uploads its inputs on the upload stream one episode ahead, which needs that stream)
    # Measured r04 (profiles/r04_hw_queues.txt): with one episode per step every cross-queue wait counts - the transfers of
    # an episode on its own caller stream (mode 3: no upload / copy streams at all) 196.6-198.3 img/s against 190.5-192.1
    # with an upload and a copy stream per caller, over 200 steps (the driver's 20-step window: equal); at 4 / 8 episodes
    # per step the transfers are larger and the separate streams are equal or 1 % better.
    xfer_mode = int(os.environ.get('FGN_XFER_MODE', '3' if args.batch <= 2 else '0'))
    if args.graphs and xfer_mode:
        model.transfer_stream(xfer_mode)
    comm_stream = torch.cuda.Stream() if world > 1 else None
    if world > 1 and backend == 'nccl':
        # RCCL runs a collective on an internal stream of its own, which takes the next hardware queue when it is first
        # used.  One warm-up collective HERE - after the communication stream, before the caller streams exist - gives
        # that stream a queue no caller stream shares: an all-gather that waits for a late rank then blocks nobody's
        # compute (same reasoning as for the transfer streams above).
        with torch.cuda.stream(comm_stream):
            warm = torch.zeros(1, device=dev)
            dist.all_reduce(warm)
        comm_stream.synchronize()
    ep_streams = [torch.cuda.Stream() for _ in range(args.streams)] if args.streams > 1 else [None]
    # Phase lock of the two caller streams (FGN.phase_counter / phase_point, detector.py).  Two streams that replay
    # episodes side by side settle in one of several steady states of their relative phase - the same binary on the same
    # box ran 192-195 img/s in most runs and 203 in some, and small changes of the stream set-up flipped it one way or the
    # other (profiles/r04_phase_lock.txt).  With the lock an episode starts when the previous one, on the other stream,
    # has passed a mark at the end of its backbone ('rpn': present on every path through the detector, the support cache
    # included): every run then sits in the fast state - one episode per step
    # 192-195 -> 202-203 img/s over 200 steps (186-190 -> 194-197 in the driver's 20-step window), two per step
    # 192.6 -> 213.6; marks from 'layer1' to 'rpn' are equal, 'rpn_conv' / 'proposals' / 'mask' are worse (197 / 200 /
    # 185).  At 4 / 8 episodes per step the lock needs the transfers on the caller streams (FGN_XFER_MODE=3) and then
    # gives 209 -> 217 / 213.5 -> 220; it is left off there by default because that arrangement disturbs the isolated
    # instrumented step the roofline is taken from (its transforms and GEMMs run 10-25 % longer - not yet explained).
    # FGN_BENCH_PHASE=off disables, =<mark> selects.
    phase_point = os.environ.get('FGN_BENCH_PHASE', 'rpn' if (args.batch <= 2 and args.graphs and args.streams == 2) else '')
    if phase_point in ('off', '0', 'none'):
        phase_point = ''
    # (armed after the warm-up: the counters' values are read once, behind a synchronisation, and counted on the host
    # from there - every launch bumps its stream's counter exactly once)
    phase_counters = torch.zeros(2, device=dev, dtype=torch.int32) if (phase_point and len(ep_streams) == 2) else None
    if phase_counters is not None:
        model.phase_point = phase_point          # which point of the episode sends the mark; the counter travels per call
    phase_armed, phase_base, phase_sent, phase_skip = [False], [0, 0], [0, 0], set()
    gathered_last = {}
    gather_on_compute = bool(os.environ.get('FGN_BENCH_GATHER_ON_COMPUTE'))
    gather_pool = None
    if world > 1 and backend == 'gloo':
        # rehearsal backend: gloo has no device collective, so the records go through the host.  Done inline that is
        # a host-blocking D2H + all-gather in the launch loop (every rank's HOST then runs in lockstep, which RCCL
        # does not do: its all-gather is enqueued and the host moves on).  A single worker thread per rank keeps the
        # rehearsal's host side shaped like the real thing: collectives are issued in step order, the launch loop
        # does not wait for them.
        from concurrent.futures import ThreadPoolExecutor
        gather_pool = ThreadPoolExecutor(max_workers=1)

    def gather(recs, cnts):
        if gather_pool is None or gather_on_compute:
            return fdist.gather_detections(recs, cnts)
        ready = torch.cuda.current_stream().record_event()

        def work():
            torch.cuda.set_device(dev)
            ready.synchronize()
            with torch.cuda.stream(comm_stream):
                return fdist.gather_detections(recs, cnts)
        return gather_pool.submit(work)

    gather_events, gather_timed = [], []      # timing events of the collectives (created before the timed region)
    jitter_ms = float(os.environ.get('FGN_BENCH_JITTER_MS', '0'))     # rehearsal: rank r is late once every `world` steps

    def launch(i, profile=None):
        """Queue one step's device work (asynchronous): H2D of the episode, the whole path, D2H of the results."""
        e = episodes[i % n_distinct]
        if jitter_ms and world > 1 and i % world == rank:
            time.sleep(jitter_ms * 1e-3)
        ops.PROFILE = profile
        st = ep_streams[i % len(ep_streams)]
        ctx = torch.cuda.stream(st) if st is not None else contextlib.nullcontext()
        try:
            with ctx:
                mark = None
                if phase_counters is not None:
                    # phase lock of the two caller streams: this episode starts when the previous one (on the other
                    # stream) has passed its mark; its own mark releases the next one
                    k_ = i % 2
                    if phase_armed[0] and i not in phase_skip:
                        ops.phase_wait(phase_counters[1 - k_:2 - k_], phase_base[1 - k_] + phase_sent[1 - k_])
                    mark = phase_counters[k_:k_ + 1]
                    phase_sent[k_] += 1
                dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'],
                                           e['img_shape'], support_code=e['code'], qry_isegmaps=e['qry_isegmaps'],
                                           phase_counter=mark)
        finally:
            ops.PROFILE = None
        if world > 1:
            # one RCCL all-gather of fixed-size padded records (boxes, scores, labels, mask probabilities) per step.
            # The records are packed on the CALLER stream - five small copies out of the episode's output buffers,
            # which a replayed hipGraph overwrites with its next replay, into fresh memory - and the collective itself
            # runs on the communication stream behind an event: the next episode's kernels never queue behind it, so a
            # rank that runs a step late delays the others' gathered results, not their compute (eager and graph
            # mode alike; FGN_BENCH_GATHER_ON_COMPUTE=1 puts it back on the caller stream for the A/B of
            # tools/rehearse_jitter.sh)
            with ctx:
                recs, cnts = fdist.pack_detections(dets, max_det)
                packed = torch.cuda.current_stream().record_event()
            if gather_on_compute:
                with ctx:
                    gathered_last['g'] = gather(recs, cnts)
            else:
                comm_stream.wait_event(packed)
                with torch.cuda.stream(comm_stream):
                    # the collective's own duration on the communication stream (gather_ms_p50 / p99 of the line: a rank
                    # that waits for a late peer shows here, not in its compute)
                    ev = (gather_events.pop(), gather_events.pop()) if len(gather_events) >= 2 else None
                    if ev is not None:
                        ev[0].record()
                    gathered_last['g'] = gather(recs, cnts)
                    if ev is not None and gather_pool is None:
                        ev[1].record()
                        gather_timed.append(ev)
                recs.record_stream(comm_stream)
                cnts.record_stream(comm_stream)
        return e, dets

    latencies = []        # seconds from the start of an episode's launch to its packed result dicts (host clock)

    def finish(pending):
        e, dets = pending[0], pending[1]
        out = model.pack_results(dets, args.batch, qry_bboxes=e['qry_bboxes'], qry_cat_ids=e['qry_cat_ids'],
                                 qry_isegmaps=e['qry_isegmaps'], img_shape=e['img_shape'], idx=e['idx'])
        if len(pending) > 2:
            latencies.append(time.perf_counter() - pending[2])
        return out

    def run(n_steps, prof=None, prof_steps=(), alone=None):
        """Software-pipelined: episode i+1 is queued before the results of episode i are packed,
        so host-side result packing overlaps device work.  Every result is still delivered.
        ``prof`` / ``prof_steps``: steps whose conv launches are event-stamped while the pipeline runs as usual;
        ``alone``: {step: ConvProfile} - steps that are event-stamped while they have the GPU to themselves: the step
        is queued behind every episode in flight ON THE GPU (its caller stream waits for their completion events; the
        host does not drain, so the GPU never idles in front of it and its clocks are those of the running pipeline)
        and the compute of the following steps waits for it; its kernels share the chip with nothing but their own
        side stream."""
        n_det = n_gt = 0
        pending = []
        last = None
        alone = alone or {}
        for i in range(n_steps):
            t_a = time.perf_counter()
            if i in alone:
                st_i = ep_streams[i % len(ep_streams)]
                st_i = st_i if st_i is not None else torch.cuda.current_stream()
                for pe in pending:
                    st_i.wait_event(pe[1][0]['host_ready'])
                phase_skip.update(range(i, i + 1 + args.inflight))     # no phase wait in or right behind an isolated step
                pending.append(launch(i, alone[i]) + (t_a,))
                for st in ep_streams:
                    (st if st is not None else torch.cuda.current_stream()).wait_event(pending[-1][1][0]['host_ready'])
            else:
                pending.append(launch(i, prof if (prof is not None and i in prof_steps) else None) + (t_a,))
            if len(pending) > args.inflight:
                last = finish(pending.pop(0))
                n_det += sum(len(r['dt_scores']) for r in last)
                n_gt += sum(len(r['qry_isegmaps_rle']) for r in last)
        while pending:
            last = finish(pending.pop(0))
            n_det += sum(len(r['dt_scores']) for r in last)
            n_gt += sum(len(r['qry_isegmaps_rle']) for r in last)
        return n_det, n_gt, last

    # setup (not a warm-up step): pack the weights for the device, fill the caching allocator's pools,
    # pin the host slots and let every kernel set its LDS attribute once
    prime = ops.ConvProfile()
    n_setup = 2 * len(ep_streams)         # every caller stream captures its hipGraph here, not in a warm-up / timed step
    model.stamp_capacity = 256 if args.launch_records else 0     # launch records of the dominant kernel inside the graphs
    run(n_setup + 1, prof=prime, prof_steps=(n_setup,))   # also creates the first timing events (a one-time ~40 ms in HIP)
    # Instrumentation (timing events are created here, outside the timed region: HIP grows its event pool in bursts that
    # cost tens of ms):
    #  * every launch of the dominant kernel in EVERY timed step adds its span to a launch record inside the kernel
    #    (in-kernel 100 MHz stamps, first workgroup start -> last workgroup end: works inside the replayed graphs at two
    #    atomics per workgroup) -> `roofline.timed_window`: the untraced pipeline (a rocprofv3 kernel trace slows the step
    #    to ~6 ms and its launches hardly overlap: its averages are the isolated regime's);
    #  * `--isolated-steps` (default: the last timed step) are launched eagerly with a start / stop HIP event pair per
    #    convolution launch while they have the GPU to themselves -> `roofline.achieved / frac / by_kernel /
    #    launch_classes`.  Rounds 1-4 instrumented step 0 - the first work after the barrier's device synchronisation, on
    #    an idle chip: its launches read 5 % longer than the same launches anywhere else;
    #  * one warm-up step is event-stamped while episodes overlap (`roofline.overlapped`, informational).
    # All of it is --full only: a plain run's warm-up and timed steps are the replayed pipeline and nothing else.
    if not args.full or args.isolated_steps == 'none':
        alone_steps = []
    elif args.isolated_steps == 'last':
        alone_steps = [args.steps - 1]
    else:
        alone_steps = sorted({int(t) for t in args.isolated_steps.split(',') if t.strip() != '' and 0 <= int(t) < args.steps})
    overlapped_in_warmup = args.full and args.warmup >= 3
    prof_steps = [] if (overlapped_in_warmup or not args.full) else \
        ([args.steps // 2] if args.steps >= 4 and (args.steps // 2) not in alone_steps else [])
    prof = ops.ConvProfile()                                         # overlapped step
    if args.full:
        prof.reserve(2 * len(prime) + 16)
    prof_alone = {i: ops.ConvProfile().reserve(2 * len(prime) + 16) for i in alone_steps}      # isolated steps -> roofline
    for pr in [prof] + list(prof_alone.values()):
        for ev in pr.pool:
            ev.record()
    if world > 1:
        gather_events.extend(torch.cuda.Event(enable_timing=True) for _ in range(2 * (args.steps + args.warmup + 2)))
        for ev in gather_events:
            ev.record()
    # (Measured, r03: a Python garbage collection never fell into the 20-step window - collector on / off 185.5 / 184.4
    # img/s -, but an IDLE GPU right before it does cost: a gc.collect() of ~50 ms placed between the warm-up and the timed
    # region took 2.5 % off the 20 steps, the first of which then ran at a lower clock.  Nothing sits between the warm-up
    # steps and the timed region but the barrier.)
    if overlapped_in_warmup:
        run(args.warmup, prof, prof_steps=[max(1, args.warmup - 3)])     # two more steps queue up behind it
    else:
        run(args.warmup)

    def barrier():
        g = gathered_last.get('g')
        if hasattr(g, 'result'):      # gloo rehearsal: the worker thread's collectives are done before the main thread's
            g.result()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    if phase_counters is not None:
        phase_base[:] = [int(v) for v in phase_counters.tolist()]
        phase_sent[:] = [0, 0]
        phase_armed[0] = True
        phase_skip.clear()
    graphs = list(model._graphs.values())
    for ge in graphs:                      # launch records: forget the set-up and warm-up replays
        if ge.stamps is not None:
            ops.reset_stamps(ge.stamps)
    gather_timed.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # in the instrumented steps every convolution kernel launch stamps a start/stop HIP event pair
    # (hipExtLaunchKernelGGL: the kernel's own duration, on the stream it runs on)
    latencies.clear()
    n_d, n_gt, last_results = run(args.steps, prof, prof_steps=prof_steps, alone=prof_alone)
    timed_latencies = sorted(latencies)
    barrier()
    dt = time.perf_counter() - t0
    per_rank_dt = [dt]
    rank_info = [dict(rank=rank, **placement)]
    if world > 1:
        # every rank's own wall time of the K steps and its host placement, gathered after the timed region;
        # `value` uses the MAX over ranks
        t = torch.zeros(world, device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
        t[rank] = dt
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        per_rank_dt = [float(v) for v in t.cpu()]
        dt = max(per_rank_dt)
        try:
            gathered_info = [None] * world
            dist.all_gather_object(gathered_info, dict(rank=rank, **placement))
            rank_info = gathered_info
        except Exception as e:       # diagnostics must never cost the bench line
            rank_info = [dict(rank=rank, **placement), {'gather_error': f'{type(e).__name__}: {e}'}]
    if args.dump_outputs and rank == 0:
        dump_outputs(last_results, args.dump_outputs)
    roofline = None
    if args.full:
        n_prof_steps = 1

        # ---- roofline of the dominant kernel, from the HIP events recorded live ----------------------------------
        def per_kernel(records):
            out = {}
            for rec in records:
                ms = rec['e0'].elapsed_time(rec['e1'])
                n = rec['n_img'] if rec['n_img_dev'] is None else min(rec['n_img'], int(rec['n_img_dev'].item()))
                k = out.setdefault(rec['kernel'], dict(ms=0.0, launches=0, issued=0.0, direct=0.0))
                k['ms'] += ms
                k['launches'] += 1
                k['issued'] += rec['flop_issued'] * n
                k['direct'] += rec['flop_direct'] * n
            return out
        def launch_classes(records, kernel):
            """The launches of one kernel split by what bounds them on paper: algorithmic bytes of a launch = (A + B + C
            (+ residual)) x 4 B, arithmetic intensity = issued FLOP / those bytes, against the machine balance 157.3 TF/s /
            8 TB/s = 19.7 FLOP/B.  A 1x1 convolution with K = 64 writes 4 bytes per 128 FLOP of its row: no MFMA rate
            can make it faster than its output stream."""
            out = {'mfma_bound': dict(launches=0, ms=0.0, flop=0.0, bytes=0.0), 'hbm_bound': dict(launches=0, ms=0.0, flop=0.0, bytes=0.0)}
            # f32-equivalent MFMA ceiling of the kernel: the f32 pipe, or the bf16 pipe at six products per f32 product
            peak_eq = mfma_terms(kernel)[1] / mfma_terms(kernel)[0]
            for rec in records:
                if rec['kernel'] != kernel or 'gemm' not in rec:
                    continue
                n = rec['n_img'] if rec['n_img_dev'] is None else min(rec['n_img'], int(rec['n_img_dev'].item()))
                g, rows, N, K = rec['gemm']
                M = rows * n if rec['kind'] == 'conv' else rows
                byts = 4.0 * g * (M * K + N * K + M * N * (2 if rec.get('residual') else 1))
                flop = rec['flop_issued'] * n
                c = out['mfma_bound' if flop / max(byts, 1.0) >= peak_eq / 8.0 else 'hbm_bound']
                c['launches'] += 1
                c['ms'] += rec['e0'].elapsed_time(rec['e1'])
                c['flop'] += flop
                c['bytes'] += byts
            res = {}
            for k, c in out.items():
                if c['launches']:
                    res[k] = {'launches': c['launches'], 'ms': round(c['ms'], 3), 'tflops': round(c['flop'] / c['ms'] / 1e9, 1),
                              'frac_of_mfma_peak': round(c['flop'] / c['ms'] / 1e9 / peak_eq, 4),
                              'algorithmic_tb_per_s': round(c['bytes'] / c['ms'] / 1e9, 2),
                              'frac_of_hbm_peak': round(c['bytes'] / c['ms'] / 1e9 / 8.0, 4)}
            return res
        by_kernel_overlapped = per_kernel(prof)
        # the isolated steps: the dominant kernel is the one with the largest summed duration; `roofline` reports the MEDIAN
        # isolated step (by the dominant kernel's time), the others as min / max
        iso = {i: per_kernel(pr) for i, pr in prof_alone.items() if len(pr)}
        dom_votes = [max(bk, key=lambda n: bk[n]['ms']) for bk in iso.values()]
        dom_name = max(set(dom_votes), key=dom_votes.count) if dom_votes else \
            (max(by_kernel_overlapped, key=lambda n: by_kernel_overlapped[n]['ms']) if by_kernel_overlapped else 'none')
        iso_order = sorted(iso, key=lambda i: iso[i].get(dom_name, {'ms': 0.0})['ms'])
        med_step = iso_order[len(iso_order) // 2] if iso_order else None
        by_kernel = iso[med_step] if med_step is not None else by_kernel_overlapped
        records_med = prof_alone[med_step] if med_step is not None else prof
        tot = dict(ms=sum(k['ms'] for k in by_kernel.values()), launches=sum(k['launches'] for k in by_kernel.values()),
                   issued=sum(k['issued'] for k in by_kernel.values()), direct=sum(k['direct'] for k in by_kernel.values()))
        dom = by_kernel.get(dom_name, dict(ms=0.0, launches=0, issued=0.0, direct=0.0))
        tf = lambda flop, ms: flop / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # conv_pw_x3_kernel issues X3_TERMS bf16 MFMA products per f32 product of its GEMM: its roofline is the bf16 pipe,
        # `achieved` the bf16 MFMA FLOPs it issued per second; the f32 products per second are reported beside it
        dom_terms, dom_peak = mfma_terms(dom_name)
        dom_x3 = dom_terms > 1               # a kernel on the 16-bit matrix pipe (conv_pw_x3_kernel / conv_pw_h2_kernel)
        achieved = tf(dom['issued'], dom['ms']) * dom_terms
        iso_table = [dict(step=i, kernel_ms=round(iso[i][dom_name]['ms'], 4), launches=iso[i][dom_name]['launches'],
                          avg_launch_us=round(iso[i][dom_name]['ms'] * 1e3 / max(iso[i][dom_name]['launches'], 1), 2),
                          frac=round(tf(iso[i][dom_name]['issued'], iso[i][dom_name]['ms']) * dom_terms / dom_peak, 4),
                          all_conv_ms=round(sum(k['ms'] for k in iso[i].values()), 3))
                     for i in sorted(iso) if dom_name in iso[i]]

        # ---- the dominant kernel over the WHOLE timed window: the launch records inside the captured graphs --------------
        window = None
        # launch records are handed out in launch order to every launch of the two persistent GEMM kernels (f32 and x3)
        takes_record = lambda rec: rec['kernel'] == 'conv_pw_persist_kernel' or mfma_terms(rec['kernel'])[0] > 1
        rec_sites = [rec for rec in records_med if takes_record(rec)]
        keep = [i for i, rec in enumerate(rec_sites) if rec['kernel'] == dom_name]
        sites = [rec_sites[i] for i in keep]
        if model.use_graphs and sites and (dom_name == 'conv_pw_persist_kernel' or dom_x3):
            per_site = [dict(executions=0, total_us=0.0, min_us=None, max_us=None) for _ in sites]
            # (a graph whose captured launch sequence does not have the isolated step's launch sites cannot be matched)
            ok = bool(graphs) and all(ge.stamps is not None and ge.stamp_count == len(rec_sites) for ge in graphs)
            for ge in graphs if ok else []:
                all_recs = ops.read_stamps(ge.stamps, ge.stamp_count)
                for a, b in zip(per_site, [all_recs[i] for i in keep]):
                    a['executions'] += b['executions']
                    a['total_us'] += b['total_us']
                    if b['executions']:
                        a['min_us'] = b['min_us'] if a['min_us'] is None else min(a['min_us'], b['min_us'])
                        a['max_us'] = b['max_us'] if a['max_us'] is None else max(a['max_us'], b['max_us'])
            n_exec = sum(a['executions'] for a in per_site)
            if ok and n_exec:
                flop_of = []
                for rec in sites:
                    n = rec['n_img'] if rec['n_img_dev'] is None else min(rec['n_img'], int(rec['n_img_dev'].item()))
                    flop_of.append(rec['flop_issued'] * n)
                w_us = sum(a['total_us'] for a in per_site)
                w_flop = sum(f * a['executions'] for f, a in zip(flop_of, per_site))
                ratios = sorted(a['total_us'] / a['executions'] / (1e3 * r['e0'].elapsed_time(r['e1']))
                                for a, r in zip(per_site, sites) if a['executions'] and r['e0'].elapsed_time(r['e1']) > 0)
                window = {'what': 'EVERY launch of the kernel in the timed region (all steps, both caller streams, inside the '
                                  'replayed hipGraphs): span first workgroup start -> last workgroup end on the 100 MHz '
                                  'in-kernel clock, folded into a launch record by the kernel itself (fgn_profile_stamps): the '
                                  'launches as they run in the untraced pipeline, beside the other caller stream',
                          'launches': n_exec, 'launch_sites_per_step': len(sites),
                          'executions_per_site': sorted({a['executions'] for a in per_site}),
                          'avg_launch_us': round(w_us / n_exec, 2),
                          'achieved': round(w_flop / w_us / 1e6 * dom_terms, 2),
                          'frac': round(w_flop / w_us / 1e6 * dom_terms / dom_peak, 4),
                          'site_us_over_isolated_event_us': ({'p10': round(ratios[len(ratios) // 10], 3), 'p50': round(ratios[len(ratios) // 2], 3),
                                                              'p90': round(ratios[(len(ratios) * 9) // 10], 3)} if ratios else None),
                          'largest_site': (lambda k: {'avg_us': round(per_site[k]['total_us'] / per_site[k]['executions'], 1),
                                                      'min_us': per_site[k]['min_us'], 'max_us': per_site[k]['max_us'],
                                                      'isolated_event_us': round(1e3 * sites[k]['e0'].elapsed_time(sites[k]['e1']), 1)})(
                              max(range(len(sites)), key=lambda k: flop_of[k]))}

        # HBM traffic of the dominant kernel: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this same command
        # (tools/profile_round.sh), corrected per MI355X_MICROARCH.md; PMC collection serialises kernels, so it is
        # read from the committed profile, not collected inside the timed run
        traffic = None
        pdir = os.path.join(ROOT, 'profiles')
        tfiles = sorted(f for f in os.listdir(pdir) if f.endswith('conv_traffic.json')) if os.path.isdir(pdir) else []
        if tfiles and args.workload == 'cfg3' and args.batch == 1:
            with open(os.path.join(pdir, tfiles[-1])) as fh:
                tj = json.load(fh)
            per = tj.get('per_kernel', {})
            hit = [v for name, v in per.items() if name.replace(' ', '') == dom_name.replace(' ', '')]
            traffic = hit[0]['hbm_bytes_per_launch'] if hit else None
        # frac = MFMA FLOPs the dominant kernel actually ISSUED / its summed HIP-event launch durations / peak.
        # Reproducible from profiles/rNN_kernel_stats.csv: flop_per_step * steps / TotalDurationNs of `kernel`.
        roofline = {'bound': 'mfma', 'kernel': dom_name,
                    'achieved': round(achieved, 2), 'peak': dom_peak, 'unit': 'TFLOP/s',
                    'frac': round(achieved / dom_peak, 4),
                    'traffic': traffic,
                    'mfma': ('v_mfma_f32_16x16x32_f16: %d f16 products per f32 product of the GEMM (two-way splits of the '
                             'power-of-two scaled f32 operands, f32 accumulation); achieved / peak are f16 MFMA FLOP/s' % H2_TERMS)
                            if dom_name.startswith('conv_pw_h2_kernel') else
                            ('v_mfma_f32_16x16x32_bf16: %d bf16 products per f32 product of the GEMM (exact 3-way splits of '
                             'both f32 operands, f32 accumulation); achieved / peak are bf16 MFMA FLOP/s' % X3_TERMS) if dom_x3
                            else 'v_mfma_f32_16x16x4_f32 (f32 operands)',
                    # the GEMM's own (f32) products per second, and against the f32-input MFMA peak this kernel no
                    # longer runs on - above 1.0 means faster than any f32-MFMA kernel could be
                    'f32_equivalent_tflops': round(achieved / dom_terms, 2),
                    'f32_equivalent_over_f32_mfma_peak': round(achieved / dom_terms / PEAK_FP32_MFMA_TFLOPS, 4),
                    'flop_per_step': round(dom['issued'] / n_prof_steps),
                    'launches_per_step': dom['launches'] / n_prof_steps,
                    'avg_launch_us': round(dom['ms'] * 1e3 / max(dom['launches'], 1), 2),
                    'kernel_ms_per_step': round(dom['ms'] / n_prof_steps, 3),
                    'share_of_conv_time': round(dom['ms'] / tot['ms'], 3) if tot['ms'] else None,
                    # `frac` is the average over ALL launches of the kernel; split by the bound a launch has on
                    # paper (arithmetic intensity against 157.3 TF/s / 8 TB/s): the MFMA-bound ones against the
                    # MFMA peak, the output-bound 1x1 convolutions of layer1 / layer2 against the HBM peak
                    'launch_classes': launch_classes(records_med, dom_name),
                    'profiled_steps': n_prof_steps,
                    'timing': 'start/stop HIP events stamped by each launch of the kernel itself (hipExtLaunchKernelGGL) on '
                              'its own stream, in the isolated timed step(s) below: queued behind the episodes in flight '
                              'on the GPU (no idle chip in front of them), no other episode beside them (their own side '
                              'stream only).  With several isolated steps this is the MEDIAN one',
                    'isolated_steps': iso_table,
                    'frac_min_max_over_isolated_steps': ([min(r_['frac'] for r_ in iso_table), max(r_['frac'] for r_ in iso_table)]
                                                         if iso_table else None),
                    'timed_window': window,
                    # the same kernel in a mid-run step, while two episodes overlap on the two caller streams (the
                    # way the other steps run): launches share the CUs with another episode's kernels
                    'overlapped': (lambda k: None if not k or not k['ms'] else {
                        'avg_launch_us': round(k['ms'] * 1e3 / max(k['launches'], 1), 2),
                        'achieved': round(tf(k['issued'], k['ms']), 2),
                        'frac': round(tf(k['issued'], k['ms']) * dom_terms / dom_peak, 4),
                        'all_conv_ms_per_step': round(sum(v['ms'] for v in by_kernel_overlapped.values()), 3),
                        'measured_in': 'a warm-up step with steps queued before and behind it' if overlapped_in_warmup else 'a mid-run timed step',
                        'what': 'per-launch durations while another episode runs on the second caller stream: '
                                'not a kernel-quality figure'})(by_kernel_overlapped.get(dom_name)),
                    # every MFMA FLOP issued in a step over the wall time of a step (all kernels, all gaps)
                    'whole_step': {'issued_gflop': round(tot['issued'] / 1e9, 1),
                                   'tflops': round(tot['issued'] / (dt / args.steps) / 1e12, 2),
                                   'frac': round(tot['issued'] / (dt / args.steps) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)},
                    'all_conv_launches': {
                        'what': 'every convolution-family kernel of a step (implicit-GEMM kernels, Winograd transforms, '
                                'split-K reduces)',
                        'ms_per_step': round(tot['ms'] / n_prof_steps, 3),
                        'launches_per_step': tot['launches'] / n_prof_steps,
                        'issued_gflop_per_step': round(tot['issued'] / n_prof_steps / 1e9, 1),
                        'issued_tflops': round(tf(tot['issued'], tot['ms']), 2),
                        'issued_frac': round(tf(tot['issued'], tot['ms']) / PEAK_FP32_MFMA_TFLOPS, 4),
                        'direct_form_gflop_per_step': round(tot['direct'] / n_prof_steps / 1e9, 1),
                        'direct_form_tflops_not_a_utilisation_figure': round(tf(tot['direct'], tot['ms']), 2)},
                    'by_kernel': [dict(kernel=n, ms_per_step=round(k['ms'] / n_prof_steps, 3),
                                       launches_per_step=k['launches'] / n_prof_steps,
                                       issued_gflop_per_step=round(k['issued'] / n_prof_steps / 1e9, 1),
                                       issued_tflops=round(tf(k['issued'], k['ms']), 1))
                                  for n, k in sorted(by_kernel.items(), key=lambda kv: -kv[1]['ms'])]}

    if rank == 0:
        R = cfg['test_cfg']['rpn']['max_per_img']
        gflop = algorithmic_gflop(cfg, shape['height'], shape['width'], shape['spp_size'], R, n_d / args.steps / args.batch)
        if args.cache_supports:     # support backbone + support shared_head leave the timed step
            gflop -= algorithmic_gflop(cfg, 0, 0, shape['spp_size'], 0, 0)
        h2d_bytes = sum(t.numel() * t.element_size() for k in ('qry_img', 'spp_imgs', 'spp_bboxes', 'spp_isegmaps')
                        for t in [episodes[0][k]]) + sum(t.numel() for t in episodes[0]['qry_isegmaps'])
        out = {
            'metric': 'query-imgs/sec (3-way 3-shot, 800x1333 FGN simple_test)',
            'value': world * args.steps * args.batch / dt,
            'unit': 'img/s',
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': dt / args.steps * 1e3,
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,
            'dtype': 'f32',
            # operands, accumulation, epilogues and results are f32 in every setting; 'h2' (default) computes the GEMM-shaped
            # launches' products as three f16 MFMA products of two-way splits of the power-of-two scaled operands, 'x3' as
            # six bf16 MFMA products of exact three-way splits (both: the error against fp64 of the f32 MFMA kernels,
            # tests/test_hip_conv.py::test_h2_* / test_x3_*), 'f32' (FGN_GEMM_MATH=f32) on the f32-input MFMA
            'gemm_math': ops.GEMM_MATH,
            'data': 'synthetic',
            'config': {'workload': f'{args.workload}: {DATASET.get(args.workload, "synthetic")} {shape["n_ways"]}-way {shape["k_shots"]}-shot, '
                                   f'query 3x{shape["height"]}x{shape["width"]}, supports '
                                   f'{shape["n_ways"] * shape["k_shots"]}x3x{shape["spp_size"]}^2, ResNet-50-C4, '
                                   f'R<={R} proposals, D<={max_det} detections, {args.batch} episode(s) per GPU per step',
                       'h2d_in_step': not args.resident_inputs, 'h2d_bytes_per_step': h2d_bytes,
                       'gt_mask_rle_in_step': True, 'gt_masks_per_step': n_gt / args.steps,
                       'world_size_seen': world, 'collective_backend': backend if world > 1 else None,
                       # read back from the process group, not from the command line
                       'rccl_world_size': (dist.get_world_size() if (world > 1 and dist.get_backend() == 'nccl') else None),
                       'process_group': ({'backend': dist.get_backend(), 'world_size': dist.get_world_size()}
                                         if world > 1 else None),
                       # host clock, launch of an episode -> its packed result dicts, with `inflight` episodes queued
                       # ahead of packing (the pipelined mode of this bench: ~inflight x ms_per_step; not the metric)
                       'episode_latency_ms': ({'p50': round(timed_latencies[len(timed_latencies) // 2] * 1e3, 2),
                                               'p95': round(timed_latencies[min(len(timed_latencies) - 1, int(len(timed_latencies) * 0.95))] * 1e3, 2),
                                               'max': round(timed_latencies[-1] * 1e3, 2), 'episodes_in_flight': args.inflight}
                                              if timed_latencies else None),
                       'per_rank_ms_per_step': {'min': round(min(per_rank_dt) / args.steps * 1e3, 3),
                                                'max': round(max(per_rank_dt) / args.steps * 1e3, 3),
                                                'all': [round(v / args.steps * 1e3, 3) for v in per_rank_dt]},
                       'rank_placement': rank_info,
                       # the collective's own duration on the communication stream, per timed step (HIP events around it)
                       'gather_ms': ((lambda v: {'p50': round(v[len(v) // 2], 3), 'p99': round(v[min(len(v) - 1, int(len(v) * 0.99))], 3),
                                                 'max': round(v[-1], 3), 'steps': len(v)})(
                           sorted(a.elapsed_time(b) for a, b in gather_timed)) if gather_timed else None),
                       # with one rank there is no process group, no communication stream and no collective: `python bench.py`
                       # and `torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` run the same code
                       'single_rank_path': 'no process group / communication stream / collective' if world == 1 else None,
                       'gather_stream': (None if world == 1 else 'caller' if gather_on_compute else 'communication'),
                       'phase_lock': phase_point or None,
                       'jitter_ms_rehearsal': jitter_ms or None,
                       'peak_memory_gib': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                       'reserved_memory_gib': round(torch.cuda.memory_reserved() / 2 ** 30, 2),
                       'caller_streams': args.streams, 'support_cache': bool(args.cache_supports), 'hip_graph': bool(model.use_graphs),
                       'winograd_3x3': {0: 'off', 2: 'F(2x2,3x3)', 4: 'F(4x4,3x3)'}[model.use_winograd],
                       'episodes_per_step_per_gpu': args.batch,
                       'avg_detections': n_d / args.steps / args.batch,
                       # the REFERENCE's formulation of an episode (direct 3x3 convs, relation conv on the
                       # concatenated tensor) - a unit of work for comparing builds, NOT a utilisation figure: the
                       # build issues fewer FLOPs (roofline.flop_per_step), so this rate may exceed the 157.3 TF/s peak
                       'reference_formulation_gflop_per_episode': round(gflop, 1),
                       'reference_formulation_tflops_not_a_utilisation_figure':
                           round(gflop * world * args.steps * args.batch / dt / 1e3, 2)},
        }
        if roofline is not None:
            out['roofline'] = roofline
        if args.full and world > 1 and 'g' in gathered_last:
            # rank 0 holds every rank's detections of the last step incl. the mask probabilities: materialise the
            # complete result dicts of all `world` episodes from the gathered records (off the timed path) and
            # check rank 0's own episode against the dict its normal path produced
            g = gathered_last['g']
            g_recs, g_cnts = g.result() if hasattr(g, 'result') else g
            torch.cuda.synchronize()
            ih, iw = int(episodes[0]['img_shape'][0][0]), int(episodes[0]['img_shape'][0][1])
            full = fdist.results_from_gathered(g_recs.reshape(-1, *g_recs.shape[2:]), g_cnts.reshape(-1), (ih, iw),
                                               cfg['test_cfg']['rcnn']['mask_thr_binary'])
            mine = full[rank * args.batch]
            same = (mine['dt_isegmaps_rle'] == last_results[0]['dt_isegmaps_rle'] and
                    bool((mine['dt_scores'] == last_results[0]['dt_scores']).all()))
            out['gather'] = {'episodes_materialised_on_rank0': len(full), 'bytes_per_episode': int(g_recs[0, 0].numel() * 4 + 4),
                             'rank0_episode_identical_to_local_result': same}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out.update(cpu_and_accuracy(args, cfg, sd, shape, model))
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def cpu_and_accuracy(args, cfg, sd, shape, model) -> dict:
    """The CPU baseline (the oracle timed on the host cores: 2 warm-up + N timed episodes) and the accuracy half of
    the metric on the same episodes - the ONLY place bench.py touches oracle/."""
    import numpy as np
    import torch
    from fgn_amd.agreement import episode_maxima
    from fgn_amd.episodes import make_batch
    from fgn_amd.fsiseg_eval import as_ground_truth, evaluate_results
    from oracle import fgn_ref_cpu as O

    n_timed = args.cpu_episodes
    n_acc = max(args.accuracy_episodes, n_timed)
    for j in (1000, 1001):
        O.simple_test(sd, cfg, **make_batch(j, 1, **shape))          # warm-up
    cpu_res, cpu_tr, batches = [], [], []
    cdt = 0.0
    for j in range(n_acc):
        b = make_batch(2000 + j, 1, **shape)
        tr = {}
        t0 = time.perf_counter()
        r = O.simple_test(sd, cfg, **b, trace=tr)
        if j < n_timed:
            cdt += time.perf_counter() - t0
        if n_acc > n_timed:          # a long leg: show progress (a silent run looks hung to a job scheduler)
            print(f'[accuracy] oracle episode {j + 1}/{n_acc}', file=sys.stderr, flush=True)
        batches.append(b)
        cpu_res.extend(r)
        cpu_tr.append({k: tr[k] for k in ('mask_prob',) if k in tr})
    hip_res, maxima = [], []
    for b, r, tr in zip(batches, cpu_res, cpu_tr):
        dets = model.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                                   qry_isegmaps=b['qry_isegmaps'])
        h = model.pack_results(dets, 1, qry_bboxes=b['qry_bboxes'], qry_cat_ids=b['qry_cat_ids'],
                               qry_isegmaps=b['qry_isegmaps'], img_shape=b['img_shape'], idx=b['idx'])
        hip_res.extend(h)
        n = len(h[0]['dt_scores'])
        if n and len(r['dt_scores']):
            maxima.append(episode_maxima(r, h[0], tr['mask_prob'].numpy(), dets[0]['mask_prob'][:n].cpu().numpy()))
    n_ways = cfg['n_ways']
    ap_cpu, ap_hip = evaluate_results(cpu_res, n_ways), evaluate_results(hip_res, n_ways)
    out = {}
    # AP50 of each path against the synthetic ground truth (FSISEGEval protocol).  The weights are seeded random
    # initialisations (no checkpoint of the reference exists, README.md:27), so both are ~0; the criterion is the
    # difference, |dAP| <= 0.1 - and, sharper, the agreement numbers below
    out['ap50_vs_cpu_ref'] = {k: {'hip': round(ap_hip[k], 4), 'cpu_ref': round(ap_cpu[k], 4)}
                              for k in ('bbox_mAP50', 'segm_mAP50')}
    # what computes every AP in this line: fgn_amd.fsiseg_eval.  Its record building, grouping and `summarize_short` are
    # pinned by goldens from the reference's fsisegeval.py; `evaluate` / `accumulate` restate pycocotools' COCOeval,
    # which is absent from /root/reference and from this image: parity of that half is UNPINNED (known-answer tests
    # only).  Both paths are scored by the same evaluator, so the HIP-vs-CPU difference does not depend on it.
    out['ap50_evaluator'] = ('fgn_amd.fsiseg_eval: FSISEGEval glue pinned by goldens from the reference; '
                             'evaluate/accumulate = pycocotools COCOeval restated, parity unpinned')
    agree = {}
    for thr in (0.5, 0.75, 0.95):
        a = evaluate_results(as_ground_truth(cpu_res, hip_res), n_ways, iou_thr=thr)
        agree[f'iou_{thr}'] = {k: round(v, 4) for k, v in a.items() if 'mAP' in k}
    out['hip_detections_scored_against_cpu_detections'] = agree
    if maxima:
        out['matched_pair_maxima'] = {
            'episodes': len(maxima), 'detections_cpu': int(sum(m['n_ref'] for m in maxima)),
            'matched': int(sum(m['matched'] for m in maxima)),
            'selection_flips_cpu_only': int(sum(m['flips_ref'] for m in maxima)),
            'selection_flips_hip_only': int(sum(m['flips_got'] for m in maxima)),
            'max_abs_dscore': float(np.max([m['max_dscore'] for m in maxima])),
            'max_abs_dmask_prob': float(np.max([m['max_dprob'] for m in maxima])),
            'max_abs_dbox_px': float(np.max([m['max_dbox'] for m in maxima])),
            'tolerance': 'north_star: scores / mask probabilities within 1e-4'}
    if args.train_heads_steps > 0:
        try:
            out['trained_heads'] = trained_heads_leg(args, cfg, sd, batches)
        except Exception as e:          # the accuracy extra must never cost the bench line
            out['trained_heads'] = {'error': f'{type(e).__name__}: {e}'}
    out['cpu_baseline'] = {'value': n_timed / cdt, 'unit': 'img/s', 'cores': torch.get_num_threads(), 'kind': 'port',
                           'cpu_model': cpu_model(),
                           'sample': f'{n_timed} {args.workload} episodes (after 2 warm-up episodes) through '
                                     'oracle/fgn_ref_cpu.py (PyTorch fp32 CPU restatement of the reference path)'}
    return out


def trained_heads_leg(args, cfg, sd, batches) -> dict:
    """Seeded random weights detect nothing, so AP against the synthetic ground truth is 0 for both paths.  Here the
    heads are overfitted on the accuracy episodes themselves (fgn_amd.train.Trainer: the reference's forward_train +
    backward + Adagrad, backbone frozen as in fgn_r50_c4_densecl.py:31), and BOTH paths then score those episodes with
    the same trained weights: a parity vehicle with real detections, not a generalisation claim."""
    import numpy as np
    import torch
    from fgn_amd.agreement import episode_maxima
    from fgn_amd.detector import FGN
    from fgn_amd.fsiseg_eval import as_ground_truth, evaluate_results
    from fgn_amd.train import Trainer
    from oracle import fgn_ref_cpu as O
    n_ways, k_shots = cfg['n_ways'], cfg['k_shots']
    train_b = batches[:5]
    m = FGN(n_ways, k_shots, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
            test_cfg=cfg['test_cfg'], state_dict=sd)
    tr = Trainer(m)
    t0 = time.perf_counter()
    first = last = None
    for it in range(args.train_heads_steps):
        torch.manual_seed(it)
        L = tr.step(train_b[it % len(train_b)])
        tot = sum(float(v[0] if isinstance(v, list) else v) for k, v in L.items() if 'loss' in k)
        first = tot if first is None else first
        last = tot
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    sd2 = tr.state_dict()
    del tr, m
    # a model of its own for the scoring: packed without a live Trainer, i.e. with the build's default GEMM arithmetic
    m = FGN(n_ways, k_shots, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
            test_cfg=cfg['test_cfg'], state_dict=sd2)
    ev_b = train_b[:max(1, args.trained_eval_episodes)]
    hip_res, cpu_res, maxima = [], [], []
    for j, b in enumerate(ev_b):
        trc = {}
        r = O.simple_test(sd2, cfg, **b, trace=trc)
        print(f'[trained heads] oracle episode {j + 1}/{len(ev_b)}', file=sys.stderr, flush=True)
        dets = m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                               qry_isegmaps=b['qry_isegmaps'])
        h = m.pack_results(dets, 1, qry_bboxes=b['qry_bboxes'], qry_cat_ids=b['qry_cat_ids'],
                           qry_isegmaps=b['qry_isegmaps'], img_shape=b['img_shape'], idx=b['idx'])
        cpu_res.extend(r)
        hip_res.extend(h)
        n = len(h[0]['dt_scores'])
        if n and len(r[0]['dt_scores']) and 'mask_prob' in trc:
            maxima.append(episode_maxima(r[0], h[0], trc['mask_prob'].numpy(), dets[0]['mask_prob'][:n].cpu().numpy()))
    ap_cpu, ap_hip = evaluate_results(cpu_res, n_ways), evaluate_results(hip_res, n_ways)
    out = {'what': f'heads overfitted for {args.train_heads_steps} Trainer steps on {len(train_b)} of the accuracy '
                   f'episodes (frozen random backbone), {len(ev_b)} of them scored by both paths with those weights',
           'train_seconds': round(t_train, 2), 'summed_loss_first_last': [round(first, 4), round(last, 4)],
           'ap50_vs_ground_truth': {k: {'hip': round(ap_hip[k], 4), 'cpu_ref': round(ap_cpu[k], 4)}
                                    for k in ('bbox_mAP50', 'segm_mAP50')},
           'detections': {'hip': [len(r['dt_scores']) for r in hip_res], 'cpu_ref': [len(r['dt_scores']) for r in cpu_res]}}
    agree = {}
    for thr in (0.5, 0.95):
        a = evaluate_results(as_ground_truth(cpu_res, hip_res), n_ways, iou_thr=thr)
        agree[f'iou_{thr}'] = {k: round(v, 4) for k, v in a.items() if 'mAP' in k}
    out['hip_detections_scored_against_cpu_detections'] = agree
    if maxima:
        out['matched_pair_maxima'] = {
            'matched': int(sum(x['matched'] for x in maxima)), 'detections_cpu': int(sum(x['n_ref'] for x in maxima)),
            'selection_flips': int(sum(x['flips_ref'] + x['flips_got'] for x in maxima)),
            'max_abs_dscore': float(np.max([x['max_dscore'] for x in maxima])),
            'max_abs_dmask_prob': float(np.max([x['max_dprob'] for x in maxima]))}
    return out


if __name__ == '__main__':
    main()
