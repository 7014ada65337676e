#!/usr/bin/env python3
"""A/B of the two ways a photometrically augmented query reaches ``Trainer.step`` on one GPU, one process.

Both arms hand over source-size pixels with ``qry_resize_to``.  Arm A ('host'): the loader's route -
``fewshot_ds.photometric_image_u8`` changes the source image on the host (one core, numpy: the integer rule, not
imgaug's C code) and the changed pixels are uploaded; the operator changes with every step, so its host time is part of
the arm's step and is reported separately too.  Arm B ('device'): the plain pixels and ``qry_photometric``; the operator
runs in ``photometric_u8hwc3_kernel`` behind the upload.

cfg3 shapes (800x1333, 3-way 3-shot, ResNet-50-C4 frozen, heads trained), a 600x1000 source, one image per step, the six
operators in turn.  The step time is the host clock around ``Trainer.step`` and a device synchronisation.  Arms alternate
in blocks; per arm the block medians, their median and spread (max - min).  Both arms compute the same step
(tests/test_hip_qry_photometric_e2e.py pins that byte for byte).  Beside them the duration of the kernel per operator
next to the resize kernel it feeds (mean of back-to-back launches between two events: wrappers and launch gaps included).
``--kernels-only`` runs just those launches, operator by operator, for a kernel trace; ``--trace-csv`` reads that trace
back and gives the kernel's own duration per operator (the launches of ``--kernels-only`` in their order).

    python tools/qry_photometric_ab.py --out profiles/qry_photometric_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/qry_photometric_ab.py --kernels-only
    python tools/qry_photometric_ab.py --trace-csv <..._kernel_trace.csv>
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgn_amd import fewshot_ds as fd, ops                                       # noqa: E402
from fgn_amd.config import fgn_r50_c4_config                                    # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, make_batch                                # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402
from qry_augment_ab import MEAN, STD, instances, pixels                         # noqa: E402

# the six operators at the far end of the ranges of ``fewshot_ds.draw_query_augment_full``, one per step in turn
ROWS = [np.array(r, np.float64) for r in ((1, 1.0, 11), (2, 0.03, 12), (3, 3.0, 0), (4, 50, 0), (5, -75, 0), (6, 30, 0))]
NAMES = [fd.PHOTO_OPS[int(r[0])] for r in ROWS]
WARM, REPS = 3, 20


def device_us(fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def kernel_times(lut, q_src, H, W, dev) -> dict:
    """The photometric kernel per operator (and as a plain copy), then the resize kernel at the same shapes, through
    their Python wrappers: WARM + REPS launches each, in this order."""
    h, w = q_src.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(q_src)).reshape(1, -1).to(dev)
    src_hw = torch.tensor([[h, w]], dtype=torch.int32, device=dev)
    out = {}
    for name, r in zip(['copy'] + NAMES, [None] + ROWS):
        rec = torch.from_numpy(fd.query_photometric_record(r, (h, w), (H, W))[None]).to(dev)
        out[f'photometric_u8hwc3_{name}'] = round(device_us(lambda: ops.photometric_u8(src, rec)), 2)
    out['resize_u8hwc3_to_nhwc4'] = round(device_us(lambda: ops.resize_u8_to_nhwc4(src, src_hw, lut, H, W)), 2)
    out['note'] = (f'source {h}x{w}, network {H}x{W} (the blur: sigma 3 network pixels = radius 7 on both axes); mean of '
                   f'{REPS} back-to-back launches between two events (wrapper, allocation and launch gaps included)')
    return out


def trace_summary(path: str) -> dict:
    """The kernel's own durations from the kernel trace of a ``--kernels-only`` run: its launches in order, WARM + REPS per
    operator, the first WARM of each dropped."""
    with open(path, newline='') as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r['Start_Timestamp']))
    dur = lambda name: [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows
                        if r['Kernel_Name'].startswith(name)]
    ph, rs = dur('photometric_u8hwc3_kernel'), dur('resize_u8hwc3_to_nhwc4_kernel')
    names = ['copy'] + NAMES
    if len(ph) != len(names) * (WARM + REPS) or len(rs) != WARM + REPS:
        raise SystemExit(f'{path}: {len(ph)} + {len(rs)} launches, expected those of one --kernels-only run')
    stat = lambda v: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    out = {f'photometric_u8hwc3_{n}': stat(ph[i * (WARM + REPS) + WARM:(i + 1) * (WARM + REPS)]) for i, n in enumerate(names)}
    out['resize_u8hwc3_to_nhwc4'] = stat(rs[WARM:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(600, 1000), metavar=('h', 'w'))
    ap.add_argument('--masks', type=int, default=32, help='ground-truth masks per query')
    ap.add_argument('--blocks', type=int, default=4, help='blocks per arm')
    ap.add_argument('--steps', type=int, default=6, help='steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='steps per arm before the first block')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the kernels alone (no model, no steps) and print their event means: the run to put under '
                         '`rocprofv3 --kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    ap.add_argument('--trace-csv', default=None, help='the kernel trace of a --kernels-only run: durations per operator')
    args = ap.parse_args()
    if args.trace_csv:
        print(json.dumps(dict(tool='qry_photometric_ab', kernel_trace_us=trace_summary(args.trace_csv))), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit('qry_photometric_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    H, W = shape['height'], shape['width']
    h, w = args.source
    rng = np.random.RandomState(0)
    dev = torch.device('cuda', torch.cuda.current_device())
    q_src = pixels(rng, h, w)
    m_src, boxes, cats = instances(rng, args.masks, h, w, shape['n_ways'])
    if args.kernels_only:
        lut = torch.from_numpy(ops.input_lut(MEAN, STD, 255.0)).to(dev)
        print(json.dumps(dict(tool='qry_photometric_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              kernels_us=kernel_times(lut, q_src, H, W, dev))), flush=True)
        return

    from fgn_amd.train import Trainer
    cfg = fgn_r50_c4_config(shape['n_ways'], shape['k_shots'])
    model = FGN(cfg['n_ways'], cfg['k_shots'], state_dict=init_state_dict(cfg, 0))
    model.set_input_norm(mean=MEAN, std=STD)
    trainer = Trainer(model)
    b = make_batch(0, 1, **shape)                           # supports of a seeded episode
    S = shape['spp_size']
    nk = shape['n_ways'] * shape['k_shots']
    common = dict(spp_imgs=torch.from_numpy(np.stack([pixels(rng, S, S) for _ in range(nk)]))[None].pin_memory(),
                  spp_bboxes=b['spp_bboxes'], spp_isegmaps=b['spp_isegmaps'], img_shape=b['img_shape'],
                  qry_cat_ids=[torch.from_numpy(cats)], qry_bboxes=[torch.from_numpy(boxes)],
                  qry_isegmaps=[torch.from_numpy(m_src).pin_memory()], qry_resize_to=(H, W))
    src_img = torch.from_numpy(q_src)[None].pin_memory()
    host_ms = {n: [] for n in NAMES}

    def step(arm, j):
        r = ROWS[j % len(ROWS)]
        if arm == 'host':
            t0 = time.perf_counter()
            img = fd.photometric_image_u8(q_src, fd.query_photometric_record(r, (h, w), (H, W)))
            host_ms[NAMES[j % len(ROWS)]].append((time.perf_counter() - t0) * 1e3)
            batch = dict(common, qry_img=torch.from_numpy(img)[None])
        else:
            batch = dict(common, qry_img=src_img, qry_photometric=r[None])
        torch.manual_seed(j)
        losses = trainer.step(batch)
        torch.cuda.synchronize()
        return losses

    for arm in ('host', 'device'):
        for j in range(args.warmup):
            step(arm, j)
    for v in host_ms.values():
        v.clear()
    blocks = {'host': [], 'device': []}
    for blk in range(args.blocks):
        for arm in (('host', 'device') if blk % 2 == 0 else ('device', 'host')):      # alternate, and alternate who goes first
            times = []
            for j in range(args.steps):
                t0 = time.perf_counter()
                step(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))

    kernels_us = kernel_times(model._lut_on(dev), q_src, H, W, dev)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3),
                    spread_ms=round(max(v) - min(v), 3))
    all_host = [x for v in host_ms.values() for x in v]
    res = dict(tool='qry_photometric_ab', workload=f'{args.workload} training step (Trainer.step), batch 1',
               device=torch.cuda.get_device_name(0), source_hw=[h, w], network_hw=[H, W], gt_masks=args.masks,
               rows=[r.tolist() for r in ROWS], blocks_per_arm=args.blocks, steps_per_block=args.steps,
               warmup_per_arm=args.warmup, host_arm=arm_stats(blocks['host']), device_arm=arm_stats(blocks['device']),
               host_photometric_ms_per_step=dict(median=round(statistics.median(all_host), 3),
                                                 per_operator_median={n: round(statistics.median(v), 3)
                                                                      for n, v in host_ms.items() if v},
                                                 note='fewshot_ds.photometric_image_u8 on one core (numpy, the integer '
                                                      'rule); INSIDE the host arm\'s step time'),
               kernels_us=kernels_us)
    res['device_minus_host_median_ms'] = round(res['device_arm']['median_ms'] - res['host_arm']['median_ms'], 3)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
