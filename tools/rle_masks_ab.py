#!/usr/bin/env python3
"""A/B of the two forms the ground-truth masks of a query reach ``FGN.detect_device`` in, one GPU, one process.

Arm A ('dense'): ``qry_isegmaps`` as [n,H,W] bool arrays, uploaded byte per pixel (what the reference's COCO dataset
makes on the host with ``maskUtils.decode`` for every sample, coco_ds.py:265-278).  Arm B ('rle'): the same masks as
COCO RLE dicts, the form that dataset holds them in; the strings are parsed on the host (``rle.as_masks``, INSIDE the
episode time), their run ends are uploaded and ``fgn_rle_decode_u8`` makes the dense bytes on the device (DESIGN.md
4.4.10).  Everything behind the decoded tensor is the same in both arms.

cfg3 shapes (800x1333), the seeded episodes of ``episodes.make_batch`` (elliptic instances), graph replay, transfers on
the caller stream, one episode in flight: the episode time is the host clock from ``detect_device`` to the end of
``pack_results``.  Arms alternate in blocks; per arm the block medians, their median and spread (max - min).  Beside
them the mask bytes an episode uploads per arm and the time of the decode next to the dense upload it replaces (mean of
back-to-back calls between two events: the wrapper, its upload of the runs and launch gaps included).  There is no pass
or fail threshold on time: the upload is overlapped, and this record is what says whether it was on the critical path.

``--kernels-only`` launches the decode alone (no model, no episodes), 3 + 20 times with a synchronisation between
launches: the run to put under a kernel trace, whose durations of ``rle_decode_kernel`` exclude the wrapper, the upload
of the runs and the launch gaps (profiles/rle_masks_kernel_stats.csv).

    python tools/rle_masks_ab.py --out profiles/rle_masks_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/rle_masks_ab.py --kernels-only
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgn_amd import ops, rle                                                    # noqa: E402
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402


def device_us(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def clock_ms(fn, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=40, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=15, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the decode of the first episode\'s masks alone, 3 + 20 times: the run to put under '
                         '`rocprofv3 --kernel-trace --stats`, whose durations are the kernel\'s own')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rle_masks_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    dev = torch.device('cuda', torch.cuda.current_device())
    if args.kernels_only:
        m0 = rle.as_masks(rle.encode_many(np.asarray(make_batch(0, 1, **shape)['qry_isegmaps'][0]).astype(bool)))
        for _ in range(23):
            out = ops.rle_decode_masks(m0, device=dev)
            torch.cuda.synchronize()
        print(json.dumps(dict(tool='rle_masks_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              masks=list(m0.shape), runs=int(m0.ends.size), launches=23,
                              bytes_written=int(out.numel()))), flush=True)
        return
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)

    pin = lambda t: t.pin_memory() if isinstance(t, torch.Tensor) else t
    eps = []
    for j in range(args.distinct):
        b = {k: pin(v) for k, v in make_batch(j, 1, **shape).items()}
        dense = [pin(torch.as_tensor(g).to(torch.bool).contiguous()) for g in b['qry_isegmaps']]
        runs = [rle.encode_many(g.numpy()) for g in dense]
        eps.append({'dense': dict(b, qry_isegmaps=dense), 'rle': dict(b, qry_isegmaps=runs)})
    checked = [[rle.as_masks(g) for g in e['rle']['qry_isegmaps']] for e in eps]
    uploaded = dict(
        dense=[sum(g.numel() for g in e['dense']['qry_isegmaps']) for e in eps],
        rle=[sum(m.ends.nbytes + 4 * ops.RLE_REC_INTS * len(m) for m in ms) for ms in checked],
        instances=[sum(len(m) for m in ms) for ms in checked],
        runs=[sum(int(m.ends.size) for m in ms) for ms in checked],
        string_bytes=[sum(len(it['counts']) for g in e['rle']['qry_isegmaps'] for it in g) for e in eps])

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'], qry_isegmaps=e['qry_isegmaps'])

    same = all(episode('dense', j)[0]['qry_isegmaps_rle'] == episode('rle', j)[0]['qry_isegmaps_rle'] and
               np.array_equal(episode('dense', j)[0]['dt_scores'], episode('rle', j)[0]['dt_scores'])
               for j in range(len(eps)))
    for arm in ('dense', 'rle'):
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {'dense': [], 'rle': []}
    for blk in range(args.blocks):
        for arm in (('dense', 'rle') if blk % 2 == 0 else ('rle', 'dense')):      # alternate, and alternate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    g0, m0 = eps[0]['dense']['qry_isegmaps'][0], checked[0][0]
    kernels_us = dict(
        dense_upload=round(device_us(lambda: g0.to(dev, non_blocking=True)), 2),
        rle_decode_masks=round(device_us(lambda: ops.rle_decode_masks(m0, device=dev)), 2),
        note=f'{len(m0)} masks of {m0.shape[1]}x{m0.shape[2]}, {int(m0.ends.size)} runs: the pinned dense copy against '
             f'the upload of the runs plus the decode launch; mean of 20 back-to-back calls between two events')
    host_ms = dict(as_masks=round(clock_ms(lambda: rle.as_masks(eps[0]['rle']['qry_isegmaps'][0])), 4),
                   dense_on_host=round(clock_ms(lambda: m0.dense()), 4),
                   note='one core, the masks of one image: parsing and checking the strings (inside the rle arm\'s episode '
                        'time) beside the host decode the dense arm\'s loader would do (outside its episode time)')

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    res = dict(tool='rle_masks_ab', workload=args.workload, device=torch.cuda.get_device_name(0),
               image_hw=[shape['height'], shape['width']], blocks_per_arm=args.blocks, episodes_per_block=args.episodes,
               warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True, transfer_mode=3, pinned_inputs=True,
               arms_agree=bool(same), graphs=len(model._graphs), dense_arm=arm_stats(blocks['dense']),
               rle_arm=arm_stats(blocks['rle']), uploaded_mask_bytes_per_episode=uploaded, kernels_us=kernels_us,
               host_ms=host_ms)
    res['rle_minus_dense_median_ms'] = round(res['rle_arm']['median_ms'] - res['dense_arm']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
