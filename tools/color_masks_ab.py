#!/usr/bin/env python3
"""A/B of the two forms the ground-truth masks of a character-dataset query reach ``FGN.detect_device`` in, one GPU,
one process.

Arm A ('dense'): ``qry_isegmaps`` as [n,H,W] bool arrays, uploaded byte per pixel - what the reference's MNISTISEG /
OMNIISEG loader derives on the host for every sample (``get_char_mask_by_color``, create_img_from_chars.py:136-158) and
what ``cluttered_chars.char_mask_by_color`` restates.  Arm B ('color'): the same instances as box + colour
(``colormask.ColorMasks``, 7 integers each, what the dataset stores); ``fgn_color_mask_u8`` makes the dense bytes on the
device from the image bytes that are uploaded in both arms anyway.  Everything behind the masks is the
same in both arms.

cfg3 shapes (800x1333): the seeded episodes of ``episodes.make_batch``, whose elliptic instances are painted in palette
colours on a white uint8 image (so that the colour rule has something to find; the masks of BOTH arms are the rule's, on
those bytes); graph replay, transfers on the caller stream, one episode in flight: the episode time is the host clock
from ``detect_device`` to the end of ``pack_results``.  Arms alternate in blocks; per arm the block medians, their median
and spread (max - min).  Beside them the mask bytes an episode uploads per arm, the time of the kernel (mean of
back-to-back launches between two events, once through ``ops.color_masks`` - wrapper, upload of the records and launch
gaps included - and once the launch alone from records already on the device) next to the dense upload it replaces, and
the host time of ``char_mask_by_color`` that a loader yielding box + colour no longer spends.  There is no pass or fail
threshold on time.

    python tools/color_masks_ab.py --out profiles/color_masks_ab.json
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
from fgn_amd import colormask, ops                                              # noqa: E402
from fgn_amd.cluttered_chars import PALETTE                                     # noqa: E402
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402

MEAN, STD = (0.95, 0.95, 0.95), (0.17, 0.17, 0.17)          # (about MNISTISEG's; any table serves both arms alike)


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


def painted(masks: np.ndarray):
    """The instances of an episode painted on a white image: -> (img uint8 [h,w,3], ColorMasks)."""
    n, h, w = masks.shape
    img = np.full((h, w, 3), 255, np.uint8)
    boxes = []
    for i, m in enumerate(masks):
        img[m] = PALETTE[i % len(PALETTE)]
        ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        boxes.append([ys[0], xs[0], ys[-1] + 1, xs[-1] + 1] if len(ys) else [0, 0, 0, 0])
    colors = PALETTE[np.arange(n) % len(PALETTE)]
    return img, colormask.as_color_masks({'bboxes': np.asarray(boxes).reshape(-1, 4), 'colors': colors}, (h, w), 'episode')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=40, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=15, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('color_masks_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    dev = torch.device('cuda', torch.cuda.current_device())
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.set_input_norm(mean=MEAN, std=STD)
    model.use_graphs = True
    model.transfer_stream(3)

    pin = lambda t: t.pin_memory() if isinstance(t, torch.Tensor) else t
    eps, items = [], []
    for j in range(args.distinct):
        b = {k: pin(v) for k, v in make_batch(j, 1, **shape).items()}
        img, item = painted(np.asarray(b['qry_isegmaps'][0]).astype(bool))
        b['qry_img'] = pin(torch.from_numpy(img)[None].contiguous())
        dense = [pin(torch.from_numpy(item.dense(img)))]
        eps.append({'dense': dict(b, qry_isegmaps=dense), 'color': dict(b, qry_isegmaps=[item])})
        items.append((img, item))
    uploaded = dict(dense=[sum(g.numel() for g in e['dense']['qry_isegmaps']) for e in eps],
                    color=[4 * ops.CM_REC_INTS * len(it) for _, it in items],
                    instances=[len(it) for _, it in items],
                    image_bytes_both_arms=[int(e['dense']['qry_img'].numel()) for e in eps])

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'], qry_isegmaps=e['qry_isegmaps'])

    same = all(episode('dense', j)[0]['qry_isegmaps_rle'] == episode('color', j)[0]['qry_isegmaps_rle'] and
               np.array_equal(episode('dense', j)[0]['dt_scores'], episode('color', j)[0]['dt_scores'])
               for j in range(len(eps)))
    for arm in ('dense', 'color'):
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {'dense': [], 'color': []}
    for blk in range(args.blocks):
        for arm in (('dense', 'color') if blk % 2 == 0 else ('color', 'dense')):    # alternate, and alternate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    img0, it0 = items[0]
    g0 = eps[0]['dense']['qry_isegmaps'][0]
    slot = torch.from_numpy(img0).to(dev).view(1, -1)
    recs = np.concatenate(ops._color_records([(0, it0)], 1, slot.shape[1], 'color_masks_ab'))
    recs[:, 13] = np.arange(len(it0))
    drecs = torch.from_numpy(recs).to(dev)
    out = torch.empty((len(it0), it0.shape[1] * it0.shape[2]), dtype=torch.uint8, device=dev)
    launch = lambda: ops._lib.check(ops._lib.load().fgn_color_mask_u8(
        slot.data_ptr(), slot.shape[1], slot.shape[1], 1, drecs.data_ptr(), len(it0), out.data_ptr(), out.shape[1], len(it0),
        it0.shape[1], it0.shape[2], torch.cuda.current_stream().cuda_stream), 'fgn_color_mask_u8')
    kernels_us = dict(
        dense_upload=round(device_us(lambda: g0.to(dev, non_blocking=True)), 2),
        color_masks=round(device_us(lambda: ops.color_masks(slot, [(0, it0)])), 2),
        launch_alone=round(device_us(launch), 2),
        note=f'{len(it0)} masks of {it0.shape[1]}x{it0.shape[2]}: the pinned dense copy against ops.color_masks (allocation, '
             f'upload of the records and the launch) and against the launch alone from records on the device; mean of 20 '
             f'back-to-back calls between two events')
    host_ms = dict(char_mask_by_color=round(clock_ms(lambda: it0.dense(img0)), 4),
                   as_color_masks=round(clock_ms(lambda: colormask.as_color_masks(
                       {'bboxes': it0.boxes, 'colors': it0.colors}, it0.shape[1:])), 4),
                   note='one core, the masks of one image: the host rule a loader that yields box + colour no longer runs '
                        '(outside the dense arm\'s episode time), beside the check of the colour entry (inside the colour '
                        'arm\'s episode time)')

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    res = dict(tool='color_masks_ab', workload=args.workload, device=torch.cuda.get_device_name(0),
               image_hw=[shape['height'], shape['width']], blocks_per_arm=args.blocks, episodes_per_block=args.episodes,
               warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True, transfer_mode=3, pinned_inputs=True,
               arms_agree=bool(same), graphs=len(model._graphs), dense_arm=arm_stats(blocks['dense']),
               color_arm=arm_stats(blocks['color']), uploaded_mask_bytes_per_episode=uploaded, kernels_us=kernels_us,
               host_ms=host_ms)
    res['color_minus_dense_median_ms'] = round(res['color_arm']['median_ms'] - res['dense_arm']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
