#!/usr/bin/env python3
"""A/B of the two ways an augmented query reaches ``Trainer.step`` on one GPU, one process.

Arm A ('host'): the loader's route - ``fewshot_ds.augment_query`` warps the image and every ground-truth mask to the
network size on the host (``get_query`` with ``augment_qry``, base_fst.py:876-891) and the trainer gets network-size
uint8 pixels.  The augmentation changes with every step, so its host time is part of the arm's step; it is reported
separately too (one core, numpy: the integer rule, not imgaug's C code).  Arm B ('device'): source-size pixels, masks,
``qry_resize_to`` and ``qry_augment``; image and masks are warped by two kernels behind the upload.

cfg3 shapes (800x1333, 3-way 3-shot, ResNet-50-C4 frozen, heads trained), 600x1000 sources, a few dozen ground-truth
masks, one image per step, a cycle of augmentation rows (rotation, scale, shear, translation, flip; channel orders).
The step time is the host clock around ``Trainer.step`` and a device synchronisation.  Arms alternate in blocks; per arm
the block medians, their median and spread (max - min).  Both arms compute the same step (tests/
test_hip_qry_augment_e2e.py pins that byte for byte).  Beside them the bytes a step uploads for the query and the
durations of the two augmentation kernels next to the two resize kernels at the same shapes (mean of back-to-back
launches between two events: wrappers and launch gaps included).  ``--kernels-only`` runs just those launches, for a
kernel trace of the kernels' own durations.

    python tools/qry_augment_ab.py --out profiles/qry_augment_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/qry_augment_ab.py --kernels-only
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
from fgn_amd import fewshot_ds as fd, ops                                       # noqa: E402
from fgn_amd.config import fgn_r50_c4_config                                    # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, make_batch                                # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402

MEAN = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['mean'], np.float32)
STD = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['std'], np.float32)


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


# the operators of ``fewshot_ds.draw_query_augment``, one per step in turn
ROWS = [row(rotate=10, border=1), row(scale=0.85, order=3), row(shear=-8, border=1), row(tx=17, ty=-12), row(flip=1),
        row(scale=1.15), row(shear=9, border=1, order=5), row(tx=-20, ty=20)]


def pixels(rng, h, w):
    """A page-like image: white ground, dark tinted blobs (values over the whole byte range)."""
    img = np.full((h, w, 3), 255, np.uint8)
    for _ in range(24):
        y, x = int(rng.randint(0, h - 8)), int(rng.randint(0, w - 8))
        dy, dx = int(rng.randint(8, max(9, h // 6))), int(rng.randint(8, max(9, w // 6)))
        img[y:y + dy, x:x + dx] = rng.randint(0, 256, size=(min(dy, h - y), min(dx, w - x), 3), dtype=np.uint8)
    return img


def instances(rng, n, h, w, n_ways):
    """n rectangular instances in the middle of the image (no augmentation row moves one out): masks, boxes YXYX, class
    ids."""
    m = np.zeros((n, h, w), bool)
    boxes = np.zeros((n, 4), np.float32)
    for g in range(n):
        y, x = int(rng.randint(h // 4, h // 2)), int(rng.randint(w // 4, w // 2))
        dy, dx = int(rng.randint(16, h // 4)), int(rng.randint(16, w // 4))
        m[g, y:y + dy, x:x + dx] = True
        boxes[g] = (y, x, y + dy, x + dx)
    return m, boxes, rng.randint(0, n_ways, size=n).astype(np.int64)


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


def kernel_times(lut, q_src, m_src, H, W, dev) -> dict:
    """The two augmentation kernels (rotation by 10 degrees, symmetric border: the slanted gather; and a flip: the
    resize's taps) beside the two resize kernels at the same shapes, through their Python wrappers."""
    h, w = q_src.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(q_src)).reshape(1, -1).to(dev)
    src_hw = torch.tensor([[h, w]], dtype=torch.int32, device=dev)
    msk = torch.from_numpy(np.ascontiguousarray(m_src)).to(dev)
    rec = {k: torch.from_numpy(fd.query_augment_record(r, (h, w), (H, W))[None]).to(dev)
           for k, r in (('rot10', ROWS[0]), ('flip', ROWS[4]))}
    us = lambda fn: round(device_us(fn), 2)
    return dict(resize_u8hwc3_to_nhwc4=us(lambda: ops.resize_u8_to_nhwc4(src, src_hw, lut, H, W)),
                augment_u8hwc3_to_nhwc4_rot10=us(lambda: ops.augment_u8_to_nhwc4(src, rec['rot10'], lut, H, W)),
                augment_u8hwc3_to_nhwc4_flip=us(lambda: ops.augment_u8_to_nhwc4(src, rec['flip'], lut, H, W)),
                resize_mask_u8=us(lambda: ops.resize_masks(msk, H, W)),
                augment_mask_u8_rot10=us(lambda: ops.augment_masks(msk, rec['rot10'][0], H, W)),
                augment_mask_u8_flip=us(lambda: ops.augment_masks(msk, rec['flip'][0], H, W)),
                note=f'output {H}x{W}, source {h}x{w}, {len(m_src)} masks in one launch; mean of 20 back-to-back '
                     f'launches between two events (launch gaps included)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(600, 1000), metavar=('h', 'w'))
    ap.add_argument('--masks', type=int, default=32, help='ground-truth masks per query')
    ap.add_argument('--blocks', type=int, default=4, help='blocks per arm')
    ap.add_argument('--steps', type=int, default=8, help='steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='steps per arm before the first block')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the four kernels alone (no model, no steps) and print their event means: the run to put '
                         'under `rocprofv3 --kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('qry_augment_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    H, W = shape['height'], shape['width']
    h, w = args.source
    rng = np.random.RandomState(0)
    dev = torch.device('cuda', torch.cuda.current_device())
    q_src = pixels(rng, h, w)
    m_src, boxes, cats = instances(rng, args.masks, h, w, shape['n_ways'])
    if args.kernels_only:
        lut = torch.from_numpy(ops.input_lut(MEAN, STD, 255.0)).to(dev)
        print(json.dumps(dict(tool='qry_augment_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              kernels_us=kernel_times(lut, q_src, m_src, H, W, dev))), flush=True)
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
                  qry_cat_ids=[torch.from_numpy(cats)])
    src_img, src_masks = torch.from_numpy(q_src)[None].pin_memory(), torch.from_numpy(m_src).pin_memory()
    host_ms = []

    def step(arm, j):
        r = ROWS[j % len(ROWS)]
        if arm == 'host':
            t0 = time.perf_counter()
            img, bx, mk = fd.augment_query(q_src, boxes, m_src, H, W, r)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            batch = dict(common, qry_img=torch.from_numpy(img)[None], qry_bboxes=[torch.from_numpy(bx)],
                         qry_isegmaps=[torch.from_numpy(mk)])
        else:
            batch = dict(common, qry_img=src_img, qry_bboxes=[torch.from_numpy(boxes)], qry_isegmaps=[src_masks],
                         qry_resize_to=(H, W), qry_augment=r[None])
        torch.manual_seed(j)
        losses = trainer.step(batch)
        torch.cuda.synchronize()
        return losses

    for r in ROWS:                                          # every row is applied: no fallback in either arm
        rec, _ = fd.augment_plan(r, boxes, (h, w), (H, W))
        assert rec[2:6].any()
    for arm in ('host', 'device'):
        for j in range(args.warmup):
            step(arm, j)
    host_ms.clear()
    blocks = {'host': [], 'device': []}
    for blk in range(args.blocks):
        for arm in (('host', 'device') if blk % 2 == 0 else ('device', 'host')):      # alternate, and alternate who goes first
            times = []
            for j in range(args.steps):
                t0 = time.perf_counter()
                step(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))

    kernels_us = kernel_times(model._lut_on(dev), q_src, m_src, H, W, dev)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3),
                    spread_ms=round(max(v) - min(v), 3))
    res = dict(tool='qry_augment_ab', workload=f'{args.workload} training step (Trainer.step), batch 1',
               device=torch.cuda.get_device_name(0), source_hw=[h, w], network_hw=[H, W], gt_masks=args.masks,
               rows=[r.tolist() for r in ROWS], blocks_per_arm=args.blocks, steps_per_block=args.steps,
               warmup_per_arm=args.warmup, host_arm=arm_stats(blocks['host']), device_arm=arm_stats(blocks['device']),
               host_augment_ms_per_step=dict(median=round(statistics.median(host_ms), 3), min=round(min(host_ms), 3),
                                             max=round(max(host_ms), 3),
                                             note='fewshot_ds.augment_query on one core (numpy, the integer rule); '
                                                  'INSIDE the host arm\'s step time'),
               uploaded_query_bytes_per_step=dict(host=dict(image=3 * H * W, gt_masks=args.masks * H * W),
                                                  device=dict(image=3 * h * w, gt_masks=args.masks * h * w, records=64)),
               kernels_us=kernels_us)
    res['device_minus_host_median_ms'] = round(res['device_arm']['median_ms'] - res['host_arm']['median_ms'], 3)
    res['host_arm_minus_its_augment_ms'] = round(res['host_arm']['median_ms'] - res['host_augment_ms_per_step']['median'], 3)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
