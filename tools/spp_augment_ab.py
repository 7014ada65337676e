#!/usr/bin/env python3
"""A/B of the two ways an augmented support set reaches ``Trainer.step`` on one GPU, one process.

Arm A ('host'): the loader's route - ready S x S uint8 supports come in (their cut is done ahead of the timed steps) and
``fewshot_ds.augment_support`` augments each of the N*K instances on the host (``get_support`` with ``augment_spp``,
base_fst.py:1151-1153); the trainer gets ready uint8 supports, masks and boxes.  The augmentation changes with every
step, so its host time is part of the arm's step; it is reported separately too (one core, numpy: the integer rule, not
imgaug's C code).  Arm B ('device'): the instances' source images, masks and boxes with ``spp_crop_to``, ``spp_augment``
and ``spp_photometric``; the supports are made by three launches behind the upload.  Its step time INCLUDES the host
part of that path (geometry, window packing and the plan per instance).

cfg3 shapes (800x1333, 3-way 3-shot, S = 256, ResNet-50-C4 frozen, heads trained), nine supports on 480x640 sources,
batch 1, eager, a cycle of row pairs that covers every geometric and every photometric operator (instance i of step j
takes pair i + j).  The step time is the host clock around ``Trainer.step`` and a device synchronisation.  Arms
alternate in blocks; per arm the block medians, their median and spread (max - min).  Both arms compute the same step
(tests/test_hip_spp_augment_e2e.py pins that byte for byte).  Beside them the bytes a step uploads for its supports and
the durations of the launches (mean of back-to-back launches between two events: wrappers and launch gaps included).
``--kernels-only`` runs just those launches, for a kernel trace of the kernels' own durations.

    python tools/spp_augment_ab.py --out profiles/spp_augment_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/spp_augment_ab.py --kernels-only
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


# the operators of ``fewshot_ds.draw_support_augment``: five geometric ones, a channel order, the neutral row ...
GEO = [row(rotate=10, border=1), row(scale=0.85), row(shear=-8, border=1), row(tx=17, ty=-12), row(flip=1), row(order=3),
       row(), row(scale=1.15), row(shear=9, border=1)]
# ... and noise, impulse noise, blur, hue, saturation, brightness, none
PHOTO = [np.array(p, np.float64) for p in ((1, 1.0, 11), (2, 0.02, 12), (3, 1.5, 0), (4, 40, 0), (5, -60, 0), (6, 25, 0),
                                           (0, 0, 0))]


def pixels(rng, h, w):
    """A page-like image: white ground, dark tinted blobs (values over the whole byte range)."""
    img = np.full((h, w, 3), 255, np.uint8)
    for _ in range(24):
        y, x = int(rng.randint(0, h - 8)), int(rng.randint(0, w - 8))
        dy, dx = int(rng.randint(8, max(9, h // 6))), int(rng.randint(8, max(9, w // 6)))
        img[y:y + dy, x:x + dx] = rng.randint(0, 256, size=(min(dy, h - y), min(dx, w - x), 3), dtype=np.uint8)
    return img


def instance(rng, h, w, lo, hi):
    """One support instance on its own source image: (image, box YXYX float32, mask) - an ellipse in a box of lo..hi
    pixels per side, anywhere on the image (boxes at the border get reflected context)."""
    bh, bw = int(rng.randint(lo, min(hi, h) + 1)), int(rng.randint(lo, min(hi, w) + 1))
    y, x = int(rng.randint(0, h - bh + 1)), int(rng.randint(0, w - bw + 1))
    yy, xx = np.mgrid[0:bh, 0:bw]
    mask = np.zeros((h, w), bool)
    mask[y:y + bh, x:x + bw] = ((yy - bh / 2 + 0.5) / (bh / 2)) ** 2 + ((xx - bw / 2 + 0.5) / (bw / 2)) ** 2 <= 1.0
    return pixels(rng, h, w), np.array([y, x, y + bh, x + bw], np.float32), mask


def rows_of(j, nk):
    return (np.stack([GEO[(i + j) % len(GEO)] for i in range(nk)]), np.stack([PHOTO[(i + j) % len(PHOTO)] for i in range(nk)]))


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


def kernel_times(lut, insts, S, dev) -> dict:
    """The direct launch beside the three of the augmented path on the same nine instances, through their wrappers; the
    rows of step 0 (every operator on some instance) and, for the gather, nine rotations and nine flips as well."""
    geos = [fd.support_geometry(im.shape[0], im.shape[1], bb, S) for im, bb, _ in insts]
    wins = [fd.support_window(im, mk, g[0]) for (im, _, mk), g in zip(insts, geos)]
    n = len(insts)
    src = torch.zeros((n, max(w.size for w, _ in wins)), dtype=torch.uint8)
    msk = torch.zeros((n, max(m.size for _, m in wins)), dtype=torch.uint8)
    for i, (w, m) in enumerate(wins):
        src[i, :w.size] = torch.from_numpy(w.reshape(-1))
        msk[i, :m.size] = torch.from_numpy(m.reshape(-1))
    src, msk = src.to(dev), msk.to(dev)
    srec = torch.from_numpy(np.stack([g[0] for g in geos])).to(dev)
    geo, photo = rows_of(0, n)
    recs, precs, _, fell = fd.support_augment_plan(geo, photo, np.stack([g[1] for g in geos]), S)
    assert not fell.any()
    plan = lambda r: torch.from_numpy(np.stack([fd.query_augment_record(r, (S, S), (S, S))] * n)).to(dev)
    recs, precs, rot, flip = torch.from_numpy(recs).to(dev), torch.from_numpy(precs).to(dev), plan(GEO[0]), plan(GEO[4])
    crop, m0 = ops.support_from_source_u8(src, msk, srec, S)
    slots = crop.view(n, -1)
    us = lambda fn: round(device_us(fn), 2)
    return dict(support_from_source=us(lambda: ops.support_from_source(src, msk, srec, lut, S)),
                support_from_source_u8=us(lambda: ops.support_from_source_u8(src, msk, srec, S)),
                photometric_u8_mixed=us(lambda: ops.photometric_u8(slots, precs)),
                support_augment_mixed=us(lambda: ops.support_augment(crop, m0, recs, lut, S)),
                support_augment_rot10=us(lambda: ops.support_augment(crop, m0, rot, lut, S)),
                support_augment_flip=us(lambda: ops.support_augment(crop, m0, flip, lut, S)),
                note=f'{n} instances at S = {S} in one launch each; "mixed": the row pairs of step 0, one operator per '
                     f'instance; mean of 20 back-to-back launches between two events (launch gaps included)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(480, 640), metavar=('h', 'w'))
    ap.add_argument('--blocks', type=int, default=4, help='blocks per arm')
    ap.add_argument('--steps', type=int, default=8, help='steps per block')
    ap.add_argument('--warmup', type=int, default=3, help='steps per arm before the first block')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the kernels alone (no model, no steps) and print their event means: the run to put under '
                         '`rocprofv3 --kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spp_augment_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    S, nk = shape['spp_size'], shape['n_ways'] * shape['k_shots']
    h, w = args.source
    rng = np.random.RandomState(0)
    dev = torch.device('cuda', torch.cuda.current_device())
    insts = [instance(rng, h, w, 40, 400) for _ in range(nk)]
    if args.kernels_only:
        lut = torch.from_numpy(ops.input_lut(MEAN, STD, 255.0)).to(dev)
        print(json.dumps(dict(tool='spp_augment_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              kernels_us=kernel_times(lut, insts, S, dev))), flush=True)
        return

    from fgn_amd.train import Trainer
    cfg = fgn_r50_c4_config(shape['n_ways'], shape['k_shots'])
    model = FGN(cfg['n_ways'], cfg['k_shots'], state_dict=init_state_dict(cfg, 0))
    model.set_input_norm(mean=MEAN, std=STD)
    trainer = Trainer(model)
    b = make_batch(0, 1, **shape)                           # the query of a seeded episode, as uint8 pixels
    H, W = shape['height'], shape['width']
    common = dict(qry_img=torch.from_numpy(pixels(rng, H, W))[None].pin_memory(), qry_bboxes=b['qry_bboxes'],
                  qry_cat_ids=b['qry_cat_ids'], qry_isegmaps=b['qry_isegmaps'], img_shape=b['img_shape'])
    ready = [fd.support_from_source(im, bb, mk, S) for im, bb, mk in insts]      # the host arm's input: ready supports
    source = dict(spp_imgs=[[torch.from_numpy(im).pin_memory() for im, _, _ in insts]],
                  spp_isegmaps=[[torch.from_numpy(mk).pin_memory() for _, _, mk in insts]],
                  spp_bboxes=torch.from_numpy(np.stack([bb for _, bb, _ in insts]))[None], spp_crop_to=S)
    for j in range(max(len(GEO), len(PHOTO))):              # every row is applied: no fallback in either arm
        geo, photo = rows_of(j, nk)
        assert not fd.support_augment_plan(geo, photo, np.stack([bx for _, bx, _ in ready]), S)[3].any()
    host_ms = []

    def step(arm, j):
        geo, photo = rows_of(j, nk)
        if arm == 'host':
            t0 = time.perf_counter()
            made = [fd.augment_support(c, bx, m, g, p) for (c, bx, m), g, p in zip(ready, geo, photo)]
            host_ms.append((time.perf_counter() - t0) * 1e3)
            batch = dict(common, spp_imgs=torch.from_numpy(np.stack([c for c, _, _ in made]))[None],
                         spp_bboxes=torch.from_numpy(np.stack([bx for _, bx, _ in made]))[None],
                         spp_isegmaps=torch.from_numpy(np.stack([m for _, _, m in made]))[None])
        else:
            batch = dict(common, **source, spp_augment=geo[None], spp_photometric=photo[None])
        torch.manual_seed(j)
        losses = trainer.step(batch)
        torch.cuda.synchronize()
        return losses

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

    kernels_us = kernel_times(model._lut_on(dev), insts, S, dev)
    sp = model._source_supports(source['spp_imgs'], source['spp_bboxes'], source['spp_isegmaps'], S)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3),
                    spread_ms=round(max(v) - min(v), 3))
    res = dict(tool='spp_augment_ab', workload=f'{args.workload} training step (Trainer.step), batch 1, eager',
               device=torch.cuda.get_device_name(0), source_hw=[h, w], S=S, supports=nk,
               geometric_rows=[r.tolist() for r in GEO], photometric_rows=[r.tolist() for r in PHOTO],
               blocks_per_arm=args.blocks, steps_per_block=args.steps, warmup_per_arm=args.warmup,
               host_arm=arm_stats(blocks['host']), device_arm=arm_stats(blocks['device']),
               host_augment_ms_per_step=dict(median=round(statistics.median(host_ms), 3), min=round(min(host_ms), 3),
                                             max=round(max(host_ms), 3),
                                             note=f'fewshot_ds.augment_support on {nk} ready supports, one core (numpy, '
                                                  f'the integer rule); INSIDE the host arm\'s step time'),
               uploaded_support_bytes_per_step=dict(host=dict(images=nk * S * S * 3, masks=nk * S * S, boxes=nk * 16),
                                                    device=dict(windows=sp['window_bytes'], boxes=nk * 16,
                                                                records=nk * 4 * (16 + 16 + 64))),
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
