#!/usr/bin/env python3
"""The reference's training loop body (mmcv EpochBasedRunner + OptimizerHook + StepLrUpdaterHook with
fgn_train_schedule.py: Adagrad lr 0.005, weight decay 1e-5, lr_mult 0.1 under roi_head, step [3] x0.1, linear
warm-up 100 iterations, 3 epochs) on the MI355X path: DataLoader(ds, collate_fn_new) -> Trainer.step(batch)
-> mmcv-style checkpoint -> the trained heads evaluated through simple_test + ds.evaluate.

    python examples/train_loop.py --dataset OMNIISEG --episodes 32 --epochs 3
    python examples/train_loop.py --dataset SYNTH --height 320 --width 480 --episodes 16
    python examples/train_loop.py --dataset SYNTH --height 320 --width 480 --episodes 16 --poly-masks
    python examples/train_loop.py --dataset OMNIISEG --source-size 320 --spp-source --augment
    python examples/train_loop.py --dataset OMNIISEG --source-size 320 --augment --photometric
    python examples/train_loop.py --dataset OMNIISEG --spp-source --augment-spp --photometric-spp
    python examples/train_loop.py --dataset OMNIISEG --source-size 320 --augment --photometric --augs coco
    python examples/train_loop.py --dataset OMNIISEG --source-size 320 --spp-source --augment --rle-masks
    python examples/train_loop.py --dataset OMNIISEG --source-size 320 --spp-source --augment --photometric --color-masks
    python examples/train_loop.py --dataset MNISTISEG --optimizer Adam --lr 0.01 --lr-policy CosineAnnealing
    python examples/train_loop.py --dataset OMNIISEG --optimizer SGD --grad-clip 35 --cumulative-iters 4

``--source-size S``: the loader hands over decoded S x S pixels and the detector resizes them on the GPU
(``qry_resize_to``); ``--spp-source``: the supports are cut from their source images on the GPU (``spp_crop_to``);
``--augment`` (needs ``--source-size``): the queries are augmented on the GPU together with the resize
(``qry_augment``: flip, affine warp, channel order, drawn per image and epoch - ``augment_qry=True`` of the reference's
training configurations); ``--photometric`` (needs ``--augment``): the other six operators of the reference's
``augs_seq`` - Gaussian and impulse noise, blur, hue, saturation, brightness - run on the source pixels on the GPU as
well (``qry_photometric``), and both rows come from one joint draw.  ``--augment-spp`` (needs ``--spp-source``): every
support instance is augmented on the GPU behind its cut (``spp_augment``, one row per instance and epoch -
``augment_spp=True`` of the reference's training configurations); ``--photometric-spp`` (needs ``--augment-spp``): the
photometric operators as well (``spp_photometric``).  ``--augs coco``: the rows are drawn like COCO's ``augs_seq`` (flip,
one of hue / saturation / brightness, then a blur) and the photometric half travels as a chain of two operators per image
(``qry_photometric_chain`` / ``spp_photometric_chain``), which one kernel applies in one pass.  ``--rle-masks``: the
ground-truth masks (with ``--spp-source`` the support masks too) travel as COCO RLE, the form the reference's COCO
dataset holds them in, and are decoded on the GPU.  ``--color-masks`` (needs ``--source-size`` or ``--spp-source``: the
images travel as bytes): the masks travel as box + colour, all the character datasets store, and are made on the GPU
from the image bytes as uploaded, ahead of any augmentation.  ``--poly-masks`` (``--dataset SYNTH``): the synthetic
instances are polygons and their masks travel as COCO polygons, rasterised on the GPU; ``--poly-dense``: the same
episodes with ``polygon.dense`` of the same vertices handed over dense - the same losses and weights.  The evaluation at the end is without augmentation.

``--optimizer`` chooses among the three optimizers the schedule files list (Adagrad; Adam; SGD with momentum 0.9 and
Nesterov), ``--grad-clip MAX_NORM`` is mmcv's ``optimizer_config.grad_clip`` (global L2 norm, logged as ``grad_norm``),
``--cumulative-iters N`` its GradientCumulativeOptimizerHook (an update every N iterations; what is pending at the end
of the run is applied by ``Trainer.flush()``), ``--lr-policy`` one of the three learning-rate policies of ``lr_config``
(Step [3] x0.1; Fixed; CosineAnnealing to 0.01 of the base), each with the linear warm-up of 100 iterations.

The backbone is frozen as in fgn_r50_c4_densecl.py:31; with no pretrained checkpoint here it is randomly
initialised, so this demonstrates the loop (losses fall on the training episodes), not a trained detector.
"""
import argparse
import os
import sys
import tempfile
import time

import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgn_amd.detector import FGN                          # noqa: E402
from fgn_amd.episodes import collate                      # noqa: E402
from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG, SyntheticFewShotISEG   # noqa: E402
from fgn_amd.train import Trainer, scheduled_lr          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=16)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--n-ways', type=int, default=3)
    ap.add_argument('--k-shots', type=int, default=1)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--dataset', default='OMNIISEG', choices=['SYNTH', 'MNISTISEG', 'OMNIISEG'])
    ap.add_argument('--lr', type=float, default=0.005)
    ap.add_argument('--checkpoint', default=None, help='mmcv checkpoint to start from')
    ap.add_argument('--save', default=None)
    ap.add_argument('--source-size', type=int, default=None, help='decoded S x S query images, resized on the GPU')
    ap.add_argument('--spp-source', action='store_true', help='supports cut from their source images on the GPU')
    ap.add_argument('--augment', action='store_true', help='augment the queries on the GPU (needs --source-size)')
    ap.add_argument('--photometric', action='store_true',
                    help='noise, blur, hue, saturation, brightness on the GPU as well (needs --augment)')
    ap.add_argument('--augment-spp', action='store_true',
                    help='augment every support instance on the GPU behind its cut (needs --spp-source)')
    ap.add_argument('--photometric-spp', action='store_true',
                    help='the photometric operators on the supports as well (needs --augment-spp)')
    ap.add_argument('--augs', default='natural', choices=['natural', 'coco'],
                    help='the sequence the augmentation rows are drawn like: natural_fst\'s or COCO\'s (a chain)')
    ap.add_argument('--rle-masks', action='store_true',
                    help='masks travel as COCO RLE and are decoded on the GPU (character datasets)')
    ap.add_argument('--color-masks', action='store_true',
                    help='masks travel as box + colour and are made on the GPU from the image bytes (character datasets; '
                         'needs --source-size or --spp-source)')
    ap.add_argument('--poly-masks', action='store_true',
                    help='synthetic episodes of polygonal instances; masks travel as COCO polygons, rasterised on the GPU')
    ap.add_argument('--poly-dense', action='store_true',
                    help='the same polygonal episodes, masks handed over dense: the other arm of --poly-masks')
    ap.add_argument('--optimizer', default='Adagrad', choices=['Adagrad', 'Adam', 'SGD'])
    ap.add_argument('--grad-clip', type=float, default=None, metavar='MAX_NORM', help='clip the global gradient L2 norm')
    ap.add_argument('--cumulative-iters', type=int, default=1, help='accumulate the gradients of N iterations per update')
    ap.add_argument('--lr-policy', default='Step', choices=['Step', 'Fixed', 'CosineAnnealing'])
    args = ap.parse_args()
    if args.rle_masks and args.dataset == 'SYNTH':
        ap.error('--rle-masks needs a character dataset (MNISTISEG, OMNIISEG)')
    if (args.poly_masks or args.poly_dense) and args.dataset != 'SYNTH':
        ap.error('--poly-masks / --poly-dense need --dataset SYNTH (the character datasets hold no polygons)')
    if args.poly_masks and args.poly_dense:
        ap.error('--poly-masks and --poly-dense are the two arms of one comparison: choose one')
    if args.color_masks and args.rle_masks:
        ap.error('--color-masks and --rle-masks are two forms of one argument: choose one')
    if args.color_masks and args.source_size is None and not args.spp_source:
        ap.error('--color-masks needs --source-size or --spp-source: the detector makes the masks from the image bytes')
    if args.augment_spp and not args.spp_source:
        ap.error('--augment-spp needs --spp-source: the supports are augmented behind their cut from the source images')
    if args.photometric_spp and not args.augment_spp:
        ap.error('--photometric-spp needs --augment-spp: the two rows of an instance are one joint draw')
    if args.photometric and not args.augment:
        ap.error('--photometric needs --augment: the two are one joint draw of the reference\'s augs_seq')
    source = args.source_size is not None or args.spp_source
    if (source or args.augment) and args.dataset == 'SYNTH':
        ap.error('--source-size / --spp-source / --augment need a character dataset (MNISTISEG, OMNIISEG)')
    if args.augment and args.source_size is None:
        ap.error('--augment needs --source-size: the query is augmented together with its resize')
    if args.dataset == 'SYNTH':
        ds = SyntheticFewShotISEG(args.n_ways, args.k_shots, args.episodes, args.height, args.width, batch=args.batch,
                                  polygons='poly' if args.poly_masks else 'dense' if args.poly_dense else None)
    else:
        ds = ClutteredCharsFewShotISEG(args.dataset, args.n_ways, args.k_shots, n_imgs=args.episodes,
                                       img_size=128 if args.dataset == 'MNISTISEG' else 256, batch=args.batch,
                                       raw_uint8=source, source_size=args.source_size, spp_source=args.spp_source,
                                       augment_qry=args.augment, photometric_qry=args.photometric,
                                       augment_spp=args.augment_spp, photometric_spp=args.photometric_spp,
                                       augs=args.augs, rle_masks=args.rle_masks, color_masks=args.color_masks)
    model = FGN(args.n_ways, args.k_shots)
    if source:
        model.set_input_norm(**ds.input_norm)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'))
    trainer = Trainer(model, lr=args.lr, optimizer=args.optimizer, cumulative_iters=args.cumulative_iters,
                      grad_clip=None if args.grad_clip is None else dict(max_norm=args.grad_clip, norm_type=2))
    lr_config = dict({'Step': dict(policy='Step', step=[3], gamma=0.1, min_lr=0.000001), 'Fixed': dict(policy='Fixed'),
                      'CosineAnnealing': dict(policy='CosineAnnealing', min_lr_ratio=0.01)}[args.lr_policy],
                     warmup='linear', warmup_iters=100, warmup_ratio=0.01)
    it = 0
    for epoch in range(args.epochs):
        if args.augment or args.augment_spp:
            ds.reshuffle(e=epoch)                             # (another epoch, another draw of the augmentation)
        else:
            ds.reshuffle()
        loader = DataLoader(ds, batch_size=ds.batch, num_workers=2, collate_fn=collate)
        t0, tot, n = time.perf_counter(), {}, 0
        for data in loader:
            trainer.set_lr(scheduled_lr(lr_config, args.lr, it, epoch, args.epochs))
            losses = trainer.step(data)
            for k, v in losses.items():
                tot[k] = tot.get(k, 0.0) + float(v[0] if isinstance(v, list) else v)
            it, n = it + 1, n + 1
        dt = time.perf_counter() - t0
        print(f'epoch {epoch}: {n} iterations in {dt:.2f} s, lr {trainer.lr:.2e}, ' +
              ', '.join(f'{k} {v / n:.4f}' for k, v in tot.items()))
    trainer.flush()                                           # a pending partial accumulation (mmcv: remainder_iters)
    sd = trainer.state_dict()
    if args.save:
        torch.save(trainer.checkpoint(meta={'iter': it, 'epoch': args.epochs}), args.save)   # resumable: Trainer.resume
    model.load_state_dict(sd)
    with tempfile.TemporaryDirectory() as work_dir:
        loader = DataLoader(ds, batch_size=ds.batch, num_workers=2, collate_fn=collate)
        results = [r for data in loader
                   for r in model.simple_test(**{k: v for k, v in data.items()
                                                 if k not in ('qry_augment', 'qry_photometric', 'spp_augment',
                                                              'spp_photometric', 'qry_photometric_chain',
                                                              'spp_photometric_chain')}, rescale=True)]
        print(ds.evaluate(results=results, model_dir=work_dir))


if __name__ == '__main__':
    main()
