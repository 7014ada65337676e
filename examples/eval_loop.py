#!/usr/bin/env python3
"""The reference's evaluation loop (OptEvalHook._do_evaluate, main.py:269-326) on the MI355X path:
DataLoader(ds, batch_size=ds.batch, collate_fn=collate_fn_new) -> model.simple_test(**data, rescale=True)
-> chunked result pickles -> ds.evaluate(results_pkl_dir_fp=...).

    python examples/eval_loop.py --episodes 8 --batch 2 --height 320 --width 480
    python examples/eval_loop.py --dataset OMNIISEG --episodes 16 --n-ways 3 --k-shots 1     (cfg2-shaped)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --uint8      (decoded pixels in, normalised on the GPU)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --source-size 200     (200^2 sources, resized to 128^2 on the GPU)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --source-size 200 --results-at-source     (... results in the 200^2 frame)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --spp-source     (supports cropped, resized and padded on the GPU)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --spp-source --rle-masks     (masks travel as COCO RLE, decoded on the GPU)
    python examples/eval_loop.py --dataset MNISTISEG --episodes 16 --spp-source --color-masks     (masks travel as box + colour, made on the GPU from the image bytes)
    python examples/eval_loop.py --episodes 8 --poly-masks     (polygonal instances; masks travel as COCO polygons, rasterised on the GPU)
    python examples/eval_loop.py --episodes 8 --poly-dense     (the same episodes and the same truth, masks handed over dense)
    python examples/eval_loop.py --episodes 8 --match-on-device     (mask overlaps counted on the GPU: the evaluator decodes no RLE)
    python examples/eval_loop.py --episodes 8 --eval-on-device --iou-thrs coco     (greedy matching on the GPU too; AP at COCO's ten thresholds)
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
from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG, SyntheticFewShotISEG, write_chunked   # noqa: E402
from fgn_amd.fsiseg_eval import COCO_IOU_THRS, evaluate_results_multi                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=8)
    ap.add_argument('--batch', type=int, default=4)       # eval_ds_cfg batch of the reference
    ap.add_argument('--n-ways', type=int, default=3)
    ap.add_argument('--k-shots', type=int, default=3)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1333)
    ap.add_argument('--dataset', default='SYNTH', choices=['SYNTH', 'MNISTISEG', 'OMNIISEG'])
    ap.add_argument('--checkpoint', default=None, help='mmcv checkpoint of a trained reference FGN')
    ap.add_argument('--uint8', action='store_true',
                    help='character datasets: the loader yields uint8 pixels, the detector normalises them on the GPU')
    ap.add_argument('--source-size', type=int, default=None, metavar='S',
                    help='character datasets: queries are generated at S x S and stay at that size in the loader; the '
                         'detector resizes image and masks to the network size on the GPU (qry_resize_to; implies --uint8)')
    ap.add_argument('--results-at-source', action='store_true',
                    help='with --source-size: boxes, masks, ground truth and overlap counts of the results are in the frame '
                         'of the S x S source image (results_at_source), no ground-truth mask is resized')
    ap.add_argument('--spp-source', action='store_true',
                    help='character datasets: the loader hands over the supports\' source images, masks and boxes; the '
                         'detector crops, resizes and pads them on the GPU (spp_crop_to; implies --uint8)')
    ap.add_argument('--rle-masks', action='store_true',
                    help='character datasets: the loader yields the ground-truth masks as COCO RLE dicts (the form the '
                         'reference\'s COCO dataset holds them in), with --spp-source the support masks too; the detector '
                         'decodes them on the GPU and only their runs are uploaded')
    ap.add_argument('--color-masks', action='store_true',
                    help='character datasets: the loader yields the ground-truth masks as box + colour, all that MNISTISEG / '
                         'OMNIISEG store per instance, with --spp-source the support masks too; the detector makes the '
                         'masks on the GPU from the image bytes (implies --uint8; not beside --rle-masks)')
    ap.add_argument('--poly-masks', action='store_true',
                    help='synthetic episodes: the instances are polygons and the loader yields the ground-truth masks as '
                         'COCO polygons ({\'polygons\': [...], \'size\': [h, w]}); the detector rasterises them on the GPU and '
                         'only their vertices are uploaded')
    ap.add_argument('--poly-dense', action='store_true',
                    help='synthetic episodes: the same polygonal instances with their masks handed over dense '
                         '(polygon.dense of the same vertices): the other arm of --poly-masks, same results')
    ap.add_argument('--match-on-device', action='store_true',
                    help='count the overlaps of detections and ground truth on the GPU (FGN.match_on_device): the results '
                         'carry dt_gt_inter / dt_area / gt_area and the evaluator decodes no RLE')
    ap.add_argument('--eval-on-device', action='store_true',
                    help="match detections to ground truth on the GPU as well (FGN.evaluate_on_device; implies the counts): "
                         'the results carry one matched bit per detection, IoU type and threshold, and the evaluator forms '
                         'no IoU')
    ap.add_argument('--iou-thrs', default=None, metavar='T',
                    help="IoU thresholds to report besides the reference's 0.5: 'coco' (0.5:0.05:0.95) or a comma-separated "
                         'list of at most 16 (evaluate_results_multi; with --eval-on-device they are matched on the GPU)')
    args = ap.parse_args()
    args.uint8 = args.uint8 or args.source_size is not None or args.spp_source or args.color_masks
    if args.results_at_source and args.source_size is None:
        ap.error('--results-at-source needs --source-size')
    if args.rle_masks and args.dataset == 'SYNTH':
        ap.error('--rle-masks needs --dataset MNISTISEG or OMNIISEG')
    if args.color_masks and args.rle_masks:
        ap.error('--color-masks and --rle-masks are two forms of one argument: choose one')
    if (args.poly_masks or args.poly_dense) and args.dataset != 'SYNTH':
        ap.error('--poly-masks / --poly-dense need --dataset SYNTH (the character datasets hold no polygons)')
    if args.poly_masks and args.poly_dense:
        ap.error('--poly-masks and --poly-dense are the two arms of one comparison: choose one')
    if args.uint8 and args.dataset == 'SYNTH':
        ap.error('--uint8 / --source-size / --spp-source need --dataset MNISTISEG or OMNIISEG (the synthetic images are Gaussian floats, not pixels)')

    if args.dataset == 'SYNTH':
        ds = SyntheticFewShotISEG(args.n_ways, args.k_shots, args.episodes, args.height, args.width, batch=args.batch,
                                  polygons='poly' if args.poly_masks else 'dense' if args.poly_dense else None)
    else:       # cluttered characters: 128^2 (MNISTISEG, cfg1) / 256^2 (OMNIISEG, cfg2) queries, 128^2 supports
        ds = ClutteredCharsFewShotISEG(args.dataset, args.n_ways, args.k_shots, n_imgs=args.episodes,
                                       img_size=128 if args.dataset == 'MNISTISEG' else 256, batch=args.batch,
                                       raw_uint8=args.uint8, source_size=args.source_size, spp_source=args.spp_source,
                                       rle_masks=args.rle_masks, color_masks=args.color_masks)
    model = FGN(args.n_ways, args.k_shots)
    if args.uint8:
        model.set_input_norm(**ds.input_norm)
    model.match_on_device = args.match_on_device
    iou_thrs = None
    if args.iou_thrs is not None:
        iou_thrs = COCO_IOU_THRS if args.iou_thrs == 'coco' else tuple(float(t) for t in args.iou_thrs.split(','))
    model.evaluate_on_device = args.eval_on_device
    if args.eval_on_device and iou_thrs is not None:
        model.eval_iou_thrs = iou_thrs if 0.5 in iou_thrs else (0.5,) + tuple(iou_thrs)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location='cpu'))
    # (source-size queries of one size stack like any other; a real loader hands qry_img over as a list when they differ)
    loader = DataLoader(ds, batch_size=ds.batch, num_workers=2, collate_fn=collate)

    kept = []

    def results():
        for data in loader:
            res = model.simple_test(**data, rescale=True, results_at_source=args.results_at_source)
            if iou_thrs is not None:
                kept.extend(res)
            yield res

    with tempfile.TemporaryDirectory() as work_dir:
        out = os.path.join(work_dir, 'ResultsChunked')
        t0 = time.perf_counter()
        write_chunked(results(), out)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        metrics = ds.evaluate(results_pkl_dir_fp=out, model_dir=work_dir)
        de = time.perf_counter() - t0
    print(f'{len(ds)} episodes in {dt:.2f} s ({len(ds) / dt:.1f} img/s incl. data loading and H2D), '
          f'evaluation {de:.2f} s ({de / len(ds) * 1e3:.1f} ms per image)')
    print(metrics)
    if iou_thrs is not None:
        t0 = time.perf_counter()
        multi = evaluate_results_multi(kept, args.n_ways, iou_thrs)
        print(f'{len(iou_thrs)} thresholds in {time.perf_counter() - t0:.2f} s:',
              {k: round(v, 4) for k, v in multi.items() if k.endswith(('mAP', 'mAR'))})


if __name__ == '__main__':
    main()
