#!/usr/bin/env python3
"""A/B of the two ways the evaluator learns which detections matched, one GPU, one process: the greedy matching in
Python on the overlap counts of the result dicts (``FGN.match_on_device``) against the matched bits
``FGN.evaluate_on_device`` puts into them (``ops.eval_match``).

Three measurements, arms alternating in blocks (who goes first alternates too); per arm the median of every block,
the median and the spread (max - min) of those block medians:

  evaluator   host seconds per image of ``evaluate_results`` (bbox + segm at 0.5) and of ``evaluate_results_multi`` at
              COCO's ten thresholds on the SAME result dicts with and without the flag keys (compared for equality
              before anything is timed);
  kernels     device microseconds (events around back-to-back calls, all launches and uploads of the op included) of
              ``ops.eval_match`` at 1 and at 10 thresholds - and of its launch alone, the host operands already on the
              device - beside ``ops.mask_overlap`` and ``ops.mask_rle`` on the tensors of the same finished episode;
  gather      bytes per episode of the records ``dist.pack_detections`` and ``dist.pack_matches`` make of it.

    python tools/eval_match_ab.py --out profiles/eval_match_ab.json
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
from fgn_amd import dist as fdist, lib, ops                                         # noqa: E402
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.fsiseg_eval import (COCO_IOU_THRS, _xywh, evaluate_results, evaluate_results_multi,   # noqa: E402
                                 match_flags)
from fgn_amd.weights import init_state_dict                                     # noqa: E402

FLAG_KEYS = ('dt_match_bbox', 'dt_match_segm', 'eval_iou_thrs', 'gt_per_cat')


def arm_stats(v, unit, digits=4):
    return {f'block_medians_{unit}': [round(x, digits) for x in v], f'median_{unit}': round(statistics.median(v), digits),
            f'spread_{unit}': round(max(v) - min(v), digits)}


def alternate(arms: dict, blocks: int):
    """arms: name -> callable returning one block's figure; returns name -> list of block figures"""
    out = {k: [] for k in arms}
    names = list(arms)
    for blk in range(blocks):
        for name in (names if blk % 2 == 0 else names[::-1]):
            out[name].append(arms[name]())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--eval-reps', type=int, default=3, help='evaluator passes over the result list per block')
    ap.add_argument('--kernel-reps', type=int, default=100, help='back-to-back calls per block (kernel timing)')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes evaluated')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_match_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    n_ways = shape['n_ways']
    cfg = with_caps(fgn_r50_c4_config(n_ways, shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    thrs = tuple(COCO_IOU_THRS)
    model.eval_iou_thrs = thrs
    eps = [make_batch(j, 1, **shape) for j in range(args.distinct)]

    def episode(evaluate, j, keep=None):
        e = eps[j]
        model.match_on_device, model.evaluate_on_device = not evaluate, evaluate
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'], qry_bboxes=e['qry_bboxes'], qry_cat_ids=e['qry_cat_ids'])
        if keep is not None:
            keep.append(dets)
        return model.pack_results(dets, 1, qry_bboxes=e['qry_bboxes'], qry_cat_ids=e['qry_cat_ids'],
                                  qry_isegmaps=e['qry_isegmaps'], img_shape=e['img_shape'])

    # ---- the result dicts of both arms: equal but for the flag keys, the flags are the host rule's, equal evaluation
    counts, flagged, keep = [], [], []
    for j in range(len(eps)):
        a, b = episode(False, j), episode(True, j, keep)
        assert set(b[0]) - set(a[0]) == set(FLAG_KEYS)
        for kind in ('bbox', 'segm'):
            assert np.array_equal(b[0]['dt_match_' + kind], match_flags(a[0], thrs, kind, n_ways=n_ways)), (j, kind)
        counts += a
        flagged += b
    model.match_on_device = model.evaluate_on_device = False
    assert evaluate_results(flagged, n_ways) == evaluate_results(counts, n_ways)
    assert evaluate_results_multi(flagged, n_ways, thrs) == evaluate_results_multi(counts, n_ways, thrs)
    n_img = len(counts)

    def eval_block(res):
        def run():
            t = []
            for _ in range(args.eval_reps):
                t0 = time.perf_counter()
                evaluate_results(res, n_ways)
                t1 = time.perf_counter()
                evaluate_results_multi(res, n_ways, thrs)
                t2 = time.perf_counter()
                t.append(((t1 - t0) / n_img, (t2 - t1) / n_img))
            return statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
        return run
    ev = alternate({'host_matching': eval_block(counts), 'device_flags': eval_block(flagged)}, args.blocks)
    evaluator = {arm: dict(evaluate_results=arm_stats([x[0] for x in v], 's_per_image', 6),
                           evaluate_results_multi=arm_stats([x[1] for x in v], 's_per_image', 6)) for arm, v in ev.items()}

    # ---- the kernels, on the device tensors of one finished (eager) episode
    torch.cuda.synchronize()
    d, e = keep[0][0], eps[0]
    gt = e['qry_isegmaps'][0].cuda()
    ih, iw = d['img_hw']
    thr = model.cfg['test_cfg']['rcnn']['mask_thr_binary']
    bits = ops.mask_bits(gt)
    ov = ops.mask_overlap(d['mask_prob'], d['det_bboxes'], bits, ih, iw, thr, d['n_dets'])
    xywh = _xywh(np.asarray(e['qry_bboxes'][0]))
    cats = np.asarray(e['qry_cat_ids'][0]).reshape(-1)

    def timed(fn):
        def run():
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            torch.cuda.synchronize()
            s.record()
            for _ in range(args.kernel_reps):
                fn()
            t.record()
            t.synchronize()
            return s.elapsed_time(t) * 1e3 / args.kernel_reps
        return run

    def match(t):
        return lambda: ops.eval_match(d['det_bboxes'], d['det_labels'], xywh, cats, t, n_ways, overlap=ov, n_dev=d['n_dets'])

    def launch(t):
        # the launch alone: the host operands ([thr | gt_xywh | gt_cat] as ``ops.eval_match`` uploads them) are on the device
        tt = np.minimum(np.asarray(t, np.float64), 1 - 1e-10)
        blob = torch.from_numpy(np.concatenate([tt.view(np.uint8), xywh.reshape(-1).view(np.uint8),
                                                cats.astype(np.int32).view(np.uint8)])).cuda()
        out = torch.empty((2, d['det_bboxes'].shape[0]), device='cuda', dtype=torch.int32)
        fn, base, g = lib.load().fgn_eval_match_i32, blob.data_ptr(), len(cats)
        a = (d['det_bboxes'].data_ptr(), 5, d['det_labels'].data_ptr(), d['n_dets'].data_ptr(), ov[0].data_ptr(),
             ov[1].data_ptr(), ov[2].data_ptr(), base + 8 * len(tt), base + 8 * len(tt) + 32 * g, base, out.data_ptr(),
             out.shape[1], g, len(tt), n_ways, 100, 0, 0, 0, 0)

        def run():
            keep_alive = blob                                        # noqa: F841
            lib.check(fn(*a, torch.cuda.current_stream().cuda_stream), 'fgn_eval_match_i32')
        return run
    kern = alternate({
        'mask_rle': timed(lambda: ops.mask_rle(d['mask_prob'], d['det_bboxes'], ih, iw, thr, d['n_dets'])),
        'mask_overlap': timed(lambda: ops.mask_overlap(d['mask_prob'], d['det_bboxes'], bits, ih, iw, thr, d['n_dets'])),
        'eval_match_1thr': timed(match((0.5,))),
        'eval_match_10thr': timed(match(thrs)),
        'eval_match_launch_1thr': timed(launch((0.5,))),
        'eval_match_launch_10thr': timed(launch(thrs)),
    }, args.blocks)
    kernels = {k: arm_stats(v, 'us', 2) for k, v in kern.items()}

    # ---- the two gathers: bytes per episode
    max_det = d['det_bboxes'].shape[0]
    recs, cnts = fdist.pack_detections(keep[0], max_det)
    m_recs, m_head = fdist.pack_matches(keep[0], max_det, n_ways)
    gather = dict(max_det=max_det,
                  detections_bytes_per_episode=(recs[0].numel() + 1) * recs.element_size(),
                  matches_bytes_per_episode=(m_recs[0].numel() + m_head[0].numel()) * m_recs.element_size())

    res = dict(tool='eval_match_ab', workload=args.workload, device=torch.cuda.get_device_name(0), blocks_per_arm=args.blocks,
               images=n_img, iou_thrs=list(thrs), detections_per_image=[len(r['dt_scores']) for r in counts],
               gt_per_image=[len(r['qry_cat_ids']) for r in counts], results_identical=True,
               evaluator=dict(passes_per_block=args.eval_reps, **evaluator),
               kernels=dict(calls_per_block=args.kernel_reps, detections=int(d['n_dets'].cpu()[0]), gt=int(gt.shape[0]),
                            note='device events around back-to-back calls of the op: every launch of the op is inside '
                                 '(eval_match: the upload of thresholds / ground-truth boxes and labels from pageable '
                                 'host memory + the kernel - back to back that upload paces the loop; eval_match_launch: '
                                 'the kernel alone; mask_overlap: zero fill + count + the copy of gt_area)', **kernels),
               gather=gather)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
