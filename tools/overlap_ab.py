#!/usr/bin/env python3
"""A/B of the two ways the evaluator gets its mask overlaps, one GPU, one process: decoding the RLE strings of the result
dicts on the host (``_mask_iou`` / ``_rle_area``) against the exact counts ``FGN.match_on_device`` puts into them.

Three measurements, arms alternating in blocks (who goes first alternates too); per arm the median of every block,
the median and the spread (max - min) of those block medians:

  evaluator   host seconds per image of ``evaluate_results`` (bbox + segm) and of ``FSISEGEval.annotations()`` on the
              SAME result dicts with and without the three count keys (compared for equality before anything is timed);
  kernels     device microseconds (events around back-to-back calls, all launches of the op included) of
              ``ops.mask_bits`` and ``ops.mask_overlap`` on the tensors of a finished episode, beside ``ops.mask_rle``
              on the same tensors;
  episode     host clock from ``detect_device`` to the end of ``pack_results`` with the switch off and on (graph replay,
              pinned inputs, transfers on the caller stream, one episode in flight).

    python tools/overlap_ab.py --out profiles/overlap_ab.json
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
from fgn_amd import ops                                                         # noqa: E402
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.fsiseg_eval import COUNT_KEYS, FSISEGEval, evaluate_results        # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402


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
    ap.add_argument('--episodes', type=int, default=40, help='episodes per block (episode A/B)')
    ap.add_argument('--eval-reps', type=int, default=3, help='evaluator passes over the result list per block')
    ap.add_argument('--kernel-reps', type=int, default=100, help='back-to-back calls per block (kernel timing)')
    ap.add_argument('--warmup', type=int, default=10, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('overlap_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)
    pin = lambda t: t.pin_memory()
    eps = []
    for j in range(args.distinct):
        b = make_batch(j, 1, **shape)
        eps.append(dict(b, qry_img=pin(b['qry_img']), spp_imgs=pin(b['spp_imgs']), spp_bboxes=pin(b['spp_bboxes']),
                        spp_isegmaps=pin(b['spp_isegmaps']), qry_isegmaps=[pin(m) for m in b['qry_isegmaps']]))

    def episode(on, j, keep=None):
        e = eps[j % len(eps)]
        model.match_on_device = on
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'])
        if keep is not None:
            keep.append(dets)
        return model.pack_results(dets, 1, qry_bboxes=e['qry_bboxes'], qry_cat_ids=e['qry_cat_ids'],
                                  qry_isegmaps=e['qry_isegmaps'], img_shape=e['img_shape'])

    # ---- the result dicts of both arms: equal but for the three keys, equal evaluation
    with_counts, without = [], []
    for j in range(len(eps)):
        a, b = episode(False, j), episode(True, j)
        for k in a[0]:
            if k.endswith('_rle'):
                assert a[0][k] == b[0][k], (j, k)
            elif a[0][k] is not None:
                assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k])), (j, k)
        assert set(b[0]) - set(a[0]) == set(COUNT_KEYS)
        without += a
        with_counts += b
    n_ways = shape['n_ways']
    assert evaluate_results(with_counts, n_ways) == evaluate_results(without, n_ways)
    n_img = len(without)

    def eval_block(res):
        def run():
            t = []
            for _ in range(args.eval_reps):
                t0 = time.perf_counter()
                evaluate_results(res, n_ways)
                t1 = time.perf_counter()
                FSISEGEval(results=res, n_ways=n_ways).annotations()
                t2 = time.perf_counter()
                t.append(((t1 - t0) / n_img, (t2 - t1) / n_img))
            return statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
        return run
    ev = alternate({'decode_rle': eval_block(without), 'device_counts': eval_block(with_counts)}, args.blocks)
    evaluator = {arm: dict(evaluate_results=arm_stats([x[0] for x in v], 's_per_image', 6),
                           annotations=arm_stats([x[1] for x in v], 's_per_image', 6)) for arm, v in ev.items()}

    # ---- the kernels, on the device tensors of one finished episode
    keep = []
    model.use_graphs = False                      # eager outputs: tensors of this episode alone
    episode(False, 0, keep)
    torch.cuda.synchronize()
    d = keep[0][0]
    e = eps[0]
    gt = e['qry_isegmaps'][0].cuda()
    ih, iw = d['img_hw']
    thr = model.cfg['test_cfg']['rcnn']['mask_thr_binary']
    bits = ops.mask_bits(gt)

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
    kern = alternate({
        'mask_rle': timed(lambda: ops.mask_rle(d['mask_prob'], d['det_bboxes'], ih, iw, thr, d['n_dets'])),
        'mask_bits': timed(lambda: ops.mask_bits(gt)),
        'mask_overlap': timed(lambda: ops.mask_overlap(d['mask_prob'], d['det_bboxes'], bits, ih, iw, thr, d['n_dets'])),
    }, args.blocks)
    kernels = {k: arm_stats(v, 'us', 2) for k, v in kern.items()}
    n_det = int(d['n_dets'].cpu()[0])
    model.use_graphs = True

    # ---- the episode, switch off / on
    for on in (False, True):
        for j in range(args.warmup):
            episode(on, j)
    torch.cuda.synchronize()

    def episode_block(on):
        def run():
            t = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(on, j)
                t.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(t)
        return run
    epi = alternate({'off': episode_block(False), 'on': episode_block(True)}, args.blocks)
    model.match_on_device = False

    res = dict(tool='overlap_ab', workload=args.workload, device=torch.cuda.get_device_name(0), blocks_per_arm=args.blocks,
               images=n_img, detections_per_image=[len(r['dt_scores']) for r in without],
               gt_masks_per_image=[len(r['qry_isegmaps_rle']) for r in without], results_identical=True,
               evaluator=dict(passes_per_block=args.eval_reps, **evaluator),
               kernels=dict(calls_per_block=args.kernel_reps, detections=n_det, gt_masks=int(gt.shape[0]),
                            note='device events around back-to-back calls of the op: every launch of the op is inside '
                                 '(mask_bits: zero fill + pack; mask_overlap: zero fill + count + the copy of gt_area)',
                            **kernels),
               episode=dict(episodes_per_block=args.episodes, warmup_per_arm=args.warmup, hip_graph=True, transfer_mode=3,
                            episodes_in_flight=1, off=arm_stats(epi['off'], 'ms'), on=arm_stats(epi['on'], 'ms')))
    res['episode']['on_minus_off_median_ms'] = round(res['episode']['on']['median_ms'] - res['episode']['off']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
