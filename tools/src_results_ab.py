#!/usr/bin/env python3
"""A/B of the two frames ``FGN.simple_test`` can return the results of source-size queries in, one GPU, one process.

Both arms feed source-size pixels, masks and ``qry_resize_to`` with ``match_on_device`` on.  Arm A ('network'): the
results are in the network frame - the ground-truth masks are resized to the network size on the device, one RLE launch
per image pastes at the network size.  Arm B ('source', ``results_at_source``): the ground truth is encoded and
bit-packed as given, one RLE launch for the batch pastes at each image's own size.

cfg3 shapes, 480x640 sources, four ground-truth masks, graph replay, pinned host tensors, transfers on the caller stream
(bench.py's arrangement at one episode per step), one episode in flight: the episode time is the host clock from
``detect_device`` to the end of ``pack_results``.  Arms alternate in blocks; per arm the block medians, their median and
spread (max - min).  Beside them, per arm, the device time of the launches that differ - the detections' RLE, the
ground-truth work (resize / RLE / bit planes) and the overlap counts, on the mask probabilities and boxes of a real
episode: mean of back-to-back launches between two events, wrappers and launch gaps included - and the evaluator's
host time per episode on the arm's result dicts.

    python tools/src_results_ab.py --out profiles/src_results_ab.json
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
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.fsiseg_eval import evaluate_results                                # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402

MEAN = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['mean'], np.float32)
STD = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['std'], np.float32)
ARMS = ('network', 'source')


def pixels(rng, h, w):
    """A page-like image: white ground, dark tinted blobs (values over the whole byte range)."""
    img = np.full((h, w, 3), 255, np.uint8)
    for _ in range(24):
        y, x = int(rng.randint(0, h - 8)), int(rng.randint(0, w - 8))
        dy, dx = int(rng.randint(8, max(9, h // 6))), int(rng.randint(8, max(9, w // 6)))
        img[y:y + dy, x:x + dx] = rng.randint(0, 256, size=(min(dy, h - y), min(dx, w - x), 3), dtype=np.uint8)
    return img


def blobs(rng, n, h, w):
    m = np.zeros((n, h, w), bool)
    for g in range(n):
        y, x = int(rng.randint(0, h // 2)), int(rng.randint(0, w // 2))
        m[g, y:y + int(rng.randint(16, h // 2)), x:x + int(rng.randint(16, w // 2))] = True
    return m


def device_us(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def launch_times(prob, det, n_det, masks, hw, net_hw, thr, skip_empty) -> dict:
    """Per arm, the launches of one episode (B = 1) that differ between the arms, through their Python wrappers."""
    h, w = hw
    H, W = net_hw
    src_hw = torch.tensor([[h, w]], dtype=torch.int32, device=prob.device)
    g_net = ops.resize_masks(masks, H, W)
    bits_net, bits_src = ops.mask_bits(g_net), ops.mask_bits(masks)
    out = {'network': dict(
        det_rle=device_us(lambda: ops.mask_rle(prob, det, H, W, thr, n_det, skip_empty=skip_empty)),
        gt_resize=device_us(lambda: ops.resize_masks(masks, H, W)),
        gt_rle=device_us(lambda: ops.dense_mask_rle(g_net, packed=True)),
        gt_bits=device_us(lambda: ops.mask_bits(g_net)),
        overlap=device_us(lambda: ops.mask_overlap(prob, det, bits_net, H, W, thr, n_det, skip_empty=skip_empty))),
        'source': dict(
        det_rle=device_us(lambda: ops.mask_rle_src(prob, det, src_hw, (H, W), thr, n_det, skip_empty=skip_empty)),
        gt_resize=0.0,
        gt_rle=device_us(lambda: ops.dense_mask_rle(masks, packed=True)),
        gt_bits=device_us(lambda: ops.mask_bits(masks)),
        overlap=device_us(lambda: ops.mask_overlap_src(prob, det, bits_src, (h, w), (H, W), thr, n_det,
                                                       skip_empty=skip_empty)))}
    for arm in out.values():
        arm['sum'] = round(sum(arm.values()), 2)
    out['note'] = (f'network {H}x{W}, source {h}x{w}, {masks.shape[0]} ground-truth masks, {int(n_det.item())} detections of '
                   f'a real episode; mean of 20 back-to-back launches between two events (wrappers and launch gaps included)')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(480, 640), metavar=('h', 'w'))
    ap.add_argument('--masks', type=int, default=4, help='ground-truth masks per query')
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=50, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=20, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('src_results_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.match_on_device = True
    model.transfer_stream(3)
    model.set_input_norm(mean=MEAN, std=STD)

    H, W, S = shape['height'], shape['width'], shape['spp_size']
    h, w = args.source
    model.query_source_capacity = max(int(model.query_source_capacity), 3 * h * w)
    nk = shape['n_ways'] * shape['k_shots']
    rng = np.random.RandomState(0)
    pin = lambda t: t.pin_memory()
    eps = []
    for j in range(args.distinct):
        b = make_batch(j, 1, **shape)                       # support boxes, masks and ids of a seeded episode
        q_src, m_src = pixels(rng, h, w), blobs(rng, args.masks, h, w)
        boxes = np.array([[ys.min(), xs.min(), ys.max() + 1, xs.max() + 1] for ys, xs in map(np.nonzero, m_src)], np.float32)
        eps.append(dict(spp_imgs=pin(torch.from_numpy(np.stack([pixels(rng, S, S) for _ in range(nk)]))[None]),
                        spp_bboxes=pin(b['spp_bboxes']), spp_isegmaps=pin(b['spp_isegmaps']), img_shape=b['img_shape'],
                        qry_img=pin(torch.from_numpy(q_src)[None]), qry_isegmaps=[pin(torch.from_numpy(m_src))],
                        qry_cat_ids=[torch.arange(args.masks) % shape['n_ways']],
                        qry_bboxes={'source': [boxes], 'network': [fd.scale_boxes_yxyx(boxes, h, w, H, W)]}))

    def episode(arm, j):
        e = eps[j % len(eps)]
        at_source = arm == 'source'
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'], qry_resize_to=(H, W), results_at_source=at_source)
        return model.pack_results(dets, 1, img_shape=e['img_shape'], qry_isegmaps=e['qry_isegmaps'],
                                  qry_cat_ids=e['qry_cat_ids'], qry_bboxes=e['qry_bboxes'][arm], qry_resize_to=(H, W),
                                  results_at_source=at_source)

    results = {arm: [episode(arm, j) for j in range(len(eps))] for arm in ARMS}
    n_det = [len(r[0]['dt_scores']) for r in results['source']]
    for arm in ARMS:
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {arm: [] for arm in ARMS}
    for blk in range(args.blocks):
        for arm in (ARMS if blk % 2 == 0 else ARMS[::-1]):          # alternate, and alternate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    # the launches that differ, on the detections of a real episode (eager: the tensors outlive the call)
    model.use_graphs = False
    e = eps[0]
    dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                               qry_resize_to=(H, W))
    torch.cuda.synchronize()
    d = dets[0]
    dev = d['mask_prob'].device
    launches_us = launch_times(d['mask_prob'].clone(), d['det_bboxes'].clone(), d['n_dets'].clone(),
                               e['qry_isegmaps'][0].to(dev).view(torch.uint8).contiguous(), (h, w), (H, W),
                               model.cfg['test_cfg']['rcnn']['mask_thr_binary'], model._skip_empty())
    model.release_results(dets)

    def evaluate_ms(arm):
        flat = [r for res in results[arm] for r in res]
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            evaluate_results(flat, shape['n_ways'])
            ts.append((time.perf_counter() - t0) * 1e3 / len(flat))
        return round(statistics.median(ts), 4)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    res = dict(tool='src_results_ab', workload=args.workload, device=torch.cuda.get_device_name(0), source_hw=[h, w],
               network_hw=[H, W], gt_masks=args.masks, blocks_per_arm=args.blocks, episodes_per_block=args.episodes,
               warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True, transfer_mode=3, pinned_inputs=True,
               match_on_device=True, detections_per_episode=n_det,
               network_arm=arm_stats(blocks['network']), source_arm=arm_stats(blocks['source']),
               launches_us=launches_us,
               evaluate_ms_per_episode={arm: evaluate_ms(arm) for arm in ARMS})
    res['source_minus_network_median_ms'] = round(res['source_arm']['median_ms'] - res['network_arm']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
