#!/usr/bin/env python3
"""A/B of the two ways a support set reaches ``FGN.simple_test`` on one GPU, one process.

Arm A ('host'): the loader builds every support on a core - crop, bicubic resize, centre pad (``get_support``,
base_fst.py:1043-1167) - and the detector gets N*K ready S x S uint8 crops with their masks: the existing path.  The
loader's work is done ahead of the timed episodes and reported separately as host milliseconds on one core: the float
``support_from_instance`` (what the datasets do today) and the integer ``support_from_source``.  Arm B ('device'): the
instances' source images, masks and boxes with ``spp_crop_to``; its episode time INCLUDES the host part of the new path
(``support_geometry`` per instance and cutting the windows).

cfg3 shapes, 480x640 sources with instances of 40..400 pixels (some upscaled to S, some downscaled), graph replay, pinned
host tensors, transfers on the caller stream (bench.py's arrangement at one episode per step), one episode in flight:
the episode time is the host clock from ``detect_device`` to the end of ``pack_results``.  Arms alternate in blocks; per
arm the block medians, their median and spread (max - min).  Arm A is timed only; arm B's bytes are what
tests/test_hip_spp_source_e2e.py pins.  Beside them the bytes an episode uploads for its supports and the duration of
the new kernel next to ``u8hwc3_to_nhwc4`` of the ready crops (mean of back-to-back launches between two events:
wrappers and launch gaps included).  ``--kernels-only`` runs just those launches, for a kernel trace of the kernels' own
durations.

    python tools/spp_source_ab.py --out profiles/spp_source_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/spp_source_ab.py --kernels-only
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
from fgn_amd.weights import init_state_dict                                     # noqa: E402

MEAN = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['mean'], np.float32)
STD = np.asarray(fd.ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['std'], np.float32)


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


def clock(fn, reps=3):
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(best)


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


def packed(insts, S):
    """The windows of one support set as the rows of two slot buffers, and its records."""
    recs = [fd.support_geometry(im.shape[0], im.shape[1], bb, S)[0] for im, bb, _ in insts]
    wins = [fd.support_window(im, mk, rec) for (im, _, mk), rec in zip(insts, recs)]
    src = np.zeros((len(insts), max(w.size for w, _ in wins)), np.uint8)
    msk = np.zeros((len(insts), max(m.size for _, m in wins)), np.uint8)
    for i, (w, m) in enumerate(wins):
        src[i, :w.size], msk[i, :m.size] = w.reshape(-1), m.reshape(-1)
    return torch.from_numpy(src), torch.from_numpy(msk), torch.from_numpy(np.stack(recs))


def kernel_times(lut, insts, S, dev) -> dict:
    """The support kernel beside ``u8hwc3_to_nhwc4`` of the ready crops, through their Python wrappers."""
    src, msk, recs = (t.to(dev) for t in packed(insts, S))
    crops = torch.from_numpy(np.stack([fd.support_from_source(im, bb, mk, S)[0] for im, bb, mk in insts])).to(dev)
    return dict(u8hwc3_to_nhwc4=round(device_us(lambda: ops.u8hwc3_to_nhwc4(crops, lut)), 2),
                support_from_source=round(device_us(lambda: ops.support_from_source(src, msk, recs, lut, S)), 2),
                note=f'{len(insts)} instances to {S}x{S} in one launch, window rows of {src.shape[1]} + {msk.shape[1]} '
                     f'bytes; mean of 20 back-to-back launches between two events (launch gaps included)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(480, 640), metavar=('h', 'w'))
    ap.add_argument('--extent', type=int, nargs=2, default=(40, 400), metavar=('lo', 'hi'), help='instance box sides')
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=50, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=20, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the two kernels alone (no model, no episodes) and print their event means: the run to '
                         'put under `rocprofv3 --kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spp_source_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    H, W, S = shape['height'], shape['width'], shape['spp_size']
    h, w = args.source
    nk = shape['n_ways'] * shape['k_shots']
    rng = np.random.RandomState(0)
    dev = torch.device('cuda', torch.cuda.current_device())
    if args.kernels_only:
        insts = [instance(rng, h, w, *args.extent) for _ in range(nk)]
        lut = torch.from_numpy(ops.input_lut(MEAN, STD, 255.0)).to(dev)
        print(json.dumps(dict(tool='spp_source_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              kernels_us=kernel_times(lut, insts, S, dev))), flush=True)
        return
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)
    model.set_input_norm(mean=MEAN, std=STD)

    pin = lambda t: t.pin_memory()
    eps, host_ms, sets = [], [], []
    for j in range(args.distinct):
        b = make_batch(j, 1, **shape)                       # the query side of a seeded episode
        insts = [instance(rng, h, w, *args.extent) for _ in range(nk)]
        sets.append(insts)
        host_ms.append(dict(
            float_rule=clock(lambda: [fd.support_from_instance(im, bb, mk, S) for im, bb, mk in insts]),
            integer_rule=clock(lambda: [fd.support_from_source(im, bb, mk, S) for im, bb, mk in insts]),
            geometry_and_windows=clock(lambda: model._source_supports(
                [torch.from_numpy(im) for im, _, _ in insts], np.stack([bb for _, bb, _ in insts]),
                [mk for _, _, mk in insts], S, graphed=True))))
        made = [fd.support_from_source(im, bb, mk, S) for im, bb, mk in insts]
        common = dict(qry_img=pin(torch.from_numpy(pixels(rng, H, W))[None]), img_shape=b['img_shape'])
        eps.append({'host': dict(common, spp_imgs=pin(torch.from_numpy(np.stack([c for c, _, _ in made]))[None]),
                                 spp_bboxes=pin(torch.from_numpy(np.stack([x for _, x, _ in made]))[None]),
                                 spp_isegmaps=pin(torch.from_numpy(np.stack([m for _, _, m in made]))[None]),
                                 spp_crop_to=None),
                    'device': dict(common, spp_imgs=[pin(torch.from_numpy(im)) for im, _, _ in insts],
                                   spp_bboxes=torch.from_numpy(np.stack([bb for _, bb, _ in insts])),
                                   spp_isegmaps=[pin(torch.from_numpy(mk)) for _, _, mk in insts], spp_crop_to=S)})
    nbytes = lambda t: t.numel() * t.element_size()
    sp = [model._source_supports(e['device']['spp_imgs'], e['device']['spp_bboxes'], e['device']['spp_isegmaps'], S,
                                 graphed=True) for e in eps]
    uploaded = dict(
        host=dict(supports=[sum(nbytes(e['host'][k]) for k in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps')) for e in eps]),
        device=dict(supports=[s['window_bytes'] + nbytes(s['rec']) + nbytes(s['boxes']) for s in sp],
                    of_which_window_bytes=[s['window_bytes'] for s in sp],
                    copies_per_episode=2 * nk + 2))

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   spp_crop_to=e['spp_crop_to'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'])

    n_det = [len(episode('device', j)[0]['dt_scores']) for j in range(len(eps))]
    same = all(np.array_equal(episode('host', j)[0]['dt_scores'], episode('device', j)[0]['dt_scores'])
               for j in range(len(eps)))
    for arm in ('host', 'device'):
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {'host': [], 'device': []}
    for blk in range(args.blocks):
        for arm in (('host', 'device') if blk % 2 == 0 else ('device', 'host')):      # alternate, and alternate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    kernels_us = kernel_times(model._lut_on(dev), sets[0], S, dev)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    med = lambda k: round(statistics.median(d[k] for d in host_ms), 3)
    spread = lambda k: round(max(d[k] for d in host_ms) - min(d[k] for d in host_ms), 3)
    res = dict(tool='spp_source_ab', workload=args.workload, device=torch.cuda.get_device_name(0), source_hw=[h, w],
               instance_extent=list(args.extent), support_size=S, instances_per_episode=nk, blocks_per_arm=args.blocks,
               episodes_per_block=args.episodes, warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True,
               transfer_mode=3, pinned_inputs=True, detections_per_episode=n_det, arms_agree_on_scores=bool(same),
               graphs=len(model._graphs), host_arm=arm_stats(blocks['host']), device_arm=arm_stats(blocks['device']),
               host_support_ms_per_episode=dict(
                   float_rule=med('float_rule'), float_rule_spread=spread('float_rule'),
                   integer_rule=med('integer_rule'), integer_rule_spread=spread('integer_rule'),
                   geometry_and_windows=med('geometry_and_windows'),
                   note='one core, all instances of an episode; float_rule = fewshot_ds.support_from_instance (torch '
                        'bicubic: what the loader does today, removed by the device arm), integer_rule = '
                        'support_from_source (numpy), geometry_and_windows = FGN._source_supports, what stays on the host in the device arm '
                        '(inside its episode time); spread = max - min over the distinct episodes'),
               uploaded_bytes_per_episode=uploaded, kernels_us=kernels_us)
    res['device_minus_host_median_ms'] = round(res['device_arm']['median_ms'] - res['host_arm']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
