#!/usr/bin/env python3
"""A/B of the two image input forms of ``FGN.simple_test`` on one GPU, one process: float32 NCHW tensors normalised on
the host (the data loader's ``ToTensor`` + ``Normalize``) against uint8 channels-last pixels normalised on the device
(``FGN.set_input_norm``).  cfg3 shapes by default, graph replay, pinned host tensors, transfers on the caller stream
(bench.py's arrangement at one episode per step), one episode in flight: the episode time is the host clock from
``detect_device`` to the end of ``pack_results`` (which waits for the results).

Arms alternate in blocks; per arm the median episode time of every block, the median and the spread (max - min) of those
block medians.  Beside them what the uint8 form is for: the host time of the normalisation it removes (measured here on
one core, against nothing) and the bytes an episode uploads.  Both arms see the same pixels, and their results are
compared byte for byte before anything is timed.

    python tools/u8_input_ab.py --out profiles/u8_input_ab.json
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
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG                        # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402

MEAN = np.asarray(ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['mean'], np.float32)
STD = np.asarray(ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']['std'], np.float32)


def host_norm(img_u8: np.ndarray) -> np.ndarray:
    """``ClutteredCharsFewShotISEG._norm``: what the loader does per image when the detector takes floats."""
    return ((img_u8.astype(np.float32) / 255.0 - MEAN) / STD).transpose(2, 0, 1).copy()


def pixels(rng, h, w):
    """A page-like image: white ground, dark tinted blobs (values over the whole byte range)."""
    img = np.full((h, w, 3), 255, np.uint8)
    for _ in range(24):
        y, x = int(rng.randint(0, h - 8)), int(rng.randint(0, w - 8))
        dy, dx = int(rng.randint(8, max(9, h // 6))), int(rng.randint(8, max(9, w // 6)))
        img[y:y + dy, x:x + dx] = rng.randint(0, 256, size=(min(dy, h - y), min(dx, w - x), 3), dtype=np.uint8)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=50, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=20, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('u8_input_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)
    model.set_input_norm(mean=MEAN, std=STD)

    H, W, S = shape['height'], shape['width'], shape['spp_size']
    nk = shape['n_ways'] * shape['k_shots']
    rng = np.random.RandomState(0)
    pin = lambda t: t.pin_memory()
    eps, prep_ms = [], []
    for j in range(args.distinct):
        b = make_batch(j, 1, **shape)                       # boxes, masks and ids of a seeded episode; images replaced
        q_u8 = pixels(rng, H, W)
        s_u8 = [pixels(rng, S, S) for _ in range(nk)]
        t0 = time.perf_counter()
        q_f = host_norm(q_u8)
        s_f = [host_norm(s) for s in s_u8]
        prep_ms.append((time.perf_counter() - t0) * 1e3)
        common = dict(spp_bboxes=pin(b['spp_bboxes']), spp_isegmaps=pin(b['spp_isegmaps']), img_shape=b['img_shape'],
                      qry_isegmaps=[pin(m) for m in b['qry_isegmaps']])
        eps.append({'f32': dict(common, qry_img=pin(torch.from_numpy(q_f)[None]),
                                spp_imgs=pin(torch.from_numpy(np.stack(s_f))[None])),
                    'u8': dict(common, qry_img=pin(torch.from_numpy(q_u8)[None]),
                               spp_imgs=pin(torch.from_numpy(np.stack(s_u8))[None]))})
    uploaded = {arm: sum(eps[0][arm][k].numel() * eps[0][arm][k].element_size()
                         for k in ('qry_img', 'spp_imgs', 'spp_bboxes', 'spp_isegmaps')) for arm in ('f32', 'u8')}

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'])

    # same pixels -> same bytes out, before anything is timed
    n_det = []
    for j in range(len(eps)):
        a, b = episode('f32', j), episode('u8', j)
        n_det.append(len(a[0]['dt_scores']))
        for k in ('dt_scores', 'dt_bboxes', 'dt_cat_ids'):
            assert a[0][k].tobytes() == b[0][k].tobytes(), (j, k)
        assert a[0]['dt_isegmaps_rle'] == b[0]['dt_isegmaps_rle'], j
    for arm in ('f32', 'u8'):
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {'f32': [], 'u8': []}
    for blk in range(args.blocks):
        for arm in (('f32', 'u8') if blk % 2 == 0 else ('u8', 'f32')):        # alternate, and alternate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    res = dict(tool='u8_input_ab', workload=args.workload, device=torch.cuda.get_device_name(0), blocks_per_arm=args.blocks,
               episodes_per_block=args.episodes, warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True,
               transfer_mode=3, pinned_inputs=True, detections_per_episode=n_det, outputs_identical=True,
               f32=arm_stats(blocks['f32']), u8=arm_stats(blocks['u8']),
               host_norm_ms_per_episode=dict(f32=round(statistics.median(prep_ms), 3), u8=0.0,
                                             note='numpy on one core: ((u8.astype(f32) / 255 - mean) / std)'
                                                  '.transpose(2, 0, 1).copy() of the query and the supports'),
               uploaded_bytes_per_episode=uploaded)
    res['u8_minus_f32_median_ms'] = round(res['u8']['median_ms'] - res['f32']['median_ms'], 4)
    res['u8_within_f32_spread'] = bool(res['u8_minus_f32_median_ms'] <= res['f32']['spread_ms'])
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
