#!/usr/bin/env python3
"""A/B of the two ways a decoded query reaches ``FGN.simple_test`` on one GPU, one process.

Arm A ('host'): the loader resizes image and ground-truth masks to the network size (``get_query``, base_fst.py:876-887)
and the detector gets network-size uint8 pixels - the existing path.  The loader's work is done ahead of the timed
episodes and reported separately as host milliseconds on one core: the integer rule of ``fewshot_ds`` and, as the faster
stand-in for cv2.resize, PIL's bilinear.  Arm B ('device'): source-size pixels, masks and ``qry_resize_to``.

cfg3 shapes, 480x640 sources, four ground-truth masks, graph replay, pinned host tensors, transfers on the caller stream
(bench.py's arrangement at one episode per step), one episode in flight: the episode time is the host clock from
``detect_device`` to the end of ``pack_results``.  Arms alternate in blocks; per arm the block medians, their median and
spread (max - min).  Arm A is timed only; arm B's bytes are what tests/test_hip_src_resize_e2e.py pins.  Beside them the
bytes an episode uploads and the durations of the two resize kernels next to ``u8hwc3_to_nhwc4`` at the same output
size (mean of back-to-back launches between two events: wrappers and launch gaps included).  ``--kernels-only`` runs
just those launches, for a kernel trace of the kernels' own durations.

    python tools/src_resize_ab.py --out profiles/src_resize_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/src_resize_ab.py --kernels-only
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


def blobs(rng, n, h, w):
    m = np.zeros((n, h, w), bool)
    for g in range(n):
        y, x = int(rng.randint(0, h // 2)), int(rng.randint(0, w // 2))
        m[g, y:y + int(rng.randint(16, h // 2)), x:x + int(rng.randint(16, w // 2))] = True
    return m


def clock(fn, reps=3):
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(best)


def pil_bilinear(a: np.ndarray, H: int, W: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((W, H), Image.BILINEAR))


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


def kernel_times(lut, q_src, q_net, m_src, H, W, dev) -> dict:
    """The two resize kernels beside ``u8hwc3_to_nhwc4`` at the same output size, through their Python wrappers."""
    h, w = q_src.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(q_src)).reshape(1, -1).to(dev)
    src_hw = torch.tensor([[h, w]], dtype=torch.int32, device=dev)
    net = torch.from_numpy(np.ascontiguousarray(q_net))[None].to(dev)
    msk = torch.from_numpy(np.ascontiguousarray(m_src)).to(dev)
    return dict(u8hwc3_to_nhwc4=round(device_us(lambda: ops.u8hwc3_to_nhwc4(net, lut)), 2),
                resize_u8hwc3_to_nhwc4=round(device_us(lambda: ops.resize_u8_to_nhwc4(src, src_hw, lut, H, W)), 2),
                resize_mask_u8=round(device_us(lambda: ops.resize_masks(msk, H, W)), 2),
                note=f'output {H}x{W}, source {h}x{w}, {len(m_src)} masks in one launch; mean of 20 back-to-back '
                     f'launches between two events (launch gaps included)')


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
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the three kernels alone (no model, no episodes) and print their event means: the run to '
                         'put under `rocprofv3 --kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('src_resize_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    if args.kernels_only:
        H, W = shape['height'], shape['width']
        h, w = args.source
        rng = np.random.RandomState(0)
        dev = torch.device('cuda', torch.cuda.current_device())
        q_src, m_src = pixels(rng, h, w), blobs(rng, args.masks, h, w)
        lut = torch.from_numpy(ops.input_lut(MEAN, STD, 255.0)).to(dev)
        print(json.dumps(dict(tool='src_resize_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              kernels_us=kernel_times(lut, q_src, fd.resize_image_u8(q_src, H, W), m_src, H, W, dev))), flush=True)
        return
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)
    model.set_input_norm(mean=MEAN, std=STD)

    H, W, S = shape['height'], shape['width'], shape['spp_size']
    h, w = args.source
    nk = shape['n_ways'] * shape['k_shots']
    rng = np.random.RandomState(0)
    pin = lambda t: t.pin_memory()
    eps, host_ms = [], []
    for j in range(args.distinct):
        b = make_batch(j, 1, **shape)                       # support boxes, masks and ids of a seeded episode
        q_src, m_src = pixels(rng, h, w), blobs(rng, args.masks, h, w)
        host_ms.append(dict(image_rule=clock(lambda: fd.resize_image_u8(q_src, H, W)),
                            image_pil=clock(lambda: pil_bilinear(q_src, H, W)),
                            masks_rule=clock(lambda: fd.resize_masks(m_src, H, W)),
                            masks_pil=clock(lambda: [pil_bilinear(m.astype(np.uint8), H, W).astype(bool) for m in m_src])))
        q_net, m_net = fd.resize_image_u8(q_src, H, W), fd.resize_masks(m_src, H, W)
        common = dict(spp_imgs=pin(torch.from_numpy(np.stack([pixels(rng, S, S) for _ in range(nk)]))[None]),
                      spp_bboxes=pin(b['spp_bboxes']), spp_isegmaps=pin(b['spp_isegmaps']), img_shape=b['img_shape'])
        eps.append({'host': dict(common, qry_img=pin(torch.from_numpy(q_net)[None]),
                                 qry_isegmaps=[pin(torch.from_numpy(m_net))], qry_resize_to=None),
                    'device': dict(common, qry_img=pin(torch.from_numpy(q_src)[None]),
                                   qry_isegmaps=[pin(torch.from_numpy(m_src))], qry_resize_to=(H, W))})
    nbytes = lambda t: t.numel() * t.element_size()
    uploaded = {arm: dict(query=nbytes(eps[0][arm]['qry_img']), gt_masks=sum(nbytes(m) for m in eps[0][arm]['qry_isegmaps']),
                          supports=sum(nbytes(eps[0][arm][k]) for k in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps')))
                for arm in ('host', 'device')}

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'], qry_resize_to=e['qry_resize_to'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'], qry_isegmaps=e['qry_isegmaps'],
                                  qry_resize_to=e['qry_resize_to'])

    n_det = [len(episode('device', j)[0]['dt_scores']) for j in range(len(eps))]
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

    # the kernels alone, at the same output size
    dev = torch.device('cuda', torch.cuda.current_device())
    e = eps[0]
    kernels_us = kernel_times(model._lut_on(dev), e['device']['qry_img'][0].numpy(), e['host']['qry_img'][0].numpy(),
                              e['device']['qry_isegmaps'][0].numpy(), H, W, dev)

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    med = lambda k: round(statistics.median(d[k] for d in host_ms), 3)
    res = dict(tool='src_resize_ab', workload=args.workload, device=torch.cuda.get_device_name(0), source_hw=[h, w],
               network_hw=[H, W], gt_masks=args.masks, blocks_per_arm=args.blocks, episodes_per_block=args.episodes,
               warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True, transfer_mode=3, pinned_inputs=True,
               detections_per_episode=n_det, host_arm=arm_stats(blocks['host']), device_arm=arm_stats(blocks['device']),
               host_resize_ms_per_episode=dict(image_rule=med('image_rule'), image_pil=med('image_pil'),
                                               masks_rule=med('masks_rule'), masks_pil=med('masks_pil'),
                                               saved_pil=round(med('image_pil') + med('masks_pil'), 3),
                                               saved_rule=round(med('image_rule') + med('masks_rule'), 3),
                                               note='one core; rule = fewshot_ds.resize_image_u8 / resize_masks (numpy), '
                                                    'pil = PIL.Image.resize(BILINEAR), the faster stand-in for cv2.resize; '
                                                    'not part of either arm\'s episode time'),
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
