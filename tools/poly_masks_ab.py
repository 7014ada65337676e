#!/usr/bin/env python3
"""A/B of three forms the ground-truth masks of a query reach ``FGN.detect_device`` in, one GPU, one process.

Arm 'dense': ``qry_isegmaps`` as [n,H,W] bool arrays, uploaded byte per pixel.  Arm 'rle': the same masks as COCO RLE
dicts, decoded on the device.  Arm 'poly': the same masks as the COCO polygons they were made from,
``{'polygons': [...], 'size': [h, w]}``; the vertices are checked and rounded on the host (``polygon.as_polys`` and the
edge records, INSIDE the episode time), one blob of records is uploaded and ``fgn_poly_masks_u8`` makes the dense bytes
on the device in two launches.  Everything behind the dense tensor is the same in all arms.

cfg3 shapes (800x1333), the seeded polygonal episodes of ``episodes.make_batch(polygons=...)`` - star-shaped instances
whose dense truth is ``polygon.dense`` of the same vertices, so all arms see one truth -, graph replay, transfers on the
caller stream, one episode in flight: the episode time is the host clock from ``detect_device`` to the end of
``pack_results``.  Arms alternate in blocks, and who goes first rotates; per arm the block medians, their median and
spread (max - min).  Beside them the mask bytes an episode uploads per arm and the device-side step of each form (mean
of back-to-back calls between two events: the wrapper, its upload and launch gaps included).  There is no pass or fail
threshold on time: the upload is overlapped, and this record is what says whether it was on the critical path.

``--kernels-only`` runs the rasterisation alone (no model, no episodes), 3 + 20 times with a synchronisation between
calls: the run to put under a kernel trace, whose durations of ``poly_crossings_kernel`` and ``poly_fill_kernel``
exclude the wrapper, the upload and the launch gaps (profiles/poly_masks_kernel_stats.csv).

    python tools/poly_masks_ab.py --out profiles/poly_masks_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/poly_masks_ab.py --kernels-only
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
from fgn_amd import ops, polygon, rle                                                    # noqa: E402
from fgn_amd.config import fgn_r50_c4_config, with_caps                         # noqa: E402
from fgn_amd.detector import FGN                                                # noqa: E402
from fgn_amd.episodes import CONFIGS, RPN_MAX_PER_IMG, make_batch               # noqa: E402
from fgn_amd.weights import init_state_dict                                     # noqa: E402


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


def clock_ms(fn, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--episodes', type=int, default=40, help='episodes per block')
    ap.add_argument('--warmup', type=int, default=15, help='episodes per arm before the first block')
    ap.add_argument('--distinct', type=int, default=4, help='distinct episodes cycled through')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='rasterise the first episode\'s polygons alone, 3 + 20 times: the run to put under '
                         '`rocprofv3 --kernel-trace --stats`, whose durations are the kernels\' own')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('poly_masks_ab needs a GPU: a CPU run measures nothing')

    shape = CONFIGS[args.workload]
    dev = torch.device('cuda', torch.cuda.current_device())
    if args.kernels_only:
        hw = (shape['height'], shape['width'])
        p0 = polygon.as_polys(make_batch(0, 1, polygons='poly', **shape)['qry_isegmaps'][0], hw)
        for _ in range(23):
            out = ops.poly_masks(p0, device=dev)
            torch.cuda.synchronize()
        print(json.dumps(dict(tool='poly_masks_ab', kernels_only=True, device=torch.cuda.get_device_name(0),
                              masks=list(p0.shape), vertices=int(p0.xy.size // 2),
                              crossing_bound=[int(v) for v in p0.crossing_bound], calls=23,
                              bytes_written=int(out.numel()))), flush=True)
        return
    cfg = with_caps(fgn_r50_c4_config(shape['n_ways'], shape['k_shots']), rpn_max=RPN_MAX_PER_IMG.get(args.workload))
    model = FGN(cfg['n_ways'], cfg['k_shots'], test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    model.use_graphs = True
    model.transfer_stream(3)

    pin = lambda t: t.pin_memory() if isinstance(t, torch.Tensor) else t
    eps = []
    for j in range(args.distinct):
        b = {k: pin(v) for k, v in make_batch(j, 1, polygons='poly', **shape).items()}
        polys = list(b['qry_isegmaps'])
        hw = (shape['height'], shape['width'])
        dense = [pin(torch.from_numpy(polygon.as_polys(g, hw).dense()).to(torch.bool).contiguous()) for g in polys]
        runs = [rle.encode_many(g.numpy()) for g in dense]
        eps.append({'dense': dict(b, qry_isegmaps=dense), 'rle': dict(b, qry_isegmaps=runs), 'poly': dict(b, qry_isegmaps=polys)})
    hw = (shape['height'], shape['width'])
    checked = [[rle.as_masks(g) for g in e['rle']['qry_isegmaps']] for e in eps]
    carried = [[polygon.as_polys(g, hw) for g in e['poly']['qry_isegmaps']] for e in eps]

    def blob_bytes(pm):         # the three tables of fgn_poly_masks_u8: 8 ints per mask, part and edge (one edge per vertex)
        return 4 * ops.POLY_REC_INTS * (len(pm) + (len(pm.part_first) - 1) + pm.xy.size // 2)
    uploaded = dict(
        dense=[sum(g.numel() for g in e['dense']['qry_isegmaps']) for e in eps],
        rle=[sum(m.ends.nbytes + 4 * ops.RLE_REC_INTS * len(m) for m in ms) for ms in checked],
        poly=[sum(blob_bytes(pm) for pm in ps) for ps in carried],
        instances=[sum(len(m) for m in ms) for ms in checked],
        runs=[sum(int(m.ends.size) for m in ms) for ms in checked],
        vertices=[sum(int(pm.xy.size // 2) for pm in ps) for ps in carried],
        vertex_bytes_as_float64=[sum(int(pm.xy.nbytes) for pm in ps) for ps in carried],
        host_route_instances=[sum(int(pm.on_host().sum()) for pm in ps) for ps in carried])

    def episode(arm, j):
        e = eps[j % len(eps)][arm]
        dets = model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'],
                                   qry_isegmaps=e['qry_isegmaps'])
        return model.pack_results(dets, 1, img_shape=e['img_shape'], qry_isegmaps=e['qry_isegmaps'])

    arms = ('dense', 'rle', 'poly')
    same = all(episode('dense', j)[0]['qry_isegmaps_rle'] == episode(arm, j)[0]['qry_isegmaps_rle'] and
               np.array_equal(episode('dense', j)[0]['dt_scores'], episode(arm, j)[0]['dt_scores'])
               for j in range(len(eps)) for arm in arms[1:])
    for arm in arms:
        for j in range(args.warmup):
            episode(arm, j)
    torch.cuda.synchronize()

    blocks = {arm: [] for arm in arms}
    for blk in range(args.blocks):
        for arm in arms[blk % 3:] + arms[:blk % 3]:                               # alternate, and rotate who goes first
            times = []
            for j in range(args.episodes):
                t0 = time.perf_counter()
                episode(arm, j)
                times.append((time.perf_counter() - t0) * 1e3)
            blocks[arm].append(statistics.median(times))
    torch.cuda.synchronize()

    g0, m0, p0 = eps[0]['dense']['qry_isegmaps'][0], checked[0][0], carried[0][0]
    device_step_us = dict(
        dense_upload=round(device_us(lambda: g0.to(dev, non_blocking=True)), 2),
        rle_decode_masks=round(device_us(lambda: ops.rle_decode_masks(m0, device=dev)), 2),
        poly_masks=round(device_us(lambda: ops.poly_masks(p0, device=dev)), 2),
        note=f'{len(p0)} masks of {p0.shape[1]}x{p0.shape[2]}, {int(m0.ends.size)} runs, {int(p0.xy.size // 2)} vertices: '
             f'the pinned dense copy against the upload of the runs plus the decode launch against the upload of the '
             f'records plus the two polygon launches (host-side edge records included); mean of 20 back-to-back calls '
             f'between two events.  The kernels\' own durations come from the --kernels-only run under a kernel trace')
    host_ms = dict(as_polys=round(clock_ms(lambda: polygon.as_polys(eps[0]['poly']['qry_isegmaps'][0], hw)), 4),
                   as_masks=round(clock_ms(lambda: rle.as_masks(eps[0]['rle']['qry_isegmaps'][0])), 4),
                   polygon_dense_on_host=round(clock_ms(lambda: p0.dense(), reps=3), 4),
                   note='one core, the masks of one image: checking the polygons / parsing the strings (inside their '
                        'arm\'s episode time) beside the host rasterisation the dense arm\'s loader would do (outside '
                        'its episode time)')

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                    spread_ms=round(max(v) - min(v), 4))
    res = dict(tool='poly_masks_ab', workload=args.workload, device=torch.cuda.get_device_name(0),
               image_hw=[shape['height'], shape['width']], blocks_per_arm=args.blocks, episodes_per_block=args.episodes,
               warmup_per_arm=args.warmup, episodes_in_flight=1, hip_graph=True, transfer_mode=3, pinned_inputs=True,
               arms_agree=bool(same), graphs=len(model._graphs), dense_arm=arm_stats(blocks['dense']),
               rle_arm=arm_stats(blocks['rle']), poly_arm=arm_stats(blocks['poly']),
               uploaded_mask_bytes_per_episode=uploaded, device_step_us=device_step_us, host_ms=host_ms)
    res['poly_minus_dense_median_ms'] = round(res['poly_arm']['median_ms'] - res['dense_arm']['median_ms'], 4)
    res['poly_minus_rle_median_ms'] = round(res['poly_arm']['median_ms'] - res['rle_arm']['median_ms'], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
