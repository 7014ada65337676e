#!/usr/bin/env python3
"""``Trainer.forward_backward`` with and without ``feature_grads`` on cfg3 training steps (batch 1, eager, the model and
inputs of tools/optim_ab.py), and the two feature-gradient launches alone against the bytes they must move.

Arms, alternating in one process on ONE trainer (``forward_backward`` changes no weight; six blocks per arm, who goes
first rotates; the figure of an arm is the median of its block medians, the spread is max - min of them):
  off   forward_backward(batch): the step every earlier version made
  on    forward_backward(batch, feature_grads=True): block 0 of the shared head returns its data gradient for both
        batches, the tap product, the host index and ``ops.guidance_backward``, two ``ops.roi_align_backward``

Launches alone: the calls of ``ops.roi_align_backward`` (RoI batch, support batch) and ``ops.guidance_backward`` of one
real step, recorded with their operands and replayed 20 times back to back between two events (launch gaps, the Python
wrapper and - for the guidance - the index upload included), beside ``floor_us`` = (gradient read once + result written
once) / 6.3 TB/s (the achievable HBM rate; the floor is derived).

usage (GPU box): python tools/feature_grads_ab.py [--blocks 6] [--steps 8] [--out profiles/feature_grads_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch                                             # noqa: E402
from fgn_amd import ops                                   # noqa: E402
from fgn_amd.config import fgn_r50_c4_config              # noqa: E402
from fgn_amd.detector import FGN                          # noqa: E402
from fgn_amd.episodes import CONFIGS, make_batch          # noqa: E402
from fgn_amd.train import Trainer                         # noqa: E402
from fgn_amd.weights import init_state_dict               # noqa: E402

HBM = 6.3e12


def device_us(fn, n=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def launches_alone(tr, batch):
    """One real step with the two wrappers recording their operands, then each call replayed alone."""
    calls = []
    real_roi, real_gd = ops.roi_align_backward, ops.guidance_backward

    def rec_roi(dy, rois, shape, scale, sr, aligned, out=None, accumulate=False):
        calls.append(('roi_align_backward', (dy, rois, tuple(shape), scale, sr, aligned)))
        return real_roi(dy, rois, shape, scale, sr, aligned, out=out, accumulate=accumulate)

    def rec_gd(taps, index, qry, vec, out=None, accumulate=False, upload=None):
        calls.append(('guidance_backward', (taps, index, qry, vec)))
        return real_gd(taps, index, qry, vec, out=out, accumulate=accumulate, upload=upload)
    ops.roi_align_backward, ops.guidance_backward = rec_roi, rec_gd
    try:
        torch.manual_seed(0)
        tr.forward_backward(batch, feature_grads=True)
    finally:
        ops.roi_align_backward, ops.guidance_backward = real_roi, real_gd
    out = {}
    for name, a in calls:
        if name == 'roi_align_backward':
            dy, rois, shape, scale, sr, aligned = a
            dx = torch.zeros(shape, device=dy.device)
            us = device_us(lambda: real_roi(dy, rois, shape, scale, sr, aligned, out=dx, accumulate=True))
            nbytes = 4 * (dy.numel() + dx.numel())
            key = f'roi_align_backward R={dy.shape[0]} -> {list(shape)} aligned={int(aligned)} sr={sr}'
        else:
            taps, index, qry, vec = a
            us = device_us(lambda: real_gd(taps, index, qry, vec))
            nbytes = 4 * (taps.numel() + qry.numel())
            key = f'guidance_backward rows={taps.shape[0]} touched={index["pix"].size} -> {list(qry.shape)}'
        floor = nbytes / HBM * 1e6
        out[key] = dict(us=round(us, 1), bytes=nbytes, floor_us=round(floor, 1), over_floor=round(us / floor, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--steps', type=int, default=8, help='steps per block')
    ap.add_argument('--warmup', type=int, default=4, help='steps per arm before the first block')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feature_grads_ab needs a GPU: a CPU run measures nothing')
    cfg = fgn_r50_c4_config(3, 3)
    sd = init_state_dict(cfg, 0)
    batches = [make_batch(i, 1, **CONFIGS['cfg3']) for i in range(4)]
    batches = [{k: (v.pin_memory() if isinstance(v, torch.Tensor) else
                    [t.pin_memory() if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, (list, tuple)) else v)
                for k, v in b.items()} for b in batches]
    tr = Trainer(FGN(3, 3, state_dict=sd))
    arms = {'off': False, 'on': True}

    def step(name, j):
        torch.manual_seed(j)
        t0 = time.perf_counter()
        tr.forward_backward(batches[j % 4], feature_grads=arms[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name in arms:
        for j in range(args.warmup):
            step(name, j)
    blocks = {name: [] for name in arms}
    names = list(arms)
    for blk in range(args.blocks):
        for name in names[blk % 2:] + names[:blk % 2]:                 # alternate, and rotate who goes first
            blocks[name].append(statistics.median(step(name, j) for j in range(args.steps)))

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3),
                    spread_ms=round(max(v) - min(v), 3))
    res = dict(tool='feature_grads_ab',
               workload='cfg3 training step without the update (Trainer.forward_backward), batch 1, eager, page-locked inputs',
               device=torch.cuda.get_device_name(0), blocks_per_arm=args.blocks, steps_per_block=args.steps,
               warmup_per_arm=args.warmup, arms={k: arm_stats(v) for k, v in blocks.items()},
               launches_alone=launches_alone(tr, batches[0]),
               note='floor_us = (gradient read once + result written once) / 6.3 TB/s, derived; us = mean of 20 back-to-back '
                    'calls between two events, Python wrapper, index upload and launch gaps included')
    res['cost_ms'] = round(res['arms']['on']['median_ms'] - res['arms']['off']['median_ms'], 3)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(os.path.join(R, args.out), 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
