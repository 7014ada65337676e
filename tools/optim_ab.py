#!/usr/bin/env python3
"""Optimiser recipes of ``Trainer`` against each other on cfg3 training steps (batch 1, eager, the model and inputs of
tools/train_bench.py), and the optimiser launches alone against the bytes they must move.

Arms, alternating in one process (six blocks per arm, who goes first rotates; the figure of an arm is the median of its
block medians, the spread is max - min of them):
  adagrad        Trainer(model): the default path (``ops.adagrad_multi``), what every earlier version launched
  adam           optimizer='Adam'
  sgd_nesterov   optimizer='SGD' (momentum 0.9, Nesterov)
  adam_clip      optimizer='Adam', grad_clip=dict(max_norm=35, norm_type=2)
  accum4         cumulative_iters=4 on the default optimizer: micro-steps and boundary steps timed apart
Each arm has its own model (a Trainer owns its model's packed head layers).

Launches alone: every rule of ``ops.optim_multi``, ``ops.grad_norm_multi`` and ``ops.grad_accumulate_multi`` over the
trainer's real tensor list, 20 back-to-back calls between two events (launch gaps and the Python wrapper included),
beside ``floor_us`` = the bytes the call must move / 6.3 TB/s (the achievable HBM rate; the floor is derived, and
back-to-back calls over ~105 MB tensors may find part of them in the 256 MB Infinity Cache).

usage (GPU box): python tools/optim_ab.py [--blocks 6] [--steps 8] [--out profiles/optim_ab.json]"""
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
ARMS = {'adagrad': {}, 'adam': dict(optimizer='Adam'), 'sgd_nesterov': dict(optimizer='SGD'),
        'adam_clip': dict(optimizer='Adam', grad_clip=dict(max_norm=35.0, norm_type=2)),
        'accum4': dict(cumulative_iters=4)}


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


def launches_alone(tr):
    """Clones of the trainer's tensors (the timed calls change them), its real sizes and learning rates."""
    keys = list(tr.W)
    P = [tr.W[k].clone() for k in keys]
    G = [torch.randn_like(p) * 1e-3 for p in P]
    S1, S2, A = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P], [torch.empty_like(p) for p in P]
    lrs = [tr.lr * (tr.mult if k.startswith('roi_head') else 1.0) for k in keys]
    nbytes = 4 * sum(p.numel() for p in P)
    rec = ops.grad_norm_multi(G, 35.0)
    tabs = [{} for _ in range(6)]
    step = [0]

    def adam(coef=None, tab=tabs[2]):
        step[0] += 1
        ops.optim_multi('Adam', P, G, list(zip(S1, S2)), lrs, 1e-5, step=step[0], coef=coef, table=tab)
    calls = {
        'adagrad_multi (train_bwd.hip, the default path)': (5, lambda: ops.adagrad_multi(P, G, S1, lrs, 1e-5, table=tabs[0])),
        'optim_multi Adagrad': (5, lambda: ops.optim_multi('Adagrad', P, G, S1, lrs, 1e-5, table=tabs[1])),
        'optim_multi Adam': (7, adam),
        'optim_multi Adam with clip coefficient': (7, lambda: adam(rec, tabs[3])),
        'optim_multi SGD momentum 0.9 Nesterov': (5, lambda: ops.optim_multi('SGD', P, G, S1, lrs, 1e-5, momentum=0.9,
                                                                               nesterov=True, table=tabs[4])),
        'optim_multi SGD without momentum': (3, lambda: ops.optim_multi('SGD', P, G, None, lrs, 1e-5, table=tabs[5])),
        'grad_norm_multi (two launches)': (1, lambda: ops.grad_norm_multi(G, 35.0, out=rec)),
        'grad_accumulate_multi first': (2, lambda: ops.grad_accumulate_multi(A, G, 0.25, True)),
        'grad_accumulate_multi': (3, lambda: ops.grad_accumulate_multi(A, G, 0.25, False)),
    }
    out = {}
    for name, (passes, fn) in calls.items():
        us = device_us(fn)
        floor = passes * nbytes / HBM * 1e6
        out[name] = dict(us=round(us, 1), passes=passes, floor_us=round(floor, 1), over_floor=round(us / floor, 2))
    return dict(tensors=len(P), parameters=nbytes // 4, bytes_per_pass=nbytes, calls=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm')
    ap.add_argument('--steps', type=int, default=8, help='steps per block')
    ap.add_argument('--warmup', type=int, default=4, help='steps per arm before the first block')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_ab needs a GPU: a CPU run measures nothing')
    cfg = fgn_r50_c4_config(3, 3)
    sd = init_state_dict(cfg, 0)
    batches = [make_batch(i, 1, **CONFIGS['cfg3']) for i in range(4)]
    batches = [{k: (v.pin_memory() if isinstance(v, torch.Tensor) else
                    [t.pin_memory() if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, (list, tuple)) else v)
                for k, v in b.items()} for b in batches]
    trainers = {name: Trainer(FGN(3, 3, state_dict=sd), **kw) for name, kw in ARMS.items()}

    def step(name, j):
        tr = trainers[name]
        torch.manual_seed(j)
        t0 = time.perf_counter()
        tr.step(batches[j % 4])
        torch.cuda.synchronize()
        boundary = tr.cumulative_iters > 1 and tr._pending == 0
        return (time.perf_counter() - t0) * 1e3, boundary

    for name in ARMS:
        for j in range(args.warmup):
            step(name, j)
    blocks = {name: [] for name in ARMS}
    blocks['accum4 boundary step'] = []
    names = list(ARMS)
    for blk in range(args.blocks):
        for name in names[blk % len(names):] + names[:blk % len(names)]:         # alternate, and rotate who goes first
            times = [step(name, j) for j in range(args.steps)]
            if name == 'accum4':
                blocks['accum4'].append(statistics.median(t for t, b in times if not b))
                blocks['accum4 boundary step'].append(statistics.median(t for t, b in times if b))
            else:
                blocks[name].append(statistics.median(t for t, _ in times))

    def arm_stats(v):
        return dict(block_medians_ms=[round(x, 3) for x in v], median_ms=round(statistics.median(v), 3),
                    spread_ms=round(max(v) - min(v), 3))
    res = dict(tool='optim_ab', workload='cfg3 training step (Trainer.step), batch 1, eager, page-locked inputs',
               device=torch.cuda.get_device_name(0), blocks_per_arm=args.blocks, steps_per_block=args.steps,
               warmup_per_arm=args.warmup, arms={('accum4 micro-step' if k == 'accum4' else k): arm_stats(v)
                                                 for k, v in blocks.items()},
               launches_alone=launches_alone(trainers['adagrad']),
               note='floor_us = passes x bytes_per_pass / 6.3 TB/s, derived; us = mean of 20 back-to-back calls between two '
                    'events, Python wrapper and launch gaps included')
    print(json.dumps(res), flush=True)
    if args.out:
        with open(os.path.join(R, args.out), 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
