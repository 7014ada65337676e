#!/usr/bin/env python3
"""A/B of the two ways a chain of two photometric operators (COCO's ``augs_seq``: an HSV operator, then a blur) is
applied to a source-size image on one GPU, one process.

Arm A ('chain'): one launch of ``photometric_chain_u8hwc3_kernel`` (``ops.photometric_chain_u8``) - the point operator
runs on every pixel while the blur stages its tile, the image is read once and written once.  Arm B ('two_pass'): two
launches of ``photometric_u8hwc3_kernel`` (``ops.photometric_u8`` twice) through an intermediate buffer - what the code
could do before the chain kernel existed; it allocates one more buffer and reads and writes every byte once more.  Both
arms compute the same bytes (tests/test_hip_photo_chain.py pins the chain kernel to the fold bit for bit; the tool asserts
the equality once per case).

A 600x1000 source under the cfg3 network size (800x1333), the cases "hue 10 then blur 1.5" and "brightness 30 then blur
1.5" - the far ends of ``fewshot_ds.draw_coco_augment``.  Arms alternate in blocks; a block is SAMPLES samples, each the
mean of REPS back-to-back calls between two events (wrapper, allocation and launch gaps included); per arm the block
medians, their median and spread (max - min).  ``--kernels-only`` runs just the launches, case by case and arm by arm,
for a kernel trace; ``--trace-csv`` reads that trace back and gives the kernels' own durations.

    python tools/photo_chain_ab.py --out profiles/photo_chain_ab.json
    rocprofv3 --kernel-trace --stats -- python tools/photo_chain_ab.py --kernels-only
    python tools/photo_chain_ab.py --trace-csv <..._kernel_trace.csv>
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgn_amd import fewshot_ds as fd, ops                                       # noqa: E402
from fgn_amd.episodes import CONFIGS                                            # noqa: E402
from qry_augment_ab import pixels                                               # noqa: E402

CASES = {'hue10_blur1.5': [(4, 10, 0), (3, 1.5, 0)], 'brightness30_blur1.5': [(6, 30, 0), (3, 1.5, 0)]}
WARM, REPS, SAMPLES = 3, 20, 7


def device_us(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def arms(src, chain, hw, net_hw, dev) -> dict:
    """The two arms of one case as callables on the uploaded slot ``src`` [1, 3 h w]."""
    recs = fd.photometric_chain_records(chain, hw, net_hw)
    assert recs[:, 2].tolist() == [int(chain[0][0]), 3, 0]
    both = torch.from_numpy(np.ascontiguousarray(recs[None, :2])).to(dev)
    first, second = (torch.from_numpy(np.ascontiguousarray(recs[None, i])).to(dev) for i in range(2))
    return dict(chain=lambda: ops.photometric_chain_u8(src, both),
                two_pass=lambda: ops.photometric_u8(ops.photometric_u8(src, first), second))


def trace_summary(path: str) -> dict:
    """The kernels' own durations from the kernel trace of a ``--kernels-only`` run: per case WARM + REPS launches of the
    chain kernel, then WARM + REPS pairs (point operator, blur) of the single-operator kernel; the first WARM dropped."""
    with open(path, newline='') as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r['Start_Timestamp']))
    dur = lambda name: [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows
                        if r['Kernel_Name'].startswith(name)]
    ch, one = dur('photometric_chain_u8hwc3_kernel'), dur('photometric_u8hwc3_kernel')
    n = WARM + REPS
    if len(ch) != len(CASES) * n or len(one) != 2 * len(CASES) * n:
        raise SystemExit(f'{path}: {len(ch)} + {len(one)} launches, expected those of one --kernels-only run')
    stat = lambda v: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    out = {}
    for i, name in enumerate(CASES):
        pairs = one[2 * i * n + 2 * WARM:2 * (i + 1) * n]
        out[name] = dict(chain_kernel=stat(ch[i * n + WARM:(i + 1) * n]), two_pass_point_kernel=stat(pairs[0::2]),
                         two_pass_blur_kernel=stat(pairs[1::2]))
        out[name]['two_pass_sum_of_medians_us'] = round(out[name]['two_pass_point_kernel']['median_us'] +
                                                        out[name]['two_pass_blur_kernel']['median_us'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='cfg3', choices=sorted(CONFIGS))
    ap.add_argument('--source', type=int, nargs=2, default=(600, 1000), metavar=('h', 'w'))
    ap.add_argument('--blocks', type=int, default=6, help='blocks per arm and case')
    ap.add_argument('--out', default=None, help='write the JSON result here as well')
    ap.add_argument('--kernels-only', action='store_true',
                    help='launch the kernels alone, case by case and arm by arm: the run to put under `rocprofv3 '
                         '--kernel-trace --stats`, whose durations exclude the wrappers and launch gaps')
    ap.add_argument('--trace-csv', default=None, help='the kernel trace of a --kernels-only run: durations per kernel')
    args = ap.parse_args()
    if args.trace_csv:
        print(json.dumps(dict(tool='photo_chain_ab', kernel_trace_us=trace_summary(args.trace_csv))), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit('photo_chain_ab needs a GPU: a CPU run measures nothing')
    shape = CONFIGS[args.workload]
    net_hw, hw = (shape['height'], shape['width']), tuple(args.source)
    dev = torch.device('cuda', torch.cuda.current_device())
    img = pixels(np.random.RandomState(0), *hw)
    src = torch.from_numpy(np.ascontiguousarray(img)).reshape(1, -1).to(dev)
    res = dict(tool='photo_chain_ab', device=torch.cuda.get_device_name(0), source_hw=list(hw), network_hw=list(net_hw),
               cases={k: [list(r) for r in v] for k, v in CASES.items()})
    if args.kernels_only:
        res.update(kernels_only=True, event_means_us={})
        for name, chain in CASES.items():
            for arm, fn in arms(src, chain, hw, net_hw, dev).items():       # WARM + REPS calls per arm, in this order
                device_us(fn, WARM)
                res['event_means_us'][f'{name}/{arm}'] = round(device_us(fn), 2)
        print(json.dumps(res), flush=True)
        return
    res.update(blocks_per_arm=args.blocks, samples_per_block=SAMPLES, calls_per_sample=REPS, results={})
    for name, chain in CASES.items():
        fns = arms(src, chain, hw, net_hw, dev)
        a, b = fns['chain'](), fns['two_pass']()
        torch.cuda.synchronize()
        if not torch.equal(a, b):
            raise SystemExit(f'{name}: the chain kernel and the two passes disagree')
        for fn in fns.values():
            device_us(fn, WARM)
        blocks = {arm: [] for arm in fns}
        for blk in range(args.blocks):
            for arm in (('chain', 'two_pass') if blk % 2 == 0 else ('two_pass', 'chain')):    # alternate who goes first
                blocks[arm].append(statistics.median(device_us(fns[arm]) for _ in range(SAMPLES)))
        stat = lambda v: dict(block_medians_us=[round(x, 2) for x in v], median_us=round(statistics.median(v), 2),
                              spread_us=round(max(v) - min(v), 2))
        res['results'][name] = {arm: stat(v) for arm, v in blocks.items()}
        res['results'][name]['chain_over_two_pass'] = round(res['results'][name]['chain']['median_us'] /
                                                            res['results'][name]['two_pass']['median_us'], 3)
    res['note'] = ('event means per call: the Python wrapper, the output allocation (two for two_pass) and the launch gaps '
                   'are inside both arms; the kernels\' own durations come from a kernel trace of --kernels-only')
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
