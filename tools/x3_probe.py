#!/usr/bin/env python3
"""conv_pw_h2_kernel (two-f16-plane products) and conv_pw_x3_kernel (three-bf16-plane products) against the f32-MFMA kernels: error against fp64 and time per launch on
the GEMM shapes of a cfg3 episode, the variants taking turns.  python tools/x3_probe.py [--reps 10]
h2_bm64_kg2 = the 64-row tile on two K-groups (tile code 1064; skipped where K / 32 is odd or below 4); --im2col adds
layer3.0's 3x3 / stride 2 convolution of the query map and the support maps as one implicit GEMM (6504 x 2304 -> 256).
FGN_HIP_LIB=tools/micro/libfgn_hip_exp.so adds the instances that were measured and not chosen (128-row tiles, 16x16x32
MFMA); FGN_HIP_LIB=tools/micro/libfgn_hip_x3ph.so --phases the phase clocks of one wave."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgn_amd import ops  # noqa: E402

SHAPES = [   # name, groups, rows per group (allocated), valid rows, K, N
    ('relq 14700x1024>1024', 1, 14700, 14700, 1024, 1024),
    ('sh conv3 15141x512>1024', 1, 15141, 15141, 512, 1024),
    ('sh conv1 15141x1024>512', 1, 15141, 15141, 1024, 512),
    ('wino sh300 36x1236 512>512', 36, 1280, 1236, 512, 512),
    ('wino agrpn 36x819 1024>1024', 36, 896, 819, 1024, 1024),
    ('wino mask 36x400 512>512', 36, 512, 400, 512, 512),
    ('layer1 conv3 103664x64>256', 1, 103664, 103664, 64, 256),
    ('layer2 conv3 25916x128>512', 1, 25916, 25916, 128, 512),
    ('layer2 conv1 25916x512>128', 1, 25916, 25916, 512, 128),
    ('layer3 conv1 6504x1024>256', 1, 6504, 6504, 1024, 256),
    ('layer3 conv3 6504x256>1024', 1, 6504, 6504, 256, 1024),
    # the 204-tile grid of layer3's conv1 at shallower K loops (--only kgsweep): where two K-groups start to pay
    ('kgsweep 6504x512>256', 1, 6504, 6504, 512, 256),
    ('kgsweep 6504x256>256', 1, 6504, 6504, 256, 256),
]


def probe_im2col(dev, reps):
    """layer3.0 conv2 (3x3 / stride 2, 256 -> 256) on the 1 x 100 x 167 query map and nine 32 x 32 support maps in one
    launch: 4200 + 2304 = 6504 rows, 72 K-tiles, 204 tiles - one K-group against two."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(2)
    c = 256
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(wt, stride=2, pad=1, relu=False).to(dev)
    xq, xs = torch.randn(1, 100, 167, c, generator=g).relu_(), torch.randn(9, 32, 32, c, generator=g).relu_()
    buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).to(dev)
    q_d, s_d = buf[:xq.numel()].view(xq.shape), buf[xq.numel():].view(xs.shape)
    refs = [F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), stride=2, padding=1).permute(0, 2, 3, 1) for x in (xq, xs)]
    scale = max(r.abs().max().item() for r in refs)
    rows = sum(r.shape[0] * r.shape[1] * r.shape[2] for r in refs)
    rec = dict(shape='layer3.0 conv2 3x3/2 im2col %dx2304>256' % rows, gflop=2.0 * rows * 9 * c * c / 1e9)
    fns = {}
    for tag, bm in (('h2_bm64', 64), ('h2_bm64_kg2', 1064)):
        o0, o1 = torch.zeros(refs[0].shape, device=dev), torch.zeros(refs[1].shape, device=dev)
        fn = (lambda bm=bm, o0=o0, o1=o1: ops.conv2d_pair(q_d, s_d, layer, out0=o0, out1=o1, bm=bm))
        fn()
        torch.cuda.synchronize()
        rec[tag] = dict(max_err=max((o.cpu().double() - r).abs().max().item() for o, r in ((o0, refs[0]), (o1, refs[1]))) / scale)
        fns[tag] = fn
    for k, us in timed_round_robin(fns, reps).items():
        rec[k]['us'] = us
        rec[k]['tflops_f32_equiv'] = round(rec['gflop'] / us * 1e-3, 1)
    print(json.dumps(rec), flush=True)


# --epilogue: the shapes whose time outside the K-tiles profiles/h2_epilogue_phases.jsonl splits, on the instance the
# launcher picks (tile code 0) unless one is named: name, groups, rows per group, valid rows, K, N, residual, tile code
EPILOGUE_SHAPES = [
    ('relq 14700x1024>1024', 1, 14700, 14700, 1024, 1024, False, 64),
    ('relq 14700x1024>1024', 1, 14700, 14700, 1024, 1024, False, 128),
    ('wino agrpn 36x819 1024>1024', 36, 896, 819, 1024, 1024, False, 0),
    ('layer3 conv1 6504x1024>256', 1, 6504, 6504, 1024, 256, False, 0),
    ('layer3 conv3 6504x256>1024 +residual', 1, 6504, 6504, 256, 1024, True, 0),
    ('layer1 conv1 103664x256>64', 1, 103664, 103664, 256, 64, False, 0),
]


def probe_epilogue(dev, reps, build):
    """One record per shape of EPILOGUE_SHAPES: the phase clocks with the epilogue's split (a library built with
    -DH2_PHASES) and the time per launch, shift + ReLU (+ residual) in the epilogue."""
    L = ops._lib.load()
    g = torch.Generator().manual_seed(3)
    for name, G, gr, valid, K, N, with_res, bm in EPILOGUE_SHAPES:
        x = torch.randn(G, gr, K, generator=g).relu_().to(dev)
        w = (torch.randn(G, N, K, generator=g) * (1.0 / K ** 0.5)).to(dev)
        shift = torch.randn(N, generator=g).to(dev)
        res = torch.randn(G, gr, N, generator=g).to(dev) if with_res else None
        img = ops.pack_h2(w)
        out = torch.zeros(G, gr, N, device=dev)
        fn = (lambda: ops.gemm_h2(x, img, N, shift=shift, residual=res, relu=True, groups=G, grp_valid=valid, bm=bm, out=out))
        fn()
        torch.cuda.synchronize()
        tile = bm or L.fgn_h2_row_tile(G * gr, N, K, gr if G > 1 else 0, valid if G > 1 else 0)
        kg = L.fgn_h2_k_groups(G * gr, N, K, gr if G > 1 else 0, valid if G > 1 else 0) if bm == 0 else 1
        rec = dict(build=build, shape=name, tile=tile, k_groups=kg, wg0_cycles_per_ktile=h2_phases(fn))
        rec['us'] = timed_round_robin({'h2': fn}, reps)['h2']
        print(json.dumps(rec), flush=True)
        del x, w, res, out, img


def timed_round_robin(fns: dict, reps: int, rounds: int = 5) -> dict:
    """Median over `rounds` of the time per launch of every variant, the variants taking turns (the clock the chip holds
    depends on what ran just before: one variant after the other ranks them by their place in the queue)."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1000.0 / reps)
    return {k: round(sorted(v)[len(v) // 2], 1) for k, v in res.items()}


def h2_phases(fn):
    """Phase clocks of wave 0 of workgroup 0 of one conv_pw_h2_kernel launch (a library built with -DH2_PHASES:
    tools/micro/build_x3_phases.sh, FGN_HIP_LIB=tools/micro/libfgn_hip_h2ph.so), cycles per K-tile."""
    import ctypes
    raw = ctypes.CDLL(ops._lib.LIB_PATH)
    if not hasattr(raw, 'fgn_x3_phases'):
        return None
    buf = (ctypes.c_ulonglong * 16)()
    ep = (ctypes.c_ulonglong * 16)() if hasattr(raw, 'fgn_h2_epilogue_phases') else None
    raw.fgn_x3_phases(buf)                      # clear
    if ep is not None:
        raw.fgn_h2_epilogue_phases(ep)
    fn()
    if ep is not None and raw.fgn_h2_epilogue_phases(ep) != 0:
        return None
    if raw.fgn_x3_phases(buf) != 0:
        return None
    v = list(buf[0:8])
    steps = max(v[6], 1)
    rec = dict(wait_barrier=round(v[0] / steps), issue=round(v[1] / steps), lds_landed=round(v[2] / steps),
               watch_split0=round(v[3] / steps), mfma=round(v[4] / steps), outside_per_ktile=round(v[5] / steps),
               ktiles=v[6], kernel_cycles=v[7])
    if ep is not None:
        # the time outside the K-tiles by its parts (conv_pw_h2.h, ph_[7 .. 13]), cycles per OUTPUT TILE of the wave: what
        # the kernel books under "outside" and under "wait + barrier" is put back so that both keep their meaning
        e = list(ep[0:8])
        tiles = max(e[6], 1)
        rec['wait_barrier'] = round((v[0] + e[0]) / steps)
        rec['outside_per_ktile'] = round((v[5] + e[1] + e[2] + e[3] + e[4] + e[5]) / steps)
        rec['outside_per_tile'] = dict(a_skew_to_first_barrier=round(e[1] / tiles), b_lds_writes_and_barriers=round(e[2] / tiles),
                                       c_wait_in_flight_residual=round(e[3] / tiles), d_lds_reads_math_stores=round(e[4] / tiles),
                                       e_tile_walk=round(e[5] / tiles), between_ktiles_per_ktile=round(v[5] / steps), f_vmcnt_first_ktile_of_later_tiles=round(e[0] / max(tiles - 1, 1)),
                                       tiles=e[6])
    return rec


# default instances (16x16x32 MFMA): 64 / 128 rows, nine terms; + 2000: the 32x32x16 form (experiments build)
VARIANTS = (('x6_bm64', 64, 6), ('x6_bm128', 128, 6), ('x9_bm64', 64, 9), ('x6_bm64_mfma32', 2064, 6), ('x6_bm128_mfma32', 2128, 6),
            ('x6_bm129_mfma32', 2129, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only', default='')
    ap.add_argument('--im2col', action='store_true', help="layer3.0's 3x3 / stride 2 implicit GEMM, one K-group against two")
    ap.add_argument('--epilogue', default='', metavar='BUILD',
                    help="the epilogue's phase split on EPILOGUE_SHAPES, the records labelled BUILD (FGN_HIP_LIB=tools/micro/"
                         'libfgn_hip_h2ph.so, or libfgn_hip_h2ph_passes.so for the pass-per-wave-row form)')
    ap.add_argument('--phases', action='store_true', help='phase clocks (FGN_HIP_LIB=tools/micro/libfgn_hip_x3ph.so for conv_pw_x3_kernel, libfgn_hip_h2ph.so for conv_pw_h2_kernel)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    if args.im2col:
        probe_im2col(dev, args.reps)
    if args.epilogue:
        probe_epilogue(dev, args.reps, args.epilogue)
        return
    for name, G, gr, valid, K, N in SHAPES:
        if args.only and args.only not in name:
            continue
        x = torch.randn(G, gr, K, generator=g).relu_().to(dev)          # post-ReLU activations
        w = (torch.randn(G, N, K, generator=g) * (1.0 / K ** 0.5)).to(dev)
        shift = torch.randn(N, generator=g).to(dev)
        ref = torch.einsum('grk,gnk->grn', x[:, :valid].double(), w.double()) + shift.double()
        scale = ref.abs().max().item()
        img = ops.pack_x3(w)
        img32 = ops.pack_x3(w, mfma32=True)
        rec = dict(shape=name, gflop=2.0 * G * valid * K * N / 1e9)
        fns, outs = {}, {}
        # conv_pw_h2_kernel (three f16 products of scaled two-way splits): 64 / 128 rows
        imgh = ops.pack_h2(w)
        for tag, bm in (('h2_bm64', 64), ('h2_bm64_kg2', 1064), ('h2_bm128', 128)):
            if G > 1 and gr % (128 if bm == 128 else 64):
                continue
            if bm == 1064 and ((K // 32) % 2 or K // 32 < 4):
                continue
            out = torch.zeros(G, gr, N, device=dev)
            fn = (lambda bm=bm, out=out: ops.gemm_h2(x, imgh, N, shift=shift, groups=G, grp_valid=valid, bm=bm, out=out))
            fn()
            torch.cuda.synchronize()
            d = (out[:, :valid].double() - ref).abs()
            outs[tag], fns[tag] = out, fn
            rec[tag] = dict(max_err=d.max().item() / scale, mean_err=d.mean().item() / scale)
            if args.phases:
                ph = h2_phases(fn)
                if ph:
                    rec[tag]['wg0_cycles_per_ktile'] = ph
        for tag, bm, nt in VARIANTS:
            if G > 1 and gr % (128 if bm % 1000 >= 128 else 64):
                continue
            out = torch.zeros(G, gr, N, device=dev)
            fn = (lambda bm=bm, nt=nt, out=out: ops.gemm_x3(x, img32 if bm >= 2000 else img, N, shift=shift, groups=G, grp_valid=valid,
                                                            bm=bm, nterms=nt, out=out))
            try:
                fn()
            except ops._lib.FgnHipError:        # an instance of the experiments build (FGN_HIP_LIB=tools/micro/libfgn_hip_exp.so)
                continue
            torch.cuda.synchronize()
            d = (out[:, :valid].double() - ref).abs()
            outs[tag], fns[tag] = out, fn
            rec[tag] = dict(max_err=d.max().item() / scale, mean_err=d.mean().item() / scale)
            if args.phases:
                import ctypes
                raw = ctypes.CDLL(ops._lib.LIB_PATH)
                buf = (ctypes.c_ulonglong * 16)()
                raw.fgn_x3_phases(buf)                      # clear
                fn()
                if raw.fgn_x3_phases(buf) == 0:
                    v = list(buf[0:7])
                    steps = max(v[5], 1)
                    rec[tag]['wg0_cycles_per_ktile'] = dict(
                        wait_barrier=round(v[0] / steps), issue=round(v[1] / steps), lds_landed=round(v[2] / steps),
                        split_mfma=round(v[3] / steps), epilogue_per_ktile=round(v[4] / steps), ktiles=v[5], kernel_cycles=v[6])
        # the f32 MFMA path: a 1x1 convolution packed for it (or the Winograd grouped GEMM entry) on the same operands
        if G == 1:
            with ops.gemm_math('f32'):
                layer = ops.pack_conv(w[0].reshape(N, K, 1, 1), bias=shift).to(dev)
            xin = x[0].reshape(1, gr, 1, K)
            out = torch.zeros(1, gr, 1, N, device=dev)
            fn = lambda: ops.conv2d(xin, layer, out=out)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            d = (out.reshape(gr, N)[:valid].double() - ref[0]).abs()
        else:
            L = ops._lib.load()
            cout_pad = (N + 127) // 128 * 128
            u = torch.zeros(G, cout_pad, K, device=dev)
            u[:, :N] = w
            out = torch.zeros(G, gr, N, device=dev)
            fn = lambda: ops._lib.check(L.fgn_winograd_gemm_f32(x.data_ptr(), u.data_ptr(), out.data_ptr(), None, 1, valid, gr, K, N,  # noqa: E731
                                                                cout_pad, G, torch.cuda.current_stream().cuda_stream), 'wg')
            fn()
            torch.cuda.synchronize()
            d = (out[:, :valid].double() - (ref - shift.double())).abs()
        rec['f32_mfma'] = dict(max_err=d.max().item() / scale, mean_err=d.mean().item() / scale)
        fns['f32_mfma'] = fn
        for k, us in timed_round_robin(fns, args.reps).items():
            rec[k]['us'] = us
            rec[k]['tflops_f32_equiv'] = round(rec['gflop'] / us * 1e-3, 1)
        rec['row_tiles_equal'] = bool('x6_bm128' not in outs or torch.equal(outs['x6_bm64'][:, :valid], outs['x6_bm128'][:, :valid]))
        rec['auto_row_tile'] = ops._lib.load().fgn_x3_row_tile(G * gr, N, K, gr if G > 1 else 0, valid if G > 1 else 0)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
