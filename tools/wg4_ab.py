"""Time the F(4x4) transform kernels alone at the cfg3 layer shapes (diagnostic): the wide (64-bit index) instance at the
vector width of the library's rule against the narrow (32-bit offset) instance at 4, 8 and 16 bytes per thread, through
the entry points that force both (fgn_winograd4_input_ix_f32 / fgn_winograd4_output_ix_f32).  The variants of a shape
take turns, `rounds` times; the median of the rounds is printed.  usage: wg4_ab.py [rounds]"""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fgn_amd import lib
L = lib.load()
g = torch.Generator().manual_seed(0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
def t(fn, reps=30):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
VARIANTS = (('wide', 64, 0), ('n4', 32, 1), ('n8', 32, 2), ('n16', 32, 4))
print('shape   rule  | input: ' + ' '.join(f'{v[0]:>6s}' for v in VARIANTS) + ' | output: ' + ' '.join(f'{v[0]:>6s}' for v in VARIANTS) + '   (us, back-to-back launches)')
for name, n, H, W, cin, cout, div in (('agrpn', 1, 50, 84, 1024, 1024, 3), ('sh300', 300, 7, 7, 512, 512, 1), ('sh100', 100, 7, 7, 512, 512, 1),
                                      ('mask0', 100, 7, 7, 1024, 256, 1), ('mask1', 100, 7, 7, 256, 256, 1), ('l3', 1, 50, 84, 256, 256, 1),
                                      ('l2', 1, 100, 167, 128, 128, 1), ('l1', 1, 200, 334, 64, 64, 1), ('spp_l3', 9, 16, 16, 256, 256, 1), ('spp_l2', 9, 32, 32, 128, 128, 1)):
    tiles = ((H + 3) // 4) * ((W + 3) // 4)
    t_pad = L.fgn_winograd_t_pad(n * div * tiles)
    x = torch.randn(n, H, W, cin, generator=g).cuda()
    V = torch.empty(36, t_pad, cin, device='cuda')
    Mo = torch.randn(36, t_pad, cout, generator=g).cuda()
    y = torch.empty(n * div, H, W, cout, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ti, to = {v[0]: [] for v in VARIANTS}, {v[0]: [] for v in VARIANTS}
    for _ in range(rounds):
        for vn, bits, vec in VARIANTS:
            ti[vn].append(t(lambda: L.fgn_winograd4_input_ix_f32(x.data_ptr(), None, V.data_ptr(), None, n * div, div, H, W, cin, t_pad,
                                                                 None, 0, 1, 1, bits, vec, st)))
            to[vn].append(t(lambda: L.fgn_winograd4_output_ix_f32(Mo.data_ptr(), y.data_ptr(), None, None, n * div, H, W, cout, t_pad, 1,
                                                                  None, 0, 1, 1, bits, vec, st)))
    rule = L.fgn_winograd4_variant(n * div * tiles, cin, 0) // 10
    print(f'{name:7s} {rule * 4:3d} B | input: ' + ' '.join(f'{statistics.median(ti[v[0]]):6.1f}' for v in VARIANTS) +
          ' | output: ' + ' '.join(f'{statistics.median(to[v[0]]):6.1f}' for v in VARIANTS), flush=True)
