"""conv_pw_h2_kernel on two K-groups (csrc/conv_pw_h2.h, KG = 2): two sets of four waves on one 64-row
output tile, each on every other K-tile with a ring, accumulators and an activation scale of its own, summed in a fixed
order in the epilogue.  Forced through the tile code 1064 of ``ops.gemm_h2`` / ``ops.conv2d_pair`` on shapes a few tiles
large, and once through the routing rule itself (``fgn_h2_k_groups``) on the smallest plain 1x1 launch it picks."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KG2 = 1064            # forced tile code: 64 rows, two K-groups

# rows x K x N: a ragged last tile (200 = 3 x 64 + 8), channels that do not fill the second column tile, 4 / 6 / 8 K-tiles
_SHAPES = [(200, 128, 128), (200, 192, 132), (1000, 256, 260)]
_cache = {}


def _operands(rows, K, N):
    """Post-ReLU activations x random weights with columns of different magnitude, a shift and a residual; the fp64
    products once per shape (shared by the cases of a shape, never written)."""
    key = (rows, K, N)
    if key not in _cache:
        from fgn_amd import ops
        g = torch.Generator().manual_seed(rows + K + N)
        x = torch.randn(rows, K, generator=g).relu_()
        w = torch.randn(N, K, generator=g) / K ** 0.5
        w[1::3] *= 40.0
        shift = torch.randn(N, generator=g)
        res = torch.randn(rows, N, generator=g) * 3.0
        _cache[key] = dict(x=x.cuda(), w=w, shift=shift, res=res, img=ops.pack_h2(w.cuda()), prod=x.double() @ w.double().T)
    return _cache[key]


@pytest.mark.parametrize('epilogue', ['plain', 'shift+residual+relu'])
@pytest.mark.parametrize('rows,K,N', _SHAPES)
def test_two_groups_against_fp64_and_against_one_group(rows, K, N, epilogue):
    """Within 2e-6 of the fp64 range (the bound of test_h2_gemm_is_as_close_to_fp64_as_the_f32_mfma_kernel) and within 1e-6
    of the range of the single-group tile on the same operands (the K order of the additions differs: the bits may);
    two launches give the same bits; the rows past M keep theirs."""
    from fgn_amd import ops
    o = _operands(rows, K, N)
    full = epilogue != 'plain'
    ref = o['prod']
    if full:
        ref = torch.relu(ref + o['shift'].double() + o['res'].double())
    kw = dict(shift=o['shift'].cuda(), residual=o['res'].cuda(), relu=True) if full else {}
    outs = []
    for bm in (KG2, KG2, 64):
        out = torch.full((rows + 64, N), -7.0, device='cuda')
        ops.gemm_h2(o['x'], o['img'], N, bm=bm, out=out[:rows], **kw)
        assert (out[rows:] == -7.0).all(), bm
        outs.append(out[:rows])
    rng = ref.abs().max().item()
    err = (outs[0].cpu().double() - ref).abs().max().item()
    one = (outs[0] - outs[2]).abs().max().item()
    print(f'{rows}x{K}x{N} {epilogue}: |kg2 - fp64| {err / rng:.2e}, |kg2 - bm64| {one / rng:.2e} of the range')
    assert err <= 2e-6 * rng
    assert one <= 1e-6 * rng
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('K', [64, 96])
def test_forced_code_needs_an_even_count_of_at_least_four_k_tiles(K):
    from fgn_amd import lib, ops
    x = torch.ones(128, K, device='cuda')
    img = ops.pack_h2(torch.ones(128, K, device='cuda'))
    with pytest.raises(lib.FgnHipError, match='unsupported shape'):
        ops.gemm_h2(x, img, 128, bm=KG2)
    ops.gemm_h2(x, img, 128, bm=64)                     # (the single-group tile takes the shape)


def _scaled_k_tiles(case):
    """x [1000, 256] (8 K-tiles: group 0 owns the even ones, group 1 the odd ones) for a per-group scale case."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(1000, 256, generator=g)
    kt = torch.arange(256) // 32
    if case in ('even 1e-3, odd 1e3', 'even 1e3, odd 1e-3'):
        small = (kt % 2 == 0) if case.startswith('even 1e-3') else (kt % 2 == 1)
        x[:, small] *= 1e-3
        x[:, ~small] *= 1e3
    elif case in ('group 0 all zero', 'group 1 all zero'):
        x[:, kt % 2 == int(case[6])] = 0.0
    elif case == 'K-tile 5 is 3e4 above':           # group 1's third K-tile: only that group picks a new scale
        x[:, kt == 5] *= 3e4
    else:
        assert case == 'K-tile 4 is 3e4 above'      # group 0's third K-tile
        x[:, kt == 4] *= 3e4
    return x


@pytest.mark.parametrize('case', ['even 1e-3, odd 1e3', 'even 1e3, odd 1e-3', 'group 0 all zero', 'group 1 all zero',
                                  'K-tile 5 is 3e4 above', 'K-tile 4 is 3e4 above'])
def test_each_group_keeps_its_own_activation_scale(case):
    """The groups see K-tiles of different magnitude, so they choose different scales (or one chooses none, or one
    re-scales its accumulators mid-way) and each takes its own out again before the sum: every row within 2e-6 of its own
    sum |a| |b| (as test_h2_gemm_epilogue_and_dynamic_range bounds its cases; the rows here are statistically alike, so a
    wave's shared scale costs a row nothing)."""
    from fgn_amd import ops
    N = 260
    o = _operands(1000, 256, N)
    x = _scaled_k_tiles(case)
    ref = x.double() @ o['w'].double().T
    got = ops.gemm_h2(x.cuda(), o['img'], N, bm=KG2).cpu().double()
    row_scale = (x.double().abs() @ o['w'].double().abs().T).max(1, keepdim=True).values
    worst = ((got - ref).abs() / row_scale).max().item()
    print(f'{case}: worst row error {worst:.2e} of its own sum |a| |b|')
    assert torch.isfinite(got).all()
    assert ((got - ref).abs() <= 2e-6 * row_scale).all()


def test_an_inf_in_a_k_tile_of_the_second_group_stays_in_its_row():
    """One +Inf in row 70, in K-tile 1 (group 1's first): that row comes out non-finite, every other row keeps the bits it
    has with the element replaced by zero and stays within 2e-6 of the fp64 range of its wave's 32 rows (the kernel's
    contract) - the Inf-row test of the single-group kernel (tests/test_hip_launches.py) on the two-group instance.  The
    rows sit at about 1e5 and 1e-4 in blocks of 8, so no wave can keep the scale 1."""
    from fgn_amd import ops
    g = torch.Generator().manual_seed(8)
    rows, K, N = 512, 128, 64
    x = torch.randn(rows, K, generator=g).abs_() + 0.1
    big = (torch.arange(rows) // 8) % 2 == 0
    x[big] *= 1e5
    x[~big] *= 1e-4
    x0 = x.clone()
    x0[70, 40] = 0.0
    x[70, 40] = float('inf')
    w = torch.randn(N, K, generator=g) / K ** 0.5
    shift = torch.randn(N, generator=g)
    img = ops.pack_h2(w.cuda())
    got = ops.gemm_h2(x.cuda(), img, N, shift=shift.cuda(), bm=KG2).cpu()
    zero = ops.gemm_h2(x0.cuda(), img, N, shift=shift.cuda(), bm=KG2).cpu()
    assert not torch.isfinite(got[70]).any()
    others = torch.arange(rows) != 70
    assert torch.isfinite(got[others]).all()
    assert torch.equal(got[others].view(torch.int32), zero[others].view(torch.int32))
    ref = x0.double() @ w.double().T + shift.double()
    err = (got.double() - ref).abs().max(1).values
    err[70] = 0.0
    blk_rng = ref.abs().max(1).values.view(-1, 32).max(1).values.repeat_interleave(32)
    assert (err <= 2e-6 * blk_rng).all(), (err / blk_rng).max().item()


def test_implicit_gemm_on_two_groups_with_the_seam_inside_a_tile():
    """3x3 / stride 2 / pad 1, 64 -> 128 channels (18 K-tiles: nine per group, the filter taps alternating between them) on a
    1 x 9 x 11 and a 2 x 6 x 6 tensor in one launch (30 + 18 output rows: the seam and every border pixel inside one
    64-row tile): each tensor within 2e-6 of its fp64 range."""
    from fgn_amd import ops
    g = torch.Generator().manual_seed(17)
    cin, cout = 64, 128
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bn = dict(weight=torch.rand(cout, generator=g) + 0.5, bias=torch.randn(cout, generator=g) * 0.1,
              running_mean=torch.randn(cout, generator=g) * 0.1, running_var=torch.rand(cout, generator=g) + 0.5)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(wt, bn=bn, stride=2, pad=1, relu=False).to('cuda')
    assert layer.wh is not None
    xq = torch.randn(1, 9, 11, cin, generator=g).relu_()
    xs = torch.randn(2, 6, 6, cin, generator=g).relu_()
    buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).cuda()
    q_d, s_d = buf[:xq.numel()].view(xq.shape), buf[xq.numel():].view(xs.shape)
    yq, ys = ops.conv2d_pair(q_d, s_d, layer, bm=KG2)
    assert tuple(yq.shape) == (1, 5, 6, cout) and tuple(ys.shape) == (2, 3, 3, cout)
    sc = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + 1e-5)
    sh = bn['bias'].double() - bn['running_mean'].double() * sc
    for x, y in ((xq, yq), (xs, ys)):
        r = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), stride=2, padding=1)
        r = (r * sc[None, :, None, None] + sh[None, :, None, None]).permute(0, 2, 3, 1)
        rng = r.abs().max().item()
        err = (y.cpu().double() - r).abs().max().item()
        assert err <= 2e-6 * rng, err / rng


def test_the_routing_rule_picks_two_groups_by_itself():
    """A plain 1x1 convolution of 12300 rows x 1024 -> 128 (193 tiles of 64 x 128: the fewest the GEMM kernels take, at most
    one per CU, 32 K-tiles) with nothing forced: the launch record and ``ops.h2_kernel`` name the two-group instance, and
    the output is within 2e-6 of the fp64 range."""
    from fgn_amd import lib, ops
    rows, K, N = 12300, 1024, 128
    assert lib.load().fgn_h2_k_groups(rows, N, K, 0, 0) == 2
    assert ops.h2_kernel(rows, N, K) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 2>'
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, K, generator=g).relu_()
    w = torch.randn(N, K, generator=g) / K ** 0.5
    shift = torch.randn(N, generator=g)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(w.reshape(N, K, 1, 1), bias=shift).to('cuda')
    prev = ops.PROFILE
    ops.PROFILE = ops.ConvProfile()
    try:
        y = ops.conv2d(x.cuda().view(1, rows, 1, K), layer)
        torch.cuda.synchronize()
        recs = [(r.get('math'), r['kernel']) for r in ops.PROFILE]
    finally:
        ops.PROFILE = prev
    assert recs == [('h2', 'conv_pw_h2_kernel<2, 2, 1, 2, false, 2>')], recs
    ref = x.double() @ w.double().T + shift.double()
    rng = ref.abs().max().item()
    err = (y.view(rows, N).cpu().double() - ref).abs().max().item()
    assert err <= 2e-6 * rng, err / rng
