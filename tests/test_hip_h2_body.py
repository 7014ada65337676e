"""The K-tile body of conv_pw_h2_kernel (csrc/conv_pw_h2.h): the issue cursor that walks the K-tiles of an
output tile and crosses into the next one, and the split issued among the MFMAs.  A workgroup must walk MORE THAN ONE
output tile for the cursor to cross a tile boundary, so the GEMM and dual shapes have a few tiles more than the persistent
grid holds workgroups (768 / 512 / 256 for the 64-row / 128-row / two-K-group tiles), a ragged last tile and few K-tiles
(two: a tile boundary at every second K-tile; odd counts); every instance the launcher uses, with and without the
implicit-GEMM loader, the second operand and the grouped form.  (Of the six implicit-GEMM cases only stride 1 on the 64-row
tile has more tiles than workgroups: the others check the tap cursor inside one output tile per workgroup.)  Every case against the fp64 product within 2e-6 of its range - the bound of
tests/test_hip_conv.py::test_h2_gemm_is_as_close_to_fp64_as_the_f32_mfma_kernel - and run twice: identical bytes."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H2_BOUND = 2e-6       # of the fp64 range (tests/test_hip_conv.py::test_h2_*)
_cache = {}


def _operands(rows, K, N):
    """Post-ReLU activations x random weights with columns of different magnitude, a shift and a residual, and the fp64
    product (torch, float64) - once per shape, shared by the cases of the shape and never written."""
    key = (rows, K, N)
    if key not in _cache:
        from fgn_amd import ops
        g = torch.Generator().manual_seed(rows + 7 * K + N)
        x = torch.randn(rows, K, generator=g).relu_().cuda()
        w = torch.randn(N, K, generator=g) / K ** 0.5
        w[1::3] *= 40.0
        w = w.cuda()
        _cache[key] = dict(x=x, w=w, shift=torch.randn(N, generator=g).cuda(), res=(torch.randn(rows, N, generator=g) * 3.0).cuda(),
                           img=ops.pack_h2(w), prod=x.double() @ w.double().T)
    return _cache[key]


def _check(tag, run, ref):
    """``run()`` -> output (rows x N) twice: identical bytes, and within the bound of ``ref`` (fp64)."""
    a = run()
    b = run()
    assert torch.equal(a, b), f'{tag}: two runs differ'
    rng = ref.abs().max().item()
    err = (a.double() - ref).abs().max().item()
    print(f'{tag}: max error {err / rng:.2e} of the range')
    assert err <= H2_BOUND * rng, (tag, err / rng)


def _gemm(o, rows, N, bm, full=False):
    from fgn_amd import ops
    kw = dict(shift=o['shift'], residual=o['res'], relu=True) if full else {}

    def run():
        out = torch.full((rows + 64, N), -7.0, device='cuda')
        ops.gemm_h2(o['x'], o['img'], N, bm=bm, out=out[:rows], **kw)
        assert (out[rows:] == -7.0).all()              # the ragged last tile stops at M
        return out[:rows]
    ref = torch.relu(o['prod'] + o['shift'].double() + o['res'].double()) if full else o['prod']
    return run, ref


# tile code, rows, N, K, epilogue: tiles over workgroups in the comment
_GEMM_CASES = [
    (64, 6203, 1024, 64, False),        # 97 x 8 = 776 tiles on 768 workgroups, two K-tiles
    (64, 6203, 1024, 96, False),        # three
    (64, 6203, 1024, 160, False),       # five
    (64, 6203, 132, 96, False),         # the column guard (132 of 256 columns)
    (64, 6203, 1024, 96, True),         # shift + residual + ReLU
    (128, 8317, 1024, 64, False),       # 65 x 8 = 520 tiles on 512 workgroups
    (128, 8317, 1024, 160, False),
    (264, 98425, 64, 64, False),        # 128 rows x 64 columns: 769 tiles on 768 workgroups
    (1064, 2111, 1024, 128, False),     # two K-groups: 33 x 8 = 264 tiles on 256 workgroups, two K-steps
    (1064, 2111, 1024, 320, False),     # five K-steps
]


@pytest.mark.parametrize('bm,rows,N,K,full', _GEMM_CASES)
def test_workgroups_that_walk_more_than_one_output_tile(bm, rows, N, K, full):
    o = _operands(rows, K, N)
    run, ref = _gemm(o, rows, N, bm, full)
    _check(f'bm {bm} {rows}x{K}->{N}{" epilogue" if full else ""}', run, ref)


@pytest.mark.parametrize('bm', [64, 128])
def test_grouped_launch_with_inactive_tiles(bm):
    """4 groups of 256 rows of which 70 are valid (K = 64, N = 256): the tiles past the valid rows are skipped by the tile
    walk, the valid tile's rows past 70 are fetched as zeros - 3e38 lies there, as in the existing garbage test - and the
    weight offset of a group enters the cursor."""
    from fgn_amd import ops
    groups, grp_rows, valid, K, N = 4, 256, 70, 64, 256
    g = torch.Generator().manual_seed(41)
    x = torch.randn(groups, grp_rows, K, generator=g).relu_().cuda()
    x[:, valid:] = 3e38
    w = (torch.randn(groups, N, K, generator=g) / K ** 0.5).cuda()
    shift = torch.randn(N, generator=g).cuda()
    img = ops.pack_h2(w)
    ref = torch.einsum('grk,gnk->grn', x[:, :valid].double(), w.double()) + shift.double()

    def run():
        out = torch.full((groups, grp_rows, N), float('nan'), device='cuda')
        ops.gemm_h2(x, img, N, shift=shift, groups=groups, grp_valid=valid, bm=bm, out=out)
        assert torch.isnan(out[:, -(-valid // bm) * bm:]).all()          # whole tiles past the valid rows are not written
        return out[:, :valid].contiguous()
    _check(f'grouped bm {bm}', run, ref)


@pytest.mark.parametrize('table', [False, True])
def test_second_operand_switches_inside_the_k_loop(table):
    """``ops.conv1x1_dual`` with Cin1 = Cin2 = 64 -> 1024 channels on 6203 rows (776 tiles of 64 rows): the operand
    switches at K-tile 2 of 4; once with the second operand's rows taken through ``x2_rows`` (every other row of a
    buffer twice as long).  Reference: fp64 over the layer's own folded f32 weights."""
    from fgn_amd import lib, ops
    rows, cin, cout = 6203, 64, 1024
    assert lib.load().fgn_h2_row_tile(rows, cout, 2 * cin, 0, 0) == 64
    g = torch.Generator().manual_seed(43)
    y = torch.randn(rows, cin, generator=g).relu_().cuda()
    x = torch.randn(2 * rows if table else rows, cin, generator=g).relu_().cuda()
    w3, wd = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5, torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    mk = lambda: dict(weight=torch.rand(cout, generator=g) + 0.5, bias=torch.randn(cout, generator=g) * 0.1,
                      running_mean=torch.randn(cout, generator=g) * 0.1, running_var=torch.rand(cout, generator=g) + 0.5)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv_dual(w3, mk(), wd, mk(), relu=True).to('cuda')
    assert layer.wh is not None
    tab = (torch.arange(rows, dtype=torch.int32) * 2).cuda() if table else None
    x_used = x[tab.long()] if table else x
    ref = torch.relu(torch.cat((y, x_used), 1).double() @ layer.w[:cout].double().T + layer.shift.double())
    run = lambda: ops.conv1x1_dual(y.view(1, rows, 1, cin), x.view(1, -1, 1, cin), layer, x2_rows=tab).view(rows, cout)
    with ops.gemm_math('h2'):
        _check(f'dual{" x2_rows" if table else ""}', run, ref)


def _conv_case(stride):
    """3x3 / pad 1 / stride ``stride``, 64 -> 1024 channels with bias and ReLU on a 1 x 80 x 80 and a 2 x 5 x 7 tensor that lie
    in one buffer; the fp64 convolution of both once per stride."""
    key = ('conv', stride)
    if key not in _cache:
        g = torch.Generator().manual_seed(47 + stride)
        cin, cout = 64, 1024
        wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        bias = torch.randn(cout, generator=g)
        xq = torch.randn(1, 80, 80, cin, generator=g).relu_()
        xs = torch.randn(2, 5, 7, cin, generator=g).relu_()
        buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).cuda()
        refs = [torch.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), bias.double(), stride=stride,
                                    padding=1)).permute(0, 2, 3, 1).contiguous().cuda() for x in (xq, xs)]
        _cache[key] = dict(wt=wt, bias=bias, q=buf[:xq.numel()].view(xq.shape), s=buf[xq.numel():].view(xs.shape), refs=refs)
    return _cache[key]


@pytest.mark.parametrize('bm,cout', [(64, 1024), (1064, 1024), (264, 64)])
@pytest.mark.parametrize('stride', [1, 2])
def test_implicit_gemm_on_two_tensors(stride, bm, cout):
    """``ops.conv2d_pair`` with the tile code forced: 18 K-tiles over nine filter taps, the tap offsets advanced per K-tile
    (stride 1: 6470 rows = 816 tiles of 64 x 128 on 768 workgroups); the rows of the small tensor have taps outside the
    image; 264: the first 64 output channels on the 128 x 64 tile."""
    from fgn_amd import ops
    c = _conv_case(stride)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(c['wt'][:cout], bias=c['bias'][:cout], stride=stride, pad=1, relu=True).to('cuda')
    assert layer.wh is not None
    ref = torch.cat([r[..., :cout].reshape(-1, cout) for r in c['refs']])

    def run():
        yq, ys = ops.conv2d_pair(c['q'], c['s'], layer, bm=bm)
        return torch.cat((yq.reshape(-1, cout), ys.reshape(-1, cout)))
    _check(f'conv2d_pair 3x3/{stride} bm {bm} ->{cout}', run, ref)


def test_device_image_count_cuts_m_inside_a_tile():
    """A 1x1 convolution of up to 100 images of 7 x 7 (64 -> 1024 channels: the 64-row tile) with a device count of 37:
    M = 1813 rows ends inside a tile; the rows of the images past the count keep their bytes."""
    from fgn_amd import lib, ops
    n_img, cnt, cin, cout = 100, 37, 64, 1024
    assert lib.load().fgn_h2_row_tile(n_img * 49, cout, cin, 0, 0) == 64
    g = torch.Generator().manual_seed(53)
    x = torch.randn(n_img, 7, 7, cin, generator=g).relu_().cuda()
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bias = torch.randn(cout, generator=g)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(w, bias=bias).to('cuda')
    assert layer.wh is not None
    count = torch.tensor([cnt], dtype=torch.int32, device='cuda')
    ref = x[:cnt].reshape(-1, cin).double() @ w.reshape(cout, cin).double().cuda().T + bias.double().cuda()

    def run():
        out = torch.full((n_img, 7, 7, cout), -7.0, device='cuda')
        ops.conv2d(x, layer, n_img_dev=count, out=out)
        assert (out[cnt:] == -7.0).all()
        return out[:cnt].reshape(-1, cout)
    _check('device count', run, ref)
