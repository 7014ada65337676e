"""The epilogue of conv_pw_h2_kernel (csrc/conv_pw_h2.h; DESIGN 4.1.2, "the epilogue"): on the one-K-group instances every
wave takes its own accumulators through a region of the free LDS stage that only it uses, behind ONE workgroup barrier,
waits for everything it has in flight before its first store, and the first K-tile of the next output tile no longer waits
for the stores.  What can go wrong is a C element taken from another wave's region or from a stale block, another row's
residual, a store past M or past Cout, a row of the second tensor sent to the first, and a K-tile multiplied before it
has landed - the last only where a workgroup walks from one tile's epilogue into another tile.  So the shapes have a few
tiles more than the persistent grid holds workgroups (768 / 512 / 768 / 256 for the 64-row, 128-row, 128 x 64 and
two-K-group instances), a ragged last row tile and two K-tiles (the shortest loop: the epilogue's wait stands right
behind the request it waits for), with shift, residual and ReLU.

Every case is run twice (identical bytes) into a buffer with 64 sentinel rows behind the output, once against fp64 within
2e-6 of the range - the bound of tests/test_hip_h2_body.py - and once on exactly summable operands (tests/_exact_ref.py:
contract (1) / (2) of include/fgn_hip.h), bit for bit against the integer result."""
import pytest
import torch
import torch.nn.functional as F

import _exact_ref as R

pytestmark = pytest.mark.gpu

H2_BOUND = 2e-6       # of the fp64 range (tests/test_hip_conv.py::test_h2_*, tests/test_hip_h2_body.py)
SENTINEL = -7.0
_cache = {}

# tile code, rows, N, K: tiles over workgroups in the comment
CASES = [
    (64, 6203, 1024, 64),         # 97 x 8 = 776 tiles on 768 workgroups
    (64, 6203, 132, 64),          # the column guard: 132 of 256 columns - a write past column 132 lands in the next row
    (128, 8317, 1024, 64),        # 65 x 8 = 520 tiles on 512 workgroups
    (264, 98425, 64, 64),         # 128 rows x 64 columns: 769 tiles on 768 workgroups
    (1064, 2111, 1024, 128),      # two K-groups (the pass form is kept): 33 x 8 = 264 tiles on 256 workgroups
]
# contract (1): the exact classes with a shift; (2): rows up to 2^15 apart inside a wave, both planes in use (no shift)
EXACT_CLASSES = ('small', 'two_plane', 'rows_apart15')
# one output tile: a wave whose rows all lie past M (70 rows: the second wave row of each tile), one row into the second
# tile, and a workgroup with no next tile - the early wait has nothing to wait for and no K-tile follows it
ONE_TILE = [(64, 70, 132), (64, 65, 132), (128, 70, 132), (128, 129, 132), (264, 70, 52), (264, 129, 52)]


def _tile_rows(bm):
    return 64 if bm in (64, 1064) else 128


def _operands(rows, K, N):
    """tests/test_hip_h2_body.py::_operands: post-ReLU activations x weights with columns of different magnitude, a shift, a
    residual and the fp64 result - once per shape, shared and never written."""
    key = (rows, K, N)
    if key not in _cache:
        from fgn_amd import ops
        g = torch.Generator().manual_seed(rows + 7 * K + N)
        x = torch.randn(rows, K, generator=g).relu_()
        w = torch.randn(N, K, generator=g) / K ** 0.5
        w[1::3] *= 40.0
        shift, res = torch.randn(N, generator=g), torch.randn(rows, N, generator=g) * 3.0
        ref = torch.relu(x.double() @ w.double().T + shift.double() + res.double())
        _cache[key] = dict(x=x.cuda(), img=ops.pack_h2(w.cuda()), shift=shift.cuda(), res=res.cuda(), ref=ref.cuda())
    return _cache[key]


def _twice(tag, run):
    a = run()
    b = run()
    assert torch.equal(a, b), f'{tag}: two runs differ'
    return a


def _bounded(tag, got, ref):
    rng = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f'{tag}: max error {err / rng:.2e} of the range')
    assert err <= H2_BOUND * rng, (tag, err / rng)


def _exact(tag, got, want, tile):
    if torch.equal(got, want):
        return
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = bad.nonzero()
    print(f'{tag}: {int(bad.sum())} of {bad.numel()} elements wrong')
    for r, c in idx[:8].tolist():
        print(f'  row {r} (mod 16: {r % 16}, mod {tile}: {r % tile}) column {c}: got {got[r, c].item()!r}, want {want[r, c].item()!r}')
    assert False, f'{tag}: {int(bad.sum())} elements differ from the exact result (first: {idx[0].tolist()})'


def _gemm_run(x, img, rows, N, bm, **kw):
    from fgn_amd import ops

    def run():
        out = torch.full((rows + 64, N), SENTINEL, device='cuda')
        ops.gemm_h2(x, img, N, bm=bm, out=out[:rows], **kw)
        assert (out[rows:] == SENTINEL).all()              # the ragged last tile stops at M
        return out[:rows]
    return run


@pytest.mark.parametrize('bm,rows,N,K', CASES)
def test_full_epilogue_on_every_instance(bm, rows, N, K):
    o = _operands(rows, K, N)
    tag = f'bm {bm} {rows}x{K}->{N}'
    _bounded(tag, _twice(tag, _gemm_run(o['x'], o['img'], rows, N, bm, shift=o['shift'], residual=o['res'], relu=True)), o['ref'])


@pytest.mark.parametrize('cls', EXACT_CLASSES)
@pytest.mark.parametrize('bm,rows,N,K', CASES)
def test_full_epilogue_is_exact_on_summable_operands(bm, rows, N, K, cls):
    """``gemm_case`` asserts the class condition (``check_class``) on the CPU before anything is launched."""
    from fgn_amd import ops
    c = R.gemm_case(rows, K, N, cls, 'h2', False, 2 if bm == 1064 else 1, seed=9)
    x, img = c['x'][0].cuda(), ops.pack_h2(c['w'][0].cuda())
    shift = None if c['shift'] is None else c['shift'].cuda()
    tag = f'bm {bm} {rows}x{K}->{N} {cls}'
    got = _twice(tag, _gemm_run(x, img, rows, N, bm, shift=shift, residual=c['res'][0].cuda(), relu=True))
    _exact(tag, got, c['full'][0].float().cuda(), _tile_rows(bm))


@pytest.mark.parametrize('bm,rows,N', ONE_TILE)
def test_one_tile_launches(bm, rows, N):
    o = _operands(rows, 64, N)
    tag = f'one tile bm {bm} {rows}->{N}'
    _bounded(tag, _twice(tag, _gemm_run(o['x'], o['img'], rows, N, bm, shift=o['shift'], residual=o['res'], relu=True)), o['ref'])


@pytest.mark.parametrize('valid', [200, 70])
@pytest.mark.parametrize('bm', [128, 64])
def test_grouped_launch_walking_tiles(bm, valid):
    """36 groups of 256 rows (N = 1024, K = 64, with shift): 576 tiles of 128 rows on 512 workgroups, 1152 of 64 rows on
    768.  200 valid rows: the last active tile of a group is cut by them; 70: whole tiles are skipped by the walk and stay
    NaN.  3e38 lies in the rows past the valid ones: it must be fetched as zeros."""
    from fgn_amd import ops
    groups, grp_rows, K, N = 36, 256, 64, 1024
    key = ('grouped', valid)
    if key not in _cache:
        g = torch.Generator().manual_seed(61 + valid)
        x = torch.randn(groups, grp_rows, K, generator=g).relu_()
        x[:, valid:] = 3e38
        w = torch.randn(groups, N, K, generator=g) / K ** 0.5
        shift = torch.randn(N, generator=g)
        ref = torch.einsum('grk,gnk->grn', x[:, :valid].double(), w.double()) + shift.double()
        _cache[key] = dict(x=x.cuda(), img=ops.pack_h2(w.cuda()), shift=shift.cuda(), ref=ref.cuda())
    o = _cache[key]

    def run():
        buf = torch.full((groups * grp_rows + 64, N), float('nan'), device='cuda')
        buf[groups * grp_rows:] = SENTINEL
        out = buf[:groups * grp_rows].view(groups, grp_rows, N)
        ops.gemm_h2(o['x'], o['img'], N, shift=o['shift'], groups=groups, grp_valid=valid, bm=bm, out=out)
        assert (buf[groups * grp_rows:] == SENTINEL).all()
        assert torch.isnan(out[:, -(-valid // bm) * bm:]).all()          # whole tiles past the valid rows are not written
        return out[:, :valid].contiguous()
    tag = f'grouped bm {bm} valid {valid}'
    _bounded(tag, _twice(tag, run), o['ref'])


def _pair_case(stride):
    """3x3 / pad 1, 32 -> 128 channels with bias and ReLU on a 1 x 9 x 11 query and two 5 x 5 supports in one buffer: 99 + 50
    output rows at stride 1, 30 + 18 at stride 2 - the tensor boundary lies inside the first row tile, and inside a wave's
    16-row block (99 = 6 x 16 + 3, 30 = 16 + 14)."""
    key = ('pair', stride)
    if key not in _cache:
        g = torch.Generator().manual_seed(71 + stride)
        cin, cout = 32, 128
        wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        bias = torch.randn(cout, generator=g)
        xq = torch.randn(1, 9, 11, cin, generator=g).relu_()
        xs = torch.randn(2, 5, 5, cin, generator=g).relu_()
        buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).cuda()
        refs = [torch.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), bias.double(), stride=stride,
                                    padding=1)).permute(0, 2, 3, 1).contiguous().cuda() for x in (xq, xs)]
        _cache[key] = dict(wt=wt, bias=bias, q=buf[:xq.numel()].view(xq.shape), s=buf[xq.numel():].view(xs.shape), refs=refs)
    return _cache[key]


@pytest.mark.parametrize('bm', [64, 128, 264])
@pytest.mark.parametrize('cout', [64, 128])
@pytest.mark.parametrize('stride', [1, 2])
def test_two_tensor_boundary_inside_a_row_tile(stride, cout, bm):
    """``ops.conv2d_pair`` with the tile code forced: the rows from M0 = 99 / 30 on go to the second output."""
    from fgn_amd import ops
    c = _pair_case(stride)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(c['wt'][:cout], bias=c['bias'][:cout], stride=stride, pad=1, relu=True).to('cuda')
    # (pack_conv routes layers of at least 64 input channels to this kernel; the entry itself takes any multiple of 32)
    assert tuple(layer.w.shape) == (128, 9 * 32)
    if layer.wh is None:
        layer.wh = ops.pack_h2(layer.w)
    rq, rs = (r[..., :cout] for r in c['refs'])
    assert rq[0].numel() // cout == (99 if stride == 1 else 30)
    ref = torch.cat([rq.reshape(-1, cout), rs.reshape(-1, cout)])

    def run():
        outs = []
        for r in (rq, rs):
            rows = r.numel() // cout
            buf = torch.full((rows + 64, cout), SENTINEL, device='cuda')
            outs.append((buf, buf[:rows].view(r.shape)))
        ops.conv2d_pair(c['q'], c['s'], layer, out0=outs[0][1], out1=outs[1][1], bm=bm)
        for buf, o in outs:
            assert (buf[o.numel() // cout:] == SENTINEL).all()
        return torch.cat([o.reshape(-1, cout) for _, o in outs])
    tag = f'conv2d_pair 3x3/{stride} bm {bm} ->{cout}'
    _bounded(tag, _twice(tag, run), ref)


def test_dual_operand_launch_with_the_row_table():
    """``ops.conv1x1_dual``, 64 + 64 -> 1024 channels on 6203 rows (776 tiles of 64 rows on 768 workgroups), the second
    operand's rows taken through ``x2_rows``.  Reference: fp64 over the layer's own folded f32 weights."""
    from fgn_amd import lib, ops
    rows, cin, cout = 6203, 64, 1024
    assert lib.load().fgn_h2_row_tile(rows, cout, 2 * cin, 0, 0) == 64
    g = torch.Generator().manual_seed(83)
    y = torch.randn(rows, cin, generator=g).relu_().cuda()
    x = torch.randn(2 * rows, cin, generator=g).relu_().cuda()
    w3, wd = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5, torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    mk = lambda: dict(weight=torch.rand(cout, generator=g) + 0.5, bias=torch.randn(cout, generator=g) * 0.1,  # noqa: E731
                      running_mean=torch.randn(cout, generator=g) * 0.1, running_var=torch.rand(cout, generator=g) + 0.5)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv_dual(w3, mk(), wd, mk(), relu=True).to('cuda')
    assert layer.wh is not None
    tab = (torch.arange(rows, dtype=torch.int32) * 2).cuda()
    ref = torch.relu(torch.cat((y, x[tab.long()]), 1).double() @ layer.w[:cout].double().T + layer.shift.double())

    def run():
        buf = torch.full((rows + 64, cout), SENTINEL, device='cuda')
        ops.conv1x1_dual(y.view(1, rows, 1, cin), x.view(1, -1, 1, cin), layer, out=buf[:rows].view(1, rows, 1, cout), x2_rows=tab)
        assert (buf[rows:] == SENTINEL).all()
        return buf[:rows]
    with ops.gemm_math('h2'):
        _bounded('dual x2_rows', _twice('dual x2_rows', run), ref)
