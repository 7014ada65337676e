"""Every conv and GEMM kernel held to the EXACT result on exactly summable operands (tests/_exact_ref.py: the operand classes
and the condition mag / unit <= 2^22 that makes every product and partial sum exact in f32, whatever the order of the sum,
the tile, the split or the arithmetic).  Every comparison is ``torch.equal`` against integer arithmetic on the whole
output: one wrong element anywhere fails it, however small beside its neighbours - a row of a wave, a column of a ragged
tile, a tap at an image border - which the bounds relative to the output range of tests/test_hip_conv.py,
test_hip_h2_body.py, test_hip_h2_kgroups.py and test_hip_train.py cannot see.  A mismatch prints the number of wrong
elements, the first eight as (row, column, got, want) and those rows modulo 32 and modulo the tile before it fails.

 conv_pw_h2_kernel   direct entry (ops.gemm_h2) on every tile code, grouped launches, and through ops.conv2d (1x1, device
                     count), ops.conv1x1_dual (with and without x2_rows), ops.conv2d_pair (3x3, stride 1 and 2, tile forced)
 f32 MFMA kernels    conv_igemm_kernel and its DMA / pair / persistent forms and splitk_epilogue_kernel through ops.conv2d,
                     ops.conv1x1_dual, ops.conv2d_pair under gemm_math('f32')
 conv_pw_x3_kernel   ops.gemm_x3, 64- and 128-row tile, six and nine terms
 gradient GEMMs      gemm_tn_kernel + gemm_tn_reduce_kernel (ops.gemm_tn), gemm_small_kernel (ops.gemm_small)
The one bounded test is ``test_h2_contract_beyond_the_exact_region``: where the header promises an absolute error only."""
import pytest
import torch

import _exact_ref as R

pytestmark = pytest.mark.gpu

SCALED = [False, True]


def _report(tag, got, want, tile=64):
    """``got`` == ``want`` (2-D, rows x columns) or a report of where they differ, then the failure"""
    if torch.equal(got, want):
        return
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = bad.nonzero()
    print(f'{tag}: {int(bad.sum())} of {bad.numel()} elements wrong')
    for r, c in idx[:8].tolist():
        print(f'  row {r} (mod 32: {r % 32}, mod {tile}: {r % tile}) column {c}: got {got[r, c].item()!r}, want {want[r, c].item()!r}')
    assert False, f'{tag}: {int(bad.sum())} elements differ from the exact result (first: {idx[0].tolist()})'


def _route(fn):
    """tests/test_hip_conv.py::_route: (result, the arithmetic each MFMA launch of ``fn`` ran on)"""
    from fgn_amd import ops
    prev, ops.PROFILE = ops.PROFILE, ops.ConvProfile()
    try:
        out = fn()
        maths = [r.get('math', 'f32') for r in ops.PROFILE if r['kind'] in ('conv', 'wg_gemm')]
    finally:
        ops.PROFILE = prev
    return out, maths


def _tile_rows(bm):
    return 64 if bm in (64, 1064) else 128


# ----------------------------------------------------------------------------------------------------------------------
# conv_pw_h2_kernel, direct entry
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.CLASSES)
@pytest.mark.parametrize('bm,rows,N,K', R.H2_GEMM)
def test_h2_gemm_is_exact(bm, rows, N, K, cls, scaled):
    """Persistent grids walked past their end, ragged last tiles, two to ten K-tiles, the column guard, two K-groups: no
    epilogue, and shift + residual + ReLU; the rows behind M keep their bytes."""
    from fgn_amd import ops
    c = R.gemm_case(rows, K, N, cls, 'h2', scaled, 2 if bm == 1064 else 1)
    x, img = c['x'][0].cuda(), ops.pack_h2(c['w'][0].cuda())
    shift = None if c['shift'] is None else c['shift'].cuda()
    for full in (False, True):
        out = torch.full((rows + 64, N), -7.0, device='cuda')
        kw = dict(shift=shift, residual=c['res'][0].cuda(), relu=True) if full else {}
        ops.gemm_h2(x, img, N, bm=bm, out=out[:rows], **kw)
        assert (out[rows:] == -7.0).all()
        _report(f'h2 bm {bm} {rows}x{K}->{N} {cls}{" 2^-9" if scaled else ""}{" epilogue" if full else ""}', out[:rows],
                (c['full'] if full else c['prod'])[0].float().cuda(), _tile_rows(bm))


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.CLASSES)
@pytest.mark.parametrize('bm,groups,grp_rows,valid,K,N', R.H2_GROUPED)
def test_grouped_h2_gemm_is_exact(bm, groups, grp_rows, valid, K, N, cls, scaled):
    """Fewer valid rows than a group holds, 3e38 behind them: it must reach neither a wave's scale nor the output; whole
    tiles past the valid rows are not written; the weight offset of a group enters the cursor."""
    from fgn_amd import ops
    c = R.gemm_case(valid, K, N, cls, 'h2', scaled, groups=groups)
    x = torch.full((groups, grp_rows, K), 3e38, device='cuda')
    x[:, :valid] = c['x'].cuda()
    res = torch.zeros(groups, grp_rows, N, device='cuda')
    res[:, :valid] = c['res'].cuda()
    img = ops.pack_h2(c['w'].cuda())
    tile = _tile_rows(bm)
    for full in (False, True):
        out = torch.full((groups, grp_rows, N), float('nan'), device='cuda')
        kw = dict(shift=None if c['shift'] is None else c['shift'].cuda(), residual=res, relu=True) if full else {}
        ops.gemm_h2(x, img, N, groups=groups, grp_valid=valid, bm=bm, out=out, **kw)
        assert torch.isnan(out[:, -(-valid // tile) * tile:]).all()
        _report(f'h2 grouped bm {bm} {cls}{" 2^-9" if scaled else ""}{" epilogue" if full else ""}',
                out[:, :valid].reshape(-1, N), (c['full'] if full else c['prod']).float().cuda().reshape(-1, N), tile)


# ----------------------------------------------------------------------------------------------------------------------
# the same kernel through the product's entries
# ----------------------------------------------------------------------------------------------------------------------
def _layer(c, stride, pad, relu, math, **kw):
    """``ops.pack_conv`` of a conv_case's integer weights under ``math``, then the exact epilogue set on the packed layer
    (BatchNorm's own fold is not exact): powers of two as scale, integers as shift; the packed weights are the integers."""
    from fgn_amd import ops
    wt = c['wt']
    with ops.gemm_math(math):
        layer = ops.pack_conv(wt, stride=stride, pad=pad, relu=relu, **kw)
    cout, cin, k, _ = wt.shape
    if layer.cin != 4:
        assert torch.equal(layer.w[:cout, :k * k * cin], wt.permute(0, 2, 3, 1).reshape(cout, -1))
        assert (layer.w[cout:] == 0).all() and (layer.w[:, k * k * cin:] == 0).all()
    layer.scale, layer.shift = c['scale'], c['shift']
    return layer.to('cuda')


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.ROW_CLASSES)
def test_h2_conv1x1_with_a_device_count_is_exact(cls, scaled):
    """ops.conv2d, 1x1, 64 -> 1024 channels on up to 100 images of 7 x 7 with a device count of 37: M = 1813 ends inside a
    64-row tile; scale, shift, residual and ReLU in the epilogue; the images past the count keep their bytes."""
    from fgn_amd import lib, ops
    n_img, cnt = 100, 37
    assert lib.load().fgn_h2_row_tile(n_img * 49, 1024, 64, 0, 0) == 64
    c = R.conv_named('h2_device_count', cls, scaled)
    layer = _layer(c, 1, 0, True, 'h2')
    assert layer.wh is not None
    count = torch.tensor([cnt], dtype=torch.int32, device='cuda')
    out = torch.full((n_img, 7, 7, 1024), -7.0, device='cuda')
    _, route = _route(lambda: ops.conv2d(c['xs'][0].cuda(), layer, residual=c['ress'][0].cuda(), n_img_dev=count, out=out))
    assert route == ['h2'], route
    assert (out[cnt:] == -7.0).all()
    _report(f'h2 conv2d device count {cls}', out[:cnt].reshape(-1, 1024), c['refs'][0][:cnt].float().cuda().reshape(-1, 1024))


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.CLASSES)
@pytest.mark.parametrize('table', [False, True])
@pytest.mark.parametrize('rows,cin1,cin2,cout,math', R.DUAL)
def test_dual_operand_conv_is_exact(rows, cin1, cin2, cout, math, table, cls, scaled):
    """ops.conv1x1_dual: on conv_pw_h2_kernel the operand switches inside the K loop (776 tiles of 64 rows on 768
    workgroups), on conv_pw_persist_kernel under gemm_math('f32'); with ``table`` the second operand's rows are every
    other row of a buffer twice as long (x2_rows).  float64 BatchNorm statistics whose folded scales are exactly 1 or 2:
    the packed weights are the integers."""
    from fgn_amd import ops
    c = R.dual_case(rows, cin1, cin2, cout, math, cls, scaled)
    with ops.gemm_math(math):
        layer = ops.pack_conv_dual(c['w1'], c['bn1'], c['w2'], c['bn2'], relu=True).to('cuda')
    assert torch.equal(layer.w[:cout].cpu(), c['w'][0]) and (layer.wh is not None) == (math == 'h2')
    assert torch.equal(layer.shift.cpu(), torch.zeros(cout) if c['shift'] is None else c['shift'])
    y, x = c['x'][0][:, :cin1].contiguous().cuda(), c['x'][0][:, cin1:].contiguous().cuda()
    tab = None
    if table:
        buf = torch.full((2 * rows, cin2), 3.0, device='cuda')
        buf[::2] = x
        x, tab = buf, (torch.arange(rows, dtype=torch.int32) * 2).cuda()
    got, route = _route(lambda: ops.conv1x1_dual(y.view(1, rows, 1, cin1), x.view(1, -1, 1, cin2), layer, x2_rows=tab))
    assert route == [math], route
    ref = torch.relu(c['prod'][0] + (0.0 if c['shift'] is None else c['shift'].double()))
    _report(f'dual {math} {rows} {cls}{" x2_rows" if table else ""}', got.view(rows, cout), ref.float().cuda())


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.CONV_CLASSES)
@pytest.mark.parametrize('bm,cout', [(64, 1024), (1064, 1024), (264, 64)])
@pytest.mark.parametrize('stride', [1, 2])
def test_h2_implicit_gemm_on_two_tensors_is_exact(stride, bm, cout, cls, scaled):
    """ops.conv2d_pair, 3x3 / pad 1 with the tile code forced, on a 1 x 80 x 80 and a 2 x 5 x 7 tensor in one buffer: 18
    K-tiles over nine taps, taps outside the image, the seam between the tensors inside a tile (264: the first 64 output
    channels on the 128 x 64 tile)."""
    from fgn_amd import ops
    c = R.conv_named(f'h2_pair_s{stride}', cls, scaled)
    sub = dict(c, wt=c['wt'][:cout], scale=c['scale'][:cout], shift=None if c['shift'] is None else c['shift'][:cout])
    layer = _layer(sub, stride, 1, True, 'h2')
    assert layer.wh is not None
    xq, xs = c['xs']
    buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).cuda()
    yq, ys = ops.conv2d_pair(buf[:xq.numel()].view(xq.shape), buf[xq.numel():].view(xs.shape), layer, bm=bm)
    got = torch.cat((yq.reshape(-1, cout), ys.reshape(-1, cout)))
    ref = torch.cat([r[..., :cout].reshape(-1, cout) for r in c['refs']]).float().cuda()
    _report(f'h2 conv2d_pair 3x3/{stride} bm {bm} {cls}', got, ref, _tile_rows(bm))


# ----------------------------------------------------------------------------------------------------------------------
# f32 MFMA kernels
# ----------------------------------------------------------------------------------------------------------------------
def _nhwc_rows(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.F32_CLASSES)
@pytest.mark.parametrize('case', range(len(R.F32_CASES)))
def test_f32_conv_is_exact_on_every_tile(case, cls, scaled):
    """The seven CASES of tests/test_hip_conv.py at every tile hint (0 = the plan's own choice, split-K where it splits)."""
    from fgn_amd import ops
    n, cin, h, w, cout, k, stride, pad, bn, bias, res, relu = R.F32_CASES[case]
    c = R.conv_named(f'f32_case{case}', cls, scaled)
    layer = _layer(c, stride, pad, relu, 'f32')
    assert layer.wh is None and layer.w3 is None
    r = None if c['ress'][0] is None else c['ress'][0].cuda()
    x, ref = c['xs'][0].cuda(), _nhwc_rows(c['refs'][0]).float().cuda()
    for tile in (0, 1, 2, 3, 4, -4):
        y, route = _route(lambda: ops.conv2d(x, layer, residual=r, tile_hint=tile))
        assert route == ['f32'], route
        _report(f'f32 case {case} tile {tile} {cls}', _nhwc_rows(y), ref)


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', ['small', 'two_plane'])
def test_f32_stem_is_exact(cls, scaled):
    """The Cin-4 7x7 / stride 2 stem (three real channels) on the LDS-DMA kernel's stem loader, tiles 0, 1, 3."""
    from fgn_amd import ops
    c = R.conv_named('f32_stem', cls, scaled)
    layer = _layer(dict(c, wt=c['wt'][:, :3].contiguous()), 2, 3, True, 'f32', pad_cin_to=4)
    assert layer.cin == 4 and float(c['xs'][0][..., 3].abs().max()) == 0.0
    for tile in (0, 1, 3):
        y = ops.conv2d(c['xs'][0].cuda(), layer, tile_hint=tile)
        _report(f'stem tile {tile} {cls}', _nhwc_rows(y), _nhwc_rows(c['refs'][0]).float().cuda())


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.F32_CLASSES)
def test_f32_input_scale_image_div_and_device_count_are_exact(cls, scaled):
    """Three output images per input image (a_img_div), each under its own per-channel input scale (powers of two), and a
    device count that stops the launch after four of the six: the rest keep their bytes."""
    from fgn_amd import ops
    c = R.conv_named('f32_in_scale', cls, scaled)
    layer = _layer(c, 1, 1, True, 'f32')
    x, vec, ref = c['xs'][0].cuda(), c['in_scale'][0].cuda(), c['refs'][0].float().cuda()
    with ops.gemm_math('f32'):
        y = ops.conv2d(x, layer, in_scale=vec, a_img_div=3)
        _report(f'in_scale {cls}', _nhwc_rows(y), _nhwc_rows(ref))
        out = torch.full_like(y, -7.0)
        ops.conv2d(x, layer, in_scale=vec, a_img_div=3, n_img_dev=torch.tensor([4], dtype=torch.int32, device='cuda'), out=out)
    assert (out[4:] == -7.0).all()
    _report(f'in_scale device count {cls}', _nhwc_rows(out[:4]), _nhwc_rows(ref[:4]))


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.F32_CLASSES)
@pytest.mark.parametrize('i', range(len(R.SPLIT_K)))
def test_split_k_is_exact(i, cls, scaled):
    """The three split-K shapes of tests/test_hip_conv.py and a 1x1 of exactly 32 K-tiles.  Where the plan splits the
    workspace is non-zero - asserted - so splitk_epilogue_kernel adds the slabs, the shift and the residual (once).  The
    plan splits no reduction of fewer than 32 K-tiles (plan_splits, csrc/conv_igemm.hip), which leaves the second and the
    third shape - 4 and 18 K-tiles - to one pass of the DMA kernel: asserted too, so that a plan that splits them again
    is noticed here.  The device count is honoured."""
    from fgn_amd import lib, ops
    n, h, w, cin, cout, k = R.SPLIT_K[i]
    ws = lib.load().fgn_conv2d_workspace_bytes(n, h, w, cin, cout, k, k, 1, k // 2, 0)
    assert (ws > 0) == (k * k * cin // 32 >= 32), ws
    c = R.conv_named(f'f32_splitk{i}', cls, scaled)
    layer = _layer(c, 1, k // 2, True, 'f32')
    x, r, ref = c['xs'][0].cuda(), c['ress'][0].cuda(), c['refs'][0].float().cuda()
    y, route = _route(lambda: ops.conv2d(x, layer, residual=r))
    assert route == ['f32'], route
    _report(f'split-K {i} {cls}', _nhwc_rows(y), _nhwc_rows(ref))
    if n > 2:
        out = torch.full_like(y, -3.0)
        ops.conv2d(x, layer, residual=r, n_img_dev=torch.tensor([n - 3], dtype=torch.int32, device='cuda'), out=out)
        assert (out[n - 3:] == -3.0).all()
        _report(f'split-K {i} device count {cls}', _nhwc_rows(out[:n - 3]), _nhwc_rows(ref[:n - 3]))


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.F32_CLASSES)
def test_persistent_pointwise_kernel_is_exact(cls, scaled):
    """conv_pw_persist_kernel at 4097 x 64 -> 1024: 65 x 16 = 1040 tiles on 1024 workgroups, a last tile of one row;
    kernel id 44 (tests/test_hip_conv.py::_ID_CASES)."""
    from fgn_amd import lib, ops
    c = R.conv_named('f32_persist', cls, scaled)
    layer = _layer(c, 1, 0, False, 'f32')
    assert lib.load().fgn_conv2d_kernel_id(1, 4097, 1, 64, 1024, layer.cout_pad, 1, 1, 1, 0, 1, 0, 1, 0) == 44
    y, route = _route(lambda: ops.conv2d(c['xs'][0].cuda(), layer, residual=c['ress'][0].cuda()))
    assert route == ['f32'], route
    _report(f'persist {cls}', _nhwc_rows(y), _nhwc_rows(c['refs'][0]).float().cuda())


@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', ['small', 'two_plane'])
@pytest.mark.parametrize('i', range(len(R.PAIR_F32)))
def test_f32_two_tensor_launch_is_exact(i, cls, scaled):
    """ops.conv2d_pair on conv_igemm_dma_pair_kernel: a 1 x 40 x 67 query map and nine 32 x 32 supports, 3x3 / 2, 1x1 / 2,
    3x3 / 1 and the 7x7 / 2 stem."""
    from fgn_amd import ops
    cin, cout, k, stride = R.PAIR_F32[i]
    c = R.conv_named(f'f32_pair{i}', cls, scaled)
    sub = dict(c, wt=c['wt'][:, :3].contiguous()) if cin == 4 else c
    layer = _layer(sub, stride, k // 2, True, 'f32', **({'pad_cin_to': 4} if cin == 4 else {}))
    assert layer.wh is None
    (yq, ys), route = _route(lambda: ops.conv2d_pair(c['xs'][0].cuda(), c['xs'][1].cuda(), layer))
    assert route == ['f32'], route
    _report(f'f32 pair {i} query {cls}', _nhwc_rows(yq), _nhwc_rows(c['refs'][0]).float().cuda())
    _report(f'f32 pair {i} supports {cls}', _nhwc_rows(ys), _nhwc_rows(c['refs'][1]).float().cuda())


# ----------------------------------------------------------------------------------------------------------------------
# conv_pw_x3_kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scaled', SCALED)
@pytest.mark.parametrize('cls', R.X3_CLASSES)
@pytest.mark.parametrize('groups,grp_rows,valid,K,N', R.X3_GEMM)
def test_x3_gemm_is_exact(groups, grp_rows, valid, K, N, cls, scaled):
    """ops.gemm_x3 on the 64- and the 128-row tile with six and nine terms (the library has nine for the 64-row tile only):
    at most 16 significant bits per operand, so the third planes are zero and the dropped terms vanish."""
    from fgn_amd import lib, ops
    c = R.gemm_case(valid, K, N, cls, 'x3', scaled, groups=groups)
    x = torch.full((groups, grp_rows, K), 3e38, device='cuda')
    x[:, :valid] = c['x'].cuda()
    res = torch.zeros(groups, grp_rows, N, device='cuda')
    res[:, :valid] = c['res'].cuda()
    img = ops.pack_x3(c['w'].cuda())
    ran = 0
    for bm in (64, 128):
        if groups > 1 and grp_rows % bm:
            continue
        for nt in (6, 9):
            for full in (False, True):
                out = torch.full((groups, grp_rows, N), float('nan'), device='cuda')
                kw = dict(shift=None if c['shift'] is None else c['shift'].cuda(), residual=res, relu=True) if full else {}
                try:
                    ops.gemm_x3(x, img, N, groups=groups, grp_valid=valid, bm=bm, nterms=nt, out=out, **kw)
                except lib.FgnHipError:
                    assert bm == 128 and nt == 9
                    continue
                ran += 1
                assert torch.isnan(out[:, -(-valid // bm) * bm:]).all()
                _report(f'x3 bm {bm} nterms {nt} {groups}x{valid}x{K}->{N} {cls}{" epilogue" if full else ""}',
                        out[:, :valid].reshape(-1, N), (c['full'] if full else c['prod']).float().cuda().reshape(-1, N), bm)
    assert ran >= 6


# ----------------------------------------------------------------------------------------------------------------------
# gradient GEMMs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R_,M,N', R.TN_GEMM)
def test_weight_gradient_gemm_is_exact(R_, M, N):
    """ops.gemm_tn on the shapes of tests/test_hip_train.py (6272 and 5000 rows shrunk to 520: still two row slabs, so
    gemm_tn_reduce_kernel runs - asserted)."""
    from fgn_amd import lib, ops
    a, b, ref = R.grad_case(R_, M, N)
    if R_ == 520:
        assert lib.load().fgn_gemm_tn_workspace_bytes(R_, M, N) > 0
    _report(f'gemm_tn {R_}x{M}x{N}', ops.gemm_tn(a.cuda(), b.cuda()), ref.float().cuda())


@pytest.mark.parametrize('m,k,n,trans,stride_pad', R.SMALL_GEMM)
def test_small_gemm_is_exact(m, k, n, trans, stride_pad):
    from fgn_amd import ops
    a, b, ref = R.grad_case(k, m, n)                         # a [k, m]
    a_full = torch.full((k, m + stride_pad) if trans else (m, k + stride_pad), 5.0)
    if trans:
        a_full[:, :m] = a
        av = a_full.cuda()[:, :m]
    else:
        a_full[:, :k] = a.t()
        av = a_full.cuda()[:, :k]
    _report(f'gemm_small {m}x{k}x{n}', ops.gemm_small(av, b.cuda(), trans_a=trans), ref.float().cuda())


# ----------------------------------------------------------------------------------------------------------------------
# the h2 contract beyond the exact region
# ----------------------------------------------------------------------------------------------------------------------
def test_h2_contract_beyond_the_exact_region():
    """Rows up to 2^30 (even 128-row tiles) and 2^40 (odd ones) below the largest row of their 32-row block, where
    csrc/conv_pw_h2.h promises an absolute error only: for every element

        |got - ref| <= 2^-38 Amax sum_k |w[n, k]| + 3 K 2^-24 mag

    Amax = the largest |a| among the rows of the element's output tile (an upper bound of whatever maximum a wave chose its
    scale for), 2^-38 = half an f16 subnormal quantum over 2^13 (the header's constant), the second term the f32 roundings
    that appear once values are no longer multiples of one unit.  The rows within 2^15 of their wave's maximum are still
    exact (their elements have at most 22 significant bits: both planes at full precision), every output is finite.
    bm 64: a wave holds 32 rows; bm 128: 64."""
    from fgn_amd import ops
    rows, K, N = 1000, 96, 260
    o = R.make(rows, K, N, 'two_plane', 'h2', seed=90)
    r = torch.arange(rows)
    top = torch.where((r // 128) % 2 == 0, 30, 40)
    drop = ((r * 7) % 32) * top // 31                        # 0 .. top inside every 32 rows
    a = o['a'] * (2.0 ** (top - drop).double())[:, None]
    w = o['w'][:, 0]
    x32, w32 = a.float(), w.float()
    assert torch.equal(x32.double(), a) and torch.equal(w32.double(), w)
    ref, mag = a @ w.T, a.abs() @ w.abs().T                  # exact in float64: one row exponent per element
    wsum = w.abs().sum(1)
    img = ops.pack_h2(w32.cuda())
    rowmax = a.abs().amax(1)
    for bm, wave in ((64, 32), (128, 64)):
        got = ops.gemm_h2(x32.cuda(), img, N, bm=bm).cpu().double()
        assert torch.isfinite(got).all()
        tile = _tile_rows(bm)
        pad = -(-rows // tile) * tile
        amax = torch.zeros(pad, dtype=torch.float64)
        amax[:rows] = rowmax
        amax = amax.view(-1, tile).amax(1).repeat_interleave(tile)[:rows]
        bound = 2.0 ** -38 * amax[:, None] * wsum[None, :] + 3 * K * 2.0 ** -24 * mag
        err = (got - ref).abs()
        print(f'bm {bm}: worst error / bound {(err / bound).max().item():.3g}; inexact elements {int((err > 0).sum())}')
        assert (err <= bound).all(), (bm, (err / bound).max().item())
        wmax = torch.zeros(-(-rows // wave) * wave, dtype=torch.float64)
        wmax[:rows] = rowmax
        wmax = wmax.view(-1, wave).amax(1).repeat_interleave(wave)[:rows]
        near = rowmax * 2.0 ** 15 >= wmax
        assert near.any() and (~near).any()
        _report(f'h2 contract bm {bm}: rows within 2^15 of their wave\'s maximum', got[near].float(), ref[near].float(), tile)
