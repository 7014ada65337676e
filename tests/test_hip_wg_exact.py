"""The Winograd path held to the EXACT result, in two layers, every comparison ``torch.equal`` on whole tensors
against float64 integer arithmetic - the style of tests/test_hip_conv_exact.py, which this path was the one family left
out of.  A mismatch prints the number of wrong elements, the first eight as (group / image, row, column, got, want) and
those rows modulo 32, 64 and 128 before it fails.

 1. The three grouped-GEMM entry points ALONE - ``fgn_winograd_gemm_f32``, ``fgn_winograd_gemm_x3_f32``,
    ``fgn_winograd_gemm_h2_f32`` - called as ``ops._winograd_gemm`` calls them, on the operand classes of
    tests/_exact_ref.py drawn per group (``wg_gemm_case``; the condition mag / unit <= 2^22 asserted there), at the smallest
    shapes that reach each instance (``WG_GEMM``: the tile every shape must be routed to is asserted, so a moved threshold
    fails here instead of unhooking the test).  V rows [valid, t_pad) of every group hold 3e38, Mo is filled with a finite
    sentinel pattern and compared as int32, and the launch runs under every kind of device count (``wg_counts``).
 2. Whole convolutions through ``ops.conv3x3_winograd`` / ``ops.conv3x3_winograd_multi`` on operands for which all four
    stages are exact (``wg_conv_case``: the per-stage conditions asserted on the CPU): equal to float64 ``F.conv2d`` and,
    bit for bit, to the direct kernel on the same operands; under gemm_math 'h2', 'x3' and 'f32', the route and the kernel
    of the grouped GEMM asserted from its profile record; images past a device count keep their bytes.

There is no tolerance in this file but the weight pack's (16 * 2^-53 mag before the one rounding to f32), which
the F(4x4) pack needs where the rational U is exactly 0 (``_layer``).  Not reached: the 16-byte instances of the F(4x4)
transforms (tiles * C >= 4 Mi: no float64 convolution of that size on a CPU; 7.4 bounds them alone)."""
import pytest
import torch

import _exact_ref as R
import _wg_ref
from test_hip_wg_bound import SENTINEL

pytestmark = pytest.mark.gpu

ERR_SHAPE = -1                      # FGN_ERR_SHAPE (include/fgn_hip.h)
ENTRY = {'h2': 'fgn_winograd_gemm_h2_f32', 'x3': 'fgn_winograd_gemm_x3_f32', 'f32': 'fgn_winograd_gemm_f32'}
F32_TILE = 64                       # fgn_winograd_gemm_f32 runs the 64 x 64 tile of the f32 MFMA kernels
MINUS_ZERO = -2 ** 31               # the bit pattern of -0.0 as int32


def _L():
    from fgn_amd import lib
    return lib.load()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _report(tag, got, want):
    """``got`` == ``want`` ([groups or images, rows, columns]) or a report of where they differ, then the failure"""
    if torch.equal(got, want):
        return
    got, want = got.reshape(got.shape[0], -1, got.shape[-1]), want.reshape(want.shape[0], -1, want.shape[-1])
    bad = (got != want) | (torch.isnan(got) != torch.isnan(want))
    idx = bad.nonzero()
    print(f'{tag}: {int(bad.sum())} of {bad.numel()} elements wrong')
    for g, r, c in idx[:8].tolist():
        print(f'  group / image {g} row {r} (mod 32: {r % 32}, mod 64: {r % 64}, mod 128: {r % 128}) column {c}: '
              f'got {got[g, r, c].item()!r}, want {want[g, r, c].item()!r}')
    assert False, f'{tag}: {int(bad.sum())} elements differ from the exact result (first: {idx[0].tolist()})'


# ----------------------------------------------------------------------------------------------------------------------
# 1. the grouped-GEMM entry points alone
# ----------------------------------------------------------------------------------------------------------------------
def _pack_u(arith, w, cout_pad):
    """U [groups, N, K] zero-padded to cout_pad rows, in the form the entry of ``arith`` reads"""
    from fgn_amd import ops
    groups, N, K = w.shape
    up = torch.zeros(groups, cout_pad, K, device='cuda')
    up[:, :N] = w.cuda()
    return up if arith == 'f32' else (ops.pack_h2(up) if arith == 'h2' else ops.pack_x3(up))


def _launch(arith, V, U, Mo, count, n_img, tiles_per_img, cout_pad):
    groups, t_pad, K = V.shape
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
    rc = getattr(_L(), ENTRY[arith])(V.data_ptr(), U.data_ptr(), Mo.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                     n_img, tiles_per_img, t_pad, K, Mo.shape[-1], cout_pad, groups,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _assert_tile(i):
    groups, t_pad, valid, K, N, n_img, tpi, tile = R.WG_GEMM[i]
    assert n_img * tpi == valid
    assert _L().fgn_h2_row_tile(groups * t_pad, N, K, t_pad, valid) == tile
    assert _L().fgn_x3_row_tile(groups * t_pad, N, K, t_pad, valid) == tile
    return tile


def _grouped(i, arith, x, w, prod, tag):
    """One operand set through the entry of ``arith`` under every device count of ``wg_counts``.  Per group: rows below
    min(n_img, count) * tiles_per_img equal the reference; rows from the next multiple of the row tile up to t_pad keep the
    sentinel.  The rows between - the rest of the last row tile a group computes - are UNSPECIFIED (the kernels write whole
    tiles: those rows hold products of the 3e38 pad rows or of images past the count), as the grouped tests of
    tests/test_hip_conv_exact.py treat them.  Columns are checked to N exactly: Mo is [groups, t_pad, N], not padded."""
    groups, t_pad, valid, K, N, n_img, tpi, tile = R.WG_GEMM[i]
    tile = tile if arith != 'f32' else F32_TILE
    cout_pad = (N + 127) // 128 * 128
    V = torch.full((groups, t_pad, K), 3e38, device='cuda')
    V[:, :valid] = x.cuda()
    U = _pack_u(arith, w, cout_pad)
    want = prod.float().cuda()
    assert torch.equal(want.double().cpu(), prod)
    for count in R.wg_counts(n_img, tpi, tile):
        rows = (n_img if count is None else min(n_img, count)) * tpi
        Mo = _sentinel(groups, t_pad, N)
        assert _launch(arith, V, U, Mo, count, n_img, tpi, cout_pad) == 0
        assert _untouched(Mo[:, -(-rows // tile) * tile:]), (tag, count)
        _report(f'{tag} count {count}', Mo[:, :rows], want[:, :rows])


def _cases():
    out = []
    for i, shape in enumerate(R.WG_GEMM):
        for arith, classes in R.WG_GEMM_CLASSES.items():
            if shape[7] == 0 and arith != 'f32':
                continue                                    # refused: test_image_entries_refuse_what_the_rule_leaves_to_f32
            out += [pytest.param(i, arith, cls, id=f'{"x".join(map(str, shape[:5]))}-{arith}-{cls}') for cls in classes]
    return out


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('i,arith,cls', _cases())
def test_grouped_gemm_entry_is_exact(i, arith, cls, scaled):
    """Every shape of ``WG_GEMM`` on every entry that takes it, all seven classes for h2, the classes of
    tests/test_hip_conv_exact.py for x3 and f32, each once more times 2^-9.  The epilogue of these entries has neither
    shift nor residual: the reference is ``prod``, group g's V times group g's U."""
    assert _assert_tile(i) > 0 or arith == 'f32'
    c = R.wg_gemm_case(i, cls, arith, scaled)
    _grouped(i, arith, c['x'], c['w'], c['prod'], f'{ENTRY[arith]} {R.WG_GEMM[i][:5]} {cls}{" 2^-9" if scaled else ""}')


@pytest.mark.parametrize('arith', ['h2', 'x3', 'f32'])
@pytest.mark.parametrize('i', [0, 3])
def test_only_one_groups_weights_are_non_zero(i, arith):
    """All of U zero but one group's: output computed from another group's weights shows at once (64- and 128-row tile)."""
    _assert_tile(i)
    c = R.wg_gemm_case(i, 'small', arith, False)
    g = 5
    w, prod = torch.zeros_like(c['w']), torch.zeros_like(c['prod'])
    w[g], prod[g] = c['w'][g], c['prod'][g]
    assert prod[g].abs().max() > 0
    _grouped(i, arith, c['x'], w, prod, f'{ENTRY[arith]} {R.WG_GEMM[i][:5]} one group')


@pytest.mark.parametrize('i', [i for i, s in enumerate(R.WG_GEMM) if s[7] == 0])
def test_image_entries_refuse_what_the_rule_leaves_to_f32(i):
    """Where ``fgn_h2_row_tile`` / ``fgn_x3_row_tile`` return 0 the image entries return FGN_ERR_SHAPE and write nothing
    (the f32 entry runs these shapes: test_grouped_gemm_entry_is_exact)."""
    assert _assert_tile(i) == 0
    groups, t_pad, valid, K, N, n_img, tpi, _ = R.WG_GEMM[i]
    c = R.wg_gemm_case(i, 'small', 'f32', False)
    cout_pad = (N + 127) // 128 * 128
    V = torch.zeros(groups, t_pad, K, device='cuda')
    V[:, :valid] = c['x'].cuda()
    for arith in ('h2', 'x3'):
        Mo = _sentinel(groups, t_pad, N)
        assert _launch(arith, V, _pack_u(arith, c['w'], cout_pad), Mo, None, n_img, tpi, cout_pad) == ERR_SHAPE
        assert _untouched(Mo)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the whole convolution
# ----------------------------------------------------------------------------------------------------------------------
def _layer(c, math, shifted, relu):
    """``ops.pack_winograd`` of the case's weights under ``math``.  The host pack is float64: for F(2x2) it returns the
    integer U bit for bit (asserted).  For F(4x4) it is within the pack's bound of the integer U everywhere and
    equal to it wherever |U| >= 1 (asserted) - but where the rational U is exactly 0, products of fl(1/3) and fl(1/15) that
    do not cancel leave residues of about 1e-14, which would turn an exact zero of Mo into 1e-13.  So the integer U is
    written into ``layer.u`` and the plane images are refreshed the way ``ops.repack_winograd_`` refreshes them."""
    from fgn_amd import ops
    m, cout = c['m'], c['cout']
    with ops.gemm_math(math):
        layer = ops.pack_winograd(c['wt'], bias=c['shift'] if shifted else None, relu=relu, m=m)
    _, mag = _wg_ref.pack_weights(c['wt'], _wg_ref.g64(m), m)
    assert _wg_ref.pack_ratio(layer.u[:, :cout], c['u'], mag) <= 1.0
    big = c['u'].abs() >= 1
    assert torch.equal(layer.u[:, :cout].double()[big], c['u'][big]) and (layer.u[:, cout:] == 0).all()
    if m == 2:
        assert torch.equal(layer.u[:, :cout].double(), c['u'])
    layer.u[:, :cout] = c['u'].float()
    if layer.uh is not None:
        layer.uh.copy_(ops.pack_h2(layer.u))
    if layer.u3 is not None:
        layer.u3.copy_(ops.pack_x3(layer.u))
    if shifted:
        assert torch.equal(layer.shift, c['shift'])
    return layer.to('cuda')


def _profiled(fn):
    """(result, the wg_gemm records of the launches ``fn`` makes)"""
    from fgn_amd import ops
    prev, ops.PROFILE = ops.PROFILE, ops.ConvProfile()
    try:
        out = fn()
        recs = [r for r in ops.PROFILE if r['kind'] == 'wg_gemm']
    finally:
        ops.PROFILE = prev
    return out, recs


def _expect(c, math):
    """-> (route, kernel name) of the grouped GEMM of case ``c`` under ``math``"""
    from fgn_amd import ops
    if math == 'f32' or c['route'] == 'f32':
        return 'f32', None
    if math == 'h2':
        return 'h2', ops.H2_KERNELS[c['tile']] % 'false'
    return 'x3', ops.X3_KERNELS[c['tile']]


def _assert_route(c, math, recs):
    assert len(recs) == 1, recs
    route, kernel = _expect(c, math)
    assert recs[0]['math'] == route, (recs[0]['math'], route)
    if kernel is not None:
        assert recs[0]['kernel'] == kernel, (recs[0]['kernel'], kernel)
    else:
        assert 'conv_pw_h2' not in recs[0]['kernel'] and 'conv_pw_x3' not in recs[0]['kernel'], recs[0]['kernel']


def _direct(c, x, vec, shifted, relu):
    """The same convolution on the direct kernel: ``ops.conv2d`` of ``ops.pack_conv(w, pad=1)``"""
    from fgn_amd import ops
    layer = ops.pack_conv(c['wt'], bias=c['shift'] if shifted else None, pad=1, relu=relu).to('cuda')
    return ops.conv2d(x, layer, in_scale=vec, a_img_div=c['div'])


SINGLE = [n for n, s in R.WG_CONV.items() if len(s[1]) == 1]
PAIRS = [n for n, s in R.WG_CONV.items() if len(s[1]) == 2]


@pytest.mark.parametrize('epilogue', [False, True])
@pytest.mark.parametrize('math', ['h2', 'x3', 'f32'])
@pytest.mark.parametrize('name', SINGLE)
def test_winograd_convolution_is_exact(name, math, epilogue):
    """``ops.conv3x3_winograd`` on every single-tensor case of ``WG_CONV``, without an epilogue and with an integer shift
    (in units of y's unit, at most 2^17 of them) and ReLU: equal to float64 F.conv2d, equal to the direct kernel bit for
    bit, no output -0.0 under ReLU.  Under every device count of the case the images below it are exact and the images
    from it on keep their sentinel bytes ("rows past a device count keep their bytes", tests/test_hip_launches.py)."""
    from fgn_amd import ops
    c = R.wg_conv_case(name)
    layer = _layer(c, math, epilogue, epilogue)
    (n, H, W), x = c['shapes'][0], c['xs'][0].cuda()
    n_img = n * c['div']
    vec = None if c['in_scale'][0] is None else c['in_scale'][0].cuda()
    want = c['refs'][0][(epilogue, epilogue)].float().cuda()
    assert torch.equal(want.double().cpu(), c['refs'][0][(epilogue, epilogue)])
    tag = f'{name} {math}{" shift + ReLU" if epilogue else ""}'
    for count in c['counts']:
        cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
        out = _sentinel(n_img, H, W, c['cout'])
        got, recs = _profiled(lambda: ops.conv3x3_winograd(x, layer, in_scale=vec, a_img_div=c['div'], n_img_dev=cnt, out=out))
        assert got is out
        _assert_route(c, math, recs)
        done = n_img if count is None else min(n_img, count)
        assert _untouched(out[done:]), (tag, count)
        _report(f'{tag} count {count}', out[:done].reshape(done, H * W, c['cout']), want[:done].reshape(done, H * W, c['cout']))
        if epilogue:
            assert not bool((out[:done].contiguous().view(torch.int32) == MINUS_ZERO).any())
    _report(f'{tag} against the direct kernel', _direct(c, x, vec, epilogue, epilogue).reshape(n_img, H * W, c['cout']),
            want.reshape(n_img, H * W, c['cout']))


@pytest.mark.parametrize('epilogue', [False, True])
@pytest.mark.parametrize('math', ['h2', 'x3', 'f32'])
@pytest.mark.parametrize('name', PAIRS)
def test_two_tensor_winograd_convolution_is_exact(name, math, epilogue):
    """``ops.conv3x3_winograd_multi`` on a 2 x 13 x 10 and a 3 x 7 x 9 tensor, F(4x4) (the two-tensor transform kernels)
    and F(2x2) (per-tensor launches), the outputs views of ONE sentinel buffer with a gap before, between and behind them:
    each equals the exact result and the single-tensor call bit for bit, no sentinel is left inside either output and none
    has changed around them."""
    from fgn_amd import ops
    c = R.wg_conv_case(name)
    layer = _layer(c, math, epilogue, epilogue)
    xs = [x.cuda() for x in c['xs']]
    gap, cout = 1024, c['cout']
    sizes = [x.shape[0] * x.shape[1] * x.shape[2] * cout for x in xs]
    buf = _sentinel(3 * gap + sum(sizes))
    o0, o1 = gap, 2 * gap + sizes[0]
    outs = [buf[o0:o0 + sizes[0]].view(*xs[0].shape[:3], cout), buf[o1:o1 + sizes[1]].view(*xs[1].shape[:3], cout)]
    _, recs = _profiled(lambda: ops.conv3x3_winograd_multi(xs, layer, outs))
    total = sum(n * R.wg_tiles(H, W, c['m']) for n, H, W in c['shapes'])
    t_pad = _L().fgn_winograd_t_pad(total)
    route = ops._gemm_route(_L(), layer.u3, layer.uh, layer.groups * t_pad, cout, c['cin'], t_pad, total)
    assert route == _expect(c, math)[0]
    if c['m'] == 4:                                           # (the per-tensor form of F(2x2) is not instrumented)
        _assert_route(c, math, recs)
    assert _untouched(buf[:o0]) and _untouched(buf[o0 + sizes[0]:o1]) and _untouched(buf[o1 + sizes[1]:])
    for i, (out, x) in enumerate(zip(outs, xs)):
        want = c['refs'][i][(epilogue, epilogue)].float().cuda()
        assert not bool((out.contiguous().view(torch.int32) == SENTINEL).any())
        _report(f'{name} {math} tensor {i}', out.reshape(out.shape[0], -1, cout), want.reshape(out.shape[0], -1, cout))
        assert torch.equal(ops.conv3x3_winograd(x, layer), out)
        if epilogue:
            assert not bool((out.contiguous().view(torch.int32) == MINUS_ZERO).any())


@pytest.mark.parametrize('name', ['f4_ragged', 'f4_guided', 'f4_small1', 'f2_dense'])
def test_device_pack_on_the_exact_weights(name):
    """``ops.repack_winograd_`` (wg_pack_weights_kernel, float64 on the device) on the weights of the exact cases: within
    the pack's bound of the integer U everywhere, equal to it wherever |U| >= 1 - and for F(2x2) everywhere.  Prints how
    many of the exact zeros of F(4x4) come out as exactly 0 (not required: DESIGN 7.8)."""
    from fgn_amd import ops
    c = R.wg_conv_case(name)
    m, cout = c['m'], c['cout']
    with ops.gemm_math('f32'):
        layer = ops.pack_winograd(torch.ones_like(c['wt']), m=m).to('cuda')
    ops.repack_winograd_(layer, c['wt'].cuda())
    got = layer.u[:, :cout].cpu()
    _, mag = _wg_ref.pack_weights(c['wt'], _wg_ref.g64(m), m)
    assert _wg_ref.pack_ratio(got, c['u'], mag) <= 1.0
    big = c['u'].abs() >= 1
    assert torch.equal(got.double()[big], c['u'][big]) and bool((layer.u[:, cout:] == 0).all())
    zeros = c['u'] == 0
    print(f'[wg-exact] device pack {name}: {int((got[zeros] == 0).sum())} of {int(zeros.sum())} exact zeros of U are 0')
    if m == 2:
        assert torch.equal(got.double(), c['u'])
