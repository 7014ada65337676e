"""The Winograd cases of tests/_exact_ref.py (``WG_GEMM`` / ``wg_gemm_case``, ``WG_CONV`` / ``wg_conv_case``) pinned without a
GPU, for every shape and class tests/test_hip_wg_exact.py runs: the conditions hold per element, the float64 chain through
tests/_wg_ref.py IS the convolution, the host pack has the two properties the GPU file relies on, the routing table is what
the host rule returns, and a numpy f32 restatement of the two transforms - every multiply and add rounded to f32, and once
more with ``fmaf`` as one rounding (tests/test_wg_ref_cpu.py's emulation) - returns the float64 result BIT FOR BIT on these
operands: the witness that a mismatch on the GPU is the kernel's and not the class's."""
import numpy as np
import pytest
import torch

import _exact_ref as R
import _wg_ref
from test_wg_ref_cpu import _at2, _at4, _bt2, _bt4, _two_passes


@pytest.fixture(scope='module')
def L():
    from fgn_amd import lib
    return lib.load()


# ------------------------------------------------------------------------------------------ routing (host logic)
@pytest.mark.parametrize('i', range(len(R.WG_GEMM)))
def test_grouped_gemm_shapes_reach_the_tile_they_are_listed_for(L, i):
    groups, t_pad, valid, K, N, n_img, tpi, tile = R.WG_GEMM[i]
    assert n_img * tpi == valid <= t_pad and t_pad % 128 == 0 and groups in (16, 36)
    assert L.fgn_h2_row_tile(groups * t_pad, N, K, t_pad, valid) == tile
    assert L.fgn_x3_row_tile(groups * t_pad, N, K, t_pad, valid) == tile
    nt = -(-N // 128)
    if i == 1:
        assert groups * t_pad // 64 * nt == 192                       # exactly the threshold ...
        assert L.fgn_h2_row_tile(groups * (t_pad - 64), N, K, t_pad - 64, valid) == 0       # ... one row tile fewer: refused
        assert 192 < valid < 256                                      # valid ends inside the fourth tile
    if i == 4:
        assert groups * (t_pad // 128) * nt == 400
        assert L.fgn_h2_row_tile(groups * t_pad, N - 128, K, t_pad, valid) == 64           # one column tile fewer: 64 rows
    if tile == 128:
        assert L.fgn_h2_row_tile(groups * t_pad, N, 128, t_pad, valid) == 64               # K < 256: 64 rows
    for c in R.wg_counts(n_img, tpi, tile or 64):
        assert c is None or 0 <= c <= n_img + 2
    inside, edge = R.wg_counts(n_img, tpi, tile or 64)[2:4]
    assert (inside * tpi) % (tile or 64) != 0
    if n_img * tpi > (tile or 64):
        assert edge not in (0, n_img + 2) and (edge * tpi) % (tile or 64) == 0


@pytest.mark.parametrize('name', sorted(R.WG_CONV))
def test_convolution_cases_reach_the_route_they_are_listed_for(L, name):
    """The grouped GEMM of every case under gemm_math('h2') / ('x3'): the layer carries the image (``ops._h2_ok`` /
    ``_x3_ok``) and the tile rule takes the launch, or the f32 entry runs it."""
    from fgn_amd import ops
    m, shapes, cin, cout, kind, div, counts, route, tile = R.WG_CONV[name]
    total = sum(n * div * R.wg_tiles(H, W, m) for n, H, W in shapes)
    t_pad = L.fgn_winograd_t_pad(total)
    rows = (m + 2) ** 2 * t_pad
    for math, ok, rule in (('h2', ops._h2_ok, L.fgn_h2_row_tile), ('x3', ops._x3_ok, L.fgn_x3_row_tile)):
        with ops.gemm_math(math):
            got = rule(rows, cout, cin, t_pad, total) if ok(cin, cout) else 0
        assert got == tile, (math, got)
    assert (route == 'h2') == (tile > 0)
    assert all(c is None or 0 <= c for c in counts)


# ------------------------------------------------------------------------------------------ the grouped-GEMM operands
def _gemm_params():
    return [(i, a, cls) for i, s in enumerate(R.WG_GEMM) for a, classes in R.WG_GEMM_CLASSES.items()
            if s[7] > 0 or a == 'f32' for cls in classes]


@pytest.mark.parametrize('i,arith,cls', _gemm_params())
def test_grouped_operands_meet_the_condition(i, arith, cls):
    """``gemm_case`` asserts mag / unit <= 2^22 per element; the groups' operands differ; the operands survive f32; the
    scaled case is the unscaled one times powers of two."""
    c = R.wg_gemm_case(i, cls, arith, False)
    groups, _, valid, K, N = R.WG_GEMM[i][:5]
    assert tuple(c['x'].shape) == (groups, valid, K) and tuple(c['w'].shape) == (groups, N, K)
    assert not torch.equal(c['x'][0], c['x'][1]) and not torch.equal(c['w'][0], c['w'][groups - 1])
    g = groups - 1
    assert torch.equal(c['x'][g].double() @ c['w'][g].double().T, c['prod'][g])          # group g's V times group g's U
    s = R.wg_gemm_case(i, cls, arith, True)
    assert torch.equal(s['prod'].float().double(), s['prod']) and s['x'].dtype == torch.float32


def test_scaled_grouped_case_is_gemm_case_scaled():
    c = R.gemm_case(100, 64, 384, 'two_plane', 'h2', True, groups=36, seed=300)
    s = R.wg_gemm_case(0, 'two_plane', 'h2', True)
    assert torch.equal(c['x'], s['x']) and torch.equal(c['w'], s['w']) and torch.equal(c['prod'], s['prod'])


# ------------------------------------------------------------------------------------------ whole convolutions
@pytest.mark.parametrize('name', sorted(R.WG_CONV))
def test_convolution_case_meets_the_conditions_and_the_host_pack_properties(name):
    """``wg_conv_case`` asserts the four conditions per element and that the float64 chain pack -> input transform ->
    einsum -> output transform equals F.conv2d exactly.  Here: its U is what tests/_wg_ref.py's float64 pack returns to
    within the pack bound; ``ops.pack_winograd`` is within that bound of the integer U everywhere and equal to it wherever
    |U| >= 1; for F(2x2) it IS the integer U; for F(4x4) it is not, exactly where the rational U is 0 (residues of
    fl(1/3) and fl(1/15) products, below 1e-12) - the reason the GPU file writes the integers into the layer."""
    from fgn_amd import ops
    c = R.wg_conv_case(name)
    m, cout = c['m'], c['cout']
    print(f'[wg-exact] {name}: worst mag / unit = ' + ', '.join(f'{k} 2^{np.log2(v):.2f}' for k, v in c['worst'].items()))
    assert c['worst']['v'] <= R.WG_LIMIT and c['worst']['y'] <= R.WG_LIMIT
    assert c['worst']['mo'] <= R.LIMIT and c['worst']['direct'] <= R.LIMIT
    assert torch.equal(c['u'], c['u'].round()) and torch.equal(c['u'].float().double(), c['u'])
    want, mag = _wg_ref.pack_weights(c['wt'], _wg_ref.g64(m), m)
    assert _wg_ref.pack_ratio(c['u'].float(), want, mag) <= 1.0
    for math in ('h2', 'f32'):
        with ops.gemm_math(math):
            layer = ops.pack_winograd(c['wt'], bias=c['shift'], relu=True, m=m)
        got = layer.u[:, :cout].double()
        assert _wg_ref.pack_ratio(layer.u[:, :cout], c['u'], mag) <= 1.0
        big = c['u'].abs() >= 1
        assert torch.equal(got[big], c['u'][big])
        off = got != c['u']
        if m == 2:
            assert not off.any()
        else:
            assert (c['u'][off] == 0).all() and (got[off].abs() < 1e-12).all()
        assert torch.equal(layer.shift, c['shift'])
    for refs in c['refs']:
        assert (refs[(False, False)] != 0).double().mean() > 0.05             # not a test of zeros


def _patches(xp, R_, m, ty, tx):
    """xp [n, m ty + 2, m tx + 2, C] -> [n ty tx C, R, R] in the order of V's rows (tile-major, channel-minor)"""
    p = xp.unfold(1, R_, m).unfold(2, R_, m)                                   # [n, ty, tx, C, R, R]
    assert p.shape[1] == ty and p.shape[2] == tx
    return p.reshape(-1, R_, R_).numpy().astype(np.float32)


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('name', sorted(R.WG_CONV))
def test_f32_restatement_of_the_transforms_is_exact(name, fused):
    """The kernels' 1-D passes in numpy float32 (no contraction at all / every ``fmaf`` one rounding) on the operands of the
    case: the input transform returns V and the output transform returns y (with and without the shift), equal to the
    float64 chain in every bit."""
    c = R.wg_conv_case(name)
    m, C, cout, div = c['m'], c['cin'], c['cout'], c['div']
    R_ = m + 2
    bt, at = (_bt4, _at4) if m == 4 else (_bt2, _at2)
    for (n, H, W), x, vec, v, mo, refs in zip(c['shapes'], c['xs'], c['in_scale'], c['v'], c['mo'], c['refs']):
        ty, tx = _wg_ref.tiles_of(H, W, m)
        n_img = n * div
        xe = x.repeat_interleave(div, 0)
        if vec is not None:
            xe = xe * vec[:, None, None, :]                                   # f32 product (a power of two: exact)
        xp = torch.zeros(n_img, m * ty + 2, m * tx + 2, C)
        xp[:, 1:H + 1, 1:W + 1] = xe
        got = _two_passes(_patches(xp, R_, m, ty, tx), bt, fused)             # [tiles C, R, R]
        want = v.reshape(R_, R_, n_img * ty * tx * C).permute(2, 0, 1).numpy()
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
        q = mo.reshape(R_, R_, -1).permute(2, 0, 1).numpy()
        assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
        yt = _two_passes(q.astype(np.float32), at, fused)                      # [tiles cout, m, m]
        for sh in (False, True):
            y = yt + c['shift'].numpy()[None, :].repeat(n_img * ty * tx, 0).reshape(-1)[:, None, None] if sh else yt
            assert y.dtype == np.float32
            y = y.reshape(n_img, ty, tx, cout, m, m).transpose(0, 1, 4, 2, 5, 3).reshape(n_img, ty * m, tx * m, cout)
            assert np.array_equal(y[:, :H, :W].astype(np.float64), refs[(sh, False)].numpy())
