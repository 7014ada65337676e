"""conv_pw_h2_kernel_dual (two operands: conv3 + shortcut as one K loop) against the one-operand conv_pw_h2_kernel on the
concatenated operand [rows, Cin1 + Cin2] with the same packed weight image: both walk the same K-tiles on the same
fragments, so the results are the same bytes on every tile code and on the unforced route."""
import pytest
import torch

_ROWS = 6200                    # ragged against 64 (96.875 tiles) and 128
_COUT = 256
_SHAPES = [(64, 64), (128, 256)]
_CODES = [0, 64, 128, 264, 1064]    # 0: the library's choice


def _layer(cin1, cin2, seed):
    from fgn_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(_COUT, cin1 + cin2, generator=g) * 0.05
    shift = torch.randn(_COUT, generator=g)
    return ops.DualConvLayer(w.contiguous(), shift.contiguous(), cin1, cin2, _COUT, _COUT, True, None, ops.pack_h2(w)).to('cuda')


_CACHE = {}


def _case(cin1, cin2, gather):
    """(layer, x1, x2, x2_rows, the concatenated operand), computed once per shape"""
    key = (cin1, cin2, gather)
    if key not in _CACHE:
        g = torch.Generator(device='cuda').manual_seed(cin1 + 3 * cin2 + gather)
        layer = _layer(cin1, cin2, cin1 + cin2)
        x1 = torch.randn(_ROWS, cin1, generator=g, device='cuda')
        x2 = torch.randn(_ROWS * (2 if gather else 1), cin2, generator=g, device='cuda') * 3.0
        rows = torch.arange(0, 2 * _ROWS, 2, dtype=torch.int32, device='cuda') if gather else None
        cat = torch.cat((x1, x2[::2] if gather else x2), 1).contiguous()
        _CACHE[key] = (layer, x1, x2, rows, cat)
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize('gather', [False, True])
@pytest.mark.parametrize('bm', _CODES)
@pytest.mark.parametrize('cin1,cin2', _SHAPES)
def test_dual_instance_equals_one_operand_instance(cin1, cin2, bm, gather):
    from fgn_amd import ops
    layer, x1, x2, rows, cat = _case(cin1, cin2, gather)
    prev, ops.PROFILE = ops.PROFILE, ops.ConvProfile()
    try:
        y2 = ops.conv1x1_dual(x1, x2, layer, x2_rows=rows, bm=bm)
        recs = list(ops.PROFILE)
    finally:
        ops.PROFILE = prev
    y1 = ops.gemm_h2(cat, layer.wh, _COUT, shift=layer.shift, relu=True, bm=bm)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    assert (y2 > 0).any() and (y2 == 0).any()                     # shift and ReLU acted
    # the record names the dual instance of the tile the launch ran on
    k = cin1 + cin2
    code = bm
    if code == 0:
        code = 1064 if ops.h2_kernel(_ROWS, _COUT, k).endswith('2>') else 64
    assert len(recs) == 1 and recs[0]['math'] == 'h2' and recs[0]['kernel'] == ops.H2_DUAL_KERNELS[code], recs


def test_kernel_names_are_unchanged():
    from fgn_amd import ops
    assert ops.H2_KERNELS == {64: 'conv_pw_h2_kernel<2, 2, 1, 2, %s, 1>', 128: 'conv_pw_h2_kernel<2, 2, 2, 2, %s, 1>',
                              264: 'conv_pw_h2_kernel<4, 1, 1, 2, %s, 1>', 1064: 'conv_pw_h2_kernel<2, 2, 1, 2, %s, 2>'}
    assert ops.h2_kernel(6504, 256, 1024) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 2>'
    assert ops.h2_kernel(6504, 256, 2304, im2col=True) == 'conv_pw_h2_kernel<2, 2, 1, 2, true, 2>'
    assert ops.h2_kernel(6504, 1024, 256) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 1>'
    assert ops.h2_kernel(36 * 1280, 512, 512, 1280, 1236) == 'conv_pw_h2_kernel<2, 2, 2, 2, false, 1>'
    assert ops.h2_kernel(_ROWS, _COUT, 128) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 1>'
    assert ops.h2_kernel(_ROWS, _COUT, 384) == 'conv_pw_h2_kernel<2, 2, 1, 2, false, 2>'
    # the dual records: one instance per tile code, every name under the same prefix
    assert set(ops.H2_DUAL_KERNELS) == set(ops.H2_KERNELS)
    assert all(n.startswith('conv_pw_h2_kernel') for n in ops.H2_DUAL_KERNELS.values())
    assert ops.h2_dual_kernel(_ROWS, _COUT, 128) == 'conv_pw_h2_kernel_dual<2, 2, 1, 2, 1>'
    assert ops.h2_dual_kernel(_ROWS, _COUT, 384) == 'conv_pw_h2_kernel_dual<2, 2, 1, 2, 2>'
    assert ops.h2_dual_kernel(_ROWS, _COUT, 384, bm=128) == 'conv_pw_h2_kernel_dual<2, 2, 2, 2, 1>'
