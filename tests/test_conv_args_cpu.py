"""Return-code contract of the GEMM-shaped conv entry points (csrc/conv_igemm.hip) - host logic, no GPU involved.

Every entry point validates its arguments before its first HIP call and in a fixed order: a null required pointer gives
FGN_ERR_ARG (-2), then empty work gives FGN_OK (0), then an unsupported shape gives FGN_ERR_SHAPE (-1).  A call that
returns there never dereferences its pointers, so fabricated addresses serve as "a pointer".  The whole file is skipped
where a device is present: a wrongly ordered check must never be able to launch on a fabricated address, and without a
device it cannot (the first HIP call of every launcher fails and its code - a positive hipError_t - is returned)."""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='fabricated pointers: only where nothing can launch')

OK, ERR_SHAPE, ERR_ARG = 0, -1, -2
P = [0x10000000 + i * 0x01000000 for i in range(8)]       # "pointers", 16 MB apart

# name -> (argument names in ABI order, a call that passes validation, the required pointers, the row-count argument)
_CONV1X1 = ('x w y scale shift residual n_img_dev n_img H W Cin Cout cout_pad relu stream'.split(),
            dict(x=P[0], w=P[1], y=P[2], scale=P[3], shift=P[4], residual=None, n_img_dev=None, n_img=3, H=64, W=64, Cin=64,
                 Cout=128, cout_pad=128, relu=1, stream=None), ('x', 'w', 'y'), 'n_img')
_DUAL = ('x x2 x2_rows x2_total_rows w y shift rows Cin1 Cin2 Cout cout_pad relu stream'.split(),
         dict(x=P[0], x2=P[1], x2_rows=None, x2_total_rows=12288, w=P[2], y=P[3], shift=P[4], rows=12288, Cin1=64, Cin2=64,
              Cout=128, cout_pad=128, relu=1, stream=None), ('x', 'x2', 'w', 'y'), 'rows')
_WINOGRAD = ('V U Mo n_img_dev n_img tiles_per_img t_pad Cin Cout cout_pad n_groups stream'.split(),
             dict(V=P[0], U=P[1], Mo=P[2], n_img_dev=None, n_img=4, tiles_per_img=256, t_pad=1024, Cin=64, Cout=128,
                  cout_pad=128, n_groups=16, stream=None), ('V', 'U', 'Mo'), 'n_img')
_GEMM = dict(x=P[0], w=P[1], y=P[2], shift=P[3], residual=None, rows=12288, K=64, Cout=128, cout_pad=128, relu=0, grp_rows=0,
             grp_valid=0, n_groups=1, bm=0, nterms=6, stream=None)
ENTRIES = {
    'fgn_conv1x1_x3_nhwc_f32': _CONV1X1,
    'fgn_conv1x1_h2_nhwc_f32': _CONV1X1,
    'fgn_conv1x1_dual_nhwc_f32': _DUAL,
    'fgn_conv1x1_dual_x3_nhwc_f32': _DUAL,
    'fgn_conv1x1_dual_h2_nhwc_f32': _DUAL,
    'fgn_winograd_gemm_f32': _WINOGRAD,
    'fgn_winograd_gemm_x3_f32': _WINOGRAD,
    'fgn_winograd_gemm_h2_f32': _WINOGRAD,
    'fgn_gemm_x3_f32': ('x w y shift residual rows K Cout cout_pad relu grp_rows grp_valid n_groups bm nterms stream'.split(),
                        _GEMM, ('x', 'w', 'y'), 'rows'),
    'fgn_gemm_h2_f32': ('x w y shift residual rows K Cout cout_pad relu grp_rows grp_valid n_groups bm stream'.split(),
                        _GEMM, ('x', 'w', 'y'), 'rows'),
    'fgn_conv2d_nhwc_f32': ('x w y scale shift residual in_scale n_img_dev n_img H W Cin Cout cout_pad KH KW stride pad a_img_div '
                            'relu tile_hint ws ws_bytes stream'.split(),
                            dict(x=P[0], w=P[1], y=P[2], scale=P[3], shift=P[4], residual=None, in_scale=None, n_img_dev=None,
                                 n_img=2, H=32, W=32, Cin=64, Cout=128, cout_pad=128, KH=3, KW=3, stride=1, pad=1, a_img_div=1,
                                 relu=1, tile_hint=0, ws=None, ws_bytes=0, stream=None), ('x', 'w', 'y'), 'n_img'),
    'fgn_conv2d_pair_nhwc_f32': ('x0 y0 n_img0 H0 W0 x1 y1 n_img1 H1 W1 w scale shift Cin Cout cout_pad KH KW stride pad relu '
                                 'stream'.split(),
                                 dict(x0=P[0], y0=P[2], n_img0=1, H0=64, W0=64, x1=P[1], y1=P[3], n_img1=2, H1=32, W1=32, w=P[4],
                                      scale=P[5], shift=P[6], Cin=64, Cout=128, cout_pad=128, KH=3, KW=3, stride=2, pad=1, relu=1,
                                      stream=None), ('x0', 'y0', 'x1', 'y1', 'w'), 'n_img0'),
    'fgn_conv2d_pair_h2_nhwc_f32': ('x0 n_img0 H0 W0 x1 n_img1 H1 W1 w y0 y1 scale shift Cin Cout cout_pad KH KW stride pad relu '
                                    'stream'.split(),
                                    dict(x0=P[0], n_img0=1, H0=64, W0=64, x1=P[1], n_img1=2, H1=64, W1=64, w=P[4], y0=P[2],
                                         y1=P[3], scale=P[5], shift=P[6], Cin=64, Cout=128, cout_pad=128, KH=3, KW=3, stride=1,
                                         pad=1, relu=1, stream=None), ('x0', 'w', 'y0'), 'n_img0'),
}
PAIRS = ('fgn_conv2d_pair_nhwc_f32', 'fgn_conv2d_pair_h2_nhwc_f32')
CONV1X1 = [n for n, e in ENTRIES.items() if e is _CONV1X1]
DUAL = [n for n, e in ENTRIES.items() if e is _DUAL]
WINOGRAD = [n for n, e in ENTRIES.items() if e is _WINOGRAD]
GEMM = ['fgn_gemm_x3_f32', 'fgn_gemm_h2_f32']


def call(name, **changes):
    from fgn_amd import lib
    names, base, _, _ = ENTRIES[name]
    unknown = set(changes) - set(names)
    assert not unknown, f'{name} has no argument {unknown}'
    args = {**base, **changes}
    return getattr(lib.load(), name)(*[args[n] for n in names])


@pytest.mark.parametrize('name', ENTRIES)
def test_a_valid_description_gets_as_far_as_the_launch(name):
    """The calls the cases below are derived from pass every check: what comes back is the hipError_t of the launcher's
    first HIP call (positive), so each case below is rejected for the one thing it changes."""
    assert call(name) > 0


@pytest.mark.parametrize('name', ENTRIES)
def test_null_required_pointer_is_a_bad_argument_before_anything_else(name):
    _, _, required, rows = ENTRIES[name]
    for ptr in required:
        assert call(name, **{ptr: None}) == ERR_ARG, ptr
        assert call(name, **{ptr: None, rows: 0, 'cout_pad': 100}) == ERR_ARG, ptr      # before empty work and the shape
    if name == 'fgn_conv2d_pair_h2_nhwc_f32':
        assert call(name, y1=None) == ERR_ARG               # a second tensor needs its output
        assert call(name, x1=None, y1=None, n_img0=3) > 0   # one tensor: no second output needed


@pytest.mark.parametrize('name', ENTRIES)
def test_empty_work_is_ok_before_the_shape_is_looked_at(name):
    rows = ENTRIES[name][3]
    expect = ERR_SHAPE if name in PAIRS else OK             # the pair entries have no empty form
    for n in (0, -1):
        assert call(name, **{rows: n}) == expect
        assert call(name, **{rows: n, 'cout_pad': 100}) == expect
    if name in PAIRS:
        assert call(name, n_img1=0) == ERR_SHAPE


@pytest.mark.parametrize('name', ENTRIES)
def test_output_channel_padding_and_count_are_checked(name):
    assert call(name, cout_pad=100) == ERR_SHAPE            # not whole column tiles
    assert call(name, Cout=256) == ERR_SHAPE                # cout_pad < Cout
    if name != 'fgn_conv2d_nhwc_f32':                       # (the generic entry takes any channel count)
        assert call(name, Cout=6) == ERR_SHAPE              # rows are written 16 bytes at a time


@pytest.mark.parametrize('name', CONV1X1)
def test_conv1x1_shapes(name):
    assert call(name, Cin=48) == ERR_SHAPE
    assert call(name, Cin=32) == ERR_SHAPE                  # x3 / h2 need two K-tiles ...
    assert call(name, H=0) == ERR_SHAPE
    assert call(name, n_img=1, H=8, W=8) == ERR_SHAPE       # 64 rows x 128 x 64: the row-tile rule leaves it to the f32 entry


def test_the_f32_dual_and_winograd_entries_take_one_k_tile_per_operand():
    """... the f32 kernels do not: Cin 32 passes their validation (and fails at the first HIP call, there being no device)."""
    assert call('fgn_conv1x1_dual_nhwc_f32', Cin1=32, Cin2=32) > 0
    assert call('fgn_winograd_gemm_f32', Cin=32) > 0
    assert call('fgn_winograd_gemm_x3_f32', Cin=32) == ERR_SHAPE
    assert call('fgn_winograd_gemm_h2_f32', Cin=32) == ERR_SHAPE


@pytest.mark.parametrize('name', DUAL)
def test_dual_operands(name):
    assert call(name, Cin1=48) == ERR_SHAPE
    assert call(name, Cin2=0) == ERR_SHAPE
    assert call(name, x2_total_rows=12000) == ERR_ARG                       # no row table: x2 holds exactly the output's rows
    assert call(name, x2_total_rows=12000, x2_rows=P[7]) > 0                # with a table it may hold any number ...
    assert call(name, x2_total_rows=0, x2_rows=P[7]) == ERR_ARG             # ... but one
    assert call(name, x2_total_rows=12000, cout_pad=100) == ERR_SHAPE       # the shape is checked first


@pytest.mark.parametrize('name', WINOGRAD)
def test_winograd_gemm_shapes(name):
    assert call(name, Cin=48) == ERR_SHAPE
    assert call(name, n_groups=9) == ERR_SHAPE              # 16 = F(2x2), 36 = F(4x4)
    assert call(name, n_groups=36) > 0
    assert call(name, n_img=5) == ERR_SHAPE                 # 5 x 256 tiles > t_pad
    assert call(name, t_pad=96, n_img=1, tiles_per_img=96) == ERR_SHAPE     # a group is whole 64-row tiles


@pytest.mark.parametrize('name', GEMM)
def test_direct_gemm_shapes(name):
    assert call(name, K=48) == ERR_SHAPE
    assert call(name, K=0) == ERR_SHAPE
    assert call(name, K=32) == ERR_SHAPE                    # one K-tile: the launcher's check
    assert call(name, n_groups=0) == ERR_SHAPE
    assert call(name, n_groups=2, grp_rows=6144) > 0
    assert call(name, n_groups=2, grp_rows=6000) == ERR_SHAPE               # n_groups * grp_rows != rows
    assert call(name, n_groups=2, grp_rows=0) == ERR_SHAPE
    assert call(name, n_groups=2, grp_rows=6144, grp_valid=7000) == ERR_SHAPE
    assert call(name, bm=96) == ERR_SHAPE
    assert call(name, bm=64) > 0


def test_generic_and_pair_conv_shapes():
    for name in ('fgn_conv2d_nhwc_f32',) + PAIRS:
        assert call(name, Cin=48) == ERR_SHAPE
        assert call(name, stride=0) == ERR_SHAPE
    assert call('fgn_conv2d_nhwc_f32', a_img_div=0) == ERR_SHAPE
    assert call('fgn_conv2d_nhwc_f32', KH=9, KW=9, pad=4) == ERR_SHAPE      # tap validity is a 64-bit mask
    assert call('fgn_conv2d_nhwc_f32', H=1, W=1, pad=0) == ERR_SHAPE        # no output pixel
    assert call('fgn_conv2d_pair_nhwc_f32', H1=1, W1=1, pad=0) == ERR_SHAPE
    name = 'fgn_conv2d_pair_h2_nhwc_f32'
    assert call(name, Cin=96) == ERR_SHAPE                  # Cin / 32 not a power of two
    assert call(name, Cin=128) > 0
    assert call(name, KH=1, KW=3) == ERR_SHAPE              # KH != KW
    assert call(name, KH=5, KW=5, pad=2) == ERR_SHAPE       # 1x1 or 3x3
    assert call(name, x1=P[0] + (1 << 31)) == ERR_SHAPE     # both tensors within one 2 GiB descriptor
