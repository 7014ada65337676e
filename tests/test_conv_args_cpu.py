"""Return-code contract of the GEMM-shaped conv entry points (csrc/conv_igemm.hip) - host logic, no GPU involved.

Every entry point validates its arguments before its first HIP call and in a fixed order: a null required pointer gives
FGN_ERR_ARG (-2), then empty work gives FGN_OK (0), then an unsupported shape gives FGN_ERR_SHAPE (-1).  A call that
returns there never dereferences its pointers, so fabricated addresses serve as "a pointer".  The whole file is skipped
where a device is present: a wrongly ordered check must never be able to launch on a fabricated address, and without a
device it cannot (the first HIP call of every launcher fails and its code - a positive hipError_t - is returned).

The second half pins what the direct family decides per launch - fgn_conv2d_kernel_id, fgn_conv2d_workspace_bytes and the
return code of fgn_conv2d_nhwc_f32 come from one plan (ConvPlan in conv_igemm.hip) - at the launches of a cfg3 episode and
on both sides of every threshold of that plan."""
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
    name = 'fgn_conv2d_nhwc_f32'
    assert call(name, n_img=2, H=4096, W=4096) == ERR_SHAPE                 # 2^31 input elements: offsets are 32-bit
    assert call(name, n_img=1, H=1 << 23, W=1, Cin=32, Cout=1024, cout_pad=1024, KH=1, KW=1, pad=0) == ERR_SHAPE   # M * Cout = 2^33
    stem = dict(n_img=2, H=224, W=224, Cin=4, Cout=64, KH=7, KW=7, stride=2, pad=3)
    assert call(name, **stem) > 0
    assert call(name, **{**stem, 'KW': 9}) == ERR_SHAPE                     # a stem K-tile holds 8 pixels of a filter row
    assert call(name, in_scale=P[6], **stem) == ERR_SHAPE                   # the stem kernel has no fused input scale
    assert call(name, tile_hint=5) == ERR_ARG                               # no such tile
    assert call(name, tile_hint=5, Cin=48) == ERR_SHAPE                     # the shape is judged first
    name = 'fgn_conv2d_pair_nhwc_f32'
    for t in '01':                                                          # per tensor
        assert call(name, **{'H' + t: 1, 'W' + t: 1, 'pad': 0}) == ERR_SHAPE            # no output pixel
        assert call(name, **{'n_img' + t: 1, 'H' + t: 4096, 'W' + t: 2048}) == ERR_SHAPE   # 2^31 bytes >= 0x7fffff00
        assert call(name, **{'n_img' + t: 1, 'H' + t: 4096, 'W' + t: 2047}) > 0
    assert call(name, Cout=6) == ERR_SHAPE
    assert call(name, KH=9, KW=9, pad=4) == ERR_SHAPE                       # KH * KW > 64
    name = 'fgn_conv2d_pair_h2_nhwc_f32'
    assert call(name, Cin=96) == ERR_SHAPE                  # Cin / 32 not a power of two
    assert call(name, Cin=128) > 0
    assert call(name, KH=1, KW=3) == ERR_SHAPE              # KH != KW
    assert call(name, KH=5, KW=5, pad=2) == ERR_SHAPE       # 1x1 or 3x3
    assert call(name, x1=P[0] + (1 << 31)) == ERR_SHAPE     # both tensors within one 2 GiB descriptor


# ------------------------------------------------------------------------------------------------------------------
# The plan of a direct launch: fgn_conv2d_kernel_id (tile * 10 + mode), fgn_conv2d_workspace_bytes (the split-K slabs) and
# the launch itself decide from one place.  The expectations below were read from the library BEFORE that place existed.
# ------------------------------------------------------------------------------------------------------------------
def _conv(n_img=1, H=1, W=1, Cin=64, Cout=1024, cout_pad=None, k=1, KW=None, stride=1, pad=0, a_img_div=1, in_scale=0,
          residual=0, tile_hint=0):
    """Arguments of a direct launch; the default is a point-wise launch of H rows ([1, rows, 1, Cin])."""
    return dict(n_img=n_img, H=H, W=W, Cin=Cin, Cout=Cout, cout_pad=(Cout + 127) // 128 * 128 if cout_pad is None else cout_pad,
                KH=k, KW=k if KW is None else KW, stride=stride, pad=pad, a_img_div=a_img_div, in_scale=in_scale,
                residual=residual, tile_hint=tile_hint)


def kernel_id(a):
    from fgn_amd import lib
    return lib.load().fgn_conv2d_kernel_id(a['n_img'], a['H'], a['W'], a['Cin'], a['Cout'], a['cout_pad'], a['KH'], a['KW'],
                                           a['stride'], a['pad'], a['a_img_div'], a['in_scale'], a['residual'], a['tile_hint'])


def workspace(a):
    from fgn_amd import lib
    return lib.load().fgn_conv2d_workspace_bytes(a['n_img'], a['H'], a['W'], a['Cin'], a['Cout'], a['KH'], a['KW'], a['stride'],
                                                 a['pad'], a['tile_hint'])


def launch(a):
    """fgn_conv2d_nhwc_f32 on fabricated pointers, with the workspace fgn_conv2d_workspace_bytes asks for."""
    ws = workspace(a)
    return call('fgn_conv2d_nhwc_f32', residual=P[5] if a['residual'] else None, in_scale=P[6] if a['in_scale'] else None,
                ws=P[7] if ws else None, ws_bytes=ws,
                **{k: a[k] for k in 'n_img H W Cin Cout cout_pad KH KW stride pad a_img_div tile_hint'.split()})


def _slabs(a):
    """Workspace of ``a`` in slabs of one output (M x Cout floats)."""
    ho, wo = (a['H'] + 2 * a['pad'] - a['KH']) // a['stride'] + 1, (a['W'] + 2 * a['pad'] - a['KW']) // a['stride'] + 1
    s, rem = divmod(workspace(a), a['n_img'] * ho * wo * a['Cout'] * 4)
    assert rem == 0
    return s


_W512 = dict(Cin=1024, Cout=512)                   # the 1024 -> 512 conv on RoIs: the 128x128 window
_SK = dict(Cin=1024, Cout=64)                      # 32 K-tiles, one column tile: blocks = row tiles
_SK2 = dict(Cin=2048, Cout=64)                     # 64 K-tiles
_3X3 = dict(n_img=2, H=32, W=32, Cin=64, Cout=128, k=3, pad=1)
# (arguments, kernel id, workspace in slabs)
THRESHOLDS = [
    # conv_pw_persist_kernel: more than 1024 output tiles of 64x64
    (_conv(H=4096), 41, 0), (_conv(H=4097), 44, 0), (_conv(H=4097, tile_hint=-4), 44, 0),
    (_conv(H=8194, Cout=1022), 41, 0),                                       # rows are written 16 bytes at a time
    # the 128x128 tile: 420 .. 512 tiles of 128 rows, no residual
    (_conv(H=13312, **_W512), 44, 0), (_conv(H=13313, **_W512), 11, 0), (_conv(H=16384, **_W512), 11, 0),
    (_conv(H=16385, **_W512), 44, 0), (_conv(H=13313, residual=1, **_W512), 44, 0), (_conv(H=16384, residual=1, **_W512), 44, 0),
    (_conv(H=13312, residual=1, **_W512), 44, 0),
    # split-K: 32 K-tiles below 320 workgroups, deeper below 512; never 16 K-tiles, a negative hint or another tile
    (_conv(H=319 * 64, **_SK), 41, 3), (_conv(H=320 * 64, **_SK), 41, 0), (_conv(H=100 * 64, **_SK), 41, 8),
    (_conv(H=511 * 64, **_SK2), 41, 3), (_conv(H=512 * 64, **_SK2), 41, 0), (_conv(H=3 * 64, **_SK2), 41, 16),
    (_conv(H=100 * 64, Cin=512, Cout=64), 41, 0), (_conv(H=100 * 64, tile_hint=-4, **_SK), 41, 0),
    (_conv(H=100 * 64, tile_hint=1, **_SK), 11, 0), (_conv(H=100 * 64, tile_hint=4, **_SK), 41, 8),
    (_conv(H=100 * 64, tile_hint=104, **_SK), 43, 8), (_conv(H=3 * 64, tile_hint=4, **_SK2), 41, 16),
    # the loader / addressing mode
    (_conv(n_img=2, H=224, W=224, Cin=4, Cout=64, k=7, stride=2, pad=3), 42, 0),
    (_conv(**_3X3), 40, 0), (_conv(in_scale=1, **_3X3), 43, 0), (_conv(tile_hint=100, **_3X3), 43, 0),
    (_conv(a_img_div=2, **_3X3), 40, 0), (_conv(H=4097, in_scale=1), 43, 0), (_conv(n_img=2, H=4097, a_img_div=2), 40, 0),
]


# The direct launches (ops.conv2d on the f32 kernels, and the ids ops._winograd_records asks for: tile_hint 4) of one cfg3
# episode under GEMM_MATH 'h2' and 'f32', from its ConvProfile: the arguments of fgn_conv2d_kernel_id -> (id, slabs)
CFG3 = [
    ((1, 50, 84, 1024, 512, 512, 1, 1, 1, 0, 1, 0, 0, 0), 41, 0),
    ((1, 6504, 1, 256, 1024, 1024, 1, 1, 1, 0, 1, 0, 1, 0), 44, 0),
    ((1, 6504, 1, 1024, 256, 256, 1, 1, 1, 0, 1, 0, 0, 0), 41, 0),
    ((1, 25916, 1, 128, 512, 512, 1, 1, 1, 0, 1, 0, 1, 0), 44, 0),
    ((1, 25916, 1, 512, 128, 128, 1, 1, 1, 0, 1, 0, 0, 0), 41, 0),
    ((1, 25916, 1, 512, 256, 256, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((1, 103664, 1, 64, 64, 128, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((1, 103664, 1, 64, 256, 256, 1, 1, 1, 0, 1, 0, 1, 0), 44, 0),
    ((1, 103664, 1, 256, 64, 128, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((1, 103664, 1, 256, 128, 128, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((3, 7, 7, 1024, 1024, 1024, 1, 1, 1, 0, 1, 0, 0, 0), 41, 8),
    ((3, 50, 84, 1024, 76, 128, 1, 1, 1, 0, 1, 0, 0, 0), 41, 0),
    ((9, 7, 7, 1024, 512, 512, 1, 1, 1, 0, 1, 0, 0, 0), 41, 8),
    ((100, 7, 7, 256, 1024, 1024, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((100, 7, 7, 512, 1024, 1024, 1, 1, 1, 0, 1, 0, 1, 0), 44, 0),
    ((100, 7, 7, 1024, 512, 512, 1, 1, 1, 0, 1, 0, 0, 0), 41, 0),
    ((300, 7, 7, 1024, 1024, 1024, 1, 1, 1, 0, 1, 0, 0, 0), 44, 0),
    ((309, 7, 7, 512, 1024, 1024, 1, 1, 1, 0, 1, 0, 1, 0), 44, 0),
    ((309, 7, 7, 1024, 512, 512, 1, 1, 1, 0, 1, 0, 0, 0), 11, 0),
    ((18432, 1, 1, 256, 256, 256, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
    ((18432, 1, 1, 512, 512, 512, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
    ((18432, 1, 1, 1024, 256, 256, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
    ((32256, 1, 1, 1024, 1024, 1024, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
    ((46080, 1, 1, 512, 512, 512, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
    ((59904, 1, 1, 128, 128, 128, 1, 1, 1, 0, 1, 0, 0, 4), 44, 0),
]
_KID_ARGS = 'n_img H W Cin Cout cout_pad KH KW stride pad a_img_div in_scale residual tile_hint'.split()
TABLE = THRESHOLDS + [(dict(zip(_KID_ARGS, args)), kid, slabs) for args, kid, slabs in CFG3]


@pytest.mark.parametrize('i', range(len(TABLE)))
def test_kernel_id_and_workspace_of_the_cfg3_launches_and_on_both_sides_of_every_threshold(i):
    a, kid, slabs = TABLE[i]
    assert launch(a) > 0                                    # a launch the library accepts
    assert kernel_id(a) == kid
    assert _slabs(a) == slabs


def _grid():
    """Point-wise launches whose row counts, depths and widths cross every threshold of THRESHOLDS, in every form of the
    hint, with and without what changes the kernel; 3x3 / 7x7 / strided geometries; and what the launch refuses."""
    rows = (1, 64, 192, 4096, 4097, 6400, 13312, 13313, 16384, 16385, 20416, 20480, 32704, 32768, 65537)
    for h in rows:
        for cin in (32, 64, 512, 1024, 2048):
            for cout in (64, 512, 1022, 1024):
                for hint in (0, 1, 2, 3, 4, -4, -1, 100, 104, 5, 105, -5):
                    for residual, in_scale, div in ((0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 2), (1, 1, 2)):
                        yield _conv(n_img=div, H=h, Cin=cin, Cout=cout, tile_hint=hint, residual=residual, in_scale=in_scale,
                                    a_img_div=div)
    for k, stride in ((3, 1), (3, 2), (7, 2), (1, 2)):
        for cin in (4, 32, 256, 1056):
            for n, hw in ((1, 7), (9, 32), (2, 224), (300, 7)):
                for cout in (64, 75, 512):
                    for hint in (0, 4, -4, 100, 5):
                        for in_scale in (0, 1):
                            yield _conv(n_img=n, H=hw, W=hw, Cin=cin, Cout=cout, k=k, stride=stride, pad=k // 2,
                                        tile_hint=hint, in_scale=in_scale)
    stem = dict(n_img=2, H=224, W=224, Cin=4, Cout=64, k=7, stride=2, pad=3)
    yield _conv(**{**stem, 'KW': 9})
    yield _conv(**{**stem, 'in_scale': 1})
    yield _conv(**{**stem, 'tile_hint': 5})
    yield _conv(**{**stem, 'tile_hint': 100})                               # the stem stays on its LDS-DMA kernel
    yield _conv(**{**stem, 'n_img': 1, 'H': 16384, 'W': 8192})              # Cin 4 beyond the 2 GiB of a buffer descriptor
    yield _conv(n_img=2, H=4096, W=4096, Cin=64, Cout=128, k=3, pad=1)      # 2^31 input elements
    yield _conv(n_img=1, H=8192, W=1024, Cin=64, Cout=128, k=3, pad=1)      # input of 2^31 bytes: register-staged
    yield _conv(H=1 << 23, Cin=32, Cout=1024)                               # M * Cout = 2^33
    yield _conv(Cin=48, tile_hint=5)
    yield _conv(**{**_3X3, 'k': 9, 'pad': 4})
    yield _conv(**{**_3X3, 'pad': 0, 'H': 1})
    yield _conv(**{**_3X3, 'cout_pad': 100})
    yield _conv(**{**_3X3, 'a_img_div': 0})


def test_kernel_id_names_a_kernel_or_gives_the_code_the_launch_refuses_with():
    """Whatever fgn_conv2d_nhwc_f32 refuses on shape or hint, fgn_conv2d_kernel_id refuses with the same code; whatever
    gets as far as the launch (no device here: a positive hipError_t) has an id that names a kernel."""
    from fgn_amd import ops
    refused = 0
    for a in _grid():
        rc, kid = launch(a), kernel_id(a)
        if rc < 0:
            refused += 1
            assert kid == rc, (a, rc, kid)
        else:
            assert rc > 0 and kid > 0 and ops.kernel_name(kid), (a, rc, kid)
    assert refused > 1000


def test_persistent_launches_take_no_workspace_and_a_workspace_is_whole_slabs():
    """conv_pw_persist_kernel has no split-K form: id mode 4 implies no workspace; a workspace is 2 .. 16 slabs of the
    output (M x Cout floats)."""
    split = persistent = 0
    for a in _grid():
        kid, ws = kernel_id(a), workspace(a)
        if kid > 0 and kid % 10 == 4:
            persistent += 1
            assert ws == 0, a
        if ws:
            split += 1
            assert kid > 0 and 2 <= _slabs(a) <= 16, a
    assert split > 100 and persistent > 100
