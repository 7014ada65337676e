"""The narrow (32-bit offset) instances of the F(4x4) Winograd transforms against the wide (64-bit index) ones, byte for
byte, through the entry points that force the instance (ops.winograd4_input / winograd4_output, index_bits 32 / 64); and the
launcher's choice between them from the sizes alone."""
import pytest
import torch

_MAPS = [(7, 7), (10, 13), (16, 16)]       # two partial tiles per axis / partial on both axes / no partial tile
_FILL = 12345.5                            # what buffers hold before a launch: untouched bytes must survive


def _t_pad(tiles):
    from fgn_amd import lib
    return lib.load().fgn_winograd_t_pad(tiles)


def _tiles(h, w):
    return ((h + 3) // 4) * ((w + 3) // 4)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rand(*shape, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(*shape, generator=g, device='cuda')


def _input_pair(x, t_pad, **kw):
    """V of the wide and of the narrow instance, both over a pre-filled buffer"""
    from fgn_amd import ops
    out = []
    for bits in (64, 32):
        V = torch.full((36, t_pad, x.shape[3]), _FILL, device='cuda')
        ops.winograd4_input(x, V, index_bits=bits, **kw)
        out.append(V)
    torch.cuda.synchronize()
    return out


def _output_pair(Mo, shape, y1_shape=None, **kw):
    from fgn_amd import ops
    out = []
    for bits in (64, 32):
        y = torch.full(shape, _FILL, device='cuda')
        y1 = None if y1_shape is None else torch.full(y1_shape, _FILL, device='cuda')
        ops.winograd4_output(Mo, y, y1=y1, index_bits=bits, **kw)
        out.append((y, y1))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('c', [128, 256, 96])          # 96: 48 channel vectors, no power of two
@pytest.mark.parametrize('h,w', _MAPS)
def test_input_narrow_equals_wide(h, w, c):
    n = 3
    x = _rand(n, h, w, c, seed=h * w + c)
    t_pad = _t_pad(n * _tiles(h, w))
    wide, narrow = _input_pair(x, t_pad)
    assert _same(wide, narrow)
    assert not (wide[:, :n * _tiles(h, w)] == _FILL).any()          # every valid tile was written
    assert (narrow[:, n * _tiles(h, w):] == _FILL).all()            # and nothing behind them


@pytest.mark.gpu
@pytest.mark.parametrize('c', [128, 256, 96])
@pytest.mark.parametrize('h,w', _MAPS)
@pytest.mark.parametrize('relu', [False, True])
def test_output_narrow_equals_wide(h, w, c, relu):
    n = 3
    t_pad = _t_pad(n * _tiles(h, w))
    Mo = _rand(36, t_pad, c, seed=h + w + c)
    shift = _rand(c, seed=7)
    (yw, _), (yn, _) = _output_pair(Mo, (n, h, w, c), shift=shift, relu=relu)
    assert _same(yw, yn)
    assert not (yn == _FILL).any()
    (yw, _), (yn, _) = _output_pair(Mo, (n, h, w, c))                # no shift
    assert _same(yw, yn)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', _MAPS)
def test_guided_input(h, w):
    """three logical images per map, each with its own channel scale (no power of two: the product rounds)"""
    n_in, div, c = 2, 3, 128
    x = _rand(n_in, h, w, c, seed=1)
    s = (_rand(n_in * div, c, seed=2) * 0.37 + 1.3).contiguous()
    t_pad = _t_pad(n_in * div * _tiles(h, w))
    wide, narrow = _input_pair(x, t_pad, in_scale=s, a_img_div=div)
    assert _same(wide, narrow)
    plain = _input_pair(x, _t_pad(n_in * _tiles(h, w)))[1]
    assert not _same(plain[:, :_tiles(h, w)], narrow[:, :_tiles(h, w)])   # the scale was applied


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', _MAPS)
@pytest.mark.parametrize('guided', [False, True])
def test_device_count_below_capacity(h, w, guided):
    """count 5 of 9 images: the rows past the count keep their bytes in V (the tiles of whole images) and in y"""
    cap, cnt, c = 9, 5, 128
    div = 3 if guided else 1
    x = _rand(cap // div, h, w, c, seed=3)
    s = (_rand(cap, c, seed=4) * 0.37 + 1.3).contiguous() if guided else None
    n_dev = torch.tensor([cnt], dtype=torch.int32, device='cuda')
    tiles = _tiles(h, w)
    t_pad = _t_pad(cap * tiles)
    wide, narrow = _input_pair(x, t_pad, in_scale=s, a_img_div=div, n_img_dev=n_dev)
    assert _same(wide, narrow)
    assert (narrow[:, cnt * tiles:] == _FILL).all() and not (narrow[:, :cnt * tiles] == _FILL).any()
    full = _input_pair(x, t_pad, in_scale=s, a_img_div=div)[1]
    assert _same(full[:, :cnt * tiles], narrow[:, :cnt * tiles])

    Mo = _rand(36, t_pad, c, seed=5)
    shift = _rand(c, seed=6)
    (yw, _), (yn, _) = _output_pair(Mo, (cap, h, w, c), shift=shift, relu=True, n_img_dev=n_dev)
    assert _same(yw, yn)
    assert (yn[cnt:] == _FILL).all() and not (yn[:cnt] == _FILL).any()
    # a count past the capacity is the capacity
    n_big = torch.tensor([cap + 4], dtype=torch.int32, device='cuda')
    (yw, _), (yn, _) = _output_pair(Mo, (cap, h, w, c), shift=shift, relu=True, n_img_dev=n_big)
    assert _same(yw, yn) and not (yn == _FILL).any()


@pytest.mark.gpu
@pytest.mark.parametrize('c', [128, 96])
def test_two_tensor_form(c):
    """a 1 x 10 x 13 map followed by nine 8 x 8 maps in one launch"""
    from fgn_amd import ops
    x0, x1 = _rand(1, 10, 13, c, seed=8), _rand(9, 8, 8, c, seed=9)
    t0, t1 = _tiles(10, 13), 9 * _tiles(8, 8)
    t_pad = _t_pad(t0 + t1)
    wide, narrow = _input_pair(x0, t_pad, x1=x1)
    assert _same(wide, narrow)
    assert not (narrow[:, :t0 + t1] == _FILL).any() and (narrow[:, t0 + t1:] == _FILL).all()
    # each range is the transform of its tensor alone
    alone = torch.full((36, t_pad, c), _FILL, device='cuda')
    ops.winograd4_input(x1, alone, index_bits=32)
    assert _same(alone[:, :t1], narrow[:, t0:t0 + t1])

    Mo = _rand(36, t_pad, c, seed=10)
    shift = _rand(c, seed=11)
    (yw0, yw1), (yn0, yn1) = _output_pair(Mo, (1, 10, 13, c), (9, 8, 8, c), shift=shift, relu=True)
    assert _same(yw0, yn0) and _same(yw1, yn1)
    assert not (yn0 == _FILL).any() and not (yn1 == _FILL).any()


@pytest.mark.gpu
def test_sixteen_byte_vectors():
    """the smallest launch the width rule gives 16-byte vectors (4 Mi (tile, channel) pairs): 4096 maps of 7 x 7 x 256"""
    from fgn_amd import lib
    n, h, w, c = 4096, 7, 7, 256
    assert lib.load().fgn_winograd4_variant(n * _tiles(h, w), c, 0) // 10 == 4
    assert lib.load().fgn_winograd4_variant(n * _tiles(h, w) - 1, c, 0) // 10 == 2
    x = _rand(n, h, w, c, seed=12)
    t_pad = _t_pad(n * _tiles(h, w))
    wide, narrow = _input_pair(x, t_pad)
    assert _same(wide, narrow)
    del wide
    (yw, _), (yn, _) = _output_pair(narrow, (n, h, w, c), shift=_rand(c, seed=13), relu=True)
    assert _same(yw, yn)


def test_launcher_picks_the_wide_instance_past_31_bits():
    """from the sizes alone: nothing is allocated or launched"""
    from fgn_amd import ops
    # every layer of cfg3: narrow
    for n, h, w, c, div in ((1, 50, 84, 1024, 3), (300, 7, 7, 512, 1), (1, 100, 167, 128, 1), (8, 200, 334, 64, 1)):
        t_pad = _t_pad(n * div * _tiles(h, w))
        assert ops.winograd4_index_bits(n * div, h, w, c, t_pad, a_img_div=div, with_scale=div > 1) == 32
    # V / Mo [36][t_pad][C] reach 2 GiB: 36 * 14592 * 1024 * 4 bytes
    assert ops.winograd4_index_bits(1, 480, 480, 1024, 14592) == 64
    assert ops.winograd4_index_bits(1, 480, 480, 1024, 14400) == 32
    # x itself: 2200 * 50 * 84 * 64 * 4 bytes
    assert ops.winograd4_index_bits(2200, 50, 84, 64, 1 << 14) == 64
    assert ops.winograd4_index_bits(2200, 50, 84, 32, 1 << 14) == 32
    # the output transform has its own sizes: y of n_img images, no scale
    assert ops.winograd4_index_bits(6600, 50, 84, 32, 1 << 14, a_img_div=3) == 32          # x: 2200 images
    assert ops.winograd4_index_bits(6600, 50, 84, 32, 1 << 14, output=True) == 64          # y: 6600 images
    # the second tensor of the two-tensor form
    assert ops.winograd4_index_bits(1, 8, 8, 64, 1 << 14, second=(2200, 50, 84)) == 64
    assert ops.winograd4_index_bits(1, 8, 8, 64, 1 << 14, second=(9, 8, 8)) == 32


@pytest.mark.gpu
def test_forced_narrow_refuses_what_it_cannot_address():
    from fgn_amd import lib
    L = lib.load()
    x = torch.zeros(1, 8, 8, 1024, device='cuda')
    V = torch.zeros(4, device='cuda')              # never touched: the launcher refuses on the sizes
    rc = L.fgn_winograd4_input_ix_f32(x.data_ptr(), None, V.data_ptr(), None, 1, 1, 8, 8, 1024, 14592, None, 0, 1, 1, 32, 0, None)
    assert rc == -1
    rc = L.fgn_winograd4_output_ix_f32(V.data_ptr(), x.data_ptr(), None, None, 1, 8, 8, 1024, 14592, 0, None, 0, 1, 1, 32, 0, None)
    assert rc == -1
    assert L.fgn_winograd4_input_ix_f32(x.data_ptr(), None, V.data_ptr(), None, 1, 1, 8, 8, 1024, 64, None, 0, 1, 1, 7, 0, None) == -2
    assert L.fgn_winograd4_input_ix_f32(x.data_ptr(), None, V.data_ptr(), None, 1, 1, 8, 8, 1024, 64, None, 0, 1, 1, 0, 3, None) == -2
