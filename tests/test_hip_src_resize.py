"""The two query-resize kernels on the GPU against the host restatement of ``fgn_amd.fewshot_ds`` - bit for bit:
``resize_u8hwc3_to_nhwc4_kernel`` = ``u8hwc3_to_nhwc4(resize_image_u8(...))``, ``resize_mask_u8_kernel`` =
``resize_masks``; slots that are not dword-aligned, several source sizes in one launch, guard regions, refused sizes
and the return codes of both entries."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

CH = np.arange(3)
# a clearly different table per channel (a channel mix-up cannot cancel)
LUT = ops.input_lut((0.11, 0.52, 0.93), (0.21, 0.34, 0.47))

# source -> destination; 2x2 -> 300x300: every tap is clamped or inside one pixel pair; 5x3000 -> 8x4099: several
# 64-pixel chunks per row and a tail; 1x16384 -> 1x16383: the largest dimensions the int32 rule admits
CASES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((2, 2), (1, 1)), ((3, 5), (3, 5)), ((7, 9), (16, 12)),
         ((37, 53), (64, 91)), ((150, 131), (128, 128)), ((64, 160), (128, 128)), ((2, 2), (300, 300)),
         ((1, 16384), (1, 16383)), ((5, 3000), (8, 4099))]
SMALL = CASES[:9]


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _pixels(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)


def _want(imgs, H, W, lut=LUT) -> torch.Tensor:
    """Host resize, then the existing uint8 kernel."""
    x = np.stack([fd.resize_image_u8(im, H, W) for im in imgs])
    return ops.u8hwc3_to_nhwc4(torch.from_numpy(x).cuda(), torch.from_numpy(lut).cuda())


def _slots(imgs, stride, lead=0, fill=0xFF):
    """The images at the start of consecutive slots of ``stride`` bytes, ``lead`` bytes into a buffer of ``fill``."""
    buf = torch.full((lead + stride * len(imgs) + 16,), fill, dtype=torch.uint8)
    for i, im in enumerate(imgs):
        buf[lead + i * stride: lead + i * stride + im.size] = torch.from_numpy(im.reshape(-1))
    dev = buf.cuda()
    return dev, dev[lead: lead + stride * len(imgs)].view(len(imgs), stride)


@pytest.mark.parametrize('src,dst', CASES)
def test_image_kernel_is_bitwise_the_host_resize(src, dst):
    img = _pixels(src, src[0] * 7 + dst[1])
    _, slot = _slots([img], img.size)
    hw = torch.tensor([src], dtype=torch.int32).cuda()
    got = ops.resize_u8_to_nhwc4(slot, hw, torch.from_numpy(LUT).cuda(), *dst)
    want = _want([img], *dst)
    assert got.shape == want.shape == (1,) + dst + (4,) and got.dtype == torch.float32
    assert torch.equal(_ibits(got), _ibits(want))
    assert int(_ibits(got[..., 3]).abs().max()) == 0                                # +0.0, not -0.0


def test_three_source_sizes_in_one_launch_of_unaligned_slots():
    """Slots of an odd stride behind an odd offset: no slot base is dword-aligned; what lies behind each image in its
    slot is 0xFF and must not show; the guard bytes around the slots and the zeros behind y stay as they are."""
    sizes = [(37, 53), (20, 61), (5, 9)]
    imgs = [_pixels(s, 11 + i) for i, s in enumerate(sizes)]
    stride, lead, H, W = 37 * 53 * 3 + 6, 1, 33, 47          # 5889: odd
    buf, slot = _slots(imgs, stride, lead)
    assert all((slot.data_ptr() + i * stride) % 4 for i in range(3)) and slot.is_contiguous()
    before = buf.clone()
    hw = torch.tensor(sizes, dtype=torch.int32).cuda()
    n_out = 3 * H * W * 4
    ybuf = torch.zeros(n_out + 64, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(LUT).cuda()
    rc = lib.load().fgn_resize_u8hwc3_to_nhwc4_f32(slot.data_ptr(), stride, hw.data_ptr(), lut.data_ptr(), ybuf.data_ptr(),
                                                   3, H, W, st)
    assert rc == 0
    torch.cuda.synchronize()
    got = ybuf[:n_out].view(3, H, W, 4)
    assert torch.equal(_ibits(got), _ibits(_want(imgs, H, W)))
    assert int(_ibits(ybuf[n_out:]).abs().max()) == 0                               # nothing behind y
    assert torch.equal(buf, before)                                                 # the source is only read
    assert torch.equal(_ibits(ops.resize_u8_to_nhwc4(slot, hw, lut, H, W)), _ibits(got))       # the wrapper, same view


def test_a_refused_size_comes_out_as_zeros_and_is_not_read():
    """``src_hw`` of 0x0, a negative size, one above 16384 and one that exceeds its slot: all +0.0; the image between
    them is resized as usual."""
    good = _pixels((6, 7), 3)
    stride = good.size
    _, slot = _slots([good] * 5, stride, fill=0x55)
    hw = torch.tensor([[0, 0], [6, 7], [-3, 7], [1, 16385], [6, 8]], dtype=torch.int32).cuda()
    got = ops.resize_u8_to_nhwc4(slot.contiguous(), hw, torch.from_numpy(LUT).cuda(), 9, 10)
    assert torch.equal(_ibits(got[1]), _ibits(_want([good], 9, 10)[0]))
    for i in (0, 2, 3, 4):
        assert int(_ibits(got[i]).abs().max()) == 0, i


def test_image_entry_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(LUT).cuda()
    src = torch.zeros(64, dtype=torch.uint8, device='cuda')
    hw = torch.tensor([[2, 2]], dtype=torch.int32).cuda()
    y = torch.zeros(256, dtype=torch.float32, device='cuda')
    p = (src.data_ptr(), 64, hw.data_ptr(), lut.data_ptr(), y.data_ptr())
    f = L.fgn_resize_u8hwc3_to_nhwc4_f32
    for i in (0, 2, 3, 4):                                                          # each pointer null in turn
        assert f(*[None if j == i else v for j, v in enumerate(p)], 1, 2, 2, st) == -2
    for dims in ((-1, 2, 2), (1, -2, 2), (1, 2, -2), (1, 16385, 2), (1, 2, 16385)):
        assert f(*p, *dims, st) == -1
    assert f(p[0], -1, *p[2:], 1, 2, 2, st) == -1                                   # negative stride
    for dims in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):                                  # empty: no launch
        assert f(*p, *dims, st) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0
    assert tuple(ops.resize_u8_to_nhwc4(src.view(1, 64)[:0], hw[:0], lut, 4, 5).shape) == (0, 4, 5, 4)
    assert tuple(ops.resize_u8_to_nhwc4(src.view(1, 64), hw, lut, 0, 5).shape) == (1, 0, 5, 4)
    with pytest.raises(lib.FgnHipError):
        ops.resize_u8_to_nhwc4(src.view(1, 64), hw, lut, 4, 16385)
    with pytest.raises(lib.FgnHipError):
        ops.resize_u8_to_nhwc4(src.view(1, 64), hw.long(), lut, 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.resize_u8_to_nhwc4(src.view(1, 64), hw, lut[:, :255].contiguous(), 4, 4)


# ------------------------------------------------------------------------------------------------ masks
def _masks(G, hw, seed):
    return np.random.RandomState(seed).rand(G, *hw) > 0.5


@pytest.mark.parametrize('G', [0, 1, 3])
@pytest.mark.parametrize('src,dst', SMALL + [((9, 300), (5, 519))])
def test_mask_kernel_is_bitwise_the_host_resize(src, dst, G):
    """W of 1, 7, 5, 12, 91, 128, 300, 519: multiples of 4 and not, rows that start at every dword offset, a row of more
    than one 256-pixel chunk (519)."""
    m = _masks(G, src, G * 100 + src[1] + dst[0])
    want = fd.resize_masks(m, *dst)
    got = ops.resize_masks(torch.from_numpy(m).cuda(), *dst)                        # bool input
    assert got.dtype == torch.uint8 and tuple(got.shape) == (G,) + dst
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8))                 # 0 / 1 bytes
    # uint8 input with nonzero bytes other than 1
    m8 = (m * np.random.RandomState(1).randint(1, 256, m.shape)).astype(np.uint8)
    assert ((m8 != 0) == m).all()
    got8 = ops.resize_masks(torch.from_numpy(m8).cuda(), *dst)
    assert torch.equal(got8, got)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_mask_kernel_writes_only_its_output(offset):
    """dst at every byte offset of a dword inside a buffer of 7s: the dword stores stay aligned and inside."""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    G, (h, w), (H, W) = 2, (7, 9), (11, 13)
    m = _masks(G, (h, w), offset)
    src = torch.from_numpy(m).cuda()
    buf = torch.full((G * H * W + 16,), 7, dtype=torch.uint8, device='cuda')
    dst = buf[offset: offset + G * H * W]
    assert dst.data_ptr() % 4 == offset
    assert L.fgn_resize_mask_u8(src.data_ptr(), dst.data_ptr(), G, h, w, H, W, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(G, H, W), fd.resize_masks(m, H, W).astype(np.uint8))
    assert int((buf[:offset] != 7).sum()) == 0 and int((buf[offset + G * H * W:] != 7).sum()) == 0


def test_mask_entry_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    src = torch.ones(64, dtype=torch.uint8, device='cuda')
    dst = torch.zeros(64, dtype=torch.uint8, device='cuda')
    f = L.fgn_resize_mask_u8
    assert f(None, dst.data_ptr(), 1, 2, 2, 2, 2, st) == -2
    assert f(src.data_ptr(), None, 1, 2, 2, 2, 2, st) == -2
    for dims in ((-1, 2, 2, 2, 2), (1, -2, 2, 2, 2), (1, 2, -2, 2, 2), (1, 2, 2, -2, 2), (1, 2, 2, 2, -2),
                 (1, 16385, 2, 2, 2), (1, 2, 16385, 2, 2), (1, 2, 2, 16385, 2), (1, 2, 2, 2, 16385), (1, 0, 2, 2, 2)):
        assert f(src.data_ptr(), dst.data_ptr(), *dims, st) == -1, dims
    for dims in ((0, 2, 2, 2, 2), (1, 2, 2, 0, 2), (1, 2, 2, 2, 0)):                # empty: no launch
        assert f(src.data_ptr(), dst.data_ptr(), *dims, st) == 0
    torch.cuda.synchronize()
    assert int(dst.max()) == 0
    with pytest.raises(lib.FgnHipError):
        ops.resize_masks(torch.zeros((1, 2, 2), dtype=torch.float32, device='cuda'), 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.resize_masks(torch.zeros((2, 2), dtype=torch.bool, device='cuda'), 4, 4)
