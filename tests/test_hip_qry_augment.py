"""The two query-augmentation kernels on the GPU against the host rule of ``fgn_amd.fewshot_ds`` - bit for bit:
``augment_u8hwc3_to_nhwc4_kernel`` = ``u8hwc3_to_nhwc4(augment_image_u8(...))``, ``augment_mask_u8_kernel`` =
``augment_masks``; every operator, both borders, all six channel orders, slots that are not dword-aligned, several
records in one launch, guard regions, refused records and the return codes of both entries."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

# a clearly different table per channel (a channel mix-up cannot cancel)
LUT = ops.input_lut((0.11, 0.52, 0.93), (0.21, 0.34, 0.47))


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


OPERATORS = {'neutral': row(), 'flip': row(flip=1), 'rot10_sym': row(rotate=10, border=1), 'rot10_const': row(rotate=10),
             'scale0.8': row(scale=0.8), 'scale0.8_sym': row(scale=0.8, border=1), 'scale1.2': row(scale=1.2),
             'shear+10_sym': row(shear=10, border=1), 'shear-10_sym': row(shear=-10, border=1),
             'shear+10_const': row(shear=10), 'shift_const': row(tx=-20, ty=13), 'shift_sym': row(tx=-20, ty=13, border=1),
             'composed_sym': row(1, 33, 1.1, 5, 3.3, -7.7, 1, 4), 'composed_const': row(1, 33, 1.1, 5, 3.3, -7.7, 0, 3)}
SHAPES = [((7, 9), (16, 12)), ((37, 53), (64, 91)), ((150, 131), (128, 128)), ((101, 77), (128, 128)),
          ((2, 2), (300, 300)), ((1, 1), (5, 7))]
WIDE = ((5, 3000), (8, 4099))


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _pixels(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)


def _want(imgs, recs, H, W) -> torch.Tensor:
    """The host rule, then the existing uint8 kernel."""
    x = np.stack([fd.augment_image_u8(im, r, H, W) for im, r in zip(imgs, recs)])
    return ops.u8hwc3_to_nhwc4(torch.from_numpy(x).cuda(), torch.from_numpy(LUT).cuda())


def _slots(imgs, stride, lead=0, fill=0xFF):
    """The images at the start of consecutive slots of ``stride`` bytes, ``lead`` bytes into a buffer of ``fill``."""
    buf = torch.full((lead + stride * len(imgs) + 16,), fill, dtype=torch.uint8)
    for i, im in enumerate(imgs):
        buf[lead + i * stride: lead + i * stride + im.size] = torch.from_numpy(im.reshape(-1))
    dev = buf.cuda()
    return dev, dev[lead: lead + stride * len(imgs)].view(len(imgs), stride)


def _run(img, rec, dst):
    _, slot = _slots([img], img.size)
    return ops.augment_u8_to_nhwc4(slot, torch.from_numpy(rec[None]).cuda(), torch.from_numpy(LUT).cuda(), *dst)


@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('name', OPERATORS)
def test_image_kernel_is_bitwise_the_host_rule(src, dst, name):
    img = _pixels(src, src[0] * 7 + dst[1])
    rec = fd.query_augment_record(OPERATORS[name], src, dst)
    got = _run(img, rec, dst)
    want = _want([img], [rec], *dst)
    assert got.shape == want.shape == (1,) + dst + (4,) and got.dtype == torch.float32
    assert torch.equal(_ibits(got), _ibits(want))
    assert int(_ibits(got[..., 3]).abs().max()) == 0                                # +0.0, not -0.0


def test_image_kernel_on_a_wide_image_needs_its_int64_coordinates():
    """5x3000 -> 8x4099 under a rotation: the coordinate passes 2^31 units of 2^-20; several chunks per row and a tail."""
    src, dst = WIDE
    img = _pixels(src, 5)
    rec = fd.query_augment_record(OPERATORS['rot10_sym'], src, dst)
    assert abs(int(rec[6])) * 4098 > 2 ** 31
    assert torch.equal(_ibits(_run(img, rec, dst)), _ibits(_want([img], [rec], *dst)))


@pytest.mark.parametrize('order', range(6))
@pytest.mark.parametrize('params', [row(), row(flip=1), row(rotate=10, border=1), row(scale=1.2)])
def test_all_six_channel_orders(order, params):
    src, dst = (37, 53), (64, 91)
    img = _pixels(src, 9)
    p = params.copy()
    p[7] = order
    rec = fd.query_augment_record(p, src, dst)
    got = _run(img, rec, dst)
    assert torch.equal(_ibits(got), _ibits(_want([img], [rec], *dst)))
    # and by the definition: out[c] = in[order[c]] of the image without a channel order, each through table c
    base = fd.augment_image_u8(img, fd.query_augment_record(params, src, dst), *dst)
    x = np.ascontiguousarray(base[..., list(fd.CHANNEL_ORDERS[order])])
    assert torch.equal(_ibits(got), _ibits(ops.u8hwc3_to_nhwc4(torch.from_numpy(x[None]).cuda(),
                                                                 torch.from_numpy(LUT).cuda())))


def test_three_images_of_different_sizes_kinds_and_records_in_one_launch_of_unaligned_slots():
    """Slots of an odd stride behind an odd offset: no slot base is dword-aligned; what lies behind each image in its
    slot is 0xFF and must not show; the guard bytes around the slots and the zeros behind y stay as they are."""
    sizes = [(37, 53), (20, 61), (5, 9)]
    imgs = [_pixels(s, 11 + i) for i, s in enumerate(sizes)]
    stride, lead, H, W = 37 * 53 * 3 + 6, 1, 33, 47          # 5889: odd
    params = [row(flip=1, order=2), row(1, 33, 1.1, 5, 3.3, -7.7, 1, 5), row(tx=-20, ty=13)]
    recs = np.stack([fd.query_augment_record(p, s, (H, W)) for p, s in zip(params, sizes)])
    assert recs[:, 2].tolist() == [0, 1, 1]
    buf, slot = _slots(imgs, stride, lead)
    assert all((slot.data_ptr() + i * stride) % 4 for i in range(3)) and slot.is_contiguous()
    before = buf.clone()
    drec = torch.from_numpy(recs).cuda()
    n_out = 3 * H * W * 4
    ybuf = torch.zeros(n_out + 64, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(LUT).cuda()
    rc = lib.load().fgn_augment_u8hwc3_to_nhwc4_f32(slot.data_ptr(), stride, drec.data_ptr(), lut.data_ptr(),
                                                    ybuf.data_ptr(), 3, H, W, st)
    assert rc == 0
    torch.cuda.synchronize()
    got = ybuf[:n_out].view(3, H, W, 4)
    assert torch.equal(_ibits(got), _ibits(_want(imgs, recs, H, W)))
    assert int(_ibits(ybuf[n_out:]).abs().max()) == 0                               # nothing behind y
    assert torch.equal(buf, before)                                                 # the source is only read
    assert torch.equal(_ibits(ops.augment_u8_to_nhwc4(slot, drec, lut, H, W)), _ibits(got))    # the wrapper, same view


@pytest.mark.parametrize('src,dst', [((150, 131), (128, 128)), ((7, 9), (16, 12)), ((3, 5), (3, 5))])
def test_a_kind_0_record_gives_the_bytes_of_the_resize_kernel(src, dst):
    img = _pixels(src, 21)
    _, slot = _slots([img], img.size)
    lut = torch.from_numpy(LUT).cuda()
    want = ops.resize_u8_to_nhwc4(slot, torch.tensor([src], dtype=torch.int32).cuda(), lut, *dst)
    for params in (None, row(), row(border=1)):
        rec = fd.query_augment_record(params, src, dst)
        assert rec[2] == 0
        assert torch.equal(_ibits(ops.augment_u8_to_nhwc4(slot, torch.from_numpy(rec[None]).cuda(), lut, *dst)),
                           _ibits(want))
    rec = fd.query_augment_record(row(flip=1), src, dst)
    assert rec[2] == 0 and rec[3] == 1
    assert torch.equal(_ibits(ops.augment_u8_to_nhwc4(slot, torch.from_numpy(rec[None]).cuda(), lut, *dst)),
                       _ibits(torch.flip(want, dims=(2,))))                         # the resize, flipped along W


def test_a_refused_record_or_size_comes_out_as_zeros_and_is_not_read():
    """Records with a size of 0, a negative one, one above 16384, one that exceeds its slot, a kind / flip / border /
    channel order outside its set and coefficients beyond the bounds: all +0.0; the images between them as usual."""
    good = _pixels((6, 7), 3)
    H, W = 9, 10
    ok = fd.query_augment_record(row(rotate=10, border=1), (6, 7), (H, W))

    def mod(**kw):
        r = ok.copy()
        for k, v in kw.items():
            i = fd.AUG_REC_FIELDS.index(k)
            r[i] = v
        return r
    bad = [mod(h=0, w=0), mod(h=-3), mod(w=16385), mod(w=8), mod(kind=2), mod(kind=-1), mod(flip=2), mod(border=2),
           mod(perm=6), mod(perm=-1), mod(c00=(1 << 26) + 1), mod(c01=-(1 << 26) - 1), mod(c10=(1 << 26) + 1),
           mod(c11=-(1 << 26) - 1), mod(c02_lo=1, c02_hi=1 << 8), mod(c12_lo=-1, c12_hi=-(1 << 8) - 1)]
    recs = np.stack([ok] + bad + [ok])
    _, slot = _slots([good] * len(recs), good.size, fill=0x55)
    got = ops.augment_u8_to_nhwc4(slot.contiguous(), torch.from_numpy(recs).cuda(), torch.from_numpy(LUT).cuda(), H, W)
    want = _want([good], [ok], H, W)[0]
    assert torch.equal(_ibits(got[0]), _ibits(want)) and torch.equal(_ibits(got[-1]), _ibits(want))
    for i in range(1, len(recs) - 1):
        assert int(_ibits(got[i]).abs().max()) == 0, i
    # the bounds themselves are inside
    edge = mod(c00=1 << 26, c11=-(1 << 26), c02_lo=0, c02_hi=1 << 8, c12_lo=0, c12_hi=-(1 << 8))
    assert torch.equal(_ibits(_run(good, edge, (H, W))), _ibits(_want([good], [edge], H, W)))


def test_image_entry_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(LUT).cuda()
    src = torch.zeros(64, dtype=torch.uint8, device='cuda')
    rec = torch.from_numpy(fd.query_augment_record(row(flip=1), (2, 2), (2, 2))[None]).cuda()
    y = torch.zeros(256, dtype=torch.float32, device='cuda')
    p = (src.data_ptr(), 64, rec.data_ptr(), lut.data_ptr(), y.data_ptr())
    f = L.fgn_augment_u8hwc3_to_nhwc4_f32
    for i in (0, 2, 3, 4):                                                          # each pointer null in turn
        assert f(*[None if j == i else v for j, v in enumerate(p)], 1, 2, 2, st) == -2
    for dims in ((-1, 2, 2), (1, -2, 2), (1, 2, -2), (1, 16385, 2), (1, 2, 16385)):
        assert f(*p, *dims, st) == -1
    assert f(p[0], -1, *p[2:], 1, 2, 2, st) == -1                                   # negative stride
    for dims in ((0, 2, 2), (1, 0, 2), (1, 2, 0)):                                  # empty: no launch
        assert f(*p, *dims, st) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0
    assert tuple(ops.augment_u8_to_nhwc4(src.view(1, 64)[:0], rec[:0], lut, 4, 5).shape) == (0, 4, 5, 4)
    assert tuple(ops.augment_u8_to_nhwc4(src.view(1, 64), rec, lut, 0, 5).shape) == (1, 0, 5, 4)
    with pytest.raises(lib.FgnHipError):
        ops.augment_u8_to_nhwc4(src.view(1, 64), rec, lut, 4, 16385)
    with pytest.raises(lib.FgnHipError):
        ops.augment_u8_to_nhwc4(src.view(1, 64), rec.long(), lut, 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.augment_u8_to_nhwc4(src.view(1, 64), rec[:, :15].contiguous(), lut, 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.augment_u8_to_nhwc4(src.view(1, 64), rec, lut[:, :255].contiguous(), 4, 4)


# ------------------------------------------------------------------------------------------------ masks
def _masks(G, hw, seed):
    return np.random.RandomState(seed).rand(G, *hw) > 0.5


MASK_OPS = ('neutral', 'flip', 'rot10_sym', 'scale0.8', 'shear-10_sym', 'shift_const', 'composed_sym')


@pytest.mark.parametrize('G', [0, 1, 3])
@pytest.mark.parametrize('src,dst', SHAPES + [((9, 300), (5, 519))])
def test_mask_kernel_is_bitwise_the_host_rule(src, dst, G):
    """W of 7, 12, 91, 128, 300, 519: multiples of 4 and not, rows that start at every dword offset, a row of more than
    one 256-pixel chunk (519); every operator per shape."""
    m = _masks(G, src, G * 100 + src[1] + dst[0])
    dm = torch.from_numpy(m).cuda()
    m8 = (m * np.random.RandomState(1).randint(1, 256, m.shape)).astype(np.uint8)   # nonzero bytes other than 1
    assert ((m8 != 0) == m).all()
    d8 = torch.from_numpy(m8).cuda()
    for name in MASK_OPS:
        rec = fd.query_augment_record(OPERATORS[name], src, dst)
        drec = torch.from_numpy(rec).cuda()
        want = fd.augment_masks(m, rec, *dst)
        got = ops.augment_masks(dm, drec, *dst)                                     # bool input
        assert got.dtype == torch.uint8 and tuple(got.shape) == (G,) + dst
        assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8)), name       # 0 / 1 bytes
        assert torch.equal(ops.augment_masks(d8, drec, *dst), got), name


@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('src,dst', [((7, 9), (16, 12)), ((9, 300), (5, 519)), ((3, 5), (3, 5))])
def test_a_kind_0_record_gives_the_masks_of_the_resize_kernel(src, dst, G):
    """The two mask kernels against each other, byte for byte.  W of 12, 519 and 5: a row of whole dwords, a row of more
    than one 256-pixel chunk with a ragged end, a row shorter than two dwords."""
    dm = torch.from_numpy(_masks(G, src, G * 10 + dst[1])).cuda()
    want = ops.resize_masks(dm, *dst)
    assert want.dtype == torch.uint8 and tuple(want.shape) == (G,) + dst
    for params in (None, row(), row(border=1)):
        rec = fd.query_augment_record(params, src, dst)
        assert rec[2] == 0 and rec[3] == 0
        assert torch.equal(ops.augment_masks(dm, torch.from_numpy(rec).cuda(), *dst), want)
    rec = fd.query_augment_record(row(flip=1), src, dst)
    assert rec[2] == 0 and rec[3] == 1
    assert torch.equal(ops.augment_masks(dm, torch.from_numpy(rec).cuda(), *dst), torch.flip(want, dims=(2,)))


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_mask_kernel_writes_only_its_output(offset):
    """dst at every byte offset of a dword inside a buffer of 7s: the dword stores stay aligned and inside."""
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    G, (h, w), (H, W) = 2, (7, 9), (11, 13)
    m = _masks(G, (h, w), offset)
    src = torch.from_numpy(m).cuda()
    for name in ('flip', 'composed_sym'):
        rec = fd.query_augment_record(OPERATORS[name], (h, w), (H, W))
        drec = torch.from_numpy(rec).cuda()
        buf = torch.full((G * H * W + 16,), 7, dtype=torch.uint8, device='cuda')
        dst = buf[offset: offset + G * H * W]
        assert dst.data_ptr() % 4 == offset
        assert L.fgn_augment_mask_u8(src.data_ptr(), dst.data_ptr(), drec.data_ptr(), G, h, w, H, W, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy().reshape(G, H, W), fd.augment_masks(m, rec, H, W).astype(np.uint8))
        assert int((buf[:offset] != 7).sum()) == 0 and int((buf[offset + G * H * W:] != 7).sum()) == 0


def test_mask_entry_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    src = torch.ones(64, dtype=torch.uint8, device='cuda')
    dst = torch.zeros(64, dtype=torch.uint8, device='cuda')
    rec = torch.from_numpy(fd.query_augment_record(row(flip=1), (2, 2), (2, 2))).cuda()
    f = L.fgn_augment_mask_u8
    s, d, r = src.data_ptr(), dst.data_ptr(), rec.data_ptr()
    assert f(None, d, r, 1, 2, 2, 2, 2, st) == -2
    assert f(s, None, r, 1, 2, 2, 2, 2, st) == -2
    assert f(s, d, None, 1, 2, 2, 2, 2, st) == -2
    for dims in ((-1, 2, 2, 2, 2), (1, -2, 2, 2, 2), (1, 2, -2, 2, 2), (1, 2, 2, -2, 2), (1, 2, 2, 2, -2),
                 (1, 16385, 2, 2, 2), (1, 2, 16385, 2, 2), (1, 2, 2, 16385, 2), (1, 2, 2, 2, 16385), (1, 0, 2, 2, 2)):
        assert f(s, d, r, *dims, st) == -1, dims
    for dims in ((0, 2, 2, 2, 2), (1, 2, 2, 0, 2), (1, 2, 2, 2, 0)):                # empty: no launch
        assert f(s, d, r, *dims, st) == 0
    torch.cuda.synchronize()
    assert int(dst.max()) == 0
    # a record for another source size, and one out of range: empty masks (the source is all ones)
    dst.fill_(7)
    other = torch.from_numpy(fd.query_augment_record(row(flip=1), (2, 3), (2, 2))).cuda()
    assert f(s, d, other.data_ptr(), 1, 2, 2, 2, 2, st) == 0
    torch.cuda.synchronize()
    assert dst[:4].tolist() == [0, 0, 0, 0] and int((dst[4:] != 7).sum()) == 0
    bad = rec.clone()
    bad[2] = 2
    assert int(ops.augment_masks(src[:4].view(1, 2, 2), bad, 3, 3).max()) == 0
    assert int(ops.augment_masks(src[:4].view(1, 2, 2), rec, 3, 3).min()) == 1
    with pytest.raises(lib.FgnHipError):
        ops.augment_masks(torch.zeros((1, 2, 2), dtype=torch.float32, device='cuda'), rec, 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.augment_masks(torch.zeros((2, 2), dtype=torch.bool, device='cuda'), rec, 4, 4)
    with pytest.raises(lib.FgnHipError):
        ops.augment_masks(torch.zeros((1, 2, 2), dtype=torch.bool, device='cuda'), rec[:15].contiguous(), 4, 4)
