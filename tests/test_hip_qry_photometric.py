"""``photometric_u8hwc3_kernel`` on the GPU against the host rule ``fewshot_ds.photometric_image_u8`` - bit for bit:
every operator on shapes at the tile and dword edges and with an axis shorter than the blur's radius, several images of
different sizes and operators in one launch of slots that are not dword-aligned, guard bytes, refused records and the
return codes of the entry."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

ROWS = {'neutral': (0, 0, 0), 'noise1': (1, 1.0, 1234), 'noise2': (1, 2.0, 2 ** 32 - 1), 'impulse': (2, 0.03, 77),
        'impulse_all': (2, 1.0, 5), 'blur0.4': (3, 0.4, 0), 'blur3': (3, 3.0, 0), 'hue': (4, -37.5, 0),
        'saturation': (5, 60.25, 0), 'saturation-': (5, -75, 0), 'brightness': (6, 30, 0), 'brightness-': (6, -100.5, 0)}
SHAPES = [(1, 1), (2, 3), (3, 40), (37, 53), (64, 65), (129, 127), (5, 3000)]
FILL = 0xA5


def _pixels(hw, seed):
    img = np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)
    img.reshape(-1, 3)[::7] = (0, 255, 255)                      # saturated pixels and both clip ends among the noise
    img.reshape(-1, 3)[3::11] = 128                              # greys: no hue
    return img


def _slots(imgs, stride, lead=0, fill=FILL):
    """The images at the start of consecutive slots of ``stride`` bytes, ``lead`` bytes into a buffer of ``fill``."""
    buf = torch.full((lead + stride * len(imgs) + 16,), fill, dtype=torch.uint8)
    for i, im in enumerate(imgs):
        buf[lead + i * stride: lead + i * stride + im.size] = torch.from_numpy(im.reshape(-1))
    dev = buf.cuda()
    return dev, dev[lead: lead + stride * len(imgs)].view(len(imgs), stride)


def _run(img, rec):
    _, slot = _slots([img], img.size)
    out = ops.photometric_u8(slot, torch.from_numpy(rec[None]).cuda())
    assert out.shape == slot.shape and out.dtype == torch.uint8 and out.data_ptr() != slot.data_ptr()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize('hw', SHAPES)
@pytest.mark.parametrize('name', ROWS)
def test_kernel_is_bitwise_the_host_rule(hw, name):
    img = _pixels(hw, hw[0] * 5 + hw[1])
    rec = fd.query_photometric_record(ROWS[name], hw, hw)
    assert (rec[2] == 0) == (name == 'neutral')
    assert np.array_equal(_run(img, rec), fd.photometric_image_u8(img, rec))


@pytest.mark.parametrize('hw', SHAPES)
def test_blur_with_a_size_ratio_that_gives_radius_16(hw):
    """sigma 10.6 network pixels at 1/2 source pixel per network pixel on x and 1/3 on y: 5.3 and 3.53 source pixels,
    radius 16 - the largest - and 11."""
    rec = fd.query_photometric_record((3, 10.6, 0), hw, (3 * hw[0], 2 * hw[1]))
    assert rec[6] == 16 and rec[7] == 11
    img = _pixels(hw, 3)
    assert np.array_equal(_run(img, rec), fd.photometric_image_u8(img, rec))


def test_three_images_of_different_sizes_and_operators_in_one_launch_of_unaligned_slots():
    """Slots of an odd stride behind an odd offset: no slot base is dword-aligned in either buffer.  The bytes behind
    each image in its slot and the guard bytes around the slots of the destination stay as they were; the source is only
    read."""
    sizes = [(37, 53), (20, 61), (5, 9)]
    rows = [(3, 2.0, 0), (1, 2.0, 99), (4, 50, 0)]
    imgs = [_pixels(s, 11 + i) for i, s in enumerate(sizes)]
    stride, lead = 37 * 53 * 3 + 6, 1                        # 5889: odd
    recs = np.stack([fd.query_photometric_record(r, s, s) for r, s in zip(rows, sizes)])
    buf, slot = _slots(imgs, stride, lead)
    dbuf = torch.full((lead + stride * 3 + 16,), 0x5A, dtype=torch.uint8).cuda()
    dst = dbuf[lead: lead + stride * 3].view(3, stride)
    assert all((slot.data_ptr() + i * stride) % 4 and (dst.data_ptr() + i * stride) % 4 for i in range(3))
    before = buf.clone()
    drec = torch.from_numpy(recs).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.load().fgn_photometric_u8hwc3(slot.data_ptr(), dst.data_ptr(), stride, drec.data_ptr(), 3, st)
    assert rc == 0
    torch.cuda.synchronize()
    got = dbuf.cpu().numpy()
    want = np.full_like(got, 0x5A)
    for i, (im, r) in enumerate(zip(imgs, recs)):
        want[lead + i * stride: lead + i * stride + im.size] = fd.photometric_image_u8(im, r).reshape(-1)
    assert np.array_equal(got, want)                                                # images, slot tails and guards
    assert torch.equal(buf, before)
    # the wrapper on the same view
    out = ops.photometric_u8(slot, drec).cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i, :im.size], want[lead + i * stride: lead + i * stride + im.size])
    # aligned slots (stride a multiple of 4, offset 0): the dword path of the point operators
    buf4, slot4 = _slots(imgs, stride + 3, 0)
    assert all((slot4.data_ptr() + i * (stride + 3)) % 4 == 0 for i in range(3))
    out4 = ops.photometric_u8(slot4, drec).cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(out4[i, :im.size], want[lead + i * stride: lead + i * stride + im.size])


def test_a_refused_record_or_size_is_written_as_zeros_and_the_others_stay_intact():
    """Sizes of 0, negative, above 16384 or beyond the slot; an operator, radius, weight sum or amount outside its set:
    the whole slot is zeros; the images between them as usual.  A refused image's source bytes do not matter."""
    hw = (6, 7)
    good = _pixels(hw, 3)
    blur = fd.query_photometric_record((3, 1.0, 0), hw, hw)
    hue = fd.query_photometric_record((4, 50, 0), hw, hw)

    def mod(rec, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[fd.PHOTO_REC_HEADER.index(k) if k in fd.PHOTO_REC_HEADER else int(k[1:])] = v
        return r
    refused = [mod(hue, h=0), mod(hue, w=-3), mod(hue, h=fd.RESIZE_MAX_DIM + 1), mod(hue, h=7),      # 7*7*3 > the slot
               mod(hue, operator=7), mod(hue, operator=-1), mod(hue, a0=6 << 16), mod(hue, a0=-1),
               mod(blur, rx=0), mod(blur, ry=17), mod(blur, rx=-2), mod(blur, i8=int(blur[8]) + 2),
               mod(blur, i26=-1, i25=int(blur[25]) + 2), mod(hue, operator=5, a0=(1 << 23) + 1),
               mod(hue, operator=6, a0=-(255 << 7) - 1), mod(hue, operator=2, a0=1, a1=1), mod(hue, operator=2, a1=2)]
    recs = []
    for r in refused:
        recs += [blur, r, hue]
    recs = np.stack(recs)
    n = len(recs)
    _, slot = _slots([good] * n, good.size)
    out = ops.photometric_u8(slot, torch.from_numpy(recs).cuda()).cpu().numpy()
    want = {0: fd.photometric_image_u8(good, blur).reshape(-1), 2: fd.photometric_image_u8(good, hue).reshape(-1)}
    for i in range(n):
        if i % 3 == 1:
            assert not out[i].any(), i
        else:
            assert np.array_equal(out[i], want[i % 3]), i
    for j, r in enumerate(refused):                             # the host rule refuses the same records
        if j != 3:                                              # (all but the one that only its slot is too small for)
            with pytest.raises(ValueError):
                fd._photo_fields(r)


def test_return_codes():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    img = _pixels((6, 7), 1)
    _, slot = _slots([img], img.size)
    dst = torch.empty_like(slot)
    rec = torch.from_numpy(fd.query_photometric_record((3, 1.0, 0), (6, 7), (6, 7))[None]).cuda()
    s, d, r, n = slot.data_ptr(), dst.data_ptr(), rec.data_ptr(), img.size
    assert L.fgn_photometric_u8hwc3(s, d, n, r, 1, st) == 0
    assert L.fgn_photometric_u8hwc3(s, s, n, r, 1, st) == -2                        # in place: the blur reads neighbours
    two = torch.empty(2 * n + 8, dtype=torch.uint8, device='cuda')
    assert L.fgn_photometric_u8hwc3(two.data_ptr(), two.data_ptr() + n - 1, n, r, 1, st) == -2      # overlapping slots
    assert L.fgn_photometric_u8hwc3(two.data_ptr(), two.data_ptr() + n, n, r, 1, st) == 0           # adjacent ones
    for args in ((None, d, n, r, 1), (s, None, n, r, 1), (s, d, n, None, 1)):
        assert L.fgn_photometric_u8hwc3(*args, st) == -2
    assert L.fgn_photometric_u8hwc3(s, d, n, r, 0, st) == 0                         # nothing to do
    assert L.fgn_photometric_u8hwc3(s, d, n, r, -1, st) == -1
    assert L.fgn_photometric_u8hwc3(s, d, -1, r, 1, st) == -1
    torch.cuda.synchronize()
    with pytest.raises(lib.FgnHipError):
        ops.photometric_u8(slot, rec.reshape(-1))
    with pytest.raises(lib.FgnHipError):
        ops.photometric_u8(slot, rec[:, :16].contiguous())
    assert ops.photometric_u8(slot[:0], rec[:0]).shape == (0, n)
