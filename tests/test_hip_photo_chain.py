"""``photometric_chain_u8hwc3_kernel`` on the GPU against the host rule ``fewshot_ds.photometric_chain_u8`` (the left fold
of ``photometric_image_u8`` over the records) - bit for bit: point operators ahead of a blur (the noise ones catch a halo
pixel staged with the wrong counter), point operators alone, neutral records anywhere, shapes at the tile and dword
edges, several images in one launch of slots that are not dword-aligned, refused chains and the entry's return codes."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

HUE, SAT, BRI = (4, -37.5, 0), (5, 60.25, 0), (6, -100.5, 0)
GAUSS, IMPULSE, BLUR, NONE = (1, 2.0, 1234), (2, 0.3, 77), (3, 1.5, 0), (0, 0, 0)
CHAINS = {
    'hue_blur': [HUE, BLUR], 'saturation_blur': [SAT, BLUR], 'brightness_blur': [BRI, BLUR],
    'gauss_blur': [GAUSS, BLUR], 'impulse_blur': [IMPULSE, BLUR], 'gauss_hue_blur': [GAUSS, HUE, BLUR],
    'hue_brightness': [HUE, BRI], 'gauss_saturation_impulse': [GAUSS, SAT, IMPULSE],
    'neutral_neutral_blur': [NONE, NONE, BLUR], 'blur_alone': [BLUR], 'hue_alone': [HUE], 'all_neutral': [NONE, NONE],
}
SHAPES = [(1, 1), (2, 3), (3, 40), (37, 53), (64, 65), (129, 127), (5, 3000), (33, 33), (1, 70)]
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


def _run(img, recs):
    _, slot = _slots([img], img.size)
    out = ops.photometric_chain_u8(slot, torch.from_numpy(np.ascontiguousarray(recs[None])).cuda())
    assert out.shape == slot.shape and out.dtype == torch.uint8 and out.data_ptr() != slot.data_ptr()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize('hw', SHAPES)
@pytest.mark.parametrize('name', CHAINS)
def test_kernel_is_bitwise_the_fold_of_the_host_rule(hw, name):
    img = _pixels(hw, hw[0] * 5 + hw[1])
    recs = fd.photometric_chain_records(CHAINS[name], hw, hw)
    assert recs.shape == (3, 64) and int((recs[:, 2] != 0).sum()) == sum(r[0] != 0 for r in CHAINS[name])
    assert np.array_equal(_run(img, recs), fd.photometric_chain_u8(img, recs))
    n = max(1, int((recs[:, 2] != 0).sum()))                     # n_ops = the chain's own length, 1 to 3
    assert np.array_equal(_run(img, recs[:n]), fd.photometric_chain_u8(img, recs[:n]))


@pytest.mark.parametrize('hw', SHAPES)
def test_a_neutral_record_between_two_active_ones(hw):
    """Uncompacted records, as a caller of the C entry may pass them: operator 0 stands anywhere."""
    img = _pixels(hw, 9)
    rec = [fd.query_photometric_record(r, hw, hw) for r in (GAUSS, NONE, BLUR)]
    recs = np.stack(rec)
    assert recs[:, 2].tolist() == [1, 0, 3]
    assert np.array_equal(_run(img, recs), fd.photometric_chain_u8(img, recs))
    recs = np.stack([rec[0], rec[1], fd.query_photometric_record(HUE, hw, hw)])
    assert np.array_equal(_run(img, recs), fd.photometric_chain_u8(img, recs))


@pytest.mark.parametrize('hw', SHAPES)
def test_noise_then_a_blur_of_radius_16_by_11_through_a_size_ratio(hw):
    """sigma 10.6 network pixels at 1/2 source pixel per network pixel on x and 1/3 on y: radius 16 - the largest halo
    - and 11; every halo pixel carries the noise of its own source index."""
    recs = fd.photometric_chain_records([GAUSS, (3, 10.6, 0)], hw, (3 * hw[0], 2 * hw[1]))
    assert recs[1, 6] == 16 and recs[1, 7] == 11
    img = _pixels(hw, 3)
    assert np.array_equal(_run(img, recs[:2]), fd.photometric_chain_u8(img, recs[:2]))


def test_three_images_of_different_sizes_and_chains_in_one_launch_of_unaligned_slots():
    """Slots of an odd stride behind an odd offset: no slot base is dword-aligned in either buffer.  The bytes behind
    each image in its slot and the guard bytes around the slots of the destination stay as they were; the source is only
    read.  Then the same on aligned slots: the dword path of the point stages."""
    sizes = [(37, 53), (20, 61), (5, 9)]
    chains = [[GAUSS, BLUR], [HUE, BRI, IMPULSE], [SAT, (3, 0.6, 0)]]
    imgs = [_pixels(s, 11 + i) for i, s in enumerate(sizes)]
    stride, lead = 37 * 53 * 3 + 6, 1                        # 5889: odd
    recs = np.stack([fd.photometric_chain_records(c, s, s) for c, s in zip(chains, sizes)])
    buf, slot = _slots(imgs, stride, lead)
    dbuf = torch.full((lead + stride * 3 + 16,), 0x5A, dtype=torch.uint8).cuda()
    dst = dbuf[lead: lead + stride * 3].view(3, stride)
    assert all((slot.data_ptr() + i * stride) % 4 and (dst.data_ptr() + i * stride) % 4 for i in range(3))
    before = buf.clone()
    drec = torch.from_numpy(recs).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.load().fgn_photometric_chain_u8hwc3(slot.data_ptr(), dst.data_ptr(), stride, drec.data_ptr(), 3, 3, st)
    assert rc == 0
    torch.cuda.synchronize()
    got = dbuf.cpu().numpy()
    want = np.full_like(got, 0x5A)
    for i, (im, r) in enumerate(zip(imgs, recs)):
        want[lead + i * stride: lead + i * stride + im.size] = fd.photometric_chain_u8(im, r).reshape(-1)
    assert np.array_equal(got, want)                                                # images, slot tails and guards
    assert torch.equal(buf, before)
    out = ops.photometric_chain_u8(slot, drec).cpu().numpy()                        # the wrapper on the same view
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i, :im.size], want[lead + i * stride: lead + i * stride + im.size])
    buf4, slot4 = _slots(imgs, stride + 3, 0)
    assert all((slot4.data_ptr() + i * (stride + 3)) % 4 == 0 for i in range(3))
    out4 = ops.photometric_chain_u8(slot4, drec).cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(out4[i, :im.size], want[lead + i * stride: lead + i * stride + im.size])


def test_a_refused_chain_is_written_as_zeros_and_the_others_stay_intact():
    """An active record behind a blur, (h, w) differing between an image's records, an operator of 7, weights that do
    not sum to 2048, an image larger than its slot: the whole slot is zeros, the images around it as usual.  The host
    rule refuses the same chains."""
    hw = (6, 7)
    good = _pixels(hw, 3)
    rec = {k: fd.query_photometric_record(v, hw, hw) for k, v in
           dict(blur=(3, 1.0, 0), hue=HUE, none=NONE, gauss=GAUSS).items()}
    other = fd.query_photometric_record(HUE, (7, 6), (7, 6))                       # same area, another (h, w)

    def mod(r, **kw):
        r = r.copy()
        for k, v in kw.items():
            r[fd.PHOTO_REC_HEADER.index(k) if k in fd.PHOTO_REC_HEADER else int(k[1:])] = v
        return r
    big = [mod(rec['hue'], h=7), mod(rec['blur'], h=7), mod(rec['none'], h=7)]    # 7*7*3 > the slot, in every record
    refused = [[rec['blur'], rec['hue'], rec['none']], [rec['blur'], rec['none'], rec['gauss']],
               [rec['blur'], rec['blur'], rec['none']], [rec['hue'], other, rec['none']],
               [rec['hue'], rec['blur'], mod(rec['none'], w=6)], [mod(rec['hue'], operator=7), rec['blur'], rec['none']],
               [rec['hue'], mod(rec['blur'], i8=int(rec['blur'][8]) + 2), rec['none']],
               [rec['gauss'], rec['hue'], mod(rec['none'], operator=-1)], big]
    ok_a, ok_b = np.stack([rec['gauss'], rec['blur'], rec['none']]), np.stack([rec['hue'], rec['none'], rec['blur']])
    recs = []
    for r in refused:
        recs += [ok_a, np.stack(r), ok_b]
    recs = np.stack(recs)
    n = len(recs)
    _, slot = _slots([good] * n, good.size)
    out = ops.photometric_chain_u8(slot, torch.from_numpy(recs).cuda()).cpu().numpy()
    want = {0: fd.photometric_chain_u8(good, ok_a).reshape(-1), 2: fd.photometric_chain_u8(good, ok_b).reshape(-1)}
    for i in range(n):
        if i % 3 == 1:
            assert not out[i].any(), i
        else:
            assert np.array_equal(out[i], want[i % 3]), i
    for r in refused[:-1]:                                      # (all but the one that only its slot is too small for)
        with pytest.raises(ValueError):
            fd.photometric_chain_u8(np.zeros((int(r[0][0]), int(r[0][1]), 3), np.uint8), np.stack(r))


def test_return_codes():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    img = _pixels((6, 7), 1)
    _, slot = _slots([img], img.size)
    dst = torch.empty_like(slot)
    rec = torch.from_numpy(fd.photometric_chain_records([HUE, (3, 1.0, 0)], (6, 7), (6, 7))[None]).cuda()
    s, d, r, n = slot.data_ptr(), dst.data_ptr(), rec.data_ptr(), img.size
    f = L.fgn_photometric_chain_u8hwc3
    assert f(s, d, n, r, 3, 1, st) == 0
    assert f(s, s, n, r, 3, 1, st) == -2                                            # in place: the blur reads neighbours
    two = torch.empty(2 * n + 8, dtype=torch.uint8, device='cuda')
    assert f(two.data_ptr(), two.data_ptr() + n - 1, n, r, 3, 1, st) == -2          # overlapping slots
    assert f(two.data_ptr(), two.data_ptr() + n, n, r, 3, 1, st) == 0               # adjacent ones
    for args in ((None, d, n, r, 3, 1), (s, None, n, r, 3, 1), (s, d, n, None, 3, 1)):
        assert f(*args, st) == -2
    assert f(s, d, n, r, 0, 1, st) == -1 and f(s, d, n, r, 4, 1, st) == -1          # n_ops outside 1..3
    assert f(s, d, n, r, 3, 0, st) == 0                                             # nothing to do
    assert f(s, d, n, r, 3, -1, st) == -1
    assert f(s, d, -1, r, 3, 1, st) == -1
    torch.cuda.synchronize()
    with pytest.raises(lib.FgnHipError):
        ops.photometric_chain_u8(slot, rec[0])                                      # [3,64]: no image dimension
    with pytest.raises(lib.FgnHipError):
        ops.photometric_chain_u8(slot, torch.cat([rec, rec[:, :1]], 1))             # four records
    with pytest.raises(lib.FgnHipError):
        ops.photometric_chain_u8(slot, rec[:, :, :16].contiguous())
    assert ops.photometric_chain_u8(slot[:0], rec[:0]).shape == (0, n)
