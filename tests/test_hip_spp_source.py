"""``support_from_source_kernel`` on the GPU against the host restatement of ``fgn_amd.fewshot_ds`` - bit for bit: the
stem input = ``u8hwc3_to_nhwc4(support_from_source(..))`` and the mask bytes; up- and downscale, reflection over several
periods, zero mode, instances of differing sizes in unaligned slots between guard bytes, a refused record among good
ones, a grid that loops, and the return codes of the entry."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

# a clearly different table per channel (a channel mix-up cannot cancel); byte 0 maps to three different non-zero values,
# so padding written as 0.0 instead of "byte 0 through the table" shows
LUT = ops.input_lut((0.11, 0.52, 0.93), (0.21, 0.34, 0.47))


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _scene(h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.rand(h, w) > 0.4


def _instance(hw, box, S, seed, crop_square=True):
    """-> (record, image window, mask window, wanted crop [S,S,3], wanted mask [S,S])."""
    img, mask = _scene(*hw, seed)
    rec, _ = fd.support_geometry(hw[0], hw[1], box, S, crop_square=crop_square)
    crop, _, m = fd.support_from_source(img, box, mask, S, crop_square=crop_square)
    return (rec,) + fd.support_window(img, mask, rec) + (crop, m)


def _slots(wins, stride, lead, fill):
    """The windows at the start of consecutive slots of ``stride`` bytes, ``lead`` bytes into a buffer of ``fill``."""
    buf = torch.full((lead + stride * len(wins) + 16,), fill, dtype=torch.uint8)
    for i, w in enumerate(wins):
        buf[lead + i * stride: lead + i * stride + w.size] = torch.from_numpy(w.reshape(-1))
    dev = buf.cuda()
    return dev, dev[lead: lead + stride * len(wins)].view(len(wins), stride)


def _want(crops, masks):
    y = ops.u8hwc3_to_nhwc4(torch.from_numpy(np.stack(crops)).cuda(), torch.from_numpy(LUT).cuda())
    return y, torch.from_numpy(np.stack(masks).astype(np.uint8)).cuda()


def _run(insts, S, stride=None, mstride=None):
    stride = max(i[1].size for i in insts) if stride is None else stride
    mstride = max(i[2].size for i in insts) if mstride is None else mstride
    _, src = _slots([i[1] for i in insts], stride, 0, 0xFF)
    _, msk = _slots([i[2] for i in insts], mstride, 0, 0xFF)
    recs = torch.from_numpy(np.stack([i[0] for i in insts])).cuda()
    return ops.support_from_source(src.contiguous(), msk.contiguous(), recs, torch.from_numpy(LUT).cuda(), S)


# (image size, box YXYX, S): a 5x7 crop upscaled (zero offsets: extents below 9; parity pixel on both axes), a 150-pixel
# crop downscaled to 16, the 6x40 image (pads of 21 rows on 6: several reflections), a 1x1 image, boxes on the borders;
# S = 33 is no multiple of the wave's 64 pixels and gives unaligned mask rows
CASES = [((12, 14), [3, 4, 8, 11], 16), ((12, 14), [3, 4, 8, 11], 33), ((170, 180), [10, 5, 131, 126], 16),
         ((170, 180), [10, 5, 131, 126], 33), ((6, 40), [0, 0, 6, 40], 33), ((6, 40), [1, 3, 5, 38], 16),
         ((6, 40), [0, 0, 1, 1], 16), ((1, 1), [0, 0, 1, 1], 16), ((1, 1), [0, 0, 1, 1], 33),
         ((50, 60), [0, 41, 21, 60], 33), ((50, 60), [29, 0, 50, 17], 16), ((50, 60), [20, 20, 29, 60], 70)]


@pytest.mark.parametrize('crop_square', [True, False])
@pytest.mark.parametrize('hw,box,S', CASES)
def test_kernel_is_bitwise_the_host_rule(hw, box, S, crop_square):
    inst = _instance(hw, box, S, seed=hw[0] + S, crop_square=crop_square)
    y, m = _run([inst], S)
    want_y, want_m = _want([inst[3]], [inst[4]])
    assert y.shape == (1, S, S, 4) and y.dtype == torch.float32 and m.shape == (1, S, S) and m.dtype == torch.uint8
    assert torch.equal(_ibits(y), _ibits(want_y))
    assert int(_ibits(y[..., 3]).abs().max()) == 0                                  # +0.0, not -0.0
    assert torch.equal(m, want_m)
    if max(box[2] - box[0], box[3] - box[1]) >= 9 and hw != (1, 1):
        assert inst[0][10] == int(crop_square)                                      # the zero mode was really taken


def test_three_instances_of_differing_sizes_in_unaligned_slots_between_guards():
    """Slots of an odd stride behind an odd offset: no slot base is dword-aligned; what lies behind each window in its
    slot is 0xFF and must not show; the guard bytes around the slots stay as they are, and so do the guard regions
    behind y and around m (S = 33: m starts at an odd address inside its buffer)."""
    S = 33
    insts = [_instance((50, 60), [10, 0, 30, 17], S, 1), _instance((6, 40), [1, 3, 5, 38], S, 2, crop_square=False),
             _instance((170, 180), [10, 5, 131, 126], S, 3)]
    stride = max(i[1].size for i in insts) + 2
    stride += (1 - stride) % 4                                                      # 1 mod 4: slot bases at 1, 2, 3 mod 4
    mstride = max(i[2].size for i in insts) + 1
    mstride += 1 - mstride % 2
    buf, src = _slots([i[1] for i in insts], stride, 1, 0xFF)
    mbuf, msk = _slots([i[2] for i in insts], mstride, 3, 0xFF)
    assert all((src.data_ptr() + i * stride) % 4 for i in range(3)) and all((msk.data_ptr() + i * mstride) % 4 for i in (0, 2))
    before, mbefore = buf.clone(), mbuf.clone()
    recs = torch.from_numpy(np.stack([i[0] for i in insts])).cuda()
    lut = torch.from_numpy(LUT).cuda()
    n_y, n_m = 3 * S * S * 4, 3 * S * S
    ybuf = torch.zeros(n_y + 64, dtype=torch.float32, device='cuda')
    mout = torch.full((5 + n_m + 16,), 7, dtype=torch.uint8, device='cuda')
    rc = lib.load().fgn_support_from_source_f32(src.data_ptr(), stride, msk.data_ptr(), mstride, recs.data_ptr(),
                                                lut.data_ptr(), ybuf.data_ptr(), mout[5:].data_ptr(), 3, S,
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    want_y, want_m = _want([i[3] for i in insts], [i[4] for i in insts])
    assert torch.equal(_ibits(ybuf[:n_y].view(3, S, S, 4)), _ibits(want_y))
    assert torch.equal(mout[5:5 + n_m].view(3, S, S), want_m)
    assert int(_ibits(ybuf[n_y:]).abs().max()) == 0                                 # nothing behind y
    assert int((mout[:5] != 7).sum()) == 0 and int((mout[5 + n_m:] != 7).sum()) == 0      # nothing around m
    assert torch.equal(buf, before) and torch.equal(mbuf, mbefore)                  # the sources are only read
    y2, m2 = ops.support_from_source(src, msk, recs, lut, S)                        # the wrapper, same views
    assert torch.equal(_ibits(y2), _ibits(want_y)) and torch.equal(m2, want_m)


def _padding(n, S):
    lut = torch.from_numpy(LUT[:, 0].copy())
    y = torch.zeros((n, S, S, 4))
    y[..., :3] = lut
    return y.cuda()


def test_refused_records_come_out_as_padding_and_the_others_are_unaffected():
    """One field out of range per record: a size of 0 or above 16384, nh / top / left that do not fit S, a border mode of
    2, a window that leaves its image, one above its image slot, one above its mask slot; the good instances between
    them are cut as usual."""
    S = 16
    good = _instance((50, 60), [10, 0, 30, 17], S, 4)
    stride, mstride = good[1].size, good[2].size
    f = {k: i for i, k in enumerate(fd.SPP_REC_FIELDS)}
    bad = []
    for field, value in (('H', 0), ('W', 16385), ('ch', 0), ('cw', 16385), ('nh', S + 1), ('nw', 0), ('top', -1),
                         ('top', S - int(good[0][f['nh']]) + 1), ('left', S), ('reflect', 2), ('y0', -40000),
                         ('wy', -1), ('wh', 51), ('ww', 0), ('wx', 59)):
        rec = good[0].copy()
        rec[f[field]] = value
        bad.append((rec,) + good[1:])
    insts = [good] + bad + [good]
    y, m = _run(insts, S, stride, mstride)
    want_y, want_m = _want([good[3]], [good[4]])
    pad = _padding(1, S)[0]
    for i in (0, len(insts) - 1):
        assert torch.equal(_ibits(y[i]), _ibits(want_y[0])) and torch.equal(m[i], want_m[0])
    for i in range(1, len(insts) - 1):
        assert torch.equal(_ibits(y[i]), _ibits(pad)), i
        assert int(m[i].max()) == 0, i
    # a slot one byte too small for the window: image slot, then mask slot
    for st, mst in ((stride - 1, mstride), (stride, mstride - 1)):
        _, src = _slots([good[1][..., :0]] * 2, st, 0, 0x55)                      # (never read: left as fill)
        _, msk = _slots([good[2][..., :0]] * 2, mst, 0, 0x55)
        recs = torch.from_numpy(np.stack([good[0]] * 2)).cuda()
        y, m = ops.support_from_source(src.contiguous(), msk.contiguous(), recs, torch.from_numpy(LUT).cuda(), S)
        assert torch.equal(_ibits(y), _ibits(_padding(2, S))) and int(m.max()) == 0


def test_enough_instances_that_the_capped_grid_loops():
    """2048 workgroups of 4 waves take 8192 row units per pass; 530 instances at S = 16 are 8480."""
    S, n = 16, 530
    kinds = [_instance((12, 14), [3, 4, 8, 11], S, 1), _instance((6, 40), [1, 3, 5, 38], S, 2),
             _instance((50, 60), [29, 0, 50, 17], S, 3, crop_square=False)]
    insts = [kinds[(i * 7) % 3] for i in range(n)]
    assert n * S > 256 * 8 * 4
    y, m = _run(insts, S)
    want_y, want_m = _want([k[3] for k in kinds], [k[4] for k in kinds])
    order = torch.tensor([(i * 7) % 3 for i in range(n)], device='cuda')
    assert torch.equal(_ibits(y), _ibits(want_y[order])) and torch.equal(m, want_m[order])


def test_entry_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(LUT).cuda()
    good = _instance((12, 14), [3, 4, 8, 11], 4, 1)
    src = torch.zeros(256, dtype=torch.uint8, device='cuda')
    msk = torch.zeros(128, dtype=torch.uint8, device='cuda')
    recs = torch.from_numpy(good[0][None]).cuda()
    y = torch.zeros(256, dtype=torch.float32, device='cuda')
    m = torch.zeros(64, dtype=torch.uint8, device='cuda')
    f = L.fgn_support_from_source_f32
    p = [src.data_ptr(), 256, msk.data_ptr(), 128, recs.data_ptr(), lut.data_ptr(), y.data_ptr(), m.data_ptr()]
    for i in (0, 2, 4, 5, 6, 7):                                                    # each pointer null in turn
        assert f(*[None if j == i else v for j, v in enumerate(p)], 1, 4, st) == -2, i
    for n, S in ((-1, 4), (1, -4), (1, 16385)):
        assert f(*p, n, S, st) == -1
    assert f(p[0], -1, *p[2:], 1, 4, st) == -1                                      # negative strides
    assert f(*p[:3], -1, *p[4:], 1, 4, st) == -1
    for n, S in ((0, 4), (1, 0)):                                                   # empty: no launch
        assert f(*p, n, S, st) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0 and int(m.max()) == 0
    s2, m2 = src.view(1, 256), msk.view(1, 128)
    y0, m0 = ops.support_from_source(s2[:0], m2[:0], recs[:0], lut, 4)
    assert tuple(y0.shape) == (0, 4, 4, 4) and tuple(m0.shape) == (0, 4, 4)
    y0, m0 = ops.support_from_source(s2, m2, recs, lut, 0)
    assert tuple(y0.shape) == (1, 0, 0, 4) and tuple(m0.shape) == (1, 0, 0)
    for bad in (dict(S=16385), dict(recs=recs.long()), dict(recs=recs[:, :15].contiguous()), dict(lut=lut[:, :255].contiguous()),
                dict(msk=torch.cat([m2, m2])), dict(src=s2.float())):
        args = dict(src=s2, msk=m2, recs=recs, lut=lut, S=4)
        args.update(bad)
        with pytest.raises(lib.FgnHipError):
            ops.support_from_source(**args)
