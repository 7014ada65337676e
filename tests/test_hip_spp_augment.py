"""The support-augmentation kernels on the GPU against the host rule of ``fgn_amd.fewshot_ds`` - bit for bit:
``support_from_source_u8`` = ``support_from_source`` (crop and mask bytes), ``support_augment`` = ``augment_image_u8`` /
``augment_masks`` at S -> S followed by the table, and the three-launch chain = ``augment_support``."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import lib, ops

pytestmark = pytest.mark.gpu

# a clearly different table per channel (a channel mix-up cannot cancel); byte 0 maps to three different non-zero values
LUT = ops.input_lut((0.11, 0.52, 0.93), (0.21, 0.34, 0.47))


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


# the fourteen operator rows of tests/test_hip_qry_augment.py
OPERATORS = {'neutral': row(), 'flip': row(flip=1), 'rot10_sym': row(rotate=10, border=1), 'rot10_const': row(rotate=10),
             'scale0.8': row(scale=0.8), 'scale0.8_sym': row(scale=0.8, border=1), 'scale1.2': row(scale=1.2),
             'shear+10_sym': row(shear=10, border=1), 'shear-10_sym': row(shear=-10, border=1),
             'shear+10_const': row(shear=10), 'shift_const': row(tx=-20, ty=13), 'shift_sym': row(tx=-20, ty=13, border=1),
             'composed_sym': row(1, 33, 1.1, 5, 3.3, -7.7, 1, 4), 'composed_const': row(1, 33, 1.1, 5, 3.3, -7.7, 0, 3)}
SOURCES = [((1, 1), [0, 0, 1, 1]), ((3, 40), [0, 2, 3, 31]), ((37, 53), [0, 30, 20, 53]), ((150, 131), [40, 0, 131, 70])]
SIZES = (1, 5, 63, 64, 65, 130)             # 65: the smallest S with a second 64-lane chunk, of one lane


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _lut():
    return torch.from_numpy(LUT).cuda()


def _scene(hw, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, tuple(hw) + (3,)).astype(np.uint8), rs.rand(*hw) > 0.4


def _instance(hw, box, S, seed, crop_square=True):
    """-> (record, image window, mask window, wanted crop [S,S,3], wanted mask [S,S], box in the crop)."""
    img, mask = _scene(hw, seed)
    rec, _ = fd.support_geometry(hw[0], hw[1], box, S, crop_square=crop_square)
    crop, b, m = fd.support_from_source(img, box, mask, S, crop_square=crop_square)
    return (rec,) + fd.support_window(img, mask, rec) + (crop, m, b)


def _slots(wins, fill=0xFF):
    stride = max(w.size for w in wins)
    buf = torch.full((len(wins), stride), fill, dtype=torch.uint8)
    for i, w in enumerate(wins):
        buf[i, :w.size] = torch.from_numpy(w.reshape(-1))
    return buf.cuda()


def _inputs(insts):
    return (_slots([i[1] for i in insts]), _slots([i[2] for i in insts]),
            torch.from_numpy(np.stack([i[0] for i in insts])).cuda())


@pytest.fixture(scope='module')
def cuts():
    """Per S and crop mode the four source cases: the host's crops and masks, computed once and left unchanged."""
    return {(S, sq): [_instance(hw, box, S, hw[0] + S, sq) for hw, box in SOURCES] for S in SIZES for sq in (True, False)}


# ------------------------------------------------------------------------------------------- support_from_source_u8
@pytest.mark.parametrize('crop_square', [True, False])
@pytest.mark.parametrize('S', SIZES)
def test_the_byte_form_is_bitwise_the_host_rule_and_the_float_form_through_the_table(cuts, S, crop_square):
    insts = cuts[(S, crop_square)]
    src, msk, recs = _inputs(insts)
    crop, m = ops.support_from_source_u8(src, msk, recs, S)
    assert crop.dtype == torch.uint8 and tuple(crop.shape) == (4, S, S, 3) and m.dtype == torch.uint8
    assert tuple(m.shape) == (4, S, S)
    assert np.array_equal(crop.cpu().numpy(), np.stack([i[3] for i in insts]))
    assert np.array_equal(m.cpu().numpy(), np.stack([i[4] for i in insts]).astype(np.uint8))
    y, m2 = ops.support_from_source(src, msk, recs, _lut(), S)
    assert torch.equal(_ibits(ops.u8hwc3_to_nhwc4(crop, _lut())), _ibits(y)) and torch.equal(m, m2)
    if S >= 63:
        assert insts[3][0][10] == int(crop_square)                                   # the zero mode was really taken


def test_a_bad_record_between_two_good_ones_gives_zeros_and_an_empty_mask(cuts):
    S = 65
    good = cuts[(S, True)][2]
    bad = good[0].copy()
    bad[6] = S + 1                                                                   # nh does not fit S
    src, msk, _ = _inputs([good] * 3)
    recs = torch.from_numpy(np.stack([good[0], bad, good[0]])).cuda()
    n_c, n_m = 3 * S * S * 3, 3 * S * S
    cbuf = torch.full((7 + n_c + 16,), 9, dtype=torch.uint8, device='cuda')
    mbuf = torch.full((5 + n_m + 16,), 7, dtype=torch.uint8, device='cuda')
    rc = lib.load().fgn_support_from_source_u8(src.data_ptr(), src.shape[1], msk.data_ptr(), msk.shape[1], recs.data_ptr(),
                                               cbuf[7:].data_ptr(), mbuf[5:].data_ptr(), 3, S,
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    crop, m = cbuf[7:7 + n_c].view(3, S, S, 3).cpu().numpy(), mbuf[5:5 + n_m].view(3, S, S).cpu().numpy()
    for i in (0, 2):
        assert np.array_equal(crop[i], good[3]) and np.array_equal(m[i], good[4].astype(np.uint8))
    assert not crop[1].any() and not m[1].any() and good[3].any() and good[4].any()
    assert int((cbuf[:7] != 9).sum()) == 0 and int((cbuf[7 + n_c:] != 9).sum()) == 0      # nothing around crop
    assert int((mbuf[:5] != 7).sum()) == 0 and int((mbuf[5 + n_m:] != 7).sum()) == 0      # nothing around m


def test_byte_form_return_codes():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    b = lambda n: torch.zeros(n, dtype=torch.uint8, device='cuda')
    src, msk, crop, m = b(64), b(64), b(64), b(64)
    rec = torch.zeros((1, 16), dtype=torch.int32, device='cuda')
    p = (src.data_ptr(), 64, msk.data_ptr(), 64, rec.data_ptr(), crop.data_ptr(), m.data_ptr())
    f = L.fgn_support_from_source_u8
    for i in (0, 2, 4, 5, 6):
        assert f(*[None if j == i else v for j, v in enumerate(p)], 1, 2, st) == -2
    for dims in ((-1, 2), (1, -1), (1, 16385)):
        assert f(*p, *dims, st) == -1
    assert f(p[0], -1, *p[2:], 1, 2, st) == -1 and f(*p[:3], -1, *p[4:], 1, 2, st) == -1
    for dims in ((0, 2), (1, 0)):
        assert f(*p, *dims, st) == 0
    assert tuple(ops.support_from_source_u8(src.view(1, 64)[:0], msk.view(1, 64)[:0], rec[:0], 4)[0].shape) == (0, 4, 4, 3)
    with pytest.raises(lib.FgnHipError):
        ops.support_from_source_u8(src.view(1, 64), msk.view(1, 64), rec.long(), 4)
    with pytest.raises(lib.FgnHipError):
        ops.support_from_source_u8(src.view(1, 64), msk.view(2, 32), rec, 4)
    with pytest.raises(lib.FgnHipError):
        ops.support_from_source_u8(src.view(1, 64).cpu(), msk.view(1, 64), rec, 4)
    with pytest.raises(lib.FgnHipError):
        ops.support_from_source_u8(src.view(1, 64), msk.view(1, 64), rec, 16385)


# --------------------------------------------------------------------------------------------------- support_augment
def _want(crops, masks, recs, S):
    """The host rule at S -> S, then the existing uint8 kernel."""
    x = np.stack([fd.augment_image_u8(c, r, S, S) for c, r in zip(crops, recs)])
    m = np.stack([fd.augment_masks(k[None], r, S, S)[0] for k, r in zip(masks, recs)]).astype(np.uint8)
    return ops.u8hwc3_to_nhwc4(torch.from_numpy(x).cuda(), _lut()), torch.from_numpy(m).cuda()


def _augment(crops, masks, recs, S):
    return ops.support_augment(torch.from_numpy(np.stack(crops)).cuda(), torch.from_numpy(np.stack(masks)).cuda(),
                               torch.from_numpy(np.stack(recs)).cuda(), _lut(), S)


@pytest.mark.parametrize('S', SIZES)
def test_the_gather_is_bitwise_the_host_rule_on_every_operator_row(cuts, S):
    """All fourteen rows as fourteen instances of ONE launch, on a cut crop with pad bands (3x40) and on a full one."""
    for which in (1, 3):
        crop, mask = cuts[(S, True)][which][3:5]
        recs = [fd.query_augment_record(p, (S, S), (S, S)) for p in OPERATORS.values()]
        y, m = _augment([crop] * len(recs), [mask] * len(recs), recs, S)
        want_y, want_m = _want([crop] * len(recs), [mask] * len(recs), recs, S)
        assert y.dtype == torch.float32 and tuple(y.shape) == (len(recs), S, S, 4) and m.dtype == torch.uint8
        for i, name in enumerate(OPERATORS):
            assert torch.equal(_ibits(y[i]), _ibits(want_y[i])), name
            assert torch.equal(m[i], want_m[i]), name
        assert int(_ibits(y[..., 3]).abs().max()) == 0                              # +0.0, not -0.0


@pytest.mark.parametrize('S', SIZES)
@pytest.mark.parametrize('base', ['neutral', 'flip', 'rot10_sym', 'scale1.2'])
def test_all_six_channel_orders(cuts, base, S):
    crop, mask = cuts[(S, True)][2][3:5]
    rows = []
    for order in range(6):
        p = OPERATORS[base].copy()
        p[7] = order
        rows.append(p)
    recs = [fd.query_augment_record(p, (S, S), (S, S)) for p in rows]
    y, m = _augment([crop] * 6, [mask] * 6, recs, S)
    want_y, want_m = _want([crop] * 6, [mask] * 6, recs, S)
    assert torch.equal(_ibits(y), _ibits(want_y)) and torch.equal(m, want_m)
    plain = fd.augment_image_u8(crop, recs[0], S, S)
    for order in range(6):                  # by the definition: out[c] = in[order[c]], each through table c
        x = np.ascontiguousarray(plain[..., list(fd.CHANNEL_ORDERS[order])])
        assert torch.equal(_ibits(y[order]), _ibits(ops.u8hwc3_to_nhwc4(torch.from_numpy(x[None]).cuda(), _lut())[0]))
        assert torch.equal(m[order], m[0])


def test_three_instances_of_different_kinds_in_one_launch_between_guards(cuts):
    S = 65
    insts = cuts[(S, True)][1:]
    crops, masks = [i[3] for i in insts], [(i[4] * 200).astype(np.uint8) for i in insts]     # nonzero bytes other than 1
    recs = np.stack([fd.query_augment_record(p, (S, S), (S, S)) for p in
                     (row(flip=1, order=2), row(1, 33, 1.1, 5, 3.3, -7.7, 1, 5), row(tx=-20, ty=13))])
    assert recs[:, 2].tolist() == [0, 1, 1]
    dcrop, dmsk = torch.from_numpy(np.stack(crops)).cuda(), torch.from_numpy(np.stack(masks)).cuda()
    before = dcrop.clone(), dmsk.clone()
    n_y, n_m = 3 * S * S * 4, 3 * S * S
    ybuf = torch.zeros(16 + n_y + 64, dtype=torch.float32, device='cuda')
    mbuf = torch.full((5 + n_m + 16,), 7, dtype=torch.uint8, device='cuda')
    drec = torch.from_numpy(recs).cuda()
    rc = lib.load().fgn_support_augment_f32(dcrop.data_ptr(), dmsk.data_ptr(), drec.data_ptr(), _lut().data_ptr(),
                                            ybuf[16:].data_ptr(), mbuf[5:].data_ptr(), 3, S,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    want_y, want_m = _want(crops, [i[4] for i in insts], recs, S)
    assert torch.equal(_ibits(ybuf[16:16 + n_y].view(3, S, S, 4)), _ibits(want_y))
    assert torch.equal(mbuf[5:5 + n_m].view(3, S, S), want_m)
    assert int(_ibits(ybuf[:16]).abs().max()) == 0 and int(_ibits(ybuf[16 + n_y:]).abs().max()) == 0
    assert int((mbuf[:5] != 7).sum()) == 0 and int((mbuf[5 + n_m:] != 7).sum()) == 0
    assert torch.equal(dcrop, before[0]) and torch.equal(dmsk, before[1])           # the sources are only read
    y2, m2 = ops.support_augment(dcrop, dmsk > 0, drec, _lut(), S)                  # the wrapper, a bool mask
    assert torch.equal(_ibits(y2), _ibits(want_y)) and torch.equal(m2, want_m)


@pytest.mark.parametrize('S', SIZES)
def test_the_neutral_record_is_the_identity_through_the_table(cuts, S):
    insts = cuts[(S, True)]
    crops, masks = [i[3] for i in insts], [i[4] for i in insts]
    recs = [fd.query_augment_record(p, (S, S), (S, S)) for p in (None, row(), row(border=1), None)]
    y, m = _augment(crops, masks, recs, S)
    src, msk, srec = _inputs(insts)
    want_y, want_m = ops.support_from_source(src, msk, srec, _lut(), S)             # the direct path's bytes
    assert torch.equal(_ibits(y), _ibits(want_y)) and torch.equal(m, want_m)


def _padding(S):
    y = torch.zeros((S, S, 4))
    y[..., :3] = torch.from_numpy(LUT[:, 0].copy())
    return y.cuda()


def test_a_refused_record_gives_padding_and_an_empty_mask_for_that_instance_only(cuts):
    S = 65
    crop, mask = cuts[(S, True)][3][3:5]
    ok = fd.query_augment_record(row(rotate=10, border=1), (S, S), (S, S))

    def mod(**kw):
        r = ok.copy()
        for k, v in kw.items():
            r[fd.AUG_REC_FIELDS.index(k)] = v
        return r
    bad = [mod(h=S - 1), mod(w=S + 1), mod(h=S + 1, w=S + 1), mod(h=0), mod(w=-3), mod(h=16385), mod(kind=2), mod(kind=-1),
           mod(flip=2), mod(border=2), mod(perm=6), mod(perm=-1), mod(c00=(1 << 26) + 1), mod(c01=-(1 << 26) - 1),
           mod(c10=(1 << 26) + 1), mod(c11=-(1 << 26) - 1), mod(c02_lo=1, c02_hi=1 << 8), mod(c12_lo=-1, c12_hi=-(1 << 8) - 1),
           fd.query_augment_record(row(flip=1), (S, S + 1), (S, S))]
    recs = [ok] + bad + [ok]
    y, m = _augment([crop] * len(recs), [np.ones_like(mask)] * len(recs), recs, S)
    want_y, want_m = _want([crop], [np.ones_like(mask)], [ok], S)
    pad = _padding(S)
    for i in (0, len(recs) - 1):
        assert torch.equal(_ibits(y[i]), _ibits(want_y[0])) and torch.equal(m[i], want_m[0])
    assert int(want_m.max()) == 1
    for i in range(1, len(recs) - 1):
        assert torch.equal(_ibits(y[i]), _ibits(pad)), i
        assert int(m[i].max()) == 0, i
    edge = mod(c00=1 << 26, c11=-(1 << 26), c02_lo=0, c02_hi=1 << 8, c12_lo=0, c12_hi=-(1 << 8))      # the bounds are inside
    y, m = _augment([crop], [mask], [edge], S)
    want_y, want_m = _want([crop], [mask], [edge], S)
    assert torch.equal(_ibits(y), _ibits(want_y)) and torch.equal(m, want_m)


def test_gather_return_codes_and_nothing_written():
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S = 2
    crop = torch.zeros(64, dtype=torch.uint8, device='cuda')
    msk = torch.zeros(64, dtype=torch.uint8, device='cuda')
    m = torch.zeros(64, dtype=torch.uint8, device='cuda')
    y = torch.zeros(256, dtype=torch.float32, device='cuda')
    rec = torch.from_numpy(fd.query_augment_record(row(flip=1), (S, S), (S, S))[None]).cuda()
    lut = _lut()
    p = (crop.data_ptr(), msk.data_ptr(), rec.data_ptr(), lut.data_ptr(), y.data_ptr(), m.data_ptr())
    f = L.fgn_support_augment_f32
    for i in range(6):                                                              # each pointer null in turn
        assert f(*[None if j == i else v for j, v in enumerate(p)], 1, S, st) == -2
    # crop / y and msk / m overlapping (n * S * S = 4 pixels: 12 bytes of crop, 64 of y, 4 of msk and of m); adjacent is fine
    yb = y.view(torch.uint8)
    assert f(yb.data_ptr(), *p[1:], 1, S, st) == -2
    assert f(yb[63:].data_ptr(), *p[1:], 1, S, st) == -2 and f(yb[64:].data_ptr(), *p[1:], 1, S, st) == 0
    assert f(*p[:5], msk.data_ptr(), 1, S, st) == -2
    assert f(*p[:5], msk[3:].data_ptr(), 1, S, st) == -2 and f(*p[:5], msk[4:].data_ptr(), 1, S, st) == 0
    for dims in ((-1, S), (1, -1), (1, 16385)):
        assert f(*p, *dims, st) == -1
    y.zero_(), m.zero_(), msk.zero_()
    for dims in ((0, S), (1, 0)):                                                   # empty: no launch
        assert f(*p, *dims, st) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0 and int(m.max()) == 0
    c4, k4 = crop[:12].view(1, S, S, 3), msk[:4].view(1, S, S)
    assert tuple(ops.support_augment(c4[:0], k4[:0], rec[:0], lut, S)[0].shape) == (0, S, S, 4)
    assert tuple(ops.support_augment(c4[:, :0, :0], k4[:, :0, :0], rec, lut, 0)[1].shape) == (1, 0, 0)
    for args in ((c4.float(), k4, rec, lut, S), (c4, k4.float(), rec, lut, S), (c4, k4, rec.long(), lut, S),
                 (c4, k4, rec[:, :15].contiguous(), lut, S), (c4, k4, rec, lut[:, :255].contiguous(), S),
                 (c4, k4, rec, lut, 3), (c4.cpu(), k4, rec, lut, S), (c4, k4, rec, lut, 16385),
                 (crop[:24].view(2, S, S, 3)[:, :, :1], k4, rec, lut, S)):
        with pytest.raises(lib.FgnHipError):
            ops.support_augment(*args)


# ----------------------------------------------------------------------------------------------- the three-launch chain
def test_the_chain_on_three_instances_is_bitwise_augment_support(cuts):
    S = 65
    insts = cuts[(S, True)][1:]
    geo = [row(), row(rotate=10, border=1, order=4), row()]
    photo = [(3, 1.2, 0), (4, 50, 0), (0, 0, 0)]                                     # blur, hue with rotation, neutral
    recs, precs, boxes, fell = fd.support_augment_plan(geo, photo, np.stack([i[5] for i in insts]), S)
    assert not fell.any() and precs[:, 2].tolist() == [3, 4, 0] and recs[:, 2].tolist() == [0, 1, 0]
    src, msk, srec = _inputs(insts)
    crop, m0 = ops.support_from_source_u8(src, msk, srec, S)
    crop2 = ops.photometric_u8(crop.view(3, -1), torch.from_numpy(precs).cuda()).view(3, S, S, 3)
    y, m = ops.support_augment(crop2, m0, torch.from_numpy(recs).cuda(), _lut(), S)
    want = [fd.augment_support(i[3], i[5], i[4], g, p) for i, g, p in zip(insts, geo, photo)]
    want_y = ops.u8hwc3_to_nhwc4(torch.from_numpy(np.stack([w[0] for w in want])).cuda(), _lut())
    assert torch.equal(_ibits(y), _ibits(want_y))
    assert np.array_equal(m.cpu().numpy(), np.stack([w[2] for w in want]).astype(np.uint8))
    assert np.array_equal(boxes, np.stack([w[1] for w in want]))
    assert not np.array_equal(want[0][0], insts[0][3]) and not np.array_equal(want[1][0], insts[1][3])
    direct = ops.support_from_source(src, msk, srec, _lut(), S)                      # the neutral instance: the direct
    assert torch.equal(_ibits(y[2]), _ibits(direct[0][2])) and torch.equal(m[2], direct[1][2])          # path's bytes
