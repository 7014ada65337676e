"""The host rule of the query augmentation (``fgn_amd.fewshot_ds``: ``query_augment_record`` / ``augment_image_u8`` /
``augment_masks`` / ``augment_boxes_yxyx`` / ``augment_query`` / ``draw_query_augment``): the neutral row is
``resize_query``, flip is an exact reversal, known answers at equal size, kind 1 within one grey level of a float64
bilinear gather written here, the fallback, the coefficient bounds, the draw and the loader's samples."""
import itertools

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

NEUTRAL = [0, 0, 1, 0, 0, 0, 0, 0]


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


# the operators of ``augs_seq`` at the ends of their ranges, and one composed row
OPERATORS = {'rot10_sym': row(rotate=10, border=1), 'scale0.8': row(scale=0.8), 'scale1.2': row(scale=1.2),
             'shear+10_sym': row(shear=10, border=1), 'shear-10_sym': row(shear=-10, border=1),
             'shift_const': row(tx=-20, ty=13), 'composed_sym': row(1, 33, 1.1, 5, 3.3, -7.7, 1)}
SHAPES = [((7, 9), (16, 12)), ((37, 53), (64, 91)), ((150, 131), (128, 128)), ((101, 77), (128, 128)),
          ((2, 2), (300, 300)), ((1, 1), (5, 7)), ((5, 3000), (8, 4099))]


def _pixels(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)


def _sample(hw, seed, G=3):
    """An image, G masks and G boxes YXYX inside it."""
    rs = np.random.RandomState(seed)
    h, w = hw
    img = _pixels(hw, seed)
    masks = rs.rand(G, h, w) > 0.5
    y0, x0 = rs.uniform(0, h / 2, G), rs.uniform(0, w / 2, G)
    boxes = np.stack([y0, x0, y0 + rs.uniform(h / 4, h / 2, G), x0 + rs.uniform(w / 4, w / 2, G)], 1).astype(np.float32)
    return img, boxes, masks


# ------------------------------------------------------------------------------------ neutral row, flip
@pytest.mark.parametrize('src,dst', [((150, 131), (128, 128)), ((128, 128), (128, 128))])
@pytest.mark.parametrize('params', [None, NEUTRAL, row(border=1)])
def test_a_neutral_row_is_resize_query(src, dst, params):
    img, boxes, masks = _sample(src, 1)
    want = fd.resize_query(img, boxes, masks, *dst)
    got = fd.augment_query(img, boxes, masks, *dst, params)
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if src == dst:
        assert got[0] is img and got[1] is boxes and got[2] is masks
    rec = fd.query_augment_record(params, src, dst)
    assert rec.dtype == np.int32 and rec.shape == (16,) and rec.tolist()[:6] == [*src, 0, 0, int(bool(params is not None and params[6])), 0]
    assert np.array_equal(fd.augment_image_u8(img, rec, *dst), fd.resize_image_u8(img, *dst))
    assert np.array_equal(fd.augment_masks(masks, rec, *dst), fd.resize_masks(masks, *dst))


@pytest.mark.parametrize('src,dst', [((150, 131), (128, 128)), ((37, 53), (64, 91)), ((9, 9), (9, 9))])
def test_flip_alone_is_the_reversed_resize(src, dst):
    img, boxes, masks = _sample(src, 2)
    H, W = dst
    gi, gb, gm = fd.augment_query(img, boxes, masks, H, W, row(flip=1))
    assert np.array_equal(gi, fd.resize_image_u8(img, H, W)[:, ::-1])
    assert np.array_equal(gm, fd.resize_masks(masks, H, W)[:, :, ::-1])
    sb = fd.scale_boxes_yxyx(boxes, *src, H, W)
    want = np.stack([sb[:, 0], np.float32(W) - sb[:, 3], sb[:, 2], np.float32(W) - sb[:, 1]], 1)
    assert gb.dtype == np.float32 and gb.tobytes() == want.astype(np.float32).tobytes()
    assert fd.query_augment_record(row(flip=1), src, dst).tolist()[2:6] == [0, 1, 0, 0]


# ------------------------------------------------------------------------------------ known answers at 9 x 9
def _known(params, G=2):
    img, _, masks = _sample((9, 9), 5, G)
    rec = fd.query_augment_record(params, (9, 9), (9, 9))
    assert rec[2] == 1
    return img, masks, fd.augment_image_u8(img, rec, 9, 9), fd.augment_masks(masks, rec, 9, 9)


def test_rotation_by_90_degrees_is_rot90():
    for border in (0, 1):
        img, masks, gi, gm = _known(row(rotate=90, border=border))
        assert np.array_equal(gi, np.rot90(img, 3))
        assert np.array_equal(gm, np.rot90(masks, 3, axes=(1, 2)))


def test_translation_with_a_constant_border_is_the_shifted_image_with_zeros():
    img, masks, gi, gm = _known(row(tx=2, ty=-3))
    want = np.zeros_like(img)
    want[:6, 2:] = img[3:, :7]                      # out[y, x] = in[y + 3, x - 2]
    wm = np.zeros_like(masks)
    wm[:, :6, 2:] = masks[:, 3:, :7]
    assert np.array_equal(gi, want) and np.array_equal(gm, wm)


def test_translation_with_a_symmetric_border_is_the_slice_of_the_padded_image():
    img, masks, gi, gm = _known(row(tx=2, ty=-3, border=1))
    pad = np.pad(img, ((3, 3), (3, 3), (0, 0)), mode='symmetric')
    assert np.array_equal(gi, pad[3 + 3: 3 + 3 + 9, 3 - 2: 3 - 2 + 9])
    wm = np.zeros_like(masks)                       # the masks never see the symmetric border
    wm[:, :6, 2:] = masks[:, 3:, :7]
    assert np.array_equal(gm, wm)
    # further out than one image: the periodic extension
    img, _, gi, _ = _known(row(tx=-20, ty=13, border=1))
    pad = np.pad(img, ((27, 27), (27, 27), (0, 0)), mode='symmetric')
    assert np.array_equal(gi, pad[27 - 13: 27 - 13 + 9, 27 + 20: 27 + 20 + 9])


@pytest.mark.parametrize('order', range(6))
@pytest.mark.parametrize('params', [row(), row(flip=1), row(tx=1)])
def test_all_six_channel_orders(order, params):
    perm = list(itertools.permutations(range(3)))[order]
    assert fd.CHANNEL_ORDERS[order] == perm
    img = _pixels((9, 9), 8)
    p = params.copy()
    base = fd.augment_image_u8(img, fd.query_augment_record(p, (9, 9), (12, 11)), 12, 11)
    p[7] = order
    got = fd.augment_image_u8(img, fd.query_augment_record(p, (9, 9), (12, 11)), 12, 11)
    assert np.array_equal(got, base[..., list(perm)])
    if order == 0:
        assert np.array_equal(got, base)


# ------------------------------------------------------------------------------------ kind 1 against float64
def _matrix(p, src, dst):
    """M of the rule, restated: A = T(c) T(t) Rot ShearX Scale FlipX T(-c); M = Rz A^-1 P."""
    (h, w), (H, W) = src, dst
    T = lambda x, y: np.array([[1, 0, x], [0, 1, y], [0, 0, 1]], np.float64)
    th, ph = np.deg2rad(p[1]), np.deg2rad(p[3])
    rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    shear = np.array([[1, -np.tan(ph), 0], [0, 1, 0], [0, 0, 1]])
    A = T(W / 2, H / 2) @ T(p[4], p[5]) @ rot @ shear @ np.diag([p[2], p[2], 1]) @ np.diag([-1 if p[0] else 1, 1, 1]) \
        @ T(-W / 2, -H / 2)
    Rz = np.array([[w / W, 0, -0.5], [0, h / H, -0.5], [0, 0, 1]])
    return A, Rz @ np.linalg.inv(A) @ T(0.5, 0.5)


def _float_gather(img, M, dst, symmetric):
    """float64 bilinear gather of uint8 [h,w,C]: coordinates from M, floor, four taps, the two borders."""
    h, w = img.shape[:2]
    H, W = dst
    ox, oy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u = M[0, 0] * ox + M[0, 1] * oy + M[0, 2]
    v = M[1, 0] * ox + M[1, 1] * oy + M[1, 2]
    i0, j0 = np.floor(u), np.floor(v)
    fx, fy = u - i0, v - j0
    ext = np.zeros((h + 1, w + 1) + img.shape[2:], np.float64)
    ext[:h, :w] = img

    def index(k, n):
        k = k.astype(np.int64)
        if symmetric:
            r = np.mod(k, 2 * n)
            return np.where(r < n, r, 2 * n - 1 - r)
        return np.where((k >= 0) & (k < n), k, n)
    out = 0
    for a, wy in ((0, 1 - fy), (1, fy)):
        for b, wx in ((0, 1 - fx), (1, fx)):
            out = out + ext[index(j0 + a, h), index(i0 + b, w)] * (wy * wx)[..., None]
    return out


@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('name', OPERATORS)
def test_kind_1_is_within_one_grey_level_of_a_float64_gather(src, dst, name):
    p = OPERATORS[name]
    img = _pixels(src, src[1] + dst[0])
    rec = fd.query_augment_record(p, src, dst)
    assert rec[2] == 1 and rec[4] == int(p[6])
    _, M = _matrix(p, src, dst)
    assert np.allclose(fd.augment_source_matrix(p, src, dst), M[:2], rtol=0, atol=1e-9)
    want = _float_gather(img, M, dst, bool(p[6]))
    got = fd.augment_image_u8(img, rec, *dst).astype(np.float64)
    err_unrounded = np.abs(got - want).max()
    err = np.abs(got - np.floor(want + 0.5)).max()
    print(f'{name} {src}->{dst}: {err_unrounded:.3f} levels from the float64 value, {err:.0f} from the rounded one')
    assert err <= 1
    # the masks: the same taps on 0/1 with a constant border.  Per axis the weight is off by at most 2^-12 (11-bit
    # rounding) + (W + H) * 2^-21 (coefficients rounded to 2^-20, at most 4107 * 2^-21 = 2e-3 here), so the blended value
    # by less than 5e-3: only there around one half may the integer mask differ from the float one
    masks = np.random.RandomState(3).rand(2, *src) > 0.5
    gm = fd.augment_masks(masks, rec, *dst)
    fm = np.moveaxis(_float_gather(np.moveaxis(masks, 0, 2).astype(np.uint8), M, dst, False), 2, 0)
    assert gm.dtype == bool and gm.shape == (2,) + dst
    assert not (gm != (fm >= 0.5))[np.abs(fm - 0.5) > 5e-3].any()


def test_boxes_go_through_the_forward_matrix_in_float64():
    src, dst = (101, 77), (128, 128)
    _, boxes, _ = _sample(src, 4)
    sb = fd.scale_boxes_yxyx(boxes, *src, *dst)
    p = OPERATORS['composed_sym']
    A, _ = _matrix(p, src, dst)
    got, ok = fd.augment_boxes_yxyx(sb, p, *dst)
    assert ok and got.dtype == np.float32 and got.shape == sb.shape
    for b, g in zip(sb.astype(np.float64), got):
        c = np.array([[x, y, 1.] for y in (b[0], b[2]) for x in (b[1], b[3])]) @ A.T
        hull = np.array([c[:, 1].min(), c[:, 0].min(), c[:, 1].max(), c[:, 0].max()])
        assert np.allclose(g, np.clip(hull, 0, 128).astype(np.float32), rtol=0, atol=1e-4)
    assert (got >= 0).all() and (got <= 128).all()


# ------------------------------------------------------------------------------------ fallback, bounds, contract
def test_a_translation_that_moves_the_only_box_out_falls_back_to_the_plain_sample():
    src, dst = (150, 131), (128, 128)
    img, _, masks = _sample(src, 6, G=1)
    boxes = np.array([[10, 5, 60, 18]], np.float32)              # x2 = 18 * 128 / 131 < 20
    p = row(tx=-20, order=3)
    got = fd.augment_query(img, boxes, masks, *dst, p)
    want = fd.resize_query(img, boxes, masks, *dst)
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    rec, b2 = fd.augment_plan(p, boxes, src, dst)
    assert rec.tolist() == fd.query_augment_record(None, src, dst).tolist() and b2.tobytes() == want[1].tobytes()
    assert fd.augment_boxes_yxyx(want[1], p, *dst) == (None, False)
    # one pixel less and the box stays: augmented, clipped at 0
    gi, gb, _ = fd.augment_query(img, boxes, masks, *dst, row(tx=-17))
    assert not np.array_equal(gi, want[0]) and gb[0, 1] == 0 and 0 < gb[0, 3] < 1


def test_coefficients_beyond_the_bounds_are_refused():
    with pytest.raises(ValueError):
        fd.query_augment_record(row(scale=1e-3), (16384, 16384), (8, 8))        # 2048 / 1e-3 source pixels per pixel
    with pytest.raises(ValueError):
        fd.query_augment_record(row(tx=3e6), (128, 128), (128, 128))             # offset beyond 2^20 pixels
    assert fd.query_augment_record(row(scale=0.5), (16384, 16384), (512, 512))[6] == 64 << 20       # 2^26: the bound itself
    for bad in (row(flip=2), row(border=-1), row(order=6), row(order=1.5), row(scale=0), row(scale=-1),
                row(rotate=np.nan), row(tx=np.inf), np.zeros(7), np.zeros((2, 8)), ['a'] * 8):
        with pytest.raises(ValueError):
            fd.query_augment_record(bad, (9, 9), (9, 9))
    with pytest.raises(ValueError):
        fd.query_augment_record(row(), (0, 9), (9, 9))
    rec = fd.query_augment_record(row(tx=1), (9, 9), (9, 9))
    bad = rec.copy()
    bad[6] = (1 << 26) + 1
    with pytest.raises(ValueError):
        fd.augment_image_u8(_pixels((9, 9), 0), bad, 9, 9)
    with pytest.raises(ValueError):
        fd.augment_image_u8(_pixels((8, 9), 0), rec, 9, 9)                       # not the record's source size


# ------------------------------------------------------------------------------------ the draw and the loader
def test_draw_query_augment_is_deterministic_and_inside_the_operators_ranges():
    a = np.stack([fd.draw_query_augment(np.random.default_rng(7)) for _ in range(3)])
    assert (a == a[0]).all()
    rng = np.random.default_rng(11)
    rows = np.stack([fd.draw_query_augment(rng) for _ in range(4000)])
    assert rows.dtype == np.float64 and rows.shape == (4000, 8)
    for r in rows:
        fd.check_augment_params(r)
        geo = [r[0] == 1, r[1] != 0, r[2] != 1, r[3] != 0, bool(r[4] or r[5])]
        assert sum(geo) <= 1                                                     # one operator of five, or none
        assert r[1] in (0, 10) and 0.8 <= r[2] <= 1.2 and -10 <= r[3] <= 10
        assert r[4] == int(r[4]) and r[5] == int(r[5]) and abs(r[4]) <= 20 and abs(r[5]) <= 20
        assert r[6] == (1 if r[1] or r[3] else 0)
    frac = lambda m: float(np.mean(m))
    assert 0.07 < frac(rows[:, 0] == 1) < 0.13 and 0.07 < frac(rows[:, 1] == 10) < 0.13      # 1/10 each
    assert 0.45 < frac((rows[:, :6] != np.array(NEUTRAL[:6])).any(1)) < 0.55
    assert 0.03 < frac(rows[:, 7] != 0) < 0.09                                   # 1/14 * 5/6
    assert set(rows[:, 7]) == set(range(6))
    # a RandomState serves as well
    assert fd.draw_query_augment(np.random.RandomState(3)).tolist() == fd.draw_query_augment(np.random.RandomState(3)).tolist()


def test_loader_samples_carry_rows_that_collate():
    kw = dict(dataset='MNISTISEG', n_ways=2, k_shots=1, n_imgs=6, img_size=64, spp_img_size=32, raw_uint8=True,
              source_size=80)
    plain = fd.ClutteredCharsFewShotISEG(**kw)
    ds = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=True)
    off = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=False)
    for i in range(len(ds)):
        a, b, c = plain[i], ds[i], off[i]
        assert list(a) == list(c) and list(b) == list(a) + ['qry_augment']
        for k in a:                                  # everything else of the sample is what it was
            for x, y in ((a[k], b[k]), (a[k], c[k])):
                assert type(x) is type(y)
                assert torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y), k
        assert b['qry_augment'].dtype == np.float64 and b['qry_augment'].shape == (8,)
        assert np.array_equal(b['qry_augment'], ds[i]['qry_augment'])            # per (seed, child, epoch)
    batch = collate([ds[i] for i in range(4)])
    assert isinstance(batch['qry_augment'], torch.Tensor) and tuple(batch['qry_augment'].shape) == (4, 8)
    assert batch['qry_augment'].dtype == torch.float64
    before = np.stack([ds[i]['qry_augment'] for i in range(len(ds))])
    ds.reshuffle(e=9)
    after = np.stack([ds[i]['qry_augment'] for i in range(len(ds))])
    assert not np.array_equal(before, after)                                     # another epoch, another draw
    ds.reshuffle(e=0)
    ds.epoch = 0
    with pytest.raises(ValueError):
        fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_imgs=2, img_size=64, raw_uint8=True, augment_qry=True)
