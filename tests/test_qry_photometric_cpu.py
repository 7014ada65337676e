"""The host rule of the photometric query augmentation (``fgn_amd.fewshot_ds``: ``query_photometric_record``,
``photometric_image_u8``, ``draw_query_augment_full``) - no GPU: Philox known answers, hue / saturation / brightness
against the float64 closed form, the blur against a float64 convolution, the statistics of the two noises at fixed seeds,
the joint draw, the record's contract errors and the loader's flag."""
import math

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

NET = (64, 64)


def _pixels(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)


def _apply(img, row, net=None):
    hw = img.shape[:2]
    return fd.photometric_image_u8(img, fd.query_photometric_record(row, hw, hw if net is None else net))


def test_philox4x32_10_known_answers():
    def words(s):
        return [int(v, 16) for v in s.split()]
    for ctr, key, out in (([0] * 4, [0] * 2, '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
                          ([0xffffffff] * 4, [0xffffffff] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
                          (words('243f6a88 85a308d3 13198a2e 03707344'), words('a4093822 299f31d0'),
                           'd16cfe09 94fdcceb 5001e420 24126ea1')):
        got = fd.philox4x32(ctr, key)
        assert got.dtype == np.uint32 and got.tolist() == words(out)
    # vectorised over counters, the key broadcast
    both = fd.philox4x32([[0] * 4, [0xffffffff] * 4], [0, 0])
    assert both.shape == (2, 4) and both[0].tolist() == words('6627e8d5 e169c58d bc57ac4c 9b00dbd8')


def test_a_neutral_row_returns_identical_bytes():
    img = _pixels((37, 53), 1)
    keep = img.copy()
    for row in (None, (0, 0, 0), (0, 7.5, 9), (2, 0, 3), (3, 0, 0), (4, 0, 0), (5, 0, 0), (6, 0, 5)):
        rec = fd.query_photometric_record(row, (37, 53), NET)
        assert rec.dtype == np.int32 and rec.shape == (fd.PHOTO_REC_INTS,) == (64,)
        assert rec[:2].tolist() == [37, 53] and not rec[2:].any()
        out = fd.photometric_image_u8(img, rec)
        assert out is not img and np.array_equal(out, keep)
    assert np.array_equal(img, keep)
    assert fd.PHOTO_PARAMS == ('operator', 'amount', 'seed')


# ---- hue, saturation, brightness ------------------------------------------------------------------------------------
def _lattice():
    lv = np.array(list(range(0, 255, 5)) + [255], np.uint8)
    assert len(lv) == 52
    r, g, b = np.meshgrid(lv, lv, lv, indexing='ij')
    return np.stack([r, g, b], -1).reshape(52, 52 * 52, 3)


def _hsv_float(img, op, amount):
    """The closed form in float64 -> the unrounded channels [...,3]."""
    r, g, b = (img[..., c].astype(np.float64) for c in range(3))
    V = np.maximum(np.maximum(r, g), b)
    d = V - np.minimum(np.minimum(r, g), b)
    dd = np.where(d == 0, 1.0, d)
    S = np.where(V == 0, 0.0, d / np.where(V == 0, 1.0, V))
    h6 = np.where(V == r, np.mod((g - b) / dd, 6.0), np.where(V == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    h6 = np.where(d == 0, 0.0, h6)
    if op == 4:
        h6 = np.mod(h6 + amount * 3.0 / 255.0, 6.0)
    elif op == 5:
        S = np.clip(S + amount / 255.0, 0.0, 1.0)
    else:
        V = np.clip(V + amount, 0.0, 255.0)
    out = []
    for n in (5, 3, 1):
        k = np.mod(n + h6, 6.0)
        out.append(V - V * S * np.maximum(0.0, np.minimum(np.minimum(k, 4.0 - k), 1.0)))
    return np.stack(out, -1)


HSV_AMOUNTS = {4: (-255, -50, -17.3, 50, 170, 255), 5: (-255, -75, -20.5, 33, 75, 255), 6: (-255, -30, -7.25, 30, 100, 255)}


@pytest.mark.parametrize('op', (4, 5, 6))
def test_hue_saturation_brightness_within_one_level_of_the_float64_closed_form(op):
    """Every byte within 1 level of the rounded float64 value on the 52^3 lattice; the derivation bounds
    the integer rule's error before its own rounding by 0.02 level, so from the unrounded value it stays below 0.52."""
    img = _lattice()
    worst = 0.0
    for amount in HSV_AMOUNTS[op]:
        got = _apply(img, (op, amount, 0)).astype(np.float64)
        ref = _hsv_float(img, op, float(amount))
        worst = max(worst, float(np.abs(got - ref).max()))
        assert np.abs(got - np.rint(ref)).max() <= 1, (op, amount)
    print(f'operator {op}: largest distance from the unrounded float64 value {worst:.4f} levels')
    assert worst < 0.52


def test_hsv_known_answers():
    img = _lattice()
    assert np.array_equal(_apply(img, (4, 170, 0)), img[..., [2, 0, 1]])           # two sextants: (b, r, g), exactly
    assert np.array_equal(_apply(img, (4, -170, 0)), img[..., [1, 2, 0]])
    mx = img.max(-1, keepdims=True)
    assert np.array_equal(_apply(img, (5, -255, 0)), np.repeat(mx, 3, -1))          # no saturation: all channels = max
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, -1)
    for a in (1, 30, 100, 255, -1, -30, -255):
        want = np.clip(grey.astype(np.int64) + a, 0, 255).astype(np.uint8)
        assert np.array_equal(_apply(grey, (6, a, 0)), want), a
    assert np.array_equal(_apply(grey, (4, 77, 0)), grey) and np.array_equal(_apply(grey, (5, -60, 0)), grey)


# ---- blur -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', (0.05, 0.5, 1, 3))
def test_blur_weights_are_symmetric_and_sum_to_2048(sigma):
    src, net = (60, 100), (80, 133)                                                  # a non-square size ratio
    rec = fd.query_photometric_record((3, sigma, 0), src, net)
    g = fd._photo_fields(rec)
    for n_src, n_net, r, w in ((100, 133, g['rx'], g['wx']), (60, 80, g['ry'], g['wy'])):
        s = sigma * n_src / n_net
        assert r == max(1, math.ceil(3 * s)) and len(w) == r + 1
        assert w.min() >= 0 and w[0] + 2 * w[1:].sum() == 2048                      # (stored once per |offset|: symmetric)
        assert np.all(np.diff(w) <= 0)
        k = np.arange(-r, r + 1)
        gk = np.exp(-k * k / (2.0 * s * s))
        assert np.abs(w[1:] - (2048 * gk / gk.sum())[r + 1:]).max() <= 0.5 + 1e-9    # rounded; the centre takes the rest
        assert abs(w[0] - 2048 * gk[r] / gk.sum()) <= r + 1e-9


def test_blur_of_a_constant_image_and_with_a_tiny_sigma():
    for hw in ((1, 1), (2, 3), (3, 40), (37, 53)):
        const = np.full(hw + (3,), 0, np.uint8)
        const[..., 0], const[..., 1], const[..., 2] = 255, 77, 1
        for sigma in (0.4, 1, 3, 5.3):
            assert np.array_equal(_apply(const, (3, sigma, 0)), const)
        img = _pixels(hw, 5)
        rec = fd.query_photometric_record((3, 0.05, 0), hw, hw)
        assert rec[2] == 3 and rec[8] == 2048 and rec[25] == 2048                    # the centre weight is all of it
        assert np.array_equal(fd.photometric_image_u8(img, rec), img)


@pytest.mark.parametrize('hw', ((1, 1), (2, 3), (3, 40), (37, 53)))
@pytest.mark.parametrize('sigma', (0.5, 1.0, 3.0))
def test_blur_within_one_level_of_a_float64_convolution(hw, sigma):
    """scipy's correlate1d(mode='mirror') per axis with the float64 normalised weights of the same radius, at sigmas over
    the range of the draw.  Every byte within 1 level of the rounded float64 value (fixed seeds: deterministic)."""
    from scipy.ndimage import correlate1d
    img = _pixels(hw, hw[0] + 3)
    got = _apply(img, (3, sigma, 0)).astype(np.float64)
    r = max(1, math.ceil(3 * sigma))
    k = np.arange(-r, r + 1)
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    g /= g.sum()
    ref = correlate1d(correlate1d(img.astype(np.float64), g, axis=1, mode='mirror'), g, axis=0, mode='mirror')
    print(f'blur {hw} sigma {sigma}: largest distance from the unrounded float64 value {np.abs(got - ref).max():.4f}')
    assert np.abs(got - np.rint(ref)).max() <= 1


def test_reflect101_indices():
    assert fd.reflect101(np.arange(-5, 9), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert fd.reflect101(np.arange(-40, 40), 1).tolist() == [0] * 80
    assert fd.reflect101(np.arange(-4, 5), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]


# ---- noise ----------------------------------------------------------------------------------------------------------
def _phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


@pytest.mark.parametrize('scale,seed', ((1.0, 1234), (2.0, 99)))
def test_gaussian_noise_statistics_and_determinism(scale, seed):
    n = 256
    img = np.full((n, n, 3), 128, np.uint8)
    out = _apply(img, (1, scale, seed))
    assert np.array_equal(out, _apply(img, (1, scale, seed)))                         # deterministic per (seed, pixel)
    assert not np.array_equal(out, _apply(img, (1, scale, seed + 1)))                 # another seed, another field
    k = out.astype(np.int64) - 128
    assert np.array_equal(k[..., 0], k[..., 1]) and np.array_equal(k[..., 0], k[..., 2])    # the channels move together
    k = k[..., 0].astype(np.float64)
    assert np.abs(k).max() <= 12
    # rounded N(0, scale^2) in float64: P(k) = Phi((k + 1/2) / s) - Phi((k - 1/2) / s)
    ks = np.arange(-40, 41)
    pk = np.array([_phi((v + 0.5) / scale) - _phi((v - 0.5) / scale) for v in ks])
    var = float((pk * ks * ks).sum())
    m4 = float((pk * ks ** 4).sum())
    N = n * n
    assert abs(k.mean()) <= 5 * math.sqrt(var / N)
    assert abs(k.var() - var) <= 5 * math.sqrt((m4 - var * var) / N)
    # a pixel's noise is its own: the top-left crop of the same width draws the same values
    assert np.array_equal(_apply(img[:7], (1, scale, seed)), out[:7])


def test_gaussian_noise_clips_at_both_ends():
    lo, hi = np.zeros((64, 64, 3), np.uint8), np.full((64, 64, 3), 255, np.uint8)
    a, b = _apply(lo, (1, 2, 7)).astype(int), _apply(hi, (1, 2, 7)).astype(int)
    mid = _apply(np.full((64, 64, 3), 128, np.uint8), (1, 2, 7)).astype(int) - 128
    assert np.array_equal(a, np.clip(mid, 0, 255)) and np.array_equal(b, np.clip(255 + mid, 0, 255))
    assert (mid < 0).any() and (mid > 0).any()


def test_noise_thresholds_are_the_normal_cdf():
    for scale in (0.3, 1.0, 2.0):
        L = fd.noise_thresholds(scale)
        assert L.shape == (12,) and np.all(np.diff(L) >= 0) and L.min() >= 0 and L.max() < 2 ** 31
        for j in (0, 5, 11):
            assert abs(int(L[j]) - _phi((j - 11.5) / scale) * 2.0 ** 32) <= 1
    assert fd.noise_thresholds(2.0)[0] == 19                                         # Phi(-5.75) * 2^32 = 19.2


def test_impulse_noise_share_values_and_untouched_bytes():
    n = 256
    img = np.full((n, n, 3), 100, np.uint8)
    img[::2] = 200
    out = _apply(img, (2, 0.03, 4321))
    hit = out != img
    cnt = int(hit.sum())
    sd = math.sqrt(n * n * 3 * 0.03 * 0.97)
    print(f'impulse noise: {cnt} of {n * n * 3} bytes replaced (expected {n * n * 3 * 0.03:.0f} +- {sd:.0f})')
    assert abs(cnt - n * n * 3 * 0.03) <= 5 * sd                                       # 5898 +- 5 * 75.6 = 378
    vals = out[hit]
    assert set(np.unique(vals).tolist()) == {0, 255}
    assert abs(int((vals == 255).sum()) - cnt / 2) <= 5 * math.sqrt(cnt) / 2
    assert np.array_equal(out[~hit], img[~hit])
    per_ch = hit.reshape(-1, 3).sum(0)
    assert all(abs(int(c) - n * n * 0.03) <= 5 * math.sqrt(n * n * 0.03 * 0.97) for c in per_ch)    # each channel on its own
    assert not np.array_equal(hit[..., 0], hit[..., 1])
    assert np.array_equal(_apply(img, (2, 0, 4321)), img)                              # p = 0
    full = _apply(img, (2, 1, 4321))                                                   # p = 1: every byte
    assert set(np.unique(full).tolist()) == {0, 255}
    assert np.array_equal(out, _apply(img, (2, 0.03, 4321))) and not np.array_equal(out, _apply(img, (2, 0.03, 4322)))


# ---- the joint draw -------------------------------------------------------------------------------------------------
def test_joint_draw_ranges_exclusion_and_frequencies():
    a = [fd.draw_query_augment_full(np.random.default_rng([7, i])) for i in range(50)]
    b = [fd.draw_query_augment_full(np.random.default_rng([7, i])) for i in range(50)]
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    rng = np.random.default_rng(2024)
    n = 4000
    counts = np.zeros(8, np.int64)                      # operators 1..6 of the second row, 7: a channel-order draw
    geo = 0
    ranges = {1: (1, 1), 2: (0, 0.03), 3: (0, 3), 4: (-50, 50), 5: (-75, 75), 6: (-30, 30)}
    rng_shuffle = 0
    for _ in range(n):
        p, q = fd.draw_query_augment_full(rng)
        assert p.shape == (8,) and q.shape == (3,) and p.dtype == q.dtype == np.float64
        fd.check_augment_params(p)
        fd.check_photometric_params(q)
        assert not (p[7] != 0 and q[0] != 0)                                         # never both
        if q[0]:
            lo, hi = ranges[int(q[0])]
            assert lo <= q[1] <= hi and 0 <= q[2] < 2 ** 32 and q[2] == int(q[2])
            counts[int(q[0])] += 1
        else:
            assert q.tolist() == [0, 0, 0]
        rng_shuffle += p[7] != 0
        geo += fd.augment_kind(p) == 1 or p[0] == 1
    sd = math.sqrt(n * (1 / 14) * (13 / 14))
    assert all(abs(int(c) - n / 14) <= 5 * sd for c in counts[1:7]), counts
    # the channel order is drawn with 1/14 too; order 0 of its six is the identity: 5/6 of them show
    assert abs(int(rng_shuffle) - n * 5 / 84) <= 5 * math.sqrt(n * (5 / 84) * (79 / 84))
    assert abs(geo - n / 2) <= 5 * math.sqrt(n / 4)                                  # the geometric half, as it was
    # draw_query_augment and its stream are what they were
    assert np.array_equal(fd.draw_query_augment(np.random.default_rng(5)), fd.draw_query_augment(np.random.default_rng(5)))


# ---- contract errors of the record ----------------------------------------------------------------------------------
def test_record_errors():
    ok = lambda row, src=(37, 53), net=(37, 53): fd.query_photometric_record(row, src, net)
    ok((1, 2.0, 2 ** 32 - 1))
    ok((3, 5.3, 0))
    bad = [(1, 2.0001, 0), (1, 0, 0), (1, -1, 0),                                     # noise scale in (0, 2]
           (2, -0.01, 0), (2, 1.01, 0),                                               # p in [0, 1]
           (3, -1, 0), (3, 5.34, 0),                                                  # sigma >= 0; radius 17
           (4, 255.5, 0), (5, -256, 0), (6, 300, 0),
           (7, 0, 0), (-1, 0, 0), (1.5, 1, 0),                                        # operators
           (1, 1, -1), (1, 1, 2 ** 32), (1, 1, 0.5),                                  # seeds
           (np.nan, 0, 0), (1, np.inf, 0), (1, 1, np.nan),                            # non-finite
           (1, 1), (1, 1, 1, 1), [[1, 1, 1]], 'abc']                                  # shapes
    for row in bad:
        with pytest.raises(ValueError, match='qry_photometric'):
            ok(row)
    with pytest.raises(ValueError, match='qry_photometric'):                         # radius 16 at equal size, 17 through the ratio
        ok((3, 5.3, 0), (37, 60), (37, 53))
    with pytest.raises(ValueError):
        ok((1, 1, 0), (0, 5))
    with pytest.raises(ValueError):
        ok((1, 1, 0), (5, 5), (5, fd.RESIZE_MAX_DIM + 1))
    img = _pixels((37, 53), 2)
    rec = ok((3, 1, 0))
    with pytest.raises(ValueError):
        fd.photometric_image_u8(img[:30], rec)                                         # another size than the record's
    with pytest.raises(ValueError):
        fd.photometric_image_u8(img, rec[:16])
    for i, v in ((2, 7), (6, 17), (8, rec[8] + 1), (0, 0)):                            # what the kernel refuses
        r = rec.copy()
        r[i] = v
        with pytest.raises(ValueError):
            fd.photometric_image_u8(img, r)


def test_the_sibling_of_augment_query_and_its_fallback():
    img = _pixels((40, 50), 3)
    masks = np.zeros((1, 40, 50), bool)
    masks[0, 10:20, 10:30] = True
    boxes = np.array([[10, 10, 20, 30]], np.float32)
    flip = np.array([1, 0, 1, 0, 0, 0, 0, 0], np.float64)
    hue = (4, 50, 0)
    a = fd.augment_query_full(img, boxes, masks, 64, 64, flip, hue)
    rec = fd.query_photometric_record(hue, (40, 50), (64, 64))
    b = fd.augment_query(fd.photometric_image_u8(img, rec), boxes, masks, 64, 64, flip)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], fd.augment_query(img, boxes, masks, 64, 64, flip)[0])
    plain = fd.augment_query(img, boxes, masks, 64, 64, None)
    for x, y in zip(fd.augment_query_full(img, boxes, masks, 64, 64), plain):          # no rows: resize_query
        assert np.array_equal(x, y)
    gone = np.array([0, 0, 1, 0, -500, 0, 0, 0], np.float64)                          # the box leaves: neither half
    for x, y in zip(fd.augment_query_full(img, boxes, masks, 64, 64, gone, hue), plain):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match='qry_photometric'):                         # its errors, fallback or not
        fd.augment_query_full(img, boxes, masks, 64, 64, gone, (9, 0, 0))


# ---- the loader and the detector's contract -------------------------------------------------------------------------
def test_loader_flag_keys_dtype_collate_and_redraw():
    kw = dict(dataset='MNISTISEG', n_ways=1, k_shots=1, n_imgs=6, img_size=64, spp_img_size=32, raw_uint8=True,
              source_size=80)
    with pytest.raises(ValueError, match='augment_qry'):
        fd.ClutteredCharsFewShotISEG(**kw, photometric_qry=True)
    base = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=True)
    ds = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=True, photometric_qry=True)
    off = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=True, photometric_qry=False)
    for i in range(len(ds)):
        a, b, c = base[i], ds[i], off[i]
        assert list(b) == list(a) + ['qry_photometric'] and list(c) == list(a)
        for k in a:                                                                    # flag off: today's samples
            x, y = a[k], c[k]
            assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(np.asarray(x), np.asarray(y))), k
        assert b['qry_photometric'].dtype == np.float64 and b['qry_photometric'].shape == (3,)
        assert b['qry_augment'].dtype == np.float64 and b['qry_augment'].shape == (8,)
        p, q = fd.draw_query_augment_full(np.random.default_rng([int(ds.seed), int(ds.order[i]), 0]))
        assert np.array_equal(b['qry_augment'], p) and np.array_equal(b['qry_photometric'], q)
        assert np.array_equal(b['qry_photometric'], ds[i]['qry_photometric'])
    batch = collate([ds[i] for i in range(4)])
    assert isinstance(batch['qry_photometric'], torch.Tensor) and tuple(batch['qry_photometric'].shape) == (4, 3)
    assert batch['qry_photometric'].dtype == torch.float64 and tuple(batch['qry_augment'].shape) == (4, 8)
    rows = lambda: np.stack([np.concatenate([ds[i]['qry_augment'], ds[i]['qry_photometric']]) for i in range(len(ds))])
    before = rows()
    ds.reshuffle(e=1)
    after = rows()
    assert not np.array_equal(before, after)                                          # another epoch, another draw
    ds.reshuffle(e=0)
    assert np.array_equal(rows(), before)


def test_the_detector_refuses_the_keyword_where_it_cannot_apply():
    """Host-only contract errors (this test has no GPU): without ``qry_resize_to``, on ``simple_test``; and the ABI
    table declares and binds the new entry."""
    import inspect
    import os
    import re
    from fgn_amd import lib
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    cfg = tiny_config(1, 1, 2)
    m = FGN(1, 1, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'])
    img = torch.zeros((1, 3, 64, 64))
    rows = np.array([[4, 50, 0]], np.float64)
    with pytest.raises(ValueError, match='qry_photometric'):
        m.forward_train(img, [np.zeros((1, 4), np.float32)], [np.zeros(1, np.int64)], [np.zeros((1, 64, 64), bool)],
                        qry_photometric=rows)
    with pytest.raises(ValueError, match='qry_photometric'):
        m.simple_test(img, qry_photometric=rows, rescale=True)
    for fn in (FGN.forward_train, FGN.simple_test, FGN._train_front):
        assert inspect.signature(fn).parameters['qry_photometric'].default is None
    rs = dict(B=2, hw=(64, 64), sizes=[(40, 50), (30, 20)])
    two = np.array([[3, 1, 0], [4, 50, 0]], np.float64)
    recs = FGN._photometric_records(two, rs)
    assert recs.dtype == torch.int32 and tuple(recs.shape) == (2, 64) and recs[:, 2].tolist() == [3, 4]
    assert FGN._photometric_records(np.zeros((2, 3)), rs) is None                      # all neutral: nothing to launch
    for bad in (two[:1], two[:, :2], two.reshape(-1), np.array([[3, 9, 0], [0, 0, 0]], np.float64),
                np.array([[7, 0, 0], [0, 0, 0]], np.float64), np.array([[1, np.nan, 0], [0, 0, 0]], np.float64)):
        with pytest.raises(ValueError, match='qry_photometric'):
            FGN._photometric_records(bad, rs)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgn_hip.h')).read()
    params = re.search(r'\bfgn_photometric_u8hwc3\s*\(([^)]*)\)', header).group(1)
    assert len(lib.SIGNATURES['fgn_photometric_u8hwc3'][1]) == len(params.split(','))
