"""Supports from the source image, host side: the integer bicubic rule of ``fgn_amd.fewshot_ds``
(``cubic_taps``), the geometry record (``support_geometry``) and the gather (``support_from_source``) - against a plain
Python-int loop, against ``get_crop``'s own (golden-pinned) output and against the float ``support_from_instance``; the
contract of ``spp_crop_to``; the dataset switch.  No GPU."""
import numpy as np
import pytest
import torch

from fgn_amd import cluttered_chars as cc
from fgn_amd import episodes
from fgn_amd import fewshot_ds as fd
from fgn_amd import ops
from fgn_amd.lib import FgnHipError

AXES = [(1, 1), (1, 9), (7, 7), (5, 64), (150, 16), (40, 33), (33, 40), (2, 300), (16384, 3), (3, 16384), (16384, 16383)]


def _taps_loop(n_src, n_dst):
    """``cubic_taps`` in Python ints, one destination sample at a time, as DESIGN 4.4.4 states the rule."""
    idx, W = [], []
    for j in range(n_dst):
        num, den = (2 * j + 1) * n_src - n_dst, 2 * n_dst
        i0 = num // den
        rem = num - i0 * den
        assert 0 <= rem < den
        u = (rem * 2048 + den) // (2 * den)
        v = 1024 - u
        w_m1, w_p2 = -3 * u * v * v, -3 * u * u * v
        w_0, w_p1 = 5 * u ** 3 - 9216 * u ** 2 + 2 ** 32, 5 * v ** 3 - 9216 * v ** 2 + 2 ** 32
        assert w_m1 + w_0 + w_p1 + w_p2 == 2 ** 32
        W_m1, W_p1, W_p2 = (w_m1 + 2 ** 20) >> 21, (w_p1 + 2 ** 20) >> 21, (w_p2 + 2 ** 20) >> 21
        W.append([W_m1, 2048 - W_m1 - W_p1 - W_p2, W_p1, W_p2])
        idx.append([min(max(i0 + k, 0), n_src - 1) for k in (-1, 0, 1, 2)])
    return np.array(idx), np.array(W)


@pytest.mark.parametrize('n_src,n_dst', [a for a in AXES if a[1] <= 300])
def test_cubic_taps_equal_the_plain_integer_loop(n_src, n_dst):
    idx, W = fd.cubic_taps(n_src, n_dst)
    want_idx, want_W = _taps_loop(n_src, n_dst)
    assert idx.dtype == W.dtype == np.int32 and idx.shape == W.shape == (n_dst, 4)
    assert np.array_equal(idx, want_idx) and np.array_equal(W, want_W)


@pytest.mark.parametrize('n_src,n_dst', AXES)
def test_cubic_weights_sum_to_2048_and_their_magnitudes_to_at_most_2816(n_src, n_dst):
    idx, W = fd.cubic_taps(n_src, n_dst)
    assert (W.sum(1) == 2048).all()
    assert np.abs(W).sum(1).max() <= fd.CUBIC_ABS_SUM == 2816
    assert idx.min() >= 0 and idx.max() <= n_src - 1 and (np.diff(idx, axis=1) >= 0).all()


def test_every_fraction_gives_weights_inside_the_bound():
    """All 1025 values of u, straight from the formulas: the bound on the magnitudes does not depend on which sizes a
    test happens to try; the widest 2^-32 intermediate needs 34 bits (so the kernel computes them in int64)."""
    u = np.arange(1025, dtype=np.int64)
    v = 1024 - u
    w = np.stack([-3 * u * v * v, 5 * u ** 3 - 9216 * u ** 2 + 2 ** 32, 5 * v ** 3 - 9216 * v ** 2 + 2 ** 32, -3 * u * u * v])
    assert (w.sum(0) == 2 ** 32).all() and w.min() >= -2 ** 31 and w.max() == 2 ** 32
    assert max(np.abs(5 * u ** 3).max(), np.abs(9216 * u ** 2).max()) < 2 ** 34
    W = (w + 2 ** 20) >> 21
    W[1] = 2048 - W[0] - W[2] - W[3]
    assert np.abs(W).sum(0).max() == 2816                   # at u = 512: (-192, 1216, 1216, -192)
    assert np.abs(W[1] - ((w[1] + 2 ** 20) >> 21)).max() <= 1       # the remainder weight is the rounded one or next to it


@pytest.mark.parametrize('n_src,n_dst', [(16384, 16384), (16384, 1), (1, 16384), (16383, 16384)])
def test_no_intermediate_leaves_its_declared_width_at_the_largest_dimension(n_src, n_dst):
    """The kernel's widths, recomputed in int64: num + den and rem * 2048 + den in uint32 (below 2^30 and 2^27), a row
    sum of four bytes in int32 (<= 255 * 2816), the accumulator in int32 (<= 255 * 2816^2 < 2^31)."""
    j = np.arange(n_dst, dtype=np.int64)
    den = 2 * n_dst
    nump = (2 * j + 1) * n_src + n_dst
    assert nump.min() >= 1 and nump.max() < 2 ** 30
    rem = nump - (nump // den) * den
    assert (rem * 2048 + den).max() < 2 ** 27
    _, W = fd.cubic_taps(n_src, n_dst)
    assert 255 * int(np.abs(W).sum(1).max()) <= 255 * 2816 < 2 ** 20
    assert 255 * 2816 ** 2 < 2 ** 31


def test_cubic_taps_refuse_dimensions_outside_1_to_16384():
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385), (-1, 4)):
        with pytest.raises(ValueError):
            fd.cubic_taps(*bad)


def test_the_rule_is_the_identity_at_equal_size():
    idx, W = fd.cubic_taps(9, 9)
    assert np.array_equal(W, [[0, 2048, 0, 0]] * 9) and np.array_equal(idx[:, 1], np.arange(9))
    # a box whose crop is exactly S x S: 8 x 8 (zero offsets: floor(8 * 0.12) = 0, even extents: no parity pixel)
    rs = np.random.RandomState(0)
    img, m = rs.randint(0, 256, (12, 14, 3)).astype(np.uint8), rs.rand(12, 14) > 0.5
    crop, box, mask = fd.support_from_source(img, [2, 3, 10, 11], m, 8)
    assert np.array_equal(crop, img[2:10, 3:11]) and np.array_equal(mask, m[2:10, 3:11])
    assert np.array_equal(box, np.array([0, 0, 8, 8], np.float32))


def test_reflect_index_is_numpy_reflect_padding_for_pads_beyond_the_axis():
    for n in (1, 2, 3, 6, 40):
        a = np.arange(n)
        for pad in (0, 1, n, 3 * n + 2, 21):
            want = np.pad(a, (pad, pad + 1), mode='reflect')
            assert np.array_equal(fd.reflect_index(np.arange(-pad, n + pad + 1), n), want), (n, pad)


# ---- the gather against get_crop's own output ----------------------------------------------------------------------
def _int_resize(planes: np.ndarray, nh: int, nw: int) -> np.ndarray:
    """[h,w,c] bytes -> int64 accumulators [nh,nw,c] of the rule on a crop that EXISTS (taps clamped into it)."""
    iy, wy = fd.cubic_taps(planes.shape[0], nh)
    ix, wx = fd.cubic_taps(planes.shape[1], nw)
    p = planes.astype(np.int64)
    acc = np.zeros((nh, nw, planes.shape[2]), np.int64)
    for a in range(4):
        for b in range(4):
            acc += p[iy[:, a]][:, ix[:, b]] * (wy[:, a].astype(np.int64)[:, None, None] * wx[:, b][None, :, None])
    return acc


def _via_get_crop(img, bbox, mask, S, fill=0.8, crop_square=True):
    """``support_from_instance`` with its float ``_resize`` replaced by the integer rule: get_crop -> resize -> pad."""
    ymin, xmin, ymax, xmax = np.array(bbox).astype(np.int32)
    r = fd.spp_offset_ratio(fill)
    w_off, h_off = int(np.floor((xmax - xmin) * r)), int(np.floor((ymax - ymin) * r))
    crop, _ = fd.get_crop(img, ymin, xmin, ymax, xmax, h_off, w_off, crop_square=crop_square)
    mcrop, _ = fd.get_crop(mask[:, :, None], ymin, xmin, ymax, xmax, h_off, w_off, crop_square=crop_square,
                           mode='constant')
    ch, cw = crop.shape[:2]
    nh, nw = (S, max(1, int(np.round(S * cw / ch)))) if ch >= cw else (max(1, int(np.round(S * ch / cw))), S)
    top, left = (S - nh) // 2, (S - nw) // 2
    out, m = np.zeros((S, S, 3), np.uint8), np.zeros((S, S), bool)
    out[top:top + nh, left:left + nw] = np.clip((_int_resize(crop, nh, nw) + 2 ** 21) >> 22, 0, 255)
    m[top:top + nh, left:left + nw] = _int_resize(mcrop.astype(np.uint8), nh, nw)[:, :, 0] > 2 ** 21
    return out, m, (ch, cw, nh, nw, top, left)


def _scene(h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.rand(h, w) > 0.4


# (image size, box YXYX, S): a 6x40 image (pads of 21 rows on 6: several reflections), a 1x1 image, boxes
# touching every border and all of them, odd and even extents, up- and downscale, tall and wide, zero offsets
GATHER_CASES = [((6, 40), [0, 0, 6, 40], 32), ((6, 40), [1, 3, 5, 38], 32), ((6, 40), [0, 0, 1, 1], 32),
                ((1, 1), [0, 0, 1, 1], 16), ((1, 1), [0, 0, 1, 1], 1),
                ((50, 60), [0, 10, 21, 30], 16), ((50, 60), [29, 10, 50, 33], 16), ((50, 60), [10, 0, 30, 17], 33),
                ((50, 60), [10, 41, 31, 60], 33), ((50, 60), [0, 0, 50, 60], 16), ((50, 60), [20, 20, 25, 27], 33),
                ((50, 60), [20, 20, 29, 60], 16), ((180, 170), [10, 5, 160, 131], 16), ((9, 9), [4, 4, 5, 5], 7),
                ((30, 30), [3.7, 2.2, 20.9, 11.5], 24)]


@pytest.mark.parametrize('crop_square', [True, False])
@pytest.mark.parametrize('hw,box,S', GATHER_CASES)
def test_support_from_source_is_bitwise_the_integer_resize_of_get_crop(hw, box, S, crop_square):
    img, mask = _scene(*hw, seed=hw[0] + S)
    want_img, want_m, (ch, cw, nh, nw, top, left) = _via_get_crop(img, box, mask, S, crop_square=crop_square)
    got_img, got_box, got_m = fd.support_from_source(img, box, mask, S, crop_square=crop_square)
    assert got_img.dtype == np.uint8 and got_m.dtype == bool and got_box.dtype == np.float32
    assert np.array_equal(got_img, want_img) and np.array_equal(got_m, want_m)
    ref = fd.support_from_instance(img, box, mask, S, crop_square=crop_square)
    assert got_box.tobytes() == ref[1].tobytes()
    rec, gbox = fd.support_geometry(hw[0], hw[1], box, S, crop_square=crop_square)
    g = dict(zip(fd.SPP_REC_FIELDS, rec.tolist()))
    assert rec.dtype == np.int32 and rec.shape == (fd.SPP_REC_INTS,) and gbox.tobytes() == got_box.tobytes()
    assert (g['H'], g['W'], g['ch'], g['cw'], g['nh'], g['nw'], g['top'], g['left']) == (*hw, ch, cw, nh, nw, top, left)
    assert max(nh, nw) == S
    # the padding is zero and empty
    pad = np.ones((S, S), bool)
    pad[top:top + nh, left:left + nw] = False
    assert not got_img[pad].any() and not got_m[pad].any()


@pytest.mark.parametrize('crop_square', [True, False])
@pytest.mark.parametrize('hw,box,S', GATHER_CASES)
def test_every_tap_lies_inside_the_window_of_support_geometry(hw, box, S, crop_square):
    rec, _ = fd.support_geometry(hw[0], hw[1], box, S, crop_square=crop_square)
    g = dict(zip(fd.SPP_REC_FIELDS, rec.tolist()))
    assert 0 <= g['wy'] and g['wy'] + g['wh'] <= hw[0] and 0 <= g['wx'] and g['wx'] + g['ww'] <= hw[1]
    assert g['wh'] >= 1 and g['ww'] >= 1
    for o, n_crop, n_dst, n, lo, ln in ((g['y0'], g['ch'], g['nh'], hw[0], g['wy'], g['wh']),
                                        (g['x0'], g['cw'], g['nw'], hw[1], g['wx'], g['ww'])):
        t = fd.cubic_taps(n_crop, n_dst)[0].astype(np.int64) + o
        src = fd.reflect_index(t, n) if g['reflect'] else t[(t >= 0) & (t < n)]
        assert src.min() >= lo and src.max() < lo + ln
    # the window is all the function reads: everything outside it may change
    img, mask = _scene(*hw, seed=3)
    want = fd.support_from_source(img, box, mask, S, crop_square=crop_square)
    keep = np.zeros(hw, bool)
    keep[g['wy']:g['wy'] + g['wh'], g['wx']:g['wx'] + g['ww']] = True
    img2, mask2 = np.where(keep[:, :, None], img, 255 - img).astype(np.uint8), np.where(keep, mask, ~mask)
    got = fd.support_from_source(img2, box, mask2, S, crop_square=crop_square)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    iw, mw = fd.support_window(img, mask, rec)
    assert iw.shape == (g['wh'], g['ww'], 3) and mw.shape == (g['wh'], g['ww']) and mw.dtype == np.uint8
    assert iw.flags.c_contiguous and mw.flags.c_contiguous and set(np.unique(mw)) <= {0, 1}


def test_reflect_mode_follows_get_crop():
    """get_crop pads by zeros only for crop_square=False WITH an offset; zero offsets (extents below 9) keep reflect."""
    assert fd.support_geometry(50, 60, [10, 10, 30, 30], 16, crop_square=True)[0][10] == 1
    assert fd.support_geometry(50, 60, [10, 10, 30, 30], 16, crop_square=False)[0][10] == 0
    assert fd.support_geometry(50, 60, [10, 10, 15, 17], 16, crop_square=False)[0][10] == 1


def test_support_geometry_refuses_boxes_outside_or_empty_and_large_sizes():
    for bad in ([0, 0, 0, 5], [3, 3, 3, 9], [5, 5, 4, 9], [-1, 0, 5, 5], [0, -1, 5, 5], [0, 0, 11, 5], [0, 0, 5, 13],
                [2.2, 1, 2.9, 5]):                                                  # (the last: empty once truncated)
        with pytest.raises(ValueError):
            fd.support_geometry(10, 12, bad, 16)
    for H, W, S in ((0, 5, 8), (5, 16385, 8), (5, 5, 0), (5, 5, 16385)):
        with pytest.raises(ValueError):
            fd.support_geometry(H, W, [0, 0, 1, 1], S)
    with pytest.raises(ValueError):                                                 # the crop with its context
        fd.support_geometry(16384, 16384, [0, 0, 16384, 16384], 8)
    with pytest.raises(ValueError):
        fd.support_from_source(np.zeros((4, 4, 3), np.float32), [0, 0, 2, 2], np.zeros((4, 4), bool), 8)
    with pytest.raises(ValueError):
        fd.support_from_source(np.zeros((4, 4, 3), np.uint8), [0, 0, 2, 2], np.zeros((4, 5), bool), 8)


# ---- against the float path ------------------------------------------------------------------------------------------
def test_against_support_from_instance_on_the_character_images():
    """Every instance of six 160^2 character images at S = 16 and 64: boxes bit-equal, image bytes within one grey level,
    at most 0.1 % of the mask pixels differing (measured when the rule was written: 0.19 % of the bytes differ, by 1; 0 of
    78 336 mask pixels)."""
    worst, n_diff, n_bytes, m_diff, m_pix = 0, 0, 0, 0, 0
    for seed in range(6):
        im = cc.make_image(seed, 160, np.arange(10))
        for o in range(len(im['cat_ids'])):
            for S in (16, 64):
                a = fd.support_from_instance(im['img'], im['bboxes'][o], im['isegmaps'][o], S)
                b = fd.support_from_source(im['img'], im['bboxes'][o], im['isegmaps'][o], S)
                assert a[1].tobytes() == b[1].tobytes()
                d = np.abs(a[0].astype(np.int32) - b[0].astype(np.int32))
                worst, n_diff, n_bytes = max(worst, int(d.max())), n_diff + int((d > 0).sum()), n_bytes + d.size
                m_diff, m_pix = m_diff + int((a[2] != b[2]).sum()), m_pix + a[2].size
    print(f'bytes differing {n_diff} / {n_bytes} (max {worst}), mask pixels differing {m_diff} / {m_pix}')
    assert worst <= 1
    assert m_diff <= 0.001 * m_pix


@pytest.mark.parametrize('crop_square', [True, False])
def test_against_support_from_instance_on_the_6x40_image(crop_square):
    img, mask = _scene(6, 40, seed=5)
    for box in ([0, 0, 6, 40], [1, 3, 5, 38], [0, 0, 1, 1]):
        a = fd.support_from_instance(img, box, mask, 32, crop_square=crop_square)
        b = fd.support_from_source(img, box, mask, 32, crop_square=crop_square)
        assert a[1].tobytes() == b[1].tobytes()
        assert np.abs(a[0].astype(np.int32) - b[0].astype(np.int32)).max() <= 1
        assert (a[2] != b[2]).sum() <= 0.001 * a[2].size


# ---- contract, dataset -----------------------------------------------------------------------------------------------
def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(3, 2, width_div=2)
    return FGN(3, 2, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _six(seed=0, sizes=((40, 50), (30, 30), (64, 20), (40, 50), (25, 70), (33, 33))):
    rs = np.random.RandomState(seed)
    imgs = [torch.from_numpy(rs.randint(0, 256, s + (3,)).astype(np.uint8)) for s in sizes]
    masks = [rs.rand(*s) > 0.5 for s in sizes]
    boxes = np.array([[2, 3, s[0] - 4, s[1] - 5] for s in sizes], np.float32)
    return imgs, boxes, masks


def test_spp_crop_to_contract_is_checked_on_the_host():
    """Every contract error is a ValueError raised before the GPU is looked for (this test runs without one)."""
    m = _model()
    assert m.support_source_capacity == 3 * 640 * 640
    imgs, boxes, masks = _six()
    with pytest.raises(ValueError, match='set_input_norm'):
        m._source_supports(imgs, boxes, masks, 32)                                             # no table
    m.set_input_norm(**fd.ClutteredCharsFewShotISEG(n_imgs=1, img_size=64, spp_img_size=32).input_norm)
    sp = m._source_supports(imgs, boxes, masks, 32)
    assert (sp['B'], sp['n'], sp['S']) == (1, 6, 32) and tuple(sp['rec'].shape) == (6, 16) and sp['rec'].dtype == torch.int32
    assert tuple(sp['boxes'].shape) == (1, 6, 4) and sp['boxes'].dtype == torch.float32
    for i in range(6):
        rec, box = fd.support_geometry(*imgs[i].shape[:2], boxes[i], 32)
        assert np.array_equal(sp['rec'][i].numpy(), rec) and sp['boxes'][0, i].numpy().tobytes() == box.tobytes()
        iw, mw = fd.support_window(imgs[i].numpy(), masks[i], rec)
        assert sp['flats'][i].dtype == sp['mflats'][i].dtype == torch.uint8 and sp['flats'][i].is_contiguous()
        assert np.array_equal(sp['flats'][i].numpy(), iw.reshape(-1))
        assert np.array_equal(sp['mflats'][i].numpy(), mw.reshape(-1))
    assert sp['capacity'] == sp['need'] == max(f.numel() for f in sp['flats'])
    assert sp['mcapacity'] == sp['mneed'] == max(f.numel() for f in sp['mflats']) and 3 * sp['mneed'] == sp['need']
    assert sp['need'] <= 3 * 64 * 70
    assert sp['window_bytes'] == sum(f.numel() for f in sp['flats'] + sp['mflats'])
    # B lists, tensors or arrays alike; under graphs the slot is the attribute
    sp2 = m._source_supports([imgs, imgs], np.stack([boxes, boxes]), [masks, [torch.from_numpy(k) for k in masks]], 32,
                             graphed=True)
    assert (sp2['B'], sp2['n']) == (2, 12) and sp2['capacity'] == m.support_source_capacity
    assert sp2['mcapacity'] == m.support_source_capacity // 3 and sp2['need'] == sp['need'] and len(sp2['flats']) == 12
    outside = boxes.copy()
    outside[2, 2] = 65
    for bad in (dict(spp_imgs=[t.float() for t in imgs]),                                      # float images
                dict(spp_imgs=[t.permute(2, 0, 1).contiguous() for t in imgs]),                # CHW
                dict(spp_imgs=torch.zeros((6, 32, 32, 3), dtype=torch.uint8)),                 # ready crops, no list
                dict(spp_imgs=imgs[:5]), dict(spp_isegmaps=masks[:5]), dict(spp_bboxes=boxes[:5]),
                dict(spp_isegmaps=[masks[1]] + masks[1:]),                                     # a mask at another size
                dict(spp_bboxes=outside), dict(spp_crop_to=(32, 32)), dict(spp_crop_to=32.0), dict(spp_crop_to=0),
                dict(spp_crop_to=True), dict(spp_crop_to=16385), dict(spp_imgs=[imgs], spp_isegmaps=masks)):
        args = dict(spp_imgs=imgs, spp_bboxes=boxes, spp_isegmaps=masks, spp_crop_to=32)
        args.update(bad)
        with pytest.raises(ValueError):
            m._source_supports(**args)
    m.support_source_capacity = sp['need'] - 1
    with pytest.raises(ValueError, match='support_source_capacity'):
        m._source_supports(imgs, boxes, masks, 32, graphed=True)
    assert m._source_supports(imgs, boxes, masks, 32)['capacity'] == sp['need']                # eager: what the batch needs
    # through the public entries: refused before anything else happens
    qry = torch.zeros((1, 64, 64, 3), dtype=torch.uint8)
    for call in (lambda **kw: m.simple_test(qry_img=qry, **kw), lambda **kw: m.detect_device(qry, img_shape=None, **kw),
                 lambda **kw: m.encode_supports(**kw),
                 lambda **kw: m.forward_train(qry_img=qry, qry_bboxes=None, qry_cat_ids=None, qry_isegmaps=None, **kw)):
        with pytest.raises(ValueError):
            call(spp_imgs=[t.float() for t in imgs], spp_bboxes=boxes, spp_isegmaps=masks, spp_crop_to=32)
    assert m._graphs == {}


def test_support_op_has_no_cpu_fallback():
    with pytest.raises(FgnHipError):
        ops.support_from_source(torch.zeros((1, 12), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.uint8),
                                torch.zeros((1, 16), dtype=torch.int32), torch.zeros((3, 256)), 4)


@pytest.mark.parametrize('raw', [False, True])
def test_dataset_without_spp_source_is_unchanged(raw):
    kw = dict(dataset='MNISTISEG', n_ways=3, k_shots=2, n_imgs=6, img_size=96, spp_img_size=48, seed=7, raw_uint8=raw)
    ds, ds_off = fd.ClutteredCharsFewShotISEG(**kw), fd.ClutteredCharsFewShotISEG(**kw, spp_source=False)
    for idx in (0, 3, 5):
        s, t = ds[idx], ds_off[idx]
        assert list(s) == list(t) and 'spp_crop_to' not in s
        for k in s:
            a, b = np.asarray(s[k]), np.asarray(t[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        # ... and what they always were: the supports are support_from_instance's crops
        assert tuple(s['spp_imgs'].shape)[:1] == (6,) and s['spp_isegmaps'].shape == (6, 48, 48)


def test_dataset_spp_source_samples_and_collate():
    kw = dict(dataset='MNISTISEG', n_ways=3, k_shots=2, n_imgs=6, img_size=96, spp_img_size=48, seed=7)
    with pytest.raises(ValueError):
        fd.ClutteredCharsFewShotISEG(**kw, spp_source=True)                     # needs raw_uint8
    host = fd.ClutteredCharsFewShotISEG(**kw, raw_uint8=True)
    ds = fd.ClutteredCharsFewShotISEG(**kw, raw_uint8=True, spp_source=True)
    s, h = ds[2], host[2]
    assert list(s) == list(h) + ['spp_crop_to', 'spp_fill_ratio', 'crop_square']
    assert s['spp_crop_to'] == 48 and s['spp_fill_ratio'] == 0.8 and s['crop_square'] is True
    assert isinstance(s['spp_imgs'], list) and len(s['spp_imgs']) == len(s['spp_isegmaps']) == 6
    assert s['spp_bboxes'].shape == (6, 4) and s['spp_bboxes'].dtype == np.float32
    assert np.array_equal(s['spp_insts_ids'], h['spp_insts_ids'])
    for i in range(6):                          # the host's crop of the same instance, by the float and the integer rule
        im, mk = s['spp_imgs'][i], s['spp_isegmaps'][i]
        assert im.dtype == torch.uint8 and tuple(im.shape) == (96, 96, 3) and mk.shape == (96, 96) and mk.dtype == bool
        crop, box, mask = fd.support_from_instance(im.numpy(), s['spp_bboxes'][i], mk, 48)
        assert np.array_equal(crop, h['spp_imgs'][i].numpy()) and np.array_equal(mask, h['spp_isegmaps'][i])
        assert box.tobytes() == h['spp_bboxes'][i].tobytes()
    for k in h:
        if k not in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps'):
            assert np.asarray(s[k]).tobytes() == np.asarray(h[k]).tobytes(), k
    batch = episodes.collate([ds[0], ds[1]])
    assert batch['spp_crop_to'] == 48 and batch['crop_square'] is True and batch['spp_fill_ratio'] == 0.8
    assert len(batch['spp_imgs']) == 2 and len(batch['spp_imgs'][0]) == 6 and batch['spp_imgs'][1][3].dtype == torch.uint8
    assert batch['spp_isegmaps'][0][0].dtype == torch.bool and tuple(batch['spp_bboxes'].shape) == (2, 6, 4)
    sp = _model_with_norm(ds)._source_supports(batch['spp_imgs'], batch['spp_bboxes'], batch['spp_isegmaps'],
                                               batch['spp_crop_to'], batch['spp_fill_ratio'], batch['crop_square'])
    assert (sp['B'], sp['n'], sp['S']) == (2, 12, 48)
    # without the switch collate does what it did
    old = episodes.collate([host[0], host[1]])
    assert tuple(old['spp_imgs'].shape) == (2, 6, 48, 48, 3) and 'spp_crop_to' not in old


def _model_with_norm(ds):
    m = _model()
    m.set_input_norm(**ds.input_norm)
    return m
