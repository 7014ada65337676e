"""Source-size query images, host side (no GPU): the integer bilinear rule that ``fewshot_ds`` states and the kernels
of csrc/spatial.hip repeat, ``resize_query`` against base_fst.py:876-887, the dataset's
``source_size`` form and the contract errors of ``qry_resize_to``."""
import hashlib

import numpy as np
import pytest
import torch

from fgn_amd import cluttered_chars as cc
from fgn_amd import fewshot_ds as fd
from fgn_amd import ops
from fgn_amd.lib import FgnHipError

AXES = [(1, 1), (2, 1), (1, 5), (3, 9), (7, 5), (53, 91), (16384, 16383)]
SHAPES = [((37, 53), (64, 91)), ((480, 640), (800, 1066)), ((1200, 1600), (800, 1066)), ((96, 80), (128, 106))]


def _taps_python(n_src, n_dst):
    """The rule of the issue in plain Python integers (unbounded), one destination sample at a time."""
    out = []
    for j in range(n_dst):
        num, den = (2 * j + 1) * n_src - n_dst, 2 * n_dst
        i0 = num // den
        rem = num - i0 * den
        assert 0 <= rem < den
        w1 = (rem * 4096 + den) // (2 * den)
        if i0 < 0:
            w1 = 0
        i1 = min(i0 + 1, n_src - 1)
        i0 = min(max(i0, 0), n_src - 1)
        out.append((i0, i1, 2048 - w1, w1))
    return np.array(out, np.int64).T


@pytest.mark.parametrize('n_src,n_dst', AXES)
def test_resize_taps_equal_the_plain_integer_loop(n_src, n_dst):
    got = fd.resize_taps(n_src, n_dst)
    assert all(a.dtype == np.int32 and a.shape == (n_dst,) for a in got)
    want = _taps_python(n_src, n_dst)
    for g, w in zip(got, want):
        assert np.array_equal(g.astype(np.int64), w)
    i0, i1, w0, w1 = got
    assert (w0 + w1 == 2048).all() and (w1 >= 0).all() and (w1 <= 2048).all()
    assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= n_src - 1).all() and (i1 - i0 <= 1).all()


@pytest.mark.parametrize('n_src,n_dst', [(16384, 16383), (16384, 1), (1, 16384), (16384, 16384), (16383, 16384)])
def test_no_intermediate_reaches_2_31_at_the_largest_dimension(n_src, n_dst):
    """int64 recomputation of every intermediate of the tap rule and of the largest accumulator."""
    j = np.arange(n_dst, dtype=np.int64)
    den = 2 * n_dst
    num = (2 * j + 1) * n_src - n_dst
    i0 = num // den
    rem = num - i0 * den
    w1n = rem * 4096 + den
    # the kernel divides num + den (unsigned) instead of flooring a negative num
    for v in (num, num + den, i0 * den, rem, w1n, 2 * den * np.ones(1, np.int64)):
        assert np.abs(v).max() < 2 ** 31
    assert ((num + den) >= 1).all()
    # the kernel's form gives the same taps: q = (num + den) / den = i0 + 1
    q = (num + den) // den
    assert np.array_equal(q - 1, i0) and np.array_equal(num + den - q * den, rem)
    got = fd.resize_taps(n_src, n_dst)
    assert np.array_equal(got[3].astype(np.int64), np.where(i0 < 0, 0, w1n // (2 * den)))
    assert 255 * 2048 * 2048 + (1 << 21) < 2 ** 31


def test_resize_refuses_dimensions_outside_the_int32_range():
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385), (-1, 4)):
        with pytest.raises(ValueError):
            fd.resize_taps(*bad)
    with pytest.raises(ValueError):
        fd.resize_image_u8(np.zeros((2, 2, 3), np.uint8), 16385, 2)
    with pytest.raises(ValueError):
        fd.resize_masks(np.zeros((1, 2, 2), bool), 2, 0)


def test_resize_image_is_the_identity_at_equal_size():
    rng = np.random.RandomState(0)
    for h, w in ((1, 1), (3, 5), (37, 53)):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(fd.resize_image_u8(img, h, w), img)
        m = rng.rand(2, h, w) > 0.5
        assert np.array_equal(fd.resize_masks(m, h, w), m)


@pytest.mark.parametrize('src,dst', SHAPES)
def test_resize_image_is_within_one_level_of_the_float_bilinear(src, dst):
    rng = np.random.RandomState(src[0])
    img = rng.randint(0, 256, src + (3,)).astype(np.uint8)
    got = fd.resize_image_u8(img, *dst)
    assert got.dtype == np.uint8 and got.shape == dst + (3,) and got.flags['C_CONTIGUOUS']
    for c in range(3):
        ref = cc.resize_nearest_area(img[:, :, c], *dst)
        assert np.abs(got[:, :, c].astype(np.int32) - ref.astype(np.int32)).max() <= 1


def test_2x2_to_1x1_is_the_rounded_mean():
    rng = np.random.RandomState(3)
    for _ in range(64):
        img = rng.randint(0, 256, (2, 2, 3)).astype(np.uint8)
        want = (img.astype(np.int32).sum((0, 1)) + 2) >> 2
        assert np.array_equal(fd.resize_image_u8(img, 1, 1)[0, 0], want.astype(np.uint8))


def test_mask_2_to_1_downscale_is_at_least_half_set():
    rng = np.random.RandomState(5)
    m = rng.rand(3, 24, 34) > 0.5
    got = fd.resize_masks(m, 12, 17)
    want = m.reshape(3, 12, 2, 17, 2).sum((2, 4)) >= 2
    assert got.dtype == bool and np.array_equal(got, want)
    # nonzero bytes other than 1 count as set; no masks -> no masks
    assert np.array_equal(fd.resize_masks(m.astype(np.uint8) * 200, 12, 17), want)
    assert fd.resize_masks(np.zeros((0, 24, 34), bool), 12, 17).shape == (0, 12, 17)


def test_resize_query_boxes_masks_and_passthrough():
    rng = np.random.RandomState(9)
    h, w, H, W = 37, 53, 64, 91
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    masks = rng.rand(2, h, w) > 0.6
    boxes = np.array([[1.5, 2.25, 30.0, 50.75], [0.0, 0.0, 37.0, 53.0]], np.float32)
    keep = boxes.copy()
    img2, boxes2, masks2 = fd.resize_query(img, boxes, masks, H, W)
    # base_fst.py:877-878 in float32: the array times the Python float, rows 0, 2 and 1, 3
    want = keep.copy()
    want[:, [0, 2]] = want[:, [0, 2]] * (H / h)
    want[:, [1, 3]] = want[:, [1, 3]] * (W / w)
    assert boxes2.dtype == np.float32 and np.array_equal(boxes2.view(np.int32), want.view(np.int32))
    assert np.array_equal(boxes, keep)                                  # the caller's boxes are not written
    assert np.array_equal(img2, fd.resize_image_u8(img, H, W)) and np.array_equal(masks2, fd.resize_masks(masks, H, W))
    same = fd.resize_query(img, boxes, masks, h, w)
    assert same[0] is img and same[1] is boxes and same[2] is masks     # nothing copied, nothing changed


KEYS = ['idx', 'qry_child_idx', 'qry_img', 'qry_cat_ids_real', 'qry_cat_ids', 'qry_bboxes', 'qry_isegmaps', 'spp_imgs',
        'spp_bboxes', 'spp_isegmaps', 'cats_ids_to_sample_real', 'cats_ids_to_sample', 'spp_insts_ids', 'img_shape']
# sha256 over the query side of samples 0, 3, 5 as the dataset produced them before ``source_size`` existed
PINNED = {False: 'a2d00bff66b5a4284e636a785681a8e05dd50b63ffbdf079036465775d908211',
          True: '970b15da30c8859636f23afde59a2baca860d1ac8071c380ab0fee4561073b45'}


@pytest.mark.parametrize('raw', [False, True])
def test_dataset_without_source_size_is_unchanged(raw):
    kw = dict(dataset='MNISTISEG', n_ways=3, k_shots=2, n_imgs=6, img_size=96, spp_img_size=48, seed=7, raw_uint8=raw)
    ds, ds_none = fd.ClutteredCharsFewShotISEG(**kw), fd.ClutteredCharsFewShotISEG(**kw, source_size=None)
    digest = hashlib.sha256()
    for idx in (0, 3, 5):
        s, t = ds[idx], ds_none[idx]
        assert list(s) == KEYS == list(t)
        for k in KEYS:
            a, b = np.asarray(s[k]), np.asarray(t[k])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        for k in ('qry_img', 'qry_cat_ids_real', 'qry_cat_ids', 'qry_bboxes', 'qry_isegmaps', 'cats_ids_to_sample_real',
                  'spp_insts_ids', 'img_shape'):
            a = np.ascontiguousarray(np.asarray(s[k]))
            for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
                digest.update(part)
    assert digest.hexdigest() == PINNED[raw]


def test_dataset_source_size_samples():
    kw = dict(dataset='MNISTISEG', n_ways=3, k_shots=2, n_imgs=6, img_size=96, spp_img_size=48, seed=7)
    with pytest.raises(ValueError):
        fd.ClutteredCharsFewShotISEG(**kw, source_size=120)                     # needs raw_uint8
    ds = fd.ClutteredCharsFewShotISEG(**kw, raw_uint8=True, source_size=120)
    s = ds[2]
    assert list(s) == KEYS + ['qry_resize_to']
    assert s['qry_img'].dtype == torch.uint8 and tuple(s['qry_img'].shape) == (120, 120, 3)
    assert s['qry_isegmaps'].shape[1:] == (120, 120) and s['qry_isegmaps'].dtype == bool
    assert np.array_equal(s['qry_resize_to'], [96, 96]) and np.array_equal(s['img_shape'], [96, 96, 3])
    assert tuple(s['spp_imgs'].shape) == (6, 48, 48, 3)
    assert s['qry_bboxes'].max() > 96 * 0.6 and s['qry_bboxes'].max() <= 120    # source-size coordinates
    # the host route gives a network-size sample
    img, boxes, masks = fd.resize_query(s['qry_img'].numpy(), s['qry_bboxes'], s['qry_isegmaps'], *s['qry_resize_to'])
    assert img.shape == (96, 96, 3) and masks.shape[1:] == (96, 96) and boxes.max() <= 96


def test_resize_ops_have_no_cpu_fallback():
    with pytest.raises(FgnHipError):
        ops.resize_u8_to_nhwc4(torch.zeros((1, 12), dtype=torch.uint8), torch.tensor([[2, 2]], dtype=torch.int32),
                               torch.zeros((3, 256)), 4, 4)
    with pytest.raises(FgnHipError):
        ops.resize_masks(torch.zeros((1, 2, 2), dtype=torch.bool), 4, 4)


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(3, 2, width_div=2)
    return FGN(3, 2, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def test_qry_resize_to_contract_is_checked_on_the_host():
    """Every contract error is a ValueError raised before the GPU is looked for (this test runs without one)."""
    m = _model()
    assert m.query_source_capacity == 3 * 2_000_000
    u8 = torch.zeros((2, 20, 30, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match='set_input_norm'):
        m._source_query(u8, (32, 32), None)                                                   # no table
    m.set_input_norm(**fd.ClutteredCharsFewShotISEG(n_imgs=1, img_size=64, spp_img_size=32).input_norm)
    rs = m._source_query(u8, (32, 48), None)
    assert rs['B'] == 2 and rs['hw'] == (32, 48) and rs['sizes'] == [(20, 30)] * 2 and rs['capacity'] == 1800
    assert np.array_equal(rs['img_shape'], [[32, 48, 3]] * 2) and [f.numel() for f in rs['flats']] == [1800] * 2
    rs = m._source_query([u8[0], u8[1, :10, :7]], torch.tensor([[32, 48], [32, 48]]), [(32, 48, 3)] * 2, graphed=True)
    assert rs['sizes'] == [(20, 30), (10, 7)] and rs['capacity'] == m.query_source_capacity
    assert rs['flats'][1].numel() == 210 and rs['flats'][1].is_contiguous()
    for bad in (dict(qry_img=u8.float()), dict(qry_img=u8.permute(0, 3, 1, 2).contiguous()),    # float, NCHW
                dict(qry_img=[u8[0], u8[1].float()]), dict(img_shape=[(32, 32, 3), (32, 48, 3)]),
                dict(qry_resize_to=torch.tensor([[32, 48], [32, 32]])), dict(qry_resize_to=(32,)),
                dict(qry_resize_to=(0, 48)), dict(qry_resize_to=(32, 16385)),
                dict(qry_isegmaps=[np.zeros((1, 20, 30), bool), np.zeros((1, 32, 48), bool)])):
        args = dict(qry_img=u8, qry_resize_to=(32, 48), img_shape=None)
        args.update(bad)
        with pytest.raises(ValueError):
            m._source_query(**args)
    m.query_source_capacity = 1799
    with pytest.raises(ValueError, match='query_source_capacity'):
        m._source_query(u8, (32, 48), None, graphed=True)
    assert m._source_query(u8, (32, 48), None)['capacity'] == 1800                            # eager: what the batch needs
    # through the public entries: refused before anything else happens
    for call in (m.simple_test, m.forward_train):
        with pytest.raises(ValueError):
            call(qry_img=u8.float(), qry_bboxes=None, qry_cat_ids=None, qry_isegmaps=None, qry_resize_to=(32, 48))
    assert m._graphs == {}


def test_scaled_boxes_follow_resize_query():
    m = _model()
    boxes = [np.array([[1.5, 2.25, 19.0, 29.75]], np.float32), torch.tensor([[0.5, 1.0, 9.5, 6.25]])]
    keep = [np.asarray(b).copy() for b in boxes]
    got = m._scaled_boxes(boxes, [(20, 30), (32, 48)], (32, 48))
    want = fd.resize_query(np.zeros((20, 30, 3), np.uint8), boxes[0], np.zeros((0, 20, 30), bool), 32, 48)[1]
    assert np.array_equal(got[0].view(np.int32), want.view(np.int32))
    assert got[1] is boxes[1]                                                                 # equal size: untouched
    assert all(np.array_equal(np.asarray(b), k) for b, k in zip(boxes, keep))
    t = m._scaled_boxes([torch.from_numpy(keep[0])], [(20, 30)], (32, 48))[0]
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy().view(np.int32), want.view(np.int32))
