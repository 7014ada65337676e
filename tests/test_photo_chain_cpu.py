"""Chains of photometric operators on the host (no GPU): the records are the existing records compacted, the rule is the
left fold of ``photometric_image_u8``; known answers; the structural rule and its refusals; the commutation of HSV + blur
chains with a horizontal flip (why COCO's flip-first order and the project's flip-last order give one image); the draw
``draw_coco_augment``; the loader's ``augs`` flag; the detector's host-only contract; the ABI table."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

HUE, SAT, BRI, GAUSS, IMPULSE, BLUR, NONE = (4, -37.5, 0), (5, 60.25, 0), (6, -100.5, 0), (1, 2.0, 1234), (2, 0.3, 77), \
    (3, 1.5, 0), (0, 0, 0)


def _pixels(hw, seed):
    img = np.random.RandomState(seed).randint(0, 256, size=tuple(hw) + (3,), dtype=np.uint8)
    img.reshape(-1, 3)[::7] = (0, 255, 255)
    img.reshape(-1, 3)[3::11] = 128
    return img


# ---- records and the fold ---------------------------------------------------------------------------------------------
def test_the_records_are_the_existing_records_compacted():
    src, net = (37, 53), (64, 96)
    assert fd.PHOTO_CHAIN_MAX == 3
    neutral = fd.query_photometric_record(None, src, net)
    for chain in ([HUE, BLUR], [NONE, GAUSS, BLUR], [HUE, NONE, BRI], [SAT, (3, 0, 0)], [NONE], [BLUR], [GAUSS, HUE, BLUR],
                  [(6, 0, 5), IMPULSE, NONE]):
        recs = fd.photometric_chain_records(chain, src, net)
        assert recs.dtype == np.int32 and recs.shape == (3, 64)
        active = [fd.query_photometric_record(r, src, net) for r in chain
                  if not fd.photometric_is_neutral(np.asarray(r, np.float64))]
        for i in range(3):
            assert np.array_equal(recs[i], active[i] if i < len(active) else neutral), (chain, i)
    assert np.array_equal(fd.photometric_chain_records(None, src, net), np.tile(neutral, (3, 1)))
    assert np.array_equal(fd.photometric_chain_records(torch.tensor([HUE, BLUR], dtype=torch.float64), src, net),
                          fd.photometric_chain_records([HUE, BLUR], src, net))


@pytest.mark.parametrize('hw', [(1, 1), (2, 3), (37, 53)])
def test_the_fold_equals_hand_composed_single_passes(hw):
    img = _pixels(hw, 4)
    before = img.copy()
    one = lambda row, x: fd.photometric_image_u8(x, fd.query_photometric_record(row, hw, hw))
    for chain in ([HUE, BLUR], [GAUSS, BLUR], [IMPULSE, SAT, BLUR], [BRI, HUE, SAT], [GAUSS, NONE, BLUR]):
        want = img
        for row in chain:
            want = one(row, want)
        got = fd.photometric_chain_u8(img, fd.photometric_chain_records(chain, hw, hw))
        assert got.dtype == np.uint8 and np.array_equal(got, want), chain
    assert np.array_equal(img, before)                                                # the image is not changed
    a = fd.photometric_chain_u8(img, fd.photometric_chain_records([GAUSS, BLUR], hw, hw))
    b = fd.photometric_chain_u8(img, fd.photometric_chain_records([GAUSS, HUE], hw, hw))
    if hw != (1, 1):
        assert not np.array_equal(a, b)


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_hue_170_three_times_is_the_identity_and_one_step_rotates_the_channels():
    """170 grey levels of imgaug's hue are 170 * 3 / 255 = 2 sextants exactly: one step sends (r, g, b) to (b, r, g)."""
    img = _pixels((37, 53), 1)
    step = fd.photometric_chain_records([(4, 170, 0)], (37, 53), (37, 53))
    assert step[0, 4] == 2 << fd.PHOTO_HUE_BITS
    assert np.array_equal(fd.photometric_chain_u8(img, step), img[..., [2, 0, 1]])
    recs = fd.photometric_chain_records([(4, 170, 0)] * 3, (37, 53), (37, 53))
    assert (recs[:, 2] == 4).all()
    assert np.array_equal(fd.photometric_chain_u8(img, recs), img)


@pytest.mark.parametrize('v', (0, 100, 250))
def test_brightness_then_blur_on_a_constant_grey_image_is_the_clipped_constant(v):
    img = np.full((9, 14, 3), v, np.uint8)
    out = fd.photometric_chain_u8(img, fd.photometric_chain_records([(6, 10, 0), (3, 2.0, 0)], (9, 14), (9, 14)))
    assert (out == min(v + 10, 255)).all()


def test_saturation_minus_255_then_brightness_0_gives_the_maximum_on_all_channels():
    img = _pixels((20, 31), 2)
    recs = fd.photometric_chain_records([(5, -255, 0), (6, 0, 0)], (20, 31), (20, 31))
    assert recs[:, 2].tolist() == [5, 0, 0]                                            # brightness 0 is neutral
    out = fd.photometric_chain_u8(img, recs)
    assert np.array_equal(out, np.repeat(img.max(-1, keepdims=True), 3, -1))
    both = np.stack([fd.query_photometric_record((5, -255, 0), (20, 31), (20, 31)),
                     fd.query_photometric_record((6, 1e-9, 0), (20, 31), (20, 31))])  # an active brightness of a0 = 0
    assert both[1, 2] == 6 and both[1, 4] == 0
    assert np.array_equal(fd.photometric_chain_u8(img, both), out)


# ---- structure --------------------------------------------------------------------------------------------------------
def test_a_chain_with_one_active_row_is_the_single_operator_rule_and_a_neutral_chain_returns_its_input():
    img = _pixels((40, 50), 3)
    masks = np.zeros((1, 40, 50), bool)
    masks[0, 10:20, 10:30] = True
    boxes = np.array([[10, 10, 20, 30]], np.float32)
    flip = np.array([1, 0, 1, 0, 0, 0, 0, 0], np.float64)
    for row in (HUE, GAUSS, BLUR, IMPULSE):
        rec = fd.query_photometric_record(row, (40, 50), (64, 64))
        for chain in ([row], [NONE, row], [row, NONE, (6, 0, 7)]):
            recs = fd.photometric_chain_records(chain, (40, 50), (64, 64))
            assert np.array_equal(recs[0], rec) and not recs[1:, 2].any()
            assert np.array_equal(fd.photometric_chain_u8(img, recs), fd.photometric_image_u8(img, rec))
            a = fd.augment_query_chain(img, boxes, masks, 64, 64, flip, chain)
            b = fd.augment_query_full(img, boxes, masks, 64, 64, flip, row)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for chain in ([NONE], [NONE, (3, 0, 0), (6, 0, 7)], None):
        recs = fd.photometric_chain_records(chain, (40, 50), (64, 64))
        out = fd.photometric_chain_u8(img, recs)
        assert np.array_equal(out, img) and out is not img
        for x, y in zip(fd.augment_query_chain(img, boxes, masks, 64, 64, flip, chain),
                        fd.augment_query(img, boxes, masks, 64, 64, flip)):
            assert np.array_equal(x, y)
    # the fallback drops both halves; the chain's errors are raised, fallback or not
    gone = np.array([0, 0, 1, 0, -500, 0, 0, 0], np.float64)
    plain = fd.augment_query(img, boxes, masks, 64, 64, None)
    for x, y in zip(fd.augment_query_chain(img, boxes, masks, 64, 64, gone, [HUE, BLUR]), plain):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match='qry_photometric_chain'):
        fd.augment_query_chain(img, boxes, masks, 64, 64, gone, [BLUR, HUE])
    # the supports' form: the same fold at equal size, one box and one mask
    crop, mask, box = _pixels((48, 48), 5), np.zeros((48, 48), bool), np.array([8, 8, 40, 40], np.float32)
    mask[8:40, 8:40] = True
    a = fd.augment_support(crop, box, mask, flip, photometric_chain=[HUE, BLUR])
    b = fd.augment_query_chain(crop, box[None], mask[None], 48, 48, flip, [HUE, BLUR])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1][0]) and np.array_equal(a[2], b[2][0])
    c = fd.augment_support(crop, box, mask, flip, HUE)
    assert all(np.array_equal(x, y) for x, y in zip(fd.augment_support(crop, box, mask, flip, photometric_chain=[HUE]), c))
    with pytest.raises(ValueError, match='not both'):
        fd.augment_support(crop, box, mask, flip, HUE, photometric_chain=[HUE])


def test_refusals_name_the_rule():
    ok = fd.check_photometric_chain
    assert ok([HUE, BLUR]).shape == (2, 3) and ok([BLUR, NONE, (6, 0, 0)]).shape == (3, 3) and ok([BLUR]).shape == (1, 3)
    for bad in ([BLUR, HUE], [BLUR, NONE, GAUSS], [HUE, BLUR, SAT]):                    # blur not last
        with pytest.raises(ValueError, match='point operators, then at most one blur'):
            ok(bad)
    for bad in ([BLUR, BLUR], [BLUR, NONE, BLUR], [(3, 0, 0), BLUR]):                   # two blurs
        with pytest.raises(ValueError, match='at most once'):
            ok(bad)
    for bad in (np.zeros((0, 3)), np.zeros((4, 3)), np.zeros(3), np.zeros((2, 2)), np.zeros((1, 2, 3)), [['a', 0, 0]]):
        with pytest.raises(ValueError, match=r'\[P,3\]'):                             # P = 0, P = 4, wrong shapes
            ok(bad)
    for bad in ([HUE, (7, 0, 0)], [(1, 2.5, 0), BLUR], [HUE, (np.nan, 0, 0)], [(4, 256, 0)], [(1, 1, 0.5)]):   # a bad row
        with pytest.raises(ValueError, match='qry_photometric_chain'):
            ok(bad)
    with pytest.raises(ValueError, match='spp_photometric_chain'):
        ok([BLUR, HUE], 'spp_photometric_chain')
    with pytest.raises(ValueError, match='qry_photometric_chain.*radius'):             # sigma 6 source pixels: radius 18
        fd.photometric_chain_records([HUE, (3, 6.0, 0)], (40, 50), (40, 50))
    # records, as the kernel checks them
    img = _pixels((6, 7), 1)
    rec = {k: fd.query_photometric_record(v, (6, 7), (6, 7)) for k, v in dict(blur=BLUR, hue=HUE, none=NONE).items()}
    other = fd.query_photometric_record(HUE, (7, 6), (7, 6))
    bad7 = rec['hue'].copy()
    bad7[2] = 7
    for bad in ([rec['blur'], rec['hue']], [rec['blur'], rec['blur']], [rec['hue'], other], [bad7, rec['blur']],
                [rec['hue']] * 4, []):
        with pytest.raises(ValueError):
            fd.photometric_chain_u8(img, np.stack(bad) if bad else np.zeros((0, 64), np.int32))
    with pytest.raises(ValueError):
        fd.photometric_chain_u8(img, rec['hue'])                                      # one record is [1,64], not [64]
    assert np.array_equal(fd.photometric_chain_u8(img, np.stack([rec['hue'], rec['none'], rec['blur']])),
                          fd.photometric_chain_u8(img, np.stack([rec['hue'], rec['blur']])))


# ---- the flip commutes with HSV + blur chains -----------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (2, 3), (37, 53)])
def test_hsv_then_blur_commutes_with_the_horizontal_flip(hw):
    """The reference's order is flip, HSV operator, blur; the project's is HSV operator, blur, then the gather that flips.
    The HSV operators do not depend on position and the blur has symmetric weights and a reflect-101 border, so both
    commute with the flip exactly - the two orders give identical bytes.  Not so for noise, whose counter is the pixel
    index."""
    h, w = hw
    img = _pixels(hw, 8)
    masks = np.ones((1, h, w), bool)
    boxes = np.array([[0, 0, h, w]], np.float32)
    flip, stay = np.array([1, 0, 1, 0, 0, 0, 0, 0], np.float64), np.array([0, 0, 1, 0, 0, 0, 0, 0], np.float64)
    for first in (HUE, SAT, BRI):
        chain = [first, BLUR]
        ours, _, _ = fd.augment_query_chain(img, boxes, masks, h, w, flip, chain)           # chain, then the flip
        unflipped, _, _ = fd.augment_query_chain(img, boxes, masks, h, w, stay, chain)
        assert np.array_equal(ours, unflipped[:, ::-1])
        theirs, _, _ = fd.augment_query_chain(np.ascontiguousarray(img[:, ::-1]), boxes, masks, h, w, stay, chain)
        assert np.array_equal(ours, theirs)                                                 # the flip, then the chain
    if w > 1:
        noisy = [GAUSS, BLUR]
        a, _, _ = fd.augment_query_chain(img, boxes, masks, h, w, flip, noisy)
        b, _, _ = fd.augment_query_chain(np.ascontiguousarray(img[:, ::-1]), boxes, masks, h, w, stay, noisy)
        assert not np.array_equal(a, b)


# ---- the draws --------------------------------------------------------------------------------------------------------
def test_draw_coco_augment_ranges_operator_set_and_determinism():
    rng = np.random.default_rng(5)
    rows, chains = zip(*(fd.draw_coco_augment(rng) for _ in range(4000)))
    rows, chains = np.stack(rows), np.stack(chains)
    assert rows.shape == (4000, 8) and chains.shape == (4000, 2, 3) and rows.dtype == chains.dtype == np.float64
    assert set(rows[:, 0]) == {0., 1.} and 0.45 < rows[:, 0].mean() < 0.55                  # the flip, p = 1/2
    neutral = np.array(fd.AUG_NEUTRAL)
    assert (rows[:, 1:] == neutral[1:]).all()                                               # no rotation, scale, shear ...
    assert set(chains[:, 0, 0]) == {4., 5., 6.} and (chains[:, 1, 0] == 3).all()            # never noise; the blur second
    assert (chains[:, :, 2] == 0).all()
    for op, lim in ((4, 10), (5, 25), (6, 30)):
        a = chains[chains[:, 0, 0] == op, 0, 1]
        assert 0.28 < len(a) / 4000 < 0.39 and -lim <= a.min() < -0.9 * lim and 0.9 * lim < a.max() <= lim
    s = chains[:, 1, 1]
    assert 0 <= s.min() < 0.05 and 1.45 < s.max() <= 1.5
    for row, chain in zip(rows[:200], chains[:200]):                                        # every draw is a valid pair
        fd.check_augment_params(row)
        fd.photometric_chain_records(chain, (600, 1000), (800, 1333))
    for make in (np.random.default_rng, np.random.RandomState):
        a, b, c = (fd.draw_coco_augment(make(s)) for s in (3, 3, 4))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])


# (geometric row of draw_query_augment; both rows of draw_query_augment_full, from np.random.default_rng(seed); both rows
# of draw_support_augment from np.random.RandomState(seed)) as the parent commit of this feature drew them
PARENT_DRAWS = {
    1: ([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
        [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0],
        [0.0, 0.0, 1.0, -9.997712503653101, 0.0, 0.0, 1.0, 0.0], [1.0, 1.0, 799981516.0]),
    2: ([0.0, 10.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0],
        [0.0, 10.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [5.0, 34.28407902176919, 807028964.0],
        [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [3.0, 0.9910044630116224, 878959190.0]),
    3: ([0.0, 10.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0],
        [0.0, 10.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0],
        [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [4.0, 39.29469543476547, 3849549504.0]),
    5: ([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0],
        [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0],
        [0.0, 0.0, 1.0, 0.0, -12.0, 17.0, 0.0, 0.0], [0.0, 0.0, 0.0]),
    11: ([0.0, 0.0, 1.040599343049343, 0.0, 0.0, 0.0, 0.0, 0.0],
         [0.0, 0.0, 1.040599343049343, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0],
         [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),
}


@pytest.mark.parametrize('seed', sorted(PARENT_DRAWS))
def test_the_existing_draws_keep_their_random_streams(seed):
    geo, full_p, full_q, spp_p, spp_q = PARENT_DRAWS[seed]
    assert fd.draw_query_augment(np.random.default_rng(seed)).tolist() == geo
    p, q = fd.draw_query_augment_full(np.random.default_rng(seed))
    assert p.tolist() == full_p and q.tolist() == full_q
    p, q = fd.draw_support_augment(np.random.RandomState(seed))
    assert p.tolist() == spp_p and q.tolist() == spp_q


# ---- the loader ---------------------------------------------------------------------------------------------------------
def _same(x, y):
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    return torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(np.asarray(x), np.asarray(y))


def test_loader_augs_flag_keys_shapes_and_collate():
    kw = dict(dataset='MNISTISEG', n_ways=2, k_shots=1, n_imgs=6, img_size=64, spp_img_size=32, raw_uint8=True,
              source_size=80, spp_source=True)
    on = dict(augment_qry=True, photometric_qry=True, augment_spp=True, photometric_spp=True)
    with pytest.raises(ValueError, match='augs'):
        fd.ClutteredCharsFewShotISEG(**kw, augs='imagenet')
    for flags in ({}, dict(augment_qry=True, augment_spp=True), on):
        base, nat = fd.ClutteredCharsFewShotISEG(**kw, **flags), fd.ClutteredCharsFewShotISEG(**kw, **flags, augs='natural')
        for i in range(len(base)):                                                     # key for key, byte for byte
            a, b = base[i], nat[i]
            assert list(a) == list(b) and all(_same(a[k], b[k]) for k in a), (flags, i)
    nat, coco = fd.ClutteredCharsFewShotISEG(**kw, **on), fd.ClutteredCharsFewShotISEG(**kw, **on, augs='coco')
    rename = {'qry_photometric': 'qry_photometric_chain', 'spp_photometric': 'spp_photometric_chain'}
    for i in range(len(coco)):
        a, b = nat[i], coco[i]
        assert [rename.get(k, k) for k in a] == list(b)
        for k in a:
            if 'augment' not in k and 'photometric' not in k:
                assert _same(a[k], b[k]), k                                            # the episode itself is the same
        assert b['qry_augment'].shape == (8,) and b['qry_photometric_chain'].shape == (2, 3)
        assert b['spp_augment'].shape == (2, 8) and b['spp_photometric_chain'].shape == (2, 2, 3)
        assert all(b[k].dtype == np.float64 for k in b if 'augment' in k or 'photometric' in k)
        row, chain = fd.draw_coco_augment(np.random.default_rng([int(coco.seed), int(coco.order[i]), 0]))
        assert np.array_equal(b['qry_augment'], row) and np.array_equal(b['qry_photometric_chain'], chain)
        for j in range(2):
            row, chain = fd.draw_coco_augment(np.random.default_rng([int(coco.seed), int(coco.order[i]), 0, 1 + j]))
            assert np.array_equal(b['spp_augment'][j], row) and np.array_equal(b['spp_photometric_chain'][j], chain)
        assert (b['spp_augment'][:, 1:] == np.array(fd.AUG_NEUTRAL)[1:]).all()
    geo_only = fd.ClutteredCharsFewShotISEG(**kw, augment_qry=True, augment_spp=True, augs='coco')[0]
    assert not any('photometric' in k for k in geo_only)
    assert np.array_equal(geo_only['qry_augment'], coco[0]['qry_augment'])              # one joint draw either way
    batch = collate([coco[i] for i in range(4)])
    assert tuple(batch['qry_photometric_chain'].shape) == (4, 2, 3) and batch['qry_photometric_chain'].dtype == torch.float64
    assert tuple(batch['spp_photometric_chain'].shape) == (4, 2, 2, 3) and tuple(batch['spp_augment'].shape) == (4, 2, 8)
    before = np.stack([coco[i]['qry_photometric_chain'] for i in range(len(coco))])
    coco.reshuffle(e=1)
    assert not np.array_equal(before, np.stack([coco[i]['qry_photometric_chain'] for i in range(len(coco))]))


# ---- the detector's host-only contract and the ABI table ----------------------------------------------------------------
def test_the_detector_refuses_the_keywords_where_they_cannot_apply():
    from fgn_amd import lib, ops
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    cfg = tiny_config(1, 1, 2)
    m = FGN(1, 1, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'])
    img = torch.zeros((1, 3, 64, 64))
    gt = ([np.zeros((1, 4), np.float32)], [np.zeros(1, np.int64)], [np.zeros((1, 64, 64), bool)])
    chain = np.array([[HUE, BLUR]], np.float64)
    spp_chain = chain[None]
    with pytest.raises(ValueError, match='qry_photometric_chain needs qry_resize_to'):
        m.forward_train(img, *gt, qry_photometric_chain=chain)
    with pytest.raises(ValueError, match='spp_photometric_chain needs spp_crop_to'):
        m.forward_train(img, *gt, spp_photometric_chain=spp_chain)
    with pytest.raises(ValueError, match='qry_photometric and qry_photometric_chain'):
        m.forward_train(img, *gt, qry_photometric=np.zeros((1, 3)), qry_photometric_chain=chain)
    with pytest.raises(ValueError, match='spp_photometric and spp_photometric_chain'):
        m.forward_train(img, *gt, spp_photometric=np.zeros((1, 1, 3)), spp_photometric_chain=spp_chain)
    with pytest.raises(ValueError, match='qry_photometric_chain is for forward_train'):
        m.simple_test(img, qry_photometric_chain=chain, rescale=True)
    with pytest.raises(ValueError, match='spp_photometric_chain is for forward_train'):
        m.simple_test(img, spp_photometric_chain=spp_chain, rescale=True)
    with pytest.raises(ValueError, match='spp_photometric_chain is for forward_train'):
        m.encode_supports(None, None, None, spp_photometric_chain=spp_chain)
    with pytest.raises(ValueError, match='spp_photometric_chain is for forward_train'):
        m.detect_device(img, None, None, None, None, spp_photometric_chain=spp_chain)
    for fn in (FGN.forward_train, FGN.simple_test, FGN._train_front):
        for name in ('qry_photometric_chain', 'spp_photometric_chain'):
            assert inspect.signature(fn).parameters[name].default is None
    # the launch selection, on the host: none, the single-operator records, the chain records cut to the longest chain
    rs = dict(B=2, hw=(64, 64), sizes=[(40, 50), (30, 20)])
    recs = FGN._photometric_chain_records(np.array([[HUE, BLUR, NONE], [NONE, NONE, NONE]], np.float64), rs)
    assert recs.dtype == torch.int32 and tuple(recs.shape) == (2, 2, 64) and recs[:, :, 2].tolist() == [[4, 3], [0, 0]]
    assert recs.is_contiguous() and recs[1, :, :2].tolist() == [[30, 20]] * 2
    recs = FGN._photometric_chain_records(np.array([[GAUSS, SAT, BLUR], [NONE, HUE, NONE]], np.float64), rs)
    assert tuple(recs.shape) == (2, 3, 64) and recs[:, :, 2].tolist() == [[1, 5, 3], [4, 0, 0]]
    one = np.array([[NONE, BLUR, NONE], [HUE, NONE, (3, 0, 0)]], np.float64)
    recs = FGN._photometric_chain_records(one, rs)
    assert tuple(recs.shape) == (2, 64) and torch.equal(recs, FGN._photometric_records(np.array([BLUR, HUE], np.float64), rs))
    assert FGN._photometric_chain_records(np.zeros((2, 1, 3)), rs) is None
    gone = np.array([[0, 0, 1, 0, -500, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0]], np.float64)   # image 0 fell back
    aug = np.zeros((2, 16), np.int32)
    recs = FGN._photometric_chain_records(np.array([[HUE, BLUR], [SAT, NONE]], np.float64), rs, gone, aug)
    assert tuple(recs.shape) == (2, 64) and recs[:, 2].tolist() == [0, 5]
    for bad in (one[:1], one[0], one[..., :2], np.zeros((2, 0, 3)), np.zeros((2, 4, 3)),
                np.array([[BLUR, HUE], [NONE, NONE]], np.float64), np.array([[HUE, (7, 0, 0)], [NONE, NONE]], np.float64)):
        with pytest.raises(ValueError, match='qry_photometric_chain'):
            FGN._photometric_chain_records(bad, rs)
    # the ABI: a pure addition
    assert lib.ABI_VERSION == 33 and ops.PHOTO_CHAIN_MAX == fd.PHOTO_CHAIN_MAX
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fgn_hip.h')).read()
    params = re.search(r'\bfgn_photometric_chain_u8hwc3\s*\(([^)]*)\)', header).group(1)
    assert len(lib.SIGNATURES['fgn_photometric_chain_u8hwc3'][1]) == len(params.split(',')) == 7
    single = re.search(r'\bfgn_photometric_u8hwc3\s*\(([^)]*)\)', header).group(1)
    assert len(lib.SIGNATURES['fgn_photometric_u8hwc3'][1]) == len(single.split(',')) == 6
