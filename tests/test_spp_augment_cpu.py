"""Support augmentation on the host (``fewshot_ds.augment_support`` / ``support_augment_plan`` / ``draw_support_augment``),
the loader flags and the detector's contract - no GPU.  The rule is the queries' at equal size, in the reference's order
(``get_support`` with ``augment_spp``, base_fst.py:1151-1153): every comparison is bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


# the operator rows of tests/test_hip_qry_augment.py, with the photometric rows going round beside them
GEO = {'neutral': row(), 'flip': row(flip=1), 'rot10_sym': row(rotate=10, border=1), 'rot10_const': row(rotate=10),
       'scale0.8': row(scale=0.8), 'scale0.8_sym': row(scale=0.8, border=1), 'scale1.2': row(scale=1.2),
       'shear+10_sym': row(shear=10, border=1), 'shear-10_sym': row(shear=-10, border=1),
       'shear+10_const': row(shear=10), 'shift_const': row(tx=-2, ty=1), 'shift_sym': row(tx=-2, ty=1, border=1),
       'composed_sym': row(1, 33, 1.1, 5, 1.3, -0.7, 1, 4), 'composed_const': row(1, 33, 1.1, 5, 1.3, -0.7, 0, 3)}
PHOTO = [(0, 0, 0), (1, 1.0, 7), (2, 0.03, 11), (3, 0.7, 0), (4, 50, 0), (5, -75, 0), (6, 30, 0)]
# (source size, box YXYX): a 1x1 image, a flat one, boxes at the image border (the cut's reflect path), a large one
SOURCES = [((1, 1), [0, 0, 1, 1]), ((3, 40), [0, 2, 3, 31]), ((37, 53), [0, 30, 20, 53]), ((150, 131), [40, 0, 131, 70])]
SIZES = (1, 5, 65)


def _scene(hw, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, hw + (3,)).astype(np.uint8), rs.rand(*hw) > 0.4


def _cut(hw, box, S, seed=0):
    img, mask = _scene(hw, seed + hw[0])
    return fd.support_from_source(img, box, mask, S)


def _composition(crop, box, mask, params, photometric):
    """The rule of one instance written out: the photometric pass on the crop, the gather of the record at S -> S on
    image and mask, the box through the matrix; all of it dropped where the box leaves the open S x S rectangle."""
    S = crop.shape[0]
    p = fd.check_augment_params(params)
    prec = fd.query_photometric_record(photometric, (S, S), (S, S))
    if fd.augment_is_neutral(p):
        return (fd.photometric_image_u8(crop, prec) if prec[2] else crop), box, mask
    nb, ok = fd.augment_boxes_yxyx(box[None], p, S, S)
    if not ok:
        return crop, box, mask
    rec = fd.query_augment_record(p, (S, S), (S, S))
    img = fd.photometric_image_u8(crop, prec) if prec[2] else crop
    return fd.augment_image_u8(img, rec, S, S), nb[0], fd.augment_masks(mask[None], rec, S, S)[0]


@pytest.mark.parametrize('S', SIZES)
@pytest.mark.parametrize('hw,box', SOURCES)
def test_augment_support_is_the_composition_in_the_reference_order(hw, box, S):
    crop, b, mask = _cut(hw, box, S)
    assert crop.shape == (S, S, 3) and mask.shape == (S, S) and b.dtype == np.float32
    for i, (name, geo) in enumerate(GEO.items()):
        photo = PHOTO[i % len(PHOTO)]
        got = fd.augment_support(crop, b, mask, geo, photo)
        want = _composition(crop, b, mask, geo, photo)
        for x, y in zip(got, want):
            assert np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y), name
        assert got[0].shape == (S, S, 3) and got[0].dtype == np.uint8 and got[1].shape == (4,) and got[2].shape == (S, S)
    for photo in PHOTO:                                         # every photometric operator alone, and beside a warp
        for geo in (None, GEO['rot10_sym']):
            got = fd.augment_support(crop, b, mask, geo, photo)
            want = _composition(crop, b, mask, row() if geo is None else geo, photo)
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), photo


def test_the_blur_sigma_is_in_crop_pixels_on_both_axes():
    rec = fd.query_photometric_record((3, 1.0, 0), (65, 65), (65, 65))
    assert rec[6] == rec[7] == 3 and np.array_equal(rec[8:12], rec[25:29])


def test_known_answers_at_equal_size():
    S = 65
    crop, box, mask = _cut((37, 53), [0, 30, 20, 53], S)
    assert mask.any() and not mask.all() and not np.array_equal(mask, mask[:, ::-1])
    c, b, m = fd.augment_support(crop, box, mask, row(flip=1))
    assert np.array_equal(c, crop[:, ::-1]) and np.array_equal(m, mask[:, ::-1])
    assert np.allclose(b, [box[0], S - box[3], box[2], S - box[1]], atol=1e-4)
    c, b, m = fd.augment_support(crop, box, mask, row(tx=3, ty=-2))          # content moves right by 3 and up by 2
    want, wm = np.zeros_like(crop), np.zeros_like(mask)
    want[:-2, 3:], wm[:-2, 3:] = crop[2:, :-3], mask[2:, :-3]
    assert np.array_equal(c, want) and np.array_equal(m, wm)
    assert np.allclose(b, np.clip(box + np.array([-2, 3, -2, 3], np.float32), 0, S), atol=1e-4)
    for geo, photo in ((None, None), (row(), (0, 0, 0)), (row(border=1), (4, 0, 0)), (row(), (3, 0, 5))):
        c, b, m = fd.augment_support(crop, box, mask, geo, photo)
        assert np.array_equal(c, crop) and np.array_equal(b, box) and np.array_equal(m, mask)
    # the symmetric border reflects the padded S x S frame: a shift by 3 brings columns 2, 1, 0 of the FRAME back
    c, _, m = fd.augment_support(crop, box, mask, row(tx=3, border=1))
    assert np.array_equal(c[:, :3], crop[:, 2::-1]) and np.array_equal(c[:, 3:], crop[:, :-3])
    assert not m[:, :3].any() and np.array_equal(m[:, 3:], mask[:, :-3])     # the mask reads 0 outside, whatever the border


def test_a_box_moved_fully_out_falls_back_in_both_halves_for_that_instance_alone():
    S = 65
    crops = [_cut(hw, box, S, seed=i) for i, (hw, box) in enumerate(SOURCES[1:])]
    gone, hue = row(tx=-500), (4, 50, 0)
    c, b, m = fd.augment_support(*crops[1], gone, hue)
    assert np.array_equal(c, crops[1][0]) and np.array_equal(b, crops[1][1]) and np.array_equal(m, crops[1][2])
    assert not np.array_equal(fd.augment_support(*crops[1], None, hue)[0], crops[1][0])       # the hue alone is applied
    with pytest.raises(ValueError, match='qry_photometric'):                # its errors are raised, fallback or not
        fd.augment_support(*crops[1], gone, (9, 0, 0))
    rows = np.stack([row(flip=1), gone, row(rotate=10, border=1)])
    photo = np.array([(3, 0.7, 0), hue, (0, 0, 0)], np.float64)
    boxes = np.stack([c[1] for c in crops])
    recs, precs, nb, fell = fd.support_augment_plan(rows, photo, boxes, S)
    assert recs.dtype == np.int32 and recs.shape == (3, 16) and precs.dtype == np.int32 and precs.shape == (3, 64)
    assert nb.dtype == boxes.dtype and nb.shape == (3, 4) and fell.tolist() == [False, True, False]
    assert not recs[1, 2:6].any() and precs[1, 2] == 0 and np.array_equal(nb[1], boxes[1])
    assert recs[0, 3] == 1 and recs[2, 2] == 1 and precs[0, 2] == 3 and precs[2, 2] == 0
    assert np.array_equal(recs[1], fd.query_augment_record(None, (S, S), (S, S)))
    for i, cr in enumerate(crops):                              # the plan is what augment_support does, per instance
        img, b, m = fd.augment_support(*cr, rows[i], photo[i])
        assert np.array_equal(b, nb[i])
        x = fd.photometric_image_u8(cr[0], precs[i])
        assert np.array_equal(img, fd.augment_image_u8(x, recs[i], S, S))
        assert np.array_equal(m, fd.augment_masks(cr[2][None], recs[i], S, S)[0])
    # either half may be missing; the boxes are a copy
    r2, p2, b2, f2 = fd.support_augment_plan(None, photo, boxes, S)
    assert not r2[:, 2:6].any() and p2[:, 2].tolist() == [3, 4, 0] and np.array_equal(b2, boxes) and b2 is not boxes
    r3, p3, _, _ = fd.support_augment_plan(rows, None, boxes, S)
    assert np.array_equal(r3, recs) and not p3[:, 2].any()
    with pytest.raises(ValueError):
        fd.support_augment_plan(rows[:2], photo, boxes, S)


def test_draw_support_augment_is_reproducible_and_the_joint_draw():
    for i in range(40):
        a = fd.draw_support_augment(np.random.default_rng([7, 3, 0, 1 + i]))
        b = fd.draw_support_augment(np.random.default_rng([7, 3, 0, 1 + i]))
        c = fd.draw_query_augment_full(np.random.default_rng([7, 3, 0, 1 + i]))
        assert a[0].shape == (8,) and a[1].shape == (3,) and a[0].dtype == a[1].dtype == np.float64
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, c))
        fd.query_augment_record(a[0], (64, 64), (64, 64))
        fd.query_photometric_record(a[1], (64, 64), (64, 64))
    draws = [np.concatenate(fd.draw_support_augment(np.random.default_rng([7, 3, 0, 1 + i]))) for i in range(40)]
    assert len({d.tobytes() for d in draws}) > 10


def _same_value(x, y):
    if isinstance(x, list):
        return len(x) == len(y) and all(_same_value(a, b) for a, b in zip(x, y))
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    return np.array_equal(np.asarray(x), np.asarray(y))


def test_loader_flags_keys_streams_and_collate():
    kw = dict(dataset='MNISTISEG', n_ways=3, k_shots=2, n_imgs=6, img_size=64, spp_img_size=32, raw_uint8=True,
              source_size=80, spp_source=True)
    with pytest.raises(ValueError, match='spp_source'):
        fd.ClutteredCharsFewShotISEG(**dict(kw, spp_source=False), augment_spp=True)
    with pytest.raises(ValueError, match='augment_spp'):
        fd.ClutteredCharsFewShotISEG(**kw, photometric_spp=True)
    qry = dict(augment_qry=True, photometric_qry=True)
    base = fd.ClutteredCharsFewShotISEG(**kw, **qry)
    off = fd.ClutteredCharsFewShotISEG(**kw, **qry, augment_spp=False, photometric_spp=False)
    geo = fd.ClutteredCharsFewShotISEG(**kw, **qry, augment_spp=True)
    both = fd.ClutteredCharsFewShotISEG(**kw, **qry, augment_spp=True, photometric_spp=True)
    alone = fd.ClutteredCharsFewShotISEG(**dict(kw, source_size=None), augment_spp=True, photometric_spp=True)
    for i in range(len(base)):
        a, o, g, b = base[i], off[i], geo[i], both[i]
        assert list(o) == list(a) and list(g) == list(a) + ['spp_augment']
        assert list(b) == list(a) + ['spp_augment', 'spp_photometric']
        for k in a:                         # flags off: today's samples; flags on: nothing else moves, qry_* included
            assert _same_value(a[k], o[k]) and _same_value(a[k], g[k]) and _same_value(a[k], b[k]), k
        assert g['spp_augment'].dtype == np.float64 and g['spp_augment'].shape == (6, 8)
        assert b['spp_augment'].shape == (6, 8) and b['spp_photometric'].dtype == np.float64
        assert b['spp_photometric'].shape == (6, 3)
        child = int(both.order[i])
        for j in range(6):
            p, q = fd.draw_support_augment(np.random.default_rng([int(both.seed), child, 0, 1 + j]))
            assert np.array_equal(b['spp_augment'][j], p) and np.array_equal(b['spp_photometric'][j], q)
            assert np.array_equal(g['spp_augment'][j],
                                  fd.draw_query_augment(np.random.default_rng([int(geo.seed), child, 0, 1 + j])))
        assert np.array_equal(alone[i]['spp_augment'], b['spp_augment']) and 'qry_augment' not in alone[i]
    assert any(both[i]['spp_augment'][:, :7].any() and both[i]['spp_photometric'][:, 0].any() for i in range(len(both)))
    batch = collate([both[i] for i in range(4)])
    assert isinstance(batch['spp_augment'], torch.Tensor) and tuple(batch['spp_augment'].shape) == (4, 6, 8)
    assert batch['spp_augment'].dtype == torch.float64 and tuple(batch['spp_photometric'].shape) == (4, 6, 3)
    rows = lambda: np.stack([both[i]['spp_augment'] for i in range(len(both))])
    before = rows()
    both.reshuffle(e=1)
    assert not np.array_equal(before, rows())                                         # another epoch, another draw
    both.reshuffle(e=0)
    assert np.array_equal(rows(), before)


def _model(n_ways=3, k_shots=1):
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    cfg = tiny_config(n_ways, k_shots, 2)
    m = FGN(n_ways, k_shots, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'])
    m.set_input_norm(mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.2))
    return m


def test_every_contract_error_is_raised_with_no_gpu_present():
    from fgn_amd.detector import FGN
    m = _model()
    S, NK = 32, 3
    rs = np.random.RandomState(0)
    imgs = [torch.from_numpy(rs.randint(0, 256, (40 + 3 * i, 50, 3)).astype(np.uint8)) for i in range(NK)]
    masks = [np.zeros(tuple(t.shape[:2]), bool) for t in imgs]
    for mk in masks:
        mk[10:30, 12:40] = True
    boxes = np.array([[10, 12, 30, 40]] * NK, np.float32)
    qry = (torch.zeros((1, 64, 64, 3), dtype=torch.uint8), [np.array([[5, 5, 30, 30]], np.float32)], [np.zeros(1, np.int64)],
           [np.zeros((1, 64, 64), bool)])
    spp = dict(spp_imgs=imgs, spp_bboxes=boxes, spp_isegmaps=masks)
    geo = np.stack([row(flip=1), row(rotate=10, border=1), row()])
    photo = np.array([(3, 0.7, 0), (4, 50, 0), (0, 0, 0)], np.float64)

    def refused(name, **kw):
        with pytest.raises(ValueError, match=name):
            m.forward_train(*qry, **{**spp, 'spp_crop_to': S, **kw})

    # either argument without spp_crop_to
    ready = dict(spp_imgs=torch.zeros((1, NK, S, S, 3), dtype=torch.uint8), spp_bboxes=boxes[None],
                 spp_isegmaps=torch.zeros((1, NK, S, S), dtype=torch.bool))
    for name, rows in (('spp_augment', geo), ('spp_photometric', photo)):
        with pytest.raises(ValueError, match=f'{name} needs spp_crop_to'):
            m.forward_train(*qry, **ready, **{name: rows})
    # shapes
    for bad in (geo[:2], geo[:, :7], geo.reshape(-1), np.stack([geo, geo]), geo[None, None], geo.astype(str)):
        refused('spp_augment', spp_augment=bad)
    for bad in (photo[:2], photo[:, :2], photo.reshape(-1), np.stack([photo, photo]), torch.from_numpy(photo)[..., None]):
        refused('spp_photometric', spp_photometric=bad)

    def one(r, width):
        out = np.zeros((NK, width), np.float64)
        if width == 8:
            out[:, 2] = 1
        out[1] = r
        return out
    # non-finite entries; flip / border / channel order / scale; coefficients beyond the bounds
    for r in (row(rotate=np.nan), row(tx=np.inf), row(flip=2), row(flip=0.5), row(border=2), row(border=-1), row(order=6),
              row(order=1.5), row(scale=0), row(scale=-1), row(scale=1e-3), row(tx=2.0 ** 21), row(shear=89.9999)):
        refused('spp_augment', spp_augment=one(r, 8))
        refused('spp_augment', spp_augment=one(r, 8), spp_photometric=photo)
    # operator / amount / seed outside their sets; a blur radius beyond 16
    for r in ((np.nan, 0, 0), (1, np.inf, 0), (1, 1, np.nan), (7, 0, 0), (-1, 0, 0), (2.5, 0, 0), (1, 1, -1),
              (1, 1, 2.0 ** 32), (1, 1, 0.5), (1, 2.5, 0), (1, 0, 0), (2, 1.5, 0), (2, -0.1, 0), (3, -1, 0), (4, 256, 0),
              (5, -300, 0), (6, 255.5, 0), (3, 5.4, 0)):
        refused('spp_photometric', spp_photometric=one(r, 3))
        refused('spp_photometric', spp_augment=geo, spp_photometric=one(r, 3))
    refused('spp_photometric', spp_augment=one(row(tx=-500), 8), spp_photometric=one((9, 0, 0), 3))   # fallback or not
    # the test path is without augmentation
    for name, rows in (('spp_augment', geo), ('spp_photometric', photo)):
        with pytest.raises(ValueError, match=f'{name} is for forward_train'):
            m.simple_test(qry[0], **spp, spp_crop_to=S, rescale=True, **{name: rows})
        with pytest.raises(ValueError, match=f'{name} is for forward_train'):
            m.encode_supports(imgs, boxes, masks, spp_crop_to=S, **{name: rows})
        with pytest.raises(ValueError, match=f'{name} is for forward_train'):
            m.detect_device(qry[0], imgs, boxes, masks, None, spp_crop_to=S, **{name: rows})
    for fn in (FGN.forward_train, FGN.simple_test, FGN._train_front, FGN.encode_supports, FGN.detect_device):
        for name in ('spp_augment', 'spp_photometric'):
            assert inspect.signature(fn).parameters[name].default is None
    # good rows pass the contract and fail only for want of a GPU
    if not torch.cuda.is_available():
        from fgn_amd.lib import FgnHipError
        with pytest.raises(FgnHipError):
            m.forward_train(*qry, **spp, spp_crop_to=S, spp_augment=geo, spp_photometric=photo)


def test_the_plan_of_the_detector_and_its_carrier():
    from fgn_amd.detector import FGN, _SupportWindows
    m = _model()
    S, NK = 32, 3
    rs = np.random.RandomState(1)
    imgs = [torch.from_numpy(rs.randint(0, 256, (40, 50 + i, 3)).astype(np.uint8)) for i in range(NK)]
    masks = [np.ones(tuple(t.shape[:2]), bool) for t in imgs]
    boxes = np.array([[10, 12, 30, 40]] * NK, np.float32)
    sp = m._source_supports(imgs, boxes, masks, S)
    geo = np.stack([row(flip=1), row(tx=-500), row(rotate=10, border=1)])
    photo = np.array([(3, 0.7, 0), (4, 50, 0), (0, 0, 0)], np.float64)
    want = fd.support_augment_plan(geo, photo, sp['boxes'].numpy().reshape(NK, 4), S)
    for g, p in ((geo, photo), (geo[None], torch.from_numpy(photo)[None])):
        out = FGN._support_plans(g, p, sp)
        assert out['aug'].dtype == torch.int32 and np.array_equal(out['aug'].numpy(), want[0])
        assert out['photo'].dtype == torch.int32 and np.array_equal(out['photo'].numpy(), want[1])
        assert tuple(out['boxes'].shape) == (1, NK, 4) and np.array_equal(out['boxes'].numpy()[0], want[2])
        assert out['rec'] is sp['rec'] and 'aug' not in sp                            # (the input dict is not changed)
    assert FGN._support_plans(geo, None, sp)['photo'] is None                          # no photometric launch
    out = FGN._support_plans(None, photo, sp)
    assert not out['aug'].numpy()[:, 2:6].any() and out['photo'].numpy()[:, 2].tolist() == [3, 4, 0]
    # every instance neutral after the fallback: the dict of the direct path, today's launch
    for g, p in ((np.stack([row()] * 3), np.zeros((3, 3))), (np.stack([row(), row(tx=-500), row(border=1)]),
                                                           np.array([(0, 0, 0), (1, 1, 3), (6, 0, 0)], np.float64))):
        out = FGN._support_plans(g, p, sp)
        assert 'aug' not in out and 'photo' not in out and torch.equal(out['boxes'], sp['boxes'])
    assert _SupportWindows._fields == ('src', 'msk', 'rec', 'S', 'aug', 'photo')
    assert _SupportWindows._field_defaults == dict(aug=None, photo=None)
    src, msk = torch.zeros((3, 8), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.uint8)
    a = _SupportWindows(src, msk, sp['rec'], S, torch.from_numpy(want[0]), None)
    assert a.shape == (3, S, S, 3) and a.to('cpu').photo is None
    assert _SupportWindows(src, msk, sp['rec'], S) == _SupportWindows(src, msk, sp['rec'], S, None, None)


def test_header_and_signatures_agree_on_the_two_entries_and_the_abi_stays_33():
    from fgn_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'fgn_hip.h')).read()
    for name, n_args in (('fgn_support_from_source_u8', 10), ('fgn_support_augment_f32', 9)):
        params = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header).group(1).split(',')
        assert len(params) == n_args == len(lib.SIGNATURES[name][1])
        assert lib.SIGNATURES[name][0] is lib._i
        for text, ctype in zip(params, lib.SIGNATURES[name][1]):
            want = lib._p if '*' in text else (lib.C.c_longlong if 'long long' in text else lib._i)
            assert ctype is want, (name, text)
    assert lib.ABI_VERSION == 33
    src = open(os.path.join(root, 'fgn_amd', 'csrc', 'spatial.hip')).read()
    for name in ('fgn_support_from_source_u8', 'fgn_support_augment_f32'):
        assert re.search(r'extern "C" int %s\(' % name, src)
