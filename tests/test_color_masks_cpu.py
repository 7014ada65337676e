"""Masks as box + colour, host side: ``colormask.as_color_masks`` / ``is_color`` / ``ColorMasks``
against an independent second formulation of the rule, the dataset option, the binding table, and the detector's
refusals that need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from fgn_amd import colormask as cm
from fgn_amd import rle


def _second_formulation(img, boxes, colors, shift):
    """Predicate, then max_pool2d(3, 1, 1) on the box crop ALONE (the pool pads with -inf: nothing outside the crop
    contributes), pasted into zeros."""
    h, w = img.shape[:2]
    out = np.zeros((len(boxes), h, w), bool)
    for i, ((y0, x0, y1, x1), c) in enumerate(zip(boxes, colors)):
        if y1 <= y0 or x1 <= x0:
            continue
        roi = torch.from_numpy(img[y0:y1, x0:x1].astype(np.int64))
        lo = torch.clamp(torch.tensor([int(v) for v in c]) - shift, min=0)
        hi = torch.clamp(torch.tensor([int(v) for v in c]) + shift, max=255)
        p = ((roi >= lo) & (roi <= hi)).all(-1).float()[None, None]
        d = torch.nn.functional.max_pool2d(p, kernel_size=3, stride=1, padding=1)[0, 0]
        out[i, y0:y1, x0:x1] = d.numpy() > 0
    return out


def cases():
    """(name, img uint8 [h,w,3], boxes [n,4], colors [n,3], shift) - the shapes the device test runs too."""
    rng = np.random.RandomState(11)
    out = []

    def speckle(h, w, color, density=0.3, other=(255, 255, 255)):
        img = np.empty((h, w, 3), np.uint8)
        img[:] = other
        sel = rng.rand(h, w) < density
        img[sel] = color
        noise = rng.rand(h, w) < 0.1
        img[noise] = rng.randint(0, 256, (int(noise.sum()), 3))
        return img
    one = np.full((1, 1, 3), 200, np.uint8)
    out.append(('1x1', one, [[0, 0, 1, 1]], [[200, 200, 200]], 75))
    out.append(('1x1-miss', one, [[0, 0, 1, 1]], [[10, 10, 10]], 75))
    out.append(('empty-box', speckle(9, 7, (230, 25, 75)), [[3, 2, 3, 6], [0, 0, 0, 0], [9, 7, 9, 7], [2, 4, 8, 4]],
                [[230, 25, 75]] * 4, 75))
    H, W = 37, 53
    img = speckle(H, W, (60, 180, 75), 0.15)
    corners = [[0, 0, 9, 11], [0, W - 12, 8, W], [H - 7, 0, H, 13], [H - 9, W - 10, H, W]]
    edges = [[0, 20, 5, 33], [H - 4, 17, H, 40], [10, 0, 30, 3], [12, W - 2, 29, W], [0, 0, H, W]]
    out.append(('corners-edges', img, corners + edges, [[60, 180, 75]] * 9, 75))
    for bw in (1, 63, 64, 65, 129):
        for bh in (1, 2, 3, 17):
            ih, iw = bh + 4, bw + 5
            out.append((f'box{bh}x{bw}', speckle(ih, iw, (0, 130, 200), 0.2), [[2, 3, 2 + bh, 3 + bw]], [[0, 130, 200]], 75))
    # a matching pixel directly outside every side (and corner) of the box must not dilate in
    img = np.full((20, 90, 3), 255, np.uint8)
    y0, x0, y1, x1 = 5, 10, 12, 80
    img[y0 - 1, x0 - 1:x1 + 1] = img[y1, x0 - 1:x1 + 1] = (128, 0, 0)
    img[y0 - 1:y1 + 1, x0 - 1] = img[y0 - 1:y1 + 1, x1] = (128, 0, 0)
    img[8, 40] = (128, 0, 0)
    out.append(('ring-outside', img, [[y0, x0, y1, x1]], [[128, 0, 0]], 75))
    # two adjacent boxes of the same colour, a seam of matching pixels on both sides
    img = np.full((16, 140, 3), 255, np.uint8)
    img[3:12, 60:80] = (145, 30, 180)
    out.append(('adjacent', img, [[2, 5, 13, 70], [2, 70, 13, 135]], [[145, 30, 180]] * 2, 75))
    for color in ((0, 0, 0), (255, 255, 255), (10, 128, 250)):
        for shift in (0, 75, 255):
            img = rng.randint(0, 256, (13, 71, 3)).astype(np.uint8)
            img[rng.rand(13, 71) < 0.3] = color
            out.append((f'clamp{color}-{shift}', img, [[1, 2, 12, 69], [0, 0, 13, 71]], [list(color)] * 2, shift))
    return out


CASES = cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_dense_equals_a_second_formulation(case):
    _, img, boxes, colors, shift = case
    m = cm.as_color_masks({'bboxes': boxes, 'colors': colors, 'shift': shift}, img.shape[:2], 'case')
    got = m.dense(img)
    assert got.dtype == bool and got.shape == (len(boxes),) + img.shape[:2] == m.shape
    assert np.array_equal(got, _second_formulation(img, boxes, colors, shift))
    lo, hi = m.bounds()
    c = np.asarray(colors, np.int64)
    assert np.array_equal(lo, np.maximum(c - shift, 0)) and np.array_equal(hi, np.minimum(c + shift, 255))


def test_the_cases_exercise_the_rule():
    """Somewhere a mask is non-empty, dilation adds pixels, and a matching pixel outside a box stays out."""
    by = {c[0]: c for c in CASES}
    _, img, boxes, colors, shift = by['ring-outside']
    d = cm.as_color_masks({'bboxes': boxes, 'colors': colors}, img.shape[:2]).dense(img)[0]
    assert d.sum() == 9 and d[7:10, 39:42].all()            # the one inner pixel, dilated; the ring contributes nothing
    _, img, boxes, colors, shift = by['adjacent']
    d = cm.as_color_masks({'bboxes': boxes, 'colors': colors}, img.shape[:2]).dense(img)
    assert d[0][:, 70:].sum() == 0 and d[1][:, :70].sum() == 0 and d[0][:, 69].any() and d[1][:, 70].any()


def test_as_color_masks_accepts_the_forms():
    d = {'bboxes': [[1, 2, 5, 6], [0, 0, 8, 9]], 'colors': [[1, 2, 3], [255, 0, 7]]}
    m = cm.as_color_masks(d, (8, 9), 'x')
    assert m.shape == (2, 8, 9) and len(m) == 2 and m.shift == 75
    assert m.boxes.dtype == np.int32 and m.boxes.shape == (2, 4) and m.colors.dtype == np.uint8 and m.colors.shape == (2, 3)
    assert cm.as_color_masks(m, (8, 9), 'x').shape == (2, 8, 9) and cm.as_color_masks(m, None).shape == (2, 8, 9)
    f = cm.as_color_masks({'bboxes': np.array(d['bboxes'], np.float32), 'colors': torch.tensor(d['colors']), 'shift': 0},
                          (8, 9))
    assert np.array_equal(f.boxes, m.boxes) and np.array_equal(f.colors, m.colors) and f.shift == 0
    one = cm.as_color_masks({'bboxes': [1, 2, 5, 6], 'colors': np.array([9, 8, 7], np.uint8)}, (8, 9))      # one item
    assert one.shape == (1, 8, 9)
    none = cm.as_color_masks({'bboxes': np.zeros((0, 4)), 'colors': np.zeros((0, 3))}, (8, 9))
    assert none.shape == (0, 8, 9) and none.dense(np.zeros((8, 9, 3), np.uint8)).shape == (0, 8, 9)
    empty = cm.as_color_masks({'bboxes': [[3, 3, 3, 7]], 'colors': [[0, 0, 0]]}, (8, 9))
    assert not empty.dense(np.zeros((8, 9, 3), np.uint8)).any()


BOX, COL = [[1, 2, 5, 6]], [[1, 2, 3]]


@pytest.mark.parametrize('entry,hw,word', [
    ({'bboxes': [[-1, 2, 5, 6]], 'colors': COL}, (8, 9), 'box 0'),
    ({'bboxes': [[1, 2, 9, 6]], 'colors': COL}, (8, 9), 'box 0'),
    ({'bboxes': BOX + [[1, 2, 5, 10]], 'colors': COL * 2}, (8, 9), 'box 1'),
    ({'bboxes': [[5, 2, 1, 6]], 'colors': COL}, (8, 9), 'box 0'),
    ({'bboxes': [[1, 6, 5, 2]], 'colors': COL}, (8, 9), 'box 0'),
    ({'bboxes': [[1.5, 2, 5, 6]], 'colors': COL}, (8, 9), 'integral'),
    ({'bboxes': [[1, 2, 5]], 'colors': COL}, (8, 9), 'bboxes'),
    ({'bboxes': BOX, 'colors': [[1, 2, 256]]}, (8, 9), 'colour 0'),
    ({'bboxes': BOX, 'colors': [[-1, 2, 3]]}, (8, 9), 'colour 0'),
    ({'bboxes': BOX, 'colors': [[1, 2]]}, (8, 9), 'colors'),
    ({'bboxes': BOX, 'colors': [[1, 2, 3.5]]}, (8, 9), 'integral'),
    ({'bboxes': BOX * 2, 'colors': COL}, (8, 9), '2 boxes for 1'),
    ({'bboxes': BOX, 'colors': COL, 'shift': 256}, (8, 9), 'shift'),
    ({'bboxes': BOX, 'colors': COL, 'shift': -1}, (8, 9), 'shift'),
    ({'bboxes': BOX, 'colors': COL, 'shift': 7.5}, (8, 9), 'shift'),
    ({'bboxes': BOX, 'colors': COL}, (0, 9), 'within'),
    ({'bboxes': BOX, 'colors': COL}, (8, 16385), 'within'),
    ({'bboxes': BOX, 'colors': COL}, None, 'size'),
    ({'bboxes': BOX, 'colours': COL}, (8, 9), 'expected'),
    (np.zeros((1, 8, 9), bool), (8, 9), 'expected'),
])
def test_refusals_name_the_item(entry, hw, word):
    with pytest.raises(ValueError) as err:
        cm.as_color_masks(entry, hw, what='qry_isegmaps[3]')
    assert 'qry_isegmaps[3]' in str(err.value) and word in str(err.value), str(err.value)


def test_a_colormasks_at_another_size_is_refused():
    m = cm.as_color_masks({'bboxes': BOX, 'colors': COL}, (8, 9))
    with pytest.raises(ValueError):
        cm.as_color_masks(m, (8, 10), 'x')
    with pytest.raises(ValueError):
        m.dense()                                        # no image bound
    with pytest.raises(ValueError):
        m.dense(np.zeros((8, 10, 3), np.uint8))


def test_is_color_decides_by_type_and_leaves_the_rle_predicates_alone():
    pair = [[4, 5], rle.counts_to_string(np.array([20]))]
    probes = [np.zeros((2, 4, 5), bool), torch.zeros((1, 4, 5), dtype=torch.uint8), pair, [pair, pair], [pair],
              {'size': [4, 5], 'counts': [20]}, [{'size': [4, 5], 'counts': [20]}], {'counts': [20]}, [], None, 'ab',
              [np.zeros((4, 5), bool), np.zeros((4, 5), bool)], rle.as_masks([pair])]
    want = [(False, False), (False, False), (False, True), (True, False), (True, False), (False, True), (True, False),
            (False, True), (True, False), (False, False), (False, False), (False, False), (True, False)]
    for p, (is_rle, is_item) in zip(probes, want):
        assert rle.is_rle(p) == is_rle and rle.is_item(p) == is_item, p
        assert not cm.is_color(p), p
    col = {'bboxes': BOX, 'colors': COL}
    m = cm.as_color_masks(col, (8, 9))
    assert cm.is_color(col) and cm.is_color(dict(col, shift=3)) and cm.is_color(m)
    assert not cm.is_color(dict(col, size=[8, 9])) and not cm.is_color({'bboxes': BOX}) and not cm.is_color([col])
    assert not rle.is_rle(m) and not rle.is_item(m) and not rle.is_rle(col)


def test_binding_table_and_constants():
    from fgn_amd import lib, ops
    res, args = lib.SIGNATURES['fgn_color_mask_u8']
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'fgn_hip.h')).read()
    proto = re.search(r'int fgn_color_mask_u8\(([^;]*)\);', header).group(1)
    assert len(args) == len(proto.split(',')) == 12
    assert lib.ABI_VERSION == 33
    assert cm.MAX_DIM == ops.RESIZE_MAX_DIM == 16384 and ops.CM_REC_INTS == 16 and cm.DEFAULT_SHIFT == 75


DS_KW = dict(n_ways=2, k_shots=1, n_imgs=6, img_size=48, spp_img_size=32, raw_uint8=True)


@pytest.mark.parametrize('source_size', (None, 60))
def test_dataset_option_and_collate(source_size):
    from fgn_amd.episodes import collate
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    kw = dict(DS_KW, spp_source=True, source_size=source_size)
    plain, col = DS(**kw), DS(**kw, color_masks=True)
    for i in range(len(plain)):
        a, b = plain[i], col[i]
        assert set(a) == set(b)
        g = b['qry_isegmaps']
        assert isinstance(g, cm.ColorMasks) and g.shape == a['qry_isegmaps'].shape
        assert np.array_equal(g.dense(b['qry_img']), a['qry_isegmaps'])
        assert np.array_equal(g.boxes, a['qry_bboxes'].astype(np.int32))
        for im, want, it in zip(b['spp_imgs'], a['spp_isegmaps'], b['spp_isegmaps']):
            assert isinstance(it, cm.ColorMasks) and len(it) == 1 and np.array_equal(it.dense(im)[0], want)
        for k in a:                                     # nothing else of a sample changes
            if k not in ('qry_isegmaps', 'spp_isegmaps'):
                x, y = a[k], b[k]
                same = all(torch.equal(p, q) for p, q in zip(x, y)) if isinstance(x, list) else \
                    np.array_equal(np.asarray(x), np.asarray(y))
                assert same, k
    bt = collate([col[0], col[1]])
    assert all(isinstance(g, cm.ColorMasks) for g in bt['qry_isegmaps'])
    assert len(bt['spp_isegmaps']) == 2 and all(isinstance(it, cm.ColorMasks) for lst in bt['spp_isegmaps'] for it in lst)
    qonly = DS(**dict(DS_KW, source_size=source_size), color_masks=True)[0]      # ready supports stay dense
    assert isinstance(qonly['qry_isegmaps'], cm.ColorMasks) and np.asarray(qonly['spp_isegmaps']).dtype == bool
    with pytest.raises(ValueError):
        DS(**kw, color_masks=True, rle_masks=True)
    with pytest.raises(ValueError):
        DS(**dict(DS_KW, raw_uint8=False), color_masks=True)


def _tiny(n_ways=2, k_shots=1):
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(n_ways, k_shots, width_div=2)
    return FGN(n_ways, k_shots, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def test_source_supports_take_colour_items_and_upload_no_mask_byte():
    """``_source_supports`` (host only): the geometry is that of the dense call, no mask byte travels for a colour
    instance, its item is moved into the window's frame and the window holds its whole box."""
    from fgn_amd import ops
    from fgn_amd.fewshot_ds import SPP_REC_FIELDS
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    kw = dict(DS_KW, spp_source=True)
    a, b = DS(**kw)[0], DS(**kw, color_masks=True)[0]
    m = _tiny()
    m.set_input_norm(**DS(**kw).input_norm)
    want = m._source_supports(a['spp_imgs'], a['spp_bboxes'], a['spp_isegmaps'], 32)
    assert want['mcol'] == []
    as_dict = [{'bboxes': it.boxes, 'colors': it.colors} for it in b['spp_isegmaps']]
    mixed = [b['spp_isegmaps'][0], a['spp_isegmaps'][1]]
    for masks, n_col in ((b['spp_isegmaps'], 2), (as_dict, 2), (mixed, 1)):
        got = m._source_supports(a['spp_imgs'], a['spp_bboxes'], masks, 32)
        assert torch.equal(got['rec'], want['rec']) and torch.equal(got['boxes'], want['boxes'])
        assert (got['need'], got['mneed'], got['capacity'], got['mcapacity']) == \
            (want['need'], want['mneed'], want['capacity'], want['mcapacity'])
        assert all(torch.equal(x, y) for x, y in zip(got['flats'], want['flats']))
        assert len(got['mcol']) == n_col and got['mrle'] == []
        for row, item in got['mcol']:
            assert got['mflats'][row].numel() == 0
            g = dict(zip(SPP_REC_FIELDS, (int(v) for v in got['rec'][row])))
            assert item.shape == (1, g['wh'], g['ww'])
            window = got['flats'][row].numpy().reshape(g['wh'], g['ww'], 3)
            assert np.array_equal(item.dense(window)[0].reshape(-1).view(np.uint8), want['mflats'][row].numpy())
        assert got['window_bytes'] == sum(f.numel() for f in got['flats'] + got['mflats']) + 4 * ops.CM_REC_INTS * n_col
    with pytest.raises(ValueError) as err:              # a box that is not the instance's: it leaves the window
        far = {'bboxes': [[0, 0, 48, 48]], 'colors': [[1, 2, 3]]}
        m._source_supports(a['spp_imgs'], a['spp_bboxes'], [far, a['spp_isegmaps'][1]], 32)
    assert 'spp_isegmaps[0]' in str(err.value)
    with pytest.raises(ValueError) as err:              # two masks for one instance
        two = {'bboxes': [[0, 0, 4, 4]] * 2, 'colors': [[1, 2, 3]] * 2}
        m._source_supports(a['spp_imgs'], a['spp_bboxes'], [a['spp_isegmaps'][0], two], 32)
    assert 'spp_isegmaps[1]' in str(err.value)
    with pytest.raises(ValueError) as err:              # outside its image
        out = {'bboxes': [[0, 0, 49, 4]], 'colors': [[1, 2, 3]]}
        m._source_supports(a['spp_imgs'], a['spp_bboxes'], [out, a['spp_isegmaps'][1]], 32)
    assert 'spp_isegmaps[0]' in str(err.value)


def test_detector_refusals_that_need_no_gpu():
    """Float input with a colour entry (the mask is made from the image's bytes) and colour supports without
    ``spp_crop_to`` are contract errors, raised on the host by every entry point."""
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    from fgn_amd.episodes import collate
    m = _tiny()
    ds = DS(**dict(DS_KW, spp_source=True), color_masks=True)
    m.set_input_norm(**ds.input_norm)
    b = collate([ds[0]])
    flt = torch.zeros((1, 3, 48, 48))
    for call in (lambda: m.simple_test(**dict(b, qry_img=flt)),
                 lambda: m.forward_train(**dict(b, qry_img=flt)),
                 lambda: m.detect_device(flt, b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                                         qry_isegmaps=b['qry_isegmaps'], spp_crop_to=32)):
        with pytest.raises(ValueError) as err:
            call()
        assert 'qry_isegmaps[0]' in str(err.value) and 'uint8' in str(err.value) and 'float' in str(err.value)
    ready = torch.zeros((1, 2, 32, 32, 3), dtype=torch.uint8)
    plain = {k: v for k, v in b.items() if k not in ('spp_crop_to', 'spp_fill_ratio', 'crop_square')}
    boxes = torch.zeros((1, 2, 4))
    for call in (lambda: m.simple_test(**dict(plain, spp_imgs=ready, spp_bboxes=boxes)),
                 lambda: m.forward_train(**dict(plain, spp_imgs=ready, spp_bboxes=boxes)),
                 lambda: m.detect_device(b['qry_img'], ready, boxes, b['spp_isegmaps'], b['img_shape']),
                 lambda: m.encode_supports(ready, boxes, b['spp_isegmaps']),
                 lambda: m.encode_supports(ready, boxes, b['spp_isegmaps'][0])):
        with pytest.raises(ValueError) as err:
            call()
        assert 'spp_crop_to' in str(err.value) and 'colour' in str(err.value)
    # a colour entry at another size than its image; sizes come from the image where img_shape is absent
    wrong = cm.as_color_masks({'bboxes': [[0, 0, 4, 4]], 'colors': [[1, 2, 3]]}, (48, 47))
    with pytest.raises(ValueError) as err:
        m.simple_test(**dict(b, qry_isegmaps=[wrong]))
    assert 'qry_isegmaps[0]' in str(err.value)
    with pytest.raises(ValueError) as err:
        m.simple_test(**dict(b, qry_isegmaps=[{'bboxes': [[0, 0, 4, 49]], 'colors': [[1, 2, 3]]}]))
    assert 'qry_isegmaps[0]' in str(err.value) and 'box 0' in str(err.value)
