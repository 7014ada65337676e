"""``fgn_amd.maskforms``: the one table that tells the forms of a mask apart gives what the per-form
modules' own predicates and checkers give, asked in the order colour, polygons, RLE - host only."""
import numpy as np
import pytest
import torch

from fgn_amd import colormask, maskforms, ops, polygon, rle
from fgn_amd.episodes import collate

H, W = 12, 10
IMG = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
DENSE = np.zeros((2, H, W), bool)
DENSE[0, 2:7, 1:5] = DENSE[1, 5:11, 4:9] = True
TRI = [1.0, 1.0, 8.0, 2.0, 4.0, 10.0]
COLOR = {'bboxes': [[2, 1, 7, 5], [5, 4, 11, 9]], 'colors': [[10, 20, 30], [200, 100, 0]]}
POLY = {'polygons': [[TRI], [TRI, [2.0, 2.0, 9.0, 3.0, 5.0, 11.0]]]}
RLE_DICTS = rle.encode_many(DENSE)
PAIRS = [[np.array([H, W], np.int16), d['counts']] for d in RLE_DICTS]

ENTRIES = [
    rle.as_masks(RLE_DICTS, (H, W)), RLE_DICTS, PAIRS, [],
    colormask.as_color_masks(COLOR, (H, W)), COLOR, dict(COLOR, shift=40),
    polygon.as_polys(POLY, (H, W)), POLY, dict(POLY, size=[H, W]),
    DENSE, torch.from_numpy(DENSE), DENSE.astype(np.uint8).tolist(),
    {'size': [H, W], 'counts': RLE_DICTS[0]['counts'], 'area': 20},      # a dict that matches none of the key sets
]


def _by_the_predicates(x, predicates):
    """The parent's answer: the modules' own predicates asked in the order colour, polygons, RLE."""
    return next((form for form, pred in zip(maskforms.FORMS, predicates) if pred(x)), None)


def test_the_table_is_in_precedence_order():
    assert maskforms.FORMS == (maskforms.COLOR, maskforms.POLY, maskforms.RLE)
    assert [f.carrier for f in maskforms.FORMS] == [colormask.ColorMasks, polygon.PolyMasks, rle.RleMasks]
    assert colormask.REC_BYTES == 4 * ops.CM_REC_INTS


@pytest.mark.parametrize('i', range(len(ENTRIES)))
def test_form_of_is_the_predicates_in_order(i):
    x = ENTRIES[i]
    assert maskforms.form_of(x) is _by_the_predicates(x, (colormask.is_color, polygon.is_poly, rle.is_rle))
    assert maskforms.form_of_one(x) is _by_the_predicates(
        x, (colormask.is_color, polygon.is_poly, lambda v: rle.is_item(v) or isinstance(v, rle.RleMasks)))


def test_the_forms_of_the_case_list():
    C, P, R = maskforms.FORMS
    assert [maskforms.form_of(x) for x in ENTRIES] == [R, R, R, R, C, C, C, P, P, P, None, None, None, None]
    # ONE mask: any dict is an RLE item, a list of items is not one item, a [size, counts] pair is
    assert [maskforms.form_of_one(x) for x in ENTRIES] == [R, None, None, None, C, C, C, P, P, P, None, None, None, R]
    assert maskforms.form_of_one(PAIRS[0]) is R and maskforms.form_of_one(RLE_DICTS[0]) is R
    assert maskforms.is_pair(PAIRS[0]) and not maskforms.is_pair(PAIRS) and not maskforms.is_pair(RLE_DICTS[0])


def _same_carrier(a, b):
    assert type(a) is type(b) and a.shape == b.shape
    fields = {k: v for k, v in vars(a).items()}
    assert set(fields) == set(vars(b))
    for k, v in fields.items():
        w = vars(b)[k]
        assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v is w or v == w, k


def test_checked_is_the_direct_checker():
    _same_carrier(maskforms.checked(COLOR, (H, W), 'e', img=IMG), colormask.as_color_masks(COLOR, (H, W), 'e', img=IMG))
    _same_carrier(maskforms.checked(POLY, (H, W), 'e'), polygon.as_polys(POLY, (H, W), 'e'))
    _same_carrier(maskforms.checked(RLE_DICTS, (H, W), 'e'), rle.as_masks(RLE_DICTS, (H, W), 'e'))
    _same_carrier(maskforms.checked([], (H, W), 'e'), rle.as_masks([], (H, W), 'e'))       # the empty list: RLE, sized by hw
    for dense in (DENSE, ENTRIES[11], ENTRIES[12]):
        assert maskforms.checked(dense, (H, W), 'e') is dense
        assert maskforms.dense(dense) is dense
    assert np.array_equal(maskforms.dense(maskforms.checked(COLOR, (H, W), img=IMG)),
                          colormask.as_color_masks(COLOR, (H, W)).dense(IMG))
    assert np.array_equal(maskforms.dense(dict(POLY, size=[H, W])), polygon.as_polys(POLY, (H, W)).dense())
    assert np.array_equal(maskforms.dense(RLE_DICTS), DENSE)


def test_checked_one_is_the_direct_checker_of_one_mask():
    one_c = {'bboxes': COLOR['bboxes'][:1], 'colors': COLOR['colors'][:1]}
    one_p = {'polygons': POLY['polygons'][1]}                   # the parts of ONE instance
    _same_carrier(maskforms.checked_one(one_c, (H, W), 's'), colormask.as_color_masks(one_c, (H, W), 's'))
    _same_carrier(maskforms.checked_one(one_p, (H, W), 's'), polygon.as_polys(one_p, (H, W), 's', single=True))
    for item in (RLE_DICTS[0], PAIRS[1], rle.as_masks(RLE_DICTS[:1], (H, W))):
        _same_carrier(maskforms.checked_one(item, (H, W), 's'),
                      rle.as_masks(item if isinstance(item, rle.RleMasks) else [item], (H, W), 's'))
    one = DENSE[0]
    assert maskforms.checked_one(one, (H, W), 's') is one


def _text(fn, *a, **k):
    with pytest.raises(ValueError) as err:
        fn(*a, **k)
    return str(err.value)


def test_the_refusals_are_the_checkers_own():
    big = (H + 1, W)
    for wrong in (COLOR, (H - 2, W)), (colormask.as_color_masks(COLOR, (H, W)), big):    # a box outside; another size
        assert _text(maskforms.checked, *wrong, 'qry_isegmaps[0]', img=IMG) == \
            _text(colormask.as_color_masks, *wrong, 'qry_isegmaps[0]', img=IMG)
    assert _text(maskforms.checked, dict(POLY, size=[H, W]), big, 'qry_isegmaps[1]') == \
        _text(polygon.as_polys, dict(POLY, size=[H, W]), big, 'qry_isegmaps[1]')
    assert _text(maskforms.checked, RLE_DICTS, big, 'qry_isegmaps[2]') == _text(rle.as_masks, RLE_DICTS, big, 'qry_isegmaps[2]')
    assert _text(maskforms.checked_one, RLE_DICTS[0], big, 'spp_isegmaps[3]') == \
        _text(rle.as_masks, [RLE_DICTS[0]], big, 'spp_isegmaps[3]')
    # two masks for one support instance, in the two forms that can hold two
    for two in (COLOR, rle.as_masks(RLE_DICTS, (H, W))):
        assert _text(maskforms.checked_one, two, (H, W), 'spp_isegmaps[4]') == \
            'spp_isegmaps[4]: one mask per support instance, got 2'


def test_gt_entries_refuses_a_colour_entry_without_image_bytes():
    from fgn_amd.detector import _gt_entries
    text = _text(_gt_entries, [DENSE, COLOR], [(H, W)] * 2, None)
    assert text.startswith('qry_isegmaps[1]: a box + colour entry is made into a mask from the image\'s bytes')
    got = _gt_entries([DENSE, COLOR, POLY, RLE_DICTS, []], [(H, W)] * 5, [torch.from_numpy(IMG)] * 5)
    assert got[0] is DENSE and [type(g) for g in got[1:]] == \
        [colormask.ColorMasks, polygon.PolyMasks, rle.RleMasks, rle.RleMasks]
    assert got[1].img is not None and len(got[4]) == 0 and got[4].shape == (0, H, W)


def test_collate_leaves_compact_entries_and_items_as_they_are():
    one_c = {'bboxes': COLOR['bboxes'][:1], 'colors': COLOR['colors'][:1]}
    items = [DENSE[0], RLE_DICTS[0], PAIRS[1], one_c, colormask.as_color_masks(one_c, (H, W)),
             {'polygons': [TRI]}, polygon.as_polys({'polygons': [TRI]}, (H, W), single=True),
             rle.as_masks(RLE_DICTS[:1], (H, W)), DENSE[1].tolist()]
    entries = [e for e in ENTRIES if not isinstance(e, dict) or maskforms.form_of(e) is not None]
    samples = [{'qry_isegmaps': e, 'spp_isegmaps': items} for e in entries]
    batch = collate(samples)
    for e, got in zip(entries, batch['qry_isegmaps']):
        if maskforms.form_of(e) is None:
            assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), np.asarray(e))
        else:
            assert got is e
    for lst in batch['spp_isegmaps']:
        for item, got in zip(items, lst):
            if maskforms.form_of_one(item) is None:
                assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), np.asarray(item))
            else:
                assert got is item
