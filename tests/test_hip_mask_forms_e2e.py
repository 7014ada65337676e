"""All four forms of a mask in ONE batch: four query images whose ground truth comes dense (none), as
COCO RLE, as box + colour and as COCO polygons, with source-size supports whose N*K masks cycle through the four forms -
against the twin call in which every entry is its carrier's host ``dense()``, every result key byte for byte, eager and
under a replayed graph, with one decode, one colour and one polygon call for the query side and one each for the
supports.  The batch in which a wrong precedence of the forms, or a dropped list of instances, shows."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import colormask as cm
from fgn_amd import fewshot_ds as fd
from fgn_amd import polygon, rle
from fgn_amd.episodes import collate, star_polygon

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
NK = N_WAYS * K_SHOTS
FORMS = ('dense', 'rle', 'colour', 'poly')


def _query(sample: dict, form: str, seed: int) -> tuple:
    """The top-left NET x NET window of a pool sample as the query, its ground truth in ``form`` (the dense image has no
    instance) -> (the entry, its carrier's host ``dense()``, the annotations that go with it)."""
    img = sample['qry_img'][:NET, :NET].contiguous()
    boxes = sample['qry_isegmaps'].boxes.clip(0, NET)
    keep = (boxes[:, 2] - boxes[:, 0] >= 6) & (boxes[:, 3] - boxes[:, 1] >= 6)
    assert keep.any()
    if form == 'dense':
        keep[:] = False
    boxes = boxes[keep]
    if form == 'colour':        # the colour of a pixel inside each box: that pixel, at the least, is in the mask
        entry = {'bboxes': boxes, 'colors': np.stack([img[(y0 + y1) // 2, (x0 + x1) // 2].numpy() for y0, x0, y1, x1 in boxes])}
        dense = cm.as_color_masks(entry, (NET, NET)).dense(img)
    elif form == 'poly':
        rng = np.random.RandomState(seed)
        entry = {'polygons': [[star_polygon(rng, *[float(v) for v in b])] for b in boxes]}
        dense = polygon.as_polys(entry, (NET, NET)).dense()
    else:
        dense = sample['qry_isegmaps'].dense(sample['qry_img'])[keep][:, :NET, :NET]
        entry = rle.encode_many(dense) if form == 'rle' else dense
        if form == 'rle':
            dense = rle.as_masks(entry, (NET, NET)).dense()
    assert len(dense) == len(boxes) and all(m.any() for m in dense)
    ann = dict(qry_img=img, qry_bboxes=boxes.astype(np.float32), qry_cat_ids=np.asarray(sample['qry_cat_ids'])[keep],
               qry_cat_ids_real=np.asarray(sample['qry_cat_ids_real'])[keep], img_shape=np.array([NET, NET, 3], np.int32))
    return entry, dense, ann


def _supports(sample: dict, first: int, seed: int) -> tuple:
    """The N*K support masks of a sample, instance i in the form ``FORMS[(first + i) % 4]`` -> (the items, the host
    ``dense()`` of each)."""
    rng = np.random.RandomState(seed)
    items, dense = [], []
    for i, (im, mk, bb) in enumerate(zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])):
        form, hw = FORMS[(first + i) % 4], tuple(im.shape[:2])
        if form == 'poly':
            item = {'polygons': [star_polygon(rng, *[float(v) for v in bb])]}
            d = polygon.as_polys(item, hw, single=True).dense()[0]
        else:
            d = mk.dense(im)[0]
            item = mk if form == 'colour' else rle.encode(d) if form == 'rle' else d
            if form == 'rle':
                d = rle.as_masks([item], hw).dense()[0]
        assert d.any()
        items.append(item)
        dense.append(d)
    return items, dense


@contextlib.contextmanager
def _launches():
    """Counts the calls of the three private launchers of ``ops`` while it is entered: name -> [records of each call]."""
    from fgn_amd import ops
    real = {n: getattr(ops, n) for n in ('_rle_decode', '_color_launch', '_poly_launch')}
    calls = {n: [] for n in real}
    size = {'_rle_decode': lambda a: a[1].shape[0], '_color_launch': lambda a: a[1].shape[0], '_poly_launch': lambda a: len(a[0])}
    for n in real:
        setattr(ops, n, lambda *a, _n=n, **k: calls[_n].append(size[_n](a)) or real[_n](*a, **k))
    try:
        yield calls
    finally:
        for n, f in real.items():
            setattr(ops, n, f)


def _same_results(want, got):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
            elif isinstance(a[k], (list, tuple)) and len(a[k]) and isinstance(a[k][0], np.ndarray):
                assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) and len(a[k]) == len(b[k]), k
            else:
                assert a[k] == b[k], k


def test_one_batch_in_which_all_four_forms_meet():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    ds = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                      spp_img_size=SPP, raw_uint8=True, spp_source=True, color_masks=True)
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    m = FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
            test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    m.query_source_capacity = m.support_source_capacity = 3 * POOL * POOL
    m.set_input_norm(**ds.input_norm)
    m.match_on_device = m.evaluate_on_device = True
    mixed, twin = [], []
    for i, form in enumerate(FORMS):
        sample = ds[i]
        entry, dense, ann = _query(sample, form, 90 + i)
        items, sdense = _supports(sample, i, 95 + i)
        mixed.append(dict(sample, **ann, qry_isegmaps=entry, spp_isegmaps=items))
        twin.append(dict(sample, **ann, qry_isegmaps=dense, spp_isegmaps=sdense))
    mixed, twin = collate(mixed), collate(twin)
    n = [len(g) for g in twin['qry_isegmaps']]
    assert n[0] == 0 and min(n[1:]) > 0
    assert [type(g) for g in mixed['qry_isegmaps']] == [torch.Tensor, list, dict, dict]
    want = m.simple_test(**twin, rescale=True)
    assert want[0]['qry_isegmaps_rle'] == [] and all(len(w['qry_isegmaps_rle']) == k for w, k in zip(want, n))
    with _launches() as calls:
        _same_results(want, m.simple_test(**mixed, rescale=True))
    per_form = len(FORMS) * NK // 4                 # the support instances of each form
    assert sorted(calls['_rle_decode']) == sorted([n[1], len(FORMS) * NK])      # (one record per row of the mask slot)
    assert sorted(calls['_color_launch']) == sorted([n[2], per_form])
    assert sorted(calls['_poly_launch']) == sorted([n[3], per_form])
    m.use_graphs = True
    for rep in range(2):                            # captured, then replayed
        _same_results(want, m.simple_test(**mixed, rescale=True))
