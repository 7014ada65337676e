"""The evaluator on result dicts that carry the exact overlap counts (``dt_gt_inter`` / ``dt_area`` / ``gt_area``, what
``FGN.match_on_device`` adds): every value it produces equals the RLE-decoding path's, and no RLE is decoded."""
import numpy as np
import pytest

from fgn_amd import fsiseg_eval as E
from fgn_amd import rle

H, W, N_WAYS = 64, 80, 3


def _ellipse(rng):
    yy, xx = np.mgrid[:H, :W]
    cy, cx = rng.uniform(10, H - 10), rng.uniform(10, W - 10)
    ry, rx = rng.uniform(4, 20), rng.uniform(4, 25)
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1


def _box(m):
    if not m.any():
        return np.array([3., 4., 9., 11.], np.float32)
    ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return np.array([ys[0], xs[0], ys[-1] + 1, xs[-1] + 1], np.float32)           # YXYX


def _image(seed, n_gt, n_dt, gt_cats, dt_cats):
    rng = np.random.default_rng(seed)
    gts = [_ellipse(rng) for _ in range(n_gt)]
    # detections: jittered copies of the ground truth (matches above and below IoU 0.5) and free ellipses
    dts = []
    for k in range(n_dt):
        if gts and k < 2 * n_gt:
            m = np.roll(gts[k % n_gt], (int(rng.integers(-6, 7)), int(rng.integers(-8, 9))), (0, 1))
        else:
            m = _ellipse(rng)
        dts.append(m)
    if seed == 0:
        dts[1] = np.zeros((H, W), bool)             # a detection with an empty mask
        gts[1] = np.zeros((H, W), bool)             # an empty ground-truth mask
    gts, dts = np.array(gts).reshape(-1, H, W), np.array(dts).reshape(-1, H, W)
    res = {'qry_img_shape': np.array([H, W, 3]),
           'qry_bboxes': np.array([_box(m) for m in gts], np.float32).reshape(-1, 4),
           'qry_cat_ids': np.asarray(gt_cats, np.int64),
           'qry_isegmaps_rle': rle.encode_many(gts),
           'dt_bboxes': np.array([_box(m) for m in dts], np.float32).reshape(-1, 4),
           'dt_cat_ids': np.asarray(dt_cats, np.int64),
           'dt_scores': rng.uniform(0.05, 1.0, len(dts)).astype(np.float32),
           'dt_isegmaps_rle': rle.encode_many(dts)}
    d2, g2 = dts.reshape(len(dts), -1), gts.reshape(len(gts), -1)
    counts = {'dt_gt_inter': (d2[:, None, :] & g2[None, :, :]).sum(-1).astype(np.int32).reshape(len(dts), len(gts)),
              'dt_area': d2.sum(-1).astype(np.int32), 'gt_area': g2.sum(-1).astype(np.int32)}
    return res, counts


@pytest.fixture(scope='module')
def results():
    """(without the keys, with the keys on every image, with the keys on images 0 and 2 only)"""
    spec = [(0, 4, 9, [0, 0, 1, 2], [0, 0, 0, 1, 1, 2, 2, 0, 1]),
            (1, 3, 7, [0, 0, 1], [0, 1, 2, 2, 0, 1, 2]),           # category 2: detections, no ground truth
            (2, 2, 5, [1, 2], [1, 2, 1, 2, 0])]
    plain, full = [], []
    for s in spec:
        res, counts = _image(*s)
        plain.append(res)
        full.append({**res, **counts})
    mixed = [full[0], plain[1], full[2]]
    return plain, full, mixed


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def _everything(res_list, kind):
    ev = E.FSISEGEval(results=res_list, n_ways=N_WAYS, iou_type=kind)
    summary = ev.run()
    per = {k: (None if v is None else (v[0], v[1], v[2])) for k, v in ev._per.items()}
    imgs, gts, dts = ev.annotations()
    return dict(summary=summary, per=per, precision=ev.eval['precision'], recall=ev.eval['recall'],
                gt_area=[g['area'] for g in gts], dt_area=[d['area'] for d in dts], groups=list(ev.groups()),
                types=[type(r['area']).__name__ for r in gts + dts])


@pytest.mark.parametrize('kind', ['segm', 'bbox'])
def test_counts_give_the_same_evaluation(results, kind):
    plain, full, mixed = results
    want = _everything(plain, kind)
    assert any(v is not None and v[1].any() for v in want['per'].values())          # something matches ...
    assert any(v is not None and len(v[1]) and not v[1].all() for v in want['per'].values())   # ... and something does not
    assert 0 in want['dt_area'] and 0 in want['gt_area']
    assert _same(_everything(full, kind), want)
    assert _same(_everything(mixed, kind), want)
    assert _same(E.evaluate_results(full, N_WAYS), E.evaluate_results(plain, N_WAYS))


def test_no_rle_is_decoded_when_every_image_carries_the_counts(results, monkeypatch):
    plain, full, _ = results
    want = {kind: _everything(plain, kind) for kind in ('segm', 'bbox')}

    def boom(*a, **k):
        raise AssertionError('an RLE was decoded although the result carries the counts')
    monkeypatch.setattr(E, '_mask_iou', boom)
    monkeypatch.setattr(E._rle, 'decode', boom)
    for kind in ('segm', 'bbox'):
        assert _same(_everything(full, kind), want[kind])
