"""Result dicts for the tests of the matched bits (``fsiseg_eval.match_flags`` / ``ops.eval_match``): random small
images and crafted edge cases, plus the evaluator's greedy matching written out once more (``plain_evaluate_img``: the
double loop ``FSISEGEval._evaluate_img`` has always been), so that the rule is pinned by a statement that shares no
helper with the code under test."""
import numpy as np

N_WAYS = 3
THR_SETS = {1: (0.5,), 10: tuple(np.linspace(.5, 0.95, 10).tolist()),
            16: tuple(np.linspace(0.05, 0.8, 16).tolist())}


def plain_evaluate_img(res, cat, iou_type, iou_thr, max_dets=100):
    """(scores, dtm, n_gt) of one (image, category), or None: the evaluator's rule from the counts / boxes of the dict."""
    g_sel = np.flatnonzero(np.asarray(res['qry_cat_ids']).reshape(-1) == cat)
    d_sel = np.flatnonzero(np.asarray(res['dt_cat_ids']).reshape(-1) == cat)
    if len(g_sel) == 0 and len(d_sel) == 0:
        return None
    scores = np.asarray(res['dt_scores'], np.float64).reshape(-1)[d_sel]
    order = np.argsort(-scores, kind='mergesort')[:max_dets]
    d_sel, scores = d_sel[order], scores[order]
    if iou_type == 'segm':
        da, ga = np.asarray(res['dt_area']).reshape(-1), np.asarray(res['gt_area']).reshape(-1)
        inter = np.asarray(res['dt_gt_inter']).reshape(len(da), len(ga))[np.ix_(d_sel, g_sel)].astype(np.float64)
        union = da[d_sel].astype(np.float64)[:, None] + ga[g_sel].astype(np.float64)[None, :] - inter
        with np.errstate(invalid='ignore', divide='ignore'):
            ious = np.where(union > 0, inter / union, 0.0)
    else:
        def xywh(b):
            b = np.asarray(b).reshape(-1, 4)
            one = b.dtype.type(1)
            return np.column_stack((b[:, 1], b[:, 0], np.maximum(b[:, 3] - b[:, 1], one),
                                    np.maximum(b[:, 2] - b[:, 0], one))).astype(np.float64)
        d, g = xywh(res['dt_bboxes'])[d_sel], xywh(res['qry_bboxes'])[g_sel]
        ious = np.zeros((len(d), len(g)))
        for i in range(len(d)):
            for j in range(len(g)):
                w = max(min(d[i, 0] + d[i, 2], g[j, 0] + g[j, 2]) - max(d[i, 0], g[j, 0]), 0.0)
                h = max(min(d[i, 1] + d[i, 3], g[j, 1] + g[j, 3]) - max(d[i, 1], g[j, 1]), 0.0)
                ious[i, j] = w * h / (d[i, 2] * d[i, 3] + g[j, 2] * g[j, 3] - w * h)
    thr = min(iou_thr, 1 - 1e-10)
    gtm = np.zeros(len(g_sel), bool)
    dtm = np.zeros(len(d_sel), bool)
    for di in range(len(d_sel)):
        best, m = thr, -1
        for gi in range(len(g_sel)):
            if gtm[gi] or ious[di, gi] < best:
                continue
            best, m = ious[di, gi], gi
        if m >= 0:
            gtm[m] = True
            dtm[di] = True
    return scores, dtm, len(g_sel), d_sel


def plain_flags(res, thrs, iou_type, max_dets=100, n_ways=N_WAYS):
    """``match_flags`` from ``plain_evaluate_img``."""
    cats = np.asarray(res['dt_cat_ids']).reshape(-1)
    flags = np.where((cats >= 0) & (cats < n_ways), -1, 0).astype(np.int32)
    for k in range(n_ways):
        for t, thr in enumerate(thrs):
            e = plain_evaluate_img(res, k, iou_type, thr, max_dets)
            if e is None:
                continue
            if t == 0:
                flags[e[3]] = 0
            flags[e[3]] |= e[1].astype(np.int32) << t
    return flags


def make_res(scores, boxes, cats, gt_boxes, gt_cats, inter, d_area, g_area):
    n, g = len(scores), len(gt_cats)
    return {'dt_scores': np.asarray(scores, np.float32).reshape(n),
            'dt_bboxes': np.asarray(boxes, np.float32).reshape(n, 4),
            'dt_cat_ids': np.asarray(cats, np.int64).reshape(n),
            'qry_bboxes': np.asarray(gt_boxes, np.float32).reshape(g, 4),
            'qry_cat_ids': np.asarray(gt_cats, np.int64).reshape(g),
            'dt_gt_inter': np.asarray(inter, np.int32).reshape(n, g),
            'dt_area': np.asarray(d_area, np.int32).reshape(n), 'gt_area': np.asarray(g_area, np.int32).reshape(g),
            'qry_img_shape': np.array([64, 64, 3], np.int32)}


def _boxes(rng, n, grid):
    """YXYX float32; ``grid``: integer corners on a coarse lattice (many exactly equal IoUs), else fractional."""
    if grid:
        y0, x0 = rng.randint(0, 6, n) * 8.0, rng.randint(0, 6, n) * 8.0
        h, w = rng.randint(0, 4, n) * 8.0, rng.randint(0, 4, n) * 8.0          # 0: narrower than 1, clamps to 1
    else:
        y0, x0 = rng.rand(n) * 40, rng.rand(n) * 40
        h, w = rng.rand(n) * 30, rng.rand(n) * 30
    return np.stack([y0, x0, y0 + h, x0 + w], 1).astype(np.float32)


def random_res(seed, d=None, g=None, tie_scores=None, outside_labels=True):
    """One random image: D in 0..130, G in 0..70 unless given; small integer counts (equal IoUs are frequent), some
    empty masks (a union of 0), scores from a few levels in half of the images (ties), a label outside the ways now
    and then."""
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 131) if d is None else d
    g = rng.randint(0, 71) if g is None else g
    tie_scores = bool(seed & 1) if tie_scores is None else tie_scores
    scores = rng.randint(1, 8, d) / 8.0 if tie_scores else rng.rand(d)
    cats = rng.randint(0, N_WAYS, d)
    if outside_labels and d:
        cats[rng.rand(d) < 0.03] = N_WAYS + 1
    gt_cats = rng.randint(0, N_WAYS, g)
    d_area, g_area = rng.randint(0, 7, d), rng.randint(0, 7, g)
    inter = np.minimum(rng.randint(0, 7, (d, g)), np.minimum(d_area[:, None], g_area[None, :]))
    grid = bool(seed & 2)
    return make_res(scores, _boxes(rng, d, grid), cats, _boxes(rng, g, grid), gt_cats, inter, d_area, g_area)


def crafted():
    """name -> (res, thresholds, max_dets, expected flags per IoU type or None)."""
    out = {}
    unit = [0, 0, 8, 8]
    # equal scores inside a category: index order decides who takes the only ground truth
    out['equal_scores'] = (make_res([.5, .5, .5], [unit] * 3, [0, 0, 0], [unit], [0], [[4], [4], [4]], [4] * 3, [4]),
                           (0.5,), 100, {'bbox': [1, 0, 0], 'segm': [1, 0, 0]})
    # two ground truths with identical IoU: the larger index is taken first, the smaller by the next detection
    out['equal_ious'] = (make_res([.9, .8, .7], [unit] * 3, [1, 1, 1], [unit, unit], [1, 1], [[4, 4]] * 3, [4] * 3, [4, 4]),
                         (0.5,), 100, {'bbox': [1, 1, 0], 'segm': [1, 1, 0]})
    # which one it was shows where the second detection overlaps the first ground truth only
    out['larger_index_wins'] = (make_res([.9, .8], [unit, unit], [0, 0], [unit, unit], [0, 0], [[3, 3], [0, 3]],
                                         [3, 3], [3, 3]), (0.5,), 100, {'segm': [1, 0], 'bbox': [1, 1]})
    # IoU exactly at the threshold: segm 1 / (1 + 2 - 1), bbox [0,0,1,2] against [0,0,1,1] = 1 / 2
    out['iou_at_threshold'] = (make_res([.9], [[0, 0, 1, 2]], [0], [[0, 0, 1, 1]], [0], [[1]], [1], [2]),
                               (0.5, 0.5 + 2 ** -40), 100, {'bbox': [1], 'segm': [1]})
    # a threshold of 1.0 becomes 1 - 1e-10: an exact overlap matches
    out['threshold_one'] = (make_res([.9, .8], [unit, [0, 0, 8, 9]], [2, 2], [unit, unit], [2, 2], [[5, 5], [5, 5]],
                                     [5, 6], [5, 5]), (1.0, 0.5), 100, {'bbox': [3, 2], 'segm': [3, 2]})
    # a union of 0: IoU 0, matches at no positive threshold - and at threshold 0 it does
    out['union_zero'] = (make_res([.9], [unit], [0], [unit], [0], [[0]], [0], [0]), (0.5, 0.0), 100,
                         {'segm': [2], 'bbox': [3]})
    # a box narrower than 1 clamps to 1: [0,0,8,0.25] is 1 x 8 against a 1 x 8 ground truth
    out['narrow_box'] = (make_res([.9], [[0, 0, 8, 0.25]], [0], [[0, 0, 8, 1]], [0], [[1]], [1], [1]), (1.0,), 100,
                         {'bbox': [1], 'segm': [1]})
    # 130 detections of one category, max_dets 100: the 30 lowest scores are not evaluated
    sc = np.linspace(0.1, 0.9, 130)[np.random.RandomState(3).permutation(130)]
    r = make_res(sc, [unit] * 130, [1] * 130, [unit] * 3, [1, 1, 0], np.full((130, 3), 2), [2] * 130, [2] * 3)
    want = np.zeros(130, np.int32)
    by = np.argsort(-sc.astype(np.float32).astype(np.float64), kind='mergesort')
    want[by[:2]] = 1
    want[by[100:]] = -1
    out['beyond_max_dets'] = (r, (0.5,), 100, {'bbox': want.tolist(), 'segm': want.tolist()})
    # a label outside the ways is 0, whatever it overlaps
    out['label_outside'] = (make_res([.9, .8, .7], [unit] * 3, [3, -1, 0], [unit], [0], [[4]] * 3, [4] * 3, [4]), (0.5,),
                            100, {'bbox': [0, 0, 1], 'segm': [0, 0, 1]})
    out['no_ground_truth'] = (random_res(5, d=7, g=0), (0.5, 0.75), 100, {'bbox': [0] * 7, 'segm': [0] * 7})
    out['no_detections'] = (random_res(6, d=0, g=5), (0.5,), 100, {'bbox': [], 'segm': []})
    return out
