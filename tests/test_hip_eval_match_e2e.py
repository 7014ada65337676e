"""``FGN.evaluate_on_device`` end to end: the matched bits a result dict carries are ``match_flags`` of that very dict,
the evaluator returns what it returns for the switch-off run, every other key is byte-equal to the ``match_on_device``
run - eager, captured and replayed, at source size, under both paste semantics - and with the switch off nothing is
added or launched."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH, N_WAYS = 2, 3
BASE_KEYS = {'dt_scores', 'dt_bboxes', 'dt_cat_ids', 'dt_isegmaps_rle', 'idx', 'qry_bboxes', 'qry_img_shape', 'qry_cat_ids',
             'qry_child_idx', 'cats_ids_to_sample_real', 'spp_insts_ids', 'qry_isegmaps_rle'}
COUNT_KEYS = {'dt_gt_inter', 'dt_area', 'gt_area'}
FLAG_KEYS = {'dt_match_bbox', 'dt_match_segm', 'eval_iou_thrs', 'gt_per_cat'}
# ten thresholds from loose to strict: the detections of a randomly initialised model overlap their ground truth little
TEN = (0.01, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.75)


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, 2, width_div=2)
    return FGN(N_WAYS, 2, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


@pytest.fixture(scope='module')
def setup():
    from fgn_amd.episodes import make_batch
    model = _model()
    eps = [make_batch(11 * q, BATCH, N_WAYS, 2, 160, 224, 64) for q in range(2)]
    assert not model.evaluate_on_device and tuple(model.eval_iou_thrs) == (0.5,)        # the defaults
    off = [model.simple_test(**e, rescale=True) for e in eps]                           # both switches off, eager
    model.match_on_device = True
    counts = [model.simple_test(**e, rescale=True) for e in eps]                        # the counts alone
    model.match_on_device = False
    assert all(len(r['dt_scores']) > 0 for w in off for r in w)
    return model, eps, off, counts


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _check(got, off, counts, thrs=(0.5,), segm=True):
    """``got`` (switch on) against the run with both switches off and the run with the counts alone"""
    from fgn_amd.fsiseg_eval import evaluate_results, evaluate_results_multi, gt_per_cat, match_flags
    assert len(got) == len(off) == len(counts)
    matched = 0
    for i, (g, o, c) in enumerate(zip(got, off, counts)):
        assert set(g) == set(c) | (FLAG_KEYS if segm else FLAG_KEYS - {'dt_match_segm'})
        for k in c:                                                    # the counts and every other key: byte-equal
            assert _same(g[k], c[k]), (i, k)
        assert set(c) - set(o) <= COUNT_KEYS and all(_same(c[k], o[k]) for k in o)
        n = len(g['dt_scores'])
        for kind in ('bbox', 'segm') if segm else ('bbox',):
            f = g['dt_match_' + kind]
            assert f.dtype == np.int32 and f.shape == (n,)
            assert np.array_equal(f, match_flags(c, thrs, kind, n_ways=N_WAYS)), (i, kind)
            matched += int((f > 0).sum())
        assert g['eval_iou_thrs'].dtype == np.float64 and g['eval_iou_thrs'].tolist() == list(thrs)
        assert g['gt_per_cat'].dtype == np.int32 and np.array_equal(g['gt_per_cat'], gt_per_cat(c['qry_cat_ids'], N_WAYS))
    print('matched bits:', matched, 'thresholds:', len(thrs))
    assert matched > 0 or len(thrs) == 1                               # the episodes do match their ground truth
    if not segm:                                                       # (no masks came with the call: boxes alone)
        from fgn_amd.fsiseg_eval import FSISEGEval
        for t in thrs:
            assert FSISEGEval(results=got, n_ways=N_WAYS, iou_type='bbox', iou_thr=t).run() == \
                FSISEGEval(results=off, n_ways=N_WAYS, iou_type='bbox', iou_thr=t).run()
        return
    assert evaluate_results(got, N_WAYS, iou_thr=thrs[0]) == evaluate_results(off, N_WAYS, iou_thr=thrs[0])
    if len(thrs) > 1:
        assert evaluate_results_multi(got, N_WAYS, thrs) == evaluate_results_multi(off, N_WAYS, thrs)


def _count_ops(monkeypatch):
    """every function of ``fgn_amd.ops`` counts its calls"""
    from fgn_amd import ops
    calls = {}
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith('_'):
            def wrap(*a, _fn=fn, _name=name, **k):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(*a, **k)
            monkeypatch.setattr(ops, name, wrap)
    return calls


def test_switch_off_adds_and_launches_nothing(setup, monkeypatch):
    model, eps, off, counts = setup
    assert all(set(r) == BASE_KEYS for w in off for r in w)
    assert all(set(r) == BASE_KEYS | COUNT_KEYS for w in counts for r in w)
    calls = _count_ops(monkeypatch)
    assert _same(model.simple_test(**eps[0], rescale=True), off[0])
    n_off = dict(calls)
    assert all('mt_buf' not in s for ring in model._pinned.values() for s in ring)      # no new pinned buffer
    assert not {'eval_match', 'mask_overlap', 'mask_bits'} & set(n_off)
    calls.clear()
    model.match_on_device = True
    try:
        model.simple_test(**eps[0], rescale=True)
    finally:
        model.match_on_device = False
    n_counts = dict(calls)
    calls.clear()
    model.evaluate_on_device = True
    try:
        model.simple_test(**eps[0], rescale=True)
    finally:
        model.evaluate_on_device = False
    n_on = dict(calls)
    # the switch implies the counts and adds one eval_match per image to them - nothing else
    assert {k: v for k, v in n_on.items() if k != 'eval_match'} == n_counts and n_on['eval_match'] == BATCH
    assert 'eval_match' not in n_counts and sum(n_counts.values()) > sum(n_off.values())
    calls.clear()
    assert _same(model.simple_test(**eps[0], rescale=True), off[0])                    # off again: today's calls
    assert dict(calls) == n_off


def test_flags_eager(setup):
    model, eps, off, counts = setup
    model.evaluate_on_device = True
    try:
        for e, o, c in zip(eps, off, counts):
            _check(model.simple_test(**e, rescale=True), o, c)
        model.eval_iou_thrs = TEN
        for e, o, c in zip(eps, off, counts):
            _check(model.simple_test(**e, rescale=True), o, c, TEN)
        # without ground-truth masks: bbox bits only, and no counts; without boxes or labels: no flag key
        e = dict(eps[0], qry_isegmaps=None)
        got = model.simple_test(**e, rescale=True)
        base = [{k: v for k, v in r.items() if k != 'qry_isegmaps_rle'} for r in off[0]]
        _check(got, base, base, TEN, segm=False)
        got = model.simple_test(**dict(eps[0], qry_cat_ids=None), rescale=True)
        assert all(set(r) == BASE_KEYS | COUNT_KEYS for r in got)
    finally:
        model.evaluate_on_device = False
        model.eval_iou_thrs = (0.5,)


def test_flags_under_graph_capture_and_replay(setup):
    model, eps, off, counts = setup
    model.use_graphs = True
    try:
        first = [model.simple_test(**e, rescale=True) for e in eps]    # captures; the switch is no part of the cache key
        n_graphs = len(model._graphs)
        assert _same(first, off)
        model.evaluate_on_device = True
        model.eval_iou_thrs = TEN
        for rep in range(2):                                           # replays of the graph captured above
            for e, o, c in zip(eps, off, counts):
                _check(model.simple_test(**e, rescale=True), o, c, TEN)
        assert len(model._graphs) == n_graphs                          # the matching launch is eager: no new graph
        model.evaluate_on_device = False
        for e, o in zip(eps, off):
            assert _same(model.simple_test(**e, rescale=True), o)
    finally:
        model.use_graphs = False
        model.evaluate_on_device = False
        model.eval_iou_thrs = (0.5,)


def test_graph_captured_with_the_switch_on(setup):
    """a fresh model whose FIRST graphed call has the switch on: capture, then replay"""
    _, eps, off, counts = setup
    model = _model()
    model.use_graphs = True
    model.evaluate_on_device = True
    model.eval_iou_thrs = TEN
    _check(model.simple_test(**eps[0], rescale=True), off[0], counts[0], TEN)  # capture
    _check(model.simple_test(**eps[1], rescale=True), off[1], counts[1], TEN)  # replay
    _check(model.simple_test(**eps[0], rescale=True), off[0], counts[0], TEN)  # replay
    assert len(model._graphs) == 1


def test_flags_under_the_other_paste_semantics(setup):
    _, eps, _, _ = setup
    model = _model()
    model.paste_semantics = 'cuda'
    off = model.simple_test(**eps[0], rescale=True)
    model.match_on_device = True
    counts = model.simple_test(**eps[0], rescale=True)
    model.match_on_device = False
    model.evaluate_on_device = True
    model.eval_iou_thrs = TEN
    _check(model.simple_test(**eps[0], rescale=True), off, counts, TEN)


def test_flags_at_source_size():
    """source-size queries: the bits are formed against the scaled ground-truth boxes without ``results_at_source``, and
    with it from the boxes the device divides, against the boxes as given"""
    from fgn_amd import fewshot_ds as fd
    from fgn_amd.episodes import collate
    net, pool, sizes = 128, 160, [(150, 131), (101, 77)]
    ds = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=2, n_imgs=8, img_size=pool,
                                      spp_img_size=64, raw_uint8=True)
    src = []
    for i, (h, w) in enumerate(sizes):                                 # the top-left window of a pool sample
        s = ds[i]
        masks = np.asarray(s['qry_isegmaps'])[:, :h, :w]
        boxes = np.asarray(s['qry_bboxes'], np.float32).copy()
        boxes[:, [0, 2]] = boxes[:, [0, 2]].clip(0, h)
        boxes[:, [1, 3]] = boxes[:, [1, 3]].clip(0, w)
        keep = masks.any((1, 2)) & (boxes[:, 2] - boxes[:, 0] >= 2) & (boxes[:, 3] - boxes[:, 1] >= 2)
        assert keep.any()
        s = dict(s)
        s.update(qry_img=s['qry_img'][:h, :w].contiguous(), qry_isegmaps=np.ascontiguousarray(masks[keep]),
                 qry_bboxes=boxes[keep], qry_cat_ids=np.asarray(s['qry_cat_ids'])[keep],
                 qry_cat_ids_real=np.asarray(s['qry_cat_ids_real'])[keep],
                 img_shape=np.array([net, net, 3], np.int32), qry_resize_to=np.array([net, net], np.int32))
        src.append(s)
    imgs = [s.pop('qry_img') for s in src]
    bs = collate(src)
    bs['qry_img'] = imgs
    model = _model()
    model.query_source_capacity = 3 * pool * pool
    model.set_input_norm(**ds.input_norm)
    for kw in (dict(results_at_source=True), dict()):
        model.match_on_device = model.evaluate_on_device = False
        off = model.simple_test(**bs, rescale=True, **kw)
        model.match_on_device = True
        counts = model.simple_test(**bs, rescale=True, **kw)
        model.match_on_device = False
        model.evaluate_on_device = True
        model.eval_iou_thrs = TEN
        _check(model.simple_test(**bs, rescale=True, **kw), off, counts, TEN)
