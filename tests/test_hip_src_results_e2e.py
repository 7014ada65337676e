"""Results at source size through the detector (``results_at_source``) against the same call without the
flag: the same detections, scores and order; boxes divided by the image's scale; masks pasted at the source size from
those boxes; the ground truth encoded and counted as given - eager, graphed, with the overlap counts, through the dense
fallback, and the contract error.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import rle
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
OVERLAP = ('dt_gt_inter', 'dt_area', 'gt_area')
CASES = [(0, [(150, 131)]), (1, [(101, 77)]), (3, [(64, 160)]), (0, [(150, 131), (101, 77)])]


def _crop(sample: dict, size) -> dict:
    """The top-left (h, w) window of a pool sample as a source-size query: image, masks and boxes cut to it."""
    h, w = size
    masks = np.asarray(sample['qry_isegmaps'])[:, :h, :w]
    boxes = np.asarray(sample['qry_bboxes'], np.float32).copy()
    boxes[:, [0, 2]] = boxes[:, [0, 2]].clip(0, h)
    boxes[:, [1, 3]] = boxes[:, [1, 3]].clip(0, w)
    keep = masks.any((1, 2)) & (boxes[:, 2] - boxes[:, 0] >= 2) & (boxes[:, 3] - boxes[:, 1] >= 2)
    assert keep.any()
    out = dict(sample)
    out.update(qry_img=sample['qry_img'][:h, :w].contiguous(), qry_isegmaps=np.ascontiguousarray(masks[keep]),
               qry_bboxes=boxes[keep], qry_cat_ids=np.asarray(sample['qry_cat_ids'])[keep],
               qry_cat_ids_real=np.asarray(sample['qry_cat_ids_real'])[keep],
               img_shape=np.array([NET, NET, 3], np.int32), qry_resize_to=np.array([NET, NET], np.int32))
    return out


class _Env:
    """One model, the pool dataset, the source-size batches and, per batch, the network-frame results of the call
    without the flag (eager), computed once."""

    def __init__(self):
        from fgn_amd.config import tiny_config
        from fgn_amd.detector import FGN
        from fgn_amd.weights import init_state_dict
        self.ds = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8,
                                               img_size=POOL, spp_img_size=SPP, raw_uint8=True)
        cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
        self.model = FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
                         test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
        self._net = {}

    def reset(self):
        m = self.model
        m.use_graphs = False
        m.transfer_mode = 0
        m.match_on_device = False
        m.query_source_capacity = 3 * POOL * POOL
        m.set_input_norm(**self.ds.input_norm)
        return m

    def batch(self, first, sizes):
        src = [_crop(self.ds[first + i], s) for i, s in enumerate(sizes)]
        imgs = [s.pop('qry_img') for s in src]
        bs = collate(src)
        bs['qry_img'] = torch.stack(imgs) if len(set(sizes)) == 1 else imgs
        return bs

    def net(self, first, sizes):
        key = (first, tuple(sizes))
        if key not in self._net:
            self._net[key] = self.reset().simple_test(**self.batch(first, sizes), rescale=True)
        return self._net[key]


@pytest.fixture(scope='module')
def env():
    return _Env()


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _np(v):
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)


def _check_frame(net, got, bs, sizes):
    """``got`` (flag on) against ``net`` (flag off) and the caller's inputs - everything but the masks' pixels."""
    assert len(net) == len(got) == len(sizes)
    for i, (a, b, hw) in enumerate(zip(net, got, sizes)):
        assert len(a['dt_scores']) > 0 and set(a) == set(b) - set(OVERLAP)
        for k in ('dt_scores', 'dt_cat_ids'):                     # selection untouched: same detections, same order
            assert _same(a[k], b[k]), (i, k)
        want = fd.boxes_to_source(a['dt_bboxes'], hw, (NET, NET))
        assert want is not a['dt_bboxes'] and _same(want, b['dt_bboxes'])
        assert all(r['size'] == list(hw) for r in b['dt_isegmaps_rle']) and len(b['dt_isegmaps_rle']) == len(a['dt_scores'])
        gt = _np(bs['qry_isegmaps'][i])
        assert len(gt) > 0 and b['qry_isegmaps_rle'] == rle.encode_many(gt)
        assert _same(b['qry_bboxes'], _np(bs['qry_bboxes'][i]))   # the caller's bytes, unscaled
        assert not _same(a['qry_bboxes'], b['qry_bboxes'])        # (the call without the flag scales them)
        assert b['qry_img_shape'].tolist() == [hw[0], hw[1], 3] and b['qry_img_shape'].dtype == a['qry_img_shape'].dtype
        for k in ('idx', 'qry_cat_ids', 'qry_child_idx', 'cats_ids_to_sample_real', 'spp_insts_ids'):
            assert _same(a[k], b[k]), (i, k)


@pytest.mark.parametrize('first,sizes', CASES)
def test_results_are_in_the_frame_of_each_source_image(env, first, sizes):
    from fgn_amd import ops
    net = env.net(first, sizes)
    m = env.reset()
    bs = env.batch(first, sizes)
    # detect_device + pack_results by hand: the per-image dicts carry the episode's mask probabilities
    dets = m.detect_device(bs['qry_img'], bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], bs['img_shape'],
                           qry_isegmaps=bs['qry_isegmaps'], qry_resize_to=bs['qry_resize_to'], results_at_source=True)
    assert [d['src_hw'] for d in dets] == list(sizes) and all(d['img_hw'] == (NET, NET) for d in dets)
    got = m.pack_results(dets, len(sizes), results_at_source=True,
                         **{k: bs[k] for k in ('qry_bboxes', 'qry_cat_ids', 'qry_isegmaps', 'img_shape', 'qry_child_idx',
                                               'cats_ids_to_sample_real', 'spp_insts_ids', 'idx')})
    _check_frame(net, got, bs, sizes)
    thr = m.cfg['test_cfg']['rcnn']['mask_thr_binary']
    for a, b, d, (h, w) in zip(net, got, dets, sizes):
        n = len(a['dt_scores'])
        xyxy = np.ascontiguousarray(b['dt_bboxes'][:, [1, 0, 3, 2]])
        dense = ops.mask_paste(d['mask_prob'][:n].contiguous(), torch.from_numpy(xyxy).cuda(), h, w, thr,
                               skip_empty=m._skip_empty()).cpu().numpy()
        assert dense.any()
        assert b['dt_isegmaps_rle'] == [rle.encode(x) for x in dense]
    # the public call gives the same dicts; ``rescale`` stays accepted and changes nothing
    for kw in (dict(rescale=True), dict(rescale=False)):
        assert _same(got, m.simple_test(**bs, results_at_source=True, **kw))


def test_at_the_network_size_the_flag_changes_no_byte(env):
    m = env.reset()
    bs = env.batch(2, [(NET, NET)])
    want = m.simple_test(**bs, rescale=True)
    got = m.simple_test(**bs, rescale=True, results_at_source=True)
    assert len(want[0]['dt_scores']) > 0 and set(want[0]) == set(got[0])
    assert _same(want, got)
    m.match_on_device = True
    assert _same(m.simple_test(**bs, rescale=True), m.simple_test(**bs, rescale=True, results_at_source=True))


def test_overlap_counts_are_counted_at_source_size(env):
    from fgn_amd.fsiseg_eval import evaluate_results
    first, sizes = CASES[3]
    m = env.reset()
    bs = env.batch(first, sizes)
    plain = m.simple_test(**bs, rescale=True, results_at_source=True)
    m.match_on_device = True
    got = m.simple_test(**bs, rescale=True, results_at_source=True)
    _check_frame(env.net(first, sizes), got, bs, sizes)
    for i, (g, p) in enumerate(zip(got, plain)):
        assert set(g) == set(p) | set(OVERLAP) and all(_same(g[k], p[k]) for k in p)
        gt = _np(bs['qry_isegmaps'][i]).astype(bool)
        dt = [rle.decode(r).astype(bool) for r in g['dt_isegmaps_rle']]
        assert all(d.shape == sizes[i] for d in dt)
        inter = np.array([[np.count_nonzero(d & x) for x in gt] for d in dt], np.int64).reshape(len(dt), len(gt))
        assert all(g[k].dtype == np.int32 for k in OVERLAP)
        assert g['dt_gt_inter'].shape == inter.shape and np.array_equal(g['dt_gt_inter'], inter)
        assert np.array_equal(g['dt_area'], np.array([d.sum() for d in dt], np.int64))
        assert np.array_equal(g['gt_area'], gt.reshape(len(gt), -1).sum(1))
        assert inter.any() and g['gt_area'].all()
    a, b = evaluate_results(got, N_WAYS), evaluate_results(plain, N_WAYS)
    assert a == b and set(a) == {'bbox_mAP50', 'bbox_mAR', 'segm_mAP50', 'segm_mAR'}


def test_one_graph_serves_every_source_size_and_leaves_the_other_mode_alone(env):
    cases = CASES[:3]
    m = env.reset()
    want = [m.simple_test(**env.batch(*c), rescale=True, results_at_source=True) for c in cases]
    m.use_graphs = True
    for c, w in list(zip(cases, want)) + [(cases[0], want[0])]:            # three sizes and a repeat
        assert _same(w, m.simple_test(**env.batch(*c), rescale=True, results_at_source=True))
    assert len(m._graphs) == 1
    first = next(iter(m._graphs.values()))
    # flag off: a second graph; the first is left alone and still replays correctly
    assert _same(env.net(*cases[1]), m.simple_test(**env.batch(*cases[1]), rescale=True))
    assert len(m._graphs) == 2 and first in m._graphs.values()
    assert _same(want[2], m.simple_test(**env.batch(*cases[2]), rescale=True, results_at_source=True))
    assert _same(env.net(*cases[0]), m.simple_test(**env.batch(*cases[0]), rescale=True))
    assert len(m._graphs) == 2
    # a batch of two images of different sizes, with the counts, through a graph of its own
    m.use_graphs = False
    m.match_on_device = True
    w2 = m.simple_test(**env.batch(*CASES[3]), rescale=True, results_at_source=True)
    m.use_graphs = True
    for _ in range(2):
        assert _same(w2, m.simple_test(**env.batch(*CASES[3]), rescale=True, results_at_source=True))
    assert len(m._graphs) == 3


def test_the_dense_fallback_pastes_at_source_size(env, monkeypatch):
    from fgn_amd import ops
    first, sizes = CASES[3]
    m = env.reset()
    m.match_on_device = True
    bs = env.batch(first, sizes)
    want = m.simple_test(**bs, rescale=True, results_at_source=True)
    monkeypatch.setattr(ops, 'RLE_TRANS_CAP', 64)
    dets = m.detect_device(bs['qry_img'], bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], bs['img_shape'],
                           qry_isegmaps=bs['qry_isegmaps'], qry_resize_to=bs['qry_resize_to'], results_at_source=True)
    dets[0]['host_ready'].synchronize()
    assert dets[0]['host']['rle_ovf'].numpy().any()                 # the cap does overflow: the fallback runs
    m.release_results(dets)
    assert _same(want, m.simple_test(**bs, rescale=True, results_at_source=True))


def test_the_flag_without_qry_resize_to_is_refused_before_anything_is_queued(env):
    m = env.reset()
    m.use_graphs = True
    bs = env.batch(*CASES[1])
    m.simple_test(**bs, rescale=True, results_at_source=True)
    graphs = dict(m._graphs)
    assert graphs
    img, boxes, masks = fd.resize_query(bs['qry_img'][0].numpy(), _np(bs['qry_bboxes'][0]), _np(bs['qry_isegmaps'][0]),
                                        NET, NET)
    nb = {k: v for k, v in bs.items() if k != 'qry_resize_to'}
    nb.update(qry_img=torch.from_numpy(np.ascontiguousarray(img))[None], qry_bboxes=[torch.from_numpy(boxes)],
              qry_isegmaps=[torch.from_numpy(masks)])

    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_source', '_resized_masks', '_detect_eager', '_detect_graphed', '_stem_input')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for n in names:
        setattr(m, n, boom)
    try:
        with pytest.raises(ValueError, match='qry_resize_to'):
            m.simple_test(**nb, rescale=True, results_at_source=True)
        with pytest.raises(ValueError, match='qry_resize_to'):
            m.detect_device(nb['qry_img'], nb['spp_imgs'], nb['spp_bboxes'], nb['spp_isegmaps'], nb['img_shape'],
                            results_at_source=True)
    finally:
        for n in names:
            delattr(m, n)
    assert torch.cuda.memory_allocated() == before and m._graphs == graphs
    # detections made without the flag cannot be packed with it
    m.use_graphs = False
    dets = m.detect_device(bs['qry_img'], bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], bs['img_shape'],
                           qry_resize_to=bs['qry_resize_to'])
    with pytest.raises(ValueError, match='results_at_source'):
        m.pack_results(dets, 1, results_at_source=True)
    m.release_results(dets)


def test_debug_trace_holds_the_masks_at_source_size(env):
    """``debug_trace`` with the flag: the per-image dense masks are pasted at the source size from the boxes the device
    divided (the ``boxes_src`` output of the RLE launch), and decode to the strings of the result."""
    first, sizes = CASES[3]
    m = env.reset()
    m.debug_trace = {}
    try:
        got = m.simple_test(**env.batch(first, sizes), rescale=True, results_at_source=True)
        per_image = m.debug_trace['per_image']
    finally:
        m.debug_trace = None
    assert _same(got, m.simple_test(**env.batch(first, sizes), rescale=True, results_at_source=True))
    for g, pi, (h, w) in zip(got, per_image, sizes):
        n = len(g['dt_scores'])
        masks = pi['masks'].cpu().numpy()
        assert n > 0 and masks.shape[1:] == (h, w)
        assert g['dt_isegmaps_rle'] == [rle.encode(x) for x in masks[:n]]
