"""``ops.eval_match`` (eval_match_kernel) against ``fsiseg_eval.match_flags``: exact, on the crafted edge cases and on
random images at the sizes where the kernel changes its path (one lane, a full wave, a second pass of ground truths,
more detections than max_dets), for 1, 10 and 16 thresholds."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _eval_match_cases import N_WAYS, THR_SETS, crafted, random_res   # noqa: E402

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = -1, -2


def _operands(res):
    """what ``detect_device`` holds for the image of a result dict: boxes [D,5] XYXY + score, labels, the counts"""
    b = res['dt_bboxes']
    boxes = torch.from_numpy(np.column_stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], res['dt_scores']]).astype(np.float32))
    ov = tuple(torch.from_numpy(np.ascontiguousarray(res[k])).cuda() for k in ('dt_gt_inter', 'dt_area', 'gt_area'))
    return boxes.reshape(-1, 5).cuda(), torch.from_numpy(res['dt_cat_ids']).cuda(), ov


def _device_flags(res, thrs, max_dets=100, segm=True, **kw):
    from fgn_amd import ops
    from fgn_amd.fsiseg_eval import _xywh
    boxes, labels, ov = _operands(res)
    return ops.eval_match(boxes, labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], thrs, N_WAYS,
                          overlap=ov if segm else None, max_dets=max_dets, **kw)


def _check(res, thrs, max_dets=100):
    from fgn_amd.fsiseg_eval import match_flags
    bbox, segm = _device_flags(res, thrs, max_dets)
    assert bbox.dtype == segm.dtype == torch.int32 and bbox.shape == segm.shape == (len(res['dt_scores']),)
    want_b = match_flags(res, thrs, 'bbox', max_dets, n_ways=N_WAYS)
    want_s = match_flags(res, thrs, 'segm', max_dets, n_ways=N_WAYS)
    assert np.array_equal(bbox.cpu().numpy(), want_b)
    assert np.array_equal(segm.cpu().numpy(), want_s)
    return want_b, want_s


@pytest.mark.parametrize('name', sorted(crafted()))
def test_crafted(name):
    res, thrs, max_dets, want = crafted()[name]
    b, s = _check(res, thrs, max_dets)
    assert b.tolist() == list(want['bbox']) and s.tolist() == list(want['segm'])


@pytest.mark.parametrize('n_thr', [1, 10, 16])
@pytest.mark.parametrize('d,g', [(1, 1), (63, 1), (64, 64), (65, 65), (100, 7), (130, 3)])
def test_random(d, g, n_thr):
    matched = cut = 0
    for seed in range(4):                                     # (seed bits: tied scores, boxes on a lattice)
        res = random_res(1000 * d + 4 * g + seed, d=d, g=g)
        if (d, g) == (130, 3):                                # one category holds more than max_dets detections
            res['dt_cat_ids'][:120] = 1
        b, s = _check(res, THR_SETS[n_thr])
        matched += int((b > 0).sum() + (s > 0).sum())
        cut += int((b == -1).sum())
    assert matched > 0 and (cut > 0) == ((d, g) == (130, 3))


def test_second_pass_of_ground_truths_is_used():
    """(65, 65): the only ground truth a detection overlaps is the one of lane pass 1"""
    res = random_res(7, d=65, g=65, outside_labels=False)
    res['dt_cat_ids'][:] = 0
    res['qry_cat_ids'][:] = 0
    res['dt_gt_inter'][:] = 0
    res['dt_area'][:] = 3
    res['gt_area'][:] = 3
    res['dt_gt_inter'][10, 64] = 3
    res['dt_gt_inter'][11, 64] = 3
    res['dt_scores'][10], res['dt_scores'][11] = 0.99, 0.98
    _, s = _check(res, (0.5,))
    assert s[10] == 1 and s[11] == 0 and s.sum() == 1


def test_device_count_and_guard_words():
    """n_dev < D: rows at and beyond it are 0, the rows below are those of the shorter image, and the words around the
    output stay as they were"""
    from fgn_amd import lib
    from fgn_amd.fsiseg_eval import _xywh, match_flags
    res = random_res(11, d=90, g=9)
    n, d, g = 57, 90, 9
    boxes, labels, (inter, da, ga) = _operands(res)
    thrs = np.minimum(np.asarray(THR_SETS[10]), 1 - 1e-10)
    f64 = torch.from_numpy(np.concatenate([thrs, _xywh(res['qry_bboxes']).reshape(-1)])).cuda()
    cat = torch.from_numpy(res['qry_cat_ids'].astype(np.int32)).cuda()
    cnt = torch.tensor([n], dtype=torch.int32).cuda()
    guard = 64
    buf = torch.full((guard + 2 * d + guard,), 0x5a5a5a5a, dtype=torch.int32).cuda()
    out = buf[guard:guard + 2 * d]
    rc = lib.load().fgn_eval_match_i32(boxes.data_ptr(), 5, labels.data_ptr(), cnt.data_ptr(), inter.data_ptr(),
                                       da.data_ptr(), ga.data_ptr(), f64.data_ptr() + 8 * len(thrs), cat.data_ptr(),
                                       f64.data_ptr(), out.data_ptr(), d, g, len(thrs), N_WAYS, 100, 0, 0, 0, 0,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    host = buf.cpu().numpy()
    assert np.all(host[:guard] == 0x5a5a5a5a) and np.all(host[guard + 2 * d:] == 0x5a5a5a5a)
    got = host[guard:guard + 2 * d].reshape(2, d)
    assert np.all(got[:, n:] == 0)
    short = {k: (v[:n] if k.startswith('dt_') else v) for k, v in res.items()}
    assert np.array_equal(got[0, :n], match_flags(short, THR_SETS[10], 'bbox', n_ways=N_WAYS))
    assert np.array_equal(got[1, :n], match_flags(short, THR_SETS[10], 'segm', n_ways=N_WAYS))
    # the wrapper with the count, and a count beyond D
    from fgn_amd import ops
    b, s = ops.eval_match(boxes, labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], THR_SETS[10], N_WAYS,
                          overlap=(inter, da, ga), n_dev=cnt)
    assert np.array_equal(torch.stack([b, s]).cpu().numpy(), got)
    b, s = ops.eval_match(boxes, labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], THR_SETS[10], N_WAYS,
                          overlap=(inter, da, ga), n_dev=torch.tensor([1000], dtype=torch.int32).cuda())
    assert np.array_equal(b.cpu().numpy(), match_flags(res, THR_SETS[10], 'bbox', n_ways=N_WAYS))


def test_without_counts_there_is_no_segm_row():
    from fgn_amd import ops
    from fgn_amd.fsiseg_eval import _xywh, match_flags
    res = random_res(21, d=100, g=7)
    bbox, segm = _device_flags(res, THR_SETS[10], segm=False)
    assert segm is None
    assert np.array_equal(bbox.cpu().numpy(), match_flags(res, THR_SETS[10], 'bbox', n_ways=N_WAYS))
    boxes, labels, _ = _operands(res)
    b, s, buf = ops.eval_match(boxes, labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], (0.5,), N_WAYS, packed=True)
    assert s is None and buf.shape == (2, 100) and buf.data_ptr() == b.data_ptr()
    assert np.all(buf[1].cpu().numpy() == 0)                                  # (the allocation is fully written)


def test_packed_views_one_allocation():
    res = random_res(22, d=100, g=7)
    b, s, buf = _device_flags(res, (0.5,), packed=True)
    assert buf.shape == (2, 100) and b.data_ptr() == buf.data_ptr() and s.data_ptr() == buf[1].data_ptr()


def test_boxes_divided_to_source_size():
    """``src_hw`` / ``net_hw``: the device divides the network-frame boxes as ``boxes_to_source`` does"""
    from fgn_amd.fewshot_ds import boxes_to_source
    from fgn_amd.fsiseg_eval import match_flags
    res = random_res(33, d=100, g=7)
    src, net = (47, 61), (160, 224)
    at_src = dict(res)
    at_src['dt_bboxes'] = boxes_to_source(res['dt_bboxes'], src, net, order='yxyx')
    assert not np.array_equal(at_src['dt_bboxes'], res['dt_bboxes'])
    bbox, segm = _device_flags(res, THR_SETS[10], src_hw=src, net_hw=net)
    want = match_flags(at_src, THR_SETS[10], 'bbox', n_ways=N_WAYS)
    assert np.array_equal(bbox.cpu().numpy(), want)
    assert not np.array_equal(want, match_flags(res, THR_SETS[10], 'bbox', n_ways=N_WAYS))
    assert np.array_equal(segm.cpu().numpy(), match_flags(res, THR_SETS[10], 'segm', n_ways=N_WAYS))


def test_empty_sides():
    from fgn_amd.fsiseg_eval import match_flags
    res = random_res(41, d=0, g=5)
    b, s = _device_flags(res, (0.5,))
    assert b.shape == s.shape == (0,)
    res = random_res(42, d=130, g=0, outside_labels=False)
    res['dt_cat_ids'][:110] = 2
    b, s = _check(res, THR_SETS[16])
    assert (b == -1).sum() == (res['dt_cat_ids'] == 2).sum() - 100 >= 10 and set(b.tolist()) == {0, -1}
    assert np.array_equal(b, s)
    assert np.array_equal(b, match_flags(res, THR_SETS[16], 'bbox', n_ways=N_WAYS))


def test_return_codes():
    from fgn_amd import lib, ops
    from fgn_amd.fsiseg_eval import _xywh
    res = random_res(51, d=20, g=4)
    boxes, labels, (inter, da, ga) = _operands(res)
    f64 = torch.from_numpy(np.concatenate([[0.5], _xywh(res['qry_bboxes']).reshape(-1)])).cuda()
    cat = torch.from_numpy(res['qry_cat_ids'].astype(np.int32)).cuda()
    out = torch.full((2, 20), 77, dtype=torch.int32).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(boxes=boxes.data_ptr(), stride=5, labels=labels.data_ptr(), n_dev=None, inter=inter.data_ptr(),
                da=da.data_ptr(), ga=ga.data_ptr(), xywh=f64.data_ptr() + 8, cat=cat.data_ptr(), thr=f64.data_ptr(),
                flags=out.data_ptr(), d=20, g=4, t=1, ways=N_WAYS, max_dets=100, sh=0, sw=0, nh=0, nw=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.load().fgn_eval_match_i32(*[a[k] for k in good], stream)
    assert call() == 0
    for key in ('boxes', 'labels', 'thr', 'flags', 'xywh', 'cat', 'inter', 'ga'):
        assert call(**{key: None}) == ERR_ARG, key
    assert call(stride=4) == ERR_ARG
    for kw in (dict(t=0), dict(t=17), dict(d=-1), dict(g=-1), dict(max_dets=0), dict(ways=0), dict(g=4097),
               dict(d=2000, max_dets=2000), dict(d=2049), dict(sh=10, sw=0, nh=5, nw=5), dict(sh=10, sw=10, nh=0, nw=5)):
        assert call(**kw) == ERR_SHAPE, kw
    torch.cuda.synchronize()
    before = out.cpu().numpy().copy()
    assert call(d=0, boxes=None, labels=None) == 0                            # no detections: nothing is launched
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), before) and not np.any(before == 77)
    with pytest.raises(lib.FgnHipError):
        ops.eval_match(boxes, labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], np.linspace(0.1, 0.9, 17), N_WAYS)
    with pytest.raises(lib.FgnHipError):
        ops.eval_match(boxes.cpu(), labels, _xywh(res['qry_bboxes']), res['qry_cat_ids'], (0.5,), N_WAYS)
