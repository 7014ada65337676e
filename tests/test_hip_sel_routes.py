"""Every route of the proposal and detection selection (csrc/rpn_post.hip, csrc/det_post.hip), driven alone at the
smallest size that reaches it, bit for bit against the oracle - with the route that ran asserted.

The scenarios, references and the route model live in tests/_sel_ref.py; tests/test_sel_ref_cpu.py checks them without a
GPU (every scenario takes the route it is named for).  A proposal scenario runs twice: plainly, and with
``debug_topk=True, with_info=True``.  The second run must return the same bytes and tells which route ran:
info[b, 3..5] (candidate count, ok flag, finished by rpn_matrix_nms_kernel), the finish mark behind the debug buffer, and
how many ranks rpn_proposals_kernel wrote into it (0: it returned at once; 1536: its attempt 0 alone; n_sel: a full
attempt)."""
import numpy as np
import pytest
import torch

import _sel_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = ref.proposal_cases()
DBG_W = 8192                  # words per image of the debug buffer; the last 16 are phase stamps, [9] the finish mark


def _launch(case, **kw):
    from fgn_amd import ops
    b, n = case.scores.shape
    # the outputs are torch.empty: leave NaN bytes in the blocks the allocator hands out next for these two sizes, so that
    # a row the kernels forget to write is not zero by luck
    junk = [torch.full((b, case.max_out, 5), float('nan'), device='cuda') for _ in range(2)]
    del junk
    return ops.rpn_proposals(torch.from_numpy(case.scores).cuda(), torch.zeros(b, n, 4, device='cuda'),
                             torch.from_numpy(case.anchors).cuda(), 1, 1, 16, ref.IMG, ref.IMG, ref.MEANS, ref.STDS,
                             case.nms_pre, case.min_size, case.iou_thr, case.max_out, **kw)


def _observed_route(case, b, dbg, info):
    """The route image b took, from the three places that record it; they must agree with each other."""
    mark = int(dbg[b, DBG_W - 16 + 9])
    written = int((dbg[b, :DBG_W - 16] >= 0).sum())
    n_cand, ok, fin = int(info[b, 3]), int(info[b, 4]), int(info[b, 5])
    assert ok in (0, 1) and fin in (0, 1) and mark in (-1, 1)
    assert (mark == 1) == (fin == 1)
    if not info[b].any():
        assert written == case.n_sel and mark == -1
        return 'single', written
    assert n_cand >= ref.FAST_SEL and ok == (n_cand <= ref.FAST_CAP)
    if fin:
        assert ok == 1 and written == 0
        return 'matrix', written
    assert written in (ref.FAST_SEL, case.n_sel)
    if ok:
        assert written == case.n_sel
        return 'dry', written
    return ('invalid-fast' if written == ref.FAST_SEL else 'invalid-full'), written


def _check(case):
    """Both runs of one launch against the reference; -> (proposals [B, max_out, 5] as numpy, observed routes)."""
    from fgn_amd import lib
    props, n_props, rois = _launch(case, with_rois=True)
    props, n_props, rois = props.cpu().numpy(), n_props.cpu().numpy(), rois.cpu().numpy()
    mo = case.max_out
    for b in range(len(case.scores)):
        want, k = case.reference(b)
        assert int(n_props[b]) == k, (case.name, b, int(n_props[b]), k)
        assert props[b].tobytes() == want.tobytes(), (case.name, b, np.nonzero((props[b] != want).any(1))[0][:8])
        want_rois = np.concatenate([np.full((mo, 1), b, F32), want[:, :4]], 1)          # zero boxes past n_props
        assert rois[b * mo:(b + 1) * mo].tobytes() == want_rois.tobytes(), (case.name, b)
    if case.routes[0] == 'large':
        for kw in (dict(debug_topk=True, with_info=True), dict(with_info=True), dict(debug_topk=True)):
            with pytest.raises(lib.FgnHipError, match='unsupported shape'):
                _launch(case, **kw)
        return props, ['large'] * len(case.scores)
    p2, n2, dbg, info = _launch(case, debug_topk=True, with_info=True)
    assert p2.cpu().numpy().tobytes() == props.tobytes() and np.array_equal(n2.cpu().numpy(), n_props)
    dbg, info = dbg.cpu().numpy(), info.cpu().numpy()
    assert info.shape == (len(case.scores), 8) and info.dtype == np.int32
    seen = []
    for b in range(len(case.scores)):
        name, written = _observed_route(case, b, dbg, info)
        model, n_cand, ok, _ = case.route(b)
        assert name == model == case.routes[b], (case.name, b, name, model, info[b])
        if name != 'single':
            assert (int(info[b, 3]), int(info[b, 4])) == (n_cand, ok) and n_cand == case.n_cand[b]
            assert tuple(info[b, :3]) == ref.preselect_bins(case.scores[b])
        if written:
            assert np.array_equal(dbg[b, :written], ref.ranked_ref(case.scores[b], written)), (case.name, b)
        seen.append(name)
    return props, seen


@pytest.mark.parametrize('name', sorted(CASES))
def test_proposal_route(name):
    case = CASES[name]()
    _, seen = _check(case)
    assert seen == case.routes


def test_proposals_of_five_images_on_five_routes_in_one_launch():
    """fill, exhaust, dry, invalid-fast and invalid-full side by side: every image equals its reference (in _check), takes
    its own route, and equals its own single-image launch."""
    case = ref.batch_case()
    props, seen = _check(case)
    assert seen == ['matrix', 'matrix', 'dry', 'invalid-fast', 'invalid-full']
    for b in range(len(case.scores)):
        one = ref.Case('batch-%d' % b, case.scores[b], case.anchors, case.nms_pre, case.max_out, case.routes[b],
                       case.n_cand[b])
        p1, s1 = _check(one)
        assert p1[0].tobytes() == props[b].tobytes() and s1 == [case.routes[b]]


def test_proposals_of_images_on_different_attempts_do_not_share_scratch():
    """ref.scratch_case: dry and invalid-full images of one launch at a sort buffer of 4096, placed eight workgroups apart
    so that they share an L2.  (Before the fix of the scratch pitch in rpn_proposals_kernel the attempt 0 of image b wrote
    its sorted boxes into the range image b // 2 was using.)"""
    case = ref.scratch_case()
    for _ in range(2):
        _, seen = _check(case)
        assert seen == case.routes


def test_info_words_are_zero_when_the_preselection_is_not_launched_and_the_default_call_is_unchanged():
    case = CASES['edge-1536']()
    out = _launch(case)
    assert len(out) == 2
    props, n, info = _launch(case, with_info=True)
    assert tuple(info.shape) == (1, 8) and info.dtype == torch.int32 and int(info.abs().sum()) == 0
    assert torch.equal(props, out[0]) and torch.equal(n, out[1])
    p3, n3, rois, info3 = _launch(CASES['fill-64'](), with_rois=True, with_info=True)
    assert tuple(rois.shape) == (64, 5) and info3[0, 3:6].tolist() == [1536, 1, 1]


def test_more_anchors_than_the_score_cache_holds_are_refused():
    from fgn_amd import lib
    n = ref.N_TOTAL_MAX + 1
    case = ref.Case('size-65537', ref.distinct_top24(n), ref.disjoint(n, per_row=256), 2000, 64, 'matrix', 1536)
    with pytest.raises(lib.FgnHipError, match='fgn_rpn_proposals_f32 failed: unsupported shape'):
        _launch(case)


# ------------------------------------------------------------------------------------------ detections
def _det(rois, cls, reg, n_ways, score_thr, iou_thr, max_out, **kw):
    from fgn_amd import ops
    return ops.det_post(torch.from_numpy(np.ascontiguousarray(rois, F32)).cuda(), torch.from_numpy(cls).cuda(),
                        torch.from_numpy(reg).cuda(), n_ways, ref.IMG, ref.IMG, ref.MEANS, ref.STDS, score_thr, iou_thr,
                        max_out, **kw)


def _check_det(rois, cls, n_ways, score_thr, iou_thr, max_out, n_valid=None):
    """One image against det_ref: detections, labels, zero rows, the kernel's own n_valid, the mask RoIs."""
    from fgn_amd import ops
    reg = np.zeros((len(cls), 4), F32)
    dets, labels, nv = ref.det_ref(rois, cls, reg, n_ways, (ref.IMG, ref.IMG), ref.MEANS, ref.STDS, score_thr, iou_thr, max_out)
    if n_valid is not None:
        assert nv == n_valid
    det, lab, n, _ = _det(rois, cls, reg, n_ways, score_thr, iou_thr, max_out, debug_scores=True)
    assert int(ops.det_post.last_stamps[5]) == nv
    det, lab, n = det.cpu().numpy(), lab.cpu().numpy(), int(n[0])
    assert n == len(dets), (n, len(dets), nv)
    assert det[:n].tobytes() == dets.tobytes(), np.nonzero((det[:n] != dets).any(1))[0][:8]
    assert np.array_equal(lab[:n], labels)
    assert not det[n:].view(np.uint32).any() and not lab[n:].any()
    d2, l2, n2, mr = _det(rois, cls, reg, n_ways, score_thr, iou_thr, max_out, img_index=3)
    assert d2.cpu().numpy().tobytes() == det.tobytes() and np.array_equal(l2.cpu().numpy(), lab) and int(n2[0]) == n
    assert mr.cpu().numpy().tobytes() == np.concatenate([np.full((max_out, 1), 3, F32), det[:, :4]], 1).tobytes()
    return dets, labels, nv


@pytest.mark.parametrize('n_ways', [1, 3, 8])
@pytest.mark.parametrize('n_valid', [0, 1, 64, 1023, 1024, 1025, 2048, 2049])
def test_det_post_at_the_counts_where_the_sort_changes(n_valid, n_ways):
    """0 and 1 candidates, one wavefront, both sides of the register sort / LDS sort split (1024) and of the next
    power of two (2048): distinct scores, half of the RoIs overlapping a neighbour."""
    r = -(-max(n_valid, 1) // n_ways) + 3
    cls = ref.cls_for_valid(r, n_ways, n_valid, seed=n_valid + n_ways)
    _check_det(ref.det_rois(r, seed=n_valid), cls, n_ways, 0.05, 0.5, 100, n_valid=n_valid)


@pytest.mark.parametrize('n_ways,n_valid', [(3, 900), (8, 1024), (1, 1025), (3, 2049)])
def test_det_post_orders_equal_scores_by_candidate_index(n_ways, n_valid):
    """Rows of cls_raw repeated over RoIs and classes: every passing candidate of a RoI with m of them scores 1/m.  Among
    equals the order is the candidate index r * N + n (the low word of the sort key)."""
    r = -(-n_valid // n_ways) + 3
    cls = ref.cls_for_valid(r, n_ways, n_valid, seed=7, equal=True)
    dets, labels, _ = _check_det(ref.det_rois(r, seed=1), cls, n_ways, 0.05, 0.5, 100, n_valid=n_valid)
    assert len(np.unique(dets[:, 4])) <= n_ways and len(dets) == 100
    # all RoIs disjoint and every candidate passing with one score: the result is the first max_out candidate indices
    rois = ref.disjoint(r, per_row=32, origin=(0.0, 0.0))
    rois = np.concatenate([np.zeros((r, 1), F32), rois], 1)
    cls = ref.cls_for_valid(r, n_ways, r * n_ways, equal=True)
    dets, labels, _ = _check_det(rois, cls, n_ways, 0.05, 0.5, 100, n_valid=r * n_ways)
    ci = np.arange(100)
    assert np.array_equal(labels, ci % n_ways) and dets[:, :4].tobytes() == rois[ci // n_ways, 1:].tobytes()


def test_det_post_with_a_score_exactly_on_the_threshold():
    """score > score_thr: a candidate whose score IS the threshold stays out; with the next float below it comes in."""
    from oracle import fgn_ref_cpu as O
    r, n_ways = 120, 3
    cls = ref.cls_for_valid(r, n_ways, 200, seed=3)
    cs, _ = O.count_modified_cls_bbox(r, torch.from_numpy(cls), torch.zeros(r * n_ways, 4), n_ways)
    scores = O.softmax32(cs.numpy())[:, :-1].reshape(-1)
    on = np.sort(scores[scores > 0.05])[100]                   # the float the oracle computes for one passing row
    rois = ref.det_rois(r, seed=4)
    _, _, nv_on = _check_det(rois, cls, n_ways, float(on), 0.5, 100)
    _, _, nv_below = _check_det(rois, cls, n_ways, float(np.nextafter(on, F32(0))), 0.5, 100)
    assert nv_on == int((scores > on).sum()) and nv_below == nv_on + int((scores == on).sum()) > nv_on


def _family_rois(thr, degenerate=True):
    pairs = [p for p in ref.near_threshold_pairs(thr) if degenerate or p[0] not in ref.DEGENERATE]
    b = ref.pair_boxes(pairs)
    return np.concatenate([np.zeros((len(b), 1), F32), b], 1).astype(F32)


def _descending_cls(r, n_ways):
    """Every class of every RoI passes; RoI k scores a little less than RoI k - 1, the classes of a RoI equally."""
    cls = np.zeros((r * n_ways, 2), F32)
    cls[:, 0] = -30.0
    if n_ways == 1:
        cls[:, 0] = 0.0
        cls[:, 1] = (2.0 - 0.02 * np.arange(r)).astype(F32)
        return cls
    # more than one class: the scores of a RoI sum to one whatever the logits are; rank the RoIs by a background share
    cls[:, 0] = np.repeat(-3.0 + 0.02 * np.arange(r), n_ways).astype(F32)
    return cls


@pytest.mark.parametrize('thr', [0.3, 0.5, 0.7])
def test_det_post_on_the_near_threshold_family(thr):
    """The pairs of the proposal threshold scenario as RoIs (the degenerate ones too: no min-size filter here): under one
    label; under three labels, where the same box under two labels is kept twice and the label offsets move every pair;
    and with a huge box under the score threshold, which must not move the offsets (max_coord is taken over the valid
    candidates only: with its 2^24 the half-integer pairs would round)."""
    rois = _family_rois(thr)
    r = len(rois)
    d1, _, _ = _check_det(rois, _descending_cls(r, 1), 1, 0.05, thr, 100, n_valid=r)
    d3, l3, _ = _check_det(rois, _descending_cls(r, 3), 3, 0.05, thr, 300, n_valid=3 * r)
    assert d3[l3 == 0][:, :4].tobytes() == d1[:, :4].tobytes()                          # label 0 carries no offset
    same = (d3[:, :4] == rois[0, 1:]).all(1)                                            # one box under three labels
    assert same.sum() == 3 and sorted(l3[same].tolist()) == [0, 1, 2]
    grid = ref.det_rois(40, seed=2)
    grid[:, [2, 4]] += 100.0
    small = np.concatenate([_family_rois(thr)[:8], grid])                               # the 'exact' pairs + a grid
    small[:8, 1:] *= 0.5
    small[:8, 1:] += np.array([0.5, 0.0, 0.5, 0.0], F32)                                # quarter- and half-integers
    r = len(small)
    cls = _descending_cls(r + 1, 3)
    cls[-3:] = (30.0, -30.0)                                                            # the huge box: background only
    huge = np.array([[0, 0, 0, ref.IMG - 1, ref.IMG - 1]], F32)
    dh, lh, _ = _check_det(np.concatenate([small, huge]), cls, 3, 0.05, thr, 300, n_valid=3 * r)
    ds, ls, _ = _check_det(small, cls[:-3], 3, 0.05, thr, 300, n_valid=3 * r)
    assert dh.tobytes() == ds.tobytes() and np.array_equal(lh, ls)


@pytest.mark.parametrize('max_out', [1, 100, 1024])
def test_det_post_cuts_more_survivors_than_max_per_img(max_out):
    r = 2052
    rois, cls = ref.det_rois(r, seed=5), ref.cls_for_valid(r, 1, 2049, seed=5)
    everything, _, _ = ref.det_ref(rois, cls, np.zeros((r, 4), F32), 1, (ref.IMG, ref.IMG), ref.MEANS, ref.STDS, 0.05, 0.5, 0)
    assert len(everything) > 1024
    dets, _, _ = _check_det(rois, cls, 1, 0.05, 0.5, max_out, n_valid=2049)
    assert dets.tobytes() == everything[:max_out].tobytes()


def test_det_post_three_images_on_both_sort_branches_and_an_empty_one_in_one_launch():
    """n_valid 1500 (LDS sort), 700 (register sort, inside a device count of 300 RoIs whose later rows would pass) and 0:
    one launch equals three launches and the reference; the mask RoIs carry img_index + i."""
    r, n_ways, mo = 600, 3, 100
    cnt = [600, 300, 600]
    cls = [ref.cls_for_valid(r, n_ways, 1500, seed=11),
           np.concatenate([ref.cls_for_valid(300, n_ways, 700, seed=12), ref.cls_for_valid(300, n_ways, 900, seed=13)]),
           ref.cls_for_valid(r, n_ways, 0, seed=14)]
    rois = [ref.det_rois(r, seed=20 + i) for i in range(3)]
    reg = np.zeros((3 * r * n_ways, 4), F32)
    cnt_dev = torch.tensor(cnt, dtype=torch.int32, device='cuda')
    det, lab, n, mr = _det(np.concatenate(rois), np.concatenate(cls), reg, n_ways, 0.05, 0.5, mo, n_rois_dev=cnt_dev,
                           img_index=5, batch=3)
    det, lab, n, mr = det.cpu().numpy(), lab.cpu().numpy(), n.cpu().numpy(), mr.cpu().numpy()
    want_nv = [1500, 700, 0]
    for i in range(3):
        c = cnt[i]
        dets, labels, nv = ref.det_ref(rois[i][:c], cls[i][:c * n_ways], reg[:c * n_ways], n_ways, (ref.IMG, ref.IMG),
                                       ref.MEANS, ref.STDS, 0.05, 0.5, mo)
        assert nv == want_nv[i] and (len(dets) == mo or i == 2)
        sl = slice(i * mo, (i + 1) * mo)
        assert int(n[i]) == len(dets) and det[sl][:len(dets)].tobytes() == dets.tobytes()
        assert np.array_equal(lab[sl][:len(dets)], labels)
        assert not det[sl][len(dets):].view(np.uint32).any() and not lab[sl][len(dets):].any()
        assert mr[sl].tobytes() == np.concatenate([np.full((mo, 1), 5 + i, F32), det[sl][:, :4]], 1).tobytes()
        d1, l1, n1, m1 = _det(rois[i], cls[i], reg[:r * n_ways], n_ways, 0.05, 0.5, mo, n_rois_dev=cnt_dev[i:i + 1],
                              img_index=5 + i)
        assert d1.cpu().numpy().tobytes() == det[sl].tobytes() and np.array_equal(l1.cpu().numpy(), lab[sl])
        assert int(n1[0]) == int(n[i]) and m1.cpu().numpy().tobytes() == mr[sl].tobytes()
