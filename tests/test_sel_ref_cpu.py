"""tests/_sel_ref.py checked without a GPU: the route model's constants against the kernel sources, every named scenario
against the route it is built for (a construction that drifts fails here), the composed references against the oracle's own
entry points, and the numpy emulation of post_common.h::iou_gt against the oracle's division on the near-threshold pairs and
on two million pairs swept across the crossing in float steps - the CPU check of the kernel's 4e-6 shortcut margin."""
import numpy as np
import pytest
import torch

import _sel_ref as ref
from oracle import fgn_ref_cpu as O

F32 = np.float32
CASES = ref.proposal_cases()


def test_model_constants_equal_the_sources():
    c = ref.source_constants()
    assert c['FAST_SEL'] == ref.FAST_SEL and c['FAST_CAP'] == ref.FAST_CAP
    assert c['SORT_MAX'] == c['SORT_MAX_py'] == ref.SORT_MAX and c['OUT_MAX'] == c['OUT_MAX_py'] == ref.OUT_MAX
    assert c['N_TOTAL_MAX'] == ref.N_TOTAL_MAX and c['DET_SPLIT'] == ref.DET_SPLIT
    assert c['launch'] == ('RPN_FAST_SEL', 'RPN_FAST_CAP')      # the pre-selection launches above these two
    assert c['BINS'] == 4096                                     # 12 + 12 bits of the 24 the model's threshold uses


def test_composite_key_order_is_the_stable_descending_argsort():
    rs = np.random.RandomState(0)
    for s in (ref.shared_top24(2304, 600, 1500), ref.all_equal(50), rs.rand(5000).astype(F32),
              np.round(rs.rand(5000) * 8).astype(F32) / 8 + F32(0.01)):
        s = s[rs.permutation(len(s))]
        key = (ref.key_hi(s).astype(np.uint64) << np.uint64(32)) | np.arange(len(s), dtype=np.uint64)
        assert np.array_equal(np.argsort(key, kind='stable'), ref.ranked_ref(s, len(s)))
        assert np.array_equal(ref.ranked_ref(s, 7), ref.ranked_ref(s, len(s))[:7])


def test_score_builders_have_the_bit_structure_they_claim():
    for s in (ref.distinct_top24(2304), ref.distinct_top24(65536), ref.shared_top24(2304, 549, 1500),
              ref.fill_bin_exactly(1), ref.fill_bin_exactly(2), ref.fill_bin_exactly(2, lead=3), ref.first_bin()):
        assert s.dtype == F32 and (s > 0).all() and (s <= 1).all()
        assert (np.diff(ref.key_hi(s).astype(np.int64)) >= 0).all()          # by rank: descending score
    t = ref.key_hi(ref.distinct_top24(2304)) >> 8
    assert len(np.unique(t)) == 2304 and len(np.unique(t >> 12)) == 2
    t = ref.key_hi(ref.shared_top24(2304, 600, 1500)) >> 8
    assert (t == t[1500]).sum() == 600 and len(np.unique(ref.shared_top24(2304, 600, 1500)[1500:2100])) == 256
    t = ref.key_hi(ref.fill_bin_exactly(1)) >> 8
    assert t[1535] & 4095 == 4095 and t[1536] & 4095 == 0 and (t[:1536] >> 12 == t[0] >> 12).all()
    t = ref.key_hi(ref.fill_bin_exactly(2)) >> 8
    assert t[1535] == t[1532] != t[1536] and (np.bincount(t - t[0]) == 4).all()
    t = ref.key_hi(ref.fill_bin_exactly(2, lead=3)) >> 8
    assert t[1535] == t[1538] != t[1539] and t[1534] != t[1535]
    t = ref.key_hi(ref.distinct_top24(2304, t0=ref.T0)) >> 8
    assert len(np.unique(t >> 12)) == 1 and t[0] & 4095 == 0
    assert ref.all_equal(5).view(np.uint32).tolist() == [0x3f800000] * 5


def test_box_builders_keep_what_they_claim():
    z = np.zeros
    assert len(O.nms(ref.disjoint(300), z(300, F32), 0.7)[1]) == 300
    assert len(O.nms(ref.clusters(300, 7), z(300, F32), 0.7)[1]) == 7
    assert O.nms(ref.staircase(128, 10), z(128, F32), 0.7)[1].tolist() == list(range(0, 128, 2))
    k3 = O.nms(ref.staircase(128, 3), z(128, F32), 0.7)[1]
    assert k3[0] == 0 and (np.diff(k3) > 2).all()                            # each kept box suppresses its next few


# ------------------------------------------------------------------------------------------ scenarios and routes
@pytest.mark.parametrize('name', sorted(CASES))
def test_scenario_takes_the_route_it_is_named_for(name):
    c = CASES[name]()
    got, n_cand, ok, kept = c.route()
    assert got == c.routes[0], (got, n_cand, ok, kept)
    if c.n_cand[0] is not None:
        assert n_cand == c.n_cand[0] and ok == (n_cand <= ref.FAST_CAP)
    pre = name.split('-')[0]
    if pre == 'exhaust':
        assert kept < c.max_out and min(n_cand, c.n_sel) >= c.n_sel          # finished by exhaustion, zero rows follow
        assert c.reference()[1] == kept == 5
    if pre == 'fill':
        assert c.reference()[1] == c.max_out
    if name in ('dry', 'dry-4096', 'dry-8192'):
        assert kept < c.max_out == c.reference()[1]
    if name == 'dry-zero':
        assert kept < c.reference()[1] < c.max_out
    if pre == 'large':
        assert c.reference()[1] == c.max_out > 1024
    if pre == 'threshold':
        assert 2 * (len(ref.near_threshold_pairs(c.iou_thr)) - 3) < c.max_out    # every pair decides inside the output


def test_batch_scenario_puts_five_images_on_five_ends():
    c = ref.batch_case()
    got = [c.route(b) for b in range(5)]
    assert [g[0] for g in got] == c.routes == ['matrix', 'matrix', 'dry', 'invalid-fast', 'invalid-full']
    assert [g[1] for g in got] == c.n_cand
    assert got[0][3] >= c.max_out and got[1][3] < c.max_out                  # fill against exhaust
    assert [c.reference(b)[1] for b in range(5)] == [32, 10, 32, 32, 10]


def test_shared_scratch_scenario_mixes_attempts_and_needs_the_late_ranks():
    c = ref.scratch_case()
    got = [c.route(b) for b in range(17)]
    assert [g[0] for g in got] == c.routes and [g[1] for g in got] == c.n_cand
    assert [b for b in range(17) if c.routes[b] == 'dry'] == [7, 8]
    assert [b for b in range(17) if c.routes[b] == 'invalid-full'] == [15, 16]          # b and b + 8: one XCD
    assert [c.reference(b)[1] for b in range(17)] == [1000] * 17
    assert 4096 >= c.n_sel > ref.FAST_CAP                            # the two pitches differ: b * 2048 against b * 4096
    for b in (15, 16):                                               # the old attempt-0 range lay inside image b // 2's
        assert (b // 2) * 4096 <= b * 2048 < b * 2048 + ref.FAST_SEL <= (b // 2 + 1) * 4096 and c.routes[b // 2] == 'dry'
    for b in (7, 8, 15, 16):                                         # the 232 boxes that fill max_out rank behind 2048
        rows = c.reference(b)[0]
        assert got[b][3] == 768 and (rows[:768, 1] < 3000).all() and (rows[768:, 1] >= 3000).all()
        assert len(ref.proposals_ref(c.scores[b], c.anchors, np.zeros((c.n_total, 4), F32), 2048, 1000, 0.7, 0.0,
                                     (ref.IMG, ref.IMG), ref.MEANS, ref.STDS)) == 768


def test_scenarios_reach_every_route():
    seen = {CASES[n]().routes[0] for n in CASES} | set(ref.batch_case().routes)
    assert seen == set(ref.ROUTES)


def test_route_model_edges():
    """n_cand 2048 against 2049, nms_pre 1536 against 1537, n_total 2048 against 2049."""
    boxes, valid = ref.disjoint(2304), np.ones(2304, bool)
    assert ref.route(ref.shared_top24(2304, 548, 1500), boxes, valid, 2000, 64, 0.7)[:3] == ('matrix', 2048, 1)
    assert ref.route(ref.shared_top24(2304, 549, 1500), boxes, valid, 2000, 64, 0.7)[:3] == ('invalid-fast', 2049, 0)
    s = ref.distinct_top24(2304)
    assert ref.route(s, boxes, valid, 1536, 64, 0.7)[0] == 'single'
    assert ref.route(s, boxes, valid, 1537, 64, 0.7)[0] == 'matrix'
    assert ref.route(s[:2048], boxes[:2048], valid[:2048], 2000, 64, 0.7)[0] == 'single'
    assert ref.route(s[:2049], boxes[:2049], valid[:2049], 2000, 64, 0.7)[0] == 'matrix'
    assert ref.route(s, boxes, valid, 2000, 1025, 0.7)[0] == 'large'
    big = ref.distinct_top24(9000)
    assert ref.route(big, ref.disjoint(9000), np.ones(9000, bool), 8193, 64, 0.7)[0] == 'large'
    assert ref.route(big, ref.disjoint(9000), np.ones(9000, bool), 8192, 64, 0.7)[0] == 'matrix'


# ------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize('min_size,ties', [(0, False), (40, True), (-1, False)])
def test_proposals_ref_equals_the_oracles_entry_point(min_size, ties):
    from fgn_amd.config import fgn_r50_c4_config, with_caps
    fh, fw, ih, iw = 20, 31, 317, 491
    cfg = with_caps(fgn_r50_c4_config(3, 3), nms_pre=1000, rpn_max=77)
    cfg['test_cfg']['rpn']['min_bbox_size'] = min_size
    g = torch.Generator().manual_seed(3)
    cls = torch.randn(15, fh, fw, generator=g) * 3
    if ties:
        cls = (cls * 2).round() / 2
    reg = torch.randn(60, fh, fw, generator=g) * 0.5
    want = O.rpn_get_bboxes(cls.numpy(), reg.numpy(), np.array([ih, iw, 3]), cfg)
    rp = cfg['rpn_head']
    anchors = O.grid_anchors(O.base_anchors(rp['anchor_scales'], rp['anchor_ratios'], 16), fh, fw, 16)
    scores = O.sigmoid32(cls.permute(1, 2, 0).reshape(-1).numpy())
    deltas = reg.permute(1, 2, 0).reshape(-1, 4).numpy()
    got = ref.proposals_ref(scores, anchors, deltas, 1000, 77, 0.7, min_size, (ih, iw), rp['target_means'], rp['target_stds'])
    assert len(want) == 77 and got.tobytes() == want.tobytes()


def test_scenario_decode_is_the_identity():
    """Zero deltas, means 0, stds 1, a 2^24 image: delta2bbox returns the anchors bit for bit, the wide flat boxes of the
    near-threshold pairs and the half-integer ones included."""
    for thr in (0.3, 0.5, 0.7):
        b = ref.pair_boxes(ref.near_threshold_pairs(thr))
        assert b.max() < (1 << 24)                                        # halving an integer below 2^24 is exact
        got = O.delta2bbox(b, np.zeros_like(b), ref.MEANS, ref.STDS, (ref.IMG, ref.IMG))
        assert got.tobytes() == b.tobytes()
    b = CASES['size-65536']().anchors
    assert O.delta2bbox(b, np.zeros_like(b), ref.MEANS, ref.STDS, (ref.IMG, ref.IMG)).tobytes() == b.tobytes()


def test_det_ref_equals_the_oracles_entry_point_and_the_builder_fixes_n_valid():
    from fgn_amd.config import fgn_r50_c4_config
    for n_ways, n_valid in ((1, 0), (3, 1), (3, 700), (8, 1025), (1, 300)):
        r = -(-max(n_valid, 1) // n_ways) + 3
        rois, reg = ref.det_rois(r, 1), np.zeros((r * n_ways, 4), F32)
        for equal in (False, True):
            cls = ref.cls_for_valid(r, n_ways, n_valid, seed=2, equal=equal)
            dets, labels, nv = ref.det_ref(rois, cls, reg, n_ways, (ref.IMG, ref.IMG), ref.MEANS, ref.STDS, 0.05, 0.5, 100)
            assert nv == n_valid
            cfg = fgn_r50_c4_config(n_ways, 1)
            cfg['roi_head']['bbox_head'].update(target_means=ref.MEANS, target_stds=ref.STDS)
            cs, bp = O.count_modified_cls_bbox(r, torch.from_numpy(cls), torch.from_numpy(reg), n_ways)
            wb, wl = O.bbox_get_bboxes(rois, cs.numpy(), bp.numpy(), np.array([ref.IMG, ref.IMG, 3]), cfg)
            assert dets.tobytes() == wb.tobytes() and np.array_equal(labels, wl)
            assert cfg['test_cfg']['rcnn']['score_thr'] == 0.05 and cfg['test_cfg']['rcnn']['nms_iou_threshold'] == 0.5


# ------------------------------------------------------------------------------------------ iou_gt
@pytest.mark.parametrize('thr', [0.3, 0.5, 0.7])
def test_iou_gt_emulation_equals_the_oracle_on_the_near_threshold_pairs(thr):
    pairs = ref.near_threshold_pairs(thr)
    t = F32(thr)
    groups = {}
    for grp, a, b in pairs:
        got, ex = ref.iou_gt_emulated(a, b, thr, with_exit=True)
        # the oracle itself: greedy NMS over the two boxes keeps one box iff the first suppresses the second
        kept = len(O.nms(np.stack([a, b]), np.array([0.9, 0.8], F32), thr)[1])
        assert bool(got[0]) == (kept == 1) == bool(ref.iou_gt_oracle(a, b, thr)[0]), (grp, a, b)
        groups.setdefault(grp, []).append((bool(got[0]), int(ex[0])))
        area = lambda v: (float(v[2]) - float(v[0])) * (float(v[3]) - float(v[1]))
        if grp == 'exact':
            inter = max(0.0, min(a[2], b[2]) - max(a[0], b[0])) * float(a[3] - a[1])
            p, q = ref._RATIONAL[thr]
            assert inter * q == (area(a) + area(b) - inter) * p               # the real-number IoU is p/q
        if grp in ('below', 'above', 'div-', 'div+'):
            fa, fb = F32(area(a)), F32(area(b))                               # b inside a: inter = area_b
            quo = fb / ((fa + fb) - fb)                                       # the oracle's fp32 expression
            d = int(np.array(quo).view(np.uint32)) - int(np.array(t).view(np.uint32))
            assert d in {'below': (-1,), 'above': (1,), 'div-': (-2, -8, -32), 'div+': (2, 8, 32)}[grp]
    assert all(g == (False, 3) for g in groups['exact'] + groups['below'] + groups['div-'] + groups['zero-zero'])
    assert all(g == (True, 3) for g in groups['above'] + groups['div+'])
    assert groups['zero-inside'] == [(False, 2)] and groups['identical'] == [(True, 1)]
    assert len(groups['div-']) == len(groups['div+']) == 6 and len(groups['exact']) == 4
    # the pairs that only the margin of the first shortcut decides rightly: without it they would be suppressed
    rnd = [(a, b) for grp, a, b in pairs if grp == 'round']
    assert len(rnd) == (0 if thr == 0.5 else 3) and all(g == (False, 3) for g in groups.get('round', []))
    for a, b in rnd:
        got, ex = ref.iou_gt_emulated(a, b, thr, with_exit=True, margins=(1.0, 0.999996))
        assert bool(got[0]) and int(ex[0]) == 1


def test_iou_gt_emulation_equals_the_oracle_on_two_million_pairs_swept_across_the_threshold():
    """One box fixed, the other shifted along x; its left edge is swept in steps of 1 or 8 floats through the shift
    at which the IoU crosses thr.  The emulated shortcuts may never decide differently from the oracle's division, and
    the family must leave through all three exits.  (2.06 M pairs per threshold.)"""
    rs = np.random.RandomState(1234)
    n_base, k = 8000, np.arange(-128, 129)
    for thr in (0.3, 0.5, 0.7):
        ox, oy = rs.uniform(0, 900, n_base), rs.uniform(0, 900, n_base)
        w, h = rs.uniform(8, 400, n_base), rs.uniform(8, 400, n_base)
        a = np.stack([ox, oy, ox + w, oy + h], 1).astype(F32)
        wf = a[:, 2].astype(np.float64) - a[:, 0]
        v = 2.0 * wf * float(F32(thr)) / (1.0 + float(F32(thr)))             # overlap width at which IoU == thr
        x1 = (a[:, 0] + (wf - v)).astype(F32)                                 # the crossing, rounded
        step = rs.choice([1, 1, 8], n_base)
        bits = x1.view(np.int32)[:, None] + (k[None, :] * step[:, None]).astype(np.int32)
        bx1 = bits.astype(np.int32).view(F32)
        bx2 = (bx1 + (a[:, 2] - a[:, 0])[:, None]).astype(F32)
        A = np.broadcast_to(a[:, None, :], (n_base, len(k), 4)).reshape(-1, 4)
        B = np.stack([bx1, np.broadcast_to(a[:, 1:2], bx1.shape), bx2, np.broadcast_to(a[:, 3:4], bx1.shape)], -1).reshape(-1, 4)
        assert len(A) >= 2_000_000
        got, ex = ref.iou_gt_emulated(A, B, thr, with_exit=True)
        want = ref.iou_gt_oracle(A, B, thr)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (thr, A[bad[:3]], B[bad[:3]])
        counts = np.bincount(ex, minlength=4)[1:]
        print('thr %g: exits (true shortcut, false shortcut, division) = %s, suppressing %d' % (thr, counts.tolist(), want.sum()))
        assert (counts > 50_000).all(), counts
        assert want[ex == 3].any() and not want[ex == 3].all()               # the division decides both ways
