"""Reference, route model and scenario builders for the selection stages (csrc/rpn_post.hip, csrc/det_post.hip,
csrc/post_common.h).  No GPU, no torch.cuda: tests/test_sel_ref_cpu.py checks this module on its own, and
tests/test_hip_sel_routes.py drives the kernels with it.

* ``proposals_ref`` / ``det_ref``: the expected bytes, composed from the oracle's own pieces (stable argsort, delta2bbox,
  min-size filter, nms / batched_nms; count_modified_cls_bbox, softmax32, multiclass_nms).
* ``route``: the integer rule by which ``fgn_rpn_proposals_f32`` picks one of its six routes, restated.
* builders: scores written as bit patterns (so the 12/12/8-bit histograms see a chosen structure) and box sets whose
  greedy NMS result is known by construction.  A scenario uses ``feat_h = feat_w = 1``, ``A = n_total``, zero deltas,
  ``means = 0``, ``stds = 1`` and a large image: candidate i is then exactly ``anchors[i]``.
* ``iou_gt_emulated``: post_common.h::iou_gt line by line in numpy fp32, with the exit each pair leaves through.
"""
import os
import re

import numpy as np
import torch

from oracle import fgn_ref_cpu as O

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'fgn_amd', 'csrc')

# ---------------------------------------------------------------------------------------------- the kernels' constants
FAST_SEL = 1536        # RPN_FAST_SEL: rank whose top-24 key bits are the pre-selection's threshold
FAST_CAP = 2048        # RPN_FAST_CAP: most candidates the pre-selection accepts
SORT_MAX = 8192        # largest in-LDS sort of rpn_proposals_kernel; more candidates -> the global sort
OUT_MAX = 1024         # most proposals rpn_proposals_kernel keeps; more -> the global sort
N_TOTAL_MAX = 65536    # RPN_EPT * POST_THREADS
DET_SPLIT = 1024       # POST_THREADS: n_valid <= this sorts in registers, above in LDS
ROUTES = ('single', 'matrix', 'dry', 'invalid-fast', 'invalid-full', 'large')

IMG = 1 << 24          # image side of the scenarios: every coordinate used is exact in fp32 and never clipped
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)


def source_constants() -> dict:
    """The same constants as the sources state them: the ``constexpr int`` lines of rpn_post.hip / post_common.h, the
    shape test of fgn_rpn_proposals_f32, the sort split of det_post_kernel and the route test of ops.rpn_proposals."""
    rpn = open(os.path.join(CSRC, 'rpn_post.hip')).read()
    com = open(os.path.join(CSRC, 'post_common.h')).read()
    det = open(os.path.join(CSRC, 'det_post.hip')).read()
    ops = open(os.path.join(ROOT, 'fgn_amd', 'ops.py')).read()

    def cx(text, name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))
    shape = re.search(r'if \(cap > (\d+) \|\| max_per_img > (\d+) \|\| max_per_img < 1\) return FGN_ERR_SHAPE;', rpn)
    py = re.search(r'if \(n_sel > (\d+) or max_per_img > (\d+)\) and not', ops)
    launch = re.search(r'n_sel > (\w+) && p\.n_total > (\w+)\)', rpn)
    assert re.search(r'if \(n_valid <= POST_THREADS\) \{', det)
    assert re.search(r'if \(p\.n_total > RPN_EPT \* POST_THREADS\) return FGN_ERR_SHAPE;', rpn)
    return {'FAST_SEL': cx(rpn, 'RPN_FAST_SEL'), 'FAST_CAP': cx(rpn, 'RPN_FAST_CAP'),
            'SORT_MAX': int(shape.group(1)), 'OUT_MAX': int(shape.group(2)),
            'SORT_MAX_py': int(py.group(1)), 'OUT_MAX_py': int(py.group(2)),
            'N_TOTAL_MAX': cx(rpn, 'RPN_EPT') * cx(com, 'POST_THREADS'), 'DET_SPLIT': cx(com, 'POST_THREADS'),
            'launch': (launch.group(1), launch.group(2)), 'BINS': cx(rpn, 'RPN_BINS')}


# ---------------------------------------------------------------------------------------------- keys and ranking
def key_hi(scores: np.ndarray) -> np.ndarray:
    """h = ~ordered(score), the high word of the kernels' composite sort key (ascending h = descending score)."""
    b = np.ascontiguousarray(scores, F32).view(np.uint32)
    ordered = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return (~ordered).astype(np.uint32)


def scores_from_keys(top24: np.ndarray, low: np.ndarray) -> np.ndarray:
    """The positive float whose key h is ``(top24 << 8) | low``."""
    h = (np.asarray(top24, np.int64) << 8) | np.asarray(low, np.int64)
    bits = 0x7fffffff - h
    assert (bits > 0x00800000).all() and (bits <= 0x3f800000).all(), 'score outside (0, 1] or denormal'
    return bits.astype(np.uint32).view(F32)


def ranked_ref(scores: np.ndarray, n: int) -> np.ndarray:
    """The first n anchor indices of the oracle's stable descending order."""
    return np.argsort(-np.asarray(scores, F32), kind='stable')[:n]


# ---------------------------------------------------------------------------------------------- references
def proposals_ref(scores, anchors, deltas, nms_pre, max_out, iou_thr, min_size, img_hw, means, stds) -> np.ndarray:
    """RPNHead._get_bboxes_single for one image from the oracle's pieces -> [k, 5].  ``min_size < 0``: no filter."""
    scores, anchors, deltas = np.asarray(scores, F32), np.asarray(anchors, F32), np.asarray(deltas, F32)
    if 0 < nms_pre < scores.shape[0]:
        rank = ranked_ref(scores, nms_pre)
        scores, deltas, anchors = scores[rank], deltas[rank], anchors[rank]
    props = O.delta2bbox(anchors, deltas, means, stds, (int(img_hw[0]), int(img_hw[1])))
    if min_size >= 0:
        ok = ((props[:, 2] - props[:, 0]) > min_size) & ((props[:, 3] - props[:, 1]) > min_size)
        props, scores = props[ok], scores[ok]
    if props.size == 0:
        return np.zeros((0, 5), F32)
    dets, _ = O.batched_nms(props, scores, np.zeros(len(props), np.int64), iou_thr)
    return dets[:max_out]


def det_ref(rois, cls_raw, reg_raw, n_ways, img_hw, means, stds, score_thr, iou_thr, max_out):
    """BBoxHead.get_bboxes behind count_modified_cls_bbox from the oracle's pieces -> (dets [k, 5], labels [k], n_valid);
    n_valid = the candidates over ``score_thr`` (what det_post_kernel sorts)."""
    r = rois.shape[0]
    cls_score, bbox_pred = O.count_modified_cls_bbox(r, torch.as_tensor(cls_raw), torch.as_tensor(reg_raw), n_ways)
    scores = O.softmax32(cls_score.numpy())
    n_valid = int((scores[:, :-1] > F32(score_thr)).sum())
    if r == 0:
        return np.zeros((0, 5), F32), np.zeros((0,), np.int64), 0
    boxes = O.delta2bbox(np.asarray(rois, F32)[:, 1:], bbox_pred.numpy(), means, stds, (int(img_hw[0]), int(img_hw[1])))
    dets, labels = O.multiclass_nms(boxes, scores, score_thr, iou_thr, max_out)
    return dets, labels, n_valid


# ---------------------------------------------------------------------------------------------- route model
def route(scores, boxes, valid, nms_pre, max_out, iou_thr):
    """-> (route name, n_cand, ok, kept_in_prefix): which of ROUTES fgn_rpn_proposals_f32 (behind ops.rpn_proposals)
    takes for one image.  ``boxes`` / ``valid``: decoded box and min-size flag per anchor index."""
    scores = np.asarray(scores, F32)
    n_total = scores.shape[0]
    n_sel = nms_pre if 0 < nms_pre < n_total else n_total
    if n_sel > SORT_MAX or max_out > OUT_MAX:
        return 'large', 0, 0, -1
    if n_sel <= FAST_SEL or n_total <= FAST_CAP:
        return 'single', 0, 0, -1
    order = ranked_ref(scores, n_total)
    t24 = key_hi(scores) >> 8
    thr24 = t24[order[FAST_SEL - 1]]
    n_cand = int((t24 <= thr24).sum())
    ok = n_cand <= FAST_CAP
    n = min(n_cand, n_sel) if ok else FAST_SEL
    pre = order[:n]
    pre = pre[np.asarray(valid, bool)[pre]]
    kept = len(O.nms(np.asarray(boxes, F32)[pre], scores[pre], iou_thr)[1]) if len(pre) else 0
    if ok:
        name = 'matrix' if (kept >= max_out or n >= n_sel) else 'dry'
    else:
        name = 'invalid-fast' if kept >= max_out else 'invalid-full'
    return name, n_cand, int(ok), kept


def preselect_bins(scores):
    """(b1, count before b1, b2) of the two histogram levels, as rpn_find_bin reports them in info[0..2]."""
    scores = np.asarray(scores, F32)
    t24 = key_hi(scores) >> 8
    thr24 = int(np.sort(t24)[FAST_SEL - 1])
    return thr24 >> 12, int(((t24 >> 12) < (thr24 >> 12)).sum()), thr24 & 4095


# ---------------------------------------------------------------------------------------------- score patterns (by rank)
T0 = 0x409000          # first top-24 value of level-1 bin 0x409; 1.0f has top-24 0x407fff, low byte 0xff


def _low(n):
    return (np.arange(n) * 37 + 11) % 256


def distinct_top24(n, t0=T0 - 700):
    """n scores, every one with its own top-24 key bits: n_cand == 1536.  The default start puts 700 keys in level-1 bin
    0x408 and the rest in 0x409."""
    return scores_from_keys(t0 + np.arange(n), _low(n))


def shared_top24(n, count, at_rank, t0=T0 - 700):
    """As distinct_top24, but ranks [at_rank, at_rank + count) share one top-24 value (low bytes ascending, repeating
    once count > 256): with at_rank < 1536 <= at_rank + count, n_cand == at_rank + count."""
    i = np.arange(n)
    top = np.where(i < at_rank, i, np.where(i < at_rank + count, at_rank, i - count + 1))
    low = np.where((i >= at_rank) & (i < at_rank + count), ((i - at_rank) * 256) // max(count, 1), _low(n))
    return scores_from_keys(t0 + top, low)


def fill_bin_exactly(level, n=2304, lead=0):
    """The cumulative count reaches 1536 exactly at the end of a bin.  level 1: rank 1535 holds the last level-2 slot of
    its level-1 bin, rank 1536 opens the next level-1 bin.  level 2: four keys per top-24 value, 1536 = 384 whole bins;
    ``lead`` (1..3) keys in front shift the groups, so that rank 1536 falls inside a bin (n_cand == 1536 + lead)."""
    i = np.arange(n)
    if level == 1:
        return scores_from_keys(T0 + 4096 - FAST_SEL + i, _low(n))
    g = np.where(i < lead, 0, (i - lead) // 4 + (1 if lead else 0))
    low = np.where(i < lead, i, ((i - lead) % 4) * 64)
    return scores_from_keys(T0 - 100 + g, low)


def first_bin(n=2304, first=1700):
    """The threshold lies in the first non-empty level-1 bin (count before it 0); the other keys two bins on."""
    i = np.arange(n)
    return scores_from_keys(np.where(i < first, T0 + i, T0 + 8192 + i), _low(n))


def all_equal(n):
    return np.full(n, 1.0, F32)


# ---------------------------------------------------------------------------------------------- box sets (by rank)
def disjoint(n, per_row=64, size=20.0, cell=24.0, origin=(0.0, 1000.0)):
    k = np.arange(n)
    x = origin[0] + cell * (k % per_row)
    y = origin[1] + cell * (k // per_row)
    return np.stack([x, y, x + size, y + size], 1).astype(F32)


def clusters(n, m, origin=(0.0, 0.0)):
    """Box k lies in cluster k % m, jittered by 0..3 px inside it: the first box of a cluster suppresses the others
    (IoU >= 47 / 53)."""
    k = np.arange(n)
    x = origin[0] + 100.0 * (k % m) + ((k // m) % 4)
    y = np.full(n, origin[1])
    return np.stack([x, y, x + 50.0, y + 50.0], 1).astype(F32)


def staircase(n, shift, origin=(0.0, 0.0)):
    """64 x 64 boxes, each ``shift`` px right of the one before: with 10 every box overlaps only its neighbours above the
    0.7 threshold (54/74), with 3 its next few."""
    x = origin[0] + float(shift) * np.arange(n)
    y = np.full(n, origin[1])
    return np.stack([x, y, x + 64.0, y + 64.0], 1).astype(F32)


# ---------------------------------------------------------------------------------------------- iou_gt
def iou_gt_emulated(a, b, thr, with_exit=False, margins=(1.000004, 0.999996)):
    """post_common.h::iou_gt(a, b, thr) in numpy fp32, one line per line.  a, b: [..., 4].  ``with_exit``: also the exit
    taken (1 = first shortcut, true; 2 = second shortcut, false; 3 = the division).  ``margins``: the two factors of the
    shortcuts, the kernel's by default (a test narrows them to show which pairs they protect)."""
    a = np.asarray(a, F32).reshape(-1, 4)
    b = np.asarray(b, F32).reshape(-1, 4)
    thr = F32(thr)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    xx1, yy1 = np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])
    xx2, yy2 = np.minimum(a[:, 2], b[:, 2]), np.minimum(a[:, 3], b[:, 3])
    w, h = np.maximum(F32(0), xx2 - xx1), np.maximum(F32(0), yy2 - yy1)
    inter = w * h
    uni = (area_a + area_b) - inter
    tu = thr * uni
    assert inter.dtype == uni.dtype == tu.dtype == F32
    e1 = (inter > tu * F32(margins[0])) & (uni > F32(0)) & (tu < F32(3.0e38))
    e2 = ~e1 & (inter < tu * F32(margins[1])) & (uni > F32(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        ovr = inter / uni
    res = np.where(e1, True, np.where(e2, False, ovr > thr))
    if with_exit:
        return res, np.where(e1, 1, np.where(e2, 2, 3))
    return res


def iou_gt_oracle(a, b, thr):
    """The oracle's test (O.nms): ``inter / ((area_a + area_b) - inter) > thr`` in fp32."""
    a = np.asarray(a, F32).reshape(-1, 4)
    b = np.asarray(b, F32).reshape(-1, 4)
    area_a = ((a[:, 2] - a[:, 0]).astype(F32) * (a[:, 3] - a[:, 1]).astype(F32)).astype(F32)
    area_b = ((b[:, 2] - b[:, 0]).astype(F32) * (b[:, 3] - b[:, 1]).astype(F32)).astype(F32)
    w = np.maximum(F32(0), (np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0])).astype(F32))
    h = np.maximum(F32(0), (np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1])).astype(F32))
    inter = (w * h).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        ovr = (inter / ((area_a + area_b).astype(F32) - inter).astype(F32)).astype(F32)
    return ovr > F32(thr)


_RATIONAL = {0.3: (3, 10), 0.5: (1, 2), 0.7: (7, 10)}


def _contained(wa, ha, wb, hb):
    """a = [0, 0, wa, ha] and b = [0, 0, wb, hb] inside it: inter = wb * hb, union = wa * ha, integers below 2^24."""
    return np.array([0, 0, wa, ha], F32), np.array([0, 0, wb, hb], F32)


def _search_contained(target, want=2):
    """Contained pairs whose fp32 quotient ``inter / ((area_a + area_b) - inter)`` is exactly the float ``target``.
    Every coordinate stays below 2^23 (so that box centres, halves of odd widths, are exact in the decode) and the
    union below 2^24; the heights (ha, hb) open unions that are odd and near 2^24, which 0.5 - 1 ulp needs."""
    found = []
    for ha, hb in ((1, 1), (5, 3), (3, 2), (7, 4), (7, 5), (5, 4), (3, 1), (7, 3)):
        hi = min((1 << 24) // ha, 1 << 23) - 1
        wa = np.arange(hi - 60000, hi, dtype=np.int64)
        for off in (0, 1):
            wb = np.floor(float(target) * (wa * ha) / hb).astype(np.int64) + off
            fa, fb = (wa * ha).astype(F32), (wb * hb).astype(F32)            # the areas: exact products
            quo = fb / ((fa + fb) - fb)
            for j in np.nonzero((quo == target) & (wb <= wa) & (wb > 0))[0][:want - len(found)]:
                found.append(_contained(int(wa[j]), ha, int(wb[j]), hb))
            if len(found) >= want:
                return found
    return found


def _search_round(t, want=3):
    """Contained pairs of height 1 with fl(inter / union) == t although ``inter > fl(t * union)``: the real quotient lies
    above t by less than half a float of t, and the product rounds down past inter.  A first shortcut without its margin
    would suppress here; the division does not.  (None exist at 0.5: t * union is exact.)"""
    found = []
    for lo in (11_200_001, 13_000_001, 5_600_001):
        wa = np.arange(lo, lo + 60000, dtype=np.int64)
        for off in (0, 1):
            wb = np.floor(float(t) * wa).astype(np.int64) + off
            fa, fb = wa.astype(F32), wb.astype(F32)
            uni = (fa + fb) - fb
            hit = np.nonzero((fb / uni == t) & (fb > t * uni) & (wb <= wa))[0]
            found += [_contained(int(wa[j]), 1, int(wb[j]), 1) for j in hit[::max(len(hit) // want, 1)][:want]]
            if len(found) >= want:
                return found[:want]
    return found


_PAIRS = {}


def near_threshold_pairs(thr):
    """[(group, a, b)] of integer / half-integer boxes at the origin, a the earlier box, for thr in {0.3, 0.5, 0.7}:
      'exact'  the real-number IoU is the rational p/q that rounds to thr (two boxes of one height, shifted)
      'below' / 'above'  fl(inter / union) is the float next to thr (a box inside a wide, flat box)
      'div-'  / 'div+'   fl(inter / union) lies 2, 8 or 32 floats from thr: inside the 4e-6 margin, the division decides
      'round'  fl(inter / union) == thr, not suppressed, though inter > fl(thr * union) (0.3 and 0.7 only): _search_round
      'zero-zero', 'zero-inside', 'identical'  the degenerate pairs (0/0 = NaN; inter 0; IoU 1).
    No box is higher than 7."""
    key = round(float(thr), 1)
    if key in _PAIRS:
        return _PAIRS[key]
    p, q = _RATIONAL[key]
    t = F32(thr)
    out = []
    for k, hgt in ((1, 1.0), (2, 2.5), (3, 7.0), (8, 4.0)):
        wid, s = (p + q) * k / 2.0, (q - p) * k / 2.0
        out.append(('exact', np.array([0, 0, wid, hgt], F32), np.array([s, 0, s + wid, hgt], F32)))
    tb = int(np.array(t).view(np.uint32))
    for grp, steps in (('below', (-1,)), ('above', (1,)), ('div-', (-2, -8, -32)), ('div+', (2, 8, 32))):
        for d in steps:
            hits = _search_contained(np.array(tb + d, np.uint32).view(F32))
            assert hits, (thr, grp, d)
            out += [(grp, a, b) for a, b in hits]
    out += [('round', a, b) for a, b in _search_round(t)]
    z = np.array([5, 3, 5, 3], F32)
    out.append(('zero-zero', z, z.copy()))
    out.append(('zero-inside', np.array([0, 0, 10, 6], F32), z.copy()))
    out.append(('identical', np.array([0, 0, 10, 6], F32), np.array([0, 0, 10, 6], F32)))
    _PAIRS[key] = out
    return out


DEGENERATE = ('zero-zero', 'zero-inside', 'identical')


def pair_boxes(pairs, pitch=8.0):
    """The pairs laid out as ranked neighbours (rows 2j, 2j + 1), pair j moved down by j * pitch: isolated from each
    other (no pair is higher than 7)."""
    rows = []
    for j, (_, a, b) in enumerate(pairs):
        o = np.array([0, j * pitch, 0, j * pitch], F32)
        rows += [a + o, b + o]
    return np.stack(rows).astype(F32)


# ---------------------------------------------------------------------------------------------- proposal scenarios
class Case:
    """One launch: scores [B, n_total] and the box of every anchor; per image the route it is built to take and the
    candidate count it claims (None where the pre-selection does not run)."""

    def __init__(self, name, scores, anchors, nms_pre, max_out, routes, n_cand, iou_thr=0.7, min_size=0.0):
        self.name = name
        self.scores = np.ascontiguousarray(np.atleast_2d(scores), F32)
        self.anchors = np.ascontiguousarray(anchors, F32)
        self.nms_pre, self.max_out, self.iou_thr, self.min_size = nms_pre, max_out, iou_thr, float(min_size)
        self.routes = [routes] * len(self.scores) if isinstance(routes, str) else list(routes)
        self.n_cand = n_cand if isinstance(n_cand, (list, tuple)) else [n_cand] * len(self.scores)
        self._memo = {}

    @property
    def n_total(self):
        return self.scores.shape[1]

    @property
    def n_sel(self):
        return self.nms_pre if 0 < self.nms_pre < self.n_total else self.n_total

    def valid(self):
        b = self.anchors
        if self.min_size < 0:
            return np.ones(len(b), bool)
        return ((b[:, 2] - b[:, 0]) > F32(self.min_size)) & ((b[:, 3] - b[:, 1]) > F32(self.min_size))

    def route(self, b=0):
        key = ('route', self.scores[b].tobytes())                     # (images with the same scores share the work)
        if key not in self._memo:
            self._memo[key] = route(self.scores[b], self.anchors, self.valid(), self.nms_pre, self.max_out, self.iou_thr)
        return self._memo[key]

    def reference(self, b=0):
        """The [max_out, 5] rows of image b (zero rows after the kept ones) and the kept count."""
        key = ('ref', self.scores[b].tobytes())
        if key in self._memo:
            return self._memo[key]
        n = self.n_total
        ref = proposals_ref(self.scores[b], self.anchors, np.zeros((n, 4), F32), self.nms_pre, self.max_out, self.iou_thr,
                            self.min_size, (IMG, IMG), MEANS, STDS)
        out = np.zeros((self.max_out, 5), F32)
        out[:len(ref)] = ref
        self._memo[key] = (out, len(ref))
        return out, len(ref)


def _case(name, by_rank, boxes_by_rank, nms_pre, max_out, routes, n_cand, seed=0, **kw):
    """Scores scattered over the anchor indices by a seeded permutation; the box of rank r goes to the anchor that really
    ranks r-th (among equal scores: the lower anchor index)."""
    n = len(by_rank)
    assert len(boxes_by_rank) == n
    scores = np.empty(n, F32)
    scores[np.random.RandomState(seed).permutation(n)] = by_rank
    anchors = np.empty((n, 4), F32)
    anchors[ranked_ref(scores, n)] = boxes_by_rank
    return Case(name, scores, anchors, nms_pre, max_out, routes, n_cand, **kw)


def _clustered_then_disjoint(n, head, m):
    return np.concatenate([clusters(head, m), disjoint(n - head)])


N, PRE = 2304, 2000       # the workhorse: three histogram workgroups, the last one partial


def _threshold_case(thr, nms_pre):
    pairs = [pr for pr in near_threshold_pairs(thr) if pr[0] not in DEGENERATE]
    pb = pair_boxes(pairs)
    boxes = np.concatenate([pb, disjoint(N - len(pb), origin=(0.0, 100000.0))])
    single = nms_pre <= FAST_SEL
    return _case('threshold-%g-%d' % (thr, nms_pre), distinct_top24(N), boxes, nms_pre, 300,
                 'single' if single else 'matrix', None if single else 1536, iou_thr=thr, seed=5)


def _min_size_boxes(n):
    """Disjoint 20 x 20 boxes; at ranks 0, 63, 64 and 128..191 boxes only 16 high (not > 16) that cover most of the NEXT
    valid box (IoU 0.8): an invalid box that suppressed, or was kept, would change the result."""
    b = disjoint(n)
    bad = np.r_[0, 63, 64, 128:192]
    nxt = {0: 1, 63: 65, 64: 65}
    for r in bad:
        t = nxt.get(int(r), 192 + (int(r) - 128))
        b[r] = b[t]
        b[r, 3] = b[r, 1] + 16.0
    return b


def batch_case():
    """Five images in one launch, each on another route.  One anchor set serves them all: 2200 clustered boxes (10
    clusters) then 104 disjoint ones; each image ranks them in its own order."""
    anchors = np.concatenate([clusters(2200, 10), disjoint(104)])
    cl, dj = np.arange(2200), np.arange(2200, 2304)
    plans = [('matrix', distinct_top24(N), np.r_[dj, cl], 1536),                         # fill
             ('matrix', shared_top24(N, 548, 1500), np.r_[cl, dj], 2048),                # exhaust: 10 kept of 2000
             ('dry', distinct_top24(N), np.r_[cl[:1700], dj, cl[1700:]], 1536),
             ('invalid-fast', shared_top24(N, 600, 1500), np.r_[dj, cl], 2100),
             ('invalid-full', all_equal(N), np.arange(N), N)]
    scores = np.empty((len(plans), N), F32)
    for b, (_, by_rank, anchor_of_rank, _) in enumerate(plans):
        scores[b, anchor_of_rank] = by_rank
    return Case('batch', scores, anchors, PRE, 32, [p[0] for p in plans], [p[3] for p in plans])


def scratch_case():
    """Seventeen images at nms_pre 3000 (a sort buffer of 4096 boxes per image), four of which are inside
    rpn_proposals_kernel at the same time on different attempts: images 7 and 8 start at the full attempt (dry), images 15
    and 16 (all scores equal) run attempt 0 on 1536 candidates and then the full attempt.  The scratch of image b's attempt
    0 used to start at b * 2048 boxes: image 15's inside the 4096 of image 7, image 16's inside those of image 8 - and
    workgroups b and b + 8 share an XCD and its L2, so each sees the other's stores.  (Across XCDs the L2s are not
    coherent and hide the overlap; that is why the pairs sit eight apart.  The other images fill from their ranked
    prefix and leave at once.)  So that either image of a pair is still reading when the other one writes, both NMS walks
    are long: ranks 0..1535 alternate 768 disjoint boxes with 768 copies moved by a pixel (768 kept, slowly), ranks
    1536..2047 are more copies, and max_out 1000 is only reached with the fresh boxes of ranks 2048..2999.  A full attempt
    that reads another image's attempt-0 boxes there finds copies and ends short of 1000; an attempt 0 that reads another
    image's fresh boxes can fill 1000 and never reach its full attempt."""
    n, images = 6100, 17
    g1 = disjoint(768)
    anchors = disjoint(n, origin=(0.0, 3000.0))
    anchors[0:1536:2] = g1
    anchors[1:1536:2] = g1 + np.array([1, 0, 1, 0], F32)
    anchors[1536:2048] = g1[:512] + np.array([0, 2, 0, 2], F32)
    scores = np.empty((images, n), F32)
    scores[:, np.r_[2048:n, 0:2048]] = distinct_top24(n)              # the fresh boxes rank first: fills from the prefix
    routes, n_cand = ['matrix'] * images, [1536] * images
    for b in (7, 8):
        rs = np.random.RandomState(31 + b)
        scores[b, np.r_[0:2048, 2048 + rs.permutation(n - 2048)]] = distinct_top24(n)
        routes[b] = 'dry'
    for b in (15, 16):
        scores[b] = 1.0
        routes[b], n_cand[b] = 'invalid-full', n
    return Case('batch-scratch', scores, anchors, 3000, 1000, routes, n_cand)


def proposal_cases():
    """name -> builder of every single-launch proposal scenario.  Builders, so that collecting the tests
    costs nothing."""
    c = {}

    def add(name, fn):
        assert name not in c
        c[name] = fn
    for mo in (1, 63, 64, 65, 128, 300):
        add('fill-%d' % mo, lambda mo=mo: _case('fill', distinct_top24(N), disjoint(N), PRE, mo, 'matrix', 1536, seed=1))
    for sh in (10, 3):
        add('staircase-%d' % sh, lambda sh=sh: _case('staircase', distinct_top24(N), np.concatenate(
            [staircase(200, sh), disjoint(N - 200)]), PRE, 300, 'matrix', 1536, seed=2))
    for pre in (1537, 1600, 2048):
        add('exhaust-%d' % pre, lambda pre=pre: _case('exhaust', shared_top24(N, 548, 1500), clusters(N, 5), pre, 64,
                                                       'matrix', 2048, seed=3))
    add('edge-1536', lambda: _case('edge-1536', distinct_top24(N), disjoint(N), 1536, 300, 'single', None, seed=4))
    add('edge-1537', lambda: _case('edge-1537', distinct_top24(N), disjoint(N), 1537, 300, 'matrix', 1536, seed=4))
    add('dry', lambda: _case('dry', distinct_top24(N), _clustered_then_disjoint(N, 1700, 10), PRE, 64, 'dry', 1536, seed=6))
    add('dry-zero', lambda: _case('dry-zero', distinct_top24(N), _clustered_then_disjoint(N, 1700, 10), PRE, 400, 'dry',
                                  1536, seed=7))
    for pre in (3000, 6000):
        add('dry-%d' % (4096 if pre == 3000 else 8192), lambda pre=pre: _case(
            'dry-big', distinct_top24(6100), _clustered_then_disjoint(6100, 1700, 10), pre, 64, 'dry', 1536, seed=8))
    for tag, by_rank, nc in (('2049', lambda: shared_top24(N, 549, 1500), 2049),
                             ('2100', lambda: shared_top24(N, 600, 1500), 2100), ('equal', lambda: all_equal(N), N)):
        add('invalid-fast-' + tag, lambda f=by_rank, nc=nc: _case('invalid-fast', f(), disjoint(N), PRE, 64,
                                                                  'invalid-fast', nc, seed=9))
        add('invalid-full-' + tag, lambda f=by_rank, nc=nc: _case('invalid-full', f(), _clustered_then_disjoint(N, 1700, 10),
                                                                  PRE, 64, 'invalid-full', nc, seed=10))
    add('boundary-2048', lambda: _case('boundary-2048', shared_top24(N, 548, 1500), disjoint(N), PRE, 64, 'matrix', 2048,
                                       seed=11))
    add('boundary-2048-dry', lambda: _case('boundary-2048-dry', shared_top24(N, 548, 1500),
                                           _clustered_then_disjoint(N, 2100, 10), 2200, 64, 'dry', 2048, seed=11))
    add('boundary-l1-end', lambda: _case('l1-end', fill_bin_exactly(1), disjoint(N), PRE, 64, 'matrix', 1536, seed=12))
    add('boundary-l2-end', lambda: _case('l2-end', fill_bin_exactly(2), disjoint(N), PRE, 64, 'matrix', 1536, seed=12))
    add('boundary-l2-inside', lambda: _case('l2-inside', fill_bin_exactly(2, lead=3), disjoint(N), PRE, 64, 'matrix', 1539,
                                            seed=12))
    add('boundary-one-l1-bin', lambda: _case('one-l1-bin', distinct_top24(N, t0=T0), _clustered_then_disjoint(N, 1700, 10),
                                             PRE, 64, 'dry', 1536, seed=13))
    add('boundary-first-bin', lambda: _case('first-bin', first_bin(), disjoint(N), PRE, 64, 'matrix', 1536, seed=13))
    add('min-size-16', lambda: _case('min-size-16', distinct_top24(N), _min_size_boxes(N), PRE, 300, 'matrix', 1536,
                                     min_size=16.0, seed=14))

    def zero_width():
        b = disjoint(N)
        b[::3, 2] = b[::3, 0]                      # every third rank: width 0, height 20
        return b
    add('min-size-0', lambda: _case('min-size-0', distinct_top24(N), zero_width(), PRE, 300, 'matrix', 1536, seed=15))

    def zero_area():
        deg = [pr for pr in near_threshold_pairs(0.7) if pr[0] in DEGENERATE]
        b = disjoint(N, origin=(0.0, 100000.0))
        b[:2 * len(deg)] = pair_boxes(deg)
        b[10::7, 2:] = b[10::7, :2]                # points: zero width and height, each alone
        return b
    add('min-size-off', lambda: _case('min-size-off', distinct_top24(N), zero_area(), PRE, 300, 'matrix', 1536,
                                      min_size=-1.0, seed=16))
    for thr in (0.3, 0.5, 0.7):
        for pre in (PRE, 1536):
            add('threshold-%g-%d' % (thr, pre), lambda thr=thr, pre=pre: _threshold_case(thr, pre))
    add('size-2049', lambda: _case('size-2049', distinct_top24(2049), disjoint(2049), 1537, 64, 'matrix', 1536, seed=17))
    add('size-3000', lambda: _case('size-3000', distinct_top24(3000), _clustered_then_disjoint(3000, 1700, 10), PRE, 64,
                                   'dry', 1536, seed=18))
    add('size-65536', lambda: _case('size-65536', distinct_top24(65536), disjoint(65536, per_row=256), PRE, 64, 'matrix',
                                    1536, seed=19))
    add('size-65536-dry', lambda: _case('size-65536-dry', distinct_top24(65536),
                                        _clustered_then_disjoint(65536, 1700, 10), PRE, 64, 'dry', 1536, seed=20))

    def straddle(n):
        b = disjoint(n, per_row=128)
        b[1020:1028, 3] = b[1020:1028, 1] + 16.0   # ranks 1020..1027 fail min_size 16
        return b
    add('large-2304', lambda: _case('large', distinct_top24(N), disjoint(N, per_row=128), PRE, 1025, 'large', None, seed=21))
    add('large-2304-equal', lambda: _case('large', all_equal(N), straddle(N), PRE, 1100, 'large', None, min_size=16.0,
                                          seed=22))
    add('large-5000', lambda: _case('large', shared_top24(5000, 600, 900), straddle(5000), 4500, 1100, 'large', None,
                                    min_size=16.0, seed=23))
    add('large-5000-chains', lambda: _case('large', distinct_top24(5000), np.concatenate(
        [staircase(1200, 10), disjoint(3800, per_row=128)]), 4500, 1025, 'large', None, seed=24))
    return c


# ---------------------------------------------------------------------------------------------- detection inputs
def det_rois(r, seed=0):
    """r RoIs (image index 0): 30 x 30 boxes on a 40 px grid, every odd one moved onto its left neighbour (IoU 0.76), in
    a seeded order."""
    k = np.random.RandomState(seed).permutation(r)
    x = 40.0 * ((k // 2) % 50) + 2.0 * (k % 2)
    y = 40.0 * ((k // 2) // 50)
    return np.stack([np.zeros(r), x, y, x + 30.0, y + 30.0], 1).astype(F32)


def cls_for_valid(r, n_ways, n_valid, seed=0, equal=False):
    """cls_raw [r * n_ways, 2] (column 0 background, column 1 class) with exactly ``n_valid`` candidates over any
    score_thr in [1e-9, 0.05]: the chosen candidates carry class logits in [0, 0.5] (all 0 with ``equal``), every other
    class logit is -30; a RoI with a chosen candidate has background -30 (its chosen classes share the mass: each at
    least 1 / (1 + 7 e^0.5) = 0.08), a RoI without has background +30 (every class e^-60)."""
    rs = np.random.RandomState(seed)
    chosen = np.zeros(r * n_ways, bool)
    chosen[rs.permutation(r * n_ways)[:n_valid]] = True
    cls = np.full((r * n_ways, 2), -30.0, F32)
    cls[chosen, 1] = 0.0 if equal else rs.uniform(0.0, 0.5, n_valid).astype(F32)
    row_has = chosen.reshape(r, n_ways).any(1)
    cls[:, 0] = np.repeat(np.where(row_has, -30.0, 30.0), n_ways).astype(F32)
    return cls
