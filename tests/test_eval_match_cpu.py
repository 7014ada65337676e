"""The matched bits on the host (no GPU): ``fsiseg_eval.match_flags`` is the evaluator's own rule, the evaluator reads
the bits instead of forming IoUs and returns the same numbers, and a sharded evaluation that gathers only the bits
(``dist.pack_matches`` / ``gather_matches`` / ``results_from_matches``) equals the single-process one.  Every comparison
is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _eval_match_cases import N_WAYS, THR_SETS, crafted, plain_evaluate_img, plain_flags, random_res   # noqa: E402

TYPES = ('bbox', 'segm')


@pytest.fixture(scope='module')
def images():
    return [random_res(s) for s in range(200)]


def test_match_flags_equal_the_evaluators_matching(images):
    """200 random images, both IoU types, T = 1: bit 0 at the positions ``_evaluate_img`` selects is its ``dtm``, what
    it does not select is -1 (beyond max_dets) or 0 (label outside the ways); and ``_evaluate_img`` still is the plain
    double loop."""
    from fgn_amd.fsiseg_eval import FSISEGEval, match_flags
    seen_cut = seen_match = 0
    for res in images:
        for kind in TYPES:
            flags = match_flags(res, (0.5,), kind, n_ways=N_WAYS)
            assert flags.dtype == np.int32 and flags.shape == res['dt_scores'].shape
            assert np.array_equal(flags, plain_flags(res, (0.5,), kind))
            ev = FSISEGEval(results=[res], n_ways=N_WAYS, iou_type=kind)
            covered = np.zeros(len(flags), bool)
            for k in range(N_WAYS):
                got, want = ev._evaluate_img(res, k), plain_evaluate_img(res, k, kind, 0.5)
                assert (got is None) == (want is None)
                if got is None:
                    continue
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
                assert np.array_equal(flags[want[3]] & 1, want[1].astype(np.int32))
                covered[want[3]] = True
                seen_match += int(want[1].sum())
            cats = res['dt_cat_ids']
            inside = (cats >= 0) & (cats < N_WAYS)
            assert np.all(flags[~covered & inside] == -1) and np.all(flags[~inside] == 0)
            seen_cut += int((flags == -1).sum())
    assert seen_match > 500 and seen_cut == 0          # (no category of 130 / 3 detections exceeds 100: see the crafted case)


@pytest.mark.parametrize('n_thr', [1, 10, 16])
def test_match_flags_at_several_thresholds(images, n_thr):
    from fgn_amd.fsiseg_eval import match_flags
    thrs = THR_SETS[n_thr]
    assert len(thrs) == n_thr
    for res in images[:60]:
        for kind in TYPES:
            flags = match_flags(res, thrs, kind, n_ways=N_WAYS)
            assert np.array_equal(flags, plain_flags(res, thrs, kind))
            for t, thr in enumerate(thrs):                                   # bit t alone = the flags of thr alone
                one = match_flags(res, (thr,), kind, n_ways=N_WAYS)
                assert np.array_equal(np.where(flags < 0, -1, flags >> t & 1), one)
    with pytest.raises(ValueError):
        match_flags(images[0], np.linspace(0.1, 0.9, 17), 'bbox')
    with pytest.raises(ValueError):
        match_flags(images[0], (), 'bbox')


@pytest.mark.parametrize('name', sorted(crafted()))
def test_match_flags_crafted(name):
    from fgn_amd.fsiseg_eval import match_flags
    res, thrs, max_dets, want = crafted()[name]
    for kind in TYPES:
        flags = match_flags(res, thrs, kind, max_dets, n_ways=N_WAYS)
        assert np.array_equal(flags, plain_flags(res, thrs, kind, max_dets)), kind
        assert flags.tolist() == list(want[kind]), kind
    if name == 'beyond_max_dets':
        assert (flags == -1).sum() == 30
        few = match_flags(res, thrs, 'bbox', 10, n_ways=N_WAYS)
        assert (few == -1).sum() == 120 and np.array_equal(few, plain_flags(res, thrs, 'bbox', 10))


def _with_flags(res, thrs, max_dets=100):
    from fgn_amd.fsiseg_eval import gt_per_cat, match_flags
    r = dict(res)
    for kind in TYPES:
        r['dt_match_' + kind] = match_flags(res, thrs, kind, max_dets, n_ways=N_WAYS)
    r['eval_iou_thrs'] = np.asarray(thrs, np.float64)
    r['gt_per_cat'] = gt_per_cat(res['qry_cat_ids'], N_WAYS)
    return r


def _raiser(name):
    def f(*a, **k):
        raise AssertionError(f'{name} was called')
    return f


def _run(results, kind, thr):
    from fgn_amd.fsiseg_eval import FSISEGEval
    ev = FSISEGEval(results=results, n_ways=N_WAYS, iou_type=kind, iou_thr=thr)
    out = ev.run()
    return ev.eval['precision'], ev.eval['recall'], out


def test_evaluator_reads_the_flags_and_returns_the_same(images, monkeypatch):
    from fgn_amd import fsiseg_eval as fe, rle
    thrs = THR_SETS[10]
    plain_res = images[:80] + [c[0] for c in crafted().values()]
    flagged = [_with_flags(r, thrs) for r in plain_res]
    assert all(np.array_equal(f['gt_per_cat'], np.bincount(r['qry_cat_ids'], minlength=N_WAYS)[:N_WAYS])
               for f, r in zip(flagged, plain_res))
    plain = {(k, t): _run(plain_res, k, t) for k in TYPES for t in thrs + (0.3,)}
    multi_plain = fe.evaluate_results_multi(plain_res, N_WAYS, thrs)
    with monkeypatch.context() as mp:
        for name in ('_mask_iou', '_count_iou', '_bbox_iou'):
            mp.setattr(fe, name, _raiser(name))
        mp.setattr(rle, 'decode', _raiser('rle.decode'))
        for kind in TYPES:
            for thr in thrs:
                p, r, out = _run(flagged, kind, thr)
                assert p.tobytes() == plain[kind, thr][0].tobytes() and r.tobytes() == plain[kind, thr][1].tobytes()
                assert out == plain[kind, thr][2]
        # the ground-truth labels may be absent: the instance counts then come from gt_per_cat
        bare = [{k: v for k, v in f.items() if k not in ('qry_cat_ids', 'qry_bboxes')} for f in flagged]
        p, r, _ = _run(bare, 'segm', thrs[3])
        assert p.tobytes() == plain['segm', thrs[3]][0].tobytes() and r.tobytes() == plain['segm', thrs[3]][1].tobytes()
        assert fe.evaluate_results_multi(flagged, N_WAYS, thrs) == multi_plain
        assert fe.evaluate_results(flagged, N_WAYS, iou_thr=thrs[0]) == \
            {k: multi_plain[k if 'mAP' in k else k + '50'] for k in ('bbox_mAP50', 'bbox_mAR', 'segm_mAP50', 'segm_mAR')}
        with pytest.raises(AssertionError, match='was called'):             # a threshold not in the list: the plain path
            _run(flagged, 'bbox', 0.3)
        with pytest.raises(AssertionError, match='was called'):             # another max_dets than the flags were made with
            ev = fe.FSISEGEval(results=flagged, n_ways=N_WAYS, iou_type='bbox', iou_thr=thrs[0])
            ev.max_dets = 10
            ev.run()
    for kind in TYPES:                                                          # ... which returns what it always did
        p, r, out = _run(flagged, kind, 0.3)
        assert p.tobytes() == plain[kind, 0.3][0].tobytes() and r.tobytes() == plain[kind, 0.3][1].tobytes()
    assert set(multi_plain) == {f'{k}_{m}{s}' for k in TYPES for m in ('mAP', 'mAR')
                                for s in [''] + [str(int(round(t * 100))) for t in thrs]}
    assert multi_plain['segm_mAP'] == float(np.mean([multi_plain[f'segm_mAP{int(round(t * 100))}'] for t in thrs]))
    assert 0 < multi_plain['bbox_mAP'] < 1


def test_minimal_dicts_refuse_annotations():
    from fgn_amd.fsiseg_eval import FSISEGEval
    f = _with_flags(random_res(0), (0.5,))
    bare = {k: f[k] for k in ('dt_scores', 'dt_cat_ids', 'dt_match_bbox', 'dt_match_segm', 'eval_iou_thrs', 'gt_per_cat')}
    ev = FSISEGEval(results=[bare], n_ways=N_WAYS)
    assert set(ev.run()) == {'mAP', 'mAR'}
    with pytest.raises(ValueError, match='minimal'):
        ev.annotations()
    with pytest.raises(ValueError, match='minimal'):
        ev.groups()


# ---- world-2 gloo round trip --------------------------------------------------------------------------------------
MAX_DET, N_EPISODES, GLOO_THRS = 40, 5, (0.5, 0.75)


def _episode(e):
    """(full result dict with flags, the per-image dict ``detect_device`` would hold for it - CPU tensors)"""
    res = _with_flags(random_res(100 + e, d=7 * e + 3, g=4 + e), GLOO_THRS)
    n = len(res['dt_scores'])
    det = torch.zeros(MAX_DET, 5)
    det[:n, 4] = torch.from_numpy(res['dt_scores'])
    det[n:, 4] = 7.0                                           # rows beyond the count hold anything
    lab = torch.full((MAX_DET,), 2, dtype=torch.int64)
    lab[:n] = torch.from_numpy(res['dt_cat_ids'])
    match = torch.full((2, MAX_DET), 5, dtype=torch.int32)
    match[0, :n] = torch.from_numpy(res['dt_match_bbox'])
    match[1, :n] = torch.from_numpy(res['dt_match_segm'])
    return res, dict(det_bboxes=det, det_labels=lab, n_dets=torch.tensor([n], dtype=torch.int32), match=match,
                     gt_per_cat=torch.from_numpy(res['gt_per_cat']))


def _match_worker(rank, world, port, q):
    import torch.distributed as dist
    from fgn_amd import dist as fd
    from fgn_amd.fsiseg_eval import FSISEGEval
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    try:
        mine = fd.shard_episodes(N_EPISODES, rank, world)                 # world 2: ranks hold 3 and 2 episodes
        per = fd.episodes_per_rank(N_EPISODES, world)
        recs, head = fd.pack_matches([_episode(e)[1] for e in mine], MAX_DET, N_WAYS, pad_to=per)
        assert recs.shape == (per, MAX_DET, 4) and head.shape == (per, 1 + N_WAYS)
        calls = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, msg, *a, **k: (calls.append(tuple(msg.shape)), real(out, msg, *a, **k))[1]
        try:
            g_recs, g_head = fd.gather_matches(recs, head)
        finally:
            dist.all_gather_into_tensor = real
        res = fd.results_from_matches(fd.interleave(g_recs)[:N_EPISODES], fd.interleave(g_head)[:N_EPISODES], GLOO_THRS)
        evals = {(k, t): (lambda ev: (ev.run(), ev.eval['precision'].tobytes(), ev.eval['recall'].tobytes()))(
            FSISEGEval(results=res, n_ways=N_WAYS, iou_type=k, iou_thr=t)) for k in TYPES for t in GLOO_THRS}
        q.put((rank, mine, calls, [sorted(r) for r in res], evals))
    finally:
        dist.destroy_process_group()


def test_match_gather_world2_gloo():
    import torch.multiprocessing as mp
    from fgn_amd.fsiseg_eval import FSISEGEval
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29700 + os.getpid() % 1000
    procs = [ctx.Process(target=_match_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out[0][1] == [0, 2, 4] and out[1][1] == [1, 3]                 # unequal episode counts
    full = [{k: v for k, v in _episode(e)[0].items() if not k.startswith('dt_match') and k != 'eval_iou_thrs'
             and k != 'gt_per_cat'} for e in range(N_EPISODES)]          # the full dicts, matched on the host
    positive = []
    for kind in TYPES:
        for thr in GLOO_THRS:
            ev = FSISEGEval(results=full, n_ways=N_WAYS, iou_type=kind, iou_thr=thr)
            want = (ev.run(), ev.eval['precision'].tobytes(), ev.eval['recall'].tobytes())
            positive.append(want[0]['mAP'] > 0)
            for r in out:
                assert r[4][kind, thr] == want
    assert any(positive)                                                  # (the episodes do match something)
    per = (N_EPISODES + 1) // 2
    for r in out:
        # ONE collective for the step, and at most max_det * 4 + 1 + n_ways numbers per episode
        assert r[2] == [(per, MAX_DET * 4 + 1 + N_WAYS)]
        assert all(keys == sorted(['dt_scores', 'dt_cat_ids', 'dt_match_bbox', 'dt_match_segm', 'eval_iou_thrs',
                                   'gt_per_cat']) for keys in r[3])
