"""Ground-truth and support masks given as COCO RLE through the detector and the trainer against the
SAME call with the masks given dense - every result key, loss and trained tensor byte for byte: at network size, with
``qry_resize_to``, with ``results_at_source``, dense and RLE entries mixed in a batch, an image without instances, eager
and under graphs, supports under one graph for sets of differing source sizes, and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import rle
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
NK = N_WAYS * K_SHOTS
QRY_SIZES = [(150, 131), (141, 160)]
SPP_KEYS = ('spp_crop_to', 'spp_fill_ratio', 'crop_square', 'spp_augment', 'spp_photometric')


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return [flip, rotate, scale, shear, tx, ty, border, order]


GEO = np.array([[row(flip=1), row(rotate=10, border=1, order=4), row()] * 2,
                [row(tx=7, ty=-5), row(scale=1.2), row(shear=-10, border=1)] * 2], np.float64)
QRY_GEO = np.array([row(flip=1), row(rotate=10, border=1, order=4)], np.float64)


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _query(sample: dict, size, resize: bool, empty: bool = False) -> dict:
    """The top-left (h, w) window of a pool sample as the query (``empty``: with none of its instances)."""
    h, w = size
    masks = np.asarray(sample['qry_isegmaps'])[:, :h, :w]
    boxes = np.asarray(sample['qry_bboxes'], np.float32).copy()
    boxes[:, [0, 2]] = boxes[:, [0, 2]].clip(0, h)
    boxes[:, [1, 3]] = boxes[:, [1, 3]].clip(0, w)
    keep = masks.any((1, 2)) & (boxes[:, 2] - boxes[:, 0] >= 2) & (boxes[:, 3] - boxes[:, 1] >= 2)
    assert keep.any()
    if empty:
        keep[:] = False
    out = dict(sample)
    out.update(qry_img=sample['qry_img'][:h, :w].contiguous(), qry_isegmaps=np.ascontiguousarray(masks[keep]),
               qry_bboxes=boxes[keep], qry_cat_ids=np.asarray(sample['qry_cat_ids'])[keep],
               qry_cat_ids_real=np.asarray(sample['qry_cat_ids_real'])[keep], img_shape=np.array([NET, NET, 3], np.int32))
    if resize:
        out['qry_resize_to'] = np.array([NET, NET], np.int32)
    return out


def _cut(sample: dict, k: int) -> dict:
    """The supports' source images cut to windows around their instances, margins chosen by (instance, ``k``)."""
    imgs, masks, boxes = [], [], []
    for i, (im, mk, bb) in enumerate(zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])):
        H, W = im.shape[:2]
        a, b = 1 + 5 * ((i + k) % 4), 2 + 7 * ((i + 2 * k) % 3)
        t, l = max(0, int(bb[0]) - a), max(0, int(bb[1]) - b)
        bt, r = min(H, int(np.ceil(bb[2])) + b), min(W, int(np.ceil(bb[3])) + a)
        imgs.append(im[t:bt, l:r].contiguous())
        masks.append(np.ascontiguousarray(mk[t:bt, l:r]))
        boxes.append(np.asarray(bb, np.float32) - np.array([t, l, t, l], np.float32))
    return dict(sample, spp_imgs=imgs, spp_isegmaps=masks, spp_bboxes=np.stack(boxes))


def _ready_supports(sample: dict) -> dict:
    """Ready S x S supports for the plain path (dense support tensor, no ``spp_crop_to``)."""
    made = [fd.support_from_source(im.numpy(), bb, mk, sample['spp_crop_to'], sample['spp_fill_ratio'], sample['crop_square'])
            for im, mk, bb in zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])]
    out = {k: v for k, v in sample.items() if k not in SPP_KEYS}
    out.update(spp_imgs=torch.from_numpy(np.stack([c for c, _, _ in made])), spp_bboxes=np.stack([b for _, b, _ in made]),
               spp_isegmaps=np.stack([m for _, _, m in made]))
    return out


def _batch(samples: list) -> dict:
    if len({tuple(s['qry_img'].shape) for s in samples}) > 1:                       # (images of two sizes: a list)
        imgs = [s['qry_img'] for s in samples]
        b = collate([{k: v for k, v in s.items() if k != 'qry_img'} for s in samples])
        b['qry_img'] = imgs
        return b
    return collate(samples)


def _as_rle(batch: dict, qry=(), spp: bool = False, form: str = 'dict') -> dict:
    """``batch`` with the ground truth of the images ``qry`` (and, ``spp``, every support mask) given as COCO RLE:
    pycocotools dicts, or the reference's ``[size, counts]`` pairs with an ``np.int16`` size."""
    def item(m):
        e = rle.encode(np.asarray(m))
        return e if form == 'dict' else [np.array(e['size'], np.int16), e['counts']]
    out = dict(batch)
    out['qry_isegmaps'] = [[item(m) for m in np.asarray(g)] if i in qry else g for i, g in enumerate(batch['qry_isegmaps'])]
    if spp:
        out['spp_isegmaps'] = [[item(m) for m in lst] for lst in batch['spp_isegmaps']]
    return out


@pytest.fixture(scope='module')
def ds():
    return fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                        spp_img_size=SPP, raw_uint8=True, spp_source=True)


@pytest.fixture(scope='module')
def model(ds):
    return _model()


def _reset(m, ds):
    m.use_graphs = False
    m.transfer_mode = 0
    m.match_on_device = m.evaluate_on_device = False
    m.query_source_capacity = 3 * POOL * POOL
    m.support_source_capacity = 3 * POOL * POOL
    m.set_input_norm(**ds.input_norm)
    return m


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


def _decoded_on_the_device():
    """Counts the decode launches through ``ops`` while it is entered."""
    from fgn_amd import ops

    @contextlib.contextmanager
    def counted():
        calls, real = [], ops._rle_decode
        ops._rle_decode = lambda *a, **k: calls.append(a[1].shape[0]) or real(*a, **k)
        try:
            yield calls
        finally:
            ops._rle_decode = real
    return counted()


@pytest.mark.parametrize('graphs', (False, True), ids=('eager', 'graphs'))
@pytest.mark.parametrize('frame', ('network', 'resize', 'source'))
def test_simple_test_with_rle_ground_truth_is_the_dense_call(ds, model, frame, graphs):
    """Two images, the second without an instance; every key, overlap and match keys included.  All entries RLE, then
    a dense and an RLE entry mixed."""
    m = _reset(model, ds)
    m.match_on_device = m.evaluate_on_device = True
    resize = frame != 'network'
    samples = [_query(ds[0], QRY_SIZES[0] if resize else (NET, NET), resize),
               _query(ds[1], QRY_SIZES[1] if resize else (NET, NET), resize, empty=True)]
    dense = _batch(samples)
    kw = dict(rescale=True, results_at_source=frame == 'source')
    want = m.simple_test(**dense, **kw)
    assert all(k in want[0] for k in ('dt_gt_inter', 'dt_area', 'gt_area', 'dt_match_bbox', 'dt_match_segm'))
    assert len(want[0]['qry_isegmaps_rle']) > 0 and want[1]['qry_isegmaps_rle'] == []
    m.use_graphs = graphs
    with _decoded_on_the_device() as calls:
        _same_results(want, m.simple_test(**_as_rle(dense, qry=(0, 1)), **kw))
    assert calls == [len(want[0]['qry_isegmaps_rle'])]                     # one launch per image that has masks
    _same_results(want, m.simple_test(**_as_rle(dense, qry=(0,), form='pair'), **kw))       # mixed: RLE, dense
    _same_results(want, m.simple_test(**_as_rle(dense, qry=(1,)), **kw))                    # mixed: dense, the empty list
    if frame == 'source':              # canonical input strings come back unchanged, and the input is not mutated
        given = _as_rle(dense, qry=(0,))
        strings = [dict(it) for it in given['qry_isegmaps'][0]]
        got = m.simple_test(**given, **kw)
        assert got[0]['qry_isegmaps_rle'] == strings and given['qry_isegmaps'][0] == strings
        assert [tuple(it['size']) for it in strings] == [QRY_SIZES[0]] * len(strings)


@pytest.mark.parametrize('resize', (False, True), ids=('network', 'resize'))
def test_pack_results_host_fallback_decodes_rle(ds, model, resize):
    """Where no device string exists for the ground truth (here: ``detect_device`` was not given the masks; the same
    ``host_mask`` serves a device RLE that overflowed), ``pack_results`` decodes RLE entries on the host
    (``RleMasks.dense()``) and resizes them as it resizes dense ones."""
    m = _reset(model, ds)
    dense = _batch([_ready_supports(_query(ds[i], QRY_SIZES[i] if resize else (NET, NET), resize)) for i in range(2)])
    runs = _as_rle(dense, qry=(0,), form='pair')                           # one RLE entry, one dense
    kw = dict(qry_resize_to=dense['qry_resize_to']) if resize else {}
    out = []
    for b in (dense, runs, _as_rle(dense, qry=(0, 1))):
        dets = m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'], **kw)
        assert all('gt_slice' not in d for d in dets)
        out.append(m.pack_results(dets, 2, qry_isegmaps=b['qry_isegmaps'], img_shape=b['img_shape'],
                                  qry_resize_to=(NET, NET) if resize else None))
    for got in out[1:]:
        for a, g in zip(out[0], got):
            assert len(a['qry_isegmaps_rle']) > 0 and a['qry_isegmaps_rle'] == g['qry_isegmaps_rle']
            assert a['qry_isegmaps_rle'][0]['size'] == [NET, NET]
            assert a['dt_isegmaps_rle'] == g['dt_isegmaps_rle'] and a['dt_scores'].tobytes() == g['dt_scores'].tobytes()


def _two_sets(ds, resize=False):
    """Two batches of one episode each, whose support sets have differing source sizes."""
    return [_batch([_cut(_query(ds[2 + i], (NET, NET), resize), i)]) for i in range(2)]


def test_rle_supports_are_the_dense_supports_eager_and_under_one_graph(ds, model):
    m = _reset(model, ds)
    sets = _two_sets(ds)
    sizes = [[tuple(t.shape[:2]) for t in b['spp_imgs'][0]] for b in sets]
    assert sizes[0] != sizes[1] and len(set(sizes[0])) > 1
    want = [m.simple_test(**b, rescale=True) for b in sets]
    runs = [_as_rle(b, qry=(0,), spp=True) for b in sets]
    with _decoded_on_the_device() as calls:
        _same_results(want[0], m.simple_test(**runs[0], rescale=True))
    assert sorted(calls) == sorted([NK, len(want[0][0]['qry_isegmaps_rle'])])     # one launch for the N*K windows
    mixed = dict(runs[1], spp_isegmaps=[[a if i % 2 else b for i, (a, b) in
                                         enumerate(zip(sets[1]['spp_isegmaps'][0], runs[1]['spp_isegmaps'][0]))]])
    _same_results(want[1], m.simple_test(**mixed, rescale=True))                  # dense and RLE instances in one set
    m.use_graphs = True
    before = set(m._graphs)
    for rep in range(2):
        for w, b in zip(want, runs):
            _same_results(w, m.simple_test(**b, rescale=True))
    _same_results(want[1], m.simple_test(**_as_rle(sets[1], spp=True, form='pair'), rescale=True))
    new = [k for k in m._graphs if k not in before]
    assert len(new) == 1                            # one graph for both support sets and both forms
    ge = m._graphs[new[0]]
    assert tuple(ge.static['spp_msk'].shape) == (NK, POOL * POOL)
    # the static mask slot holds the decoded windows of the last set
    sp = m._source_supports(sets[1]['spp_imgs'], sets[1]['spp_bboxes'], sets[1]['spp_isegmaps'], SPP, graphed=True)
    torch.cuda.synchronize()
    for i in range(NK):
        assert torch.equal(ge.static['spp_msk'][i, :sp['mflats'][i].numel()].cpu(), sp['mflats'][i]), i
    m.use_graphs = False
    # the support code
    a, b = sets[0], runs[0]
    want_code = m.encode_supports(a['spp_imgs'], a['spp_bboxes'], a['spp_isegmaps'], spp_crop_to=SPP)
    code = m.encode_supports(b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], spp_crop_to=SPP)
    for k in ('vec', 'S', 'cat_mean_mp', 'spp_masks', 'spp_xyxy'):
        assert torch.equal(code[k].contiguous().view(torch.uint8), want_code[k].contiguous().view(torch.uint8)), k


def _val(v):
    return torch.as_tensor(v[0] if isinstance(v, list) else v).detach().cpu().reshape(-1)


def _same_losses(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = _val(a[k]), _val(b[k])
        assert x.dtype == y.dtype and x.numpy().tobytes() == y.numpy().tobytes(), k
    assert all(np.isfinite(float(_val(v)[0])) for v in a.values())
    assert float(_val(a['loss_rpn_cls'])[0]) > 0 and float(_val(a['loss_mask'])[0]) > 0


def _losses(m, batch, seed=3):
    m._PT = None                                    # fresh running statistics
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    return m.forward_train(**batch, perm_fn=lambda n: torch.randperm(n, generator=g))


def _train_batches(ds, kind):
    """(dense batch, the same batch with RLE masks) of two episodes for one training form."""
    if kind == 'plain':                             # network-size query, ready supports (dense tensor, stays dense)
        dense = _batch([_ready_supports(_query(ds[i], (NET, NET), False)) for i in range(2)])
        return dense, _as_rle(dense, qry=(0, 1))
    if kind == 'qry_augment':                       # source-size queries of two sizes, warped with their masks
        dense = _batch([dict(_ready_supports(_query(ds[i], QRY_SIZES[i], True)), qry_augment=QRY_GEO[i]) for i in range(2)])
        return dense, _as_rle(dense, qry=(0, 1), form='pair')
    dense = _batch([dict(_cut(_query(ds[i], (NET, NET), False), i), spp_augment=GEO[i]) for i in range(2)])
    return dense, _as_rle(dense, qry=(1,), spp=True)          # source supports, augmented behind their cut; mixed query


@pytest.mark.parametrize('kind', ('plain', 'qry_augment', 'spp_augment'))
def test_forward_train_losses_are_bit_equal_to_dense(ds, model, kind):
    m = _reset(model, ds)
    dense, runs = _train_batches(ds, kind)
    with _decoded_on_the_device() as calls:
        got = _losses(m, runs)
    assert len(calls) >= 1
    _same_losses(_losses(m, dense), got)


def _step(batch, ds, seed=5):
    from fgn_amd.train import Trainer
    m = _model()
    m.set_input_norm(**ds.input_norm)
    tr = Trainer(m)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    losses = tr.step(batch, perm_fn=lambda n: torch.randperm(n, generator=g))
    torch.cuda.synchronize()
    tensors = {f'{part}/{k}': v.detach().cpu() for part, d in (('W', tr.W), ('state', tr.state), ('bn', tr.buffers))
               for k, v in d.items()}
    assert tr.n_steps == 1
    return losses, tensors


def test_one_trainer_step_leaves_equal_weights(ds):
    dense, runs = _train_batches(ds, 'spp_augment')
    a, b = _step(dense, ds), _step(runs, ds)
    _same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].dtype == b[1][k].dtype and torch.equal(a[1][k].view(torch.uint8), b[1][k].view(torch.uint8)), k


@contextlib.contextmanager
def _refused_before_anything_is_queued(m):
    """A ValueError inside, raised before the detector uploads, allocates on the device or launches."""
    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_supports', '_supports_on_device', '_support_front', '_detect_eager', '_detect_graphed',
             '_stem_input', '_device_masks')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for n in names:
        setattr(m, n, boom)
    try:
        with pytest.raises(ValueError) as err:
            yield err
    finally:
        for n in names:
            delattr(m, n)
    assert torch.cuda.memory_allocated() == before


def test_contract_errors_queue_nothing(ds, model):
    m = _reset(model, ds)
    net = _as_rle(_batch([_cut(_query(ds[0], (NET, NET), False), 0)]), qry=(0,), spp=True)
    src = _as_rle(_batch([_cut(_query(ds[0], QRY_SIZES[0], True), 0)]), qry=(0,))
    ready = _batch([_ready_supports(_query(ds[0], (NET, NET), False))])

    def qry(b, fn):
        items = [dict(it) for it in b['qry_isegmaps'][0]]
        fn(items)
        return dict(b, qry_isegmaps=[items])

    def spp(b, fn):
        items = [dict(it) for it in b['spp_isegmaps'][0]]
        fn(items)
        return dict(b, spp_isegmaps=[items])
    bad_counts = rle.counts_to_string(np.array([5, NET * NET - 6]))
    bad = [
        (qry(net, lambda it: it[0].update(size=[NET, NET + 1])), 'qry_isegmaps[0]'),       # not the network size
        (qry(src, lambda it: it[0].update(size=[NET, NET])), 'qry_isegmaps[0]'),           # not its image's source size
        (qry(net, lambda it: it[0].update(counts=bad_counts)), 'sum'),                     # everything as_masks refuses
        (qry(net, lambda it: it[0].update(counts=[-1, NET * NET + 1])), 'negative'),
        (qry(net, lambda it: it[0].update(counts=b'')), 'no run'),
        (qry(net, lambda it: it[0].update(size=[0, NET])), 'within'),
        (spp(net, lambda it: it[2].update(size=[POOL, POOL + 1])), 'spp_isegmaps[2]'),      # not its image's size
        (spp(net, lambda it: it[1].update(counts=[3])), 'spp_isegmaps[1]'),
        (dict(ready, spp_isegmaps=net['spp_isegmaps']), 'dense'),                           # the plain path is dense only
    ]
    for b, word in bad:
        for graphs in (False, True):
            m.use_graphs = graphs
            with _refused_before_anything_is_queued(m) as err:
                m.simple_test(**b, rescale=True)
            assert word in str(err.value), str(err.value)
        m.use_graphs = False
        with _refused_before_anything_is_queued(m) as err:
            m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                            qry_isegmaps=b['qry_isegmaps'], spp_crop_to=b.get('spp_crop_to'),
                            qry_resize_to=b.get('qry_resize_to'))
        assert word in str(err.value)
        with _refused_before_anything_is_queued(m) as err:
            m.forward_train(**b)
        assert word in str(err.value)
    with _refused_before_anything_is_queued(m):
        m.encode_supports(ready['spp_imgs'], ready['spp_bboxes'], net['spp_isegmaps'])
    with _refused_before_anything_is_queued(m):
        m.encode_supports(net['spp_imgs'], net['spp_bboxes'],
                          spp(net, lambda it: it[0].update(counts=[1]))['spp_isegmaps'], spp_crop_to=SPP)
