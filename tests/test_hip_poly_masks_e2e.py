"""Ground-truth and support masks given as COCO polygons through the detector and the trainer against
the SAME call with ``polygon.dense`` of the same vertices given dense - every result key, loss and trained tensor byte for
byte: at network size, with ``qry_resize_to``, with ``results_at_source``, dense, RLE and polygon entries mixed in a
batch, eager and under a replayed graph, supports rasterised straight into their rows, and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import polygon, rle
from fgn_amd.episodes import collate, star_polygon

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
NK = N_WAYS * K_SHOTS
QRY_SIZES = [(150, 131), (141, 160)]
QRY_GEO = np.array([[1, 0., 1., 0., 0., 0., 0, 0], [0, 10., 1., 0., 0., 0., 1, 4]], np.float64)


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _query(sample: dict, size, resize: bool, seed: int, empty: bool = False) -> dict:
    """The top-left (h, w) window of a pool sample as the query, its instances replaced by polygons in their boxes - one
    of them of two overlapping parts, one leaving the image: ``qry_polygons`` holds them, ``qry_isegmaps`` is
    ``polygon.dense`` of them (``empty``: with none of its instances)."""
    h, w = size
    rng = np.random.RandomState(seed)
    boxes = np.asarray(sample['qry_bboxes'], np.float32).copy()
    boxes[:, [0, 2]] = boxes[:, [0, 2]].clip(0, h)
    boxes[:, [1, 3]] = boxes[:, [1, 3]].clip(0, w)
    keep = (boxes[:, 2] - boxes[:, 0] >= 6) & (boxes[:, 3] - boxes[:, 1] >= 6)
    assert keep.any()
    if empty:
        keep[:] = False
    insts = []
    for j, (y0, x0, y1, x1) in enumerate(boxes[keep]):
        parts = [star_polygon(rng, y0, x0, y1, x1)]
        if j == 0:
            parts.append(star_polygon(rng, y0 + 2, x0 + 2, y1 + 3, x1 + 9))         # overlaps the first; may leave the image
        insts.append(parts)
    masks = np.stack([polygon.dense(p, h, w) for p in insts]).astype(bool) if insts else np.zeros((0, h, w), bool)
    assert all(m.any() for m in masks)
    out = dict(sample)
    out.update(qry_img=sample['qry_img'][:h, :w].contiguous(), qry_isegmaps=masks, qry_polygons=insts,
               qry_bboxes=boxes[keep], qry_cat_ids=np.asarray(sample['qry_cat_ids'])[keep],
               qry_cat_ids_real=np.asarray(sample['qry_cat_ids_real'])[keep], img_shape=np.array([NET, NET, 3], np.int32))
    if resize:
        out['qry_resize_to'] = np.array([NET, NET], np.int32)
    return out


def _poly_supports(sample: dict, seed: int) -> dict:
    """The supports' source images with every instance's mask replaced by a polygon in its box (``spp_polygons``: the
    parts of each), ``spp_isegmaps`` dense of the same vertices in the image's frame."""
    rng = np.random.RandomState(seed)
    parts, masks = [], []
    for im, bb in zip(sample['spp_imgs'], sample['spp_bboxes']):
        p = [star_polygon(rng, *[float(v) for v in bb])]
        parts.append(p)
        masks.append(polygon.dense(p, *im.shape[:2]).astype(bool))
        assert masks[-1].any()
    return dict(sample, spp_isegmaps=masks, spp_polygons=parts)


def _ready_supports(sample: dict) -> dict:
    """Ready S x S supports for the plain path (dense support tensor, no ``spp_crop_to``)."""
    keys = ('spp_crop_to', 'spp_fill_ratio', 'crop_square', 'spp_augment', 'spp_photometric')
    made = [fd.support_from_source(im.numpy(), bb, mk, sample['spp_crop_to'], sample['spp_fill_ratio'], sample['crop_square'])
            for im, mk, bb in zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])]
    out = {k: v for k, v in sample.items() if k not in keys}
    out.update(spp_imgs=torch.from_numpy(np.stack([c for c, _, _ in made])), spp_bboxes=np.stack([b for _, b, _ in made]),
               spp_isegmaps=np.stack([m for _, _, m in made]))
    return out


def _batch(samples: list) -> tuple:
    """-> (the dense batch, per image the polygon entry, per support set the polygon instances or None)."""
    qp = [{'polygons': s['qry_polygons']} for s in samples]
    sp = [s.get('spp_polygons') for s in samples]
    samples = [{k: v for k, v in s.items() if k not in ('qry_polygons', 'spp_polygons')} for s in samples]
    if len({tuple(s['qry_img'].shape) for s in samples}) > 1:                       # (images of two sizes: a list)
        imgs = [s['qry_img'] for s in samples]
        b = collate([{k: v for k, v in s.items() if k != 'qry_img'} for s in samples])
        b['qry_img'] = imgs
    else:
        b = collate(samples)
    return b, qp, sp


def _as_poly(batch, qp, sp=None, qry=(), spp: bool = False, form=None) -> dict:
    """``batch`` with the ground truth of the images ``qry`` (and, ``spp``, every support mask) given as polygons;
    ``form`` maps an image to another form of its entry: 'rle' (COCO RLE dicts), 'carrier' (a ``PolyMasks``), 'sized' (the
    dict with its ``size``)."""
    form = form or {}
    out = dict(batch)
    ents = []
    for i, g in enumerate(batch['qry_isegmaps']):
        hw = tuple(int(v) for v in g.shape[1:])
        if form.get(i) == 'rle':
            g = rle.encode_many(np.asarray(g))
        elif i in qry:
            g = dict(qp[i])
            if form.get(i) == 'sized':
                g['size'] = list(hw)
            elif form.get(i) == 'carrier':
                g = polygon.as_polys(g, hw)
        ents.append(g)
    out['qry_isegmaps'] = ents
    if spp:
        out['spp_isegmaps'] = [[{'polygons': p} for p in lst] for lst in sp]
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


@contextlib.contextmanager
def _rasterised_on_the_device():
    """Counts the polygon launches through ``ops`` (the instances of each) while it is entered."""
    from fgn_amd import ops
    calls, real = [], ops._poly_launch
    ops._poly_launch = lambda *a, **k: calls.append(len(a[0])) or real(*a, **k)
    try:
        yield calls
    finally:
        ops._poly_launch = real


@pytest.mark.parametrize('frame', ('network', 'resize', 'source'))
def test_simple_test_with_polygon_ground_truth_is_the_dense_call(ds, model, frame):
    """Two images, the second without an instance; every key, the RLE strings, overlap and match keys included.  All
    entries polygons, then dense, RLE and polygon entries mixed, then the same under a graph that is replayed."""
    m = _reset(model, ds)
    m.match_on_device = m.evaluate_on_device = True
    resize = frame != 'network'
    samples = [_ready_supports(_query(ds[0], QRY_SIZES[0] if resize else (NET, NET), resize, 1)),
               _ready_supports(_query(ds[1], QRY_SIZES[1] if resize else (NET, NET), resize, 2, empty=True))]
    dense, qp, _ = _batch(samples)
    kw = dict(rescale=True, results_at_source=frame == 'source')
    want = m.simple_test(**dense, **kw)
    assert all(k in want[0] for k in ('dt_gt_inter', 'dt_area', 'gt_area', 'dt_match_bbox', 'dt_match_segm'))
    assert len(want[0]['qry_isegmaps_rle']) > 0 and want[1]['qry_isegmaps_rle'] == []
    with _rasterised_on_the_device() as calls:
        _same_results(want, m.simple_test(**_as_poly(dense, qp, qry=(0, 1)), **kw))
    assert calls == [len(want[0]['qry_isegmaps_rle'])]                     # one call for the image that has masks
    _same_results(want, m.simple_test(**_as_poly(dense, qp, qry=(0,), form={0: 'carrier'}), **kw))   # mixed: polygons, dense
    _same_results(want, m.simple_test(**_as_poly(dense, qp, qry=(1,), form={0: 'rle', 1: 'sized'}), **kw))   # RLE, polygons (none)
    m.use_graphs = True
    for rep in range(3):                                                  # captured, then replayed with polygons
        _same_results(want, m.simple_test(**_as_poly(dense, qp, qry=(0, 1)), **kw))
    m.use_graphs = False


def _three_forms(ds):
    """One batch of three images whose ground truth comes dense, as RLE and as polygons."""
    samples = [_ready_supports(_query(ds[i], (NET, NET), False, 10 + i)) for i in range(3)]
    dense, qp, _ = _batch(samples)
    return dense, _as_poly(dense, qp, qry=(2,), form={1: 'rle'})


def test_one_batch_mixes_dense_rle_and_polygon_entries(ds, model):
    m = _reset(model, ds)
    dense, mixed = _three_forms(ds)
    assert isinstance(mixed['qry_isegmaps'][0], torch.Tensor) and rle.is_rle(mixed['qry_isegmaps'][1]) and \
        polygon.is_poly(mixed['qry_isegmaps'][2])
    _same_results(m.simple_test(**dense, rescale=True), m.simple_test(**mixed, rescale=True))


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
    """(dense batch, the same batch with polygon masks) of two episodes for one training form."""
    if kind == 'plain':                             # network-size query, ready supports (dense tensor, stays dense)
        dense, qp, _ = _batch([_ready_supports(_query(ds[i], (NET, NET), False, 20 + i)) for i in range(2)])
        return dense, _as_poly(dense, qp, qry=(0, 1))
    if kind == 'qry_augment':                       # source-size queries of two sizes, warped with their masks
        dense, qp, _ = _batch([dict(_ready_supports(_query(ds[i], QRY_SIZES[i], True, 30 + i)), qry_augment=QRY_GEO[i])
                               for i in range(2)])
        return dense, _as_poly(dense, qp, qry=(0, 1), form={1: 'sized'})
    dense, qp, sp = _batch([_poly_supports(_query(ds[i], (NET, NET), False, 40 + i), 50 + i) for i in range(2)])
    return dense, _as_poly(dense, qp, sp, qry=(1,), spp=True)     # source supports as polygons; mixed query


@pytest.mark.parametrize('kind', ('plain', 'qry_augment', 'spp_source'))
def test_forward_train_losses_are_bit_equal_to_dense(ds, model, kind):
    m = _reset(model, ds)
    dense, polys = _train_batches(ds, kind)
    with _rasterised_on_the_device() as calls:
        got = _losses(m, polys)
    assert len(calls) >= 1
    _same_losses(_losses(m, dense), got)


def _steps(batches, ds, seed=5):
    from fgn_amd.train import Trainer
    m = _model()
    m.set_input_norm(**ds.input_norm)
    tr = Trainer(m)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    losses = [tr.step(b, perm_fn=lambda n: torch.randperm(n, generator=g)) for b in batches]
    torch.cuda.synchronize()
    tensors = {f'{part}/{k}': v.detach().cpu() for part, d in (('W', tr.W), ('state', tr.state), ('bn', tr.buffers))
               for k, v in d.items()}
    assert tr.n_steps == len(batches)
    return losses, tensors


def test_two_trainer_steps_leave_equal_weights(ds):
    first, second = _train_batches(ds, 'spp_source'), _train_batches(ds, 'plain')
    a, b = _steps([first[0], second[0]], ds), _steps([first[1], second[1]], ds)
    for x, y in zip(a[0], b[0]):
        _same_losses(x, y)
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].dtype == b[1][k].dtype and torch.equal(a[1][k].view(torch.uint8), b[1][k].view(torch.uint8)), k


def test_polygon_supports_are_the_dense_supports_eager_and_under_one_graph(ds, model):
    m = _reset(model, ds)
    sets = [_batch([_poly_supports(_query(ds[2 + i], (NET, NET), False, 60 + i), 70 + i)]) for i in range(2)]
    want = [m.simple_test(**b, rescale=True) for b, _, _ in sets]
    polys = [_as_poly(b, qp, sp, qry=(0,), spp=True) for b, qp, sp in sets]
    # the rows of spp_msk, byte for byte, and no mask byte uploaded
    dev = torch.device('cuda', torch.cuda.current_device())
    for (b, _, _), p in zip(sets, polys):
        sd = m._source_supports(b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], SPP)
        sq = m._source_supports(p['spp_imgs'], p['spp_bboxes'], p['spp_isegmaps'], SPP)
        assert all(f.numel() == 0 for f in sq['mflats']) and len(sq['mpoly']) == NK and not sq['mrle']
        assert sq['window_bytes'] < sd['window_bytes']
        a, c = m._upload_supports(sd, dev)['spp_msk'], m._upload_supports(sq, dev)['spp_msk']
        torch.cuda.synchronize()
        for i in range(NK):
            n = sd['mflats'][i].numel()
            assert n > 0 and torch.equal(a[i, :n].cpu(), sd['mflats'][i]) and torch.equal(c[i, :n].cpu(), sd['mflats'][i]), i
    with _rasterised_on_the_device() as calls:
        _same_results(want[0], m.simple_test(**polys[0], rescale=True))
    assert sorted(calls) == sorted([NK, len(want[0][0]['qry_isegmaps_rle'])])     # one call for the N*K windows
    b1, p1 = sets[1][0], polys[1]
    mixed = dict(p1, spp_isegmaps=[[a if i % 3 == 0 else rle.encode(np.asarray(a)) if i % 3 == 1 else c for i, (a, c) in
                                    enumerate(zip(b1['spp_isegmaps'][0], p1['spp_isegmaps'][0]))]])
    _same_results(want[1], m.simple_test(**mixed, rescale=True))                  # dense, RLE and polygon instances in one set
    m.use_graphs = True
    before = set(m._graphs)
    for rep in range(2):
        for w, p in zip(want, polys):
            _same_results(w, m.simple_test(**p, rescale=True))
    new = [k for k in m._graphs if k not in before]
    assert len(new) == 1                            # one graph for both support sets
    ge = m._graphs[new[0]]
    sd = m._source_supports(b1['spp_imgs'], b1['spp_bboxes'], b1['spp_isegmaps'], SPP, graphed=True)
    torch.cuda.synchronize()
    for i in range(NK):                             # the static mask slot holds the rasterised windows of the last set
        assert torch.equal(ge.static['spp_msk'][i, :sd['mflats'][i].numel()].cpu(), sd['mflats'][i]), i
    m.use_graphs = False
    a, p = sets[0][0], polys[0]
    want_code = m.encode_supports(a['spp_imgs'], a['spp_bboxes'], a['spp_isegmaps'], spp_crop_to=SPP)
    code = m.encode_supports(p['spp_imgs'], p['spp_bboxes'], p['spp_isegmaps'], spp_crop_to=SPP)
    for k in ('vec', 'S', 'cat_mean_mp', 'spp_masks', 'spp_xyxy'):
        assert torch.equal(code[k].contiguous().view(torch.uint8), want_code[k].contiguous().view(torch.uint8)), k


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
    b, qp, sp = _batch([_poly_supports(_query(ds[0], (NET, NET), False, 80), 81)])
    net = _as_poly(b, qp, sp, qry=(0,), spp=True)
    bs, qs, _ = _batch([_poly_supports(_query(ds[0], QRY_SIZES[0], True, 82), 83)])
    src = _as_poly(bs, qs, qry=(0,))
    rb, rq, _ = _batch([_ready_supports(_query(ds[0], (NET, NET), False, 84))])
    ready = _as_poly(rb, rq, qry=(0,))

    def qry(batch, fn):
        e = {k: [list(p) for p in v] if k == 'polygons' else v for k, v in batch['qry_isegmaps'][0].items()}
        fn(e)
        return dict(batch, qry_isegmaps=[e])

    def spp(batch, i, parts):
        items = list(batch['spp_isegmaps'][0])
        items[i] = {'polygons': parts}
        return dict(batch, spp_isegmaps=[items])
    tri = [1.0, 1.0, 30.0, 2.0, 5.0, 40.0]
    bad = [
        (dict(ready, spp_isegmaps=net['spp_isegmaps']), 'dense'),                           # the plain path is dense only
        (dict(ready, spp_isegmaps=net['spp_isegmaps'][0][0]), 'dense'),
        (dict(net, qry_isegmaps=[qp[0]['polygons']]), 'never as bare lists'),               # a bare nested list
        (dict(net, qry_isegmaps=[[[tri]]]), 'never as bare lists'),
        (qry(net, lambda e: e.update(size=[NET, NET + 1])), 'qry_isegmaps[0]'),             # not the network size
        (qry(src, lambda e: e.update(size=[NET, NET])), 'qry_isegmaps[0]'),                 # not its image's source size
        (qry(net, lambda e: e['polygons'][0].append([1.0, 2.0, 3.0, 4.0])), 'instance 0, part 2'),
        (qry(net, lambda e: e['polygons'].append([])), 'has no part'),
        (qry(net, lambda e: e['polygons'][0].__setitem__(0, [1.0, 2.0, float('nan'), 4.0, 5.0, 6.0])), 'not finite'),
        (qry(net, lambda e: e['polygons'][0].__setitem__(0, [1.0, 2.0, 1e6, 4.0, 5.0, 6.0])), '65536'),
        (spp(net, 2, []), 'spp_isegmaps[2]'),
        (spp(net, 1, [tri, [1.0, 2.0, 3.0]]), 'spp_isegmaps[1]'),
    ]
    for batch, word in bad:
        for graphs in (False, True):
            m.use_graphs = graphs
            with _refused_before_anything_is_queued(m) as err:
                m.simple_test(**batch, rescale=True)
            assert word in str(err.value), str(err.value)
        m.use_graphs = False
        with _refused_before_anything_is_queued(m) as err:
            m.detect_device(batch['qry_img'], batch['spp_imgs'], batch['spp_bboxes'], batch['spp_isegmaps'],
                            batch['img_shape'], qry_isegmaps=batch['qry_isegmaps'], spp_crop_to=batch.get('spp_crop_to'),
                            qry_resize_to=batch.get('qry_resize_to'))
        assert word in str(err.value), str(err.value)
        with _refused_before_anything_is_queued(m) as err:
            m.forward_train(**batch)
        assert word in str(err.value), str(err.value)
    with _refused_before_anything_is_queued(m):
        m.encode_supports(ready['spp_imgs'], ready['spp_bboxes'], net['spp_isegmaps'])
    with _refused_before_anything_is_queued(m):
        m.encode_supports(net['spp_imgs'], net['spp_bboxes'], spp(net, 0, [])['spp_isegmaps'], spp_crop_to=SPP)
