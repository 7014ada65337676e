"""Ground-truth and support masks given as box + colour through the detector and the trainer against
the SAME call with the masks given dense (``ColorMasks.dense`` of the same image bytes) - every result key, loss and
trained tensor byte for byte: at network size, with ``qry_resize_to``, with ``results_at_source``, with the overlaps and
the matching made on the device, dense, RLE and colour entries mixed in a batch, an image without instances, eager and
under graphs with consecutive episodes through the same static slots, ahead of the photometric pass and of the support
cut - and nothing of it in a call without a colour entry."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import colormask as cm
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
SPP_PHOTO = np.array([[(3, 1.5, 0), (4, 50, 0), (0, 0, 0)] * 2, [(1, 2.0, 9), (0, 0, 0), (6, -30, 0)] * 2], np.float64)
QRY_GEO = np.array([row(flip=1), row(rotate=10, border=1, order=4)], np.float64)
QRY_PHOTO = np.array([[4, 50, 0], [6, -40, 0]], np.float64)          # hue, brightness: both move pixels out of the window


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _query(sample: dict, size, resize: bool, empty: bool = False) -> dict:
    """The top-left (h, w) window of a pool sample as the query, its instances as box + colour with the boxes cut to
    the window (``empty``: with none of them)."""
    h, w = size
    g = sample['qry_isegmaps']
    boxes = g.boxes.copy()
    boxes[:, [0, 2]] = boxes[:, [0, 2]].clip(0, h)
    boxes[:, [1, 3]] = boxes[:, [1, 3]].clip(0, w)
    keep = (boxes[:, 2] - boxes[:, 0] >= 2) & (boxes[:, 3] - boxes[:, 1] >= 2)
    assert keep.any()
    if empty:
        keep[:] = False
    out = dict(sample)
    out.update(qry_img=sample['qry_img'][:h, :w].contiguous(),
               qry_isegmaps=cm.as_color_masks({'bboxes': boxes[keep], 'colors': g.colors[keep]}, (h, w)),
               qry_bboxes=boxes[keep].astype(np.float32), qry_cat_ids=np.asarray(sample['qry_cat_ids'])[keep],
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
        masks.append(cm.as_color_masks({'bboxes': mk.boxes - np.array([t, l, t, l], np.int32), 'colors': mk.colors},
                                       (bt - t, r - l)))
        boxes.append(np.asarray(bb, np.float32) - np.array([t, l, t, l], np.float32))
    return dict(sample, spp_imgs=imgs, spp_isegmaps=masks, spp_bboxes=np.stack(boxes))


def _ready_supports(sample: dict) -> dict:
    """Ready S x S supports for the plain path (dense support tensor, no ``spp_crop_to``)."""
    made = [fd.support_from_source(im.numpy(), bb, mk.dense(im)[0], sample['spp_crop_to'], sample['spp_fill_ratio'],
                                   sample['crop_square'])
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


def _dense(batch: dict, qry=None, spp: bool = True, runs=()) -> dict:
    """``batch`` (all masks box + colour) with the ground truth of the images ``qry`` (default: all) given dense - the
    host rule on the same bytes -, of the images ``runs`` as COCO RLE of that, and (``spp``) every colour support mask
    dense."""
    out = dict(batch)
    qry = range(len(batch['qry_isegmaps'])) if qry is None else qry
    out['qry_isegmaps'] = [g.dense(batch['qry_img'][i]) if i in qry or i in runs else g
                           for i, g in enumerate(batch['qry_isegmaps'])]
    out['qry_isegmaps'] = [rle.encode_many(g) if i in runs else g for i, g in enumerate(out['qry_isegmaps'])]
    if spp and isinstance(batch['spp_isegmaps'], list):
        out['spp_isegmaps'] = [[mk.dense(im)[0] if cm.is_color(mk) else mk for im, mk in zip(ims, mks)]
                               for ims, mks in zip(batch['spp_imgs'], batch['spp_isegmaps'])]
    return out


@pytest.fixture(scope='module')
def ds():
    return fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                        spp_img_size=SPP, raw_uint8=True, spp_source=True, color_masks=True)


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
def _made_on_the_device():
    """Counts the calls into the two new ``ops`` functions while it is entered: (name, masks) each."""
    from fgn_amd import ops
    calls, real = [], (ops.color_masks, ops.color_mask_rows)
    ops.color_masks = lambda s, items, *a, **k: calls.append(('masks', sum(len(m) for _, m in items))) or real[0](s, items, *a, **k)
    ops.color_mask_rows = lambda s, t, items: calls.append(('rows', len(items))) or real[1](s, t, items)
    try:
        yield calls
    finally:
        ops.color_masks, ops.color_mask_rows = real


@pytest.mark.parametrize('graphs', (False, True), ids=('eager', 'graphs'))
@pytest.mark.parametrize('frame', ('network', 'resize', 'source'))
def test_simple_test_with_colour_ground_truth_is_the_dense_call(ds, model, frame, graphs):
    """Two images, the second without an instance; every key, the overlap counts and the matched bits of the device
    included.  All entries colour, then dense / colour and RLE / colour mixed."""
    m = _reset(model, ds)
    m.match_on_device = m.evaluate_on_device = True
    resize = frame != 'network'
    samples = [_query(ds[0], QRY_SIZES[0] if resize else (NET, NET), resize),
               _query(ds[1], QRY_SIZES[1] if resize else (NET, NET), resize, empty=True)]
    colour = _batch([_ready_supports(s) for s in samples])
    kw = dict(rescale=True, results_at_source=frame == 'source')
    want = m.simple_test(**_dense(colour), **kw)
    assert all(k in want[0] for k in ('dt_gt_inter', 'dt_area', 'gt_area', 'dt_match_bbox', 'dt_match_segm'))
    assert len(want[0]['qry_isegmaps_rle']) > 0 and want[1]['qry_isegmaps_rle'] == []
    assert sum(rle.decode(s).sum() for s in want[0]['qry_isegmaps_rle']) > 0
    m.use_graphs = graphs
    with _made_on_the_device() as calls:
        _same_results(want, m.simple_test(**colour, **kw))
    assert calls == [('masks', len(want[0]['qry_isegmaps_rle']))]          # ONE launch for the batch
    as_dict = dict(colour, qry_isegmaps=[{'bboxes': g.boxes, 'colors': g.colors} for g in colour['qry_isegmaps']])
    _same_results(want, m.simple_test(**as_dict, **kw))                     # the dict form
    _same_results(want, m.simple_test(**_dense(colour, qry=(1,)), **kw))    # mixed: colour, dense (empty)
    _same_results(want, m.simple_test(**_dense(colour, qry=(), runs=(1,)), **kw))           # mixed: colour, RLE (the empty list)
    both = _batch([_ready_supports(s) for s in (samples[0], samples[0])])
    want2 = m.simple_test(**_dense(both), **kw)
    _same_results(want2, m.simple_test(**_dense(both, qry=(), runs=(0,)), **kw))            # mixed: RLE, colour
    _same_results(want2, m.simple_test(**_dense(both, qry=(1,)), **kw))                     # mixed: colour, dense


@pytest.mark.parametrize('mode', (0, 3), ids=('upload-stream', 'caller-stream'))
@pytest.mark.parametrize('frame', ('network', 'resize'))
def test_consecutive_episodes_replay_one_graph_through_the_same_static_slot(ds, model, frame, mode):
    """Graph replay on: episodes with DIFFERENT images alternate through one captured graph - with the transfers on the
    caller stream the bytes go straight into the graph's static slot and the masks are made from there - and every one
    gives the dense eager call's results: each mask is made from the bytes of ITS episode."""
    m = _reset(model, ds)
    resize = frame == 'resize'
    sizes = [(150, 131), (141, 160), (150, 131)] if resize else [(NET, NET)] * 3
    eps = [_batch([_ready_supports(_query(ds[2 + i], sizes[i], resize))]) for i in range(3)]
    want = [m.simple_test(**_dense(b), rescale=True) for b in eps]
    assert want[0][0]['qry_isegmaps_rle'] != want[1][0]['qry_isegmaps_rle']
    m.use_graphs, m.transfer_mode = True, mode
    before = set(m._graphs)
    for i in (0, 1, 2, 1, 0):
        _same_results(want[i], m.simple_test(**eps[i], rescale=True))
    assert len([k for k in m._graphs if k not in before]) == 1
    m.use_graphs, m.transfer_mode = False, 0


def test_colour_supports_are_the_dense_supports_eager_and_under_one_graph(ds, model):
    m = _reset(model, ds)
    sets = [_batch([_cut(_query(ds[2 + i], (NET, NET), False), i)]) for i in range(2)]
    sizes = [[tuple(t.shape[:2]) for t in b['spp_imgs'][0]] for b in sets]
    assert sizes[0] != sizes[1] and len(set(sizes[0])) > 1
    want = [m.simple_test(**_dense(b), rescale=True) for b in sets]
    with _made_on_the_device() as calls:
        _same_results(want[0], m.simple_test(**sets[0], rescale=True))
    assert sorted(calls) == sorted([('rows', NK), ('masks', len(want[0][0]['qry_isegmaps_rle']))])   # one launch for N*K windows
    dense1 = _dense(sets[1])
    mixed = dict(sets[1], spp_isegmaps=[[a if i % 3 == 0 else rle.encode(b) if i % 3 == 1 else b for i, (a, b) in
                                         enumerate(zip(sets[1]['spp_isegmaps'][0], dense1['spp_isegmaps'][0]))]])
    _same_results(want[1], m.simple_test(**mixed, rescale=True))            # colour, RLE and dense instances in one set
    for mode in (0, 3):
        m.use_graphs, m.transfer_mode = True, mode
        before = set(m._graphs)
        for rep in range(2):
            for w, b in zip(want, sets):
                _same_results(w, m.simple_test(**b, rescale=True))
        new = [k for k in m._graphs if k not in before]
        assert len(new) == 1                        # one graph for both support sets
    ge = m._graphs[new[0]]
    assert tuple(ge.static['spp_msk'].shape) == (NK, POOL * POOL)
    sp = m._source_supports(dense1['spp_imgs'], dense1['spp_bboxes'], dense1['spp_isegmaps'], SPP, graphed=True)
    torch.cuda.synchronize()
    for i in range(NK):                             # the static mask slot holds the windows of the last set
        assert torch.equal(ge.static['spp_msk'][i, :sp['mflats'][i].numel()].cpu(), sp['mflats'][i]), i
    m.use_graphs, m.transfer_mode = False, 0
    a, b = _dense(sets[0]), sets[0]
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


def _train_batch(ds, kind):
    """Two episodes, all masks box + colour, for one training form."""
    if kind == 'plain':                             # network-size uint8 query, ready supports (dense tensor, stays dense)
        return _batch([_ready_supports(_query(ds[i], (NET, NET), False)) for i in range(2)])
    if kind == 'qry_photometric':                   # source-size queries of two sizes: photometric pass, then the warp
        return _batch([dict(_ready_supports(_query(ds[i], QRY_SIZES[i], True)), qry_augment=QRY_GEO[i],
                            qry_photometric=QRY_PHOTO[i]) for i in range(2)])
    return _batch([dict(_cut(_query(ds[i], (NET, NET), False), i), spp_augment=GEO[i], spp_photometric=SPP_PHOTO[i])
                   for i in range(2)])             # source supports, cut, then augmented; network-size query


@pytest.mark.parametrize('kind', ('plain', 'qry_photometric', 'spp_augment'))
def test_forward_train_losses_are_bit_equal_to_dense(ds, model, kind):
    """Also where the image is changed after its upload: the masks come from the bytes as uploaded, ahead of the
    photometric pass (queries) and of the cut and its augmentation (supports), as the reference derives them before it
    augments."""
    m = _reset(model, ds)
    colour = _train_batch(ds, kind)
    with _made_on_the_device() as calls:
        got = _losses(m, colour)
    assert sorted(n for n, _ in calls) == (['masks', 'rows'] if kind == 'spp_augment' else ['masks'])
    _same_losses(_losses(m, _dense(colour)), got)
    _same_losses(got, _losses(m, _dense(colour, qry=(0,), spp=False)))       # mixed: dense, colour


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
    colour = _train_batch(ds, 'spp_augment')
    a, b = _step(_dense(colour), ds), _step(colour, ds)
    _same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].dtype == b[1][k].dtype and torch.equal(a[1][k].view(torch.uint8), b[1][k].view(torch.uint8)), k


def test_pack_results_host_fallback_derives_colour_masks(ds, model):
    """Where no device string exists for the ground truth (``detect_device`` was not given the masks), ``pack_results``
    derives a colour entry on the host from the image it was bound to."""
    m = _reset(model, ds)
    colour = _batch([_ready_supports(_query(ds[i], (NET, NET), False)) for i in range(2)])
    out = []
    for b in (_dense(colour), colour):
        dets = m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'])
        assert all('gt_slice' not in d for d in dets)
        gts = m._gt_front(b['qry_isegmaps'], b['qry_img'], b['img_shape'], None)
        out.append(m.pack_results(dets, 2, qry_isegmaps=gts, img_shape=b['img_shape']))
    for a, g in zip(*out):
        assert len(a['qry_isegmaps_rle']) > 0 and a['qry_isegmaps_rle'] == g['qry_isegmaps_rle']


def test_without_a_colour_entry_nothing_new_is_called(ds, model):
    m = _reset(model, ds)
    dense = _dense(_batch([_cut(_query(ds[0], QRY_SIZES[0], True), 0)]))
    runs = _dense(_batch([_cut(_query(ds[0], QRY_SIZES[0], True), 0)]), qry=(), runs=(0,))
    with _made_on_the_device() as calls:
        for graphs in (False, True):
            m.use_graphs = graphs
            m.simple_test(**dense, rescale=True)
            m.simple_test(**runs, rescale=True)
        m.use_graphs = False
        _losses(m, dense)
        m.encode_supports(dense['spp_imgs'], dense['spp_bboxes'], dense['spp_isegmaps'], spp_crop_to=SPP)
    assert calls == []
