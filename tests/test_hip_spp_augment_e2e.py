"""Support augmentation through the detector and the trainer (``spp_augment`` / ``spp_photometric``) against the same code
fed the host-prepared batch of ready S x S uint8 supports from ``fewshot_ds.augment_support`` - byte for byte: the losses
of ``forward_train``, the losses and every trained tensor of ``Trainer.step``, with and without ``qry_augment``; the
per-instance fallback, neutral rows with their launches, and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import ops
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 1, 160, 128, 96
NK = N_WAYS * K_SHOTS
QRY_SIZES = [(150, 131), (101, 77)]
SPP_KEYS = ('spp_crop_to', 'spp_fill_ratio', 'crop_square', 'spp_augment', 'spp_photometric')
LAUNCHES = ('support_from_source', 'support_from_source_u8', 'photometric_u8', 'support_augment')


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return [flip, rotate, scale, shear, tx, ty, border, order]


# per episode and instance: a flip, a rotation with a channel order, a neutral instance | a shift, a scale, a shear
GEO = np.array([[row(flip=1), row(rotate=10, border=1, order=4), row()],
                [row(tx=7, ty=-5), row(scale=1.2), row(shear=-10, border=1)]], np.float64)
# a blur, a hue, nothing | noise, nothing, brightness
PHOTO = np.array([[(3, 1.5, 0), (4, 50, 0), (0, 0, 0)], [(1, 2.0, 9), (0, 0, 0), (6, -30, 0)]], np.float64)
QRY_GEO = np.array([row(flip=1), row(rotate=10, border=1, order=4)], np.float64)


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _query(sample: dict, size, resize: bool) -> dict:
    """The top-left (h, w) window of a pool sample as the query: at network size as it is, or (``resize``) as a
    source-size query for ``qry_resize_to``."""
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
               qry_cat_ids_real=np.asarray(sample['qry_cat_ids_real'])[keep], img_shape=np.array([NET, NET, 3], np.int32))
    if resize:
        out['qry_resize_to'] = np.array([NET, NET], np.int32)
    return out


def _cut(sample: dict, k: int) -> dict:
    """The supports' source images cut to windows around their instances, margins chosen by (instance, ``k``): the
    images of a support set get differing sizes and the crops' context leaves the cut images (reflection)."""
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


def _host_supports(sample: dict) -> dict:
    """The loader's route: ``support_from_source`` and ``augment_support`` per instance on the host, ready S x S uint8
    supports for the existing uint8 path."""
    geo, photo = sample.get('spp_augment'), sample.get('spp_photometric')
    made = []
    for i, (im, mk, bb) in enumerate(zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])):
        crop, box, mask = fd.support_from_source(im.numpy(), bb, mk, sample['spp_crop_to'], sample['spp_fill_ratio'],
                                                 sample['crop_square'])
        made.append(fd.augment_support(crop, box, mask, None if geo is None else geo[i], None if photo is None else photo[i]))
    out = {k: v for k, v in sample.items() if k not in SPP_KEYS}
    out.update(spp_imgs=torch.from_numpy(np.stack([np.ascontiguousarray(c) for c, _, _ in made])),
               spp_bboxes=np.stack([b for _, b, _ in made]).astype(np.float32),
               spp_isegmaps=np.stack([np.asarray(m, bool) for _, _, m in made]))
    return out


@pytest.fixture(scope='module')
def ds():
    return fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                        spp_img_size=SPP, raw_uint8=True, spp_source=True)


def _pair(ds, geo, photo, qry_geo=None):
    """(source-support batch carrying the rows, host-prepared batch) of two episodes; with ``qry_geo`` the queries come
    at two source sizes with ``qry_augment``, in both batches alike."""
    src = []
    for i in range(2):
        s = _cut(_query(ds[i], QRY_SIZES[i] if qry_geo is not None else (NET, NET), qry_geo is not None), i)
        if qry_geo is not None:
            s['qry_augment'] = np.asarray(qry_geo[i], np.float64)
        for key, rows in (('spp_augment', geo), ('spp_photometric', photo)):
            if rows is not None:
                s[key] = np.asarray(rows[i], np.float64)
        src.append(s)
    sizes = [tuple(t.shape[:2]) for s in src for t in s['spp_imgs']]
    assert len(set(sizes)) > 1                                                      # sources of differing sizes
    host = [_host_supports(s) for s in src]
    out = []
    for samples in (src, host):
        if qry_geo is not None:                                                     # (images of two sizes: a list)
            imgs = [s.pop('qry_img') for s in samples]
            b = collate(samples)
            b['qry_img'] = imgs
        else:
            b = collate(samples)
        out.append(b)
    bs, hb = out
    if geo is not None:
        assert tuple(bs['spp_augment'].shape) == (2, NK, 8)
    assert not any(k in hb for k in SPP_KEYS) and tuple(hb['spp_imgs'].shape) == (2, NK, SPP, SPP, 3)
    assert hb['spp_imgs'].dtype == torch.uint8 and bs['spp_crop_to'] == SPP
    return bs, hb


@pytest.fixture(scope='module')
def model(ds):
    m = _model()
    m.set_input_norm(**ds.input_norm)
    return m


def _val(v):
    return torch.as_tensor(v[0] if isinstance(v, list) else v).detach().cpu().reshape(-1)


def _bytes(losses):
    return {k: _val(v).numpy().tobytes() for k, v in losses.items()}


def _same_losses(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = _val(a[k]), _val(b[k])
        assert x.dtype == y.dtype and x.numpy().tobytes() == y.numpy().tobytes(), k
    assert all(np.isfinite(float(_val(v)[0])) for v in a.values())
    assert float(_val(a['loss_rpn_cls'])[0]) > 0 and float(_val(a['loss_cls'])[0]) > 0


def _losses(m, batch, seed=3):
    m._PT = None                                    # fresh running statistics
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    return m.forward_train(**batch, perm_fn=lambda n: torch.randperm(n, generator=g))


@contextlib.contextmanager
def _counted():
    """The calls into ``ops`` that make supports, in order."""
    calls, real = [], {n: getattr(ops, n) for n in LAUNCHES}
    for n in LAUNCHES:
        setattr(ops, n, (lambda name: lambda *a, **k: calls.append(name) or real[name](*a, **k))(n))
    try:
        yield calls
    finally:
        for n in LAUNCHES:
            setattr(ops, n, real[n])


@pytest.fixture(scope='module')
def plain(ds, model):
    """The losses of the batch without the arguments and the launches it makes: computed once, shared."""
    with _counted() as calls:
        losses = _losses(model, _pair(ds, None, None)[0])
    assert calls == ['support_from_source']
    return losses


@pytest.mark.parametrize('qry_geo', (None, QRY_GEO), ids=('supports', 'supports+qry_augment'))
def test_forward_train_on_source_supports_gives_the_losses_of_the_host_prepared_batch(ds, model, plain, qry_geo):
    bs, host = _pair(ds, GEO, PHOTO, qry_geo)
    with _counted() as calls:
        got = _losses(model, bs)
    assert calls == ['support_from_source_u8', 'photometric_u8', 'support_augment']    # three launches, whatever n
    _same_losses(_losses(model, host), got)
    base = plain if qry_geo is None else _losses(model, _pair(ds, None, None, qry_geo)[0])
    assert _bytes(got) != _bytes(base)                                                 # the operators are seen
    if qry_geo is None:
        # each half alone, seen and equal to its host batch; without photometric rows the pass is not launched
        for geo, photo, want in ((GEO, None, ['support_from_source_u8', 'support_augment']),
                                 (None, PHOTO, ['support_from_source_u8', 'photometric_u8', 'support_augment'])):
            b2, h2 = _pair(ds, geo, photo)
            with _counted() as calls:
                half = _losses(model, b2)
            assert calls == want
            _same_losses(_losses(model, h2), half)
            assert _bytes(half) != _bytes(got) and _bytes(half) != _bytes(plain)
        # rows as arrays
        kw = {k: v for k, v in bs.items() if k not in ('spp_augment', 'spp_photometric')}
        _same_losses(got, _losses(model, dict(kw, spp_augment=GEO, spp_photometric=PHOTO)))


def test_an_instance_whose_box_leaves_its_crop_is_used_unaugmented_alone(ds, model):
    geo, photo = GEO.copy(), PHOTO.copy()
    geo[0, 1] = row(tx=-500, order=3)                                                  # its box leaves the crop
    photo[0, 1] = (1, 2.0, 5)
    bs, host = _pair(ds, geo, photo)
    sp = model._source_supports(bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], SPP)
    *_, fell = fd.support_augment_plan(geo.reshape(-1, 8), photo.reshape(-1, 3), sp['boxes'].numpy().reshape(-1, 4), SPP)
    assert fell.tolist() == [False, True, False, False, False, False]
    got = _losses(model, bs)
    _same_losses(_losses(model, host), got)
    geo[0, 1], photo[0, 1] = row(), (0, 0, 0)                                          # the same batch, that instance neutral
    _same_losses(_losses(model, _pair(ds, geo, photo)[0]), got)
    photo[0, 1] = (1, 2.0, 5)                                                          # (its noise alone is seen)
    assert _bytes(_losses(model, _pair(ds, geo, photo)[0])) != _bytes(got)


def test_all_neutral_rows_match_the_call_without_the_arguments_and_make_its_launches(ds, model, plain):
    neutral = np.tile(np.array(row(), np.float64), (2, NK, 1))
    gone = neutral.copy()
    gone[1, 2] = row(tx=-500)                                                          # all neutral after the fallback
    for geo, photo in ((neutral, np.zeros((2, NK, 3))), (neutral, None), (None, np.zeros((2, NK, 3))),
                       (gone, np.array([[(3, 0, 0), (6, 0, 9), (0, 0, 0)], [(0, 0, 0), (0, 0, 0), (1, 2.0, 5)]], np.float64))):
        with _counted() as calls:
            got = _losses(model, _pair(ds, geo, photo)[0])
        assert calls == ['support_from_source']
        _same_losses(plain, got)


def _step(batch, ds, seed=5):
    """One ``Trainer.step`` of a freshly built, identically seeded model -> (losses, every trained tensor)."""
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
    assert tr.n_steps == 1 and m._tape is None
    return losses, tensors


@pytest.mark.parametrize('qry_geo', (None, QRY_GEO), ids=('supports', 'supports+qry_augment'))
def test_trainer_step_on_source_supports_is_the_step_on_the_host_prepared_batch(ds, qry_geo):
    bs, host = _pair(ds, GEO, PHOTO, qry_geo)
    a, b = _step(host, ds), _step(bs, ds)
    _same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].numpy().tobytes() == b[1][k].numpy().tobytes(), k
    assert any(float(v.abs().max()) > 0 for k, v in a[1].items() if k.startswith('state/'))     # the step trained


@contextlib.contextmanager
def _refused_before_anything_is_queued(m, name):
    """A ValueError that names the keyword, raised before the detector uploads, allocates on the device or launches:
    every step that queues work is replaced by one that fails the test, and the allocator's byte count does not move."""
    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_source', '_upload_supports', '_supports_on_device', '_support_front', '_detect_eager',
             '_detect_graphed', '_stem_input')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for n in names:
        setattr(m, n, boom)
    try:
        with pytest.raises(ValueError, match=name):
            yield
    finally:
        for n in names:
            delattr(m, n)                       # (instance attributes: the class's methods are back)
    assert torch.cuda.memory_allocated() == before


def test_contract_errors_queue_nothing(ds, model):
    m = model
    bs, host = _pair(ds, GEO, PHOTO)
    plain_b = {k: v for k, v in bs.items() if k not in ('spp_augment', 'spp_photometric')}

    def geo_with(r):
        g = GEO.copy()
        g[1, 0] = r
        return g

    def photo_with(r):
        p = PHOTO.copy()
        p[0, 2] = r
        return p
    with _counted() as calls:
        for name, rows in (('spp_augment', GEO), ('spp_photometric', PHOTO)):          # no source supports to work on
            with _refused_before_anything_is_queued(m, name):
                m.forward_train(**host, **{name: rows})
        for bad in (GEO[:1], GEO[:, :2], GEO[..., :7], GEO.reshape(-1, 8), GEO[0], geo_with(row(rotate=np.nan)),
                    geo_with(row(flip=2)), geo_with(row(border=2)), geo_with(row(order=6)), geo_with(row(scale=0)),
                    geo_with(row(tx=2.0 ** 21))):
            for extra in ({}, {'spp_photometric': PHOTO}):
                with _refused_before_anything_is_queued(m, 'spp_augment'):
                    m.forward_train(**plain_b, **extra, spp_augment=bad)
        for bad in (PHOTO[:1], PHOTO[..., :2], PHOTO.reshape(-1, 3), torch.from_numpy(PHOTO)[..., None],
                    photo_with((np.nan, 0, 0)), photo_with((7, 0, 0)), photo_with((1, 2.5, 0)), photo_with((1, 1, 0.5)),
                    photo_with((1, 1, 2.0 ** 32)), photo_with((2, 1.5, 0)), photo_with((4, 256, 0)),
                    photo_with((3, 5.4, 0))):                                       # sigma 5.4 crop pixels: a radius of 17
            for extra in ({}, {'spp_augment': GEO}):
                with _refused_before_anything_is_queued(m, 'spp_photometric'):
                    m.forward_train(**plain_b, **extra, spp_photometric=bad)
        for name in ('spp_augment', 'spp_photometric'):                                # the test is without augmentation
            with _refused_before_anything_is_queued(m, name):
                m.simple_test(**plain_b, **{name: bs[name]}, rescale=True)
            with _refused_before_anything_is_queued(m, name):
                m.encode_supports(bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], spp_crop_to=SPP, **{name: bs[name]})
            with _refused_before_anything_is_queued(m, name):
                m.detect_device(bs['qry_img'], bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], bs['img_shape'],
                                spp_crop_to=SPP, **{name: bs[name]})
        # the trainer goes through the same front
        from fgn_amd.train import Trainer
        m2 = _model()
        m2.set_input_norm(**ds.input_norm)
        tr = Trainer(m2)
        for name, b in (('spp_augment', dict(host, spp_augment=GEO)),
                        ('spp_photometric', dict(bs, spp_photometric=photo_with((7, 0, 0))))):
            with _refused_before_anything_is_queued(m2, name):
                tr.step(b)
            assert m2._tape is None and tr.n_steps == 0
    assert calls == []
