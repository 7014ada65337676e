"""Photometric augmentation of source-size queries through the detector and the trainer (``qry_photometric``) against
the same code fed the host-prepared network-size batch of ``fewshot_ds.augment_query_full`` through the uint8 path - byte
for byte: the losses of ``forward_train``, the losses and every trained tensor of ``Trainer.step``, with and without
``qry_augment``; the fallback, neutral rows and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import ops
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
SIZES = [(150, 131), (101, 77)]
GEO = np.array([[1, 0, 1, 0, 0, 0, 0, 0], [0, 10, 1, 0, 0, 0, 1, 4]], np.float64)      # a flip; a rotation with an order
PHOTO = np.array([[3, 2.0, 0], [4, 50, 0]], np.float64)                                # blur on one image, hue on the other
KEYS = ('qry_resize_to', 'qry_augment', 'qry_photometric')


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


def _crop(sample: dict, size) -> dict:
    """The top-left (h, w) window of a pool sample as a source-size query: image, masks and boxes cut to it; instances
    that the window leaves nothing of are dropped."""
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


def _host_query(sample: dict) -> dict:
    """The loader's route: ``augment_query_full`` on the host, a network-size sample for the existing uint8 path."""
    img, boxes, masks = fd.augment_query_full(sample['qry_img'].numpy(), sample['qry_bboxes'], sample['qry_isegmaps'],
                                              NET, NET, sample.get('qry_augment'), sample.get('qry_photometric'))
    out = {k: v for k, v in sample.items() if k not in KEYS}
    out.update(qry_img=torch.from_numpy(np.ascontiguousarray(img)), qry_bboxes=boxes, qry_isegmaps=masks)
    return out


def _pair(ds, geo, photo):
    """(source batch, host-prepared batch) of the two source sizes; ``geo`` / ``photo``: the rows of each image or None."""
    src = [_crop(ds[i], s) for i, s in enumerate(SIZES)]
    for key, rows in (('qry_augment', geo), ('qry_photometric', photo)):
        if rows is not None:
            for s, r in zip(src, rows):
                s[key] = np.asarray(r, np.float64)
    host = collate([_host_query(s) for s in src])
    imgs = [s.pop('qry_img') for s in src]
    bs = collate(src)
    bs['qry_img'] = imgs
    if photo is not None:
        assert tuple(bs['qry_photometric'].shape) == (len(SIZES), 3) and not any(k in host for k in KEYS)
    return bs, host


@pytest.fixture(scope='module')
def ds():
    return fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                        spp_img_size=SPP, raw_uint8=True)


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


@pytest.fixture(scope='module')
def plain(ds, model):
    """The losses of the batch without either augmentation: computed once, shared."""
    return _losses(model, _pair(ds, None, None)[0])


@pytest.mark.parametrize('geo', (None, GEO), ids=('photometric', 'augment+photometric'))
def test_forward_train_on_source_pixels_gives_the_losses_of_the_host_prepared_batch(ds, model, plain, geo):
    bs, host = _pair(ds, geo, PHOTO)
    got = _losses(model, bs)
    _same_losses(_losses(model, host), got)
    assert _bytes(got) != _bytes(plain)                                                # the operators are seen
    if geo is not None:                                                                # ... and so is each half
        assert _bytes(got) != _bytes(_losses(model, _pair(ds, geo, None)[0]))
    # rows as arrays, img_shape left to its default
    kw = {k: v for k, v in bs.items() if k not in ('img_shape', 'qry_augment', 'qry_photometric')}
    if geo is not None:
        kw['qry_augment'] = geo
    _same_losses(got, _losses(model, dict(kw, qry_photometric=PHOTO)))


def test_a_fallback_row_matches_the_call_without_either_augmentation(ds, model, plain):
    geo = np.array([[0, 0, 1, 0, -120, 0, 0, 3], [0, 0, 1, 0, 0, 0, 0, 0]], np.float64)    # a box of image 0 leaves it
    photo = np.array([[1, 2.0, 5], [0, 0, 0]], np.float64)
    bs, host = _pair(ds, geo, photo)
    rec, _ = fd.augment_plan(geo[0], bs['qry_bboxes'][0].numpy(), SIZES[0], (NET, NET))
    assert not rec[2:6].any()
    _same_losses(plain, _losses(model, bs))
    _same_losses(plain, _losses(model, host))
    # the same noise without the geometric row is applied
    assert _bytes(_losses(model, _pair(ds, None, photo)[0])) != _bytes(plain)


def test_neutral_rows_match_the_call_without_the_argument_and_launch_nothing(ds, model, plain, monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the photometric pass was launched for neutral rows')
    monkeypatch.setattr(ops, 'photometric_u8', boom)
    for photo in (np.zeros((2, 3)), np.array([[3, 0, 0], [6, 0, 9]], np.float64)):
        _same_losses(plain, _losses(model, _pair(ds, None, photo)[0]))
    geo = np.array([[0, 0, 1, 0, -120, 0, 0, 3], [0, 0, 1, 0, 0, 0, 0, 0]], np.float64)    # all neutral after the fallback
    _same_losses(plain, _losses(model, _pair(ds, geo, np.array([[1, 2.0, 5], [0, 0, 0]], np.float64))[0]))


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


@pytest.mark.parametrize('geo', (None, GEO), ids=('photometric', 'augment+photometric'))
def test_trainer_step_on_source_pixels_is_the_step_on_the_host_prepared_batch(ds, geo):
    bs, host = _pair(ds, geo, PHOTO)
    a, b = _step(host, ds), _step(bs, ds)
    _same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].numpy().tobytes() == b[1][k].numpy().tobytes(), k
    assert any(float(v.abs().max()) > 0 for k, v in a[1].items() if k.startswith('state/'))     # the step trained


@contextlib.contextmanager
def _refused_before_anything_is_queued(m):
    """A ValueError that names the keyword, raised before the detector uploads, allocates on the device or launches:
    every step that queues work is replaced by one that fails the test, and the allocator's byte count does not move."""
    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_source', '_resized_masks', '_augmented_masks', '_supports_on_device', '_detect_eager',
             '_detect_graphed', '_stem_input')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for n in names:
        setattr(m, n, boom)
    try:
        with pytest.raises(ValueError, match='qry_photometric'):
            yield
    finally:
        for n in names:
            delattr(m, n)                       # (instance attributes: the class's methods are back)
    assert torch.cuda.memory_allocated() == before


def test_contract_errors_queue_nothing(ds, model, monkeypatch):
    m = model
    bs, host = _pair(ds, GEO, PHOTO)
    monkeypatch.setattr(ops, 'photometric_u8', lambda *a, **k: pytest.fail('launched before the contract error'))
    with _refused_before_anything_is_queued(m):                                     # no source pixels to work on
        m.forward_train(**host, qry_photometric=PHOTO)

    def one(*r):
        return np.array([r, (0, 0, 0)], np.float64)
    bad = [PHOTO[:, :2], np.concatenate([PHOTO, PHOTO]), PHOTO[0], torch.from_numpy(PHOTO).reshape(2, 3, 1),       # shapes
           one(np.nan, 0, 0), one(1, np.inf, 0), one(1, 1, np.nan),                                               # non-finite
           one(7, 0, 0), one(-1, 0, 0), one(2.5, 0, 0), one(1, 1, -1), one(1, 1, 2.0 ** 32), one(1, 1, 0.5),      # sets
           one(1, 2.5, 0), one(1, 0, 0), one(2, 1.5, 0), one(2, -0.1, 0), one(3, -1, 0), one(4, 256, 0),
           one(5, -300, 0), one(6, 255.5, 0),                                                                     # amounts
           one(3, 5.0, 0)]                                             # 5 network = 5.86 source pixels: a radius of 18
    for rows in bad:
        for extra in ({}, {'qry_augment': None}):
            with _refused_before_anything_is_queued(m):
                m.forward_train(**{**bs, **extra, 'qry_photometric': rows})
    with _refused_before_anything_is_queued(m):                                     # the test is without augmentation
        m.simple_test(**{k: v for k, v in bs.items() if k != 'qry_augment'}, rescale=True)
    # the trainer goes through the same front
    from fgn_amd.train import Trainer
    m2 = _model()
    m2.set_input_norm(**ds.input_norm)
    tr = Trainer(m2)
    for b in (dict(host, qry_photometric=PHOTO), dict(bs, qry_photometric=one(7, 0, 0))):
        with _refused_before_anything_is_queued(m2):
            tr.step(b)
        assert m2._tape is None and tr.n_steps == 0
