"""Augmented source-size queries through the detector and the trainer (``qry_augment``) against the same code fed the
host-prepared network-size batch of ``fewshot_ds.augment_query`` through the uint8 path - byte for byte: the losses of
``forward_train``, the losses and every trained tensor of ``Trainer.step``, ``Trainer.step`` on source-size queries and
source supports without augmentation, the fallback and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
SIZES = [(150, 131), (101, 77)]
SPP_KEYS = ('spp_crop_to', 'spp_fill_ratio', 'crop_square')


def row(flip=0, rotate=0., scale=1., shear=0., tx=0., ty=0., border=0, order=0):
    return np.array([flip, rotate, scale, shear, tx, ty, border, order], np.float64)


ROWS = np.stack([row(flip=1), row(rotate=10, border=1, order=4)])        # one kind 0 with flip, one kind 1


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
    """The loader's route: ``augment_query`` on the host (``resize_query`` without a row), a network-size sample for the
    existing uint8 path."""
    img, boxes, masks = fd.augment_query(sample['qry_img'].numpy(), sample['qry_bboxes'], sample['qry_isegmaps'], NET, NET,
                                         sample.get('qry_augment'))
    out = {k: v for k, v in sample.items() if k not in ('qry_resize_to', 'qry_augment')}
    out.update(qry_img=torch.from_numpy(np.ascontiguousarray(img)), qry_bboxes=boxes, qry_isegmaps=masks)
    return out


def _host_supports(sample: dict) -> dict:
    """``support_from_source`` per instance on the host: ready crops for the existing uint8 path."""
    made = [fd.support_from_source(im.numpy(), bb, mk, sample['spp_crop_to'], sample['spp_fill_ratio'], sample['crop_square'])
            for im, mk, bb in zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])]
    out = {k: v for k, v in sample.items() if k not in SPP_KEYS}
    out.update(spp_imgs=torch.from_numpy(np.stack([c for c, _, _ in made])), spp_bboxes=np.stack([b for _, b, _ in made]),
               spp_isegmaps=np.stack([m for _, _, m in made]))
    return out


def _pair(ds, first, rows, supports=False):
    """(source batch, host-prepared batch) of the two source sizes; ``rows``: the augmentation of each image or None."""
    src = [_crop(ds[first + i], s) for i, s in enumerate(SIZES)]
    if rows is not None:
        for s, r in zip(src, rows):
            s['qry_augment'] = np.asarray(r, np.float64)
    host = collate([_host_supports(_host_query(s)) if supports else _host_query(s) for s in src])
    imgs = [s.pop('qry_img') for s in src]
    bs = collate(src)
    bs['qry_img'] = imgs
    if rows is not None:
        assert tuple(bs['qry_augment'].shape) == (len(SIZES), 8) and 'qry_augment' not in host
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


def test_forward_train_on_augmented_source_pixels_gives_the_losses_of_the_host_prepared_batch(ds, model):
    bs, host = _pair(ds, 0, ROWS)
    for r, b, s, kind in zip(ROWS, bs['qry_bboxes'], SIZES, (0, 1)):     # both rows are applied: no fallback here
        rec, _ = fd.augment_plan(r, b.numpy(), s, (NET, NET))
        assert rec[2] == kind and rec[2:6].any()
    _same_losses(_losses(model, host), _losses(model, bs))
    # the augmentation is seen: other losses than the plain batch gives
    plain = _losses(model, _pair(ds, 0, None)[0])
    assert any(_val(plain[k]).numpy().tobytes() != _val(v).numpy().tobytes() for k, v in _losses(model, bs).items())
    # rows as an array, img_shape left to its default
    kw = {k: v for k, v in bs.items() if k not in ('img_shape', 'qry_augment')}
    _same_losses(_losses(model, host), _losses(model, dict(kw, qry_augment=ROWS)))


def test_a_fallback_row_matches_the_call_without_augmentation(ds, model):
    rows = np.stack([row(tx=-120, order=3), row()])                      # a box of image 0 leaves it: un-augmented
    bs, host = _pair(ds, 0, rows)
    rec, _ = fd.augment_plan(rows[0], bs['qry_bboxes'][0].numpy(), SIZES[0], (NET, NET))
    assert not rec[2:6].any()
    plain, _ = _pair(ds, 0, None)
    want = _losses(model, plain)
    _same_losses(want, _losses(model, bs))
    _same_losses(want, _losses(model, host))


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


def _same_steps(a, b):
    _same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].numpy().tobytes() == b[1][k].numpy().tobytes(), k
    assert any(float(v.abs().max()) > 0 for k, v in a[1].items() if k.startswith('state/'))     # the step trained


def test_trainer_step_on_augmented_source_pixels_is_the_step_on_the_host_prepared_batch(ds):
    bs, host = _pair(ds, 0, ROWS)
    _same_steps(_step(host, ds), _step(bs, ds))


def test_trainer_step_on_source_queries_and_source_supports_is_the_step_on_the_host_built_batch():
    dss = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=POOL,
                                       spp_img_size=SPP, raw_uint8=True, spp_source=True)
    bs, host = _pair(dss, 0, None, supports=True)
    assert bs['spp_crop_to'] == SPP and isinstance(bs['spp_imgs'][0], list) and 'qry_resize_to' in bs
    assert 'spp_crop_to' not in host and 'qry_resize_to' not in host
    _same_steps(_step(host, dss), _step(bs, dss))


@contextlib.contextmanager
def _refused_before_anything_is_queued(m):
    """A ValueError inside, raised before the detector uploads, allocates on the device or launches: every step that
    queues work is replaced by one that fails the test, and the device allocator's byte count does not move."""
    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_source', '_resized_masks', '_augmented_masks', '_supports_on_device', '_detect_eager',
             '_detect_graphed', '_stem_input')
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for n in names:
        setattr(m, n, boom)
    try:
        with pytest.raises(ValueError) as err:
            yield err
    finally:
        for n in names:
            delattr(m, n)                       # (instance attributes: the class's methods are back)
    assert torch.cuda.memory_allocated() == before


def test_contract_errors_queue_nothing(ds, model):
    m = model
    bs, host = _pair(ds, 0, ROWS)
    with _refused_before_anything_is_queued(m) as err:                              # no source size to augment from
        m.forward_train(**host, qry_augment=ROWS)
    assert 'qry_resize_to' in str(err.value)

    def with_rows(rows):
        return dict(bs, qry_augment=rows)

    def one(**kw):
        return np.stack([row(**kw), row()])
    bad = [ROWS[:, :7], np.concatenate([ROWS, ROWS]), ROWS[0], torch.from_numpy(ROWS).reshape(2, 2, 4),    # shapes
           one(rotate=np.nan), one(tx=np.inf), one(scale=-np.inf),                                        # non-finite
           one(flip=2), one(flip=0.5), one(border=2), one(border=-1), one(order=6), one(order=2.5),       # outside the sets
           one(scale=0), one(scale=1e-9), one(tx=3e6), one(ty=-3e6)]                                      # beyond the bounds
    for rows in bad:
        with _refused_before_anything_is_queued(m):
            m.forward_train(**with_rows(rows))
    with _refused_before_anything_is_queued(m) as err:                              # the test is without augmentation
        m.simple_test(**bs, rescale=True)
    assert 'qry_augment' in str(err.value)
    # the trainer goes through the same front
    from fgn_amd.train import Trainer
    m2 = _model()
    m2.set_input_norm(**ds.input_norm)
    tr = Trainer(m2)
    for b in (dict(host, qry_augment=ROWS), with_rows(one(flip=2))):
        with _refused_before_anything_is_queued(m2):
            tr.step(b)
        assert m2._tape is None and tr.n_steps == 0
