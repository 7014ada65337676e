"""Chains of photometric operators through the detector and the trainer (``qry_photometric_chain`` /
``spp_photometric_chain``) against the same code fed the host-prepared batch of ``fewshot_ds.augment_query_chain`` and
``fewshot_ds.augment_support(photometric_chain=)`` - byte for byte: the losses of ``forward_train``, the losses and every
trained tensor of ``Trainer.step``, with and without a flip row; which launch a batch of chains makes; the fallback and
the contract errors.  Set-up and helpers are those of test_hip_spp_augment_e2e.py: MNISTISEG at network size 128,
queries at source sizes (150, 131) and (101, 77), six support instances cut to S = 96."""
import contextlib

import numpy as np
import pytest
import torch

import test_hip_spp_augment_e2e as sa
from fgn_amd import fewshot_ds as fd
from fgn_amd import ops
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

NET, SPP, NK, SIZES = sa.NET, sa.SPP, sa.NK, sa.QRY_SIZES
HUE, SAT, BRI, GAUSS, BLUR, NONE = (4, 50, 0), (5, -60, 0), (6, 30, 0), (1, 2.0, 9), (3, 1.5, 0), (0, 0, 0)
FLIP, STAY = sa.row(flip=1), sa.row()
# image 0: COCO's form, hue then blur; image 1: noise, brightness, blur
QRY_CHAIN = np.array([[HUE, BLUR, NONE], [GAUSS, BRI, BLUR]], np.float64)
# per episode and instance: [hue, blur], [saturation, brightness], neutral | [noise, blur], blur alone, [brightness, blur]
SPP_CHAIN = np.array([[[HUE, BLUR], [SAT, BRI], [NONE, NONE]], [[GAUSS, BLUR], [NONE, BLUR], [BRI, (3, 0.7, 0)]]], np.float64)
QRY_FLIP = np.array([FLIP, STAY], np.float64)
SPP_FLIP = np.array([[FLIP, STAY, FLIP], [STAY, FLIP, STAY]], np.float64)
DROP = ('qry_resize_to', 'qry_augment', 'qry_photometric', 'qry_photometric_chain', 'spp_augment', 'spp_photometric',
        'spp_photometric_chain', 'spp_crop_to', 'spp_fill_ratio', 'crop_square')
ROW_KEYS = ('qry_augment', 'qry_photometric', 'qry_photometric_chain', 'spp_augment', 'spp_photometric',
            'spp_photometric_chain')


def _host_sample(s: dict) -> dict:
    """The loader's route: the chain folds on the host - ``augment_query_chain`` on the source query, ``support_from_source``
    and ``augment_support`` per instance - a network-size sample with ready S x S supports for the uint8 path."""
    if s.get('qry_photometric') is not None:
        img, boxes, masks = fd.augment_query_full(s['qry_img'].numpy(), s['qry_bboxes'], s['qry_isegmaps'], NET, NET,
                                                  s.get('qry_augment'), s['qry_photometric'])
    else:
        img, boxes, masks = fd.augment_query_chain(s['qry_img'].numpy(), s['qry_bboxes'], s['qry_isegmaps'], NET, NET,
                                                   s.get('qry_augment'), s.get('qry_photometric_chain'))
    geo, one, chain = s.get('spp_augment'), s.get('spp_photometric'), s.get('spp_photometric_chain')
    made = []
    for i, (im, mk, bb) in enumerate(zip(s['spp_imgs'], s['spp_isegmaps'], s['spp_bboxes'])):
        crop, box, mask = fd.support_from_source(im.numpy(), bb, mk, s['spp_crop_to'], s['spp_fill_ratio'], s['crop_square'])
        made.append(fd.augment_support(crop, box, mask, None if geo is None else geo[i], None if one is None else one[i],
                                       photometric_chain=None if chain is None else chain[i]))
    out = {k: v for k, v in s.items() if k not in DROP}
    out.update(qry_img=torch.from_numpy(np.ascontiguousarray(img)), qry_bboxes=boxes, qry_isegmaps=masks,
               spp_imgs=torch.from_numpy(np.stack([np.ascontiguousarray(c) for c, _, _ in made])),
               spp_bboxes=np.stack([b for _, b, _ in made]).astype(np.float32),
               spp_isegmaps=np.stack([np.asarray(m, bool) for _, _, m in made]))
    return out


def _pair(ds, **rows):
    """(source batch carrying ``rows``, host-prepared batch) of two episodes: source-size queries of two sizes and
    supports as their source images.  ``rows``: any of ``ROW_KEYS``, per episode."""
    assert set(rows) <= set(ROW_KEYS)
    src = []
    for i in range(2):
        s = sa._cut(sa._query(ds[i], SIZES[i], True), i)
        for key, v in rows.items():
            if v is not None:
                s[key] = np.asarray(v[i], np.float64)
        src.append(s)
    host = collate([_host_sample(s) for s in src])
    imgs = [s.pop('qry_img') for s in src]                                          # (images of two sizes: a list)
    bs = collate(src)
    bs['qry_img'] = imgs
    assert not any(k in host for k in DROP) and tuple(host['spp_imgs'].shape) == (2, NK, SPP, SPP, 3)
    assert tuple(host['qry_img'].shape) == (2, NET, NET, 3) and host['qry_img'].dtype == torch.uint8
    return bs, host


@pytest.fixture(scope='module')
def ds():
    return fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=sa.N_WAYS, k_shots=sa.K_SHOTS, n_imgs=8,
                                        img_size=sa.POOL, spp_img_size=SPP, raw_uint8=True, spp_source=True)


@pytest.fixture(scope='module')
def model(ds):
    m = sa._model()
    m.set_input_norm(**ds.input_norm)
    return m


@contextlib.contextmanager
def _counted():
    """The calls into the two photometric entries of ``ops``, in order."""
    names = ('photometric_u8', 'photometric_chain_u8')
    calls, real = [], {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, (lambda name: lambda *a, **k: calls.append(name) or real[name](*a, **k))(n))
    try:
        yield calls
    finally:
        for n in names:
            setattr(ops, n, real[n])


@pytest.fixture(scope='module')
def plain(ds, model):
    """The losses of the batch without any row, which launches no photometric pass: computed once, shared."""
    with _counted() as calls:
        losses = sa._losses(model, _pair(ds)[0])
    assert calls == []
    return losses


def _flips(flip: bool) -> dict:
    return dict(qry_augment=QRY_FLIP, spp_augment=SPP_FLIP) if flip else {}


@pytest.mark.parametrize('flip', (False, True), ids=('chains', 'flip+chains'))
def test_forward_train_with_chains_gives_the_losses_of_the_host_prepared_batch(ds, model, plain, flip):
    bs, host = _pair(ds, qry_photometric_chain=QRY_CHAIN, spp_photometric_chain=SPP_CHAIN, **_flips(flip))
    assert tuple(bs['qry_photometric_chain'].shape) == (2, 3, 3) and tuple(bs['spp_photometric_chain'].shape) == (2, NK, 2, 3)
    with _counted() as calls:
        got = sa._losses(model, bs)
    assert calls == ['photometric_chain_u8', 'photometric_chain_u8']                   # the queries, the six instances
    sa._same_losses(sa._losses(model, host), got)
    assert sa._bytes(got) != sa._bytes(plain)
    # each side alone is seen, and equal to its host batch
    for key, rows in (('qry_photometric_chain', QRY_CHAIN), ('spp_photometric_chain', SPP_CHAIN)):
        b2, h2 = _pair(ds, **{key: rows}, **_flips(flip))
        with _counted() as calls:
            half = sa._losses(model, b2)
        assert calls == ['photometric_chain_u8']
        sa._same_losses(sa._losses(model, h2), half)
        assert sa._bytes(half) != sa._bytes(got)
    # rows as arrays
    kw = {k: v for k, v in bs.items() if k not in ('qry_photometric_chain', 'spp_photometric_chain')}
    sa._same_losses(got, sa._losses(model, dict(kw, qry_photometric_chain=QRY_CHAIN, spp_photometric_chain=SPP_CHAIN)))


@pytest.mark.parametrize('flip', (False, True), ids=('chains', 'flip+chains'))
def test_trainer_step_with_chains_is_the_step_on_the_host_prepared_batch(ds, flip):
    bs, host = _pair(ds, qry_photometric_chain=QRY_CHAIN, spp_photometric_chain=SPP_CHAIN, **_flips(flip))
    a, b = sa._step(host, ds), sa._step(bs, ds)
    sa._same_losses(a[0], b[0])
    assert set(a[1]) == set(b[1]) and len(a[1]) > 0
    for k in a[1]:
        assert a[1][k].numpy().tobytes() == b[1][k].numpy().tobytes(), k
    assert any(float(v.abs().max()) > 0 for k, v in a[1].items() if k.startswith('state/'))     # the step trained


def test_chains_of_one_active_operator_make_the_single_operator_launch(ds, model, plain):
    """At most one active operator per image after compaction: exactly ``qry_photometric``'s launch and bytes - the new
    kernel is not used.  All-neutral chains launch nothing and equal the call without the argument."""
    single = np.array([BLUR, HUE], np.float64)
    chain = np.array([[NONE, BLUR, NONE], [HUE, NONE, (3, 0, 0)]], np.float64)          # (a blur of sigma 0 is neutral)
    with _counted() as calls:
        want = sa._losses(model, _pair(ds, qry_photometric=single)[0])
    assert calls == ['photometric_u8']
    bs, host = _pair(ds, qry_photometric_chain=chain)
    with _counted() as calls:
        got = sa._losses(model, bs)
    assert calls == ['photometric_u8']
    sa._same_losses(want, got)
    sa._same_losses(sa._losses(model, host), got)
    assert sa._bytes(got) != sa._bytes(plain)
    spp_single = np.array([[BLUR, HUE, NONE], [NONE, NONE, GAUSS]], np.float64)
    spp_chain = np.array([[[BLUR, NONE], [NONE, HUE], [NONE, NONE]], [[NONE, NONE], [NONE, NONE], [GAUSS, NONE]]], np.float64)
    with _counted() as calls:
        want = sa._losses(model, _pair(ds, spp_photometric=spp_single)[0])
        got = sa._losses(model, _pair(ds, spp_photometric_chain=spp_chain)[0])
    assert calls == ['photometric_u8', 'photometric_u8']
    sa._same_losses(want, got)
    with _counted() as calls:
        for rows in (dict(qry_photometric_chain=np.zeros((2, 1, 3))), dict(spp_photometric_chain=np.zeros((2, NK, 3, 3))),
                     dict(qry_photometric_chain=np.array([[NONE, (3, 0, 0)], [(6, 0, 9), NONE]], np.float64),
                          spp_photometric_chain=np.zeros((2, NK, 1, 3)))):
            sa._same_losses(plain, sa._losses(model, _pair(ds, **rows)[0]))
    assert calls == []


def test_a_fallen_back_image_or_instance_is_used_without_its_chain(ds, model, plain):
    gone = sa.row(tx=-500)                                                             # every box leaves the frame
    qry_geo = np.array([gone, STAY], np.float64)
    chain = QRY_CHAIN.copy()
    chain[1] = NONE
    bs, host = _pair(ds, qry_augment=qry_geo, qry_photometric_chain=chain)
    rec, _ = fd.augment_plan(qry_geo[0], bs['qry_bboxes'][0].numpy(), SIZES[0], (NET, NET))
    assert not rec[2:6].any()
    with _counted() as calls:
        got = sa._losses(model, bs)
    assert calls == []                                                                 # all neutral after the fallback
    sa._same_losses(plain, got)
    sa._same_losses(plain, sa._losses(model, host))
    assert sa._bytes(sa._losses(model, _pair(ds, qry_photometric_chain=chain)[0])) != sa._bytes(plain)
    # one instance of six falls back: that instance alone loses its chain
    spp_geo = SPP_FLIP.copy()
    spp_geo[0, 0] = gone
    bs, host = _pair(ds, spp_augment=spp_geo, spp_photometric_chain=SPP_CHAIN)
    got = sa._losses(model, bs)
    sa._same_losses(sa._losses(model, host), got)
    spp_geo[0, 0], neutral0 = STAY, SPP_CHAIN.copy()
    neutral0[0, 0] = NONE
    sa._same_losses(sa._losses(model, _pair(ds, spp_augment=spp_geo, spp_photometric_chain=neutral0)[0]), got)


def test_contract_errors_queue_nothing(ds, model):
    m = model
    bs, host = _pair(ds, qry_photometric_chain=QRY_CHAIN, spp_photometric_chain=SPP_CHAIN)
    base = {k: v for k, v in bs.items() if k not in ROW_KEYS}

    def qry_with(*chain):
        return np.array([chain, [NONE] * len(chain)], np.float64)

    def spp_with(*chain):
        c = np.zeros((2, NK, len(chain), 3))
        c[1, 2] = chain
        return c
    refuse = sa._refused_before_anything_is_queued
    with _counted() as calls:
        for name, rows in (('qry_photometric_chain', QRY_CHAIN), ('spp_photometric_chain', SPP_CHAIN)):
            with refuse(m, name):                                                   # no source pixels to work on
                m.forward_train(**host, **{name: rows})
        with refuse(m, 'qry_photometric and qry_photometric_chain'):               # one argument in two forms
            m.forward_train(**base, qry_photometric=np.zeros((2, 3)), qry_photometric_chain=QRY_CHAIN)
        with refuse(m, 'spp_photometric and spp_photometric_chain'):
            m.forward_train(**base, spp_photometric=np.zeros((2, NK, 3)), spp_photometric_chain=SPP_CHAIN)
        for bad in (QRY_CHAIN[:1], QRY_CHAIN[0], QRY_CHAIN[..., :2], np.zeros((2, 0, 3)), np.zeros((2, 4, 3)),
                    torch.from_numpy(QRY_CHAIN)[..., None], qry_with(BLUR, HUE), qry_with(BLUR, BLUR),
                    qry_with(BLUR, NONE, GAUSS), qry_with(HUE, (7, 0, 0)), qry_with((1, 2.5, 0), BLUR),
                    qry_with(HUE, (np.nan, 0, 0)), qry_with(HUE, (3, 5.0, 0))):     # 5.86 source pixels: a radius of 18
            with refuse(m, 'qry_photometric_chain'):
                m.forward_train(**base, qry_photometric_chain=bad)
        for bad in (SPP_CHAIN[:1], SPP_CHAIN[:, :2], SPP_CHAIN[..., :2], SPP_CHAIN.reshape(-1, 2, 3), np.zeros((2, NK, 4, 3)),
                    spp_with(BLUR, HUE), spp_with(BLUR, BLUR), spp_with(HUE, (7, 0, 0)), spp_with(HUE, (3, 5.4, 0))):
            for extra in ({}, {'spp_augment': SPP_FLIP}):
                with refuse(m, 'spp_photometric_chain'):
                    m.forward_train(**base, **extra, spp_photometric_chain=bad)
        for name in ('qry_photometric_chain', 'spp_photometric_chain'):                 # the test is without augmentation
            with refuse(m, name):
                m.simple_test(**base, **{name: bs[name]}, rescale=True)
        with refuse(m, 'spp_photometric_chain'):
            m.encode_supports(bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], spp_crop_to=SPP,
                              spp_photometric_chain=SPP_CHAIN)
        with refuse(m, 'spp_photometric_chain'):
            m.detect_device(bs['qry_img'], bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], bs['img_shape'],
                            qry_resize_to=bs['qry_resize_to'], spp_crop_to=SPP, spp_photometric_chain=SPP_CHAIN)
        # the trainer goes through the same front
        from fgn_amd.train import Trainer
        m2 = sa._model()
        m2.set_input_norm(**ds.input_norm)
        tr = Trainer(m2)
        for name, b in (('qry_photometric_chain', dict(host, qry_photometric_chain=QRY_CHAIN)),
                        ('spp_photometric_chain', dict(bs, spp_photometric_chain=spp_with(BLUR, HUE)))):
            with refuse(m2, name):
                tr.step(b)
            assert m2._tape is None and tr.n_steps == 0
    assert calls == []
