"""Supports cut from their source images through the detector (``spp_crop_to``) against the same detector fed
host-built ``fewshot_ds.support_from_source`` crops through the existing uint8 path - byte for byte: eager, cached
support code, one graph for support sets of differing source sizes, pinned inputs into the static slots, together with
``qry_resize_to``, overlap counts, training losses and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
NK = N_WAYS * K_SHOTS
KEYS = ('dt_scores', 'dt_bboxes', 'dt_cat_ids')
OVERLAP = ('dt_gt_inter', 'dt_area', 'gt_area')
SPP_KEYS = ('spp_imgs', 'spp_bboxes', 'spp_isegmaps', 'spp_crop_to', 'spp_fill_ratio', 'crop_square')


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
    else:
        assert (h, w) == (NET, NET)
    return out


def _cut(sample: dict, k) -> dict:
    """The supports' source images cut to windows around their instances, margins chosen by (instance, ``k``): the
    images of one support set get differing sizes, two values of k give differing sets, and the crops' context leaves
    the cut images (reflection).  ``k`` None: the 160^2 images as they are."""
    if k is None:
        return sample
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
    """The loader's route: ``support_from_source`` per instance on the host, ready crops for the existing uint8 path."""
    made = [fd.support_from_source(im.numpy(), bb, mk, sample['spp_crop_to'], sample['spp_fill_ratio'], sample['crop_square'])
            for im, mk, bb in zip(sample['spp_imgs'], sample['spp_isegmaps'], sample['spp_bboxes'])]
    out = {k: v for k, v in sample.items() if k not in SPP_KEYS[3:]}
    out.update(spp_imgs=torch.from_numpy(np.stack([c for c, _, _ in made])), spp_bboxes=np.stack([b for _, b, _ in made]),
               spp_isegmaps=np.stack([m for _, _, m in made]))
    return out


class _Env:
    """One model, the pool dataset with source supports, and per case the source batch with its host-built twin."""

    def __init__(self):
        self.ds = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8,
                                               img_size=POOL, spp_img_size=SPP, raw_uint8=True, spp_source=True)
        self.model = _model()
        self._want = {}

    def reset(self):
        m = self.model
        m.use_graphs = False
        m.transfer_mode = 0
        m.match_on_device = False
        m.use_merged_backbone = m.use_merged_support_head = True
        m.query_source_capacity = 3 * POOL * POOL
        m.support_source_capacity = 3 * POOL * POOL
        m.set_input_norm(**self.ds.input_norm)
        return m

    def pair(self, first, cuts, size=(NET, NET), resize=False):
        """(source-support batch, host-built batch) of ``len(cuts)`` episodes."""
        src = [_cut(_query(self.ds[first + i], size, resize), k) for i, k in enumerate(cuts)]
        return collate(src), collate([_host_supports(s) for s in src])

    def want(self, first, cuts):
        """Results of the host-built batch through the existing uint8 path, eagerly, computed once."""
        key = (first, tuple(cuts))
        if key not in self._want:
            m = self.reset()
            self._want[key] = m.simple_test(**self.pair(first, cuts)[1], rescale=True)
        return self._want[key]


@pytest.fixture(scope='module')
def env():
    return _Env()


def _same(want, got, overlap=False):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert len(a['dt_scores']) > 0
        for k in KEYS + (OVERLAP if overlap else ()):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        assert a['dt_isegmaps_rle'] == b['dt_isegmaps_rle']
        assert len(a['qry_isegmaps_rle']) > 0 and a['qry_isegmaps_rle'] == b['qry_isegmaps_rle']
        assert np.array_equal(a['qry_img_shape'], b['qry_img_shape'])
        assert np.array_equal(a['spp_insts_ids'], b['spp_insts_ids'])


def test_the_cut_support_sets_differ_in_size(env):
    bs, host = env.pair(0, [0, 1])
    sizes = [[tuple(t.shape[:2]) for t in lst] for lst in bs['spp_imgs']]
    assert len(set(sizes[0])) > 1 and sizes[0] != sizes[1] and all(max(s) < POOL for lst in sizes for s in lst)
    assert tuple(host['spp_imgs'].shape) == (2, NK, SPP, SPP, 3) and host['spp_imgs'].dtype == torch.uint8
    assert bs['spp_crop_to'] == SPP and 'spp_crop_to' not in host


@pytest.mark.parametrize('first,cuts', [(0, [None]), (1, [0]), (2, [1]), (0, [0, 1]), (3, [2, None])])
def test_simple_test_on_source_supports_is_bytewise_the_host_crops(env, first, cuts):
    want = env.want(first, cuts)
    m = env.reset()
    bs, _ = env.pair(first, cuts)
    _same(want, m.simple_test(**bs, rescale=True))
    if len(cuts) == 1:                  # one support set as a plain list, the cut's other arguments left to their defaults
        flat = dict(bs, spp_imgs=bs['spp_imgs'][0], spp_isegmaps=bs['spp_isegmaps'][0], spp_bboxes=bs['spp_bboxes'][0])
        _same(want, m.simple_test(**{k: v for k, v in flat.items() if k not in SPP_KEYS[4:]}, rescale=True))


def test_separate_launches_and_overlap_counts(env):
    bs, host = env.pair(0, [0, 1])
    m = env.reset()
    m.match_on_device = True
    m.use_merged_backbone = m.use_merged_support_head = False
    want = m.simple_test(**host, rescale=True)
    assert all(k in want[0] for k in OVERLAP)
    _same(want, m.simple_test(**bs, rescale=True), overlap=True)
    m.use_merged_backbone = m.use_merged_support_head = True
    _same(m.simple_test(**host, rescale=True), m.simple_test(**bs, rescale=True), overlap=True)


def test_encode_supports_from_sources_gives_the_same_code(env):
    m = env.reset()
    bs, host = env.pair(4, [0, 2])
    q = lambda b: {k: v for k, v in b.items() if k not in SPP_KEYS}
    want_code = m.encode_supports(host['spp_imgs'], host['spp_bboxes'], host['spp_isegmaps'])
    code = m.encode_supports(bs['spp_imgs'], bs['spp_bboxes'], bs['spp_isegmaps'], spp_crop_to=SPP)
    for k in ('vec', 'S', 'cat_mean_mp', 'spp_masks', 'spp_xyxy'):
        assert torch.equal(code[k].contiguous().view(torch.uint8), want_code[k].contiguous().view(torch.uint8)), k
    want = m.simple_test(**q(host), support_code=want_code, rescale=True)
    _same(want, m.simple_test(**q(bs), support_code=code, rescale=True))
    m.use_graphs = True
    _same(want, m.simple_test(**q(bs), support_code=code, rescale=True))
    _same(want, m.simple_test(**bs, support_code=code, rescale=True))       # beside a code the source supports are ignored


def test_one_graph_replays_support_sets_of_different_source_sizes(env):
    cases = [(1, [0]), (2, [1]), (0, [None])]
    want = [env.want(*c) for c in cases]
    m = env.reset()
    m.use_graphs = True
    for rep in range(2):
        for w, c in zip(want, cases):
            _same(w, m.simple_test(**env.pair(*c)[0], rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    assert ge.static['spp_src'].dtype == torch.uint8 and tuple(ge.static['spp_src'].shape) == (NK, 3 * POOL * POOL)
    assert tuple(ge.static['spp_msk'].shape) == (NK, POOL * POOL) and ge.static['spp_msk'].dtype == torch.uint8
    assert ge.static['spp_rec'].dtype == torch.int32 and tuple(ge.static['spp_rec'].shape) == (NK, 16)
    assert 'spp_imgs' not in ge.static and 'spp_isegmaps' not in ge.static
    # B = 2, then the same graph with other support sets; the overlap counts ride along
    m.match_on_device = True
    a, b = (0, [0, 1]), (3, [2, None])
    m.use_graphs = False
    wa, wb = m.simple_test(**env.pair(*a)[1], rescale=True), m.simple_test(**env.pair(*b)[1], rescale=True)
    m.use_graphs = True
    for w, c in ((wa, a), (wb, b), (wa, a)):
        _same(w, m.simple_test(**env.pair(*c)[0], rescale=True), overlap=True)
    assert len(m._graphs) == 2


def _pin(v):
    if isinstance(v, torch.Tensor):
        return v.pin_memory()
    return [_pin(t) for t in v] if isinstance(v, list) else v


def test_pinned_inputs_go_straight_into_the_static_slots(env):
    cases = [(1, [0]), (2, [1])]
    want = [env.want(*c) for c in cases]
    m = env.reset()
    m.use_graphs = True
    m.transfer_mode = 3
    b0, b1 = ({k: _pin(v) for k, v in env.pair(*c)[0].items()} for c in cases)
    _same(want[0], m.simple_test(**b0, rescale=True))
    _same(want[1], m.simple_test(**b1, rescale=True))
    _same(want[0], m.simple_test(**b0, rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    torch.cuda.synchronize()
    def holds(sp):
        for i in range(NK):
            assert torch.equal(ge.static['spp_src'][i, :sp['flats'][i].numel()].cpu(), sp['flats'][i]), i
            assert torch.equal(ge.static['spp_msk'][i, :sp['mflats'][i].numel()].cpu(), sp['mflats'][i]), i
        assert torch.equal(ge.static['spp_rec'].cpu(), sp['rec'])
    holds(m._source_supports(b0['spp_imgs'], b0['spp_bboxes'], b0['spp_isegmaps'], SPP, graphed=True))
    # the upload itself: the static tensors come back, holding the other support set
    dev, main = torch.device('cuda', torch.cuda.current_device()), torch.cuda.current_stream()
    sp1 = m._source_supports(b1['spp_imgs'], b1['spp_bboxes'], b1['spp_isegmaps'], SPP, graphed=True)
    from fgn_amd.detector import _InputForm
    out, _, _ = m._upload({'qry_img': b1['qry_img'], 'spp_bboxes': sp1['boxes'].pin_memory(),
                           'spp_rec': sp1['rec'].pin_memory()}, None, dev, main, into=ge.static,
                          form=_InputForm(spp_source=sp1))
    for k in ('qry_img', 'spp_bboxes', 'spp_rec', 'spp_src', 'spp_msk'):
        assert out[k] is ge.static[k], k
    torch.cuda.synchronize()
    holds(sp1)
    m.transfer_mode = 0


def test_together_with_source_size_queries_and_results_at_source(env):
    m = env.reset()
    bs, host = env.pair(0, [0, 1], size=(150, 131), resize=True)
    assert tuple(bs['qry_resize_to'].shape) == (2, 2) and tuple(bs['qry_img'].shape) == (2, 150, 131, 3)
    want = m.simple_test(**host, rescale=True)
    _same(want, m.simple_test(**bs, rescale=True))
    m.match_on_device = True
    want_src = m.simple_test(**host, rescale=True, results_at_source=True)
    _same(want_src, m.simple_test(**bs, rescale=True, results_at_source=True), overlap=True)
    m.use_graphs = True
    _same(want_src, m.simple_test(**bs, rescale=True, results_at_source=True), overlap=True)
    _same(want_src, m.simple_test(**env.pair(0, [0, 1], size=(150, 131), resize=True)[0], rescale=True,
                                  results_at_source=True), overlap=True)
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    assert 'qry_src' in ge.static and 'spp_src' in ge.static and 'qry_img' not in ge.static


def test_forward_train_on_source_supports_gives_the_same_losses():
    env = _Env()
    m = env.reset()
    bs, host = env.pair(0, [0, 1])
    losses = []
    for b in (host, bs):
        m._PT = None                                    # fresh running statistics
        g = torch.Generator().manual_seed(3)
        torch.manual_seed(3)
        losses.append(m.forward_train(**b, perm_fn=lambda n: torch.randperm(n, generator=g)))
    val = lambda v: torch.as_tensor(v[0] if isinstance(v, list) else v).detach().cpu().reshape(-1)
    assert set(losses[0]) == set(losses[1])
    for k in losses[0]:
        a, b = val(losses[0][k]), val(losses[1][k])
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), k
    assert all(np.isfinite(float(val(v)[0])) for v in losses[0].values())
    assert float(val(losses[0]['loss_rpn_cls'])[0]) > 0 and float(val(losses[0]['loss_cls'])[0]) > 0


@contextlib.contextmanager
def _refused_before_anything_is_queued(m):
    """A ValueError inside, raised before the detector uploads, allocates on the device or launches: every step that
    queues work is replaced by one that fails the test, and the device allocator's byte count does not move."""
    def boom(*a, **k):
        raise AssertionError('work was queued before the contract error')
    names = ('_upload', '_upload_supports', '_supports_on_device', '_support_front', '_detect_eager', '_detect_graphed',
             '_stem_input')
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


def test_contract_errors_queue_nothing_and_leave_the_graphs_alone(env):
    m = env.reset()
    m.use_graphs = True
    bs, host = env.pair(0, [0])
    m.simple_test(**bs, rescale=True)
    graphs = dict(m._graphs)
    assert len(graphs) == 1
    imgs, masks, boxes = bs['spp_imgs'][0], bs['spp_isegmaps'][0], bs['spp_bboxes']
    outside = boxes.clone()
    outside[0, 1, 3] = imgs[1].shape[1] + 1
    bad = [dict(bs, spp_imgs=[[t.float() for t in imgs]]),                          # float images
           dict(bs, spp_imgs=[[t.permute(2, 0, 1).contiguous() for t in imgs]]),   # CHW
           dict(bs, spp_imgs=host['spp_imgs']),                                     # ready crops beside spp_crop_to
           dict(bs, spp_isegmaps=[[masks[1]] + masks[1:]]),                         # a mask at another image's size
           dict(bs, spp_bboxes=outside),                                            # a box that leaves its image
           dict(bs, spp_crop_to=(SPP, SPP))]
    for b in bad:
        with _refused_before_anything_is_queued(m):
            m.simple_test(**b, rescale=True)
        with _refused_before_anything_is_queued(m):
            m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                            qry_isegmaps=b['qry_isegmaps'], spp_crop_to=b['spp_crop_to'])
        with _refused_before_anything_is_queued(m):
            m.encode_supports(b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], spp_crop_to=b['spp_crop_to'])
        with _refused_before_anything_is_queued(m):
            m.forward_train(**b)
    m.support_source_capacity = 3 * 20 * 20                                         # above the slot, under graphs only
    with _refused_before_anything_is_queued(m) as err:
        m.simple_test(**bs, rescale=True)
    assert 'support_source_capacity' in str(err.value)
    assert m._graphs == graphs
    m.use_graphs = False
    assert len(m.simple_test(**bs, rescale=True)) == 1                              # eagerly: what the batch needs
    # no table
    m.set_input_norm()
    for graphs_on in (False, True):
        m.use_graphs = graphs_on
        with _refused_before_anything_is_queued(m) as err:
            m.simple_test(**bs, rescale=True)
        assert 'set_input_norm' in str(err.value)
    assert m._graphs == {}


def test_without_spp_crop_to_nothing_new_runs(env):
    """The default path as before: ready crops launch no support_from_source and allocate no window slot."""
    from fgn_amd import ops
    m = env.reset()
    _, host = env.pair(0, [0])
    calls = []
    real = ops.support_from_source
    ops.support_from_source = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        m.use_graphs = True
        m.simple_test(**host, rescale=True)
        assert calls == [] and all('spp_src' not in ge.static for ge in m._graphs.values())
        m.simple_test(**env.pair(0, [0])[0], rescale=True)
        assert len(calls) == 2                          # (the eager pass before the capture, and the capture)
    finally:
        ops.support_from_source = real
