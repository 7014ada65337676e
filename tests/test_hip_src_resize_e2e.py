"""Source-size queries through the detector (``qry_resize_to``) against the same detector fed
``fewshot_ds.resize_query`` of the same inputs through the uint8 path - byte for byte: eager, one graph for several
source sizes, pinned inputs into the static slot, cached support code, both backbone launch forms, overlap counts,
training losses and the contract errors."""
import contextlib

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.episodes import collate

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, POOL, NET, SPP = 3, 2, 160, 128, 64
KEYS = ('dt_scores', 'dt_bboxes', 'dt_cat_ids')
OVERLAP = ('dt_gt_inter', 'dt_area', 'gt_area')


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


def _host_resized(sample: dict) -> dict:
    """The loader's route: ``resize_query`` on the host, a network-size sample for the existing uint8 path."""
    img, boxes, masks = fd.resize_query(sample['qry_img'].numpy(), sample['qry_bboxes'], sample['qry_isegmaps'], NET, NET)
    out = dict(sample)
    out.pop('qry_resize_to')
    out.update(qry_img=torch.from_numpy(np.ascontiguousarray(img)), qry_bboxes=boxes, qry_isegmaps=masks)
    return out


class _Env:
    """One model, the pool dataset, and per (first sample, sizes) the source-size batch with its host-resized twin."""

    def __init__(self):
        self.ds = fd.ClutteredCharsFewShotISEG(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8,
                                               img_size=POOL, spp_img_size=SPP, raw_uint8=True)
        self.model = _model()
        self._want = {}

    def reset(self):
        m = self.model
        m.use_graphs = False
        m.transfer_mode = 0
        m.match_on_device = False
        m.use_merged_backbone = m.use_merged_support_head = True
        m.query_source_capacity = 3 * POOL * POOL
        m.set_input_norm(**self.ds.input_norm)
        return m

    def pair(self, first, sizes):
        """(source-size batch, host-resized batch).  The source images are one [B,h,w,3] tensor when the sizes agree and
        a list of [h_i,w_i,3] tensors when they do not."""
        src = [_crop(self.ds[first + i], s) for i, s in enumerate(sizes)]
        host = collate([_host_resized(s) for s in src])
        imgs = [s.pop('qry_img') for s in src]
        bs = collate(src)
        bs['qry_img'] = torch.stack(imgs) if len(set(sizes)) == 1 else imgs
        assert tuple(bs['qry_resize_to'].shape) == (len(sizes), 2)
        return bs, host

    def want(self, first, sizes):
        """Results of the host-resized batch through the existing uint8 path, eagerly, computed once."""
        key = (first, tuple(sizes))
        if key not in self._want:
            m = self.reset()
            self._want[key] = m.simple_test(**self.pair(first, sizes)[1], rescale=True)
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
        assert a['qry_bboxes'].dtype == b['qry_bboxes'].dtype and a['qry_bboxes'].tobytes() == b['qry_bboxes'].tobytes()
        assert np.array_equal(a['qry_img_shape'], b['qry_img_shape'])


@pytest.mark.parametrize('first,sizes', [(0, [(150, 131)]), (1, [(101, 77)]), (2, [(128, 128)]), (3, [(64, 160)]),
                                         (0, [(150, 131), (101, 77)]), (2, [(64, 160), (64, 160)])])
def test_simple_test_on_source_pixels_is_bytewise_the_host_resize(env, first, sizes):
    want = env.want(first, sizes)
    m = env.reset()
    bs, _ = env.pair(first, sizes)
    assert isinstance(bs['qry_img'], list) == (len(set(sizes)) > 1)
    _same(want, m.simple_test(**bs, rescale=True))
    # (H, W) as a pair and img_shape left to its default
    _same(want, m.simple_test(**{k: v for k, v in bs.items() if k not in ('img_shape', 'qry_resize_to')},
                              qry_resize_to=(NET, NET), rescale=True))


def test_separate_backbone_launches_and_overlap_counts(env):
    sizes = [(150, 131), (101, 77)]
    bs, host = env.pair(0, sizes)
    m = env.reset()
    m.match_on_device = True
    m.use_merged_backbone = m.use_merged_support_head = False
    want = m.simple_test(**host, rescale=True)
    assert all(k in want[0] for k in OVERLAP)
    _same(want, m.simple_test(**bs, rescale=True), overlap=True)
    m.use_merged_backbone = m.use_merged_support_head = True
    _same(m.simple_test(**host, rescale=True), m.simple_test(**bs, rescale=True), overlap=True)


def test_one_graph_replays_batches_of_different_source_sizes(env):
    cases = [(0, [(150, 131)]), (3, [(64, 160)]), (1, [(101, 77)])]
    want = [env.want(*c) for c in cases]
    m = env.reset()
    m.use_graphs = True
    for rep in range(2):
        for w, c in zip(want, cases):
            _same(w, m.simple_test(**env.pair(*c)[0], rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    assert ge.static['qry_src'].dtype == torch.uint8 and tuple(ge.static['qry_src'].shape) == (1, 3 * POOL * POOL)
    assert ge.static['qry_src_hw'].dtype == torch.int32 and 'qry_img' not in ge.static
    # B = 2 with differing sizes in one batch, then the same graph with other sizes
    m.match_on_device = True
    a, b = (0, [(150, 131), (101, 77)]), (2, [(64, 160), (128, 128)])
    m.use_graphs = False
    wa, wb = m.simple_test(**env.pair(*a)[1], rescale=True), m.simple_test(**env.pair(*b)[1], rescale=True)
    m.use_graphs = True
    for w, c in ((wa, a), (wb, b), (wa, a)):
        _same(w, m.simple_test(**env.pair(*c)[0], rescale=True), overlap=True)
    assert len(m._graphs) == 2


def test_pinned_source_pixels_go_straight_into_the_static_slot(env):
    cases = [(0, [(150, 131)]), (3, [(64, 160)])]
    want = [env.want(*c) for c in cases]
    m = env.reset()
    m.use_graphs = True
    m.transfer_mode = 3
    pin = lambda v: v.pin_memory() if isinstance(v, torch.Tensor) else [t.pin_memory() for t in v] \
        if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v
    b0, b1 = ({k: pin(v) for k, v in env.pair(*c)[0].items()} for c in cases)
    _same(want[0], m.simple_test(**b0, rescale=True))
    _same(want[1], m.simple_test(**b1, rescale=True))
    _same(want[0], m.simple_test(**b0, rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    torch.cuda.synchronize()
    n = 150 * 131 * 3
    assert torch.equal(ge.static['qry_src'][0, :n].cpu(), b0['qry_img'].reshape(-1))
    assert ge.static['qry_src_hw'].cpu().tolist() == [[150, 131]]
    # the upload itself: the static tensors come back, holding the other batch
    dev, main = torch.device('cuda', torch.cuda.current_device()), torch.cuda.current_stream()
    source = m._source_query(b1['qry_img'], b1['qry_resize_to'], None, graphed=True)
    from fgn_amd.detector import _InputForm
    out, _, _ = m._upload({'spp_imgs': b1['spp_imgs']}, None, dev, main, into=ge.static,
                          form=_InputForm(source=source))
    assert out['qry_src'] is ge.static['qry_src'] and out['qry_src_hw'] is ge.static['qry_src_hw']
    torch.cuda.synchronize()
    assert torch.equal(ge.static['qry_src'][0, :64 * 160 * 3].cpu(), b1['qry_img'].reshape(-1))
    assert ge.static['qry_src_hw'].cpu().tolist() == [[64, 160]]
    m.transfer_mode = 0


def test_support_code_with_source_queries(env):
    m = env.reset()
    sizes = [(150, 131), (101, 77)]
    bs, host = env.pair(4, sizes)
    q = lambda b: {k: v for k, v in b.items() if k not in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps')}
    code = m.encode_supports(host['spp_imgs'], host['spp_bboxes'], host['spp_isegmaps'])
    want = m.simple_test(**q(host), support_code=code, rescale=True)
    _same(want, m.simple_test(**q(bs), support_code=code, rescale=True))
    m.use_graphs = True
    _same(want, m.simple_test(**q(bs), support_code=code, rescale=True))
    _same(want, m.simple_test(**q(bs), support_code=code, rescale=True))


def test_forward_train_on_source_pixels_gives_the_same_losses():
    env = _Env()
    m = env.reset()
    bs, host = env.pair(0, [(150, 131), (101, 77)])
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
    names = ('_upload', '_upload_source', '_resized_masks', '_detect_eager', '_detect_graphed', '_stem_input')
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
    bs, _ = env.pair(0, [(150, 131)])
    m.simple_test(**bs, rescale=True)
    graphs = dict(m._graphs)
    assert len(graphs) == 1
    u8 = bs['qry_img']
    big = dict(bs, qry_img=torch.zeros((1, POOL + 1, POOL, 3), dtype=torch.uint8),
               qry_isegmaps=[torch.zeros((1, POOL + 1, POOL), dtype=torch.bool)])
    bad = [dict(bs, qry_img=u8.float()),                                            # a float query
           dict(bs, qry_img=u8.permute(0, 3, 1, 2).contiguous()),                   # NCHW
           dict(bs, img_shape=torch.tensor([[NET, NET + 16, 3]])),                  # img_shape != (H, W)
           big]                                                                     # above the slot, under graphs
    for b in bad:
        with _refused_before_anything_is_queued(m):
            m.simple_test(**b, rescale=True)
        with _refused_before_anything_is_queued(m):
            m.detect_device(b['qry_img'], b['spp_imgs'], b['spp_bboxes'], b['spp_isegmaps'], b['img_shape'],
                            qry_isegmaps=b['qry_isegmaps'], qry_resize_to=b['qry_resize_to'])
    with _refused_before_anything_is_queued(m) as err:
        m.simple_test(**big, rescale=True)
    assert 'query_source_capacity' in str(err.value)
    assert m._graphs == graphs
    # eagerly the slot is as large as the batch needs
    m.use_graphs = False
    assert len(m.simple_test(**big, rescale=True)) == 1
    for b in bad[:3]:
        with _refused_before_anything_is_queued(m):
            m.forward_train(**b)
    # no table
    m.set_input_norm()
    for graphs_on in (False, True):
        m.use_graphs = graphs_on
        with _refused_before_anything_is_queued(m) as err:
            m.simple_test(**bs, rescale=True)
        assert 'set_input_norm' in str(err.value)
    with _refused_before_anything_is_queued(m) as err:
        m.forward_train(**bs)
    assert 'set_input_norm' in str(err.value)
    assert m._graphs == {}


def test_without_qry_resize_to_pixels_equal_the_float_path(env):
    """The default path of one network-size batch, as before: decoded pixels against the loader's float tensors."""
    kw = dict(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=2, img_size=NET, spp_img_size=SPP)
    bf = collate([fd.ClutteredCharsFewShotISEG(**kw)[0]])
    bu = collate([fd.ClutteredCharsFewShotISEG(**kw, raw_uint8=True)[0]])
    m = env.reset()
    got = m.simple_test(**bu, rescale=True)
    m.set_input_norm()
    want = m.simple_test(**bf, rescale=True)
    _same(want, got)
