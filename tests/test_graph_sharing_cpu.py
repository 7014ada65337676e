"""Which calls share a captured graph, host side (no GPU): ``FGN._graph_key`` as a partition of calls - pairs that
must replay one graph get equal keys, pairs whose launch sequences differ get different ones - whatever the key is
made of.  The slot tensors of source-size queries and source supports never take part: a graph is keyed by the
configured capacities and the sizes the kernels write, not by what a batch happens to bring."""
from types import SimpleNamespace

import numpy as np
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd.detector import _InputForm

NK = 6


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(3, 2, width_div=2)                    # (the model of tests/test_src_resize_cpu.py, table set)
    m = FGN(3, 2, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
            test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    m.set_input_norm(**fd.ClutteredCharsFewShotISEG(n_imgs=1, img_size=64, spp_img_size=32).input_norm)
    return m


def _key(m, ins, hw, B=1, code=None, source=None, spp_source=None, at_source=False):
    return m._graph_key(ins, [(hw[0], hw[1], 3)] * B, code, None, SimpleNamespace(cuda_stream=0),
                        torch.device('cuda', 0), _InputForm(source, spp_source, at_source))


def _spp_tensors(B=1, S=16):
    return dict(spp_imgs=torch.zeros((B, NK, 3, S, S)), spp_bboxes=torch.zeros((B, NK, 4)),
                spp_isegmaps=torch.zeros((B, NK, S, S), dtype=torch.bool))


def _query(m, h, w, hw=(32, 48)):
    return m._source_query([torch.zeros((h, w, 3), dtype=torch.uint8)], hw, None, graphed=True)


def _supports(m, S, grow=0):
    imgs = [torch.zeros((40 + grow, 50 + i + grow, 3), dtype=torch.uint8) for i in range(NK)]
    masks = [np.ones(tuple(t.shape[:2]), bool) for t in imgs]
    boxes = np.array([[10, 12, 30 + grow, 40 + grow]] * NK, np.float32)
    return m._source_supports(imgs, boxes, masks, S, graphed=True)


def test_tensor_queries_share_a_graph_by_shape():
    m = _model()
    one = dict(qry_img=torch.zeros((1, 3, 32, 48)), **_spp_tensors(1))
    two = dict(qry_img=torch.zeros((2, 3, 32, 48)), **_spp_tensors(2))
    assert _key(m, one, (32, 48)) == _key(m, dict(one), (32, 48))
    assert _key(m, one, (32, 48)) != _key(m, two, (32, 48), B=2)


def test_source_size_queries_share_a_graph_by_slot_and_network_size():
    m = _model()
    spp = _spp_tensors()
    a, b = _query(m, 20, 30), _query(m, 10, 7)
    assert a['sizes'] != b['sizes'] and a['need'] != b['need']
    base = _key(m, spp, (32, 48), source=a)
    assert base == _key(m, spp, (32, 48), source=b)                            # the source sizes are read on the device
    assert base != _key(m, spp, (32, 48), source=a, at_source=True)            # another launch sequence
    assert _key(m, spp, (32, 48), source=a, at_source=True) == _key(m, spp, (32, 48), source=b, at_source=True)
    assert base != _key(m, spp, (32, 32), source=_query(m, 20, 30, (32, 32)))  # another network size
    assert base != _key(m, dict(qry_img=torch.zeros((1, 3, 32, 48)), **spp), (32, 48))
    m.query_source_capacity = 3 * 1000
    assert base != _key(m, spp, (32, 48), source=_query(m, 20, 30))            # another slot


def test_source_supports_share_a_graph_by_slot_and_support_size():
    m = _model()
    qry = dict(qry_img=torch.zeros((1, 3, 32, 48)))
    a, b = _supports(m, 16), _supports(m, 16, grow=5)
    assert a['need'] != b['need'] and not torch.equal(a['rec'], b['rec'])
    ins = lambda sp: dict(qry, spp_bboxes=sp['boxes'], spp_rec=sp['rec'])
    base = _key(m, ins(a), (32, 48), spp_source=a)
    assert base == _key(m, ins(b), (32, 48), spp_source=b)                     # no window size of a batch
    c = _supports(m, 24)
    assert base != _key(m, ins(c), (32, 48), spp_source=c)                     # another S
    assert base != _key(m, dict(qry, **_spp_tensors()), (32, 48))              # supports as tensors
    m.support_source_capacity = 3 * 4000
    d = _supports(m, 16)
    assert base != _key(m, ins(d), (32, 48), spp_source=d)                     # another slot


def test_a_support_code_is_another_graph():
    m = _model()
    qry = dict(qry_img=torch.zeros((1, 3, 32, 48)))
    with_code = _key(m, qry, (32, 48), code={})
    assert with_code != _key(m, dict(qry, **_spp_tensors()), (32, 48))
    assert with_code != _key(m, qry, (32, 48))                                  # the flag itself, not only the tensors
    assert with_code == _key(m, dict(qry), (32, 48), code={'B': 1})


def test_the_slot_tensors_take_no_part_in_the_key():
    """Before the upload ``ins`` is without them, behind it they are there at the width the batch needs (or as the
    static slots themselves): one key."""
    m = _model()
    rs, sp = _query(m, 20, 30), _supports(m, 16)
    ins = dict(spp_bboxes=sp['boxes'], spp_rec=sp['rec'])
    up = dict(ins, qry_src=torch.zeros((1, rs['need']), dtype=torch.uint8),
              qry_src_hw=torch.zeros((1, 2), dtype=torch.int32),
              spp_src=torch.zeros((NK, sp['need']), dtype=torch.uint8),
              spp_msk=torch.zeros((NK, sp['mneed']), dtype=torch.uint8))
    static = dict(up, qry_src=torch.zeros((1, rs['capacity']), dtype=torch.uint8, device='meta'),
                  spp_src=torch.zeros((NK, sp['capacity']), dtype=torch.uint8, device='meta'))
    for at_source in (False, True):
        k = _key(m, ins, (32, 48), source=rs, spp_source=sp, at_source=at_source)
        assert k == _key(m, up, (32, 48), source=rs, spp_source=sp, at_source=at_source)
        assert k == _key(m, static, (32, 48), source=rs, spp_source=sp, at_source=at_source)
