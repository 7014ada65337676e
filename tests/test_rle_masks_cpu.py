"""COCO RLE as an input form, host side: the string parser against ``rle.counts_to_string``, the
carrier's host decode against ``rle.decode``, the accepted forms and refusals of ``rle.as_masks``, the binding table,
the dataset option and the collate.  No reference-held vector pins the string format (pycocotools is not available to
the suite): the parser is held to the project's two existing restatements and to the known-answer strings of
``tests/test_oracle_golden.py``."""
import re

import numpy as np
import pytest

from fgn_amd import rle

COUNTS = [
    [5], [0, 5], [3, 2], [1, 2, 3], [0, 0, 6],                               # 1, 2, 3 runs: no delta yet
    [1, 2, 3, 4], [4, 3, 2, 1], [0, 0, 0, 7],                                 # the delta rule starts at the 4th
    [0, 4, 0, 0, 0, 3, 0, 9],                                                # zero runs: first, in the middle, runs of them
    [7, 0, 0, 0, 0, 0, 5], [2, 0, 3, 0, 4, 0],                               # ... and last
    [15, 16, 31, 32, 1023, 1024, 40000, 2 ** 20, 2 ** 25 - 1, 2 ** 25 + 7],  # 1, 2, 4 and 6 characters
    [3, 2 ** 26, 1, 5, 2 ** 20, 2, 40000, 1, 9, 2 ** 27, 0, 3],              # negative deltas, large and small
    [100, 90, 80, 70, 60, 50, 40, 30, 20, 10, 0, 0],                         # every delta negative
]


@pytest.mark.parametrize('counts', COUNTS, ids=lambda c: f'{len(c)}runs_{c[0]}')
def test_string_to_counts_inverts_counts_to_string(counts):
    c = np.asarray(counts, np.int64)
    s = rle.counts_to_string(c)
    got = rle.string_to_counts(s)
    assert got.dtype == np.int64 and np.array_equal(got, c)
    assert np.array_equal(rle.string_to_counts(s.decode('ascii')), c)         # str as well as bytes


def test_characters_per_value():
    """The cases above really need 1, 2, 4 and 6 characters (5 data bits each, the sign bit in the last)."""
    for v, n in ((15, 1), (16, 2), (511, 2), (40000, 4), (2 ** 25 + 7, 6)):
        assert len(rle.counts_to_string(np.array([v]))) == n
    assert rle.string_to_counts(b'').size == 0


def test_known_answer_strings():
    """The strings ``tests/test_oracle_golden.py`` pins for ``encode``, read back."""
    m = np.zeros((4, 5), np.uint8)
    m[1:3, 1:4] = 1
    e = rle.encode(m)
    assert np.array_equal(rle.string_to_counts(e['counts']), rle.mask_to_counts(m))
    assert np.array_equal(rle.as_masks([e]).dense()[0], m)


def test_malformed_strings_are_refused():
    for s in (b'\x20', b'0o', bytes([48 + 0x20]), b'1' * 3 + bytes([48 + 0x3f]) * 13 + b'1'):
        with pytest.raises(ValueError):
            rle.string_to_counts(s)


def _patterns(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    return [rng.rand(h, w) < 0.5, rng.rand(h, w) < 0.1, np.zeros((h, w), bool), np.ones((h, w), bool),
            (yy + xx) % 2 == 0, (yy + xx) % 2 == 1]


@pytest.mark.parametrize('hw', [(1, 1), (1, 7), (7, 1), (5, 3), (64, 65)])
def test_dense_is_rle_decode(hw):
    rng = np.random.RandomState(hw[0] * 100 + hw[1])
    masks = _patterns(*hw, rng)
    items = rle.encode_many(masks)
    m = rle.as_masks(items)
    assert m.shape == (len(masks),) + hw and m.ends.dtype == np.uint32 and m.first.dtype == np.int64
    assert m.first.shape == (len(masks) + 1,) and m.first[-1] == m.ends.size
    d = m.dense()
    assert d.dtype == np.uint8 and d.flags.c_contiguous
    for j, it in enumerate(items):
        assert np.array_equal(d[j], rle.decode(it)), j
        assert np.array_equal(d[j], masks[j].astype(np.uint8)), j


def test_non_canonical_zero_runs_decode_as_the_loop_decodes_them():
    h, w = 5, 4
    for counts in ([0, 20], [0, 0, 0, 20], [3, 0, 0, 2, 0, 5, 10], [0, 3, 0, 0, 0, 0, 17], [20, 0, 0], [4, 0, 16, 0]):
        it = {'size': [h, w], 'counts': rle.counts_to_string(np.array(counts))}
        want = rle.decode(it)
        assert np.array_equal(rle.as_masks([it]).dense()[0], want), counts
        assert np.array_equal(rle.as_masks([{'size': [h, w], 'counts': counts}]).dense()[0], want), counts


def test_as_masks_accepts_every_form():
    m = np.zeros((6, 4), bool)
    m[1:4, 1:3] = True
    e = rle.encode(m)
    cnt = rle.mask_to_counts(m)
    forms = [e, dict(e, counts=e['counts'].decode('ascii')), dict(e, counts=cnt.tolist()), dict(e, counts=cnt),
             [e['size'], e['counts']], (np.array(e['size'], np.int16), e['counts']),
             [np.array(e['size'], np.int16), cnt.astype(np.int32)], dict(e, size=np.array([6, 4], np.int16))]
    for f in forms:
        got = rle.as_masks([f])
        assert got.shape == (1, 6, 4) and np.array_equal(got.dense()[0], m)
        assert rle.is_rle([f]) and rle.is_item(f)
    both = rle.as_masks(forms, hw=(6, 4))
    assert both.shape == (len(forms), 6, 4) and np.array_equal(both.dense(), np.repeat(m[None], len(forms), 0))
    assert rle.as_masks(both) is both and rle.as_masks(both, hw=(6, 4)) is both
    empty = rle.as_masks([], hw=(3, 2))
    assert empty.shape == (0, 3, 2) and empty.dense().shape == (0, 3, 2) and empty.first.tolist() == [0]
    assert rle.is_rle([]) and rle.is_rle(both) and not rle.is_rle(np.zeros((1, 2, 2), bool))
    assert not rle.is_rle([np.zeros((2, 2), bool)])


@pytest.mark.parametrize('entry,hw,word', [
    ([{'size': [0, 4], 'counts': [0]}], None, 'within'),
    ([{'size': [2, 16385], 'counts': [2 * 16385]}], None, 'within'),
    ([{'size': [2, 2], 'counts': [4]}, {'size': [2, 3], 'counts': [6]}], None, 'item 1'),
    ([{'size': [2, 2], 'counts': [4]}], (2, 3), 'expected'),
    ([{'size': [2, 2], 'counts': [5, -1]}], None, 'negative'),
    ([{'size': [2, 2], 'counts': [3]}], None, 'sum'),
    ([{'size': [2, 2], 'counts': [2, 3]}], None, 'sum'),
    ([{'size': [2, 2], 'counts': []}], None, 'no run'),
    ([{'size': [2, 2], 'counts': b''}], None, 'no run'),
    ([{'size': [2, 2], 'counts': b'\x01'}], None, 'item 0'),
    ([{'size': [2, 2]}], None, 'item 0'),
    ([{'size': [2, 2, 2], 'counts': [8]}], None, 'item 0'),
    ([{'size': [2.0, 2.0], 'counts': [4]}], None, 'item 0'),
    ([{'size': [2, 2], 'counts': [1.5, 2.5]}], None, 'item 0'),
    ([], None, 'size'),
    ([], (0, 5), 'within'),
    (np.zeros((1, 2, 2)), None, 'expected'),
])
def test_as_masks_refusals_name_the_item(entry, hw, word):
    with pytest.raises(ValueError) as err:
        rle.as_masks(entry, hw, what='qry_isegmaps[3]')
    assert 'qry_isegmaps[3]' in str(err.value) and word in str(err.value), str(err.value)
    if isinstance(entry, list) and len(entry) == 2:
        assert 'item 1' in str(err.value)


def test_an_rlemasks_at_another_size_is_refused():
    m = rle.as_masks([{'size': [2, 2], 'counts': [4]}])
    with pytest.raises(ValueError):
        rle.as_masks(m, hw=(2, 3))


def test_binding_table_and_constants():
    import os
    from fgn_amd import lib, ops
    res, args = lib.SIGNATURES['fgn_rle_decode_u8']
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'fgn_hip.h')).read()
    proto = re.search(r'int fgn_rle_decode_u8\(([^;]*)\);', header).group(1)
    assert len(args) == len(proto.split(',')) == 9
    assert rle.MAX_DIM == ops.RESIZE_MAX_DIM == 16384 and ops.RLE_REC_INTS == 8


def test_dataset_option_and_collate():
    from fgn_amd.episodes import collate
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    kw = dict(n_ways=2, k_shots=1, n_imgs=4, img_size=48, spp_img_size=32, raw_uint8=True, spp_source=True)
    dense, runs = DS(**kw), DS(**kw, rle_masks=True)
    for i in range(2):
        a, b = dense[i], runs[i]
        assert set(a) == set(b)
        assert isinstance(b['qry_isegmaps'], list) and all(isinstance(it, dict) for it in b['qry_isegmaps'])
        assert np.array_equal(rle.as_masks(b['qry_isegmaps'], (48, 48)).dense(), a['qry_isegmaps'])
        for ma, mb in zip(a['spp_isegmaps'], b['spp_isegmaps']):
            assert np.array_equal(rle.as_masks([mb]).dense()[0], ma)
        for k in a:
            if k not in ('qry_isegmaps', 'spp_isegmaps', 'spp_imgs'):
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    bt = collate([runs[0], runs[1]])
    assert bt['qry_isegmaps'][0] is not None and rle.is_rle(bt['qry_isegmaps'][0]) and rle.is_rle(bt['qry_isegmaps'][1])
    assert all(isinstance(it, dict) for lst in bt['spp_isegmaps'] for it in lst)
    plain = DS(n_ways=2, k_shots=1, n_imgs=4, img_size=48, spp_img_size=32, rle_masks=True)[0]   # supports stay dense
    assert rle.is_rle(plain['qry_isegmaps']) and isinstance(plain['spp_isegmaps'], np.ndarray)


def test_source_supports_take_rle_items_and_upload_no_mask_byte():
    """``_source_supports`` (host only): the geometry is that of the dense call, no mask byte travels for an RLE
    instance and ``window_bytes`` counts its run ends instead."""
    import torch
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    from fgn_amd.weights import init_state_dict
    kw = dict(n_ways=2, k_shots=1, n_imgs=4, img_size=48, spp_img_size=32, raw_uint8=True, spp_source=True)
    a, b = DS(**kw)[0], DS(**kw, rle_masks=True)[0]
    cfg = tiny_config(2, 1, width_div=2)
    m = FGN(2, 1, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'], test_cfg=cfg['test_cfg'],
            state_dict=init_state_dict(cfg, 0))
    m.set_input_norm(**DS(**kw).input_norm)
    want = m._source_supports(a['spp_imgs'], a['spp_bboxes'], a['spp_isegmaps'], 32)
    pair = [[it['size'], it['counts']] for it in b['spp_isegmaps']]
    mixed = [b['spp_isegmaps'][0], a['spp_isegmaps'][1]]
    for masks, n_rle in ((b['spp_isegmaps'], 2), (pair, 2), (mixed, 1)):
        got = m._source_supports(a['spp_imgs'], a['spp_bboxes'], masks, 32)
        assert torch.equal(got['rec'], want['rec']) and torch.equal(got['boxes'], want['boxes'])
        assert (got['need'], got['mneed'], got['capacity'], got['mcapacity']) == \
            (want['need'], want['mneed'], want['capacity'], want['mcapacity'])
        assert all(torch.equal(x, y) for x, y in zip(got['flats'], want['flats']))
        assert len(got['mrle']) == n_rle
        ends = 0
        for row, runs, win in got['mrle']:
            assert got['mflats'][row].numel() == 0
            wy, wx, wh, ww = win
            assert np.array_equal(runs.dense()[0][wy:wy + wh, wx:wx + ww].reshape(-1), want['mflats'][row].numpy())
            ends += runs.ends.nbytes
        dense_rows = [i for i in range(2) if i not in [r for r, _, _ in got['mrle']]]
        assert all(torch.equal(got['mflats'][i], want['mflats'][i]) for i in dense_rows)
        assert got['window_bytes'] == sum(f.numel() for f in got['flats'] + got['mflats']) + ends
    assert want['mrle'] == []
    with pytest.raises(ValueError):                     # an RLE item at another image's size
        m._source_supports(a['spp_imgs'], a['spp_bboxes'], [dict(b['spp_isegmaps'][0], size=[48, 47])] + mixed[1:], 32)
    with pytest.raises(ValueError):                     # the plain path is dense only
        m.encode_supports(torch.zeros((2, 32, 32, 3), dtype=torch.uint8), a['spp_bboxes'], b['spp_isegmaps'])


def test_is_item_decides_by_types_alone():
    """Nothing is built from the argument: ragged and nested lists are simply not items."""
    pair = [[4, 5], rle.counts_to_string(np.array([20]))]
    assert rle.is_item(pair) and rle.is_item((np.array([4, 5], np.int16), pair[1])) and rle.is_item([[4, 5], np.array([20])])
    for other in ([pair, pair], [[pair, pair], [pair, pair]], [[0, 1], [1, 0]], [[4, 5], [20]], [[4.0, 5.0], pair[1]],
                  [[True, False], pair[1]], [np.zeros((2, 2)), pair[1]], [np.zeros(2), pair[1]], [[4, 5, 6], pair[1]],
                  [[4, 5], np.zeros((1, 2), np.int64)], [[4, 5], np.zeros(2)], [[[4, 5], pair[1]], 3], 'ab', [4, 5], None):
        assert not rle.is_item(other), other
    assert rle.is_rle([pair, pair]) and not rle.is_rle([[pair, pair], [pair, pair]])
    assert not rle.is_rle([[[0, 1], [1, 0]]]) and not rle.is_rle([[0, 1], [1, 0]])          # a 2 x 2 mask as lists is dense


def _tiny(n_ways, k_shots):
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(n_ways, k_shots, width_div=2)
    return FGN(n_ways, k_shots, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


@pytest.mark.parametrize('n_ways,k_shots', [(2, 1), (1, 2)])
def test_nested_pair_form_supports_of_two_instances(n_ways, k_shots):
    """N*K == 2: a support set of two ``[size, counts]`` pairs, nested per batch as ``collate`` nests it, is a support
    set and not one pair - in ``collate`` and in ``_source_supports``."""
    import torch
    from fgn_amd.episodes import collate
    from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG as DS
    kw = dict(n_ways=n_ways, k_shots=k_shots, n_imgs=4, img_size=48, spp_img_size=32, raw_uint8=True, spp_source=True)
    dense, runs = DS(**kw), DS(**kw, rle_masks=True)
    m = _tiny(n_ways, k_shots)
    m.set_input_norm(**dense.input_norm)

    def pairs(sample):
        return dict(sample, spp_isegmaps=[[np.array(it['size'], np.int16), it['counts']] for it in sample['spp_isegmaps']],
                    qry_isegmaps=[[it['size'], it['counts']] for it in sample['qry_isegmaps']])
    for B in (1, 2):
        want_b = collate([dense[i] for i in range(B)])
        for make in (pairs, lambda s_: s_):                                   # pair form, dict form
            got_b = collate([make(runs[i]) for i in range(B)])
            assert len(got_b['spp_isegmaps']) == B and all(len(lst) == 2 for lst in got_b['spp_isegmaps'])
            assert all(rle.is_item(it) for lst in got_b['spp_isegmaps'] for it in lst)
            assert all(rle.is_rle(g) for g in got_b['qry_isegmaps'])
            want = m._source_supports(want_b['spp_imgs'], want_b['spp_bboxes'], want_b['spp_isegmaps'], 32)
            got = m._source_supports(got_b['spp_imgs'], got_b['spp_bboxes'], got_b['spp_isegmaps'], 32)
            assert got['B'] == B and got['n'] == 2 * B and torch.equal(got['rec'], want['rec'])
            assert [r for r, _, _ in got['mrle']] == list(range(2 * B))
            for row, rm, (wy, wx, wh, ww) in got['mrle']:
                assert np.array_equal(rm.dense()[0][wy:wy + wh, wx:wx + ww].reshape(-1), want['mflats'][row].numpy())
    flat = pairs(runs[0])                                                     # one support set as a plain list of pairs
    got = m._source_supports(flat['spp_imgs'], flat['spp_bboxes'], flat['spp_isegmaps'], 32)
    assert got['B'] == 1 and len(got['mrle']) == 2


def test_network_size_comes_from_the_image_tensor_where_img_shape_is_absent():
    """An RLE entry that disagrees with the network size is refused on the host also without ``img_shape``."""
    import torch
    from fgn_amd.detector import _gt_entries
    m = _tiny(2, 1)
    item = {'size': [40, 48], 'counts': [40 * 48]}
    nchw = torch.zeros((2, 3, 40, 48))
    assert m._gt_sizes(nchw, None, None) == [(40, 48)] * 2
    assert m._gt_sizes(nchw, [(32, 32, 3)] * 2, None) == [(32, 32)] * 2
    m.set_input_norm(mean=(0.5,) * 3, std=(0.2,) * 3)
    assert m._gt_sizes(torch.zeros((1, 40, 48, 3), dtype=torch.uint8), None, None) == [(40, 48)]
    assert m._gt_sizes(torch.zeros((1, 40, 48, 3), dtype=torch.uint8), None, (32, 32)) == [(40, 48)]
    assert m._gt_sizes([torch.zeros((40, 48, 3), dtype=torch.uint8)], None, (32, 32)) == [(40, 48)]
    got = _gt_entries([[item], []], m._gt_sizes(nchw, None, None))
    assert [g.shape for g in got] == [(1, 40, 48), (0, 40, 48)]
    with pytest.raises(ValueError) as err:
        _gt_entries([[item]], m._gt_sizes(torch.zeros((1, 3, 40, 49)), None, None))
    assert 'qry_isegmaps[0]' in str(err.value)
    dense = [np.zeros((1, 40, 48), bool)]
    assert _gt_entries(dense, None) is dense                                   # no RLE entry: the argument itself
