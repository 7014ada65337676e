"""The mask tail against an independent model, bit for bit: ``ops.mask_paste``, ``ops.mask_rle``,
``ops.mask_rle_src``, ``ops.mask_overlap``, ``ops.mask_overlap_src``, ``ops.mask_bits`` and ``ops.dense_mask_rle`` against
tests/_mask_ref.py - the float32 restatement of the shared paste sample, the oracle's RLE encoder on the model's mask,
exact pixel counts.  Every comparison is array_equal, bytes-equal or integer equality: no tolerance, no excluded pixel.
tests/test_mask_ref_cpu.py holds the model to float64 and to the oracle, and every case to the route it is built for."""
import functools

import numpy as np
import pytest
import torch

import _mask_ref as ref
from oracle import fgn_ref_cpu as O

pytestmark = pytest.mark.gpu
F32 = np.float32

FAMILIES = {'generic': ref.generic_cases(), 'exact': ref.exact_cases(), 'rounded': ref.rounded_cases(),
            'geometry': ref.geometry_cases(), 'layout': ref.layout_cases(), 'route': ref.rle_route_cases(),
            'overlap': {k: c for k, (c, _) in ref.overlap_cases().items()}}
PASTE_IDS = [(f, n) for f, cases in FAMILIES.items() for n in cases]
OVERLAP, SRC = ref.overlap_cases(), ref.src_cases()


def _thrs(family, c):
    """The case's thresholds; the exact and rounded families also run one float above 0.5, where their on-threshold pixels
    clear."""
    return tuple(F32(t) for t in c.thrs) + ((np.nextafter(F32(0.5), F32(1)),) if family in ('rounded', 'exact') else ())


@functools.lru_cache(maxsize=None)
def _model(family: str, name: str, thr: float, skip_empty: bool) -> np.ndarray:
    c = FAMILIES[family][name]
    m = np.stack([ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, F32(thr), skip_empty)[0] for d in range(c.D)])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _strings(family: str, name: str, thr: float, skip_empty: bool) -> tuple:
    return tuple(O.rle_encode(m)['counts'] for m in _model(family, name, thr, skip_empty))


def _dev(c):
    return torch.from_numpy(c.prob).cuda(), torch.from_numpy(c.boxes).cuda()


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device='cuda')


def _check_strings(out, want, rows=None):
    by, ln, ovf = [t.cpu().numpy() for t in out]
    for j in (range(len(want)) if rows is None else rows):
        assert ovf[j] == 0, j
        assert by[j, :ln[j]].tobytes() == want[j], j


# ---------------------------------------------------------------------------------------------- paste and fused RLE
@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('family,name', PASTE_IDS, ids=[f'{f}-{n}' for f, n in PASTE_IDS])
def test_paste_equals_the_model_on_every_pixel(family, name, skip_empty):
    from fgn_amd import ops
    c = FAMILIES[family][name]
    prob, boxes = _dev(c)
    for thr in _thrs(family, c):
        got = ops.mask_paste(prob, boxes, c.H, c.W, float(thr), skip_empty=skip_empty).cpu().numpy()
        assert got.dtype == np.uint8 and got.max(initial=0) <= 1
        want = _model(family, name, float(thr), skip_empty)
        diff = np.argwhere(got.astype(bool) != want)
        assert len(diff) == 0, (float(thr), len(diff), diff[:5].tolist())


@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('family,name', PASTE_IDS, ids=[f'{f}-{n}' for f, n in PASTE_IDS])
def test_fused_rle_equals_the_oracle_encoding_of_the_model_mask(family, name, skip_empty):
    from fgn_amd import ops
    c = FAMILIES[family][name]
    prob, boxes = _dev(c)
    for thr in _thrs(family, c):
        _check_strings(ops.mask_rle(prob, boxes, c.H, c.W, float(thr), skip_empty=skip_empty),
                       _strings(family, name, float(thr), skip_empty))


def test_paste_grid_stride_second_pass():
    """More four-pixel groups than 256 * 32 workgroups of 256 lanes cover: the loop runs a second time."""
    from fgn_amd import ops
    c = ref.large_paste_case()
    assert ref.paste_route(c.D, c.H, c.W)['passes'] == 2
    prob, boxes = _dev(c)
    for skip_empty in (True, False):
        got = ops.mask_paste(prob, boxes, c.H, c.W, 0.5, skip_empty=skip_empty).cpu()
        want = torch.from_numpy(np.stack([ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, F32(0.5), skip_empty)[0]
                                          for d in range(c.D)]))
        assert torch.equal(got.bool(), want)
        assert int(want[2, c.claims['second_pass_from_row']:].sum()) > 1000


@pytest.mark.parametrize('name', sorted(FAMILIES['layout']))
def test_paste_device_count_zeroes_the_rows_behind_it_in_a_poisoned_output(name):
    """The C entry point on a caller-owned output full of 0xAB: rows at and beyond the device count come out zero, the
    rows in front of it equal the model - also where one lane's four bytes straddle the count."""
    from fgn_amd import lib, ops
    c = FAMILIES['layout'][name]
    prob, boxes = _dev(c)
    for n in (0, 2, c.D - 1):
        out = torch.full((c.D, c.H, c.W), 0xAB, dtype=torch.uint8, device='cuda')
        cnt = _count(n)
        lib.check(lib.load().fgn_mask_paste_u8(ops._ptr(prob), ops._ptr(boxes), boxes.shape[1], ops._ptr(out),
                                               ops._ptr(cnt), c.D, c.H, c.W, c.MS, 0.5, 1, ops._stream()),
                  'fgn_mask_paste_u8')
        got = out.cpu().numpy()
        want = _model('layout', name, 0.5, True).astype(np.uint8)
        want[n:] = 0
        assert np.array_equal(got, want), n
        assert np.array_equal(ops.mask_paste(prob, boxes, c.H, c.W, 0.5, n_dev=cnt).cpu().numpy(), want)


def test_fused_rle_device_count_and_caller_owned_outputs():
    from fgn_amd import ops
    c = FAMILIES['generic']['37x50-m14']
    prob, boxes = _dev(c)
    for skip_empty in (True, False):
        out = (torch.full((c.D, ops.RLE_BYTE_CAP), 0xAB, dtype=torch.uint8, device='cuda'),
               torch.zeros(c.D, dtype=torch.int32, device='cuda'), torch.zeros(c.D, dtype=torch.int32, device='cuda'))
        got = ops.mask_rle(prob, boxes, c.H, c.W, 0.3, _count(4), skip_empty, out=out)
        assert all(a is b for a, b in zip(got, out))
        _check_strings(got, _strings('generic', c.name, float(F32(0.3)), skip_empty), rows=range(4))
        assert got[1][4:].tolist() == [0, 0] and got[2].tolist() == [0] * c.D
        assert bool((got[0][4:] == 0xAB).all())                       # rows behind the count: not written


@pytest.mark.parametrize('name', ['rpt2', 'cpt2', 'string-deltas'])
def test_fused_rle_caps_flag_overflow_one_below_the_need_and_not_at_it(name, monkeypatch):
    from fgn_amd import ops
    c = FAMILIES['route'][name]
    prob, boxes = _dev(c)
    thr = float(F32(c.thrs[0]))
    mask = _model('route', name, thr, True)[0]
    want = _strings('route', name, thr, True)
    T = ref.transitions(mask)
    assert T >= 2 and len(want[0]) >= 9
    for cap, flagged in ((T, False), (T - 1, True)):
        monkeypatch.setattr(ops, 'RLE_TRANS_CAP', cap)
        by, ln, ovf = [t.cpu().numpy() for t in ops.mask_rle(prob, boxes, c.H, c.W, thr)]
        assert (ovf[0], ln[0]) == ((1, 0) if flagged else (0, len(want[0]))), (cap, ovf[0], ln[0])
        assert flagged or by[0, :ln[0]].tobytes() == want[0]
    monkeypatch.setattr(ops, 'RLE_TRANS_CAP', 16384)
    for cap, flagged in ((len(want[0]), False), (len(want[0]) - 1, True)):
        monkeypatch.setattr(ops, 'RLE_BYTE_CAP', cap)
        by, ln, ovf = [t.cpu().numpy() for t in ops.mask_rle(prob, boxes, c.H, c.W, thr)]
        assert by.shape[1] == cap
        assert (ovf[0], ln[0]) == ((1, 0) if flagged else (0, len(want[0]))), (cap, ovf[0], ln[0])
        assert flagged or by[0, :ln[0]].tobytes() == want[0]


def test_fused_rle_refuses_an_image_of_two_to_the_32_pixels_without_a_launch():
    from fgn_amd import lib, ops
    c = FAMILIES['layout']['layout-1x1']
    prob, boxes = _dev(c)
    with pytest.raises(lib.FgnHipError):
        ops.mask_rle(prob, boxes, 65536, 65536, 0.5)
    torch.cuda.synchronize()
    _check_strings(ops.mask_rle(prob, boxes, c.H, c.W, 0.5), _strings('layout', 'layout-1x1', 0.5, True))


# ---------------------------------------------------------------------------------------------- source size
@functools.lru_cache(maxsize=None)
def _src_model(name: str, thr: float, skip_empty: bool):
    """(boxes_src [B*D,4] f32, per row the string - None for an image outside 1..16384, '' where a cap overflows: a
    2 x 16384 image whose two rows differ alternates along thousands of columns -, masks of image 0)."""
    from fgn_amd import ops
    c, net, sizes = SRC[name]
    D = c.D // len(sizes)
    bs, strings, masks0 = [], [], []
    for r in range(c.D):
        hw = sizes[r // D]
        b = ref.box_to_source_model(c.boxes[r], hw, net)
        bs.append(b)
        if max(hw) > ref.SRC_MAX_DIM:
            strings.append(None)
            continue
        m = ref.paste_model(c.prob[r], b, hw[0], hw[1], F32(thr), skip_empty)[0]
        counts = O.rle_encode(m)['counts']
        strings.append(b'' if ref.transitions(m) > ops.RLE_TRANS_CAP or len(counts) > ops.RLE_BYTE_CAP else counts)
        if r < D:
            masks0.append(m)
    return np.stack(bs), strings, np.stack(masks0)


@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('name', sorted(SRC))
def test_rle_at_source_size_equals_the_model_pasted_from_the_divided_box(name, skip_empty):
    from fgn_amd import ops
    c, net, sizes = SRC[name]
    B, D = len(sizes), c.D // len(sizes)
    prob, boxes = _dev(c)
    src_hw = torch.tensor(sizes, dtype=torch.int32, device='cuda')
    counts = [D if b % 2 == 0 else D - 1 for b in range(B)]
    n_dev = torch.tensor(counts, dtype=torch.int32, device='cuda')
    for thr in c.thrs:
        bs_want, strings, _ = _src_model(name, float(F32(thr)), skip_empty)
        out = (torch.full((c.D, ops.RLE_BYTE_CAP), 0xAB, dtype=torch.uint8, device='cuda'),
               torch.zeros(c.D, dtype=torch.int32, device='cuda'), torch.zeros(c.D, dtype=torch.int32, device='cuda'))
        bs = torch.full((c.D, 4), float('nan'), device='cuda')
        by, ln, ovf = [t.cpu().numpy() for t in ops.mask_rle_src(prob, boxes, src_hw, net, float(F32(thr)), n_dev,
                                                                 skip_empty, out=out, boxes_src_out=bs)]
        assert np.array_equal(bs.cpu().numpy().view(np.uint32), bs_want.view(np.uint32))      # bit for bit
        n_strings = 0
        for r in range(c.D):
            if strings[r] is None or r % D >= counts[r // D]:
                assert (ovf[r], ln[r]) == (0, 0), r
            elif strings[r] == b'':
                assert (ovf[r], ln[r]) == (1, 0), r
            else:
                assert ovf[r] == 0 and by[r, :ln[r]].tobytes() == strings[r], (float(thr), r)
                n_strings += 1
        assert n_strings >= B - 2                                  # every image inside the limits yields a string


@pytest.mark.parametrize('skip_empty', [True, False])
def test_overlap_at_source_size_equals_the_model_counts(skip_empty):
    from fgn_amd import ops
    c, net, sizes = SRC['scales']
    D = c.D // len(sizes)
    h, w = sizes[0]
    prob, boxes = _dev(c)
    gt = ref.gt_masks_for(h, w, 3, seed=1)
    for thr in c.thrs:
        masks = _src_model('scales', float(F32(thr)), skip_empty)[2]
        want = ref.overlap_model(masks, gt)
        want[0][D - 1:] = 0
        want[1][D - 1:] = 0
        got = ops.mask_overlap_src(prob[:D], boxes[:D], torch.from_numpy(gt).cuda(), (h, w), net, float(F32(thr)),
                                   _count(D - 1), skip_empty)
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), b)


# ---------------------------------------------------------------------------------------------- overlap
@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('name', sorted(OVERLAP))
def test_overlap_equals_the_model_counts(name, skip_empty):
    from fgn_amd import ops
    c, G = OVERLAP[name]
    prob, boxes = _dev(c)
    gt = ref.gt_masks_for(c.H, c.W, G)
    bits = ops.mask_bits(torch.from_numpy(gt).cuda())
    # the bit planes themselves: bit b of word xw of row y of mask g = pixel (y, 64 xw + b); bits of x >= W are zero
    nw = (c.W + 63) // 64
    padded = np.zeros((G, c.H, nw * 64), bool)
    padded[:, :, :c.W] = gt
    words = np.packbits(padded.reshape(G, c.H, nw, 64), axis=-1, bitorder='little').view(np.uint64)[..., 0]
    assert np.array_equal(bits[0].cpu().numpy().view(np.uint64), words.transpose(1, 2, 0))
    assert np.array_equal(bits[1].cpu().numpy(), gt.reshape(G, -1).sum(1))
    for thr in c.thrs:
        want = ref.overlap_model(_model('overlap', name, float(F32(thr)), skip_empty), gt)
        for operand in (bits, torch.from_numpy(gt).cuda()):
            got = ops.mask_overlap(prob, boxes, operand, c.H, c.W, float(F32(thr)), skip_empty=skip_empty)
            for a, b in zip(got, want):
                assert np.array_equal(a.cpu().numpy(), b), float(thr)
        cut = [w.copy() for w in want]
        cut[0][c.D - 1:] = 0
        cut[1][c.D - 1:] = 0
        got = ops.mask_overlap(prob, boxes, bits, c.H, c.W, float(F32(thr)), _count(c.D - 1), skip_empty, packed=True)
        for a, b in zip(got[:3], cut):
            assert np.array_equal(a.cpu().numpy(), b), float(thr)
        assert np.array_equal(got[3].cpu().numpy(), np.concatenate([cut[0].reshape(-1), cut[1], cut[2]]))


# ---------------------------------------------------------------------------------------------- dense RLE
@pytest.mark.parametrize('hw', ref.DENSE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_dense_rle_equals_the_oracle_encoder(hw):
    from fgn_amd import ops
    masks = ref.dense_patterns(*hw)
    by, ln, ovf = [t.cpu().numpy() for t in ops.dense_mask_rle(torch.from_numpy(masks).cuda())]
    for j, m in enumerate(masks):
        want = O.rle_encode(m)['counts']
        if ref.transitions(m) > ops.RLE_TRANS_CAP or len(want) > ops.RLE_BYTE_CAP:
            assert (ovf[j], ln[j]) == (1, 0), j
        else:
            assert ovf[j] == 0 and by[j, :ln[j]].tobytes() == want, j
    assert ovf[:3].tolist() == [0, 0, 0] and ovf[5] == 0


@pytest.mark.parametrize('hw', [(17, 70), (1025, 3)], ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_dense_rle_transition_cap_reached_and_exceeded_by_one(hw, monkeypatch):
    from fgn_amd import ops
    masks = ref.dense_patterns(*hw)[[0, 4]]
    want = [O.rle_encode(m)['counts'] for m in masks]
    T = [ref.transitions(m) for m in masks]
    assert T[0] != T[1] and min(T) >= 2
    for cap in (max(T), max(T) - 1, min(T), min(T) - 1):
        monkeypatch.setattr(ops, 'RLE_TRANS_CAP', cap)
        by, ln, ovf = [t.cpu().numpy() for t in ops.dense_mask_rle(torch.from_numpy(masks).cuda())]
        for j in range(2):
            if T[j] > cap:
                assert (ovf[j], ln[j]) == (1, 0), (cap, j)
            else:
                assert ovf[j] == 0 and by[j, :ln[j]].tobytes() == want[j], (cap, j)
