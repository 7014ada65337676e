"""``fgn_poly_masks_u8`` (csrc/poly.hip) against ``polygon.dense``, bit for bit: every shape at which the
rule can go wrong, at the sizes where the mapping changes (one lane per column, 256 columns per workgroup, 32 rows per
row chunk), windows into slot rows at odd addresses with guard bytes, several instances of differing part counts in one
launch, the host route of an instance over the capacity, records out of range, return codes."""
import numpy as np
import pytest
import torch

from fgn_amd import polygon

from _poly_cases import shapes, star, zigzag

pytestmark = pytest.mark.gpu

GUARD = 0xFF
SIZES = [(37, 53), (70, 300), (1, 1), (1, 9)]


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _guarded(rows, cap, offset=13, pad=64):
    """A [rows, cap] slot of guard bytes at an odd byte offset inside a larger buffer of guard bytes."""
    buf = torch.full((offset + rows * cap + pad,), GUARD, dtype=torch.uint8, device=_dev())
    slot = buf[offset:offset + rows * cap].view(rows, cap)
    assert slot.data_ptr() % 2 == 1 and slot.is_contiguous()
    return buf, slot


def _check_slot(buf, slot, written: dict, offset=13):
    """Row -> the bytes expected at its front; every other byte of the buffer is still a guard."""
    rows, cap = slot.shape
    want = np.full(buf.numel(), GUARD, np.uint8)
    for row, b in written.items():
        b = np.asarray(b, np.uint8).reshape(-1)
        want[offset + row * cap:offset + row * cap + b.size] = b
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)


WINDOWS = {
    (37, 53): [(0, 0, 37, 53), (3, 5, 31, 33), (1, 1, 35, 51), (5, 0, 32, 53), (0, 7, 37, 1), (36, 0, 1, 53), (17, 23, 1, 1)],
    (70, 300): [(0, 0, 70, 300), (33, 255, 33, 3), (1, 43, 65, 257), (31, 0, 2, 300), (69, 299, 1, 1)],
    (1, 1): [(0, 0, 1, 1)],
    (1, 9): [(0, 0, 1, 9), (0, 3, 1, 5)],
}


@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_shape_whole_and_through_windows(hw):
    """All shapes of the list as the instances of ONE entry: whole masks in one call, then windows at odd offsets and of
    odd widths into slot rows at an odd address, guards behind every window and around the buffer."""
    from fgn_amd import ops
    h, w = hw
    cases = shapes(h, w)
    cases['covers the whole mask'] = [[-1, -1, -1, h + 1, w + 1, h + 1, w + 1, -1]]
    rng = np.random.RandomState(h * 1000 + w)
    cases['a seeded star'] = [star(rng, h, w, k=9)]
    cases['a star leaving the image'] = [star(rng, h, w, k=7, lo=0.6, hi=1.8)]
    pm = polygon.as_polys({'polygons': list(cases.values())}, hw)
    want = pm.dense()
    assert want[list(cases).index('covers the whole mask')].all()
    assert not want[list(cases).index('a sliver without a crossing')].any()
    routes = []
    got = ops.poly_masks(pm, routes=routes)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(cases),) + hw and got.is_contiguous()
    assert routes == ['device'] * len(cases)
    got = got.cpu().numpy()
    for i, name in enumerate(cases):
        assert np.array_equal(got[i], want[i]), (name, int((got[i] != want[i]).sum()))
    wins = WINDOWS[hw]
    for wy, wx, wh, ww in wins:
        sub = ops.poly_masks(pm, window=(wy, wx, wh, ww))
        assert tuple(sub.shape) == (len(cases), wh, ww)
        assert np.array_equal(sub.cpu().numpy(), want[:, wy:wy + wh, wx:wx + ww]), (wy, wx, wh, ww)
    cap = max(wh * ww for _, _, wh, ww in wins) + 7
    n = max(len(wins), len(cases))
    buf, slot = _guarded(n + 1, cap)
    items = [(i, pm.select([i % len(cases)]), wins[i % len(wins)]) for i in range(n)]       # (row n stays untouched)
    ops.poly_mask_rows(slot, items)
    _check_slot(buf, slot, {i: want[i % len(cases)][wy:wy + wh, wx:wx + ww]
                            for i, _, (wy, wx, wh, ww) in items})
    out = torch.full((len(cases),) + hw, GUARD, dtype=torch.uint8, device=_dev())
    assert ops.poly_masks(pm, out=out) is out and np.array_equal(out.cpu().numpy(), want)


def test_eight_instances_of_differing_part_counts_in_one_launch():
    from fgn_amd import ops
    h, w = 45, 270
    rng = np.random.RandomState(8)
    insts = [[star(rng, h, w, centre=(rng.uniform(0, w), rng.uniform(0, h))) for _ in range(k)]
             for k in (1, 5, 2, 9, 1, 3, 17, 4)]
    pm = polygon.as_polys({'polygons': insts, 'size': [h, w]}, None)
    calls = []
    real = ops._poly_launch
    ops._poly_launch = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = ops.poly_masks(pm)
    finally:
        ops._poly_launch = real
    assert calls == [1]
    assert np.array_equal(got.cpu().numpy(), pm.dense())
    assert pm.dense().reshape(8, -1).any(1).sum() >= 6


def test_no_mask_launches_nothing():
    from fgn_amd import ops
    calls = []
    real = ops._poly_launch
    ops._poly_launch = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = ops.poly_masks(polygon.as_polys({'polygons': []}, (5, 7)))
        assert tuple(got.shape) == (0, 5, 7) and got.dtype == torch.uint8 and got.is_cuda
        slot = torch.full((2, 9), GUARD, dtype=torch.uint8, device=_dev())
        assert ops.poly_mask_rows(slot, []) is slot and bool((slot == GUARD).all())
    finally:
        ops._poly_launch = real
    assert calls == []


def test_an_instance_over_the_capacity_goes_the_host_route():
    from fgn_amd import ops
    tri = [1, 1, 60, 20, 30, 60.5]
    pm = polygon.as_polys({'polygons': [[tri], [zigzag()], [tri, zigzag()], [[5, 5, 50, 9, 20, 55]]]}, (64, 64))
    want = pm.dense()
    assert want[1].any()
    routes = []
    got = ops.poly_masks(pm, routes=routes)
    assert routes == ['device', 'host', 'host', 'device']
    assert np.array_equal(got.cpu().numpy(), want)
    routes = []
    sub = ops.poly_masks(pm.select([1]), window=(3, 5, 40, 33), routes=routes)             # every instance on the host route
    assert routes == ['host'] and np.array_equal(sub.cpu().numpy()[0], want[1, 3:43, 5:38])
    buf, slot = _guarded(3, 64 * 64 + 5)
    routes = []
    ops.poly_mask_rows(slot, [(2, pm.select([1]), None), (0, pm.select([3]), (1, 2, 60, 61))], routes=routes)
    assert routes == ['host', 'device']
    _check_slot(buf, slot, {2: want[1], 0: want[3, 1:61, 2:63]})
    with pytest.raises(ops._lib.FgnHipError):                                              # the wrapper never sends one up
        ops._poly_launch([(0, (64, 64), (0, 0, 64, 64), [zigzag()])], 1, slot, slot.shape[1], 64, 64)


# ---- the clauses of the safety list, through the C entry point, with well-formed launches only -----------------------
H, W = 9, 11
TRI = [1.0, 1.0, 9.5, 2.0, 4.0, 8.5]
QUAD = [2.0, 3.0, 8.0, 3.0, 8.0, 7.0, 2.0, 7.0]


def _tables(masks, part_edit=None, edge_edit=None):
    """masks = (mask record or None for the good one, parts) -> (blob int32, n, n_parts, n_edges, scratch length)."""
    recs, parts, edges, n_edges, ends0 = [], [], [], 0, 0
    for rec, inst in masks:
        recs.append(list(rec[:6]) + [len(parts) if rec[6] is None else rec[6], len(inst) if rec[7] is None else rec[7]])
        for xy in inst:
            e, points, cap = polygon.edge_records(xy)
            parts.append([n_edges, len(e), points, ends0, cap, H, W, 0])
            edges.append(e)
            n_edges += len(e)
            ends0 += cap
    parts = np.asarray(parts, np.int32).reshape(-1, 8)
    edges = np.concatenate(edges) if edges else np.zeros((0, 8), np.int32)
    if part_edit:
        part_edit(parts)
    if edge_edit:
        edge_edit(edges)
    blob = np.concatenate([np.asarray(recs, np.int32).reshape(-1), parts.reshape(-1), edges.reshape(-1)])
    return blob.astype(np.int32), len(recs), len(parts), len(edges), ends0


def _raw(tables, out, stride, max_wh, max_ww, scratch_fill=0):
    from fgn_amd import lib, ops
    blob, n, n_parts, n_edges, slen = tables
    b = torch.from_numpy(blob).to(out.device)
    # the scratch holds zeros (or garbage) beforehand: a part that is refused must not be read
    scratch = torch.full((max(slen, 1) + 16,), scratch_fill, dtype=torch.int32, device=out.device)
    rc = lib.load().fgn_poly_masks_u8(b.data_ptr(), b.numel(), n, n_parts, n_edges, scratch.data_ptr(), slen,
                                      out.data_ptr(), stride, max_wh, max_ww, ops._stream())
    torch.cuda.synchronize()
    assert bool((scratch[slen:] == scratch_fill).all())                 # nothing behind the slices
    return rc


GOOD = [H, W, 2, 3, 5, 6, None, None]                 # window rows [2,7), columns [3,9)
BAD_MASK = {                                          # clause -> (record, its window is zero-filled)
    'h is 0': ([0, W, 2, 3, 5, 6, None, None], True),
    'w above 16384': ([H, 16385, 2, 3, 5, 6, None, None], True),
    'a size other than its parts\'': ([H + 1, W, 2, 3, 5, 6, None, None], 'empty'),
    'window empty (wh 0)': ([H, W, 2, 3, 0, 6, None, None], False),
    'window empty (ww negative)': ([H, W, 2, 3, 5, -6, None, None], False),
    'window below the mask': ([H, W, 5, 3, 5, 6, None, None], True),
    'window right of the mask': ([H, W, 2, 6, 5, 6, None, None], True),
    'negative origin': ([H, W, -1, 3, 5, 6, None, None], True),
    'wh above max_wh': ([H, W, 0, 3, 8, 6, None, None], True),
    'ww above max_ww': ([H, W, 2, 0, 5, 9, None, None], True),
    'window larger than the stride': ([H, W, 0, 0, 9, 11, None, None], False),
    'no part': ([H, W, 2, 3, 5, 6, None, 0], True),
    'negative part count': ([H, W, 2, 3, 5, 6, None, -3], True),
    'parts start before 0': ([H, W, 2, 3, 5, 6, -1, 1], True),
    'parts end behind n_parts': ([H, W, 2, 3, 5, 6, 2, 2], True),
    'parts far outside': ([H, W, 2, 3, 5, 6, 2 ** 31 - 2, 4], True),
}


@pytest.mark.parametrize('clause', list(BAD_MASK))
def test_a_mask_record_out_of_range_is_zero_filled_or_left_alone(clause):
    rec, zero_filled = BAD_MASK[clause]
    stride, max_wh, max_ww = 75, 7, 8                 # (72 = 8 x 9 fits the stride, 99 does not)
    buf, slot = _guarded(3, stride)
    assert _raw(_tables([(GOOD, [TRI]), (rec, [QUAD]), (GOOD, [QUAD])]), slot, stride, max_wh, max_ww) == 0
    written = {0: polygon.dense([TRI], H, W)[2:7, 3:9], 2: polygon.dense([QUAD], H, W)[2:7, 3:9]}
    if zero_filled:                                   # ('empty': a legal window whose only part is refused - no bit set)
        written[1] = np.zeros(rec[4] * rec[5], np.uint8)
    _check_slot(buf, slot, written)


def _set(row, col, value):
    def edit(t):
        t[row, col] = value
    return edit


BAD_PART = {                                          # a part of mask 1 (parts: 0 TRI | 1 QUAD, 2 TRI | 3 QUAD)
    'edges start before 0': _set(1, 0, -1),
    'no edge': _set(1, 1, 0),
    'edges end behind n_edges': _set(1, 1, 2 ** 30),
    'no point': _set(1, 2, 0),
    'more than 2^20 points': _set(1, 2, (1 << 20) + 1),
    'slice starts before 0': _set(1, 3, -4),
    'slice ends behind the scratch': _set(1, 3, 2 ** 31 - 9000),
    'capacity 0': _set(1, 4, 0),
    'capacity no power of two': _set(1, 4, 12),
    'capacity above 8192': _set(1, 4, 16384),
    'h is 0': _set(1, 5, 0),
    'w above 16384': _set(1, 6, 16385),
    'the size of another mask': _set(1, 5, H + 2),
}


@pytest.mark.parametrize('clause', list(BAD_PART))
def test_a_part_record_out_of_range_is_skipped(clause):
    """The part writes nothing and nobody reads it - the garbage its slice held beforehand included: its instance is the
    OR of its other parts, and the neighbours are untouched."""
    stride = H * W + 3
    buf, slot = _guarded(3, stride)
    whole = [H, W, 0, 0, H, W, None, None]
    t = _tables([(whole, [TRI]), (whole, [QUAD, TRI]), (whole, [QUAD])], part_edit=BAD_PART[clause])
    assert _raw(t, slot, stride, H, W, scratch_fill=5) == 0
    _check_slot(buf, slot, {0: polygon.dense([TRI], H, W), 1: polygon.dense([TRI], H, W), 2: polygon.dense([QUAD], H, W)})


def test_garbage_edges_stay_inside_their_tables():
    """Edge records of random bits - offsets, step counts, slopes that are NaN or huge - give garbage bits in their own
    instance: the neighbour's bytes, the guards and the scratch behind the slices are intact."""
    rng = np.random.RandomState(5)
    stride = H * W + 3
    whole = [H, W, 0, 0, H, W, None, None]
    for trial in range(4):
        def edit(e):
            n = len(TRI) // 2
            e[:n] = rng.randint(-2 ** 31, 2 ** 31, (n, 8), dtype=np.int64).astype(np.int32)
            if trial % 2:                                                # (plausible offsets, garbage everywhere else)
                e[:n, 6] = np.sort(rng.randint(0, 60, n))
                e[:n, 2] = rng.randint(0, 40, n)
        buf, slot = _guarded(2, stride)
        assert _raw(_tables([(whole, [TRI]), (whole, [QUAD])], edge_edit=edit), slot, stride, H, W) == 0
        got = slot.cpu().numpy()
        assert set(np.unique(got[0, :H * W])) <= {0, 1} and bool((got[:, H * W:] == GUARD).all())
        assert np.array_equal(got[1, :H * W].reshape(H, W), polygon.dense([QUAD], H, W))
        assert bool((buf[:13] == GUARD).all()) and bool((buf[13 + 2 * stride:] == GUARD).all())


def test_return_codes():
    from fgn_amd import lib
    L = lib.load()
    out = torch.full((64,), GUARD, dtype=torch.uint8, device=_dev())
    blob, n, n_parts, n_edges, slen = _tables([([2, 2, 0, 0, 2, 2, None, None], [[-1, -1, -1, 3, 3, 3, 3, -1]])],
                                              part_edit=lambda p: p.__setitem__((slice(None), slice(5, 7)), 2))
    b = torch.from_numpy(blob).to(_dev())
    scratch = torch.zeros(slen, dtype=torch.int32, device=_dev())
    names = ('blob', 'blob_ints', 'n', 'n_parts', 'n_edges', 'scratch', 'scratch_len', 'out', 'stride', 'max_wh', 'max_ww',
             'stream')
    ok = (b.data_ptr(), b.numel(), n, n_parts, n_edges, scratch.data_ptr(), slen, out.data_ptr(), 64, 2, 2, None)

    def call(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return L.fgn_poly_masks_u8(*(a[k] for k in names))
    assert call() == 0
    for name in ('blob', 'scratch', 'out'):
        assert call(**{name: None}) == -2, name                       # FGN_ERR_ARG
    for kw in (dict(n=-1), dict(n_parts=-1), dict(n_edges=-1), dict(blob_ints=-1), dict(scratch_len=-1), dict(stride=-1),
               dict(max_wh=-1), dict(max_ww=-2), dict(max_wh=16385), dict(max_ww=16385), dict(scratch_len=1 << 31),
               dict(blob_ints=b.numel() - 1), dict(n_edges=n_edges + 1)):
        assert call(**kw) == -1, kw                                    # FGN_ERR_SHAPE
    assert call(n=1 << 24, blob_ints=1 << 40) == -1 and call(n=1 << 18, max_ww=16384, blob_ints=1 << 40) == -1   # the grid
    for kw in (dict(n=0, blob_ints=1 << 20), dict(max_wh=0), dict(max_ww=0)):
        assert call(blob=None, scratch=None, out=None, **kw) == 0, kw  # nothing to do: no launch, no pointer looked at
    assert call(max_wh=16384, max_ww=16384) == 0
    torch.cuda.synchronize()
    assert out[:4].tolist() == [1, 1, 1, 1] and bool((out[4:] == GUARD).all())


def test_wrapper_refuses_bad_arguments():
    from fgn_amd import ops
    m = polygon.as_polys({'polygons': [[TRI]]}, (4, 5))
    for window in ((0, 0, 5, 5), (-1, 0, 2, 2), (0, 0, 0, 1), (3, 4, 2, 1)):
        with pytest.raises(ops._lib.FgnHipError):
            ops.poly_masks(m, window=window)
    slot = torch.zeros((2, 10), dtype=torch.uint8, device=_dev())
    two = polygon.as_polys({'polygons': [[TRI], [TRI]]}, (4, 5))
    for items in ([(2, m, None)], [(0, m, None)], [(0, m, (0, 0, 2, 5)), (0, m, (0, 0, 2, 5))], [(0, two, (0, 0, 1, 1))]):
        with pytest.raises(ops._lib.FgnHipError):
            ops.poly_mask_rows(slot, items)
    with pytest.raises(ops._lib.FgnHipError):
        ops.poly_masks(m, out=torch.zeros((1, 4, 4), dtype=torch.uint8, device=_dev()))
