"""``fgn_rle_decode_u8`` (csrc/mask.hip) against ``rle.decode``, bit for bit: whole masks at the sizes
where the mapping changes (one lane per column, 256 columns per workgroup, 32 rows per row chunk), every run pattern,
several masks of differing sizes in one launch, windows into slot rows at odd addresses with guard bytes, records out
of range, return codes."""
import numpy as np
import pytest
import torch

from fgn_amd import rle

pytestmark = pytest.mark.gpu

ROWS, COLS = 32, 256            # csrc/mask.hip: RLED_ROWS, RLED_THREADS
GUARD = 0xFF


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _item(h, w, counts):
    return {'size': [h, w], 'counts': rle.counts_to_string(np.asarray(counts, np.int64))}


def _patterns(h, w, seed):
    """Items of one size, one per run pattern: random (dense and sparse), empty (one run), full ([0, h*w]), the two
    checkerboards (n_runs == h*w and h*w + 1), one run spanning many columns, a column holding many runs (the rest
    empty), non-canonical zero runs in the middle."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    n = h * w
    span = np.zeros(n, bool)
    span[n // 5:n - n // 7] = True
    span = span.reshape(w, h).T                                        # (set along the column-major order)
    comb = np.zeros((h, w), bool)
    comb[::2, w // 2] = True
    items = rle.encode_many([rng.rand(h, w) < 0.5, rng.rand(h, w) < 0.03, np.zeros((h, w), bool), np.ones((h, w), bool),
                             (yy + xx) % 2 == 0, (yy + xx) % 2 == 1, span, comb])
    assert rle.string_to_counts(items[2]['counts']).tolist() == [n]
    assert rle.string_to_counts(items[3]['counts']).tolist() == [0, n]
    if h % 2:                                                          # (an odd column alternates into the next one)
        assert rle.string_to_counts(items[5]['counts']).size == n and rle.string_to_counts(items[4]['counts']).size == n + 1
    a = n // 3
    items.append(_item(h, w, [a, 0, 0, n - a]))                        # set [a, n) behind two zero runs
    items.append(_item(h, w, [a, 0, 0, 0, n - a]))                     # all clear through three zero runs
    items.append(_item(h, w, [0, 0, 0, a, 0, n - a, 0, 0]))
    items.append(_item(h, w, [a, 0, n - a, 0]))                        # all clear, a zero run in the middle
    return items


def _want(items):
    return np.stack([rle.decode(it) for it in items])


SIZES = [(1, 1), (1, 5), (5, 1), (3, 5), (63, 61), (64, 64), (65, 67), (130, 257),
         (ROWS - 1, 63), (ROWS, 64), (ROWS + 1, 65), (2 * ROWS + 1, COLS - 1), (7, COLS), (2, COLS + 1)]


@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_whole_masks_every_pattern(hw):
    from fgn_amd import ops
    items = _patterns(*hw, seed=hw[0] * 1000 + hw[1])
    m = rle.as_masks(items)
    got = ops.rle_decode_masks(m)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(items),) + hw and got.is_contiguous()
    want = _want(items)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(m.dense(), want)


@pytest.mark.parametrize('hw', [(1, 16384), (16384, 1)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_the_longest_row_and_column(hw):
    from fgn_amd import ops
    rng = np.random.RandomState(7)
    n = 16384
    flat = [rng.rand(n) < 0.5, np.arange(n) % 2 == 1, np.zeros(n, bool), np.ones(n, bool)]
    masks = [f.reshape(hw[1], hw[0]).T for f in flat]
    items = rle.encode_many(masks) + [_item(*hw, [5000, 0, 0, n - 5000])]
    got = ops.rle_decode_masks(rle.as_masks(items)).cpu().numpy()
    assert np.array_equal(got[:4], np.stack(masks).astype(np.uint8))
    assert np.array_equal(got[4].T.reshape(-1), (np.arange(n) >= 5000).astype(np.uint8))


def test_no_mask_launches_nothing():
    from fgn_amd import ops
    calls = []
    real = ops._rle_decode
    ops._rle_decode = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = ops.rle_decode_masks(rle.as_masks([], hw=(5, 7)))
        assert tuple(got.shape) == (0, 5, 7) and got.dtype == torch.uint8 and got.is_cuda
        got = ops.rle_decode_masks(rle.as_masks([], hw=(5, 7)), window=(1, 2, 3, 4))
        assert tuple(got.shape) == (0, 3, 4)
        slot = torch.full((2, 9), GUARD, dtype=torch.uint8, device=_dev())
        assert ops.rle_decode_rows(slot, []) is slot and bool((slot == GUARD).all())
    finally:
        ops._rle_decode = real
    assert calls == []


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


def test_one_launch_with_masks_of_differing_sizes_and_run_counts():
    from fgn_amd import ops
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:70, 0:90]
    masks = [np.zeros((3, 5), bool),                                   # one run ...
             (yy + xx) % 2 == 0,                                       # ... next to 6300
             rng.rand(33, 257) < 0.5, np.ones((1, 1), bool), rng.rand(130, 9) < 0.2, np.zeros((64, 64), bool)]
    runs = [rle.as_masks([rle.encode(m)]) for m in masks]
    assert runs[0].ends.size == 1 and runs[1].ends.size > 6000
    cap = 33 * 257 + 5
    buf, slot = _guarded(len(masks) + 2, cap)
    order = [3, 0, 5, 1, 6, 2]                                         # rows in no order; rows 4 and 7 stay untouched
    calls = []
    real = ops._rle_decode
    ops._rle_decode = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        ops.rle_decode_rows(slot, [(row, r, None) for row, r in zip(order, runs)])
    finally:
        ops._rle_decode = real
    assert calls == [1]
    _check_slot(buf, slot, {row: m for row, m in zip(order, masks)})


WINDOWS = {
    (37, 41): [(0, 0, 1, 1), (0, 40, 1, 1), (36, 0, 1, 1), (36, 40, 1, 1), (0, 0, 37, 41), (3, 5, 31, 33), (1, 1, 35, 39),
               (5, 0, 32, 41), (0, 7, 37, 1), (36, 0, 1, 41)],
    (70, 300): [(0, 0, 70, 300), (33, 255, 33, 3), (1, 43, 65, 257), (31, 0, 2, 300), (69, 299, 1, 1)],
}


@pytest.mark.parametrize('hw', list(WINDOWS), ids=lambda s: f'{s[0]}x{s[1]}')
def test_windows(hw):
    from fgn_amd import ops
    items = _patterns(*hw, seed=11)
    want = _want(items)
    m = rle.as_masks(items)
    for wy, wx, wh, ww in WINDOWS[hw]:
        got = ops.rle_decode_masks(m, window=(wy, wx, wh, ww))
        assert tuple(got.shape) == (len(items), wh, ww)
        assert np.array_equal(got.cpu().numpy(), want[:, wy:wy + wh, wx:wx + ww]), (wy, wx, wh, ww)
    # into slot rows at an odd address, the stride larger than any window: guards behind every window and around
    wins = WINDOWS[hw]
    cap = max(wh * ww for _, _, wh, ww in wins) + 7
    buf, slot = _guarded(len(wins), cap)
    singles = [rle.as_masks([items[i % len(items)]]) for i in range(len(wins))]
    ops.rle_decode_rows(slot, [(i, singles[i], wins[i]) for i in range(len(wins))])
    _check_slot(buf, slot, {i: want[i % len(items)][wy:wy + wh, wx:wx + ww] for i, (wy, wx, wh, ww) in enumerate(wins)})
    # ``out`` given
    out = torch.full((len(items), 31, 33), GUARD, dtype=torch.uint8, device=_dev())
    assert ops.rle_decode_masks(m, window=(3, 5, 31, 33), out=out) is out
    assert np.array_equal(out.cpu().numpy(), want[:, 3:34, 5:38])


def _raw(ends, recs, out, stride, max_wh, max_wh_w, n=None):
    from fgn_amd import lib, ops
    e = torch.from_numpy(np.asarray(ends, np.uint32).view(np.int32).copy()).to(out.device)
    r = torch.from_numpy(np.ascontiguousarray(recs, np.int32)).to(out.device)
    rc = lib.load().fgn_rle_decode_u8(e.data_ptr(), e.numel(), r.data_ptr(), out.data_ptr(), stride,
                                      r.shape[0] if n is None else n, max_wh, max_wh_w, ops._stream())
    torch.cuda.synchronize()
    return rc


H, W = 9, 11
N = H * W
GOOD = [H, W, 2, 3, 5, 6, 0, 4]                       # window rows [2,7), columns [3,9); slice [0, 4)
ENDS = [20, 50, 50, 99, 30, 99]                       # mask A = ends[0:4]; ends[4:6] belongs to nobody here
BAD = {                                               # clause -> (record, its window is zero-filled)
    'h is 0': ([0, W, 2, 3, 5, 6, 0, 4], True),
    'w above 16384': ([H, 16385, 2, 3, 5, 6, 0, 4], True),
    'window empty (wh 0)': ([H, W, 2, 3, 0, 6, 0, 4], False),
    'window empty (ww negative)': ([H, W, 2, 3, 5, -6, 0, 4], False),
    'window below the mask': ([H, W, 5, 3, 5, 6, 0, 4], True),
    'window right of the mask': ([H, W, 2, 6, 5, 6, 0, 4], True),
    'negative origin': ([H, W, -1, 3, 5, 6, 0, 4], True),
    'wh above max_wh': ([H, W, 0, 3, 8, 6, 0, 4], True),
    'ww above max_ww': ([H, W, 2, 0, 5, 9, 0, 4], True),
    'window larger than the stride': ([H, W, 0, 0, 9, 11, 0, 4], False),
    'no run': ([H, W, 2, 3, 5, 6, 0, 0], True),
    'negative run count': ([H, W, 2, 3, 5, 6, 0, -3], True),
    'slice starts before 0': ([H, W, 2, 3, 5, 6, -1, 4], True),
    'slice ends behind n_ends': ([H, W, 2, 3, 5, 6, 3, 4], True),
    'slice far outside': ([H, W, 2, 3, 5, 6, 2 ** 31 - 2, 4], True),
}


@pytest.mark.parametrize('clause', list(BAD))
def test_a_record_out_of_range_is_zero_filled_or_left_alone(clause):
    """Host-side argument cases: the kernel refuses the record before it reads a run.  The neighbours decode."""
    rec, zero_filled = BAD[clause]
    stride, max_wh, max_ww = 75, 7, 8                 # (72 = 8 x 9 fits the stride, 99 does not)
    buf, slot = _guarded(3, stride)
    rc = _raw(ENDS, [GOOD, rec, GOOD], slot, stride, max_wh, max_ww)
    assert rc == 0
    good = rle.decode(_item(H, W, [20, 30, 0, 49]))[2:7, 3:9]
    written = {0: good, 2: good}
    if zero_filled:
        written[1] = np.zeros(rec[4] * rec[5], np.uint8)
    _check_slot(buf, slot, written)


def test_garbage_ends_stay_inside_their_slice():
    """A slice that is not monotone gives garbage bits - and the neighbours' bytes and the guards are intact."""
    rng = np.random.RandomState(5)
    ends = np.concatenate([rng.randint(0, 2 ** 32, 40, dtype=np.uint64).astype(np.uint32), [20, 50, 50, 99]])
    buf, slot = _guarded(2, 40)
    assert _raw(ends, [[H, W, 2, 3, 5, 6, 0, 40], [H, W, 2, 3, 5, 6, 40, 4]], slot, 40, 5, 6) == 0
    torch.cuda.synchronize()
    got = slot.cpu().numpy()
    assert set(np.unique(got[0, :30])) <= {0, 1} and bool((got[:, 30:] == GUARD).all())
    assert np.array_equal(got[1, :30].reshape(5, 6), rle.decode(_item(H, W, [20, 30, 0, 49]))[2:7, 3:9])


def test_return_codes():
    from fgn_amd import lib
    L = lib.load()
    out = torch.full((64,), GUARD, dtype=torch.uint8, device=_dev())
    e = torch.tensor([4], dtype=torch.int32, device=_dev())
    r = torch.tensor([[2, 2, 0, 0, 2, 2, 0, 1]], dtype=torch.int32, device=_dev())
    ok = (e.data_ptr(), 1, r.data_ptr(), out.data_ptr(), 64, 1, 2, 2, None)

    def call(**kw):
        names = ('ends', 'n_ends', 'recs', 'out', 'stride', 'n', 'max_wh', 'max_ww', 'stream')
        a = dict(zip(names, ok))
        a.update(kw)
        return L.fgn_rle_decode_u8(*(a[k] for k in names))
    assert call() == 0
    for name in ('ends', 'recs', 'out'):
        assert call(**{name: None}) == -2, name                       # FGN_ERR_ARG
    for kw in (dict(n=-1), dict(stride=-1), dict(n_ends=-1), dict(max_wh=-1), dict(max_ww=-2), dict(max_wh=16385),
               dict(max_ww=16385)):
        assert call(**kw) == -1, kw                                    # FGN_ERR_SHAPE
    assert call(n=1 << 24) == -1 and call(n=1 << 18, max_ww=16384) == -1    # the grid: refused, not launched
    for kw in (dict(n=0), dict(max_wh=0), dict(max_ww=0)):
        assert call(ends=None, recs=None, out=None, **kw) == 0, kw     # nothing to do: no launch, no pointer looked at
    assert call(max_wh=16384, max_ww=16384) == 0
    torch.cuda.synchronize()
    assert out[:4].tolist() == [0, 0, 0, 0] and bool((out[4:] == GUARD).all())


def test_wrapper_refuses_bad_arguments():
    from fgn_amd import ops
    m = rle.as_masks([_item(4, 5, [20])])
    for window in ((0, 0, 5, 5), (-1, 0, 2, 2), (0, 0, 0, 1), (3, 4, 2, 1)):
        with pytest.raises(ops._lib.FgnHipError):
            ops.rle_decode_masks(m, window=window)
    slot = torch.zeros((2, 10), dtype=torch.uint8, device=_dev())
    for items in ([(2, m, None)], [(0, m, None)], [(0, m, (0, 0, 2, 5)), (0, m, (0, 0, 2, 5))],
                  [(0, rle.as_masks([_item(4, 5, [20])] * 2), (0, 0, 1, 1))]):
        with pytest.raises(ops._lib.FgnHipError):
            ops.rle_decode_rows(slot, items)
    with pytest.raises(ops._lib.FgnHipError):
        ops.rle_decode_masks(m, out=torch.zeros((1, 4, 4), dtype=torch.uint8, device=_dev()))
