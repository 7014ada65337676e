"""``ops.color_masks`` / ``ops.color_mask_rows`` (``fgn_color_mask_u8``) against
``ColorMasks.dense()`` bit for bit, at the smallest shapes where the kernel can still go wrong: the cases of
``test_color_masks_cpu`` (1 x 1, empty boxes, boxes on every corner and edge, widths around the 64-bit word and the tile
seams, matching pixels directly outside the box, adjacent boxes, the colour clamps), source rows at odd byte offsets,
1 / 5 / 70 masks over images of different sizes in one launch, the documented zeroing of an out-of-range record, and
the row form for the support slots."""
import contextlib

import numpy as np
import pytest
import torch

import test_color_masks_cpu as cpu
from fgn_amd import colormask as cm

pytestmark = pytest.mark.gpu

CASES = cpu.CASES


def _items(cases):
    return [cm.as_color_masks({'bboxes': b, 'colors': c, 'shift': s}, img.shape[:2], name) for name, img, b, c, s in cases]


@pytest.fixture(scope='module')
def want():
    """The host masks of every case, computed once."""
    return [m.dense(c[1]).view(np.uint8) for m, c in zip(_items(CASES), CASES)]


def _slot(imgs, offset=0, pad=0):
    """The images at the fronts of the rows of one device slot; ``offset``: the first row starts that many bytes into
    its allocation, ``pad``: rows that many bytes longer than the largest image (an odd pitch)."""
    cap = max(im.size for im in imgs)
    pitch = cap + pad
    host = np.full(offset + len(imgs) * pitch, 0x5a, np.uint8)
    for i, im in enumerate(imgs):
        host[offset + i * pitch: offset + i * pitch + im.size] = im.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    return buf[offset:].view(len(imgs), pitch)[:, :cap]


@contextlib.contextmanager
def _launches():
    from fgn_amd import ops
    calls, real = [], ops._color_launch
    ops._color_launch = lambda *a, **k: calls.append(int(a[1].shape[0])) or real(*a, **k)
    try:
        yield calls
    finally:
        ops._color_launch = real


@pytest.mark.parametrize('k', range(len(CASES)), ids=[c[0] for c in CASES])
def test_one_image_is_dense_bit_for_bit(want, k):
    from fgn_amd import ops
    m = _items([CASES[k]])[0]
    got = ops.color_masks(_slot([CASES[k][1]]), [(0, m)])
    assert len(got) == 1 and got[0].dtype == torch.uint8 and tuple(got[0].shape) == m.shape
    assert np.array_equal(got[0].cpu().numpy(), want[k])


def test_the_cases_are_not_all_empty(want):
    assert sum(int(w.any()) for w in want) > len(want) // 2
    assert any(w.shape[2] > 128 for w in want) and any(w.shape[1] > 32 for w in want)       # more than one tile each way


@pytest.mark.parametrize('offset', (1, 2, 3))
def test_rows_at_odd_byte_offsets_and_an_odd_pitch(want, offset):
    """Every case in ONE launch - more than 70 masks over images of more than 20 sizes, the first rows read by two items
    each: rows start at any byte."""
    from fgn_amd import ops
    items = _items(CASES)
    slot = _slot([c[1] for c in CASES], offset=offset, pad=offset + 4)
    assert slot.data_ptr() % 4 == offset and slot.stride(0) > slot.shape[1] and len({c[1].shape for c in CASES}) > 20
    pairs = list(enumerate(items)) + list(enumerate(items))[:20]
    with _launches() as calls:
        got = ops.color_masks(slot, pairs)
    assert calls == [sum(len(m) for _, m in pairs)] and calls[0] >= 70
    for g, (k, _) in zip(got, pairs):
        assert np.array_equal(g.cpu().numpy(), want[k]), CASES[k][0]


@pytest.mark.parametrize('n', (1, 5))
def test_a_few_masks_in_one_launch_with_rows_out_of_order(want, n):
    from fgn_amd import ops
    pick = [k for k, c in enumerate(CASES) if len(c[2]) == 1][3:3 + n]
    assert len(pick) == n
    items = _items([CASES[k] for k in pick])
    slot = _slot([CASES[k][1] for k in reversed(pick)])                      # item j reads row n - 1 - j
    with _launches() as calls:
        got = ops.color_masks(slot, [(n - 1 - j, m) for j, m in enumerate(items)])
    assert calls == [n]
    for g, k in zip(got, pick):
        assert np.array_equal(g.cpu().numpy(), want[k]), CASES[k][0]


def test_given_output_buffer_is_written_in_full():
    """No memset is needed: a buffer full of 0xff comes back as exactly the masks."""
    from fgn_amd import ops
    _, img, boxes, colors, shift = next(c for c in CASES if c[0] == 'corners-edges')
    m = _items([('x', img, boxes, colors, shift)])[0]
    out = torch.full((len(boxes), img.shape[0] * img.shape[1]), 0xff, dtype=torch.uint8, device='cuda')
    got = ops.color_masks(_slot([img]), [(0, m)], out=out)
    assert got[0].data_ptr() == out.data_ptr()
    assert np.array_equal(got[0].cpu().numpy(), m.dense(img).view(np.uint8))


def test_no_mask_no_launch():
    from fgn_amd import lib, ops
    slot = _slot([np.zeros((4, 5, 3), np.uint8)])
    none = cm.as_color_masks({'bboxes': np.zeros((0, 4)), 'colors': np.zeros((0, 3))}, (4, 5))
    with _launches() as calls:
        assert ops.color_masks(slot, []) == []
        got = ops.color_masks(slot, [(0, none)])
        msk = torch.zeros((1, 20), dtype=torch.uint8, device='cuda')
        assert ops.color_mask_rows(slot, msk, []) is msk
    assert calls == [] and tuple(got[0].shape) == (0, 4, 5)
    # the entry point itself: n == 0 is OK whatever the pointers; null pointers and negative counts are refused
    f = lib.load().fgn_color_mask_u8
    assert f(None, 0, 0, 0, None, 0, None, 0, 0, 4, 5, None) == 0
    assert f(None, 60, 60, 1, None, 1, None, 20, 1, 4, 5, None) == -2
    assert f(slot.data_ptr(), 60, 60, 1, slot.data_ptr(), -1, msk.data_ptr(), 20, 1, 4, 5, None) == -1
    assert f(slot.data_ptr(), 60, 60, 1, slot.data_ptr(), 1, msk.data_ptr(), -20, 1, 4, 5, None) == -1
    assert f(slot.data_ptr(), 60, 60, 1, slot.data_ptr(), 1 << 23, msk.data_ptr(), 20, 1, 4, 16384, None) == -1     # the grid


def test_an_out_of_range_record_gives_zeros_and_spares_its_neighbours():
    """Records built directly, past the host checks; every address stays inside the buffers (this checks the documented
    zeroing, nothing else): a box that leaves its image, a slot row that does not exist, an image larger than the
    launch's maximum and one larger than its row -> zeros; an output that does not fit its stride or does not exist ->
    not written at all."""
    from fgn_amd import ops
    h, w = 11, 70
    img = np.full((h, w, 3), 255, np.uint8)
    img[2:9, 3:66] = (230, 25, 75)
    slot = _slot([img])
    m = cm.as_color_masks({'bboxes': [[1, 2, 10, 68]], 'colors': [[230, 25, 75]]}, (h, w))
    good = ops._color_records([(0, m)], 1, slot.shape[1], 'test')[0][0]
    want = m.dense(img)[0].reshape(-1).view(np.uint8)
    assert want.any()

    def rec(out, **f):
        r = good.copy()
        r[13] = out
        for k, v in f.items():
            r[('row', 'h', 'w', 'y0', 'x0', 'y1', 'x1').index(k)] = v
        return r
    stride, n_out = h * w + 5, 9
    recs = np.stack([rec(0), rec(1, x1=w + 1), rec(2), rec(3, row=1), rec(4, y0=-1), rec(5, h=h + 1), rec(6, y1=0),
                     rec(7, w=w + 6), rec(n_out), rec(-1), rec(8, w=16385)])
    out = torch.full((n_out, stride), 7, dtype=torch.uint8, device='cuda')
    ops._color_launch(slot, recs, out, stride, n_out, h, w)
    got = out.cpu().numpy()
    assert (got[:, h * w:] == 7).all()                                      # behind h * w: never written
    for i in (0, 2):
        assert np.array_equal(got[i, :h * w], want), i                      # the neighbours are whole
    for i in (1, 3, 4, 6):
        assert not got[i, :h * w].any(), i                                  # zeros, in full
    assert (got[5] == 7).all() and (got[7] == 7).all() and (got[8] == 7).all()     # (h+1) * w > stride etc.: not written
    # the same larger image where it fits the stride but not the launch's maximum / its slot row: zeros
    out2 = torch.full((2, (h + 1) * w), 7, dtype=torch.uint8, device='cuda')
    ops._color_launch(slot, np.stack([rec(0, h=h + 1), rec(1)]), out2, (h + 1) * w, 2, h, w)
    got2 = out2.cpu().numpy()
    assert not got2[0].any() and np.array_equal(got2[1, :h * w], want) and (got2[1, h * w:] == 7).all()


def test_rows_form_leaves_everything_else_as_it_was():
    """``color_mask_rows``: the window's bytes at the front of its row of the mask slot; the bytes behind them and every
    other row stay."""
    from fgn_amd import ops
    pick = [next(c for c in CASES if c[0] == n) for n in ('box17x65', 'ring-outside', 'box3x129', '1x1')]
    items = _items(pick)
    slot = _slot([c[1] for c in pick] + [np.zeros((2, 2, 3), np.uint8)])
    cap = max(m.shape[1] * m.shape[2] for m in items) + 9
    msk = torch.full((5, cap), 9, dtype=torch.uint8, device='cuda')
    with _launches() as calls:
        assert ops.color_mask_rows(slot, msk, [(3, items[3]), (0, items[0]), (1, items[1])]) is msk      # rows 2, 4: no item
    assert calls == [3]
    got = msk.cpu().numpy()
    for r in (0, 1, 3):
        n = items[r].shape[1] * items[r].shape[2]
        assert np.array_equal(got[r, :n], items[r].dense(pick[r][1])[0].reshape(-1).view(np.uint8)), r
        assert (got[r, n:] == 9).all(), r
    assert (got[2] == 9).all() and (got[4] == 9).all()
    with pytest.raises(ops._lib.FgnHipError):
        ops.color_mask_rows(slot, msk, [(0, items[0]), (0, items[1])])       # one item per row
    with pytest.raises(ops._lib.FgnHipError):
        ops.color_mask_rows(slot, msk[:, :10].contiguous(), [(0, items[0])])  # the window exceeds the capacity
    with pytest.raises(ops._lib.FgnHipError):
        ops.color_masks(slot[:, :5], [(0, items[0])])                        # the image exceeds its slot row
