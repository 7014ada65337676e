"""Matching on the device: ``ops.mask_overlap`` (mask_bits_kernel + mask_overlap_kernel) against the dense paste.

Expected values are ``(dense[d] & gt[g]).sum()``, ``dense[d].sum()`` and ``gt[g].sum()`` with ``dense`` the output of
``ops.mask_paste`` for the same arguments, summed with numpy on the host.  Integer counts: every comparison is
``array_equal``, every detection and every ground-truth mask of every case is compared."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 12


def _boxes(g, d, h, w):                      # as tests/test_hip_mask.py
    x0 = torch.rand(d, generator=g) * (w * 0.7)
    y0 = torch.rand(d, generator=g) * (h * 0.7)
    bw = torch.rand(d, generator=g) * (w * 0.5) + 2
    bh = torch.rand(d, generator=g) * (h * 0.5) + 2
    return torch.stack([x0, y0, (x0 + bw).clamp(max=w), (y0 + bh).clamp(max=h), torch.rand(d, generator=g)], 1)


@functools.lru_cache(maxsize=None)
def _detections(h, w, zero_width=False):
    g = torch.Generator().manual_seed(11)
    prob = torch.rand(D, 14, 14, generator=g)
    boxes = _boxes(g, D, h, w)
    prob[0] = 1.0                                                     # saturated mask on a full-image box
    boxes[0, :4] = torch.tensor([0., 0., float(w), float(h)])
    prob[1] = 0.0                                                     # all-zero mask
    boxes[2, :4] = torch.tensor([w * 0.25, 0., w * 0.75, float(h)])   # full height
    prob[2] = (torch.rand(14, 14, generator=g) > 0.4).float()
    boxes[3, :4] = torch.tensor([w * 0.4, h * 0.5, float(w), float(h)])   # touches the bottom and right edges
    prob[3] = 1.0
    x0 = min(w * 0.3 + 0.3, 70.3) if w > 80 else w * 0.3 + 0.3        # starts at an x that is no multiple of 64
    boxes[4, :4] = torch.tensor([x0, h * 0.2, min(x0 + w * 0.55, float(w)), h * 0.9])
    prob[4] = 1.0
    iy, ix = torch.meshgrid(torch.arange(14), torch.arange(14), indexing='ij')
    prob[5] = ((iy + ix) % 2).float()                                 # checkerboard probability map
    if zero_width:
        boxes[6, :4] = torch.tensor([w * 0.3, h * 0.2, w * 0.3, h * 0.8])   # zero width (make_paste_box: whole axis)
    return prob, boxes


@functools.lru_cache(maxsize=None)
def _ground_truth(h, w, n=5):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    corners = torch.zeros(h, w, dtype=torch.bool)
    corners[0, 0] = corners[h - 1, 0] = corners[0, w - 1] = corners[h - 1, w - 1] = True
    masks = [((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2 <= 1,          # ellipse
             torch.zeros(h, w, dtype=torch.bool), torch.ones(h, w, dtype=torch.bool),     # empty, full
             (yy + xx) % 2 == 0, corners]                                                 # checkerboard, four corners
    g = torch.Generator().manual_seed(5)
    while len(masks) < n:
        masks.append(torch.rand(h, w, generator=g) > 0.5 + 0.4 * torch.rand((), generator=g))
    return torch.stack(masks[:n])


@functools.lru_cache(maxsize=None)
def _dense(h, w, thr, skip_empty, zero_width=False):
    """the reference operand, computed once per case and shared: the existing dense paste for the same arguments"""
    from fgn_amd import ops
    prob, boxes = _detections(h, w, zero_width)
    out = ops.mask_paste(prob.cuda(), boxes.cuda(), h, w, thr, skip_empty=skip_empty).cpu().numpy().astype(bool)
    out.setflags(write=False)
    return out


def _expect(dense, gt):
    gt = np.asarray(gt).astype(bool)
    inter = np.array([[np.count_nonzero(d & g) for g in gt] for d in dense], np.int64).reshape(len(dense), len(gt))
    return inter, dense.reshape(len(dense), -1).sum(1), gt.reshape(len(gt), -1).sum(1)


def _check(h, w, thr, skip_empty, n_gt=5, as_uint8=False, zero_width=False):
    from fgn_amd import ops
    prob, boxes = _detections(h, w, zero_width)
    gt = _ground_truth(h, w, n_gt)
    gt_dev = (gt.to(torch.uint8) if as_uint8 else gt).cuda()
    inter, da, ga = ops.mask_overlap(prob.cuda(), boxes.cuda(), gt_dev, h, w, thr, skip_empty=skip_empty)
    assert inter.dtype == da.dtype == ga.dtype == torch.int32
    assert tuple(inter.shape) == (D, n_gt) and tuple(da.shape) == (D,) and tuple(ga.shape) == (n_gt,)
    dense = _dense(h, w, thr, skip_empty, zero_width)
    want = _expect(dense, gt.numpy())
    assert np.array_equal(ga.cpu().numpy(), want[2])
    assert np.array_equal(da.cpu().numpy(), want[1])
    assert np.array_equal(inter.cpu().numpy(), want[0])
    return dense, want


@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('hw', [(16, 16), (130, 7), (37, 50), (97, 131)])
def test_overlap_counts_equal_the_dense_paste(hw, skip_empty):
    dense, want = _check(*hw, 0.5, skip_empty)
    # the cases are what they claim to be.  Detection 3 reaches the last row and the last column; the corner pixel
    # itself samples past the 14x14 map on both axes and may fall below thr, so it is not asked for.
    assert dense[0].mean() > 0.8 and not dense[1].any() and dense[3][-1].any() and dense[3][:, -1].any()
    assert want[2].tolist()[1:3] == [0, hw[0] * hw[1]] and want[2][4] == 4
    assert (want[0][:, 2] == want[1]).all() and not want[0][:, 1].any()      # full / empty ground truth


def test_overlap_counts_at_the_real_geometry():
    _check(800, 1333, 0.5, True)


def test_uint8_ground_truth_gives_the_same_counts():
    _check(97, 131, 0.5, True, as_uint8=True)


@pytest.mark.parametrize('hw', [(37, 50), (97, 131)])
def test_whole_image_semantic_special_cases(hw):
    """``skip_empty = 0``: thr = 0 sets the whole image, a box of zero width samples the mask's centre line in every
    column - the cases ``make_paste_box`` treats specially."""
    h, w = hw
    dense, want = _check(h, w, 0.0, False)
    assert dense.all() and (want[1] == h * w).all()
    dense, _ = _check(h, w, 0.5, False, zero_width=True)
    cols = dense[6].any(0)
    assert cols.all() or not cols.any()          # the zero-width box: every column of the image alike
    _check(h, w, 0.5, True, zero_width=True)


@pytest.mark.parametrize('n_gt', [1, 70])
def test_one_and_more_than_sixty_four_ground_truth_masks(n_gt):
    _check(37, 50, 0.5, True, n_gt=n_gt)


def test_empty_operands_return_empty_tensors():
    from fgn_amd import ops
    h, w = 37, 50
    prob, boxes = _detections(h, w)
    gt = _ground_truth(h, w)
    inter, da, ga = ops.mask_overlap(prob.cuda(), boxes.cuda(), torch.zeros(0, h, w, dtype=torch.bool, device='cuda'),
                                     h, w, 0.5)
    assert tuple(inter.shape) == (D, 0) and tuple(da.shape) == (D,) and tuple(ga.shape) == (0,)
    inter, da, ga = ops.mask_overlap(prob[:0].cuda(), boxes[:0].cuda(), gt.cuda(), h, w, 0.5)
    assert tuple(inter.shape) == (0, 5) and tuple(da.shape) == (0,) and tuple(ga.shape) == (5,)
    assert np.array_equal(ga.cpu().numpy(), gt.numpy().reshape(5, -1).sum(1))
    assert inter.dtype == da.dtype == ga.dtype == torch.int32


def test_rows_beyond_the_device_count_are_zero():
    from fgn_amd import ops
    h, w = 97, 131
    prob, boxes = _detections(h, w)
    prob, boxes = prob[[0, 4, 3]].contiguous(), boxes[[0, 4, 3]].contiguous()
    gt = _ground_truth(h, w)
    cnt = torch.tensor([2], dtype=torch.int32, device='cuda')
    inter, da, ga = ops.mask_overlap(prob.cuda(), boxes.cuda(), gt.cuda(), h, w, 0.5, cnt)
    dense = _dense(h, w, 0.5, True)[[0, 4, 3]]
    want = _expect(dense, gt.numpy())
    assert want[1][2] > 0 and want[0][2].any()              # the row would not be zero without the count
    want[0][2] = 0
    want[1][2] = 0
    assert np.array_equal(inter.cpu().numpy(), want[0])
    assert np.array_equal(da.cpu().numpy(), want[1])
    assert np.array_equal(ga.cpu().numpy(), want[2])
