"""Results at source size, kernels: ``ops.mask_rle_src`` (mask_rle_src_kernel: one launch for a batch
of images of different sizes, the sizes read from device memory) and ``ops.mask_overlap_src``.

Expected values: the boxes are ``fewshot_ds.boxes_to_source`` of the network-frame boxes (numpy on the host), the
strings are ``rle.encode`` of the existing dense paste ``ops.mask_paste`` of those host-scaled boxes at the image's own
size, the counts are numpy sums over the same dense masks.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

from fgn_amd import fewshot_ds as fd
from fgn_amd import rle

pytestmark = pytest.mark.gpu

MS, NET, D = 28, (64, 96), 8
BATCHES = {'mixed': ([(37, 53), (130, 70), (64, 96)], [8, 6, 8]),       # both up / one down, one up / identity
           'thin': ([(1, 200), (200, 1)], [7, 8])}
SEMANTICS = [(True, 0.5), (False, 0.5), (False, 0.3), (False, 0.0)]      # (skip_empty, thr)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """prob [B*D,MS,MS], network-frame boxes [B*D,5] (x0,y0,x1,y1,score), sizes, counts.  Per image: two random interior
    boxes, one covering the image, one hanging over all four edges, zero width, zero height, fully outside, sub-pixel -
    rotated by the image index, so that every kind also sits below the count of an image whose count is short."""
    sizes, counts = BATCHES[name]
    H, W = NET
    g = torch.Generator().manual_seed(17 + len(sizes))
    prob, boxes = [], []
    for b in range(len(sizes)):
        p = torch.rand(D, MS, MS, generator=g)
        x0, y0 = torch.rand(2, generator=g) * W * 0.6, torch.rand(2, generator=g) * H * 0.6
        bw, bh = torch.rand(2, generator=g) * W * 0.35 + 3, torch.rand(2, generator=g) * H * 0.35 + 3
        rows = [[x0[0], y0[0], x0[0] + bw[0], y0[0] + bh[0]], [x0[1], y0[1], x0[1] + bw[1], y0[1] + bh[1]],
                [0., 0., W, H], [-7.3, -5.1, W + 9.7, H + 3.2], [W * 0.31, H * 0.2, W * 0.31, H * 0.8],
                [W * 0.2, H * 0.43, W * 0.7, H * 0.43], [W + 5., H + 4., W + 30., H + 20.],
                [W * 0.5 + 0.2, H * 0.5 + 0.3, W * 0.5 + 0.7, H * 0.5 + 0.9]]
        p[2] = 1.0                                                        # saturated mask on the covering box
        p[3] = (torch.rand(MS, MS, generator=g) > 0.4).float()
        bx = torch.tensor([[float(v) for v in r] + [0.5] for r in rows])
        order = [(i + 3 * b) % D for i in range(D)]
        prob.append(p[order])
        boxes.append(bx[order])
    return torch.cat(prob).contiguous(), torch.cat(boxes).contiguous(), sizes, counts


@functools.lru_cache(maxsize=None)
def _host_boxes(name):
    _, boxes, sizes, _ = _inputs(name)
    out = [fd.boxes_to_source(np.ascontiguousarray(boxes[b * D:(b + 1) * D, :4].numpy()), hw, NET, order='xyxy')
           for b, hw in enumerate(sizes)]
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _dense(name, skip_empty, thr):
    """The reference operand, once per case: the existing dense paste of the host-scaled boxes at each image's size."""
    from fgn_amd import ops
    prob, _, sizes, _ = _inputs(name)
    hb = torch.from_numpy(_host_boxes(name).copy())
    out = []
    for b, (h, w) in enumerate(sizes):
        m = ops.mask_paste(prob[b * D:(b + 1) * D].cuda(), hb[b * D:(b + 1) * D].cuda().contiguous(), h, w, thr,
                           skip_empty=skip_empty).cpu().numpy().astype(bool)
        m.setflags(write=False)
        out.append(m)
    return out


def _run(name, skip_empty, thr, with_boxes=True):
    from fgn_amd import ops
    prob, boxes, sizes, counts = _inputs(name)
    hw = torch.tensor(sizes, dtype=torch.int32).cuda()
    n_dev = torch.tensor(counts, dtype=torch.int32).cuda()
    bs = torch.full((len(sizes) * D, 4), -1.0).cuda() if with_boxes else None
    by, ln, ovf = ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw, NET, thr, n_dev, skip_empty=skip_empty, boxes_src_out=bs)
    assert by.dtype == torch.uint8 and tuple(by.shape) == (len(sizes) * D, ops.RLE_BYTE_CAP)
    assert ln.dtype == ovf.dtype == torch.int32 and tuple(ln.shape) == tuple(ovf.shape) == (len(sizes) * D,)
    return by.cpu().numpy(), ln.cpu().numpy(), ovf.cpu().numpy(), None if bs is None else bs.cpu().numpy()


@pytest.mark.parametrize('skip_empty,thr', SEMANTICS)
@pytest.mark.parametrize('name', sorted(BATCHES))
def test_strings_equal_the_dense_paste_of_host_scaled_boxes(name, skip_empty, thr):
    _, _, sizes, counts = _inputs(name)
    by, ln, ovf, bs = _run(name, skip_empty, thr)
    assert bs.dtype == np.float32 and bs.tobytes() == _host_boxes(name).tobytes()
    dense = _dense(name, skip_empty, thr)
    assert not ovf.any()
    n_set = 0
    for b, (h, w) in enumerate(sizes):
        for d in range(D):
            r = b * D + d
            if d >= counts[b]:
                assert ln[r] == 0, (b, d)
                continue
            want = rle.encode(dense[b][d])
            assert want['size'] == [h, w]
            assert by[r, :ln[r]].tobytes() == want['counts'], (b, d)
            n_set += int(dense[b][d].any())
    assert n_set >= len(sizes) * 3                      # the cases paste something
    if thr == 0.0:                                      # whole-image semantic: thr = 0 sets every pixel
        assert all(m.all() for m in dense)


def test_the_identity_image_gives_the_bytes_of_mask_rle():
    from fgn_amd import ops
    prob, boxes, sizes, counts = _inputs('mixed')
    b = sizes.index(NET)
    for skip_empty, thr in SEMANTICS[:3]:
        by, ln, ovf, bs = _run('mixed', skip_empty, thr)
        p, bx = prob[b * D:(b + 1) * D].cuda(), boxes[b * D:(b + 1) * D].cuda()
        cnt = torch.tensor([counts[b]], dtype=torch.int32).cuda()
        by0, ln0, ovf0 = (t.cpu().numpy() for t in ops.mask_rle(p, bx, *NET, thr, cnt, skip_empty=skip_empty))
        assert bs[b * D:(b + 1) * D].tobytes() == boxes[b * D:(b + 1) * D, :4].contiguous().numpy().tobytes()
        assert np.array_equal(ln[b * D:(b + 1) * D], ln0) and ln0[:counts[b]].all()
        assert np.array_equal(ovf[b * D:(b + 1) * D], ovf0)
        for d in range(D):
            assert by[b * D + d, :ln0[d]].tobytes() == by0[d, :ln0[d]].tobytes()


def test_caller_owned_outputs_no_count_and_no_box_output():
    from fgn_amd import ops
    prob, boxes, sizes, counts = _inputs('mixed')
    rows = len(sizes) * D
    hw = torch.tensor(sizes, dtype=torch.int32).cuda()
    out = (torch.empty((len(sizes), D, ops.RLE_BYTE_CAP), dtype=torch.uint8, device='cuda'),
           torch.zeros((len(sizes), D), dtype=torch.int32, device='cuda'),
           torch.zeros((len(sizes), D), dtype=torch.int32, device='cuda'))
    got = ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw, NET, 0.5, None, out=out)       # no count: all D rows
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    by, ln = out[0].cpu().numpy().reshape(rows, -1), out[1].cpu().numpy().reshape(rows)
    dense = _dense('mixed', True, 0.5)
    for b in range(len(sizes)):
        for d in range(D):
            r = b * D + d
            assert by[r, :ln[r]].tobytes() == rle.encode(dense[b][d])['counts'], (b, d)


def test_an_image_outside_the_size_contract_comes_out_empty():
    """Sizes outside 1..16384 (the host refuses them earlier): lengths 0, overflow 0, zero boxes, nothing of the image
    is read; the other images of the batch are untouched by it."""
    from fgn_amd import ops
    prob, boxes, sizes, counts = _inputs('mixed')
    hw = torch.tensor([[0, 53], [130, 16385], list(sizes[2])], dtype=torch.int32).cuda()
    bs = torch.full((3 * D, 4), -1.0).cuda()
    by, ln, ovf = ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw, NET, 0.5, None, boxes_src_out=bs)
    ln, ovf, bs = ln.cpu().numpy(), ovf.cpu().numpy(), bs.cpu().numpy()
    assert not ln[:2 * D].any() and not ovf.any() and not bs[:2 * D].any()
    dense = _dense('mixed', True, 0.5)
    by = by.cpu().numpy()
    for d in range(D):
        assert by[2 * D + d, :ln[2 * D + d]].tobytes() == rle.encode(dense[2][d])['counts']


def test_wrapper_refuses_what_the_kernel_cannot_index():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    prob, boxes, sizes, _ = _inputs('mixed')
    hw = torch.tensor(sizes, dtype=torch.int32)
    with pytest.raises(FgnHipError):
        ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw, NET, 0.5)                         # sizes on the host
    with pytest.raises(FgnHipError):
        ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw[:2].cuda().long(), NET, 0.5)
    with pytest.raises(FgnHipError):
        ops.mask_rle_src(prob[:-1].cuda(), boxes[:-1].cuda(), hw.cuda(), NET, 0.5)        # rows no multiple of B
    with pytest.raises(FgnHipError):
        ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw.cuda(), (0, 96), 0.5)
    with pytest.raises(FgnHipError):
        ops.mask_rle_src(prob.cuda(), boxes.cuda(), hw.cuda(), NET, 0.5, boxes_src_out=torch.zeros(3, 4).cuda())
    with pytest.raises(FgnHipError):
        ops.mask_overlap_src(prob[:D].cuda(), boxes[:D].cuda(), torch.zeros(2, 37, 53, dtype=torch.bool).cuda(),
                             (37, 54), NET, 0.5)


@functools.lru_cache(maxsize=None)
def _ground_truth(h, w, n):
    g = torch.Generator().manual_seed(1000 * h + w + n)
    gt = torch.rand(n, h, w, generator=g) > (0.2 + 0.6 * torch.rand(n, 1, 1, generator=g))
    gt[0] = True
    if n > 1:
        gt[1] = False
    return gt


@pytest.mark.parametrize('n_gt', [3, 70])
@pytest.mark.parametrize('skip_empty,thr', SEMANTICS[:3])
@pytest.mark.parametrize('name', sorted(BATCHES))
def test_overlap_counts_at_source_size(name, skip_empty, thr, n_gt):
    from fgn_amd import ops
    prob, boxes, sizes, counts = _inputs(name)
    dense = _dense(name, skip_empty, thr)
    for b, (h, w) in enumerate(sizes):
        gt = _ground_truth(h, w, n_gt)
        cnt = torch.tensor([counts[b]], dtype=torch.int32).cuda()
        p, bx = prob[b * D:(b + 1) * D].cuda(), boxes[b * D:(b + 1) * D].cuda()
        inter, da, ga = ops.mask_overlap_src(p, bx, gt.cuda(), (h, w), NET, thr, cnt, skip_empty=skip_empty)
        assert inter.dtype == da.dtype == ga.dtype == torch.int32 and tuple(inter.shape) == (D, n_gt)
        m = dense[b].copy()
        m[counts[b]:] = False                           # rows at or beyond the count are zero
        g = gt.numpy()
        want = np.array([[np.count_nonzero(a & c) for c in g] for a in m], np.int64)
        assert np.array_equal(ga.cpu().numpy(), g.reshape(n_gt, -1).sum(1))
        assert np.array_equal(da.cpu().numpy(), m.reshape(D, -1).sum(1)), (b,)
        assert np.array_equal(inter.cpu().numpy(), want), (b,)
        assert (want[:, 0] == m.reshape(D, -1).sum(1)).all() and want.any()
    # the bit planes as mask_bits made them are accepted in place of the masks, and the identity image gives the counts
    # of the existing mask_overlap
    if NET in sizes:
        b = sizes.index(NET)
        gt = _ground_truth(*NET, n_gt).cuda()
        p, bx = prob[b * D:(b + 1) * D].cuda(), boxes[b * D:(b + 1) * D].cuda()
        a = ops.mask_overlap_src(p, bx, ops.mask_bits(gt), NET, NET, thr, skip_empty=skip_empty, packed=True)[3]
        c = ops.mask_overlap(p, bx, gt, *NET, thr, skip_empty=skip_empty, packed=True)[3]
        assert torch.equal(a, c)
