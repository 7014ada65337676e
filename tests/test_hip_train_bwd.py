"""Every backward kernel of the trainable heads (csrc/train_bwd.hip) alone against the float64 closed forms of
tests/_bwd_ref.py, bounded PER OUTPUT ELEMENT:

    |got - ref| <= c * 2^-24 * mag + 2^-126

``mag`` is that element's own term-magnitude sum (the reference expression with every term replaced by its absolute
value), ``c`` the number of fp32 roundings counted in the kernel's arithmetic (each docstring derives it; first-order
counts are rounded up to cover the second-order terms), 2^-126 the smallest normal fp32 (a result below it may lose
its last bits).  Nothing is normalised by a tensor's range: a term that is wrong only where the tensor is small fails.
Every test prints ``[bwd-bound] name: worst |err| / bound`` before it asserts (DESIGN.md section 7 carries the table).
Then the host-side helpers of fgn_amd/train.py that turn forward kernels into gradient kernels, and two stages (mask
head, AG-RPN) on identical inputs against float64 autograd.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bwd_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
TINY = ref.TINY
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(name, ratio, extra=''):
    print(f'[bwd-bound] {name}: worst |err| / bound = {ratio:.4f}{extra}')


def _bounded(name, got, want, mag, c, keep=None, slack=None):
    """Assert |got - want| <= c * 2^-24 * mag (+ slack) + 2^-126 for every element (of ``keep``); -> the worst ratio."""
    got = got.detach().cpu().to(F64).reshape(want.shape)
    assert bool(torch.isfinite(got).all()), name
    if want.numel() == 0:
        _report(name, 0.0, ' (empty)')
        return 0.0
    bound = c * U * mag + TINY
    if slack is not None:
        bound = bound + slack
    ratio = (got - want).abs() / bound
    if keep is not None:
        ratio = ratio[keep]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _report(name, worst, f' (c = {c})')
    assert worst <= 1.0, (name, worst)
    return worst


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b.to(torch.float32)))


# ------------------------------------------------------------------------------------------ loss gradients
_BCE_SPECIAL = [0.0, 1e-3, 1.0, 20.0, 90.0, 104.0]


@pytest.mark.parametrize('n', [1, 255, 257, 1048576 + 3])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('thr', [-1.0, 0.5])
def test_bce_logits_grad_per_element(n, weighted, thr):
    """dx = (sigmoid(x) - y) * w * scale.  The kernel evaluates the sigmoid in fp64 and rounds it to fp32 (1), subtracts
    (1), multiplies by w (1) and by scale (1): 4 roundings, each at most 2^-24 of (sigmoid + y) |w scale|; c = 5.
    x = +-{0, 1e-3, 1, 20, 90, 104} (sigmoid(-104) is below the fp32 range) and random; soft targets exactly at the
    threshold 0.5 count as 1; 1 048 579 elements take the grid-stride path of the 4096-block grid."""
    from fgn_amd import ops
    g = _gen(100 + n % 97)
    sp = torch.tensor([s * v for v in _BCE_SPECIAL for s in (1.0, -1.0)])
    x = torch.randn(n, generator=g) * 6
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n > 2 * sp.numel():
        x[-sp.numel():] = sp                                   # the tail: reached through the grid stride
    y = torch.rand(n, generator=g)
    y[::3] = 0.5
    y[1::7] = 0.0
    y[2::11] = 1.0
    w = (torch.rand(n, generator=g) * 2).contiguous() if weighted else None
    scale = 1.0 / 384
    want, mag = ref.bce_grad(x, y, w, scale, thr)
    got = ops.bce_logits_grad(x.cuda(), y.cuda(), None if w is None else w.cuda(), scale, y_threshold=thr)
    assert got.shape == x.shape
    _bounded(f'bce_logits_grad n={n} w={weighted} thr={thr}', got, want, mag, 5)
    if thr >= 0:                                               # a target exactly at the threshold is a positive
        s0 = float(torch.sigmoid(x[0].double()))
        assert float(got[0].cpu()) == pytest.approx((s0 - 1.0) * (float(w[0]) if weighted else 1.0) * ref.f32(scale), rel=1e-6)


def test_bce_logits_grad_of_nothing_is_empty():
    from fgn_amd import ops
    e = torch.empty(0, device='cuda')
    assert ops.bce_logits_grad(e, e.clone(), None, 1.0).shape == (0,)


@pytest.mark.parametrize('beta', [1.0, 1.0 / 9])
@pytest.mark.parametrize('n', [64, 1048576 + 5])
def test_smooth_l1_grad_per_element(beta, n):
    """g = d / beta for |d| < beta, else sign(d); d = pred - target (1 rounding), division (1), * w (1), * scale (1):
    c = 5 on |g| |w scale|.  The gradient is continuous at |d| = beta, so a difference that rounds across the kink moves
    the result by one rounding of d.  d = 0 exactly (result 0 bit for bit), |d| = beta and beta +- 1 ulp on both signs."""
    from fgn_amd import ops, lib
    g = _gen(7)
    b = np.float32(beta)
    up, dn = np.nextafter(b, np.float32(2)), np.nextafter(b, np.float32(0))
    sp = torch.tensor([0.0, float(b), -float(b), float(up), -float(up), float(dn), -float(dn), 0.5 * float(b), -0.5 * float(b),
                       3.0, -3.0], dtype=torch.float32)
    p = torch.randn(n, generator=g)
    t = torch.randn(n, generator=g)
    k = sp.numel()
    p[:k], t[:k] = sp, 0.0
    p[k:2 * k] = sp + 0.75                                      # the same differences off the origin: 0.75 + d - 0.75
    t[k:2 * k] = 0.75
    p[-k:], t[-k:] = sp, 0.0
    w = torch.rand(n, generator=g) * 2
    for ww in (None, w):
        want, mag = ref.smooth_l1_grad(p, t, ww, 1.0 / 96, beta)
        got = ops.smooth_l1_grad(p.cuda(), t.cuda(), None if ww is None else ww.cuda(), 1.0 / 96, beta=beta)
        _bounded(f'smooth_l1_grad n={n} beta={beta:.3f} w={ww is not None}', got, want, mag, 5)
        gc = got.cpu()
        assert _same_bits(gc[0:1], torch.zeros(1)) and _same_bits(gc[-k:-k + 1], torch.zeros(1))
        k1 = ref.f32(1.0 / 96)
        if ww is None:                                         # |d| = beta and beta + 1 ulp: the linear branch, exactly +-scale
            assert gc[1:5].tolist() == [k1, -k1, k1, -k1]
    with pytest.raises(lib.FgnHipError):
        ops.smooth_l1_grad(p[:8].cuda(), t[:8].cuda(), None, 1.0, beta=0.0)


@pytest.mark.parametrize('C', [1, 2, 4, 9])
@pytest.mark.parametrize('n', [1, 256, 257, 5000])
def test_softmax_ce_grad_per_element(C, n):
    """dl = (softmax - onehot) * w * scale.  The kernel forms delta = r - max in fp32 (relative error 2^-24 of |delta|, which
    the exponential turns into a RELATIVE error |delta| 2^-24 of that term and, weighted by p, of the normaliser), sums the
    exponentials in fp64, rounds p (1), subtracts the one-hot (1), forms w * scale (1) and the product (1):
    |err| <= 2^-24 |k| [p (|delta_c| + sum |delta| p) + p + 3 (p + onehot)] <= 4 * 2^-24 * mag;  c = 5.
    Logits spread over +-60 (exp(-120) underflows fp32); labels -1 and C give all-zero rows bit for bit."""
    from fgn_amd import ops
    g = _gen(300 + 10 * C + n % 7)
    z = torch.randn(n, C, generator=g) * 5
    z[::4] = torch.rand(z[::4].shape, generator=g) * 120 - 60
    lab = torch.randint(0, C, (n,), generator=g)
    if n >= 256:
        lab[5], lab[77] = -1, C
    w = torch.rand(n, generator=g) * 2
    for ww in (None, w):
        want, mag, p = ref.softmax_ce_grad(z, lab, ww, 1.0 / 128)
        got = ops.softmax_ce_grad(z.cuda(), lab.cuda(), None if ww is None else ww.cuda(), 1.0 / 128)
        _bounded(f'softmax_ce_grad n={n} C={C} w={ww is not None}', got, want, mag, 5)
        gc = got.cpu()
        if n >= 256:
            assert _same_bits(gc[5], torch.zeros(C)) and _same_bits(gc[77], torch.zeros(C))
        # every row sums to (sum p - 1) k = the reference's row sum, within the row's summed bounds
        rows = (gc.to(F64).sum(1) - want.sum(1)).abs() / ((5 * U * mag + TINY).sum(1))
        _report(f'softmax_ce_grad row sums n={n} C={C}', float(rows.max()))
        assert float(rows.max()) <= 1.0


# ------------------------------------------------------------------------------------------ ReLU backward (bit-exact)
@pytest.mark.parametrize('n', [4, 1028, 4194304 + 4004])
def test_relu_backward_bit_exact(n):
    """out = dy where y > 0 else +0.0: +0.0, -0.0, negatives and negative denormals pass nothing, positive denormals pass
    dy.  4 198 308 elements: more float4 than the 4096 x 256 threads of the clamped grid, so the loop strides."""
    from fgn_amd import ops, lib
    g = _gen(11)
    y = torch.randn(n, generator=g)
    sp = torch.tensor([0.0, -0.0, 1e-42, -1e-42, 1.4e-45, -1.0, 1.0, -3e-39, 3e-39, 2.0 ** -126, -2.0 ** -126, 0.0])
    k = min(n, sp.numel())
    y[:k] = sp[:k]
    if n > 2 * sp.numel():
        y[-sp.numel():] = sp
    dy = torch.randn(n, generator=g)
    got = ops.relu_backward(dy.cuda(), y.cuda())
    want = ref.relu_backward(dy, y).float()
    assert _same_bits(got, want)
    with pytest.raises(lib.FgnHipError):
        ops.relu_backward(torch.ones(6, device='cuda'), torch.ones(6, device='cuda'))


# ------------------------------------------------------------------------------------------ column sums
def _cancel_column(R):
    """+1e4 / -1e4 alternating around ONE 1e-3 in the middle: the sum is 1e-3 (or 1e-3 +- 1e4 for an odd count of big
    values - then the last is zero).  Every fp64 partial sum stays below 2^14 + 2^-10: exact in fp64 in row order."""
    col = torch.zeros(R)
    if R == 0:
        return col
    mid = R // 2
    idx = torch.tensor([i for i in range(R) if i != mid], dtype=torch.long)
    idx = idx[:idx.numel() // 2 * 2]
    col[idx[0::2]] = 1e4
    col[idx[1::2]] = -1e4
    col[mid] = 1e-3
    return col


def _colsum_case(R, C):
    g = _gen(1000 + R % 101 + C)
    # multiples of 2^-12 below 8: every partial sum is exact in fp64 whatever the order (reference and kernel alike)
    x = torch.randint(-(1 << 15), 1 << 15, (R, C), generator=g, dtype=torch.int32).float() * 2.0 ** -12
    exact = []
    if R:
        x[:, 0] = _cancel_column(R)
        exact.append(0)
        if C > 2:
            x[:, C - 1] = -_cancel_column(R)
            exact.append(C - 1)
    want, _ = ref.colsum(x, exact_cols=tuple(exact))
    return x, want


@pytest.mark.parametrize('C', [1, 6, 255, 256, 257, 1024])
@pytest.mark.parametrize('R', [0, 1, 63, 64, 65, 6272, 100003])
def test_colsum_is_the_fp64_sum_rounded_once(R, C):
    """fp64 partials over 64 row chunks, summed in fp64, rounded to fp32 once: the result is the exact sum rounded, so
    within 1 ulp of it (the data keeps every fp64 addition exact: multiples of 2^-12, and two columns of +-1e4 around one
    1e-3 whose exact sum math.fsum supplies).  Fewer rows than chunks, rows not a multiple of 64, C across the
    256-column block.  ``accumulate`` adds one rounded sum to ``out``: a second rounding, 2 ulp of the larger of the two.
    Two runs give the same bits."""
    from fgn_amd import ops
    x, want = _colsum_case(R, C)
    xd = x.cuda()
    got = ops.colsum(xd)
    assert got.shape == (C,)
    err = (got.cpu().to(F64) - want).abs()
    ulp = ref.ulp32(want)
    worst = float((err / ulp).max())
    _report(f'colsum R={R} C={C} (ulp)', worst)
    assert worst <= 1.0
    if R:
        assert float(want[0]) == float(torch.tensor(1e-3))                        # the big values cancel exactly
    assert _same_bits(ops.colsum(xd), got.cpu())
    out0 = torch.randn(C, generator=_gen(5)) * 3
    out = out0.clone().cuda()
    r = ops.colsum(xd, out=out, accumulate=True)
    assert r.data_ptr() == out.data_ptr()
    tot = want + out0.to(F64)
    err = (out.cpu().to(F64) - tot).abs()
    tol = 2 * torch.maximum(ref.ulp32(want), ref.ulp32(tot))
    _report(f'colsum accumulate R={R} C={C} (of 2 ulp)', float((err / tol).max()))
    assert bool((err <= tol).all())
    out2 = out0.clone().cuda()
    ops.colsum(xd, out=out2, accumulate=False)
    assert _same_bits(out2, got.cpu())


# ------------------------------------------------------------------------------------------ BatchNorm (train) backward
_BN_SHAPES = [(3, 64), (63, 4), (65, 260), (441, 1024), (6272, 512), (6273, 128), (8200, 512)]


@functools.lru_cache(maxsize=1)                                # the two y_post cases of a shape run back to back
def _bn_case(P, C):
    g = _gen(2000 + P % 89 + C)
    x = torch.randn(P, C, generator=g)
    x[:, 1] = x[:, 1] * 1e-4                                    # variance ~1e-8: rstd = 1 / sqrt(eps + 1e-8)
    x[:, 2] = x[:, 2] + 1e3                                     # mean 1e3: x - mean cancels 3 digits
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[3] = -gamma[3]
    beta = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(P, C, generator=g)
    mean = x.to(F64).mean(0).float()
    var = x.to(F64).var(0, unbiased=False).float()
    eps = 1e-5
    y = torch.relu((x - mean) / torch.sqrt(var + eps) * gamma + beta)
    y[0, :] = 0.0                                              # a row of exact zeros
    refs = {post: ref.bn_train_backward(x, y if post else None, dy, mean, var, gamma, eps) for post in (False, True)}
    return x, y, dy, mean, var, gamma, eps, refs


@pytest.mark.parametrize('post', [False, True])
@pytest.mark.parametrize('P,C', _BN_SHAPES)
def test_bn_train_backward_per_element(P, C, post):
    """rstd = 1 / sqrt(var + eps): add (1, halved by the root), sqrt (1), divide (1) -> 2.5;  xhat = (x - mean) rstd: 4.5.
    dbeta: fp64 sums, one rounding; c = 2 on sum |g| (the second for the fp64 additions).
    dgamma: each fp64 term g * xhat carries xhat's 4.5, one rounding at the end: 5.5 -> c = 6 on sum |g xhat|.
    dx = gamma rstd (g - dbeta / P - xhat dgamma / P): dbeta / P carries 1 + 1 (1 / P) + 1 = 3 on sum|g| / P;
    xhat dgamma / P carries 4.5 + 6 + 2 + 1 = 13.5 on |xhat| sum|g xhat| / P; the two subtractions 2 and gamma rstd times
    the bracket 4.5 on the whole: at most 13.5 + 2 + 4.5 = 20 on mag_dx = |gamma rstd| (|g| + sum|g| / P + |xhat| sum|g xhat| / P).
    Rows below the 64 chunks, not a multiple of the 4 row phases, C / 4 across the 64-lane block, 4 198 400 elements
    (grid stride of the apply kernel).  g (``want_g``) is dy masked by y_post > 0, bit for bit.  The column sums of dx
    and of dx * xhat (zero up to the rounding of the mean / var operands) match the reference's within the summed
    bounds.  Two runs give the same bits."""
    from fgn_amd import ops
    x, y, dy, mean, var, gamma, eps, refs = _bn_case(P, C)
    r = refs[post]
    dev = lambda t: t.cuda().contiguous()
    args = (dev(x), dev(y) if post else None, dev(dy), dev(mean), dev(var), dev(gamma), eps)
    dx, dg, db, gm = ops.bn_train_backward(*args, want_g=True)
    tag = f'bn_train_backward P={P} C={C} y_post={post}'
    _bounded(tag + ' dbeta', db, r['dbeta'], r['mag_dbeta'], 2)
    _bounded(tag + ' dgamma', dg, r['dgamma'], r['mag_dgamma'], 6)
    _bounded(tag + ' dx', dx, r['dx'], r['mag_dx'], 20)
    assert _same_bits(gm, r['g'])
    dx64 = dx.cpu().to(F64)
    bound = 20 * U * r['mag_dx'] + TINY
    s0 = (dx64.sum(0) - r['dx'].sum(0)).abs() / bound.sum(0)
    s1 = ((dx64 * r['xhat']).sum(0) - (r['dx'] * r['xhat']).sum(0)).abs() / (bound * r['xhat'].abs()).sum(0)
    _report(tag + ' column sums of dx, dx * xhat', max(float(s0.max()), float(s1.max())))
    assert float(s0.max()) <= 1.0 and float(s1.max()) <= 1.0
    # ... and are zero to the size of the terms that cancel in them
    assert bool((r['dx'].sum(0).abs() <= 1e-4 * r['mag_dx'].sum(0)).all())
    dx2, dg2, db2 = ops.bn_train_backward(*args)
    assert _same_bits(dx2, dx.cpu()) and _same_bits(dg2, dg.cpu()) and _same_bits(db2, db.cpu())


# ------------------------------------------------------------------------------------------ relation / box head backward
_REL_SHAPES = [(9, 3, 256, 8), (40, 8, 1024, 32), (33, 5, 512, 32), (17, 1, 128, 16), (20, 2, 64, 8), (12, 4, 32, 1)]
C_XHAT = 96


def _rel_operands(R, N, C, seed=22):
    """The distributions of test_relation_head_backward_alone_matches_autograd; 3 images, unsorted, image 1 without RoI."""
    g = _gen(seed + R + C)
    B = 3
    q = torch.randn(R, 7, 7, C, generator=g)
    s = torch.randn(B * N, 7, 7, C, generator=g)
    gw = torch.rand(C, generator=g) + 0.5
    gb = torch.randn(C, generator=g) * 0.1
    fcw = torch.randn(6, C, generator=g) * 0.1
    d6 = torch.randn(R * N, 6, generator=g)
    img = torch.tensor([0 if i % 3 == 1 else 2 for i in range(R)]) if R else torch.zeros(0, dtype=torch.long)
    if R > 2:
        img[0] = 2
        img[R - 1] = 0
    rois = torch.cat([img.float()[:, None], torch.zeros(R, 4)], 1)
    return q, s, rois, gw, gb, fcw, d6, img, B


@pytest.mark.parametrize('R,N,C,groups', _REL_SHAPES)
def test_relation_gn_head_backward_per_element(R, N, C, groups):
    """One workgroup per RoI, a wave per 32 channels: C / 32 = 1 .. 32 units on 8 waves (up to 4 trips of the unit loop),
    group widths 32, 16 and 8 (the ``gw >> 3`` shuffle levels), n_ways 1 .. 8.  Roundings, with D = 34 the depth of a
    group sum (28 serial additions per lane + 6 shuffle levels):
      xhat = (x - mean) rstd: x = q + s (1), mean (D + 1), subtraction (1), rstd (variance: D + 1 + twice the error of
        x - mean, halved by the root; + 2.5) and the product (1): <= 96 on xmag = rstd (|x| + mean|x|)   (C_XHAT)
      dp = d6 . fcw / 49: 6 products and additions + 1 / 49 + product: 14 on sum_j |d6_j fcw_j| / 49
      gg = dp gamma (1); m1 = mean gg (D + 2), m2 = mean(gg xhat) (D + 2 + 96 + 1)
      dZ = rstd (gg - m1 - xhat m2): xhat m2 (96 + 133 + 1), two subtractions (2), rstd (56) and the product (1) on top of
        gg's 15: <= 336 on mag_dZ;  dQ = sum_n dZ: + n_ways on sum_n mag_dZ
      pooled = mean_p relu(gamma xhat + beta): 96 + 2, 7 + 3 additions, 1 / 49 (2): 112 on mean_p(|gamma| xmag + |beta|)
      dgamma = sum [pre > 0] dp xhat: 14 + 96 + 1, 7 + 3 + n_ways additions, fp64 column sum (1): 136 on sum G xmag / |gamma|
      dbeta = sum [pre > 0] dp: 14, the same additions: 36 on sum G / |gamma|
    The kernel recomputes the ReLU mask from fp32 pre-activations: a (RoI, class, group) block is left out of dZ (and of dS,
    the per-image sum the RoI stage forms) when the reference pre-activation of any of its elements has
    |pre| <= 16 * 2^-24 (|gamma xhat| + |beta|), a dQ block when any of its classes' blocks is; dgamma / dbeta keep every
    channel and allow such an element's whole term instead.  The left-out share must stay below 2 % of the blocks."""
    from fgn_amd import ops
    q, s, rois, gw, gb, fcw, d6, img, B = _rel_operands(R, N, C)
    r = ref.relation_gn_head_backward(q, s, rois, gw, gb, fcw, d6, N, groups, 1e-5)
    dev = lambda t: t.cuda().contiguous()
    dQ, dZ, pooled, dga, dbe = ops.relation_gn_head_backward(dev(q), dev(s), dev(rois), dev(gw), dev(gb), dev(fcw), dev(d6),
                                                             N, groups, 1e-5)
    gwid = C // groups
    near = r['pre'].abs() <= 16 * U * r['pre_mag']                               # [R,N,7,7,C]
    blk_out = near.view(R, N, 49, groups, gwid).any(dim=4).any(dim=2)            # [R,N,groups]
    dq_out = blk_out.any(dim=1)                                                  # [R,groups]
    share, share_q = float(blk_out.double().mean()), float(dq_out.double().mean())
    tag = f'relation_gn_head_backward R={R} N={N} C={C} groups={groups}'
    print(f'[bwd-bound] {tag}: left out {100 * share:.3f} % of (RoI, class, group) blocks, {100 * share_q:.3f} % of dQ blocks')
    assert share <= 0.02 and share_q <= 0.02
    keepZ = (~blk_out)[:, :, None, None, :, None].expand(R, N, 7, 7, groups, gwid).reshape(R * N, 7, 7, C)
    keepQ = (~dq_out)[:, None, None, :, None].expand(R, 7, 7, groups, gwid).reshape(R, 7, 7, C)
    _bounded(tag + ' dZ', dZ, r['dZ'], r['mag_dZ'], 336, keep=keepZ)
    _bounded(tag + ' dQ', dQ, r['dQ'], r['mag_dQ'], 336 + N, keep=keepQ)
    _bounded(tag + ' pooled', pooled, r['pooled'], r['mag_pooled'], 112)
    # an element inside the margin may take the other branch: its whole term is allowed on top
    flip = near.to(F64)
    dpm = (torch.einsum('rnj,jc->rnc', d6.to(F64).view(R, N, 6).abs(), fcw.to(F64).abs()) / 49).view(R, N, 1, 1, C)
    xh_abs = ((r['pre'] - gb.to(F64)) / gw.to(F64)).abs()
    _bounded(tag + ' dgamma', dga, r['dgamma'], r['mag_dgamma'], 136, slack=(flip * dpm * xh_abs).sum(dim=(0, 1, 2, 3)) * 1.001)
    _bounded(tag + ' dbeta', dbe, r['dbeta'], r['mag_dbeta'], 36, slack=(flip * dpm).sum(dim=(0, 1, 2, 3)) * 1.001)
    # dS as the RoI stage forms it: per image the sum over its RoIs of dZ
    dZc = dZ.cpu().to(F64).view(R, N, 7, 7, C)
    dS, dS_ref, dS_mag = (torch.zeros(B, N, 7, 7, C, dtype=F64) for _ in range(3))
    s_out = torch.zeros(B, N, groups, dtype=torch.bool)
    for i in range(R):
        b = int(img[i])
        dS[b] += dZc[i]
        dS_ref[b] += r['dZ'].view(R, N, 7, 7, C)[i]
        dS_mag[b] += r['mag_dZ'].view(R, N, 7, 7, C)[i]
        s_out[b] |= blk_out[i]
    keepS = (~s_out)[:, :, None, None, :, None].expand(B, N, 7, 7, groups, gwid).reshape(B, N, 7, 7, C)
    _bounded(tag + ' dS', dS, dS_ref, dS_mag, 336 + R, keep=keepS)
    assert float(dS[1].abs().max()) == 0.0                                       # the image without RoI


def test_relation_gn_head_backward_without_rois_is_empty():
    from fgn_amd import ops
    q, s, rois, gw, gb, fcw, d6, img, B = _rel_operands(0, 3, 64)
    dev = lambda t: t.cuda().contiguous()
    dQ, dZ, pooled, dga, dbe = ops.relation_gn_head_backward(dev(q), dev(s), dev(rois), dev(gw), dev(gb), dev(fcw), dev(d6),
                                                             3, 8, 1e-5)
    assert dQ.shape == (0, 7, 7, 64) and dZ.shape == (0, 7, 7, 64) and pooled.shape == (0, 64)
    assert dga.shape == (64,) and float(dga.abs().max()) == 0.0 and float(dbe.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ mask logits backward
@pytest.mark.parametrize('D,P,C', [(0, 7, 256), (1, 7, 4), (5, 7, 256), (3, 14, 260), (100, 7, 256)])
def test_mask_logits_backward_per_element(D, P, C):
    """d_up = dlogit * w where up > 0, else 0: one fp32 product, compared bit for bit (``up`` holds exact zeros and
    negatives).  dw[c] = sum over (detection, pixel, sub-position) of dlogit * up: 4 P^2 fp32 products and additions in
    a row per detection (each partial sum bounded by the magnitude sum) and one rounding of the fp64 column sum over the
    detections: c = 4 P^2 + 1 on sum |dlogit up|."""
    from fgn_amd import ops
    g = _gen(40 + D + C)
    up = torch.randn(D, P, P, 4 * C, generator=g)
    up[:, ::2, :, ::3] = 0.0
    up[:, 1::3, :, 1::5] = -0.0
    dl = torch.randn(D, 2 * P, 2 * P, generator=g) / (4 * P * P)
    w = torch.randn(C, generator=g)
    want_up, want_dw, mag = ref.mask_logits_backward(up, dl, w, P)
    d_up, dw = ops.mask_logits_backward(up.cuda(), dl.cuda(), w.cuda(), P)
    assert d_up.shape == up.shape and dw.shape == (C,)
    assert _same_bits(d_up, want_up)
    _bounded(f'mask_logits_backward D={D} P={P} C={C} dw', dw, want_dw, mag, 4 * P * P + 1)


def test_mask_logits_backward_launcher_refuses_bad_shapes():
    """roi_size <= 0 and C <= 0 are refused by the launcher (FGN_ERR_SHAPE = -1) before anything is launched."""
    from fgn_amd import lib
    L = lib.load()
    t = torch.zeros(64, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    p = t.data_ptr()
    assert L.fgn_mask_logits_backward_f32(p, p, p, p, p, 1, 0, 4, s) == -1
    assert L.fgn_mask_logits_backward_f32(p, p, p, p, p, 1, -7, 4, s) == -1
    assert L.fgn_mask_logits_backward_f32(p, p, p, p, p, 1, 7, 0, s) == -1
    assert L.fgn_mask_logits_backward_f32(p, p, p, p, p, 0, 0, 4, s) == -1
    assert L.fgn_mask_logits_backward_f32(p, p, p, p, p, 0, 7, 4, s) == 0
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ im2col (bit-exact)
@pytest.mark.parametrize('n,H,W,C', [(1, 1, 1, 4), (2, 7, 7, 256), (3, 5, 9, 12), (1, 1, 6, 8), (40, 7, 7, 128), (60, 7, 7, 256)])
def test_im2col3x3_bit_exact(n, H, W, C):
    """Against F.unfold permuted to the (tap, ci) column order; 60 x 7 x 7 x 256 is 1.69 M float4: the grid-stride path."""
    from fgn_amd import ops
    x = torch.randn(n, H, W, C, generator=_gen(50 + n))
    cols = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1)                        # [n, C*9, H*W], row = ci*9 + tap
    want = cols.view(n, C, 9, H * W).permute(0, 3, 2, 1).reshape(n * H * W, 9 * C)
    got = ops.im2col3x3(x.cuda())
    assert got.shape == want.shape and _same_bits(got, want)
    assert torch.equal(want.to(F64), ref.im2col3x3(x))


def test_im2col3x3_refuses_channels_not_a_multiple_of_4():
    from fgn_amd import ops, lib
    with pytest.raises(lib.FgnHipError):
        ops.im2col3x3(torch.zeros(1, 3, 3, 6, device='cuda'))


# ------------------------------------------------------------------------------------------ dgrad / wgrad helpers of train.py
def _conv_grads(x, w, dy, pad, dtype=F64):
    """x [n,H,W,Cin], w [Cout,Cin,k,k], dy [n,H,W,Cout] (NHWC) -> (dx NHWC, dw) by autograd of F.conv2d."""
    X = x.permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
    Wt = w.to(dtype).requires_grad_(True)
    (F.conv2d(X, Wt, padding=pad) * dy.permute(0, 3, 1, 2).to(dtype)).sum().backward()
    return X.grad.permute(0, 2, 3, 1), Wt.grad


def _dot_bounded(name, got, x, w, dy, pad, which, K):
    """The fp32 dot-product bound K * 2^-24 * sum_k |a_k b_k| per output element (K: the reduction length); the magnitude
    sum is the same gradient of |x|, |w|, |dy|."""
    want = _conv_grads(x, w, dy, pad)[which]
    mag = _conv_grads(x.abs(), w.abs(), dy.abs(), pad)[which]
    return _bounded(name, got, want, mag, K)


@pytest.mark.parametrize('rows_shape,cout,cin', [((40, 7, 7), 128, 64), ((9, 7, 7), 64, 256), ((300,), 32, 1024), ((33, 7, 7), 6, 256),
                                                 ((500,), 76, 128)])
def test_dgrad_1x1_helper(rows_shape, cout, cin):
    """``_dgrad_1x1``: the forward convolution kernel on the transposed weight (Cout % 32 == 0) or the small-product kernel
    (Cout = 6: the fc layers, 76: the padded AG-RPN head), packed under the arithmetic a live Trainer uses ('f32')."""
    from fgn_amd import ops, train as TR
    g = _gen(60 + cout)
    dy = torch.randn(*rows_shape, cout, generator=g)
    w2 = torch.randn(cout, cin, generator=g) * 0.1
    with ops.gemm_math('f32'):
        got = TR._dgrad_1x1(dy.cuda(), w2.cuda())
    assert got.shape == tuple(rows_shape) + (cin,)
    x = torch.zeros(int(np.prod(rows_shape)), 1, 1, cin)
    _dot_bounded(f'_dgrad_1x1 rows={rows_shape} Cout={cout} Cin={cin}', got.reshape(-1, 1, 1, cin), x,
                 w2.view(cout, cin, 1, 1), dy.reshape(-1, 1, 1, cout), 0, 0, cout)


@pytest.mark.parametrize('n,H,W,cout,cin', [(5, 7, 7, 64, 32), (3, 5, 9, 32, 64), (2, 14, 14, 128, 128), (1, 1, 1, 32, 4)])
def test_conv3x3_dgrad_and_wgrad_helpers(n, H, W, cout, cin):
    """``_conv3x3_dgrad`` (forward kernel, weight flipped and channel roles swapped: reduction 9 Cout) and ``_conv3x3_wgrad``
    (im2col + the transposed-operand GEMM: reduction n H W) against float64 autograd of F.conv2d, on a non-square map too
    (a transposed or unflipped tap shows there)."""
    from fgn_amd import ops, train as TR
    g = _gen(70 + n + cout)
    x = torch.randn(n, H, W, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    dy = torch.randn(n, H, W, cout, generator=g)
    with ops.gemm_math('f32'):
        dx = TR._conv3x3_dgrad(dy.cuda(), w.cuda())
        dw = TR._conv3x3_wgrad(dy.cuda(), x.cuda())
    assert dx.shape == x.shape and dw.shape == w.shape and dw.is_contiguous()
    tag = f'n={n} {H}x{W} Cout={cout} Cin={cin}'
    _dot_bounded('_conv3x3_dgrad ' + tag, dx, x, w, dy, 1, 0, 9 * cout)
    _dot_bounded('_conv3x3_wgrad ' + tag, dw, x, w, dy, 1, 1, n * H * W)


@pytest.mark.parametrize('R,M,N', [(0, 8, 12), (37, 6, 256), (441, 6, 1024), (100, 75, 64), (300, 64, 260), (2000, 128, 36)])
def test_mm_tn_helper(R, M, N):
    """``_mm_tn`` = a^T b: no rows (zeros, nothing launched), M % 4 != 0 (the small-product kernel), else the MFMA kernel."""
    from fgn_amd import train as TR
    g = _gen(80 + R)
    a = torch.randn(R, M, generator=g)
    b = torch.randn(R, N, generator=g)
    got = TR._mm_tn(a.cuda(), b.cuda())
    assert got.shape == (M, N)
    want = a.to(F64).t() @ b.to(F64)
    mag = a.to(F64).abs().t() @ b.to(F64).abs()
    _bounded(f'_mm_tn R={R} M={M} N={N}', got, want, mag, max(R, 1))
    if R == 0:
        assert float(got.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ two stages on identical inputs
def _err(got, want):
    """(worst element / the tensor's largest element, L2 error / L2 norm)"""
    got, want = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (float((got - want).abs().max()) / (float(want.abs().max()) + 1e-300),
            float((got - want).norm()) / (float(want.norm()) + 1e-300))


def _stage_check(stage, got, ref64, ref32):
    """The margin over float64 autograd of a whole stage: the SAME graph run by float32 CPU autograd is measured against the
    float64 run (both error measures, per tensor); the HIP path - other reduction orders, the same fp32 arithmetic - is
    allowed 4 x the worst of those over the stage's tensors (one small tensor's own fp32 error is a noisy sample: a bias
    gradient of four elements can come out exact by chance)."""
    assert set(got) == set(ref64), (sorted(got), sorted(ref64))
    e32 = {k: _err(ref32[k], ref64[k]) for k in ref64}
    m0, m1 = 4 * max(v[0] for v in e32.values()), 4 * max(v[1] for v in e32.values())
    assert 0 < m0 < 1e-4 and 0 < m1 < 1e-4, (m0, m1)          # fp32 noise, not an error of the rebuilt graph
    rep = {k: _err(got[k], ref64[k]) for k in ref64}
    w0, w1 = max(v[0] for v in rep.values()), max(v[1] for v in rep.values())
    print(f'[bwd-bound] {stage}: fp32 CPU autograd vs fp64 worst (max, L2) = ({m0 / 4:.3e}, {m1 / 4:.3e}); HIP vs fp64 worst = '
          f'({w0:.3e}, {w1:.3e}); ratio to the 4x margin = ({w0 / m0:.3f}, {w1 / m1:.3f})')
    bad = {k: v for k, v in rep.items() if v[0] > m0 or v[1] > m1}
    assert not bad, (bad, m0, m1)


@functools.lru_cache(maxsize=None)
def _taped_step(with_gt: bool):
    """forward_train of the half-width tiny model under the Trainer's arithmetic, keeping the tape."""
    import copy
    from fgn_amd import ops, train as TR
    from fgn_amd.config import tiny_config
    from fgn_amd.episodes import make_batch
    from test_hip_train import _models
    cfg = tiny_config(3, 2, width_div=2)
    m, sd = _models(cfg)
    b = make_batch(4, 2, 3, 2, 160, 224, 64)
    if not with_gt:
        b = copy.deepcopy(b)
        for i in range(2):
            b['qry_bboxes'][i], b['qry_cat_ids'][i] = b['qry_bboxes'][i][:0], b['qry_cat_ids'][i][:0]
            b['qry_isegmaps'][i] = b['qry_isegmaps'][i][:0]
    tr = TR.Trainer(m)
    m._tape = {}
    try:
        torch.manual_seed(3)
        with ops.gemm_math('f32'):
            TR.forward_train(m, **b)
        tape = m._tape
    finally:
        m._tape = None
    return m, tr, tape, cfg


def _rpn_stage_reference(tr, tape, dtype):
    t = tape['rpn']
    N, A = t['n_ways'], t['A']
    c = lambda v: v.detach().cpu().to(dtype)
    names = ['rpn_head.rpn_conv', 'rpn_head.rpn_cls', 'rpn_head.rpn_reg']
    W = {k + s: c(tr.W[k + s]).requires_grad_(True) for k in names for s in ('.weight', '.bias')}
    qf, vec = c(t['qry_fmap']), c(t['vec'])                                    # [B,h,w,C], [B*N,C]
    G = vec.shape[0]
    xin = (qf.repeat_interleave(N, dim=0) * vec[:, None, None, :]).permute(0, 3, 1, 2)
    pre = F.conv2d(xin, W['rpn_head.rpn_conv.weight'], W['rpn_head.rpn_conv.bias'], padding=1)
    x = pre * (t['x'].detach().cpu().permute(0, 3, 1, 2) > 0)                  # the ReLU mask of the HIP forward pass
    assert _err(x, t['x'].permute(0, 3, 1, 2))[0] <= 1e-4
    wh = torch.cat([W['rpn_head.rpn_cls.weight'], W['rpn_head.rpn_reg.weight']], 0)
    bh = torch.cat([W['rpn_head.rpn_cls.bias'], W['rpn_head.rpn_reg.bias']], 0)
    head = F.conv2d(x, wh, bh).permute(0, 2, 3, 1).reshape(G, -1, 5 * A)       # [G, h*w, 5A]
    n_total = t['n_total']
    logits = head[:, :, :A].reshape(-1)
    deltas = head[:, :, A:].reshape(-1, 4)
    flat = np.concatenate([g * n_total + idx for g, (pos, neg) in enumerate(t['sets']) for idx in (pos, neg)])
    xc = logits[torch.from_numpy(flat).long()]
    assert _err(xc, t['x_cat'])[0] <= 1e-4
    loss = F.binary_cross_entropy_with_logits(xc, c(t['y_cat']), weight=None if t['w_cat'] is None else c(t['w_cat']),
                                              reduction='sum')
    if t['preds'] is not None:
        pf = np.concatenate([g * n_total + pos for g, (pos, neg) in enumerate(t['sets']) if pos.size])
        pr = deltas[torch.from_numpy(pf).long()]
        assert _err(pr, t['preds'])[0] <= 1e-4
        loss = loss + F.smooth_l1_loss(pr, c(t['tgts']), reduction='sum', beta=1.0)
    (loss / (float(t['n_samples']) * N)).backward()
    return {k: v.grad for k, v in W.items()}


@pytest.mark.parametrize('with_gt', [True, False])
def test_rpn_stage_backward_alone_matches_autograd(with_gt):
    """``_backward_rpn_stage`` from the tape of a HIP forward pass: the guided 3x3 convolution (ReLU mask of the tape), the
    objectness / delta head, the sampled sigmoid and smooth-L1 losses rebuilt in float64 on the CPU.  Without ground truth
    no anchor is positive (``preds is None``): the delta head gets exact zeros."""
    from fgn_amd import ops, train as TR
    m, tr, tape, cfg = _taped_step(with_gt)
    assert (tape['rpn']['preds'] is not None) == with_gt
    grads = {}
    with ops.gemm_math('f32'):
        TR._backward_rpn_stage(m, tr.W, tape, grads)
    r64, r32 = _rpn_stage_reference(tr, tape, F64), _rpn_stage_reference(tr, tape, torch.float32)
    if not with_gt:
        for k in ('rpn_head.rpn_reg.weight', 'rpn_head.rpn_reg.bias'):
            assert float(grads[k].abs().max()) == 0.0 and float(r64[k].abs().max()) == 0.0
            grads.pop(k), r64.pop(k), r32.pop(k)
    _stage_check(f'AG-RPN stage with_gt={with_gt}', grads, r64, r32)


def _mask_stage_reference(tr, tape, cfg, dtype):
    tm, tr_ = tape['mask'], tape['roi']
    c = lambda v: v.detach().cpu().to(dtype)
    nchw = lambda v: v.permute(0, 3, 1, 2)
    W = {k: c(v).requires_grad_(True) for k, v in tr.W.items() if k.startswith('roi_head.mask_head.')}
    mfeat, vmask = c(tm['mfeat']).requires_grad_(True), c(tm['vmask']).requires_grad_(True)
    x = nchw(mfeat * vmask[:, None, None, :])
    for li, act in enumerate(tm['acts']):
        p = f'roi_head.mask_head.convs.{li}.conv'
        x = F.conv2d(x, W[p + '.weight'], W[p + '.bias'], padding=1) * (nchw(act.detach().cpu()) > 0)
        assert _err(x, nchw(act))[0] <= 1e-4
    up = F.conv_transpose2d(x, W['roi_head.mask_head.upsample.weight'], W['roi_head.mask_head.upsample.bias'], stride=2)
    D, P = up.shape[0], up.shape[2] // 2
    cu = up.shape[1]
    shuf = lambda v: v.view(D, P, P, 2, 2, cu).permute(0, 5, 1, 3, 2, 4).reshape(D, cu, 2 * P, 2 * P)
    up = up * (shuf(tm['up'].detach().cpu()) > 0)
    assert _err(up, shuf(tm['up']))[0] <= 1e-4
    logit = F.conv2d(up, W['roi_head.mask_head.conv_logits.weight'], W['roi_head.mask_head.conv_logits.bias'])[:, 0]
    assert _err(logit, tm['mlog'])[0] <= 1e-4
    F.binary_cross_entropy_with_logits(logit, (c(tm['tgt']) >= 0.5).to(dtype), reduction='mean').backward()
    out = {k: v.grad for k, v in W.items()}
    d_feats = torch.zeros(tuple(tr_['feats'].shape), dtype=dtype)
    d_feats.index_add_(0, tr_['pos_rows'].cpu(), mfeat.grad)
    out['d_feats'] = d_feats
    N = cfg['n_ways']
    dmp = torch.zeros((tape['spp']['B'] * N, vmask.shape[1]), dtype=dtype)
    dmp.index_add_(0, torch.from_numpy(np.asarray(tm['rows_h'])).long(), vmask.grad)
    out['d_cat_mean_mp'] = dmp
    return out


def test_mask_head_backward_alone_matches_autograd():
    """``_backward_mask_head`` from the tape of a HIP forward pass: guided input, four 3x3 convolutions, the 2x2 deconvolution,
    the logit convolution and the thresholded sigmoid loss rebuilt in float64 with the tape's ReLU masks.  Every
    ``roi_head.mask_head.*`` gradient, the gradient that reaches ``feats`` and the one of the masked-pooled class vectors."""
    from fgn_amd import ops, train as TR
    m, tr, tape, cfg = _taped_step(True)
    assert tape['mask'] is not None and tape['mask']['mfeat'].shape[0] >= 2
    grads = {}
    with ops.gemm_math('f32'):
        d_feats, d_mp = TR._backward_mask_head(m, tr.W, tape, grads)
    assert set(grads) == {k for k in tr.W if k.startswith('roi_head.mask_head.')}
    grads['d_feats'], grads['d_cat_mean_mp'] = d_feats, d_mp
    _stage_check('mask head stage', grads, _mask_stage_reference(tr, tape, cfg, F64),
                 _mask_stage_reference(tr, tape, cfg, torch.float32))
