"""The float64 closed forms of tests/_bwd_ref.py against torch.autograd in float64, to 1e-12 of each tensor's largest
element: pins the reference of tests/test_hip_train_bwd.py on a machine without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _bwd_ref as ref

F64 = torch.float64


def _close(got, want, what=''):
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.numel():
        err = float((got - want).abs().max())
        assert err <= 1e-12 * max(float(want.abs().max()), 1e-300), (what, err, float(want.abs().max()))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('thr', [-1.0, 0.5])
@pytest.mark.parametrize('weighted', [False, True])
def test_bce_grad_is_the_autograd_of_bce_with_logits(thr, weighted):
    g = _gen(1)
    x = torch.cat([torch.tensor([0., 1e-3, -1e-3, 1., -1., 20., -20., 90., -90., 104., -104.]), torch.randn(300, generator=g) * 4])
    y = torch.rand(x.numel(), generator=g)
    y[::7] = 0.5
    w = torch.rand(x.numel(), generator=g) if weighted else None
    scale = 1.0 / 37
    got, mag = ref.bce_grad(x, y, w, scale, thr)
    xx = x.to(F64).requires_grad_(True)
    yy = (y >= thr).to(F64) if thr >= 0 else y.to(F64)
    loss = F.binary_cross_entropy_with_logits(xx, yy, weight=None if w is None else w.to(F64), reduction='sum') * ref.f32(scale)
    loss.backward()
    _close(got, xx.grad, 'bce')
    assert bool((mag >= got.abs() * (1 - 1e-15)).all())


@pytest.mark.parametrize('beta', [1.0, 1.0 / 9])
def test_smooth_l1_grad_is_the_autograd_of_smooth_l1(beta):
    g = _gen(2)
    b = ref.f32(beta)
    p = torch.cat([torch.tensor([0., b / 2, -b / 2, 3 * b, -3 * b]), torch.randn(400, generator=g)]).float()
    t = torch.cat([torch.zeros(5), torch.randn(400, generator=g)]).float()
    w = torch.rand(p.numel(), generator=g)
    got, mag = ref.smooth_l1_grad(p, t, w, 0.25, beta)
    pp = p.to(F64).requires_grad_(True)
    (F.smooth_l1_loss(pp, t.to(F64), reduction='none', beta=b) * w.to(F64)).sum().mul(0.25).backward()
    _close(got, pp.grad, 'smooth l1')
    assert float(got[0]) == 0.0 and bool((mag >= got.abs() * (1 - 1e-15)).all())


@pytest.mark.parametrize('C', [1, 2, 4, 9])
def test_softmax_ce_grad_is_the_autograd_of_cross_entropy(C):
    g = _gen(3)
    n = 257
    z = (torch.randn(n, C, generator=g) * 8).float()
    z[::5] = (torch.rand(z[::5].shape, generator=g) * 120 - 60).float()
    lab = torch.randint(0, C, (n,), generator=g)
    lab[3], lab[4] = -1, C
    w = torch.rand(n, generator=g)
    got, mag, p = ref.softmax_ce_grad(z, lab, w, 1.0 / 11)
    zz = z.to(F64).requires_grad_(True)
    ok = (lab >= 0) & (lab < C)
    ce = F.cross_entropy(zz[ok], lab[ok], reduction='none')
    (ce * w.to(F64)[ok]).sum().mul(ref.f32(1.0 / 11)).backward()
    _close(got, zz.grad, 'softmax ce')
    assert float(got[3].abs().max()) == 0.0 and float(got[4].abs().max()) == 0.0
    assert bool((mag >= got.abs() * (1 - 1e-15)).all())


def test_relu_backward_colsum_and_im2col_closed_forms():
    g = _gen(4)
    y = torch.randn(64, 12, generator=g)
    y[0, :4] = torch.tensor([0.0, -0.0, 1e-42, -1e-42])
    dy = torch.randn(64, 12, generator=g)
    yy = y.to(F64).requires_grad_(True)
    # relu is applied to the PRE-activation; its output y has the same sign pattern (y > 0 <=> pre > 0)
    (torch.relu(yy) * dy.to(F64)).sum().backward()
    _close(ref.relu_backward(dy, torch.relu(y)), yy.grad, 'relu')
    assert ref.relu_backward(dy, y)[0, :4].tolist() == [0.0, 0.0, float(dy[0, 2]), 0.0]
    x = torch.randn(5, 7, 6, generator=g)
    s, a = ref.colsum(x, exact_cols=(2,))
    _close(s, x.to(F64).reshape(-1, 6).sum(0), 'colsum')
    _close(a, x.to(F64).abs().reshape(-1, 6).sum(0), 'colsum abs')
    cancel = torch.tensor([[1e4], [1e-3], [-1e4]] * 1)
    assert float(ref.colsum(cancel, exact_cols=(0,))[0][0]) == float(torch.tensor(1e-3).to(F64))
    for (n, H, W, C) in [(1, 1, 1, 4), (3, 5, 9, 12), (1, 1, 6, 8)]:
        x = torch.randn(n, H, W, C, generator=g)
        cols = F.unfold(x.permute(0, 3, 1, 2).to(F64), 3, padding=1)                 # [n, C*9, H*W], row = ci*9 + tap
        want = cols.view(n, C, 9, H * W).permute(0, 3, 2, 1).reshape(n * H * W, 9 * C)
        assert torch.equal(ref.im2col3x3(x), want)


@pytest.mark.parametrize('P,C,post', [(3, 64, True), (63, 4, False), (65, 260, True), (441, 16, True)])
def test_bn_train_backward_is_the_autograd_of_batch_norm_then_relu(P, C, post):
    g = _gen(5)
    x = torch.randn(P, C, generator=g)
    x[:, 1] = x[:, 1] * 1e-4
    x[:, 2] = x[:, 2] + 1e3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(P, C, generator=g)
    eps = 1e-5
    e32 = ref.f32(eps)
    xx = x.to(F64).requires_grad_(True)
    ga = gamma.to(F64).requires_grad_(True)
    be = beta.to(F64).requires_grad_(True)
    pre = F.batch_norm(xx.t()[None], None, None, ga, be, True, 0.1, e32)[0].t()
    out = torch.relu(pre) if post else pre
    (out * dy.to(F64)).sum().backward()
    mean = x.to(F64).mean(0)
    var = x.to(F64).var(0, unbiased=False)
    # the reference takes mean / var as float64 here (the kernel's fp32 operands are a rounding of these)
    r = ref.bn_train_backward(x, out.detach() if post else None, dy, mean, var, gamma, eps)
    _close(r['dx'], xx.grad, 'dx')
    _close(r['dgamma'], ga.grad, 'dgamma')
    _close(r['dbeta'], be.grad, 'dbeta')
    _close(r['g'], dy.to(F64) * ((pre.detach() > 0) if post else 1), 'g')
    assert bool((r['mag_dx'] >= r['dx'].abs() * (1 - 1e-12)).all())
    assert bool((r['mag_dgamma'] >= r['dgamma'].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('R,N,C,groups', [(9, 3, 256, 8), (5, 8, 64, 2), (7, 1, 128, 16), (6, 2, 64, 8), (4, 4, 32, 1)])
def test_relation_head_backward_is_the_autograd_of_group_norm_relu_mean_linear(R, N, C, groups):
    g = _gen(6)
    B = 3
    q = torch.randn(R, 7, 7, C, generator=g)
    s = torch.randn(B * N, 7, 7, C, generator=g)
    gw = torch.rand(C, generator=g) + 0.5
    gb = torch.randn(C, generator=g) * 0.1
    fcw = torch.randn(6, C, generator=g) * 0.1
    d6 = torch.randn(R * N, 6, generator=g)
    img = torch.tensor([(2 * i + 2) % B if (2 * i + 2) % B != 1 else 0 for i in range(R)])        # unsorted, image 1 unused
    rois = torch.cat([img.float()[:, None], torch.zeros(R, 4)], 1)
    leaf = lambda t: t.to(F64).requires_grad_(True)
    Q, S, GW, GB, FW = leaf(q.permute(0, 3, 1, 2)), leaf(s.permute(0, 3, 1, 2)), leaf(gw), leaf(gb), leaf(fcw)
    z = (Q[:, None] + S.view(B, N, C, 7, 7)[img]).reshape(R * N, C, 7, 7)
    z.retain_grad()
    pre = F.group_norm(z, groups, GW, GB, ref.f32(1e-5))
    pooled = torch.relu(pre).mean(dim=(2, 3))
    ((pooled @ FW.t()) * d6.to(F64)).sum().backward()
    r = ref.relation_gn_head_backward(q, s, rois, gw, gb, fcw, d6, N, groups, 1e-5)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    _close(r['dZ'], nhwc(z.grad), 'dZ')
    _close(r['dQ'], nhwc(Q.grad), 'dQ')
    _close(r['pooled'], pooled.detach(), 'pooled')
    _close(r['dgamma'], GW.grad, 'dgamma')
    _close(r['dbeta'], GB.grad, 'dbeta')
    _close(r['pre'].reshape(R * N, 7, 7, C), nhwc(pre.detach()), 'pre')
    dS = torch.zeros(B * N, 7, 7, C, dtype=F64)
    dZ = r['dZ'].view(R, N, 7, 7, C)
    for i in range(R):
        dS[int(img[i]) * N:(int(img[i]) + 1) * N] += dZ[i]
    _close(dS, nhwc(S.grad), 'dS')
    assert float(dS[N:2 * N].abs().max()) == 0.0
    for k in ('dZ', 'dQ', 'pooled', 'dgamma', 'dbeta'):
        assert bool((r['mag_' + k] >= r[k].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize('D,P,C', [(0, 7, 8), (1, 7, 4), (3, 14, 12)])
def test_mask_logits_backward_is_the_autograd_of_relu_then_conv1x1(D, P, C):
    g = _gen(7)
    pre = torch.randn(D, P, P, 4 * C, generator=g)
    up = torch.relu(pre)                   # the operand is the deconv's output AFTER its ReLU: zeros and positives
    dl = torch.randn(D, 2 * P, 2 * P, generator=g)
    w = torch.randn(C, generator=g)
    d_up, dw, mag = ref.mask_logits_backward(up, dl, w, P)
    # pixel shuffle of the sub-position-major deconv output: [D, i, j, dy, dx, C] -> NCHW [D, C, 2P, 2P]
    U = pre.to(F64).requires_grad_(True)
    W = w.to(F64).requires_grad_(True)
    full = U.view(D, P, P, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(D, C, 2 * P, 2 * P)
    logit = F.conv2d(torch.relu(full), W.view(1, C, 1, 1))[:, 0]
    (logit * dl.to(F64)).sum().backward()
    assert d_up.dtype == torch.float32
    if D:
        # d_up is ONE fp32 product: within half an ulp of the float64 gradient, and exactly 0 where up <= 0
        want = U.grad
        assert bool(((d_up.to(F64) - want).abs() <= 2.0 ** -24 * want.abs() + 1e-300).all())
        assert bool((d_up[up <= 0] == 0).all())
        _close(dw, W.grad, 'dw')
        assert bool((mag >= dw.abs() * (1 - 1e-12)).all())
    else:
        assert d_up.numel() == 0 and float(dw.abs().max()) == 0.0
