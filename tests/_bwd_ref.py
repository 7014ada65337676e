"""Closed-form float64 restatements of the backward kernels of fgn_amd/csrc/train_bwd.hip (CPU, torch.float64).

Every function takes the operands of its ``ops.*`` wrapper in the same NHWC layouts (fp32 tensors, on any device; they
are moved to the CPU and widened) and returns float64 tensors.  Scalars the C ABI carries as ``float`` (scale, beta,
y_threshold, eps) are rounded to fp32 first: the reference works on the operands the kernel sees.

Beside every result that is a sum of signed terms the functions return that element's TERM-MAGNITUDE SUM (the same
expression with every term replaced by its absolute value, ``mag``): the per-element error bounds of
tests/test_hip_train_bwd.py are ``c * 2^-24 * mag`` with ``c`` a counted number of fp32 roundings.
tests/test_bwd_ref_cpu.py pins every closed form to torch.autograd in float64.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24            # unit roundoff of fp32
TINY = 2.0 ** -126        # smallest normal fp32: results below it may lose bits (or be flushed)


def d(t):
    return None if t is None else t.detach().to('cpu', F64)


def f32(v: float) -> float:
    return float(np.float32(v))


def ulp32(t: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 at |t| (float64 tensor in, float64 out)."""
    a = t.abs().to(torch.float32).numpy()
    return torch.from_numpy(np.spacing(a).astype(np.float64))


# ------------------------------------------------------------------------------------------ loss gradients
def bce_grad(x, y, w, scale: float, y_threshold: float = -1.0):
    """d/dx sum_i w_i BCEWithLogits(x_i, y_i) * scale -> (dx, mag); mag = (sigmoid + y) * |w * scale|."""
    x, y, w = d(x), d(y), d(w)
    thr = f32(y_threshold)
    if thr >= 0:
        y = (y >= thr).to(F64)
    s = torch.sigmoid(x)
    k = f32(scale) * (w if w is not None else torch.ones_like(x))
    return (s - y) * k, (s.abs() + y.abs()) * k.abs()


def smooth_l1_grad(pred, target, w, scale: float, beta: float = 1.0):
    """-> (dpred, mag); the gradient is continuous at |d| = beta, mag = |clamp(d / beta, -1, 1)| * |w * scale|."""
    p, t, w = d(pred), d(target), d(w)
    b = f32(beta)
    dd = p - t
    g = torch.where(dd.abs() < b, dd / b, torch.sign(dd))
    k = f32(scale) * (w if w is not None else torch.ones_like(p))
    return g * k, g.abs() * k.abs()


def softmax_ce_grad(logits, labels, w, scale: float):
    """-> (dlogits, mag, p).  Rows whose label is outside [0, C) are zero.  The kernel forms r - max in fp32 before the
    exponential, so a probability carries the relative error |r_c - max| * 2^-24 of its own exponent and of the
    normaliser: mag = (p_c * (1 + |delta_c| + sum_c' |delta_c'| p_c') + [c == label]) * |w * scale|."""
    z, w = d(logits), d(w)
    lab = labels.detach().cpu().long()
    n, C = z.shape
    ok = (lab >= 0) & (lab < C)
    delta = z - z.max(dim=1, keepdim=True).values
    e = torch.exp(delta)
    p = e / e.sum(dim=1, keepdim=True)
    one = torch.zeros_like(z)
    one[ok, lab[ok]] = 1.0
    k = (f32(scale) * (w if w is not None else torch.ones(n, dtype=F64)))[:, None]
    g = (p - one) * k
    mag = (p * (1.0 + delta.abs() + (delta.abs() * p).sum(dim=1, keepdim=True)) + one) * k.abs()
    okc = ok[:, None].to(F64)
    return g * okc, mag * okc, p


def relu_backward(dy, y):
    """dy * [y > 0], exact (a masked-out element is +0.0)."""
    dy, y = d(dy), d(y)
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def colsum(x, exact_cols=()):
    """x [..., C] -> (sum over the leading dims [C], sum of |x| [C]).  ``exact_cols``: columns summed without any
    rounding (math.fsum), for data whose float64 sum depends on the order."""
    x = d(x)
    x = x.reshape(-1, x.shape[-1]) if x.shape[-1] else x.reshape(0, 0)
    s = x.sum(dim=0)
    for c in exact_cols:
        s[c] = math.fsum(x[:, c].tolist())
    return s, x.abs().sum(dim=0)


def im2col3x3(x):
    """x [n,H,W,C] -> [n*H*W, 9*C], column = (ky*3 + kx)*C + ci (3x3, stride 1, pad 1), exact."""
    x = d(x)
    n, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, dim=3).reshape(n * H * W, 9 * C)


# ------------------------------------------------------------------------------------------ BatchNorm (train) backward
def bn_train_backward(x_pre, y_post, dy, mean, var, gamma, eps: float):
    """Rows [P, C] (any leading dims).  -> dict(dx, dgamma, dbeta, g, xhat, mag_dx, mag_dgamma, mag_dbeta):
      g = dy * [y_post > 0];  xhat = (x - mean) / sqrt(var + eps);  dbeta = sum g;  dgamma = sum g xhat
      dx = gamma rstd (g - dbeta / P - xhat dgamma / P)
      mag_dbeta = sum |g|;  mag_dgamma = sum |g xhat|;  mag_dx = |gamma rstd| (|g| + sum|g| / P + |xhat| sum|g xhat| / P)"""
    x, dy_, mean, var, gamma = d(x_pre), d(dy), d(mean), d(var), d(gamma)
    C = x.shape[-1]
    x, dy_ = x.reshape(-1, C), dy_.reshape(-1, C)
    P = x.shape[0]
    g = dy_ if y_post is None else torch.where(d(y_post).reshape(-1, C) > 0, dy_, torch.zeros_like(dy_))
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xh = (x - mean) * rstd
    db, dg = g.sum(0), (g * xh).sum(0)
    mdb, mdg = g.abs().sum(0), (g * xh).abs().sum(0)
    dx = gamma * rstd * (g - db / P - xh * dg / P)
    mdx = (gamma * rstd).abs() * (g.abs() + mdb / P + xh.abs() * mdg / P)
    return dict(dx=dx, dgamma=dg, dbeta=db, g=g, xhat=xh, mag_dx=mdx, mag_dgamma=mdg, mag_dbeta=mdb)


# ------------------------------------------------------------------------------------------ relation / box head backward
def relation_gn_head_backward(q, s, rois, gn_w, gn_b, fc_w, d_out6, n_ways: int, gn_groups: int, eps: float):
    """q [R,7,7,C], s [B*N,7,7,C], rois [R,5] (column 0: image), d_out6 [R*N,6], fc_w [6,C].  Per (RoI r, class n):
      x = q[r] + s[img, n];  xhat = GroupNorm statistics over (49, C/groups);  pre = gamma xhat + beta
      pooled = mean_p relu(pre);  dp = d_out6[r,n] . fc_w / 49;  gg = [pre > 0] dp gamma
      dZ = rstd (gg - mean_grp gg - xhat mean_grp(gg xhat));  dQ = sum_n dZ;  dgamma = sum [pre > 0] dp xhat;  dbeta = sum [..] dp
    -> dict with those, ``pre`` and ``pre_mag`` = |gamma xhat| + |beta| (the ReLU margin rule), and the magnitude sums
      xmag = rstd (|x| + mean_grp |x|)            (xhat is a difference; its fp32 error scales with this, not with |xhat|)
      G = [pre > 0] |gamma| sum_j |d6_j fcw_j| / 49
      mag_dZ = rstd (G + mean_grp G + xmag mean_grp(G xmag));  mag_dQ = sum_n mag_dZ
      mag_pooled = mean_p (|gamma| xmag + |beta|);  mag_dgamma = sum G xmag / |gamma|;  mag_dbeta = sum G / |gamma|"""
    q, s, gw_, gb_, fcw, d6 = d(q), d(s), d(gn_w), d(gn_b), d(fc_w), d(d_out6)
    R, ps, _, C = q.shape
    N, P, gwid = n_ways, ps * ps, C // gn_groups
    img = rois.detach().cpu()[:, 0].long()
    x = (q[:, None] + s.view(-1, N, ps, ps, C)[img]).reshape(R, N, P, gn_groups, gwid)
    grp = lambda t: t.mean(dim=(2, 4), keepdim=True)
    mean = grp(x)
    var = grp((x - mean) ** 2)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xh = (x - mean) * rstd
    xmag = rstd * (x.abs() + grp(x.abs()))
    ga, be = gw_.view(1, 1, 1, gn_groups, gwid), gb_.view(1, 1, 1, gn_groups, gwid)
    pre = ga * xh + be
    pre_mag = (ga * xh).abs() + be.abs()
    on = (pre > 0).to(F64)
    pooled = (pre * on).mean(dim=2)                                          # [R,N,groups,gw]
    d6 = d6.view(R, N, 6)
    dp = (torch.einsum('rnj,jc->rnc', d6, fcw) / P).view(R, N, 1, gn_groups, gwid)
    dpmag = (torch.einsum('rnj,jc->rnc', d6.abs(), fcw.abs()) / P).view(R, N, 1, gn_groups, gwid)
    g = on * dp
    gg = g * ga
    G = on * dpmag * ga.abs()
    dZ = rstd * (gg - grp(gg) - xh * grp(gg * xh))
    mag_dZ = rstd * (G + grp(G) + xmag * grp(G * xmag))
    flat = lambda t: t.reshape(R, N, ps, ps, C)
    return dict(dZ=flat(dZ).reshape(R * N, ps, ps, C), dQ=flat(dZ).sum(1), pooled=pooled.reshape(R * N, C),
                dgamma=(g * xh).sum(dim=(0, 1, 2)).reshape(C), dbeta=g.sum(dim=(0, 1, 2)).reshape(C),
                pre=flat(pre), pre_mag=flat(pre_mag),
                mag_dZ=flat(mag_dZ).reshape(R * N, ps, ps, C), mag_dQ=flat(mag_dZ).sum(1),
                mag_pooled=(ga.abs() * xmag + be.abs()).mean(dim=2).reshape(R * N, C),
                mag_dgamma=(on * dpmag * xmag).sum(dim=(0, 1, 2)).reshape(C),
                mag_dbeta=(on * dpmag).sum(dim=(0, 1, 2)).reshape(C))


# ------------------------------------------------------------------------------------------ mask logits backward
def mask_logits_backward(up, dlogit, w, roi_size: int):
    """up [D,P,P,4*C] (sub-position major: channel index = sub*C + c, sub = 2*dy + dx), dlogit [D,2P,2P], w [C]
    -> (d_up, dw [C], mag_dw [C]);  d_up = dlogit[d, 2i+dy, 2j+dx] * w[c] * [up > 0] as the ONE fp32 product the
    kernel forms (bit-comparable), dw = sum dlogit * up, mag_dw = sum |dlogit * up|.  ``up`` is the deconv's output
    AFTER its ReLU (the forward kernel applies none), so on the operands of a training step dw is the gradient of
    conv_logits(relu(deconv)); an element <= 0 passes no gradient down and enters dw with its own value."""
    D, P = up.shape[0], roi_size
    C = w.numel()
    upc = up.detach().cpu().float().reshape(D, P, P, 2, 2, C)
    dl32 = dlogit.detach().cpu().float().reshape(D, P, 2, P, 2).permute(0, 1, 3, 2, 4)[..., None]   # [D,i,j,dy,dx,1]
    prod32 = dl32 * w.detach().cpu().float().view(1, 1, 1, 1, 1, C)                                   # one fp32 rounding
    d_up = torch.where(upc > 0, prod32, torch.zeros_like(prod32)).reshape(D, P, P, 4 * C)
    t = dl32.to(F64) * upc.to(F64)
    return d_up, t.sum(dim=(0, 1, 2, 3, 4)), t.abs().sum(dim=(0, 1, 2, 3, 4))
