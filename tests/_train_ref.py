"""Closed-form float64 restatements of the forward kernels of the training path (csrc/train.hip: the weighted loss sums,
bbox2delta, BatchNorm in training mode) and of the Adagrad update (csrc/train_bwd.hip); CPU, float64.

As in tests/_bwd_ref.py and tests/_fwd_ref.py every function takes the operands of its ``ops.*`` wrapper (fp32 tensors on
any device), widens them to float64 and returns the value and, per output element, its TERM-MAGNITUDE SUM ``mag`` (the
reference expression with every term replaced by its absolute value, plus a conditioning term where the kernel subtracts
rounded quantities).  tests/test_hip_train_fwd_bound.py bounds every output by ``c * 2^-24 * mag + 2^-126``;
tests/test_train_ref_cpu.py pins every closed form to an independent implementation and shows, with a numpy emulation
of each kernel's arithmetic, that the bound holds on every input the GPU tests use.  Scalars the C ABI carries as
``float`` (y_threshold, beta, eps, momentum, lr, weight decay, the coder's means and stds) are rounded to fp32 first;
``avg_factor`` travels as a double.

The second half of the file builds the inputs of the GPU tests (seeded, on the CPU), so that both test files see the
same tensors.
"""
import numpy as np
import torch

from _bwd_ref import F64, TINY, U, d, f32  # noqa: F401  (re-exported to the tests)

F32 = np.float32

# Rounding counts of the bounds; the docstrings of tests/test_hip_train_fwd_bound.py derive each from the kernel's code.
C_BCE, C_SL1, C_CE = 3, 7, 5
C_BBOX_XY, C_BBOX_WH = 8, 7
C_BN_MEAN, C_BN_RM, C_BN_RV, C_BN_Y = 2, 6, 5, 10      # running_var: C_BN_RV + c_var; y: + 0.5 c_var on its rstd part
C_ADA_STATE, C_ADA_P = 5, 11


# ------------------------------------------------------------------------------------------ loss sums
def _weights(w, like):
    return torch.ones_like(like) if w is None else d(w).reshape(like.shape)


def bce_sum(x, y, w, avg: float, y_thr: float = -1.0):
    """sum_i w_i l_i / avg, l_i = max(x, 0) - x y + log1p(exp(-|x|)) (y binarised at y_thr when y_thr >= 0) -> (val, mag);
    mag = sum_i |w_i| (max(x, 0) + |x y| + log1p(exp(-|x|))) / |avg|."""
    x, y = d(x).reshape(-1), d(y).reshape(-1)
    w = _weights(w, x)
    thr = f32(y_thr)
    if thr >= 0:
        y = (y >= thr).to(F64)
    t1, t2, t3 = x.clamp_min(0.0), x * y, torch.log1p(torch.exp(-x.abs()))
    val = (w * (t1 - t2 + t3)).sum() / avg
    mag = (w.abs() * (t1 + t2.abs() + t3)).sum() / abs(avg)
    return val, mag


def smooth_l1_sum(pred, target, w, avg: float, beta: float = 1.0):
    """sum_i w_i l_i / avg, l = |d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta, d = p - t -> (val, mag);
    mag_i = l_i + min(|d| / beta, 1) (|p| + |t|) (+ 0.5 beta on the linear branch): the difference p - t carries
    |p| + |t|, scaled by the slope of the branch."""
    p, t = d(pred).reshape(-1), d(target).reshape(-1)
    w = _weights(w, p)
    b = f32(beta)
    dd = (p - t).abs()
    quad = dd < b
    l = torch.where(quad, 0.5 * dd * dd / b, dd - 0.5 * b)
    mag_i = l + (dd / b).clamp_max(1.0) * (p.abs() + t.abs()) + torch.where(quad, torch.zeros_like(dd), torch.full_like(dd, 0.5 * b))
    return (w * l).sum() / avg, (w.abs() * mag_i).sum() / abs(avg)


def _ce_rows(logits, labels):
    z = d(logits)
    lab = labels.detach().cpu().long().reshape(-1)
    n, C = z.shape
    ok = (lab >= 0) & (lab < C)
    m = z.max(dim=1).values if n else z.new_zeros(0)
    delta = z - m[:, None]
    e = torch.exp(delta)
    s = e.sum(dim=1)
    picked = z.gather(1, lab.clamp(0, C - 1)[:, None])[:, 0] if n else z.new_zeros(0)
    l = m + torch.log(s) - picked
    mag = m.abs() + torch.log(s).abs() + picked.abs()
    cond = (e * delta.abs()).sum(dim=1) / s
    okf = ok.to(F64)
    return l * okf, mag * okf, cond * okf


def softmax_ce_sum(logits, labels, w, avg: float):
    """sum_i w_i (logsumexp(row_i) - row_i[label_i]) / avg over the rows whose label is in [0, C) -> (val, mag);
    mag_i = |max| + |log s| + |row[label]|, s = sum_c exp(row_c - max)."""
    l, mag_i, _ = _ce_rows(logits, labels)
    w = _weights(w, l)
    return (w * l).sum() / avg, (w.abs() * mag_i).sum() / abs(avg)


def softmax_ce_conditioning(logits, labels) -> float:
    """The kernel forms row_c - max in fp32 before the exponential; that rounding moves log s by at most
    2^-24 cond_i, cond_i = sum_c p_c |row_c - max| (<= log C).  -> max_i cond_i / mag_i over the counted rows (0 where
    cond_i is 0): the tests' logits keep it <= 1, so that the rounding counts once on mag_i."""
    _, mag_i, cond = _ce_rows(logits, labels)
    nz = cond > 0
    return float((cond[nz] / mag_i[nz]).max()) if bool(nz.any()) else 0.0


# ------------------------------------------------------------------------------------------ bbox2delta
def bbox2delta(p, g, means, stds):
    """DeltaXYWHBBoxCoder.encode in float64 -> (val, mag) [n,4].
      dx = ((gx - px) / pw - mean) / std, gx = (g0 + g2) / 2:  mag = (((|g0| + |g2|) / 2 + (|p0| + |p2|) / 2) / |pw| + |mean|) / |std|
      dw = (log(gw / pw) - mean) / std:  mag = (|log(gw / pw)| + 1 + |mean|) / |std|; the 1 is the conditioning of the
      logarithm (a relative error of its argument is an absolute error of its value).
    A zero-width proposal gives non-finite values (left to ``bbox2delta_f32``)."""
    p, g = d(p), d(g)
    mu = torch.tensor([f32(v) for v in means], dtype=F64)
    sd = torch.tensor([f32(v) for v in stds], dtype=F64)
    val, mag = torch.zeros(p.shape[0], 4, dtype=F64), torch.zeros(p.shape[0], 4, dtype=F64)
    for a in (0, 1):
        pw, gw = p[:, a + 2] - p[:, a], g[:, a + 2] - g[:, a]
        px, gx = (p[:, a] + p[:, a + 2]) * 0.5, (g[:, a] + g[:, a + 2]) * 0.5
        ctr_mag = (g[:, a].abs() + g[:, a + 2].abs()) * 0.5 + (p[:, a].abs() + p[:, a + 2].abs()) * 0.5
        val[:, a] = ((gx - px) / pw - mu[a]) / sd[a]
        mag[:, a] = (ctr_mag / pw.abs() + mu[a].abs()) / sd[a].abs()
        lg = torch.log(gw / pw)
        val[:, a + 2] = (lg - mu[a + 2]) / sd[a + 2]
        mag[:, a + 2] = (lg.abs() + 1.0 + mu[a + 2].abs()) / sd[a + 2].abs()
    return val, mag


def bbox2delta_f32(p, g, means, stds) -> np.ndarray:
    """bbox2delta_kernel's own operation sequence in numpy.float32 (csrc/train.hip is built without mul+add contraction),
    the logarithm taken in float64 and rounded once: the bit-level reference -> float32 [n,4]."""
    p = p.detach().cpu().numpy().astype(F32)
    g = g.detach().cpu().numpy().astype(F32)
    mu, sd = [F32(v) for v in means], [F32(v) for v in stds]
    out = np.zeros((p.shape[0], 4), dtype=F32)
    half = F32(0.5)
    with np.errstate(all='ignore'):
        for a in (0, 1):
            px, gx = (p[:, a] + p[:, a + 2]) * half, (g[:, a] + g[:, a + 2]) * half
            pw, gw = p[:, a + 2] - p[:, a], g[:, a + 2] - g[:, a]
            dx = (gx - px) / pw
            dw = np.log((gw / pw).astype(np.float64)).astype(F32)
            out[:, a] = (dx - mu[a]) / sd[a]
            out[:, a + 2] = (dw - mu[a + 2]) / sd[a + 2]
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------------------------------ BatchNorm, training mode
BN_CHUNKS = 64            # csrc/train.hip


def bn_sum_depth(P: int) -> int:
    """Longest chain of fp64 additions behind a channel's moment in bn_partial_kernel + bn_finalize_kernel: the serial
    additions of a row phase, the 4 phases, the 64 chunks in order."""
    rows_per = -(-P // BN_CHUNKS)
    return -(-rows_per // 4) + 3 + BN_CHUNKS


def bn_var_count(P: int, x0, mean, var):
    """Rounding count of the biased variance [C] (relative to the variance itself).  The kernel sums d = x - K and d^2 in
    fp64, K = x0 = the channel's value in row 0, and forms E[d^2] - E[d]^2: each of the D = bn_sum_depth(P) additions
    behind the two sums rounds at 2^-53 of a partial sum, E[d]^2 carries the error of the first sum twice:
    3 D 2^-53 ((K - mean)^2 + var) in all, that is 3 D (k^2 + 1) 2^-29 units of 2^-24 var with k = (K - mean) / std (K is
    one of the channel's own values: k^2 <= P); the differences and the four fp64 operations of the finalize kernel are
    inside the rounding-up.  Then the rounding to fp32 (1), + 1:
      c_var = 2 + ceil(3 D (k^2 + 1) 2^-29),
    3 for every input of the tests.  (Sums of the raw values, which the kernel formed before, have mean / std in the place
    of k: 8 at mean / std = 3000, 60 at 1e4, 5800 at 1e5.)  A channel of variance 0 has K = mean: its bound is 2^-126."""
    k2 = torch.where(var > 0, (d(x0) - mean) ** 2 / var.clamp_min(1e-300), torch.zeros_like(var))
    return 2.0 + torch.ceil(3.0 * bn_sum_depth(P) * (k2 + 1.0) * 2.0 ** -29)


def bn_train(x, gamma, beta, eps: float, momentum: float, rm=None, rv=None, residual=None, relu: bool = False):
    """x [P,C] -> dict of float64 tensors, two-pass statistics over the rows:
      mean, mean_mag = mean |x|;  var (biased; its bound is relative: c_var 2^-24 var, c_var [C] of ``bn_var_count``)
      rm, rm_mag = (1 - mom) |rm| + mom mean |x|;  rv, rv_mag = (1 - mom) |rv| + mom var P / (P - 1)  (P = 1: var)
      y = relu?(gamma (x - mean) rstd + beta + residual), y_mag = |gamma| rstd (|x| + mean |x|) + |beta| + |residual|
      y_rstd = |gamma| rstd |x - mean|: the part of y that a relative error of rstd scales."""
    x, ga, be = d(x), d(gamma), d(beta)
    P, C = x.shape
    mom, e = f32(momentum), f32(eps)
    mean = x.mean(dim=0)
    var = ((x - mean) ** 2).mean(dim=0)
    amean = x.abs().mean(dim=0)
    rstd = 1.0 / torch.sqrt(var + e)
    y = ga * (x - mean) * rstd + be
    y_mag = ga.abs() * rstd * (x.abs() + amean) + be.abs()
    if residual is not None:
        y, y_mag = y + d(residual), y_mag + d(residual).abs()
    if relu:
        y = y.clamp_min(0.0)
    out = dict(mean=mean, mean_mag=amean, var=var, c_var=bn_var_count(P, x[0], mean, var), y=y, y_mag=y_mag, y_rstd=ga.abs() * rstd * (x - mean).abs())
    unbiased = var * (P / (P - 1.0)) if P > 1 else var
    if rm is not None:
        out['rm'] = (1.0 - mom) * d(rm) + mom * mean
        out['rm_mag'] = (1.0 - mom) * d(rm).abs() + mom * amean
    if rv is not None:
        out['rv'] = (1.0 - mom) * d(rv) + mom * unbiased
        out['rv_mag'] = (1.0 - mom) * d(rv).abs() + mom * unbiased
    return out


# ------------------------------------------------------------------------------------------ Adagrad
def adagrad(p, g, state, lr: float, wd: float, eps: float = 1e-10):
    """torch.optim.Adagrad (lr_decay 0) -> dict:
      g' = g + wd p, mag_g = |g| + |wd p|
      state' = state + g'^2, state_mag = state + g'^2 + 2 |g'| mag_g  (the last term: what an error of g' does to g'^2)
      p' = p - lr g' / (sqrt(state') + eps), p_mag = |p| + |step| + |lr| mag_g / (sqrt(state') + eps)."""
    p, g, st = d(p), d(g), d(state)
    lr, wd, eps = f32(lr), f32(wd), f32(eps)
    gv = g + wd * p
    mag_g = g.abs() + (wd * p).abs()
    st2 = st + gv * gv
    den = torch.sqrt(st2) + eps
    step = lr * gv / den
    return dict(state=st2, state_mag=st + gv * gv + 2.0 * gv.abs() * mag_g, p=p - step,
                p_mag=p.abs() + step.abs() + abs(lr) * mag_g / den)


# ------------------------------------------------------------------------------------------ the bound
def worst_ratio(got, want, mag, c, slack=None):
    """-> worst |got - want| / (c 2^-24 mag (+ slack) + 2^-126) over the elements."""
    got = torch.as_tensor(np.asarray(got, dtype=np.float64)).reshape(want.shape) if not torch.is_tensor(got) else got.to(F64)
    if want.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all())
    bound = c * U * mag + TINY
    if slack is not None:
        bound = bound + slack
    return float(((got - want).abs() / bound).max())


def bn_ratios(got, r, with_var=True):
    """-> {output: worst |err| / bound} of a BatchNorm result (dict of arrays / tensors) against ``bn_train``."""
    t = lambda a: a.detach().cpu().to(F64) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float64))
    cv = r['c_var']
    out = {'mean': worst_ratio(t(got['mean']), r['mean'], r['mean_mag'], C_BN_MEAN),
           'y': worst_ratio(t(got['y']), r['y'], r['y_mag'], C_BN_Y, slack=0.5 * cv * U * r['y_rstd'])}
    var = float(((t(got['var']) - r['var']).abs() / (cv * U * r['var'] + TINY)).max())
    out['var' if with_var else 'var (not asserted)'] = var
    if 'rm' in r:
        out['running_mean'] = worst_ratio(t(got['rm']), r['rm'], r['rm_mag'], C_BN_RM)
        rv = float(((t(got['rv']) - r['rv']).abs() / ((C_BN_RV + cv) * U * r['rv_mag'] + TINY)).max())
        out['running_var' if with_var else 'running_var (not asserted)'] = rv
    return out


# ==========================================================================================
# Inputs of tests/test_hip_train_fwd_bound.py (and of the emulation tests of tests/test_train_ref_cpu.py)
# ==========================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _next(v, to):
    return float(np.nextafter(F32(v), F32(to)))


LOSS_SIZES = (0, 1, 63, 1023, 1024, 1025, 100003)
LOSS_AVG = 77.3                                    # not a power of two
LOSS_PROBES = (0, 63, 64, 1023, 1024, -1)          # one-hot weights: first / last lane of a wave, the block edge, the tail
BCE_LOGITS = [s * v for v in (0.0, 1e-3, 1.0, 20.0, 30.0, 40.0, 90.0, 104.0) for s in (1.0, -1.0)]
BCE_KINDS = ('thr', 'soft', 'hard')


def probe_indices(n):
    return sorted({i % n for i in LOSS_PROBES if -n <= i < n}) if n else []


def bce_case(n: int, kind: str):
    """-> (x, y, w, y_thr).  x = randn * 4 with the logits of BCE_LOGITS (+-{0, 1e-3, 1, 20, 30, 40, 90, 104}) on every
    third element.  Targets: 'thr' = probabilities binarised at 0.5 with every fifth element exactly at, one ulp below
    or one ulp above 0.5; 'soft' = probabilities as they are (y_thr -1); 'hard' = 0 / 1.  At the probe indices the
    logit is negative (-40, -30, -20, -1, -90, -1e-3 in turn) with target 0: the loss is log1p(exp(x)) alone, down to
    4e-18, and so is its magnitude."""
    g = _gen(100 + n + 7 * BCE_KINDS.index(kind))
    x = torch.randn(n, generator=g) * 4
    sp = torch.tensor(BCE_LOGITS)
    idx = torch.arange(n)
    sel = idx % 3 == 0
    x[sel] = sp[(idx[sel] // 3) % len(sp)]
    y = torch.rand(n, generator=g)
    if kind == 'thr':
        edge = torch.tensor([0.5, _next(0.5, 0.0), _next(0.5, 1.0)])
        sel = idx % 5 == 0
        y[sel] = edge[(idx[sel] // 5) % 3]
    if kind == 'hard':
        y = (y > 0.7).float()
    low = {'thr': _next(0.5, 0.0), 'soft': 0.0, 'hard': 0.0}[kind]
    for k, i in enumerate(probe_indices(n)):
        x[i] = (-40.0, -30.0, -20.0, -1.0, -90.0, -1e-3)[k % 6]
        y[i] = low
    w = torch.rand(n, generator=g) * 2
    w[idx % 11 == 3] = 0.0
    return x.contiguous(), y.contiguous(), w.contiguous(), (0.5 if kind == 'thr' else -1.0)


SL1_BETAS = (1.0, 1.0 / 9.0)


def smooth_l1_case(n: int, beta: float):
    """-> (pred, target, w).  randn * 2 against randn; every third element takes a difference from
    {beta, beta -+ 1 ulp, 0, and their negatives} (beta as the fp32 the kernel sees), alternately at the origin
    (target 0) and off it (target 0.75, pred = fl(0.75 + d) and its two fp32 neighbours: the difference the kernel forms is then d only to an
    ulp of the sum, on either side of the branch edge)."""
    g = _gen(200 + n + int(beta * 9))
    p, t = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    b = f32(beta)
    ds = [b, _next(b, 0.0), _next(b, 2.0), 0.0]
    ds = torch.tensor(ds + [-v for v in ds])
    idx = torch.arange(n)
    sel = idx % 3 == 0
    k = idx[sel] // 3
    base = torch.where(k % 2 == 0, torch.tensor(0.0), torch.tensor(0.75))
    t[sel] = base
    ps = (base + ds[(k // 2) % len(ds)]).numpy()
    shift = ((k // 16) % 3 - 1).numpy()                 # off the origin also one ulp of the sum below and above
    ps = np.where((base.numpy() > 0) & (shift != 0), np.nextafter(ps, np.where(shift > 0, F32(9), F32(-9)).astype(F32)), ps)
    p[sel] = torch.from_numpy(ps.astype(F32))
    w = torch.rand(n, generator=g) * 2
    w[idx % 11 == 3] = 0.0
    return p.contiguous(), t.contiguous(), w.contiguous()


CE_CLASSES = (1, 2, 4, 9)


def softmax_ce_case(n: int, C: int, all_ignored: bool = False):
    """-> (logits [n,C], labels [n] int64, w [n]).  Rows of randn * 3, each moved up until its maximum is at least 3
    (so that sum_c p_c |row_c - max| <= log 9 < |max|: ``softmax_ce_conditioning`` <= 1).  Every seventh row is special,
    in turn: the label's logit is the maximum by 100; all logits equal; logits at +-1e4 (label on +1e4, then on -1e4).
    Every fifth label is ignored: -1, C, 255 in turn.  C = 1: every counted row is exactly +0."""
    g = _gen(300 + n + C)
    z = torch.randn(n, C, generator=g) * 3
    z = z + (3.0 - z.max(dim=1, keepdim=True).values).clamp_min(0.0) if n else z
    lab = torch.randint(0, C, (n,), generator=g)
    for i in range(0, n, 7):
        k = (i // 7) % 4
        if k == 0:
            z[i] = torch.rand(C, generator=g) * 2
            z[i, lab[i]] = z[i].max() + 100.0
        elif k == 1:
            z[i] = 1.7
        else:
            z[i] = torch.where(torch.arange(C) % 2 == 0, torch.tensor(1e4), torch.tensor(-1e4))
            lab[i] = 0 if k == 2 else min(1, C - 1)
    ign = torch.tensor([-1, C, 255])
    idx = torch.arange(n)
    sel = idx % 5 == 4
    lab[sel] = ign[(idx[sel] // 5) % 3]
    if all_ignored:
        lab = ign[idx % 3]
    for i in probe_indices(n):                      # the probes look at counted rows
        if not all_ignored and not 0 <= int(lab[i]) < C:
            lab[i] = i % C
    w = torch.rand(n, generator=g) * 2
    return z.contiguous(), lab.contiguous(), w.contiguous()


# ---- bbox2delta
BBOX_SIZES = (0, 1, 255, 256, 257, 5000)
BBOX_CODERS = (((0., 0., 0., 0.), (1., 1., 1., 1.)), ((0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)))     # fgn_amd/config.py


def bbox_case(n: int):
    """-> (proposals, gts, kind [n]).  Row i is of kind i % 6: 0 generic boxes; 1 the GT is the proposal (all four deltas
    exactly 0); 2 boxes 1e3 from the origin with sides of about 4 px (the centres cancel); 3 / 4 the GT is 1e-3 / 1e3
    times as wide and high; 5 generic, but every tenth of them (i % 60 == 5) has a proposal of zero width."""
    g = _gen(400 + n)

    def boxes(span, lo, hi):
        ctr = torch.rand(n, 2, generator=g) * span
        wh = torch.rand(n, 2, generator=g) * (hi - lo) + lo
        return torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    p, q = boxes(300.0, 4.0, 84.0), boxes(300.0, 4.0, 84.0)
    kind = torch.arange(n) % 6
    q[kind == 1] = p[kind == 1]
    far_p, far_q = boxes(8.0, 3.5, 4.5) + 1000.0, boxes(8.0, 3.5, 4.5) + 1000.0
    p[kind == 2], q[kind == 2] = far_p[kind == 2], far_q[kind == 2]
    for k, ratio in ((3, 1e-3), (4, 1e3)):
        m = kind == k
        c = (p[m, :2] + p[m, 2:]) / 2 + torch.randn(int(m.sum()), 2, generator=g)
        wh = (p[m, 2:] - p[m, :2]) * ratio
        q[m] = torch.cat([c - wh / 2, c + wh / 2], 1)
    zero = torch.arange(n) % 60 == 5
    p[zero, 2] = p[zero, 0]
    return p.contiguous(), q.contiguous(), kind


# ---- BatchNorm
BN_SHAPES = ((1, 4), (3, 64), (63, 4), (64, 8), (65, 260), (441, 1024), (6273, 128), (8200, 512))
BN_RATIOS = (0, 0.25, 30, 1000, 3000)              # mean / std with every output asserted
BN_FAR_RATIOS = (1e4, 1e5)                         # y and mean asserted, the variance measured
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_case(P: int, C: int, ratio: float):
    """-> dict(x [P,C], gamma, beta, rm, rv, res).  Channel c is randn * s_c + sign_c ratio s_c with s_c in [0.65, 1.95]
    (mean / std = ratio up to the sample's own deviation).  Channel 0 is constant (variance exactly 0), channel 1 is
    scaled by 1e-4 (variance ~1e-8, far below eps), gamma[2] is negative and gamma[3] zero."""
    g = _gen(500 + P + C + int(ratio * 4) % 100003)
    s = 1.3 * (0.5 + torch.rand(C, generator=g))
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    x = torch.randn(P, C, generator=g) * s + sign * ratio * s
    x[:, 0] = 3.7 + float(sign[0]) * ratio * 1.3
    x[:, 1] *= 1e-4
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    gamma[2], gamma[3] = -gamma[2], 0.0
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    res = torch.randn(P, C, generator=g)
    return dict(x=x.contiguous(), gamma=gamma, beta=beta, rm=rm, rv=rv, res=res)


# ---- Adagrad
ADAGRAD_SIZES = (1, 255, 4095, 4096, 4097, 1048576 + 3)
ADAGRAD_PAIRS = ((1e-5, 0.005), (0.0, 0.01), (1e-4, 0.01))        # (weight decay, lr)
ADAGRAD_EPS = 1e-10


def adagrad_case(n: int, wd: float, warm: bool, seed: int = 0):
    """-> (p, g, state, kind [n]).  p = randn, g = +-10^U(-6, 1), state = 0 (fresh) or 10^U(-8, 2) (warm).  Element i
    is of kind i % 8: 3 -> g = 0 on a zero state (and p = 0 on every other of them: with weight decay only those keep
    g' = 0); 5 -> g = -wd p (1 +- 1e-3), the cancelling gradient; 6 -> g = 1e-25 with p = 0, whose square underflows;
    the others generic.  The kinds repeat to the last element, so every launch has them beyond its first grid pass."""
    g_ = _gen(600 + n + seed + (1 if warm else 0) + int(wd * 1e6))
    p = torch.randn(n, generator=g_)
    mant = torch.rand(n, generator=g_) * 7 - 6
    gr = (10.0 ** mant) * (torch.randint(0, 2, (n,), generator=g_).float() * 2 - 1)
    st = 10.0 ** (torch.rand(n, generator=g_) * 10 - 8) if warm else torch.zeros(n)
    idx = torch.arange(n)
    kind = idx % 8
    z = kind == 3
    gr[z], st[z] = 0.0, 0.0
    p[z & (idx % 16 == 3)] = 0.0
    c = kind == 5
    gr[c] = (-f32(wd) * p[c].double() * (1.0 + 1e-3 * torch.randn(int(c.sum()), generator=g_).double())).float()
    u = kind == 6
    gr[u], p[u] = 1e-25, 0.0
    return p.contiguous(), gr.contiguous(), st.contiguous(), kind


ADAGRAD_MULTI_SIZES = (0, 1, 4096, 4097, 5)
ADAGRAD_MULTI_LRS = (0.005, 0.0005, 0.01, 0.003, 0.02)
