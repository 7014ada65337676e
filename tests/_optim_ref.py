"""Closed-form float64 restatements of the optimiser kernels of fgn_amd/csrc/optim.hip (CPU, torch.float64): the Adam,
SGD and Adagrad rules of ``fgn_optim_multi_f32`` with its gradient multiplier, the global gradient norm and clip
coefficient of ``fgn_grad_sqnorm_multi_f32`` and the accumulation of ``fgn_grad_accumulate_multi_f32``.

Conventions of tests/_bwd_ref.py and tests/_train_ref.py: operands are fp32 tensors (any device) widened to float64;
scalars the C ABI carries as ``float`` (lr, weight decay, eps, betas, momentum, max_norm, the accumulation weight) are
rounded to fp32 first, because the reference works on the operands the kernel sees; Adam's bias corrections are formed
in double from the fp32 betas, as the host side of the kernel forms them.  ``gmul`` is the gradient multiplier as a
double: the exact product of the fp32 clip coefficient and the fp32 host scale (1.0: none).  Every function returns the
result and, per element, its TERM-MAGNITUDE SUM ``*_mag``: the expression with every term replaced by its absolute
value, plus the conditioning terms written out in each docstring (what an error of g' does further down).
tests/test_hip_optim.py bounds every output by ``c * 2^-24 * mag + 2^-126`` with the counts below;
tests/test_optim_ref_cpu.py pins each closed form to torch.optim in float64 and holds an fp32 numpy emulation of each
kernel to the same bound on the same inputs.
"""
import math

import numpy as np
import torch

from _bwd_ref import TINY, U, d, f32  # noqa: F401  (re-exported to the tests)
from _train_ref import (ADAGRAD_EPS, ADAGRAD_MULTI_LRS, ADAGRAD_MULTI_SIZES, ADAGRAD_PAIRS, ADAGRAD_SIZES,  # noqa: F401
                        adagrad_case, worst_ratio)

F64 = torch.float64

# Rounding counts; the docstrings of tests/test_hip_optim.py derive each from the kernel's code.
C_G = 4                                   # g' = g mul + wd p
C_ADAM_M, C_ADAM_V, C_ADAM_P = 7, 6, 12
C_SGD_BUF, C_SGD_P = 5, 10
C_ADA_STATE, C_ADA_P = 5, 9
C_NORM, C_COEF = 2, 4
C_ACC = 2

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
SGD_MOMENTUM = 0.9
SIZES, PAIRS = ADAGRAD_SIZES, ADAGRAD_PAIRS
# 70 tensors, 4 of them empty (the first, two inside, the last): 66 take a slot, so the list fills one 64-slot table and
# continues in a second launch
MANY_SIZES = tuple(0 if i in (0, 17, 40, 69) else [3, 4097, 1, 260, 4096, 7][i % 6] for i in range(70))
assert sum(1 for n in MANY_SIZES if n) > 64


def _gprime(p, g, wd, gmul):
    gm = g * float(gmul)
    return gm + wd * p, gm.abs() + (wd * p).abs()


def adam(p, g, m, v, t: int, lr: float, wd: float, betas=ADAM_BETAS, eps: float = ADAM_EPS, gmul: float = 1.0):
    """torch.optim.Adam (L2 decay, no amsgrad), step number ``t`` (counting this one) -> dict:
      g' = g gmul + wd p, mag_g = |g gmul| + |wd p|
      m' = b1 m + (1 - b1) g', m_mag = |b1 m| + (1 - b1) mag_g
      v' = b2 v + (1 - b2) g'^2, v_mag = v' + (1 - b2) 2 |g'| mag_g          (what an error of g' does to g'^2)
      den = sqrt(v') / sqrt(bc2) + eps, s = lr / bc1, step = s m' / den
      p' = p - step, p_mag = |p| + |step| + s m_mag / den + |step| (1 - b2) |g'| mag_g / (sqrt(v') sqrt(bc2) den)
    (the last term: the error of g' through v' under the square root)."""
    p, g, m, v = d(p), d(g), d(m), d(v)
    lr, wd, eps = f32(lr), f32(wd), f32(eps)
    b1, b2 = f32(betas[0]), f32(betas[1])
    bc1, bc2 = 1.0 - b1 ** int(t), 1.0 - b2 ** int(t)
    gv, mag_g = _gprime(p, g, wd, gmul)
    m2 = b1 * m + (1.0 - b1) * gv
    m_mag = (b1 * m).abs() + (1.0 - b1) * mag_g
    v2 = b2 * v + (1.0 - b2) * gv * gv
    v_mag = v2 + (1.0 - b2) * 2.0 * gv.abs() * mag_g
    rs = math.sqrt(bc2)
    sv = torch.sqrt(v2)
    den = sv / rs + eps
    s = lr / bc1
    step = s * m2 / den
    thru = torch.where(sv > 0, step.abs() * (1.0 - b2) * gv.abs() * mag_g / (sv.clamp_min(1e-300) * rs * den),
                       torch.zeros_like(sv))
    return dict(m=m2, m_mag=m_mag, v=v2, v_mag=v_mag, p=p - step,
                p_mag=p.abs() + step.abs() + s * m_mag / den + thru)


def sgd(p, g, buf, lr: float, wd: float, momentum: float = SGD_MOMENTUM, nesterov: bool = False, gmul: float = 1.0):
    """torch.optim.SGD (dampening 0); ``buf`` None with momentum 0 -> dict:
      g' = g gmul + wd p;  buf' = mu buf + g', buf_mag = |mu buf| + mag_g  (momentum 0: buf' = g', no state)
      p' = p - lr (g' + mu buf')  [Nesterov]  |  p - lr buf';  p_mag = |p| + lr (mag_g + mu buf_mag)  |  |p| + lr buf_mag."""
    p, g = d(p), d(g)
    lr, wd, mu = f32(lr), f32(wd), f32(momentum)
    gv, mag_g = _gprime(p, g, wd, gmul)
    if mu == 0.0:
        return dict(buf=None, buf_mag=None, p=p - lr * gv, p_mag=p.abs() + lr * mag_g)
    b2 = mu * d(buf) + gv
    b_mag = (mu * d(buf)).abs() + mag_g
    if nesterov:
        return dict(buf=b2, buf_mag=b_mag, p=p - lr * (gv + mu * b2), p_mag=p.abs() + lr * (mag_g + mu * b_mag))
    return dict(buf=b2, buf_mag=b_mag, p=p - lr * b2, p_mag=p.abs() + lr * b_mag)


def adagrad(p, g, state, lr: float, wd: float, eps: float = ADAGRAD_EPS, gmul: float = 1.0):
    """torch.optim.Adagrad (lr_decay 0), the terms of ``_train_ref.adagrad`` with the multiplied gradient -> dict:
      state' = state + g'^2, state_mag = state + g'^2 + 2 |g'| mag_g
      p' = p - lr g' / (sqrt(state') + eps), p_mag = |p| + |step| + lr mag_g / (sqrt(state') + eps)."""
    p, g, st = d(p), d(g), d(state)
    lr, wd, eps = f32(lr), f32(wd), f32(eps)
    gv, mag_g = _gprime(p, g, wd, gmul)
    st2 = st + gv * gv
    den = torch.sqrt(st2) + eps
    step = lr * gv / den
    return dict(state=st2, state_mag=st2 + 2.0 * gv.abs() * mag_g, p=p - step,
                p_mag=p.abs() + step.abs() + lr * mag_g / den)


def grad_norm(grads, max_norm: float):
    """clip_grad_norm_(max_norm, norm_type=2): -> (norm, coef) as Python floats, norm = sqrt(fsum g^2) (every square and
    the sum exact), coef = min(1, max_norm / (norm + 1e-6)) with max_norm and 1e-6 as fp32.  Both are their own
    magnitudes (sums of positive terms)."""
    sq = []
    for g in grads:
        a = d(g).reshape(-1).numpy()
        sq.append(a * a)                                             # exact in double: 24-bit mantissas
    norm = math.sqrt(math.fsum(np.concatenate(sq).tolist())) if sq else 0.0
    return norm, min(1.0, f32(max_norm) / (norm + f32(1e-6)))


def accumulate(acc, g, a: float, first: bool):
    """acc' = (0 if first else acc) + a g -> (acc', mag = |acc| + |a g|)."""
    ag = f32(a) * d(g)
    if first:
        return ag, ag.abs()
    return d(acc) + ag, d(acc).abs() + ag.abs()


# ------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def emul_gprime(p, g, wd, coef, scale):
    """update_one's first two lines, one fp32 operation each (contraction off): mul = coef * scale, g * mul, + wd * p."""
    F = np.float32
    if coef is not None or F(scale) != F(1.0):
        mul = F(scale) if coef is None else F(coef) * F(scale)
        g = g * mul
    return g + F(wd) * p


def emul_adam(p, g, m, v, t, lr, wd, betas=ADAM_BETAS, eps=ADAM_EPS, coef=None, scale=1.0):
    F = np.float32
    p, g, m, v = _np(p), _np(g), _np(m), _np(v)
    b1, b2 = F(betas[0]), F(betas[1])
    bc1, bc2 = 1.0 - float(b1) ** int(t), 1.0 - float(b2) ** int(t)
    s, rs = F(float(F(lr)) / bc1), F(math.sqrt(bc2))
    gv = emul_gprime(p, g, wd, coef, scale)
    m2 = b1 * m + (F(1.0) - b1) * gv
    v2 = b2 * v + (F(1.0) - b2) * (gv * gv)
    p2 = p - s * m2 / (np.sqrt(v2) / rs + F(eps))
    return p2, m2, v2


def emul_sgd(p, g, buf, lr, wd, momentum=SGD_MOMENTUM, nesterov=False, coef=None, scale=1.0):
    F = np.float32
    p, g = _np(p), _np(g)
    mu = F(momentum)
    gv = emul_gprime(p, g, wd, coef, scale)
    if mu == 0:
        return p - F(lr) * gv, None
    b2 = mu * _np(buf) + gv
    return p - F(lr) * ((gv + mu * b2) if nesterov else b2), b2


def emul_adagrad(p, g, st, lr, wd, eps=ADAGRAD_EPS, coef=None, scale=1.0):
    F = np.float32
    p, g, st = _np(p), _np(g), _np(st)
    gv = emul_gprime(p, g, wd, coef, scale)
    st2 = st + gv * gv
    return p - F(lr) * gv / (np.sqrt(st2) + F(eps)), st2


def emul_grad_norm(grads, max_norm):
    """Both stages in the kernel's order: thread t of a chunk adds elements 1024 j + 4 t + e in (j, e) order, xor
    butterfly over 64 lanes, 4 wave sums in order; the final block adds partials t, t + 256, ... and reduces alike."""
    def block(vals256):
        w = vals256.reshape(4, 64).copy()
        m = 32
        while m >= 1:
            w = w + w[:, np.arange(64) ^ m]
            m >>= 1
        s = w[0, 0]
        for i in range(1, 4):
            s = s + w[i, 0]
        return s
    parts = []
    for g in grads:
        a = _np(g).reshape(-1).astype(np.float64)
        for c0 in range(0, a.size, 4096):
            ch = np.zeros(4096)
            seg = a[c0:c0 + 4096]
            ch[:seg.size] = seg
            sq = (ch * ch).reshape(4, 256, 4)                       # [j, t, e]
            acc = np.zeros(256)
            for j in range(4):
                for e in range(4):
                    acc = acc + sq[j, :, e]
            parts.append(block(acc))
    acc = np.zeros(256)
    pa = np.asarray(parts, dtype=np.float64)
    for i0 in range(0, pa.size, 256):
        seg = pa[i0:i0 + 256]
        acc[:seg.size] = acc[:seg.size] + seg
    F = np.float32
    norm = F(math.sqrt(block(acc)))
    c = F(max_norm) / (norm + F(1e-6))
    return norm, (F(1.0) if c > 1 else c)


def emul_accumulate(acc, g, a, first):
    r = np.float32(a) * _np(g)
    return r if first else _np(acc) + r


# ------------------------------------------------------------------------------------------ inputs of the tests
def warm_state(n: int, seed: int):
    """Adam / SGD state after some steps: exp_avg / momentum buffer = randn * 10^U(-6, 0), exp_avg_sq = 10^U(-10, 1)."""
    g_ = torch.Generator().manual_seed(7100 + n + seed)
    m = torch.randn(n, generator=g_) * 10.0 ** (torch.rand(n, generator=g_) * 6 - 6)
    v = 10.0 ** (torch.rand(n, generator=g_) * 11 - 10)
    return m.contiguous(), v.contiguous()


def optim_case(n: int, wd: float, warm: bool, seed: int = 0):
    """-> (p, g, m, v, kind): the parameter / gradient classes of ``adagrad_case`` with an Adam / SGD state: zeros
    (fresh) or ``warm_state``; kind 3 (g = 0 on zero state) keeps a zero state in the warm case too."""
    p, g, _, kind = adagrad_case(n, wd, warm, seed)
    if warm:
        m, v = warm_state(n, seed)
        m[kind == 3], v[kind == 3] = 0.0, 0.0
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v, kind


# ------------------------------------------------------------------------------------------ the cases, shared by the
# GPU test (tests/test_hip_optim.py) and the emulation test (tests/test_optim_ref_cpu.py)
RULES = (('Adam', {}), ('SGD', dict(momentum=SGD_MOMENTUM, nesterov=True)), ('SGD', dict(momentum=SGD_MOMENTUM, nesterov=False)),
         ('SGD', dict(momentum=0.0)), ('Adagrad', {}))
# (coef, scale) of the gradient multiplier: the clip coefficient alone, the host rescale alone, both
MULTIPLIERS = ((0.37, 1.0), (None, 2.0), (0.37, 4.0 / 3.0))


def rule_id(rule_opts) -> str:
    rule, o = rule_opts
    if rule != 'SGD':
        return rule
    return 'SGD-mu0' if o['momentum'] == 0.0 else ('SGD-nesterov' if o.get('nesterov') else 'SGD-momentum')


def initial_state(rule, opts, n, wd, warm, seed=0):
    """-> (p, g, [state tensors], kind)."""
    p, g, m, v, kind = optim_case(n, wd, warm, seed)
    if rule == 'Adam':
        return p, g, [m, v], kind
    if rule == 'SGD':
        return p, g, ([] if opts['momentum'] == 0.0 else [m]), kind
    st = adagrad_case(n, wd, warm, seed)[2]
    return p, g, [st], kind


def reference(rule, opts, p, g, states, t, lr, wd, gmul):
    """-> (p', p_mag, c_p, [(state', state_mag, c_state), ...]) of one step."""
    if rule == 'Adam':
        r = adam(p, g, states[0], states[1], t, lr, wd, gmul=gmul)
        return r['p'], r['p_mag'], C_ADAM_P, [(r['m'], r['m_mag'], C_ADAM_M), (r['v'], r['v_mag'], C_ADAM_V)]
    if rule == 'SGD':
        r = sgd(p, g, states[0] if states else None, lr, wd, opts['momentum'], opts.get('nesterov', False), gmul=gmul)
        return r['p'], r['p_mag'], C_SGD_P, ([(r['buf'], r['buf_mag'], C_SGD_BUF)] if states else [])
    r = adagrad(p, g, states[0], lr, wd, gmul=gmul)
    return r['p'], r['p_mag'], C_ADA_P, [(r['state'], r['state_mag'], C_ADA_STATE)]


def emulate(rule, opts, p, g, states, t, lr, wd, coef, scale):
    """The kernel's fp32 arithmetic in numpy -> (p', [state', ...]) as fp32 CPU tensors."""
    with np.errstate(under='ignore'):
        if rule == 'Adam':
            out = emul_adam(p, g, states[0], states[1], t, lr, wd, coef=coef, scale=scale)
            res = [out[0], out[1], out[2]]
        elif rule == 'SGD':
            p2, b2 = emul_sgd(p, g, states[0] if states else None, lr, wd, opts['momentum'], opts.get('nesterov', False),
                              coef=coef, scale=scale)
            res = [p2] + ([b2] if states else [])
        else:
            res = list(emul_adagrad(p, g, states[0], lr, wd, coef=coef, scale=scale))
    assert all(a.dtype == np.float32 for a in res)
    res = [torch.from_numpy(np.ascontiguousarray(a)) for a in res]
    return res[0], res[1:]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_steps(tag, step_fn, rule, opts, n, wd, lr, warm, t0=1, steps=3, coef=None, scale=1.0):
    """``steps`` consecutive updates by ``step_fn(rule, opts, p, g, states, t, lr, wd, coef, scale) -> (p', states')`` (CPU
    fp32 tensors in and out), each bounded against the reference started from step_fn's OWN previous parameters and
    state, so errors do not compound into the bound.  Where g' = 0 on a zero state p keeps its bits and the state stays
    +0.  Prints and returns the worst |err| / bound of the parameter and of each state."""
    p, g, states, kind = initial_state(rule, opts, n, wd, warm)
    gmul = (1.0 if coef is None else float(np.float32(coef))) * float(np.float32(scale))
    worst = {}
    still = (kind == 3) & ((p == 0) | (f32(wd) == 0))
    assert n < 255 or int(still.sum()) > 0
    for s_ in range(steps):
        t = t0 + s_
        pr, pmag, cp, sts = reference(rule, opts, p, g, states, t, lr, wd, gmul)
        p2, states2 = step_fn(rule, opts, p, g, states, t, lr, wd, coef, scale)
        worst['p'] = max(worst.get('p', 0.0), worst_ratio(p2, pr, pmag, cp))
        for i, ((sr, smag, cs), s2) in enumerate(zip(sts, states2)):
            worst[f'state{i}'] = max(worst.get(f'state{i}', 0.0), worst_ratio(s2, sr, smag, cs))
        if s_ == 0:
            assert torch.equal(_bits(p2[still]), _bits(p[still])), tag
            for s2 in states2:
                assert bool((_bits(s2[still]) == 0).all()), tag
        if rule != 'SGD':
            assert bool((states2[-1] >= 0).all())
        p, states = p2, states2
    print(f'[optim-bound] {tag}: worst |err| / bound ' + ', '.join(f'{k} = {v:.4f}' for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    return worst
