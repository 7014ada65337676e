"""The float64 closed forms of tests/_train_ref.py pinned to independent implementations (no GPU), and a numpy emulation
of each kernel's arithmetic (fp32 where the kernel is fp32, fp64 where it accumulates in fp64, in the kernel's order)
held to the bound of tests/test_hip_train_fwd_bound.py on every input that file uses: the closed forms and the derived
rounding counts are shown to fit each other before a GPU is involved.  Each emulation test prints
``[train-emul] name: worst |err| / bound`` (DESIGN.md section 7.3 carries the table)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _train_ref as ref
from oracle import fgn_train_cpu as T

F64 = torch.float64
F32 = np.float32
U, TINY = ref.U, ref.TINY


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_ratio = ref.worst_ratio


def _report(name, worst):
    print(f'[train-emul] {name}: worst |err| / bound = {worst:.4f}')
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------------ closed forms, pinned
@pytest.mark.parametrize('kind', ref.BCE_KINDS)
def test_bce_sum_matches_torch_float64(kind):
    x, y, w, thr = ref.bce_case(1025, kind)
    yd = (y >= np.float32(thr)).to(F64) if thr >= 0 else y.to(F64)
    per = F.binary_cross_entropy_with_logits(x.to(F64), yd, reduction='none')
    for ww in (None, w):
        val, mag = ref.bce_sum(x, y, ww, ref.LOSS_AVG, thr)
        wd = torch.ones_like(per) if ww is None else ww.to(F64)
        assert float((val - (per * wd).sum() / ref.LOSS_AVG).abs()) <= 1e-13 * float(mag)
        # mag, a plain second formulation: element by element, |x| where the first two terms do not cancel
        xs, ys = x.tolist(), yd.tolist()
        m2 = sum(abs(wi) * (max(xi, 0.0) + abs(xi * yi) + np.log1p(np.exp(-abs(xi)))) for xi, yi, wi in zip(xs, ys, wd.tolist()))
        assert float(mag) == pytest.approx(m2 / ref.LOSS_AVG, rel=1e-12)
        assert abs(float(val)) <= float(mag)
    assert float(ref.bce_sum(x[:0], y[:0], None, 3.0)[0]) == 0.0


@pytest.mark.parametrize('beta', ref.SL1_BETAS)
def test_smooth_l1_sum_matches_torch_float64_and_the_oracle(beta):
    p, t, w = ref.smooth_l1_case(1025, beta)
    b = ref.f32(beta)
    pd, td, wd = p.to(F64), t.to(F64), w.to(F64)
    val, mag = ref.smooth_l1_sum(p, t, w, ref.LOSS_AVG, beta)
    per = F.smooth_l1_loss(pd, td, reduction='none', beta=b)
    assert float((val - (per * wd).sum() / ref.LOSS_AVG).abs()) <= 1e-13 * float(mag)
    assert float((val - T.smooth_l1_weighted(pd, td, wd, ref.LOSS_AVG, beta=b)).abs()) <= 1e-13 * float(mag)
    val1, _ = ref.smooth_l1_sum(p, t, None, ref.LOSS_AVG, beta)
    assert float((val1 - per.sum() / ref.LOSS_AVG).abs()) <= 1e-13 * float(mag) * 2
    m2 = 0.0
    for pi, ti, wi in zip(pd.tolist(), td.tolist(), wd.tolist()):
        dd = abs(pi - ti)
        m2 += wi * ((0.5 * dd * dd / b + dd / b * (abs(pi) + abs(ti))) if dd < b else (dd - 0.5 * b + abs(pi) + abs(ti) + 0.5 * b))
    assert float(mag) == pytest.approx(m2 / ref.LOSS_AVG, rel=1e-12)


@pytest.mark.parametrize('C', ref.CE_CLASSES)
def test_softmax_ce_sum_matches_torch_float64_and_the_oracle(C):
    z, lab, w = ref.softmax_ce_case(1025, C)
    zd, wd = z.to(F64), w.to(F64)
    ok = (lab >= 0) & (lab < C)
    lab_t = torch.where(ok, lab, torch.tensor(-100))
    val, mag = ref.softmax_ce_sum(z, lab, w, ref.LOSS_AVG)
    per = F.cross_entropy(zd, lab_t, reduction='none', ignore_index=-100)
    assert float((val - (per * wd).sum() / ref.LOSS_AVG).abs()) <= 1e-13 * float(mag) + 1e-300
    assert float((val - T.softmax_ce_weighted(zd, lab_t, wd, ref.LOSS_AVG)).abs()) <= 1e-13 * float(mag) + 1e-300
    m2 = 0.0
    for r, li, wi in zip(zd.tolist(), lab.tolist(), wd.tolist()):
        if 0 <= li < C:
            mx = max(r)
            m2 += wi * (abs(mx) + abs(np.log(sum(np.exp(v - mx) for v in r))) + abs(r[li]))
    assert float(mag) == pytest.approx(m2 / ref.LOSS_AVG, rel=1e-12, abs=1e-300)
    assert int((~ok).sum()) > 100 and {-1, C, 255} <= set(lab[~ok].tolist())
    z0, lab0, _ = ref.softmax_ce_case(63, C, all_ignored=True)
    assert float(ref.softmax_ce_sum(z0, lab0, None, 2.0)[0]) == 0.0 and float(ref.softmax_ce_sum(z0, lab0, None, 2.0)[1]) == 0.0


@pytest.mark.parametrize('coder', ref.BBOX_CODERS)
def test_bbox2delta_matches_the_oracle_and_its_fp32_form(coder):
    """The oracle's bbox2delta is fp32 torch (its logarithm within an ulp): it and the bit-level fp32 form are inside the
    bound of the float64 form wherever that is finite; GT == proposal is exactly 0; a zero-width proposal is non-finite
    in dx and dw in both."""
    means, stds = coder
    p, q, kind = ref.bbox_case(5000)
    val, mag = ref.bbox2delta(p, q, means, stds)
    fin = torch.isfinite(val)
    c = torch.tensor([ref.C_BBOX_XY, ref.C_BBOX_XY, ref.C_BBOX_WH, ref.C_BBOX_WH], dtype=F64)
    e32 = torch.from_numpy(ref.bbox2delta_f32(p, q, means, stds))
    with np.errstate(all='ignore'):
        orc = T.bbox2delta(p, q, means, stds)
    for got in (e32, orc):
        assert torch.equal(torch.isfinite(got), fin)
        err = ((got.to(F64) - val).abs() / (c * U * mag + TINY))[fin]
        assert float(err.max()) <= 1.0
    assert bool((val[kind == 1] == 0).all()) and bool((e32[kind == 1] == 0).all())
    zero = (p[:, 2] == p[:, 0])
    assert int(zero.sum()) > 50 and bool((~fin[zero][:, [0, 2]]).all()) and bool(fin[zero][:, [1, 3]].all())
    assert bool(fin[~zero].all())
    # plain second formulation of dx and dw on one row
    i = 6
    pw, gw = float(p[i, 2].double() - p[i, 0].double()), float(q[i, 2].double() - q[i, 0].double())
    dx = ((float(q[i, 0].double() + q[i, 2].double()) - float(p[i, 0].double() + p[i, 2].double())) / 2 / pw - ref.f32(means[0])) / ref.f32(stds[0])
    assert float(val[i, 0]) == pytest.approx(dx, rel=1e-12)
    assert float(val[i, 2]) == pytest.approx((np.log(gw / pw) - ref.f32(means[2])) / ref.f32(stds[2]), rel=1e-12)


@pytest.mark.parametrize('P,C,ratio', [(3, 64, 0.25), (65, 260, 30), (441, 8, 3000), (1, 4, 0)])
def test_bn_train_matches_torch_float64(P, C, ratio):
    k = ref.bn_case(P, C, ratio)
    x, ga, be, rm, rv, res = (k[n].to(F64) for n in ('x', 'gamma', 'beta', 'rm', 'rv', 'res'))
    eps, mom = ref.f32(ref.BN_EPS), ref.f32(ref.BN_MOMENTUM)
    r = ref.bn_train(k['x'], k['gamma'], k['beta'], ref.BN_EPS, ref.BN_MOMENTUM, k['rm'], k['rv'], k['res'], True)
    rm_t, rv_t = rm.clone(), rv.clone()
    if P > 1:
        want = F.batch_norm(x.t()[None].contiguous(), rm_t, rv_t, ga, be, True, mom, eps)[0].t()
    else:                                            # torch refuses one value per channel: the kernel's convention
        want = be.expand(1, C).clone()
        rm_t, rv_t = (1 - mom) * rm + mom * x[0], (1 - mom) * rv
    assert bool(((r['y'] - F.relu(want + res)).abs() <= 1e-9 * r['y_mag']).all())
    assert torch.allclose(r['rm'], rm_t, rtol=1e-12, atol=1e-14) and torch.allclose(r['rv'], rv_t, rtol=1e-9, atol=1e-14)
    assert torch.allclose(r['mean'], x.mean(0), rtol=1e-12, atol=1e-14)
    if P > 1:
        assert torch.allclose(r['var'], x.var(0, unbiased=False), rtol=1e-6, atol=1e-300)
    assert bool((r['var'][0] == 0)) and bool((r['var'] >= 0).all())
    # mag: the formulation with explicit loops over the channels
    for c in (0, 1, 2, 3):
        xa = x[:, c].abs()
        rstd = 1.0 / np.sqrt(float(r['var'][c]) + eps)
        m2 = abs(float(ga[c])) * rstd * (xa + xa.mean()) + abs(float(be[c])) + res[:, c].abs()
        assert torch.allclose(r['y_mag'][:, c], m2, rtol=1e-12, atol=0)
        assert float(r['rm_mag'][c]) == pytest.approx((1 - mom) * abs(float(rm[c])) + mom * float(xa.mean()), rel=1e-12)
    plain = ref.bn_train(k['x'], k['gamma'], k['beta'], ref.BN_EPS, ref.BN_MOMENTUM)
    assert 'rm' not in plain and bool(((plain['y'] - want).abs() <= 1e-9 * plain['y_mag']).all())
    assert bool((plain['y_rstd'] <= plain['y_mag'] * (1 + 1e-12)).all())


@pytest.mark.parametrize('wd,lr', ref.ADAGRAD_PAIRS)
def test_adagrad_matches_torch_float64(wd, lr):
    p, g, st, _ = ref.adagrad_case(4097, wd, True)
    wdf, lrf, eps = ref.f32(wd), ref.f32(lr), ref.f32(ref.ADAGRAD_EPS)
    q = torch.nn.Parameter(p.to(F64).clone())
    opt = torch.optim.Adagrad([q], lr=lrf, weight_decay=wdf, eps=eps)
    q.grad = torch.zeros_like(q)
    opt.state[q]['sum'].copy_(st.to(F64))
    cur_p, cur_s = p.to(F64), st.to(F64)
    for _ in range(3):
        q.grad = g.to(F64).clone()
        opt.step()
        r = ref.adagrad(cur_p, g, cur_s, lr, wd, ref.ADAGRAD_EPS)
        cur_p, cur_s = r['p'], r['state']
        assert torch.allclose(cur_s, opt.state[q]['sum'], rtol=1e-13, atol=0)
        assert torch.allclose(cur_p, q.detach(), rtol=1e-13, atol=1e-300)
    gv = g.to(F64) + wdf * p.to(F64)
    r = ref.adagrad(p, g, st, lr, wd, ref.ADAGRAD_EPS)
    mg = g.to(F64).abs() + abs(wdf) * p.to(F64).abs()
    assert torch.allclose(r['state_mag'], st.to(F64) + gv ** 2 + 2 * gv.abs() * mg, rtol=1e-13, atol=0)
    den = (st.to(F64) + gv ** 2).sqrt() + eps
    assert torch.allclose(r['p_mag'], p.to(F64).abs() + (lrf * gv / den).abs() + lrf * mg / den, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------ emulations of the kernels
def _block_sum(terms, avg):
    """loss_block_finish: thread t adds its elements t, t + 1024, ... in order, a 64-lane xor butterfly, the 16 wave
    partials in order, the division by avg_factor in fp64, one rounding to fp32."""
    n = terms.size
    rows = max(-(-n // 1024), 1)
    pad = np.zeros(rows * 1024)
    pad[:n] = terms
    acc = np.zeros(1024)
    for r in pad.reshape(rows, 1024):
        acc = acc + r
    v = acc.reshape(16, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    s = 0.0
    for part in v[:, 0]:
        s = s + part
    return F32(s / avg)


def _np(t, dtype=F32):
    return t.detach().cpu().numpy().astype(dtype)


def emul_bce(x, y, w, avg, thr):
    xd, y32 = _np(x, np.float64), _np(y)
    yv = (y32 >= F32(thr)).astype(np.float64) if F32(thr) >= 0 else y32.astype(np.float64)
    l = np.maximum(xd, 0.0) - xd * yv + np.log1p(np.exp(-np.abs(xd)))
    lf = l.astype(F32).astype(np.float64)
    return _block_sum(lf if w is None else _np(w, np.float64) * lf, avg)


def emul_smooth_l1(p, t, w, avg, beta):
    b = F32(beta)
    dd = np.abs(_np(p) - _np(t))
    with np.errstate(under='ignore'):
        l = np.where(dd < b, F32(0.5) * dd * dd / b, dd - F32(0.5) * b).astype(F32)
        term = l if w is None else _np(w) * l
    assert term.dtype == F32
    return _block_sum(term.astype(np.float64), avg)


def emul_softmax_ce(z, lab, w, avg):
    z32, lab = _np(z), lab.numpy()
    n, C = z32.shape
    if n == 0:
        return _block_sum(np.zeros(0), avg)
    m = z32.max(axis=1)
    s = np.exp((z32 - m[:, None]).astype(np.float64)).sum(axis=1)       # (C <= 9 terms in order; fp64)
    ok = (lab >= 0) & (lab < C)
    picked = z32[np.arange(n), np.clip(lab, 0, C - 1)]
    l = (m.astype(np.float64) + np.log(s) - picked.astype(np.float64)).astype(F32)
    term = l if w is None else _np(w) * l
    return _block_sum(np.where(ok, term.astype(np.float64), 0.0), avg)


def test_loss_sum_emulations_stay_inside_the_bound():
    """Every (size, target kind / beta / class count, weights) case of the GPU tests and every one-hot probe."""
    worst = {'bce': 0.0, 'smooth_l1': 0.0, 'softmax_ce': 0.0}

    def onehots(n, w):
        for i in ref.probe_indices(n):
            hot = torch.zeros(n)
            hot[i] = 1.0 + float(w[i])
            yield hot
    for n in ref.LOSS_SIZES:
        for kind in ref.BCE_KINDS:
            x, y, w, thr = ref.bce_case(n, kind)
            for ww in [None, w] + list(onehots(n, w)):
                val, mag = ref.bce_sum(x, y, ww, ref.LOSS_AVG, thr)
                worst['bce'] = max(worst['bce'], _ratio(emul_bce(x, y, ww, ref.LOSS_AVG, thr), val, mag, ref.C_BCE))
        for beta in ref.SL1_BETAS:
            p, t, w = ref.smooth_l1_case(n, beta)
            for ww in [None, w] + list(onehots(n, w)):
                val, mag = ref.smooth_l1_sum(p, t, ww, ref.LOSS_AVG, beta)
                worst['smooth_l1'] = max(worst['smooth_l1'],
                                         _ratio(emul_smooth_l1(p, t, ww, ref.LOSS_AVG, beta), val, mag, ref.C_SL1))
        for C in ref.CE_CLASSES:
            z, lab, w = ref.softmax_ce_case(n, C)
            assert ref.softmax_ce_conditioning(z, lab) <= 1.0
            for ww in [None, w] + list(onehots(n, w)):
                val, mag = ref.softmax_ce_sum(z, lab, ww, ref.LOSS_AVG)
                worst['softmax_ce'] = max(worst['softmax_ce'],
                                          _ratio(emul_softmax_ce(z, lab, ww, ref.LOSS_AVG), val, mag, ref.C_CE))
    for k, v in worst.items():
        _report(k + '_sum', v)


def test_loss_cases_hold_what_they_are_for():
    """The special logits, the three threshold neighbours, the smooth-L1 branch edge on both sides and off the origin,
    the special rows and ignored labels of the cross-entropy are all present at n = 1025, and a probe's own loss is tiny
    where the sum of the others is not."""
    x, y, w, thr = ref.bce_case(1025, 'thr')
    assert {ref.f32(v) for v in ref.BCE_LOGITS} <= set(x.tolist())
    half = np.float32(0.5)
    for v in (half, np.nextafter(half, F32(0)), np.nextafter(half, F32(1))):
        assert int((y == float(v)).sum()) > 50
    val, mag = ref.bce_sum(x, y, torch.eye(1025)[0], 1.0, thr)
    assert 0 < float(mag) < 1e-17 and float(ref.bce_sum(x, y, None, 1.0, thr)[1]) > 100
    for beta in ref.SL1_BETAS:
        p, t, _ = ref.smooth_l1_case(1025, beta)
        b = np.float32(beta)
        dd = (p.double() - t.double()).abs()
        for v in (b, np.nextafter(b, F32(0)), np.nextafter(b, F32(2))):
            assert int(((dd == float(v)) & (t == 0)).sum()) >= 20, (beta, v)
        # off the origin fl(0.75 + d) - 0.75 is d only to an ulp of the sum: on either side of the branch edge
        off = (t == 0.75) & ((dd - float(b)).abs() <= 2.0 ** -23)
        assert int((off & (dd < float(b))).sum()) >= 5 and int((off & (dd >= float(b))).sum()) >= 5, beta
        assert int((dd == 0).sum()) >= 40
    for C in ref.CE_CLASSES:
        z, lab, _ = ref.softmax_ce_case(1025, C)
        assert bool((z.abs().max(dim=1).values == 1e4).any()) and bool(((z.max(1).values - z.min(1).values) == 0).any())
        if C > 1:
            top2 = z.topk(2, dim=1).values
            assert bool(((top2[:, 0] - top2[:, 1]) >= 100).any())


def test_bbox2delta_emulation_stays_inside_the_bound():
    worst = 0.0
    c = torch.tensor([ref.C_BBOX_XY, ref.C_BBOX_XY, ref.C_BBOX_WH, ref.C_BBOX_WH], dtype=F64)
    for n in ref.BBOX_SIZES:
        p, q, _ = ref.bbox_case(n)
        for means, stds in ref.BBOX_CODERS:
            val, mag = ref.bbox2delta(p, q, means, stds)
            got = torch.from_numpy(ref.bbox2delta_f32(p, q, means, stds)).to(F64)
            fin = torch.isfinite(val)
            assert torch.equal(torch.isfinite(got), fin)
            if bool(fin.any()):
                worst = max(worst, float(((got - val).abs() / (c * U * mag + TINY))[fin].max()))
    _report('bbox2delta', worst)


def emul_bn(x, gamma, beta, eps, momentum, rm, rv, res, relu):
    """bn_partial_kernel (fp64 sums of d = x - x[0] and d d: per chunk of ceil(P / 64) rows four row phases, each serial;
    the phases ((0 + 1) + 2) + 3), bn_finalize_kernel (the chunks in order; md = s / P, m = x[0] + md,
    v = max(q / P - md md, 0); running estimates in fp32), bn_apply_kernel (fp32, no contraction)."""
    x32 = _np(x)
    P, C = x32.shape
    rows_per = -(-P // ref.BN_CHUNKS)
    steps = -(-rows_per // 4)
    pad = np.zeros((ref.BN_CHUNKS, steps * 4, C))
    flat = np.zeros((ref.BN_CHUNKS * rows_per, C))
    flat[:P] = x32.astype(np.float64) - x32[0].astype(np.float64)
    pad[:, :rows_per] = flat.reshape(ref.BN_CHUNKS, rows_per, C)
    pad = pad.reshape(ref.BN_CHUNKS, steps, 4, C)
    s, q = np.zeros((ref.BN_CHUNKS, 4, C)), np.zeros((ref.BN_CHUNKS, 4, C))
    for i in range(steps):
        v = pad[:, i]
        s, q = s + v, q + v * v
    tot = []
    for a in (s, q):
        part = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
        acc = np.zeros(C)
        for k in range(ref.BN_CHUNKS):
            acc = acc + part[k]
        tot.append(acc)
    md = tot[0] / P
    m = x32[0].astype(np.float64) + md
    v = np.maximum(tot[1] / P - md * md, 0.0)
    mean, var = m.astype(F32), v.astype(F32)
    mom = F32(momentum)
    out = dict(mean=mean, var=var)
    if rm is not None:
        out['rm'] = (F32(1) - mom) * _np(rm) + mom * mean
        unb = v * (float(P) / float(P - 1)) if P > 1 else v
        out['rv'] = (F32(1) - mom) * _np(rv) + mom * unb.astype(F32)
    y = (x32 - mean) * (F32(1) / np.sqrt(var + F32(eps))) * _np(gamma) + _np(beta)
    if res is not None:
        y = y + _np(res)
    if relu:
        y = np.maximum(y, F32(0))
    assert y.dtype == F32
    out['y'] = y
    return out


@pytest.mark.parametrize('P,C', ref.BN_SHAPES)
def test_bn_train_emulation_stays_inside_the_bound(P, C):
    """Every (shape, mean / std) case of the GPU test, plain and with residual + ReLU + running statistics.  At
    mean / std 1e4 and 1e5 only y and the mean are held; the variance ratio of the raw-moment formula is printed."""
    worst = {}
    for ratio in ref.BN_RATIOS + ref.BN_FAR_RATIOS:
        k = ref.bn_case(P, C, ratio)
        far = ratio in ref.BN_FAR_RATIOS
        for full in (False, True):
            rm, rv, res = (k['rm'], k['rv'], k['res']) if full else (None, None, None)
            r = ref.bn_train(k['x'], k['gamma'], k['beta'], ref.BN_EPS, ref.BN_MOMENTUM, rm, rv, res, full)
            got = emul_bn(k['x'], k['gamma'], k['beta'], ref.BN_EPS, ref.BN_MOMENTUM, rm, rv, res, full)
            for name, v in ref.bn_ratios(got, r, with_var=not far).items():
                key = f'{name} at mean/std {ratio:g}' if far else name
                worst[key] = max(worst.get(key, 0.0), v)
    for name, v in sorted(worst.items()):
        if 'not asserted' in name:
            print(f'[train-emul] bn_train {(P, C)} {name}: worst |err| / bound = {v:.4f}')
        else:
            _report(f'bn_train {(P, C)} {name}', v)


def emul_adagrad(p, g, st, lr, wd, eps, fused):
    """adagrad_kernel in fp32; csrc/train_bwd.hip allows contraction: ``fused`` forms g + wd p and state + g' g' with one
    rounding each (the exact product and sum in fp64, rounded to fp32)."""
    p32, g32, s32 = _np(p), _np(g), _np(st)
    lr, wd, eps = F32(lr), F32(wd), F32(eps)
    with np.errstate(under='ignore'):
        if fused:
            gv = (g32.astype(np.float64) + float(wd) * p32.astype(np.float64)).astype(F32)
            s2 = (s32.astype(np.float64) + gv.astype(np.float64) ** 2).astype(F32)
        else:
            gv = g32 + wd * p32
            s2 = s32 + gv * gv
        p2 = p32 - lr * gv / (np.sqrt(s2) + eps)
    assert s2.dtype == F32 and p2.dtype == F32
    return torch.from_numpy(p2), torch.from_numpy(s2)


@pytest.mark.parametrize('fused', [False, True])
def test_adagrad_emulation_stays_inside_the_bound(fused):
    """Every (size, (wd, lr), fresh / warm) case of the GPU test, three consecutive steps, each against the reference
    started from the emulation's own previous p and state; then the multi-tensor list."""
    ws = wp = 0.0
    cases = [(n, wd, lr, warm) for n in ref.ADAGRAD_SIZES for wd, lr in ref.ADAGRAD_PAIRS for warm in (False, True)]
    cases += [(n, 1e-5, lr, True) for n, lr in zip(ref.ADAGRAD_MULTI_SIZES, ref.ADAGRAD_MULTI_LRS)]
    for n, wd, lr, warm in cases:
        p, g, st, kind = ref.adagrad_case(n, wd, warm)
        for step in range(3 if n < 10 ** 6 else 1):
            r = ref.adagrad(p, g, st, lr, wd, ref.ADAGRAD_EPS)
            p2, s2 = emul_adagrad(p, g, st, lr, wd, ref.ADAGRAD_EPS, fused)
            ws = max(ws, _ratio(s2, r['state'], r['state_mag'], ref.C_ADA_STATE))
            wp = max(wp, _ratio(p2, r['p'], r['p_mag'], ref.C_ADA_P))
            if step == 0 and not warm:
                still = (kind == 3) & ((p == 0) | (ref.f32(wd) == 0))
                assert torch.equal(p2[still].view(torch.int32), p[still].view(torch.int32))
                assert bool((s2[still].view(torch.int32) == 0).all())
            p, st = p2, s2
    _report(f'adagrad state fused={fused}', ws)
    _report(f'adagrad p fused={fused}', wp)
