"""No GPU: (1) the float64 closed forms of tests/_optim_ref.py against torch.optim.Adam / SGD / Adagrad and
``clip_grad_norm_`` run in float64; (2) an fp32 numpy emulation of each kernel of csrc/optim.hip, operation by operation
with contraction off, held to the bound of tests/test_hip_optim.py on every case of that test - the counted ``c`` is
sufficient; (3) the torch.optim state-dict layouts ``fgn_amd.train`` writes and parses, against real torch optimizers;
(4) ``scheduled_lr``."""
import numpy as np
import pytest
import torch

import _optim_ref as ref

F64 = torch.float64


def _torch_run(make_opt, p, g, preset, read, ref_step, steps=3):
    q = torch.nn.Parameter(p.to(F64).clone())
    opt = make_opt(q)
    preset(opt, q)
    for t in range(1, steps + 1):
        q.grad = g.to(F64).clone()
        # every step against the closed form started from torch's own previous parameters and state (created lazily:
        # zeros before the first step), so the roundoff of earlier steps does not compound into the comparison
        before = [s.clone() for s in read(opt, q)] if opt.state[q] else None
        p_before = q.detach().clone()
        opt.step()
        (want_p, p_mag), want_states = ref_step(t, p_before, before)
        # float64 roundoff of the element's own term magnitudes (torch forms exp_avg with lerp_, another order of the
        # same sum: a cancelling element agrees to its terms' roundoff, not to its own)
        assert bool(((want_p - q.detach()).abs() <= 64 * 2.0 ** -53 * p_mag + 1e-300).all())
        for (w, mag), s in zip(want_states, read(opt, q)):
            assert bool(((w - s).abs() <= 64 * 2.0 ** -53 * mag + 1e-300).all())


@pytest.mark.parametrize('wd,lr', ref.PAIRS)
def test_adam_matches_torch_float64(wd, lr):
    """Fresh state, three steps (t = 1, 2, 3), torch given the fp32-rounded scalars the closed form works on."""
    p, g, _, _, _ = ref.optim_case(4097, wd, False)
    b = tuple(ref.f32(x) for x in ref.ADAM_BETAS)
    z = torch.zeros(4097, dtype=F64)

    def step(t, p_, st):
        m_, v_ = st or (z, z)
        r = ref.adam(p_, g, m_, v_, t, lr, wd)
        return (r['p'], r['p_mag']), [(r['m'], r['m_mag']), (r['v'], r['v_mag'])]
    _torch_run(lambda q: torch.optim.Adam([q], lr=ref.f32(lr), betas=b, eps=ref.f32(ref.ADAM_EPS), weight_decay=ref.f32(wd)),
               p, g, lambda o, q: None, lambda o, q: [o.state[q]['exp_avg'], o.state[q]['exp_avg_sq']], step)


@pytest.mark.parametrize('nesterov,mu', [(True, 0.9), (False, 0.9), (False, 0.0)])
@pytest.mark.parametrize('wd,lr', ref.PAIRS)
def test_sgd_matches_torch_float64(wd, lr, nesterov, mu):
    p, g, _, _, _ = ref.optim_case(4097, wd, False)
    z = torch.zeros(4097, dtype=F64)

    def step(t, p_, st):
        r = ref.sgd(p_, g, (st[0] if st else z) if mu else None, lr, wd, mu, nesterov)
        return (r['p'], r['p_mag']), ([(r['buf'], r['buf_mag'])] if mu else [])
    _torch_run(lambda q: torch.optim.SGD([q], lr=ref.f32(lr), momentum=ref.f32(mu), nesterov=nesterov,
                                         weight_decay=ref.f32(wd)),
               p, g, lambda o, q: None, lambda o, q: ([o.state[q]['momentum_buffer']] if mu else []), step)


@pytest.mark.parametrize('wd,lr', ref.PAIRS)
def test_adagrad_with_multiplier_matches_torch_float64(wd, lr):
    """The multiplied gradient: torch steps on g * gmul."""
    p, g, st, _ = ref.adagrad_case(4097, wd, True)
    gmul = float(np.float32(0.37)) * float(np.float32(4.0 / 3.0))

    def step(t, p_, s_):
        r = ref.adagrad(p_, g, s_[0], lr, wd, gmul=gmul)
        return (r['p'], r['p_mag']), [(r['state'], r['state_mag'])]
    _torch_run(lambda q: torch.optim.Adagrad([q], lr=ref.f32(lr), weight_decay=ref.f32(wd), eps=ref.f32(ref.ADAGRAD_EPS)),
               p, (g.to(F64) * gmul), lambda o, q: o.state[q]['sum'].copy_(st.to(F64)), lambda o, q: [o.state[q]['sum']], step)
    # and Adam / SGD take the multiplier the same way
    r1 = ref.adam(p, g, st, st, 2, lr, wd, gmul=gmul)
    r2 = ref.adam(p, g.to(F64) * gmul, st, st, 2, lr, wd)
    assert torch.equal(r1['p'], r2['p']) and torch.equal(r1['p_mag'], r2['p_mag'])
    r1 = ref.sgd(p, g, st, lr, wd, 0.9, True, gmul=gmul)
    r2 = ref.sgd(p, g.to(F64) * gmul, st, lr, wd, 0.9, True)
    assert torch.equal(r1['p'], r2['p'])


def _grad_list(sizes, scale, seed=0):
    g_ = torch.Generator().manual_seed(4400 + seed)
    return [(torch.randn(n, generator=g_) * scale).contiguous() for n in sizes]


@pytest.mark.parametrize('max_norm', [0.5, 1e4])
def test_grad_norm_matches_clip_grad_norm_float64(max_norm):
    gs = _grad_list((0, 1, 4096, 4097, 5), 0.1)
    ps = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=F64)) for g in gs]
    for q, g in zip(ps, gs):
        q.grad = g.to(F64).clone()
    total = torch.nn.utils.clip_grad_norm_(ps, ref.f32(max_norm), norm_type=2)
    norm, coef = ref.grad_norm(gs, max_norm)
    assert norm == pytest.approx(float(total), rel=1e-12)
    for q, g in zip(ps, gs):
        assert torch.allclose(q.grad, g.to(F64) * coef, rtol=1e-9, atol=0)     # (torch adds a float64 1e-6, not the fp32 one)
    assert (coef == 1.0) == (max_norm > norm)
    assert ref.grad_norm([torch.zeros(7)], 1.0) == (0.0, 1.0) and ref.grad_norm([], 1.0) == (0.0, 1.0)


def test_accumulate_closed_form():
    g = torch.randn(100)
    a1, m1 = ref.accumulate(torch.full((100,), float('nan')), g, 0.25, True)
    assert torch.equal(a1, 0.25 * g.to(F64)) and torch.equal(m1, a1.abs())
    a2, m2 = ref.accumulate(a1.float(), g, 0.25, False)
    assert torch.equal(a2, 0.5 * g.to(F64)) and torch.equal(m2, 0.5 * g.to(F64).abs())


# ------------------------------------------------------------------------------------------ emulation inside the bound
def _emul_step(rule, opts, p, g, states, t, lr, wd, coef, scale):
    return ref.emulate(rule, opts, p, g, states, t, lr, wd, coef, scale)


@pytest.mark.parametrize('rule_opts', ref.RULES, ids=ref.rule_id)
def test_update_emulation_stays_inside_the_bound(rule_opts):
    """Every (size, (wd, lr), fresh / warm) case of tests/test_hip_optim.py, three steps each; the multiplier cases; Adam
    at t = 1000."""
    rule, opts = rule_opts
    for n in ref.SIZES:
        for wd, lr in ref.PAIRS:
            for warm in (False, True):
                ref.check_steps(f'emul {ref.rule_id(rule_opts)} n={n} wd={wd:g} lr={lr:g} warm={warm}', _emul_step, rule, opts,
                                n, wd, lr, warm)
    for coef, scale in ref.MULTIPLIERS:
        for warm in (False, True):
            ref.check_steps(f'emul {ref.rule_id(rule_opts)} coef={coef} scale={scale:g} warm={warm}', _emul_step, rule, opts,
                            4097, 1e-5, 0.005, warm, coef=coef, scale=scale)
    if rule == 'Adam':
        ref.check_steps('emul Adam t=1000', _emul_step, rule, opts, 4097, 1e-5, 0.005, True, t0=1000, steps=1)


def test_grad_norm_emulation_stays_inside_the_bound():
    for seed, (sizes, scale, max_norm) in enumerate([((0, 1, 4096, 4097, 5), 0.1, 0.5), ((0, 1, 4096, 4097, 5), 0.1, 1e4),
                                                     ((255,), 1e-3, 1.0), ((4096 * 3 + 1,), 30.0, 35.0), ((7,), 0.0, 1.0)]):
        gs = _grad_list(sizes, scale, seed)
        norm, coef = ref.grad_norm(gs, max_norm)
        n32, c32 = ref.emul_grad_norm(gs, max_norm)
        assert abs(float(n32) - norm) <= ref.C_NORM * ref.U * norm + ref.TINY
        assert abs(float(c32) - coef) <= ref.C_COEF * ref.U * coef
        if norm < max_norm * (1 - 1e-6):
            assert float(c32) == 1.0


def test_accumulate_emulation_stays_inside_the_bound():
    g = ref.adagrad_case(4097, 1e-5, True)[1]
    acc = torch.full((4097,), float('nan'))
    for i in range(4):
        want, mag = ref.accumulate(acc, g, 0.25, i == 0)
        acc = torch.from_numpy(ref.emul_accumulate(acc, g, 0.25, i == 0))
        assert ref.worst_ratio(acc, want, mag, ref.C_ACC) <= 1.0
    exact = (0.75 * g.to(F64)).float().to(F64) == 0.75 * g.to(F64)
    assert int(exact.sum()) > 100 and torch.equal(acc[exact], g[exact])


# ------------------------------------------------------------------------------------------ state-dict layouts
ORDER = [('backbone.conv1.weight', (4, 3)), ('backbone.bn1.weight', (4,)), ('rpn_head.rpn_conv.weight', (5, 4)),
         ('rpn_head.rpn_conv.bias', (5,)), ('roi_head.bbox_head.fc_cls.weight', (2, 5)), ('backbone.layer4.0.conv1.weight', (3,))]
TRAINED = ['rpn_head.rpn_conv.weight', 'rpn_head.rpn_conv.bias', 'roi_head.bbox_head.fc_cls.weight']


def _torch_opt(kind, cfg, params):
    groups = [{'params': [q]} for q in params]
    if kind == 'Adam':
        return torch.optim.Adam(groups, lr=cfg['lr'], betas=cfg['betas'], eps=cfg['eps'], weight_decay=cfg['weight_decay'])
    return torch.optim.SGD(groups, lr=cfg['lr'], momentum=cfg['momentum'], nesterov=cfg['nesterov'],
                           weight_decay=cfg['weight_decay'])


def _params():
    g_ = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(shape, generator=g_)) for _, shape in ORDER]
    for (k, _), q in zip(ORDER, ps):
        q.requires_grad_(k in TRAINED)
    return ps


@pytest.mark.parametrize('kind', ['Adam', 'SGD'])
def test_written_layout_loads_into_a_real_torch_optimizer_and_parses_back(kind):
    from fgn_amd import train as T
    cfg = T.optimizer_config(kind, lr=0.01, weight_decay=5e-5, roi_head_lr_mult=0.1)
    g_ = torch.Generator().manual_seed(6)
    keys = {'Adam': ('exp_avg', 'exp_avg_sq'), 'SGD': ('momentum_buffer',)}[kind]
    shapes = dict(ORDER)
    trained = {k: {key: torch.rand(shapes[k], generator=g_) for key in keys} for k in TRAINED}
    sd = T.build_optimizer_state_dict(cfg, ORDER, trained, lr=0.001, base_lr=0.01, n_steps=2)
    # groups for ALL parameters, state for the trained ones alone
    assert len(sd['param_groups']) == len(ORDER) and sorted(sd['state']) == [2, 3, 4]
    ps = _params()
    opt = _torch_opt(kind, cfg, ps)
    assert set(sd['param_groups'][0]) - {'initial_lr'} == set(opt.state_dict()['param_groups'][0])
    opt.load_state_dict({k: v for k, v in sd.items()})
    for i, (k, _) in enumerate(ORDER):
        if k in TRAINED:
            for key in keys:
                assert torch.equal(opt.state[ps[i]][key], trained[k][key])
            if kind == 'Adam':
                assert float(opt.state[ps[i]]['step']) == 2.0 and opt.state[ps[i]]['step'].dtype == torch.float32
        else:
            assert len(opt.state[ps[i]]) == 0
    assert opt.param_groups[4]['lr'] == pytest.approx(0.0001) and opt.param_groups[4]['initial_lr'] == pytest.approx(0.001)
    assert opt.param_groups[2]['lr'] == pytest.approx(0.001) and opt.param_groups[0]['lr'] == pytest.approx(0.001)
    parsed = T.parse_optimizer_state_dict(sd, [k for k, _ in ORDER], TRAINED, expect=kind)
    assert parsed['type'] == kind and sorted(parsed['states']) == sorted(TRAINED)
    assert parsed['step'] == (2 if kind == 'Adam' else None)
    for k in TRAINED:
        for key in keys:
            assert torch.equal(parsed['states'][k][key], trained[k][key])
    assert parsed['group']['lr'] == pytest.approx(0.001) and parsed['group']['initial_lr'] == pytest.approx(0.01)
    # before the first step: no state at all, recognised from the group keys
    sd0 = T.build_optimizer_state_dict(cfg, ORDER, trained, lr=0.01, base_lr=0.01, n_steps=0)
    assert sd0['state'] == {} and T.optimizer_kind(sd0) == kind
    opt.load_state_dict(sd0)


@pytest.mark.parametrize('kind', ['Adam', 'SGD'])
def test_state_of_a_real_torch_optimizer_parses_back(kind):
    """A real optimizer, one group per parameter over ALL parameters (mmcv's constructor), two CPU steps: its
    state_dict() - written by torch, no ``param_names`` - parses back to the same tensors; frozen parameters carry no
    state entry."""
    from fgn_amd import train as T
    cfg = T.optimizer_config(kind, lr=0.01, weight_decay=5e-5)
    ps = _params()
    opt = _torch_opt(kind, cfg, ps)
    g_ = torch.Generator().manual_seed(8)
    for _ in range(2):
        for q in ps:
            q.grad = torch.randn(q.shape, generator=g_) if q.requires_grad else None
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd['state']) == [2, 3, 4]
    parsed = T.parse_optimizer_state_dict(sd, [k for k, _ in ORDER], TRAINED, expect=kind)
    assert parsed['type'] == kind and parsed['step'] == (2 if kind == 'Adam' else None)
    for i, (k, _) in enumerate(ORDER):
        if k in TRAINED:
            for key in ({'Adam': ('exp_avg', 'exp_avg_sq'), 'SGD': ('momentum_buffer',)}[kind]):
                assert torch.equal(parsed['states'][k][key], opt.state[ps[i]][key])
        else:
            assert k not in parsed['states']
    other = 'SGD' if kind == 'Adam' else 'Adam'
    with pytest.raises(ValueError, match=f'{kind}.*{other}'):
        T.parse_optimizer_state_dict(sd, [k for k, _ in ORDER], TRAINED, expect=other)
    with pytest.raises(ValueError, match='Adagrad'):
        T.parse_optimizer_state_dict(sd, [k for k, _ in ORDER], TRAINED, expect='Adagrad')


def test_optimizer_kind_from_state_and_group_keys():
    from fgn_amd import train as T
    ps = _params()
    ada = torch.optim.Adagrad([{'params': [q]} for q in ps], lr=0.01).state_dict()
    assert T.optimizer_kind(ada) == 'Adagrad'
    ada['state'] = {}
    assert T.optimizer_kind(ada) == 'Adagrad'                          # lr_decay in the groups
    assert T.optimizer_kind(torch.optim.Adam(ps).state_dict()) == 'Adam'
    assert T.optimizer_kind(torch.optim.SGD(ps, lr=0.1).state_dict()) == 'SGD'
    with pytest.raises(ValueError):
        T.optimizer_kind({'state': {}, 'param_groups': [{'lr': 0.1, 'params': [0]}]})


def test_optimizer_config_reads_the_schedule_files_dict():
    from fgn_amd import train as T
    c = T.optimizer_config(dict(type='SGD', momentum=0.9, nesterov=True, lr=0.005, weight_decay=1e-5,
                                paramwise_cfg=dict(custom_keys={'roi_head': dict(lr_mult=0.1, decay_mult=1.0)})))
    assert (c['type'], c['momentum'], c['nesterov'], c['lr'], c['weight_decay'], c['lr_mult']) == ('SGD', 0.9, True, 0.005, 1e-5, 0.1)
    c = T.optimizer_config(dict(type='Adam', lr=0.01, weight_decay=5e-5))
    assert c['betas'] == (0.9, 0.999) and c['eps'] == 1e-8 and c['lr_mult'] == 1.0
    assert T.optimizer_config('Adagrad')['eps'] == 1e-10 and T.optimizer_config('Adam')['eps'] == 1e-8
    assert T.optimizer_config('SGD')['nesterov'] is True
    with pytest.raises(ValueError):
        T.optimizer_config(dict(type='SGD', momentum=0.9, dampening=0.1))
    with pytest.raises(NotImplementedError):
        T.optimizer_config(dict(type='Adam', amsgrad=True))
    with pytest.raises(ValueError):
        T.optimizer_config('AdamW')


# ------------------------------------------------------------------------------------------ schedules
STEP_CFG = dict(policy='Step', step=[3], gamma=0.1, min_lr=0.000001, by_epoch=True, warmup='linear', warmup_iters=100,
                warmup_ratio=0.01)


def test_scheduled_lr():
    from fgn_amd.train import scheduled_lr, step_lr
    for it in (0, 1, 50, 99, 100, 5000):
        for epoch in (0, 1, 2, 3, 4, 7):
            assert scheduled_lr(STEP_CFG, 0.005, it, epoch, 8) == step_lr(0.005, it, epoch)
            assert scheduled_lr(dict(policy='Fixed'), 0.005, it, epoch, 8) == 0.005
    cos = dict(policy='CosineAnnealing', min_lr_ratio=0.01)
    assert scheduled_lr(cos, 0.01, 1000, 0, 12) == pytest.approx(0.01, rel=1e-15)
    assert scheduled_lr(cos, 0.01, 1000, 12, 12) == pytest.approx(0.0001, rel=1e-12)
    assert scheduled_lr(cos, 0.01, 1000, 6, 12) == pytest.approx(0.5 * (0.01 + 0.0001), rel=1e-12)
    assert scheduled_lr(dict(policy='CosineAnnealing', min_lr=0.002), 0.01, 1000, 12, 12) == pytest.approx(0.002, rel=1e-12)
    lrs = [scheduled_lr(cos, 0.01, 1000, e, 12) for e in range(13)]
    assert all(a > b for a, b in zip(lrs, lrs[1:]))
    # linear warm-up multiplies the regular lr as in step_lr
    warm = dict(warmup='linear', warmup_iters=100, warmup_ratio=0.01)
    for it in (0, 37, 99):
        k = step_lr(1.0, it, 0) / 1.0
        assert scheduled_lr(dict(cos, **warm), 0.01, it, 3, 12) == pytest.approx(k * scheduled_lr(cos, 0.01, it, 3, 12), rel=1e-15)
        assert scheduled_lr(dict(policy='Fixed', **warm), 0.01, it, 3, 12) == pytest.approx(k * 0.01, rel=1e-15)
    assert scheduled_lr(dict(policy='Fixed', **warm), 0.01, 100, 3, 12) == 0.01
    with pytest.raises(NotImplementedError):
        scheduled_lr(dict(policy='Fixed', warmup='exp', warmup_iters=10), 0.01, 0, 0, 12)
    with pytest.raises(NotImplementedError):
        scheduled_lr(dict(policy='Poly'), 0.01, 0, 0, 12)
    with pytest.raises(ValueError):
        scheduled_lr(dict(policy='CosineAnnealing'), 0.01, 0, 0, 12)
