"""``Trainer`` with Adam / SGD, gradient clipping and accumulation (fgn_amd/train.py over csrc/optim.hip) on the tiny
configuration the other trainer tests use.  The optimiser is isolated from the convolution noise of the step: the
weights, the optimizer state and ``tr.grads`` are read back around ``apply_gradients()`` and every element of the update
is held to the float64 closed forms of tests/_optim_ref.py under the bound of tests/test_hip_optim.py,
``|got - ref| <= c * 2^-24 * mag + 2^-126`` with the counts derived there."""
import numpy as np
import pytest
import torch

import _optim_ref as ref

pytestmark = pytest.mark.gpu

F64 = torch.float64
SGD_N = dict(momentum=0.9, nesterov=True)


def _model(seed=0):
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(3, 2, width_div=2)
    sd = init_state_dict(cfg, seed)
    g = torch.Generator().manual_seed(99)
    for k in sd:                     # non-trivial BatchNorm parameters of the shared head, as tests/test_hip_train.py sets
        if k.startswith('roi_head.shared_head') and k.endswith('.weight') and sd[k].dim() == 1:
            sd[k] = 0.75 + 0.5 * torch.rand(sd[k].shape, generator=g)
        if k.startswith('roi_head.shared_head') and k.endswith('.bias') and sd[k].dim() == 1:
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    return FGN(cfg['n_ways'], cfg['k_shots'], backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=sd)


@pytest.fixture(scope='module')
def batch():
    from fgn_amd.episodes import make_batch
    return make_batch(2, 1, 3, 2, 160, 224, 64)


def _f(v):
    v = v[0] if isinstance(v, list) else v
    return float(v.detach().reshape(-1)[0]) if isinstance(v, torch.Tensor) else float(v)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _cpu(d_):
    return {k: v.detach().cpu().clone().reshape(-1) for k, v in d_.items()}


def _states(tr, snap):
    """name -> list of state tensors in the order of ``ref.reference``."""
    if tr.optimizer == 'Adam':
        return {k: [snap['state'][k], snap['state2'][k]] for k in tr.W}
    return {k: ([snap['state'][k]] if snap['state'] else []) for k in tr.W}


def _snapshot(tr):
    return dict(W=_cpu(tr.W), state=_cpu(tr.state), state2=_cpu(tr.state2))


def _rule(tr):
    return tr.optimizer, (dict(momentum=tr.opt['momentum'], nesterov=tr.opt['nesterov']) if tr.optimizer == 'SGD' else {})


def _check_update(tag, tr, before, after, grads, t, gmul=1.0, lr_of=None):
    """Every tensor of the heads: ``after`` is one reference update of ``before`` by ``grads`` (CPU copies) -> worst ratio."""
    rule, opts = _rule(tr)
    sb, sa = _states(tr, before), _states(tr, after)
    worst = 0.0
    for k in tr.W:
        lr = tr.lr * (tr.mult if k.startswith('roi_head') else 1.0) if lr_of is None else lr_of(k)
        pr, pmag, cp, sts = ref.reference(rule, opts, before['W'][k], grads[k], sb[k], t, lr, tr.wd, gmul)
        worst = max(worst, ref.worst_ratio(after['W'][k], pr, pmag, cp))
        for (sr, smag, cs), s2 in zip(sts, sa[k]):
            worst = max(worst, ref.worst_ratio(s2, sr, smag, cs))
    print(f'[optim-bound] trainer {tag}: worst |err| / bound over {len(tr.W)} tensors = {worst:.4f}')
    return worst


@pytest.mark.parametrize('optimizer', ['Adam', dict(type='SGD', momentum=0.9, nesterov=True, lr=0.005, weight_decay=1e-5,
                                                    paramwise_cfg=dict(custom_keys={'roi_head': dict(lr_mult=0.1)}))],
                         ids=['Adam', 'SGD-nesterov-dict'])
def test_two_steps_are_the_reference_update_of_the_recorded_gradients(optimizer, batch):
    """Adam (by name) and SGD-Nesterov (the schedule file's dict), two steps each; lr_mult 0.1 under roi_head visibly
    applied: the reference at the full learning rate misses the bound on the roi_head tensors."""
    from fgn_amd.train import Trainer
    tr = Trainer(_model(), optimizer=optimizer)
    assert tr.mult == 0.1 and tr.n_steps == 0
    for it in range(2):
        torch.manual_seed(it)
        losses = tr.forward_backward(batch)
        before, grads = _snapshot(tr), _cpu(tr.grads)
        assert tr.apply_gradients() == {} and 'grad_norm' not in losses
        after = _snapshot(tr)
        assert tr.n_steps == it + 1
        assert _check_update(f'{tr.optimizer} step {it + 1}', tr, before, after, grads, it + 1) <= 1.0
        assert _check_update(f'{tr.optimizer} step {it + 1} WITHOUT lr_mult (must miss)', tr, before, after, grads, it + 1,
                             lr_of=lambda k: tr.lr) > 1.0
        moved = [k for k in tr.W if not torch.equal(before['W'][k], after['W'][k])]
        assert any(k.startswith('roi_head') for k in moved) and any(k.startswith('rpn_head') for k in moved)


@pytest.mark.parametrize('optimizer', ['Adagrad', 'Adam'])
@pytest.mark.parametrize('above', [False, True], ids=['norm-above-max', 'norm-below-max'])
def test_clipping(optimizer, above, batch):
    """max_norm at half / twice the measured norm: ``grad_norm`` of the losses is the fp64 norm of ``tr.grads`` (c = 2),
    the update is that of the gradient scaled by the coefficient the kernel formed from ITS norm (min(1, max_norm /
    (norm + 1e-6)) in fp32, within c = 4 of the fp64 coefficient; exactly 1 above).  The default optimiser clips too."""
    from fgn_amd.train import Trainer
    tr = Trainer(_model(), optimizer=optimizer, grad_clip=dict(max_norm=1.0, norm_type=2))
    torch.manual_seed(0)
    tr.forward_backward(batch)
    grads = _cpu(tr.grads)
    norm, _ = ref.grad_norm(list(grads.values()), 1.0)
    assert norm > 1e-3
    tr.grad_clip['max_norm'] = max_norm = float(np.float32(norm * (2.0 if above else 0.5)))
    _, coef = ref.grad_norm(list(grads.values()), max_norm)
    before = _snapshot(tr)
    out = tr.apply_gradients()
    after = _snapshot(tr)
    gn = out['grad_norm']
    assert gn.is_cuda and gn.dim() == 0
    got = float(gn)
    F = np.float32
    c32 = F(max_norm) / (F(got) + F(1e-6))
    c32 = F(1.0) if c32 > 1 else c32
    print(f'[optim-bound] trainer clip {optimizer}: grad_norm {got!r} (fp64 {norm!r}), coef {float(c32)!r} (fp64 {coef!r})')
    assert abs(got - norm) <= ref.C_NORM * ref.U * norm + ref.TINY
    assert abs(float(c32) - coef) <= ref.C_COEF * ref.U * coef
    assert (float(c32) == 1.0) == above
    assert _check_update(f'clip {optimizer} above={above}', tr, before, after, grads, 1, gmul=float(c32)) <= 1.0
    torch.manual_seed(1)
    assert 'grad_norm' in tr.step(batch) and tr.n_steps == 2


def test_norm_types_other_than_2_are_refused():
    from fgn_amd.train import Trainer
    with pytest.raises(NotImplementedError):
        Trainer(_model(), grad_clip=dict(max_norm=1.0, norm_type=1))
    with pytest.raises(ValueError):
        Trainer(_model(), optimizer=dict(type='SGD', momentum=0.9, dampening=0.5))


def _packed(m):
    out = {}
    for k, v in m._P.items():
        for i, l in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            t = l if torch.is_tensor(l) else getattr(l, 'w', None)
            if torch.is_tensor(t):
                out[f'{k}.{i}'] = t.detach().cpu().clone()
    for b, blk in enumerate(m._PT['shared']):
        for name in ('conv1', 'conv2', 'conv3'):
            out[f'shared.{b}.{name}'] = getattr(blk, name).w.detach().cpu().clone()
    return out


def test_accumulation_and_flush(batch):
    """cumulative_iters = 2.  Micro-step 1 leaves W, the packed layers and n_steps as they were and moves the running
    statistics; micro-step 2 updates from the accumulators, which hold g1 / 2 + g2 / 2 (c = 2 per accumulation), by
    the reference rule.  flush() after one pending micro-step applies that gradient at full weight (multiplier 2 on
    g / 2); a second flush() does nothing."""
    from fgn_amd.train import Trainer
    m = _model()
    tr = Trainer(m, optimizer='Adam', cumulative_iters=2)
    w0, packed0 = _snapshot(tr), _packed(m)
    buf0 = {k: v.detach().cpu().clone() for k, v in tr.buffers.items()}
    calls0 = tr._bn_calls
    torch.manual_seed(0)
    losses = tr.step(batch)
    g1 = _cpu(tr.grads)
    assert 'loss_cls' in losses and tr.n_steps == 0 and tr._bn_calls > calls0
    for k in tr.W:
        assert torch.equal(_bits(tr.W[k]).reshape(-1), _bits(w0['W'][k])), k
    for k, v in _packed(m).items():
        assert torch.equal(_bits(v), _bits(packed0[k])), k
    assert any(not torch.equal(tr.buffers[k].cpu(), buf0[k]) for k in buf0)
    assert m._shared_dirty is not None
    acc1 = _cpu(tr.acc)
    for k in tr.W:
        want, mag = ref.accumulate(None, g1[k], 0.5, True)
        assert ref.worst_ratio(acc1[k], want, mag, ref.C_ACC) <= 1.0
    torch.manual_seed(1)
    before = _snapshot(tr)
    tr.step(batch)
    g2, acc2, after = _cpu(tr.grads), _cpu(tr.acc), _snapshot(tr)
    assert tr.n_steps == 1
    for k in tr.W:
        want, mag = ref.accumulate(acc1[k], g2[k], 0.5, False)
        assert ref.worst_ratio(acc2[k], want, mag, ref.C_ACC) <= 1.0
        mean = 0.5 * (g1[k].to(F64) + g2[k].to(F64))
        assert bool(((acc2[k].to(F64) - mean).abs() <= 2 * ref.C_ACC * ref.U * 0.5 * (g1[k].abs() + g2[k].abs()).to(F64) + ref.TINY).all())
    assert _check_update('accumulated Adam step', tr, before, after, acc2, 1) <= 1.0
    assert any(not torch.equal(v, packed0[k]) for k, v in _packed(m).items())
    # a pending micro-step, then flush(): the gradient at full weight
    torch.manual_seed(2)
    tr.step(batch)
    assert tr.n_steps == 1 and tr._pending == 1
    acc3, before = _cpu(tr.acc), _snapshot(tr)
    assert tr.flush() == {}
    after = _snapshot(tr)
    assert tr.n_steps == 2 and tr._pending == 0
    assert _check_update('flush of 1 of 2', tr, before, after, acc3, 2, gmul=2.0) <= 1.0
    assert tr.flush() == {} and tr.n_steps == 2
    for k in tr.W:
        assert torch.equal(_bits(tr.W[k]).reshape(-1), _bits(after['W'][k]))


@pytest.mark.parametrize('optimizer', ['Adam', 'SGD'])
def test_checkpoint_resume_continues_the_run(optimizer, batch):
    """Two steps, checkpoint, a fresh Trainer resumed from it: the third step gives the same losses and weights (the
    tolerances of tests/test_hip_train.py::test_checkpoint_resume_continues_the_run).  The checkpoint's ``optimizer``
    entry loads into a real torch optimizer built over all parameters; resuming it into an Adagrad trainer raises."""
    from fgn_amd.train import Trainer, reference_param_order
    t1 = Trainer(_model(), optimizer=optimizer)
    for it in range(2):
        torch.manual_seed(it)
        t1.step(batch)
    ck = t1.checkpoint(meta={'iter': 2})
    torch.manual_seed(2)
    l1 = t1.step(batch)
    t2 = Trainer(_model(), optimizer=optimizer)
    t2.resume(ck)
    assert t2.n_steps == 2
    torch.manual_seed(2)
    l2 = t2.step(batch)
    for k in l1:
        assert _f(l1[k]) == pytest.approx(_f(l2[k]), rel=1e-5, abs=1e-7), k
    for k in t1.W:
        d = float((t1.W[k] - t2.W[k]).abs().max())
        assert d <= 1e-5 * max(1.0, float(t1.W[k].abs().max())), (k, d)
    # a real torch optimizer over ALL parameters of the reference model, one group each (mmcv's constructor)
    order = reference_param_order(t1.model._sd, t1.model.cfg['backbone'])
    params = [torch.nn.Parameter(torch.zeros(shape)) for _, shape in order]
    groups = [{'params': [q]} for q in params]
    opt = torch.optim.Adam(groups, lr=0.1) if optimizer == 'Adam' else torch.optim.SGD(groups, lr=0.1, momentum=0.9, nesterov=True)
    opt.load_state_dict(ck['optimizer'])
    n_state = sum(1 for q in params if len(opt.state[q]))
    assert n_state == len(t1.W) and len(ck['optimizer']['param_groups']) == len(order) > n_state
    t3 = Trainer(_model())
    w = {k: v.clone() for k, v in t3.W.items()}
    with pytest.raises(ValueError, match=f'{optimizer}.*Adagrad'):
        t3.resume(ck)
    assert all(torch.equal(w[k], t3.W[k]) for k in w)                 # refused before anything was loaded


def test_default_path_is_bitwise_the_same(batch):
    from fgn_amd.train import Trainer
    t1, t2 = Trainer(_model()), Trainer(_model(), optimizer='Adagrad', grad_clip=None, cumulative_iters=1)
    for t in (t1, t2):
        torch.manual_seed(0)
        t.forward_backward(batch)
    # the same recorded gradients through both: the update itself is compared, not two runs of the convolutions
    t2.grads = {k: v.clone() for k, v in t1.grads.items()}
    t1.apply_gradients(), t2.apply_gradients()
    for k in t1.W:
        assert torch.equal(_bits(t1.W[k]), _bits(t2.W[k])) and torch.equal(_bits(t1.state[k]), _bits(t2.state[k]))
    assert hasattr(t1, '_adagrad_table') and not hasattr(t1, '_optim_table')     # ops.adagrad_multi, nothing new launched
    assert t1.eps == 1e-10 and t1.optimizer == 'Adagrad'


def test_sixty_adam_steps_learn(batch):
    """The wiring learns: 60 Adam steps on one tiny batch bring the summed loss below half its first value."""
    from fgn_amd.train import Trainer
    tr = Trainer(_model(), optimizer='Adam', lr=0.001)
    first = last = None
    for it in range(60):
        torch.manual_seed(it)
        losses = tr.step(batch)
        if it in (0, 59):
            total = sum(_f(v) for k, v in losses.items() if 'loss' in k)
            first, last = (total, last) if it == 0 else (first, total)
    print(f'[optim] 60 Adam steps: summed loss {first:.4f} -> {last:.4f}')
    assert last < 0.5 * first
