"""The optimiser kernels of csrc/optim.hip alone (``ops.optim_multi``, ``ops.grad_norm_multi``,
``ops.grad_accumulate_multi``) against the float64 closed forms of tests/_optim_ref.py, every output element bounded by

    |got - ref| <= c * 2^-24 * mag + 2^-126

``mag`` is the element's own term-magnitude sum, ``c`` the number of fp32 roundings counted in the kernel's arithmetic
(first-order, rounded up; the constants live in tests/_optim_ref.py).  The translation unit is compiled with contraction
off and fp32 division and sqrtf are correctly rounded, so every operation written in ``update_one`` is one rounding.
tests/test_optim_ref_cpu.py holds a numpy emulation of each kernel to the same bounds on the same cases.  Nothing is
normalised by a tensor's range.  Every test prints ``[optim-bound] name: worst |err| / bound`` before it asserts.

The counts (u = 2^-24; the host forms 1 - beta, lr / bc1 and sqrt(bc2) with one rounding each):
  g' = g mul + wd p     mul = coef * scale (1), g mul (1), wd p (1), the sum (1): c_g = 4 on mag_g = |g mul| + |wd p|
  Adam m'               beta1 m (1); 1 - beta1 (1), its product with g' (1), the sum (1) and the error of g' (4) on
                        (1 - beta1) mag_g: c = 7 on |beta1 m| + (1 - beta1) mag_g
  Adam v'               beta2 v (1) and the sum (1); on (1 - beta2) g'^2: the square (1), 1 - beta2 (1), the product
                        (1), the sum (1) = 4; the error of g' enters g'^2 as 2 |g'| c_g u mag_g: 4 on the term
                        (1 - beta2) 2 |g'| mag_g of the magnitude; rounded up: c = 6
  Adam p'               on |step|: s = lr / bc1 (1), s m' (1), the division (1), the subtraction (1), in the denominator
                        sqrtf (1), sqrt(bc2) (1), the division by it (1), + eps (1), and half the relative error of v'
                        from its own roundings (0.5 x 6 = 3) = 11; on s mag_m / den: the error of m' (7); on the
                        through-v' term |step| (1 - beta2) |g'| mag_g / (sqrt(v') sqrt(bc2) den): c_g = 4; on |p|: the
                        subtraction (1); rounded up: c = 12
  SGD buf'              mu buf (1), the sum (1), the error of g' (4) on mag_g: c = 5 on |mu buf| + mag_g
  SGD p'                Nesterov p - lr (g' + mu buf'): mu buf' (1), the sum (1), lr x (1), the subtraction (1) on top
                        of the error of buf' (5) on lr mu mag_buf = 9; rounded up: c = 10 on |p| + lr (mag_g + mu mag_buf);
                        without Nesterov (5 + 2) and without momentum (4 + 2) the same constant is held
  Adagrad state'        as test_adagrad_step_and_multi_bound with c_g = 4: the square and the sum (2) on state + g'^2,
                        4 on 2 |g'| mag_g; rounded up: c = 5
  Adagrad p'            on lr mag_g / den: the error of g' directly (4) and through state' under the root (0.5 x 2 x 4 =
                        4) = 8; on |step|: state's own roundings (1), sqrtf, + eps, lr g', the division, the subtraction
                        (5) = 6; rounded up: c = 9.  Not compared with the contracted kernel of train_bwd.hip.
  norm                  squares and sums in fp64 (2^-53 each), sqrt in fp64, x grad_scale in fp64, one rounding to fp32;
                        rounded up: c = 2.  coef = max_norm / (norm + 1e-6): the error of norm (1), the sum (1), the
                        division (1); rounded up: c = 4, relative to coef
  accumulate            a g (1), the sum (1): c = 2 on |acc| + |a g|
"""
import numpy as np
import pytest
import torch

import _optim_ref as ref

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _states_arg(rule, states):
    if rule == 'Adam':
        return [(states[0], states[1])]
    return [states[0]] if states else None


def _gpu_step(rule, opts, p, g, states, t, lr, wd, coef, scale):
    from fgn_amd import ops
    pd, sd = p.cuda(), [s.cuda() for s in states]
    rec = None if coef is None else torch.tensor([0.0, coef], dtype=torch.float32).cuda()
    ops.optim_multi(rule, [pd], [g.cuda()], _states_arg(rule, sd), [lr], wd, step=t, coef=rec, grad_scale=scale, **opts)
    return pd.cpu(), [s.cpu() for s in sd]


@pytest.mark.parametrize('warm', [False, True], ids=['fresh', 'warm'])
@pytest.mark.parametrize('wd,lr', ref.PAIRS)
@pytest.mark.parametrize('n', ref.SIZES)
@pytest.mark.parametrize('rule_opts', ref.RULES, ids=ref.rule_id)
def test_update_rules_bound(rule_opts, n, wd, lr, warm):
    """``optim_multi_kernel``, each rule: n in {1, 255, 4095, 4096, 4097, 2^20 + 3} (the chunk edge, the float4 path of a
    full chunk and the element path of a tail, many chunks); (wd, lr) of ADAGRAD_PAIRS; the gradient classes of
    ``adagrad_case`` (+-(1e-6 .. 10), g = 0 on zero state, g = -wd p (1 +- 1e-3), g = 1e-25 with p = 0) on a fresh (zero)
    and a warm state; Adam at betas (0.9, 0.999), eps 1e-8, SGD at momentum 0.9 with and without Nesterov and at 0.
    Three steps (t = 1, 2, 3), each against the reference started from the kernel's own previous parameters and state.
    Where g' = 0 on a zero state p keeps its bits and the state stays +0.  Counts: the module docstring."""
    rule, opts = rule_opts
    ref.check_steps(f'{ref.rule_id(rule_opts)} n={n} wd={wd:g} lr={lr:g} {"warm" if warm else "fresh"}', _gpu_step, rule,
                    opts, n, wd, lr, warm)


def test_adam_late_step_bound():
    """t = 1000: bc1 = 1 - 0.9^1000 is 1 to the last bit, bc2 = 0.63."""
    ref.check_steps('Adam t=1000', _gpu_step, 'Adam', {}, 4097, 1e-5, 0.005, True, t0=1000, steps=1)


@pytest.mark.parametrize('coef,scale', ref.MULTIPLIERS)
@pytest.mark.parametrize('rule_opts', ref.RULES, ids=ref.rule_id)
def test_gradient_multiplier_bound(rule_opts, coef, scale):
    """The multiplier: the device coefficient alone, the host scale alone, both (mul = coef * scale is one rounding,
    g * mul a second: the 2 of c_g = 4), fresh and warm."""
    rule, opts = rule_opts
    for warm in (False, True):
        ref.check_steps(f'{ref.rule_id(rule_opts)} coef={coef} scale={scale:g} warm={warm}', _gpu_step, rule, opts, 4097,
                        1e-5, 0.005, warm, coef=coef, scale=scale)


@pytest.mark.parametrize('rule_opts', ref.RULES, ids=ref.rule_id)
def test_unit_multiplier_leaves_the_gradient_bitwise(rule_opts):
    """A null coefficient with scale 1 and a coefficient of exactly 1.0f (a norm below max_norm) give the bits of a
    call whose gradient was multiplied by nothing."""
    from fgn_amd import ops
    rule, opts = rule_opts
    p, g, states, _ = ref.initial_state(rule, opts, 4097, 1e-5, True)
    plain_p, plain_s = _gpu_step(rule, opts, p, g, states, 2, 0.005, 1e-5, None, 1.0)
    rec = ops.grad_norm_multi([g.cuda()], 1e6)
    assert float(rec[1]) == 1.0
    pd, sd = p.cuda(), [s.cuda() for s in states]
    ops.optim_multi(rule, [pd], [g.cuda()], _states_arg(rule, sd), [0.005], 1e-5, step=2, coef=rec, **opts)
    assert torch.equal(_bits(pd), _bits(plain_p))
    for a, b in zip(sd, plain_s):
        assert torch.equal(_bits(a), _bits(b))
    r = ref.reference(rule, opts, p, g, states, 2, 0.005, 1e-5, 1.0)
    assert ref.worst_ratio(plain_p, r[0], r[1], r[2]) <= 1.0


def _list_case(rule, opts, sizes, lrs, wd):
    cases = [ref.initial_state(rule, opts, n, wd, True, seed=i) for i, n in enumerate(sizes)]
    P = [c[0].cuda() for c in cases]
    G = [c[1].cuda() for c in cases]
    S = [[s.cuda() for s in c[2]] for c in cases]
    if rule == 'Adam':
        arg = [tuple(s) for s in S]
    else:
        arg = [s[0] for s in S] if S[0] else None
    return cases, P, G, S, arg


@pytest.mark.parametrize('rule_opts', ref.RULES, ids=ref.rule_id)
def test_update_list_bound_and_one_launch_per_tensor_bitwise(rule_opts):
    """Five tensors of 0, 1, 4096, 4097 and 5 elements with five learning rates in ONE launch, then 70 tensors with empty
    ones among them (more than one 64-slot table: the second launch starts where the first stopped): every tensor is
    updated exactly once - held to the bound of a single update - and equals one launch per tensor bit for bit."""
    from fgn_amd import ops
    rule, opts = rule_opts
    wd, t = 1e-5, 2
    for sizes, lrs in ((ref.ADAGRAD_MULTI_SIZES, ref.ADAGRAD_MULTI_LRS),
                       (ref.MANY_SIZES, tuple(0.001 * (1 + i % 7) for i in range(len(ref.MANY_SIZES))))):
        cases, P, G, S, arg = _list_case(rule, opts, sizes, lrs, wd)
        ops.optim_multi(rule, P, G, arg, list(lrs), wd, step=t, **opts)
        worst = 0.0
        for (p0, g, s0, _), pd, sd, lr in zip(cases, P, S, lrs):
            pr, pmag, cp, sts = ref.reference(rule, opts, p0, g, s0, t, lr, wd, 1.0)
            worst = max(worst, ref.worst_ratio(pd.cpu(), pr, pmag, cp))
            for (sr, smag, cs), s2 in zip(sts, sd):
                worst = max(worst, ref.worst_ratio(s2.cpu(), sr, smag, cs))
            one_p, one_s = _gpu_step(rule, opts, p0, g, s0, t, lr, wd, None, 1.0)
            assert torch.equal(_bits(pd), _bits(one_p))
            for a, b in zip(sd, one_s):
                assert torch.equal(_bits(a), _bits(b))
        print(f'[optim-bound] {ref.rule_id(rule_opts)} list of {len(sizes)}: worst |err| / bound = {worst:.4f}')
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------ norm
def _grads(sizes, scale, seed=0):
    g_ = torch.Generator().manual_seed(4400 + seed)
    return [(torch.randn(n, generator=g_) * scale).contiguous() for n in sizes]


@pytest.mark.parametrize('sizes,scale,max_norm,gscale', [
    ((0, 1, 4096, 4097, 5), 0.1, 0.5, 1.0),              # a norm (9.05) above max_norm
    ((0, 1, 4096, 4097, 5), 0.1, 1e4, 1.0),              # below: coef is exactly 1
    ((255,), 1e-3, 1.0, 1.0), ((4096 * 3 + 1,), 30.0, 35.0, 1.0), ((1048576 + 3,), 1.0, 1.0, 1.0),
    ((0, 1, 4096, 4097, 5), 0.1, 12.0, 4.0 / 3.0),       # the rescaled gradient of flush(): norm x 4/3 is above 12
    (ref.MANY_SIZES, 0.5, 1.0, 1.0)])                    # more than one table
def test_grad_norm_bound_and_repeatable(sizes, scale, max_norm, gscale):
    """norm relative to the fp64 norm (c = 2), coef relative to the fp64 coefficient (c = 4); the same call twice gives
    the same bits."""
    from fgn_amd import ops
    gs = _grads(sizes, scale, len(sizes))
    gd = [g.cuda() for g in gs]
    rec = ops.grad_norm_multi(gd, max_norm, grad_scale=gscale)
    again = ops.grad_norm_multi(gd, max_norm, grad_scale=gscale)
    assert torch.equal(_bits(rec), _bits(again))
    norm, _ = ref.grad_norm(gs, max_norm)
    norm *= ref.f32(gscale)
    coef = min(1.0, ref.f32(max_norm) / (norm + ref.f32(1e-6)))
    got_n, got_c = float(rec[0]), float(rec[1])
    print(f'[optim-bound] grad_norm sizes={sizes[:5]} max_norm={max_norm:g}: norm {got_n!r} (fp64 {norm!r}), coef {got_c!r} '
          f'(fp64 {coef!r}); |err| / bound = {abs(got_n - norm) / (ref.C_NORM * ref.U * norm + ref.TINY):.4f}, '
          f'{abs(got_c - coef) / (ref.C_COEF * ref.U * coef):.4f}')
    assert abs(got_n - norm) <= ref.C_NORM * ref.U * norm + ref.TINY
    assert abs(got_c - coef) <= ref.C_COEF * ref.U * coef
    if norm < max_norm * (1 - 1e-6):
        assert got_c == 1.0
    else:
        assert got_c < 1.0


def test_grad_norm_zero_gradients_and_empty_list():
    from fgn_amd import ops
    rec = ops.grad_norm_multi([torch.zeros(4097).cuda(), torch.zeros(0).cuda(), torch.zeros(3).cuda()], 2.0)
    assert float(rec[0]) == 0.0 and float(rec[1]) == 1.0
    rec = ops.grad_norm_multi([], 2.0)
    assert float(rec[0]) == 0.0 and float(rec[1]) == 1.0


def test_grad_norm_same_bits_for_another_split_at_chunk_boundaries():
    """One buffer of 5 x 4096 + 77 elements as one tensor, as (4096, 2 x 4096, 2 x 4096 + 77) and as five chunks and the
    tail: the chunk partials and their order are the same, so are the bits; ``out=`` is filled in place."""
    from fgn_amd import ops
    g = _grads((5 * 4096 + 77,), 0.3, 9)[0].cuda()
    whole = ops.grad_norm_multi([g], 1.0)
    out = torch.empty(2, device='cuda')
    for cuts in ((4096, 3 * 4096), (4096, 2 * 4096, 3 * 4096, 4 * 4096, 5 * 4096)):
        parts = [t.contiguous() for t in torch.tensor_split(g, cuts)]
        assert ops.grad_norm_multi(parts, 1.0, out=out) is out
        assert torch.equal(_bits(out), _bits(whole))
    # a misaligned view walks the element path over the same assignment: same bits again
    buf = torch.empty(g.numel() + 1, device='cuda')
    buf[1:].copy_(g)
    assert buf[1:].data_ptr() % 16 == 4
    assert torch.equal(_bits(ops.grad_norm_multi([buf[1:]], 1.0)), _bits(whole))


def test_grad_norm_nonfinite_gives_nan():
    """torch with error_if_nonfinite=False: a NaN gradient makes the norm, the coefficient and every clipped gradient NaN."""
    from fgn_amd import ops
    g = torch.ones(300)
    g[17] = float('nan')
    rec = ops.grad_norm_multi([g.cuda()], 1.0)
    assert bool(torch.isnan(rec).all())
    p = torch.ones(300).cuda()
    ops.optim_multi('SGD', [p], [g.cuda()], None, [0.1], 0.0, momentum=0.0, coef=rec)
    assert bool(torch.isnan(p).all())


# ------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize('n', ref.SIZES)
def test_grad_accumulate_bound(n):
    """``first`` overwrites whatever the accumulator held (NaN bytes included); four accumulations of the same g with
    a = 0.25, each within c = 2 of the reference started from the kernel's own previous accumulator; where 0.75 g is an
    fp32 number every partial sum is exact and the result is g bit for bit."""
    from fgn_amd import ops
    g = ref.adagrad_case(n, 1e-5, True)[1]
    acc = torch.full((n,), float('nan')).cuda()
    gd = g.cuda()
    prev, worst = acc.cpu(), 0.0
    for i in range(4):
        want, mag = ref.accumulate(prev, g, 0.25, i == 0)
        ops.grad_accumulate_multi([acc], [gd], 0.25, first=i == 0)
        prev = acc.cpu()
        worst = max(worst, ref.worst_ratio(prev, want, mag, ref.C_ACC))
    print(f'[optim-bound] accumulate n={n}: worst |err| / bound = {worst:.4f}')
    assert worst <= 1.0
    exact = ((0.75 * g.to(F64)).float().to(F64) == 0.75 * g.to(F64)) & (g.abs() > 1e-30)
    assert n < 255 or int(exact.sum()) > n // 8
    assert torch.equal(_bits(prev[exact]), _bits(g[exact]))


def test_grad_accumulate_list_of_more_than_one_table():
    from fgn_amd import ops
    gs = _grads(ref.MANY_SIZES, 1.0, 3)
    gd = [g.cuda() for g in gs]
    accs = [torch.full((g.numel(),), float('nan')).cuda() for g in gs]
    ops.grad_accumulate_multi(accs, gd, 0.5, first=True)
    ops.grad_accumulate_multi(accs, gd, 0.5, first=False)
    for a, g in zip(accs, gs):
        assert torch.equal(_bits(a), _bits(g))               # g / 2 + g / 2 is exact


# ------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    p, g, s = torch.zeros(8).cuda(), torch.zeros(8).cuda(), torch.zeros(8).cuda()
    with pytest.raises(FgnHipError):
        ops.optim_multi('Adam', [p], [torch.zeros(7).cuda()], [(s, s.clone())], [0.1])           # size mismatch
    with pytest.raises(FgnHipError):
        ops.optim_multi('Adam', [p], [g], [(torch.zeros(9).cuda(), s)], [0.1])
    with pytest.raises(FgnHipError):
        ops.optim_multi('SGD', [p], [torch.zeros(16).cuda()[::2]], [s], [0.1], momentum=0.9)        # non-contiguous
    with pytest.raises(FgnHipError):
        ops.optim_multi('SGD', [p], [torch.zeros(8)], [s], [0.1], momentum=0.9)                     # CPU tensor
    with pytest.raises(FgnHipError):
        ops.optim_multi('Adagrad', [torch.zeros(8)], [g], [s], [0.1])
    with pytest.raises(FgnHipError):
        ops.optim_multi('SGD', [p], [g], [s], [0.1], momentum=0.9, dampening=0.5)                   # before any launch
    with pytest.raises(FgnHipError):
        ops.optim_multi('SGD', [p], [g], None, [0.1], momentum=0.9)                                 # momentum needs its buffer
    with pytest.raises(FgnHipError):
        ops.optim_multi('AdamW', [p], [g], [(s, s)], [0.1])
    with pytest.raises(FgnHipError):
        ops.optim_multi('Adam', [p, p], [g], [(s, s)], [0.1])
    with pytest.raises(FgnHipError):
        ops.grad_norm_multi([g], 1.0, norm_type=1)
    with pytest.raises(FgnHipError):
        ops.grad_norm_multi([g], 1.0, norm_type=float('inf'))
    with pytest.raises(FgnHipError):
        ops.grad_norm_multi([torch.zeros(8)], 1.0)
    with pytest.raises(FgnHipError):
        ops.grad_norm_multi([torch.zeros(16).cuda()[::2]], 1.0)
    with pytest.raises(FgnHipError):
        ops.grad_accumulate_multi([p], [torch.zeros(7).cuda()], 0.5, True)
    with pytest.raises(FgnHipError):
        ops.grad_accumulate_multi([p], [torch.zeros(8)], 0.5, True)
    assert float(p.abs().sum()) == 0.0 and float(s.abs().sum()) == 0.0                              # nothing ran
