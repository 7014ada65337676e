"""The forward kernels of the training path (csrc/train.hip: the weighted loss sums, bbox2delta, BatchNorm in training
mode) and the Adagrad kernels (csrc/train_bwd.hip) alone against the float64 closed forms of tests/_train_ref.py, bounded
as the backward kernels are in tests/test_hip_train_bwd.py and the forward feature kernels in tests/test_hip_fwd_bound.py:

    |got - ref| <= c * 2^-24 * mag + 2^-126

``mag`` is the output's own term-magnitude sum, ``c`` the number of fp32 roundings counted in the kernel's arithmetic (each
docstring derives it from the code; first-order counts are rounded up; the constants live in tests/_train_ref.py, where
tests/test_train_ref_cpu.py holds a numpy emulation of each kernel to the same bound on the same inputs).  A loss sum is
one number, so it gets its per-element test from one-hot weights: the sum is then one element's loss and the bound that
element's own magnitude.  Every test prints ``[train-bound] name: worst |err| / bound`` before it asserts (DESIGN.md
section 7.3 carries the table).
"""
import numpy as np
import pytest
import torch

import _train_ref as ref

pytestmark = pytest.mark.gpu

U, TINY = ref.U, ref.TINY
F64 = torch.float64


def _bounded(name, got, want, mag, c, slack=None):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    worst = ref.worst_ratio(got, want, mag, c, slack)
    print(f'[train-bound] {name}: worst |err| / bound = {worst:.4f}')
    assert worst <= 1.0, (name, worst)
    return worst


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _dev(t):
    return None if t is None else t.cuda()


def _weightings(n, w):
    """No weights, the case's weights, then one-hot weights at the probe indices (0, 63, 64, 1023, 1024, n - 1)."""
    out = [('w=None', None), ('w', w)]
    for i in ref.probe_indices(n):
        hot = torch.zeros(n)
        hot[i] = 1.0 + float(w[i])
        out.append((f'one-hot {i}', hot))
    return out


# ------------------------------------------------------------------------------------------ loss sums
@pytest.mark.parametrize('kind', ref.BCE_KINDS)
@pytest.mark.parametrize('n', ref.LOSS_SIZES)
def test_bce_logits_sum_bound(n, kind):
    """bce_sum_kernel: the element's loss is formed in fp64 and rounded to fp32 (1 rounding, on l_i <= mag_i), multiplied
    by the weight and accumulated in fp64 (thread-serial, xor butterfly, 16 wave partials: 2^-53 each), divided by
    avg_factor in fp64 and rounded to fp32 (1, on |sum| <= mag); rounded up: c = 3.
    Logits +-{0, 1e-3, 1, 20, 30, 40, 90, 104} among randn * 4; targets binarised at 0.5 with values at, one ulp below
    and one ulp above the threshold / soft targets as they are / hard 0 / 1 targets.  With and without weights, avg_factor
    77.3; one-hot weights at 0, 63, 64, 1023, 1024 and n - 1, where the logit is -40 .. -1e-3 with target 0: the sum
    is log1p(exp(x)) of one element, down to 4e-18, and must be right to 3 * 2^-24 of THAT.  n = 0 is exactly +0; two runs
    give the same bits."""
    from fgn_amd import ops
    x, y, w, thr = ref.bce_case(n, kind)
    xd, yd = x.cuda(), y.cuda()
    worst = 0.0
    for tag, ww in _weightings(n, w):
        val, mag = ref.bce_sum(x, y, ww, ref.LOSS_AVG, thr)
        got = ops.bce_logits_sum(xd, yd, _dev(ww), ref.LOSS_AVG, y_threshold=thr)
        assert got.shape == (1,)
        worst = max(worst, _bounded(f'bce_logits_sum n={n} {kind} {tag}', got[0], val, mag, ref.C_BCE))
        assert torch.equal(_bits(got), _bits(ops.bce_logits_sum(xd, yd, _dev(ww), ref.LOSS_AVG, y_threshold=thr)))
        if n == 0:
            assert int(_bits(got)[0]) == 0
    print(f'[train-bound] bce_logits_sum n={n} {kind}: worst of the case = {worst:.4f}')


@pytest.mark.parametrize('beta', ref.SL1_BETAS)
@pytest.mark.parametrize('n', ref.LOSS_SIZES)
def test_smooth_l1_sum_bound(n, beta):
    """smooth_l1_sum_kernel, fp32 per element: d = |p - t| (1 rounding; the bound gives it |p| + |t| scaled by the slope
    of the branch); quadratic branch 0.5 d exact, * d (1), / beta (1), the error of d enters twice (2 l 2^-24): 4 on l;
    linear branch: d - 0.5 beta (1) and the error of d on l + 0.5 beta: 2.  ``w * l`` in fp32 (1), then fp64 accumulation
    and the final rounding (1): c = 4 + 1 + 1 + 1 (rounded up) = 7.  The branch is taken on the fp32 d; the loss is
    continuously differentiable at |d| = beta, so a d that rounds across the edge moves the value in second order only.
    Differences exactly beta, beta -+ 1 ulp, 0 (both signs) at the origin and off it (0.75 + d - 0.75, with the fp32
    neighbours of the sum) among randn * 2 - randn, beta in {1, 1 / 9}; one-hot weights at the probe indices."""
    from fgn_amd import ops
    p, t, w = ref.smooth_l1_case(n, beta)
    pd, td = p.cuda(), t.cuda()
    worst = 0.0
    for tag, ww in _weightings(n, w):
        val, mag = ref.smooth_l1_sum(p, t, ww, ref.LOSS_AVG, beta)
        got = ops.smooth_l1_sum(pd, td, _dev(ww), ref.LOSS_AVG, beta=beta)
        worst = max(worst, _bounded(f'smooth_l1_sum n={n} beta={beta:.4f} {tag}', got[0], val, mag, ref.C_SL1))
        assert torch.equal(_bits(got), _bits(ops.smooth_l1_sum(pd, td, _dev(ww), ref.LOSS_AVG, beta=beta)))
        if n == 0:
            assert int(_bits(got)[0]) == 0
    print(f'[train-bound] smooth_l1_sum n={n} beta={beta:.4f}: worst of the case = {worst:.4f}')


@pytest.mark.parametrize('C', ref.CE_CLASSES)
@pytest.mark.parametrize('n', ref.LOSS_SIZES)
def test_softmax_ce_sum_bound(n, C):
    """softmax_ce_sum_kernel: the row maximum in fp32 (exact), r_c - max in fp32 (1 rounding per class; it moves log s
    by 2^-24 sum_c p_c |r_c - max|, which the rows of the tests keep below mag_i = |max| + |log s| + |r_label| -
    ``softmax_ce_conditioning`` <= 1 is asserted - so the C roundings count once), exponentials, their sum, the logarithm
    and max + log s - r_label in fp64, rounded to fp32 (1), ``w * l`` in fp32 (1), fp64 accumulation, the final rounding
    (1); rounded up: c = 5.
    C in {1, 2, 4, 9}; rows whose label is the maximum by 100 (loss ~e^-100 of the terms), rows of equal logits, logits
    at +-1e4 with the label on either; every fifth label ignored (-1, C, 255).  C = 1 gives exactly +0, all labels
    ignored exactly +0.  One-hot weights at the probe indices (on counted rows)."""
    from fgn_amd import ops
    z, lab, w = ref.softmax_ce_case(n, C)
    assert ref.softmax_ce_conditioning(z, lab) <= 1.0
    zd, ld = z.cuda(), lab.cuda()
    worst = 0.0
    for tag, ww in _weightings(n, w):
        val, mag = ref.softmax_ce_sum(z, lab, ww, ref.LOSS_AVG)
        got = ops.softmax_ce_sum(zd, ld, _dev(ww), ref.LOSS_AVG)
        worst = max(worst, _bounded(f'softmax_ce_sum n={n} C={C} {tag}', got[0], val, mag, ref.C_CE))
        assert torch.equal(_bits(got), _bits(ops.softmax_ce_sum(zd, ld, _dev(ww), ref.LOSS_AVG)))
        if C == 1 or n == 0:
            assert int(_bits(got)[0]) == 0
    z0, lab0, w0 = ref.softmax_ce_case(n, C, all_ignored=True)
    for ww in (None, w0):
        assert int(_bits(ops.softmax_ce_sum(z0.cuda(), lab0.cuda(), _dev(ww), ref.LOSS_AVG))[0]) == 0
    print(f'[train-bound] softmax_ce_sum n={n} C={C}: worst of the case = {worst:.4f}')


def test_loss_sums_still_refuse_bad_arguments():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    x, y, w, _ = ref.bce_case(63, 'hard')
    x, y, w = x.cuda(), y.cuda(), w.cuda()
    for beta in (0.0, -1.0, float('nan')):
        with pytest.raises(FgnHipError):
            ops.smooth_l1_sum(x, y, w, 1.0, beta=beta)
    with pytest.raises(FgnHipError):
        ops.softmax_ce_sum(torch.zeros(3, 0).cuda(), torch.zeros(3, dtype=torch.int64).cuda(), None, 1.0)
    with pytest.raises(FgnHipError):
        ops.bce_logits_sum(x, y[:62], None, 1.0)
    with pytest.raises(FgnHipError):
        ops.bce_logits_sum(x, y, w[:62], 1.0)
    with pytest.raises(FgnHipError):
        ops.smooth_l1_sum(x, y[:62], None, 1.0)
    z, lab, lw = ref.softmax_ce_case(63, 4)
    with pytest.raises(FgnHipError):
        ops.softmax_ce_sum(z.cuda(), lab[:62].cuda(), None, 1.0)
    with pytest.raises(FgnHipError):
        ops.softmax_ce_sum(z.cuda(), lab.cuda(), lw[:62].cuda(), 1.0)


# ------------------------------------------------------------------------------------------ bbox2delta
@pytest.mark.parametrize('coder', range(len(ref.BBOX_CODERS)))
@pytest.mark.parametrize('n', ref.BBOX_SIZES)
def test_bbox2delta_bits_and_bound(n, coder):
    """bbox2delta_kernel against ``bbox2delta_f32`` (its own operation sequence in numpy.float32): csrc/train.hip is built
    with -ffp-contract=off (asserted), so dx and dy are those BIT FOR BIT; dw and dh go through the device's fp64
    logarithm, which may differ from the host's in its last place: within one fp32 ulp, the number that differ is
    printed.  A zero-width proposal gives the same non-finite pattern (inf of either sign, NaN).
    Float64 bound.  dx: gx and px (1 each, on (|g0| + |g2|) / 2 and (|p0| + |p2|) / 2), their difference (1), pw (1), the
    division (1), ``- mean`` (1), ``/ std`` (1), rounded up: c = 8 on (((|g0| + |g2|) + (|p0| + |p2|)) / 2 / |pw| +
    |mean|) / |std|.  dw: gw, pw and their quotient (3: a relative error of the argument is an absolute error of the
    logarithm, the 1 of the magnitude), the logarithm rounded to fp32 (1), ``- mean`` (1), ``/ std`` (1), rounded up:
    c = 7 on (|log(gw / pw)| + 1 + |mean|) / |std|.
    Rows: generic boxes; GT = proposal (all four exactly 0); boxes 1e3 from the origin with 4 px sides (the centres
    cancel); width ratios 1e-3 and 1e3; zero-width proposals.  Both coders of fgn_amd/config.py."""
    from fgn_amd import build, ops
    assert ('train.hip', ['-ffp-contract=off']) in build.SOURCES
    means, stds = ref.BBOX_CODERS[coder]
    p, q, kind = ref.bbox_case(n)
    got = ops.bbox2delta(p.cuda(), q.cuda(), means, stds).cpu()
    assert got.shape == (n, 4)
    if n == 0:
        return
    e32 = torch.from_numpy(ref.bbox2delta_f32(p, q, means, stds))
    val, mag = ref.bbox2delta(p, q, means, stds)
    fin = torch.isfinite(e32)
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(torch.isnan(got), torch.isnan(e32))
    assert torch.equal(got[torch.isinf(e32)], e32[torch.isinf(e32)])                  # the same sign of infinity
    assert torch.equal(torch.isfinite(val), fin)
    rows = fin.all(dim=1)
    assert torch.equal(_bits(got[rows][:, :2]), _bits(e32[rows][:, :2]))             # dx, dy bit for bit
    assert torch.equal(_bits(got[:, 1][fin[:, 1]]), _bits(e32[:, 1][fin[:, 1]]))     # dy of the zero-width rows too
    wh_got, wh_ref = got[:, 2:][fin[:, 2:]], e32[:, 2:][fin[:, 2:]]
    ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(wh_ref.numpy()), np.float32(2.0 ** -126))))
    differ = int((wh_got != wh_ref).sum())
    print(f'[train-bound] bbox2delta n={n} coder={coder}: dx, dy bit for bit; dw, dh differ by an ulp in {differ} of '
          f'{wh_ref.numel()} elements')
    assert bool(((wh_got.double() - wh_ref.double()).abs() <= ulp.double()).all())
    assert bool((got[kind == 1] == 0).all())
    c = torch.tensor([ref.C_BBOX_XY, ref.C_BBOX_XY, ref.C_BBOX_WH, ref.C_BBOX_WH], dtype=F64).expand(n, 4)
    _bounded(f'bbox2delta n={n} coder={coder}', got[fin], val[fin], mag[fin], c[fin])
    if n >= 255:
        zero = p[:, 2] == p[:, 0]
        assert bool(zero.any()) and bool((~fin[zero][:, [0, 2]]).all()) and bool(fin[zero][:, [1, 3]].all())


# ------------------------------------------------------------------------------------------ BatchNorm, training mode
def _bn_call(k, full, inplace):
    from fgn_amd import ops
    x = k['x'].cuda()
    rm, rv = (k['rm'].cuda(), k['rv'].cuda()) if full else (None, None)
    y, mean, var = ops.bn_train(x, k['gamma'].cuda(), k['beta'].cuda(), ref.BN_EPS, ref.BN_MOMENTUM, rm, rv,
                                residual=k['res'].cuda() if full else None, relu=full, inplace=inplace)
    assert (y.data_ptr() == x.data_ptr()) == inplace
    out = dict(y=y, mean=mean, var=var)
    if full:
        out.update(rm=rm, rv=rv)
    return out


@pytest.mark.parametrize('ratio', ref.BN_RATIOS + ref.BN_FAR_RATIOS)
@pytest.mark.parametrize('P,C', ref.BN_SHAPES)
def test_bn_train_bound(P, C, ratio):
    """fgn_bn_train_f32 on x [P,C], channel c = randn s_c + sign_c ratio s_c, plain and with residual + ReLU + running
    statistics.  Statistics: fp64 sums of x - x[0] and its square (bn_partial_kernel; 64 chunks x 4 row phases), so
      mean          the fp64 value rounded (1), rounded up: c = 2 on mean |x|
      var           c_var = 2 + ceil(3 D (k^2 + 1) 2^-29) of ``_train_ref.bn_var_count`` (= 3 here) RELATIVE to the variance
                    itself: the backward pass and the next step's rstd consume it
      running_mean  1 - momentum (1), its product (1), momentum * mean (1) with the rounded mean (1), the sum (1),
                    rounded up: c = 6 on (1 - mom) |rm| + mom mean |x|
      running_var   the same with the unbiased variance (its rounding is inside c_var): c = 5 + c_var on
                    (1 - mom) |rv| + mom var P / (P - 1); P = 1 uses var
      y             mean rounded (1, on |gamma| rstd |mean|), var + eps (1), sqrtf (1), 1 / (1), x - mean (1), * rstd (1),
                    * gamma (1), + beta (1), + residual (1), rounded up: c = 10 on |gamma| rstd (|x| + mean |x|) + |beta| +
                    |residual|, plus 0.5 c_var 2^-24 on |gamma| rstd |x - mean| (the variance's own relative error, halved
                    by the square root).  ReLU is 1-Lipschitz.
    Shapes: P = 1; P = 3 and 63 below the 64 chunks and P = 64 at them; 65 rows (not a multiple of the 4 phases) with
    C / 4 = 65 across the 64-lane block; (441, 1024) and (6273, 128) of the shared head; (8200, 512) = 1 049 600 float4,
    over the 4096-block grid-stride cap of bn_apply_kernel.  Channel 0 is constant (variance exactly 0: y = beta +
    residual), channel 1 scaled by 1e-4 (variance far below eps), gamma[2] < 0, gamma[3] = 0.
    mean / std in {0, 0.25, 30, 1000, 3000}: every output asserted.  mean / std in {1e4, 1e5}: y and mean asserted (their
    bounds are linear in the offset); the variance and running_var are measured and printed, NOT asserted: sums of the raw
    values, which the kernel formed until this test existed, lose (mean / std)^2 2^-53 of the variance - in emulation
    about 2 units of 2^-24 var at 1e4 and 100 to 180 at 1e5 - and that is beyond the range GroupNorm was committed to
    (3000).  The sums of shifted values keep the printed ratios where they are inside that range.
    The call with out = x gives the bytes of the out-of-place call (y, mean, var, running statistics); two runs give
    the same bits."""
    k = ref.bn_case(P, C, ratio)
    far = ratio in ref.BN_FAR_RATIOS
    for full in (False, True):
        r = ref.bn_train(k['x'], k['gamma'], k['beta'], ref.BN_EPS, ref.BN_MOMENTUM, k['rm'] if full else None,
                         k['rv'] if full else None, k['res'] if full else None, full)
        got = _bn_call(k, full, inplace=False)
        tag = f'bn_train {(P, C)} mean/std={ratio:g}' + (' res+relu+running' if full else '')
        ratios = ref.bn_ratios(got, r, with_var=not far)
        for name, v in ratios.items():
            print(f'[train-bound] {tag} {name}: worst |err| / bound = {v:.4f}')
        for name, v in ratios.items():
            assert 'not asserted' in name or v <= 1.0, (tag, name, v)
        assert int(_bits(got['var'])[0]) == 0                                       # the constant channel: exactly +0
        want0 = k['beta'][0] + (k['res'][:, 0] if full else 0.0)
        want0 = want0.clamp_min(0.0) if full else want0.expand(P)
        assert torch.equal(_bits(got['y'][:, 0]), _bits(want0.float()))
        assert float(got['var'][1]) < 1e-2 * ref.BN_EPS                               # the channel scaled by 1e-4
        for other in (_bn_call(k, full, inplace=True), _bn_call(k, full, inplace=False)):
            for name in got:
                assert torch.equal(_bits(other[name]), _bits(got[name])), (tag, name)


def test_bn_train_still_refuses_bad_shapes():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    with pytest.raises(FgnHipError):
        ops.bn_train(torch.zeros(5, 6).cuda(), torch.ones(6).cuda(), torch.zeros(6).cuda(), 1e-5, 0.1)
    with pytest.raises(FgnHipError):
        ops.bn_train(torch.zeros(5, 8).cuda(), torch.ones(8).cuda(), torch.zeros(8).cuda(), 1e-5, 0.1,
                     residual=torch.zeros(4, 8).cuda())


# ------------------------------------------------------------------------------------------ Adagrad
def _adagrad_check(tag, step_fn, p, g, st, lr, wd):
    """One update of (p, g, st) (CPU fp32 tensors) by ``step_fn(p_dev, g_dev, st_dev)`` -> the new (p, state) on the CPU,
    both bounded against the reference started from the same p and state."""
    r = ref.adagrad(p, g, st, lr, wd, ref.ADAGRAD_EPS)
    pd, sd = p.cuda(), st.cuda()
    step_fn(pd, g.cuda(), sd)
    p2, s2 = pd.cpu(), sd.cpu()
    ws = _bounded(tag + ' state', s2, r['state'], r['state_mag'], ref.C_ADA_STATE)
    wp = _bounded(tag + ' p', p2, r['p'], r['p_mag'], ref.C_ADA_P)
    assert bool((s2 >= 0).all())
    return p2, s2, ws, wp


@pytest.mark.parametrize('warm', [False, True])
@pytest.mark.parametrize('wd,lr', ref.ADAGRAD_PAIRS)
@pytest.mark.parametrize('n', ref.ADAGRAD_SIZES)
def test_adagrad_step_and_multi_bound(n, wd, lr, warm):
    """adagrad_kernel / adagrad_multi_kernel, fp32; csrc/train_bwd.hip allows contraction, the counts cover the fused
    and the unfused form (a contraction removes a rounding).
      g' = g + wd p        wd p (1), the sum (1): 2 on mag_g = |g| + |wd p|
      state' = state + g'^2   the error of g' enters g'^2 twice (2 x 2 |g'| mag_g 2^-24: the term 2 |g'| mag_g of the
                           magnitude, counted 2), the square (1), the sum (1), rounded up: c = 5 on state + g'^2 +
                           2 |g'| mag_g
      p' = p - lr g' / (sqrt(state') + eps)   the error of g' directly (2, on lr mag_g / den) and through state' under
                           the square root (0.5 x 4 = 2 on the same term, 0.5 x 2 = 1 on |step|), sqrtf (1), + eps (1),
                           lr g' (1), the division (1), the subtraction (1), rounded up: c = 11 on |p| + |step| +
                           lr mag_g / den.  (A square that underflows moves the denominator by at most sqrt(2^-126) =
                           1e-19 against eps = 1e-10: inside the rounding-up.)
    n in {1, 255, 4095, 4096, 4097, 2^20 + 3}: the 4096-element chunk edge of the multi kernel, the grid stride of the
    single one; (wd, lr) in {(1e-5, 0.005), (0, 0.01), (1e-4, 0.01)}; fresh (zero) and warm (1e-8 .. 1e2) state;
    g = +-(1e-6 .. 10), g = 0 on a zero state, g = -wd p (1 +- 1e-3), g = 1e-25 with p = 0.  One step from identical
    inputs through either entry point, then two more through ``adagrad_step``, each against the reference started from
    the kernel's own previous p and state (errors do not compound into the bound).  Where g' = 0 on a zero state p
    keeps its bits and the state stays +0."""
    from fgn_amd import ops
    p0, g, st0, kind = ref.adagrad_case(n, wd, warm)
    single = lambda p, gr, s: ops.adagrad_step(p, gr, s, lr, wd, ref.ADAGRAD_EPS)
    multi = lambda p, gr, s: ops.adagrad_multi([p], [gr], [s], [lr], wd, ref.ADAGRAD_EPS)
    tag = f'adagrad n={n} wd={wd:g} lr={lr:g} {"warm" if warm else "fresh"}'
    p1, s1, ws, wp = _adagrad_check(tag + ' step 1', single, p0, g, st0, lr, wd)
    pm, sm, _, _ = _adagrad_check(tag + ' multi', multi, p0, g, st0, lr, wd)
    assert torch.equal(_bits(pm), _bits(p1)) and torch.equal(_bits(sm), _bits(s1))
    if not warm:
        still = (kind == 3) & ((p0 == 0) | (ref.f32(wd) == 0))
        assert torch.equal(_bits(p1[still]), _bits(p0[still])) and bool((_bits(s1[still]) == 0).all())
        assert n < 255 or int(still.sum()) > 0
    p, s = p1, s1
    for step in (2, 3):
        p, s, a, b = _adagrad_check(f'{tag} step {step}', single, p, g, s, lr, wd)
        ws, wp = max(ws, a), max(wp, b)
    print(f'[train-bound] {tag}: worst of the case state = {ws:.4f}, p = {wp:.4f}')


@pytest.mark.parametrize('wd', [1e-5, 0.0])
def test_adagrad_multi_list_bound(wd):
    """Five tensors of 0, 1, 4096, 4097 and 5 elements (an empty one, one chunk exactly, one element into the next
    chunk) with five learning rates in ONE launch: every tensor held to the bounds of the single launch."""
    from fgn_amd import ops
    cases = [ref.adagrad_case(n, wd, True, seed=i) for i, n in enumerate(ref.ADAGRAD_MULTI_SIZES)]
    P = [c[0].cuda() for c in cases]
    G = [c[1].cuda() for c in cases]
    S = [c[2].cuda() for c in cases]
    ops.adagrad_multi(P, G, S, list(ref.ADAGRAD_MULTI_LRS), wd, ref.ADAGRAD_EPS)
    for (p0, g, s0, _), pd, sd, lr in zip(cases, P, S, ref.ADAGRAD_MULTI_LRS):
        r = ref.adagrad(p0, g, s0, lr, wd, ref.ADAGRAD_EPS)
        tag = f'adagrad_multi list n={p0.numel()} lr={lr:g} wd={wd:g}'
        _bounded(tag + ' state', sd, r['state'], r['state_mag'], ref.C_ADA_STATE)
        _bounded(tag + ' p', pd, r['p'], r['p_mag'], ref.C_ADA_P)
