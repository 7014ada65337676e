"""Feature gradients through ``Trainer``: ``forward_backward(..., features=, feature_grads=True)`` against
torch.autograd on the training oracle started from IDENTICAL feature tensors, the properties of the interface, and a
finite-difference check of the whole chain through an elementwise feature transform.

Measured on an MI355X (L2 error / L2 norm, worst element / largest element), (n_ways, k_shots) = (3, 2) | (1, 2):
see DESIGN 7.9."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _models(cfg, seed=0):
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    sd = init_state_dict(cfg, seed)
    # non-trivial BatchNorm parameters for the shared head so that the train-mode statistics matter
    g = torch.Generator().manual_seed(99)
    for k in sd:
        if k.startswith('roi_head.shared_head') and k.endswith('.weight') and sd[k].dim() == 1:
            sd[k] = 0.75 + 0.5 * torch.rand(sd[k].shape, generator=g)
        if k.startswith('roi_head.shared_head') and k.endswith('.bias') and sd[k].dim() == 1:
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    m = FGN(cfg['n_ways'], cfg['k_shots'], backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
            test_cfg=cfg['test_cfg'], state_dict=sd)
    return m, sd


def _f(v):
    v = v[0] if isinstance(v, list) else v
    return float(v.detach().reshape(-1)[0]) if isinstance(v, torch.Tensor) else float(v)


def _compare_losses(got, ref, rel):
    for k in ('loss_rpn_cls', 'loss_rpn_bbox', 'loss_cls', 'loss_bbox', 'loss_mask'):
        assert _f(got[k]) == pytest.approx(_f(ref[k]), rel=rel, abs=1e-7), k
    for k in ('ACC-Unbalanced', 'ACC-Balanced'):
        assert _f(got[k]) == pytest.approx(_f(ref[k]), abs=1e-6), k
    assert set(got) == set(ref)


def _setup(n_ways, k_shots):
    """-> (cfg, batch, a fresh trainer, its model's own two feature tensors)."""
    from fgn_amd.config import tiny_config
    from fgn_amd.episodes import make_batch
    from fgn_amd.train import Trainer
    cfg = tiny_config(n_ways, k_shots, width_div=2)
    m, sd = _models(cfg)
    b = make_batch(0, 2, n_ways, k_shots, 160, 224, 64)
    tr = Trainer(m)
    feats = (m.extract_feat(b['qry_img']), m.extract_feat(b['spp_imgs'].reshape(-1, *b['spp_imgs'].shape[-3:])))
    return cfg, sd, b, tr, feats


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (float((got - ref).norm()) / (float(ref.norm()) + 1e-30),
            float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30))


@pytest.mark.parametrize('n_ways,k_shots,l2_bound,max_bound', [(3, 2, 3e-3, 3e-2), (1, 2, 1e-2, 6e-2)])
def test_feature_grads_match_autograd_of_the_oracle(n_ways, k_shots, l2_bound, max_bound, monkeypatch):
    """Both sides start from the same two feature tensors (the model's own ``extract_feat``): the trainer takes them as
    ``features=``, the oracle through a stand-in for its backbone that returns them as NCHW leaves.  What remains between
    the two is what remains in the parameter-gradient test: ReLU sign flips behind train-mode BatchNorm - its bounds, per
    tensor; the AG-RPN parts sit behind one ReLU only and take the tight 3e-3 in both configurations."""
    from oracle import fgn_ref_cpu as O, fgn_train_cpu as T
    cfg, sd, b, tr, feats = _setup(n_ways, k_shots)
    leaves = [f.permute(0, 3, 1, 2).contiguous().cpu().requires_grad_(True) for f in feats]
    n_qry = b['qry_img'].shape[0]
    handed = []

    def stand_in(img, sd_, cfg_):
        leaf = leaves[len(handed)]
        assert img.shape[0] == (n_qry if not handed else leaves[1].shape[0])
        handed.append(leaf)
        return leaf
    monkeypatch.setattr(O, 'backbone_c4', stand_in)
    torch.manual_seed(5)
    ref_losses = T.forward_train({k: v.clone() for k, v in sd.items()}, cfg, grad=True, **b)
    monkeypatch.undo()
    assert len(handed) == 2
    rpn_sum = ref_losses['loss_rpn_cls'][0] + ref_losses['loss_rpn_bbox'][0]
    roi_sum = ref_losses['loss_cls'] + ref_losses['loss_bbox'] + ref_losses['loss_mask']
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    g_rpn = [nhwc(t) for t in torch.autograd.grad(rpn_sum, leaves, retain_graph=True)]
    g_roi = [nhwc(t) for t in torch.autograd.grad(roi_sum, leaves, retain_graph=True)]
    g_all = [nhwc(t) for t in torch.autograd.grad(T.total_loss(ref_losses), leaves)]
    assert all(float(t.abs().max()) > 0 for t in g_rpn + g_roi)
    print(f'oracle: |d_qry| {float(g_all[0].norm()):.3f} |d_spp| {float(g_all[1].norm()):.3f}')

    tr.model.debug_trace = {}
    torch.manual_seed(5)
    got_losses = tr.forward_backward(b, features=feats, feature_grads=True)
    _compare_losses(got_losses, ref_losses, 1e-4)
    fg, trace = tr.feature_grads, tr.model.debug_trace
    assert set(fg) == {'qry_fmap', 'spp_fmaps'}
    checks = [('qry_fmap', fg['qry_fmap'], g_all[0], l2_bound, max_bound),
              ('spp_fmaps', fg['spp_fmaps'], g_all[1], l2_bound, max_bound),
              ('d_qry_fmap_rpn', trace['d_qry_fmap_rpn'], g_rpn[0], 3e-3, 3e-2),
              ('d_spp_fmaps_vec', trace['d_spp_fmaps_vec'], g_rpn[1], 3e-3, 3e-2),
              ('d_qry_fmap_roi', trace['d_qry_fmap_roi'], g_roi[0], l2_bound, max_bound),
              ('d_spp_fmaps_roi', trace['d_spp_fmaps_roi'], g_roi[1], l2_bound, max_bound)]
    rep = {name: _rel(got, ref) for name, got, ref, _, _ in checks}
    print(f'({n_ways},{k_shots}) feature gradients (L2/L2, max/max):', {k: (f'{v[0]:.2e}', f'{v[1]:.2e}') for k, v in rep.items()})
    bad = {name: rep[name] for name, _, _, l2, mx in checks if rep[name][0] > l2 or rep[name][1] > mx}
    assert not bad, bad
    # the parts add up to the results: the RoIAlign backward adds its overwrite result onto the AG-RPN part
    assert torch.equal(trace['d_qry_fmap_rpn'] + trace['d_qry_fmap_roi'], fg['qry_fmap'])
    assert torch.equal(trace['d_spp_fmaps_vec'] + trace['d_spp_fmaps_roi'], fg['spp_fmaps'])
    # the given tensors were read, never written
    assert all(torch.equal(f.cpu(), nhwc(l.detach())) for f, l in zip(feats, leaves))


def test_feature_grads_leave_the_parameter_gradients_alone_and_repeat_bit_for_bit():
    """(1) self.grads with feature_grads=True are the bytes of an identically seeded trainer without it; (2) features =
    the model's own extract_feat gives the losses and gradients of the plain call; (3) two identically seeded trainers
    give the same feature-gradient bytes; (6) under cumulative_iters=2 a micro-step's feature gradients are those of
    cumulative_iters=1 (not divided)."""
    from fgn_amd.train import Trainer
    cfg, sd, b, tr_a, feats = _setup(3, 2)
    torch.manual_seed(5)
    la = tr_a.forward_backward(b, feature_grads=True)
    assert set(tr_a.feature_grads) == {'qry_fmap', 'spp_fmaps'}
    assert tuple(tr_a.feature_grads['qry_fmap'].shape) == tuple(feats[0].shape)
    assert tuple(tr_a.feature_grads['spp_fmaps'].shape) == tuple(feats[1].shape)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in tr_a.feature_grads.values())
    _, _, _, tr_b, _ = _setup(3, 2)
    torch.manual_seed(5)
    lb = tr_b.forward_backward(b)
    assert tr_b.feature_grads == {}
    assert set(tr_a.grads) == set(tr_b.grads) and all(torch.equal(tr_a.grads[k], tr_b.grads[k]) for k in tr_b.grads)
    assert all(_f(la[k]) == _f(lb[k]) for k in lb)
    # (2) features in: the same bytes as the plain call
    _, _, _, tr_c, feats_c = _setup(3, 2)
    torch.manual_seed(5)
    lc = tr_c.forward_backward(b, features=feats_c, feature_grads=True)
    assert all(_f(lc[k]) == _f(lb[k]) for k in lb)
    assert all(torch.equal(tr_c.grads[k], tr_b.grads[k]) for k in tr_b.grads)
    # (3) bit-reproducible
    assert all(torch.equal(tr_c.feature_grads[k], tr_a.feature_grads[k]) for k in tr_a.feature_grads)
    # refreshed per call: {} again when not asked
    torch.manual_seed(5)
    tr_c.forward_backward(b)
    assert tr_c.feature_grads == {}
    # (6) accumulation does not rescale them
    m_d, _ = _models(cfg)
    tr_d = Trainer(m_d, cumulative_iters=2)
    torch.manual_seed(5)
    tr_d.step(b, feature_grads=True)
    assert tr_d._pending == 1
    assert all(torch.equal(tr_d.feature_grads[k], tr_a.feature_grads[k]) for k in tr_a.feature_grads)


def test_feature_grads_of_a_step_that_samples_no_roi():
    """No ground truth and no proposals: no RoI is sampled, the RoI stage contributes nothing - both tensors are still
    returned, from the AG-RPN alone."""
    cfg, sd, b, tr, feats = _setup(3, 2)
    empty = copy.deepcopy(b)
    for i in range(2):
        empty['qry_bboxes'][i], empty['qry_cat_ids'][i] = b['qry_bboxes'][i][:0], b['qry_cat_ids'][i][:0]
        empty['qry_isegmaps'][i] = b['qry_isegmaps'][i][:0]
    empty['proposals'] = [torch.zeros(0, 5) for _ in range(2)]
    m = tr.model
    m.debug_trace = {}
    torch.manual_seed(5)
    losses = tr.forward_backward(empty, feature_grads=True)
    assert 'loss_cls' not in losses and m.debug_trace['rois'].shape[0] == 0          # no RoI was sampled
    fg = tr.feature_grads
    trace = m.debug_trace
    assert tuple(fg['qry_fmap'].shape) == tuple(feats[0].shape) and tuple(fg['spp_fmaps'].shape) == tuple(feats[1].shape)
    assert float(trace['d_qry_fmap_roi'].abs().max()) == 0.0 and float(trace['d_spp_fmaps_roi'].abs().max()) == 0.0
    assert float(fg['qry_fmap'].abs().max()) > 0.0 and float(fg['spp_fmaps'].abs().max()) > 0.0
    assert torch.equal(fg['qry_fmap'], trace['d_qry_fmap_rpn']) and torch.equal(fg['spp_fmaps'], trace['d_spp_fmaps_vec'])


def test_features_of_the_wrong_kind_are_refused_by_name():
    cfg, sd, b, tr, (q, s) = _setup(1, 2)
    cases = {'shape': (q[:, :-1].contiguous(), s), 'dtype': (q.double(), s), 'device': (q.cpu(), s),
             'stride': (q.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), s)}
    for what, pair in cases.items():
        with pytest.raises(ValueError, match='qry_fmap'):
            tr.forward_backward(b, features=pair)
    for what, bad in {'shape': s[:-1].contiguous(), 'dtype': s.half(), 'device': s.cpu(),
                      'stride': s.transpose(1, 2).contiguous().transpose(1, 2)}.items():
        with pytest.raises(ValueError, match='spp_fmaps'):
            tr.forward_backward(b, features=(q, bad))
    with pytest.raises(ValueError, match='pair'):
        tr.forward_backward(b, features=q)
    # ... and FGN.forward_train takes the same pair
    torch.manual_seed(5)
    plain = tr.model.forward_train(**b)
    torch.manual_seed(5)
    given = tr.model.forward_train(features=(q, s), **b)
    assert all(_f(plain[k]) == _f(given[k]) for k in plain)


def test_feature_grads_are_the_derivative_of_the_summed_loss():
    """Sign and scale of the whole chain by finite differences, through an elementwise transform of the features:
    f = extract_feat(x) * g + b per channel.  The analytic directional derivative <d loss / d g, d> - from
    f.backward(trainer.feature_grads) - against the central differences of the summed loss over g +- eps d at two eps a
    factor 4 apart, with the proposals passed in and the sampler's permutations fixed so that every selection is the
    same in all calls.  The two differences must agree with each other better than either agrees with zero, and the
    analytic value must lie within their spread of them.  Not a precision bound."""
    cfg, sd, b, tr, (q0, s0) = _setup(3, 2)
    perm = lambda n: torch.randperm(n, generator=torch.Generator().manual_seed(1000 + n))
    tr.model.debug_trace = {}
    tr.forward_backward(b, perm_fn=perm)
    fixed = dict(b, proposals=[p.clone() for p in tr.model.debug_trace['proposals']])
    tr.model.debug_trace = None
    C = q0.shape[-1]
    gen = torch.Generator().manual_seed(7)
    g = (1.0 + 0.1 * torch.randn(C, generator=gen)).cuda().requires_grad_(True)
    bias = (0.05 * torch.randn(C, generator=gen)).cuda().requires_grad_(True)
    d = torch.randn(C, generator=gen).cuda()

    def total(gv, want_grads):
        fq, fs = q0 * gv + bias, s0 * gv + bias
        losses = tr.forward_backward(fixed, perm_fn=perm, features=(fq.detach().contiguous(), fs.detach().contiguous()),
                                     feature_grads=want_grads)
        return sum(_f(v) for k, v in losses.items() if 'loss' in k), (fq, fs)

    _, (fq, fs) = total(g, True)
    fq.backward(tr.feature_grads['qry_fmap'])
    fs.backward(tr.feature_grads['spp_fmaps'])
    analytic = float((g.grad.double() * d.double()).sum())
    fd = []
    for eps in (4e-3, 1.6e-2):
        with torch.no_grad():
            up, _ = total(g + eps * d, False)
            dn, _ = total(g - eps * d, False)
        fd.append((up - dn) / (2 * eps))
    spread = abs(fd[0] - fd[1])
    print(f'directional derivative: analytic {analytic:.6f}, central differences {fd[0]:.6f} (eps 4e-3) {fd[1]:.6f} (eps 1.6e-2)')
    assert spread < min(abs(fd[0]), abs(fd[1])), (analytic, fd)
    assert min(fd) - spread <= analytic <= max(fd) + spread, (analytic, fd)
    assert float(bias.grad.abs().max()) > 0
