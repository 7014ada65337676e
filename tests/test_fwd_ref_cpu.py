"""The float64 closed forms of tests/_fwd_ref.py pinned to independent implementations (no GPU), and the RoI cases of
tests/test_hip_fwd_bound.py checked for what they are meant to reach: were a closed form wrong, the per-element bounds
of the GPU tests would hold the kernels to the wrong function."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fwd_ref as ref
from oracle import fgn_ref_cpu as O

F64 = torch.float64
U = ref.U


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _all_roi_cases():
    cases = dict(ref.roi_span_cases())
    cases.update(ref.roi_edge_cases())
    for (aligned, sr) in ref.ROI_GRID_SEEDS:
        cases[f'grid_a{int(aligned)}_sr{sr}'] = ref.roi_grid_case(aligned, sr)
    return cases


_CASES = _all_roi_cases()


@pytest.mark.parametrize('name', sorted(_CASES))
def test_roi_align_matches_the_oracle_within_its_fp32_error(name):
    """oracle.fgn_ref_cpu.roi_align forms the same fp32 coordinates and sums the samples in fp32: per sample 3 roundings
    of the corner weight, the product, the corners' additions and a sum over gh * gw samples, the division: its error is
    at most (gh gw + 10) 2^-24 mag.  An RoI whose grid is empty on one axis is zero in both."""
    c = _CASES[name]
    B, H, W = c['shape']
    f = torch.randn(B, H, W, 4, generator=_gen(3)) * (0.1 + 3 * torch.rand(B, H, W, 1, generator=_gen(4)))
    r = ref.roi_align(f, c['rois'], c['P'], c['scale'], c['sr'], c['aligned'])
    want = O.roi_align(f.permute(0, 3, 1, 2).contiguous(), c['rois'].numpy(), c['P'], c['scale'], c['sr'], c['aligned'])
    want = want.permute(0, 2, 3, 1).to(F64)
    cnt = (r['gh'].clamp_min(0) * r['gw'].clamp_min(0) + 10)[:, None, None, None].to(F64)
    assert bool(((r['val'] - want).abs() <= cnt * U * r['mag'] + ref.TINY).all())
    assert bool((r['val'].abs() <= r['mag'] * (1 + 1e-12)).all())
    # post_shift and ReLU are applied after the division
    sh = torch.randn(4, generator=_gen(5))
    r2 = ref.roi_align(f, c['rois'], c['P'], c['scale'], c['sr'], c['aligned'], post_shift=sh, relu=True)
    assert torch.equal(r2['val'], (r['val'] + sh.to(F64)).clamp_min(0)) and torch.equal(r2['mag'], r['mag'] + sh.to(F64).abs())


def test_roi_cases_reach_what_they_are_for():
    """Spans of 32, 33 and beyond and both kernel bodies in every span case; every generic RoI 16 ulps or more from a
    grid-count or validity discontinuity (the share of RoIs left out of the GPU tests is 0); the exact RoIs on them."""
    for name, c in _CASES.items():
        B, H, W = c['shape']
        r = ref.roi_align(torch.zeros(B, H, W, 4), c['rois'], c['P'], c['scale'], c['sr'], c['aligned'])
        gen = ~c['exact']
        assert bool((r['grid_margin'][gen] >= 16).all()) and bool((r['edge_margin'][gen] >= 16).all()), name
    for name, c in ref.roi_span_cases().items():
        B, H, W = c['shape']
        r = ref.roi_align(torch.zeros(B, H, W, 4), c['rois'], c['P'], c['scale'], c['sr'], c['aligned'])
        long_, short = (r['nx'], r['ny']) if name[0] == 'x' else (r['ny'], r['nx'])
        assert {32, 33} <= set(long_.flatten().tolist()) and int(long_.max()) > 34 and int(short.max()) <= 32
        assert bool(r['separable'].any()) and bool((~r['separable']).any())
    e = ref.roi_edge_cases()
    B, H, W = e['exact_edges']['shape']
    r = ref.roi_align(torch.ones(B, H, W, 4), e['exact_edges']['rois'], 1, 1.0, 1, False)
    assert r['edge_margin'].tolist() == [0.0, 1.0] * 4                       # on the edge, one fp32 beyond
    assert r['val'][:, 0, 0, 0].tolist() == [1.0, 0.0] * 4                   # valid (the border pixel) / no weight
    r = ref.roi_align(torch.ones(B, H, W, 4), e['exact_grid']['rois'], 2, 1.0, 0, False)
    assert r['grid_margin'].tolist() == [0.0, 0.0] and r['gh'].tolist() == [2, 2] and r['gw'].tolist() == [3, 3]
    for (H, W), rois in ref.MASK_ROIS.items():
        for aligned in (False, True):
            r = ref.roi_align(torch.zeros(2, H, W), torch.tensor(rois), 7, 1.0, -1, aligned)
            assert bool((r['grid_margin'] >= 16).all()) and bool((r['edge_margin'] >= 16).all()), (H, W, aligned)
    r = ref.roi_align(torch.zeros(2, 64, 64), torch.tensor(ref.MASK_ROIS[(64, 64)]), 7, 1.0, -1, False)
    n = (r['gh'] * r['gw']).tolist()
    assert n[0] == 1 and 64 < n[1] <= 128 and n[2] > 1024


def test_roi_coordinate_slack_covers_a_moved_coordinate():
    """``slack`` (coord_ulps = 4) bounds what happens when every coordinate moves by up to 4 ulps of the largest one:
    boxes shifted by 1 and 2 ulps of their largest coordinate change no generic bin by more than the slack.  A constant
    map has no slack."""
    c = ref.roi_span_cases()['x_sr0']
    B, H, W = c['shape']
    f = torch.randn(B, H, W, 4, generator=_gen(8))
    keep = ~c['exact']
    rois = c['rois'][keep]
    r = ref.roi_align(f, rois, c['P'], c['scale'], c['sr'], c['aligned'], coord_ulps=4)
    assert float(r['slack'].min()) > 0
    for k in (1, 2):
        moved = rois.clone()
        step = torch.from_numpy(np.spacing(rois[:, 1:].abs().max(dim=1).values.numpy()))
        moved[:, 1:] += k * step[:, None]
        r2 = ref.roi_align(f, moved, c['P'], c['scale'], c['sr'], c['aligned'])
        assert torch.equal(r2['gw'], r['gw']) and torch.equal(r2['gh'], r['gh'])
        assert bool(((r2['val'] - r['val']).abs() <= r['slack'] + 1e-12 * r['mag']).all())
    flat = ref.roi_align(torch.full((B, H, W, 4), 2.5), rois, c['P'], c['scale'], c['sr'], c['aligned'], coord_ulps=4)
    assert float(flat['slack'].max()) == 0.0


@pytest.mark.parametrize('n,h,w,c,groups', [(2, 8, 8, 64, 32), (2, 5, 3, 96, 8), (2, 1, 1, 32, 32)])
def test_group_norm_matches_torch_float64(n, h, w, c, groups):
    g = _gen(c)
    x = torch.randn(n, h, w, c, generator=g) * 1.3 + 40.0
    gamma, beta, res = torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(n, h, w, c, generator=g)
    eps = ref.f32(1e-5)
    want = F.group_norm(x.to(F64).permute(0, 3, 1, 2), groups, gamma.to(F64), beta.to(F64), eps).permute(0, 2, 3, 1)
    r = ref.group_norm(x, gamma, beta, groups, 1e-5)
    assert bool(((r['val'] - want).abs() <= 1e-12 * r['mag']).all())
    r2 = ref.group_norm(x, gamma, beta, groups, 1e-5, residual=res, relu=True)
    assert bool(((r2['val'] - F.relu(want + res.to(F64))).abs() <= 1e-12 * r2['mag']).all())
    assert bool((r['val'].abs() <= r['mag'] * (1 + 1e-12)).all())
    assert torch.allclose(r2['mag'], r['mag'] + res.to(F64).abs(), rtol=1e-14, atol=0)


@pytest.mark.parametrize('n,h,w,c', [(1, 1, 5, 32), (2, 17, 17, 8), (1, 2, 2, 4), (1, 1, 1, 4), (1, 6, 9, 4)])
def test_avgpool2x2_matches_torch_float64(n, h, w, c):
    x = torch.randn(n, h, w, c, generator=_gen(h * w))
    want = F.avg_pool2d(x.to(F64).permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    val, mag = ref.avgpool2x2(x)
    assert val.shape == want.shape and bool(((val - want).abs() <= 1e-15 * mag).all())
    wa = F.avg_pool2d(x.to(F64).abs().permute(0, 3, 1, 2), 2, 2, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
    assert bool(((mag - wa).abs() <= 1e-15 * mag).all())


def test_support_reductions_match_plain_einsums():
    g = _gen(2)
    G, K, P, C = 3, 4, 6, 8
    x = torch.randn(G * K, P, C, generator=g)
    w = torch.randn(G * K, P, generator=g)
    x5, w4 = x.to(F64).view(G, K, P, C), w.to(F64).view(G, K, P)
    val, mag = ref.class_vectors(x, w, G, K)
    assert torch.allclose(val, torch.einsum('gkpc,gkp->gc', x5, w4) / (K * P), rtol=1e-13, atol=1e-15)
    assert torch.allclose(mag, torch.einsum('gkpc,gkp->gc', x5.abs(), w4.abs()) / (K * P), rtol=1e-13, atol=0)
    val, mag = ref.class_vectors(x, None, G, K)
    assert torch.allclose(val, torch.einsum('gkpc->gc', x5) / (K * P), rtol=1e-13, atol=1e-15)
    val, mag = ref.kmean(x, G, K)
    assert torch.allclose(val, torch.einsum('gkpc->gpc', x5) / K, rtol=1e-13, atol=1e-15)
    assert torch.allclose(mag, torch.einsum('gkpc->gpc', x5.abs()) / K, rtol=1e-13, atol=0)
    v = torch.randn(G * K * 3, C, generator=g)
    sc = ref.scale_channels(x, v, 3)
    assert sc.dtype == torch.float32 and sc.shape == (G * K * 3, P, C)
    for n in (0, 4, 35):
        assert torch.equal(sc[n], x[n // 3] * v[n][None, :])
    assert ref.scale_channels(x[:0], v[:0], 3).shape == (0, P, C)


@pytest.mark.parametrize('R,N,C,groups', [(5, 3, 64, 8), (4, 1, 32, 1), (3, 2, 96, 3)])
def test_relation_outputs_match_the_oracle_in_float64(R, N, C, groups):
    """oracle.relation concatenates (RoI, class mean) and runs the shared 1x1 conv; with the weight [I | I] and no bias
    that conv is q + s, then GroupNorm, ReLU, the average pool and the two linear layers, all in float64."""
    g = _gen(R + C)
    B = 2
    q = torch.randn(R, 7, 7, C, generator=g)
    s = torch.randn(B * N, 7, 7, C, generator=g)
    gw, gb = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.3
    fcw, fcb = torch.randn(6, C, generator=g), torch.randn(6, generator=g)
    img = torch.arange(R) % B
    rois = torch.cat([img.float()[:, None], torch.zeros(R, 4)], 1)
    eye = torch.eye(C, dtype=F64)
    sd = {'roi_head.cls_reg_shared_conv.weight': torch.cat([eye, eye], 1)[:, :, None, None],
          'roi_head.cls_reg_shared_conv.bias': torch.zeros(C, dtype=F64),
          'roi_head.cls_reg_shared_conv_norm.weight': gw.to(F64), 'roi_head.cls_reg_shared_conv_norm.bias': gb.to(F64),
          'roi_head.bbox_head.fc_cls.weight': fcw[:2].to(F64), 'roi_head.bbox_head.fc_cls.bias': fcb[:2].to(F64),
          'roi_head.bbox_head.fc_reg.weight': fcw[2:].to(F64), 'roi_head.bbox_head.fc_reg.bias': fcb[2:].to(F64)}
    cfg = {'roi_head': {'relation': {'gn_groups': groups, 'gn_eps': ref.f32(1e-5)}}}
    feats = q.to(F64).permute(0, 3, 1, 2)
    cat_mean = s.to(F64).permute(0, 3, 1, 2).reshape(B, N, C, 7, 7)
    y = O.relation(feats, rois.numpy(), cat_mean, sd, cfg, N)
    cls_w, reg_w = O.bbox_head_forward(y, sd)
    cls, reg, mag = ref.relation_gn_head(q, s, rois, gw, gb, fcw, fcb, N, groups, 1e-5)
    assert bool(((cls - cls_w).abs() <= 1e-12 * mag[:, :2]).all()) and bool(((reg - reg_w).abs() <= 1e-12 * mag[:, 2:]).all())
    assert bool((torch.cat([cls, reg], 1).abs() <= mag * (1 + 1e-12)).all())


def test_mask_logits_match_a_loop_over_sub_positions():
    g = _gen(6)
    D, P, C = 3, 7, 8
    x = torch.randn(D, P, P, 4 * C, generator=g)
    w = torch.randn(C, generator=g)
    val, mag = ref.mask_logits(x, w, 0.37, P)
    want = torch.zeros(D, 2 * P, 2 * P, dtype=F64)
    wa = torch.zeros_like(want)
    for dy in range(2):
        for dx in range(2):
            sub = x.to(F64)[..., (2 * dy + dx) * C:(2 * dy + dx + 1) * C]
            want[:, dy::2, dx::2] = sub @ w.to(F64) + ref.f32(0.37)
            wa[:, dy::2, dx::2] = sub.abs() @ w.to(F64).abs() + ref.f32(0.37)
    assert torch.allclose(val, want, rtol=1e-13, atol=1e-14) and torch.allclose(mag, wa, rtol=1e-13, atol=0)
    assert ref.mask_logits(x[:0], w, 0.37, P)[0].shape == (0, 14, 14)
