"""The float64 closed forms of tests/_featgrad_ref.py pinned to independent implementations, and the host-side index
builder ``ops.guidance_index`` against a brute-force enumeration (CPU only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _featgrad_ref as R
import _fwd_ref as FR
from fgn_amd import ops


def _cases():
    out = dict(FR.roi_span_cases())
    out.update(FR.roi_edge_cases())
    for aligned in (True, False):
        for sr in (0, -1, 2):
            out[f'grid_a{int(aligned)}_sr{sr}'] = FR.roi_grid_case(aligned, sr)
    return out


CASES = _cases()


def _operands(case, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, H, W = case['shape']
    rois, P = case['rois'], case['P']
    return torch.randn(B, H, W, C, generator=g), torch.randn(rois.shape[0], P, P, C, generator=g)


@pytest.mark.parametrize('name', sorted(CASES))
def test_roi_align_backward_is_the_adjoint_of_the_forward_form(name):
    """<roi_align(x), dy> = <x, roi_align_backward(dy)> in float64, with the forward closed form of _fwd_ref."""
    case = CASES[name]
    x, dy = _operands(case, 4)
    fwd = FR.roi_align(x, case['rois'], case['P'], case['scale'], case['sr'], case['aligned'])['val']
    bwd = R.roi_align_backward(dy, case['rois'], x.shape, case['scale'], case['sr'], case['aligned'])
    lhs, rhs = float((fwd * dy.double()).sum()), float((x.double() * bwd['val']).sum())
    scale = float((fwd.abs() * dy.double().abs()).sum()) + 1e-300
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)
    # generic boxes stay 16 ulps clear of every discontinuity: no case is left out of the kernel tests
    generic = ~case['exact']
    assert bool((bwd['grid_margin'][generic] >= 16).all()) and bool((bwd['edge_margin'][generic] >= 16).all())
    # a pixel that receives something receives at least one term, and nothing is larger than its magnitude sum
    assert bool((bwd['val'].abs() <= bwd['mag'] * (1 + 1e-12) + 1e-300).all())
    assert bool(((bwd['mag'].sum(-1) > 0) <= (bwd['terms'] > 0)).all())


@pytest.mark.parametrize('name', ['generic_a1_sr0', 'generic_a0_sr2', 'grid_a1_sr0', 'grid_a0_sr-1', 'grid_a1_sr2', 'exact_grid'])
def test_roi_align_backward_matches_autograd_of_the_oracle(name):
    """oracle.fgn_ref_cpu.roi_align indexes the map with torch ops: torch.autograd differentiates it (fp32)."""
    from oracle import fgn_ref_cpu as O
    case = CASES[name]
    x, dy = _operands(case, 4, seed=1)
    leaf = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = O.roi_align(leaf, case['rois'].numpy(), case['P'], case['scale'], case['sr'], case['aligned'])   # [R,C,P,P]
    out.backward(dy.permute(0, 3, 1, 2).contiguous())
    ref = leaf.grad.permute(0, 2, 3, 1).double()
    got = R.roi_align_backward(dy, case['rois'], x.shape, case['scale'], case['sr'], case['aligned'])
    assert float(ref.abs().max()) > 0
    err = (got['val'] - ref).abs()
    assert bool((err <= 64 * 2.0 ** -24 * got['mag'] + 1e-30).all()), float((err / (got['mag'] + 1e-30)).max())


def test_roi_align_backward_of_no_roi_and_of_empty_boxes_is_zero():
    dy = torch.randn(3, 7, 7, 4)
    rois = torch.tensor([[0, 4.3, 3.2, 4.3, 3.2],            # no extent (aligned: an empty adaptive grid)
                         [1, -20.5, -18.2, -6.3, -5.1],      # wholly outside the map
                         [1, 15.2, 13.7, 25.8, 22.3]])
    got = R.roi_align_backward(dy, rois, (2, 9, 11, 4), 1.0, 0, True)
    assert float(got['mag'].sum()) == 0.0 and float(got['terms'].sum()) == 0.0
    got = R.roi_align_backward(dy[:0], rois[:0], (2, 9, 11, 4), 1.0, 0, True)
    assert float(got['val'].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ guidance
@pytest.mark.parametrize('B,N', [(2, 3), (1, 1)])
@pytest.mark.parametrize('kind', ['placed', 'single', 'all'])
def test_guidance_index_matches_brute_force(B, N, kind):
    h, w = 8, 10
    g, y, x = R.guidance_rows(B, N, h, w, kind)
    ix = ops.guidance_index(g, y, x, B, N, h, w)
    table = R.guidance_index_brute(g, y, x, B, N, h, w)
    pix = sorted({p for p, _ in table})
    assert ix['pix'].tolist() == pix and all(v.dtype == np.int32 for v in ix.values())
    assert ix['seg'].size == len(pix) * N + 1 and ix['seg'][0] == 0 and ix['seg'][-1] == ix['ent'].size
    for t, p in enumerate(pix):
        for n in range(N):
            got = ix['ent'][ix['seg'][t * N + n]:ix['seg'][t * N + n + 1]].tolist()
            assert got == table.get((p, n), []), (p, n)
    assert ix['ent'].size == sum(len(v) for v in table.values())
    for b in range(B):
        assert [p for p in pix if p // (h * w) == b] == ix['pix'][ix['img_seg'][b]:ix['img_seg'][b + 1]].tolist()
    if kind == 'placed':
        # corners keep 4 of their 9 taps; adjacent rows share pixels; two passes meet at one pixel
        n_taps = np.bincount(ix['ent'] // 9, minlength=g.size)
        assert n_taps[:4].tolist() == [4, 4, 4, 4] and n_taps[4:6].tolist() == [9, 9]
        assert table[((0 * h + 3) * w + 4, 0)] == [4 * 9 + 4, 5 * 9 + 3]     # its own centre tap, its neighbour's left tap
        if N > 1:
            p = (0 * h + 5) * w + 2
            assert len(table[(p, 0)]) == 1 and len(table[(p, 1)]) == 1
    if kind == 'all':
        assert len(pix) == B * h * w and max(len(v) for v in table.values()) == 9


def test_guidance_index_refuses_rows_outside_the_map():
    with pytest.raises(ValueError):
        ops.guidance_index([0], [8], [0], 1, 1, 8, 10)
    with pytest.raises(ValueError):
        ops.guidance_index([3], [0], [0], 1, 3, 8, 10)
    empty = ops.guidance_index([], [], [], 2, 3, 8, 10)
    assert empty['pix'].size == 0 and empty['seg'].tolist() == [0] and empty['img_seg'].tolist() == [0, 0, 0]


@pytest.mark.parametrize('B,N', [(2, 3), (1, 1)])
@pytest.mark.parametrize('kind', ['placed', 'single', 'all'])
def test_guidance_backward_matches_autograd(B, N, kind):
    """The sparse route (taps = dpre x W, index, gather) against torch.autograd through
    (qry[:, None] * vec) -> conv2d(padding=1) with the dense dpre, in float64."""
    h, w, C, Cf = 8, 10, 4, 5
    gen = torch.Generator().manual_seed(B * 10 + N)
    g, y, x = R.guidance_rows(B, N, h, w, kind)
    qry = torch.randn(B, h, w, C, generator=gen, dtype=torch.float64)
    vec = torch.randn(B * N, C, generator=gen, dtype=torch.float64)
    Wc = torch.randn(Cf, C, 3, 3, generator=gen, dtype=torch.float64)
    dpre_rows = torch.randn(g.size, Cf, generator=gen, dtype=torch.float64)
    dpre = torch.zeros(B * N, Cf, h, w, dtype=torch.float64)
    dpre[torch.from_numpy(g), :, torch.from_numpy(y), torch.from_numpy(x)] = dpre_rows
    ql, vl = qry.clone().requires_grad_(True), vec.clone().requires_grad_(True)
    guided = (ql.permute(0, 3, 1, 2)[:, None] * vl.view(B, N, C, 1, 1)).reshape(B * N, C, h, w)
    F.conv2d(guided, Wc, padding=1).backward(dpre)
    taps = (dpre_rows @ Wc.permute(0, 2, 3, 1).reshape(Cf, 9 * C)).view(-1, 9, C)
    got = R.guidance_backward(taps, ops.guidance_index(g, y, x, B, N, h, w), qry, vec)
    for name, ref in (('d_qry', ql.grad), ('d_vec', vl.grad)):
        assert float(ref.abs().max()) > 0
        err = (got[name] - ref).abs()
        mag = got['mag_qry' if name == 'd_qry' else 'mag_vec']
        assert bool((err <= 1e-12 * mag + 1e-300).all()), (name, float(err.max()))
    # untouched pixels carry nothing
    untouched = got['c_qry'] == 0
    assert float(got['mag_qry'][untouched].sum()) == 0.0
