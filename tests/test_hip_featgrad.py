"""The two feature-gradient kernels alone (csrc/train_bwd.hip: ``fgn_roi_align_backward_nhwc_f32``,
``fgn_guidance_backward_f32``) against the float64 closed forms of tests/_featgrad_ref.py, per element:

    |got - ref64| <= c * 2^-24 * mag

with ``c`` counted from the kernel's own operation order, never from a measurement.

RoIAlign backward, one term (RoI r, bin p, q) of an element: wy is a sum of at most 2 gh bilinear weights (h = 1 - l is
one rounding, l is exact), all positive, so it carries at most 2 gh relative roundings; wx likewise 2 gw; then the
product wy * wx, the division by count and the product with dy: 3; then the term is added to the accumulator, and every
later addition rounds the partial sum again: at most ``terms`` more.  c = 2 (gh + gw) + 3 + terms (+ 1 when the result is
added onto a given dx).  Guidance backward: a tap passes through the additions of its list (<= its length), one product
and the additions over the N passes (d_qry: c = longest list + N, + 1 onto a given d_qry) or over the touched pixels of
its image (d_vec: c = longest list + touched pixels).
"""
import numpy as np
import pytest
import torch

import _featgrad_ref as R
import _fwd_ref as FR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _ratio(got, ref, mag, c):
    """Worst |got - ref| / (c u mag) over the elements (c broadcast over the channels); elements of zero magnitude must be
    exactly zero."""
    got = got.detach().cpu().double()
    c = c[..., None] if c.dim() == got.dim() - 1 else c
    zero = mag == 0
    assert bool((got[zero] == 0).all()), 'an element without terms is not zero'
    bound = c * U * mag
    return float(((got - ref).abs()[~zero] / bound.expand_as(mag)[~zero]).max()) if bool((~zero).any()) else 0.0


def _roi_case_run(case, C, seed=0):
    from fgn_amd import ops
    g = torch.Generator().manual_seed(seed)
    B, H, W = case['shape']
    rois, P = case['rois'], case['P']
    dy = torch.randn(rois.shape[0], P, P, C, generator=g)
    ref = R.roi_align_backward(dy, rois, (B, H, W, C), case['scale'], case['sr'], case['aligned'])
    generic = ~case['exact']
    assert bool((ref['grid_margin'][generic] >= 16).all()) and bool((ref['edge_margin'][generic] >= 16).all())
    got = ops.roi_align_backward(dy.cuda(), rois.cuda(), (B, H, W, C), case['scale'], case['sr'], case['aligned'])
    again = ops.roi_align_backward(dy.cuda(), rois.cuda(), (B, H, W, C), case['scale'], case['sr'], case['aligned'])
    assert torch.equal(got, again), 'two runs on the same inputs differ'
    return _ratio(got, ref['val'], ref['mag'], ref['grid'] + 3 + ref['terms']), got, ref, dy


@pytest.mark.parametrize('name', sorted(FR.roi_span_cases()))
def test_roi_align_backward_both_sides_of_the_32_pixel_span(name):
    ratio, _, ref, _ = _roi_case_run(FR.roi_span_cases()[name], 4)
    print(f'{name}: worst error / bound {ratio:.3f}, most terms {int(ref["terms"].max())}')
    assert ratio <= 1.0


@pytest.mark.parametrize('name', sorted(FR.roi_edge_cases()))
def test_roi_align_backward_at_the_edges_of_the_map(name):
    ratio, _, ref, _ = _roi_case_run(FR.roi_edge_cases()[name], 8)
    print(f'{name}: worst error / bound {ratio:.3f}, most terms {int(ref["terms"].max())}')
    assert ratio <= 1.0


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('sr', [0, -1, 2])
@pytest.mark.parametrize('C', [4, 64, 1024])
def test_roi_align_backward_both_flavours(aligned, sr, C):
    ratio, _, ref, _ = _roi_case_run(FR.roi_grid_case(aligned, sr), C)
    print(f'aligned={aligned} sr={sr} C={C}: worst error / bound {ratio:.3f}, most terms {int(ref["terms"].max())}')
    assert ratio <= 1.0


def _overlap_case():
    """Six RoIs of two images, interleaved and overlapping on the same pixels: the order of accumulation matters."""
    rois = [[0, 20.3, 30.7, 150.2, 140.9], [1, 10.4, 12.2, 200.7, 160.3], [0, 40.6, 50.1, 120.8, 180.4],
            [1, 60.2, 20.9, 170.5, 100.6], [0, 30.9, 35.3, 140.1, 150.7], [1, 15.7, 30.2, 190.3, 120.8]]
    return dict(shape=(2, 13, 17), P=7, scale=1.0 / 16, sr=0, aligned=True,
                rois=torch.tensor(rois, dtype=torch.float32), exact=torch.zeros(6, dtype=torch.bool))


def test_roi_align_backward_overlapping_rois_of_two_images():
    case = _overlap_case()
    ratio, got, ref, dy = _roi_case_run(case, 64)
    alone = [R.roi_align_backward(dy[i:i + 1], case['rois'][i:i + 1], got.shape, case['scale'], case['sr'],
                                  case['aligned'])['terms'] > 0 for i in range(6)]
    assert int(sum(a.long() for a in alone).max()) == 3       # some pixels collect from all three RoIs of their image
    print(f'overlap: worst error / bound {ratio:.3f}, most terms {int(ref["terms"].max())}')
    assert ratio <= 1.0


def test_roi_align_backward_accumulates_onto_a_given_map():
    from fgn_amd import ops
    case = _overlap_case()
    _, over, ref, dy = _roi_case_run(case, 64)
    base = torch.randn(over.shape, generator=torch.Generator().manual_seed(3)).cuda()
    out = base.clone()
    res = ops.roi_align_backward(dy.cuda(), case['rois'].cuda(), over.shape, case['scale'], case['sr'], case['aligned'],
                                 out=out, accumulate=True)
    assert res is out
    assert torch.equal(out, base + over)                      # dx + the overwrite result, one rounding per element
    # ... and within the bound of the sum itself
    mag = ref['mag'] + base.cpu().double().abs()
    assert _ratio(out, ref['val'] + base.cpu().double(), mag, ref['grid'] + 4 + ref['terms']) <= 1.0
    # overwrite really overwrites
    again = ops.roi_align_backward(dy.cuda(), case['rois'].cuda(), over.shape, case['scale'], case['sr'], case['aligned'],
                                   out=out, accumulate=False)
    assert torch.equal(again, over)


def test_roi_align_backward_no_roi_empty_boxes_and_bad_channels():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    shape = (2, 9, 11, 8)
    out = torch.full(shape, 7.0, device='cuda')
    ops.roi_align_backward(torch.zeros(0, 7, 7, 8, device='cuda'), torch.zeros(0, 5, device='cuda'), shape, 1.0, 0, True,
                           out=out)
    assert float(out.abs().max()) == 0.0                      # R = 0, overwrite: zero fill
    out.fill_(7.0)
    ops.roi_align_backward(torch.zeros(0, 7, 7, 8, device='cuda'), torch.zeros(0, 5, device='cuda'), shape, 1.0, 0, True,
                           out=out, accumulate=True)
    assert float((out - 7.0).abs().max()) == 0.0              # R = 0, accumulate: untouched
    rois = torch.tensor([[0, 4.3, 3.2, 4.3, 3.2],             # no extent: an empty adaptive grid
                         [1, -20.5, -18.2, -6.3, -5.1],       # wholly outside the map, above and left
                         [1, 15.2, 13.7, 25.8, 22.3]])        # ... below and right
    dy = torch.randn(3, 7, 7, 8, generator=torch.Generator().manual_seed(0))
    for aligned, sr in ((True, 0), (True, 2), (False, -1)):
        ref = R.roi_align_backward(dy[1:], rois[1:], shape, 1.0, sr, aligned)
        assert float(ref['mag'].sum()) == 0.0
        got = ops.roi_align_backward(dy[1:].cuda(), rois[1:].cuda(), shape, 1.0, sr, aligned)
        assert float(got.abs().max()) == 0.0
    got = ops.roi_align_backward(dy[:1].cuda(), rois[:1].cuda(), shape, 1.0, 0, True)
    assert float(got.abs().max()) == 0.0
    with pytest.raises(FgnHipError, match='unsupported shape'):
        ops.roi_align_backward(torch.zeros(1, 7, 7, 6, device='cuda'), rois[:1].cuda(), (2, 9, 11, 6), 1.0, 0, True)


# ------------------------------------------------------------------------------------------ guidance backward
@pytest.mark.parametrize('B,N', [(2, 3), (1, 1)])
@pytest.mark.parametrize('C', [4, 1024])
@pytest.mark.parametrize('kind', ['placed', 'single', 'all'])
def test_guidance_backward_matches_the_closed_form(B, N, C, kind):
    from fgn_amd import ops
    h, w = 8, 10
    gen = torch.Generator().manual_seed(B * 100 + N * 10 + (C > 4))
    g, y, x = R.guidance_rows(B, N, h, w, kind)
    taps = torch.randn(g.size, 9, C, generator=gen)
    qry, vec = torch.randn(B, h, w, C, generator=gen), torch.randn(B * N, C, generator=gen)
    index = ops.guidance_index(g, y, x, B, N, h, w)
    ref = R.guidance_backward(taps, index, qry, vec)
    d_qry, d_vec = ops.guidance_backward(taps.cuda(), index, qry.cuda(), vec.cuda())
    d_qry2, d_vec2 = ops.guidance_backward(taps.cuda(), index, qry.cuda(), vec.cuda())
    assert torch.equal(d_qry, d_qry2) and torch.equal(d_vec, d_vec2), 'two runs on the same inputs differ'
    rq = _ratio(d_qry, ref['d_qry'], ref['mag_qry'], ref['c_qry'])
    rv = _ratio(d_vec, ref['d_vec'], ref['mag_vec'], ref['c_vec'])
    print(f'B={B} N={N} C={C} {kind}: worst error / bound d_qry {rq:.3f} d_vec {rv:.3f}')
    assert rq <= 1.0 and rv <= 1.0
    untouched = (ref['c_qry'] == 0)
    assert float(d_qry.cpu()[untouched].abs().sum()) == 0.0                # accumulate = 0: zero where nothing arrives
    if kind != 'all':
        assert bool(untouched.any())
    # accumulate = 1: added onto the touched pixels, as it was elsewhere
    base = torch.randn(B, h, w, C, generator=gen).cuda()
    out = base.clone()
    res, d_vec3 = ops.guidance_backward(taps.cuda(), index, qry.cuda(), vec.cuda(), out=out, accumulate=True)
    assert res is out and torch.equal(d_vec3, d_vec)
    assert torch.equal(out.cpu()[untouched], base.cpu()[untouched])
    assert torch.equal(out, base + d_qry)
    mag = ref['mag_qry'] + base.cpu().double().abs()
    assert _ratio(out, ref['d_qry'] + base.cpu().double(), mag, ref['c_qry'] + 1) <= 1.0


def test_guidance_backward_without_active_rows_and_with_a_bad_index():
    from fgn_amd import ops
    from fgn_amd.lib import FgnHipError
    B, N, h, w, C = 2, 3, 8, 10, 8
    qry, vec = torch.randn(B, h, w, C).cuda(), torch.randn(B * N, C).cuda()
    index = ops.guidance_index([], [], [], B, N, h, w)
    d_qry, d_vec = ops.guidance_backward(torch.zeros(0, 9, C, device='cuda'), index, qry, vec)
    assert float(d_qry.abs().max()) == 0.0 and float(d_vec.abs().max()) == 0.0
    index = ops.guidance_index([0, 4], [1, 2], [1, 2], B, N, h, w)
    with pytest.raises(FgnHipError, match='index'):                         # an entry past the last tap row
        ops.guidance_backward(torch.zeros(1, 9, C, device='cuda'), index, qry, vec)
    bad = dict(index, pix=index['pix'] + B * h * w)
    with pytest.raises(FgnHipError, match='index'):                         # a pixel past the map
        ops.guidance_backward(torch.zeros(2, 9, C, device='cuda'), bad, qry, vec)
