"""tests/_mask_ref.py checked without a GPU: the model's constants against mask.hip, the float32 restatement of the paste
sample against the same formula in float64 (inside the derived ``paste_bound``) and against the oracle's grid_sample paste
(every pixel outside the bound - and no pixel of the generic cases lies inside it), exact three-way agreement where
every float32 operation is exact (on-threshold pixels included), the existence of samples a few floats to either side of
the threshold in the rounded families (what makes bit equality on the GPU a real statement), every case builder against
the route it claims, the band of the whole-image semantic against the whole image, and the oracle's RLE encoder against
the product's on every model mask."""
import functools

import numpy as np
import pytest
import torch

import _mask_ref as ref
from fgn_amd import rle
from oracle import fgn_ref_cpu as O

F32 = np.float32
GENERIC, EXACT, ROUNDED = ref.generic_cases(), ref.exact_cases(), ref.rounded_cases()
GEOMETRY, LAYOUT, RLE_ROUTES = ref.geometry_cases(), ref.layout_cases(), ref.rle_route_cases()
OVERLAP, SRC = ref.overlap_cases(), ref.src_cases()


def test_model_constants_equal_the_sources():
    c = ref.source_constants()
    for k in ('RLE_THREADS', 'OVL_ROWS', 'OVL_THREADS', 'BITS_ROWS', 'DENSE_SEGS', 'DENSE_THREADS', 'SRC_MAX_DIM',
              'PASTE_THREADS', 'PASTE_GRID_CAP'):
        assert c[k] == getattr(ref, k), k
    assert c['LDS_MASK'] == [ref.LDS_MASK] and c['n_lds'] == 4          # both RLE and both overlap kernels
    assert c['MASK_SIZE_MAX'] == [ref.LDS_MASK] and c['n_size_tests'] == 4


@functools.lru_cache(maxsize=None)
def _oracle(family: str, name: str, thr: float, skip_empty: bool) -> np.ndarray:
    c = {'generic': GENERIC, 'exact': EXACT, 'rounded': ROUNDED}[family][name]
    return O.paste_masks(torch.from_numpy(c.prob)[:, None], c.boxes, c.H, c.W, thr, skip_empty=skip_empty)


def _three_way(c, family, thr, skip_empty):
    """Per detection: model mask, float64 mask, oracle mask, |s32 - s64|, bound, |s64 - thr| on the evaluated region."""
    want = _oracle(family, c.name, thr, skip_empty)
    for d in range(c.D):
        mask, s32, (x0, y0, x1, y1) = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, thr, skip_empty)
        assert O.rle_encode(mask) == rle.encode(mask)
        s64 = ref.sample64(c.prob[d], c.boxes[d], c.H, c.W)
        m64 = np.zeros_like(mask)
        m64[y0:y1, x0:x1] = s64[y0:y1, x0:x1] >= np.float64(F32(thr))
        sl = (slice(y0, y1), slice(x0, x1))
        yield d, mask, m64, want[d], np.abs(s32[sl].astype(np.float64) - s64[sl]), \
            ref.paste_bound(c.prob[d], c.boxes[d], c.H, c.W)[sl], np.abs(s64[sl] - np.float64(F32(thr))), sl


@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('name', sorted(GENERIC))
def test_generic_model_equals_fp64_and_the_oracle_and_no_pixel_lies_inside_the_bound(name, skip_empty):
    c = GENERIC[name]
    worst, pixels = 0.0, 0
    for thr in c.thrs:
        for d, mask, m64, want, err, bound, dist, sl in _three_way(c, 'generic', thr, skip_empty):
            assert (err <= bound).all(), (thr, d, float((err / bound).max()))
            worst = max(worst, float((err / bound).max())) if err.size else worst
            pixels += err.size
            assert np.count_nonzero(dist <= bound) == 0, (thr, d, 'a sample lies inside the bound: choose another seed')
            assert np.array_equal(mask, m64), (thr, d)
            assert np.array_equal(mask, want), (thr, d)
    print(f'[mask model {name} skip_empty={skip_empty}] {pixels} samples, worst |s32 - s64| / bound = {worst:.3f}, '
          f'0 samples inside the bound')
    assert 0 < worst <= 1


@pytest.mark.parametrize('skip_empty', [True, False])
@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_cases_agree_three_ways_on_every_pixel_with_on_threshold_pixels(name, skip_empty):
    c = EXACT[name]
    for thr in c.thrs:
        on_thr = 0
        for d, mask, m64, want, err, bound, dist, sl in _three_way(c, 'exact', thr, skip_empty):
            assert err.max() == 0, (thr, d, 'an operation of the float32 sample was not exact')
            on_thr += int(np.count_nonzero(dist == 0))
            assert np.array_equal(mask, m64) and np.array_equal(mask, want), (thr, d)
            assert mask[sl][dist == 0].all()                     # >= : a sample on the threshold is set
        print(f'[mask model {name} thr={thr} skip_empty={skip_empty}] {on_thr} on-threshold pixels, ratio 0')
        assert on_thr > 0, (thr, 'no on-threshold pixel')


@pytest.mark.parametrize('name', sorted(ROUNDED))
def test_rounded_cases_have_samples_within_four_ulps_on_both_sides_of_the_threshold(name):
    c = ROUNDED[name]
    thr = F32(c.thrs[0])
    ulp = np.spacing(thr)
    total = np.zeros(3, int)
    for d in range(c.D):
        mask, s32, (x0, y0, x1, y1) = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, thr, True)
        s = s32[y0:y1, x0:x1].astype(np.float64)
        near = np.abs(s - thr) <= 4 * ulp
        below, on, above = int((near & (s < thr)).sum()), int((s == thr).sum()), int((near & (s > thr)).sum())
        print(f'[mask model {name} det {d}] within 4 ulps of {thr}: {below} below, {on} on, {above} above')
        total += (below, on, above)
        # fp64 and the bound: the model is right wherever float64 can tell
        s64 = ref.sample64(c.prob[d], c.boxes[d], c.H, c.W)[y0:y1, x0:x1]
        bound = ref.paste_bound(c.prob[d], c.boxes[d], c.H, c.W)[y0:y1, x0:x1]
        assert (np.abs(s - s64) <= bound).all()
        clear = np.abs(s64 - thr) > bound
        assert np.array_equal(mask[y0:y1, x0:x1][clear], (s64 >= thr)[clear])
        # one float above the threshold the on-threshold pixels clear
        up = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, np.nextafter(thr, F32(1)), True)[0]
        assert int(mask.sum()) - int(up.sum()) >= on
    assert (total > 0).all(), total


# ---------------------------------------------------------------------------------------------- band, encoders
def _all_paste_cases():
    for fam in (GENERIC, EXACT, ROUNDED, GEOMETRY, LAYOUT, RLE_ROUTES):
        for c in fam.values():
            yield c
    for c, _ in OVERLAP.values():
        yield c


@pytest.mark.parametrize('c', list(_all_paste_cases()), ids=lambda c: c.name)
def test_band_of_the_whole_image_semantic_cuts_no_set_pixel_and_the_encoders_agree(c):
    for thr in c.thrs:
        for d in range(c.D):
            band = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, thr, False)[0]
            whole = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, thr, False, whole_image=True)[0]
            assert np.array_equal(band, whole), (thr, d)
            assert O.rle_encode(band) == rle.encode(band)
            win = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, thr, True)[0]
            assert O.rle_encode(win) == rle.encode(win)
            assert not (win & ~whole).any()                       # the CPU window only ever cuts


def test_geometry_cases_hold_what_they_are_named_for():
    c = GEOMETRY['geometry-m14']
    k = ref.GEOMETRY_NAMES.index
    m = lambda name, thr, se: ref.paste_model(c.prob[k(name)], c.boxes[k(name)], c.H, c.W, thr, se)
    assert m('inside', 0.5, True)[0].sum() > 0 and m('out-left-top', 0.5, True)[0][0, 0]
    for name in ('beyond-left', 'beyond-right', 'beyond-top', 'beyond-bottom', 'inverted', 'inverted-x'):
        x0, y0, x1, y1 = m(name, 0.5, True)[2]
        assert not (x0 < x1 and y0 < y1), name                    # empty region
    assert np.isnan(m('zero-width-on-centre', 0.5, False)[1][6:29, 10]).all()       # 0 / 0 -> NaN sample, not set
    assert not m('zero-width-on-centre', 0.5, False)[0][:, 10].any()
    assert m('zero-width', 0.5, False)[2][0::2] == (0, c.W)                          # the whole axis
    assert m('zero-both', 0.3, False)[2] == (0, 0, c.W, c.H)
    assert m('inside', 0.0, False)[0].all() and m('inside', -0.5, False)[0].all()    # thr <= 0: the whole image
    assert not m('inside', 0.0, True)[0].all()
    assert not m('inside', 1.5, False)[0].any() and not m('full-image', 1.5, True)[0].any()
    x0, y0, x1, y1 = m('very-wide', 0.5, False)[2]
    assert (x0, y0, x1, y1) == (0, 0, c.W, c.H)
    assert m('sub-pixel', 0.3, True)[0].sum() <= 1


# ---------------------------------------------------------------------------------------------- routes
def test_layout_cases_pack_two_detections_into_one_lane_and_store_a_byte_tail():
    for c in LAYOUT.values():
        r = ref.paste_route(c.D, c.H, c.W)
        assert r['straddle'] > 0 and r['tail'] and r['passes'] == 1, (c.name, r)
    c = ref.large_paste_case()
    r = ref.paste_route(c.D, c.H, c.W)
    assert r['grid'] == ref.PASTE_GRID_CAP and r['passes'] == 2, r
    assert c.boxes[2, 1] - 1 >= c.claims['second_pass_from_row']          # its whole region is second-pass work
    assert ref.paste_model(c.prob[2], c.boxes[2], c.H, c.W, 0.5, True)[0].sum() > 1000


@pytest.mark.parametrize('name', sorted(RLE_ROUTES))
def test_rle_case_reaches_the_route_it_claims(name):
    c = RLE_ROUTES[name]
    hit = {k: False for k in c.claims}
    for d in range(c.D):
        mask, _, region = ref.paste_model(c.prob[d], c.boxes[d], c.H, c.W, c.thrs[0], True)
        r = ref.rle_route(mask, region, c.H, c.W)
        for k, v in c.claims.items():
            if k == 'runs':
                hit[k] |= r['runs'][:len(v)] == v
            elif k == 'first_run_above':
                hit[k] |= r['first_run'] > v
            else:
                hit[k] |= r[k] == v
    assert all(hit.values()), hit


def test_string_cases_cover_the_character_count_edges():
    """Encoded values (the first three runs, then deltas against the run two back) at the edges of 1 / 2 / 3 characters."""
    seen = set()
    for name, c in RLE_ROUTES.items():
        if not name.startswith('string-'):
            continue
        runs = ref.run_lengths(ref.paste_model(c.prob[0], c.boxes[0], c.H, c.W, 0.5, True)[0])
        seen |= {r - (runs[i - 2] if i > 2 else 0) for i, r in enumerate(runs)}
    assert {-17, -16, -1, 0, 15, 16, 31, 32, 1023, 1024} <= seen, sorted(seen)


@pytest.mark.parametrize('name', sorted(OVERLAP))
def test_overlap_case_reaches_the_route_it_claims(name):
    c, G = OVERLAP[name]
    routes = [ref.overlap_route(ref.paste_region(c.boxes[d], c.H, c.W, c.MS, 0.5, True), G) for d in range(c.D)]
    for d, blocks in c.claims.get('blocks', {}).items():
        assert routes[d]['blocks'] == blocks, (d, routes[d])
    for d, x0 in c.claims.get('x0', {}).items():
        reg = ref.paste_region(c.boxes[d], c.H, c.W, c.MS, 0.5, True)
        assert reg[0] == x0 and reg[2] == c.claims['x1'] and routes[d]['words'][-1] == 1, (d, reg)
    for d in c.claims.get('empty', []):
        assert routes[d]['empty'] and not routes[d - 1]['empty']
    assert routes[0]['passes'] == -(-G // 64)


def test_overlap_sizes_cover_the_seams():
    sizes = [(c.H, c.W, G) for n, (c, G) in OVERLAP.items() if n.startswith('size-')]
    assert {w for _, w, _ in sizes} >= {1, 63, 64, 65, 129}
    assert {h for h, _, _ in sizes} >= {1, 7, 8, 9, 33}
    assert {g for _, _, g in sizes} >= {1, 64, 65, 129}
    g = ref.gt_masks_for(9, 65, 129)
    assert g[0, :, 63:].all() and g[1, :, 64].all() and not g[1, :, :64].any() and g[2].all() and not g[3].any()


def test_dense_sizes_reach_every_branch_of_the_walk():
    r = {hw: ref.dense_route(*hw) for hw in ref.DENSE_SIZES}
    assert {v['cpc'] for v in r.values()} >= {1, 2, 64, 65}
    assert all((v['branch'] == 'dx0') == (hw[0] > 1024) for hw, v in r.items())
    assert all(v['segs'] < ref.DENSE_SEGS for v in r.values())                        # segments without a chunk
    # the (column, chunk) advance is used from the second step of a wave on: more than 8192 chunks
    assert r[(1025, 130)]['steps'] == 2 and r[(1025, 130)]['branch'] == 'dx0' and r[(1025, 130)]['dk'] == 64
    assert r[(1024, 130)]['steps'] == 2 and r[(1024, 130)]['dx'] == 1 and r[(1024, 130)]['dk'] == 0
    assert all(v['steps'] == 1 for hw, v in r.items() if hw[1] <= 70)


def test_source_cases_hold_the_sizes_and_scales_they_claim():
    c, net, sizes = SRC['scales']
    assert float(F32(net[1] / sizes[0][1])) != net[1] / sizes[0][1] and float(F32(net[0] / sizes[0][0])) != net[0] / sizes[0][0]
    assert len(set(sizes)) == len(sizes) == 2 and c.D == 2 * 3
    c, net, sizes = SRC['limits']
    assert {1, 16384, 16385} <= {v for s in sizes for v in s}
    assert (ref.box_to_source_model(c.boxes[0], (16385, 2), net) == 0).all()
    b = ref.box_to_source_model([10.5, 7.25, 50, 40], (333, 500), (800, 1333))
    assert b.dtype == F32 and b[0] == F32(10.5) / F32(1333 / 500) and b[3] == F32(40) / F32(800 / 333)
