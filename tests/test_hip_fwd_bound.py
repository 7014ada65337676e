"""The forward feature kernels between the convolutions and the selection stages (RoIAlign, the support-set reductions,
GroupNorm, the average pool, the relation head's cls / reg outputs, the mask logits) alone against the float64 closed
forms of tests/_fwd_ref.py, bounded PER OUTPUT ELEMENT as the backward kernels are in tests/test_hip_train_bwd.py:

    |got - ref| <= c * 2^-24 * mag + 2^-126

``mag`` is that element's own term-magnitude sum, ``c`` the number of fp32 roundings counted in the kernel's arithmetic
(each docstring derives it from the code; first-order counts are rounded up), 2^-126 the smallest normal fp32.  Nothing is
divided by a tensor's range, so a kernel that is wrong only where its output is small fails, and the inputs include the
badly conditioned ones (GroupNorm at mean / std up to 3000, RoI bins that are nearly all outside the map).  A ReLU needs
no exclusion: it is 1-Lipschitz, the bound on the pre-activation carries over.  Every test prints
``[fwd-bound] name: worst |err| / bound`` before it asserts (DESIGN.md section 7.2 carries the table).
"""
import functools

import pytest
import torch

import _fwd_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
TINY = ref.TINY
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bounded(name, got, want, mag, c, slack=None):
    """Assert |got - want| <= c * 2^-24 * mag (+ slack) + 2^-126 for every element (``c``: a number or a tensor that
    broadcasts against the elements); -> the worst ratio."""
    got = got.detach().cpu().to(F64).reshape(want.shape)
    assert bool(torch.isfinite(got).all()), name
    if want.numel() == 0:
        print(f'[fwd-bound] {name}: worst |err| / bound = 0.0000 (empty)')
        return 0.0
    bound = c * U * mag + TINY
    if slack is not None:
        bound = bound + slack
    worst = float(((got - want).abs() / bound).max())
    cmax = int(c.max()) if torch.is_tensor(c) else c
    print(f'[fwd-bound] {name}: worst |err| / bound = {worst:.4f} (c <= {cmax})')
    assert worst <= 1.0, (name, worst)
    return worst


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b.to(torch.float32)))


def _is_pos_zero(t):
    return bool((_bits(t) == 0).all())


# ------------------------------------------------------------------------------------------ RoIAlign
@functools.lru_cache(maxsize=None)
def _fmap(B, H, W, C, seed=5):
    """A map with signed values of mixed magnitude (so that sums cancel and some bins are small)."""
    g = _gen(seed + H * W + C)
    return (torch.randn(B, H, W, C, generator=g) * (0.1 + 3.0 * torch.rand(B, H, W, 1, generator=g))).contiguous()


def _no_contraction():
    """The coordinate slack of the RoIAlign bound is 4 ulps PER CONTRACTED mul+add; csrc/spatial.hip is built with
    -ffp-contract=off (fgn_amd/build.py), so the kernel's coordinates are those of _fwd_ref.roi_geometry bit for bit
    and the slack is 0.  Without that flag the tests would have to pass coord_ulps=4 to the reference."""
    from fgn_amd import build
    assert ('spatial.hip', ['-ffp-contract=off']) in build.SOURCES
    return 0


def _generic_ok(r, case):
    """No generic RoI within 16 ulps of a discontinuity (grid count, validity edge): the share left out is 0."""
    gen = ~case['exact']
    assert bool((r['grid_margin'][gen] >= 16).all()) and bool((r['edge_margin'][gen] >= 16).all()), \
        (r['grid_margin'], r['edge_margin'])


def _roi_c(r):
    """Per-bin rounding count of roi_align_kernel; l = c - lo is exact, h = 1 - l is one rounding.
    Separable body: a weight slot takes at most g non-zero additions (every sample adds to it once; a clamped sample's
    l is exactly 0), the first to 0 exact, + the rounding of h: g per axis.  Row sums: product + nx additions, then
    ``wy * racc`` + ny additions: (nx + 1) + (ny + 1).  Division by the count (1), post_shift (1), rounded up (+1):
      c_sep = gh + gw + ny + nx + 5.
    Per-sample body: each corner weight is a product of two factors with one rounding each (3), times v (1), three
    additions of the four corners (3), the accumulation over the gh * gw samples, division, post_shift, + 1:
      c_smp = gh * gw + 10."""
    return torch.where(r['separable'], r['c_sep'], r['c_smp'])[..., None].to(F64)


def _roi_run(name, fmap, case, post_shift=None, relu=False):
    from fgn_amd import ops
    r = ref.roi_align(fmap, case['rois'], case['P'], case['scale'], case['sr'], case['aligned'], post_shift, relu,
                      coord_ulps=_no_contraction())
    _generic_ok(r, case)
    got = ops.roi_align(fmap.cuda(), case['rois'].cuda(), case['P'], case['scale'], case['sr'], case['aligned'],
                        post_shift=None if post_shift is None else post_shift.cuda(), relu=relu)
    _bounded(name, got, r['val'], r['mag'], _roi_c(r))
    return r, got.cpu()


@pytest.mark.parametrize('name', ['x_sr0', 'x_sr2', 'y_sr0', 'y_sr2'])
def test_roi_align_span_edge_reaches_both_bodies(name):
    """Maps [1,6,300,8] and [1,300,6,8]: bins whose samples span more than MAXS = 32 columns (rows) take the per-sample
    body of roi_align_kernel, which no other test reaches; spans of exactly 32 (separable) and 33 (per-sample) sit on
    the ``n <= MAXS`` edge.  The reference knows the body of every bin: both must occur, and both edge spans."""
    case = ref.roi_span_cases()[name]
    B, H, W = case['shape']
    r, _ = _roi_run(f'roi_align span {name}', _fmap(B, H, W, 8), case)
    sep = r['separable']
    assert bool(sep.any()) and bool((~sep).any())
    spans = set((r['nx'] if name[0] == 'x' else r['ny']).flatten().tolist())
    assert {ref.MAXS, ref.MAXS + 1} <= spans and max(spans) > 40 - 6 * (case['sr'] == 2), spans
    other = r['ny'] if name[0] == 'x' else r['nx']
    assert int(other.max()) <= ref.MAXS


@pytest.mark.parametrize('name', sorted(ref.roi_edge_cases()))
def test_roi_align_map_edges(name):
    """Boxes reaching outside a [2,9,11] map on every side (samples below -1, in [-1, 0], in [size - 1, size], beyond),
    wholly outside (every bin +0.0 bit for bit), of zero and negative extent, below a pixel; exact boxes whose samples
    sit on -1.0 and ``size`` (valid) and one fp32 beyond (no weight), and whose rh / P is an integer."""
    case = ref.roi_edge_cases()[name]
    B, H, W = case['shape']
    fmap = _fmap(B, H, W, 8)
    r, got = _roi_run(f'roi_align edges {name}', fmap, case)
    if name.startswith('generic'):
        assert _is_pos_zero(got[3]) and _is_pos_zero(got[4])            # wholly outside
        assert bool((r['mag'][0] == 0).any()) and bool((r['mag'][0] > 0).any())   # bins with every sample outside, and not
    if name == 'exact_edges':
        for i in range(8):                                              # on the edge: the border pixel; beyond: nothing
            if i % 2:
                assert _is_pos_zero(got[i]), i
            else:
                assert float(r['mag'][i].min()) > 0 and float(got[i].abs().max()) > 0, i
    if name == 'exact_grid':
        assert r['gh'].tolist() == [2, 2] and r['gw'].tolist() == [3, 3]


@pytest.mark.parametrize('C', [4, 64, 512, 1024])
@pytest.mark.parametrize('sr', [0, -1, 2])
@pytest.mark.parametrize('aligned', [True, False])
def test_roi_align_parameter_grid(aligned, sr, C):
    """Map [3,13,17,C] at spatial_scale 1/16, six seeded boxes on all three images (inside and across the border), for
    every (aligned, sampling_ratio) and the thread counts 64 (C = 4, 64), 128 (512) and 256 (1024).  Plain, then with
    post_shift + ReLU, then with the device RoI count (4) below the capacity (6): rows past it keep the bytes of a
    pre-filled buffer."""
    from fgn_amd import ops
    case = ref.roi_grid_case(aligned, sr)
    (B, H, W), rois = case['shape'], case['rois']
    fmap = _fmap(B, H, W, C)
    tag = f'roi_align grid a={int(aligned)} sr={sr} C={C}'
    r, got = _roi_run(tag, fmap, case)
    assert int(rois[:, 0].max()) == B - 1
    shift = torch.randn(C, generator=_gen(C)) * 0.5
    r2, got2 = _roi_run(tag + ' shift+relu', fmap, case, post_shift=shift, relu=True)
    assert float(got2.min()) >= 0.0 and bool((got2 == 0).any()) and bool((got2 > 0).any())
    fill = torch.full((rois.shape[0], 7, 7, C), float('nan')).view(torch.int32).fill_(0x7FC01234).view(torch.float32)
    out = fill.clone().cuda()
    n_dev = torch.tensor([4], dtype=torch.int32, device='cuda')
    ops.roi_align(fmap.cuda(), rois.cuda(), 7, 1.0 / 16, sr, aligned, n_rois_dev=n_dev, out=out)
    assert torch.equal(_bits(out[:4]), _bits(got[:4])) and torch.equal(_bits(out[4:]), _bits(fill[4:]))


@pytest.mark.parametrize('C,C2', [(1024, 512), (64, 32)])
def test_roi_align2_same_bytes_as_two_launches(C, C2):
    """(1024 + 512) / 4 = 384 channel quads take the 192-thread launch, (64 + 32) / 4 = 24 the 64-thread one; the outputs
    are the bytes of the two single launches (which test_roi_align_parameter_grid bounds)."""
    from fgn_amd import ops
    case = ref.roi_grid_case(True, 0)
    (B, H, W), rois = case['shape'], case['rois'].cuda()
    f1, f2 = _fmap(B, H, W, C).cuda(), _fmap(B, H, W, C2, seed=9).cuda()
    shift = (torch.randn(C2, generator=_gen(3)) * 0.5).cuda()
    o1, o2 = ops.roi_align2(f1, f2, rois, 7, 1.0 / 16, 0, True, post_shift2=shift, relu2=True)
    assert torch.equal(_bits(o1), _bits(ops.roi_align(f1, rois, 7, 1.0 / 16, 0, True)))
    assert torch.equal(_bits(o2), _bits(ops.roi_align(f2, rois, 7, 1.0 / 16, 0, True, post_shift=shift, relu=True)))


@pytest.mark.parametrize('H,W', sorted(ref.MASK_ROIS))
def test_roi_align_mask_per_element(H, W):
    """roi_align_mask_kernel: one wave per bin, lanes stride over the gh * gw samples.  Per sample the weight product
    (h is one rounding per axis, the product one: 3; v is 0 or 1, exact), three additions of the corners and the lane's
    accumulation: ceil(gh gw / 64) serial additions; six shuffle levels, the division, + 1:
      c = ceil(gh gw / 64) + 14 on mag = sum w v / count.
    aligned = False, sampling_ratio -1 as the support branch calls it, and aligned = True.  An all-ones mask under a box
    inside the map gives 1 within the bound, an all-zero mask +0.0 bit for bit."""
    from fgn_amd import ops
    rois = torch.tensor(ref.MASK_ROIS[(H, W)], dtype=torch.float32)
    m = (torch.rand(2, H, W, generator=_gen(H)) < 0.6).to(torch.uint8)
    m[:, H // 2:, : W // 3] = 1
    passes = set()
    for aligned in (False, True):
        r = ref.roi_align(m.to(torch.float32), rois, 7, 1.0, -1, aligned)
        _generic_ok(r, dict(exact=torch.zeros(len(rois), dtype=torch.bool)))
        n = (r['gh'].clamp_min(0) * r['gw'].clamp_min(0))
        passes |= set(((n + 63) // 64).tolist())
        c = ((n + 63) // 64 + 14)[:, None, None].to(F64)
        got = ops.roi_align_mask(m.cuda(), rois.cuda(), 7, 1.0, -1, aligned)
        _bounded(f'roi_align_mask {H}x{W} a={int(aligned)}', got, r['val'][..., 0], r['mag'][..., 0], c)
        ones = ops.roi_align_mask(torch.ones_like(m).cuda(), rois.cuda(), 7, 1.0, -1, aligned).cpu()
        inside = 1 if (H, W) == (64, 64) else 0
        assert float((ones[inside].to(F64) - 1.0).abs().max()) <= float(c[inside].max()) * U
        assert _is_pos_zero(ops.roi_align_mask(torch.zeros_like(m).cuda(), rois.cuda(), 7, 1.0, -1, aligned))
    if (H, W) == (64, 64):
        assert 1 in passes and 2 in passes and max(passes) > 16, passes


# ------------------------------------------------------------------------------------------ support reductions
@pytest.mark.parametrize('C', [4, 96, 256, 260, 1024])
@pytest.mark.parametrize('K,P', [(1, 1), (3, 5), (2, 8), (17, 1), (3, 49)])
def test_support_class_vectors_per_element(K, P, C):
    """class_vector_kernel: 16 waves split the K P items (wave w takes items w, w + 16, ...: with K P = 1 and 15 some
    waves have none), lanes own 4 channels; C > 256 takes a second channel slab (260: one quad in it).  Per element the
    product with the weight and ceil(K P / 16) serial additions, the 16 partials in order, 1 / (K P) rounded and the
    product: c = ceil(K P / 16) + 16 + 2 on mag = sum |x w| / (K P).  x = randn: signed terms cancel.  A group whose
    weights are all zero is +0.0 bit for bit."""
    from fgn_amd import ops
    G = 3
    g = _gen(K * P + C)
    x = torch.randn(G * K, P, C, generator=g)
    w = torch.randn(G * K, P, generator=g)
    w[K:2 * K] = 0.0
    c = -(-K * P // 16) + 16 + 2
    for ww in (None, w):
        want, mag = ref.class_vectors(x, ww, G, K)
        got = ops.support_class_vectors(x.cuda(), None if ww is None else ww.cuda(), G, K)
        assert got.shape == (G, C)
        _bounded(f'support_class_vectors K={K} P={P} C={C} w={ww is not None}', got, want, mag, c)
        if ww is not None:
            assert _is_pos_zero(got[1])


@pytest.mark.parametrize('G,K,P,C', [(3, 1, 49, 64), (3, 2, 49, 64), (2, 5, 9, 260), (1, 1, 2049, 1024), (1, 2, 2049, 1024)])
def test_support_kmean_per_element(G, K, P, C):
    """kmean_kernel: K serial additions (the first to 0 is exact), 1 / K rounded and the product: c = K + 1 on
    mag = sum_k |x| / K.  [1, 2049, 1024] is 2049 * 256 float4 of output, one more row than the 2048-block grid covers
    at once: the grid-stride loop."""
    from fgn_amd import ops
    x = torch.randn(G * K, P, C, generator=_gen(K + P))
    want, mag = ref.kmean(x, G, K)
    got = ops.support_kmean(x.cuda(), G, K)
    assert got.shape == (G, P, C)
    _bounded(f'support_kmean G={G} K={K} P={P} C={C}', got, want, mag, K + 1)


@pytest.mark.parametrize('n_in,div,P,C', [(2, 1, 5, 4), (2, 3, 5, 4), (2, 1, 3, 1024), (1, 3, 7, 1024), (1, 3, 1366, 1024),
                                          (0, 3, 5, 4)])
def test_scale_channels_bit_exact(n_in, div, P, C):
    """out[n] = x[n // div] * v[n]: one fp32 product per element, compared bit for bit with the product formed on the
    CPU.  [3, 1366, 1024] is 1 049 088 float4, past the 4096 x 256 lanes of the grid: the grid-stride loop.  An empty
    tensor is an empty result."""
    from fgn_amd import ops
    g = _gen(n_in * div + P)
    x = torch.randn(n_in, P, C, generator=g)
    v = torch.randn(n_in * div, C, generator=g)
    got = ops.scale_channels(x.cuda(), v.cuda(), div)
    want = ref.scale_channels(x, v, div)
    assert got.shape == want.shape == (n_in * div, P, C)
    assert torch.equal(_bits(got), _bits(want))
    print(f'[fwd-bound] scale_channels n_in={n_in} div={div} P={P} C={C}: bit for bit')


# ------------------------------------------------------------------------------------------ GroupNorm, average pool
_GN_SHAPES = [(2, 8, 8, 64, 32), (2, 5, 3, 96, 8), (1, 1, 1, 32, 32), (1, 33, 47, 64, 32), (1, 130, 130, 32, 32),
              (9, 8, 8, 1024, 32)]
GN_C = 10


def _gn_input(n, h, w, c, groups, ratio):
    """randn * 1.3 plus, per (image, group), an offset of +-ratio * 1.3 (mean / std = ratio); ratio None: one constant."""
    g = _gen(h * w + c + (0 if ratio is None else int(ratio * 4)))
    if ratio is None:
        return torch.full((n, h, w, c), 3.7)
    off = (torch.randint(0, 2, (n, 1, 1, groups, 1), generator=g).float() * 2 - 1) * ratio * 1.3
    x = torch.randn(n, h, w, groups, c // groups, generator=g) * 1.3 + off
    return x.reshape(n, h, w, c).contiguous()


def _gn_check(tag, x, gamma, beta, groups, res, relu):
    from fgn_amd import ops
    r = ref.group_norm(x, gamma, beta, groups, 1e-5, res, relu)
    got = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), groups, 1e-5, relu=relu,
                         residual=None if res is None else res.cuda())
    worst = _bounded(tag, got, r['val'], r['mag'], GN_C)
    xin = x.cuda()
    again = ops.group_norm(xin, gamma.cuda(), beta.cuda(), groups, 1e-5, relu=relu,
                           residual=None if res is None else res.cuda(), inplace=True)
    assert again.data_ptr() == xin.data_ptr() and torch.equal(_bits(again), _bits(got))
    return worst


@pytest.mark.parametrize('ratio', [0, 0.25, 30, 1000, 3000, None])
@pytest.mark.parametrize('n,h,w,c,groups', _GN_SHAPES)
def test_group_norm_per_element(n, h, w, c, groups, ratio):
    """y = x sc + (beta - mean sc) (+ residual), sc = rstd gamma, mean and rstd rounded to fp32 from fp64 statistics.
    Roundings, each at most 2^-24 of mag = |gamma| rstd (|x| + mean_grp |x|) + |beta| + |residual|: mean (1, on
    |gamma| rstd |mean|), rstd (1, on |gamma| rstd |x - mean|), sc (1), x sc (1), mean sc (1), beta - mean sc (1), the
    sum (1), the residual (1), the fp64 statistics themselves (shifted sums: below 1), rounded up: c = 10.
    The bound is LINEAR in mean / std, which fp32 sums of raw squares were not (E[x^2] - mean^2 loses (mean / std)^2
    units: before the statistics were formed in fp64 on shifted values, 12 cases failed this test on the MI355X - every
    shape with more than one value per group at mean / std = 1000 (ratios 6.3 .. 108) and 3000 (10.3 .. 855), two
    shapes already at 30 (1.1, 3.2) - DESIGN.md 7.2).  Shapes: C / 4 not dividing the block (96), one value
    per group (variance 0: the output is beta), 49 chunks, the 128-chunk cap with uneven chunks (130 x 130), 1024
    channels.  ratio None: a constant input (variance exactly 0).  Residual and ReLU on and off; the in-place call
    gives the same bytes."""
    x = _gn_input(n, h, w, c, groups, ratio)
    g = _gen(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    res = torch.randn(n, h, w, c, generator=g)
    tag = f'group_norm {(n, h, w, c, groups)} mean/std={ratio}'
    _gn_check(tag, x, gamma, beta, groups, None, False)
    _gn_check(tag + ' res+relu', x, gamma, beta, groups, res, True)


@pytest.mark.parametrize('n,h,w,c', [(1, 1, 5, 32), (2, 17, 17, 256), (1, 2, 2, 4), (1, 1, 1, 4), (1, 1, 8193, 1024)])
def test_avgpool2x2_per_element(n, h, w, c):
    """avgpool2x2_kernel: up to 3 additions (the first to 0 is exact), the count converted exactly, one division, + 1:
    c = 5 on mag = sum |x| over the window / count.  Odd sizes leave partial windows on the last row, the last column
    and the corner (count 2, 2, 1); [1, 1, 8193, 1024] is 4097 * 256 float4 of output, past the 4096-block grid."""
    from fgn_amd import ops
    x = torch.randn(n, h, w, c, generator=_gen(h + w))
    want, mag = ref.avgpool2x2(x)
    got = ops.avgpool2x2(x.cuda())
    assert got.shape == want.shape
    _bounded(f'avgpool2x2 {(n, h, w, c)}', got, want, mag, 5)
    if h % 2 and w % 2:                                     # the corner window holds one pixel: the value itself
        assert _same_bits(got[:, -1, -1], x[:, -1, -1])


# ------------------------------------------------------------------------------------------ relation head, mask logits
REL_WAVES = 4                 # csrc/relation.hip


@functools.lru_cache(maxsize=None)
def _rel_operands(R, N, C):
    g = _gen(31 + R + C)
    B = 3
    q = torch.randn(R, 7, 7, C, generator=g)
    s = torch.randn(B * N, 7, 7, C, generator=g)
    gw = torch.rand(C, generator=g) + 0.5
    gb = torch.randn(C, generator=g) * 0.1
    fcw = torch.randn(6, C, generator=g) * 0.1
    fcb = torch.randn(6, generator=g) * 0.1
    img = torch.tensor([0 if i % 3 == 1 else 2 for i in range(R)]) if R else torch.zeros(0, dtype=torch.long)
    if R > 2:
        img[0], img[R - 1] = 2, 0
    rois = torch.cat([img.float()[:, None], torch.zeros(R, 4)], 1)
    return q, s, rois, gw, gb, fcw, fcb


@pytest.mark.parametrize('R,N,C,groups', [(9, 3, 256, 8), (17, 1, 128, 16), (12, 8, 1024, 32), (5, 5, 96, 3)])
def test_relation_gn_head_outputs_per_element(R, N, C, groups):
    """cls / reg = fc(mean_p relu(GroupNorm(q + s))).  ``pooled`` carries 112 roundings on mag_pooled (DESIGN.md 7.1:
    xhat 96 + 2, 7 + 3 additions, 1 / 49); the channel sum adds a product and 3 additions per lane (4), 3 DPP levels,
    the ``* 1 / 49`` (1), the REL_WAVES partials of a workgroup, the C / 128 chunks in order and the bias (1):
      c = 112 + 4 + 3 + 1 + REL_WAVES + chunks + 1 on mag_j = sum_c mag_pooled_c |fcw_jc| + |b_j|.
    Group widths 32, 8, 32 and 32; (5, 5, 96, 3) leaves the fourth wave of the only workgroup idle; images 0 and 2
    unsorted.  Then the device RoI count below the capacity: the rows past it stay zero, the others keep their bytes."""
    from fgn_amd import ops
    q, s, rois, gw, gb, fcw, fcb = _rel_operands(R, N, C)
    cls_w, reg_w, mag = ref.relation_gn_head(q, s, rois, gw, gb, fcw, fcb, N, groups, 1e-5)
    dev = lambda t: t.cuda().contiguous()
    args = [dev(t) for t in (q, s, rois, gw, gb, fcw, fcb)]
    cls, reg = ops.relation_gn_head(*args, N, groups, 1e-5)
    chunks = -(-(C // 32) // REL_WAVES)
    c = 112 + 4 + 3 + 1 + REL_WAVES + chunks + 1
    tag = f'relation_gn_head R={R} N={N} C={C} groups={groups}'
    _bounded(tag + ' cls', cls, cls_w, mag[:, :2], c)
    _bounded(tag + ' reg', reg, reg_w, mag[:, 2:], c)
    keep = R - 2
    n_dev = torch.tensor([keep], dtype=torch.int32, device='cuda')
    cls2, reg2 = ops.relation_gn_head(*args, N, groups, 1e-5, n_rois_dev=n_dev)
    assert torch.equal(_bits(cls2[:keep * N]), _bits(cls[:keep * N])) and _is_pos_zero(cls2[keep * N:])
    assert torch.equal(_bits(reg2[:keep * N]), _bits(reg[:keep * N])) and _is_pos_zero(reg2[keep * N:])


def test_relation_gn_head_without_rois_is_empty():
    from fgn_amd import ops
    q, s, rois, gw, gb, fcw, fcb = _rel_operands(0, 3, 64)
    cls, reg = ops.relation_gn_head(*[t.cuda().contiguous() for t in (q, s, rois, gw, gb, fcw, fcb)], 3, 8, 1e-5)
    assert cls.shape == (0, 2) and reg.shape == (0, 4)


@pytest.mark.parametrize('C', [4, 64, 256])
@pytest.mark.parametrize('D', [0, 1, 5])
def test_mask_logits_per_element(D, C):
    """logit = sum_c x w + bias on the un-shuffled deconv output [D,7,7,(dy,dx),C]: C products, fewer than C additions
    (4 per lane and trip, six shuffle levels), the bias: c = C + 2 on mag = sum_c |x w| + |b|.  The output index carries
    the pixel shuffle: (2 i + dy, 2 j + dx).  The bias as a float and as a device tensor give the same bytes."""
    from fgn_amd import ops
    g = _gen(D + C)
    x = torch.randn(D, 7, 7, 4 * C, generator=g)
    w = torch.randn(C, generator=g)
    b = 0.37
    want, mag = ref.mask_logits(x, w, b, 7)
    logits, prob = ops.mask_logits(x.cuda(), w.cuda(), b, 7)
    assert logits.shape == prob.shape == (D, 14, 14)
    _bounded(f'mask_logits D={D} C={C}', logits, want, mag, C + 2)
    l2, _ = ops.mask_logits(x.cuda(), w.cuda(), torch.tensor([b], device='cuda'), 7)
    assert torch.equal(_bits(l2), _bits(logits))
