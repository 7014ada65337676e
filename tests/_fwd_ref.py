"""Closed-form float64 restatements of the forward feature kernels between the convolutions and the selection stages
(csrc/spatial.hip, csrc/norm.hip, csrc/relation.hip, csrc/mask.hip; CPU, float64).

As in tests/_bwd_ref.py every function takes the operands of its ``ops.*`` wrapper in the same NHWC layouts (fp32
tensors on any device) and returns float64 tensors: the value and, for every output element, its TERM-MAGNITUDE SUM
``mag`` (the same expression with every term replaced by its absolute value).  tests/test_hip_fwd_bound.py bounds every
element by ``c * 2^-24 * mag``; tests/test_fwd_ref_cpu.py pins every closed form to an independent implementation.
Scalars the C ABI carries as ``float`` (spatial_scale, eps, the mask bias) are rounded to fp32 first.
"""
import numpy as np
import torch

from _bwd_ref import F64, TINY, U, d, f32, relation_gn_head_backward, ulp32  # noqa: F401  (re-exported to the tests)

F32 = np.float32
MAXS = 32                 # roi_align_kernel: longest row / column weight vector of the separable body


# ------------------------------------------------------------------------------------------ RoIAlign
def _axis(coord, size):
    """axis_sample of csrc/spatial.hip on fp32 coordinates -> (lo, hi, l, h, valid); l is the kernel's own fp32
    difference (exact: coord and lo are less than 1 apart), h = 1 - l in float64 (the kernel rounds it: 1 rounding)."""
    coord = np.asarray(coord, dtype=F32)
    valid = ~((coord < F32(-1.0)) | (coord > F32(size)))
    c = np.where(coord <= 0, F32(0), coord).astype(F32)
    lo = c.astype(np.int64)
    clamp = lo >= size - 1
    lo = np.where(clamp, size - 1, lo)
    hi = np.where(clamp, size - 1, lo + 1)
    c = np.where(clamp, lo.astype(F32), c)
    l = (c - lo.astype(F32)).astype(F32).astype(np.float64)
    return lo, hi, l, 1.0 - l, valid


def roi_geometry(roi, P, spatial_scale, sampling_ratio, aligned, H, W):
    """The fp32 coordinate arithmetic of one RoI in the kernel's operation order (the order of
    oracle.fgn_ref_cpu.roi_align; csrc/spatial.hip is built without mul+add contraction, so these are the kernel's own
    coordinates bit for bit) -> dict: gh, gw, count, ys [P, gh], xs [P, gw] (fp32), rh_over_p, rw_over_p (the fp32
    quotients the adaptive grid takes the ceiling of), coord_max (largest magnitude entering a coordinate expression)."""
    scale = F32(spatial_scale)
    off = F32(0.5) if aligned else F32(0.0)
    x1, y1, x2, y2 = (F32(F32(roi[i]) * scale) - off for i in (1, 2, 3, 4))
    rw, rh = F32(x2 - x1), F32(y2 - y1)
    if not aligned:
        rw, rh = max(rw, F32(1.0)), max(rh, F32(1.0))
    bin_h, bin_w = F32(rh / F32(P)), F32(rw / F32(P))
    gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bin_h))
    gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bin_w))

    def coords(start, step, g):
        if g <= 0:
            return np.zeros((P, 0), dtype=F32)
        p = np.arange(P, dtype=F32)[:, None]
        i = np.arange(g, dtype=F32)[None, :]
        base = (start + (p * step).astype(F32)).astype(F32)
        return (base + (((i + F32(0.5)).astype(F32) * step).astype(F32) / F32(g)).astype(F32)).astype(F32)

    ys, xs = coords(y1, bin_h, gh), coords(x1, bin_w, gw)
    cmax = max([abs(float(v)) for v in (x1, y1, x2, y2)] + [float(np.abs(a).max()) for a in (ys, xs) if a.size] + [1.0])
    return dict(gh=gh, gw=gw, count=max(gh * gw, 1), ys=ys, xs=xs, rh_over_p=float(bin_h), rw_over_p=float(bin_w),
                coord_max=cmax, adaptive=sampling_ratio <= 0)


def roi_margins(geo, H, W):
    """-> (grid, edge) in fp32 ulps: how far rh / P and rw / P are from an integer (adaptive grids only, else inf) and
    how far the nearest sample coordinate is from the validity edges -1 and ``size``.  The "generic" RoIs of the tests
    keep both above 16, so that no rounding of a coordinate can change a grid count or a sample's validity."""
    grid = float('inf')
    if geo['adaptive']:
        for q in (geo['rh_over_p'], geo['rw_over_p']):
            if q > 0:
                grid = min(grid, abs(q - round(q)) / float(np.spacing(F32(max(abs(q), 1.0)))))
    edge = float('inf')
    for a, size in ((geo['ys'], H), (geo['xs'], W)):
        for e in (-1.0, float(size)):
            if a.size:
                dist = np.abs(a.astype(np.float64) - e)
                edge = min(edge, float((dist / np.spacing(np.maximum(np.abs(a), F32(1.0))).astype(np.float64)).min()))
    return grid, edge


def _axis_weights(coords, size):
    """coords [P, g] -> W [P, size] float64 (bilinear row weights of the valid samples, summed per bin),
    N [P, size] (number of valid samples of the bin between rows k and k + 1), first / n [P]: the span
    [lo of the first sample, hi of the last] the separable body of the kernel walks."""
    P, g = coords.shape
    Wt = np.zeros((P, size))
    Nt = np.zeros((P, size))
    first = np.zeros(P, dtype=np.int64)
    n = np.zeros(P, dtype=np.int64)
    if g == 0:
        return Wt, Nt, first, n
    lo, hi, l, h, valid = _axis(coords, size)
    for p in range(P):
        np.add.at(Wt[p], lo[p][valid[p]], h[p][valid[p]])
        np.add.at(Wt[p], hi[p][valid[p]], l[p][valid[p]])
        between = valid[p] & (hi[p] != lo[p])
        np.add.at(Nt[p], lo[p][between], 1.0)
    first = np.minimum(lo[:, 0], lo[:, -1])              # (a negative extent under a fixed grid runs downwards)
    n = np.maximum(hi[:, 0], hi[:, -1]) - first + 1
    return Wt, Nt, first, n


def roi_align(fmap, rois, P, spatial_scale, sampling_ratio, aligned, post_shift=None, relu=False, coord_ulps=0):
    """fmap [B,H,W,C] fp32 (or a [B,H,W] mask of 0 / 1), rois [R,5] -> dict of float64 [R,P,P,C] tensors and per-bin facts:
      val   = relu?(sum over the valid samples and their 4 corners of w v / count + post_shift), weights, sums and the
              division in float64 on the fp32 coordinates of ``roi_geometry``
      mag   = sum w |v| / count + |post_shift|
      slack = sum over the samples of (delta |d_y v| + delta |d_x v|) / count, delta = ``coord_ulps`` ulps of the RoI's
              largest coordinate magnitude, |d_y v| <= the x-interpolated |v(hi) - v(lo)|: what a coordinate that is
              ``coord_ulps`` off can move a sample by (bilinear interpolation is continuous); 0 for coord_ulps = 0
      separable [R,P,P] bool: the body of roi_align_kernel the bin takes;  ny, nx [R,P]: its spans;  gh, gw [R]
      c_sep, c_smp [R,P,P]: the rounding counts of the two bodies (tests/test_hip_fwd_bound.py derives them)
      grid_margin, edge_margin [R]: ``roi_margins``."""
    f = d(fmap)
    if f.dim() == 3:
        f = f[..., None]
    B, H, W, C = f.shape
    fa = f.abs()
    rois_np = rois.detach().cpu().numpy().astype(F32)
    R = rois_np.shape[0]
    val, mag, slack = (torch.zeros(R, P, P, C, dtype=F64) for _ in range(3))
    sep = torch.zeros(R, P, P, dtype=torch.bool)
    ny_t, nx_t = torch.zeros(R, P, dtype=torch.long), torch.zeros(R, P, dtype=torch.long)
    gh_t, gw_t = torch.zeros(R, dtype=torch.long), torch.zeros(R, dtype=torch.long)
    gm, em = torch.zeros(R, dtype=F64), torch.zeros(R, dtype=F64)
    gy = torch.zeros_like(f)
    gy[:, :-1] = (f[:, 1:] - f[:, :-1]).abs()
    gx = torch.zeros_like(f)
    gx[:, :, :-1] = (f[:, :, 1:] - f[:, :, :-1]).abs()
    for r in range(R):
        b = int(rois_np[r, 0])
        geo = roi_geometry(rois_np[r], P, spatial_scale, sampling_ratio, aligned, H, W)
        WY, NY, _, ny = _axis_weights(geo['ys'], H)
        WX, NX, _, nx = _axis_weights(geo['xs'], W)
        if geo['gh'] <= 0 or geo['gw'] <= 0:          # an empty grid has no samples on either axis
            WY[:], WX[:], NY[:], NX[:] = 0.0, 0.0, 0.0, 0.0
        WY, WX, NY, NX = (torch.from_numpy(a) for a in (WY, WX, NY, NX))
        val[r] = torch.einsum('py,qx,yxc->pqc', WY, WX, f[b]) / geo['count']
        mag[r] = torch.einsum('py,qx,yxc->pqc', WY, WX, fa[b]) / geo['count']
        if coord_ulps:
            delta = coord_ulps * float(np.spacing(F32(geo['coord_max'])))
            slack[r] = delta * (torch.einsum('py,qx,yxc->pqc', NY, WX, gy[b]) +
                                torch.einsum('py,qx,yxc->pqc', WY, NX, gx[b])) / geo['count']
        ny_t[r], nx_t[r] = torch.from_numpy(ny), torch.from_numpy(nx)
        sep[r] = (ny_t[r] <= MAXS)[:, None] & (nx_t[r] <= MAXS)[None, :]
        gh_t[r], gw_t[r] = geo['gh'], geo['gw']
        gm[r], em[r] = roi_margins(geo, H, W)
    if post_shift is not None:
        ps = d(post_shift).view(1, 1, 1, C)
        val, mag = val + ps, mag + ps.abs()
    if relu:
        val = val.clamp_min(0.0)
    g_h, g_w = gh_t.clamp_min(0)[:, None, None], gw_t.clamp_min(0)[:, None, None]
    c_sep = g_h + g_w + ny_t.clamp_min(0)[:, :, None] + nx_t.clamp_min(0)[:, None, :] + 5
    c_smp = g_h * g_w + 10
    return dict(val=val, mag=mag, slack=slack, separable=sep, ny=ny_t, nx=nx_t, gh=gh_t, gw=gw_t, c_sep=c_sep,
                c_smp=c_smp, grid_margin=gm, edge_margin=em)


# ------------------------------------------------------------------------------------------ support reductions
def class_vectors(x, w, n_groups: int, k: int):
    """x [n_groups*k, P.., C], w [n_groups*k, P..] or None -> (val, mag) [n_groups, C]: mean over (k, P) of x w."""
    x = d(x)
    C = x.shape[-1]
    x = x.reshape(n_groups, -1, C)
    t = x if w is None else x * d(w).reshape(n_groups, -1, 1)
    kp = x.shape[1]
    return t.sum(dim=1) / kp, t.abs().sum(dim=1) / kp


def kmean(x, n_groups: int, k: int):
    """x [n_groups*k, ...] -> (val, mag) [n_groups, ...]: mean over the k shots."""
    x = d(x)
    x = x.reshape((n_groups, k) + tuple(x.shape[1:]))
    return x.sum(dim=1) / k, x.abs().sum(dim=1) / k


def scale_channels(x, v, div: int):
    """x [n_in, ..., C], v [n_in*div, C] -> fp32 [n_in*div, ..., C]: the ONE fp32 product the kernel forms."""
    x32, v32 = x.detach().cpu().float(), v.detach().cpu().float()
    n_out, C = v32.shape
    idx = torch.arange(n_out) // div
    return x32[idx] * v32.view((n_out,) + (1,) * (x32.dim() - 2) + (C,))


# ------------------------------------------------------------------------------------------ GroupNorm, average pool
def group_norm(x, gamma, beta, groups: int, eps: float, residual=None, relu: bool = False):
    """x [n,H,W,C] -> dict(val, mag, mean, rstd), two-pass float64:
      val = relu?(gamma (x - mean) rstd + beta + residual), statistics over (H, W, C / groups) of one image
      mag = |gamma| rstd (|x| + mean_grp |x|) + |beta| + |residual|
    (x - mean is a difference: its fp32 error scales with |x| + |mean|, not with the difference)."""
    x, ga, be = d(x), d(gamma), d(beta)
    n, H, W, C = x.shape
    cpg = C // groups
    xg = x.reshape(n, H * W, groups, cpg)
    grp = lambda t: t.mean(dim=(1, 3), keepdim=True)
    mean = grp(xg)
    var = grp((xg - mean) ** 2)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    ga_, be_ = ga.view(1, 1, groups, cpg), be.view(1, 1, groups, cpg)
    val = (ga_ * (xg - mean) * rstd + be_).reshape(n, H, W, C)
    mag = (ga_.abs() * rstd * (xg.abs() + grp(xg.abs())) + be_.abs()).reshape(n, H, W, C)
    if residual is not None:
        val, mag = val + d(residual), mag + d(residual).abs()
    if relu:
        val = val.clamp_min(0.0)
    return dict(val=val, mag=mag, mean=mean.reshape(n, groups), rstd=rstd.reshape(n, groups))


def avgpool2x2(x):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) over NHWC -> (val, mag = sum |x| over the window / count)."""
    x = d(x)
    n, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    s, a, cnt = torch.zeros(n, Ho, Wo, C, dtype=F64), torch.zeros(n, Ho, Wo, C, dtype=F64), torch.zeros(1, Ho, Wo, 1, dtype=F64)
    for ky in range(2):
        for kx in range(2):
            t = x[:, ky::2, kx::2]
            s[:, :t.shape[1], :t.shape[2]] += t
            a[:, :t.shape[1], :t.shape[2]] += t.abs()
            cnt[:, :t.shape[1], :t.shape[2]] += 1.0
    return s / cnt, a / cnt


# ------------------------------------------------------------------------------------------ relation head, mask logits
def relation_gn_head(q, s, rois, gn_w, gn_b, fc_w, fc_b, n_ways: int, gn_groups: int, eps: float):
    """-> (cls [R*N,2], reg [R*N,4], mag [R*N,6]): ``pooled`` and ``mag_pooled`` of
    _bwd_ref.relation_gn_head_backward, then out_j = sum_c pooled_c fcw_jc + b_j in float64,
    mag_j = sum_c mag_pooled_c |fcw_jc| + |b_j|."""
    R, C = q.shape[0], q.shape[-1]
    fw, fb = d(fc_w), d(fc_b)
    r = relation_gn_head_backward(q, s, rois, gn_w, gn_b, fc_w, torch.zeros(R * n_ways, 6), n_ways, gn_groups, eps)
    out = r['pooled'].reshape(R * n_ways, C) @ fw.t() + fb
    mag = r['mag_pooled'].reshape(R * n_ways, C) @ fw.abs().t() + fb.abs()
    return out[:, :2], out[:, 2:], mag


def mask_logits(x, w, bias: float, roi_size: int):
    """x [D,P,P,4*C] (sub-position major: channel = sub*C + c, sub = 2*dy + dx), w [C] -> (logits, mag) [D,2P,2P]:
    logit[d, 2i+dy, 2j+dx] = sum_c x[d,i,j,sub,c] w[c] + bias;  mag = sum_c |x w| + |bias|."""
    D, P = x.shape[0], roi_size
    w_ = d(w)
    C = w_.numel()
    t = d(x).reshape(D, P, P, 2, 2, C) * w_
    b = f32(bias)
    shuffle = lambda u: u.permute(0, 1, 3, 2, 4).reshape(D, 2 * P, 2 * P)      # [D,i,j,dy,dx] -> [D,(i,dy),(j,dx)]
    return shuffle(t.sum(dim=-1)) + b, shuffle(t.abs().sum(dim=-1)) + abs(b)


# ------------------------------------------------------------------------------------------ RoI cases of the tests
# Shared by tests/test_fwd_ref_cpu.py (which asserts on the CPU what each case reaches: spans, bodies, margins) and
# tests/test_hip_fwd_bound.py.  Each case: dict(shape = map [B,H,W], P, scale, sr, aligned, rois [R,5], exact [R] bool).
# "Exact" RoIs have coordinate arithmetic that is exact in fp32 and may sit on a discontinuity; every other RoI is
# "generic" and must keep 16 ulps from every discontinuity (``roi_margins``).
def _case(shape, P, scale, sr, aligned, generic, exact=()):
    rois = torch.tensor(list(generic) + list(exact), dtype=torch.float32).reshape(-1, 5)
    flags = torch.tensor([False] * len(generic) + [True] * len(exact), dtype=torch.bool)
    return dict(shape=shape, P=P, scale=scale, sr=sr, aligned=aligned, rois=rois, exact=flags)


def _swap(case):
    """The same case with x and y exchanged (map and boxes)."""
    B, H, W = case['shape']
    r = case['rois']
    return dict(case, shape=(B, W, H), rois=r[:, [0, 2, 1, 4, 3]].contiguous())


def roi_span_cases():
    """Map [1,6,300]: bins wider than MAXS pixels in x (the per-sample body), narrow in y.  sr = 0: bins of 41.1 px
    (nx = 43), of 31.3 px (nx = 32 .. 34 with the bin's phase), of 8.7 px (separable) and the exact 32 px bin (grid
    count exactly 32, nx = 33).  sr = 2 (P = 4): the span is bin / 2 + 2: bins of 66.2, 61.1, 20.4 px and the exact 60
    and 62 px bins (nx = 32, 33).  Then both with x and y exchanged."""
    a = _case((1, 6, 300), 7, 1.0, 0, True,
              [[0, 5.3, 0.7, 293.1, 5.1], [0, 40.37, 1.2, 259.67, 4.9], [0, 100.3, 0.4, 160.9, 5.2]],
              [[0, 16, 0, 240, 3.5]])
    b = _case((1, 6, 300), 4, 1.0, 2, True,
              [[0, 10.3, 0.6, 275.1, 5.0], [0, 20.2, 0.6, 264.6, 5.0], [0, 100.3, 0.4, 181.9, 5.2]],
              [[0, 16, 0, 256, 4], [0, 16, 0, 264, 4]])
    return {'x_sr0': a, 'x_sr2': b, 'y_sr0': _swap(a), 'y_sr2': _swap(b)}


def roi_edge_cases():
    """Map [2,9,11].  Generic boxes reaching outside the map on every side, on two sides, wholly outside (rows 3, 4:
    every bin +0.0), of zero and negative extent, below a pixel; for both ``aligned`` values and sr in {0, 2}.  Exact
    boxes (P = 1, one sample per bin, aligned = False so that the zero extent is clamped to exactly 1): the sample at
    exactly -1.0 and exactly ``size`` (valid) and at the next fp32 beyond each (no weight), per axis; P = 2 boxes whose
    rh / P and rw / P are the integers 2 and 3 (grid counts exactly 2 and 3)."""
    generic = [[1, -3.3, -2.7, 14.6, 12.2], [0, -5.2, -4.1, 4.3, 3.7], [1, 6.4, 5.3, 17.9, 15.2],
               [0, -20.5, -18.2, -6.3, -5.1], [1, 15.2, 13.7, 25.8, 22.3],
               [0, 4.3, 3.2, 4.3, 3.2], [1, 7.6, 6.1, 3.2, 2.4], [0, 5.21, 4.33, 5.47, 4.71]]
    out = {}
    for aligned in (True, False):
        for sr in (0, 2):
            out[f'generic_a{int(aligned)}_sr{sr}'] = _case((2, 9, 11), 7, 1.0, sr, aligned, generic)
    nxt = lambda v, to: float(np.nextafter(F32(v), F32(to)))
    ex = []
    for x in (-1.5, nxt(-1.5, -9), 10.5, nxt(10.5, 99)):          # W = 11: samples at -1, just below, 11, just above
        ex.append([1, x, 3.25, x, 3.25])
    for y in (-1.5, nxt(-1.5, -9), 8.5, nxt(8.5, 99)):            # H = 9
        ex.append([0, 4.25, y, 4.25, y])
    out['exact_edges'] = _case((2, 9, 11), 1, 1.0, 1, False, [], ex)
    out['exact_grid'] = _case((2, 9, 11), 2, 1.0, 0, False, [], [[0, 1, 1, 7, 5], [1, 2, 0, 8, 4]])
    out['exact_scale16'] = _case((2, 9, 11), 2, 1.0 / 16, 0, False, [], [[1, 16, 32, 112, 96], [0, 0, 16, 128, 144]])
    return out


def roi_grid_rois(seed: int, B: int, H: int, W: int, scale: float, R: int = 6):
    """R seeded boxes of mixed sizes inside and across the border of a [B,H,W] map, in image coordinates."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(R, 4, generator=g)
    cx, cy = (u[:, 0] * 1.2 - 0.1) * W, (u[:, 1] * 1.2 - 0.1) * H
    w, h = (0.05 + u[:, 2] ** 2) * W, (0.05 + u[:, 3] ** 2) * H
    b = torch.arange(R) % B
    rois = torch.stack([b.float(), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1) / scale
    rois[:, 0] = b.float()
    return rois.float().contiguous()


ROI_GRID_SEEDS = {(True, 0): 1, (True, -1): 2, (True, 2): 3, (False, 0): 4, (False, -1): 5, (False, 2): 6}


def roi_grid_case(aligned: bool, sr: int):
    """Map [3,13,17] at spatial_scale 1/16, six seeded generic boxes on all three images."""
    B, H, W = 3, 13, 17
    rois = roi_grid_rois(ROI_GRID_SEEDS[(aligned, sr)], B, H, W, 1.0 / 16)
    return dict(shape=(B, H, W), P=7, scale=1.0 / 16, sr=sr, aligned=aligned, rois=rois,
                exact=torch.zeros(rois.shape[0], dtype=torch.bool))


# boxes of the roi_align_mask tests, per mask size (H, W); two masks, P = 7, spatial_scale 1.0, sampling_ratio -1
MASK_ROIS = {
    (64, 64): [[0, 10.2, 11.3, 14.1, 15.9],            # grid 1 x 1
               [1, 3.2, 5.1, 60.3, 62.7],              # 9 x 9 = 81 samples: two passes of the 64 lanes
               [0, -80.3, -90.2, 150.4, 160.1],        # 36 x 33 = 1188 samples: 19 passes, most samples outside
               [1, 20.4, -7.7, 75.2, 30.9]],
    (7, 130): [[0, 2.3, 0.4, 127.9, 6.3],              # 1 x 18
               [1, -30.6, -2.2, 160.8, 9.1],           # 2 x 28
               [0, 60.2, 2.1, 61.1, 2.9]],
}
