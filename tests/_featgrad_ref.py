"""Closed-form float64 restatements of the two feature-gradient kernels of fgn_amd/csrc/train_bwd.hip (CPU):
``fgn_roi_align_backward_nhwc_f32`` and ``fgn_guidance_backward_f32`` (bounds in DESIGN 7.9).

As in tests/_bwd_ref.py and tests/_fwd_ref.py every function takes the operands of its ``ops.*`` wrapper in the same
NHWC layouts and returns float64 tensors: the value, the TERM-MAGNITUDE SUM ``mag`` of every element (the same sum with
every term replaced by its absolute value) and the number of terms, from which tests/test_hip_featgrad.py counts the
roundings ``c`` of its bound ``c * 2^-24 * mag``.  tests/test_featgrad_ref_cpu.py pins both forms to torch.autograd.

RoIAlign backward stands on ``_fwd_ref.roi_geometry`` / ``_axis_weights``: the sample coordinates are the kernel's own
fp32 values (bit for bit), the bilinear weights, their sums and the division by the sample count are float64.
"""
import numpy as np
import torch

from _fwd_ref import F64, _axis_weights, d, roi_geometry, roi_margins


def roi_align_backward(dy, rois, fmap_shape, spatial_scale, sampling_ratio, aligned):
    """dy [R,P,P,C], rois [R,5] -> dict of float64:
      val, mag [B,H,W,C]:  val[b,y,x,c] = sum over the RoIs r of image b and their bins (p,q) of
                           WY_r[p,y] WX_r[q,x] dy[r,p,q,c] / count_r  (WY / WX: ``_axis_weights``), mag with |dy|
      terms [B,H,W]:       the number of (r,p,q) with a non-zero weight at the pixel - the additions of the kernel
      grid [B,H,W]:        the largest 2 (gh + gw) among the RoIs that reach the pixel (weight roundings, see the test)
      grid_margin, edge_margin [R]: ``_fwd_ref.roi_margins`` of every RoI."""
    B, H, W, C = (int(v) for v in fmap_shape)
    g = d(dy)
    R, P = g.shape[0], g.shape[1]
    rois_np = rois.detach().cpu().numpy().astype(np.float32).reshape(R, 5)
    val, mag = torch.zeros(B, H, W, C, dtype=F64), torch.zeros(B, H, W, C, dtype=F64)
    terms, grid = torch.zeros(B, H, W, dtype=F64), torch.zeros(B, H, W, dtype=F64)
    gm, em = torch.zeros(R, dtype=F64), torch.zeros(R, dtype=F64)
    for r in range(R):
        b = int(rois_np[r, 0])
        geo = roi_geometry(rois_np[r], P, spatial_scale, sampling_ratio, aligned, H, W)
        gm[r], em[r] = roi_margins(geo, H, W)
        if geo['gh'] <= 0 or geo['gw'] <= 0 or not 0 <= b < B:
            continue
        WY, WX = (torch.from_numpy(_axis_weights(c_, n_)[0]) for c_, n_ in ((geo['ys'], H), (geo['xs'], W)))
        val[b] += torch.einsum('py,qx,pqc->yxc', WY, WX, g[r]) / geo['count']
        mag[b] += torch.einsum('py,qx,pqc->yxc', WY, WX, g[r].abs()) / geo['count']
        hit = torch.einsum('py,qx->yx', (WY != 0).to(F64), (WX != 0).to(F64))
        terms[b] += hit
        grid[b] = torch.maximum(grid[b], (hit > 0).to(F64) * 2.0 * (geo['gh'] + geo['gw']))
    return dict(val=val, mag=mag, terms=terms, grid=grid, grid_margin=gm, edge_margin=em)


def guidance_index_brute(g, y, x, batch, n_ways, h, w):
    """``ops.guidance_index`` by plain enumeration: {(pixel, pass): [row*9 + tap, ...]} in ascending entry order."""
    table = {}
    for r, (gi, yi, xi) in enumerate(zip(g, y, x)):
        for tap in range(9):
            ty, tx = int(yi) + tap // 3 - 1, int(xi) + tap % 3 - 1
            if 0 <= ty < h and 0 <= tx < w:
                table.setdefault((((int(gi) // n_ways) * h + ty) * w + tx, int(gi) % n_ways), []).append(r * 9 + tap)
    return table


def guidance_backward(taps, index, qry_fmap, vec):
    """taps [rows,9,C], index = ``ops.guidance_index``, qry_fmap [B,h,w,C], vec [B*N,C] -> dict of float64:
      d_qry, mag_qry [B,h,w,C]: sum_n vec[bN+n] dG_n,  dG_n = the listed taps of pass n at the pixel
      c_qry [B,h,w]:            roundings of an element: the longest tap list of the pixel + N (product and additions)
      d_vec, mag_vec [B*N,C]:   sum over the touched pixels of image b of qry_fmap dG_n
      c_vec [B*N]:              the longest tap list among them + the number of touched pixels of the image."""
    T, q, v = d(taps), d(qry_fmap), d(vec)
    B, h, w, C = q.shape
    N = v.shape[0] // B
    T2, q2 = T.reshape(-1, C), q.reshape(-1, C)
    pix, seg, ent = (np.asarray(index[k], dtype=np.int64) for k in ('pix', 'seg', 'ent'))
    d_qry, mag_qry = torch.zeros(B * h * w, C, dtype=F64), torch.zeros(B * h * w, C, dtype=F64)
    c_qry = torch.zeros(B * h * w, dtype=F64)
    d_vec, mag_vec, c_vec = torch.zeros(B * N, C, dtype=F64), torch.zeros(B * N, C, dtype=F64), torch.zeros(B * N, dtype=F64)
    longest = np.zeros(B * N)
    for t, p in enumerate(pix):
        b = int(p) // (h * w)
        for n in range(N):
            e = ent[seg[t * N + n]:seg[t * N + n + 1]]
            dg, ag = T2[e].sum(0), T2[e].abs().sum(0)
            d_qry[p] += v[b * N + n] * dg
            mag_qry[p] += v[b * N + n].abs() * ag
            d_vec[b * N + n] += q2[p] * dg
            mag_vec[b * N + n] += q2[p].abs() * ag
            c_qry[p] = max(float(c_qry[p]), float(e.size))
            longest[b * N + n] = max(longest[b * N + n], e.size)
        c_qry[p] += N
    touched = np.bincount(pix // (h * w), minlength=B)
    for bn in range(B * N):
        c_vec[bn] = longest[bn] + touched[bn // N]
    return dict(d_qry=d_qry.reshape(B, h, w, C), mag_qry=mag_qry.reshape(B, h, w, C), c_qry=c_qry.reshape(B, h, w),
                d_vec=d_vec, mag_vec=mag_vec, c_vec=c_vec)


# active rows (pass g, y, x) of the guidance tests on an 8 x 10 map; tests/test_featgrad_ref_cpu.py asserts what each
# placement reaches
def guidance_rows(batch: int, n_ways: int, h: int = 8, w: int = 10, kind: str = 'placed'):
    if kind == 'single':
        return np.array([batch * n_ways - 1]), np.array([h // 2]), np.array([w // 2])
    if kind == 'all':                                  # every pixel of every pass
        g, y, x = np.meshgrid(np.arange(batch * n_ways), np.arange(h), np.arange(w), indexing='ij')
        return g.reshape(-1), y.reshape(-1), x.reshape(-1)
    last = batch * n_ways - 1
    rows = [(0, 0, 0), (0, 0, w - 1), (last, h - 1, 0), (last, h - 1, w - 1),       # the four corners
            (0, 3, 4), (0, 3, 5),                                                   # two adjacent active pixels
            (0, 5, 2), (min(n_ways - 1, 1), 5, 2)]                                  # one pixel, two passes of image 0
    if n_ways == 1:
        rows = rows[:-1]                               # (one pass per image: the pixel is active once)
    g, y, x = (np.array(c_) for c_ in zip(*rows))
    return g, y, x
