"""Float64 closed forms of the Winograd transforms and the weight pack (csrc/winograd.hip), for tests/test_wg_ref_cpu.py
and tests/test_hip_wg_bound.py.  Plain torch ops on whatever device the operands are on; nothing is imported from
``fgn_amd`` and nothing is parsed from the kernels.

The matrices are written out below as exact rationals.  F(m x m, 3 x 3) computes m outputs of a 3-tap correlation from
m + 2 inputs as  y = A^T [(G g) . (B^T d)];  in two dimensions  y = A^T [(G g G^T) . (B^T d B)] A.  It is an identity of
polynomials, so it holds exactly over the rationals: ``identity_defect`` checks it without a single rounding.

Every function returns ``(value, mag)``: the float64 value and the sum of the magnitudes of its terms, the quantity a
rounding error of the kernel is proportional to:  |got - value| <= c * 2^-24 * mag + 2^-126.
"""
from fractions import Fraction as Fr

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53        # unit roundoff of fp64
TINY = 2.0 ** -126      # smallest normal fp32


def _fr(rows):
    return [[Fr(v) for v in row] for row in rows]


# F(2x2,3x3): points {0, 1, -1, inf}.  F(4x4,3x3): Cook-Toom with the points {0, 1, -1, 1/2, -2, inf}.
BT = {
    2: _fr([[1, 0, -1, 0],
            [0, 1, 1, 0],
            [0, -1, 1, 0],
            [0, 1, 0, -1]]),
    4: _fr([[1, Fr(-3, 2), -2, Fr(3, 2), 1, 0],
            [0, -1, Fr(1, 2), Fr(5, 2), 1, 0],
            [0, 1, Fr(-5, 2), Fr(1, 2), 1, 0],
            [0, -2, -1, 2, 1, 0],
            [0, Fr(1, 2), -1, Fr(-1, 2), 1, 0],
            [0, 1, Fr(-3, 2), -2, Fr(3, 2), 1]]),
}
AT = {
    2: _fr([[1, 1, 1, 0],
            [0, 1, -1, -1]]),
    4: _fr([[1, 1, 1, 1, 1, 0],
            [0, 1, -1, Fr(1, 2), -2, 0],
            [0, 1, 1, Fr(1, 4), 4, 0],
            [0, 1, -1, Fr(1, 8), -8, 1]]),
}
G = {
    2: _fr([[1, 0, 0],
            [Fr(1, 2), Fr(1, 2), Fr(1, 2)],
            [Fr(1, 2), Fr(-1, 2), Fr(1, 2)],
            [0, 0, 1]]),
    4: _fr([[1, 0, 0],
            [Fr(1, 3), Fr(1, 3), Fr(1, 3)],
            [Fr(-1, 3), Fr(1, 3), Fr(-1, 3)],
            [Fr(-16, 15), Fr(-8, 15), Fr(-4, 15)],
            [Fr(1, 15), Fr(-2, 15), Fr(4, 15)],
            [0, 0, 1]]),
}

# Roundings of fp32 counted along the longest chain of each kernel (tests/test_hip_wg_bound.py derives them in its
# docstrings; tests/test_wg_ref_cpu.py holds a numpy emulation of the kernels' arithmetic to the same numbers).
C_IN = {4: 10, 2: 4}
C_OUT = {4: 10, 2: 6}
C_PACK64 = 16           # fp64 roundings behind one element of U, before its single rounding to fp32


def identity_defect(m, at=None, g=None, bt=None):
    """-> the (i, j, l) at which  sum_k A^T[i][k] G[k][j] B^T[k][l] != [l == i + j]  (exact rational arithmetic)."""
    at, g, bt = at or AT[m], g or G[m], bt or BT[m]
    bad = []
    for i in range(m):
        for j in range(3):
            for l in range(m + 2):
                s = sum(at[i][k] * g[k][j] * bt[k][l] for k in range(m + 2))
                if s != (1 if l == i + j else 0):
                    bad.append((i, j, l))
    return bad


def g64(m):
    """G rounded to fp64, element for element."""
    return torch.tensor([[float(v) for v in row] for row in G[m]], dtype=F64)


def zero_sum_rows(m):
    """Rows of B^T whose coefficients sum to exactly 0: they annihilate a constant."""
    return [sum(row) == 0 for row in BT[m]]


def _floats(mat):
    return [[float(v) for v in row] for row in mat]


def _apply(mat, parts, absolute=False):
    """-> [sum_k mat[i][k] * parts[k] for every row i]; with ``absolute`` the coefficients by magnitude.  ``mat`` holds
    Python floats; zero coefficients are skipped."""
    out = []
    for row in mat:
        acc = None
        for k, coef in enumerate(row):
            if coef == 0.0:
                continue
            term = parts[k] * (abs(coef) if absolute else coef)
            acc = term if acc is None else acc + term
        out.append(acc if acc is not None else torch.zeros_like(parts[0]))
    return out


def tiles_of(H, W, m):
    return (H + m - 1) // m, (W + m - 1) // m


def input_transform(x, in_scale=None, a_img_div=1, m=4):
    """x [n_in, H, W, C] (fp32 or fp64), in_scale [n_img, C] or None; logical image i reads x[i // a_img_div].
    -> (V, mag) float64 [G, tiles, C]: group g = a * (m + 2) + b, tile t = (img * ty + y) * tx + x, patch origin
    (m y - 1, m x - 1), zeros outside the map;  V = B^T (x s) B,  mag = |B^T| |x s| |B|."""
    n_in, H, W, C = x.shape
    R = m + 2
    ty, tx = tiles_of(H, W, m)
    n_img = n_in * a_img_div if in_scale is None else in_scale.shape[0]
    d = x.to(F64)
    if a_img_div != 1:
        d = d[torch.arange(n_img, device=x.device) // a_img_div]
    if in_scale is not None:
        d = d * in_scale.to(F64)[:, None, None, :]
    xp = torch.zeros(n_img, m * ty + 2, m * tx + 2, C, dtype=F64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = d
    bt = _floats(BT[m])
    res = []
    for absolute in (False, True):
        src = xp.abs() if absolute else xp
        rows = [src[:, a:a + m * ty:m] for a in range(R)]                     # [n, ty, Wp, C] each
        cols_of = _apply(bt, rows, absolute)                                  # R x [n, ty, Wp, C]
        out = []
        for t in cols_of:
            out += _apply(bt, [t[:, :, b:b + m * tx:m] for b in range(R)], absolute)   # R x [n, ty, tx, C]
        res.append(torch.stack(out).reshape(R * R, n_img * ty * tx, C))
    return res[0], res[1]


def input_transform2(x0, x1, m=4):
    """Two tensors into consecutive tile ranges: the second tensor's tiles follow the first at tiles0."""
    v0, m0 = input_transform(x0, None, 1, m)
    v1, m1 = input_transform(x1, None, 1, m)
    return torch.cat([v0, v1], 1), torch.cat([m0, m1], 1)


def output_transform(Mo, shift, relu, n_img, H, W, m=4):
    """Mo [G, >= n_img * tiles, C]; -> (y, mag) float64 [n_img, H, W, C]:  y = A^T Mo A + shift,  mag = |A^T| |Mo| |A|
    + |shift|; outputs beyond H / W are dropped; ReLU on y only (1-Lipschitz: the bound carries over)."""
    R = m + 2
    ty, tx = tiles_of(H, W, m)
    C = Mo.shape[-1]
    mo = Mo[:, :n_img * ty * tx].to(F64).reshape(R, R, n_img, ty, tx, C)
    at = _floats(AT[m])
    res = []
    for absolute in (False, True):
        src = mo.abs() if absolute else mo
        rows = _apply(at, [src[a] for a in range(R)], absolute)               # m x [R, n, ty, tx, C]
        out = [torch.stack(_apply(at, [r[b] for b in range(R)], absolute)) for r in rows]   # m x [m, n, ty, tx, C]
        y = torch.stack(out).permute(2, 3, 0, 4, 1, 5).reshape(n_img, ty * m, tx * m, C)[:, :H, :W]
        if shift is not None:
            y = y + (shift.to(F64).abs() if absolute else shift.to(F64))
        res.append(y.contiguous())
    return (torch.relu(res[0]) if relu else res[0]), res[1]


def output_transform2(Mo, shift, relu, s0, s1, m=4):
    """Two output tensors (n, H, W) from consecutive tile ranges of Mo.  -> ((y0, mag0), (y1, mag1))."""
    ty, tx = tiles_of(s0[1], s0[2], m)
    t0 = s0[0] * ty * tx
    return output_transform(Mo, shift, relu, *s0, m=m), output_transform(Mo[:, t0:], shift, relu, *s1, m=m)


def pack_weights(w, G64, m):
    """w [cout, cin, 3, 3] (fp32 or fp64), G64 [m + 2, 3] the fp64 table the caller hands the kernel (the kernel's 1/3
    is fp64's 1/3).  -> (U, mag) float64 [G, cout, cin]:  U[a (m + 2) + b] = sum_ij G[a][i] w[.., i, j] G[b][j]."""
    R = m + 2
    assert tuple(G64.shape) == (R, 3) and G64.dtype == F64
    g = G64.tolist()
    k = w.to(F64)
    res = []
    for absolute in (False, True):
        src = k.abs() if absolute else k
        t = _apply(g, [src[:, :, i, :] for i in range(3)], absolute)         # R x [cout, cin, 3]
        out = []
        for ta in t:
            out += _apply(g, [ta[:, :, j] for j in range(3)], absolute)      # R x [cout, cin]
        res.append(torch.stack(out))
    return res[0], res[1]


def worst_ratio(got, want, mag, c, slack=None):
    """-> worst |got - want| / (c 2^-24 mag (+ slack) + 2^-126) over the elements (0 for an empty tensor)."""
    if want.numel() == 0:
        return 0.0
    got = got.to(F64).reshape(want.shape)
    assert bool(torch.isfinite(got).all())
    bound = c * U * mag + TINY
    if slack is not None:
        bound = bound + slack
    return float(((got - want).abs() / bound).max())


def pack_ratio(got, want, mag):
    """The weight pack's bound: one fp32 rounding of an fp64 result that carries at most C_PACK64 fp64 roundings."""
    return worst_ratio(got, want, want.abs(), 1, C_PACK64 * U64 * mag)


# ------------------------------------------------------------------------------------------ test inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def spread(shape, g, decades=2.6):
    """Signed values whose magnitude is spread over ``2 * decades`` decades per pixel and as much again per channel, so
    that many transform outputs are small through cancellation or through small operands."""
    n, H, W, C = shape
    k = decades * float(np.log(10.0))
    px = torch.exp((torch.rand(n, H, W, 1, generator=g) * 2 - 1) * k)
    ch = torch.exp((torch.rand(1, 1, 1, C, generator=g) * 2 - 1) * k)
    return (torch.randn(n, H, W, C, generator=g) * px * ch).float().contiguous()


def with_constant_image(x, g):
    """A copy of x whose last image is constant per channel (signed, mixed magnitude)."""
    x = x.clone()
    C = x.shape[-1]
    x[-1] = (torch.randn(C, generator=g) * torch.exp((torch.rand(C, generator=g) * 2 - 1) * 4.0)).float()
    return x


def interior_tiles(H, W, m):
    """-> bool [ty, tx]: tiles whose whole (m + 2) x (m + 2) patch lies inside the map."""
    ty, tx = tiles_of(H, W, m)
    ys = torch.tensor([m * y - 1 >= 0 and m * y + m + 1 <= H for y in range(ty)])
    xs = torch.tensor([m * x - 1 >= 0 and m * x + m + 1 <= W for x in range(tx)])
    return ys[:, None] & xs[None, :]
