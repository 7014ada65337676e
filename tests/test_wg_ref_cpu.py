"""The float64 Winograd reference of tests/_wg_ref.py checked without a GPU: the triple (A^T, G, B^T) as algebra over the
rationals, the fp64 table of ``ops._WG_G``, every element of the closed forms against sums written out with
``fractions.Fraction``, their composition against float64 ``F.conv2d``, the host's ``ops.pack_winograd`` per element, and a
numpy emulation of the kernels' fp32 arithmetic held to the rounding counts tests/test_hip_wg_bound.py asserts on the GPU.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _wg_ref as ref

F64 = torch.float64


# ------------------------------------------------------------------------------------------ algebra
@pytest.mark.parametrize('m', [2, 4])
def test_transform_triple_is_an_exact_identity(m):
    """sum_k A^T[i][k] G[k][j] B^T[k][l] == [l == i + j] for all i, j, l, in exact rational arithmetic: the m outputs of
    a 3-tap correlation.  A single coefficient off breaks it (checked on a copy)."""
    assert ref.identity_defect(m) == []
    assert len(ref.BT[m]) == m + 2 and len(ref.AT[m]) == m and len(ref.G[m]) == m + 2
    bt = [row[:] for row in ref.BT[m]]
    bt[1][3] += Fr(1, 2)
    assert ref.identity_defect(m, bt=bt) != []
    g = [row[:] for row in ref.G[m]]
    g[m][1] = -g[m][1]
    assert ref.identity_defect(m, g=g) != []


@pytest.mark.parametrize('m', [2, 4])
def test_host_table_is_the_rationals_rounded_to_fp64(m):
    from fgn_amd import ops
    table = ops._WG_G[m]
    assert table.dtype == F64 and tuple(table.shape) == (m + 2, 3)
    for a in range(m + 2):
        for j in range(3):
            assert float(table[a, j]) == float(ref.G[m][a][j]), (m, a, j)       # float(Fraction) rounds correctly
    assert torch.equal(table, ref.g64(m))


def test_zero_sum_rows():
    assert ref.zero_sum_rows(4) == [True, False, True, True, True, True]
    assert ref.zero_sum_rows(2) == [True, False, True, True]


# ------------------------------------------------------------------------------------------ element by element
def _close(got, want_fr, mag_fr, what):
    """``got`` float64 against an exact rational: a few fp64 roundings of the term-magnitude sum."""
    assert abs(Fr(float(got)) - want_fr) <= Fr(64, 2 ** 53) * mag_fr, what


@pytest.mark.parametrize('m', [2, 4])
def test_closed_forms_against_written_out_rational_sums(m):
    """Index conventions and values of the three closed forms, every element of a small case against the definition
    spelled out with Fractions: group g = a (m + 2) + b, tile t = (img ty + y) tx + x, patch origin (m y - 1, m x - 1),
    zeros outside, image i reads x[i // a_img_div] scaled by in_scale[i]; outputs beyond H / W dropped; U[g][co][ci]."""
    R = m + 2
    g = ref.gen(3 + m)
    n_in, div, H, W, C = 1, 2, 5, 6, 2
    x = ref.spread((n_in, H, W, C), g, 1.0)
    s = (torch.rand(n_in * div, C, generator=g) + 0.5).float()
    ty, tx = ref.tiles_of(H, W, m)
    V, Vm = ref.input_transform(x, s, div, m)
    assert tuple(V.shape) == (R * R, n_in * div * ty * tx, C) == tuple(Vm.shape) and V.dtype == F64

    def xs(img, iy, ix, c):
        if not (0 <= iy < H and 0 <= ix < W):
            return Fr(0)
        return Fr(float(x[img // div, iy, ix, c])) * Fr(float(s[img, c]))
    for img in range(n_in * div):
        for y in range(ty):
            for xx in range(tx):
                t = (img * ty + y) * tx + xx
                for c in range(C):
                    d = [[xs(img, m * y - 1 + i, m * xx - 1 + j, c) for j in range(R)] for i in range(R)]
                    for a in range(R):
                        for b in range(R):
                            terms = [ref.BT[m][a][i] * d[i][j] * ref.BT[m][b][j] for i in range(R) for j in range(R)]
                            mag = sum(abs(v) for v in terms)
                            _close(V[a * R + b, t, c], sum(terms), mag, ('V', a, b, t, c))
                            _close(Vm[a * R + b, t, c], mag, mag, ('Vmag', a, b, t, c))

    n_img = 2
    t_rows = n_img * ty * tx + 3                                               # rows past the valid ones are ignored
    Mo = ref.spread((R * R, t_rows, 1, C), g, 1.0).reshape(R * R, t_rows, C)
    shift = torch.randn(C, generator=g)
    for sh in (None, shift):
        for relu in (False, True):
            Y, Ym = ref.output_transform(Mo, sh, relu, n_img, H, W, m)
            assert tuple(Y.shape) == (n_img, H, W, C) == tuple(Ym.shape)
            for img in range(n_img):
                for oy in range(H):
                    for ox in range(W):
                        t = (img * ty + oy // m) * tx + ox // m
                        for c in range(C):
                            terms = [ref.AT[m][oy % m][a] * Fr(float(Mo[a * R + b, t, c])) * ref.AT[m][ox % m][b]
                                     for a in range(R) for b in range(R)]
                            if sh is not None:
                                terms.append(Fr(float(sh[c])))
                            val, mag = sum(terms), sum(abs(v) for v in terms)
                            _close(Y[img, oy, ox, c], max(val, Fr(0)) if relu else val, mag, ('y', img, oy, ox, c))
                            _close(Ym[img, oy, ox, c], mag, mag, ('ymag', img, oy, ox, c))

    w = ref.spread((3, 2, 3, 3), g, 1.0)
    G64 = ref.g64(m)
    Uw, Um = ref.pack_weights(w, G64, m)
    assert tuple(Uw.shape) == (R * R, 3, 2)
    gq = [[Fr(float(G64[a, i])) for i in range(3)] for a in range(R)]
    for co in range(3):
        for ci in range(2):
            for a in range(R):
                for b in range(R):
                    terms = [gq[a][i] * Fr(float(w[co, ci, i, j])) * gq[b][j] for i in range(3) for j in range(3)]
                    mag = sum(abs(v) for v in terms)
                    _close(Uw[a * R + b, co, ci], sum(terms), mag, ('U', a, b, co, ci))
                    _close(Um[a * R + b, co, ci], mag, mag, ('Umag', a, b, co, ci))


def test_two_tensor_forms_follow_at_tiles0():
    g = ref.gen(8)
    x0, x1 = ref.spread((2, 5, 3, 4), g), ref.spread((3, 7, 9, 4), g)
    V, Vm = ref.input_transform2(x0, x1, 4)
    t0 = 2 * 2 * 1
    assert V.shape[1] == t0 + 3 * 2 * 3
    assert torch.equal(V[:, :t0], ref.input_transform(x0, None, 1, 4)[0])
    assert torch.equal(Vm[:, t0:], ref.input_transform(x1, None, 1, 4)[1])
    Mo = torch.randn(36, V.shape[1] + 5, 4, generator=g)
    (y0, _), (y1, m1) = ref.output_transform2(Mo, None, True, (2, 5, 3), (3, 7, 9), 4)
    assert torch.equal(y0, ref.output_transform(Mo, None, True, 2, 5, 3, 4)[0])
    assert torch.equal(y1, ref.output_transform(Mo[:, t0:], None, True, 3, 7, 9, 4)[0])
    assert tuple(m1.shape) == (3, 7, 9, 4)


# ------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize('m', [2, 4])
def test_composition_is_the_convolution(m):
    """output_transform(V U^T) of the closed forms equals float64 F.conv2d(padding=1) on n = 2, 7 x 9, C = 8 -> 4, with
    and without the per-(image, channel) input scale and a_img_div, to 1e-12 of each element's term-magnitude sum - the sum
    of the Winograd form: |A^T| (mag V . mag U) |A| + |shift|, which is what an error of the form is proportional to."""
    g = ref.gen(21 + m)
    n, H, W, cin, cout = 2, 7, 9, 8, 4
    x = ref.spread((n, H, W, cin), g, 1.0)
    w = ref.spread((cout, cin, 3, 3), g, 0.5)
    b = torch.randn(cout, generator=g)
    G64 = ref.g64(m)
    for div, scaled in ((1, False), (2, True)):
        s = (torch.rand(n * div, cin, generator=g) + 0.5).float() if scaled else None
        V, Vm = ref.input_transform(x, s, div, m)
        Uw, Um = ref.pack_weights(w, G64, m)
        Mo = torch.einsum('gtc,goc->gto', V, Uw)
        Mm = torch.einsum('gtc,goc->gto', Vm, Um)
        y, _ = ref.output_transform(Mo, b, False, n * div, H, W, m)
        _, ymag = ref.output_transform(Mm, b, False, n * div, H, W, m)
        xi = x.double().repeat_interleave(div, 0)
        if s is not None:
            xi = xi * s.double()[:, None, None, :]
        want = F.conv2d(xi.permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
        assert tuple(y.shape) == tuple(want.shape) == (n * div, H, W, cout)
        ratio = float(((y - want).abs() / (1e-12 * ymag)).max())
        print(f'[wg-ref] composition m={m} div={div}: worst |err| / (1e-12 mag) = {ratio:.4f}')
        assert ratio <= 1.0
        yr, _ = ref.output_transform(Mo, b, True, n * div, H, W, m)
        assert torch.equal(yr, torch.relu(y))


# ------------------------------------------------------------------------------------------ the host's pack
@pytest.mark.parametrize('m', [2, 4])
@pytest.mark.parametrize('cout,cin,fold', [(4, 32, 'bn+bias'), (96, 64, 'bias'), (132, 32, 'bn'), (8, 32, None)])
def test_host_pack_winograd_bound(cout, cin, fold, m):
    """``ops.pack_winograd``: fp64 einsum of the (BN-folded) weights, one rounding to fp32 - bounded per element like the
    pack kernel: |got - ref| <= 2^-24 |ref| + 16 * 2^-53 mag + 2^-126.  The fold is the host's own formula evaluated in
    fp64 (scale = gamma / sqrt(var + eps), w * scale; shift = beta - mean * scale (+ bias * scale)), so the folded
    weights are the same fp64 numbers; the einsum's contraction order is torch's (at most 5 + 5 fp64 roundings behind an
    element, as in the kernel).  Rows [cout, cout_pad) of every group are exactly +0."""
    from fgn_amd import ops
    g = ref.gen(cout + cin + m)
    w = ref.spread((cout, cin, 3, 3), g, 1.5)
    bias = torch.randn(cout, generator=g) if fold and 'bias' in fold else None
    bn = None
    if fold and 'bn' in fold:
        bn = dict(weight=torch.rand(cout, generator=g) + 0.5, bias=torch.randn(cout, generator=g) * 0.1,
                  running_mean=torch.randn(cout, generator=g) * 0.1, running_var=torch.rand(cout, generator=g) + 0.5)
    layer = ops.pack_winograd(w, bias=bias, bn=bn, relu=True, eps=1e-5, m=m)
    R = m + 2
    cout_pad = (cout + 127) // 128 * 128
    assert tuple(layer.u.shape) == (R * R, cout_pad, cin) and layer.u.dtype == torch.float32
    assert (layer.cin, layer.cout, layer.cout_pad, layer.m, layer.groups) == (cin, cout, cout_pad, m, R * R)
    w64, shift = w.double(), None
    if bn is not None:
        scale = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + 1e-5)
        shift = bn['bias'].double() - bn['running_mean'].double() * scale
        if bias is not None:
            shift = shift + bias.double() * scale
        w64 = w64 * scale[:, None, None, None]
    elif bias is not None:
        shift = bias.double()
    want, mag = ref.pack_weights(w64, ref.g64(m), m)
    ratio = ref.pack_ratio(layer.u[:, :cout], want, mag)
    print(f'[wg-ref] pack_winograd m={m} ({cout}, {cin}) {fold}: worst |err| / bound = {ratio:.4f}')
    assert ratio <= 1.0
    assert bool((layer.u[:, cout:].contiguous().view(torch.int32) == 0).all())
    if shift is None:
        assert layer.shift is None
    else:
        assert torch.equal(layer.shift, shift.float())


# ------------------------------------------------------------------------------------------ fp32 emulation
def _fma(k, a, acc, fused):
    if fused:       # one rounding: the product of two fp32 values is exact in fp64
        return (np.float64(k) * a.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return np.float32(k) * a + acc


def _bt4(d, fused):
    f = lambda k, a, acc: _fma(k, a, acc, fused)
    return [f(1.5, d[3] - d[1], f(-2.0, d[2], d[0])) + d[4],
            f(2.5, d[3], f(0.5, d[2], d[4] - d[1])),
            f(0.5, d[3], f(-2.5, d[2], d[1] + d[4])),
            f(2.0, d[3] - d[1], d[4] - d[2]),
            f(0.5, d[1] - d[3], d[4] - d[2]),
            f(1.5, d[4] - d[2], f(-2.0, d[3], d[1])) + d[5]]


def _at4(q, fused):
    f = lambda k, a, acc: _fma(k, a, acc, fused)
    s12, d12 = q[1] + q[2], q[1] - q[2]
    return [(q[0] + s12) + (q[3] + q[4]),
            f(-2.0, q[4], f(0.5, q[3], d12)),
            f(4.0, q[4], f(0.25, q[3], s12)),
            f(-8.0, q[4], f(0.125, q[3], d12)) + q[5]]


def _bt2(d, fused):
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def _at2(q, fused):
    return [(q[0] + q[1]) + q[2], (q[1] - q[2]) - q[3]]


def _two_passes(P, one_d, fused):
    """P [N, R, R] fp32 -> [N, r, r]: the 1-D transform down the columns, then along the rows (the kernels' order)."""
    R = P.shape[1]
    cols = [one_d([P[:, a, b] for a in range(R)], fused) for b in range(R)]            # cols[b][i]
    r = len(cols[0])
    rows = [one_d([cols[b][i] for b in range(R)], fused) for i in range(r)]            # rows[i][j]
    return np.stack([np.stack(rows[i], 1) for i in range(r)], 1)


def _np_mat(mat):
    return np.array([[float(v) for v in row] for row in mat], dtype=np.float64)


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('m', [2, 4])
def test_fp32_emulation_stays_under_the_derived_counts(m, fused):
    """The kernels' 1-D passes in numpy float32 on 2 * 10^5 patches whose values span e^+-6 in magnitude: without any
    contraction (every multiply and every add rounds: MORE roundings than the kernels, whose ``fmaf`` calls are single
    roundings) and with the ``fmaf`` calls as single roundings.  Worst |err| / (2^-24 mag) must stay below the c the GPU
    tests use: input c = 10 / 4 (with the in_scale product), output c = 10 / 6 (with the shift)."""
    rng = np.random.default_rng(100 + m)
    N, R = 200_000, m + 2
    P = (rng.standard_normal((N, R, R)) * np.exp(rng.uniform(-6, 6, (N, R, R)))).astype(np.float32)
    s = rng.uniform(0.5, 1.5, N).astype(np.float32)
    bt, at = _np_mat(ref.BT[m]), _np_mat(ref.AT[m])
    got = _two_passes(P * s[:, None, None], _bt4 if m == 4 else _bt2, fused)
    d64 = P.astype(np.float64) * s.astype(np.float64)[:, None, None]
    want = np.einsum('ai,nij,bj->nab', bt, d64, bt)
    mag = np.einsum('ai,nij,bj->nab', np.abs(bt), np.abs(d64), np.abs(bt))
    r_in = float((np.abs(got.astype(np.float64) - want) / (ref.U * mag + ref.TINY)).max())
    sh = (rng.standard_normal(N) * np.exp(rng.uniform(-6, 6, N))).astype(np.float32)
    got = _two_passes(P, _at4 if m == 4 else _at2, fused) + sh[:, None, None]
    want = np.einsum('ai,nij,bj->nab', at, P.astype(np.float64), at) + sh.astype(np.float64)[:, None, None]
    mag = np.einsum('ai,nij,bj->nab', np.abs(at), np.abs(P.astype(np.float64)), np.abs(at)) + np.abs(sh.astype(np.float64))[:, None, None]
    r_out = float((np.abs(got.astype(np.float64) - want) / (ref.U * mag + ref.TINY)).max())
    print(f'[wg-ref] fp32 emulation m={m} fused={fused}: input {r_in:.2f} of c = {ref.C_IN[m]}, '
          f'output {r_out:.2f} of c = {ref.C_OUT[m]}')
    assert r_in <= ref.C_IN[m] and r_out <= ref.C_OUT[m]
    # a constant patch: every position with a zero-sum row of B^T on either side is exactly 0 in the kernels' arithmetic
    # (with the multiplies by 3/2 and 5/2 rounded on their own, F(4x4) leaves a residue of an ulp: not asserted there)
    if m == 4 and not fused:
        return
    const = np.broadcast_to((P[:, 0, 0] * s)[:, None, None], P.shape).copy()
    v = _two_passes(const, _bt4 if m == 4 else _bt2, fused)
    z = np.array(ref.zero_sum_rows(m))
    assert (v[:, z[:, None] | z[None, :]] == 0).all()
