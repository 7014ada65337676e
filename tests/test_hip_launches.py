"""Every convolution launch of one cfg3 episode against fp64, and the edges of conv_pw_h2_kernel an episode cannot reach.

The routing rules (fgn_h2_row_tile / fgn_x3_row_tile) leave a launch that is too small for the GEMM kernels' tiles to the
f32 kernels, so a test named after an arithmetic says nothing unless it checks where its launch ran: every test here
reads the route of its launches from ``ops.PROFILE`` records (``math``: 'h2' / 'x3' / 'f32')."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _routed(fn):
    """Run ``fn`` under a ConvProfile -> (its result, the arithmetic of each of its MFMA launches: 'h2' / 'x3' / 'f32')."""
    from fgn_amd import ops
    prev = ops.PROFILE
    ops.PROFILE = ops.ConvProfile()
    try:
        out = fn()
        torch.cuda.synchronize()
        maths = [r.get('math', 'f32') for r in ops.PROFILE if r['kind'] in ('conv', 'wg_gemm')]
    finally:
        ops.PROFILE = prev
    return out, maths


def _bn(g, c):
    return dict(weight=torch.rand(c, generator=g) + 0.5, bias=torch.randn(c, generator=g) * 0.1,
                running_mean=torch.randn(c, generator=g) * 0.1, running_var=torch.rand(c, generator=g) + 0.5)


def _affine(bn):
    sc = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + 1e-5)
    return sc, bn['bias'].double() - bn['running_mean'].double() * sc


# ---------------------------------------------------------------------------------------------------------------------
# B. kernel-level edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', ['layer2.0', 'layer3.0'])
def test_strided_dual_launch_on_h2_at_production_size(stage):
    """conv3 + the 1x1 / stride 2 shortcut of layer2.0 / layer3.0 as ONE K loop on conv_pw_h2_kernel, the shortcut's rows
    read through the ``ops.strided_rows`` table over the query map and the support maps lying one behind the other in one
    buffer - the production launches (1x25916x384->512, 1x6504x768->1024), query first and supports first: within 2e-6 of
    the range of fp64, within 4e-6 of the two-launch f32 form (strided shortcut conv, then conv3 with the residual in its
    epilogue), bit-identical run to run."""
    from fgn_amd import ops
    (hq, wq), (hs, ws), cin1, cin2, cout = {'layer2.0': ((200, 334), (64, 64), 128, 256, 512),
                                            'layer3.0': ((100, 167), (32, 32), 256, 512, 1024)}[stage]
    g = torch.Generator().manual_seed(cin1)
    q = torch.randn(1, hq, wq, cin2, generator=g).relu_()
    s = torch.randn(9, hs, ws, cin2, generator=g).relu_()
    w3, wd = torch.randn(cout, cin1, 1, 1, generator=g) / cin1 ** 0.5, torch.randn(cout, cin2, 1, 1, generator=g) / cin2 ** 0.5
    bn3, bnd = _bn(g, cout), _bn(g, cout)
    mq, ms = ((hq + 1) // 2) * ((wq + 1) // 2), 9 * ((hs + 1) // 2) * ((ws + 1) // 2)
    assert mq + ms == {'layer2.0': 25916, 'layer3.0': 6504}[stage]
    yq, ys = torch.randn(mq, cin1, generator=g).relu_(), torch.randn(ms, cin1, generator=g).relu_()
    with ops.gemm_math('h2'):
        layer = ops.pack_conv_dual(w3, bn3, wd, bnd, relu=True).to('cuda')
    assert layer.wh is not None
    sc3, sh3 = _affine(bn3)
    scd, shd = _affine(bnd)
    w3d, wdd = w3.reshape(cout, cin1).double() * sc3[:, None], wd.reshape(cout, cin2).double() * scd[:, None]
    ref = {}
    for name, x, y in (('q', q, yq), ('s', s, ys)):
        sub = x[:, ::2, ::2].reshape(-1, cin2).double()
        ref[name] = torch.relu(y.double() @ w3d.T + sub @ wdd.T + (sh3 + shd))
    with ops.gemm_math('f32'):
        down = ops.pack_conv(wd, bn=bnd, stride=2).to('cuda')
        conv3 = ops.pack_conv(w3, bn=bn3, relu=True).to('cuda')
        two = {'q': ops.conv2d(yq.cuda().view(1, mq, 1, cin1), conv3, residual=ops.conv2d(q.cuda(), down).view(1, mq, 1, cout)),
               's': ops.conv2d(ys.cuda().view(1, ms, 1, cin1), conv3, residual=ops.conv2d(s.cuda(), down).view(1, ms, 1, cout))}
    for order in ('qs', 'sq'):
        xs = {'q': (q, yq, (1, hq, wq)), 's': (s, ys, (9, hs, ws))}
        buf = torch.cat([xs[k][0].reshape(-1, cin2) for k in order]).cuda()
        y = torch.cat([xs[k][1] for k in order]).cuda().view(1, -1, 1, cin1)
        tab = ops.strided_rows([xs[k][2] for k in order], 2, 'cuda')
        got, route = _routed(lambda: ops.conv1x1_dual(y, buf.view(1, -1, 1, cin2), layer, x2_rows=tab))
        assert route == ['h2'], route
        again = ops.conv1x1_dual(y, buf.view(1, -1, 1, cin2), layer, x2_rows=tab)
        assert torch.equal(got, again)
        got = got.view(-1, cout)
        m0 = 0
        for k in order:
            m = mq if k == 'q' else ms
            part = got[m0:m0 + m]
            rng = ref[k].abs().max().item()
            err = (part.cpu().double() - ref[k]).abs().max().item()
            assert err <= 2e-6 * rng, (order, k, err / rng)
            assert (part - two[k].view(m, cout)).abs().max().item() <= 4e-6 * rng, (order, k)
            m0 += m


@pytest.mark.parametrize('cin,cout,res', [(1024, 512, False), (512, 1024, True)])
def test_h2_pointwise_launch_honours_a_device_count_below_capacity(cin, cout, res):
    """The RoI-count launches of the shared head / relation Q / mask head: conv_pw_h2_kernel over M = min(n_img, count) * HW
    rows of a 300-RoI capacity (300x7x7, 1024->512 with BN + ReLU; 512->1024 with BN, residual and ReLU).  Counts: the
    capacity, 137, 1, 0 and one above the capacity (clamped).  Rows below count * 49 within 2e-6 of fp64; rows from
    count * 49 on keep their sentinel bit for bit (nothing is written there, the residual read stops at the count)."""
    from fgn_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    n, hw = 300, 49
    x = torch.randn(n, 7, 7, cin, generator=g).relu_()
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bn = _bn(g, cout)
    r = torch.randn(n, 7, 7, cout, generator=g) if res else None
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(w, bn=bn, relu=True).to('cuda')
    sc, sh = _affine(bn)
    ref = (x.reshape(-1, cin).double() @ w.reshape(cout, cin).double().T) * sc + sh
    if res:
        ref = ref + r.reshape(-1, cout).double()
    ref = torch.relu(ref)
    xc, rc = x.cuda(), None if r is None else r.cuda()
    sentinel = torch.tensor([0x7fc0beef], dtype=torch.int32).view(torch.float32).item()       # a NaN with a payload
    for count in (n, 137, 1, 0, n + 1):
        out = torch.full((n, 7, 7, cout), sentinel, device='cuda')
        pre = out.clone()
        cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
        _, route = _routed(lambda: ops.conv2d(xc, layer, residual=rc, n_img_dev=cnt, out=out))
        assert route == ['h2'], route
        v = min(count, n) * hw
        flat, pre_flat = out.view(-1, cout), pre.view(-1, cout)
        assert torch.equal(flat[v:].view(torch.int32), pre_flat[v:].view(torch.int32)), count
        if v:
            rng = ref[:v].abs().max().item()
            err = (flat[:v].cpu().double() - ref[:v]).abs().max().item()
            assert err <= 2e-6 * rng, (count, err / rng)


def _nonfinite_operands(where, bad):
    """x [512, 128]: rows alternating about 1e5 and 1e-4 in blocks of 8 (every wave's rows need a scale far from 1); one
    element of row 70 set to ``bad`` in K-tile 0 ('first'), or in K-tile 2 ('later') where every other row also grows
    1e3-fold, so that the wave must choose a new scale exactly in the K-tile that holds the non-finite element."""
    g = torch.Generator().manual_seed(8)
    rows, K = 512, 128
    x = torch.randn(rows, K, generator=g).abs_() + 0.1
    big = (torch.arange(rows) // 8) % 2 == 0
    x[big] *= 1e5
    x[~big] *= 1e-4
    k = 5 if where == 'first' else 70
    if where == 'later':
        x[:, 64:96] *= 1e3
    x0 = x.clone()
    x0[70, k] = 0.0
    x[70, k] = bad
    return x, x0


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
@pytest.mark.parametrize('where', ['first', 'later'])
@pytest.mark.parametrize('path', ['h2-64', 'h2-128', 'h2-264', 'x3', 'f32'])
def test_a_non_finite_element_stays_in_its_row(path, where, bad):
    """One +-Inf / NaN in one row of a GEMM: that row comes out non-finite (Inf or NaN: l = Inf - Inf makes h2 and x3 give
    NaN), every other row keeps the bits it has with the element replaced by 0 (h2: the wave's scale search takes finite
    elements only), and the other rows of the non-finite row's wave - 32 rows for the 64- and 264-tiles, 64 for the
    128-tile - stay within 2e-6 of the fp64 range of that block's finite rows (conv_pw_h2_kernel's contract: errors are
    relative to the wave's largest row).  The rows sit at about 1e5 and 1e-4, so that no wave can keep the scale 1;
    no ReLU.  conv_pw_x3_kernel and the f32 kernel keep rows independent: the same data through them."""
    from fgn_amd import ops
    x, x0 = _nonfinite_operands(where, bad)
    rows, K = x.shape
    N = 64
    g = torch.Generator().manual_seed(9)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    shift = torch.randn(N, generator=g)
    if path.startswith('h2'):
        bm = int(path[3:])
        img = ops.pack_h2(w.cuda())
        run = lambda a: ops.gemm_h2(a.cuda(), img, N, shift=shift.cuda(), bm=bm)
        blk = 64 if bm == 128 else 32
    elif path == 'x3':
        img = ops.pack_x3(w.cuda())
        run = lambda a: ops.gemm_x3(a.cuda(), img, N, shift=shift.cuda(), bm=64)
        blk = 1
    else:
        with ops.gemm_math('f32'):
            layer = ops.pack_conv(w.reshape(N, K, 1, 1), bias=shift).to('cuda')
        f32 = lambda a: ops.conv2d(a.cuda().view(1, rows, 1, K), layer).view(rows, N)
        assert _routed(lambda: f32(x0))[1] == ['f32']
        run = f32
        blk = 1
    got, zero = run(x).cpu(), run(x0).cpu()
    assert not torch.isfinite(got[70]).any(), (path, where, bad)
    others = torch.arange(rows) != 70
    assert torch.equal(got[others].view(torch.int32), zero[others].view(torch.int32)), (path, where, bad)
    b0 = 70 // blk * blk
    sel = [r for r in range(b0, b0 + max(blk, 32)) if r != 70]
    ref = x0[sel].double() @ w.double().T + shift.double()
    rng = ref.abs().max().item()
    assert (got[sel].double() - ref).abs().max().item() <= 2e-6 * rng, (path, where, bad)
    assert torch.isfinite(got[others]).all()


@pytest.mark.parametrize('big', ['q', 's'])
def test_pair_of_tensors_1e4_apart_is_held_to_each_tensors_own_range(big):
    """``conv2d_pair`` (layer2.0's 3x3 / stride 2, 128 channels, on conv_pw_h2_kernel's implicit-GEMM form) on a query map
    and support maps 1e4 apart in magnitude: each tensor within 2e-6 of its OWN fp64 range, except the one 32-row block
    (a wave's rows of the 64-row tile) that straddles the seam between the tensors, which shares one scale and is held
    to the larger range - the documented contract (errors relative to the wave's largest row), pinned at the seam."""
    from fgn_amd import ops
    g = torch.Generator().manual_seed(21)
    cin = cout = 128
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bn = _bn(g, cout)
    with ops.gemm_math('h2'):
        layer = ops.pack_conv(wt, bn=bn, stride=2, pad=1, relu=False).to('cuda')
    xq = torch.randn(1, 200, 334, cin, generator=g).relu_() * (1e4 if big == 'q' else 1.0)
    xs = torch.randn(9, 64, 64, cin, generator=g).relu_() * (1e4 if big == 's' else 1.0)
    buf = torch.cat([xq.reshape(-1), xs.reshape(-1)]).cuda()
    q_d, s_d = buf[:xq.numel()].view(xq.shape), buf[xq.numel():].view(xs.shape)
    (yq, ys), route = _routed(lambda: ops.conv2d_pair(q_d, s_d, layer))
    assert route == ['h2'], route
    sc, sh = _affine(bn)
    refs = []
    for x in (xq, xs):
        r = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), stride=2, padding=1)
        refs.append((r * sc[None, :, None, None] + sh[None, :, None, None]).permute(0, 2, 3, 1).reshape(-1, cout))
    got = [yq.reshape(-1, cout).cpu().double(), ys.reshape(-1, cout).cpu().double()]
    m0 = got[0].shape[0]
    assert m0 % 32 != 0                                # (16700 rows: the seam lies inside a wave's block)
    seam = m0 // 32 * 32                               # the block [seam, seam + 32) holds rows of both tensors
    both = max(refs[0].abs().max().item(), refs[1].abs().max().item())
    err = [(a - b).abs().max(1).values for a, b in zip(got, refs)]
    for t in (0, 1):
        rng = refs[t].abs().max().item()
        e = err[t].clone()
        straddle = slice(seam, m0) if t == 0 else slice(0, seam + 32 - m0)
        assert e[straddle].max().item() <= 2e-6 * both, t
        e[straddle] = 0
        assert e.max().item() <= 2e-6 * rng, (t, e.max().item() / rng)


# ---------------------------------------------------------------------------------------------------------------------
# A. one cfg3 episode, every convolution launch against an fp64 shadow of its sampled rows
# ---------------------------------------------------------------------------------------------------------------------
# The MFMA launches (kind 'conv' / 'wg_gemm') of one cfg3 episode queued by detect_device on one stream, in order, under
# GEMM_MATH 'h2': (kind, arithmetic, layer shape of the PROFILE record).  Four stay on the f32 kernels: the stem (Cin 4),
# the 9-RoI support head (441 rows), the RPN head (76 of 128 columns) and relation S (3 rows of RoIs).
_H2_EPISODE = [
    ('conv', 'f32', (10, 800, 1333, 4, 64, 7, 2)),
    ('conv', 'h2', (1, 103664, 1, 64, 64, 1, 1)), ('conv', 'h2', (10, 200, 334, 64, 64, 3, 1)),
    ('conv', 'h2', (1, 103664, 1, 128, 256, 1, 1)),
    ('conv', 'h2', (1, 103664, 1, 256, 64, 1, 1)), ('conv', 'h2', (10, 200, 334, 64, 64, 3, 1)),
    ('conv', 'h2', (1, 103664, 1, 64, 256, 1, 1)),
    ('conv', 'h2', (1, 103664, 1, 256, 64, 1, 1)), ('conv', 'h2', (10, 200, 334, 64, 64, 3, 1)),
    ('conv', 'h2', (1, 103664, 1, 64, 256, 1, 1)),
    ('conv', 'h2', (1, 103664, 1, 256, 128, 1, 1)), ('conv', 'h2', (10, 200, 334, 128, 128, 3, 2)),
    ('conv', 'h2', (1, 25916, 1, 384, 512, 1, 1))] + \
    [('conv', 'h2', (1, 25916, 1, 512, 128, 1, 1)), ('wg_gemm', 'h2', (2, 25916, 1, 128, 128, 3, 1)),
     ('conv', 'h2', (1, 25916, 1, 128, 512, 1, 1))] * 3 + [
    ('conv', 'h2', (1, 25916, 1, 512, 256, 1, 1)), ('conv', 'h2', (10, 100, 167, 256, 256, 3, 2)),
    ('conv', 'h2', (1, 6504, 1, 768, 1024, 1, 1))] + \
    [('conv', 'h2', (1, 6504, 1, 1024, 256, 1, 1)), ('wg_gemm', 'h2', (2, 6504, 1, 256, 256, 3, 1)),
     ('conv', 'h2', (1, 6504, 1, 256, 1024, 1, 1))] * 5 + [
    ('conv', 'f32', (9, 7, 7, 1024, 512, 1, 1)),
    ('wg_gemm', 'h2', (3, 50, 84, 1024, 1024, 3, 1)),
    ('conv', 'f32', (3, 50, 84, 1024, 76, 1, 1)),
    ('conv', 'h2', (1, 50, 84, 1024, 512, 1, 1))] + \
    [('wg_gemm', 'h2', (309, 7, 7, 512, 512, 3, 1)), ('conv', 'h2', (309, 7, 7, 512, 1024, 1, 1)),
     ('conv', 'h2', (309, 7, 7, 1024, 512, 1, 1))] * 2 + [
    ('wg_gemm', 'h2', (309, 7, 7, 512, 512, 3, 1)), ('conv', 'h2', (309, 7, 7, 512, 1024, 1, 1)),
    ('conv', 'f32', (3, 7, 7, 1024, 1024, 1, 1)),
    ('conv', 'h2', (300, 7, 7, 1024, 1024, 1, 1))] + \
    [('wg_gemm', 'h2', (100, 7, 7, 512, 512, 3, 1)), ('conv', 'h2', (100, 7, 7, 512, 1024, 1, 1)),
     ('conv', 'h2', (100, 7, 7, 1024, 512, 1, 1))] * 2 + [
    ('wg_gemm', 'h2', (100, 7, 7, 512, 512, 3, 1)), ('conv', 'h2', (100, 7, 7, 512, 1024, 1, 1)),
    ('wg_gemm', 'h2', (100, 7, 7, 1024, 256, 3, 1))] + \
    [('wg_gemm', 'h2', (100, 7, 7, 256, 256, 3, 1))] * 3 + [
    ('conv', 'h2', (100, 7, 7, 256, 1024, 1, 1))]
# per arithmetic: (MFMA launches, of them on the arithmetic's own kernel, of those Winograd GEMMs)
_EPISODE_COUNTS = {'h2': (67, 63, 19), 'x3': (67, 55, 19), 'f32': (67, 0, 0)}


def _sample(segs, rng, count_rows=None, tile_rows=None):
    """Rows to check of a launch over the tensors ``segs`` = [(n_img, Ho, Wo), ...] lying one behind the other in its row
    space: first / last row of every image; corners and edge midpoints of the first, the last and a few random images
    (padding taps, the last Winograd tile); both sides of 32 / 64 / 128-row boundaries at the start, the middle and the
    last tile (in the GEMM's row space: ``tile_rows`` maps a Winograd tile index to one pixel row of it); the last row
    below ``count_rows``; 256 seeded random rows.  -> sorted unique int64 array below count_rows."""
    total = sum(n * h * w for n, h, w in segs)
    valid = total if count_rows is None else min(count_rows, total)
    rows, base = [], 0
    for n, h, w in segs:
        hw = h * w
        rows += [base + i * hw for i in range(n)] + [base + i * hw + hw - 1 for i in range(n)]
        imgs = sorted({0, n - 1, *rng.integers(0, n, size=min(n, 4)).tolist()})
        for i in imgs:
            for oy, ox in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0),
                           (h // 2, w - 1)):
                rows.append(base + i * hw + oy * w + ox)
        base += n * hw
    span = total if tile_rows is None else tile_rows[1]
    edges = [e for b in (32, 64, 128) for c in (b, (span // 2) // b * b, (span - 1) // b * b) for e in (c - 1, c)]
    rows += edges if tile_rows is None else [tile_rows[0](t) for t in edges if 0 <= t < span]
    if count_rows is not None:
        rows.append(valid - 1)
    rows += rng.integers(0, max(valid, 1), size=256).tolist()
    return np.unique(np.asarray([v for v in rows if 0 <= v < valid], dtype=np.int64))


def _conv_rows_ref(x, layer_geo, w2d, rows_img, scale=None, shift=None, in_scale=None, a_img_div=1):
    """fp64 of the output rows (image, oy, ox) of a KH x KW / stride / pad convolution of the NHWC input x [n_in, H, W, C]
    (the pre-call clone): the taps of x[image // a_img_div] (times in_scale[image]) against w2d [Cout, KH KW C] in (ky, kx,
    c) order, times scale, plus shift - before residual and ReLU, which the caller adds."""
    kh, kw, stride, pad = layer_geo
    n_in, H, W, C = x.shape
    img, oy, ox = (torch.as_tensor(v, dtype=torch.int64) for v in rows_img)
    ky = torch.arange(kh).repeat_interleave(kw)
    kx = torch.arange(kw).repeat(kh)
    iy = oy[:, None] * stride - pad + ky[None, :]
    ix = ox[:, None] * stride - pad + kx[None, :]
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    src = (img // a_img_div)[:, None] * (H * W) + iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)
    p = x.reshape(-1, C)[src.to(x.device)].cpu().double() * ok[:, :, None].double()       # [R, taps, C]
    if in_scale is not None:
        p = p * in_scale[img.to(in_scale.device)].cpu().double()[:, None, :]
    ref = p.reshape(p.shape[0], -1) @ w2d.double().cpu().T
    if scale is not None:
        ref = ref * scale.cpu().double()
    if shift is not None:
        ref = ref + shift.cpu().double()
    return ref


def _layer_w2d(layer):
    """The packed ConvLayer's own f32 weights as [Cout, KH KW Cin] in (ky, kx, cin) order (the stem's Cin-4 layout: one
    32-float K-tile per filter row = 8 pixels x 4 channels, columns past kw zero)."""
    if layer.cin == 4:
        return layer.w.view(layer.cout_pad, layer.kh, 8, 4)[:layer.cout, :, :layer.kw].reshape(layer.cout, -1)
    return layer.w[:layer.cout, :layer.kh * layer.kw * layer.cin]


def _split_rows(rows, segs):
    """launch rows -> per row (segment, image, oy, ox, row within the segment)."""
    out, base = [], 0
    bounds = []
    for n, h, w in segs:
        bounds.append(base)
        base += n * h * w
    bounds = np.asarray(bounds)
    seg = np.searchsorted(bounds, rows, side='right') - 1
    res = []
    for s_i, (n, h, w) in enumerate(segs):
        loc = rows[seg == s_i] - bounds[s_i]
        res.append((loc // (h * w), (loc % (h * w)) // w, loc % w, loc))
    return res


class _Shadow:
    """The conv entry points of ``ops`` wrapped: each call runs, then its sampled rows are compared with fp64."""

    def __init__(self, ops):
        self.ops = ops
        self.lines, self.calls, self.checked, self.worst = [], 0, 0, []
        self.orig = {n: getattr(ops, n) for n in ('conv2d', 'conv2d_pair', 'conv1x1_dual', 'conv3x3_winograd',
                                                  'conv3x3_winograd_multi', 'pack_winograd')}

    def install(self, monkeypatch):
        ops = self.ops
        sig = inspect.signature(self.orig['pack_winograd'])

        def pack_winograd(*a, **k):
            layer = self.orig['pack_winograd'](*a, **k)
            b = sig.bind(*a, **k)
            b.apply_defaults()
            layer.shadow_src = {n: b.arguments[n] for n in ('weight', 'bias', 'bn', 'eps')}
            return layer
        monkeypatch.setattr(ops, 'pack_winograd', pack_winograd)
        for name in ('conv2d', 'conv2d_pair', 'conv1x1_dual', 'conv3x3_winograd', 'conv3x3_winograd_multi'):
            monkeypatch.setattr(ops, name, self._wrap(name))

    def _wrap(self, name):
        orig, check = self.orig[name], getattr(self, '_' + name)
        sig = inspect.signature(orig)

        def call(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            pre = {n: ([t.clone() for t in v] if isinstance(v, (list, tuple)) else v.clone())
                   for n, v in args.items() if isinstance(v, torch.Tensor) or
                   (isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor))}
            n_rec = len(self.ops.PROFILE)
            res = orig(*a, **k)
            torch.cuda.synchronize()
            recs = [r for r in self.ops.PROFILE[n_rec:] if r['kind'] in ('conv', 'wg_gemm')]
            self.calls += 1
            route = recs[0].get('math', 'f32') if recs else 'f32'
            rng = np.random.default_rng(self.calls)
            checks = check(args, pre, res, rng)
            for label, got, ref, tol in checks:
                r = ref.abs().max().item() if ref.numel() else 0.0
                e = (got.cpu().double() - ref).abs().max().item() if ref.numel() else 0.0
                rel = e / r if r > 0 else e
                self.lines.append(f'{self.calls:3d} {name:22s} {label:34s} {route:3s} rows {ref.shape[0]:5d}  '
                                  f'err/range {rel:.2e}  (bound {tol:.0e})')
                self.worst.append((name, label, route, rel, tol))
            self.checked += 1
            return res
        return call

    # ---- the five entry points: (label, got rows, fp64 rows, bound) per output tensor ----
    def _conv2d(self, a, pre, out, rng):
        layer, x = a['layer'], pre['x']
        n_in, H, W, C = x.shape
        n_img = a['n_img'] if a['n_img'] is not None else n_in * a['a_img_div']
        ho, wo = out.shape[1], out.shape[2]
        count = n_img if a['n_img_dev'] is None else min(n_img, int(a['n_img_dev'].item()))
        rows = _sample([(n_img, ho, wo)], rng, count_rows=count * ho * wo if a['n_img_dev'] is not None else None)
        img, oy, ox, loc = _split_rows(rows, [(n_img, ho, wo)])[0]
        ref = _conv_rows_ref(x, (layer.kh, layer.kw, layer.stride, layer.pad), _layer_w2d(layer), (img, oy, ox),
                             layer.scale, layer.shift, pre.get('in_scale'), a['a_img_div'])
        if 'residual' in pre:
            ref = ref + pre['residual'].reshape(-1, layer.cout)[torch.as_tensor(loc).to(x.device)].cpu().double()
        if layer.relu:
            ref = torch.relu(ref)
        flat = out.reshape(-1, layer.cout)
        if 'out' in pre and a['n_img_dev'] is not None:           # rows past the count keep their bytes
            v = count * ho * wo
            assert torch.equal(flat[v:].view(torch.int32), pre['out'].reshape(-1, layer.cout)[v:].view(torch.int32))
        got = flat[torch.as_tensor(rows).to(flat.device)]
        return [(f'{n_img}x{H}x{W}x{C}->{layer.cout} k{layer.kh}s{layer.stride}', got, ref, 2e-6)]

    def _conv2d_pair(self, a, pre, res, rng):
        layer = a['layer']
        xs, ys = (pre['x0'], pre['x1']), res
        segs = [tuple(y.shape[:3]) for y in ys]
        rows = _sample(segs, rng)
        checks = []
        for t, (img, oy, ox, loc) in enumerate(_split_rows(rows, segs)):
            ref = _conv_rows_ref(xs[t], (layer.kh, layer.kw, layer.stride, layer.pad), _layer_w2d(layer),
                                 (img, oy, ox), layer.scale, layer.shift)
            if layer.relu:
                ref = torch.relu(ref)
            got = ys[t].reshape(-1, layer.cout)[torch.as_tensor(loc).to(ys[t].device)]
            n, H, W, C = xs[t].shape
            checks.append((f'pair{t} {n}x{H}x{W}x{C}->{layer.cout} k{layer.kh}s{layer.stride}', got, ref, 2e-6))
        return checks

    def _conv1x1_dual(self, a, pre, out, rng):
        layer = a['layer']
        x1, x2 = pre['x1'].reshape(-1, layer.cin1), pre['x2'].reshape(-1, layer.cin2)
        M = x1.shape[0]
        rows = _sample([(1, M, 1)], rng)
        idx = torch.as_tensor(rows).to(x1.device)
        src = pre['x2_rows'].long()[idx] if 'x2_rows' in pre else idx
        w = layer.w[:layer.cout].double().cpu()
        ref = x1[idx].cpu().double() @ w[:, :layer.cin1].T + x2[src].cpu().double() @ w[:, layer.cin1:].T + \
            layer.shift.cpu().double()
        if layer.relu:
            ref = torch.relu(ref)
        got = out.reshape(-1, layer.cout)[idx]
        tab = ' strided' if 'x2_rows' in pre else ''
        return [(f'dual{tab} {M}x{layer.cin1}+{layer.cin2}->{layer.cout}', got, ref, 2e-6)]

    @staticmethod
    def _wg_weights(layer):
        s = layer.shadow_src
        w = s['weight'].detach().double().cpu()
        shift = None
        if s['bn'] is not None:
            bn = {k: v.double().cpu() for k, v in s['bn'].items()}
            sc = bn['weight'] / torch.sqrt(bn['running_var'] + s['eps'])
            shift = bn['bias'] - bn['running_mean'] * sc
            if s['bias'] is not None:
                shift = shift + s['bias'].double().cpu() * sc
            w = w * sc[:, None, None, None]
        elif s['bias'] is not None:
            shift = s['bias'].detach().double().cpu()
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), shift

    def _wg_check(self, layer, x, y, rows_t, label, in_scale=None, a_img_div=1):
        w2d, shift = self._wg_weights(layer)
        n, H, W, _ = y.shape
        img, oy, ox, loc = _split_rows(rows_t, [(n, H, W)])[0]
        ref = _conv_rows_ref(x, (3, 3, 1, 1), w2d, (img, oy, ox), None, shift, in_scale, a_img_div)
        if layer.relu:
            ref = torch.relu(ref)
        got = y.reshape(-1, layer.cout)[torch.as_tensor(loc).to(y.device)]
        return (label, got, ref, 1e-5 if layer.m == 4 else 2e-6)

    def _conv3x3_winograd(self, a, pre, y, rng):
        layer, x = a['layer'], pre['x']
        n, H, W, _ = y.shape
        count = n if a['n_img_dev'] is None else min(n, int(a['n_img_dev'].item()))
        m = layer.m
        tw, tiles = (W + m - 1) // m, ((H + m - 1) // m) * ((W + m - 1) // m)

        def tile_row(t):        # one pixel of GEMM row (tile) t: its last one inside the image
            i, r = divmod(int(t), tiles)
            ty, tx = divmod(r, tw)
            return i * H * W + min(ty * m + m - 1, H - 1) * W + min(tx * m + m - 1, W - 1)
        rows = _sample([(n, H, W)], rng, count_rows=count * H * W if a['n_img_dev'] is not None else None,
                       tile_rows=(tile_row, count * tiles))
        return [self._wg_check(layer, x, y, rows, f'wg F({m}x{m}) {n}x{H}x{W}x{layer.cin}->{layer.cout}',
                               pre.get('in_scale'), a['a_img_div'])]

    def _conv3x3_winograd_multi(self, a, pre, res, rng):
        layer, xs, outs = a['layer'], pre['xs'], a['outs']
        checks = []
        for t, (x, y) in enumerate(zip(xs, outs)):
            n, H, W, _ = y.shape
            m = layer.m
            tw, tiles = (W + m - 1) // m, ((H + m - 1) // m) * ((W + m - 1) // m)

            def tile_row(tt, H=H, W=W, tw=tw, tiles=tiles):
                i, r = divmod(int(tt), tiles)
                ty, tx = divmod(r, tw)
                return i * H * W + min(ty * m + m - 1, H - 1) * W + min(tx * m + m - 1, W - 1)
            rows = _sample([(n, H, W)], rng, tile_rows=(tile_row, n * tiles))
            checks.append(self._wg_check(layer, x, y, rows, f'wg multi{t} F({m}x{m}) {n}x{H}x{W}x{layer.cin}->{layer.cout}'))
        return checks


@pytest.mark.parametrize('math', ['h2', 'x3', 'f32'])
def test_every_conv_launch_of_a_cfg3_episode_against_fp64(math, monkeypatch):
    """One cfg3 episode (3-way 3-shot, 800x1333, ResNet-50-C4, seed 0) queued eagerly on one stream by ``detect_device``,
    the way tools/per_launch.py queues it (support branch on the caller's stream), with every call of the five conv entry
    points (conv2d, conv2d_pair, conv1x1_dual, conv3x3_winograd, conv3x3_winograd_multi) shadowed: inputs (and a
    caller's output buffer) cloned before the call, and afterwards a deterministic sample of output rows (image / tensor
    first and last rows, the seam of a pair, both sides of 32 / 64 / 128-row boundaries at the start, middle and last
    tile, border pixels, the last row below a device count, 256 seeded random rows; all columns) computed in fp64 from the
    packed layer's own f32 operands (Winograd layers: the source 3x3 weights, BN and bias attached by the wrapped
    ``pack_winograd``).  Bounds: 2e-6 of the sampled range (the direct gemm_h2 / gemm_x3 tests' bound), 1e-5 for F(4x4)
    Winograd layers (test_winograd_h2_is_as_close_to_fp64_as_x3); rows past a device count keep their bytes where the
    caller passes the output buffer.  The launch list is asserted: under 'h2' the 67 MFMA launches of _H2_EPISODE, 63 on
    conv_pw_h2_kernel (44 convolutions, 19 Winograd GEMMs); 55 on conv_pw_x3_kernel under 'x3'; none under 'f32'."""
    import time
    from fgn_amd import ops
    from fgn_amd.config import fgn_r50_c4_config
    from fgn_amd.detector import FGN
    from fgn_amd.episodes import CONFIGS, make_batch
    from fgn_amd.weights import init_state_dict
    t0 = time.time()
    sh = _Shadow(ops)
    sh.install(monkeypatch)
    cfg = fgn_r50_c4_config(3, 3)
    b = make_batch(0, 1, **CONFIGS['cfg3'])
    e = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    e['img_shape'] = e['img_shape'].cpu()
    prof = ops.ConvProfile()
    ops.PROFILE = prof
    try:
        with ops.gemm_math(math):                        # the layers are packed at the first call
            model = FGN(3, 3, state_dict=init_state_dict(cfg, 0))
            model.use_side_stream = False
            model.detect_device(e['qry_img'], e['spp_imgs'], e['spp_bboxes'], e['spp_isegmaps'], e['img_shape'])
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    print(f'\n[{math}] {sh.calls} conv calls, {len(sh.worst)} output tensors checked, {time.time() - t0:.1f} s')
    for line in sh.lines:
        print(line)
    mf = [r for r in prof if r['kind'] in ('conv', 'wg_gemm')]
    n_all, n_own, n_wg = _EPISODE_COUNTS[math]
    assert sh.checked == sh.calls > 0
    assert len(mf) == n_all, len(mf)
    own = [r for r in mf if r.get('math', 'f32') == math] if math != 'f32' else []
    assert len(own) == n_own and sum(r['kind'] == 'wg_gemm' for r in own) == n_wg
    if math == 'h2':
        got = [(r['kind'], r.get('math', 'f32'), tuple(r['shape'])) for r in mf]
        assert got == _H2_EPISODE
        assert all(r['kernel'].startswith('conv_pw_h2_kernel') for r in own)
    bad = [(n, l, rt, rel, tol) for n, l, rt, rel, tol in sh.worst if not rel <= tol]
    assert not bad, bad
    del model
    torch.cuda.empty_cache()
