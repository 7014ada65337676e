"""Exactly summable operands for the conv / GEMM kernels, and their exact references (tests/test_exact_ref_cpu.py pins
this file; tests/test_hip_conv_exact.py runs the kernels on it).

A GEMM has inputs on which its result depends on neither the order of the sum, nor the tile, nor the arithmetic: when every
product and every partial sum of an output element is a multiple of one power of two (the element's ``unit``) and smaller
than 2^24 units, every f32 operation on the way is exact, and any correct kernel returns the exact result - the f32 MFMA
kernels, the three f16 products of conv_pw_h2_kernel, the six bf16 products of conv_pw_x3_kernel, split-K, two K-groups.
The comparison is ``torch.equal`` against integer arithmetic (float64 ``@`` / ``F.conv2d``: exact below 2^53).

THE CLASS CONDITION, asserted here on the CPU for every output element before anything goes to a GPU:

    mag / unit <= 2^22,    mag = sum_k |a||w| + |shift| + |residual|,   unit = a power of two dividing every term

f32 holds 2^24.  The two spare bits are for whatever alignment the matrix pipe applies inside a 32-deep dot product (it may
align the products of one instruction to their largest before it adds them).  This is a condition, not a measurement:
where a shape cannot meet it the INTEGERS shrink (the budgets of ``make``), never the condition.  ``unit`` is 2^(row exponent + column
exponent + the exponent all operands share): every operand is an integer times its exponent, so this divides every term,
and it is the largest such power of two unless every term of an element happens to be even.

Operand classes (activations post-ReLU style, about half zeros):
 small          |a| <= 7, |w| <= 7: exact for every arithmetic.
 two_plane      ceil(K / 20) reduction positions (5 %) hold activations of more than 11 significant bits, 2048 p + q: one
                per row as wide as the budget allows - its bit length cycles from 12 up to ``a_bits`` over the rows - the
                others 12 - 13 bits; the weights there are +-1.  As many other positions hold one wide weight per column
                (bit length cycling up to ``w_bits``) against activations of 0 / 1.  Everywhere else |a| <= 7 and the
                weights are as wide as the rest of the budget allows.  (a_bits, w_bits) = (22, 11) for h2 - the activation
                lo plane in use, the weight lo plane zero, the dropped la * lb term zero -, (16, 16) for x3 - the third
                planes zero, so the dropped a2 b3, a3 b2, a3 b3 vanish -, (12, 12) for the f32 kernels.
 two_plane_w    two_plane with the bit widths of the operands exchanged: for h2 the WEIGHT lo plane is in use (ha * lb, the
                one product two_plane leaves at zero), the activation lo plane is zero and la * lb vanishes again.
 rows_apart     row r times 2^e[r], e cycling inside every 32 consecutive rows: 0..15 with two_plane activations (the
                documented "within 2^15 of the maximum keeps both planes"), or 0..24 with activations of at most 11 bits
                (h alone holds the value).  No shift: one number per column cannot be small beside every row.
 columns_apart  weight column n times 2^f[n], f cycling through -20..20.
 k_steps        the magnitude changes between K-tiles of 32: 2^3 above the ones before (leaves the f16 range: the wave
                picks a new scale and its accumulators follow), 2^2 above (the scale stays), 2^10 below; the first K-tile
                of every third 32-row block is zero (the scale comes from a later tile).  ``kgroups = 2``: even and odd
                K-tiles - the two K-groups of conv_pw_h2_kernel's KG = 2 instance - follow patterns of their own.
 Every class once more with all operands times 2^-9 (``scaled``): nothing may depend on the values being integers."""
import torch
import torch.nn.functional as F

LIMIT = float(2 ** 22)
CLASSES = ('small', 'two_plane', 'two_plane_w', 'rows_apart15', 'rows_apart24', 'columns_apart', 'k_steps')
ARITH_BITS = {'h2': (22, 11), 'x3': (16, 16), 'f32': (12, 12)}
_K_PAT = (0, 3, 5, -5)                     # exponent of K-tile t (one K-group): +3 new scale, +2 scale stays, -10
_K_PAT2 = ((0, 3, 5, -5), (4, -6, -3, -1))  # two K-groups: tile t belongs to group t % 2, step t // 2


def _ints(g, shape, hi, zeros=False, signed=True):
    """integers in [-hi, hi] (``signed``) / [0, hi], none of them 0 unless ``zeros`` (then about half are)"""
    v = torch.randint(1, hi + 1, shape, generator=g).double()
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    if zeros:
        v = v * torch.randint(0, 2, shape, generator=g).double()
    return v


def _wide(g, n, cap, lo_bits, idx):
    """``n`` odd integers whose bit length cycles with ``idx`` from ``lo_bits`` to that of ``cap``, each <= cap"""
    top = int(cap).bit_length()
    bits = lo_bits + idx % max(top - lo_bits + 1, 1)
    hi = torch.minimum(2.0 ** bits.double() - 1, torch.tensor(float(cap), dtype=torch.float64))
    lo = 2.0 ** (bits.double() - 1)
    v = torch.floor(lo + torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo + 1)).clamp_(max=float(cap))
    return torch.where(v % 2 == 0, (v - 1).clamp_(min=1.0), v)


def tile_exponents(kt, kgroups):
    """the k_steps exponent of each of ``kt`` K-tiles, shifted so that the smallest is 0"""
    e = [(_K_PAT2[t % 2][(t // 2) % 4] if kgroups == 2 else _K_PAT[t % 4]) for t in range(kt)]
    return [v - min(e) for v in e]


def make(rows, K, N, cls, arith='h2', taps=1, kgroups=1, seed=0, spread=1):
    """Integer operands of class ``cls`` for a reduction over ``taps`` x ``K`` (a convolution reads ``taps`` rows of the
    activations per output element; a GEMM one) -> dict: a [rows, K], w [N, taps, K], the row / column exponents e [rows],
    f [N] (already applied), shift [N] (None under rows_apart) and the generator g.  float64, integers times powers of two.
    The budget per output element, in units: 3 * 2^20 for the wide activations, 2^18 for the wide weights (the other way
    round where the weights are the wider operand), 2^19 for the rest, 2^17 each for shift and residual - 2^22 in all.  ``spread``: how far the activation rows of one output element may
    lie apart (a convolution's patch under rows_apart): the budgets shrink by it."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 31 * K + N + 17 * CLASSES.index(cls))
    tb = taps * spread
    a_bits, w_bits = ARITH_BITS[arith]
    base = cls
    e = torch.zeros(rows, dtype=torch.float64)
    f = torch.zeros(N, dtype=torch.float64)
    if cls == 'two_plane_w':
        base, a_bits, w_bits = 'two_plane', w_bits, a_bits
    elif cls == 'rows_apart15':
        base, e = 'two_plane', (torch.arange(rows) * 7 % 32 % 16).double()          # 0..15 inside every 32 rows
    elif cls == 'rows_apart24':
        base, a_bits = 'two_plane', min(a_bits, 11)
        e = (torch.arange(rows) * 11 % 32 % 25).double()                             # 0..24
    elif cls == 'columns_apart':
        base, f = 'small', ((torch.arange(N) * 13) % 41 - 20).double()               # -20..20
    if base == 'small':
        a = _ints(g, (rows, K), 7, zeros=True, signed=False)
        w = _ints(g, (N, taps, K), 7)
    elif base == 'k_steps':
        te = tile_exponents(K // 32, kgroups)
        hi = max(int((2 ** 21 / (tb * K * 2.0 ** max(te))) ** 0.5), 1)               # taps K hi^2 2^max(te) <= 2^21
        hi = min(hi, 7)
        a = _ints(g, (rows, K), hi, zeros=True, signed=False)
        w = _ints(g, (N, taps, K), hi)
        a = a * (2.0 ** torch.tensor(te, dtype=torch.float64)).repeat_interleave(32)[None, :]
        blk = torch.arange(rows) // 32
        a[blk % 3 == 1, :32] = 0.0                                                   # the scale comes from a later K-tile
    else:                                                                            # two_plane
        n_w = -(-K // 20)
        perm = torch.randperm(K, generator=g)
        ka, kw = perm[:n_w], perm[n_w:2 * n_w]
        a_cap, w_cap = 2 ** a_bits - 1, 2 ** w_bits - 1
        oth = min(8191, a_cap)
        ba, bw = (3 * 2 ** 20, 2 ** 18) if a_bits >= w_bits else (2 ** 18, 3 * 2 ** 20)      # the wider operand's share
        a1 = min(a_cap, ba // tb - (n_w - 1) * oth)
        w1 = min(w_cap, bw // tb - 7 * (n_w - 1))
        wr = min(w_cap, 2 ** 19 // (7 * tb * K))
        assert a1 >= 1 and w1 >= 1 and wr >= 1, (rows, K, N, cls, taps)
        a = _ints(g, (rows, K), 7, zeros=True, signed=False)
        w = _ints(g, (N, taps, K), wr)
        # wide activations: 2048 p + q at the positions ka, one of them per row as wide as the budget allows
        if oth > 2048:
            a[:, ka] = 2048.0 * torch.randint(1, oth // 2048 + 1, (rows, n_w), generator=g).double() + \
                torch.randint(1, 2048, (rows, n_w), generator=g).double()
        else:
            a[:, ka] = _ints(g, (rows, n_w), oth, signed=False)
        r = torch.arange(rows)
        a[r, ka[r % n_w]] = _wide(g, rows, a1, min(12, a_bits), r // n_w)
        w[:, :, ka] = _ints(g, (N, taps, n_w), 1)
        # wide weights at the positions kw, one per column (and tap), against activations of 0 / 1
        a[:, kw] = torch.randint(0, 2, (rows, n_w), generator=g).double()
        w[:, :, kw] = _ints(g, (N, taps, n_w), 7)
        n = torch.arange(N)
        for t in range(taps):
            w[n, t, kw[(n + t) % n_w]] = _wide(g, N, w1, min(9, w_bits), n // n_w) * \
                (torch.randint(0, 2, (N,), generator=g).double() * 2 - 1)
    a = a * (2.0 ** e)[:, None]
    w = w * (2.0 ** f)[:, None, None]
    shift = None if cls.startswith('rows_apart') else _ints(g, (N,), 2 ** 17) * 2.0 ** f
    return dict(a=a, w=w, e=e, f=f, shift=shift, g=g)


def residual(o, unit):
    """integers of up to 17 bits in each element's unit"""
    return _ints(o['g'], tuple(unit.shape), 2 ** 17) * unit


def check_class(mag, unit, tag=''):
    """THE condition: mag / unit <= 2^22 for every output element (module docstring); and mag itself stays in f32"""
    worst = (mag / unit).max().item()
    assert worst <= LIMIT, f'{tag}: mag / unit = 2^{torch.log2(torch.tensor(worst)).item():.2f} > 2^22'
    assert mag.max().item() < 2.0 ** 120 and unit.min().item() > 2.0 ** -120, tag


def gemm_case(rows, K, N, cls, arith='h2', scaled=False, kgroups=1, groups=1, seed=0):
    """A GEMM of class ``cls`` -> dict of f32 tensors x [groups, rows, K], w [groups, N, K], shift [N] or None (rows_apart),
    res [groups, rows, N], and float64 prod = x w^T, full = relu(prod + shift + res), mag, unit [groups, rows, N].  The
    condition is asserted for ``full``'s terms (it covers ``prod``); the references survive a round trip through f32."""
    xs, ws, prods, mags, units = [], [], [], [], []
    shift = None
    for gi in range(groups):
        o = make(rows, K, N, cls, arith, 1, kgroups, seed + 101 * gi)
        a, w = o['a'], o['w'][:, 0]
        if gi == 0:
            shift, g0 = o['shift'], o
        s = 2.0 ** -9 if scaled else 1.0
        xs.append(a * s)
        ws.append(w * s)
        units.append(2.0 ** (o['e'][:, None] + o['f'][None, :]) * s * s)
        prods.append(xs[-1] @ ws[-1].T)
        mags.append(xs[-1].abs() @ ws[-1].abs().T)
    x, w, prod, mag, unit = (torch.stack(t) for t in (xs, ws, prods, mags, units))
    if shift is not None:
        shift = shift * (s * s)
    res = residual(g0, unit)
    mag = mag + res.abs() + (0.0 if shift is None else shift.abs())
    check_class(mag, unit, f'{cls} {rows}x{K}->{N}')
    full = torch.relu(prod + res + (0.0 if shift is None else shift))
    for t in (x, w, prod, full, res):
        assert torch.equal(t.float().double(), t)
    return dict(x=x.float(), w=w.float(), shift=None if shift is None else shift.float(), res=res.float(), prod=prod, full=full,
                mag=mag, unit=unit)


def x_exponents(W, stride=1):
    """rows_apart for a convolution: the exponent of an input pixel depends on its column alone, a triangle wave 0..15 of
    period 30, so the nine pixels of a 3x3 patch lie within 2^2 of each other while 32 consecutive output pixels of a row
    (stride 2: 16 of them) pass through all of 0..15"""
    x = torch.arange(W)
    return ((x % 30) - 15).abs().double()


def conv_case(shapes, cin, cout, k, stride, pad, cls, arith='h2', scaled=False, seed=0, scale_pow2=False, bias=True, res=False,
              relu=True, real_cin=None, ways=1):
    """A convolution of class ``cls`` (a name of CLASSES, or 'rows_apart': ``x_exponents``; rows_apart15 / 24 and k_steps for
    1x1 only) on NHWC tensors of ``shapes`` = [(n, H, W), ...] with one weight -> dict: xs (f32 NHWC), wt [cout, cin, k, k]
    f32, scale [cout] (powers of two 1 / 2 / 4, or None), shift [cout] or None, ress (f32 NHWC or None), refs (float64 NHWC)
    = relu?(conv * scale + shift + res), in_scale.  ``real_cin``: channels past it are zero (the stem's fourth).  ``ways``
    > 1: every input image is read by ``ways`` output images, each under a per-(image, channel) input scale of 1 / 2 / 4
    (in_scale [n ways, cin]; the operands' budget shrinks by the 4)."""
    taps = k * k
    rows = sum(n * H * W for n, H, W in shapes)
    conv_rows = cls == 'rows_apart'
    assert k == 1 or cls in ('small', 'two_plane', 'columns_apart', 'rows_apart')
    o = make(rows, cin, cout, 'two_plane' if conv_rows else cls, arith, taps, 1, seed, spread=4 if conv_rows or ways > 1 else 1)
    s = 2.0 ** -9 if scaled else 1.0
    a, w = o['a'] * s, o['w'] * s                                      # w [cout, taps, cin]
    if real_cin is not None:
        a[:, real_cin:] = 0.0
    wt = w.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()
    sc = 2.0 ** (torch.arange(cout) % 3).double() if scale_pow2 else None
    shift = None if (cls.startswith('rows_apart') or not bias) else o['shift'] * (s * s) * (1.0 if sc is None else sc)
    xs, refs, ress, vecs = [], [], [], []
    r0 = 0
    for n, H, W in shapes:
        x = a[r0:r0 + n * H * W].view(n, H, W, cin).clone()
        ex = o['e'][r0:r0 + n * H * W].view(n, 1, H, W).clone()        # (zero unless rows_apart15 / 24: applied by make)
        r0 += n * H * W
        if conv_rows:
            ex = ex + x_exponents(W)[None, None, None, :]
            x = x * (2.0 ** ex[:, 0, :, :, None])
        xe, vec = x, None
        if ways > 1:
            vec = 2.0 ** torch.randint(0, 3, (n * ways, cin), generator=o['g']).double()
            xe = x.repeat_interleave(ways, 0) * vec[:, None, None, :]
            ex = ex.repeat_interleave(ways, 0)
        cols = F.unfold(xe.permute(0, 3, 1, 2), k, padding=pad, stride=stride)           # [n, cin k k, Ho Wo]
        ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        w2 = wt.reshape(cout, -1)
        y = (w2 @ cols).view(-1, cout, ho, wo)
        mag = (w2.abs() @ cols.abs()).view(-1, cout, ho, wo)
        eu = -F.max_pool2d(-ex, k, stride, pad) if k > 1 else ex[:, :, ::stride, ::stride]      # the smallest exponent of a patch
        unit = 2.0 ** (eu + o['f'][None, :, None, None]) * (s * s)
        if sc is not None:
            y, mag, unit = y * sc[None, :, None, None], mag * sc[None, :, None, None], unit * sc[None, :, None, None]
        if shift is not None:
            y, mag = y + shift[None, :, None, None], mag + shift.abs()[None, :, None, None]
        r = None
        if res:
            r = residual(o, unit.expand_as(y))
            y, mag = y + r, mag + r.abs()
        check_class(mag, unit.expand_as(mag), f'{cls} conv {n}x{H}x{W}x{cin}->{cout} k{k}/{stride}')
        if relu:
            y = torch.relu(y)
        assert torch.equal(y.float().double(), y) and torch.equal(x.float().double(), x)
        xs.append(x.float().contiguous())
        refs.append(y.permute(0, 2, 3, 1).contiguous())
        ress.append(None if r is None else r.permute(0, 2, 3, 1).float().contiguous())
        vecs.append(None if vec is None else vec.float())
    assert torch.equal(wt.float().double(), wt)
    return dict(xs=xs, wt=wt.float(), scale=None if sc is None else sc.float(), shift=None if shift is None else shift.float(),
                ress=ress, refs=refs, in_scale=vecs)


# ----------------------------------------------------------------------------------------------------------------------
# plain restatements of the two plane arithmetics: the references' witness that a mismatch on the GPU is the kernel's
# ----------------------------------------------------------------------------------------------------------------------
def _unswizzle(img16, G, planes, npad, K):
    """[G][K / 32][planes][npad][4][8] 16-bit patterns of ops.pack_h2 / pack_x3 (16x16x32 form) -> [G, planes, npad, K]"""
    pl = img16.view(G, K // 32, planes, npad, 4, 8).permute(0, 2, 3, 1, 4, 5)
    n = torch.arange(npad)
    swz = torch.tensor([0, 3, 2, 1])[(n >> 2) & 3]
    src = torch.arange(4)[None, :] ^ swz[:, None]                      # the XOR is its own inverse
    pl = torch.gather(pl, 4, src[None, None, :, None, :, None].expand(G, planes, npad, K // 32, 4, 8))
    korder = torch.tensor([4 * g + j if j < 4 else 16 + 4 * g + j - 4 for g in range(4) for j in range(8)])
    out = torch.empty(G, planes, npad, K // 32, 32, dtype=pl.dtype)
    out[..., korder] = pl.reshape(G, planes, npad, K // 32, 32)
    return out.reshape(G, planes, npad, K)


def unpack_h2(image, G, N, K):
    """ops.pack_h2's image -> hi, lo [G, npad, K] (float64 values of the f16 planes), inv [G, npad] float64"""
    npad = (N + 127) // 128 * 128
    nb = G * 2 * npad * K * 2
    pl = _unswizzle(image[:nb].cpu().view(torch.int16), G, 2, npad, K).contiguous().view(torch.float16).double()
    inv = image[nb:].cpu().view(torch.float32).view(G, npad).double()
    return pl[:, 0], pl[:, 1], inv


def unpack_x3(image, G, N, K):
    """ops.pack_x3's image (16x16x32 form) -> the three bf16 planes [3][G, npad, K] as float64"""
    npad = (N + 127) // 128 * 128
    pl = _unswizzle(image.cpu().view(torch.int16), G, 3, npad, K).contiguous()
    pl = (pl.to(torch.int32) << 16).view(torch.float32).double()
    return pl[:, 0], pl[:, 1], pl[:, 2]


def h2_scales(x, block, kgroups=1):
    """The activation scale of conv_pw_h2_kernel per ``block`` rows and K-tile (x [rows, K] float64 -> [rows, K / 32]): per
    K-group, the first K-tile with a non-zero element puts the block's largest |x| of that tile into [2^13, 2^14); a later
    tile with an element above 65504 / S picks a new S from its own maximum (csrc/conv_pw_h2.h, ``adapt``)."""
    rows, K = x.shape
    kt = K // 32
    nb = -(-rows // block)
    xp = torch.zeros(nb * block, K, dtype=torch.float64)
    xp[:rows] = x.abs()
    tmax = xp.view(nb, block, kt, 32).amax(dim=(1, 3))                  # [nb, kt]
    S = torch.ones(nb, kt, dtype=torch.float64)
    for kg in range(kgroups):
        cur = torch.ones(nb, dtype=torch.float64)
        have = torch.zeros(nb, dtype=torch.bool)
        for t in range(kg, kt, kgroups):
            m = tmax[:, t]
            new = (m > 0) & (~have | (m > 65504.0 / cur))
            ns = 2.0 ** (13.0 - torch.floor(torch.log2(torch.where(m > 0, m, torch.ones_like(m)))))
            cur = torch.where(new, ns, cur)
            have = have | new
            S[:, t] = cur
    return S.repeat_interleave(block, 0)[:rows]


def h2_restate(x, hi, lo, inv, N, block=32, kgroups=1):
    """conv_pw_h2_kernel's arithmetic in plain terms: x [rows, K] f32, the planes and inverse column scales of ``unpack_h2``
    ([npad, K], [npad]) -> [rows, N] float64: ha hb + ha lb + la hb per K-tile at that tile's scale, the scales taken out."""
    xd = x.double()
    S = h2_scales(xd, block, kgroups).repeat_interleave(32, 1)           # [rows, K]
    xs = (xd * S).float()
    assert torch.equal(xs.double(), xd * S)
    h = xs.to(torch.float16)
    assert torch.isfinite(h).all()
    l = (xs - h.float()).to(torch.float16)
    ha, la = h.double() / S, l.double() / S
    y = ha @ hi[:N].T + ha @ lo[:N].T + la @ hi[:N].T
    return y * inv[:N][None, :]


def x3_planes(v):
    """f32 -> its three bf16 truncation planes (float64), as ops.pack_x3 and conv_pw_x3_kernel split"""
    out, r = [], v.float().contiguous()
    for _ in range(3):
        p = (r.view(torch.int32) & -65536).view(torch.float32)
        out.append(p.double())
        r = r - p
    return out


def x3_restate(x, planes_w, N):
    """conv_pw_x3_kernel's six kept terms: a1 b1 + a1 b2 + a2 b1 + a1 b3 + a2 b2 + a3 b1 (header of csrc/conv_pw_x3.h)"""
    a1, a2, a3 = x3_planes(x)
    b1, b2, b3 = (p[:N].T for p in planes_w)
    return a1 @ b1 + a1 @ b2 + a2 @ b1 + a1 @ b3 + a2 @ b2 + a3 @ b1


# ----------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_hip_conv_exact.py (the CPU test walks the same lists)
# ----------------------------------------------------------------------------------------------------------------------
# conv_pw_h2_kernel, direct entry: tile code, rows, N, K (tests/test_hip_h2_body.py::_GEMM_CASES; the ragged _H2_SHAPES)
H2_GEMM = [
    (64, 6203, 1024, 64), (64, 6203, 1024, 96), (64, 6203, 1024, 160), (64, 6203, 132, 96),
    (128, 8317, 1024, 64), (128, 8317, 1024, 160), (264, 98425, 64, 64),
    (1064, 2111, 1024, 128), (1064, 2111, 1024, 320),
    (64, 130, 260, 96), (128, 130, 260, 96), (64, 3001, 76, 64), (128, 3001, 76, 64), (264, 3001, 52, 64),
]
# grouped: tile code, groups, rows of a group, valid rows, K, N
H2_GROUPED = [(64, 4, 256, 70, 64, 256), (128, 4, 256, 70, 64, 256), (264, 4, 256, 70, 64, 64)]
# conv_pw_x3_kernel: groups, rows of a group, valid rows, K, N (the last: 1040 tiles of 64 x 128 on the persistent grid)
X3_GEMM = [(1, 3001, 3001, 64, 76), (1, 130, 130, 96, 260), (36, 256, 201, 128, 132), (1, 8317, 8317, 64, 1024)]
X3_CLASSES = ('small', 'two_plane', 'columns_apart')
# fgn_gemm_tn_f32: R, M, N (tests/test_hip_train.py; 6272 and 5000 rows shrunk to 520: still two row slabs)
TN_GEMM = [(520, 1024, 512), (441, 512, 4608), (200, 1024, 9216), (1000, 76, 1024), (37, 8, 12), (300, 1024, 4),
           (520, 4, 256), (33, 64, 64)]
# fgn_gemm_small_f32: m, k, n, trans_a, stride_pad
SMALL_GEMM = [(6, 384, 1024, True, 0), (384, 6, 1024, False, 0), (190, 75, 1024, False, 1), (1, 1, 5, False, 0),
              (7, 33, 3, True, 0)]


def h2_block(bm):
    """rows that share one activation scale under tile code ``bm``: a wave's 32 RB rows (RB = 2 on the 128 x 128 tile only)"""
    return 64 if bm == 128 else 32


def grad_case(R, M, N, seed=0):
    """gemm_tn / gemm_small: class small with rows_apart applied ALONG THE REDUCTION: row r of both operands' reduction
    times 2^(r % 5) and 2^((3 r) % 4): a [R, M], b [R, N] float64 and a^T b; the condition with unit 1."""
    g = torch.Generator().manual_seed(seed + R + 3 * M + 5 * N)
    hi = 7 if R * 49 * 128 <= LIMIT else (3 if R * 9 * 128 <= LIMIT else 1)
    a = _ints(g, (R, M), hi, zeros=True) * (2.0 ** (torch.arange(R) % 5).double())[:, None]
    b = _ints(g, (R, N), hi) * (2.0 ** (torch.arange(R) * 3 % 4).double())[:, None]
    ref = a.T @ b
    check_class(a.abs().T @ b.abs(), torch.ones_like(ref), f'grad {R}x{M}x{N}')
    assert torch.equal(ref.float().double(), ref)
    return a.float(), b.float(), ref


# the convolutions of tests/test_hip_conv_exact.py through the product's entries: name -> (conv_case arguments, classes)
ROW_CLASSES = CLASSES                                   # 1x1 launches: rows are pixels, every GEMM class applies
CONV_CLASSES = ('small', 'two_plane', 'rows_apart')     # 3x3 on conv_pw_h2_kernel (tests/test_hip_h2_body.py's pair)
F32_CLASSES = ('small', 'two_plane', 'columns_apart')
# tests/test_hip_conv.py::CASES: n, cin, h, w, cout, k, stride, pad, bn, bias, residual, relu
F32_CASES = [
    (2, 64, 17, 23, 64, 1, 1, 0, True, False, False, True),
    (2, 64, 17, 23, 256, 1, 1, 0, True, False, True, True),
    (1, 128, 20, 31, 128, 3, 2, 1, True, False, False, True),
    (3, 256, 7, 7, 128, 3, 1, 1, True, False, False, True),
    (1, 256, 9, 13, 75, 1, 1, 0, False, True, False, False),
    (2, 512, 8, 8, 1024, 1, 2, 0, True, False, False, False),
    (1, 32, 40, 50, 32, 3, 1, 1, False, True, False, True),
]
# n, h, w, cin, cout, k: the three shapes of tests/test_hip_conv.py::test_split_k_* - of which the plan splits only the first
# since it stopped splitting reductions of fewer than 32 K-tiles - and a 1x1 of exactly 32 K-tiles (the plan's other branch)
SPLIT_K = [(40, 7, 7, 256, 384, 3), (2, 30, 41, 128, 256, 1), (1, 33, 47, 64, 128, 3), (1, 25, 40, 1024, 256, 1)]
PAIR_F32 = [(128, 128, 3, 2), (256, 512, 1, 2), (64, 64, 3, 1), (4, 64, 7, 2)]                # cin, cout, k, stride
PAIR_F32_SHAPES = [(1, 40, 67), (9, 32, 32)]
PAIR_H2_SHAPES = [(1, 80, 80), (2, 5, 7)]


def conv_specs():
    """name -> (keyword arguments of ``conv_case`` but class / scaled, the classes the GPU file runs it with)"""
    sp = {}
    for i, (n, cin, h, w, cout, k, stride, pad, bn, bias, res, relu) in enumerate(F32_CASES):
        sp[f'f32_case{i}'] = (dict(shapes=[(n, h, w)], cin=cin, cout=cout, k=k, stride=stride, pad=pad, arith='f32', seed=i,
                                   scale_pow2=bn, bias=True, res=res, relu=relu), F32_CLASSES)
    sp['f32_stem'] = (dict(shapes=[(2, 37, 53)], cin=4, cout=64, k=7, stride=2, pad=3, arith='f32', seed=11, scale_pow2=True,
                           relu=True, real_cin=3), ('small', 'two_plane'))
    sp['f32_in_scale'] = (dict(shapes=[(2, 9, 11)], cin=64, cout=96, k=3, stride=1, pad=1, arith='f32', seed=12, relu=True,
                               ways=3), F32_CLASSES)
    for i, (n, h, w, cin, cout, k) in enumerate(SPLIT_K):
        sp[f'f32_splitk{i}'] = (dict(shapes=[(n, h, w)], cin=cin, cout=cout, k=k, stride=1, pad=k // 2, arith='f32', seed=20 + i,
                                     res=True, relu=True), F32_CLASSES)
    sp['f32_persist'] = (dict(shapes=[(1, 4097, 1)], cin=64, cout=1024, k=1, stride=1, pad=0, arith='f32', seed=30, res=True,
                              relu=False), F32_CLASSES)
    for i, (cin, cout, k, stride) in enumerate(PAIR_F32):
        sp[f'f32_pair{i}'] = (dict(shapes=PAIR_F32_SHAPES, cin=cin, cout=cout, k=k, stride=stride, pad=k // 2, arith='f32',
                                   seed=40 + i, scale_pow2=True, relu=True, real_cin=3 if cin == 4 else None),
                              ('small', 'two_plane'))
    for stride in (1, 2):
        sp[f'h2_pair_s{stride}'] = (dict(shapes=PAIR_H2_SHAPES, cin=64, cout=1024, k=3, stride=stride, pad=1, arith='h2',
                                         seed=50 + stride, scale_pow2=True, relu=True), CONV_CLASSES)
    sp['h2_device_count'] = (dict(shapes=[(100, 7, 7)], cin=64, cout=1024, k=1, stride=1, pad=0, arith='h2', seed=60,
                                  scale_pow2=True, res=True, relu=True), ROW_CLASSES)
    return sp


_conv_cache = {}


def conv_named(name, cls, scaled):
    """``conv_case`` of a name of ``conv_specs``, once per (name, class, scaled) and never written"""
    key = (name, cls, scaled)
    if key not in _conv_cache:
        _conv_cache[key] = conv_case(cls=cls, scaled=scaled, **conv_specs()[name][0])
    return _conv_cache[key]


# the fused conv3 + shortcut: rows, Cin1, Cin2, Cout, arithmetic (h2: the operand switches inside the K loop, K-tile 2 of 4)
DUAL = [(6203, 64, 64, 1024, 'h2'), (5000, 32, 96, 132, 'f32'), (777, 128, 32, 64, 'f32')]


def dual_case(rows, cin1, cin2, cout, arith, cls, scaled):
    """conv1x1_dual: a GEMM over [y | x] whose weight columns are the FOLDED weights; the raw weights are those divided by
    the BatchNorm scales sc1 / sc2 (1 or 2 per channel: exact), the float64 statistics make the fold return them.
    -> gemm_case's dict and w1, bn1, w2, bn2 for ops.pack_conv_dual (float64 statistics)."""
    c = gemm_case(rows, cin1 + cin2, cout, cls, arith, scaled, seed=70)
    wf = c['w'][0].double()
    out = dict(c)
    shift = torch.zeros(cout, dtype=torch.float64) if c['shift'] is None else c['shift'].double()
    for j, (lo, hi) in enumerate(((0, cin1), (cin1, cin1 + cin2))):
        sc = 1.0 + ((torch.arange(cout) + j) % 2).double()
        var = 0.5 + (torch.arange(cout) % 7).double() / 8
        q = torch.sqrt(var + 1e-5)
        bn = dict(weight=sc * q, bias=shift if j == 0 else torch.zeros(cout, dtype=torch.float64),
                  running_mean=torch.zeros(cout, dtype=torch.float64), running_var=var)
        assert torch.equal(bn['weight'] / torch.sqrt(bn['running_var'] + 1e-5), sc)
        out[f'w{j + 1}'] = (wf[:, lo:hi] / sc[:, None]).float().view(cout, hi - lo, 1, 1)
        out[f'bn{j + 1}'] = bn
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the Winograd path: the grouped-GEMM entry points alone, and whole convolutions exact through all four stages
# (tests/test_hip_wg_exact.py runs them, tests/test_wg_exact_cpu.py pins them)
# ----------------------------------------------------------------------------------------------------------------------
WG_LIMIT = float(2 ** 24)          # the transform stages: plain f32 adds and fmaf, no matrix pipe - all of f32's 24 bits
# groups, t_pad, valid rows, K, N, n_img, tiles_per_img (n_img * tiles_per_img == valid), the row tile fgn_h2_row_tile /
# fgn_x3_row_tile must return for it (0: the f32 entry only - the image entries refuse the launch)
WG_GEMM = [
    (36, 128, 100, 64, 384, 25, 4, 64),        # 64-row tile, two K-tiles, 72 x 3 = 216 tiles
    (16, 256, 201, 128, 384, 67, 3, 64),       # 64 x 3 = 192 tiles: exactly the threshold; valid ends inside the fourth tile
    (36, 128, 100, 64, 132, 25, 4, 0),         # 132 of 256 columns: below 70 % - refused; the f32 entry's column guard
    (36, 256, 250, 256, 768, 125, 2, 128),     # K >= 256, rows128 == rows64, 36 x 2 x 6 = 432 >= 400: 128 rows
    (16, 640, 640, 256, 640, 40, 16, 128),     # F(2x2)'s group count: 16 x 5 x 5 = 400, exactly the threshold
    (36, 128, 100, 64, 128, 25, 4, 0),         # 72 tiles: too few
    (16, 128, 37, 32, 8, 37, 1, 0),            # K < 64, Cout < a tile
]
WG_GEMM_CLASSES = {'h2': CLASSES, 'x3': X3_CLASSES, 'f32': F32_CLASSES}
_wg_gemm_cache = {}


def wg_gemm_case(i, cls, arith, scaled):
    """``gemm_case`` of the valid rows of WG_GEMM[i] with per-group operands, once per (shape, class, arithmetic) and never
    written.  ``scaled`` is derived from the unscaled case: the same draws times 2^-9 (products times 2^-18) - exactly
    what ``gemm_case(scaled=True)`` computes, every factor being a power of two - so that the two 128-row shapes (1.8 GMAC
    of float64 each, and as much again for ``mag``) are multiplied once.  -> x [groups, valid, K], w [groups, N, K] f32,
    prod [groups, valid, N] float64."""
    key = (i, cls, arith)
    if key not in _wg_gemm_cache:
        groups, _, valid, K, N = WG_GEMM[i][:5]
        c = gemm_case(valid, K, N, cls, arith, False, groups=groups, seed=300 + i)
        assert not torch.equal(c['w'][0], c['w'][1])                    # per-group weights differ
        _wg_gemm_cache[key] = dict(x=c['x'], w=c['w'], prod=c['prod'])
    c = _wg_gemm_cache[key]
    if not scaled:
        return c
    s = 2.0 ** -9
    out = dict(x=c['x'] * s, w=c['w'] * s, prod=c['prod'] * (s * s))
    assert torch.equal(out['x'].double() @ out['w'].double()[..., :8, :].transpose(1, 2), out['prod'][..., :8])
    return out


def wg_counts(n_img, tiles_per_img, tile):
    """The device counts of a grouped launch: none, n_img, one whose last row lies inside a row tile, one whose last row
    ends a row tile (None where no count below n_img does), 0, n_img + 2 (clamped to n_img)."""
    inside = next(c for c in range(1, n_img) if (c * tiles_per_img) % tile)
    edge = next((c for c in range(1, n_img) if (c * tiles_per_img) % tile == 0), None)
    return [None, n_img, inside] + ([] if edge is None else [edge]) + [0, n_img + 2]


def wg_scaled_g(m):
    """(s, s G) with s G an integer matrix: s = 2 for F(2x2), 15 for F(4x4) (tests/_wg_ref.py's rationals)"""
    import _wg_ref
    s = 2 if m == 2 else 15
    sg = torch.tensor([[float(v * s) for v in row] for row in _wg_ref.G[m]], dtype=torch.float64)
    assert torch.equal(sg, sg.round())
    return s, sg


# whole convolutions: name -> m, shapes [(n, H, W), ...], cin, cout, operand kind, a_img_div, device counts (None: no
# count), the route of the grouped GEMM under gemm_math('h2') and its row tile (under 'x3': the same tile on
# conv_pw_x3_kernel; under 'f32' always the f32 entry)
WG_CONV = {
    'f4_ragged': (4, [(2, 13, 21)], 64, 384, 'sparse', 1, (None,), 'h2', 64),
    'f4_counts': (4, [(5, 29, 29)], 64, 128, 'sparse', 1, (None, 5, 3, 0), 'h2', 64),
    'f4_guided': (4, [(1, 13, 21)], 128, 384, 'sparse', 3, (None,), 'h2', 64),
    'f4_rois': (4, [(37, 7, 7)], 64, 64, 'sparse', 1, (None, 23), 'f32', 0),
    'f4_small0': (4, [(1, 7, 9)], 32, 8, 'sparse', 1, (None,), 'f32', 0),
    'f4_small1': (4, [(3, 5, 3)], 32, 32, 'sparse', 1, (None,), 'f32', 0),
    'f4_small2': (4, [(1, 1, 1)], 32, 4, 'sparse', 1, (None,), 'f32', 0),
    'f2_dense': (2, [(1, 29, 31)], 64, 384, 'dense', 1, (None,), 'h2', 64),
    'f2_wide': (2, [(1, 29, 31)], 256, 384, 'wide', 1, (None,), 'h2', 64),
    'f2_counts': (2, [(6, 7, 9)], 32, 32, 'dense', 1, (None, 0, 1, 5, 6, 9), 'f32', 0),
    'f4_pair': (4, [(2, 13, 10), (3, 7, 9)], 64, 384, 'sparse', 1, (None,), 'h2', 64),
    'f2_pair': (2, [(2, 13, 10), (3, 7, 9)], 64, 384, 'dense', 1, (None,), 'h2', 64),
}
# F(4x4): density of the non-zero activations / weights by input channels (module docstring of the GPU file: the chain
# needs about 27 bits plus log2 of the term count, so each output element can afford about one term)
_WG_DENSITY = {32: (0.06, 0.06), 64: (0.04, 0.04), 128: (0.04, 0.03)}
_WG_DENSITY_GUIDED = (0.02, 0.01)     # under input scales that differ by 2^2 within an image
_wg_conv_cache = {}


def wg_tiles(H, W, m):
    return -(-H // m) * -(-W // m)


def wg_conv_case(name):
    """A 3x3 / pad 1 convolution whose Winograd form is exact in f32 at EVERY stage - the weight transform, the input
    transform, the grouped GEMM and the output transform - and whose direct form is exact too.  Built once per name, never
    written.  -> dict: m, shapes, cin, cout, div, xs (f32 NHWC per tensor), wt [cout, cin, 3, 3] f32, in_scale [n div, cin]
    f32 or None, u [groups, cout, cin] float64 = G w G^T over the rationals (integers here), shift [cout] f32, and per
    tensor: refs = {(shifted?, relu?): float64 NHWC}, the stage tensors v, mo (float64) of the unshifted chain, and
    worst = {stage: the largest mag / unit} (the conditions below are asserted here, per element).

     F(2x2) 'dense'  x integers of [-7, 7] none zero, w = 4 k with k in [-7, 7]: U = (2 G) k (2 G)^T are integers.
     F(2x2) 'wide'   ceil(cin / 20) channels hold activations of 12 - 13 significant bits, 2048 p + q, against weights
                     whose only non-zero tap is the centre, 4 * +-1 (U = +-1 at the four inner positions); everywhere else
                     |x| <= 7 with half of them zero and w = 4 k.
     F(4x4) 'sparse' x in {-1, 0, 1} and w = 225 k, k in {-1, 0, 1}, non-zero with the densities of _WG_DENSITY: U = (15 G) k
                     (15 G)^T are integers, V multiples of 1/4, Mo multiples of 1/4, y multiples of 1/256.
     ``div`` > 1     every input image read by ``div`` output images under a per-(image, channel) input scale, a power of
                     two or exactly 0.  The scales span 2^-3 .. 2^3 over the images, but within one image at most 2^2 (image 0:
                     2^-3, 2^-2; image 1: 2^-1 .. 2^1; image 2: 2^2, 2^3; div = 3): an element that mixed a 2^3 term with the unit of a 2^-3 one would need six
                     bits more than F(4x4) leaves.  The unit of image i follows its smallest scale.

    THE CONDITIONS (mag = the stage's sum of absolute terms, unit = the power of two every term is a multiple of):
        input transform   mag / unit <= 2^24,  mag = |B^T| |x s| |B|
        grouped GEMM      mag / unit <= 2^22,  mag = sum_c |V| |U|              (LIMIT: two spare bits for the matrix pipe)
        output transform  mag / unit <= 2^24,  mag = |A^T| (sum_c |V| |U|) |A| + |shift|
        direct form       mag / unit <= 2^22,  mag = sum |x s| |w| + |shift|
    Where a shape does not meet them the density shrinks, never the condition."""
    if name in _wg_conv_cache:
        return _wg_conv_cache[name]
    import _wg_ref
    m, shapes, cin, cout, kind, div, counts, route, tile = WG_CONV[name]
    g = torch.Generator().manual_seed(7001 + sorted(WG_CONV).index(name))
    s, sg = wg_scaled_g(m)
    if kind == 'sparse':
        dx, dw = _WG_DENSITY[cin]
        if div > 1:
            dx, dw = _WG_DENSITY_GUIDED
        k = _ints(g, (cout, cin, 3, 3), 1) * (torch.rand(cout, cin, 3, 3, generator=g) < dw).double()
        k[0, 0, 1, 1] = 1.0
    else:
        k = _ints(g, (cout, cin, 3, 3), 7)
    ka = None
    if kind == 'wide':
        ka = torch.randperm(cin, generator=g)[:-(-cin // 20)]
        k[:, ka] = 0.0
        k[:, ka, 1, 1] = _ints(g, (cout, len(ka)), 1)
    wt = k * float(s * s)
    u = torch.einsum('ai,ocij,bj->aboc', sg, k, sg).reshape((m + 2) ** 2, cout, cin)
    unit_v, unit_y = (0.25, 1.0 / 256) if m == 4 else (1.0, 1.0)
    # integers of up to 17 bits in y's unit; under ``div`` the images' units differ by up to 2^6: multiples of the largest
    # (2^3 unit_y) that are at most 2^17 of the smallest (2^-3 unit_y)
    shift = _ints(g, (cout,), 2 ** 11) * 8.0 * unit_y if div > 1 else _ints(g, (cout,), 2 ** 17) * unit_y
    out = dict(m=m, shapes=shapes, cin=cin, cout=cout, div=div, counts=counts, route=route, tile=tile, wt=wt.float(), u=u,
               shift=shift.float(), xs=[], in_scale=[], refs=[], v=[], mo=[], worst=dict(v=0.0, mo=0.0, y=0.0, direct=0.0))
    assert torch.equal(out['wt'].double(), wt) and torch.equal(out['shift'].double(), shift)
    for n, H, W in shapes:
        if kind == 'sparse':
            x = _ints(g, (n, H, W, cin), 1) * (torch.rand(n, H, W, cin, generator=g) < dx).double()
            x[0, 0, 0, 0] = 1.0
        elif kind == 'dense':
            x = _ints(g, (n, H, W, cin), 7)
        else:
            x = _ints(g, (n, H, W, cin), 7, zeros=True)
            x[..., ka] = (2048.0 * torch.randint(1, 4, (n, H, W, len(ka)), generator=g).double() +
                          torch.randint(1, 2048, (n, H, W, len(ka)), generator=g).double()) * \
                (torch.randint(0, 2, (n, H, W, len(ka)), generator=g).double() * 2 - 1)
        vec, unit_x = None, torch.ones(n * div, dtype=torch.float64)
        if div > 1:
            assert div == 3
            img = torch.arange(n * div) % div
            lo = torch.tensor([-3.0, -1.0, 2.0], dtype=torch.float64)[img]          # image 0: 2^-3, 2^-2; 1: 2^-1 .. 2^1; 2: 2^2, 2^3
            e = lo[:, None] + torch.randint(0, 6, (n * div, cin), generator=g).double() % (2.0 + (img == 1).double())[:, None]
            vec = 2.0 ** e * (torch.rand(n * div, cin, generator=g) >= 0.1).double()
            unit_x = 2.0 ** lo
            assert (vec == 0).any() and vec.max().item() == 8.0 and vec[vec > 0].min().item() == 0.125
        n_img = n * div
        v, vmag = _wg_ref.input_transform(x, vec, div, m)
        mo = torch.einsum('gtc,goc->gto', v, u)
        momag = torch.einsum('gtc,goc->gto', v.abs(), u.abs())         # the GEMM's terms: products of its operands
        xe = x.repeat_interleave(div, 0) * (1.0 if vec is None else vec[:, None, None, :])
        xn = xe.permute(0, 3, 1, 2)
        dmag = F.conv2d(xn.abs(), wt.abs(), padding=1).permute(0, 2, 3, 1)
        tiles = wg_tiles(H, W, m)
        ut = unit_x.repeat_interleave(tiles)[None, :, None]                     # per tile row of V / Mo
        ui = unit_x[:, None, None, None]
        refs = {}
        for sh in (False, True):
            sv = shift if sh else None
            want = F.conv2d(xn, wt, sv, padding=1).permute(0, 2, 3, 1).contiguous()
            y, _ = _wg_ref.output_transform(mo, sv, False, n_img, H, W, m)
            _, ymag = _wg_ref.output_transform(momag, sv, False, n_img, H, W, m)
            assert torch.equal(y, want), name                                   # the float64 chain IS the convolution
            ud = ui * unit_y if sh else ui                                      # the direct form: integer weights, the shift's unit
            for t, unit, tag in ((v, ut * unit_v, 'v'), (mo, ut * unit_v, 'mo'), (y, ui * unit_y, 'y'), (want, ud, 'direct')):
                q = t / unit
                assert torch.equal(q, q.round()), (name, tag)                   # every value a multiple of its unit
            for mag, unit, lim, tag in ((vmag, ut * unit_v, WG_LIMIT, 'v'), (momag, ut * unit_v, LIMIT, 'mo'),
                                        (ymag, ui * unit_y, WG_LIMIT, 'y'),
                                        (dmag + (shift.abs() if sh else 0.0), ud, LIMIT, 'direct')):
                worst = (mag / unit).max().item()
                out['worst'][tag] = max(out['worst'][tag], worst)
                assert worst <= lim, f'{name} {tag}: mag / unit = 2^{torch.log2(torch.tensor(worst)).item():.2f}'
            assert torch.equal(want.float().double(), want)
            for relu in (False, True):
                refs[(sh, relu)] = torch.relu(want) if relu else want
        out['xs'].append(x.float().contiguous())
        out['in_scale'].append(None if vec is None else vec.float())
        out['refs'].append(refs)
        out['v'].append(v)
        out['mo'].append(mo)
    _wg_conv_cache[name] = out
    return out
