"""The five kernels of csrc/winograd.hip ALONE - the F(4x4) and F(2x2) input and output transforms and the weight pack -
called through the library's entry points as ``ops.conv3x3_winograd`` calls them, against the float64 closed forms of
tests/_wg_ref.py, bounded PER ELEMENT like the kernels of tests/test_hip_fwd_bound.py:

    |got - ref| <= c * 2^-24 * mag + 2^-126

``mag`` is the element's own term-magnitude sum (|B^T| |x s| |B|, |A^T| |Mo| |A| + |shift|), ``c`` the number of fp32
roundings along the longest chain of the kernel's arithmetic (each docstring derives it from the code; first-order counts
rounded up; ``fmaf`` is one rounding, and a contraction the compiler adds only removes roundings).  Nothing is divided by a
tensor's range and no GEMM sits between the transform and the check, so a transform that is wrong only where its result is
small - a border tile's padded taps, the dropped rows of a partial tile, one coefficient of a row that mostly cancels, one
channel lane of a vector - fails.  V / y / U are filled with a finite sentinel bit pattern before every launch and the rows
nobody owns (pad rows [tiles, t_pad) of every group, images past a device count, guard bands around y, rows
[cout, cout_pad) of U) are compared as int32.  Every test prints ``[wg-bound] name: worst |err| / bound`` before it
asserts (DESIGN.md section 7.4 carries the table).
"""
import time

import pytest
import torch

import _wg_ref as ref

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = 0x7B5A5A5A               # a finite fp32 (1.13e36): a row that should have been written fails its bound
GUARD = 4096                        # floats on either side of y (16-byte aligned; more than one pixel of any case)
ERR_SHAPE = -1                      # FGN_ERR_SHAPE (include/fgn_hip.h)

# (n, H, W, C): n_in for the input transforms, n_img for the output transforms
SHAPES = [
    (1, 1, 1, 4),                   # smallest legal shape
    (2, 5, 3, 8),                   # map smaller than a tile
    (3, 4, 4, 12),                  # exactly one F(4x4) tile; C / 2 odd
    (1, 6, 6, 4),                   # last tile half outside
    (1, 7, 9, 32),                  # odd sizes, no multiple of a tile
    (1, 13, 21, 36),
    (37, 7, 7, 64),                 # RoI pattern
]
COUNT_SHAPE = (6, 7, 9, 8)
COUNTS = [0, 1, 5, 6, 9]
PAIRS = [((2, 13, 10), (3, 7, 9)), ((1, 5, 3), (4, 4, 4)), ((3, 4, 4), (1, 9, 6))]


def _lib():
    from fgn_amd import lib
    return lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def _bounded(name, got, want, mag, c):
    """Assert |got - want| <= c * 2^-24 * mag + 2^-126 for every element; -> the worst ratio."""
    worst = ref.worst_ratio(got.detach().to(want.device), want, mag, c)
    print(f'[wg-bound] {name}: worst |err| / bound = {worst:.4f} (c = {c})')
    assert worst <= 1.0, (name, worst)
    return worst


def _t_pad(tiles_total):
    t_pad = _lib().fgn_winograd_t_pad(tiles_total)
    assert t_pad >= tiles_total and t_pad % 128 == 0
    return t_pad


def _run_input(m, x, s, cnt, n_img, div, V, t_pad):
    _, H, W, C = x.shape
    f = _lib().fgn_winograd4_input_f32 if m == 4 else _lib().fgn_winograd_input_f32
    return f(x.data_ptr(), _p(s), V.data_ptr(), _p(cnt), n_img, div, H, W, C, t_pad, _st())


def _run_output(m, Mo, y, shift, cnt, n_img, H, W, C, t_pad, relu):
    f = _lib().fgn_winograd4_output_f32 if m == 4 else _lib().fgn_winograd_output_f32
    return f(Mo.data_ptr(), y.data_ptr(), _p(shift), _p(cnt), n_img, H, W, C, t_pad, int(relu), _st())


def _small_variant(m, tiles_total, C):
    """The small cases run the 8-byte instances of F(4x4): a moved threshold fails here instead of unhooking the test."""
    if m == 4:
        assert _lib().fgn_winograd4_variant(tiles_total, C, 0) == 21
        assert _lib().fgn_winograd4_variant(tiles_total, C, 1) == 20


def _guarded_y(n, H, W, C):
    """-> (buffer, y): y [n, H, W, C] is a view in the middle of a larger sentinel buffer."""
    buf = _sentinel(GUARD + n * H * W * C + GUARD)
    return buf, buf[GUARD:GUARD + n * H * W * C].view(n, H, W, C)


def _guards_kept(buf):
    return _untouched(buf[:GUARD]) and _untouched(buf[-GUARD:])


def _draw_mo(R, t_pad, C, g, minus_zero_rows=None):
    """Mo drawn directly (no GEMM): signed, magnitudes spread per row and per channel over several decades."""
    Mo = ref.spread((R * R, t_pad, 1, C), g).reshape(R * R, t_pad, C)
    if minus_zero_rows is not None:
        Mo[:, minus_zero_rows[0]:minus_zero_rows[1]] = -0.0
    return Mo


# ------------------------------------------------------------------------------------------ A. input transforms
def _check_input(name, m, x, s, div, count=None):
    """One launch of the input transform into a sentinel V; rows of images below min(n_img, count) bounded, all other
    rows of every group untouched.  -> V on the host, reshaped [R, R, rows, C]."""
    n_in, H, W, C = x.shape
    R = m + 2
    ty, tx = ref.tiles_of(H, W, m)
    n_img = n_in * div
    tiles = n_img * ty * tx
    t_pad = _t_pad(tiles)
    _small_variant(m, tiles, C)
    V = _sentinel(R * R, t_pad, C)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
    xd, sd = x.cuda(), None if s is None else s.cuda()
    rc = _run_input(m, xd, sd, cnt, n_img, div, V, t_pad)
    assert rc == 0, rc
    torch.cuda.synchronize()
    V = V.cpu()
    live = (n_img if count is None else min(n_img, count)) * ty * tx
    want, mag = ref.input_transform(x, s, div, m)
    _bounded(name, V[:, :live], want[:, :live], mag[:, :live], ref.C_IN[m])
    assert _untouched(V[:, live:]), name
    return V.reshape(R, R, t_pad, C)


def _assert_constant_image_zeros(name, m, V, x, div):
    """The last image of x is constant per channel: in its interior tiles every position with a zero-sum row of B^T on
    either side is exactly 0."""
    n_in, H, W, C = x.shape
    ty, tx = ref.tiles_of(H, W, m)
    z = torch.tensor(ref.zero_sum_rows(m))
    zz = z[:, None] | z[None, :]
    inner = ref.interior_tiles(H, W, m)
    first = (n_in - 1) * div * ty * tx
    rows = V[:, :, first:first + div * ty * tx].reshape(m + 2, m + 2, div, ty, tx, C)
    picked = rows[zz][:, :, inner]
    print(f'[wg-bound] {name}: {picked.numel()} elements of the constant image must be exactly 0')
    assert bool((picked == 0).all()), name


@pytest.mark.parametrize('m', [4, 2])
@pytest.mark.parametrize('shape', SHAPES + ['guided'], ids=lambda s: s if isinstance(s, str) else 'x'.join(map(str, s)))
def test_input_transform_bound(shape, m):
    """wg4_input_kernel: d = x * s (1 rounding; s = 1 without in_scale), then ``wg4_bt`` down the columns and along the
    rows.  Its longest chains are r[0] and r[5]: a difference (1), the inner fmaf (1), the outer fmaf (1), the last
    addition (1) = 4 roundings, each of a partial sum that |B^T| |d| bounds; r[1], r[2] take 3, r[3], r[4] take 3.  The
    first pass' error (4 + 1) passes through |B^T| of the second, which adds its own 4: 9 in first order, c = 10.
    wg_input_kernel (F(2x2)): x * s (1) and one subtraction or addition per pass (1 + 1) = 3, c = 4.
    Signed inputs spread over five decades per pixel and per channel; every case runs twice, the second time with the last
    image constant per channel: its interior tiles must be exactly 0 at all positions but (1, 1).  ``guided``:
    (1, 13, 21, 32) with a_img_div = 3 and in_scale [3, 32] in [0.5, 1.5) - the AG-RPN form; its zeros need x * s
    rounded on its own (``vmul_rn``: contracted into the first difference of ``wg4_bt`` the product left
    x s - round(x s) there, inside the bound but not 0).  Pad rows [tiles, t_pad) of every group keep their bytes."""
    g = ref.gen(17 * m + (0 if isinstance(shape, str) else sum(shape)))
    if shape == 'guided':
        shape, div = (1, 13, 21, 32), 3
        s = (torch.rand(3, 32, generator=g) + 0.5).float()
    else:
        div, s = 1, None
    x = ref.spread(shape, g)
    tag = f'input F({m}x{m}) {shape} div={div}'
    _check_input(tag, m, x, s, div)
    xc = ref.with_constant_image(x, g)
    V = _check_input(tag + ' constant image', m, xc, s, div)
    _assert_constant_image_zeros(tag, m, V, xc, div)


@pytest.mark.parametrize('m', [4, 2])
def test_input_transform_device_count(m):
    """(6, 7, 9, 8) with a device-side image count of 0, 1, 5, 6 and 9: rows of images below min(n_img, count) are
    bounded, all later rows of every group keep their bytes."""
    g = ref.gen(40 + m)
    x = ref.spread(COUNT_SHAPE, g)
    for count in COUNTS:
        _check_input(f'input F({m}x{m}) {COUNT_SHAPE} count={count}', m, x, None, 1, count)


def _seg_tiles(s, m=4):
    ty, tx = ref.tiles_of(s[1], s[2], m)
    return s[0] * ty * tx


@pytest.mark.parametrize('C', [8, 36])
@pytest.mark.parametrize('s0,s1', PAIRS, ids=lambda s: 'x'.join(map(str, s)))
def test_input_transform_two_tensors(s0, s1, C):
    """fgn_winograd4_input2_f32: the second tensor's tiles follow the first's at tiles0 (same arithmetic, c = 10); both
    segments bounded - the tiles on either side of tiles0 included, they are rows of the same comparison -, pad rows
    untouched."""
    g = ref.gen(60 + C + sum(s0) + sum(s1))
    x0, x1 = ref.spread((*s0, C), g), ref.spread((*s1, C), g)
    tiles = _seg_tiles(s0) + _seg_tiles(s1)
    t_pad = _t_pad(tiles)
    _small_variant(4, tiles, C)
    V = _sentinel(36, t_pad, C)
    d0, d1 = x0.cuda(), x1.cuda()
    rc = _lib().fgn_winograd4_input2_f32(d0.data_ptr(), *s0, d1.data_ptr(), *s1, V.data_ptr(), C, t_pad, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    V = V.cpu()
    want, mag = ref.input_transform2(x0, x1, 4)
    assert want.shape[1] == tiles
    _bounded(f'input2 F(4x4) {s0} + {s1} C={C}', V[:, :tiles], want, mag, ref.C_IN[4])
    assert _untouched(V[:, tiles:])


def test_input_transform_refusals():
    """FGN_ERR_SHAPE, and V untouched: more tiles than t_pad, C % 4 != 0, a_img_div < 1 (both m); for the two-tensor entry
    point also an empty second tensor.  (That entry point has no in_scale, device count or a_img_div parameter: the
    launcher's refusal of those beside a second tensor cannot be reached through the library's interface.)"""
    L = _lib()
    x = torch.zeros(2, 7, 9, 8, device='cuda')
    V = _sentinel(36, 128, 8)
    for m in (4, 2):
        tiles = _seg_tiles((2, 7, 9), m)
        assert _run_input(m, x, None, None, 2, 1, V, tiles - 1) == ERR_SHAPE
        assert _run_input(m, x.view(2, 7, 12, 6), None, None, 2, 1, V, 128) == ERR_SHAPE
        assert _run_input(m, x, None, None, 2, 0, V, 128) == ERR_SHAPE
    two = lambda n0, n1, C, t_pad: L.fgn_winograd4_input2_f32(x.data_ptr(), n0, 7, 9, x.data_ptr(), n1, 7, 9, V.data_ptr(),
                                                               C, t_pad, _st())
    assert two(1, 1, 8, 11) == ERR_SHAPE                       # 6 + 6 tiles
    assert two(1, 1, 6, 128) == ERR_SHAPE
    assert two(1, 0, 8, 128) == ERR_SHAPE
    torch.cuda.synchronize()
    assert _untouched(V)


# ------------------------------------------------------------------------------------------ B. output transforms
def _check_output(name, m, Mo_host, Mo, shift, relu, n_img, H, W, C, t_pad, count=None):
    buf, y = _guarded_y(n_img, H, W, C)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device='cuda')
    shd = None if shift is None else shift.cuda()
    rc = _run_output(m, Mo, y, shd, cnt, n_img, H, W, C, t_pad, relu)
    assert rc == 0, rc
    torch.cuda.synchronize()
    live = n_img if count is None else min(n_img, count)
    want, mag = ref.output_transform(Mo_host, shift, relu, live, H, W, m)
    got = y.cpu()
    _bounded(name, got[:live], want, mag, ref.C_OUT[m])
    assert _untouched(got[live:]) and _guards_kept(buf), name
    if relu:
        assert bool((got[:live].contiguous().view(torch.int32) >= 0).all()), name      # neither negative nor -0


def _shift_of(C, g):
    shift = (torch.randn(C, generator=g) * torch.exp((torch.rand(C, generator=g) * 2 - 1) * 3.0)).float()
    shift[0] = -0.0
    return shift


@pytest.mark.parametrize('m', [4, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_output_transform_bound(shape, m):
    """wg4_output_kernel: ``wg4_at`` down the columns and along the rows, then + shift.  r[0] = (m0 + (m1 + m2)) +
    (m3 + m4): 4 additions; r[3]: the difference m1 - m2 (1), two fmaf (2), + m5 (1) = 4; r[1], r[2]: 3.  Two passes
    4 + 4, the shift's addition 1: 9 in first order, c = 10.  wg_output_kernel (F(2x2)): two additions per pass (2 + 2)
    and the shift (1) = 5, c = 6.  ReLU is 1-Lipschitz and exact.
    Mo is drawn directly; with n_img >= 2 the products of image 1 are all -0 and shift[0] is -0, so that a ReLU that lets
    -0 through shows.  Shift present and absent, ReLU on and off; y is a view in the middle of a larger sentinel buffer
    whose guard bands keep their bytes; outputs beyond H / W of a partial tile are dropped, which the guard band after y
    and the bound on the neighbouring pixel hold."""
    n_img, H, W, C = shape
    R = m + 2
    g = ref.gen(23 * m + sum(shape))
    ty, tx = ref.tiles_of(H, W, m)
    tiles = n_img * ty * tx
    t_pad = _t_pad(tiles)
    _small_variant(m, tiles, C)
    Mo_host = _draw_mo(R, t_pad, C, g, (ty * tx, 2 * ty * tx) if n_img >= 2 else None)
    Mo = Mo_host.cuda()
    shift = _shift_of(C, g)
    for sh in (None, shift):
        for relu in (False, True):
            _check_output(f'output F({m}x{m}) {shape} shift={sh is not None} relu={relu}', m, Mo_host, Mo, sh, relu,
                          n_img, H, W, C, t_pad)


@pytest.mark.parametrize('m', [4, 2])
def test_output_transform_device_count(m):
    """(6, 7, 9, 8) with a device-side image count of 0, 1, 5, 6 and 9: images below min(n_img, count) bounded, the later
    ones and the guard bands untouched."""
    n_img, H, W, C = COUNT_SHAPE
    g = ref.gen(80 + m)
    ty, tx = ref.tiles_of(H, W, m)
    t_pad = _t_pad(n_img * ty * tx)
    Mo_host = _draw_mo(m + 2, t_pad, C, g)
    Mo = Mo_host.cuda()
    shift = _shift_of(C, g)
    for count in COUNTS:
        _check_output(f'output F({m}x{m}) {COUNT_SHAPE} count={count}', m, Mo_host, Mo, shift, True, n_img, H, W, C,
                      t_pad, count)


@pytest.mark.parametrize('C', [8, 36])
@pytest.mark.parametrize('s0,s1', PAIRS, ids=lambda s: 'x'.join(map(str, s)))
def test_output_transform_two_tensors(s0, s1, C):
    """fgn_winograd4_output2_f32: tiles [0, tiles0) go to y0, [tiles0, ...) to y1 (c = 10); both bounded, with and without
    shift and ReLU, the guard bands of both buffers untouched."""
    g = ref.gen(90 + C + sum(s0) + sum(s1))
    tiles = _seg_tiles(s0) + _seg_tiles(s1)
    t_pad = _t_pad(tiles)
    _small_variant(4, tiles, C)
    Mo_host = _draw_mo(6, t_pad, C, g)
    Mo = Mo_host.cuda()
    shift = _shift_of(C, g)
    for sh, relu in ((None, False), (shift, True)):
        b0, y0 = _guarded_y(*s0, C)
        b1, y1 = _guarded_y(*s1, C)
        shd = None if sh is None else sh.cuda()
        rc = _lib().fgn_winograd4_output2_f32(Mo.data_ptr(), _p(shd), y0.data_ptr(), *s0, y1.data_ptr(), *s1, C, t_pad,
                                              int(relu), _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        (w0, m0), (w1, m1) = ref.output_transform2(Mo_host, sh, relu, s0, s1, 4)
        for k, (got, want, mag) in enumerate(((y0.cpu(), w0, m0), (y1.cpu(), w1, m1))):
            _bounded(f'output2 F(4x4) {s0} + {s1} C={C} relu={relu} tensor {k}', got, want, mag, ref.C_OUT[4])
            if relu:
                assert bool((got.contiguous().view(torch.int32) >= 0).all())
        assert _guards_kept(b0) and _guards_kept(b1)


def test_output_transform_refusals():
    """FGN_ERR_SHAPE, and y untouched: more tiles than t_pad, C % 4 != 0 (both m); for the two-tensor entry point also an
    empty second tensor.  (It has no device-count parameter.)"""
    L = _lib()
    Mo = torch.zeros(36, 128, 8, device='cuda')
    buf, y = _guarded_y(2, 7, 9, 8)
    for m in (4, 2):
        tiles = _seg_tiles((2, 7, 9), m)
        assert _run_output(m, Mo, y, None, None, 2, 7, 9, 8, tiles - 1, 1) == ERR_SHAPE
        assert _run_output(m, Mo, y, None, None, 2, 7, 12, 6, 128, 1) == ERR_SHAPE
    two = lambda n0, n1, C, t_pad: L.fgn_winograd4_output2_f32(Mo.data_ptr(), None, y.data_ptr(), n0, 7, 9, y.data_ptr(), n1,
                                                                7, 9, C, t_pad, 1, _st())
    assert two(1, 1, 8, 11) == ERR_SHAPE
    assert two(1, 1, 6, 128) == ERR_SHAPE
    assert two(1, 0, 8, 128) == ERR_SHAPE
    torch.cuda.synchronize()
    assert _untouched(buf)


# ------------------------------------------------------------------------------------------ C. every instance, second trip
BIG16 = (16, 64, 64, 1024)          # 4096 tiles x 1024 = 4 * 2^20 elements: the smallest size of the 16-byte instances
TRIP4 = (33, 64, 64, 1024)          # 8448 tiles x 256 vectors = 2 162 688 > the 8192 x 256 threads of the capped grid
TRIP2 = (33, 32, 32, 1024)          # the same for F(2x2) (float4 lanes)


def _instances():
    L = _lib()
    assert L.fgn_winograd4_variant(4096, 1024, 0) == 41 and L.fgn_winograd4_variant(4096, 1024, 1) == 40
    assert L.fgn_winograd4_variant(8448, 1024, 0) == 41 and L.fgn_winograd4_variant(8448, 1024, 1) == 40
    assert 8448 * 256 > 8192 * 256 > 4096 * 256


def _spread_on_device(shape, seed):
    n, H, W, C = shape
    g = torch.Generator(device='cuda').manual_seed(seed)
    px = torch.exp((torch.rand(n, H, W, 1, generator=g, device='cuda') * 2 - 1) * 6.0)
    ch = torch.exp((torch.rand(1, 1, 1, C, generator=g, device='cuda') * 2 - 1) * 6.0)
    return torch.randn(n, H, W, C, generator=g, device='cuda').mul_(px).mul_(ch)


def _worst_on_device(got, want, mag, c, worst):
    bound = mag.mul_(c * ref.U).add_(ref.TINY)
    return torch.maximum(worst, want.sub_(got).abs_().div_(bound).max())


def _big_input(shape, m, count=None):
    """Every element of V against the float64 closed form evaluated on the device, image by image (75 MB of fp64 per
    operand at a time); with ``count``, a second launch with a device count whose later rows must stay untouched."""
    n, H, W, C = shape
    R = m + 2
    ty, tx = ref.tiles_of(H, W, m)
    per = ty * tx
    t_pad = _t_pad(n * per)
    x = _spread_on_device(shape, 7 + m)
    runs = [(None, _sentinel(R * R, t_pad, C))]
    if count is not None:
        runs.append((torch.tensor([count], dtype=torch.int32, device='cuda'), _sentinel(R * R, t_pad, C)))
    for cnt, V in runs:
        assert _run_input(m, x, None, cnt, n, 1, V, t_pad) == 0
    worst = [torch.zeros((), dtype=F64, device='cuda') for _ in runs]
    for img in range(n):
        want, mag = ref.input_transform(x[img:img + 1], None, 1, m)
        for k, (cnt, V) in enumerate(runs):
            if cnt is None or img < count:
                worst[k] = _worst_on_device(V[:, img * per:(img + 1) * per].to(F64), want.clone(), mag.clone(), ref.C_IN[m],
                                            worst[k])
    for k, (cnt, V) in enumerate(runs):
        live = (n if cnt is None else count) * per
        assert _untouched(V[:, live:])
        w = float(worst[k])
        print(f'[wg-bound] input F({m}x{m}) {shape} count={None if cnt is None else count}: worst |err| / bound = {w:.4f} '
              f'(c = {ref.C_IN[m]}, all {R * R * live * C} elements)')
        assert w <= 1.0


def test_input_transform_every_instance_and_second_trip():
    """``wg4_input_kernel<4, true>`` at its smallest size, (16, 64, 64, 1024), and the second trip of the grid-stride loop
    of the F(4x4) and the F(2x2) kernel at (33, 64, 64, 1024) and (33, 32, 32, 1024): 2 162 688 threads of work on a
    grid of 2 097 152, once without a device count and once with count 32, whose boundary lies inside the second trip
    (rows of image 32 keep their bytes).  Every element is bounded (c = 10 / 4), none sampled: the closed forms run in
    float64 on the device, image by image.  The sizes are fixed by the threshold of ``wg4_vec`` and the grid cap."""
    t0 = time.perf_counter()
    _instances()
    _big_input(BIG16, 4)
    _big_input(TRIP4, 4, 32)
    _big_input(TRIP2, 2, 32)
    torch.cuda.synchronize()
    print(f'[wg-bound] input transforms, 16-byte instance and second trip: {time.perf_counter() - t0:.1f} s wall')


def _big_output(shape, m, count=None):
    n, H, W, C = shape
    R = m + 2
    ty, tx = ref.tiles_of(H, W, m)
    per = ty * tx
    t_pad = _t_pad(n * per)
    Mo = _spread_on_device((R * R, t_pad, 1, C), 11 + m).reshape(R * R, t_pad, C)
    g = torch.Generator(device='cuda').manual_seed(5)
    shift = torch.randn(C, generator=g, device='cuda')
    runs = [(None, *_guarded_y(n, H, W, C))]
    if count is not None:
        runs.append((torch.tensor([count], dtype=torch.int32, device='cuda'), *_guarded_y(n, H, W, C)))
    for cnt, buf, y in runs:
        assert _run_output(m, Mo, y, shift, cnt, n, H, W, C, t_pad, True) == 0
    worst = [torch.zeros((), dtype=F64, device='cuda') for _ in runs]
    for img in range(n):
        want, mag = ref.output_transform(Mo[:, img * per:(img + 1) * per], shift, True, 1, H, W, m)
        for k, (cnt, buf, y) in enumerate(runs):
            if cnt is None or img < count:
                worst[k] = _worst_on_device(y[img:img + 1].to(F64), want.clone(), mag.clone(), ref.C_OUT[m], worst[k])
    for k, (cnt, buf, y) in enumerate(runs):
        live = n if cnt is None else count
        assert _untouched(y[live:]) and _guards_kept(buf)
        assert bool((y[:live].view(torch.int32) >= 0).all())
        w = float(worst[k])
        print(f'[wg-bound] output F({m}x{m}) {shape} count={None if cnt is None else count}: worst |err| / bound = {w:.4f} '
              f'(c = {ref.C_OUT[m]}, all {live * H * W * C} elements)')
        assert w <= 1.0


def test_output_transform_every_instance_and_second_trip():
    """``wg4_output_kernel<4>`` at (16, 64, 64, 1024) and the second grid-stride trip of both output kernels at
    (33, 64, 64, 1024) and (33, 32, 32, 1024), without a device count and with count 32 (image 32 and the guard bands
    keep their bytes); shift and ReLU on.  Every element bounded (c = 10 / 6) against the closed form in float64 on the
    device, image by image."""
    t0 = time.perf_counter()
    _instances()
    _big_output(BIG16, 4)
    _big_output(TRIP4, 4, 32)
    _big_output(TRIP2, 2, 32)
    torch.cuda.synchronize()
    print(f'[wg-bound] output transforms, 16-byte instance and second trip: {time.perf_counter() - t0:.1f} s wall')


# ------------------------------------------------------------------------------------------ D. weight pack
@pytest.mark.parametrize('m', [4, 2])
@pytest.mark.parametrize('cout,cin,cout_pad', [(4, 32, 128), (96, 64, 128), (132, 32, 256), (1, 1, 128)])
def test_pack_weights_bound(cout, cin, cout_pad, m):
    """wg_pack_weights_kernel: t[a][j] = g0 k0 + g1 k1 + g2 k2 in fp64 - three products and two additions, 5 roundings
    without contraction -, then the same form over j on the t's: 5 more, and the 5 of the first pass carried through
    |G|: at most 10 roundings of fp64 behind an element, 16 allowed; then ONE rounding to fp32:
        |got - ref| <= 2^-24 |ref| + 16 * 2^-53 mag + 2^-126.
    G is the host's fp64 table, handed to the kernel and to the reference alike.  Weights of mixed magnitude; rows
    [cout, cout_pad) of every group keep their sentinel bytes."""
    from fgn_amd import ops
    R = m + 2
    g = ref.gen(7 * m + cout + cin)
    w = ref.spread((cout, cin, 3, 3), g, 1.5)
    G64 = ops._WG_G[m]
    Gd = G64.cuda().contiguous()
    Ud = _sentinel(R * R, cout_pad, cin)
    wd = w.cuda()
    rc = _lib().fgn_winograd_pack_weights_f32(wd.data_ptr(), Gd.data_ptr(), Ud.data_ptr(), cout, cin, cout_pad, m, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = Ud.cpu()
    want, mag = ref.pack_weights(w, G64, m)
    worst = ref.pack_ratio(got[:, :cout], want, mag)
    print(f'[wg-bound] pack F({m}x{m}) ({cout}, {cin}) cout_pad={cout_pad}: worst |err| / bound = {worst:.4f}')
    assert worst <= 1.0
    assert _untouched(got[:, cout:])


def test_pack_weights_refusals():
    from fgn_amd import ops
    w = torch.zeros(8, 32, 3, 3, device='cuda')
    U = _sentinel(36, 128, 32)
    G = ops._WG_G[4].cuda().contiguous()
    f = _lib().fgn_winograd_pack_weights_f32
    assert f(w.data_ptr(), G.data_ptr(), U.data_ptr(), 8, 32, 128, 3, _st()) == ERR_SHAPE
    assert f(w.data_ptr(), G.data_ptr(), U.data_ptr(), 8, 32, 7, 4, _st()) == ERR_SHAPE
    torch.cuda.synchronize()
    assert _untouched(U)
