"""An independent model of the mask tail (csrc/mask.hip): the paste sample restated in numpy float32 operation by
operation, the same formula in float64, a derived bound on their difference, the launch routes of the five kernels that
share the sample (mask_paste / mask_rle / mask_rle_src / mask_overlap / mask_overlap_src) and of the dense RLE walk, and
the builders of every case tests/test_hip_mask_exact.py runs.  numpy only; nothing of fgn_amd is imported.

mask.hip is compiled with -ffp-contract=off and a correctly rounded f32 division, so every sample of the kernels is one
sequence of IEEE float32 operations - the sequence written out in ``_axis`` / ``_sample`` below with dtype float32.
tests/test_mask_ref_cpu.py holds this model to the float64 form and to the oracle's grid_sample paste."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'fgn_amd', 'csrc')

# the constants the route models below use; test_mask_ref_cpu.py compares them with source_constants()
RLE_THREADS = 1024
OVL_ROWS = 32
OVL_THREADS = 256
BITS_ROWS = 8
DENSE_SEGS = 32
DENSE_THREADS = 256
SRC_MAX_DIM = 16384
PASTE_THREADS = 256
PASTE_GRID_CAP = 256 * 32
LDS_MASK = 32               # the kernels stage the mask in 32 x 32 floats of LDS: mask sizes 1..32
U = 2.0 ** -24              # unit roundoff of float32


def source_constants() -> dict:
    """The same constants as mask.hip states them: its ``constexpr int`` lines, the grid cap of fgn_mask_paste_u8, the
    LDS mask arrays and the mask-size tests of the entry points."""
    text = open(os.path.join(CSRC, 'mask.hip')).read()

    def cx(name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))
    grid = re.search(r'std::min<long long>\(\(total4 \+ 255\) / 256, (\d+) \* (\d+)\);', text)
    launch = re.search(r'hipLaunchKernelGGL\(mask_paste_kernel, dim3\(grid\), dim3\((\d+)\)', text)
    lds = re.findall(r'__shared__ float m\[(\d+) \* (\d+)\];', text)
    sizes = re.findall(r'mask_size > (\d+) \|\| mask_size < 1', text)
    return {'RLE_THREADS': cx('RLE_THREADS'), 'OVL_ROWS': cx('OVL_ROWS'), 'OVL_THREADS': cx('OVL_THREADS'),
            'BITS_ROWS': cx('BITS_ROWS'), 'DENSE_SEGS': cx('DENSE_SEGS'), 'DENSE_THREADS': cx('DENSE_THREADS'),
            'SRC_MAX_DIM': cx('SRC_MAX_DIM'), 'PASTE_THREADS': int(launch.group(1)),
            'PASTE_GRID_CAP': int(grid.group(1)) * int(grid.group(2)),
            'LDS_MASK': sorted({int(v) for pair in lds for v in pair}), 'n_lds': len(lds),
            'MASK_SIZE_MAX': sorted({int(v) for v in sizes}), 'n_size_tests': len(sizes)}


# ---------------------------------------------------------------------------------------------- the sample
def _axis(pix: np.ndarray, b0, b1, MS: int, T):
    """paste_axis for an array of pixel indices in arithmetic T: (low tap index, weight of the high tap, coordinate)."""
    with np.errstate(all='ignore'):
        g = (pix.astype(T) + T(0.5) - b0) / (b1 - b0) * T(2) - T(1)
        g = np.where(np.isinf(g), T(0), g)                       # grid coordinate inf -> 0 (mmdet); 0 / 0 stays NaN
        c = ((g + T(1)) * T(MS) - T(1)) / T(2)
        f = np.floor(c)
        lo = np.fmin(np.fmax(f, T(-2)), T(MS)).astype(np.int64)  # fmaxf(NaN, -2) = -2: np.fmax ignores a NaN as fmaxf does
        w = c - f
    return lo, w, c


def _sample(prob: np.ndarray, box, ys: np.ndarray, xs: np.ndarray, T) -> np.ndarray:
    """paste_value on the pixel rows ``ys`` x columns ``xs`` in arithmetic T: paste_row_lerp of the two mask rows
    (zero taps outside the mask, a row outside the mask is 0 whatever its weights), then the vertical lerp."""
    m = np.asarray(prob, F32).astype(T)
    MS = m.shape[0]
    b = [T(F32(v)) for v in box[:4]]
    lox, wx, _ = _axis(xs, b[0], b[2], MS, T)
    loy, wy, _ = _axis(ys, b[1], b[3], MS, T)

    def tap(rows, cols):
        ok = ((rows >= 0) & (rows < MS))[:, None] & ((cols >= 0) & (cols < MS))[None, :]
        return np.where(ok, m[np.clip(rows, 0, MS - 1)[:, None], np.clip(cols, 0, MS - 1)[None, :]], T(0))

    def row_lerp(rows):
        with np.errstate(all='ignore'):
            r = tap(rows, lox) * (T(1) - wx)[None, :] + tap(rows, lox + 1) * wx[None, :]
        return np.where(((rows >= 0) & (rows < MS))[:, None], r, T(0))
    with np.errstate(all='ignore'):
        return row_lerp(loy) * (T(1) - wy)[:, None] + row_lerp(loy + 1) * wy[:, None]


def paste_region(box, H: int, W: int, MS: int, thr, skip_empty: bool):
    """make_paste_box: the integer region [x0, x1) x [y0, y1) (possibly empty) a kernel visits."""
    bx0, by0, bx1, by1 = [F32(v) for v in box[:4]]
    fl = lambda v: int(np.floor(v))
    ce = lambda v: int(np.ceil(v))
    if skip_empty:
        return max(fl(bx0) - 1, 0), max(fl(by0) - 1, 0), min(ce(bx1) + 1, W), min(ce(by1) + 1, H)
    bw, bh = bx1 - bx0, by1 - by0
    mx, my = bw / (F32(2) * F32(MS)), bh / (F32(2) * F32(MS))
    every = not (F32(thr) > F32(0))
    fx, fy = every or not (bw > F32(0)), every or not (bh > F32(0))
    return (0 if fx else max(fl(bx0 - mx) - 1, 0), 0 if fy else max(fl(by0 - my) - 1, 0),
            W if fx else min(ce(bx1 + mx) + 1, W), H if fy else min(ce(by1 + my) + 1, H))


def paste_model(prob, box, H: int, W: int, thr, skip_empty: bool, whole_image: bool = False):
    """(mask bool [H,W], sample f32 [H,W], region): the pixels a kernel sets.  The sample is NaN where the kernel
    evaluates nothing (outside the region).  ``whole_image``: the skip_empty=False semantic evaluated on every pixel of
    the image, without the band."""
    MS = np.asarray(prob).shape[0]
    x0, y0, x1, y1 = (0, 0, W, H) if whole_image else paste_region(box, H, W, MS, thr, skip_empty)
    mask = np.zeros((H, W), bool)
    sample = np.full((H, W), np.nan, F32)
    if x0 < x1 and y0 < y1:
        s = _sample(prob, box, np.arange(y0, y1), np.arange(x0, x1), F32)
        assert s.dtype == F32
        sample[y0:y1, x0:x1] = s
        with np.errstate(invalid='ignore'):
            mask[y0:y1, x0:x1] = s >= F32(thr)
    return mask, sample, (x0, y0, x1, y1)


def sample64(prob, box, H: int, W: int) -> np.ndarray:
    """The same formula in float64 from the same float32 inputs, on every pixel of the image."""
    return _sample(prob, box, np.arange(H), np.arange(W), F64)


def paste_bound(prob, box, H: int, W: int) -> np.ndarray:
    """A bound on |s32 - s64| per pixel, for boxes of positive width and height, counted from the roundings of the code
    (u = 2^-24, first order; the closing factor 1 + 2^-10 covers the products of two errors and the float64 evaluation).

    Coordinate chain of paste_axis.  a = pix + 0.5 is exact.  t = fl(a - b0), d = fl(b1 - b0), q = fl(t / d): three
    roundings, relative error 3u.  2q is exact.  g = fl(2q - 1): error 3u|2q| + u|g|.  h = fl(g + 1): + u|h|, and
    h = 2q, so err(h) <= 4u|h| + u|g|.  p = fl(h * MS): MS err(h) + u|p| = 5u|p| + u MS|g|.  fl(p - 1): + u|p - 1|; the
    division by 2 is exact.  With p = 2c + 1, MS g = p - MS and p - 1 = 2c:
        err(c) <= u/2 (5 |2c + 1| + |2c + 1 - MS| + 2 |c|).
    The weight w = fl(c - floor(c)) is exact for c >= 0 and rounds once (<= u) for c in (-1, 0): err(w) <= err(c) + u.
    Where the two chains floor to different integers the taps differ, but the bilinear interpolant is continuous and
    piecewise linear in c, so the sample moves by at most (local slope) x err: the slope along x is the largest
    |m[r][j + 1] - m[r][j]| of the zero-padded mask over the cell of the pixel and its neighbours (columns lo - 1 .. lo + 1,
    rows lo_y - 1 .. lo_y + 2), likewise along y.
    The two lerps.  paste_row_lerp: fl(1 - w) <= u, the two products and the sum one rounding each: <= 4u M with M the
    largest mask value.  The vertical lerp carries the rows' 4u M through weights that sum to 1 and adds its own 4u M.
        bound = [Lx (err(cx) + u) + Ly (err(cy) + u) + 8u M] (1 + 2^-10)."""
    m = np.asarray(prob, F32).astype(F64)
    MS = m.shape[0]
    b = [F64(F32(v)) for v in box[:4]]
    lox, _, cx = _axis(np.arange(W), b[0], b[2], MS, F64)
    loy, _, cy = _axis(np.arange(H), b[1], b[3], MS, F64)
    pad = 5
    P = np.pad(m, pad)
    dx = np.abs(np.diff(P, axis=1))          # dx[r, j] = |P[r, j + 1] - P[r, j]|
    dy = np.abs(np.diff(P, axis=0))

    def dilate(a, rows, cols):
        out = np.zeros_like(a)
        for dr in rows:
            for dc in cols:
                out = np.maximum(out, np.roll(np.roll(a, -dr, 0), -dc, 1))   # out[r, j] covers a[r + dr, j + dc]
        return out
    DX = dilate(dx, (-1, 0, 1, 2), (-1, 0, 1))
    DY = dilate(dy, (-1, 0, 1), (-1, 0, 1, 2))
    iy = np.clip(loy, -3, MS + 2) + pad
    ix = np.clip(lox, -3, MS + 2) + pad
    Lx = DX[iy[:, None], ix[None, :]]
    Ly = DY[iy[:, None], ix[None, :]]
    err = lambda c: U / 2 * (5 * np.abs(2 * c + 1) + np.abs(2 * c + 1 - MS) + 2 * np.abs(c)) + U
    return (Lx * err(cx)[None, :] + Ly * err(cy)[:, None] + 8 * U * np.abs(m).max()) * (1 + 2.0 ** -10)


def box_to_source_model(box, src_hw, net_hw) -> np.ndarray:
    """box_to_source: each coordinate divided by float32(W / w) resp. float32(H / h) - the double quotient rounded once -
    in one correctly rounded float32 division.  A size outside 1..16384 yields zeros (nothing is computed)."""
    (h, w), (H, W) = src_hw, net_hw
    if not (1 <= h <= SRC_MAX_DIM and 1 <= w <= SRC_MAX_DIM):
        return np.zeros(4, F32)
    sx, sy = F32(W / w), F32(H / h)
    b = [F32(v) for v in box[:4]]
    return np.array([b[0] / sx, b[1] / sy, b[2] / sx, b[3] / sy], F32)


def overlap_model(det_masks, gt_masks):
    """(inter [D,G], det_area [D], gt_area [G]) as exact pixel counts."""
    d = np.asarray(det_masks, bool)
    g = np.asarray(gt_masks, bool)
    inter = np.array([[np.count_nonzero(a & b) for b in g] for a in d], np.int32).reshape(len(d), len(g))
    return inter, np.array([np.count_nonzero(a) for a in d], np.int32), np.array([np.count_nonzero(b) for b in g], np.int32)


def transitions(mask: np.ndarray) -> int:
    """Value changes of the column-major pixel sequence (a set first pixel counts: the sequence starts from 0)."""
    flat = np.asarray(mask, bool).reshape(-1, order='F')
    return int(np.count_nonzero(flat[1:] != flat[:-1])) + int(flat[0]) if flat.size else 0


def run_lengths(mask: np.ndarray) -> list:
    """The runs of the column-major sequence, the first one of zeros (possibly of length 0)."""
    flat = np.asarray(mask, np.int8).reshape(-1, order='F')
    cut = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    runs = np.diff(np.concatenate([[0], cut, [flat.size]])).tolist()
    return ([0] + runs) if flat[0] else runs


# ---------------------------------------------------------------------------------------------- launch routes
def paste_route(D: int, H: int, W: int) -> dict:
    """fgn_mask_paste_u8: four-pixel groups, workgroups, grid-stride passes, groups that hold pixels of two detections,
    and whether the byte tail store runs."""
    hw = H * W
    total4 = (D * hw + 3) // 4
    grid = min((total4 + PASTE_THREADS - 1) // PASTE_THREADS, PASTE_GRID_CAP)
    return {'total4': total4, 'grid': grid, 'passes': -(-total4 // (grid * PASTE_THREADS)),
            'straddle': sum(1 for d in range(1, D) if (d * hw) % 4), 'tail': (D * hw) % 4 != 0}


def rle_route(mask: np.ndarray, region, H: int, W: int) -> dict:
    """rle_detection on a detection whose model mask and region are given: columns scanned and columns per thread,
    transitions, runs per thread of the string emitter, and which edge rules decide."""
    x0, y0, x1, y1 = region
    xe = min(x1, W - 1)
    ncols = max(xe - x0 + 1, 0)
    T = transitions(mask)
    runs = run_lengths(mask)
    return {'ncols': ncols, 'cpt': -(-ncols // RLE_THREADS), 'T': T, 'n_runs': T + 1,
            'rpt': -(-(T + 1) // RLE_THREADS), 'bottom': y1 >= H,
            'wrap_merge': bool(W > 1 and (mask[H - 1, :-1] & mask[0, 1:]).any()),
            'last_col': x1 == W and x0 < x1 and bool(mask[:, W - 1].any()),
            'close_col': x0 < x1 <= W - 1 and bool(mask[H - 1, x1 - 1]),
            'first_run': runs[0], 'runs': runs}


def overlap_route(region, G: int) -> dict:
    x0, y0, x1, y1 = region
    empty = not (x0 < x1 and y0 < y1)
    return {'empty': empty, 'blocks': [] if empty else list(range(y0 // OVL_ROWS, (y1 - 1) // OVL_ROWS + 1)),
            'words': [] if empty else list(range(x0 >> 6, ((x1 - 1) >> 6) + 1)), 'passes': -(-G // 64)}


def dense_route(H: int, W: int) -> dict:
    """dense_rle_walk_kernel: chunks per column, chunks per segment and wave, segments that hold chunks, steps of 64
    chunks a wave makes, and the branch of the (column, chunk) advance."""
    hp = (H + 15) // 16 * 16
    cpc = hp // 16
    n_chunks = W * cpc
    nw = DENSE_THREADS // 64
    per_seg = -(-(-(-n_chunks // DENSE_SEGS)) // (64 * nw)) * (64 * nw)
    per_wave = per_seg // nw
    dx = 64 // cpc
    return {'cpc': cpc, 'n_chunks': n_chunks, 'per_seg': per_seg, 'segs': -(-n_chunks // per_seg),
            'steps': -(-min(per_wave, n_chunks) // 64),      # of the fullest wave; the advance matters from 2 on
            'dx': dx, 'dk': 64 - dx * cpc, 'branch': 'dx0' if cpc > 64 else 'dx'}


# ---------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    prob: np.ndarray            # [D, MS, MS] float32
    boxes: np.ndarray           # [D, 5] float32 (x0, y0, x1, y1, score)
    H: int
    W: int
    thrs: tuple
    claims: dict = field(default_factory=dict)   # per detection index or 'all': the route the case is built for

    @property
    def MS(self):
        return self.prob.shape[1]

    @property
    def D(self):
        return self.prob.shape[0]


def _case(name, probs, boxes, H, W, thrs, **claims) -> Case:
    b = np.zeros((len(boxes), 5), F32)
    b[:, :4] = np.asarray(boxes, F32)
    b[:, 4] = 1
    return Case(name, np.ascontiguousarray(np.stack(probs), F32), b, H, W, tuple(thrs), claims)


def generic_cases() -> dict:
    """Random boxes and probabilities; mask sizes 14 and 28; thresholds 0.5, 0.3, 0.1."""
    out = {}
    # (seeds: the first for which no sample of the image lies within paste_bound of a threshold; test_mask_ref_cpu.py
    # asserts it)
    for name, H, W, MS, seed in (('97x131-m14', 97, 131, 14, 1), ('64x64-m28', 64, 64, 28, 1),
                                 ('37x50-m14', 37, 50, 14, 2), ('300x400-m28', 300, 400, 28, 1),
                                 ('300x400-m14', 300, 400, 14, 1)):
        rs = np.random.RandomState(seed)
        D = 6
        prob = rs.rand(D, MS, MS).astype(F32)
        x0 = rs.rand(D) * W * 0.8
        y0 = rs.rand(D) * H * 0.8
        bw = rs.rand(D) * min(W, 120) * 0.5 + 2
        bh = rs.rand(D) * min(H, 120) * 0.5 + 2
        boxes = np.stack([x0, y0, np.minimum(x0 + bw, W), np.minimum(y0 + bh, H)], 1)
        out[name] = _case(name, list(prob), boxes, H, W, (0.5, 0.3, 0.1))
    return out


def _quarter(rs, MS):
    return (rs.randint(0, 5, (MS, MS)) / 4).astype(F32)


def exact_cases() -> dict:
    """Mask sizes 16 and 32, dyadic boxes (half-pixel offset at unit scale, double scale, half-pixel offset partly
    outside), binary and quarter-valued probabilities: every float32 operation of the sample is exact."""
    out = {}
    for MS in (16, 32):
        rs = np.random.RandomState(100 + MS)
        n = 2 * MS + 8
        probs = [(rs.rand(MS, MS) > 0.5).astype(F32), _quarter(rs, MS), np.ones((MS, MS), F32),
                 (rs.rand(MS, MS) > 0.5).astype(F32), _quarter(rs, MS), (rs.rand(MS, MS) > 0.5).astype(F32)]
        boxes = [[3.5, 2.5, 3.5 + MS, 2.5 + MS], [3.5, 2.5, 3.5 + MS, 2.5 + MS], [4, 2, 4 + 2 * MS, 2 + 2 * MS],
                 [4, 2, 4 + 2 * MS, 2 + 2 * MS], [-5.5, -3.5, -5.5 + MS, -3.5 + MS], [-5.5, -3.5, -5.5 + MS, -3.5 + MS]]
        out[f'exact-m{MS}'] = _case(f'exact-m{MS}', probs, boxes, n, n + 3, (0.25, 0.5, 0.75))
    return out


def rounded_cases() -> dict:
    """Mask sizes 14 and 28, binary masks, half-pixel offset boxes at unit and double scale: 1 / 14 is not a float, the
    coordinate is rounded and the samples that are exactly 0.5 in real arithmetic come out a few floats to either side."""
    out = {}
    for MS in (14, 28):
        rs = np.random.RandomState(200 + MS)
        n = 2 * MS + 8
        probs = [(rs.rand(MS, MS) > 0.5).astype(F32) for _ in range(4)]
        boxes = [[3.5, 2.5, 3.5 + MS, 2.5 + MS], [3.5, 2.5, 3.5 + 2 * MS, 2.5 + 2 * MS],
                 [-5.5, -3.5, -5.5 + MS, -3.5 + MS], [6.5, 4.5, 6.5 + 2 * MS, 4.5 + 2 * MS]]
        out[f'rounded-m{MS}'] = _case(f'rounded-m{MS}', probs, boxes, n, n + 3, (0.5,))
    return out


GEOMETRY_BOXES = {
    'inside': [5.3, 4.2, 30.7, 25.9],
    'out-left-top': [-6.5, -4.25, 12.3, 9.1],
    'out-right-bottom': [40.2, 30.5, 60.0, 47.7],
    'beyond-left': [-30, 5, -10, 20],
    'beyond-right': [60, 5, 80, 20],
    'beyond-top': [5, -30, 20, -8],
    'beyond-bottom': [5, 50, 20, 70],
    'sub-pixel': [10.2, 10.3, 10.201, 10.301],
    'zero-width': [10.25, 5, 10.25, 30],
    'zero-height': [5, 12.75, 30, 12.75],
    'zero-both': [7.25, 8.75, 7.25, 8.75],
    'zero-width-on-centre': [10.5, 5, 10.5, 30],       # pixel 10: 0 / 0 = NaN
    'zero-both-on-centre': [10.5, 12.5, 10.5, 12.5],
    'inverted': [30, 25, 5, 4],
    'inverted-x': [30, 4, 5, 25],
    'very-wide': [-1000, -800, 1200, 900],
    'full-image': [0, 0, 52, 40],
}
GEOMETRY_NAMES = list(GEOMETRY_BOXES)


def geometry_cases() -> dict:
    """Every box of GEOMETRY_BOXES in a 40 x 52 image at mask sizes 1, 2, 14, 28 and 32; thresholds 0.5, 0.3, 0 and a
    negative one (the whole image under skip_empty=False), one above 1 (nothing set)."""
    out = {}
    for MS in (1, 2, 14, 28, 32):
        rs = np.random.RandomState(300 + MS)
        probs = [rs.rand(MS, MS).astype(F32) * F32(0.8) + F32(0.2) for _ in GEOMETRY_NAMES]
        probs[0] = np.ones((MS, MS), F32)
        out[f'geometry-m{MS}'] = _case(f'geometry-m{MS}', probs, [GEOMETRY_BOXES[k] for k in GEOMETRY_NAMES], 40, 52,
                                       (0.5, 0.3, 0.0, -0.5, 1.5))
    return out


def layout_cases() -> dict:
    """Image sizes that are no multiple of 4 pixels: a lane of mask_paste_kernel packs pixels of two detections with
    different boxes, and the last group is stored byte by byte."""
    out = {}
    for H, W in ((5, 7), (1, 1), (3, 1)):
        rs = np.random.RandomState(400 + H * 8 + W)
        D = 5
        probs = [rs.rand(14, 14).astype(F32) * F32(0.5) + F32(0.5) for _ in range(D)]
        boxes = [[-1, -1, W + 1, H + 1], [0, 0, W, H], [0.25, 0.25, W * 0.75, H * 0.75], [-3, -2, W * 0.5, H * 0.5],
                 [W * 0.5, H * 0.5, W + 2, H + 3]]
        out[f'layout-{H}x{W}'] = _case(f'layout-{H}x{W}', probs, boxes, H, W, (0.5, 0.3))
    return out


def large_paste_case() -> Case:
    """3 detections at 1700 x 1700: 2 167 500 four-pixel groups, more than the 256 * 32 * 256 one pass covers; the third
    detection's box lies in the rows only the second pass of the grid-stride loop reaches."""
    rs = np.random.RandomState(500)
    probs = [rs.rand(14, 14).astype(F32) for _ in range(3)]
    return _case('large-1700', probs, [[10.5, 20.25, 300, 170], [800, 700.5, 1100.75, 1000], [100, 1550, 400.5, 1695.25]],
                 1700, 1700, (0.5,), second_pass_from_row=(PASTE_GRID_CAP * PASTE_THREADS * 4 - 2 * 1700 * 1700) // 1700 + 1)


def mask32_from_runs(runs) -> np.ndarray:
    """A 32 x 32 binary mask whose column-major sequence has the given runs (zeros first), zero-filled behind them."""
    flat = np.zeros(32 * 32, F32)
    p, v = 0, 0
    for r in runs:
        flat[p:p + r] = v
        p += r
        v ^= 1
    assert p <= flat.size
    return flat.reshape(32, 32, order='F')


def unit_box(x0: int, y0: int, MS: int = 32):
    """At mask size 32 (16) and this box pixel (x, y) samples mask element (y - y0, x - x0) exactly, weight 0."""
    return [x0, y0, x0 + MS, y0 + MS]


def rle_route_cases() -> dict:
    """One case per route of rle_detection / emit_coco_string.  ``claims``: what rle_route must report."""
    out = {}
    one = np.ones((32, 32), F32)
    rs = np.random.RandomState(600)
    # region wider than 1024 columns at H = 3: two columns per thread
    out['cpt2'] = _case('cpt2', [rs.rand(14, 14).astype(F32)], [[20.5, 0.25, 1120.25, 2.75]], 3, 1200, (0.5, 0.3), cpt=2)
    # 32 x 32 rows alternating at unit scale in 34 x 34: 1024 transitions, 1025 runs: two runs per thread
    alt = np.zeros((32, 32), F32)
    alt[0::2] = 1
    out['rpt2'] = _case('rpt2', [alt], [unit_box(1, 1)], 34, 34, (0.5,), rpt=2, T=1024)
    # the box covers the whole height (the region touches the bottom edge): columns 0, 2, .. full, columns 1, 3, .. set in
    # their upper rows, so a run of ones merges through every column wrap; beside it a region that touches the bottom edge
    # and starts mid-image
    wrap = np.zeros((32, 32), F32)
    wrap[:, 0::2] = 1
    wrap[:12, 1::2] = 1
    out['bottom-wrap'] = _case('bottom-wrap', [wrap, one], [unit_box(1, 0), [3.25, 20.5, 9.5, 32]], 32, 34, (0.5,),
                               bottom=True, wrap_merge=True)
    # mask size 8 at scale 4, all ones, thr 0.25: the region's last column (x = 37, the first one behind the box) samples
    # exactly 0.375 and is set down to the bottom row.  W = 38: it is the image's last column; W = 39: one column short of
    # it, the closing column is read
    m8 = np.ones((8, 8), F32)
    out['last-col'] = _case('last-col', [m8], [[5, 12, 37, 44]], 40, 38, (0.25,), last_col=True, bottom=True)
    out['close-col'] = _case('close-col', [m8], [[5, 12, 37, 44]], 40, 39, (0.25,), close_col=True, bottom=True)
    # string edges.  32 x 34 image, box at x0 = 1 (or 0): the mask's column-major sequence is the image's, behind 32 zeros
    # (every list ends with a run of ones, so no claimed run is lengthened by the zeros behind the mask)
    seqs = {'deltas': [5, 40, 40, 23, 24, 22, 24, 37, 40, 68, 72, 1],       # deltas -17 -16 -1 0 15 16 31 32
            'len-1024': [0, 1024], 'len-1023': [1, 1023], 'len-15-16': [3, 15, 16, 31, 32, 15, 16, 1],
            'len-31-32': [1, 31, 32, 16, 15, 1, 1, 1]}
    for k, runs in seqs.items():
        out[f'string-{k}'] = _case(f'string-{k}', [mask32_from_runs(runs)], [unit_box(1, 0)], 32, 34, (0.5,),
                                   runs=[32 + runs[0]] + runs[1:])
    out['string-run0-zero'] = _case('string-run0-zero', [mask32_from_runs([0, 15, 16, 31, 32, 1])], [unit_box(0, 0)], 32, 33,
                                    (0.5,), runs=[0, 15, 16, 31, 32, 1])
    # a first run above 2^20: a small box near the right edge of a 1100 x 1000 image
    out['first-run-2^20'] = _case('first-run-2^20', [rs.rand(14, 14).astype(F32)], [[960.5, 500.25, 990, 540]], 1100, 1000,
                                  (0.5,), first_run_above=1 << 20)
    return out


def src_cases() -> dict:
    """Source-size launches: name -> (case in the NETWORK frame, net_hw, list of src_hw; D rows per image)."""
    out = {}
    rs = np.random.RandomState(700)

    def boxes(n, H, W):
        x0, y0 = rs.rand(n) * W * 0.6, rs.rand(n) * H * 0.6
        return np.stack([x0, y0, np.minimum(x0 + rs.rand(n) * W * 0.5 + 2, W), np.minimum(y0 + rs.rand(n) * H * 0.5 + 2, H)], 1)
    # scales that are no floats: 1333 / 500 and 800 / 333; two images of different size in one launch
    D = 3
    out['scales'] = (_case('scales', list(rs.rand(2 * D, 14, 14).astype(F32)), boxes(2 * D, 800, 1333), 800, 1333, (0.5, 0.3)),
                     (800, 1333), [(333, 500), (120, 97)])
    # sizes 1, 16384 and 16385 on one axis, the other tiny; 16385 comes out empty
    D = 2
    b = np.array([[0, 0, 64, 48], [10.5, 7.25, 50, 40]] * 6, F32)
    probs = list(rs.rand(6 * D, 14, 14).astype(F32))
    probs[6] = np.ones((14, 14), F32)        # the full 2 x 16384 image: one run (a random mask alternates along the columns
    #                                          where its two rows differ and overflows the transition cap: row 7 may)
    out['limits'] = (_case('limits', probs, b, 48, 64, (0.5,)),
                     (48, 64), [(1, 5), (3, 1), (16384, 2), (2, 16384), (16385, 2), (2, 16385)])
    return out


def overlap_cases() -> dict:
    """name -> (case, G): row blocks, pixel words, mask passes and degenerate detections of overlap_detection."""
    out = {}
    rs = np.random.RandomState(800)
    pr = lambda n, MS=14: [rs.rand(MS, MS).astype(F32) * F32(0.6) + F32(0.4) for _ in range(n)]
    # rows: a region of rows 31..33, one wholly in block 0, one wholly in block 1, all three blocks
    out['row-blocks'] = (_case('row-blocks', pr(4), [[3, 32, 40, 33], [3, 1, 40, 30], [3, 33, 40, 62], [3, 1, 40, 68]], 70, 50,
                               (0.5, 0.3), blocks={0: [0, 1], 1: [0], 2: [1], 3: [0, 1, 2]}), 3)
    # words: regions that start at x = 63, 64, 65 and end at 128
    out['words'] = (_case('words', pr(4), [[64, 2, 127, 9], [65, 2, 127, 9], [66, 2, 127, 9], [1, 1, 127, 9]], 12, 129,
                          (0.5, 0.3), x0={0: 63, 1: 64, 2: 65}, x1=128), 2)
    # sizes: W in {1, 63, 64, 65, 129}, H in {1, 7, 8, 9, 33}, G in {1, 64, 65, 129}; an empty region beside full ones
    for H, W, G in ((1, 1, 1), (7, 63, 64), (8, 64, 65), (9, 65, 129), (33, 129, 65), (33, 63, 1)):
        bx = [[0, 0, W, H], [-2, -2, W + 2, H + 2], [W + 5, 1, W + 9, 4], [W * 0.25, H * 0.25, W * 0.75 + 1, H * 0.75 + 1],
              [0, 0, W, H]]
        probs = pr(5)
        probs[4] = np.ones((14, 14), F32)
        out[f'size-{H}x{W}-g{G}'] = (_case(f'size-{H}x{W}-g{G}', probs, bx, H, W, (0.5, 0.3), empty=[2]), G)
    # mask sizes other than 14 share the kernel's staging loop
    out['m28'] = (_case('m28', pr(3, 28), [[3.5, 2.25, 60, 40], [30, 31, 90, 66], [0, 0, 100, 70]], 70, 100, (0.5,)), 5)
    return out


def gt_masks_for(H: int, W: int, G: int, seed: int = 0) -> np.ndarray:
    """G ground-truth masks: random at several densities, with the pixels at and around x = W - 1 and the corners set in
    the first ones, one full and one empty."""
    rs = np.random.RandomState(900 + seed)
    g = rs.rand(G, H, W) > rs.rand(G, 1, 1)
    g[0, :, max(W - 2, 0):] = True
    if G > 1:
        g[1] = False
        g[1, :, W - 1] = True
    if G > 2:
        g[2] = True
    if G > 3:
        g[3] = False
    return g


DENSE_SIZES = [(H, W) for H in (1, 15, 16, 17, 1024, 1025, 1040) for W in (1, 3, 70)] + [(1024, 130), (1025, 130)]


def dense_patterns(H: int, W: int) -> np.ndarray:
    """first and last row of every column, full, empty, alternating rows, random."""
    ends = np.zeros((H, W), bool)
    ends[0] = ends[H - 1] = True
    alt = np.zeros((H, W), bool)
    alt[0::2] = True
    rnd = np.random.RandomState(H * 131 + W).rand(H, W) > 0.9
    last = np.zeros((H, W), bool)
    last[H - 1] = True
    return np.stack([ends, np.ones((H, W), bool), np.zeros((H, W), bool), alt, rnd, last])
