"""Instance masks as COCO polygons (host side).

Almost every non-crowd annotation of ``instances_*.json`` holds its mask as a list of polygons, ``segmentation`` =
``[[x0, y0, x1, y1, ...], ...]``.  The reference turns them into RLE once, at dataset build, through pycocotools
(``maskUtils.frPyObjects`` + ``merge``, coco_ds.py:246-263).  This module states the rule of pycocotools' ``rleFrPoly``
in numpy - restated from memory, pinned by nothing here ("Unpinned") - so that a polygon entry can be
checked on the host (``as_polys``), rasterised there (``dense``, ``to_rle``) and, from the same records, on the device
(``ops.poly_masks``): a few hundred bytes per instance cross the bus instead of runs or pixels.

The rule, for one part ``xy`` of k >= 3 vertices on an h x w mask (doubles; ``(int)`` truncates toward zero):
  1. X[j] = (int)(5 x_j + .5), Y[j] likewise; the path is closed with X[k] = X[0], Y[k] = Y[0].
  2. every edge is walked along its major axis, one point per step, the minor coordinate (int)(start + s * t + .5) with
     s the slope (one division per edge); an edge that runs against its major axis is walked from its far end with
     t counted down, so the path keeps the polygon's direction.  The points of all edges form one path u[], v[].
  3. where u changes between neighbours of the path, m = u[j] < u[j-1] ? u[j] : u[j] - 1 is a crossing of a pixel
     column's centre line iff m >= 2, m % 5 == 2 and cx = (m - 2) / 5 <= w - 1; its row is
     cy = clamp(floor((min(v[j], v[j-1]) + 2) / 5), 0, h); it toggles the column-major position cx * h + cy.
  4. pixel (y, x) is set where an odd number of positions are <= x * h + y - the rule of ``rle.RleMasks``.
  5. an instance is the OR of its parts (``maskUtils.merge``, union).
"""
from __future__ import annotations

import numpy as np

from . import rle

MAX_DIM = 16384              # ops.RESIZE_MAX_DIM (this module stays free of torch)
MAX_COORD = 65536            # |x|, |y| of a vertex: 5 * 65536 + 1 stays far inside int32 and exact in a double
CROSSING_CAP = 8192          # csrc/poly.hip: positions of one part the device sorts in LDS
POINT_CAP = 1 << 20          # dense path points of one part the device walks
EDGE_INTS = 8                # csrc/poly.hip: {xs, ys, steps, major | flip << 1, s lo, s hi, first, 0} per edge


def _upsampled(xy) -> tuple:
    """Step 1: the closed integer path (X, Y) int64 [k+1] of one part."""
    a = np.asarray(xy, np.float64).reshape(-1, 2)
    X = np.trunc(5.0 * a[:, 0] + .5).astype(np.int64)
    Y = np.trunc(5.0 * a[:, 1] + .5).astype(np.int64)
    return np.append(X, X[0]), np.append(Y, Y[0])


def part_edges(xy) -> dict:
    """Step 2 per edge, as the device reads it: ``xs``, ``ys`` the start AFTER the flip, ``steps`` = max(dx, dy),
    ``major`` (1: x, dx >= dy), ``flip``, ``s`` the slope as a double (the one division of an edge; 0 for an edge of no
    length, where C divides 0 / 0 into a v that no crossing reads) and ``first`` the index of its first point in the
    part's path; ``points`` = M and ``bound`` = sum of floor(dx / 5) + 2, which no count of crossings exceeds."""
    X, Y = _upsampled(xy)
    xs, xe, ys, ye = X[:-1], X[1:], Y[:-1], Y[1:]
    dx, dy = np.abs(xe - xs), np.abs(ye - ys)
    major = dx >= dy
    flip = (major & (xs > xe)) | (~major & (ys > ye))
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    steps = np.where(major, dx, dy)
    num = np.where(major, ye - ys, xe - xs).astype(np.float64)
    s = np.divide(num, steps.astype(np.float64), out=np.zeros(len(steps), np.float64), where=steps > 0)
    first = np.concatenate(([0], np.cumsum(steps + 1)))
    return dict(xs=xs, ys=ys, steps=steps, major=major, flip=flip, s=s, first=first[:-1], points=int(first[-1]),
                bound=int(np.sum(dx // 5 + 2)))


def edge_records(xy) -> tuple:
    """One part as the device reads it: (int32 [E, 8] records {xs, ys, steps, major | flip << 1, s lo, s hi, first, 0},
    the length M of its path, its slice capacity - the power of two that holds ``bound`` positions)."""
    e = part_edges(xy)
    r = np.zeros((len(e['steps']), EDGE_INTS), np.int32)
    r[:, 0], r[:, 1], r[:, 2] = e['xs'], e['ys'], e['steps']
    r[:, 3] = e['major'].astype(np.int32) | (e['flip'].astype(np.int32) << 1)
    r[:, 4:6] = np.ascontiguousarray(e['s'], '<f8').view('<i4').reshape(-1, 2)
    r[:, 6] = e['first']
    return r, e['points'], 1 << max(e['bound'] - 1, 0).bit_length()


def part_path(xy) -> tuple:
    """Step 2: the path (u, v) int64 [M] of one part - every point in closed form from its edge, as a lane of the
    device forms it.  ``ys + s * t + .5`` is a product rounded, then two sums rounded; numpy fuses nothing."""
    e = part_edges(xy)
    n = e['steps'] + 1
    k = np.repeat(np.arange(len(n)), n)
    d = np.arange(e['points']) - e['first'][k]
    t = np.where(e['flip'][k], e['steps'][k] - d, d)
    tf = t.astype(np.float64)
    minor0 = np.where(e['major'][k], e['ys'][k], e['xs'][k]).astype(np.float64)
    minor = np.trunc(minor0 + e['s'][k] * tf + .5).astype(np.int64)
    u = np.where(e['major'][k], e['xs'][k] + t, minor)
    v = np.where(e['major'][k], minor, e['ys'][k] + t)
    return u, v


def crossing_of(m, n, h: int, w: int) -> tuple:
    """Step 3 for arrays of ``m`` (the column candidate) and ``n`` = min(v[j], v[j-1]) -> (is a crossing, cx, cy), in
    integers.  These forms equal the C expressions exactly: xd = (m + .5) / 5 - .5 is integral iff m % 5 == 2 (then m +
    .5 = 5 cx + 2.5 and the quotient cx + .5 is exact; otherwise xd is at least .2 from an integer, far beyond any
    rounding at |m| < 2^21), and ceil(clamp((n + .5) / 5 - .5, 0, h)) = clamp(floor((n + 2) / 5), 0, h) because
    (n + .5) / 5 - .5 = (n - 2) / 5 is never integral + tiny: its fraction is one of 0, .2, .4, .6, .8 up to rounding,
    and 0 happens for n % 5 == 2 only, where it is exact.  ``double_crossing_of`` evaluates the C forms; the CPU test
    compares the two."""
    m, n = np.asarray(m, np.int64), np.asarray(n, np.int64)
    cx = (m - 2) // 5
    hit = (m >= 2) & (m % 5 == 2) & (cx <= w - 1)
    cy = np.clip((n + 2) // 5, 0, h)
    return hit, cx, cy


def double_crossing_of(m, n, h: int, w: int) -> tuple:
    """Step 3 as the C code writes it, in doubles: xd = (m + .5) / 5 - .5, a crossing iff xd is integral, >= 0 and
    <= w - 1; yd = clamp((n + .5) / 5 - .5, 0, h), cy = ceil(yd)."""
    xd = (np.asarray(m, np.float64) + .5) / 5.0 - .5
    hit = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.clip((np.asarray(n, np.float64) + .5) / 5.0 - .5, 0.0, float(h))
    return hit, xd.astype(np.int64), np.ceil(yd).astype(np.int64)


def part_crossings(xy, h: int, w: int) -> np.ndarray:
    """Steps 1-3 for one part: the sorted uint32 column-major positions at which the part's mask toggles.  With a final
    h * w they are the ``ends`` of an ``rle.RleMasks``."""
    u, v = part_path(xy)
    ch = np.flatnonzero(u[1:] != u[:-1]) + 1
    m = np.where(u[ch] < u[ch - 1], u[ch], u[ch] - 1)
    hit, cx, cy = crossing_of(m, np.minimum(v[ch], v[ch - 1]), h, w)
    return np.sort((cx[hit] * h + cy[hit]).astype(np.uint32))


def _parity(pos: np.ndarray, h: int, w: int) -> np.ndarray:
    """Step 4: uint8 [h, w] from sorted positions."""
    r = np.searchsorted(pos, np.arange(h * w, dtype=np.int64), side='right')
    return np.ascontiguousarray((r & 1).astype(np.uint8).reshape(w, h).T)


def dense(parts, h: int, w: int) -> np.ndarray:
    """Steps 1-5 for one instance: uint8 0/1 [h, w], the OR of its parts' masks."""
    out = np.zeros((h, w), np.uint8)
    for xy in parts:
        out |= _parity(part_crossings(xy, h, w), h, w)
    return out


def to_rle(parts, h: int, w: int) -> dict:
    """The instance as the dict ``rle.encode`` gives for its mask (the host route of an instance over the device's
    capacity, and what ``maskUtils.frPyObjects`` + ``merge`` hand the reference)."""
    return rle.encode(dense(parts, h, w))


class PolyMasks:
    """The n masks of one image (or the one mask of a support instance) as polygons: ``shape`` = (n, h, w); ``xy``
    float64, the vertices of all parts concatenated (x0, y0, x1, y1, ...); ``part_first`` int64 [P+1], part q owning
    ``xy[part_first[q]:part_first[q+1]]``; ``inst_first`` int64 [n+1], instance i owning the parts
    ``inst_first[i]:inst_first[i+1]``; ``crossing_bound`` int64 [n], per instance the sum over its edges of
    floor(|dX| / 5) + 2 - no instance toggles more positions; ``part_bound`` / ``part_points`` int64 [P] say the same
    and the dense path length per part, which decide the route (``on_host``).  Built by ``as_polys``, which checks what
    this class takes for granted."""

    def __init__(self, shape, xy: np.ndarray, part_first: np.ndarray, inst_first: np.ndarray):
        self.shape = tuple(int(v) for v in shape)
        self.xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
        self.part_first = np.ascontiguousarray(part_first, np.int64)
        self.inst_first = np.ascontiguousarray(inst_first, np.int64)
        P = len(self.part_first) - 1
        self.part_bound = np.zeros(P, np.int64)
        self.part_points = np.zeros(P, np.int64)
        for q in range(P):
            e = part_edges(self.part(q))
            self.part_bound[q], self.part_points[q] = e['bound'], e['points']
        csum = np.concatenate(([0], np.cumsum(self.part_bound)))
        self.crossing_bound = csum[self.inst_first[1:]] - csum[self.inst_first[:-1]]

    def __len__(self) -> int:
        return self.shape[0]

    def part(self, q: int) -> np.ndarray:
        return self.xy[self.part_first[q]:self.part_first[q + 1]]

    def parts(self, i: int) -> list:
        return [self.part(q) for q in range(int(self.inst_first[i]), int(self.inst_first[i + 1]))]

    def on_host(self) -> np.ndarray:
        """bool [n]: the instances that travel as ``to_rle`` through the RLE path - any part of theirs may toggle more
        positions than the device sorts, or walks more points than it takes.  Decided here, before anything is queued."""
        over = (self.part_bound > CROSSING_CAP) | (self.part_points > POINT_CAP)
        c = np.concatenate(([0], np.cumsum(over)))
        return (c[self.inst_first[1:]] - c[self.inst_first[:-1]]) > 0

    def select(self, idx) -> 'PolyMasks':
        """The instances ``idx`` (in that order) as a ``PolyMasks`` of their own."""
        xy, pf, inf = [], [0], [0]
        for i in idx:
            for p in self.parts(int(i)):
                xy.append(p)
                pf.append(pf[-1] + p.size)
            inf.append(len(pf) - 1)
        return PolyMasks((len(inf) - 1,) + self.shape[1:], np.concatenate(xy) if xy else np.zeros(0), pf, inf)

    def rle_items(self, idx) -> list:
        """``to_rle`` of the instances ``idx``."""
        return [to_rle(self.parts(int(i)), *self.shape[1:]) for i in idx]

    def dense(self) -> np.ndarray:
        """Host rasterisation: uint8 0/1 [n, h, w]."""
        n, h, w = self.shape
        out = np.zeros((n, h, w), np.uint8)
        for i in range(n):
            out[i] = dense(self.parts(i), h, w)
        return out


def is_poly(entry) -> bool:
    """Whether ``entry`` is a polygon entry: a ``PolyMasks``, or a dict with the key ``polygons`` (and optionally
    ``size``).  Decided by type and key names alone; a bare nested list is never one (it cannot be told from a dense mask
    given as lists)."""
    if isinstance(entry, PolyMasks):
        return True
    return isinstance(entry, dict) and set(entry.keys()) in ({'polygons'}, {'polygons', 'size'})


def _part(p, what: str) -> np.ndarray:
    if hasattr(p, 'detach'):
        p = p.detach().cpu().numpy()
    if isinstance(p, (str, bytes, dict)):
        raise ValueError(f'{what}: expected a flat sequence of numbers x0, y0, x1, y1, ..., got {type(p).__name__}')
    try:
        a = np.asarray(p)
    except Exception:
        raise ValueError(f'{what}: not a flat sequence of numbers') from None
    if a.ndim != 1 or a.dtype == bool or a.dtype.kind not in 'iuf':
        raise ValueError(f'{what}: expected a flat sequence of numbers x0, y0, x1, y1, ..., got {a.dtype} '
                         f'{list(a.shape)}')
    if a.size < 6 or a.size % 2:
        raise ValueError(f'{what}: {a.size} numbers; a part has at least 3 vertices, two numbers each')
    a = a.astype(np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{what}: a coordinate is not finite')
    if np.abs(a).max() > MAX_COORD:
        raise ValueError(f'{what}: a coordinate lies outside +-{MAX_COORD}')
    return a


def as_polys(entry, hw, what: str = 'masks', single: bool = False) -> PolyMasks:
    """One image's masks as polygons -> a checked ``PolyMasks`` at ``hw`` = (h, w) (host only; ValueError names image,
    instance and part): ``entry`` is a ``PolyMasks`` (checked against ``hw``; None: its own size) or a dict
    ``{'polygons': [instance_0, instance_1, ...][, 'size': [h, w]]}``, every instance a list of parts as COCO's
    ``segmentation`` holds them; ``size``, where given, must equal ``hw``, and stands in for it where ``hw`` is None.
    ``single``: the dict holds the parts of ONE instance, ``{'polygons': parts}`` (a support instance).  A part is a
    flat sequence of finite numbers of even length >= 6 within +-65536, an instance has at least one part, sizes lie
    within 1..16384.  An instance without a crossing is legal and gives an empty mask; n == 0 is legal."""
    if hw is not None:
        hw = (int(hw[0]), int(hw[1]))
    if isinstance(entry, PolyMasks):
        if hw is not None and entry.shape[1:] != hw:
            raise ValueError(f'{what}: polygon masks of size {list(entry.shape[1:])}, expected {list(hw)}')
        return entry
    if not is_poly(entry):
        raise ValueError(f"{what}: expected a PolyMasks or a dict {{'polygons'[, 'size']}}, got {type(entry).__name__}")
    if 'size' in entry:
        try:
            size = np.asarray(entry['size']).reshape(-1)
        except Exception:
            size = np.zeros(0)
        if size.size != 2 or size.dtype.kind not in 'iu':
            raise ValueError(f"{what}: 'size' is {entry['size']!r}, expected two integers [h, w]")
        size = (int(size[0]), int(size[1]))
        if hw is not None and size != hw:
            raise ValueError(f'{what}: polygons of size {list(size)}, expected {list(hw)}')
        hw = size
    if hw is None:
        raise ValueError(f'{what}: a polygon entry without \'size\' has no size of its own')
    if not (1 <= hw[0] <= MAX_DIM and 1 <= hw[1] <= MAX_DIM):
        raise ValueError(f'{what}: sizes must be within 1..{MAX_DIM}, got {list(hw)}')
    insts = entry['polygons']
    if not isinstance(insts, (list, tuple)):
        raise ValueError(f"{what}: 'polygons' is a list of instances, each a list of parts, got {type(insts).__name__}")
    if single:
        insts = [insts]
    xy, pf, inf = [], [0], [0]
    for i, parts in enumerate(insts):
        if not isinstance(parts, (list, tuple)):
            raise ValueError(f'{what}: instance {i} is a list of parts, got {type(parts).__name__}')
        if len(parts) == 0:
            raise ValueError(f'{what}: instance {i} has no part')
        for q, p in enumerate(parts):
            a = _part(p, f'{what}: instance {i}, part {q}')
            xy.append(a)
            pf.append(pf[-1] + a.size)
        inf.append(len(pf) - 1)
    return PolyMasks((len(insts),) + hw, np.concatenate(xy) if xy else np.zeros(0), pf, inf)
