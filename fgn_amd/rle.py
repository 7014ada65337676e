"""COCO run-length encoding of binary masks (host side of result packing).

The reference packs masks with mmdet ``encode_mask_results`` -> pycocotools
``encode`` (fgn.py:281,298): column-major runs, alternating starting with a zero-run,
compressed to the COCO ASCII string (5 data bits + continuation bit per char,
delta-coded against the run two back from the 4th run on).  Vectorised numpy: no
per-run Python loop.

The input side: the reference's COCO dataset holds every instance
as ``[size, counts]`` with the compressed string (coco_ds.py:195-207, 229-238) and
decodes it on the host per sample (``get_isegmap``, coco_ds.py:265-278).  Here
``string_to_counts`` parses the string, ``as_masks`` checks a list of such items and
turns it into an ``RleMasks`` - the cumulative run ends the device decodes from
(``ops.rle_decode_masks``) - and nothing dense crosses the bus.
"""
from __future__ import annotations

import numpy as np

MAX_DIM = 16384          # ops.RESIZE_MAX_DIM (this module stays free of torch): p = x * h + y < 2^28


def counts_to_string(counts: np.ndarray) -> bytes:
    """COCO ``rleToString`` for one uncompressed counts array."""
    x = np.asarray(counts, dtype=np.int64).copy()
    if x.size > 3:
        x[3:] -= np.asarray(counts, dtype=np.int64)[1:-2]
    n = x.size
    chars = np.zeros((n, 13), np.uint8)
    active = np.ones(n, bool)
    used = np.zeros((n, 13), bool)
    for k in range(13):
        if not active.any():
            break
        c = x & 0x1f
        x = x >> 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        c = np.where(more, c | 0x20, c) + 48
        chars[active, k] = c[active]
        used[active, k] = True
        active = active & more
    return chars[used].tobytes()


def mask_to_counts(mask: np.ndarray) -> np.ndarray:
    """Uncompressed column-major run lengths of one [H,W] binary mask."""
    flat = np.ascontiguousarray(np.asarray(mask, np.uint8).T).reshape(-1)
    if flat.size == 0:
        return np.zeros(1, np.int64)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate(([0], change, [flat.size]))
    counts = np.diff(bounds)
    if flat[0]:
        counts = np.concatenate(([0], counts))
    return counts.astype(np.int64)


def encode(mask: np.ndarray) -> dict:
    h, w = mask.shape
    return {'size': [int(h), int(w)], 'counts': counts_to_string(mask_to_counts(mask))}


def encode_many(masks) -> list:
    return [encode(m) for m in masks]


def decode(rle: dict) -> np.ndarray:
    """Inverse of :func:`encode` (used by the evaluator and the tests)."""
    h, w = rle['size']
    s = rle['counts']
    if isinstance(s, str):
        s = s.encode('ascii')
    counts = []
    p = 0
    while p < len(s):
        x = 0
        k = 0
        more = True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    flat = np.zeros(h * w, np.uint8)
    pos = 0
    v = 0
    for c in counts:
        if v:
            flat[pos:pos + c] = 1
        pos += c
        v ^= 1
    return flat.reshape(w, h).T


# ---- RLE as an INPUT form (the ground-truth and support masks of an episode) ---------------------------------------
def string_to_counts(s) -> np.ndarray:
    """COCO ``rleFrString`` for one compressed string (bytes / str): the inverse of ``counts_to_string``, int64 counts.
    No loop over characters or runs: a character carries 5 data bits, 0x20 continues the value, bit 0x10 of a value's
    last character extends the sign; from the 4th value on each is a delta against the value two back, undone by two
    strided cumulative sums (the odd chain from index 1, the even chain from index 2; index 0 stands alone)."""
    if isinstance(s, str):
        s = s.encode('ascii')
    c = np.frombuffer(bytes(s), np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return np.zeros(0, np.int64)
    if c.min() < 0 or c.max() > 63:
        raise ValueError('RLE string: a character outside the COCO alphabet (codes 48..111)')
    last = (c & 0x20) == 0                               # the last character of its value
    if not last[-1]:
        raise ValueError('RLE string: ends inside a value (continuation bit set on the last character)')
    ends = np.flatnonzero(last)
    starts = np.concatenate(([0], ends[:-1] + 1))
    length = ends - starts + 1
    if length.max() > 12:
        raise ValueError('RLE string: a value of more than 12 characters (60 bits)')
    k = np.arange(c.size) - np.repeat(starts, length)    # position of a character inside its value
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)
    x = np.where((c[ends] & 0x10) != 0, x - (np.int64(1) << (5 * length)), x)
    x[1::2] = np.cumsum(x[1::2])
    if x.size > 2:
        x[2::2] = np.cumsum(x[2::2])
    return x


class RleMasks:
    """The n masks of one image (or the one mask of a support instance) as run ends: ``shape`` = (n, h, w); ``ends``
    uint32, the cumulative run ends of all masks concatenated, each mask counted from its own 0 (its last entry is
    h * w); ``first`` int64 [n+1], mask i owning ``ends[first[i]:first[i+1]]``.  Pixel (y, x) of a mask sits at
    column-major position p = x * h + y and is set where an odd number of its ends are <= p - which is also what a
    zero-length run (a repeated end) means to pycocotools.  Built by ``as_masks``, which checks what this class takes
    for granted."""

    def __init__(self, shape, ends: np.ndarray, first: np.ndarray):
        self.shape = tuple(int(v) for v in shape)
        self.ends = np.ascontiguousarray(ends, np.uint32)
        self.first = np.ascontiguousarray(first, np.int64)

    def __len__(self) -> int:
        return self.shape[0]

    def dense(self) -> np.ndarray:
        """Host decode: uint8 0/1 [n,h,w] (one search over all masks; no loop over masks, runs or pixels)."""
        n, h, w = self.shape
        if n == 0:
            return np.zeros((0, h, w), np.uint8)
        hw = h * w
        per = np.diff(self.first)
        # mask i's ends shifted by i * (hw + 1): the concatenation is sorted, and one search serves every mask
        shift = np.arange(n, dtype=np.int64) * (hw + 1)
        keys = self.ends.astype(np.int64) + np.repeat(shift, per)
        p = np.arange(hw, dtype=np.int64)[None, :] + shift[:, None]
        r = np.searchsorted(keys, p.reshape(-1), side='right').reshape(n, hw) - self.first[:-1, None]
        return np.ascontiguousarray((r & 1).astype(np.uint8).reshape(n, w, h).transpose(0, 2, 1))


def is_rle(entry) -> bool:
    """Whether ``entry`` is in an RLE form ``as_masks`` takes (an ``RleMasks``, or a list / tuple whose items are dicts
    or ``[size, counts]`` pairs; the empty list counts) rather than a dense array or tensor."""
    if isinstance(entry, RleMasks):
        return True
    return isinstance(entry, (list, tuple)) and all(is_item(it) for it in entry)


def is_item(it) -> bool:
    """Whether ``it`` has the form of ONE RLE mask: a dict, or the reference's ``[size, counts]`` pair - ``size`` two
    integer scalars, ``counts`` the compressed string (bytes / str) or a flat integer array.  Decided by types alone:
    no array is built from the argument, which may be any nesting of lists (a support set, a dense mask as lists)."""
    if isinstance(it, dict):
        return True
    if not (isinstance(it, (list, tuple)) and len(it) == 2):
        return False
    size, counts = it
    if isinstance(size, np.ndarray):
        ok = size.shape == (2,) and size.dtype.kind in 'iu'
    else:
        ok = isinstance(size, (list, tuple)) and len(size) == 2 and \
            all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in size)
    return ok and (isinstance(counts, (bytes, str)) or
                   (isinstance(counts, np.ndarray) and counts.ndim == 1 and counts.dtype.kind in 'iu'))


def as_masks(entry, hw=None, what: str = 'masks') -> RleMasks:
    """The masks of one image in RLE -> ``RleMasks``, every check made here (host only; ValueError names the item):
    ``entry`` is a list of n items, each a pycocotools dict ``{'size': [h, w], 'counts': bytes | str | list | ndarray}``
    or the reference's ``[size, counts]`` pair (coco_ds.py:195-207; the size may be ``np.int16``) - a string is the
    compressed form, a list / array the uncompressed counts - or an ``RleMasks`` (checked against ``hw`` only), or an
    empty list, which takes its size from ``hw``.  Sizes within 1..16384, all items of one size (``hw`` where given),
    counts non-negative, summing to h * w, at least one run.  Zero-length runs are legal."""
    if hw is not None:
        hw = (int(hw[0]), int(hw[1]))
    if isinstance(entry, RleMasks):
        if hw is not None and entry.shape[1:] != hw:
            raise ValueError(f'{what}: RLE masks of size {list(entry.shape[1:])}, expected {list(hw)}')
        return entry
    if not isinstance(entry, (list, tuple)):
        raise ValueError(f'{what}: expected a list of RLE items or an RleMasks, got {type(entry).__name__}')
    if len(entry) == 0:
        if hw is None:
            raise ValueError(f'{what}: an empty list of RLE items has no size of its own')
        if not (1 <= hw[0] <= MAX_DIM and 1 <= hw[1] <= MAX_DIM):
            raise ValueError(f'{what}: sizes must be within 1..{MAX_DIM}, got {list(hw)}')
        return RleMasks((0,) + hw, np.zeros(0, np.uint32), np.zeros(1, np.int64))
    ends, first = [], [0]
    for j, it in enumerate(entry):
        if isinstance(it, dict):
            if 'size' not in it or 'counts' not in it:
                raise ValueError(f"{what}: item {j} needs 'size' and 'counts'")
            size, counts = it['size'], it['counts']
        elif is_item(it):
            size, counts = it
        else:
            raise ValueError(f'{what}: item {j} is neither an RLE dict nor a [size, counts] pair')
        size = np.asarray(size).reshape(-1)
        if size.size != 2 or size.dtype.kind not in 'iu':
            raise ValueError(f'{what}: item {j} has size {size.tolist()}, expected two integers [h, w]')
        h, w = int(size[0]), int(size[1])
        if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
            raise ValueError(f'{what}: item {j}: sizes must be within 1..{MAX_DIM}, got {[h, w]}')
        if hw is None:
            hw = (h, w)
        if (h, w) != hw:
            raise ValueError(f'{what}: item {j} is of size {[h, w]}, expected {list(hw)}')
        if isinstance(counts, (bytes, str)):
            try:
                cnt = string_to_counts(counts)
            except ValueError as e:
                raise ValueError(f'{what}: item {j}: {e}') from None
        else:
            cnt = np.asarray(counts)
            if cnt.ndim != 1 or (cnt.size and cnt.dtype.kind not in 'iu'):
                raise ValueError(f'{what}: item {j}: uncompressed counts are a flat list of integers')
            cnt = cnt.astype(np.int64)
        if cnt.size == 0:
            raise ValueError(f'{what}: item {j} has no run')
        if cnt.min() < 0:
            raise ValueError(f'{what}: item {j} has a negative count')
        if cnt.max() > h * w or int(cnt.sum()) != h * w:
            raise ValueError(f'{what}: item {j}: counts sum to {int(cnt.sum())}, the mask has {h * w} pixels')
        ends.append(np.cumsum(cnt).astype(np.uint32))
        first.append(first[-1] + cnt.size)
    return RleMasks((len(entry),) + hw, np.concatenate(ends), np.asarray(first, np.int64))
