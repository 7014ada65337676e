"""Instance masks as box + colour (host side).

The reference's character datasets (cfg1 MNISTISEG, cfg2 OMNIISEG) store no mask: per instance they hold a box
and the RGB colour the character was pasted in (``*_colors.pkl``, ``info_isegmaps``, mnistiseg_ds.py:103), and the
mask is derived from the image for every sample (``get_isegmap`` -> ``get_char_mask_by_color``,
create_img_from_chars.py:136-158, called at base_fst.py:836 for the query and :1107 for every support instance):
the pixels of the box within +-75 of the colour, dilated by a 3x3 element inside the box.  ``ColorMasks`` carries
exactly what the dataset stores - 7 integers per instance -, ``as_color_masks`` checks it, and the device makes
the masks from the image bytes it already holds (``ops.color_masks``): nothing dense crosses the bus.

The one host statement of the rule stays ``cluttered_chars.char_mask_by_color``; ``ColorMasks.dense`` calls it.
"""
from __future__ import annotations

import numpy as np

from . import cluttered_chars as cc

MAX_DIM = 16384          # ops.RESIZE_MAX_DIM (this module stays free of torch)
REC_BYTES = 64           # 4 * ops.CM_REC_INTS: the record that crosses the bus per mask
DEFAULT_SHIFT = 75       # create_img_from_chars.py:136: get_char_mask_by_color(..., shift=75)
_KEYS = ({'bboxes', 'colors'}, {'bboxes', 'colors', 'shift'})


class ColorMasks:
    """The n masks of one image (or the one mask of a support instance) as the dataset stores them: ``boxes`` int32
    [n,4] in the reference's (ymin, xmin, ymax, xmax) order, ``colors`` uint8 [n,3] RGB, ``shift`` the half width of
    the colour window, ``shape`` = (n, h, w) with (h, w) the size of the image the boxes live in.  A mask exists only
    together with its image: ``dense(img)`` derives it on the host, ``ops.color_masks`` on the device.  Built by
    ``as_color_masks``, which checks what this class takes for granted."""

    def __init__(self, boxes: np.ndarray, colors: np.ndarray, hw, shift: int = DEFAULT_SHIFT, img=None):
        self.boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        self.colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        self.shift = int(shift)
        self.shape = (int(self.boxes.shape[0]), int(hw[0]), int(hw[1]))
        self.img = img          # optional: the image [h,w,3] uint8 (array or tensor) ``dense()`` falls back to

    def __len__(self) -> int:
        return self.shape[0]

    def bounds(self) -> tuple:
        """(lo, hi) int32 [n,3]: the inclusive colour window, ``max(c - shift, 0)`` .. ``min(c + shift, 255)``."""
        c = self.colors.astype(np.int32)
        return np.maximum(c - self.shift, 0), np.minimum(c + self.shift, 255)

    def in_window(self, wy: int, wx: int, wh: int, ww: int, what: str = 'masks', reader: str = 'the crop'):
        """This ONE mask moved into the frame of the window (wy, wx, wh, ww) of its image, which ``reader`` reads; the
        window must hold the whole box - and with it every pixel the mask is made from."""
        y0, x0, y1, x1 = (int(v) for v in self.boxes[0])
        if not (wy <= y0 and y1 <= wy + wh and wx <= x0 and x1 <= wx + ww):
            raise ValueError(f'{what}: the box {[y0, x0, y1, x1]} of the colour item leaves the window '
                             f'{[wy, wx, wy + wh, wx + ww]} that {reader} reads: give the instance\'s own box')
        return ColorMasks(self.boxes - np.array([wy, wx] * 2, np.int32), self.colors, (wh, ww), self.shift)

    def dense(self, img=None) -> np.ndarray:
        """Host masks: bool [n,h,w] by ``cluttered_chars.char_mask_by_color`` on ``img`` (uint8 [h,w,3]; default: the
        image this carrier was bound to)."""
        img = self.img if img is None else img
        n, h, w = self.shape
        if img is None:
            raise ValueError('ColorMasks.dense: a colour mask is derived from its image; give img [h,w,3] uint8')
        if hasattr(img, 'detach'):
            img = img.detach().cpu().numpy()
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.shape != (h, w, 3):
            raise ValueError(f'ColorMasks.dense: img must be uint8 {[h, w, 3]}, got {img.dtype} {list(img.shape)}')
        out = np.zeros((n, h, w), bool)
        for i in range(n):
            out[i] = cc.char_mask_by_color(img, [int(v) for v in self.boxes[i]], self.colors[i], self.shift)
        return out


def is_color(entry) -> bool:
    """Whether ``entry`` is a box + colour entry: a ``ColorMasks``, or a dict with exactly the keys ``bboxes`` and
    ``colors`` (and optionally ``shift``).  Decided by type and key names alone."""
    if isinstance(entry, ColorMasks):
        return True
    return isinstance(entry, dict) and set(entry.keys()) in _KEYS


def _integral(v, what: str, shape_tail: int) -> np.ndarray:
    """A [n, shape_tail] (or [shape_tail]) array of integral numbers as int64; anything else is a ValueError."""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v)
    except Exception:
        raise ValueError(f'{what}: not an array of numbers') from None
    if a.dtype == bool or a.dtype.kind not in 'iuf':
        raise ValueError(f'{what}: expected numbers, got {a.dtype}')
    if a.ndim == 1 and a.size == shape_tail:
        a = a.reshape(1, shape_tail)
    if a.size == 0:
        a = a.reshape(0, shape_tail)
    if a.ndim != 2 or a.shape[1] != shape_tail:
        raise ValueError(f'{what}: expected [n,{shape_tail}], got {list(a.shape)}')
    if a.dtype.kind == 'f' and not (np.all(np.isfinite(a)) and np.all(a == np.floor(a))):
        raise ValueError(f'{what}: values must be integral')
    return a.astype(np.int64)


def as_color_masks(item, hw, what: str = 'masks', img=None) -> ColorMasks:
    """One image's masks as box + colour -> a checked ``ColorMasks`` at ``hw`` = (h, w) (host only; ValueError names
    the item): ``item`` is a ``ColorMasks`` (checked against ``hw``; None: its own size) or a dict
    ``{'bboxes': [n,4] YXYX, 'colors': [n,3] RGB[, 'shift': int]}``.  Sizes within 1..16384; every box integral with
    0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w - an empty box is legal and gives an empty mask; colours integral within
    0..255; as many colours as boxes; shift within 0..255.  n == 0 is legal.  ``img``: the image to bind for
    ``dense()``."""
    if isinstance(item, ColorMasks):
        boxes, colors, shift = item.boxes, item.colors, item.shift
        if hw is None:
            hw = item.shape[1:]
        elif tuple(int(v) for v in hw) != item.shape[1:]:
            raise ValueError(f'{what}: colour masks of size {list(item.shape[1:])}, expected {[int(v) for v in hw]}')
        img = item.img if img is None else img
    elif isinstance(item, dict) and set(item.keys()) in _KEYS:
        boxes, colors, shift = item['bboxes'], item['colors'], item.get('shift', DEFAULT_SHIFT)
    else:
        raise ValueError(f"{what}: expected a ColorMasks or a dict {{'bboxes', 'colors'[, 'shift']}}, got "
                         f'{type(item).__name__}')
    if hw is None:
        raise ValueError(f'{what}: a box + colour entry has no size of its own')
    h, w = int(hw[0]), int(hw[1])
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f'{what}: sizes must be within 1..{MAX_DIM}, got {[h, w]}')
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= int(shift) <= 255:
        raise ValueError(f'{what}: shift must be an int within 0..255, got {shift!r}')
    b = _integral(boxes, f'{what}: bboxes', 4)
    c = _integral(colors, f'{what}: colors', 3)
    if len(b) != len(c):
        raise ValueError(f'{what}: {len(b)} boxes for {len(c)} colours')
    bad = ~((0 <= b[:, 0]) & (b[:, 0] <= b[:, 2]) & (b[:, 2] <= h) & (0 <= b[:, 1]) & (b[:, 1] <= b[:, 3]) & (b[:, 3] <= w))
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError(f'{what}: box {j} = {b[j].tolist()} is not 0 <= y0 <= y1 <= {h}, 0 <= x0 <= x1 <= {w}')
    if c.size and (c.min() < 0 or c.max() > 255):
        j = int(np.flatnonzero(((c < 0) | (c > 255)).any(1))[0])
        raise ValueError(f'{what}: colour {j} = {c[j].tolist()} is outside 0..255')
    return ColorMasks(b, c, (h, w), int(shift), img)
