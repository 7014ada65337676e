"""Synthetic episodic dataset with the BaseFewShotISEG interface.

The reference's datasets (datasets/fewshotiseg/base_fst.py) need cv2/imgaug and real
images; the hot path only depends on their *sample dict* (base_fst.py:1248-1266) and on
``evaluate`` (base_fst.py:1516-1601).  This class produces that contract from seeded
synthetic episodes so the reference's evaluation loop (main.py:269-326) runs unchanged
on top of ``fgn_amd.detector.FGN``; visualisation side effects of ``evaluate`` are not
reproduced.
"""
from __future__ import annotations

import itertools
import math
import os
import pickle
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from . import cluttered_chars as cc
from . import colormask, episodes, rle
from .fsiseg_eval import FSISEGEval


def get_new_shape(h, w, target_size=800, max_size=1333, check_ar: bool = True):
    """Short side -> target_size, long side = target_size * aspect ratio (truncated), capped at max_size with the
    short side re-derived (cp_utils/create_img_from_chars.py:250-267).  Like the reference, raises AssertionError
    when the truncations move the aspect ratio by more than 0.015 (tiny inputs).  Pinned by
    tests/golden/data_side.npz (the reference's own function on 506 shapes)."""
    old = np.array([h, w], dtype=np.float64)
    new = np.array([h, w], dtype=np.int64)
    long_i = int(np.argmax(np.array([h, w])))
    ar = old[long_i] / old[1 - long_i]
    new[1 - long_i] = target_size
    new[long_i] = int(target_size * ar)
    if new[long_i] > max_size:
        new[long_i] = max_size
        new[1 - long_i] = int(max_size / ar)
    if check_ar:
        assert abs(old[0] / old[1] - new[0] / float(new[1])) <= 0.015, f'Old {old[0] / old[1]} New {new[0] / float(new[1])}'
    return new


def ar_grouped_order(aspect_ratios, batch, target_size=800, max_size=1333, sub_sample_ratio=16, shuffle=True,
                     seed=0, rnd=None):
    """Aspect-ratio-grouped batching (``BaseFewShotISEG.reshuffle``, base_fst.py:626-727): width/height rounded to
    one decimal, one group per value; per-group target (h, w) = get_new_shape(100 / ar, 100) rounded to multiples of
    ``sub_sample_ratio``; every group is padded to a multiple of ``batch`` by re-drawing its own members
    (``random.choices``, whether or not ``shuffle``), shuffled, cut into chunks of ``batch``; the chunks are shuffled.
    Returns (order [n_chunks*batch], group index per entry, per-group (h, w)).  The reference draws from the global
    ``random`` module; here from ``rnd`` (default ``random.Random(seed)``) in the same call order, so
    ``random.seed(s)`` there and ``seed=s`` here give the same order (tests/golden/data_side.npz)."""
    rnd = random.Random(seed) if rnd is None else rnd
    ars = np.around(np.asarray(aspect_ratios, np.float64), decimals=1)
    uniq = sorted(np.unique(ars))
    hws = []
    for a in uniq:
        hws.append(get_new_shape(100 / a, 100, target_size, max_size))
    hws = (np.around(np.array(hws) / sub_sample_ratio) * sub_sample_ratio).astype(np.int32).reshape(-1, 2)
    order, groups = [], []
    for gi, a in enumerate(uniq):
        members = np.flatnonzero(ars == a)
        elems = list(range(len(members)))
        if len(members) % batch:
            elems += rnd.choices(elems, k=batch - len(members) % batch)
        if shuffle:
            rnd.shuffle(elems)
        order.extend(members[elems].tolist())
        groups.extend([gi] * len(elems))
    order = np.asarray(order, np.int32).reshape(-1, batch)
    groups = np.asarray(groups, np.int32).reshape(-1, batch)
    chunks = list(range(len(order)))
    if shuffle:
        rnd.shuffle(chunks)
    return order[chunks].reshape(-1), groups[chunks].reshape(-1), hws


# ---- support crop geometry (BaseFewShotISEG.get_support, base_fst.py:1043-1167) ------------------------------------
def spp_offset_ratio(spp_fill_ratio: float) -> float:
    """base_fst.py:264-265: 1 / (1 + 2 * offset) = fill ratio, rounded to two decimals (0.8 -> 0.12)."""
    return float(np.around(1 / (2 * spp_fill_ratio) - 0.5, decimals=2))


def cut_algorithm(lo: int, hi: int, offset: int, max_shape: int) -> np.ndarray:
    """``BaseFewShotISEG.cut_algorithm`` (base_fst.py:991-998): cut window [lo - offset, hi + offset] clipped to
    [0, max_shape] and the object's extent inside it -> int32 [cut_lo, box_lo, cut_hi, box_hi]."""
    cut_lo = max(0, lo - offset)
    return np.array([cut_lo, lo - cut_lo, min(hi + offset, max_shape), hi - cut_lo], dtype=np.int32)


def get_crop(img: np.ndarray, ymin, xmin, ymax, xmax, h_offset, w_offset, crop_square=True, mode='reflect'):
    """``BaseFewShotISEG.get_crop`` (base_fst.py:1000-1040; pinned by tests/golden/data_side.npz): the crop of an
    instance with ``offset`` pixels of context on every side.  Context beyond the image border comes from np.pad of
    the WHOLE image at its top/left (pad = the offsets; bottom/right one more when the padded extent is odd), in
    ``mode`` ('reflect' for the image, 'constant' for the mask); with ``crop_square`` the shorter side's offset grows
    until the window is square; without it the padding is constant zeros.  Zero offsets: only the parity padding.
    img [H,W,C] -> (crop, box int32 YXYX of the instance inside the crop)."""
    h, w = ymax - ymin, xmax - xmin
    if h_offset == 0 and w_offset == 0:
        pads = ((0, h % 2), (0, w % 2))
        box = (0, 0, h, w)
    else:
        if crop_square:
            eh, ew = h + 2 * h_offset, w + 2 * w_offset
            eh, ew = eh + eh % 2, ew + ew % 2
            if eh > ew:
                w_offset += (eh - ew) // 2
            elif ew > eh:
                h_offset += (ew - eh) // 2
        else:
            mode = 'constant'
        pads = ((h_offset, h_offset + (h + 2 * h_offset) % 2), (w_offset, w_offset + (w + 2 * w_offset) % 2))
        box = (h_offset, w_offset, h_offset + h, w_offset + w)
    padded = np.pad(img, [list(pads[0]), list(pads[1]), [0, 0]], mode=mode)
    crop = padded[ymin:ymax + sum(pads[0]), xmin:xmax + sum(pads[1])]
    return crop, np.array(box, dtype=np.int32).reshape(4)


def _resize(img: np.ndarray, nh: int, nw: int, binary: bool) -> np.ndarray:
    """imgaug ``Resize`` stand-in (third party, not pinned): bicubic like its default interpolation; a mask is
    resized as float and re-thresholded at 0.5 (imgaug's handling of bool arrays)."""
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(img)).float()
    t = t[None, None] if t.dim() == 2 else t.permute(2, 0, 1)[None]
    t = F.interpolate(t, size=(nh, nw), mode='bicubic', align_corners=False)
    if binary:
        return (t[0, 0] > 0.5).numpy()
    return t[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy()


def support_from_instance(img: np.ndarray, bbox_yxyx, isegmap: np.ndarray, spp_img_size: int,
                          spp_fill_ratio: float = 0.8, crop_square: bool = True):
    """One support sample as ``BaseFewShotISEG.get_support`` builds it (base_fst.py:1104-1155): integer box ->
    offsets ``floor(extent * offset_ratio)`` -> ``get_crop`` (image: reflect context, mask: zeros) ->
    ``iaa.Resize({'longer-side': S, 'shorter-side': 'keep-aspect-ratio'})`` -> ``iaa.CenterPadToFixedSize(S, S,
    pad_mode='constant')`` (base_fst.py:478-482) with the box carried along.  The crop geometry is pinned by the
    reference's golden; the two imgaug operators are third-party and restated (bicubic resize, shorter side =
    round(S * short / long), centre padding with the odd pixel on the bottom / right).
    img [H,W,3] uint8, isegmap [H,W] bool -> (crop [S,S,3] uint8, box float32 YXYX in crop pixels, mask [S,S] bool)."""
    ymin, xmin, ymax, xmax = np.array(bbox_yxyx).astype(np.int32)
    r = spp_offset_ratio(spp_fill_ratio)
    w_off, h_off = int(np.floor((xmax - xmin) * r)), int(np.floor((ymax - ymin) * r))
    crop, box = get_crop(img, ymin, xmin, ymax, xmax, h_off, w_off, crop_square=crop_square)
    mcrop, _ = get_crop(isegmap[:, :, None], ymin, xmin, ymax, xmax, h_off, w_off, crop_square=crop_square,
                        mode='constant')
    ch, cw = crop.shape[:2]
    S = int(spp_img_size)
    if ch >= cw:
        nh, nw = S, max(1, int(np.round(S * cw / ch)))
    else:
        nh, nw = max(1, int(np.round(S * ch / cw))), S
    crop_r, mask_r = _resize(crop, nh, nw, False), _resize(mcrop[:, :, 0], nh, nw, True)
    box_r = box.astype(np.float32) * np.array([nh / ch, nw / cw, nh / ch, nw / cw], np.float32)
    top, left = (S - nh) // 2, (S - nw) // 2
    out = np.zeros((S, S, 3), np.uint8)
    out[top:top + nh, left:left + nw] = crop_r
    m = np.zeros((S, S), bool)
    m[top:top + nh, left:left + nw] = mask_r
    return out, (box_r + np.array([top, left, top, left], np.float32)).astype(np.float32), m


# ---- query resize (BaseFewShotISEG.get_query, base_fst.py:876-887) -------------------------------------------------
# cv2.resize (bilinear) is third party and its uint8 path differs between versions, so the rule is this project's own
# restatement of its design - half-pixel centres, clamped edges, 11-bit weights, round half up - in INTEGERS, so that
# the kernels of csrc/spatial.hip (resize_u8hwc3_to_nhwc4_kernel, resize_mask_u8_kernel) agree with these functions bit
# for bit.  No pin is held by the reference; a float bilinear differs by at most 1 grey level.
RESIZE_MAX_DIM = 16384        # every intermediate of the rule fits int32 up to here; larger dimensions are refused
RESIZE_W_BITS = 11            # weights 0..2048 per axis; acc <= 255 * 2^22


def _check_resize_dims(*dims) -> None:
    for d in dims:
        if not 1 <= int(d) <= RESIZE_MAX_DIM:
            raise ValueError(f'resize: every dimension must be in 1..{RESIZE_MAX_DIM}, got {int(d)}')


def resize_taps(n_src: int, n_dst: int):
    """Taps of one axis: destination sample j blends source samples i0[j], i1[j] with weights w0[j] + w1[j] = 2048.
    num = (2j+1) * n_src - n_dst over den = 2 * n_dst is the source coordinate of j's centre; i0 its floor, w1 the
    fraction rounded half up to 11 bits; left of the first centre the weight is all on sample 0, right of the last
    both taps are the last sample.  -> (i0, i1, w0, w1) int32 [n_dst]."""
    _check_resize_dims(n_src, n_dst)
    n_src, n_dst = int(n_src), int(n_dst)
    j = np.arange(n_dst, dtype=np.int32)
    den = np.int32(2 * n_dst)
    num = (2 * j + 1) * np.int32(n_src) - np.int32(n_dst)
    i0 = num // den                                     # (floor division)
    rem = num - i0 * den
    w1 = (rem * np.int32(1 << (RESIZE_W_BITS + 1)) + den) // (2 * den)
    w1 = np.where(i0 < 0, 0, w1).astype(np.int32)
    i1 = np.minimum(i0 + 1, n_src - 1).astype(np.int32)
    i0 = np.clip(i0, 0, n_src - 1).astype(np.int32)
    return i0, i1, (np.int32(1 << RESIZE_W_BITS) - w1).astype(np.int32), w1


def _resize_acc(planes: np.ndarray, H: int, W: int) -> np.ndarray:
    """planes uint8 [..,h,w] -> the int32 accumulators [..,H,W] of the rule (weights sum to 2^22)."""
    h, w = planes.shape[-2:]
    y0, y1, wy0, wy1 = resize_taps(h, H)
    x0, x1, wx0, wx1 = resize_taps(w, W)
    p = planes.astype(np.int32)
    top, bot = p[..., y0, :], p[..., y1, :]
    wy0, wy1 = wy0[:, None], wy1[:, None]
    return (top[..., x0] * (wy0 * wx0) + top[..., x1] * (wy0 * wx1)
            + bot[..., x0] * (wy1 * wx0) + bot[..., x1] * (wy1 * wx1))


def resize_image_u8(img: np.ndarray, H: int, W: int) -> np.ndarray:
    """uint8 [h,w,3] -> uint8 [H,W,3]: per channel (acc + 2^21) >> 22."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError(f'resize_image_u8: expects a uint8 [h,w,c] image, got {img.dtype} {list(img.shape)}')
    acc = _resize_acc(np.moveaxis(img, 2, 0), H, W)
    half = np.int32(1 << (2 * RESIZE_W_BITS - 1))
    return np.ascontiguousarray(np.moveaxis((acc + half) >> (2 * RESIZE_W_BITS), 0, 2).astype(np.uint8))


def resize_masks(m: np.ndarray, H: int, W: int) -> np.ndarray:
    """bool (or 0 / nonzero) [G,h,w] -> bool [G,H,W]: resized as 0/1 bytes by the same rule, set where acc >= 2^21
    (a half counts as set) - what ``cv2.resize(m.astype(uint8)).astype(bool)`` means."""
    m = np.asarray(m)
    if m.ndim != 3:
        raise ValueError(f'resize_masks: expects [G,h,w], got {list(m.shape)}')
    _check_resize_dims(H, W)
    if m.shape[0] == 0:
        return np.zeros((0, int(H), int(W)), bool)
    return _resize_acc((m != 0).astype(np.uint8), H, W) >= (1 << (2 * RESIZE_W_BITS - 1))


def scale_boxes_yxyx(bboxes_yxyx: np.ndarray, h: int, w: int, H: int, W: int) -> np.ndarray:
    """base_fst.py:877-878 on a copy: rows 0, 2 times H / h and rows 1, 3 times W / w (Python floats), in the boxes'
    own dtype."""
    out = np.array(bboxes_yxyx, copy=True)
    out[:, [0, 2]] = out[:, [0, 2]] * (H / h)
    out[:, [1, 3]] = out[:, [1, 3]] * (W / w)
    return out


def boxes_to_source(boxes: np.ndarray, src_hw, net_hw, order: str = 'yxyx') -> np.ndarray:
    """Boxes in the frame of a ``net_hw`` = (H, W) network in the frame of the ``src_hw`` = (h, w) image they were
    resized from: x coordinates divided by ``float32(W / w)``, y coordinates by ``float32(H / h)`` - mmdet's
    ``bboxes / scale_factor`` with the ``scale_factor`` its ``Resize`` forms, in float32, without clipping.  float32
    [n,4] in, float32 out; ``order``: ``'yxyx'`` (result dicts) or ``'xyxy'`` (detection records).  At equal size the
    same object comes back, like ``resize_query``."""
    if order not in ('yxyx', 'xyxy'):
        raise ValueError(f"boxes_to_source: order must be 'yxyx' or 'xyxy', got {order!r}")
    if not isinstance(boxes, np.ndarray) or boxes.dtype != np.float32 or boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError('boxes_to_source: expects a float32 [n,4] array')
    (h, w), (H, W) = (int(v) for v in src_hw), (int(v) for v in net_hw)
    _check_resize_dims(h, w, H, W)
    if (h, w) == (H, W):
        return boxes
    sy, sx = np.float32(H / h), np.float32(W / w)
    s = np.array([sy, sx, sy, sx] if order == 'yxyx' else [sx, sy, sx, sy], np.float32)
    return boxes / s


def resize_query(img: np.ndarray, bboxes_yxyx: np.ndarray, isegmaps: np.ndarray, H: int, W: int):
    """What ``get_query`` does between the decoded image and the sample (base_fst.py:876-887): image and masks to
    (H, W), boxes scaled.  At equal size everything passes through untouched (the same objects)."""
    h, w = img.shape[:2]
    if int(H) == h and int(W) == w:
        return img, bboxes_yxyx, isegmaps
    return resize_image_u8(img, H, W), scale_boxes_yxyx(bboxes_yxyx, h, w, H, W), resize_masks(isegmaps, H, W)


# ---- query augmentation (BaseFewShotISEG.augment_with_imgaug, base_fst.py:735-770; natural_fst.py:18-35) -----------
# The geometric half of the reference's ``augs_seq`` (Fliplr, Affine rotate / scale / shear / translate_px) and its
# ChannelShuffle, composed with the resize of ``get_query`` into ONE bilinear gather from the source image.  imgaug and
# cv2 are third party and pinned by no golden: like ``resize_taps`` this is the project's own restatement in INTEGERS, so
# that augment_u8hwc3_to_nhwc4_kernel and augment_mask_u8_kernel of csrc/spatial.hip agree with these functions bit for
# bit (which also lists the conventions of imgaug that were taken from memory).
AUG_PARAMS = ('flip', 'rotate', 'scale', 'shear', 'translate_x', 'translate_y', 'border', 'channel_order')
AUG_FRAC_BITS = 20            # coefficients of the source map in units of 2^-20 source pixels
AUG_LIN_MAX = 1 << 26         # |c00|, |c01|, |c10|, |c11| at most this (64 source pixels per output pixel)
AUG_OFF_MAX = 1 << 40         # |c02|, |c12| at most this; then |U| < 2^42 for ox, oy < 16384 and U >> 20 fits int32
AUG_REC_INTS = 16             # int32 per image record
AUG_REC_FIELDS = ('h', 'w', 'kind', 'flip', 'border', 'perm', 'c00', 'c01', 'c10', 'c11', 'c02_lo', 'c02_hi', 'c12_lo',
                  'c12_hi')
CHANNEL_ORDERS = tuple(itertools.permutations(range(3)))      # out[c] = in[CHANNEL_ORDERS[k][c]]; 0 = identity
AUG_NEUTRAL = (0., 0., 1., 0., 0., 0., 0., 0.)


def check_augment_params(params) -> np.ndarray:
    """One image's row ``AUG_PARAMS`` as float64 [8]; ValueError for a wrong shape, a non-finite entry, a scale that is
    not positive, or flip / border / channel order outside {0,1} / {0,1} / 0..5."""
    p = np.asarray(params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else params)
    if p.dtype.kind not in 'iuf' or p.shape != (len(AUG_PARAMS),):
        raise ValueError(f'qry_augment: one image\'s row is {len(AUG_PARAMS)} numbers {AUG_PARAMS}, got '
                         f'{p.dtype} {list(p.shape)}')
    p = p.astype(np.float64)
    if not np.isfinite(p).all():
        raise ValueError(f'qry_augment: non-finite entries in {p.tolist()}')
    if p[0] not in (0., 1.) or p[6] not in (0., 1.) or p[7] not in (0., 1., 2., 3., 4., 5.):
        raise ValueError(f'qry_augment: flip and border are 0 or 1 and the channel order is 0..5, got flip {p[0]}, '
                         f'border {p[6]}, channel order {p[7]}')
    if not p[2] > 0:
        raise ValueError(f'qry_augment: the scale must be positive, got {p[2]}')
    return p


def augment_kind(p: np.ndarray) -> int:
    """0: rotation, shear and translation are 0 and the scale is 1 (the resize's own taps, reversed under flip);
    1: an affine gather."""
    return int(not (p[1] == 0 and p[2] == 1 and p[3] == 0 and p[4] == 0 and p[5] == 0))


def augment_is_neutral(p: np.ndarray) -> bool:
    return augment_kind(p) == 0 and p[0] == 0 and p[7] == 0


def augment_forward_matrix(p: np.ndarray, net_hw) -> np.ndarray:
    """A = T(c) T(t) Rot(rotate) ShearX(shear) Scale(scale) FlipX T(-c), c = (W/2, H/2), float64 [3,3] on (x, y, 1)
    in the network frame (pixel j covers [j, j+1)).  Rot = [[cos, -sin], [sin, cos]] (y points down: positive angles
    turn clockwise on the screen), ShearX = [[1, -tan], [0, 1]], FlipX = diag(-1, 1)."""
    H, W = (float(v) for v in net_hw)
    T = lambda x, y: np.array([[1., 0., x], [0., 1., y], [0., 0., 1.]])
    th, ph = np.deg2rad(p[1]), np.deg2rad(p[3])
    rot = np.array([[np.cos(th), -np.sin(th), 0.], [np.sin(th), np.cos(th), 0.], [0., 0., 1.]])
    shear = np.array([[1., -np.tan(ph), 0.], [0., 1., 0.], [0., 0., 1.]])
    scale = np.diag([p[2], p[2], 1.])
    flip = np.diag([-1. if p[0] else 1., 1., 1.])
    return T(W / 2, H / 2) @ T(p[4], p[5]) @ rot @ shear @ scale @ flip @ T(-W / 2, -H / 2)


def augment_source_matrix(p: np.ndarray, src_hw, net_hw) -> np.ndarray:
    """M = Rz A^-1 P, float64 [2,3]: source sample coordinate (sample j at j) of output pixel (ox, oy) = M (ox, oy, 1).
    P shifts to the pixel's centre, Rz scales by (w / W, h / H) and shifts back by half a source pixel."""
    (h, w), (H, W) = (float(v) for v in src_hw), (float(v) for v in net_hw)
    P = np.array([[1., 0., .5], [0., 1., .5], [0., 0., 1.]])
    Rz = np.array([[w / W, 0., -.5], [0., h / H, -.5], [0., 0., 1.]])
    return (Rz @ np.linalg.inv(augment_forward_matrix(p, net_hw)) @ P)[:2]


def query_augment_record(params, src_hw, net_hw) -> np.ndarray:
    """What the kernels read for one image, int32 [16] (``AUG_REC_FIELDS``): source size, kind, flip, border, channel
    order and, for kind 1, c = rint(M * 2^20) with the two offsets as (low, high) halves of an int64.  ``params`` None:
    the neutral record.  ValueError for parameters outside their sets, sizes outside 1..16384 and coefficients beyond
    ``AUG_LIN_MAX`` / ``AUG_OFF_MAX``."""
    p = check_augment_params(AUG_NEUTRAL if params is None else params)
    (h, w), (H, W) = (int(v) for v in src_hw), (int(v) for v in net_hw)
    _check_resize_dims(h, w, H, W)
    rec = np.zeros(AUG_REC_INTS, np.int32)
    kind = augment_kind(p)
    rec[:6] = (h, w, kind, int(p[0]), int(p[6]), int(p[7]))
    if kind == 1:
        M = augment_source_matrix(p, (h, w), (H, W)) * float(1 << AUG_FRAC_BITS)
        if not np.isfinite(M).all() or np.abs(M[:, :2]).max() > AUG_LIN_MAX or np.abs(M[:, 2]).max() > AUG_OFF_MAX:
            raise ValueError(f'qry_augment: the source map of {p.tolist()} at {(h, w)} -> {(H, W)} exceeds the bounds of '
                             f'the integer rule (|linear| <= 2^6, |offset| <= 2^20 source pixels)')
        c = np.rint(M).astype(np.int64)
        rec[6:10] = (c[0, 0], c[0, 1], c[1, 0], c[1, 1])
        rec[10:14] = np.array([c[0, 2], c[1, 2]], np.int64).view(np.int32)       # (little endian: low, high)
    return rec


def _record_fields(rec) -> dict:
    rec = np.asarray(rec)
    if rec.dtype != np.int32 or rec.shape != (AUG_REC_INTS,):
        raise ValueError(f'an augmentation record is int32 [{AUG_REC_INTS}], got {rec.dtype} {list(rec.shape)}')
    g = dict(zip(AUG_REC_FIELDS[:10], (int(v) for v in rec[:10])))
    g['c02'], g['c12'] = (int(v) for v in np.ascontiguousarray(rec[10:14]).view(np.int64))
    if g['kind'] not in (0, 1) or g['flip'] not in (0, 1) or g['border'] not in (0, 1) or not 0 <= g['perm'] <= 5 or \
            max(abs(g[k]) for k in ('c00', 'c01', 'c10', 'c11')) > AUG_LIN_MAX or \
            max(abs(g['c02']), abs(g['c12'])) > AUG_OFF_MAX:
        raise ValueError(f'augmentation record out of range: {g}')
    return g


def _augment_acc(planes: np.ndarray, g: dict, H: int, W: int, symmetric: bool) -> np.ndarray:
    """planes uint8 [C,h,w] -> the int32 accumulators [C,H,W] of record ``g`` (weights sum to 2^22).  Kind 1 taps that
    leave the image read the symmetric extension (``symmetric``) or 0."""
    C, h, w = planes.shape
    if (h, w) != (g['h'], g['w']):
        raise ValueError(f'the record is for a {(g["h"], g["w"])} source, got {(h, w)}')
    _check_resize_dims(H, W)
    if g['kind'] == 0:
        acc = _resize_acc(planes, H, W)
        return acc[..., ::-1] if g['flip'] else acc
    ox, oy = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    one = 1 << AUG_FRAC_BITS

    def taps(c_x, c_y, c_o, n):
        U = c_x * ox + c_y * oy + c_o
        i0, f = U >> AUG_FRAC_BITS, U & (one - 1)
        w1 = (f + (1 << (AUG_FRAC_BITS - RESIZE_W_BITS - 1))) >> (AUG_FRAC_BITS - RESIZE_W_BITS)
        idx = np.stack([i0, i0 + 1])
        if symmetric:
            r = np.mod(idx, 2 * n)
            idx = np.where(r < n, r, 2 * n - 1 - r)
        else:
            idx = np.where((idx >= 0) & (idx < n), idx, n)                  # n: the zero sample appended below
        return idx, np.stack([(1 << RESIZE_W_BITS) - w1, w1]).astype(np.int32)
    ix, wx = taps(g['c00'], g['c01'], g['c02'], w)
    iy, wy = taps(g['c10'], g['c11'], g['c12'], h)
    ext = np.zeros((C, h + 1, w + 1), np.int32)
    ext[:, :h, :w] = planes
    acc = np.zeros((C, H, W), np.int32)
    for a in range(2):
        for b in range(2):
            wgt = wy[a] * wx[b]
            for c in range(C):                                              # (one plane at a time: masks come by the dozen)
                acc[c] += ext[c][iy[a], ix[b]] * wgt
    return acc


def augment_image_u8(img: np.ndarray, rec: np.ndarray, H: int, W: int) -> np.ndarray:
    """uint8 [h,w,3] -> uint8 [H,W,3] by record ``rec``: per channel (acc + 2^21) >> 22, then out[..., c] =
    in[..., order[c]].  Kind 0 without flip and with the identity order is ``resize_image_u8``."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'augment_image_u8: expects a uint8 [h,w,3] image, got {img.dtype} {list(img.shape)}')
    g = _record_fields(rec)
    acc = _augment_acc(np.moveaxis(img, 2, 0), g, int(H), int(W), bool(g['border']))
    out = np.moveaxis((acc + (1 << (2 * RESIZE_W_BITS - 1))) >> (2 * RESIZE_W_BITS), 0, 2).astype(np.uint8)
    return np.ascontiguousarray(out[..., list(CHANNEL_ORDERS[g['perm']])])


def augment_masks(m: np.ndarray, rec: np.ndarray, H: int, W: int) -> np.ndarray:
    """bool (or 0 / nonzero) [G,h,w] -> bool [G,H,W]: the image's taps on 0/1 values, set where acc >= 2^21; a tap
    outside the image is 0 whatever the record's border.  Kind 0 without flip is ``resize_masks``."""
    m = np.asarray(m)
    if m.ndim != 3:
        raise ValueError(f'augment_masks: expects [G,h,w], got {list(m.shape)}')
    g = _record_fields(rec)
    _check_resize_dims(H, W)
    if m.shape[0] == 0:
        return np.zeros((0, int(H), int(W)), bool)
    return _augment_acc((m != 0).astype(np.uint8), g, int(H), int(W), False) >= (1 << (2 * RESIZE_W_BITS - 1))


def augment_boxes_yxyx(bboxes_yxyx: np.ndarray, params, H: int, W: int):
    """Boxes YXYX in the network frame through A: the four corners in float64, their axis-aligned hull, cast to float32
    -> (boxes float32 [n,4] clipped to the image, True), or (None, False) when a hull lies fully outside the image
    (``bad_augment``, base_fst.py:751-768: the sample is then used un-augmented)."""
    p = check_augment_params(params)
    A = augment_forward_matrix(p, (H, W))
    b = np.asarray(bboxes_yxyx, np.float64).reshape(-1, 4)
    xs, ys = b[:, [1, 3, 1, 3]], b[:, [0, 0, 2, 2]]
    X = A[0, 0] * xs + A[0, 1] * ys + A[0, 2]
    Y = A[1, 0] * xs + A[1, 1] * ys + A[1, 2]
    hull = np.stack([Y.min(1), X.min(1), Y.max(1), X.max(1)], 1).astype(np.float32).reshape(-1, 4)
    out = (hull[:, 3] <= 0) | (hull[:, 1] >= W) | (hull[:, 2] <= 0) | (hull[:, 0] >= H)
    if out.any():
        return None, False
    hull[:, [0, 2]] = hull[:, [0, 2]].clip(0, H)
    hull[:, [1, 3]] = hull[:, [1, 3]].clip(0, W)
    return hull, True


def augment_plan(params, bboxes_yxyx, src_hw, net_hw):
    """Everything of one image's augmentation that is decided before a pixel is touched: -> (record int32 [16], boxes
    at the network size).  A neutral row (or None) and a row whose boxes leave the image (the fallback) give the neutral
    record and the boxes of ``resize_query``; every contract error of the row is raised here."""
    (h, w), (H, W) = (int(v) for v in src_hw), (int(v) for v in net_hw)
    plain = bboxes_yxyx if (h, w) == (H, W) or bboxes_yxyx is None else scale_boxes_yxyx(bboxes_yxyx, h, w, H, W)
    rec = query_augment_record(params, (h, w), (H, W))
    if params is None or augment_is_neutral(check_augment_params(params)):
        return query_augment_record(None, (h, w), (H, W)), plain
    if plain is None:
        return rec, None
    boxes, ok = augment_boxes_yxyx(plain, params, H, W)
    if not ok:
        return query_augment_record(None, (h, w), (H, W)), plain
    return rec, boxes


def augment_query(img: np.ndarray, bboxes_yxyx: np.ndarray, isegmaps: np.ndarray, H: int, W: int, params=None):
    """``get_query`` with ``augment_qry`` between the decoded image and the sample (base_fst.py:876-891): resize and
    augmentation as one gather of image and masks, boxes through the forward matrix.  ``params`` None or neutral, or a
    box that leaves the image: exactly ``resize_query``."""
    h, w = img.shape[:2]
    rec, boxes = augment_plan(params, bboxes_yxyx, (h, w), (H, W))
    if not rec[2:6].any():
        return resize_query(img, bboxes_yxyx, isegmaps, H, W)
    return augment_image_u8(img, rec, H, W), boxes, augment_masks(isegmaps, rec, H, W)


def draw_query_augment(rng) -> np.ndarray:
    """One row of ``AUG_PARAMS`` drawn like the geometric half of ``augs_seq`` and its ChannelShuffle
    (natural_fst.py:18-35): with p = 1/2 one of Fliplr, rotation by 10 degrees (symmetric border), scale uniform in
    [0.8, 1.2], shear uniform in [-10, 10] degrees (symmetric border), translation by integers uniform in [-20, 20] per
    axis; with p = 1/14 (1/2 x one photometric operator of seven) a uniformly drawn channel order.  ``rng``: a numpy
    Generator or RandomState (``random`` and ``uniform`` are used)."""
    p = np.array(AUG_NEUTRAL, np.float64)
    if rng.random() < 0.5:
        op = min(int(rng.random() * 5), 4)
        if op == 0:
            p[0] = 1
        elif op == 1:
            p[1], p[6] = 10, 1
        elif op == 2:
            p[2] = rng.uniform(0.8, 1.2)
        elif op == 3:
            p[3], p[6] = rng.uniform(-10, 10), 1
        else:
            p[4], p[5] = (min(int(rng.random() * 41), 40) - 20 for _ in range(2))
    if rng.random() < 1 / 14:
        p[7] = min(int(rng.random() * 6), 5)
    return p


# ---- photometric query augmentation (the other six operators of ``augs_seq``, natural_fst.py:18-35) ----------------
# AdditiveGaussianNoise, ImpulseNoise, GaussianBlur, AddToHue, AddToSaturation, AddToBrightness as ONE out-of-place pass
# over the SOURCE bytes, ahead of the resize / geometric gather above (in ``augs_seq`` the photometric half acts first).
# Like the rules above this is the project's own restatement in INTEGERS (imgaug is third party, no golden pins its
# bytes), so that photometric_u8hwc3_kernel of csrc/spatial.hip agrees with ``photometric_image_u8`` bit for bit; every
# table that depends on a float (blur weights, noise thresholds) is made here in float64 and travels in the record
# (which derives the fixed-point widths and lists the conventions of imgaug taken from memory).
PHOTO_PARAMS = ('operator', 'amount', 'seed')
PHOTO_OPS = ('none', 'gaussian_noise', 'impulse_noise', 'gaussian_blur', 'hue', 'saturation', 'brightness')
PHOTO_NEUTRAL = (0., 0., 0.)
PHOTO_REC_INTS = 64           # int32 per image record: 8 of header, then the operator's payload
PHOTO_REC_HEADER = ('h', 'w', 'operator', 'seed', 'a0', 'a1', 'rx', 'ry')
PHOTO_PAYLOAD = 8             # noise: 12 thresholds; blur: x weights w[0..16] at 8, y weights w[0..16] at 25
PHOTO_NOISE_K = 12            # the integer noise k lies in -12..12: six sigma at the largest scale
PHOTO_NOISE_SCALE_MAX = 2.0
PHOTO_BLUR_R_MAX = 16
PHOTO_HUE_BITS = 16           # hue in units of 2^-16 sextants; the ramp f of a channel in units of 2^-16
PHOTO_CHROMA_BITS = 7         # value and chroma in units of 2^-7 grey levels: 255 * 2^7 * 2^16 < 2^31
PHOTO_SAT_BITS = 23           # the saturation amount / 255 in units of 2^-23: 255 * 2^23 < 2^31
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11).  ``counter`` [...,4], ``key`` [...,2] (broadcast against each other),
    values in [0, 2^32) -> uint32 [...,4]."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M[0]) * c0, np.uint64(_PHILOX_M[1]) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(_PHILOX_W[0])) & m32, (k1 + np.uint64(_PHILOX_W[1])) & m32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def check_photometric_params(params) -> np.ndarray:
    """One image's row ``PHOTO_PARAMS`` as float64 [3]; ValueError for a wrong shape, a non-finite entry, an operator
    outside 0..6, a seed that is no integer in [0, 2^32) or an amount outside its operator's set: noise scale in (0, 2],
    impulse p in [0, 1], blur sigma >= 0, hue / saturation / brightness in [-255, 255]."""
    p = np.asarray(params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else params)
    if p.dtype.kind not in 'iuf' or p.shape != (len(PHOTO_PARAMS),):
        raise ValueError(f'qry_photometric: one image\'s row is {len(PHOTO_PARAMS)} numbers {PHOTO_PARAMS}, got '
                         f'{p.dtype} {list(p.shape)}')
    p = p.astype(np.float64)
    if not np.isfinite(p).all():
        raise ValueError(f'qry_photometric: non-finite entries in {p.tolist()}')
    op, a, seed = p
    if op not in (0., 1., 2., 3., 4., 5., 6.):
        raise ValueError(f'qry_photometric: the operator is 0..6 {PHOTO_OPS}, got {op}')
    if seed != np.floor(seed) or not 0 <= seed < 2.0 ** 32:
        raise ValueError(f'qry_photometric: the seed is an integer in [0, 2^32), got {seed}')
    ok = {0: True, 1: 0 < a <= PHOTO_NOISE_SCALE_MAX, 2: 0 <= a <= 1, 3: a >= 0}.get(int(op), -255 <= a <= 255)
    if not ok:
        raise ValueError(f'qry_photometric: amount {a} is outside the set of operator {int(op)} ({PHOTO_OPS[int(op)]}): '
                         f'noise scale in (0, {PHOTO_NOISE_SCALE_MAX}], impulse p in [0, 1], blur sigma >= 0, hue / '
                         f'saturation / brightness in [-255, 255]')
    return p


def photometric_is_neutral(p: np.ndarray) -> bool:
    """Operator 0, or an amount of 0 for operators 2 to 6."""
    return p[0] == 0 or (p[0] >= 2 and p[1] == 0)


def noise_thresholds(scale: float) -> np.ndarray:
    """The lower half of the thresholds of the integer noise, int64 [12]: L_j = floor(Phi((j - 12 + 1/2) / scale) *
    2^32) from ``erfc`` (the float64 ``erf`` saturates in the tails); the upper half is 2^32 - L_j by symmetry.  For a
    uniform 32-bit word u, k = #{j : L_j <= u} - 12 + #{j : 2^32 - L_j <= u} is N(0, scale^2) rounded to an integer,
    with the mass beyond +-12.5 on +-12."""
    return np.array([int(math.floor(0.5 * math.erfc(-(j - PHOTO_NOISE_K + 0.5) / (scale * math.sqrt(2.0))) * 2.0 ** 32))
                     for j in range(PHOTO_NOISE_K)], np.int64)


def blur_weights(sigma_axis: float):
    """One axis of the blur: radius r = max(1, ceil(3 sigma)) and the weights w[0..r] of offsets 0..r (symmetric) =
    rint(2048 g_k / sum g), the centre adjusted so that w[0] + 2 sum w[1..r] = 2048 exactly.  ValueError for r > 16."""
    s = float(sigma_axis)
    r = max(1, int(np.ceil(3.0 * s))) if np.isfinite(s) and s > 0 else -1
    if not 1 <= r <= PHOTO_BLUR_R_MAX:
        raise ValueError(f'qry_photometric: a blur of sigma {s} source pixels needs a radius beyond {PHOTO_BLUR_R_MAX}')
    k = np.arange(r + 1, dtype=np.float64)
    with np.errstate(over='ignore', under='ignore'):
        g = np.exp(-(k * k) / (2.0 * s * s))
    w = np.rint(2048.0 * g / (g[0] + 2.0 * g[1:].sum())).astype(np.int64)
    w[0] = 2048 - 2 * int(w[1:].sum())
    return r, w


def query_photometric_record(params, src_hw, net_hw) -> np.ndarray:
    """What photometric_u8hwc3_kernel reads for one image, int32 [64]: the header ``PHOTO_REC_HEADER`` and the
    operator's payload.  ``params`` None or a neutral row: operator 0 (a copy).
      noise:      12 thresholds (``noise_thresholds``) at 8.
      impulse:    (a0, a1) = low and high half of floor(p * 2^32).
      blur:       sigma per axis in SOURCE pixels, sigma * w / W and sigma * h / H; (rx, ry) and w[0..rx] at 8, w[0..ry]
                  at 25 (``blur_weights``).
      hue:        a0 = rint(amount * 3 / 255 * 2^16) mod 6 * 2^16.
      saturation: a0 = rint(amount / 255 * 2^23).        brightness: a0 = rint(amount * 2^7).
    ValueError for a row outside its sets, sizes outside 1..16384 and a blur radius beyond 16."""
    p = check_photometric_params(PHOTO_NEUTRAL if params is None else params)
    (h, w), (H, W) = (int(v) for v in src_hw), (int(v) for v in net_hw)
    _check_resize_dims(h, w, H, W)
    rec = np.zeros(PHOTO_REC_INTS, np.int64)
    rec[:2] = (h, w)
    op, a = int(p[0]), float(p[1])
    if not photometric_is_neutral(p):
        rec[2] = op
        if op in (1, 2):
            rec[3] = int(p[2])
        if op == 1:
            rec[PHOTO_PAYLOAD:PHOTO_PAYLOAD + PHOTO_NOISE_K] = noise_thresholds(a)
        elif op == 2:
            P = int(np.floor(a * 2.0 ** 32))
            rec[4:6] = (P & 0xFFFFFFFF, P >> 32)
        elif op == 3:
            (rx, wx), (ry, wy) = blur_weights(a * w / W), blur_weights(a * h / H)
            rec[6:8] = (rx, ry)
            rec[PHOTO_PAYLOAD:PHOTO_PAYLOAD + rx + 1] = wx
            rec[PHOTO_PAYLOAD + PHOTO_BLUR_R_MAX + 1:PHOTO_PAYLOAD + PHOTO_BLUR_R_MAX + 2 + ry] = wy
        elif op == 4:
            rec[4] = int(np.rint(a * 3.0 / 255.0 * (1 << PHOTO_HUE_BITS))) % (6 << PHOTO_HUE_BITS)
        elif op == 5:
            rec[4] = int(np.rint(a / 255.0 * (1 << PHOTO_SAT_BITS)))
        else:
            rec[4] = int(np.rint(a * (1 << PHOTO_CHROMA_BITS)))
    return (rec & 0xFFFFFFFF).astype(np.uint32).view(np.int32)            # (seed and thresholds: the low 32 bits as they are)


def _photo_fields(rec) -> dict:
    """The fields of a record, checked as the kernel checks them; ValueError where the kernel writes zeros."""
    rec = np.asarray(rec)
    if rec.dtype != np.int32 or rec.shape != (PHOTO_REC_INTS,):
        raise ValueError(f'a photometric record is int32 [{PHOTO_REC_INTS}], got {rec.dtype} {list(rec.shape)}')
    g = dict(zip(PHOTO_REC_HEADER, (int(v) for v in rec[:8])))
    g['seed'] &= 0xFFFFFFFF
    op, a0, a1 = g['operator'], g['a0'], g['a1']
    ok = 1 <= g['h'] <= RESIZE_MAX_DIM and 1 <= g['w'] <= RESIZE_MAX_DIM and 0 <= op <= 6
    if ok and op == 1:
        g['thresholds'] = rec[PHOTO_PAYLOAD:PHOTO_PAYLOAD + PHOTO_NOISE_K].view(np.uint32).astype(np.int64)
    elif ok and op == 2:
        ok = a1 == 0 or (a1 == 1 and a0 == 0)
        g['P'] = (a1 << 32) | (a0 & 0xFFFFFFFF)
    elif ok and op == 3:
        ok = 1 <= g['rx'] <= PHOTO_BLUR_R_MAX and 1 <= g['ry'] <= PHOTO_BLUR_R_MAX
        if ok:
            g['wx'] = rec[PHOTO_PAYLOAD:PHOTO_PAYLOAD + g['rx'] + 1].astype(np.int64)
            y0 = PHOTO_PAYLOAD + PHOTO_BLUR_R_MAX + 1
            g['wy'] = rec[y0:y0 + g['ry'] + 1].astype(np.int64)
            ok = all(wt.min() >= 0 and wt.max() <= 2048 and wt[0] + 2 * wt[1:].sum() == 2048 for wt in (g['wx'], g['wy']))
    elif ok and op == 4:
        ok = 0 <= a0 < (6 << PHOTO_HUE_BITS)
    elif ok and op == 5:
        ok = abs(a0) <= (1 << PHOTO_SAT_BITS)
    elif ok and op == 6:
        ok = abs(a0) <= (255 << PHOTO_CHROMA_BITS)
    if not ok:
        raise ValueError(f'photometric record out of range: {g}')
    return g


def reflect101(k: np.ndarray, n: int) -> np.ndarray:
    """Indices k (any integers) into an axis of n samples under reflect-101 (the edge sample is not repeated): r = k mod
    (2n - 2), r < n ? r : 2n - 2 - r; always 0 for n = 1."""
    k = np.asarray(k, np.int64)
    if n == 1:
        return np.zeros_like(k)
    r = np.mod(k, 2 * n - 2)
    return np.where(r < n, r, 2 * n - 2 - r)


def _photo_hsv(img: np.ndarray, op: int, a0: int) -> np.ndarray:
    """Hue, saturation and brightness of the record in integers.  V = max, d = V - min; the hue H in units of 2^-16
    sextants from one rounded non-negative division by d; value V7 and chroma C7 in units of 2^-7 grey levels; channel n
    of (5, 3, 1) for (R, G, B) = (V7 * 2^16 - C7 * f + 2^22) >> 23 with the ramp f = clip(min(k, 4 - k), 0, 1) of
    k = (n + H) mod 6 in units of 2^-16."""
    one, six = 1 << PHOTO_HUE_BITS, 6 << PHOTO_HUE_BITS
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    V = np.maximum(np.maximum(r, g), b)
    d = V - np.minimum(np.minimum(r, g), b)
    is_r = V == r
    is_g = ~is_r & (V == g)
    num = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
    q = (2 * np.abs(num) * one + d) // np.maximum(2 * d, 1)
    Hh = np.where(is_r, 0, np.where(is_g, 2, 4)) * one + np.where(num >= 0, q, -q)
    Hh = np.where(d == 0, 0, np.where(Hh < 0, Hh + six, Hh))
    V7, C7 = V << PHOTO_CHROMA_BITS, d << PHOTO_CHROMA_BITS
    if op == 4:
        Hh = Hh + a0
        Hh = np.where(Hh >= six, Hh - six, Hh)
    elif op == 5:
        t = (V * abs(a0) + (1 << (PHOTO_SAT_BITS - PHOTO_CHROMA_BITS - 1))) >> (PHOTO_SAT_BITS - PHOTO_CHROMA_BITS)
        C7 = np.clip(C7 + (t if a0 >= 0 else -t), 0, V7)
    else:
        V7 = np.clip(V7 + a0, 0, 255 << PHOTO_CHROMA_BITS)
        C7 = (2 * V7 * d + V) // np.maximum(2 * V, 1)
    out = np.empty(img.shape, np.uint8)
    for c, n in enumerate((5, 3, 1)):
        k = n * one + Hh
        k = np.where(k >= six, k - six, k)
        f = np.clip(np.minimum(k, 4 * one - k), 0, one)
        out[..., c] = (V7 * one - C7 * f + (1 << (PHOTO_HUE_BITS + PHOTO_CHROMA_BITS - 1))) >> \
            (PHOTO_HUE_BITS + PHOTO_CHROMA_BITS)
    return out


def photometric_image_u8(img: np.ndarray, rec: np.ndarray) -> np.ndarray:
    """uint8 [h,w,3] -> uint8 [h,w,3] by record ``rec`` (``query_photometric_record``); the image is not changed.
      noise:   Philox4x32-10 at counter (y * w + x, 0, 0, operator), key (seed, 0); k from word 0 and the thresholds, the
               same k on the three channels, byte = clip(byte + k, 0, 255).
      impulse: channel c is replaced where word c < floor(p * 2^32), by 255 where bit c of word 3 is set, else by 0.
      blur:    (sum over the window of byte * wy * wx + 2^21) >> 22 with reflect-101 borders.
      hue, saturation, brightness: ``_photo_hsv``."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'photometric_image_u8: expects a uint8 [h,w,3] image, got {img.dtype} {list(img.shape)}')
    g = _photo_fields(rec)
    h, w = img.shape[:2]
    if (h, w) != (g['h'], g['w']):
        raise ValueError(f'the record is for a {(g["h"], g["w"])} source, got {(h, w)}')
    op = g['operator']
    if op == 0:
        return img.copy()
    if op in (1, 2):
        ctr = np.zeros((h * w, 4), np.uint64)
        ctr[:, 0], ctr[:, 3] = np.arange(h * w), op
        words = philox4x32(ctr, (g['seed'], 0)).astype(np.int64).reshape(h, w, 4)
        if op == 1:
            u, L = words[..., 0, None], g['thresholds']
            k = (L <= u).sum(-1) - PHOTO_NOISE_K + (0xFFFFFFFF - u < L).sum(-1)
            return np.clip(img.astype(np.int64) + k[..., None], 0, 255).astype(np.uint8)
        hit = words[..., :3] < g['P']
        val = np.where((words[..., 3, None] >> np.arange(3)) & 1, 255, 0)
        return np.where(hit, val, img).astype(np.uint8)
    if op == 3:
        rx, ry, wx, wy = g['rx'], g['ry'], g['wx'], g['wy']
        ix, iy = reflect101(np.arange(-rx, w + rx), w), reflect101(np.arange(-ry, h + ry), h)
        p = img.astype(np.int64)
        hor = sum(p[:, ix[rx + k:rx + k + w]] * wx[abs(k)] for k in range(-rx, rx + 1))
        acc = sum(hor[iy[ry + k:ry + k + h]] * wy[abs(k)] for k in range(-ry, ry + 1))
        return ((acc + (1 << (2 * RESIZE_W_BITS - 1))) >> (2 * RESIZE_W_BITS)).astype(np.uint8)
    return _photo_hsv(img, op, g['a0'])


def augment_query_full(img: np.ndarray, bboxes_yxyx: np.ndarray, isegmaps: np.ndarray, H: int, W: int, params=None,
                       photometric=None):
    """``augment_query`` behind the photometric pass - ``augs_seq`` in the reference's order, photometric half first:
    ``photometric_image_u8`` on the SOURCE image (its blur's sigma is given in network pixels), then resize and geometry
    as one gather.  A sample whose boxes leave the image is used un-augmented in BOTH halves (``bad_augment``,
    base_fst.py:751-768)."""
    h, w = img.shape[:2]
    rec, _ = augment_plan(params, bboxes_yxyx, (h, w), (H, W))
    fell_back = params is not None and not augment_is_neutral(check_augment_params(params)) and not rec[2:6].any()
    prec = query_photometric_record(photometric, (h, w), (H, W))            # (its contract errors, fallback or not)
    if not fell_back and prec[2] != 0:
        img = photometric_image_u8(img, prec)
    return augment_query(img, bboxes_yxyx, isegmaps, H, W, params)


def draw_query_augment_full(rng):
    """(row of ``AUG_PARAMS``, row of ``PHOTO_PARAMS``) drawn like the whole ``augs_seq`` (natural_fst.py:18-35): the
    geometric half as ``draw_query_augment`` draws it; with p = 1/2 one photometric operator of seven - noise of scale 1,
    impulse noise with p uniform in [0, 0.03], blur with sigma uniform in [0, 3], hue uniform in [-50, 50], saturation
    uniform in [-75, 75], brightness uniform in [-30, 30], or a uniformly drawn channel order, which goes into the first
    row.  Never both a channel order and an operator of the second row."""
    p = draw_query_augment(rng)
    p[7] = 0                                        # (the channel order is one of the seven operators below)
    q = np.array(PHOTO_NEUTRAL, np.float64)
    if rng.random() < 0.5:
        op = min(int(rng.random() * 7), 6)
        if op == 6:
            p[7] = min(int(rng.random() * 6), 5)
        else:
            lo, hi = ((1., 1.), (0., 0.03), (0., 3.), (-50., 50.), (-75., 75.), (-30., 30.))[op]
            q[0] = op + 1
            q[1] = lo if lo == hi else rng.uniform(lo, hi)
            q[2] = min(int(rng.random() * 2.0 ** 32), 2 ** 32 - 1)
    return p, q


# ---- chains of photometric operators (COCODS.augs_seq, coco_ds.py:45-59) --------------------------------------------
# ``COCOFewShotISEG`` assigns ``augs_qry = augs_spp = COCODS.augs_seq`` (coco_fst.py:16-17): HorizontalFlip(0.5), then
# one of AddToHue / AddToSaturation / AddToBrightness, then GaussianBlur - two photometric operators per image, one
# behind the other.  A chain is up to ``PHOTO_CHAIN_MAX`` rows of ``PHOTO_PARAMS`` applied in order, of the form "point
# operators, then at most one blur".  No arithmetic is restated: the rule is the left fold of ``photometric_image_u8``
# over the chain's records, and photometric_chain_u8hwc3_kernel of csrc/spatial.hip agrees with that fold bit for bit in
# one read and one write of the image.
PHOTO_CHAIN_MAX = 3
PHOTO_BLUR_OP = PHOTO_OPS.index('gaussian_blur')


def check_photometric_chain(rows, name: str = 'qry_photometric_chain') -> np.ndarray:
    """One image's chain as float64 [P,3], P in 1..``PHOTO_CHAIN_MAX``: every row through ``check_photometric_params``,
    and the one structural rule - the blur (operator 3) appears at most once and every row behind it is neutral (point
    operators, then at most one blur).  ValueError otherwise; ``name`` is the argument the message speaks of."""
    c = np.asarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows)
    if c.dtype.kind not in 'iuf' or c.ndim != 2 or c.shape[1] != len(PHOTO_PARAMS) or \
            not 1 <= c.shape[0] <= PHOTO_CHAIN_MAX:
        raise ValueError(f'{name}: one image\'s chain is [P,{len(PHOTO_PARAMS)}] numbers {PHOTO_PARAMS} with P in 1..'
                         f'{PHOTO_CHAIN_MAX}, got {c.dtype} {list(c.shape)}')
    try:
        c = np.stack([check_photometric_params(r) for r in c])
    except ValueError as e:
        raise ValueError(str(e).replace('qry_photometric', name)) from None
    blurs = [i for i, r in enumerate(c) if r[0] == PHOTO_BLUR_OP]           # (a blur row of sigma 0 counts: it is a blur)
    if len(blurs) > 1 or (blurs and not all(photometric_is_neutral(r) for r in c[blurs[0] + 1:])):
        raise ValueError(f'{name}: a chain is point operators, then at most one blur - the blur (operator '
                         f'{PHOTO_BLUR_OP}) appears at most once and every row behind it is neutral, got operators '
                         f'{[int(r[0]) for r in c]}')
    return c


def photometric_chain_records(rows, src_hw, net_hw, name: str = 'qry_photometric_chain') -> np.ndarray:
    """What photometric_chain_u8hwc3_kernel reads for one image, int32 [``PHOTO_CHAIN_MAX``, 64]: the non-neutral rows of
    the chain compacted to the front, each as its ``query_photometric_record``, the rest the neutral record of the same
    (h, w).  ``rows`` None: all neutral."""
    neutral = query_photometric_record(None, src_hw, net_hw)
    recs = np.tile(neutral, (PHOTO_CHAIN_MAX, 1))
    if rows is None:
        return recs
    try:
        active = [query_photometric_record(r, src_hw, net_hw) for r in check_photometric_chain(rows, name)
                  if not photometric_is_neutral(r)]
    except ValueError as e:
        raise ValueError(str(e).replace('qry_photometric:', f'{name}:')) from None
    for i, rec in enumerate(active):
        recs[i] = rec
    return recs


def _check_chain_records(recs) -> np.ndarray:
    """Records int32 [P,64], P in 1..3, checked as the kernel checks a chain: one (h, w), a blur only with operator-0
    records behind it (each record's own fields are checked by ``photometric_image_u8``)."""
    recs = np.asarray(recs)
    if recs.dtype != np.int32 or recs.ndim != 2 or recs.shape[1] != PHOTO_REC_INTS or \
            not 1 <= recs.shape[0] <= PHOTO_CHAIN_MAX:
        raise ValueError(f'a photometric chain is int32 [P,{PHOTO_REC_INTS}] records with P in 1..{PHOTO_CHAIN_MAX}, got '
                         f'{recs.dtype} {list(recs.shape)}')
    if (recs[:, :2] != recs[0, :2]).any():
        raise ValueError(f'the records of a chain carry one (h, w), got {recs[:, :2].tolist()}')
    ops_ = recs[:, 2].tolist()
    if PHOTO_BLUR_OP in ops_ and any(ops_[ops_.index(PHOTO_BLUR_OP) + 1:]):
        raise ValueError(f'a blur record has only operator-0 records behind it, got operators {ops_}')
    return recs


def photometric_chain_u8(img: np.ndarray, recs: np.ndarray) -> np.ndarray:
    """uint8 [h,w,3] -> uint8 [h,w,3]: the left fold of ``photometric_image_u8`` over the records int32 [P,64]
    (``photometric_chain_records``).  The rule of photometric_chain_u8hwc3_kernel; the image is not changed."""
    recs = _check_chain_records(recs)
    for g in recs:
        _photo_fields(g)                                # (every record before any pixel, as the kernel does)
    out = np.asarray(img)
    for rec in recs:
        out = photometric_image_u8(out, rec)
    return out


def augment_query_chain(img: np.ndarray, bboxes_yxyx: np.ndarray, isegmaps: np.ndarray, H: int, W: int, params=None,
                        chain=None):
    """``augment_query_full`` with a chain of photometric rows [P,3] in place of the single row: the fold
    ``photometric_chain_u8`` on the SOURCE image (a blur's sigma is given in network pixels), then resize and geometry as
    one gather.  A sample whose boxes leave the image is used un-augmented in BOTH halves."""
    h, w = img.shape[:2]
    rec, _ = augment_plan(params, bboxes_yxyx, (h, w), (H, W))
    fell_back = params is not None and not augment_is_neutral(check_augment_params(params)) and not rec[2:6].any()
    precs = photometric_chain_records(chain, (h, w), (H, W))                # (its contract errors, fallback or not)
    if not fell_back and precs[:, 2].any():
        img = photometric_chain_u8(img, precs)
    return augment_query(img, bboxes_yxyx, isegmaps, H, W, params)


def draw_coco_augment(rng):
    """(row of ``AUG_PARAMS`` [8], chain of ``PHOTO_PARAMS`` [2,3]) drawn like ``COCODS.augs_seq`` (coco_ds.py:45-59):
    HorizontalFlip with p = 1/2 and no other geometric operator; one of hue uniform in [-10, 10], saturation uniform in
    [-25, 25], brightness uniform in [-30, 30] with equal weights; then a blur with sigma uniform in [0, 1.5].  Never a
    noise operator, so the seeds stay 0.  ``rng``: a numpy Generator or RandomState (``random`` and ``uniform``)."""
    p = np.array(AUG_NEUTRAL, np.float64)
    if rng.random() < 0.5:
        p[0] = 1
    chain = np.zeros((2, len(PHOTO_PARAMS)), np.float64)
    op = min(int(rng.random() * 3), 2)
    lo, hi = ((-10., 10.), (-25., 25.), (-30., 30.))[op]
    chain[0, :2] = (PHOTO_OPS.index('hue') + op, rng.uniform(lo, hi))
    chain[1, :2] = (PHOTO_BLUR_OP, rng.uniform(0., 1.5))
    return p, chain


# ---- supports from the source image (BaseFewShotISEG.get_support, base_fst.py:1043-1167) ---------------------------
# ``support_from_instance`` as ONE gather from the source image: crop (reflect context), bicubic resize of the longer
# side to S and centre pad, with no padded copy of the image and no float.  The crop geometry is the golden-pinned
# ``get_crop`` arithmetic; the resize is, like the query's, this project's own restatement in INTEGERS (imgaug's bicubic
# is third party and pinned by no golden) so that support_from_source_kernel of csrc/spatial.hip agrees with
# ``support_from_source`` bit for bit.  Against the float ``_resize`` of ``support_from_instance`` the
# image bytes differ by at most 1 grey level and the masks agree (tests/test_spp_source_cpu.py).
CUBIC_T_BITS = 10             # the fraction t = u / 1024
CUBIC_W_BITS = 11             # weights in units of 1/2048 per axis, sum 2048, sum of magnitudes <= CUBIC_ABS_SUM
CUBIC_ABS_SUM = 2816          # 2048 * 1.375 (t = 1/2 gives 1.25; rounding stays below): |acc| <= 255 * 2816^2 < 2^31
SPP_REC_INTS = 16             # int32 per instance record
SPP_REC_FIELDS = ('H', 'W', 'y0', 'x0', 'ch', 'cw', 'nh', 'nw', 'top', 'left', 'reflect', 'wy', 'wx', 'wh', 'ww')


def cubic_taps(n_src: int, n_dst: int):
    """Taps of one axis of the bicubic rule (cubic convolution, A = -3/4, half-pixel centres): destination sample j
    blends source samples idx[j, 0..3] = i0-1 .. i0+2, clamped into the axis, with integer weights W[j, 0..3] that sum
    to 2048.  num = (2j+1) * n_src - n_dst over den = 2 * n_dst is the source coordinate of j's centre, i0 its floor,
    u the fraction rounded half up to 10 bits, v = 1024 - u; in units of 2^-32 (int64)
        w(-1) = -3 u v^2, w(0) = 5 u^3 - 9216 u^2 + 2^32, w(+1) = 5 v^3 - 9216 v^2 + 2^32, w(+2) = -3 u^2 v,
    each but w(0) rounded to 11 bits by a floor shift, W(0) = 2048 - the other three.  At equal size the rule is the
    identity.  -> (idx int32 [n_dst,4], W int32 [n_dst,4])."""
    _check_resize_dims(n_src, n_dst)
    n_src, n_dst = int(n_src), int(n_dst)
    j = np.arange(n_dst, dtype=np.int64)
    den = 2 * n_dst
    num = (2 * j + 1) * n_src - n_dst
    i0 = num // den                                     # (floor division)
    rem = num - i0 * den
    u = (rem * (2 << CUBIC_T_BITS) + den) // (2 * den)
    v = (1 << CUBIC_T_BITS) - u
    one = np.int64(1) << 32
    w_m1, w_p2 = -3 * u * v * v, -3 * u * u * v
    w_p1 = 5 * v * v * v - 9216 * v * v + one
    half, sh = np.int64(1) << (31 - CUBIC_W_BITS), 32 - CUBIC_W_BITS
    W_m1, W_p1, W_p2 = (w_m1 + half) >> sh, (w_p1 + half) >> sh, (w_p2 + half) >> sh
    W = np.stack([W_m1, (1 << CUBIC_W_BITS) - W_m1 - W_p1 - W_p2, W_p1, W_p2], 1).astype(np.int32)
    idx = np.clip(i0[:, None] + np.arange(-1, 3), 0, n_src - 1).astype(np.int32)
    return idx, W


def reflect_index(t: np.ndarray, n: int) -> np.ndarray:
    """Index into an axis of n samples of position t of its ``np.pad(mode='reflect')`` extension, for any t: the
    periodic reflection of period 2 (n - 1); always 0 for n = 1 (numpy extends a single sample by its edge)."""
    t = np.asarray(t, np.int64)
    if n == 1:
        return np.zeros_like(t)
    p = 2 * (n - 1)
    m = np.mod(t, p)
    return np.where(m < n, m, p - m)


def support_geometry(H: int, W: int, bbox_yxyx, S: int, spp_fill_ratio: float = 0.8, crop_square: bool = True):
    """Everything ``support_from_instance`` decides before it touches a pixel, for an instance ``bbox_yxyx`` of an
    [H,W] image: -> (int32 record, float32 box YXYX in the S x S support, bit-equal to ``support_from_instance``'s).
    The record (``SPP_REC_FIELDS``, padded to ``SPP_REC_INTS``): the source size; the crop's origin (y0, x0) in the
    source frame (negative where the context leaves the image) and its size (ch, cw), parity pixel included; the
    resized size (nh, nw) and its place (top, left) in the support; ``reflect`` = 1 where ``get_crop`` pads by
    reflection, 0 where by zeros (``crop_square=False`` with a non-zero offset); the WINDOW (wy, wx, wh, ww) = the
    bounding rows and columns of the source that the crop reads after reflection - all of the image and of the mask
    that ``support_from_source`` needs.  A box that is empty (after truncation to integers) or leaves its image raises
    ValueError, as does a size outside 1..16384."""
    H, W, S = int(H), int(W), int(S)
    _check_resize_dims(H, W, S)
    ymin, xmin, ymax, xmax = np.array(bbox_yxyx).astype(np.int32).reshape(4)
    if not (0 <= ymin < ymax <= H and 0 <= xmin < xmax <= W):
        raise ValueError(f'support box {[int(v) for v in (ymin, xmin, ymax, xmax)]} (YXYX) is empty or outside its '
                         f'{H}x{W} image')
    r = spp_offset_ratio(spp_fill_ratio)
    w_off, h_off = int(np.floor((xmax - xmin) * r)), int(np.floor((ymax - ymin) * r))
    # get_crop's arithmetic, without the pixels
    h, w = ymax - ymin, xmax - xmin
    reflect = True
    if h_off == 0 and w_off == 0:
        pads = ((0, int(h % 2)), (0, int(w % 2)))
        box = (0, 0, h, w)
    else:
        if crop_square:
            eh, ew = h + 2 * h_off, w + 2 * w_off
            eh, ew = eh + eh % 2, ew + ew % 2
            if eh > ew:
                w_off += (eh - ew) // 2
            elif ew > eh:
                h_off += (ew - eh) // 2
        else:
            reflect = False
        pads = ((h_off, h_off + (h + 2 * h_off) % 2), (w_off, w_off + (w + 2 * w_off) % 2))
        box = (h_off, w_off, h_off + h, w_off + w)
    box = np.array(box, dtype=np.int32).reshape(4)
    y0, x0 = int(ymin) - int(pads[0][0]), int(xmin) - int(pads[1][0])
    ch, cw = int(h) + int(sum(pads[0])), int(w) + int(sum(pads[1]))
    _check_resize_dims(ch, cw)
    if ch >= cw:
        nh, nw = S, max(1, int(np.round(S * cw / ch)))
    else:
        nh, nw = max(1, int(np.round(S * ch / cw))), S
    box_r = box.astype(np.float32) * np.array([nh / ch, nw / cw, nh / ch, nw / cw], np.float32)
    top, left = (S - nh) // 2, (S - nw) // 2
    box_out = (box_r + np.array([top, left, top, left], np.float32)).astype(np.float32)

    def window(o, c, n):
        t = o + np.arange(c, dtype=np.int64)
        t = reflect_index(t, n) if reflect else t[(t >= 0) & (t < n)]
        return int(t.min()), int(t.max()) - int(t.min()) + 1
    (wy, wh), (wx, ww) = window(y0, ch, H), window(x0, cw, W)
    rec = np.zeros(SPP_REC_INTS, np.int32)
    rec[:len(SPP_REC_FIELDS)] = (H, W, y0, x0, ch, cw, nh, nw, top, left, int(reflect), wy, wx, wh, ww)
    return rec, box_out


def _spp_axis(o: int, n_crop: int, n_dst: int, n_src: int, reflect: bool, w_lo: int, w_len: int):
    """Taps of one axis of ``support_from_source``: crop-frame taps (``cubic_taps``) + the crop's origin ``o``, mapped
    into the source axis of ``n_src`` samples and expressed in the window [w_lo, w_lo + w_len); a tap that reads
    nothing (zero mode, outside the image) gets index ``w_len`` - the zero sample the callers append.
    -> (index into the window for the image, the same for the mask, weights)."""
    idx, wts = cubic_taps(n_crop, n_dst)
    t = idx.astype(np.int64) + o
    inside = (t >= 0) & (t < n_src)
    refl = reflect_index(t, n_src) - w_lo
    raw = np.where(inside, t - w_lo, w_len)
    if ((refl < 0) | (refl >= w_len)).any() if reflect else ((raw < 0) | (raw > w_len)).any():
        raise ValueError('support_from_source: a tap leaves the window of support_geometry')
    return (refl if reflect else raw), raw, wts.astype(np.int64)


def _spp_gather(win: np.ndarray, iy, ix, wy, wx) -> np.ndarray:
    """win [wh,ww,c] bytes -> int64 accumulators [nh,nw,c] = sum_a sum_b win[iy[:,a], ix[:,b]] * wy[:,a] * wx[:,b]; index
    wh / ww reads 0."""
    ext = np.zeros((win.shape[0] + 1, win.shape[1] + 1, win.shape[2]), np.int64)
    ext[:-1, :-1] = win
    cols = sum(ext[:, ix[:, b], :] * wx[None, :, b, None] for b in range(4))          # [wh+1,nw,c]
    return sum(cols[iy[:, a]] * wy[:, a, None, None] for a in range(4))


def support_from_source(img: np.ndarray, bbox_yxyx, isegmap: np.ndarray, spp_img_size: int,
                        spp_fill_ratio: float = 0.8, crop_square: bool = True, geometry=None):
    """``support_from_instance`` by the integer rule, as one gather from the window of ``support_geometry``: per output
    pixel inside the resized crop the 4 x 4 taps of ``cubic_taps`` in the crop frame, moved by the crop's origin and
    mapped into the source (``reflect_index``, or a zero outside the image in zero mode; the mask is always zero
    outside); image byte = clamp((acc + 2^21) >> 22, 0, 255), mask set where acc > 2^21 (strictly: ``_resize`` thresholds
    > 0.5); zeros in the padding.  img [H,W,3] uint8, isegmap [H,W] bool (or 0 / nonzero) ->
    (crop [S,S,3] uint8, box float32 YXYX, mask [S,S] bool).  ``geometry``: the (record, box) of ``support_geometry``
    when the caller has it already."""
    img, isegmap = np.asarray(img), np.asarray(isegmap)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'support_from_source: expects a uint8 [H,W,3] image, got {img.dtype} {list(img.shape)}')
    if isegmap.shape != img.shape[:2]:
        raise ValueError(f'support_from_source: the mask {list(isegmap.shape)} is not at its image\'s size '
                         f'{list(img.shape[:2])}')
    S = int(spp_img_size)
    rec, box = geometry if geometry is not None else \
        support_geometry(img.shape[0], img.shape[1], bbox_yxyx, S, spp_fill_ratio, crop_square)
    g = dict(zip(SPP_REC_FIELDS, (int(v) for v in rec)))
    iy, my, wy = _spp_axis(g['y0'], g['ch'], g['nh'], g['H'], bool(g['reflect']), g['wy'], g['wh'])
    ix, mx, wx = _spp_axis(g['x0'], g['cw'], g['nw'], g['W'], bool(g['reflect']), g['wx'], g['ww'])
    ys, xs = slice(g['wy'], g['wy'] + g['wh']), slice(g['wx'], g['wx'] + g['ww'])
    half, sh = 1 << (2 * CUBIC_W_BITS - 1), 2 * CUBIC_W_BITS
    acc = _spp_gather(img[ys, xs], iy, ix, wy, wx)
    macc = _spp_gather((isegmap[ys, xs] != 0).astype(np.uint8)[:, :, None], my, mx, wy, wx)[:, :, 0]
    assert np.abs(acc).max(initial=0) <= 255 * CUBIC_ABS_SUM ** 2
    out = np.zeros((S, S, 3), np.uint8)
    m = np.zeros((S, S), bool)
    rows, cols = slice(g['top'], g['top'] + g['nh']), slice(g['left'], g['left'] + g['nw'])
    out[rows, cols] = np.clip((acc + half) >> sh, 0, 255).astype(np.uint8)
    m[rows, cols] = macc > half
    return out, box, m


def support_window(img: np.ndarray, isegmap: np.ndarray, rec: np.ndarray):
    """The bytes of one instance that travel to the device: (image window [wh,ww,3] uint8, mask window [wh,ww] uint8
    0/1), contiguous.  (A bool mask is copied as it is stored, 0 / 1 bytes, without a comparison.)"""
    g = dict(zip(SPP_REC_FIELDS, (int(v) for v in rec)))
    ys, xs = slice(g['wy'], g['wy'] + g['wh']), slice(g['wx'], g['wx'] + g['ww'])
    m = isegmap[ys, xs]
    m = np.ascontiguousarray(m) if m.dtype == np.bool_ else np.ascontiguousarray(m != 0)
    return np.ascontiguousarray(img[ys, xs]), m.view(np.uint8)


# ---- support augmentation (BaseFewShotISEG.get_support with augment_spp, base_fst.py:1151-1153) --------------------
# ``augment_with_imgaug(self.augs_spp, img_crop_pad, box_crop_pad, isegmap_crop_pad)`` once per instance, on the S x S
# crop AFTER resize and pad, with one mask and one box.  The few-shot dataset classes assign ``augs_spp = augs_seq``, the
# queries' sequence, so the rule is the queries' by composition, at equal size: nothing new is restated here
# (DESIGN.md 4.4.7).  Unlike the queries the supports see the operators in the reference's own place, after the resize.
def augment_support(crop: np.ndarray, box, mask: np.ndarray, params=None, photometric=None, photometric_chain=None):
    """One support instance of ``support_from_source`` (crop uint8 [S,S,3], box float32 YXYX in the S x S frame, mask
    [S,S]) through one row pair (``AUG_PARAMS``, ``PHOTO_PARAMS``): ``augment_query_full`` at equal size with one box
    and one mask - ``photometric_image_u8`` (the blur's sigma in crop pixels), the gather of ``query_augment_record``
    whose symmetric border reflects the S x S frame, pad bands included, and the box through ``augment_boxes_yxyx``.  A
    box that leaves the open S x S rectangle: the instance is used un-augmented in both halves.
    ``photometric_chain`` (in place of ``photometric``, never beside it): a chain [P,3] of rows, folded by
    ``augment_query_chain`` in the same place.
    -> (crop', box' [4], mask' [S,S])."""
    crop, mask = np.asarray(crop), np.asarray(mask)
    if crop.ndim != 3 or crop.shape[0] != crop.shape[1] or mask.shape != crop.shape[:2]:
        raise ValueError(f'augment_support: expects a crop [S,S,3] and its mask [S,S], got {list(crop.shape)} and '
                         f'{list(mask.shape)}')
    S = crop.shape[0]
    box = np.asarray(box).reshape(1, 4)
    if photometric_chain is not None:
        if photometric is not None:
            raise ValueError('augment_support: give photometric or photometric_chain, not both')
        img, boxes, masks = augment_query_chain(crop, box, mask[None], S, S, params, photometric_chain)
        return img, boxes[0], masks[0]
    img, boxes, masks = augment_query_full(crop, box, mask[None], S, S, params, photometric)
    return img, boxes[0], masks[0]


def support_augment_plan(rows, photo_rows, boxes, S: int):
    """Everything of the augmentation of n support instances that is decided before a pixel is touched.  ``rows``
    [n,8] rows of ``AUG_PARAMS`` and ``photo_rows`` [n,3] rows of ``PHOTO_PARAMS`` (either may be None: neutral),
    ``boxes`` [n,4] YXYX in the S x S frame (``support_geometry``'s) -> (geometric records int32 [n,16] of
    ``query_augment_record(row, (S,S), (S,S))``, photometric records int32 [n,64] of ``query_photometric_record``,
    boxes [n,4] after the matrix in the dtype of ``boxes``, fallback flags bool [n]).  The fallback is per instance: where
    the transformed box has no overlap with the open S x S rectangle, that instance alone gets both neutral records and
    keeps its box (base_fst.py:751-768).  Every contract error of a row is raised here, fallback or not."""
    S = int(S)
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError(f'support_augment_plan: boxes must be [n,4], got {list(boxes.shape)}')
    n = boxes.shape[0]
    rows = [None] * n if rows is None else rows
    photo_rows = [None] * n if photo_rows is None else photo_rows
    if len(rows) != n or len(photo_rows) != n:
        raise ValueError(f'support_augment_plan: {n} boxes, {len(rows)} geometric and {len(photo_rows)} photometric rows')
    recs = np.zeros((n, AUG_REC_INTS), np.int32)
    precs = np.zeros((n, PHOTO_REC_INTS), np.int32)
    out = np.array(boxes, copy=True)
    fell_back = np.zeros(n, bool)
    for i, (row, prow) in enumerate(zip(rows, photo_rows)):
        recs[i] = query_augment_record(row, (S, S), (S, S))
        precs[i] = query_photometric_record(prow, (S, S), (S, S))
        if row is None or augment_is_neutral(check_augment_params(row)):
            recs[i] = query_augment_record(None, (S, S), (S, S))          # (a neutral row's border is of no account)
            continue
        nb, ok = augment_boxes_yxyx(boxes[i:i + 1], row, S, S)
        if ok:
            out[i] = nb[0]
        else:
            fell_back[i] = True
            recs[i] = query_augment_record(None, (S, S), (S, S))
            precs[i] = query_photometric_record(None, (S, S), (S, S))
    return recs, precs, out, fell_back


def support_augment_chain_plan(rows, chains, boxes, S: int):
    """``support_augment_plan`` with a chain per instance in place of the single photometric row: ``chains`` [n,P,3] (or
    None: neutral) -> (geometric records int32 [n,16], chain records int32 [n,``PHOTO_CHAIN_MAX``,64] of
    ``photometric_chain_records`` at S -> S, boxes, fallback flags).  A fallen-back instance gets the neutral chain;
    every contract error of a chain is raised, fallback or not."""
    S = int(S)
    recs, _, out, fell_back = support_augment_plan(rows, None, boxes, S)
    n = len(recs)
    chains = [None] * n if chains is None else chains
    if len(chains) != n:
        raise ValueError(f'support_augment_chain_plan: {n} boxes and {len(chains)} photometric chains')
    precs = np.stack([photometric_chain_records(c, (S, S), (S, S), 'spp_photometric_chain') for c in chains]) if n else \
        np.zeros((0, PHOTO_CHAIN_MAX, PHOTO_REC_INTS), np.int32)
    precs[fell_back] = query_photometric_record(None, (S, S), (S, S))
    return recs, precs, out, fell_back


def draw_support_augment(rng):
    """One support instance's row pair (row of ``AUG_PARAMS``, row of ``PHOTO_PARAMS``), drawn as
    ``draw_query_augment_full`` draws a query's: the few-shot dataset classes assign ``augs_spp = augs_seq``."""
    return draw_query_augment_full(rng)


class SyntheticFewShotISEG(Dataset):
    def __init__(self, n_ways=3, k_shots=3, length=64, height=800, width=1333, spp_img_size=256, batch=4,
                 seed=1234, suffix='SYNTH_val_novel', polygons=None):
        # ``polygons`` (``episodes.make_episode``): None - ellipses, dense masks, as ever; 'dense' / 'poly' - polygonal
        # instances whose masks travel dense or as COCO polygons
        self.polygons = polygons
        self.n_ways, self.k_shots = n_ways, k_shots
        self.length, self.batch = length, batch
        self.height, self.width, self.spp_img_size = height, width, spp_img_size
        if batch > 1:       # the reference rounds batched sizes to multiples of 16 (base_fst.py:693-694)
            self.height, self.width = height // 16 * 16, width // 16 * 16
        self.seed, self.suffix = seed, suffix
        self.sampling_origin_ds, self.sampling_origin_ds_subset = 'SYNTH', 'val'
        self.sampling_cats, self.sampling_scenario, self.finetune = 'novel', 'parents', 'None'

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        return episodes.make_episode(int(idx), self.n_ways, self.k_shots, self.height, self.width,
                                     self.spp_img_size, seed=self.seed, polygons=self.polygons)

    def reshuffle(self):
        self.seed += self.length

    def evaluate(self, results=None, results_pkl_dir_fp=None, model_dir=None, total=1):
        """Same return keys as BaseFewShotISEG.evaluate (base_fst.py:1597-1601)."""
        assert (results is not None) ^ (results_pkl_dir_fp is not None)
        out = {}
        for kind, key in (('segm', 'isegm'), ('bbox', 'bbox')):
            ev = FSISEGEval(results=results, results_pkl_dir_fp=results_pkl_dir_fp, n_ways=self.n_ways,
                            iou_type=kind).run()
            out[f'{key}_mAP'], out[f'{key}_mAR'] = ev['mAP'], ev['mAR']
        return out


def write_chunked(results_iter, out_dir, chunk=1000):
    """main.py:290-309: results pickled in chunks of 1000 as ResultsChunked/NN.pkl."""
    os.makedirs(out_dir, exist_ok=True)
    buf, counter = [], 0
    for res in results_iter:
        buf.extend(res)
        if len(buf) >= chunk:
            with open(os.path.join(out_dir, f'{counter:02}.pkl'), 'wb') as fh:
                pickle.dump(buf, fh)
            buf, counter = [], counter + 1
    if buf:
        with open(os.path.join(out_dir, f'{counter:02}.pkl'), 'wb') as fh:
            pickle.dump(buf, fh)


class ClutteredCharsFewShotISEG(Dataset):
    """MNISTISEG / OMNIISEG-shaped episodes (cfg1 / cfg2 of BASELINE.json) over the numpy cluttered-
    character generator: the sample dict of base_fst.py:1248-1266, class-major supports built from one
    instance each with the reference's crop geometry (``support_from_instance``: offset ratio from fill ratio 0.8,
    square reflect-padded crop, resize of the longer side, centre pad), per-episode category ids 0..N-1, images normalised with the
    dataset mean/std (datasets/mnistiseg/ParamsMNISTISEG.json:1-5, datasets/omniiseg/ParamsOMNIISEG.json:1-5).
    Character datasets are batched without aspect-ratio grouping (base_fst.py:611-624).
    ``raw_uint8``: the images stay decoded pixels - ``qry_img`` uint8 [H,W,3], ``spp_imgs`` uint8 [N*K,S,S,3] - for a
    detector that normalises on the device (``FGN.set_input_norm(**ds.input_norm)``); nothing else of the sample changes.
    ``source_size`` = S (needs ``raw_uint8``): the images are generated at S x S instead of the network size and the
    query is NOT resized by the loader (``get_query``'s cv2.resize, base_fst.py:876-887) - ``qry_img`` [S,S,3],
    ``qry_isegmaps`` and ``qry_bboxes`` stay at source size and the sample carries ``qry_resize_to`` = (img_size,
    img_size) for a detector that resizes on the device (``FGN.simple_test(qry_resize_to=...)``); ``img_shape`` is the
    network size.  Without it the samples are what they always were.
    ``spp_source`` (needs ``raw_uint8``): no support crop is built by the loader (``get_support``'s crop, resize and pad,
    base_fst.py:1043-1167) - ``spp_imgs`` is the list of the N*K instances' SOURCE images uint8 [h,w,3], ``spp_isegmaps``
    the list of their masks [h,w] bool, ``spp_bboxes`` [N*K,4] their boxes YXYX in the source frame, and the sample
    carries ``spp_crop_to`` = spp_img_size, ``spp_fill_ratio`` and ``crop_square`` for a detector that cuts the supports
    on the device (``FGN.simple_test(spp_crop_to=...)``).  Off by default: the samples are then what they always were.
    ``augment_qry`` (needs ``source_size``): the sample carries ``qry_augment``, one row of ``AUG_PARAMS`` float64 [8]
    drawn by ``draw_query_augment`` per (seed, child, epoch of ``reshuffle``), for a detector that augments the query on
    the device (``FGN.forward_train(qry_augment=...)``; ``get_query`` with ``augment_qry``, base_fst.py:889-891); the
    pixels, masks and boxes of the sample are NOT augmented.  Off by default: the samples are then what they always
    were.  ``photometric_qry`` (needs ``augment_qry``): the sample also carries ``qry_photometric``, one row of
    ``PHOTO_PARAMS`` float64 [3], and both rows come from the joint draw ``draw_query_augment_full`` (the whole
    ``augs_seq``), seeded the same way, for ``FGN.forward_train(qry_photometric=...)``.  Off by default: the samples
    are then key for key what they are without it.
    ``augment_spp`` (needs ``spp_source``): the sample carries ``spp_augment``, float64 [N*K,8], one row of ``AUG_PARAMS``
    per support instance, for a detector that augments the supports on the device behind their cut
    (``FGN.forward_train(spp_augment=...)``; ``get_support`` with ``augment_spp``, base_fst.py:1151-1153).  Instance i
    is drawn from ``np.random.default_rng([seed, child, epoch, 1 + i])`` - four words, disjoint from the query's three -
    by ``draw_query_augment``; the pixels, masks and boxes of the sample are NOT augmented.  ``photometric_spp`` (needs
    ``augment_spp``): the sample also carries ``spp_photometric`` [N*K,3] and both rows of an instance come from the
    joint draw ``draw_support_augment``, seeded the same way.  Off by default: the samples are then key for key what
    they are without them, and ``qry_augment`` / ``qry_photometric`` are the same with or without them.
    ``augs`` = 'natural' (default: everything above) or 'coco': the rows come from ``draw_coco_augment`` (COCO's
    ``augs_seq``, coco_ds.py:45-59: flip, one HSV operator, blur), seeded the same way, and with ``photometric_qry`` /
    ``photometric_spp`` the sample carries ``qry_photometric_chain`` [2,3] / ``spp_photometric_chain`` [N*K,2,3] in place
    of the single rows, for ``FGN.forward_train(qry_photometric_chain=..., spp_photometric_chain=...)``.
    ``rle_masks``: ``qry_isegmaps`` is the list of the instances' ``rle.encode`` dicts - the form the reference's COCO
    dataset holds its masks in (coco_ds.py:195-207) - for a detector that decodes on the device, and
    with ``spp_source`` every entry of ``spp_isegmaps`` is such a dict too.  Off by default; nothing else of a sample
    changes.  ``color_masks`` (needs ``raw_uint8``; not beside ``rle_masks``): ``qry_isegmaps`` is a
    ``colormask.ColorMasks`` of the kept instances - box and colour, all that MNISTISEG / OMNIISEG store per instance
    (``*_colors.pkl``, mnistiseg_ds.py:103) - for a detector that makes the masks on the device from the image bytes
    (DESIGN.md 4.4.11), and with ``spp_source`` every entry of ``spp_isegmaps`` is one such item.  Off by default;
    nothing else of a sample changes."""
    PARAMS = {'MNISTISEG': dict(mean=(0.9531239867210388, 0.9524800777435303, 0.9531603455543518),
                                std=(0.16827817261219025, 0.16883736848831177, 0.16667258739471436), n_cats=10),
              'OMNIISEG': dict(mean=(0.9628916382789612, 0.9640044569969177, 0.9626953601837158),
                               std=(0.16037128865718842, 0.15775758028030396, 0.15985246002674103), n_cats=26)}

    def __init__(self, dataset='MNISTISEG', n_ways=1, k_shots=1, n_imgs=32, img_size=128, spp_img_size=128,
                 spp_fill_ratio=0.8, batch=1, shuffle=False, seed=1234, raw_uint8=False, source_size=None,
                 spp_source=False, augment_qry=False, photometric_qry=False, augment_spp=False, photometric_spp=False,
                 augs='natural', rle_masks=False, color_masks=False):
        par = self.PARAMS[dataset]
        self.rle_masks = bool(rle_masks)
        self.color_masks = bool(color_masks)
        if self.color_masks and self.rle_masks:
            raise ValueError('color_masks and rle_masks are two forms of one argument: a sample carries its masks as '
                             'box + colour or as COCO RLE, not both')
        if self.color_masks and not raw_uint8:
            raise ValueError('color_masks needs raw_uint8=True: the detector makes the masks from the image\'s bytes')
        if augs not in ('natural', 'coco'):
            raise ValueError(f'augs is \'natural\' (natural_fst.py:18-35) or \'coco\' (coco_ds.py:45-59), got {augs!r}')
        self.augs = augs
        self.raw_uint8 = bool(raw_uint8)
        self.spp_source = bool(spp_source)
        if self.spp_source and not self.raw_uint8:
            raise ValueError('spp_source needs raw_uint8=True: supports are cut from their source images by the detector, '
                             'which takes decoded pixels')
        self.source_size = None if source_size is None else int(source_size)
        if self.source_size is not None and not self.raw_uint8:
            raise ValueError('source_size needs raw_uint8=True: source-size queries are resized by the detector, which '
                             'takes decoded pixels')
        self.augment_qry = bool(augment_qry)
        if self.augment_qry and self.source_size is None:
            raise ValueError('augment_qry needs source_size: the query is augmented by the detector together with its '
                             'resize from the source size')
        self.photometric_qry = bool(photometric_qry)
        if self.photometric_qry and not self.augment_qry:
            raise ValueError('photometric_qry needs augment_qry: the two rows are one joint draw of the reference\'s '
                             'augs_seq')
        self.augment_spp = bool(augment_spp)
        if self.augment_spp and not self.spp_source:
            raise ValueError('augment_spp needs spp_source: the supports are augmented by the detector behind their cut '
                             'from the source images')
        self.photometric_spp = bool(photometric_spp)
        if self.photometric_spp and not self.augment_spp:
            raise ValueError('photometric_spp needs augment_spp: the two rows of an instance are one joint draw of the '
                             'reference\'s augs_seq')
        self.epoch = 0                               # the ``e`` of the last ``reshuffle``: one augmentation draw per epoch
        self.n_ways, self.k_shots, self.batch, self.shuffle = n_ways, k_shots, batch, shuffle
        self.img_size, self.spp_img_size, self.spp_fill_ratio = img_size, spp_img_size, spp_fill_ratio
        self.sampling_origin_ds, self.sampling_origin_ds_subset = dataset, 'val'
        self.sampling_cats, self.sampling_scenario, self.finetune = 'all', 'parents', 'None'
        self.mean = np.asarray(par['mean'], np.float32)
        self.std = np.asarray(par['std'], np.float32)
        self.seed = seed
        cats = np.arange(par['n_cats'])
        self.images = [cc.make_image(seed + j, img_size if self.source_size is None else self.source_size, cats)
                       for j in range(n_imgs)]
        # instance table: (image, object) per class, instance id = position in this table
        self.inst = [(j, o) for j, im in enumerate(self.images) for o in range(len(im['cat_ids']))]
        self.inst_cat = np.array([self.images[j]['cat_ids'][o] for j, o in self.inst])
        self.cats = cats
        self.order_initial = np.arange(n_imgs, dtype=np.int32)
        self.order = self.order_initial.copy()

    def __len__(self):
        return len(self.order)

    def reshuffle(self, e=8):
        """base_fst.py:605-624."""
        order = list(self.order_initial)
        if self.shuffle:
            random.Random((2 ** e) % 1000).shuffle(order)
        self.order = np.array(order, dtype=np.int32)
        self.epoch = int(e)

    @property
    def input_norm(self) -> dict:
        """The normalisation ``_norm`` applies, as the arguments of ``FGN.set_input_norm``."""
        return dict(mean=self.mean.copy(), std=self.std.copy())

    def _norm(self, img_u8):
        if self.raw_uint8:
            return torch.from_numpy(img_u8.copy())         # (a private copy, like the float form)
        return torch.from_numpy(((img_u8.astype(np.float32) / 255.0 - self.mean) / self.std).transpose(2, 0, 1).copy())

    def __getitem__(self, idx):
        child = int(self.order[int(idx)])
        im = self.images[child]
        rng = np.random.RandomState(self.seed * 31 + child)
        # classes of the episode: the query's own classes first, then random others (novel classes of a
        # query always get a support; base_fst.py samples the same way from the query's categories)
        present = list(dict.fromkeys(im['cat_ids'].tolist()))
        rng.shuffle(present)
        have = set(self.inst_cat.tolist())           # only classes with at least one instance can give a support
        others = [c for c in rng.permutation(self.cats).tolist() if c not in present and c in have]
        real = np.array((present + others)[:self.n_ways], np.int64)
        if len(real) < self.n_ways:
            raise ValueError(f'the image pool holds {len(have)} classes, fewer than n_ways={self.n_ways}')
        mapping = np.full(int(self.cats.max()) + 1, -1, np.int64)
        mapping[real] = np.arange(len(real))
        keep = mapping[im['cat_ids']] >= 0
        spp_imgs, spp_boxes, spp_masks, spp_ids = [], [], [], []
        for c in real:                                   # class-major (base_fst.py:1054-1080)
            pool = np.flatnonzero(self.inst_cat == c)
            foreign = np.array([p for p in pool if self.inst[p][0] != child], np.int64)
            pool = foreign if len(foreign) >= 1 else pool
            pick = rng.choice(pool, self.k_shots, replace=len(pool) < self.k_shots)
            for p in pick:
                j, o = self.inst[p]
                src = self.images[j]
                if self.spp_source:                      # the instance as it is: image, box and mask at source size
                    spp_imgs.append(torch.from_numpy(src['img'].copy()))
                    spp_boxes.append(np.asarray(src['bboxes'][o], np.float32))
                    if self.color_masks:                 # box + colour: what the dataset stores, nothing dense
                        spp_masks.append(colormask.as_color_masks(
                            {'bboxes': src['bboxes'][o], 'colors': src['colors'][o]}, src['img'].shape[:2], 'support'))
                    else:
                        m = src['isegmaps'][o].astype(bool)
                        spp_masks.append(rle.encode(m) if self.rle_masks else m)
                    spp_ids.append(p)
                    continue
                crop, nb, m = support_from_instance(src['img'], src['bboxes'][o], src['isegmaps'][o],
                                                    self.spp_img_size, self.spp_fill_ratio)
                spp_imgs.append(self._norm(crop)); spp_boxes.append(nb); spp_masks.append(m); spp_ids.append(p)
        sample = {
            'idx': int(idx),
            'qry_child_idx': child,
            'qry_img': self._norm(im['img']),
            'qry_cat_ids_real': im['cat_ids'][keep].astype(np.int64),
            'qry_cat_ids': mapping[im['cat_ids'][keep]].astype(np.int64),
            'qry_bboxes': im['bboxes'][keep].astype(np.float32),
            'qry_isegmaps': rle.encode_many(im['isegmaps'][keep]) if self.rle_masks else
            colormask.as_color_masks({'bboxes': im['bboxes'][keep], 'colors': im['colors'][keep]}, im['img'].shape[:2],
                                     'query') if self.color_masks else im['isegmaps'][keep].astype(bool),
            'spp_imgs': spp_imgs if self.spp_source else torch.stack(spp_imgs),
            'spp_bboxes': np.stack(spp_boxes).astype(np.float32),
            'spp_isegmaps': spp_masks if self.spp_source else np.stack(spp_masks).astype(bool),
            'cats_ids_to_sample_real': real,
            'cats_ids_to_sample': np.arange(len(real), dtype=np.int64),
            'spp_insts_ids': np.asarray(spp_ids, np.int64),
            'img_shape': np.array([self.img_size, self.img_size, 3], dtype=np.int32),
        }
        if self.source_size is not None:
            sample['qry_resize_to'] = np.array([self.img_size, self.img_size], dtype=np.int32)
        coco = self.augs == 'coco'               # (one joint draw per image either way; the chain only with photometric_*)
        if coco and self.augment_qry:
            row, chain = draw_coco_augment(np.random.default_rng([int(self.seed), child, self.epoch]))
            sample['qry_augment'] = row
            if self.photometric_qry:
                sample['qry_photometric_chain'] = chain
        elif self.photometric_qry:
            sample['qry_augment'], sample['qry_photometric'] = \
                draw_query_augment_full(np.random.default_rng([int(self.seed), child, self.epoch]))
        elif self.augment_qry:
            sample['qry_augment'] = draw_query_augment(np.random.default_rng([int(self.seed), child, self.epoch]))
        if self.spp_source:
            sample.update(spp_crop_to=int(self.spp_img_size), spp_fill_ratio=float(self.spp_fill_ratio), crop_square=True)
        if self.augment_spp:                     # instance i: its own stream, disjoint from the query's three-word seed
            rngs = [np.random.default_rng([int(self.seed), child, self.epoch, 1 + i]) for i in range(len(spp_ids))]
            if coco:
                pairs = [draw_coco_augment(r) for r in rngs]
                sample['spp_augment'] = np.stack([p for p, _ in pairs])
                if self.photometric_spp:
                    sample['spp_photometric_chain'] = np.stack([q for _, q in pairs])
            elif self.photometric_spp:
                pairs = [draw_support_augment(r) for r in rngs]
                sample['spp_augment'] = np.stack([p for p, _ in pairs])
                sample['spp_photometric'] = np.stack([q for _, q in pairs])
            else:
                sample['spp_augment'] = np.stack([draw_query_augment(r) for r in rngs])
        return sample

    evaluate = SyntheticFewShotISEG.evaluate


# ------------------------------------------------------------------------------------------------
# Episodic sampling on a databag (which instances form an episode): the index half of
# BaseFewShotISEG.load_dataset / reshuffle / __getitem__ / get_query / get_support
# ------------------------------------------------------------------------------------------------
class Databag:
    """The lookup tables ``load_dataset`` collects or reads (base_fst.py:328-432): parent queries (one per image, with
    ``cats_dict`` category -> instance ids in insertion order and the ids of their child queries), child queries
    ``[parent, category]`` (one per image and category on it), per-class instance lists, per-instance parent / category
    / box.  Built from the reference's pickle (``from_pickle``: the tuple ``(qrys_parents_, qrys_children,
    cats_insts_list, insts)``; the older files hold SETS as class lists - kept in their iteration order, which is what
    the reference's list comprehensions see) or from flat arrays (``from_arrays``: tests/golden/databag_sampler.npz)."""

    def __init__(self, parents_cats, parents_children, children, class_lists, inst_parent, inst_cat, inst_bbox):
        self.parents_cats = parents_cats            # list of [(cat_id, [inst ids])] per parent, insertion order
        self.parents_children = parents_children    # list of [child ids] per parent
        self.children = children                    # [n_children, 2] (parent, category)
        self.class_lists = class_lists              # list of [inst ids] per category
        self.inst_parent, self.inst_cat, self.inst_bbox = inst_parent, inst_cat, inst_bbox

    @classmethod
    def from_pickle(cls, path: str) -> 'Databag':
        with open(path, 'rb') as fh:
            parents, children, class_lists, insts = pickle.load(fh)
        return cls([[(int(c), [int(i) for i in v]) for c, v in p['cats_dict'].items()] for p in parents],
                   [[int(c) for c in p['nums_children_qrys']] for p in parents],
                   np.asarray(children, np.int64).reshape(-1, 2), [[int(i) for i in lst] for lst in class_lists],
                   np.array([int(i.get('num_parent_qry', -1)) for i in insts]),
                   np.array([int(i['cat_id']) for i in insts]),
                   np.array([np.asarray(i['bbox'], np.float32) for i in insts], np.float32).reshape(-1, 4))

    @classmethod
    def from_arrays(cls, z, prefix: str = 'bag__') -> 'Databag':
        g = lambda k: np.asarray(z[prefix + k])
        pp, pc, pi = g('parent_ptr'), g('parent_cat'), g('parent_inst')
        parents_cats = []
        for a, b in zip(pp[:-1], pp[1:]):
            d = {}
            for c, i in zip(pc[a:b], pi[a:b]):
                d.setdefault(int(c), []).append(int(i))
            parents_cats.append(list(d.items()))
        cp, ch = g('parent_children_ptr'), g('parent_children')
        lp, li = g('class_ptr'), g('class_inst')
        return cls(parents_cats, [[int(c) for c in ch[a:b]] for a, b in zip(cp[:-1], cp[1:])], g('children'),
                   [[int(i) for i in li[a:b]] for a, b in zip(lp[:-1], lp[1:])], g('inst_parent'), g('inst_cat'),
                   g('inst_bbox'))


class DatabagEpisodeSampler:
    """Index producer of the reference's episodic dataset on a ``Databag``: ``len`` / ``order`` as ``load_dataset``
    builds them, ``sample_indices(idx)`` = everything ``__getitem__`` decides before it touches a pixel.  Draws come
    from Python's ``random`` module in the reference's call order (``random.choice`` of the child under 'parents',
    ``random.sample`` of the other categories, ``random.shuffle`` of the N, ``random.sample`` of K instances per
    category), so a seeded run replays the reference's episodes exactly (tests/golden/databag_sampler.npz)."""

    def __init__(self, bag: Databag, n_ways: int, k_shots: int, cats_novel, cats_total_amount: int,
                 sampling_cats: str = 'base_', sampling_scenario: str = 'parents', shuffle: bool = False, repeats: int = 1,
                 first_parents__only: int = 0, first_children_only: int = 0, qry_cats_choice_remove: bool = False,
                 qry_cats_choice_random: bool = False, qry_cats_order_shuffle: bool = True,
                 delete_qry_insts_in_spp_insts_on_train: bool = True, spp_random: bool = True, rng=None):
        self.bag, self.n_ways, self.k_shots = bag, int(n_ways), int(k_shots)
        self.sampling_scenario = sampling_scenario
        self.shuffle = shuffle
        self.qry_cats_choice_remove, self.qry_cats_choice_random = qry_cats_choice_remove, qry_cats_choice_random
        self.qry_cats_order_shuffle = qry_cats_order_shuffle
        self.delete_qry_insts = delete_qry_insts_in_spp_insts_on_train
        self.spp_random = spp_random
        self.random = rng if rng is not None else random          # the module itself: the reference's global stream
        # ---- cats_selection (base_fst.py:267-300)
        novel = np.array([] if sampling_cats == 'all' else cats_novel, dtype=np.int32)
        is_base = np.ones(cats_total_amount, bool)
        is_base[novel] = False
        base = np.where(is_base)[0]
        if sampling_cats == 'base_':
            self.cats_to_save = base
        elif sampling_cats == 'novel':
            self.cats_to_save = novel
        elif sampling_cats == 'all':
            self.cats_to_save = np.arange(cats_total_amount).astype(np.int32)
        else:
            raise ValueError(f'sampling_cats {sampling_cats!r}')
        self.cats_to_save_bool = np.zeros(cats_total_amount, bool)
        self.cats_to_save_bool[self.cats_to_save] = True
        # ---- order (base_fst.py:438-474)
        n_par, n_chi = len(bag.parents_cats), len(bag.children)
        if sampling_scenario not in ('parents', 'children'):
            raise ValueError(f'sampling_scenario {sampling_scenario!r}')
        order = np.arange(n_par if sampling_scenario == 'parents' else n_chi)
        if 0 < first_parents__only <= n_par:
            if sampling_scenario == 'parents':
                order = order[:first_parents__only]
            else:
                order = order[:bag.parents_children[first_parents__only - 1][-1] + 1]
        if 0 < first_children_only <= n_chi:
            if sampling_scenario == 'parents':
                order = order[:int(bag.children[first_children_only - 1][0]) + 1]
            else:
                order = order[:first_children_only]
        if not 1 <= repeats <= 100:
            repeats = 1
        self.order_initial = np.tile(order, reps=repeats)
        self.reshuffle()

    def reshuffle(self, e: int = 8) -> None:
        """``reshuffle`` of a batch-1 / synthetic-dataset run (base_fst.py:611-625): a fixed permutation per epoch seed."""
        self.order = self.order_initial.copy()
        if self.shuffle:
            order = list(self.order)
            random.Random((2 ** e) % 1000).shuffle(order)
            self.order = np.array(order, dtype=np.int32)

    def __len__(self) -> int:
        return len(self.order)

    def sample_indices(self, idx: int) -> dict:
        bag, R = self.bag, self.random
        real_idx = int(self.order[idx])
        # __getitem__ (base_fst.py:1197-1210)
        child = R.choice(bag.parents_children[real_idx]) if self.sampling_scenario == 'parents' else real_idx
        parent, cat_main = int(bag.children[child][0]), int(bag.children[child][1])
        cats_dict = dict(bag.parents_cats[parent])
        cats_on_img = list(cats_dict)
        # get_query (base_fst.py:793-824): the N - 1 other categories
        cats = [cat_main]
        keep = self.cats_to_save_bool.copy()
        keep[cat_main] = False
        if self.qry_cats_choice_remove:
            keep[cats_on_img] = False
        pool = [int(c) for c in np.nonzero(keep)[0]]
        if self.qry_cats_choice_random:
            if len(pool) < self.n_ways - 1:
                raise NotImplementedError(f'could not select {self.n_ways} categories')
            other = R.sample(pool, self.n_ways - 1)
        else:
            other = pool[:self.n_ways - 1]
        cats.extend(other)
        if self.qry_cats_order_shuffle:
            R.shuffle(cats)
        cats_real = np.array(cats, dtype=np.int32)
        # ... the query's instances (base_fst.py:826-846)
        qry_insts, qry_cats = [], []
        for c in cats_real:
            if int(c) not in cats_dict:
                continue
            qry_insts.extend(cats_dict[int(c)])
            qry_cats.extend([int(c)] * len(cats_dict[int(c)]))
        # get_support (base_fst.py:1052-1080): K instances per category
        spp = []
        for c in cats_real:
            lst = bag.class_lists[int(c)]
            pool_i = [v for v in lst if v not in qry_insts] if self.delete_qry_insts else lst
            if self.spp_random:
                if len(pool_i) < self.k_shots:
                    raise NotImplementedError(f'could not sample {self.k_shots} instances of category {int(c)}')
                spp.extend(R.sample(pool_i, self.k_shots))
            else:
                spp.extend(pool_i[:self.k_shots])
        # remap to 0..N-1 (base_fst.py:1243-1246)
        mapping = np.zeros(int(cats_real.max()) + 1, dtype=np.int32)
        mapping[cats_real] = np.arange(len(cats_real))
        qry_cats = np.array(qry_cats, dtype=np.int32)
        qry_insts = np.array(qry_insts, dtype=np.int32)
        return dict(idx=idx, qry_child_idx=int(child), idx_parent=parent, cat_id_main=cat_main,
                    cats_ids_to_sample_real=cats_real.astype(np.int64),
                    cats_ids_to_sample=mapping[cats_real].astype(np.int64),
                    qry_insts_ids=qry_insts, qry_cat_ids_real=qry_cats.astype(np.int64),
                    qry_cat_ids=mapping[qry_cats].astype(np.int64) if len(qry_cats) else np.zeros(0, np.int64),
                    qry_bboxes=bag.inst_bbox[qry_insts].astype(np.float32).reshape(-1, 4),
                    spp_insts_ids=np.array(spp).astype(np.int64))
