"""The compact forms a mask may come in, stated once (host side).

An image's ground truth, or one support instance's mask, is dense (array, tensor, nested lists) or in one of ``FORMS``:
box + colour (``colormask``), COCO polygons (``polygon``), COCO RLE (``rle``).  ``FORMS`` is in the order the forms are
asked in, and that order matters: ANY dict is an RLE item (``rle.is_item``), so the two forms whose dicts are told by
their key names come before RLE (they exclude each other).  The per-form modules keep their predicates and checkers;
the records name them, and whoever has to tell the forms apart (``detector``, ``episodes.collate``) asks here.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

from . import colormask, polygon, rle


class Form(NamedTuple):
    carrier: type           # what the checkers return
    is_entry: Callable      # (x) -> bool: x holds the masks of one image in this form
    is_one: Callable        # (x) -> bool: x holds ONE mask (a support instance's) in this form
    check: Callable         # (entry, hw, what, img) -> the carrier of one image's masks, checked
    check_one: Callable     # (item, hw, what) -> the carrier of ONE mask, checked (``checked_one`` counts it)
    nbytes: Callable        # (carrier) -> the bytes that cross the bus for it


COLOR = Form(colormask.ColorMasks, colormask.is_color, colormask.is_color,
             lambda e, hw, what, img: colormask.as_color_masks(e, hw, what, img=img), colormask.as_color_masks,
             lambda c: colormask.REC_BYTES * len(c))
POLY = Form(polygon.PolyMasks, polygon.is_poly, polygon.is_poly,
            lambda e, hw, what, img: polygon.as_polys(e, hw, what),
            lambda m, hw, what: polygon.as_polys(m, hw, what, single=True), lambda p: p.xy.nbytes)
RLE = Form(rle.RleMasks, rle.is_rle, lambda x: rle.is_item(x) or isinstance(x, rle.RleMasks),
           lambda e, hw, what, img: rle.as_masks(e, hw, what),
           lambda m, hw, what: rle.as_masks(m if isinstance(m, rle.RleMasks) else [m], hw, what), lambda r: r.ends.nbytes)
FORMS = (COLOR, POLY, RLE)


def form_of(entry) -> Optional[Form]:
    """The form of one image's entry (a carrier, or what its checker takes); None: dense.  The empty list is RLE."""
    return next((f for f in FORMS if f.is_entry(entry)), None)


def form_of_one(item) -> Optional[Form]:
    """The form of ONE support instance's mask; None: dense."""
    return next((f for f in FORMS if f.is_one(item)), None)


def is_pair(x) -> bool:
    """Whether the list / tuple ``x`` is ONE RLE mask as a ``[size, counts]`` pair - not a support set, not rows."""
    return isinstance(x, (list, tuple)) and rle.is_item(x)


def checked(entry, hw, what: str = 'masks', img=None):
    """One image's entry -> its checked carrier at ``hw`` = (h, w) (None: the entry's own size; ValueError names
    ``what``), a colour carrier bound to ``img``.  A dense entry comes back untouched."""
    form = form_of(entry)
    return entry if form is None else form.check(entry, hw, what, img)


def checked_one(item, hw, what: str = 'masks'):
    """ONE support instance's mask -> its checked carrier of exactly one mask at ``hw``; a dense mask: untouched."""
    form = form_of_one(item)
    if form is None:
        return item
    carrier = form.check_one(item, hw, what)
    if len(carrier) != 1:
        raise ValueError(f'{what}: one mask per support instance, got {len(carrier)}')
    return carrier


def dense(entry, what: str = 'masks'):
    """One image's entry on the host: the carrier's ``dense()`` (colour: of the image it is bound to); dense: untouched."""
    return entry if form_of(entry) is None else checked(entry, None, what).dense()
