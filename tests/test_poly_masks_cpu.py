"""COCO polygons as an input form, host side: the stated rule of ``fgn_amd/polygon.py`` against known
answers, its own invariances, ``rle.py`` and an independent rasteriser; the accepted forms and refusals of
``polygon.as_polys``; the bound that sizes the device's slices and the route it decides.  pycocotools is not available to
the suite: nothing here pins the rule to it ("Unpinned")."""
import numpy as np
import pytest

from fgn_amd import polygon, rle

from _poly_cases import shapes, star, zigzag


def _rect(x0, y0, x1, y1):
    return [x0, y0, x0, y1, x1, y1, x1, y0]


@pytest.mark.parametrize('hw,box', [((8, 10), (2, 1, 7, 5)), ((8, 10), (0, 0, 10, 8)), ((1, 1), (0, 0, 1, 1)),
                                    ((5, 7), (3, 0, 7, 2)), ((37, 53), (11, 7, 12, 36)), ((6, 6), (-4, -3, 3, 2)),
                                    ((6, 6), (2, 3, 40, 50))],
                         ids=lambda v: 'x'.join(str(i) for i in v))
def test_integer_rectangles_are_exact(hw, box):
    """[x0, x1) x [y0, y1), clipped to the mask: one touching all four borders, some leaving the image."""
    h, w = hw
    x0, y0, x1, y1 = box
    want = np.zeros((h, w), np.uint8)
    want[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 1
    assert np.array_equal(polygon.dense([_rect(*box)], h, w), want)


def test_the_rectangle_of_the_issue_and_one_wholly_outside():
    got = polygon.dense([[2, 1, 2, 5, 7, 5, 7, 1]], 8, 10)
    want = np.zeros((8, 10), np.uint8)
    want[1:5, 2:7] = 1
    assert np.array_equal(got, want)
    for box in ((12, 1, 20, 5), (-9, -9, -2, -2), (2, 9, 7, 15), (-30, 2, -20, 6)):
        assert polygon.part_crossings(_rect(*box), 8, 10).size % 2 == 0
        assert not polygon.dense([_rect(*box)], 8, 10).any(), box


@pytest.mark.parametrize('hw', [(1, 1), (7, 9), (100, 3000), (16384, 16384)], ids=lambda v: f'{v[0]}x{v[1]}')
def test_integer_forms_equal_the_double_expressions(hw):
    """Step 3 in integers is step 3 as C writes it in doubles, for every m, n in -20..20000."""
    v = np.arange(-20, 20001)
    a = polygon.crossing_of(v, v, *hw)
    b = polygon.double_crossing_of(v, v, *hw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][a[0]], b[1][b[0]]) and np.array_equal(a[2], b[2])
    assert a[0].any() and not a[0][v < 2].any()


def _cases():
    rng = np.random.RandomState(20261021)
    out = []
    for _ in range(400):
        h, w = int(rng.randint(8, 121)), int(rng.randint(8, 121))
        out.append((h, w, star(rng, h, w)))
    return out


STARS = _cases()


def test_reversal_and_rotation_leave_the_bits_unchanged():
    for h, w, xy in STARS[:150]:
        # (radii up to 1.6 of the half size: many of these leave the image)
        xy = (np.asarray(xy).reshape(-1, 2) - [w / 2, h / 2]) * 2.3 + [w / 2, h / 2]
        xy = np.round(xy, 2)
        want = polygon.dense([xy.reshape(-1)], h, w)
        assert np.array_equal(polygon.dense([xy[::-1].reshape(-1)], h, w), want)
        for r in range(1, len(xy)):
            assert np.array_equal(polygon.dense([np.roll(xy, r, 0).reshape(-1)], h, w), want), (h, w, r)


def test_an_instance_is_the_union_of_its_parts():
    h, w = 40, 50
    parts = shapes(h, w)['two overlapping parts']
    a, b = (polygon.dense([p], h, w) for p in parts)
    assert (a & b).any() and not np.array_equal(a | b, a ^ b)             # (XOR would differ)
    assert np.array_equal(polygon.dense(parts, h, w), a | b)
    pm = polygon.as_polys({'polygons': [parts, [parts[1]]]}, (h, w))
    assert np.array_equal(pm.dense(), np.stack([a | b, b]))


def test_consistent_with_rle():
    for h, w, xy in STARS[:60]:
        want = polygon.dense([xy], h, w)
        assert np.array_equal(rle.decode(polygon.to_rle([xy], h, w)), want)
        pos = polygon.part_crossings(xy, h, w)
        assert pos.dtype == np.uint32 and np.all(np.diff(pos.astype(np.int64)) >= 0)
        runs = rle.RleMasks((1, h, w), np.append(pos, np.uint32(h * w)), [0, pos.size + 1])
        assert np.array_equal(runs.dense()[0], want)
    for name, parts in shapes(37, 53).items():
        assert np.array_equal(rle.decode(polygon.to_rle(parts, 37, 53)), polygon.dense(parts, 37, 53)), name


def test_the_bound_is_at_least_the_count():
    cases = [(h, w, [xy]) for h, w, xy in STARS] + \
            [(h, w, parts) for h, w in ((37, 53), (70, 300), (1, 1), (1, 9)) for parts in shapes(h, w).values()] + \
            [(64, 64, [zigzag()])]
    for h, w, parts in cases:
        pm = polygon.as_polys({'polygons': [parts]}, (h, w))
        count = sum(polygon.part_crossings(p, h, w).size for p in parts)
        assert pm.crossing_bound[0] >= count, (h, w, parts)
        for q, p in enumerate(parts):
            assert pm.part_bound[q] >= polygon.part_crossings(p, h, w).size
            assert polygon.edge_records(p)[2] >= pm.part_bound[q]          # (the slice holds the bound)
            assert pm.part_points[q] == polygon.part_path(p)[0].size


def test_against_an_independent_rasteriser():
    """``PIL.ImageDraw.polygon(fill=1)`` rounds and closes differently, but both fill the same interior: the pixels that
    differ lie along the outline, at most one per unit of its L1 length.  A condition, not a tolerance: the rule alone
    measures 0.641 at worst on these 400 cases (0.56 on the 400 of another seed when the rule was first written down)."""
    from PIL import Image, ImageDraw
    worst = 0.0
    for h, w, xy in STARS:
        img = Image.new('L', (w, h), 0)
        ImageDraw.Draw(img).polygon([(xy[i], xy[i + 1]) for i in range(0, len(xy), 2)], fill=1)
        pts = np.asarray(xy).reshape(-1, 2)
        perimeter = np.abs(np.roll(pts, -1, 0) - pts).sum()
        diff = int((np.asarray(img) != polygon.dense([xy], h, w)).sum())
        worst = max(worst, diff / perimeter)
        assert diff <= 1.0 * perimeter, (h, w, xy, diff, perimeter)
    print(f'worst differing pixels / L1 perimeter: {worst:.3f}')


def test_accepted_forms():
    tri = [1, 1, 6, 2, 3, 6.5]
    pm = polygon.as_polys({'polygons': [[tri], [tri, np.asarray(tri) + 1]], 'size': [8, 9]}, None, 'x')
    assert pm.shape == (2, 8, 9) and len(pm) == 2 and pm.inst_first.tolist() == [0, 1, 3]
    assert polygon.as_polys(pm, (8, 9)) is pm and polygon.as_polys(pm, None) is pm
    assert polygon.as_polys({'polygons': [[tuple(tri)]]}, (8, 9)).shape == (1, 8, 9)
    assert polygon.as_polys({'polygons': []}, (8, 9)).shape == (0, 8, 9)
    one = polygon.as_polys({'polygons': [tri, tri]}, (8, 9), single=True)
    assert one.shape == (1, 8, 9) and np.array_equal(one.dense()[0], polygon.dense([tri], 8, 9))
    sub = pm.select([1])
    assert sub.shape == (1, 8, 9) and np.array_equal(sub.dense()[0], pm.dense()[1])
    assert polygon.is_poly(pm) and polygon.is_poly({'polygons': []}) and polygon.is_poly({'polygons': [], 'size': [1, 1]})
    for other in ([[tri]], [tri], tri, {'polygons': [], 'counts': b''}, {'size': [3, 3], 'counts': b'9'},
                  {'bboxes': [], 'colors': []}, np.zeros((1, 3, 3)), None):
        assert not polygon.is_poly(other)
    # rle.py's forms are as they were: a bare nested list is no RLE either, a polygon dict is no RLE item list
    assert not rle.is_rle([[tri]]) and not rle.is_rle({'polygons': [[tri]]}) and not rle.is_item([tri])
    # a sliver between two column centres toggles nothing: a legal, empty mask
    sliver = shapes(20, 20)['a sliver without a crossing']
    assert polygon.part_crossings(sliver[0], 20, 20).size == 0 and not polygon.dense(sliver, 20, 20).any()


TRI = [1, 1, 6, 2, 3, 6.5]
REFUSED = {
    'a bare nested list': ([[TRI]], (8, 9), 'expected a PolyMasks or a dict'),
    'a dict with other keys': ({'polygons': [[TRI]], 'counts': 1}, (8, 9), 'expected a PolyMasks or a dict'),
    'polygons is no list': ({'polygons': 5}, (8, 9), 'a list of instances'),
    'an instance is no list': ({'polygons': [5]}, (8, 9), 'instance 0 is a list of parts'),
    'an instance without a part': ({'polygons': [[TRI], []]}, (8, 9), 'instance 1 has no part'),
    'a part of odd length': ({'polygons': [[TRI, TRI + [1]]]}, (8, 9), 'instance 0, part 1: 7 numbers'),
    'a part of two vertices': ({'polygons': [[[1, 2, 3, 4]]]}, (8, 9), 'instance 0, part 0: 4 numbers'),
    'a nested part': ({'polygons': [[[[1, 2], [3, 4], [5, 6]]]]}, (8, 9), 'instance 0, part 0: expected a flat sequence'),
    'a part of strings': ({'polygons': [[['a'] * 6]]}, (8, 9), 'instance 0, part 0: expected a flat sequence'),
    'a part that is a string': ({'polygons': [['abcdef']]}, (8, 9), 'instance 0, part 0: expected a flat sequence'),
    'a part of bools': ({'polygons': [[[True] * 6]]}, (8, 9), 'instance 0, part 0: expected a flat sequence'),
    'a NaN': ({'polygons': [[TRI], [TRI, [1, 1, float('nan'), 2, 3, 3]]]}, (8, 9), 'instance 1, part 1: a coordinate is not finite'),
    'an infinity': ({'polygons': [[[1, 1, float('inf'), 2, 3, 3]]]}, (8, 9), 'not finite'),
    'a coordinate beyond 65536': ({'polygons': [[[1, 1, 65536.5, 2, 3, 3]]]}, (8, 9), 'outside +-65536'),
    'a coordinate below -65536': ({'polygons': [[[1, 1, 5, -65537, 3, 3]]]}, (8, 9), 'outside +-65536'),
    'a size that disagrees': ({'polygons': [[TRI]], 'size': [8, 10]}, (8, 9), 'of size [8, 10], expected [8, 9]'),
    'a size of three': ({'polygons': [[TRI]], 'size': [8, 9, 3]}, (8, 9), "'size' is"),
    'a size of floats': ({'polygons': [[TRI]], 'size': [8.0, 9.0]}, None, "'size' is"),
    'no size at all': ({'polygons': [[TRI]]}, None, 'no size of its own'),
    'a size of 0': ({'polygons': [[TRI]]}, (0, 9), 'within 1..16384'),
    'a size above 16384': ({'polygons': [[TRI]], 'size': [8, 16385]}, None, 'within 1..16384'),
    'a PolyMasks of another size': (polygon.PolyMasks((0, 8, 9), [], [0], [0]), (8, 10), 'polygon masks of size [8, 9]'),
}


@pytest.mark.parametrize('case', list(REFUSED))
def test_refusals_name_what_is_wrong(case):
    entry, hw, text = REFUSED[case]
    with pytest.raises(ValueError) as e:
        polygon.as_polys(entry, hw, 'qry_isegmaps[3]')
    assert str(e.value).startswith('qry_isegmaps[3]: ') and text in str(e.value), str(e.value)


def test_the_edge_values_are_accepted():
    pm = polygon.as_polys({'polygons': [[[65536, -65536, 0, 0, 3, 65536]]], 'size': [16384, 1]}, None)
    assert pm.shape == (1, 16384, 1)


def test_an_instance_over_the_capacity_goes_the_host_route():
    tri = [1, 1, 60, 20, 30, 60.5]
    pm = polygon.as_polys({'polygons': [[tri], [tri, zigzag()], [zigzag()], [tri, tri]]}, (64, 64))
    assert len(zigzag()) // 2 == 1400
    assert pm.part_bound.max() > polygon.CROSSING_CAP and pm.part_bound[0] <= polygon.CROSSING_CAP
    assert pm.on_host().tolist() == [False, True, True, False]
    items = pm.rle_items([1, 2])
    assert np.array_equal(rle.as_masks(items, (64, 64)).dense(), pm.dense()[1:3])
    assert pm.dense()[2].any()
    # ... and one with too long a path, whatever its bound: a needle of 2^20 points along y toggles at most two positions
    far = polygon.as_polys({'polygons': [[[1, -60000, 2, 60000, 1.5, 0]]]}, (64, 64))
    assert far.part_points[0] > polygon.POINT_CAP and far.part_bound[0] <= polygon.CROSSING_CAP
    assert far.on_host().tolist() == [True]


def test_the_binding_table_names_the_export():
    from fgn_amd import lib
    assert 'fgn_poly_masks_u8' in lib.SIGNATURES and len(lib.SIGNATURES['fgn_poly_masks_u8'][1]) == 12
