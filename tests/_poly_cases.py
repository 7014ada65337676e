"""Polygons shared by the polygon-mask tests: seeded star-shaped polygons, the shapes at which the rule
can go wrong, and the zigzag that exceeds the device's capacity."""
import numpy as np


def star(rng, h, w, k=None, lo=0.2, hi=0.7, centre=None):
    """One star-shaped polygon of k vertices (3..11) on an h x w mask: sorted angles, radii ``lo``..``hi`` of the half
    size, coordinates rounded to 0.01 - flat [x0, y0, x1, y1, ...]."""
    k = int(rng.randint(3, 12)) if k is None else k
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(lo, hi, k)
    cx, cy = (w / 2.0, h / 2.0) if centre is None else centre
    x = cx + rad * (w / 2.0) * np.cos(ang)
    y = cy + rad * (h / 2.0) * np.sin(ang)
    return np.round(np.stack([x, y], 1), 2).reshape(-1).tolist()


def zigzag(n_teeth=700, h=64, w=64):
    """A closed zigzag of 2 * n_teeth edges across the whole width: every edge spans the mask, so the sum over edges of
    floor(dX / 5) + 2 is far beyond the 8192 positions the device sorts per part, while the mask stays 64 x 64."""
    xy = []
    for i in range(2 * n_teeth):
        xy += [float(w) if i % 2 else 0.0, h * (i + 0.5) / (2 * n_teeth)]
    return xy


def shapes(h, w):
    """name -> one instance (a list of parts) on an h x w mask: the cases of the issue's list."""
    H, W = float(h), float(w)
    return {
        'triangle': [[0.3 * W, 0.2 * H, 0.9 * W, 0.5 * H, 0.2 * W, 0.95 * H]],
        'integer rectangle': [[1.0, 0.0, 1.0, max(H - 1, 1.0), max(W - 1, 2.0), max(H - 1, 1.0), max(W - 1, 2.0), 0.0]],
        'concave star': [[0.5 * W, 0.05 * H, 0.6 * W, 0.4 * H, 0.95 * W, 0.4 * H, 0.65 * W, 0.6 * H, 0.8 * W, 0.95 * H,
                          0.5 * W, 0.7 * H, 0.2 * W, 0.95 * H, 0.35 * W, 0.6 * H, 0.05 * W, 0.4 * H, 0.4 * W, 0.4 * H]],
        'axis-parallel edges only': [[2, 1, 2, H - 1, W / 2, H - 1, W / 2, H / 2, W - 2, H / 2, W - 2, 1]],
        'a repeated vertex': [[0.2 * W, 0.2 * H, 0.2 * W, 0.2 * H, 0.8 * W, 0.3 * H, 0.8 * W, 0.3 * H, 0.5 * W, 0.9 * H]],
        'rounding ties of 5x + .5': [[1.1, 0.9, W - 1.1, 1.3, W - 0.9, H - 1.1, 2.9, H - 0.9, 0.7, H / 2 + 0.1]],
        'negative coordinates': [[-3.7, -2.2, W / 2, -0.6, W / 3, H / 2 + 0.4, -1.5, H / 3]],
        'leaves on the left': [[-W / 2, 0.2 * H, 0.6 * W, 0.5 * H, -W / 3, 0.8 * H]],
        'leaves on the right': [[1.5 * W, 0.2 * H, 0.4 * W, 0.5 * H, 1.3 * W, 0.8 * H]],
        'leaves at the top': [[0.2 * W, -H / 2, 0.5 * W, 0.6 * H, 0.8 * W, -H / 3]],
        'leaves at the bottom': [[0.2 * W, 1.5 * H, 0.5 * W, 0.4 * H, 0.8 * W, 1.3 * H]],
        'leaves on all four sides': [[-0.5 * W, 0.5 * H, 0.5 * W, -0.6 * H, 1.5 * W, 0.5 * H, 0.5 * W, 1.7 * H]],
        'a sliver without a crossing': [[0.61, 0.2, 0.79, 0.2 + H / 2, 0.7, H - 0.1]],
        'two overlapping parts': [[0.1 * W, 0.1 * H, 0.7 * W, 0.1 * H, 0.7 * W, 0.7 * H, 0.1 * W, 0.7 * H],
                                  [0.4 * W, 0.4 * H, 0.95 * W, 0.4 * H, 0.95 * W, 0.95 * H, 0.4 * W, 0.95 * H]],
    }
