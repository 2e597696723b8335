"""Test helper for PQP_OPT_LONG_LINES (tests/test_gpu_long_lines.py): lines kilometres long with a distance layer that covers them - a
corridor-shaped map along the line, well under the 2^30-cell limit - and the handle options of the long forms."""
import numpy as np

import corridor_oracle as K
from path_optimizer_2_amd import capi

OPT_LDS_ONLY, OPT_BY_SIZE, OPT_LONG_ALWAYS = 0, 1, 2


def long_road(length, seed=0, resolution=0.2, width=60.0, amp=4.0, period=300.0):
    """A gently winding road y = amp sin(2 pi x / period) of `length` metres along x, on a map of (length + 40) x `width` metres that
    covers it, with round obstacles beside the road (6-12 m off the centre line): the road stays open, the bounds are not all the
    same.  Returns the centre line sampled every metre and the map."""
    rng = np.random.default_rng(seed)
    lx = length + 40.0
    rows, cols = int(round(lx / resolution)), int(round(width / resolution))
    lx, ly = rows * resolution, cols * resolution
    pos = (lx / 2.0 - 20.0, 0.0)                       # the map spans x in [-20, length + 20], y in [-width / 2, width / 2]
    cx = pos[0] + 0.5 * lx - 0.5 * resolution - resolution * np.arange(rows)
    cy = pos[1] + 0.5 * ly - 0.5 * resolution - resolution * np.arange(cols)
    free = np.ones((rows, cols), dtype=bool)
    centre = lambda x: amp * np.sin(2.0 * np.pi * x / period)
    for ox in np.arange(10.0, length, 25.0):
        side = rng.choice([-1.0, 1.0])
        oy = centre(ox) + side * rng.uniform(7.0, 12.0)
        r = rng.uniform(1.0, 2.5)
        i0, i1 = np.searchsorted(-cx, [-(ox + r + 1.0), -(ox - r - 1.0)])
        j0, j1 = np.searchsorted(-cy, [-(oy + r + 1.0), -(oy - r - 1.0)])
        X, Y = np.meshgrid(cx[i0:i1], cy[j0:j1], indexing="ij")
        free[i0:i1, j0:j1] &= (X - ox) ** 2 + (Y - oy) ** 2 > r * r
    from scipy import ndimage
    dist = (ndimage.distance_transform_edt(free) * resolution).astype(np.float32)
    geom = capi.PqpGridGeometry(rows, cols, resolution, lx, ly, pos[0], pos[1])
    kg = K.GridGeom(rows, cols, resolution, lx, ly, pos[0], pos[1])
    xs = np.arange(0.0, length + 1e-9, 1.0)
    return dict(x=xs, y=centre(xs), dist=dist, geom=geom, kgeom=kg, length=length)


def road_spline(road, every=1.0):
    """the road's centre line as a spline table: knots every `every` metres of chord length"""
    k = max(1, int(round(every)))
    x, y = road["x"][::k], road["y"][::k]
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    tab, ext = K.pack_spline(sx, sy)
    return dict(s=s, x=x, y=y, sx=sx, sy=sy, tab=tab, ext=ext, length=float(s[-1]))


def road_points(road, every=20.0):
    """input points of the chain along the road (bSpline's control points), start and target states at its ends"""
    k = int(round(every))
    x, y = road["x"][::k], road["y"][::k]
    pts = np.column_stack([x, y])
    h0 = np.arctan2(y[1] - y[0], x[1] - x[0])
    h1 = np.arctan2(y[-1] - y[-2], x[-1] - x[-2])
    return pts, np.array([x[0] + 0.1, y[0] + 0.1, h0 + 0.02]), np.array([x[-1], y[-1], h1])


def with_option(h, value):
    h.set_option(capi.OPT_LONG_LINES, value)
    return h
