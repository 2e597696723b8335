"""The restatement of pqp_distance_layer (include/pqp.h): the reference's cv::distanceTransform(obstacle, dist, CV_DIST_L2,
CV_DIST_MASK_PRECISE); dist *= resolution (src/test/demo.cpp:104-113) as the ABI pins it, bit for bit:
    dist = fl32( fl32(sqrt(d2)) * fl32(resolution) ),  d2 = least integer (dr)^2 + (dc)^2 to an obstacle cell (byte 0) of the map,
with d2 = rows^2 + cols^2 for a map without obstacle.  Arrays in the numpy orientation [n_maps][rows][cols] (or 2-D)."""
import numpy as np


def to_float(d2, resolution):
    """the ABI's conversion of exact squared cell distances (the double square root rounded to float is the correctly rounded one below 2^50)"""
    d2 = np.asarray(d2, dtype=np.int64)
    assert d2.size == 0 or int(d2.max()) < 2 ** 50
    return np.sqrt(d2.astype(np.float64)).astype(np.float32) * np.float32(resolution)


def _d2_one(grid):
    from scipy import ndimage
    rows, cols = grid.shape
    free = grid != 0
    if free.all():
        return np.full(grid.shape, rows * rows + cols * cols, dtype=np.int64)
    _, idx = ndimage.distance_transform_edt(free, return_indices=True)
    r, c = np.indices(grid.shape)
    return (idx[0] - r).astype(np.int64) ** 2 + (idx[1] - c).astype(np.int64) ** 2


def d2_exact(grid):
    """exact squared cell distance to the nearest obstacle: scipy's nearest-obstacle indices, the squares formed in integers"""
    g = np.asarray(grid)
    return _d2_one(g) if g.ndim == 2 else np.stack([_d2_one(m) for m in g])


def distance_layer(grid, resolution):
    return to_float(d2_exact(grid), resolution)


def d2_brute(grid):
    """O(cells x obstacles): the definition itself, for small maps"""
    g = np.asarray(grid)
    if g.ndim == 3:
        return np.stack([d2_brute(m) for m in g])
    rows, cols = g.shape
    obs = np.argwhere(g == 0)
    if len(obs) == 0:
        return np.full(g.shape, rows * rows + cols * cols, dtype=np.int64)
    r, c = np.indices(g.shape)
    d = (r[..., None] - obs[:, 0]) ** 2 + (c[..., None] - obs[:, 1]) ** 2
    return d.min(axis=-1).astype(np.int64)


def occupancy_of(dist):
    """the occupancy grid behind a layer: 0 where the layer is 0 (an obstacle cell), 255 elsewhere"""
    return np.where(np.asarray(dist) == 0, 0, 255).astype(np.uint8)


def random_maps(rng, count=200, max_rows=40, max_cols=37):
    """small maps of every density from 0 to 100 %, plus corner cells and maps without obstacle"""
    out = []
    for k in range(count):
        rows, cols = int(rng.integers(2, max_rows + 1)), int(rng.integers(2, max_cols + 1))
        kind = k % 10
        if kind == 0:
            g = np.full((rows, cols), 255, np.uint8)
        elif kind == 1:
            g = np.full((rows, cols), 255, np.uint8)
            g[[(0, 0), (0, -1), (-1, 0), (-1, -1)][(k // 10) % 4]] = 0
        else:
            dens = rng.uniform(0.0, 1.0) if kind < 8 else [0.0, 1.0][kind - 8]
            g = np.where(rng.uniform(size=(rows, cols)) < dens, 0, rng.integers(1, 256, size=(rows, cols))).astype(np.uint8)
        out.append(g)
    return out


def reference_map():
    """tests/golden/gridmap_obstacle.npz -> (grid [rows][cols] uint8 in the numpy orientation, 0 = obstacle; resolution)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gridmap_obstacle.npz"))
    rows, cols = int(z["rows"]), int(z["cols"])
    free = np.unpackbits(z["free_bits"])[:rows * cols].reshape(cols, rows).T
    return np.where(free, 255, 0).astype(np.uint8), float(z["resolution"])
