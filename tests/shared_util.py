"""Small helpers more than one test file needs: the grid geometry in its two forms and the two bit-for-bit array comparisons."""
import numpy as np

import corridor_oracle as K
from path_optimizer_2_amd import capi


def capi_geom(g):
    """the oracle's GridGeom as the ABI's PqpGridGeometry"""
    return capi.PqpGridGeometry(g.rows, g.cols, g.resolution, g.length_x, g.length_y, g.pos_x, g.pos_y)


def oracle_geom(c):
    """the oracle's GridGeom of a synth scene or of a PqpGridGeometry"""
    if isinstance(c, dict):
        return K.GridGeom(c["rows"], c["cols"], c["resolution"], c["length"][0], c["length"][1], c["pos"][0], c["pos"][1])
    return K.GridGeom(c.rows, c.cols, c.resolution, c.length_x, c.length_y, c.pos_x, c.pos_y)


def same_bytes(a, b):
    """same shape and the same bytes: NaN payloads and the sign of zero count"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits(a, b):
    """bit for bit, NaNs (whose sign and payload are no part of IEEE arithmetic) in the same places"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
