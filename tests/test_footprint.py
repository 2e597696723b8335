"""Host side of pqp_footprint_check (include/pqp.h): the footprint circles pqp_car_circles hands the kernel, against the restatement of
CarGeometry::setCircles (tests/footprint_util.py) and hand values; and the restatement of CollisionChecker itself on hand-built maps.
No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import corridor_oracle as K
import footprint_util as F
from path_optimizer_2_amd import capi


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def test_default_car_circles_bit_for_bit(hip_lib):
    car = capi.car_default_geometry(hip_lib)
    assert (car.width, car.rear_length, car.front_length) == (2.0, -1.0, 3.9)      # planning_flags.cpp:10,18,20
    got = capi.car_circles(car, hip_lib)
    assert _same(got, F.car_circles())
    corner, middle = math.sqrt(2) * 0.5, math.sqrt(4 + 1.45 ** 2) / 2
    assert got[6, 0] == 1.45 and got[6, 1] == 0.0 and got[6, 2] == math.sqrt(2.45 ** 2 + 1 ** 2)
    assert (got[:4, 2] == corner).all() and (got[4:6, 2] == middle).all()
    assert got[:4, :2].tolist() == [[-0.5, -0.5], [-0.5, 0.5], [3.4, -0.5], [3.4, 0.5]]
    assert got[4, 0] == pytest.approx(2.175, abs=1e-15) and got[5, 0] == pytest.approx(0.725, abs=1e-15)      # 1.45 +- (4.9 - 2) / 4


@pytest.mark.parametrize("geom", [(1.8, -0.9, 4.2), (2.3, 1.1, 3.6), (1.0, 0.0, 5.0)])
def test_other_car_circles_bit_for_bit(hip_lib, geom):
    car = capi.PqpCarGeometry(*geom)
    assert _same(capi.car_circles(car, hip_lib), F.car_circles(*geom))


@pytest.mark.parametrize("bad", [(math.nan, -1.0, 3.9), (2.0, math.inf, 3.9), (2.0, -1.0, -math.inf)])
def test_car_circles_refuses_a_geometry_that_is_not_finite(hip_lib, bad):
    out = np.zeros((7, 3))
    assert hip_lib.pqp_car_circles(C.byref(capi.PqpCarGeometry(*bad)), out.ctypes.data_as(C.c_void_p)) == -1
    assert hip_lib.pqp_car_circles(None, out.ctypes.data_as(C.c_void_p)) == -1


# ---- the restatement on hand-built maps -------------------------------------------------------------------------------------------
RES = 0.05


def _geom():
    return K.GridGeom.make(10.0, 10.0, RES)                # 200 x 200 cells, x and y in (-5, 5]


def _point_layer(g, points):
    """float32 layer of the exact distance from every cell centre to the nearest of `points` (an analytic obstacle field)"""
    cx = 0.5 * g.length_x - 0.5 * g.resolution - g.resolution * np.arange(g.rows)
    cy = 0.5 * g.length_y - 0.5 * g.resolution - g.resolution * np.arange(g.cols)
    d = np.full((g.rows, g.cols), np.inf)
    for px, py in points:
        d = np.minimum(d, np.hypot(cx[:, None] - px, cy[None, :] - py))
    return d.astype(np.float32)


def test_empty_map_is_free():
    g = _geom()
    dist = np.full((g.rows, g.cols), 50.0, np.float32)
    circles = F.car_circles()
    for x, y, h in [(0.0, 0.0, 0.0), (-1.0, 0.5, 1.0), (0.3, -0.2, -2.5)]:
        assert F.collision_free(dist, g, circles, x, y, h)
        assert F.collision_free_improved(dist, g, circles, x, y, h)
        assert F.margin(dist, g, circles, x, y, h) == pytest.approx(50.0 - circles[4, 2])


def test_obstacle_cell_under_one_corner_collides():
    g = _geom()
    circles = F.car_circles()
    ix, iy = K.grid_index(g, -0.5, -0.5)                   # the cell under the rear right circle's centre (state at the origin, heading 0)
    occ = np.full((g.rows, g.cols), 255, np.uint8)
    occ[ix, iy] = 0
    import distance_util as D
    dist = D.distance_layer(occ, RES)
    assert not F.collision_free(dist, g, circles, 0.0, 0.0, 0.0)
    assert not F.collision_free_improved(dist, g, circles, 0.0, 0.0, 0.0)
    assert F.margin(dist, g, circles, 0.0, 0.0, 0.0) < 0.0
    # the same car a metre ahead clears it
    assert F.collision_free(dist, g, circles, 1.0, 0.0, 0.0) and F.collision_free_improved(dist, g, circles, 1.0, 0.0, 0.0)


def test_a_circle_off_the_map_collides():
    g = _geom()
    circles = F.car_circles()
    dist = np.full((g.rows, g.cols), 50.0, np.float32)
    x = 5.0 - 3.4 + 0.1                                   # the front circles' centres 0.1 m beyond the +x edge, the rest inside
    assert not F.collision_free(dist, g, circles, x, 0.0, 0.0)
    assert F.collision_free(dist, g, circles, x - 0.2, 0.0, 0.0)
    # (Map::getObstacleDistance is 0 outside: the margin counts such a circle as touching an obstacle)
    assert F.margin(dist, g, circles, x, 0.0, 0.0) == pytest.approx(-circles[2, 2])
    for bad in [(math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, math.inf), (0.0, 0.0, math.nan)]:
        assert not F.collision_free(dist, g, circles, *bad) and not F.collision_free_improved(dist, g, circles, *bad)


def test_bounding_first_can_say_free_where_the_circles_collide():
    """The corner circles poke out of the bounding circle (|rr - bounding centre| + r = 2.72 > 2.646): an obstacle between the two radii
    along that direction is clear of the bounding circle and inside the rear right circle."""
    g = _geom()
    circles = F.car_circles()
    bc, rr = circles[6, :2], circles[0, :2]
    u = (rr - bc) / np.linalg.norm(rr - bc)
    p = bc + 2.68 * u
    dist = _point_layer(g, [tuple(p)])
    assert F.collision_free_improved(dist, g, circles, 0.0, 0.0, 0.0)
    assert not F.collision_free(dist, g, circles, 0.0, 0.0, 0.0)
    # Improved takes the exact path once the bounding circle is not clear: then both agree
    dist2 = _point_layer(g, [tuple(bc + 2.5 * u)])
    assert not F.collision_free_improved(dist2, g, circles, 0.0, 0.0, 0.0) and not F.collision_free(dist2, g, circles, 0.0, 0.0, 0.0)


def test_check_first_collision_and_ragged_counts():
    g = _geom()
    circles = F.car_circles()
    dist = np.full((g.rows, g.cols), 50.0, np.float32)
    st = np.zeros((2, 5, 7))
    st[:, :, 0] = np.linspace(-1.0, 3.0, 5)                  # the last two states put the front circles off the map
    free, first, mg = F.check(st, np.array([5, 3], np.int32), [dist], g, None, circles, 0)
    assert free.tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 0, 0]] and first.tolist() == [3, 3]
    assert (mg[1, 3:] == 0).all()
