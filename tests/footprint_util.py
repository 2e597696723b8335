"""CPU restatement of the reference's footprint check (test infrastructure):
  CarGeometry::setCircles / getCircles / getBoundingCircle   src/tools/car_geometry.cpp:38-72
  local2Global                                               src/tools/tools.cpp:50-55
  CollisionChecker::isSingleStateCollisionFree(Improved)     src/tools/collision_checker.cpp:17-58
The map lookups are oracle/corridor_oracle.py's (Map::getObstacleDistance, GridMap::isInside), by import."""
import math

import numpy as np

import corridor_oracle as K

FOOTPRINT_TOL = 1e-5             # the device's margins against this restatement's (tests/test_gpu_footprint.py), and near_threshold's default


def car_circles(width=2.0, rear_length=-1.0, front_length=3.9):
    """[7][3]: x, y, r of rr, rl, fr, fl, fm, rm, then the bounding circle, in the vehicle frame.  The checker's car is
    CarGeometry(FLAGS_car_width, fabs(FLAGS_rear_length), FLAGS_front_length) (collision_checker.cpp:9-14); math.pow is libm's pow."""
    back_length = abs(rear_length)
    length = front_length + back_length
    fl = (front_length, width / 2.0)
    fr = (front_length, -width / 2.0)
    rl = (-back_length, width / 2.0)
    rr = (-back_length, -width / 2.0)
    bx = (front_length - back_length) / 2.0
    br = math.sqrt(math.pow(length / 2, 2) + math.pow(width / 2, 2))
    shift = width / 4.0
    small_r = math.sqrt(2 * math.pow(shift, 2))
    large_r = math.sqrt(math.pow(width, 2) + math.pow((length - width) / 2.0, 2)) / 2
    return np.array([[rr[0] + shift, rr[1] + shift, small_r],
                     [rl[0] + shift, rl[1] - shift, small_r],
                     [fr[0] - shift, fr[1] + shift, small_r],
                     [fl[0] - shift, fl[1] - shift, small_r],
                     [bx + (length - width) / 4, 0.0, large_r],
                     [bx - (length - width) / 4, 0.0, large_r],
                     [bx, 0.0, br]])


def local2global(x, y, heading, tx, ty):
    c, s = (math.cos(heading), math.sin(heading)) if math.isfinite(heading) else (math.nan, math.nan)     # (libm: NaN for +-Inf)
    return tx * c - ty * s + x, tx * s + ty * c + y


def global_circles(circles, x, y, heading):
    """getCircles (the six) and getBoundingCircle (the last row) at the state (x, y, heading)"""
    return [(*local2global(x, y, heading, cx, cy), r) for cx, cy, r in circles]


def _circle_clear(dist, g, cx, cy, r):
    return K.grid_is_inside(g, cx, cy) and not (K.obstacle_distance(dist, g, cx, cy) < r)


def collision_free(dist, g, circles, x, y, heading):
    """isSingleStateCollisionFree; dist [rows][cols] float32.  A state that is not finite puts its circles at NaN / Inf positions: outside."""
    return all(_circle_clear(dist, g, *c) for c in global_circles(circles[:6], x, y, heading))


def collision_free_improved(dist, g, circles, x, y, heading):
    """isSingleStateCollisionFreeImproved"""
    bx, by, br = global_circles(circles[6:], x, y, heading)[0]
    if not K.grid_is_inside(g, bx, by):
        return False
    if K.obstacle_distance(dist, g, bx, by) < br:
        return collision_free(dist, g, circles, x, y, heading)
    return True


def clearances(dist, g, circles, x, y, heading):
    """Map::getObstacleDistance at the six circle centres (0 outside) and the radii"""
    cs = global_circles(circles[:6], x, y, heading)
    d = [K.obstacle_distance(dist, g, cx, cy) for cx, cy, _ in cs]
    return np.array(d), circles[:6, 2]


def margin(dist, g, circles, x, y, heading):
    d, r = clearances(dist, g, circles, x, y, heading)
    return float(np.min(d - r))


def fortran(dists):
    """the layers in column-major order: the oracle's lookup then reads a view of each instead of copying the whole layer per sample"""
    return [np.asfortranarray(d, dtype=np.float32) for d in dists]


def check(states, n_of, dists, g, map_of, circles, mode):
    """The whole entry point on the host: (free [B][n], first_collision [B], margin [B][n]) as pqp_footprint_check defines them."""
    B, n = states.shape[0], states.shape[1]
    free = np.zeros((B, n), np.uint8)
    mg = np.zeros((B, n))
    first = np.zeros(B, np.int32)
    fn = collision_free if mode == 0 else collision_free_improved
    dists = fortran(dists)
    for b in range(B):
        nb = n if n_of is None else int(n_of[b])
        dist = dists[0 if map_of is None else int(map_of[b])]
        first[b] = nb
        for i in range(nb):
            x, y, h = (float(v) for v in states[b, i, :3])
            free[b, i] = 1 if fn(dist, g, circles, x, y, h) else 0
            mg[b, i] = margin(dist, g, circles, x, y, h)
            if not free[b, i] and first[b] == nb:
                first[b] = i
    return free, first, mg


def near_threshold(states, n_of, dists, g, map_of, circles, tol=1e-5):
    """[B][n] bool: some circle (the six or the bounding one) has |clearance - r| < tol - where an ulp of sin / cos or the float rounding of
    the lookup may flip the comparison"""
    B, n = states.shape[0], states.shape[1]
    out = np.zeros((B, n), bool)
    dists = fortran(dists)
    for b in range(B):
        nb = n if n_of is None else int(n_of[b])
        dist = dists[0 if map_of is None else int(map_of[b])]
        for i in range(nb):
            x, y, h = (float(v) for v in states[b, i, :3])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(h)):
                continue
            for cx, cy, r in global_circles(circles, x, y, h):
                if abs(K.obstacle_distance(dist, g, cx, cy) - r) < tol:
                    out[b, i] = True
    return out
