"""Test helper: pqp_project_points restated in Python on top of oracle/corridor_oracle.py (spline_eval / spline_deriv / projection /
global2local_y), with the trace of the search that says where the oracle's own decisions are within rounding."""
import math

import numpy as np

import corridor_oracle as K

AT_END, BEFORE_START, NOT_CONVERGED, NOT_FINITE = 1, 2, 4, 8
PROJECT_TOL = 1e-9                # tests/test_gpu_corridor.py's rule for pqp_reference_length: the same search, ocml against libm in sqrt / atan2 / sin / cos
MAX_LENGTH = 1048576.0           # include/pqp.h: a longer (or infinite) line is refused like a point that is not finite


def _dist(sx, sy, s, x, y):
    return K.distance(K.spline_eval(sx, s), K.spline_eval(sy, s), x, y)


def trace(sx, sy, length, x, y):
    """the search of getProjection (tools.cpp:66-126) step by step: dict(s, coarse = the distances of the 1 m scan, end = the end point's,
    steps = the Newton steps taken (empty where the end point took over), converged); s is asserted to be corridor_oracle.projection's"""
    coarse, k = [], 0
    while float(k) <= length:
        coarse.append(_dist(sx, sy, float(k), x, y))
        k += 1
    end = _dist(sx, sy, length, x, y)
    best = int(np.argmin(coarse))                  # the first of equal minima, as the strict `<` keeps it
    steps, converged = [], True
    if end < coarse[best]:
        s = length
    else:
        cur = prev = min(float(best), length)
        converged = False
        for _ in range(20):
            px, py = K.spline_eval(sx, cur), K.spline_eval(sy, cur)
            dx, dy = K.spline_deriv(sx, 1, cur), K.spline_deriv(sy, 1, cur)
            ddx, ddy = K.spline_deriv(sx, 2, cur), K.spline_deriv(sy, 2, cur)
            j = (px - x) * dx + (py - y) * dy
            h = dx * dx + (px - x) * ddx + dy * dy + (py - y) * ddy
            cur -= j / h
            steps.append(cur - prev)
            if abs(cur - prev) < 1e-5:
                converged = True
                break
            prev = cur
        s = min(cur, length)
    assert s == K.projection(sx, sy, x, y, length, 0.0)
    return dict(s=s, coarse=coarse, end=end, steps=steps, converged=converged)


def ambiguous(tr):
    """a decision of the oracle's own search that rounding could turn: a non-zero gap below 1e-9 between the two smallest coarse distances
    or between the end distance and the minimum, or a Newton step within 1e-12 of the 1e-5 it is compared with"""
    c = sorted(tr["coarse"])
    if len(c) > 1 and 0.0 < c[1] - c[0] < 1e-9:
        return True
    if 0.0 < abs(tr["end"] - c[0]) < 1e-9:
        return True
    return any(abs(abs(d) - 1e-5) < 1e-12 for d in tr["steps"])


def state_at(sx, sy, s):
    """x, y, getHeading, getCurvature of the line at s (tools.cpp:32-44)"""
    dx, dy = K.spline_deriv(sx, 1, s), K.spline_deriv(sy, 1, s)
    ddx, ddy = K.spline_deriv(sx, 2, s), K.spline_deriv(sy, 2, s)
    return K.spline_eval(sx, s), K.spline_eval(sy, s), math.atan2(dy, dx), (dx * ddy - dy * ddx) / math.pow(dx * dx + dy * dy, 1.5)


def project(sx, sy, length, x, y, heading=None, with_trace=False):
    """one output row of pqp_project_points and its flag: s, l, t, d_heading, x_p, y_p, heading_p, k_p"""
    vals = (x, y) if heading is None else (x, y, heading)
    if not all(math.isfinite(v) for v in vals) or length >= MAX_LENGTH:
        return (np.full(8, np.nan), NOT_FINITE) + ((None,) if with_trace else ())
    tr = None
    if length > 0.0:
        tr = trace(sx, sy, length, x, y)
        s = tr["s"]
    else:
        s = 0.0                                        # getProjection's max_s <= start_s (tools.cpp:72-74), NaN included
    if not math.isfinite(s):
        return (np.full(8, np.nan), NOT_FINITE) + ((tr,) if with_trace else ())
    xp, yp, hp, kp = state_at(sx, sy, s)
    l = K.global2local_y(xp, yp, hp, x, y)
    t = (x - xp) * math.cos(hp) + (y - yp) * math.sin(hp)                      # global2Local(...).x  tools.cpp:60
    dh = 0.0 if heading is None else K.constrain_angle(heading - hp)
    flag = (AT_END if s == length else 0) | (BEFORE_START if s < 0.0 else 0) | (NOT_CONVERGED if tr is not None and not tr["converged"] else 0)
    return (np.array([s, l, t, dh, xp, yp, hp, kp]), flag) + ((tr,) if with_trace else ())


def project_many(sx, sy, length, points, has_heading=None):
    """points [q][>= 2] -> (proj [q][8], flags [q], ambiguous [q])"""
    points = np.asarray(points, dtype=np.float64)
    if has_heading is None:
        has_heading = points.shape[1] >= 3
    proj, flags, amb = np.zeros((len(points), 8)), np.zeros(len(points), np.int32), np.zeros(len(points), bool)
    for i, p in enumerate(points):
        proj[i], flags[i], tr = project(sx, sy, length, float(p[0]), float(p[1]), float(p[2]) if has_heading else None, with_trace=True)
        amb[i] = tr is not None and ambiguous(tr)
    return proj, flags, amb


def point_at(sx, sy, s, off):
    """the point `off` to the left of the line at s (the line extrapolated where s lies outside it)"""
    h = math.atan2(K.spline_deriv(sy, 1, s), K.spline_deriv(sx, 1, s))
    return K.spline_eval(sx, s) - off * math.sin(h), K.spline_eval(sy, s) + off * math.cos(h)


def scattered_points(c, length, count, seed):
    """`count` seeded points around line c (corridor_util.build): at s0 in U[-3, length + 3], offset U[-6, 6], a random heading"""
    rng = np.random.default_rng(seed)
    pts = np.zeros((count, 3))
    for i in range(count):
        s0, off = rng.uniform(-3.0, length + 3.0), rng.uniform(-6.0, 6.0)
        pts[i, :2] = point_at(c["sx"], c["sy"], s0, off)
        pts[i, 2] = rng.uniform(-math.pi, math.pi)
    return pts


def write_case(path, s, x, y, points):
    """the file tests/cpp/project_demo.cpp reads"""
    with open(path, "wb") as f:
        f.write(np.array([len(s), len(points)], np.int32).tobytes())
        for a in (s, x, y, points):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
