"""The reference's own corridor layer - tools.cpp, ReferencePath(Impl), CarGeometry, CollisionChecker, Map - as the tests see it:
oracle/_ref/libref_corridor.so (compiled by oracle/Makefile from the reference's unmodified sources over the stand-in headers of
oracle/stand_ins, driven through oracle/ref_corridor_shim.cpp), what it computed on the fixed inputs of cases(), recorded in
tests/golden/reference_corridor.npz by tests/golden/make_golden.py reference_corridor, and - where oracle/_ref has been built - the library
itself, which must still agree with the record bit for bit.

The grid_map lookup under Map::getObstacleDistance is NOT the reference's nor grid_map's code: grid_map is third-party and not available, so
oracle/stand_ins/grid_map_core restates it (the conventions of corridor_oracle.grid_*).  Everything above that lookup is the reference's.

Inputs come from the committed scenes (scene_a, scene_b, line_a, gridmap_obstacle) plus what cases() derives from them with fixed seeds; the
fixture stores the derived inputs next to the reference's outputs, so a test needs cases() only for the lines and the layers."""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libref_corridor.so")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "reference_corridor.npz")

# front_length, rear_length, car_width, safety_margin: the reference's flags, and the car of test_gpu_corridor.test_non_default_vehicle_parameters
CARS = {"default": (3.9, -1.0, 2.0, 0.3), "other": (3.2, -0.8, 1.8, 0.2)}
CAP = 256                    # states per corridor case the record has room for (the largest case builds 152)

# name: line, layer, car, ds_small, ds_large, dynamic segmentation, input states of updateBoundsOnInputStates short of the built ones
CORRIDOR_CASES = {
    "a_default": ("a", "a", "default", 0.15, 0.3, True, 0),
    "a_wall_other_coarse": ("a", "a_wall", "other", 0.5, 1.0, False, 5),
    "b_default_fixed": ("b", "b", "default", 0.15, 0.3, False, 7),
    "b_wall_other_coarse": ("b", "b_wall", "other", 0.5, 1.0, True, 0),
    "l_off_the_map_coarse": ("l", "a", "default", 0.5, 1.0, True, 3),
    "n_narrowing_other": ("n", "n", "other", 0.15, 0.3, True, 0),
}
ZERO_LENGTHS = (0.0, 5e-7, -5e-7, 2e-6)          # buildReferenceFromSpline returns false within FLAGS_epsilon = 1e-6 of zero
CLEARANCE_CASES = {"a": ("a", "default"), "a_wall": ("a_wall", "other"), "n": ("n", "default"), "n_other": ("n", "other")}
FOOTPRINT_CASES = {"a_other": ("a", "other"), "g": ("g", "default"), "g_other": ("g", "other")}
LOOKUP_LAYERS = ("a", "g")
CIRCLES_KEPT = 24            # footprint states whose seven circles are recorded (every state's clearances and answers are)


def _geom_of(v):
    import corridor_oracle as K
    return K.GridGeom(int(v[0]), int(v[1]), *[float(x) for x in v[2:]])


def _wall(K, dist, g, x_wall):
    """a wall across the road: every cell is at most |x - x_wall| from an obstacle (the walls of test_gpu_corridor)"""
    d = dist.copy()
    for i in range(g.rows):
        x, _ = K.grid_cell_position(g, i, 0)
        d[i, :] = np.minimum(d[i, :], np.float32(abs(x - x_wall)))
    return d


def _narrowing(K, g):
    """walls either side of y = 0 whose half gap grows along x from 0.9 m to 2.4 m: from a corridor that closes once the car's width is taken
    off, through one narrower than min_space = 0.2 m (no safety margin) and one that takes part of the safety margin, to one that takes all
    of it"""
    d = np.zeros((g.rows, g.cols), dtype=np.float32)
    for i in range(g.rows):
        for j in range(g.cols):
            x, y = K.grid_cell_position(g, i, j)
            half = 0.9 + 0.03 * (x - (g.pos_x - 0.5 * g.length_x))
            d[i, j] = np.float32(max(min(abs(y - half), abs(y + half)), 0.0)) if abs(y) < half else np.float32(0.0)
    return d


_CASES = None


def cases():
    """The fixed inputs: lines {name: (knots_s, knots_x, knots_y, length)}, layers {name: (dist [rows][cols] float32 in Fortran order,
    GridGeom)}, and the derived inputs of record() (seeded), keyed as the fixture stores them.  Computed once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    import corridor_oracle as K
    import distance_util as D
    fa, fb, fl = (np.load(os.path.join(GOLDEN_DIR, n + ".npz")) for n in ("scene_a", "scene_b", "line_a"))
    lines = {"a": (fa["knots_s"], fa["knots_x"], fa["knots_y"], float(fa["length"])),
             "b": (fb["knots_s"], fb["knots_x"], fb["knots_y"], float(fb["length"])),
             "l": (fl["raw_s"], fl["raw_x"], fl["raw_y"], float(fl["raw_s"][-1]))}
    g = _geom_of(fa["geom"])
    assert np.array_equal(fa["geom"], fb["geom"])
    ks = np.linspace(-22.0, 26.0, 13)                                   # straight along y = 0, knots every 4 m
    lines["n"] = (ks - ks[0], ks, np.zeros_like(ks), 45.5)                       # its last states have their front circle off the map
    kr = np.random.default_rng(75)                                      # a line on which libm's pow(v, 2) is not v * v at two of its states: "k"
    ks_k = np.cumsum(kr.uniform(2, 6, 9)); ks_k -= ks_k[0]
    lines["k"] = (ks_k, np.cumsum(kr.uniform(1, 4, 9)), np.cumsum(kr.normal(size=9)), float(ks_k[-1]))
    splines = {k: (K.spline_fit(s, x), K.spline_fit(s, y)) for k, (s, x, y, _) in lines.items()}
    layers = {"a": fa["dist"], "b": fb["dist"], "n": _narrowing(K, g)}
    for k in ("a", "b"):
        sx, _ = splines[k]
        layers[k + "_wall"] = _wall(K, layers[k], g, K.spline_eval(sx, 0.6 * lines[k][3]))
    layers = {k: (np.asfortranarray(d, dtype=np.float32), g) for k, d in layers.items()}
    occ, res = D.reference_map()
    layers["g"] = (np.asfortranarray(D.distance_layer(occ, res)), K.GridGeom(occ.shape[0], occ.shape[1], res, occ.shape[0] * res, occ.shape[1] * res, 3.0, -2.0))

    rng = np.random.default_rng(20201)
    inp = {}
    pi = math.pi
    edge_angles = np.array([0.0, pi, -pi, np.nextafter(pi, 4.0), np.nextafter(-pi, -4.0), pi / 2, -pi / 2, 3 * pi / 2 + 0.1, -3 * pi / 2 - 0.1, 2 * pi])
    for name, (ln, _, _, _, _, _, _) in CORRIDOR_CASES.items():
        inp[f"corridor_{name}_d_heading"] = rng.uniform(-0.5, 0.5, CAP)
    st_k = K.build_reference_from_spline(*splines["k"], lines["k"][3])
    inp["line_k_at_s"] = np.ascontiguousarray(st_k[sorted(set(range(0, len(st_k), 8)) | {3, 146}), 0])      # heading and curvature only
    for ln, (s, x, y, length) in lines.items():
        if ln in ("n", "k"):
            continue
        sx, sy = splines[ln]

        def at(s0, off):
            h = math.atan2(K.spline_deriv(sy, 1, s0), K.spline_deriv(sx, 1, s0))
            return K.spline_eval(sx, s0) - off * math.sin(h), K.spline_eval(sy, s0) + off * math.cos(h), h

        # left and right of the line, beyond both ends, and on it
        s0 = np.concatenate([rng.uniform(-3.0, length + 3.0, 24), rng.uniform(0.0, length, 6), [0.0, length, -2.0, length + 2.0]])
        off = np.concatenate([rng.uniform(-6.0, 6.0, 24), np.zeros(6), [1.5, -1.5, 0.0, 0.0]])
        pts = np.array([at(a, b) for a, b in zip(s0, off)])
        inp[f"line_{ln}_target"] = np.ascontiguousarray(pts[:, :2])
        inp[f"line_{ln}_target_s"] = s0
        inp[f"line_{ln}_hint"] = s0 + np.where(np.arange(len(s0)) % 2 == 0, 1.0, -1.0) * rng.uniform(0.2, 2.5, len(s0))       # hints on both sides
        # the call pattern of updateBounds: the normal through a point ahead of / behind s0, limit s0 + 5, hints s0 + front / rear length; and a tilted one
        inp[f"line_{ln}_angle"] = pts[:, 2] + pi / 2 + np.where(np.arange(len(s0)) % 3 == 0, rng.uniform(-0.3, 0.3, len(s0)), 0.0)
        inp[f"line_{ln}_dir_max_s"] = s0 + 5.0
        inp[f"line_{ln}_dir_hint"] = s0 + np.where(np.arange(len(s0)) % 2 == 0, 3.9, -1.0)
        inp[f"line_{ln}_at_s"] = np.concatenate([rng.uniform(-2.0, length + 2.0, 40), s[:8], [0.0, length, -1.5, length + 1.5]])
        x0, y0, h0 = at(0.0, 0.0)                                          # vehicle start states round the line's first point, either side of it
        inp[f"line_{ln}_start"] = np.column_stack([x0 + rng.uniform(-1.0, 1.0, 8), y0 + rng.uniform(-1.0, 1.0, 8), h0 + rng.uniform(-1.0, 1.0, 8)])
    inp["pairs_a"] = rng.uniform(-40.0, 40.0, (50, 2)); inp["pairs_b"] = rng.uniform(-40.0, 40.0, (50, 2))
    inp["pairs_b"][:5] = inp["pairs_a"][:5]
    frame = np.column_stack([rng.uniform(-30, 30, 60), rng.uniform(-30, 30, 60), rng.uniform(-2 * pi, 2 * pi, 60)])
    frame[:len(edge_angles), 2] = edge_angles
    inp["frame"] = frame
    inp["frame_target"] = np.column_stack([rng.uniform(-30, 30, 60), rng.uniform(-30, 30, 60), rng.uniform(-2 * pi, 2 * pi, 60)])

    def spread(gm, count, spill):
        """states over the map and slightly beyond it, headings all round and on the +-pi seam"""
        st = np.column_stack([gm.pos_x + rng.uniform(-0.5 - spill, 0.5 + spill, count) * gm.length_x,
                              gm.pos_y + rng.uniform(-0.5 - spill, 0.5 + spill, count) * gm.length_y, rng.uniform(-pi, pi, count)])
        st[:len(edge_angles), 2] = edge_angles
        return st

    sxa, sya = splines["a"]
    on_a = np.array([[K.spline_eval(sxa, v), K.spline_eval(sya, v), math.atan2(K.spline_deriv(sya, 1, v), K.spline_deriv(sxa, 1, v))] for v in np.arange(0.0, 24.0, 0.8)])
    for name, (layer, _) in CLEARANCE_CASES.items():
        if layer == "n":
            xs = np.arange(-24.0, 24.01, 1.0)
            st = np.concatenate([np.column_stack([xs, np.zeros_like(xs), np.zeros_like(xs)]), np.column_stack([xs, np.full_like(xs, 0.1), np.full_like(xs, pi)]),
                                 np.column_stack([xs, np.full_like(xs, -0.05), rng.uniform(-0.2, 0.2, len(xs))]),
                                 np.column_stack([xs[::3], np.full_like(xs[::3], 0.6), np.full_like(xs[::3], pi / 2)])])      # beside a wall
        else:
            st = np.concatenate([on_a, spread(g, 80, 0.03)])
        inp[f"clearance_{name}_state"] = st
    for name, (layer, _) in FOOTPRINT_CASES.items():
        inp[f"footprint_{name}_state"] = spread(layers[layer][1], 100, 0.04 if layer == "g" else 0.02)
    for layer in LOOKUP_LAYERS:
        inp[f"lookup_{layer}_point"] = lookup_points(K, layers[layer][1], rng)
    _CASES = dict(lines=lines, splines=splines, layers=layers, inputs=inp)
    return _CASES


def lookup_points(K, g, rng):
    """where a grid lookup goes wrong: cell centres, cell borders, the map's edges and corners just inside, on and just outside, far outside,
    and random points"""
    pts = []
    cells = [(0, 0), (g.rows - 1, g.cols - 1), (0, g.cols - 1), (g.rows - 1, 0), (1, 1), (g.rows // 2, g.cols // 2), (g.rows - 2, 3), (7, g.cols - 2)]
    cells += [(int(rng.integers(0, g.rows)), int(rng.integers(0, g.cols))) for _ in range(4)]
    h = 0.5 * g.resolution
    for ix, iy in cells:
        cx, cy = K.grid_cell_position(g, ix, iy)
        pts.append((cx, cy))
        for ox, oy in ((h, 0.0), (-h, 0.0), (0.0, h), (0.0, -h), (h, h), (-h, -h), (h, -h)):
            pts.append((cx + ox, cy + oy))
            pts.append((np.nextafter(cx + ox, np.inf), np.nextafter(cy + oy, -np.inf)))
            pts.append((np.nextafter(cx + ox, -np.inf), np.nextafter(cy + oy, np.inf)))
    ex = (g.pos_x - 0.5 * g.length_x, g.pos_x + 0.5 * g.length_x)
    ey = (g.pos_y - 0.5 * g.length_y, g.pos_y + 0.5 * g.length_y)
    around = lambda v: (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf), v + 1e-9, v - 1e-9, v + 0.05, v - 0.05, v + 0.15, v - 0.15)
    for x in [v for e in ex for v in around(e)]:
        for y in [v for e in ey for v in around(e)] + [g.pos_y, g.pos_y + 1.03]:
            pts.append((x, y))
    for y in [v for e in ey for v in around(e)]:
        for x in (g.pos_x, g.pos_x - 2.57):
            pts.append((x, y))
    pts += [(1e3, 0.0), (0.0, -1e3), (1e9, 1e9)]
    pts += list(zip(g.pos_x + rng.uniform(-0.52, 0.52, 120) * g.length_x, g.pos_y + rng.uniform(-0.52, 0.52, 120) * g.length_y))
    return np.array(pts, dtype=np.float64)


def built():
    return os.path.exists(LIB)


def car_of(name, dynamic=True):
    return np.array(list(CARS[name]) + [1.0 if dynamic else 0.0])


_LIBRARY = None


def library():
    global _LIBRARY
    if _LIBRARY is None:
        lib = C.CDLL(LIB)
        p, d, i = C.c_void_p, C.c_double, C.c_int
        lib.ref_line_new.restype = p; lib.ref_line_new.argtypes = [i, p, p, p]
        lib.ref_line_free.argtypes = [p]
        lib.ref_map_new.restype = p; lib.ref_map_new.argtypes = [i, i, d, d, d, d, d, p]
        lib.ref_map_free.argtypes = [p]
        lib.ref_flag_defaults.argtypes = [p]
        lib.ref_heading_curvature.argtypes = [p, i, p, p, p]
        lib.ref_distance.argtypes = [i, p, p, p]
        lib.ref_transform.argtypes = [i, i, p, p, p]
        lib.ref_projection.argtypes = [p, i, p, d, d, p]
        lib.ref_projection_newton.argtypes = [p, i, p, d, p, p]
        lib.ref_directional_projection.argtypes = [p, i, p, p, d, d, p]
        lib.ref_directional_projection_newton.argtypes = [p, i, p, p, p, p, p]
        lib.ref_corridor.restype = i; lib.ref_corridor.argtypes = [p, d, d, d, p, p, i, p, i, p, p, p, p, p]
        lib.ref_clearance.argtypes = [i, p, p, p, p]
        lib.ref_footprint.argtypes = [i, p, p, p, p, p, p]
        lib.ref_obstacle_distance.argtypes = [p, i, p, p, p]
        _LIBRARY = lib
    return _LIBRARY


def _a(x, dtype=np.float64):
    return np.ascontiguousarray(x, dtype=dtype)


class Line:
    def __init__(self, s, x, y):
        s, x, y = _a(s), _a(x), _a(y)
        self.h = library().ref_line_new(len(s), s.ctypes.data, x.ctypes.data, y.ctypes.data)

    def close(self):
        library().ref_line_free(self.h)


class Layer:
    def __init__(self, dist, g):
        flat = _a(np.asarray(dist).reshape(-1, order="F"), np.float32)          # column major: cell (ix, iy) at iy * rows + ix
        self.h = library().ref_map_new(g.rows, g.cols, g.resolution, g.length_x, g.length_y, g.pos_x, g.pos_y, flat.ctypes.data)

    def close(self):
        library().ref_map_free(self.h)

    def distance(self, points):
        pts = _a(points)
        d = np.zeros(len(pts)); inside = np.zeros(len(pts), np.uint8)
        library().ref_obstacle_distance(self.h, len(pts), pts.ctypes.data, d.ctypes.data, inside.ctypes.data)
        return d, inside


def corridor(line, max_s, ds_small, ds_large, car, layer=None, d_heading=None):
    """ref_corridor -> dict(count, states [count][5], kept, bounds [kept][10], blocked, blocked_row [10])"""
    states = np.zeros((CAP, 5)); bounds = np.zeros((CAP, 10)); row = np.zeros(10)
    kept, blocked = C.c_int(0), C.c_int(0)
    car = _a(car)
    dh = None if d_heading is None else _a(d_heading)
    n = library().ref_corridor(line.h, max_s, ds_small, ds_large, car.ctypes.data, None if layer is None else layer.h, 0 if dh is None else len(dh),
                               None if dh is None else dh.ctypes.data, CAP, states.ctypes.data, bounds.ctypes.data, C.byref(kept), C.byref(blocked), row.ctypes.data)
    assert n <= CAP, n
    return dict(count=n, states=states[:max(n, 0)].copy(), kept=kept.value, bounds=bounds[:kept.value].copy(), blocked=blocked.value, blocked_row=row)


def _f32(d):
    """Map::getObstacleDistance returns a float layer's value as a double: kept as the float it is"""
    f = d.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), d, equal_nan=True)
    return f


def record():
    """Everything the tests compare against, computed now by oracle/_ref/libref_corridor.so (which must have been built: `make -C oracle ref`)."""
    lib = library()
    c = cases()
    out = {k: v for k, v in c["inputs"].items()}
    lines = {k: Line(s, x, y) for k, (s, x, y, _) in c["lines"].items()}
    layers = {k: Layer(d, g) for k, (d, g) in c["layers"].items()}
    flags = np.zeros(5); lib.ref_flag_defaults(flags.ctypes.data)
    out["flag_defaults"] = flags.copy()

    for layer in LOOKUP_LAYERS:                              # ---- the stand-in map's lookup
        d, inside = layers[layer].distance(out[f"lookup_{layer}_point"])
        out[f"lookup_{layer}_distance"], out[f"lookup_{layer}_inside"] = _f32(d), inside

    for ln in ("a", "b", "l", "k"):                          # ---- tools.cpp
        h, length = lines[ln].h, c["lines"][ln][3]
        at_s = _a(out[f"line_{ln}_at_s"]); hd = np.zeros(len(at_s)); cv = np.zeros(len(at_s))
        lib.ref_heading_curvature(h, len(at_s), at_s.ctypes.data, hd.ctypes.data, cv.ctypes.data)
        out[f"line_{ln}_heading"], out[f"line_{ln}_curvature"] = hd, cv
        if ln == "k":
            continue
        tg = _a(out[f"line_{ln}_target"]); n = len(tg)
        for tag, start_s in (("", 0.0), ("_from5", 5.0), ("_degenerate", length + 1.0)):
            o = np.zeros((n, 4)); lib.ref_projection(h, n, tg.ctypes.data, length, start_s, o.ctypes.data)
            out[f"line_{ln}_projection{tag}"] = o[:4].copy() if tag == "_degenerate" else o         # (one answer whatever the target)
        hint = _a(out[f"line_{ln}_hint"])
        o = np.zeros((n, 4)); lib.ref_projection_newton(h, n, tg.ctypes.data, length, hint.ctypes.data, o.ctypes.data)
        out[f"line_{ln}_projection_newton"] = o
        ang, mx, dhint = _a(out[f"line_{ln}_angle"]), _a(out[f"line_{ln}_dir_max_s"]), _a(out[f"line_{ln}_dir_hint"])
        o = np.zeros((n, 4)); lib.ref_directional_projection_newton(h, n, tg.ctypes.data, ang.ctypes.data, mx.ctypes.data, dhint.ctypes.data, o.ctypes.data)
        out[f"line_{ln}_directional_newton"] = o
        o = np.zeros((n, 4)); lib.ref_directional_projection(h, n, tg.ctypes.data, ang.ctypes.data, length, 0.0, o.ctypes.data)
        out[f"line_{ln}_directional"] = o
        # PathOptimizer::processInitState and setReferencePathLength (path_optimizer.cpp:73-104; the file itself needs the solver's headers) put
        # together here from the reference's primitives: State{xs(s), ys(s)} (getProjection's max_s <= start_s return), getHeading, global2Local,
        # distance, getProjection
        ends = np.zeros((2, 4)); hd2 = np.zeros(2); cv2 = np.zeros(2); at2 = _a([0.0, length])
        lib.ref_projection(h, 1, tg.ctypes.data, 0.0, 0.0, ends[0:1].ctypes.data)
        lib.ref_projection(h, 1, tg.ctypes.data, length, length, ends[1:2].ctypes.data)
        lib.ref_heading_curvature(h, 2, at2.ctypes.data, hd2.ctypes.data, cv2.ctypes.data)
        start = _a(out[f"line_{ln}_start"]); k = len(start)
        first = _a(np.tile([ends[0, 0], ends[0, 1], hd2[0]], (k, 1)))
        loc = np.zeros((k, 3)); lib.ref_transform(k, 0, start.ctypes.data, first.ctypes.data, loc.ctypes.data)
        dist = np.zeros(k); start_xy, first_xy = _a(start[:, :2]), _a(first[:, :2])
        lib.ref_distance(k, start_xy.ctypes.data, first_xy.ctypes.data, dist.ctypes.data)
        out[f"line_{ln}_init_offset"] = np.where(loc[:, 1] < 0.0, dist, -dist)
        out[f"line_{ln}_init_heading"] = hd2[:1].copy()                       # initial_heading_error = constrainAngle(start heading - this)
        last = _a(np.tile([ends[1, 0], ends[1, 1], hd2[1]], (n, 1))); tg3 = _a(np.column_stack([tg, np.zeros(n)]))
        loc = np.zeros((n, 3)); lib.ref_transform(n, 0, last.ctypes.data, tg3.ctypes.data, loc.ctypes.data)
        out[f"line_{ln}_reference_length"] = np.where(loc[:, 0] > 0.0, length, out[f"line_{ln}_projection"][:, 3])
    a, b = _a(out["pairs_a"]), _a(out["pairs_b"]); o = np.zeros(len(a))
    lib.ref_distance(len(a), a.ctypes.data, b.ctypes.data, o.ctypes.data)
    out["pairs_distance"] = o
    fr, tg = _a(out["frame"]), _a(out["frame_target"])
    for tag, to_global in (("local2global", 1), ("global2local", 0)):
        o = np.zeros((len(fr), 3)); lib.ref_transform(len(fr), to_global, fr.ctypes.data, tg.ctypes.data, o.ctypes.data)
        out[tag] = o

    for name, (ln, layer, car, ds_small, ds_large, dynamic, short) in CORRIDOR_CASES.items():        # ---- ReferencePath
        length = c["lines"][ln][3]
        r = corridor(lines[ln], length, ds_small, ds_large, car_of(car, dynamic), layers[layer])
        assert 3 <= r["count"] <= 200, (name, r["count"])
        dh = out[f"corridor_{name}_d_heading"] = out[f"corridor_{name}_d_heading"][:r["count"] - short]
        r2 = corridor(lines[ln], length, ds_small, ds_large, car_of(car, dynamic), layers[layer], d_heading=dh)
        assert np.array_equal(r2["states"], r["states"])
        key = f"corridor_{name}_"
        out[key + "states"], out[key + "bounds"], out[key + "blocked_row"] = r["states"], r["bounds"], r["blocked_row"] if r["blocked"] else np.zeros(0)
        out[key + "on_states_bounds"], out[key + "on_states_blocked_row"] = r2["bounds"], r2["blocked_row"] if r2["blocked"] else np.zeros(0)
        # the clearance at every built state, for the tests' count of states that sit on the 0.5 m test
        out[key + "state_distance"] = _f32(layers[layer].distance(r["states"][:, 3:5])[0])
    out["zero_length_count"] = np.array([corridor(lines["a"], v, 0.15, 0.3, car_of("default"))["count"] for v in ZERO_LENGTHS], dtype=np.int64)

    for name, (layer, car) in CLEARANCE_CASES.items():       # ---- getClearanceWithDirectionStrict
        st = _a(out[f"clearance_{name}_state"]); o = np.zeros((len(st), 2)); cr = car_of(car)
        lib.ref_clearance(len(st), st.ctypes.data, cr.ctypes.data, layers[layer].h, o.ctypes.data)
        out[f"clearance_{name}_bound"] = o
        out[f"clearance_{name}_distance"] = _f32(layers[layer].distance(st[:, :2])[0])

    for name, (layer, car) in FOOTPRINT_CASES.items():       # ---- CarGeometry, CollisionChecker
        st = _a(out[f"footprint_{name}_state"]); n = len(st); cr = car_of(car)
        circles = np.zeros((n, 7, 3)); f0 = np.zeros(n, np.uint8); f1 = np.zeros(n, np.uint8)
        lib.ref_footprint(n, st.ctypes.data, cr.ctypes.data, layers[layer].h, circles.ctypes.data, f0.ctypes.data, f1.ctypes.data)
        key = f"footprint_{name}_"
        out[key + "circles"], out[key + "free_circles"], out[key + "free_bounding"] = circles[:CIRCLES_KEPT].copy(), f0, f1
        d, inside = layers[layer].distance(circles.reshape(-1, 3)[:, :2])
        out[key + "distance"], out[key + "inside"], out[key + "radius"] = _f32(d.reshape(n, 7)), inside.reshape(n, 7), circles[0, :, 2].copy()

    lib.ref_flag_defaults(flags.ctypes.data)                 # every call put the defaults back
    assert np.array_equal(flags, out["flag_defaults"])
    for v in lines.values():
        v.close()
    for v in layers.values():
        v.close()
    return out


_REFERENCE = None


def reference():
    """The recorded values; where oracle/_ref is built, first checked bit for bit (NaN where NaN) against what it computes now.  Loaded once."""
    global _REFERENCE
    if _REFERENCE is None:
        want = dict(np.load(GOLDEN))
        if built():
            live = record()
            assert sorted(live) == sorted(want)
            for k in want:
                assert live[k].shape == want[k].shape and live[k].dtype == want[k].dtype and live[k].tobytes() == want[k].tobytes(), k
        for v in want.values():
            v.setflags(write=False)
        _REFERENCE = want
    return _REFERENCE


NEAR_TOL = 1e-5              # footprint_util.near_threshold's: a clearance this close to the value it is tested against may fall either way on the device


def footprint_near(ref, name):
    """[n] bool: some circle of the state (the six or the bounding one) has |recorded clearance - radius| < NEAR_TOL"""
    d = ref[f"footprint_{name}_distance"].astype(np.float64)
    return (np.abs(d - ref[f"footprint_{name}_radius"][None]) < NEAR_TOL).any(axis=1)
