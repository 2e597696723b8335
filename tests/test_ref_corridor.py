"""The Python restatements of the corridor family - oracle/corridor_oracle.py, tests/corridor_states_util.py, tests/footprint_util.py -
against what the reference's own code computes on the same inputs: tests/golden/reference_corridor.npz, recorded from
oracle/_ref/libref_corridor.so (the reference's unmodified tools.cpp, ReferencePath(Impl), CarGeometry, CollisionChecker and Map over the
stand-in headers of oracle/stand_ins; tests/ref_corridor.py).  Where oracle/_ref is built, ref_corridor.reference() first holds the record to
a live run bit for bit; everywhere else the record alone is read.

ONE PIECE STAYS A RESTATEMENT: the grid lookup under Map::getObstacleDistance.  grid_map is a third-party library that is neither here nor in
the reference tree, so the stand-in GridMap restates it, in the conventions corridor_oracle.py cites from grid_map 1.6.x.  The first test
holds the two restatements to each other; neither has been held to grid_map itself.  Everything above that lookup is the reference's code.

Floating values are compared bit for bit throughout: no tolerance is needed once the restatements square a number the way the compiled
reference does (pow(x, 2) is compiled to x * x; Python's math.pow(x, 2) calls libm's pow, which is not always x * x to the last place)."""
import math

import numpy as np
import pytest

import corridor_oracle as K
import corridor_states_util as S
import footprint_util as F
import ref_corridor as RC

NEAR_TOL = RC.NEAR_TOL
NEAR_SHARE = 0.02


def _bits(got, want, what):
    """bit for bit, NaN where NaN, -0.0 where -0.0; says where and by how many ulps otherwise"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.int64).ravel() != want.view(np.int64).ravel())
    if bad.size:
        g, w = got.ravel()[bad], want.ravel()[bad]
        with np.errstate(all="ignore"):
            ulps = np.abs(g - w) / np.spacing(np.abs(w))
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, worst {np.nanmax(ulps):.1f} ulp, first at {bad[:5]}: {g[:5]} vs {w[:5]}")


@pytest.fixture(scope="module")
def ref():
    return RC.reference()


@pytest.fixture(scope="module")
def cs():
    return RC.cases()


def _prm(car):
    fl, rl, w, m = RC.CARS[car]
    return K.CorridorParams(front_length=fl, rear_length=rl, car_width=w, safety_margin=m)


# ---- 1. the lookup: runs first, the other comparisons mean nothing if it fails --------------------------------------------------------------
@pytest.mark.parametrize("layer", RC.LOOKUP_LAYERS)
def test_stand_in_map_lookup_is_the_oracles(ref, cs, layer):
    """cell centres, cell borders and corners (on them and an ulp either side), the map's edges and corners just inside, on and just outside,
    far outside, random points: Map::getObstacleDistance / Map::isInside over the stand-in GridMap = obstacle_distance / grid_is_inside"""
    dist, g = cs["layers"][layer]
    pts = ref[f"lookup_{layer}_point"]
    assert len(pts) > 500
    got = np.array([K.obstacle_distance(dist, g, float(x), float(y)) for x, y in pts])
    inside = np.array([K.grid_is_inside(g, float(x), float(y)) for x, y in pts])
    assert np.array_equal(inside, ref[f"lookup_{layer}_inside"].astype(bool))
    assert 0.2 < inside.mean() < 0.95 and (got[inside] > 0).any()
    _bits(got, ref[f"lookup_{layer}_distance"].astype(np.float64), layer)
    assert (got[~inside] == 0.0).all()


def test_flags_are_the_parameters_the_restatements_default_to(ref):
    p = K.CorridorParams()
    assert ref["flag_defaults"].tolist() == [p.front_length, p.rear_length, p.car_width, p.safety_margin, 1.0]
    assert ref["flag_defaults"][:4].tolist() == list(RC.CARS["default"])


# ---- 2. tools.cpp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", ["a", "b", "l", "k"])
def test_heading_and_curvature(ref, cs, ln):
    """getHeading / getCurvature inside the line, at its knots and on both extrapolations; line k: at states where squaring through libm's
    pow, as the restatement did before it was held to the reference, gives another curvature in the last place"""
    sx, sy = cs["splines"][ln]
    at_s = ref[f"line_{ln}_at_s"]
    length = cs["lines"][ln][3]
    if ln == "k":
        d = [(K.spline_deriv(sx, 1, float(s)), K.spline_deriv(sy, 1, float(s)), K.spline_deriv(sx, 2, float(s)), K.spline_deriv(sy, 2, float(s))) for s in at_s]
        through_pow = np.array([(dx * ddy - dy * ddx) / math.pow(math.pow(dx, 2) + math.pow(dy, 2), 1.5) for dx, dy, ddx, ddy in d])
        assert (through_pow != ref["line_k_curvature"]).sum() >= 1 and np.abs(through_pow - ref["line_k_curvature"]).max() < 1e-15
    else:
        assert (at_s < 0).any() and (at_s > length).any()
    _bits([K.heading(sx, sy, float(s)) for s in at_s], ref[f"line_{ln}_heading"], "heading")
    _bits([K.curvature(sx, sy, float(s)) for s in at_s], ref[f"line_{ln}_curvature"], "curvature")


def test_distance_and_the_two_transforms(ref):
    a, b = ref["pairs_a"], ref["pairs_b"]
    _bits([K.distance(*p, *q) for p, q in zip(a, b)], ref["pairs_distance"], "distance")
    assert (ref["pairs_distance"][:5] == 0.0).all()
    fr, tg = ref["frame"], ref["frame_target"]
    assert (np.abs(fr[:, 2]) > math.pi).any() and (fr[:, 2] == math.pi).any() and (fr[:, 2] == -math.pi).any()
    _bits([K.global2local_y(*f, t[0], t[1]) for f, t in zip(fr, tg)], ref["global2local"][:, 1], "global2Local.y")
    _bits([F.local2global(*f, t[0], t[1]) for f, t in zip(fr, tg)], ref["local2global"][:, :2], "local2Global")


@pytest.mark.parametrize("ln", ["a", "b", "l"])
def test_projections(ref, cs, ln):
    """getProjection (from s = 0, from s = 5, and with max_s <= start_s), getProjectionByNewton with hints on both sides, and
    getDirectionalProjectionByNewton in updateBounds' call pattern and with tilted directions: targets left and right of the line, beyond
    both ends and on it"""
    sx, sy = cs["splines"][ln]
    length = cs["lines"][ln][3]
    tg, s0 = ref[f"line_{ln}_target"], ref[f"line_{ln}_target_s"]
    assert (s0 < 0).any() and (s0 > length).any()
    for tag, start_s in (("", 0.0), ("_from5", 5.0)):
        want = ref[f"line_{ln}_projection{tag}"]
        got = np.array([K.projection(sx, sy, float(x), float(y), length, start_s) for x, y in tg])
        _bits(got, want[:, 3], "getProjection.s" + tag)
        _bits([K.spline_eval(sx, s) for s in got], want[:, 0], "getProjection.x" + tag)
        assert (want[:, 3] == length).any() and (want[:, 3] < 0.0).any() if tag == "" else True
    deg = ref[f"line_{ln}_projection_degenerate"]
    assert (deg[:, 3] == 0.0).all() and K.projection(sx, sy, 1.0, 2.0, length, length + 1.0) == 0.0
    _bits(deg[:, 0], [K.spline_eval(sx, length + 1.0)] * 4, "State{xs(start_s), ..}")
    hint = ref[f"line_{ln}_hint"]
    assert (hint > s0).any() and (hint < s0).any()
    _bits([K.projection_newton(sx, sy, float(x), float(y), length, float(h)) for (x, y), h in zip(tg, hint)], ref[f"line_{ln}_projection_newton"][:, 3], "byNewton.s")
    want = ref[f"line_{ln}_directional_newton"]
    got = np.array([K.directional_projection_newton(sx, sy, float(x), float(y), float(a), float(m), float(h))
                    for (x, y), a, m, h in zip(tg, ref[f"line_{ln}_angle"], ref[f"line_{ln}_dir_max_s"], ref[f"line_{ln}_dir_hint"])])
    _bits(got, want[:, [0, 1, 3]], "directionalByNewton x, y, s")
    # getDirectionalProjection has no restatement of its own (nothing on the device calls it): its coarse scan never records a minimum
    # (tools.cpp:146-149 assigns the wrong way round), so it is the Newton run from the scan's last sample
    last = 2.0 * math.floor(length / 2.0)
    got = np.array([K.directional_projection_newton(sx, sy, float(x), float(y), float(a), length, last) for (x, y), a in zip(tg, ref[f"line_{ln}_angle"])])
    _bits(got, ref[f"line_{ln}_directional"][:, [0, 1, 3]], "directional x, y, s")


@pytest.mark.parametrize("ln", ["a", "b", "l"])
def test_init_state_and_reference_length(ref, cs, ln):
    """process_init_state and reference_length against the same steps put together from the reference's primitives (ref_corridor.record)"""
    sx, sy = cs["splines"][ln]
    length = cs["lines"][ln][3]
    start = ref[f"line_{ln}_start"]
    got = np.array([K.process_init_state(sx, sy, *[float(v) for v in st]) for st in start])
    _bits(got[:, 0], ref[f"line_{ln}_init_offset"], "initial_offset")
    assert (got[:, 0] > 0).any() and (got[:, 0] < 0).any()
    _bits(got[:, 1], [K.constrain_angle(float(st[2]) - float(ref[f"line_{ln}_init_heading"][0])) for st in start], "initial_heading_error")
    want = ref[f"line_{ln}_reference_length"]
    assert (want == length).any() and (want < length).any()
    _bits([K.reference_length(sx, sy, length, float(x), float(y)) for x, y in ref[f"line_{ln}_target"]], want, "setReferencePathLength")


# ---- 3. ReferencePath -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_reference_states(ref, cs, name):
    ln, _, _, ds_small, ds_large, dynamic, _ = RC.CORRIDOR_CASES[name]
    sx, sy = cs["splines"][ln]
    want = ref[f"corridor_{name}_states"]
    got = K.build_reference_from_spline(sx, sy, cs["lines"][ln][3], ds_small, ds_large, dynamic)
    assert len(got) == len(want)
    _bits(got, want, name)


def test_a_line_of_zero_length_has_no_states(ref, cs):
    """buildReferenceFromSpline returns false, and builds nothing, within FLAGS_epsilon of zero (reference_path_impl.cpp:316)"""
    sx, sy = cs["splines"]["a"]
    assert ref["zero_length_count"].tolist() == [-1, -1, -1, 1]
    for max_s, want in zip(RC.ZERO_LENGTHS, ref["zero_length_count"]):
        assert len(K.build_reference_from_spline(sx, sy, max_s)) == max(int(want), 0)


def _rows(bounds, blocked):
    return np.vstack([bounds, np.asarray(blocked)[None]]) if blocked is not None else bounds


@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_update_bounds(ref, cs, name):
    """updateBounds on the states buildReferenceFromSpline built: kept count, blocked flag, the bounds of every kept state and of the one that
    blocked, and the front and rear centres"""
    ln, layer, car, _, _, _, _ = RC.CORRIDOR_CASES[name]
    sx, sy = cs["splines"][ln]
    dist, g = cs["layers"][layer]
    states, want, want_blocked = ref[f"corridor_{name}_states"], ref[f"corridor_{name}_bounds"], ref[f"corridor_{name}_blocked_row"]
    prm = _prm(car)
    got, kept, blocked = K.update_bounds_improved(states, sx, sy, dist, g, prm)
    assert kept == len(want) and (blocked is not None) == (len(want_blocked) > 0)
    assert (kept < len(states)) == (blocked is not None)
    _bits(_rows(got, blocked), _rows(want[:, :6], want_blocked[:6] if len(want_blocked) else None), name)
    centres = np.array([[x + prm.front_length * math.cos(h), y + prm.front_length * math.sin(h), x + prm.rear_length * math.cos(h), y + prm.rear_length * math.sin(h)]
                        for _, _, h, x, y in states[:kept]])
    _bits(centres, want[:, 6:], name + " centres")


@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_update_bounds_on_input_states(ref, cs, name):
    ln, layer, car, _, _, _, short = RC.CORRIDOR_CASES[name]
    sx, sy = cs["splines"][ln]
    dist, g = cs["layers"][layer]
    states, dpsi = ref[f"corridor_{name}_states"], ref[f"corridor_{name}_d_heading"]
    assert len(dpsi) == len(states) - short
    want, want_blocked = ref[f"corridor_{name}_on_states_bounds"], ref[f"corridor_{name}_on_states_blocked_row"]
    got, kept, blocked = S.update_bounds_on_input_states(states, dpsi, sx, sy, dist, g, _prm(car))
    assert kept == len(want) and (blocked is not None) == (len(want_blocked) > 0)
    _bits(_rows(got, blocked), _rows(want[:, :6], want_blocked[:6] if len(want_blocked) else None), name)


def test_the_corridor_cases_block_where_they_are_meant_to(ref):
    kept = {name: (len(ref[f"corridor_{name}_bounds"]), len(ref[f"corridor_{name}_states"])) for name in RC.CORRIDOR_CASES}
    assert kept["a_default"][0] == kept["a_default"][1]                                    # a free road
    for name in ("a_wall_other_coarse", "b_wall_other_coarse", "b_default_fixed", "l_off_the_map_coarse", "n_narrowing_other"):
        assert 3 < kept[name][0] < kept[name][1], name                                     # a wall, an obstacle, the map's edge
    # on the narrowing road every regime of the hard safety margin occurs (car "other": margin 0.2, min_space 0.2)
    b = ref["corridor_n_narrowing_other_bounds"]
    space = b[:, 5] - b[:, 4]
    assert (space < 0.2).any() and ((space > 0.2) & (space < 0.6)).any() and (space > 1.0).any()


@pytest.mark.parametrize("name", list(RC.CLEARANCE_CASES))
def test_clearance_strict(ref, cs, name):
    """getClearanceWithDirectionStrict at states on and off the road: near an obstacle (the {0, 0} return), off the map, headings on the +-pi
    seam, a corridor that closes, one narrower than min_space"""
    layer, car = RC.CLEARANCE_CASES[name]
    dist, g = cs["layers"][layer]
    st, want = ref[f"clearance_{name}_state"], ref[f"clearance_{name}_bound"]
    got = np.array([K.clearance_strict(float(x), float(y), float(h), dist, g, _prm(car))[::-1] for x, y, h in st])
    _bits(got, want, name)
    d = ref[f"clearance_{name}_distance"]
    closed = (want == 0.0).all(axis=1)
    assert ((d <= 0.5) & closed).any() and ((d > 0.5) & ~closed).any()
    if layer == "n":
        space = want[:, 1] - want[:, 0]
        assert ((d > 0.5) & closed).any() and ((space > 0) & (space < 0.2)).any()        # closed by the car's width; narrower than min_space


# ---- 4. CarGeometry and CollisionChecker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.FOOTPRINT_CASES))
def test_footprint(ref, cs, name):
    layer, car = RC.FOOTPRINT_CASES[name]
    dist, g = cs["layers"][layer]
    fl, rl, w, _ = RC.CARS[car]
    circles = F.car_circles(w, rl, fl)
    st = ref[f"footprint_{name}_state"]
    _bits(circles[:, 2], ref[f"footprint_{name}_radius"], "radii")
    for i in range(RC.CIRCLES_KEPT):
        _bits(np.array(F.global_circles(circles, *[float(v) for v in st[i]])), ref[f"footprint_{name}_circles"][i], ("circles", i))
    free = [F.collision_free(dist, g, circles, *[float(v) for v in s]) for s in st]
    improved = [F.collision_free_improved(dist, g, circles, *[float(v) for v in s]) for s in st]
    assert np.array_equal(free, ref[f"footprint_{name}_free_circles"].astype(bool))
    assert np.array_equal(improved, ref[f"footprint_{name}_free_bounding"].astype(bool))
    assert 0.05 < np.mean(free) < 0.95
    d = np.array([F.clearances(dist, g, circles, *[float(v) for v in s])[0] for s in st])
    _bits(d, ref[f"footprint_{name}_distance"][:, :6].astype(np.float64), "clearances")


# ---- 5. what the GPU tests may leave out ------------------------------------------------------------------------------------------------------
def test_few_states_sit_on_a_threshold(ref):
    """tests/test_gpu_ref_corridor.py compares discrete outputs exactly except on states where a recorded clearance is within NEAR_TOL of the
    value it is tested against - a circle's radius, or the 0.5 m search radius at the state itself: at most 2 % of any scene's states,
    counted here from the reference's recorded clearances alone"""
    for name in RC.FOOTPRINT_CASES:
        near = RC.footprint_near(ref, name)
        assert near.mean() <= NEAR_SHARE, (name, near.mean())
    for key in [f"corridor_{n}_state_distance" for n in RC.CORRIDOR_CASES] + [f"clearance_{n}_distance" for n in RC.CLEARANCE_CASES]:
        near = np.abs(ref[key].astype(np.float64) - 0.5) < NEAR_TOL
        assert near.mean() <= NEAR_SHARE, (key, near.mean())
