"""pqp_footprint_check on the GPU against the restatement of CollisionChecker (tests/footprint_util.py; reference
src/tools/collision_checker.cpp:17-58, car_geometry.cpp:38-72): random states on the reference's own map and on synth maps in both
modes, many maps per call, ragged counts, states off the map or not finite, long paths and a large batch, the check behind the
device chain, and bad arguments.  Run with -m gpu on an MI355X.

sin / cos on the device may differ from libm by an ulp and the lookup rounds to float, so `free` is compared exactly except on states
where some circle's clearance is within 1e-5 of its radius (fewer than 0.1 % of them), and `margin` to 1e-5."""
import ctypes as C
import math

import numpy as np
import pytest

import chain_util
import distance_util as D
import footprint_util as F
from path_optimizer_2_amd import capi
from path_optimizer_2_amd.synth import make_scene
from shared_util import oracle_geom

pytestmark = pytest.mark.gpu
TOL = F.FOOTPRINT_TOL


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=128)
    yield h
    h.close()


def _geom(rows, cols, res, pos=(0.0, 0.0)):
    return capi.PqpGridGeometry(rows, cols, res, rows * res, cols * res, pos[0], pos[1])


@pytest.fixture(scope="module")
def reference_layer():
    occ, res = D.reference_map()
    return D.distance_layer(occ, res), _geom(occ.shape[0], occ.shape[1], res, pos=(3.0, -2.0))


@pytest.fixture(scope="module")
def synth_layers():
    cs = [make_scene(seed=s) for s in range(4)]
    c0 = cs[0]
    return np.stack([c["dist"] for c in cs]), _geom(c0["rows"], c0["cols"], c0["resolution"])


def _random_states(rng, g, B, n, stride=7, spill=0.05):
    """states spread over the map and slightly beyond it (spill: fraction of the length), headings all round"""
    st = np.zeros((B, n, stride))
    st[:, :, 0] = g.pos_x + rng.uniform(-0.5 - spill, 0.5 + spill, (B, n)) * g.length_x
    st[:, :, 1] = g.pos_y + rng.uniform(-0.5 - spill, 0.5 + spill, (B, n)) * g.length_y
    st[:, :, 2] = rng.uniform(-math.pi, math.pi, (B, n))
    st[:, :, 3:] = rng.normal(size=(B, n, stride - 3))          # the other SlState fields: not read
    return st


def _agree(got, states, n_of, dists, g, map_of, car, mode):
    kg = oracle_geom(g)
    circles = capi.car_circles(car)
    free, first, mg = F.check(states, n_of, dists, kg, map_of, circles, mode)
    near = F.near_threshold(states, n_of, dists, kg, map_of, circles, TOL)
    counted = int(sum(states.shape[1] if n_of is None else n_of[b] for b in range(states.shape[0])))
    assert near.sum() <= 0.001 * counted, (int(near.sum()), counted)
    mism = (got["free"] != free) & ~near
    assert not mism.any(), np.argwhere(mism)[:10]
    np.testing.assert_allclose(got["margin"], mg, rtol=0, atol=TOL)
    for b in range(states.shape[0]):
        nb = states.shape[1] if n_of is None else int(n_of[b])
        if not near[b, :nb].any():
            assert got["first_collision"][b] == first[b], b
        # the device's own convention, whatever the exemptions: first index whose free is 0
        z = np.flatnonzero(got["free"][b, :nb] == 0)
        assert got["first_collision"][b] == (z[0] if z.size else nb), b
    return free


@pytest.mark.parametrize("mode", [capi.FOOTPRINT_CIRCLES, capi.FOOTPRINT_BOUNDING_FIRST])
def test_reference_map_random_states(handle, reference_layer, mode):
    dist, g = reference_layer
    rng = np.random.default_rng(7 + mode)
    states = _random_states(rng, g, 12, 150)
    n_of = rng.integers(100, 151, 12).astype(np.int32)
    car = capi.car_default_geometry()
    got = handle.footprint_check(states, n_of, dist, g, car=car, mode=mode, margin=True)
    free = _agree(got, states, n_of, [dist], g, None, car, mode)
    assert 0.01 < free.sum() / n_of.sum() < 0.99            # both answers occur


@pytest.mark.parametrize("mode", [capi.FOOTPRINT_CIRCLES, capi.FOOTPRINT_BOUNDING_FIRST])
def test_synth_maps_selected_by_map_of(handle, synth_layers, mode):
    dists, g = synth_layers
    rng = np.random.default_rng(11 + mode)
    B, n = 16, 120
    states = _random_states(rng, g, B, n, spill=0.02)
    map_of = rng.integers(0, dists.shape[0], B).astype(np.int32)
    car = capi.PqpCarGeometry(1.8, -0.9, 4.2)
    got = handle.footprint_check(states, None, dists, g, map_of=map_of, car=car, mode=mode, margin=True)
    _agree(got, states, None, list(dists), g, map_of, car, mode)
    # the map matters: the same states on map 0 alone give other answers
    other = handle.footprint_check(states, None, dists[:1], g, car=car, mode=mode)
    assert (other["free"] != got["free"]).any()


def test_bounding_first_differs_where_the_reference_does(handle, reference_layer):
    """both modes on the same states: BOUNDING_FIRST reports a collision only where CIRCLES does (its exact path is CIRCLES, and the bounding
    centre lies between the circles' centres); the converse fails through the corners, as the restatement says state by state (_agree)"""
    dist, g = reference_layer
    rng = np.random.default_rng(3)
    states = _random_states(rng, g, 8, 256, spill=0.0)
    a = handle.footprint_check(states, None, dist, g, mode=capi.FOOTPRINT_CIRCLES)
    b = handle.footprint_check(states, None, dist, g, mode=capi.FOOTPRINT_BOUNDING_FIRST)
    assert not ((b["free"] == 0) & (a["free"] == 1)).any()


def test_ragged_counts_zeros_beyond_and_clear_paths(handle, synth_layers):
    _, g = synth_layers
    dist = np.full((g.rows, g.cols), 30.0, np.float32)        # nothing near: every state in the middle is free
    B, n = 6, 300
    states = np.zeros((B, n, 7))
    states[:, :, 0] = np.linspace(-10.0, 10.0, n)
    states[:, :, 2] = 0.3
    n_of = np.array([0, 1, 2, 255, 256, 300], np.int32)
    for mode in (capi.FOOTPRINT_CIRCLES, capi.FOOTPRINT_BOUNDING_FIRST):
        got = handle.footprint_check(states, n_of, dist, g, mode=mode, margin=True)
        assert got["first_collision"].tolist() == n_of.tolist()
        for b in range(B):
            assert (got["free"][b, :n_of[b]] == 1).all() and (got["free"][b, n_of[b]:] == 0).all()
            assert (got["margin"][b, n_of[b]:] == 0).all() and (got["margin"][b, :n_of[b]] > 28.0).all()


def test_off_the_map_and_not_finite_states_collide(handle, synth_layers):
    _, g = synth_layers
    dist = np.full((g.rows, g.cols), 30.0, np.float32)
    bad = [(g.length_x, 0.0, 0.0), (0.0, -g.length_y, 1.0), (0.5 * g.length_x - 1.0, 0.0, 0.0),     # off / partly off the map
           (math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, math.inf), (0.0, 0.0, math.nan), (-math.inf, -math.inf, 0.0)]
    states = np.zeros((1, len(bad) + 1, 3))
    states[0, :len(bad)] = bad
    for mode in (capi.FOOTPRINT_CIRCLES, capi.FOOTPRINT_BOUNDING_FIRST):
        got = handle.footprint_check(states, None, dist, g, mode=mode, margin=True)
        assert got["free"][0].tolist() == [0] * len(bad) + [1]
        assert got["first_collision"][0] == 0
        assert np.isfinite(got["margin"]).all()


def test_a_path_longer_than_a_workgroup_and_a_large_batch(handle, synth_layers):
    dists, g = synth_layers
    rng = np.random.default_rng(19)
    # one path of 3000 states: the colliding states are spread over all twelve stride steps of the workgroup
    states = _random_states(rng, g, 1, 3000, stride=3, spill=0.0)
    states[0, :2500, 1] = 0.0; states[0, :2500, 2] = 0.0
    states[0, :2500, 0] = -40.0                                # far off the map: the first 2500 collide
    got = handle.footprint_check(states, np.array([3000], np.int32), dists[:1], g, margin=True)
    assert got["first_collision"][0] == 0
    states[0, :2500, 0] = 0.0
    dist = np.full((g.rows, g.cols), 30.0, np.float32)
    got = handle.footprint_check(states[:, :2500], None, dist, g)
    assert got["first_collision"][0] == 2500 and got["free"].all()
    got = handle.footprint_check(states, None, dists[:1], g, margin=True)
    sample = np.sort(rng.choice(3000, 400, replace=False))
    free, _, mg = F.check(states[:, sample], None, [dists[0]], oracle_geom(g), None, capi.car_circles(), 0)
    near = F.near_threshold(states[:, sample], None, [dists[0]], oracle_geom(g), None, capi.car_circles(), TOL)
    assert ((got["free"][:, sample] == free) | near).all()
    np.testing.assert_allclose(got["margin"][:, sample], mg, atol=TOL, rtol=0)
    # 65 536 scenarios of 80 states on four maps
    B, n = 65536, 80
    big = _random_states(rng, g, B, n, stride=3, spill=0.02)
    map_of = (np.arange(B) % 4).astype(np.int32)
    n_of = rng.integers(0, n + 1, B).astype(np.int32)
    got = handle.footprint_check(big, n_of, dists, g, map_of=map_of, mode=capi.FOOTPRINT_BOUNDING_FIRST)
    idx = np.arange(n)[None, :]
    assert (got["free"][idx >= n_of[:, None]] == 0).all()
    first = np.where((got["free"] == 0) & (idx < n_of[:, None]), idx, n).min(axis=1)
    assert (got["first_collision"] == np.minimum(first, n_of)).all()
    pick = rng.choice(B, 24, replace=False)
    free, _, _ = F.check(big[pick], n_of[pick], list(dists), oracle_geom(g), map_of[pick], capi.car_circles(), 1)
    near = F.near_threshold(big[pick], n_of[pick], list(dists), oracle_geom(g), map_of[pick], capi.car_circles(), TOL)
    assert ((got["free"][pick] == free) | near).all()


# ---- behind the device chain ---------------------------------------------------------------------------------------------------------
def test_check_footprint_behind_the_chain(hip_lib):
    B = 24
    sc = chain_util.scenarios(B)
    runs = {}
    for flag in (False, True):                         # fresh handles for each: nothing carried from one call to the other
        h, hs = chain_util.handles(B)
        runs[flag] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                                     check_footprint=flag)
        h.close(); hs.close()
    a, b = runs[False], runs[True]
    for k in ("out", "n_out", "status", "stage"):
        assert np.array_equal(a[k].view(np.uint8) if a[k].dtype == np.float64 else a[k], b[k].view(np.uint8) if b[k].dtype == np.float64 else b[k]), k
    assert (b["stage"] == 0).sum() >= B // 2
    h = capi.Handle(capi.default_params(), max_batch=B, max_n=256)
    sep = h.footprint_check(b["out"], b["n_out"], sc["dist"], sc["geom"], map_of=sc["map_of"], margin=True)
    h.close()
    assert np.array_equal(sep["free"], b["free"]) and np.array_equal(sep["first_collision"], b["first_collision"])
    assert np.array_equal(sep["margin"], b["margin"])
    _agree(b, b["out"], b["n_out"], list(sc["dist"]), sc["geom"], sc["map_of"], capi.car_default_geometry(), 0)


def test_check_footprint_on_grid_reads_the_layers_built_on_the_device(hip_lib):
    B = 8
    sc = chain_util.scenarios(B)
    occ = np.stack([D.occupancy_of(d) for d in sc["dist"]])
    h, hs = chain_util.handles(B)
    got = h.optimize_path_on_grid(sc["pts"], sc["n_pts"], sc["start"], sc["target"], occ, sc["geom"], map_of=sc["map_of"], smoother=hs,
                                  check_footprint=True, footprint_mode=capi.FOOTPRINT_BOUNDING_FIRST)
    layers = np.stack([D.distance_layer(o, sc["geom"].resolution) for o in occ])
    sep = h.footprint_check(got["out"], got["n_out"], layers, sc["geom"], map_of=sc["map_of"], mode=capi.FOOTPRINT_BOUNDING_FIRST, margin=True)
    h.close(); hs.close()
    assert np.array_equal(sep["free"], got["free"]) and np.array_equal(sep["margin"], got["margin"])
    assert np.array_equal(sep["first_collision"], got["first_collision"])


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------
def test_host_entry_point_refuses_bad_arguments_and_launches_nothing(handle, synth_layers):
    dists, g = synth_layers
    B, n = 4, 10
    states = np.zeros((B, n, 7))
    dist_cm = np.ascontiguousarray(np.transpose(dists, (0, 2, 1)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good_car, good_map = capi.car_default_geometry(), np.zeros(B, np.int32)

    def call(stride=7, map_of=good_map, car=good_car, mode=0):
        free = np.full((B, n), 7, np.uint8)
        first = np.full(B, -7, np.int32)
        rc = handle.lib.pqp_footprint_check(handle._h, B, n, stride, p(states), None, p(dist_cm), dists.shape[0], p(map_of), C.byref(g),
                                            C.byref(car), mode, p(free), p(first), None)
        return rc, (free == 7).all() and (first == -7).all()

    rc, untouched = call()
    assert rc == 0 and not untouched
    for kw in (dict(map_of=np.array([0, 1, 4, 0], np.int32)), dict(map_of=np.array([0, -1, 0, 0], np.int32)), dict(stride=2),
               dict(car=capi.PqpCarGeometry(math.nan, -1.0, 3.9)), dict(car=capi.PqpCarGeometry(2.0, -1.0, math.inf)), dict(mode=2), dict(mode=-1)):
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
