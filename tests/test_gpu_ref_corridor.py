"""The corridor, projection and footprint kernels against what the REFERENCE'S OWN CODE computed on the same inputs
(tests/golden/reference_corridor.npz, recorded by tests/ref_corridor.py from the reference's unmodified sources; nothing but the golden
files is read here).  The sibling GPU tests of these kernels compare with Python restatements of the reference; a misreading shared by a
restatement and the kernel written from it passes there and fails here.  The grid lookup under Map::getObstacleDistance is the one piece of
the record that is a restatement (grid_map is third-party and not available): see tests/test_ref_corridor.py.

Tolerances are the sibling tests', taken from them: test_gpu_corridor._compare / test_gpu_corridor_on_states._compare for the bounds (restated),
test_gpu_corridor.test_reference_states_and_initial_error for the states, test_gpu_project_points.TOL and its `ambiguous` exemption,
test_gpu_chain.test_clearance_lookup_on_the_device (equality), test_gpu_footprint._agree / TOL.  `free` is compared exactly except on states
where a RECORDED clearance is within 1e-5 of its circle's radius (ref_corridor.footprint_near: at most 2 % of a scene's states,
asserted there).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import corridor_oracle as K
import project_util as P
import ref_corridor as RC
from footprint_util import FOOTPRINT_TOL
from path_optimizer_2_amd import capi
from project_util import PROJECT_TOL
from shared_util import capi_geom

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=16, max_n=256)
    yield h
    h.close()


@pytest.fixture(scope="module")
def ref():
    return RC.reference()


@pytest.fixture(scope="module")
def cs():
    c = RC.cases()
    c["tables"] = {k: K.pack_spline(sx, sy) for k, (sx, sy) in c["splines"].items()}      # (the restated fit is the reference's bit for bit)
    return c


def _corridor_prm(handle, car):
    fl, rl, w, m = RC.CARS[car]
    return handle.corridor_params(front_length=fl, rear_length=rl, car_width=w, safety_margin=m)


def _compare(got, n_valid_got, bounds, blocked_row):
    """the rule of test_gpu_corridor._compare and test_gpu_corridor_on_states._compare, with the record in the oracle's place: n_valid exact,
    NaN where NaN, > 99 % of the entries within 1e-9, any other one off by a whole 0.05 / 0.3 m search step"""
    assert n_valid_got == len(bounds), (n_valid_got, len(bounds))
    rows = np.vstack([bounds[:, :6], blocked_row[None, :6]]) if len(blocked_row) else bounds[:, :6]
    g_rows = got[:len(rows)]
    nan = np.isnan(rows)
    assert np.array_equal(nan, np.isnan(g_rows))
    diff = np.abs(g_rows[~nan] - rows[~nan])
    exact = diff < 1e-9
    off = diff[~exact]
    assert exact.mean() > 0.99, (exact.mean(), off)
    for d in off:
        assert min(abs(d - 0.05 * k) for k in range(1, 8)) < 1e-9 or min(abs(d - 0.3 * k) for k in range(1, 4)) < 1e-9, d


@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_reference_states(handle, ref, cs, name):
    ln, _, _, ds_small, ds_large, dynamic, _ = RC.CORRIDOR_CASES[name]
    tab, ext = cs["tables"][ln]
    want = ref[f"corridor_{name}_states"]
    got, count, _ = handle.reference_states(tab[None], ext[None], np.array([cs["lines"][ln][3]]), RC.CAP, ds_small=ds_small, ds_large=ds_large, dynamic=dynamic)
    assert count[0] == len(want)
    np.testing.assert_allclose(got[0, :len(want)], want, rtol=0, atol=1e-11)
    assert np.all(got[0, len(want):] == 0.0)


def test_reference_states_of_a_line_of_zero_length(handle, ref, cs):
    """buildReferenceFromSpline builds nothing within FLAGS_epsilon of zero length (reference_path_impl.cpp:316-319)"""
    tab, ext = cs["tables"]["a"]
    k = len(RC.ZERO_LENGTHS)
    got, count, _ = handle.reference_states(np.repeat(tab[None], k, 0), np.repeat(ext[None], k, 0), np.array(RC.ZERO_LENGTHS), 8)
    assert count.tolist() == [max(int(v), 0) for v in ref["zero_length_count"]]
    assert np.all(got[:3] == 0.0)


@pytest.mark.parametrize("ln", ["a", "b", "l"])
def test_initial_error(handle, ref, cs, ln):
    tab, ext = cs["tables"][ln]
    start = ref[f"line_{ln}_start"]
    k = len(start)
    _, _, err = handle.reference_states(np.repeat(tab[None], k, 0), np.repeat(ext[None], k, 0), np.full(k, cs["lines"][ln][3]), 4, start=start)
    np.testing.assert_allclose(err[:, 0], ref[f"line_{ln}_init_offset"], rtol=0, atol=1e-12)
    want = [K.constrain_angle(float(s[2]) - float(ref[f"line_{ln}_init_heading"][0])) for s in start]
    np.testing.assert_allclose(err[:, 1], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_corridor_bounds(handle, ref, cs, name):
    ln, layer, car, _, _, _, _ = RC.CORRIDOR_CASES[name]
    tab, ext = cs["tables"][ln]
    dist, g = cs["layers"][layer]
    states = ref[f"corridor_{name}_states"]
    got, nv = handle.corridor_bounds(states[None], tab[None], ext[None], dist, capi_geom(g), prm=_corridor_prm(handle, car))
    _compare(got[0], int(nv[0]), ref[f"corridor_{name}_bounds"], ref[f"corridor_{name}_blocked_row"])


@pytest.mark.parametrize("name", list(RC.CORRIDOR_CASES))
def test_corridor_bounds_on_states(handle, ref, cs, name):
    ln, layer, car, _, _, _, _ = RC.CORRIDOR_CASES[name]
    tab, ext = cs["tables"][ln]
    dist, g = cs["layers"][layer]
    states, dpsi = ref[f"corridor_{name}_states"], ref[f"corridor_{name}_d_heading"]
    st = np.zeros((1, len(states), 5)); st[0, :len(dpsi), 4] = dpsi
    got, nv = handle.corridor_bounds_on_states(states[None], st, tab[None], ext[None], dist, capi_geom(g), prm=_corridor_prm(handle, car), n_of=[len(dpsi)])
    _compare(got[0], int(nv[0]), ref[f"corridor_{name}_on_states_bounds"], ref[f"corridor_{name}_on_states_blocked_row"])


@pytest.mark.parametrize("ln", ["a", "b", "l"])
def test_project_points(handle, ref, cs, ln):
    """s, the projected state and l against getProjection's State and global2Local of the target in its frame"""
    tab, ext = cs["tables"][ln]
    sx, sy = cs["splines"][ln]
    length = cs["lines"][ln][3]
    tg, want = ref[f"line_{ln}_target"], ref[f"line_{ln}_projection"]
    amb = P.project_many(sx, sy, length, tg, has_heading=False)[2]
    assert amb.sum() == 0                                          # (test_gpu_project_points leaves such points out; the fixture has none)
    proj, flags = handle.project_points(tab[None], ext[None], np.array([length]), tg[None], has_heading=False)
    np.testing.assert_allclose(proj[0][:, [4, 5, 6, 0]], want, rtol=0, atol=PROJECT_TOL)
    l = [K.global2local_y(float(w[0]), float(w[1]), float(w[2]), float(t[0]), float(t[1])) for w, t in zip(want, tg)]
    np.testing.assert_allclose(proj[0][:, 1], l, rtol=0, atol=PROJECT_TOL)
    assert np.array_equal(flags[0] & P.AT_END != 0, want[:, 3] == length) and np.array_equal(flags[0] & P.BEFORE_START != 0, want[:, 3] < 0.0)
    assert (flags[0] & P.AT_END).any() and (flags[0] & P.BEFORE_START).any()


@pytest.mark.parametrize("layer", RC.LOOKUP_LAYERS)
def test_clearance_lookup(handle, ref, cs, layer):
    """pqp_clearance_device = Map::getObstacleDistance: cell centres, borders and corners, the map's edges just inside and outside, far outside"""
    import torch
    dist, g = cs["layers"][layer]
    pts = ref[f"lookup_{layer}_point"]
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_dist = t(np.transpose(np.asarray(dist)[None], (0, 2, 1)), np.float32)
    d_x, d_y, d_map = t(pts[None, :, 0], np.float64), t(pts[None, :, 1], np.float64), t(np.zeros(1), np.int32)
    out = torch.full((1, len(pts)), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p = lambda a: capi.C.c_void_p(a.data_ptr())
    geom = capi_geom(g)
    assert handle.lib.pqp_clearance_device(handle._h, 1, len(pts), p(d_x), p(d_y), p(d_dist), p(d_map), capi.C.byref(geom), p(out)) == 0
    handle.sync()
    got = out.cpu().numpy()[0]
    want = ref[f"lookup_{layer}_distance"].astype(np.float64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("mode", [capi.FOOTPRINT_CIRCLES, capi.FOOTPRINT_BOUNDING_FIRST])
@pytest.mark.parametrize("name", list(RC.FOOTPRINT_CASES))
def test_footprint_check(handle, ref, cs, name, mode):
    layer, car_name = RC.FOOTPRINT_CASES[name]
    dist, g = cs["layers"][layer]
    fl, rl, w, _ = RC.CARS[car_name]
    car = capi.PqpCarGeometry(w, rl, fl)
    circles = capi.car_circles(car)
    assert np.array_equal(circles[:, 2], ref[f"footprint_{name}_radius"])
    st = ref[f"footprint_{name}_state"]
    got = handle.footprint_check(st[None], None, np.asarray(dist), capi_geom(g), car=car, mode=mode, margin=True)
    want = ref[f"footprint_{name}_free_circles" if mode == capi.FOOTPRINT_CIRCLES else f"footprint_{name}_free_bounding"]
    near = RC.footprint_near(ref, name)
    mism = (got["free"][0] != want) & ~near
    assert not mism.any(), np.flatnonzero(mism)[:10]
    d = ref[f"footprint_{name}_distance"].astype(np.float64)[:, :6]
    np.testing.assert_allclose(got["margin"][0], (d - circles[None, :6, 2]).min(axis=1), rtol=0, atol=FOOTPRINT_TOL)
    if not near.any():
        z = np.flatnonzero(want == 0)
        assert got["first_collision"][0] == (z[0] if z.size else len(st))
