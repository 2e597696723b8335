"""pqp_sample_plan on the GPU against the numpy restatement (tests/plan_util.py; tests/test_plan_sample.py holds it against a plain loop
and checks the hand case on the CPU first).  Everything is compared bit for bit - every column of `fine`, m_of, defect, excess and flags
- in both forms, the `_device` form with its outputs in sentinel-filled allocations (tests/device_form.py).

The shapes are the smallest at which the kernel can go wrong: the sample loop's tiles of 64 at M = 64, 65, 66, 71, 12 and 201, the
waypoint walk's tiles at n = 64, 65, 130 and 300 with ragged counts and a stop inside a tile, layer counts 0, 1, 2 and m in one batch,
c = 0, rows that are not finite between ordinary neighbours, a backward layer, the refine's flags mixed in one batch, and the same path
at several batch positions.  The inputs are synthetic plan rows (plan_util.synthetic) and the device's own search-then-refine output on
refine_util's seeded scenes."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import cpp_demo
import device_form as D
import plan_util as P
import refine_util as R
import search_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
KEYS = ("traj", "m_of", "defect", "excess", "flags")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _host(handle, c, r, plan=None, **kw):
    return handle.sample_plan(c["paths"], c["profile"], c["plan"] if plan is None else plan, r, dt=c["dt"], n_of=c.get("n_of"),
                              stop_before=c.get("stop_before"), **kw)


def _want(c, r, plan=None, **kw):
    return P.sample_batch(c["paths"], c["profile"], c["plan"] if plan is None else plan, r, c["dt"], c.get("n_of"), c.get("stop_before"), **kw)


def _device(handle, c, r, plan=None, count_of=None, refine_flags=None, linear=False, dt=None):
    """the device form through device_form: the outputs lie in sentinel-filled allocations with a guard band behind them"""
    paths, profile = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("paths", "profile"))
    plan = np.ascontiguousarray(c["plan"] if plan is None else plan, dtype=np.float64)
    B, n, stride = paths.shape
    m = plan.shape[1]
    opt = lambda a: None if a is None else D.to_device(a, np.int32)
    out = dict(traj=D.Out((B, P.fine_count(m, r), 8)), m_of=D.Out((B,), np.int32), defect=D.Out((B,)), excess=D.Out((B,)), flags=D.Out((B,), np.int32))
    rc = D.call(handle, "pqp_sample_plan_device", C.c_double(c["dt"] if dt is None else dt), r, int(linear), B, n, stride, D.to_device(paths),
                opt(c.get("n_of")), opt(c.get("stop_before")), D.to_device(profile), m, D.to_device(plan), opt(count_of), opt(refine_flags), *out.values())
    return (rc, out) if rc else (rc, {k: v.get() for k, v in out.items()})


def _same(a, b, where):
    for k in KEYS:
        assert same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), (where, k)


def _both_forms(handle, c, r, where, **kw):
    """host form = device form = restatement; returns the host form's"""
    want = _want(c, r, **kw)
    got = _host(handle, c, r, **kw)
    _same(got, want, (where, "host"))
    rc, dev = _device(handle, c, r, **kw)
    assert rc == 0, handle.lib.pqp_last_error()
    _same(dev, want, (where, "device"))
    return got


# ---- synthetic plans: the tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,r", ((2, 63), (2, 64), (2, 65), (8, 10), (12, 1), (3, 100)))
def test_tile_edges_of_the_sample_loop(handle, m, r):
    """M = 64, 65, 66, 71, 12 and 201 samples: one tile exactly, one sample into the second, a ragged last tile, four tiles"""
    c = P.synthetic(5, 130, m, seed=m * 1000 + r)
    assert P.fine_count(m, r) in (64, 65, 66, 71, 12, 201)
    mixed = np.array([R.REFINED, R.KEPT, R.REFINED, R.KEPT | R.INFEASIBLE, 0], np.int32)
    for kw in (dict(linear=False), dict(linear=True), dict(refine_flags=mixed)):
        got = _both_forms(handle, c, r, (m, r, kw), **kw)
        assert (got["m_of"] == P.fine_count(m, r)).all() and np.isfinite(got["traj"]).all()
    assert got["traj"][0, -1, 4] > c["profile"][0, -1, 0] and same_bits(got["traj"][0, -1, :4], c["paths"][0, -1][[0, 1, 2, 5]])      # past the path's end


@pytest.mark.parametrize("n", (64, 65, 130, 300))
def test_tile_edges_of_the_waypoint_walk(handle, n):
    """the driven counts n, n - 7, two thirds of n (a stop inside a tile) and at most 40 (n_of = n / 2 + 1, cut by the stop): for n = 300
    that is 300, 293, 200 and 40 waypoints - four tiles and most of a fifth, a ragged one, three and an eighth, less than one"""
    n_of = np.array([n, n - 7, n, n // 2 + 1], np.int32)
    stop = np.array([n, n, 2 * n // 3, 40], np.int32)
    c = P.synthetic(4, n, 8, seed=n, n_of=n_of, stop_before=stop)
    for kw in (dict(linear=False), dict(linear=True)):
        got = _both_forms(handle, c, 10, (n, kw), **kw)
        assert (got["flags"] == 0).all() and (got["m_of"] == 71).all()
    assert (np.minimum(n_of, stop) == np.array([n, n - 7, 2 * n // 3, min(n // 2 + 1, 40)])).all()


def test_layer_counts_mixed_in_one_batch_and_empty_paths(handle):
    """L = 0, 1, 2, m, a negative count and one beyond m (clamped), and c = 0 by n_of and by stop_before, each between ordinary paths"""
    m, r, B = 6, 7, 8
    n_of = np.array([130, 130, 130, 0, 130, 130, 130, 130], np.int32)
    stop = np.array([130, 130, 130, 130, 130, 0, 99, 130], np.int32)
    c = P.synthetic(B, 130, m, seed=11, n_of=n_of, stop_before=stop)
    count = np.array([0, 1, 2, m, -3, m, m + 5, m], np.int32)
    got = _both_forms(handle, c, r, "counts", count_of=count, linear=False)
    _both_forms(handle, c, r, "counts, linear", count_of=count, linear=True)
    assert got["flags"].tolist() == [P.EMPTY, 0, 0, P.EMPTY, P.EMPTY, P.EMPTY, 0, 0]
    assert got["m_of"].tolist() == [0, 1, r + 1, 0, 0, 0, P.fine_count(m, r), P.fine_count(m, r)]
    empty = got["flags"] == P.EMPTY
    assert (got["traj"][empty] == 0.0).all() and np.isnan(got["defect"][empty]).all() and np.isnan(got["excess"][empty]).all()
    assert got["defect"][1] == 0.0 and (got["traj"][1, 1:] == 0.0).all() and (got["traj"][2, r + 1:] == 0.0).all()
    # rows at i = 0 are the plan's in s and t, and t runs on by dt / r
    assert same_bits(got["traj"][7, ::r, 4], c["plan"][7, :, 4]) and same_bits(got["traj"][7, ::r, 7], np.arange(m) * np.float64(c["dt"]))


def test_rows_that_are_not_finite_leave_their_neighbours_alone(handle):
    """a path row and a plan row that are not finite, each between ordinary neighbours that keep the bits they have alone; a value that is
    not finite behind the counts, or in a column nobody reads, is not looked at"""
    m, r, B = 5, 10, 5
    n_of = np.array([130, 130, 100, 130, 130], np.int32)
    c = P.synthetic(B, 130, m, seed=23, n_of=n_of)
    count = np.array([m, m, m, m, 3], np.int32)
    alone = _host(handle, c, r, count_of=count)
    bad = dict(c, paths=c["paths"].copy(), plan=c["plan"].copy())
    bad["paths"][1, 77, 1] = math.nan                        # y of a driven row
    bad["plan"][3, 2, 6] = math.inf                          # a of a planned layer
    bad["paths"][2, 100, 0] = math.nan                       # behind n_of
    bad["plan"][4, 3, 4] = math.nan                          # behind count_of
    bad["paths"][0, 5, 3], bad["plan"][0, 1, 0], bad["plan"][0, 1, 7] = math.nan, math.inf, math.nan      # columns nobody reads
    got = _both_forms(handle, bad, r, "not finite", count_of=count)
    assert got["flags"].tolist() == [0, P.NOT_FINITE, 0, P.NOT_FINITE, 0] and got["m_of"].tolist() == [41, 0, 41, 0, 21]
    for b in (1, 3):
        assert np.isnan(got["traj"][b]).all() and np.isnan(got["defect"][b]) and np.isnan(got["excess"][b])
    for b in (0, 2, 4):
        for k in KEYS:
            assert same_bits(np.asarray(got[k][b], dtype=np.float64), np.asarray(alone[k][b], dtype=np.float64)), (b, k)


def test_a_backward_layer_stands_and_is_flagged(handle):
    m, r = 6, 4
    c = P.synthetic(3, 130, m, seed=31)
    c["plan"][1, 3, 4] = c["plan"][1, 2, 4] - 0.75
    for linear in (False, True):
        got = _both_forms(handle, c, r, ("backward", linear), linear=linear)
        assert got["flags"].tolist() == [0, P.BACKWARD, 0]
        assert (got["traj"][1, 2 * r:3 * r, 4] == c["plan"][1, 2, 4]).all() and got["traj"][1, 3 * r, 4] == c["plan"][1, 3, 4]
    assert _host(handle, c, r, count_of=np.array([m, 3, m], np.int32))["flags"].tolist() == [0, 0, 0]


def test_the_refines_flags_choose_the_kinematics_path_by_path(handle):
    """REFINED and KEPT mixed in one batch: a path's rows are what linear = 0 / linear = 1 with NULL flags give it, at any batch position"""
    m, r, B = 8, 10, 6
    c = P.synthetic(B, 130, m, seed=41)
    flags = np.array([R.REFINED, R.KEPT, R.KEPT | R.INFEASIBLE, R.REFINED, 0, R.REFINED | 8], np.int32)
    got = _both_forms(handle, c, r, "mixed", refine_flags=flags, linear=True)          # (`linear` is not read when the flags are given)
    cacc, lin = _host(handle, c, r, linear=False), _host(handle, c, r, linear=True)
    assert not same_bits(cacc["traj"], lin["traj"])
    for b in range(B):
        src = cacc if flags[b] & R.REFINED else lin
        for k in KEYS:
            assert same_bits(np.asarray(got[k][b], dtype=np.float64), np.asarray(src[k][b], dtype=np.float64)), (b, k)
    assert (lin["defect"] == 0.0).all() and (lin["traj"][:, :-1, 6] == 0.0).all() and (cacc["defect"] > 0.0).all()
    order = np.array([(5 * b + 2) % B for b in range(B)] + [0, 0, B - 1])               # a longer batch, every path somewhere else, one three times
    sel = lambda a: np.ascontiguousarray(a[order])
    moved = handle.sample_plan(sel(c["paths"]), sel(c["profile"]), sel(c["plan"]), r, dt=c["dt"], refine_flags=sel(flags))
    for at, b in enumerate(order):
        for k in KEYS:
            assert same_bits(np.asarray(moved[k][at], dtype=np.float64), np.asarray(got[k][b], dtype=np.float64)), (at, b, k)


def test_refusals_leave_the_outputs_alone(handle):
    c = P.synthetic(2, 64, 3, seed=5)
    B, n, stride = c["paths"].shape
    for dt, r, linear in ((0.0, 4, 0), (math.nan, 4, 0), (math.inf, 4, 0), (-1.0, 4, 0), (0.5, 4, 2), (0.5, 4, -1), (0.5, 0, 0), (0.5, -1, 0)):
        out = dict(traj=D.Out((B, P.fine_count(3, max(r, 1)), 8)), m_of=D.Out((B,), np.int32), defect=D.Out((B,)), excess=D.Out((B,)),
                   flags=D.Out((B,), np.int32))
        rc = D.call(handle, "pqp_sample_plan_device", C.c_double(dt), r, linear, B, n, stride, D.to_device(c["paths"]), None, None,
                    D.to_device(c["profile"]), 3, D.to_device(c["plan"]), None, None, *out.values())
        assert rc == ERR_INVALID and handle.lib.pqp_last_error().decode().startswith("pqp_sample_plan:"), (dt, r, linear)
        assert all(o.untouched() for o in out.values()), (dt, r, linear)
    with pytest.raises(capi.PqpError, match="pqp error -1: pqp_sample_plan:"):
        _host(handle, c, 0)
    # defect and excess are optional
    out = dict(traj=D.Out((B, 9, 8)), m_of=D.Out((B,), np.int32), flags=D.Out((B,), np.int32))
    rc = D.call(handle, "pqp_sample_plan_device", C.c_double(c["dt"]), 4, 0, B, n, stride, D.to_device(c["paths"]), None, None, D.to_device(c["profile"]), 3,
                D.to_device(c["plan"]), None, None, out["traj"], out["m_of"], None, None, out["flags"])
    assert rc == 0 and same_bits(out["traj"].get(), _want(c, 4)["traj"]) and out["m_of"].get().tolist() == [9, 9]


# ---- the device's own plans ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planned(name):
    """a seeded scene of refine_util through pqp_speed_search and pqp_speed_refine on the device: (case with plan and dt, search, refine)"""
    c = R.seeded(name)
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    car = capi.car_default_geometry(**S.HAND_CAR) if name in R.HAND else None
    grid = capi.search_default_params(**c["prm"])
    se = h.speed_search(c["paths"], c["profile"], c["v_start"], c["agents"], m=c.get("m"), n_of=c.get("n_of"), stop_before=c.get("stop_before"),
                        a_of=c.get("a_of"), scene_of=c.get("scene_of"), car=car, prm=grid, blocked=True)
    rf = h.speed_refine(c["paths"], c["profile"], c["v_start"], se["blocked"], se["steps"], se["reached"], se["traj"], n_of=c.get("n_of"),
                        stop_before=c.get("stop_before"), grid=grid)
    h.close()
    return dict(c, plan=rf["traj"], dt=c["prm"]["dt"]), se, rf


@pytest.mark.parametrize("name", ("rest", "quick", "wait", "m8", "m12", "tiles", "long"))
def test_the_devices_own_plans_against_the_restatement(handle, name):
    """search, refine and sample on the device; the restatement runs on the device's arrays.  Then the properties: rows on the layers are
    the plan's, r = 1 returns a refined plan in all eight columns, a refined plan's defect is within 4 x plan_util.defect_bound (the
    factor tests/test_gpu_speed_refine.py gives the device's residuals over the emulation's), a kept staircase sampled linearly has none"""
    c, se, rf = _planned(name)
    m = c["plan"].shape[1]
    got = _both_forms(handle, c, 10, name, count_of=se["reached"], refine_flags=rf["flags"])
    one = _both_forms(handle, c, 1, (name, "r = 1"), count_of=se["reached"], refine_flags=rf["flags"])
    stairs = _both_forms(handle, dict(c, plan=se["traj"]), 10, (name, "the search's rows"), count_of=se["reached"], linear=True)
    print(f"{name}: refine flags {rf['flags'].tolist()} reached {se['reached'].tolist()} defect {got['defect'].tolist()} excess {got['excess'].tolist()}")
    for b in range(len(c["paths"])):
        L = int(se["reached"][b])
        if L == 0:
            assert got["flags"][b] == P.EMPTY
            continue
        assert got["m_of"][b] == P.fine_count(L, 10) and got["flags"][b] in (0, P.BACKWARD) and stairs["defect"][b] == 0.0 and stairs["flags"][b] == 0
        assert same_bits(got["traj"][b, :got["m_of"][b]:10][:, [0, 1, 2, 3, 4, 7]], c["plan"][b, :L][:, [0, 1, 2, 3, 4, 7]]), (name, b)
        assert same_bits(stairs["traj"][b, :stairs["m_of"][b]:10][:, [0, 1, 2, 3, 4, 7]], se["traj"][b, :L][:, [0, 1, 2, 3, 4, 7]]), (name, b)
        if rf["flags"][b] == R.REFINED:
            assert L == m and np.array_equal(one["traj"][b], c["plan"][b]), (name, b)
            assert got["defect"][b] <= 4.0 * P.defect_bound(c["dt"], c["plan"][b][:, 4].max()), (name, b, got["defect"][b])
            assert got["excess"][b] >= rf["excess"][b]                                   # the layers are among the samples
        else:
            assert got["defect"][b] == 0.0
    assert name == "quick" or (rf["flags"] == R.REFINED).any()


# ---- the hand case: a disc that crosses the lane between two layers ------------------------------------------------------------------------------
def test_a_disc_crossing_between_two_layers_is_seen_on_the_fine_steps_only(handle):
    """plan_util.crossing(): pqp_agents_check on the plan's m rows against the disc at the layers is clear; pqp_sample_plan at r = 10 and
    pqp_agents_check on its rows against the disc on the fine steps is a hit at sample 34.  Heading 0 and no clearance within 1e-6 of the
    margin (tests/test_plan_sample.py holds that for every sample): the device's sincos cannot move either verdict"""
    x = P.crossing()
    c, m = x["case"], x["m"]
    car = capi.car_default_geometry(**S.HAND_CAR)
    coarse = handle.agents_check(x["plan"], x["coarse_agents"], car=car)
    assert coarse["first_hit"].tolist() == [m] and coarse["hit_agent"].tolist() == [-1]
    fine = handle.sample_plan(c["paths"], c["profile"], x["plan"], P.CROSS_R, dt=c["prm"]["dt"], refine_flags=x["flags"])
    _same(fine, P.sample_batch(c["paths"], c["profile"], x["plan"], P.CROSS_R, c["prm"]["dt"], refine_flags=x["flags"]), "crossing")
    hit = handle.agents_check(fine["traj"], x["fine_agents"], m_of=fine["m_of"], car=car, clearance=True)
    assert hit["first_hit"].tolist() == [P.CROSS_FIRST_HIT] and hit["hit_agent"].tolist() == [0]
    assert np.flatnonzero(hit["clearance"][0] < 0.0).tolist() == [34, 35, 36]


# ---- through the layers ----------------------------------------------------------------------------------------------------------------------
def test_the_fine_plan_behind_the_chain(hip_lib):
    """optimize_path(..., search=, refine=, plan_samples=10, plan_agents=): what it adds equals the stand-alone calls on the arrays it
    returns, on every candidate and on the winners of a selection, and every other key is what the same call without the two keywords
    returns; without refine= the search's rows are sampled linearly"""
    import chain_util
    B, m, r = 16, 8, 10
    M = P.fine_count(m, r)
    sc = chain_util.scenarios(B)
    gs = np.array([0, 8, 16], np.int32)
    sp = capi.speed_default_params(v_max=8.0)
    se = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    se.stations, se.w_accel, se.margin = 96, 1.0, 0.2
    rf = capi.refine_default_params(hip_lib, w_jerk=0.5, window=6)
    agents = np.zeros((2, 1, m, 6))
    for s in range(2):                                       # crosses candidate 8 s's line near its middle during layers 2 .. 4
        st, tg = sc["start"][8 * s], sc["target"][8 * s]
        agents[s, 0, :] = [0.5 * (st[0] + tg[0]), 0.5 * (st[1] + tg[1]), st[2] + 1.5, 2.2, 0.9, 0.1]
        agents[s, 0, [0, 1, 5, 6, 7], 3] = -1.0
    fine_agents = np.ascontiguousarray(agents[:, :, np.arange(M) // r])                 # every layer's row held for its sub-steps
    fine_agents[:, :, 55:, 3] = 2.2                          # and there again from t = 5.5 s on, between two layers
    scene_all, scene_grp = (np.arange(B) // 8).astype(np.int32), np.array([1, 0], np.int32)
    ap = capi.agents_default_params(hip_lib, margin=0.3)
    base = dict(speed=sp, agents=agents, agents_params=ap, search=se)
    calls = (("all", dict(base, v_start=np.linspace(0.0, 3.0, B), scene_of=scene_all, refine=rf), True),
             ("select", dict(base, select=gs, v_start=np.array([0.0, 1.0]), scene_of=scene_grp, refine=rf), False),
             ("search only", dict(base, v_start=np.linspace(0.0, 3.0, B), scene_of=scene_all), False))
    h2 = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    for name, kw, twice in calls:
        runs = []
        for new in ((dict(plan_samples=r, plan_agents=fine_agents), {}) if twice else (dict(plan_samples=r, plan_agents=fine_agents),)):
            h, hs = chain_util.handles(B)
            runs.append(h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **kw, **new))
            h.close(); hs.close()
        res = runs[0]
        added = ["plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags", "plan_first_hit", "plan_hit_agent"]
        assert list(res)[-7:] == added
        if twice:
            assert list(runs[1]) == list(res)[:-7]
            for k in runs[1]:
                assert same_bits(np.asarray(res[k], dtype=np.float64), np.asarray(runs[1][k], dtype=np.float64)), (name, k)
        on_winners, refined = "select" in kw, "refine" in kw
        paths, n_of = (res["best_paths"], res["best_n"]) if on_winners else (res["out"], res["n_out"])
        want = h2.sample_plan(paths, res["profile"], res["refine_traj"] if refined else res["search_traj"], r, dt=se.dt, n_of=n_of,
                              count_of=res["search_reached"], refine_flags=res["refine_flags"] if refined else None, linear=True)
        for k in KEYS:
            assert same_bits(np.asarray(res["plan_" + k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)), (name, k)
        assert res["plan_traj"].shape == (len(paths), M, 8)
        chk = h2.agents_check(res["plan_traj"], fine_agents, m_of=res["plan_m_of"], scene_of=kw["scene_of"], prm=ap)
        assert same_bits(res["plan_first_hit"], chk["first_hit"]) and same_bits(res["plan_hit_agent"], chk["hit_agent"]), name
        print(f"{name}: plan flags {res['plan_flags'].tolist()} m_of {res['plan_m_of'].tolist()} first hit {res['plan_first_hit'].tolist()}")
        if refined:
            assert ((res["refine_flags"] == R.REFINED) & (res["plan_flags"] == 0)).any()
    h2.close()
    with pytest.raises(ValueError):
        h, hs = chain_util.handles(B)
        try:
            h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, plan_samples=r)
        finally:
            h.close(); hs.close()


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------------
def test_plan_sampler_agrees_with_the_python_calls(handle, tmp_path):
    exe = cpp_demo.build("plan_demo")
    c, se, rf = _planned("tiles")
    want = _host(handle, c, 10, count_of=se["reached"], refine_flags=rf["flags"])
    path = tmp_path / "case.bin"
    S.write_case(path, R.seeded("tiles"))
    r = subprocess.run([exe, str(path), "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(c["paths"])
    for b, line in enumerate(lines):
        t = line.split()
        assert t[0] == "path" and [int(v) for v in t[1:6]] == [b, want["flags"][b], rf["flags"][b], se["reached"][b], want["m_of"][b]], line
        assert same_bits(np.array([float(v) for v in t[6:]]), want["traj"][b][:want["m_of"][b], 4:7].ravel()), b
    r = subprocess.run([exe, str(path), "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "pqp_sample_plan:" in r.stderr
