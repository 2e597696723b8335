"""pqp_speed_refine on the GPU against the numpy restatement (tests/refine_util.py; tests/test_speed_refine.py checks every case on the CPU
first and measures the bounds used here).  Every device input is the restatement's search output.

Exact against the restatement: `bounds` bit for bit (integers times ds, and a correctly rounded sqrt), the kept paths' rows, flags and
status, and - at the device's own s - x, y, heading, k and excess.  The solve is held to the CPU's figures: the KKT certificate of the
device's (s, v, a), recomputed from the rows with recovered multipliers (refine_util.certificate), within 4 x refine_util.KKT_WORST - the
margin is for FMA contraction in the core and the clamp of the solver's tolerance - and every variable within 2 x refine_util.HIGHS_DIST
of HiGHS.  The shapes: the hand road (m = 8), m = 2 and m = 3 one after the other on one handle (m is an argument of the call, so a
batch has one m; the rows' sparsity is uploaded per m), m = 8, 12 and 40, "tiles" (S = 70 in two station tiles) and "long" (200 stations
x 12 layers over 300 ragged waypoints), m = 86 - the first 512-lane form of the core - and m = 193, the last that fits."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import cpp_demo
import device_form as D
import refine_util as R
import search_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_CAPACITY = -1, capi.ERR_CAPACITY


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)      # the reference's ADMM setting: the refine solves exactly all the same
    yield h
    h.close()


def _inputs(name):
    """(case, search result, m) of a case, from the reference the CPU tests share"""
    r = R.reference(name)
    return r["case"], r["res"], r["m"]


def _host(handle, c, res, window=None, pick=None, **over):
    sel = (lambda a: a) if pick is None else (lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[pick]))
    prm = capi.refine_default_params(**over) if window is None else capi.refine_default_params(window=window, **over)
    return handle.speed_refine(sel(c["paths"]), sel(c["profile"]), sel(c["v_start"]), sel(res["blocked"]), sel(res["steps"]), sel(res["reached"]),
                               sel(res["traj"]), n_of=sel(c.get("n_of")), stop_before=sel(c.get("stop_before")),
                               grid=capi.search_default_params(**c["prm"]), prm=prm)


def _device(handle, c, res, m=None, window=None, arrays=None):
    """the device form through device_form: the outputs lie in sentinel-filled allocations with a guard band behind them"""
    paths, profile = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("paths", "profile"))
    B, n, stride = paths.shape
    m = m or res["traj"].shape[1]
    prm = capi.refine_default_params() if window is None else capi.refine_default_params(window=window)
    opt = lambda k: None if c.get(k) is None else D.to_device(c[k], np.int32)
    out = dict(traj=D.Out((B, m, 8)), bounds=D.Out((B, m, 3)), cost=D.Out((B,)), excess=D.Out((B,)), status=D.Out((B,), np.int32),
               iters=D.Out((B,), np.int32), flags=D.Out((B,), np.int32))
    a = arrays or res
    rc = D.call(handle, "pqp_speed_refine_device", C.byref(capi.search_default_params(**c["prm"])), prm.array(), int(prm.window), B, n, stride,
                D.to_device(paths), opt("n_of"), opt("stop_before"), D.to_device(profile), D.to_device(c["v_start"]), m,
                D.to_device(a["blocked"], np.int32), D.to_device(a["steps"], np.int32), D.to_device(a["reached"], np.int32), D.to_device(a["traj"]),
                out["traj"], out["bounds"], out["cost"], out["excess"], out["status"], out["iters"], out["flags"])
    return (rc, out) if rc else (rc, {k: v.get() for k, v in out.items()})


def _same_outputs(a, b, where):
    for k in ("traj", "bounds", "cost", "excess", "status", "iters", "flags"):
        assert same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), (where, k)


def _check_refined(name, got, b, one, c, m):
    """one refined path of the device against the restatement and the CPU's figures"""
    su, dt = one["su"], c["prm"]["dt"]
    rows = got["traj"][b]
    s, v, a = rows[:, 4], rows[:, 5], rows[:, 6]
    assert got["status"][b] == R.SOLVED and got["flags"][b] == R.REFINED and got["iters"][b] == 0, (name, b, got["status"][b], got["flags"][b])
    assert same_bits(got["bounds"][b], su["bounds"]), (name, b)
    assert (s >= su["bounds"][:, 0]).all() and (s <= su["bounds"][:, 1]).all() and (v >= 0.0).all() and a[m - 1] == 0.0, (name, b)
    assert same_bits(rows[:, 7], np.arange(m).astype(np.float64) * np.float64(dt)), (name, b)
    x = np.concatenate([s, v, a])
    P, q, A, lo, up = su["qp"]
    cert = R.certificate(P, q, A, lo, up, x)
    print(f"{name} path {b}: m = {m}, " + ", ".join(f"{k} {val:.2e}" for k, val in cert.items()) + f", to HiGHS {np.abs(x - one['xh']).max():.2e}, "
          f"to the emulation {np.abs(x - one['xe']).max():.2e}, excess {got['excess'][b]:.3e}")
    for k in cert:
        assert cert[k] <= 4.0 * R.KKT_WORST[k], (name, b, k, cert[k])
    assert np.abs(x - one["xh"]).max() <= 2.0 * R.HIGHS_DIST, (name, b)
    fin = R.finish(c["paths"][b], c["profile"][b], su, one["found"], x, R.SOLVED, dt)
    assert same_bits(fin["traj"], rows), (name, b)
    assert same_bits(fin["excess"], got["excess"][b]), (name, b)
    assert abs(got["cost"][b] - R.objective(x, su["sigma"], dt, R.DEFAULT_PRM)) <= 1e-6 * max(1.0, got["cost"][b]), (name, b)


# ---- the refined paths, shape by shape -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("rest", "wait", "m8", "m12", "m40", "tiles", "long", "m86"))
def test_refined_paths_against_the_restatement(handle, name):
    r = R.reference(name)
    c, res, m = _inputs(name)
    got = _host(handle, c, res)
    for b, one in enumerate(r["each"]):
        assert not one["su"]["kept"] and (name, b) not in R.INFEASIBLE_CASES
        _check_refined(name, got, b, one, c, m)
    rc, dev = _device(handle, c, res)
    assert rc == 0, handle.lib.pqp_last_error()
    _same_outputs(dev, got, name)


def test_two_and_three_layers_one_after_the_other(handle):
    """m = 2, m = 3 and m = 2 again on one handle: the rows' sparsity is the handle's, per m, and goes up again when m changes"""
    first = None
    for name in ("m2", "m3", "m2"):
        r = R.reference(name)
        c, res, m = _inputs(name)
        got = _host(handle, c, res)
        for b, one in enumerate(r["each"]):
            _check_refined(name, got, b, one, c, m)
        if name == "m2" and first is not None:
            _same_outputs(got, first, "m2 again")
        first = first or got


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window,edges", (("tiles", 40, {32}), ("long", 30, {32, 64}), ("tiles", 0, set())))
def test_bounds_bit_for_bit_in_both_forms_at_any_batch_position(handle, name, window, edges):
    """wide windows: the free runs cross the words' edges at stations 31 / 32 (and 63 / 64 on the long grid), end at occupied stations, at
    station 0 and at j_last; window = 0: every run is its own station (most of those QPs are infeasible, and a kept path's bounds are zeros)"""
    c, res, m = _inputs(name)
    B = len(c["paths"])
    pick = lambda a, b: None if a is None else a[b]
    sus = [R.setup(c["paths"][b], c["profile"][b], c["v_start"][b], R.found_of(res, b), m, pick(c.get("n_of"), b), pick(c.get("stop_before"), b), c["prm"],
                   window=window) for b in range(B)]
    assert not any(su["kept"] for su in sus)
    runs = [(lo, hi, int(j), su["J"]) for su, st in zip(sus, res["steps"]) for (lo, hi), j in zip(su["runs"].tolist(), st[:, 0])]
    assert {e for lo, hi, _, _ in runs for e in (32, 64) if lo < e <= hi} == edges
    if window:
        assert any(hi + 1 < J and hi < j + window for lo, hi, j, J in runs), "no run ends at an occupied station"
        assert any(lo == 0 and j - window < 0 for lo, hi, j, J in runs)
        assert name != "long" or any(hi == J - 1 and j + window > J - 1 for lo, hi, j, J in runs)     # (no plan of "tiles" gets near its path's end)
    else:
        assert all(lo == hi == j for lo, hi, j, _ in runs)
    want = np.stack([su["bounds"] for su in sus])
    got = _host(handle, c, res, window=window)
    rc, dev = _device(handle, c, res, window=window)
    assert rc == 0, handle.lib.pqp_last_error()
    refined = got["flags"] == R.REFINED
    assert refined.any() and (got["flags"][~refined] == R.KEPT | R.INFEASIBLE).all()      # (window = 0 pins every station: infeasible QPs keep zeros)
    assert same_bits(got["bounds"][refined], want[refined]) and (got["bounds"][~refined] == 0.0).all()
    _same_outputs(dev, got, (name, window))
    order = np.array([(3 * b + 1) % B for b in range(B)] + [0, B - 1])                  # a longer batch, every path somewhere else
    moved = _host(handle, c, res, window=window, pick=order)
    for at, b in enumerate(order):
        for k in ("traj", "bounds", "cost", "excess", "status", "flags"):
            assert same_bits(np.asarray(moved[k][at], dtype=np.float64), np.asarray(got[k][b], dtype=np.float64)), (name, at, b, k)


# ---- the kept paths ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """the hand road, m = 8, one grid: refined paths with a kept one between every two of them.  (names, case, search result, what is kept)"""
    hand = S.hand_cases()
    parts = [("rest", R.seeded("rest")), ("driven_into", dict(hand["driven_into"], m=S.HAND_M)), ("wait", R.seeded("wait")),
             ("empty", dict(hand["empty"], m=S.HAND_M)), ("rest", R.seeded("rest")), ("not_finite", R.seeded("rest")), ("wait", R.seeded("wait")),
             ("quick", R.seeded("quick")), ("rest", R.seeded("rest")), ("start_blocked", dict(hand["start_blocked"], m=S.HAND_M)),
             ("wait", R.seeded("wait"))]
    names = [nm for nm, _ in parts]
    paths = np.concatenate([c["paths"] for _, c in parts])
    bad = names.index("not_finite")
    paths[bad, 3, 1] = math.nan
    n = paths.shape[1]
    n_of = np.array([c["n_of"][0] if c.get("n_of") is not None else n for _, c in parts], np.int32)
    case = dict(paths=paths, profile=np.concatenate([c["profile"] for _, c in parts]), v_start=np.concatenate([c["v_start"] for _, c in parts]),
                n_of=n_of, stop_before=None, prm=R.seeded("rest")["prm"], m=S.HAND_M)
    each = [S.run_case(dict(c, paths=paths[b:b + 1]), R.circles_of("rest")) for b, (_, c) in enumerate(parts)]
    res = {k: np.concatenate([e[k] for e in each]) for k in ("blocked", "steps", "reached", "traj", "flags")}
    kept = dict(driven_into=(R.KEPT, R.UNSOLVED), empty=(R.KEPT, R.UNSOLVED), not_finite=(R.KEPT, R.UNSOLVED), start_blocked=(R.KEPT, R.UNSOLVED),
                quick=(R.KEPT | R.INFEASIBLE, R.PRIMAL_INFEASIBLE))
    return names, case, res, kept


def test_kept_paths_return_the_searchs_rows_between_refined_neighbours(handle):
    names, c, res, kept = _mixed()
    assert 0 < res["reached"][names.index("driven_into")] < S.HAND_M and res["flags"][names.index("empty")] == S.EMPTY
    assert res["flags"][names.index("not_finite")] == S.NOT_FINITE and res["reached"][names.index("start_blocked")] == 0
    assert res["reached"][names.index("quick")] == S.HAND_M
    got = _host(handle, c, res)
    rc, dev = _device(handle, c, res)
    assert rc == 0, handle.lib.pqp_last_error()
    _same_outputs(dev, got, "mixed")
    alone = {nm: _host(handle, *_inputs(nm)[:2]) for nm in ("rest", "wait")}
    for b, nm in enumerate(names):
        if nm in kept:
            flags, status = kept[nm]
            assert got["flags"][b] == flags and got["status"][b] == status, (nm, got["flags"][b], got["status"][b])
            assert same_bits(got["traj"][b], res["traj"][b]) and (got["bounds"][b] == 0.0).all() and math.isnan(got["cost"][b]), nm
            assert math.isnan(got["excess"][b]) and (got["iters"][b] == 0 or nm == "quick"), nm
        else:                                                # untouched by its neighbours: what the path gives alone
            for k in ("traj", "bounds", "cost", "excess", "status", "flags"):
                assert same_bits(np.asarray(got[k][b], dtype=np.float64), np.asarray(alone[nm][k][0], dtype=np.float64)), (b, nm, k)
            assert got["flags"][b] == R.REFINED


def test_one_layer_keeps_every_path(handle):
    c = dict(S.hand_cases()["one_layer"], m=1)
    c = {k: (np.concatenate([v] * 3) if k in ("paths", "profile", "v_start") else v) for k, v in c.items()}
    res = S.run_case(c, R.circles_of("rest"))
    assert res["reached"].tolist() == [1, 1, 1]
    got = _host(handle, c, res)
    rc, dev = _device(handle, c, res)
    assert rc == 0
    _same_outputs(dev, got, "m = 1")
    assert got["flags"].tolist() == [R.KEPT] * 3 and got["status"].tolist() == [R.UNSOLVED] * 3 and same_bits(got["traj"], res["traj"])
    assert (got["bounds"] == 0.0).all() and np.isnan(got["cost"]).all()


def test_steps_no_search_wrote_keep_the_path(handle):
    """the arrays are the device's and are judged there: a station outside the path or one that is occupied keeps the path, and its
    neighbours are untouched"""
    c, res, m = _inputs("m8")
    want = _host(handle, c, res)
    steps = res["steps"].copy()
    steps[0, 3, 0] = 10 ** 6
    steps[2, 5, 0] = -4
    got = _host(handle, c, dict(res, steps=steps))
    assert got["flags"].tolist() == [R.KEPT, R.REFINED, R.KEPT] and same_bits(got["traj"][[0, 2]], res["traj"][[0, 2]])
    assert same_bits(got["traj"][1], want["traj"][1])
    blocked = res["blocked"].copy()
    j = int(res["steps"][1, 4, 0])
    blocked[1, 5, j >> 5] |= np.int32(1 << (j & 31))         # occupied at layer k + 1
    got = _host(handle, c, dict(res, blocked=blocked))
    assert got["flags"].tolist() == [R.REFINED, R.KEPT, R.REFINED] and same_bits(got["traj"][[0, 2]], want["traj"][[0, 2]])


# ---- the capacity and the refusals -------------------------------------------------------------------------------------------------------------
def test_the_capacity_is_accepted_and_one_layer_more_is_refused(handle):
    name = "m%d" % R.CAPACITY_M
    r = R.reference(name)
    c, res, m = _inputs(name)
    assert m == R.CAPACITY_M
    rc, dev = _device(handle, c, res)
    assert rc == 0, handle.lib.pqp_last_error()
    for b, one in enumerate(r["each"]):
        _check_refined(name, dev, b, one, c, m)
    B = len(c["paths"])
    more = dict(blocked=np.zeros((B, m + 1, res["blocked"].shape[2]), np.int32), steps=np.zeros((B, m + 1, 2), np.int32),
                reached=np.full(B, m + 1, np.int32), traj=np.zeros((B, m + 1, 8)))
    rc, out = _device(handle, c, res, m=m + 1, arrays=more)
    assert rc == ERR_CAPACITY and handle.lib.pqp_last_error().decode().startswith("pqp_speed_refine:")
    assert all(o.untouched() for o in out.values())
    with pytest.raises(capi.PqpError, match=f"pqp error {ERR_CAPACITY}: pqp_speed_refine:"):
        handle.speed_refine(c["paths"], c["profile"], c["v_start"], more["blocked"], more["steps"], more["reached"], more["traj"],
                            grid=capi.search_default_params(**c["prm"]))


def test_refusals_leave_the_outputs_alone(handle):
    c, res, m = _inputs("m3")
    nan, inf = math.nan, math.inf
    grids = [dict(dt=0.0), dict(ds=nan), dict(dt=inf), dict(stations=0), dict(stations=capi.SEARCH_MAX_STATES + 1)]
    prms = [dict(w_ref=-1.0), dict(w_accel=nan), dict(w_jerk=inf), dict(w_ref=0.0, w_accel=0.0), dict(a_max=0.0), dict(d_max=-3.0), dict(a_max=inf),
            dict(window=-1)]
    B, n, stride = c["paths"].shape
    for grid_kw, prm_kw in [(g, {}) for g in grids] + [({}, p) for p in prms]:
        prm = capi.refine_default_params(**prm_kw)
        out = dict(traj=D.Out((B, m, 8)), bounds=D.Out((B, m, 3)), cost=D.Out((B,)), excess=D.Out((B,)), status=D.Out((B,), np.int32),
                   iters=D.Out((B,), np.int32), flags=D.Out((B,), np.int32))
        rc = D.call(handle, "pqp_speed_refine_device", C.byref(capi.search_default_params(**dict(c["prm"], **grid_kw))), prm.array(), int(prm.window),
                    B, n, stride, D.to_device(c["paths"]), None, None, D.to_device(c["profile"]), D.to_device(c["v_start"]), m,
                    D.to_device(res["blocked"], np.int32), D.to_device(res["steps"], np.int32), D.to_device(res["reached"], np.int32),
                    D.to_device(res["traj"]), *out.values())
        assert rc == ERR_INVALID and handle.lib.pqp_last_error().decode().startswith("pqp_speed_refine:"), (grid_kw, prm_kw)
        assert all(o.untouched() for o in out.values()), (grid_kw, prm_kw)
    # w_ref = 0 alone and w_jerk = 0 are allowed; bounds and excess are optional
    got = _host(handle, c, res, w_ref=0.0, w_jerk=0.0)
    assert (got["flags"] == R.REFINED).all()


# ---- the waiting plan back to the checker ------------------------------------------------------------------------------------------------------
def test_the_refined_waiting_plan_passes_the_agents_check(handle):
    """the waiting hand case, refined, handed back to pqp_agents_check under CHECK_MARGIN: no hit (first_hit is the count, m, as the checker
    reports "none", and hit_agent -1).  tests/test_speed_refine.py holds the whole corridor clear of the disc by more than CHECK_MARGIN + ds.
    The refine does not promise this in general: stations between two free cells are not tested, as in the search."""
    c, res, m = _inputs("wait")
    got = _host(handle, c, res)
    assert got["flags"].tolist() == [R.REFINED]
    car = capi.car_default_geometry(**S.HAND_CAR)
    chk = handle.agents_check(got["traj"], c["agents"], car=car, prm=capi.agents_default_params(margin=R.CHECK_MARGIN), clearance=True)
    assert chk["first_hit"].tolist() == [m] and chk["hit_agent"].tolist() == [-1], chk
    assert chk["clearance"].min() > R.CHECK_MARGIN + c["prm"]["ds"]
    # the search's own staircase passes too; a plan that drives through does not
    through = got["traj"].copy()
    through[0, 2] = through[0, 5]
    assert handle.agents_check(through, c["agents"], car=car, prm=capi.agents_default_params(margin=R.CHECK_MARGIN))["first_hit"].tolist() == [2]


# ---- through the layers ----------------------------------------------------------------------------------------------------------------------
def test_the_refine_behind_the_chain(hip_lib):
    """optimize_path(..., search=, refine=) = the chain, the speed profile, the search and pqp_speed_refine one after the other: what it adds
    equals the stand-alone host call on the arrays it returns, on every candidate and on the winners of a selection"""
    import chain_util
    B, m = 16, 8
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
    scene_all, scene_grp = (np.arange(B) // 8).astype(np.int32), np.array([1, 0], np.int32)
    runs = {}
    for name, kw in (("all", dict(speed=sp, v_start=np.linspace(0.0, 3.0, B), agents=agents, scene_of=scene_all, search=se, refine=rf)),
                     ("select", dict(select=gs, speed=sp, v_start=np.array([0.0, 1.0]), agents=agents, scene_of=scene_grp, search=se, refine=rf))):
        h, hs = chain_util.handles(B)
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **kw)
        h.close(); hs.close()
    every, sel = runs["all"], runs["select"]
    assert list(every)[-7:] == ["search_blocked", "refine_traj", "refine_bounds", "refine_cost", "refine_excess", "refine_status", "refine_flags"]
    assert sel["refine_traj"].shape == (2, m, 8) and every["refine_bounds"].shape == (B, m, 3)
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    for res, paths, n_of, v0 in ((every, every["out"], every["n_out"], np.linspace(0.0, 3.0, B)), (sel, sel["best_paths"], sel["best_n"], np.array([0.0, 1.0]))):
        want = h.speed_refine(paths, res["profile"], v0, res["search_blocked"], res["search_steps"], res["search_reached"], res["search_traj"], n_of=n_of,
                              grid=se, prm=rf)
        for k in ("traj", "bounds", "cost", "excess", "status", "flags"):
            assert same_bits(np.asarray(res["refine_" + k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)), k
    h.close()
    print(f"behind the chain: search reached {every['search_reached'].tolist()} refine flags {every['refine_flags'].tolist()}")
    assert (every["refine_flags"] == R.REFINED).any()


def test_a_refine_between_two_replayed_chains_changes_nothing(hip_lib):
    """PQP_OPT_CHAIN_GRAPH: the chain called until it replays, a refine call on the path handle and one on the smoother handle, then the
    chain again: the same arrays, which are the plainly launched chain's.  The refine's QPs and sparsity lie in a group of their own on
    the handle, so the smoothers' structure - part of the chain's graph key - stays what it was"""
    import chain_util
    B = 8
    sc = chain_util.scenarios(B)
    c, res, m = _inputs("m8")
    outs = []
    for graph in (0, 1):
        h, hs = chain_util.handles(B)
        h.set_option(capi.OPT_CHAIN_GRAPH, graph)
        run = lambda: h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs)
        for _ in range(4 if graph else 1):                   # plain, plain, capture, replay
            first = run()
        if graph:
            want = _host(h, c, res)
            also = _host(hs, c, res)
            _same_outputs(also, want, "either handle")
            assert (want["flags"] == R.REFINED).all()
            for _ in range(2):
                again = run()
                for k in first:
                    assert same_bits(np.asarray(again[k], dtype=np.float64), np.asarray(first[k], dtype=np.float64)), k
        outs.append(first)
        h.close(); hs.close()
    for k in outs[0]:
        assert same_bits(np.asarray(outs[1][k], dtype=np.float64), np.asarray(outs[0][k], dtype=np.float64)), k
    assert (outs[0]["stage"] == 0).any()


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------------
def test_refiner_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("refine_demo")
    c, res, m = _inputs("tiles")
    want = _host(handle, c, res)
    path = tmp_path / "case.bin"
    S.write_case(path, c)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(c["paths"])
    for b, line in enumerate(lines):
        t = line.split()
        assert t[0] == "path" and [int(v) for v in t[1:5]] == [b, want["flags"][b], want["status"][b], res["reached"][b]], line
        assert same_bits(np.array([float(v) for v in t[5:]]), want["traj"][b][:, 4:7].ravel()), b
