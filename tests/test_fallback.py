"""pqp_fallback_rows and pqp_fallback_pick without a device: the restatement of tests/fallback_util.py held against a plain per-sample
loop, the braking law against a numerical integration, what a braking plan must be by construction, hand cases on every branch, the
margins of every case the GPU test runs, the pick rule over every combination of usable and unusable levels, the binding, every refusal,
the chain's plan with fallback=, the header-only FallbackPlanner and the kernels' resources."""
import ctypes as C
import inspect
import itertools
import math
import subprocess

import numpy as np
import pytest

import build_util
import chain_plan_cases as cases
import cpp_demo
import fallback_util as U
import stitch_util as ST
from path_optimizer_2_amd import capi
from shared_util import same_bits

ROWS = ("pqp_fallback_rows", "pqp_fallback_rows_device")
PICK = ("pqp_fallback_pick", "pqp_fallback_pick_device")
CASES = U.device_cases()
LEVELS = np.array(U.LEVELS)


def _groups(c):
    """(g, the group's rows of prev cut to its count or None, its stitch flags or None) of a case"""
    for g in range(c["state"].shape[0]):
        rows = None
        if c["prev"] is not None:
            mp = c["prev"].shape[1]
            rows = c["prev"][g, :mp if c["prev_m"] is None else min(max(int(c["prev_m"][g]), 0), mp)]
        yield g, rows, None if c["stitch_flags"] is None else c["stitch_flags"][g]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_against_a_plain_loop(c):
    got = U.run_case(c)
    for g, rows, sf in _groups(c):
        for l, level in enumerate(c["levels"]):
            want_rows, stop, stop_row, flags = U.plan_rows_loop(c["state"][g], level, c["a_cap"], c["dt"], c["r"], c["m"], rows, sf)
            assert flags == got["flags"][g, l] and stop_row == got["stop_row"][g, l], (c["name"], g, l, flags, got["flags"][g, l])
            assert same_bits(np.array(stop), got["stop"][g, l]) and same_bits(np.array(want_rows), got["rows"][g, l]), (c["name"], g, l)


# ---- the law ---------------------------------------------------------------------------------------------------------------------------------
LAW_CASES = [(8.0, 0.5, 3.0, 5.0), (8.0, 1.5, 1.5, 2.5), (3.0, -3.0, 3.0, 5.0), (5.0, -6.0, 6.0, 15.0), (0.3, 0.0, 3.0, 5.0), (0.05, -0.2, 6.0, 15.0),
             (12.0, 0.0, 6.0, 15.0), (20.0, 1.0, 1.5, 2.5), (0.0, -1.0, 3.0, 5.0), (0.0, 1.0, 3.0, 5.0), (2.0, -1.4, 1.5, 2.5)]


def test_the_law_against_a_numerical_integration():
    """the closed form against Heun's rule on a' = -j clamped at -d, stopped at v = 0, at the rows' instants (dt 0.125, 8 s).  The
    integration is run at h = 2^-12 s and 2^-13 s; per case and per column, the bound on |closed form - finer integration| is ten times
    the greatest difference between the two integrations: measured against the integrator, not against the code under test.  The
    acceleration is compared away from its two events (the end of the ramp, the stop), which an integration places within a step.
    Measured as this stands, the greatest over the cases: the two step sizes differ by 1.4e-7 m and 8.9e-8 m/s (bounds 1.4e-6 m and
    8.9e-7 m/s) and the closed form is within 2.5e-8 m and 1.8e-8 m/s of the finer integration; the acceleration, linear in a phase, is
    integrated exactly by both and met exactly by the closed form.  Three cases run through the hold alone on dyadic values, where
    Heun's rule is exact: both step sizes and the closed form agree to the bit there."""
    dt, m = 0.125, 65
    at = U.times(dt, 1, m)
    worst, spread = np.zeros(3), np.zeros(3)
    for v0, a_in, d, j in LAW_CASES:
        got = U.plan_rows(np.array([0, 0, 0, 0, 0, v0, a_in, 0.0]), (d, j), U.A_CAP, dt, 1, m)["rows"]
        a0 = min(max(a_in, -d), U.A_CAP)
        coarse, fine = U.integrate(v0, a0, d, j, at, 2.0 ** -12), U.integrate(v0, a0, d, j, at, 2.0 ** -13)
        between = np.abs(coarse - fine).max(axis=0)
        err = np.abs(got[:, 4:7] - fine).max(axis=0)
        # the acceleration jumps at the stop and has a kink at t1: a row within one coarse step of either is compared on e and v alone
        a0_, t1, ts, in_ramp, v1, s1, T, eT = U.law_constants(v0, a_in, d, j, U.A_CAP)
        away = (np.abs(at - T) > 2.0 ** -11) & (np.abs(at - t1) > 2.0 ** -11)
        err[2] = np.abs(got[away, 6] - fine[away, 2]).max()
        between[2] = np.abs(coarse[away, 2] - fine[away, 2]).max()
        print(f"v0 {v0} a {a_in} d {d} j {j}: step sizes differ by {between}, closed form off by {err}")
        assert (err <= 10.0 * between).all(), ((v0, a_in, d, j), err, between)
        worst, spread = np.maximum(worst, err), np.maximum(spread, between)
    print("greatest difference between the step sizes", spread, "greatest error of the closed form", worst)


def _properties(state, level, a_cap, got, prev=None):
    rows, (T, eT), stop_row = got["rows"], got["stop"], got["stop_row"]
    d, j = level
    a0 = min(max(state[6], -d), a_cap)
    e, v, a, t = rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7]
    M = len(t)
    assert (v >= 0.0).all() and (e >= 0.0).all() and (e <= eT).all()
    # e = E(t) is a product of three roundings above a sum of two: non-decreasing up to 4 ulp of the distance
    assert (np.diff(e) >= -4.0 * np.spacing(max(eT, 1.0))).all()
    assert (a >= -d).all() and (a <= max(a0, 0.0)).all() and (a[:stop_row] <= a0).all()
    moving = slice(0, max(stop_row - 1, 0))
    step = np.diff(t)[moving]
    assert (np.abs(np.diff(a[:stop_row])) <= j * step + 4.0 * np.spacing(max(d, abs(a0)))).all()
    assert same_bits(rows[stop_row:, :7], np.broadcast_to(rows[min(stop_row, M - 1), :7], (M - stop_row, 7)))
    assert (rows[stop_row:, 5] == 0.0).all() and (rows[stop_row:, 6] == 0.0).all() and (rows[stop_row:, 4] == eT).all()
    assert bool(got["flags"] & U.HORIZON) == (stop_row == M) and (stop_row == M or t[stop_row] >= T) and (stop_row == 0 or t[stop_row - 1] < T)


def _row_0_is_the_state_s_row(state, prev, rows):
    """at t = 0 a plan on the previous plan stands where the state does when the state's station is a row's: the row the walk finds
    for sigma = state[4] - the last one whose running maximum of s is <= it - has its x, y, k bit for bit in row 0, its heading through
    constrainAngle, and e = 0.  (On a plan whose s column comes back on itself an earlier row may hold the same station: the walk's
    row is the one that counts.)  1 when the state is that row, bit for bit in its first five columns, and the property was held"""
    S = np.maximum.accumulate(prev[:, 4])
    i = max(int((S <= state[4]).sum()) - 1, 0)
    if not same_bits(prev[i, :5], state[:5]):
        return 0
    assert same_bits(rows[0, [0, 1, 3]], prev[i, [0, 1, 3]]) and rows[0, 2] == U.K.constrain_angle(float(prev[i, 2])) and rows[0, 4] == 0.0
    return 1


# the cases that put states on rows, and the least number of plans that must have been held to the property in each
ON_A_ROW = {"ragged": 18, "G67_mp64_m63_r1_L1_s8": 22, "G67_mp64_m130_r1_L1_s11": 20, "G5_mp63_m2_r1_L8_s11": 8, "G5_mp130_m65_r1_L8_s8": 8,
            "G1_mp130_m7_r10_L3_s8": 3, "stitch_flags": 6, "bad_states": 3}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_properties_of_every_plan(c):
    got = U.run_case(c)
    on_rows = 0
    for g, rows, sf in _groups(c):
        for l, level in enumerate(c["levels"]):
            one = {k: got[k][g, l] for k in ("rows", "stop", "stop_row", "flags")}
            if one["flags"] == U.BAD:
                assert not one["rows"].any() and not one["stop"].any() and one["stop_row"] == 0
                continue
            assert np.isfinite(one["rows"]).all()
            _properties(c["state"][g], level, c["a_cap"], one)
            if one["flags"] & U.ARC:
                assert same_bits(one["rows"][0, [0, 1, 3]], c["state"][g, [0, 1, 3]])          # e = 0: the state's own place
            else:
                on_rows += _row_0_is_the_state_s_row(c["state"][g], rows, one["rows"])
    if c["name"] in ON_A_ROW:
        assert on_rows >= ON_A_ROW[c["name"]], (c["name"], on_rows)
    bad = got["flags"] & U.BAD != 0
    assert (got["flags"][bad] == U.BAD).all()
    assert not ((got["flags"] & U.BAD_PLAN != 0) & (got["flags"] & U.ARC == 0)).any()


def test_every_device_case_keeps_its_margins():
    """every comparison a flag or a segment hangs on and that is not one of identical bits - t against t1 and against T, ts against t1,
    sigma against a row's s - in every case the GPU test runs, none left out, is at least 1e-6 from going the other way"""
    seen = 0
    for c in CASES:
        margins = U.run_case(c)["margins"]
        assert margins.shape == c["state"].shape[:1] + (len(c["levels"]), 4)
        assert (margins >= 1e-6).all(), (c["name"], margins.reshape(-1, 4).min(axis=0))
        seen += int(np.isfinite(margins).sum())
    assert seen > 1000


def test_hand_cases_on_every_branch():
    plan = ST.arc_plan(80, dt=0.125, v=8.0, a=0.0, curvature=0.02, t0=1.0, s0=5.0)          # 1 m between rows, s from 5 to 84
    dt, m = 0.125, 41                                                                         # a horizon of 5 s
    one = lambda v0, a, level=(3.0, 5.0), rows=plan, at=8, **kw: U.plan_rows(U.state_on(plan, at, v=v0, a=a), level, kw.pop("a_cap", U.A_CAP), dt,
                                                                             kw.pop("r", 1), kw.pop("m", m), rows, **kw)
    # a0 > 0: the car still gains speed before it brakes; the first row is the state's pose, bit for bit
    r = one(8.0, 1.0)
    assert r["flags"] == 0 and r["rows"][1, 5] > 8.0 and r["rows"][0, 6] == 1.0 and same_bits(r["rows"][0, :4], plan[8, :4]) and r["rows"][0, 4] == 0.0
    assert r["stop"][0] == (1.0 + 3.0) / 5.0 + (8.0 + (1.0 - 2.5 * 0.8) * 0.8) / 3.0                      # t1 + v1 / d
    # a0 = -d exactly: t1 = 0, the hold from row 0
    r = one(6.0, -3.0)
    assert (r["rows"][:r["stop_row"], 6] == -3.0).all() and r["stop"][0] == 2.0 and r["stop"][1] == 6.0 and r["stop_row"] == 16 and r["margins"][U.M_T] > 0.1
    # a0 < -d: clamped to -d; above a_cap: clamped to it
    assert same_bits(one(6.0, -7.5)["rows"], r["rows"]) and one(6.0, 9.0)["rows"][0, 6] == U.A_CAP
    # v0 = 0 with a0 <= 0: standing from the start, every row the state's
    for a in (0.0, -1.0, -9.0):
        r = one(0.0, a)
        assert r["stop_row"] == 0 and not r["stop"].any() and r["flags"] == 0 and not r["rows"][:, 4:7].any()
        assert same_bits(r["rows"][:, :4], np.broadcast_to(plan[8, :4], (m, 4)))
    # a stop inside the ramp, in the hold, beyond the horizon
    r = one(0.2, -0.5)
    assert r["stop"][0] < (3.0 - 0.5) / 5.0 and r["stop_row"] < m and (r["rows"][:r["stop_row"], 6] > -3.0).all()
    r = one(8.0, 0.0)
    assert r["stop"][0] > 0.6 and r["flags"] == 0 and (r["rows"][5:r["stop_row"], 6] == -3.0).all()
    r = one(8.0, 0.0, level=(1.5, 2.5), m=17)
    assert r["flags"] == U.HORIZON and r["stop_row"] == 17 and r["rows"][-1, 5] > 0.0
    # a plan that ends before the car stands: the rows behind it stand on its last row
    r = one(14.0, 0.0, at=60)
    assert r["flags"] == U.PATH_SHORT and same_bits(r["rows"][-1, :4], plan[-1, :4]) and r["rows"][-1, 4] > plan[-1, 4] - plan[60, 4]
    assert one(8.0, 0.0, at=60)["flags"] == 0
    # repeated s rows: a zero-length segment has lambda = 0, and the walk steps over it
    twice = np.concatenate([plan[:12], plan[11:12], plan[12:]])
    r = one(8.0, 0.0, rows=twice)
    assert r["flags"] == 0 and float(np.abs(r["rows"] - one(8.0, 0.0)["rows"]).max()) < 1e-12
    at_it = U.plan_rows(U.state_on(twice, 11, v=0.0, a=0.0), (3.0, 5.0), U.A_CAP, dt, 1, 3, twice)
    assert same_bits(at_it["rows"][0, :4], twice[12, :4])                                      # the later of two equal rows
    # sigma in front of row 0: the car stands on row 0 until it is past it
    st = U.state_on(plan, 0, v=4.0, a=0.0)
    st[4] -= 2.5
    r = U.plan_rows(st, (1.5, 2.5), U.A_CAP, dt, 1, m, plan)
    before = st[4] + r["rows"][:, 4] < plan[0, 4]
    assert before[:3].all() and not before[-1] and same_bits(r["rows"][before, :4], np.broadcast_to(plan[0, :4], (before.sum(), 4)))
    # the arc: no plan, a short plan, a replanned group, a row that is not a number; k0 = 0 and |k0 e| on both sides of 2^-6
    hole = plan.copy(); hole[40, 1] = np.nan
    assert one(8.0, 0.0, rows=None)["flags"] == U.ARC and one(8.0, 0.0, rows=plan[:1])["flags"] == U.ARC
    assert one(8.0, 0.0, stitch_flags=ST.REPLAN | ST.LATERAL)["flags"] == U.ARC and one(8.0, 0.0, rows=hole)["flags"] == U.ARC | U.BAD_PLAN
    assert one(8.0, 0.0, stitch_flags=ST.BAD)["flags"] == U.BAD and one(-0.1, 0.0)["flags"] == U.BAD and one(math.nan, 0.0)["flags"] == U.BAD
    ahead = np.array([3.0, -2.0, 0.0, 0.0, 7.0, 8.0, 0.0, 0.0])
    r = U.plan_rows(ahead, (3.0, 5.0), U.A_CAP, dt, 1, m)
    assert same_bits(r["rows"][:, 0], 3.0 + r["rows"][:, 4]) and (r["rows"][:, 1] == -2.0).all() and not r["rows"][:, 2:4].any()      # k0 = 0, heading 0
    for k0 in (1e-4, 0.01):                                     # the whole plan below the Taylor switch, and rows on both sides of it
        turn = ahead.copy(); turn[3] = k0
        r = U.plan_rows(turn, (3.0, 5.0), U.A_CAP, dt, 1, m)
        th = k0 * r["rows"][:, 4]
        assert (th.max() < 2.0 ** -6) == (k0 == 1e-4) and th[1] < 2.0 ** -6
        exact = np.stack([3.0 + np.sin(th) / k0, -2.0 + (1.0 - np.cos(th)) / k0], 1)
        assert float(np.abs(r["rows"][:, :2] - exact).max()) < 1e-9 and same_bits(r["rows"][:, 2], th) and (r["rows"][:, 3] == k0).all()


def test_on_the_plan_the_rows_are_the_plan_s_own_chords():
    """a car that brakes along an arc sampled every metre stays within the chord's sagitta k h^2 / 8 of the arc, at the arc length s + e"""
    k, h = 0.02, 1.0
    plan = ST.arc_plan(80, dt=0.125, v=8.0, a=0.0, curvature=k, t0=0.0, s0=0.0, x0=0.0, y0=0.0, h0=0.0)
    r = U.plan_rows(U.state_on(plan, 5, v=9.0, a=0.3, lam=0.25), (3.0, 5.0), U.A_CAP, 0.1, 1, 60, plan)
    s = plan[5, 4] + 0.25 * (plan[6, 4] - plan[5, 4]) + r["rows"][:, 4]
    exact = np.stack([np.sin(k * s) / k, (1.0 - np.cos(k * s)) / k], 1)
    assert r["flags"] == 0 and float(np.abs(r["rows"][:, :2] - exact).max()) <= k * h * h / 8.0 + 1e-9
    assert float(np.abs(r["rows"][:, 2] - k * s).max()) < 1e-9 and (r["rows"][:, 3] == k).all()


# ---- the pick -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3, 8])
def test_the_pick_against_a_plain_loop_over_every_combination(L):
    """every level of a group is one of: usable, hit at row 2, hit at row 4, collided at row 2, flagged short - all 5^L combinations for
    L = 1 and 3; for L = 8 all 3^8 of the first three kinds, which is every pattern of usable and unusable levels with ties and every
    order of the contacts in, and the other two kinds in all 5^3 combinations on levels 0, 4 and 7 over two fillings of the rest
    (fallback_util.pick_combinations); then a bad group between two good ones and groups with a winner"""
    M = 6
    rf, hit, col = U.pick_combinations(L, M)
    G = len(rf)
    assert G == {1: 5, 3: 125, 8: 3 ** 8 + 250}[L]
    rng = np.random.default_rng(L)
    rows = rng.uniform(-5.0, 5.0, (G, L, M, 8))
    got = U.fallback_pick(rows, rf, first_hit=hit.ravel(), first_collision=col.ravel())
    taken = set()
    for g in range(G):
        lv, fl = U.pick_loop(L, M, rf[g].tolist(), hit[g].tolist(), col[g].tolist())
        assert (got["level"][g], got["flags"][g]) == (lv, fl), (g, lv, fl, got["level"][g], got["flags"][g])
        assert same_bits(got["final_traj"][g], rows[g, lv]) and got["final_m"][g] == M
        taken.add((lv, bool(fl & U.NOT_CLEAR)))
    assert taken == {(l, nc) for l in range(L) for nc in (False, True)}          # every level is taken, clear and not clear
    # a verdict is read as it is: a garbage one below zero is an earlier contact than any row, and a level is still named
    junk = U.fallback_pick(rows[:2], rf[:2] * 0, first_hit=np.full(2 * L, -7), first_collision=np.array(([-9] * L + [-2 ** 31] * L)))
    assert junk["level"].tolist() == [L - 1, L - 1] and (junk["flags"] == U.TAKEN | U.NOT_CLEAR).all()
    assert U.pick_loop(L, M, [0] * L, [-7] * L, [-9] * L) == (L - 1, U.TAKEN | U.NOT_CLEAR)
    assert U.TAKEN in got["flags"].tolist() and (got["flags"] & U.NOT_CLEAR).any() and (got["flags"] & U.TAKEN).all()
    # without the verdicts every level that is not short is usable; with best, a winner keeps its rows
    free = U.fallback_pick(rows, rf)
    assert all(free["level"][g] == next((l for l in range(L) if not rf[g, l] & U.PATH_SHORT), L - 1) for g in range(G))
    c = U.pick_case(7, L, M, seed=5)
    got = U.fallback_pick(**c)
    assert got["flags"][1] == U.BAD and got["level"][1] == -1 and not got["final_traj"][1].any() and got["final_m"][1] == 0
    assert got["level"][0] >= 0 and got["level"][2] >= 0 and got["flags"][4] & U.NOT_CLEAR and got["level"][3] == L - 1      # the tie: the highest level
    for g in np.flatnonzero(c["best"] >= 0):
        assert same_bits(got["final_traj"][g], c["best_traj"][g]) and got["final_m"][g] == c["best_m"][g] and got["level"][g] == -1 and got["flags"][g] == 0
    none = U.fallback_pick(c["rows"], c["row_flags"], best=c["best"], first_hit=c["first_hit"], first_collision=c["first_collision"])
    assert not none["final_traj"][c["best"] >= 0].any() and not none["final_m"][c["best"] >= 0].any()


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------
ROWS_PARAMS = ["h", "prm", "n_levels", "levels", "dt", "r", "m", "groups", "mp", "stride", "prev", "prev_m", "state", "stitch_flags", "rows", "stop",
               "stop_row", "flags"]
PICK_PARAMS = ["h", "groups", "n_levels", "m_rows", "best", "best_traj", "best_m", "rows", "row_flags", "first_hit", "first_collision", "final_traj",
               "final_m", "level", "flags"]


def test_symbols_constants_and_defaults(hip_lib):
    assert set(ROWS + PICK + ("pqp_fallback_default_params",)) <= set(capi.EXPORTS) and all(hasattr(hip_lib, n) for n in ROWS + PICK)
    for name in ROWS:
        assert [q.name for q in capi.HEADER.functions[name].params] == ROWS_PARAMS
    for name in PICK:
        assert [q.name for q in capi.HEADER.functions[name].params] == PICK_PARAMS
    assert not any(s.startswith("pqp_fallback") for s in capi.HEADER.structs)              # plain doubles, no struct
    assert (capi.FALLBACK_PARAMS, capi.FALLBACK_MAX_LEVELS, capi.FALLBACK_DEFAULT_LEVELS, capi.FALLBACK_A_CAP) == (1, 8, 3, 0)
    names = ("BAD", "ARC", "BAD_PLAN", "PATH_SHORT", "HORIZON", "TAKEN", "NOT_CLEAR")
    assert [getattr(capi, "FALLBACK_" + n) for n in names] == [getattr(U, n) for n in names] == [1 << k for k in range(7)]
    p = capi.fallback_default_params(hip_lib)
    sp = capi.speed_default_params(hip_lib)
    assert p.levels.tolist() == [list(l) for l in U.LEVELS] and p.a_cap == U.A_CAP == sp.a_max and p.levels[1, 0] == sp.d_max
    q = capi.fallback_default_params(hip_lib, a_cap=0.5, levels=[(2.0, 4.0)])
    assert q.a_cap == 0.5 and q.level_rows()[0] == 1 and q.array().tolist() == [0.5]
    hip_lib.pqp_fallback_default_params(None, None, None)                                # NULL pointers are ignored
    assert list(inspect.signature(capi.Handle.fallback_rows).parameters) == ["self", "state", "m", "dt", "r", "prev", "prev_m", "stitch_flags", "prm"]
    assert list(inspect.signature(capi.Handle.fallback_pick).parameters) == ["self", "rows", "row_flags", "best", "best_traj", "best_m", "first_hit",
                                                                            "first_collision"]
    for f in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        names = list(inspect.signature(f).parameters)
        assert names[-8:-4] == ["fallback", "previous", "parked", "rank"]                  # in front of previous, which a test pins in front of parked


def _rows_call(lib, form, handle, **over):
    """one call with a single argument changed from a set the library would accept; never sent with none changed: `h` is not a handle"""
    G, L, mp, m, r = 3, 2, 4, 3, 2
    M = (m - 1) * r + 1
    a = dict(prm=np.array([1.5]), n_levels=L, levels=np.array([[1.5, 2.5], [3.0, 5.0]]), dt=0.5, r=r, m=m, groups=G, mp=mp, stride=8, prev=np.zeros((G, mp, 8)),
             prev_m=np.full(G, mp, np.int32), state=np.zeros((G, 8)), stitch_flags=np.zeros(G, np.int32), rows=np.full((G, L, M, 8), 7.0),
             stop=np.full((G, L, 2), 7.0), stop_row=np.full((G, L), 7, np.int32), flags=np.full((G, L), 7, np.int32))
    assert over and set(over) <= set(a) | {"h"}
    a.update(over)
    rc = getattr(lib, form)(over.get("h", handle), *[a[k] for k in ROWS_PARAMS[1:]])
    untouched = all((a[k] == 7).all() for k in ("rows", "stop", "stop_row", "flags") if a[k] is not None)
    return rc, untouched, lib.pqp_last_error().decode()


def _pick_call(lib, form, handle, **over):
    G, L, M = 3, 2, 5
    a = dict(groups=G, n_levels=L, m_rows=M, best=np.full(G, -1, np.int32), best_traj=np.zeros((G, M, 8)), best_m=np.zeros(G, np.int32),
             rows=np.zeros((G, L, M, 8)), row_flags=np.zeros((G, L), np.int32), first_hit=np.full(G * L, M, np.int32),
             first_collision=np.full(G * L, M, np.int32), final_traj=np.full((G, M, 8), 7.0), final_m=np.full(G, 7, np.int32),
             level=np.full(G, 7, np.int32), flags=np.full(G, 7, np.int32))
    assert over and set(over) <= set(a) | {"h"}
    a.update(over)
    rc = getattr(lib, form)(over.get("h", handle), *[a[k] for k in PICK_PARAMS[1:]])
    untouched = all((a[k] == 7).all() for k in ("final_traj", "final_m", "level", "flags") if a[k] is not None)
    return rc, untouched, lib.pqp_last_error().decode()


_lv = lambda *rows: np.array(rows, dtype=np.float64)
ROWS_REFUSALS = [dict(h=None), dict(prm=None), dict(levels=None), dict(state=None), dict(rows=None), dict(stop=None), dict(stop_row=None), dict(flags=None),
                 dict(groups=0), dict(n_levels=0), dict(n_levels=9), dict(groups=2 ** 30), dict(dt=0.0), dict(dt=-0.5), dict(dt=math.nan), dict(dt=math.inf),
                 dict(r=0), dict(m=0), dict(m=2 ** 30, r=4), dict(m=2 ** 31 - 64, r=1), dict(mp=0), dict(stride=7), dict(prev=None), dict(prm=np.array([-0.1])),
                 dict(prm=np.array([math.nan])), dict(levels=_lv([1.5, 2.5], [1.0, 5.0])), dict(levels=_lv([0.0, 2.5], [3.0, 5.0])),
                 dict(levels=_lv([1.5, 0.0], [3.0, 5.0])), dict(levels=_lv([1.5, 2.5], [math.inf, 5.0])), dict(levels=_lv([1.5, math.nan], [3.0, 5.0])),
                 dict(levels=_lv([-1.5, 2.5], [3.0, 5.0])), dict(levels=_lv([1.5, 2.5], [3.0, -5.0]))]
PICK_REFUSALS = [dict(h=None), dict(rows=None), dict(row_flags=None), dict(final_traj=None), dict(final_m=None), dict(level=None), dict(flags=None),
                 dict(groups=0), dict(n_levels=0), dict(n_levels=9), dict(groups=2 ** 30), dict(m_rows=0), dict(m_rows=2 ** 31 - 64), dict(best_traj=None), dict(best_m=None)]


def test_every_refusal_comes_before_the_device(hip_lib):
    """all four forms check everything before they look into the handle, so a pointer that is no handle shows the refusals here.
    (prev = None alone is refused because prev_m is still given.)"""
    no_handle = C.create_string_buffer(4096)
    for form in ROWS:
        for over in ROWS_REFUSALS:
            rc, untouched, msg = _rows_call(hip_lib, form, no_handle, **over)
            assert rc == -1 and untouched and msg.startswith("pqp_fallback_rows:"), (form, over, rc, msg)
    for form in PICK:
        for over in PICK_REFUSALS:
            rc, untouched, msg = _pick_call(hip_lib, form, no_handle, **over)
            assert rc == -1 and untouched and msg.startswith("pqp_fallback_pick:"), (form, over, rc, msg)


def test_the_wrapper_s_own_refusals(hip_lib):
    h = object.__new__(capi.Handle)
    h.lib = hip_lib
    state, prev = np.zeros((3, 8)), np.zeros((3, 4, 8))
    for args, kw, what in (((state[:, :7], 3), {}, r"state must be \[G\]\[8\]"), ((state, 3), dict(prev=prev[:2]), r"prev must be \[3\]"),
                           ((state, 3), dict(prev_m=[4, 4, 4]), "prev_m needs prev"), ((state, 3), dict(prev=prev, prev_m=[4, 4]), "prev_m must have 3"),
                           ((state, 3), dict(stitch_flags=[0]), "stitch_flags must have 3"), ((state, 2 ** 30), dict(r=4), "do not fit an int")):
        with pytest.raises(ValueError, match=what):
            h.fallback_rows(*args, **kw)
    rows, rf = np.zeros((3, 2, 5, 8)), np.zeros((3, 2), np.int32)
    for args, kw, what in (((rows[0], rf), {}, r"rows must be \[G\]\[L\]\[M\]\[8\]"), ((rows, rf[:2]), {}, "row_flags must have 6"),
                           ((rows, rf), dict(best_traj=np.zeros((3, 5, 8))), "go together"), ((rows, rf), dict(best=[0, 1]), "best must have 3"),
                           ((rows, rf), dict(first_hit=[5, 5, 5]), "first_hit must have 6"), ((rows, rf), dict(first_collision=[5]), "first_collision must have 6")):
        with pytest.raises(ValueError, match=what):
            h.fallback_pick(*args, **kw)


# ---- the chain's plan ---------------------------------------------------------------------------------------------------------------------------
def _plan(lib, kw):
    h = capi.Handle.__new__(capi.Handle)
    h.lib = lib
    cfg = capi._defaults(lib, capi.PqpChainConfig, "pqp_chain_default_config", cases.CHAIN_CONFIG)
    return h._chain_plan(points=np.zeros((cases.B, 9, 2)), cfg=cfg, **kw)


def _previous(groups, m=6):
    return (np.zeros((groups, m, 11)), np.full(groups, m, np.int32), np.zeros((groups, 6)), np.zeros(groups), None)


def test_the_chain_s_plan_with_fallback(hip_lib):
    cf = cases.configs(hip_lib)
    gs = np.array([0, 1, 4], np.int32)                            # no empty group: a braking plan is checked in its group's scene
    j = dict({k: v for k, v in cf["j"][1].items() if k != "v_start"}, rank=gs, previous=_previous(2), map_of=np.array([3, 1, 2, 0], np.int32))
    base, plan = _plan(hip_lib, j), _plan(hip_lib, dict(j, fallback=True))
    L, M = 3, cases.FINE
    keys = [("final_traj", (2, M, 8), "float64"), ("final_m", (2,), "int32"), ("fallback_level", (2,), "int32"), ("fallback_flags", (2,), "int32"),
            ("fallback_rows", (2, L, M, 8), "float64"), ("fallback_first_hit", (2 * L,), "int32"), ("fallback_first_collision", (2 * L,), "int32")]
    assert plan.result == base.result + keys and plan.on_device == base.on_device and base.fallback is None          # behind every existing key
    assert len(plan.stages) == len(base.stages) + 1
    stage = plan.stages[-1]
    assert [u[0] for u in stage.uploads] == ["fallback_scene_of", "fallback_map_of"]
    assert stage.uploads[0][1].tolist() == [0, 0, 0, 0, 0, 0] and stage.uploads[1][1].tolist() == [3, 3, 3, 1, 1, 1]      # the group's first candidate's, L times
    assert [s[0] for s in stage.scratch] == ["fallback_stop", "fallback_stop_row", "fallback_row_flags", "fallback_hit_agent", "fallback_free"]
    assert plan.fallback[0].levels.tolist() == [list(l) for l in U.LEVELS]
    # a FallbackParams of one level; scene_of of the second group's first candidate; without plan_samples= the layers' rows and steps
    one = capi.fallback_default_params(hip_lib, levels=[(4.0, 8.0)])
    plan = _plan(hip_lib, dict(j, fallback=one, scene_of=np.array([0, 1, 1, 0], np.int32), map_of=None))
    assert plan.result[-3][:2] == ("fallback_rows", (2, 1, M, 8)) and plan.stages[-1].uploads[0][1].tolist() == [0, 1] and plan.stages[-1].uploads[1][1] is None
    f = dict({k: v for k, v in cf["f"][1].items() if k != "v_start"}, rank=gs, previous=_previous(2))
    plan = _plan(hip_lib, dict(f, fallback=True))
    assert plan.result[-7][:2] == ("final_traj", (2, cases.LAYERS, 8))
    # tracks=: the prediction's fine rows
    k = dict({key: v for key, v in cf["k"][1].items() if key != "v_start"}, rank=gs, previous=_previous(2))
    assert _plan(hip_lib, dict(k, fallback=True)).result[-7][:2] == ("final_traj", (2, M, 8))
    # winners_only keeps what it kept: the fallback's keys are per group
    plan = _plan(hip_lib, dict(j, fallback=True, winners_only=True))
    assert [key for key, _, _ in plan.result][-7:] == [key for key, _, _ in keys]


def test_the_chain_s_refusals_with_fallback(hip_lib):
    cf = cases.configs(hip_lib)
    gs = np.array([0, 1, 4], np.int32)
    j = dict({k: v for k, v in cf["j"][1].items() if k != "v_start"}, rank=gs, previous=_previous(2))
    with pytest.raises(ValueError, match="fallback must be True or a FallbackParams"):
        _plan(hip_lib, dict(j, fallback="yes"))
    with pytest.raises(ValueError, match="fallback needs previous= and rank="):
        _plan(hip_lib, dict(cf["j"][1], rank=gs, fallback=True))
    with pytest.raises(ValueError, match="fallback needs previous= and rank="):
        _plan(hip_lib, dict({k: v for k, v in cf["f"][1].items() if k != "v_start"}, previous=_previous(cases.B), fallback=True))
    with pytest.raises(ValueError, match="group 1 is empty"):
        _plan(hip_lib, dict(j, rank=np.array(cases.GROUP_START, np.int32), previous=_previous(3), fallback=True))
    with pytest.raises(ValueError, match="needs plan_agents="):
        _plan(hip_lib, dict({k: v for k, v in j.items() if k != "plan_agents"}, fallback=True))
    # the parameters are refused here, before anything is launched, as pqp_fallback_rows would refuse them behind every other stage
    bad = lambda **over: capi.fallback_default_params(hip_lib, **over)
    for prm, what in ((bad(levels=[(3.0, 5.0), (1.5, 2.5)]), "d must ascend"), (bad(levels=[(1.0, 1.0)] * 9), "1 <= L <= 8"), (bad(levels=[(0.0, 5.0)]), "finite and > 0"),
                      (bad(levels=[(1.5, math.inf)]), "finite and > 0"), (bad(levels=[(1.5, -2.0)]), "finite and > 0"), (bad(a_cap=-0.5), "a_cap must be >= 0"),
                      (bad(a_cap=math.nan), "a_cap must be >= 0")):
        with pytest.raises(ValueError, match=what):
            _plan(hip_lib, dict(j, fallback=prm))
    assert _plan(hip_lib, dict(j, fallback=False)).fallback is None and _plan(hip_lib, dict(j, fallback=None)).fallback is None


# ---- the C++ class, the kernels -------------------------------------------------------------------------------------------------------------------
def test_planner_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("fallback_demo")
    import torch
    if torch.cuda.is_available():
        return
    c = U.seeded_case(2, 5, 3, 2, seed=3)
    path = tmp_path / "case.bin"
    U.write_case(path, c["prev"], c["prev_m"], np.full(2, ST.STITCHED), c["state"], c["dt"], c["r"], c["m"], np.full(6, 5), np.full(6, 5))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no fallback planner" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


def test_the_kernels_use_no_scratch_and_no_lds(hip_lib):
    """one wavefront per plan, one per group: the level's constants and the cursor live in scalar registers, a lane's sample in vector
    registers - 128 and 18 VGPRs as the build stands, read here and not pinned - and the lanes meet through ballots and DPP, so there is no
    LDS; no vector register is spilled to memory and nothing sizes a stack"""
    report = build_util.kernel_report()
    for name in ("fallback_rows_kernel", "fallback_pick_kernel"):
        r = build_util.find_kernel(report, name)
        print(name + ":", r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, r
        assert 0 < r["VGPRs"] <= 512
