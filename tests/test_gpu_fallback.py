"""pqp_fallback_rows and pqp_fallback_pick on the device, held to the restatement of tests/fallback_util.py over the cases of
fallback_util.device_cases().

What is asked bit for bit: flags, stop, stop_row and the columns s, v, a, t of every plan; the whole row of a plan on the previous plan
(chords: products, sums and quotients alone); zeros of a bad state; on the arc k, and the whole row where k0 = 0 and the heading is 0 (no
sincos enters a sum).  What is asked to 1e-9 m or rad: x, y and the heading of a plan on the arc, for coordinates within +-1000 m - the
bound pqp_predict_agents and the stitch hold their free-model poses to, the device's sincos against libm's.  With k0 = 0 the heading is
asked bit for bit too; x and y there are x0 + e cos h0, y0 + e sin h0 and are asked bit for bit at h0 = 0 alone (include/pqp.h says why).
The pick is asked bit for bit throughout.  tests/test_fallback.py shows that every comparison a flag or a segment hangs on keeps a margin
of 1e-6 in every case."""
import subprocess

import numpy as np
import pytest

import chain_plan_cases as cases
import chain_util
import cpp_demo
import device_form as D
import fallback_util as U
import stitch_util as ST
from path_optimizer_2_amd import capi
from shared_util import same_bits, same_bytes

pytestmark = pytest.mark.gpu
CASES = U.device_cases()
BY_NAME = {c["name"]: c for c in CASES}
TOL = 1e-9
KEYS = ("rows", "stop", "stop_row", "flags")
PICK_KEYS = ("final_traj", "final_m", "level", "flags")


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def restated():
    """every case's restatement, computed once and left unchanged"""
    return {c["name"]: U.run_case(c) for c in CASES}


def _prm(c):
    return capi.FallbackParams(c["levels"], c["a_cap"])


def _host(h, c, **over):
    a = dict(c, **over)
    return h.fallback_rows(a["state"], a["m"], dt=a["dt"], r=a["r"], prev=a["prev"], prev_m=a["prev_m"], stitch_flags=a["stitch_flags"], prm=_prm(a))


def _held_to(got, want, c):
    """the device's plans against the restatement's, as the module's docstring says; the greatest difference of a pose on the arc"""
    name = c["name"]
    assert np.array_equal(got["flags"], want["flags"]) and np.array_equal(got["stop_row"], want["stop_row"]), (name, got["flags"], want["flags"])
    assert same_bits(got["stop"], want["stop"]) and same_bits(got["rows"][..., 3:], want["rows"][..., 3:]), name
    bad, arc = want["flags"] == U.BAD, (want["flags"] & U.ARC) != 0
    assert not got["rows"][bad].any() and not got["stop"][bad].any()
    assert same_bits(got["rows"][~arc], want["rows"][~arc]), name
    err = 0.0
    if arc.any():
        err = float(np.abs(got["rows"][arc][..., :3] - want["rows"][arc][..., :3]).max())
        assert err <= TOL, (name, err)
        # k0 = 0: the heading is constrainAngle(h0), no sincos in it, and so are k, s, v, a, t above - bit for bit; x and y are
        # x0 + e cos h0 and y0 + e sin h0, the same bits only where sincos(h0) is exact on both sides: asked at h0 = 0, else 1e-9
        no_turn = c["state"][:, 3] == 0.0
        assert same_bits(got["rows"][no_turn][..., 2:], want["rows"][no_turn][..., 2:]), name
        straight = no_turn & (c["state"][:, 2] == 0.0)
        assert same_bits(got["rows"][straight], want["rows"][straight]), name
    assert np.isfinite(got["rows"]).all()
    return err


@pytest.mark.parametrize("name", list(BY_NAME))
def test_the_host_form_against_the_restatement(handle, restated, name):
    c = BY_NAME[name]
    got = _host(handle, c)
    err = _held_to(got, restated[name], c)
    print(f"{name}: flags {sorted(set(got['flags'].ravel().tolist()))}, poses on the arc within {err:.2e}")


def test_a_bad_group_leaves_its_neighbours_bits(handle):
    c = BY_NAME["bad_states"]
    got = _host(handle, c)
    bad = np.flatnonzero(got["flags"][:, 0] == U.BAD)
    assert bad.tolist() == [1, 3, 5]
    state = c["state"].copy()
    state[bad] = state[0]
    other = _host(handle, c, state=state)
    good = np.setdiff1d(np.arange(len(state)), bad)
    assert not (other["flags"][bad] & U.BAD).any()
    for k in KEYS:
        assert same_bytes(got[k][good], other[k][good]), k
    c = BY_NAME["stitch_flags"]
    got = _host(handle, c)
    assert np.flatnonzero(got["flags"][:, 0] == U.BAD).tolist() == [2, 6] and (got["flags"][[1, 4]] & U.ARC).all() and not (got["flags"][[0, 3]] & U.ARC).any()


@pytest.mark.parametrize("name", ["G5_mp65_m14_r10_L8_s11", "nan_rows", "stitch_flags"])
def test_the_same_group_elsewhere_in_a_larger_batch_has_the_same_bits(handle, name):
    c = BY_NAME[name]
    got = _host(handle, c)
    G, mp, stride = c["prev"].shape
    big = U.seeded_case(2 * G + 3, mp, c["m"], c["r"], seed=12, L=len(c["levels"]), stride=stride, dt=c["dt"])
    at = np.random.default_rng(11).permutation(2 * G + 3)[:G]
    big["prev"][at], big["state"][at] = c["prev"], c["state"]
    big["prev_m"][at] = mp if c["prev_m"] is None else c["prev_m"]
    flags = np.full(2 * G + 3, ST.STITCHED, np.int32)
    flags[at] = ST.STITCHED if c["stitch_flags"] is None else c["stitch_flags"]
    other = _host(handle, dict(c, prev=big["prev"], prev_m=big["prev_m"], state=big["state"], stitch_flags=flags))
    for k in KEYS:
        assert same_bytes(got[k], other[k][at]), (name, k)


def _device_form(h, c):
    G, L = c["state"].shape[0], len(c["levels"])
    M = (c["m"] - 1) * c["r"] + 1
    o = dict(rows=D.Out((G, L, M, 8)), stop=D.Out((G, L, 2)), stop_row=D.Out((G, L), np.int32), flags=D.Out((G, L), np.int32))
    opt = lambda a: None if a is None else D.to_device(a, np.int32)
    mp, stride = (0, 0) if c["prev"] is None else c["prev"].shape[1:]
    prm = _prm(c)
    rc = D.call(h, "pqp_fallback_rows_device", prm.array(), L, prm.level_rows()[1], float(c["dt"]), c["r"], c["m"], G, mp, stride,
                None if c["prev"] is None else D.to_device(c["prev"]), opt(c["prev_m"]), D.to_device(c["state"]), opt(c["stitch_flags"]),
                *(o[k] for k in KEYS))
    return rc, o


@pytest.mark.parametrize("name", ["G67_mp64_m130_r1_L1_s11", "G5_mp130_m65_r1_L8_s8", "G1_mp2_m1_r10_L3_s8", "ragged", "stitch_flags", "nan_rows", "arc"])
def test_the_device_form_on_guarded_buffers_gives_the_host_form_s_bits(handle, name):
    c = BY_NAME[name]
    host = _host(handle, c)
    rc, o = _device_form(handle, c)
    assert rc == 0, handle.lib.pqp_last_error()
    for k in KEYS:
        assert same_bytes(o[k].get(), host[k]), (name, k)


def test_refusals_on_the_device_leave_the_outputs_untouched(handle):
    c = BY_NAME["ragged"]
    for over in (dict(dt=0.0), dict(r=0), dict(a_cap=-1.0), dict(levels=np.array([[3.0, 5.0], [1.5, 2.5]])), dict(levels=np.zeros((9, 2)) + 1.0)):
        rc, o = _device_form(handle, dict(c, **over))
        assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_fallback_rows:"), over
        assert all(v.untouched() for v in o.values()), over


# ---- the pick ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,L,M", [(1, 1, 1), (5, 3, 65), (67, 8, 9), (7, 3, 130)])
def test_the_pick_against_the_restatement(handle, G, L, M):
    c = U.pick_case(G, L, M, seed=G + L + M)
    want, got = U.fallback_pick(**c), handle.fallback_pick(**c)
    for k in PICK_KEYS:
        assert same_bytes(got[k], want[k].astype(got[k].dtype)), (k, got[k], want[k])
    keeps = c["best"] >= 0
    assert same_bits(got["final_traj"][keeps], c["best_traj"][keeps]) and np.array_equal(got["final_m"][keeps], c["best_m"][keeps])
    assert (got["level"][keeps] == -1).all() and not got["flags"][keeps].any()
    # best = NULL falls back everywhere; without the verdicts every level that is not short or bad is usable
    for kw in (dict(first_hit=c["first_hit"], first_collision=c["first_collision"]), dict(first_hit=c["first_hit"]), dict()):
        want, got = U.fallback_pick(c["rows"], c["row_flags"], **kw), handle.fallback_pick(c["rows"], c["row_flags"], **kw)
        for k in PICK_KEYS:
            assert same_bytes(got[k], want[k].astype(got[k].dtype)), (k, kw.keys())
        assert ((got["flags"] & U.TAKEN) != 0).sum() == G - int((got["flags"] == U.BAD).sum())
    # the device form on guarded buffers
    o = dict(final_traj=D.Out((G, M, 8)), final_m=D.Out((G,), np.int32), level=D.Out((G,), np.int32), flags=D.Out((G,), np.int32))
    i32 = lambda a: D.to_device(a, np.int32)
    rc = D.call(handle, "pqp_fallback_pick_device", G, L, M, i32(c["best"]), D.to_device(c["best_traj"]), i32(c["best_m"]), D.to_device(c["rows"]),
                i32(c["row_flags"]), i32(c["first_hit"]), i32(c["first_collision"]), *(o[k] for k in PICK_KEYS))
    assert rc == 0, handle.lib.pqp_last_error()
    host = handle.fallback_pick(**c)
    for k in PICK_KEYS:
        assert same_bytes(o[k].get(), host[k]), k


def test_the_pick_over_every_combination_of_eight_levels(handle):
    """fallback_util.pick_combinations(8, 6) - all 3^8 patterns of usable and hit levels with two contact rows, and the collided and
    short kinds layered over them - and verdicts below zero, which are read as they are"""
    L, M = 8, 6
    rf, hit, col = U.pick_combinations(L, M)
    G = len(rf)
    rows = np.random.default_rng(8).uniform(-5.0, 5.0, (G, L, M, 8))
    want, got = U.fallback_pick(rows, rf, first_hit=hit, first_collision=col), handle.fallback_pick(rows, rf, first_hit=hit, first_collision=col)
    for k in PICK_KEYS:
        assert same_bytes(got[k], want[k].astype(got[k].dtype)), k
    assert set(got["level"].tolist()) == set(range(L)) and (got["flags"] & U.NOT_CLEAR).any()
    junk = handle.fallback_pick(rows[:2], rf[:2] * 0, first_hit=np.full(2 * L, -7), first_collision=np.array([-9] * L + [-2 ** 31] * L))
    assert junk["level"].tolist() == [L - 1, L - 1] and (junk["flags"] == U.TAKEN | U.NOT_CLEAR).all() and same_bits(junk["final_traj"], rows[:2, L - 1])


def test_a_disc_across_the_old_plan_the_gentle_level_hits_the_harder_one_stops_short(handle):
    """a straight plan along x at 8 m/s, the car at s = 10 m; a pedestrian (a disc of 0.4 m) steps onto the plan at t = 1.5 s, 2.5 m
    beyond where the front circles of level 2's plan come to stand, and stays.  Level 0 (1.5 m/s^2) needs 23.7 m and runs over the
    place, level 1 (3 m/s^2) needs 13.0 m and does too, level 2 (6 m/s^2) stands after 6.9 m; the pick takes level 2, and that plan
    passes pqp_agents_check by itself"""
    dt, m, r = 0.5, 13, 2
    M = (m - 1) * r + 1
    plan = ST.arc_plan(100, dt=0.125, v=8.0, a=0.0, curvature=0.0, x0=0.0, y0=0.0, h0=0.0)
    state = U.state_on(plan, 10, v=8.0, a=0.0)[None]
    rows = handle.fallback_rows(state, m, dt=dt, r=r, prev=plan[None])
    assert not rows["flags"].any() and rows["stop"][0, :, 1].tolist() == sorted(rows["stop"][0, :, 1].tolist(), reverse=True)
    car = capi.car_default_geometry(handle.lib)
    front = float(capi.car_circles(car, handle.lib)[:, 0].max())
    t = U.times(dt, r, m)
    agents = np.zeros((1, 1, M, 6))
    agents[0, 0] = [10.0 + rows["stop"][0, 2, 1] + front + 2.5, 0.0, 0.0, 0.0, 0.0, 0.4]
    agents[0, 0, t < 1.5, 3] = -1.0                                 # not there yet
    checked = handle.agents_check(rows["rows"].reshape(3, M, 8), agents)
    first_hit = checked["first_hit"]
    assert first_hit[0] < M and first_hit[1] < M and first_hit[2] == M, (first_hit, rows["stop"])
    got = handle.fallback_pick(rows["rows"], rows["flags"], first_hit=first_hit)
    assert got["level"][0] == 2 and got["flags"][0] == U.TAKEN and got["final_m"][0] == M and same_bits(got["final_traj"][0], rows["rows"][0, 2])
    alone = handle.agents_check(got["final_traj"], agents)
    assert alone["first_hit"][0] == M and alone["hit_agent"][0] == -1
    assert got["final_traj"][0, -1, 5] == 0.0 and got["final_traj"][0, -1, 0] + front < agents[0, 0, -1, 0] - 0.4
    # with the disc 5 m nearer, and there from the start, every level hits: the latest contact is taken, and says so
    agents[0, 0, :, 0] -= 5.0
    agents[0, 0, :, 3] = 0.0
    first_hit = handle.agents_check(rows["rows"].reshape(3, M, 8), agents)["first_hit"]
    got = handle.fallback_pick(rows["rows"], rows["flags"], first_hit=first_hit)
    assert (first_hit < M).all() and got["flags"][0] == U.TAKEN | U.NOT_CLEAR and got["level"][0] == int(np.flatnonzero(first_hit == first_hit.max())[-1])


def test_planner_gives_the_wrapper_s_bits(handle, tmp_path):
    exe = cpp_demo.build("fallback_demo")
    c = U.seeded_case(7, 40, 8, 10, seed=21, dt=0.5, ragged=False)
    c["prev_m"][2], c["prev_m"][5] = 1, 0
    flags = np.full(7, ST.STITCHED, np.int32)
    flags[3], flags[4] = ST.REPLAN | ST.LATERAL, ST.BAD
    rng = np.random.default_rng(2)
    M = (c["m"] - 1) * c["r"] + 1
    hit = np.where(rng.random(21) < 0.5, M, rng.integers(0, M, 21)).astype(np.int32)
    col = np.where(rng.random(21) < 0.7, M, rng.integers(0, M, 21)).astype(np.int32)
    path = tmp_path / "case.bin"
    U.write_case(path, c["prev"], c["prev_m"], flags, c["state"], c["dt"], c["r"], c["m"], hit, col)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    prev = np.ascontiguousarray(c["prev"][:, :, :8])
    prev[:, :, 7] = 0.0                                              # (the planner's states carry no time; the column is not read)
    want = handle.fallback_rows(c["state"], c["m"], dt=c["dt"], r=c["r"], prev=prev, prev_m=c["prev_m"], stitch_flags=flags)
    pick = handle.fallback_pick(want["rows"], want["flags"], first_hit=hit, first_collision=col)
    assert (want["flags"] & U.ARC).any() and (want["flags"] == U.BAD).any() and not (want["flags"][0] & U.ARC).any() and pick["level"][4] == -1
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    for p in range(21):
        g, l = divmod(p, 3)
        assert lines[p][0] == "plan" and [int(v) for v in lines[p][1:3]] == [want["flags"][g, l], want["stop_row"][g, l]]
        assert same_bits(np.array([float(v) for v in lines[p][3:]]), want["stop"][g, l])
    at = 21
    for g in range(7):
        n = int(pick["final_m"][g])
        assert lines[at][0] == "group" and [int(v) for v in lines[at][1:]] == [pick["level"][g], pick["flags"][g], n]
        rows = lines[at + 1:at + 1 + n]
        assert all(l[0] == "row" for l in rows) and same_bits(np.array([[float(v) for v in l[1:]] for l in rows]).reshape(n, 8), pick["final_traj"][g, :n])
        at += 1 + n
    assert at == len(lines)


# ---- three cycles through the chain -----------------------------------------------------------------------------------------------------------
LAYERS, R = 5, 2
FINE = (LAYERS - 1) * R + 1
GROUP_START = np.array([0, 2, 4], np.int32)


def _measured_on(traj, count, lat=0.1):
    """per group a car 40 % of the way from row 0 to row 1 of its plan, `lat` m to its left, at that time (a group without a plan: zeros)"""
    G = len(count)
    meas, t_now = np.zeros((G, 6)), np.zeros(G)
    for g in range(G):
        if count[g] >= 2:
            at = traj[g, 0] + 0.4 * (traj[g, 1] - traj[g, 0])
            at[2] = traj[g, 0, 2]
            meas[g], t_now[g] = ST.displaced(at, 0.0, lat, 0.0), at[7]
    return meas, t_now


def test_three_cycles_through_the_chain(hip_lib):
    """cycle 0 plans on an open road and ranks; cycle 1 starts on its winners, and a standing agent - a disc of 10 m, its rim 14 m
    ahead - lies across every candidate on the fine steps for the whole horizon: no candidate is eligible, and each group gets the
    gentlest braking plan that stands in front of it; cycle 2 stitches onto that plan, where the ranking's empty best_traj leaves it
    nothing to stitch onto.  Cycle 1 without fallback= is cycle 1 with it, bit for bit in every key they share"""
    sc = chain_util.scenarios(4)
    h, hs = chain_util.handles(cases.B, max_n=(cases.N_MAX, cases.N_MAX))
    sp = capi.speed_default_params(hip_lib, v_max=8.0)
    se = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    se.stations, se.margin = 96, 0.2
    absent = lambda steps: np.tile(np.array(U.PR.ABSENT_ROW), (2, 1, steps, 1))
    # (a group's candidates share their group's map, as its braking plans are checked on the first candidate's: candidates 1 and 3 run
    #  on their neighbours' maps)
    kw = dict(map_of=np.array([0, 0, 2, 2], np.int32), smoother=hs, cfg=h.chain_config(**cases.CHAIN_CONFIG), check_footprint=True, speed=sp, search=se,
              refine=capi.refine_default_params(hip_lib, w_jerk=0.5, window=6), plan_samples=R, agents=absent(LAYERS), scene_of=np.array([0, 0, 1, 1], np.int32),
              rank=GROUP_START)
    run = lambda start, more: h.optimize_path(sc["pts"], sc["n_pts"], start, sc["target"], sc["dist"], sc["geom"], **dict(kw, **more))
    first = run(sc["start"], dict(v_start=np.full(4, 4.0), plan_agents=absent(FINE)))
    best_traj, best_m = first["best_traj"], first["best_m"]
    assert (first["rank_best"] >= 0).all() and (best_m >= 2).all(), (first["rank_best"], best_m, first["search_flags"], first["stage"])

    meas, t_now = _measured_on(best_traj, best_m)
    blocked = absent(FINE)
    for g in range(2):
        x, y, hd = best_traj[g, 1, :3]
        blocked[g, 0, :] = [x + 24.0 * np.cos(hd), y + 24.0 * np.sin(hd), 0.0, 0.0, 0.0, 10.0]
    second_kw = dict(previous=(best_traj, best_m, meas, t_now, None), plan_agents=blocked)
    second = run(None, dict(second_kw, fallback=True))
    plain = run(None, second_kw)
    assert list(second)[:len(plain)] == list(plain) and list(second)[len(plain):] == ["final_traj", "final_m", "fallback_level", "fallback_flags", "fallback_rows",
                                                                                      "fallback_first_hit", "fallback_first_collision"]
    for k, v in plain.items():
        assert same_bytes(second[k], v), k
    assert (second["stitch_flags"] == ST.STITCHED).all(), second["stitch_flags"]
    assert (second["rank_best"] == -1).all() and not second["best_m"].any(), (second["rank_best"], second["plan_first_hit"], second["plan_m_of"])
    level, flags, final = second["fallback_level"], second["fallback_flags"], second["final_traj"]
    print("levels", level, "flags", flags, "first hits", second["fallback_first_hit"], "first collisions", second["fallback_first_collision"])
    assert (level >= 0).all() and (flags & U.TAKEN).all() and not (flags & (U.NOT_CLEAR | U.BAD)).any() and (second["final_m"] == FINE).all()
    L = 3
    for g in range(2):
        assert same_bits(final[g], second["fallback_rows"][g, level[g]])
        assert second["fallback_first_hit"][g * L + level[g]] == FINE and second["fallback_first_collision"][g * L + level[g]] == FINE
        assert final[g, -1, 5] == 0.0 and np.hypot(*(final[g, -1, :2] - blocked[g, 0, 0, :2])) > 10.0          # it stands, in front of the agent
    # the plans are the restatement's: on the plan the stitch read, from the state it wrote
    want = U.fallback_rows(second["stitch_state"], U.LEVELS, U.A_CAP, 1.0, R, LAYERS, best_traj, best_m, second["stitch_flags"])
    assert same_bits(second["fallback_rows"], want["rows"])

    meas, t_now = _measured_on(final, second["final_m"])
    third = run(None, dict(previous=(final, second["final_m"], meas, t_now, None), plan_agents=blocked))
    lost = run(None, dict(previous=(second["best_traj"], second["best_m"], meas, t_now, None), plan_agents=blocked))
    assert (third["stitch_flags"] == ST.STITCHED).all(), third["stitch_flags"]
    assert (lost["stitch_flags"] & ST.NO_PREVIOUS).all() and not (lost["stitch_flags"] & ST.STITCHED).any(), lost["stitch_flags"]
    h.close(); hs.close()
