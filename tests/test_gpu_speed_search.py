"""pqp_speed_search on the GPU against the numpy restatement (tests/search_util.py, known answers in tests/test_speed_search.py).

Exact against the restatement: blocked, steps, reached, flags, cost and traj bit for bit (no sincos enters traj; the occupancy passes
through the device's sincos, and tests/test_speed_search.py holds every seed's |clear - margin| above 1e-6 m, a million times what a few
ulp of sin / cos can move a clearance by, and every cost gap that is not a tie above 1e-9); frames under test_gpu_agents_check.py's
bounds.  The shapes are the smallest that reach each piece of the kernels:
  the hand cases in one batch of mixed driven counts, through both forms, the device form inside sentinel-filled allocations;
  "tiles"  S = 70, Q = 5, m = 6, batch 5, two scenes: a second station tile, blocked runs across stations 31 / 32 and 63 / 64 (with Q = 5
           and six layers no plan gets to station 32, so the steps that cross those word edges are the next case's);
  "cap"    S = 64, Q = 63, q_up = q_down = 63, m = 3: the widest step and window at 4096 states exactly - and one state more refused;
  "long"   S = 200, Q = 19, m = 12, n = 300, ragged n_of and stop_before: 4000 states on 256 lanes, five waypoint tiles, steps across the
           words' edges up to station 120.
Every plan of these gets through.  tests/test_gpu_speed_search_table.py has the plans that die late, more layers than lanes, other steps
and weights, q_max = 0 - and holds the device form's whole `parents` table, of these cases too, to the restatement's."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import agents_util as A
import cpp_demo
import device_form as D
import search_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
EXACT = ("steps", "reached", "flags", "blocked")


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def circles(hand=False):
    return capi.car_circles(capi.car_default_geometry(**S.HAND_CAR)) if hand else capi.car_circles()


def _prm(p):
    return capi.search_default_params(**p)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """computed once per case and shared; nobody writes to it"""
    c = S.seeded(name)
    return c, S.run_case(c, circles())


def _host(handle, c, car=None, blocked=True):
    return handle.speed_search(c["paths"], c["profile"], c["v_start"], c["agents"], m=c.get("m"), n_of=c.get("n_of"), stop_before=c.get("stop_before"),
                               a_of=c.get("a_of"), scene_of=c.get("scene_of"), car=car, prm=_prm(c["prm"]), blocked=blocked)


TABLE_SENTINEL = 77                                          # what `parents` is filled with before a call: no step is that large


def _device(handle, c, car=None, table=None):
    """the device form through device_form: the outputs lie in sentinel-filled allocations with a guard band behind them.
    table: a list that gets `parents` [B][m][S][Q + 1] as the call left it (tests/test_gpu_speed_search_table.py reads it)"""
    import torch
    paths, profile, agents = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("paths", "profile", "agents"))
    B, n, stride = paths.shape
    n_scenes, a_max, m = agents.shape[:3]
    m = c.get("m") or m
    p = c["prm"]
    Sn, Q1 = p["stations"], p["q_max"] + 1
    opt = lambda k: None if c.get(k) is None else D.to_device(c[k], np.int32)
    out = dict(blocked=D.Out((B, m, S.words(Sn)), np.int32), steps=D.Out((B, m, 2), np.int32), traj=D.Out((B, m, 8)), cost=D.Out((B,)),
               reached=D.Out((B,), np.int32), flags=D.Out((B,), np.int32))
    frames = D.Out((n_scenes, a_max, m, 8)) if a_max else None
    parents = torch.full((B * m * Sn * Q1 + D.GUARD,), TABLE_SENTINEL, dtype=torch.uint8, device=D.dev())
    car = car if car is not None else capi.car_default_geometry()
    rc = D.call(handle, "pqp_speed_search_device", C.byref(_prm(p)), C.byref(car), B, n, stride, D.to_device(paths), opt("n_of"), opt("stop_before"),
                D.to_device(profile), D.to_device(c["v_start"]), m, n_scenes, a_max, D.to_device(agents) if a_max else None, opt("a_of"), opt("scene_of"),
                frames, out["blocked"], C.c_void_p(parents.data_ptr()), out["steps"], out["traj"], out["cost"], out["reached"], out["flags"])
    if rc:
        return rc, out, frames
    bytes_ = parents.cpu().numpy()
    assert (bytes_[B * m * Sn * Q1:] == TABLE_SENTINEL).all(), "the device form wrote behind the parents"
    if table is not None:
        table.append(bytes_[:B * m * Sn * Q1].reshape(B, m, Sn, Q1))
    return rc, {k: v.get() for k, v in out.items()}, None if frames is None else frames.get()


def _same(got, want, where):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (where, k, got[k].tolist() if got[k].size < 200 else None, want[k].tolist() if want[k].size < 200 else None)
    assert same_bits(got["cost"], want["cost"]), (where, got["cost"], want["cost"])
    assert same_bits(got["traj"], want["traj"]), where


def _hand_batch():
    """the hand cases that share the road's shape in one batch, one scene each: mixed driven counts, agent counts and parameters apart"""
    cases = S.hand_cases()
    groups = {}
    for name, c in cases.items():
        key = (tuple(sorted(c["prm"].items())), c["agents"].shape[2])
        groups.setdefault(key, []).append(name)
    batches = []
    for names in groups.values():
        cs = [cases[nm] for nm in names]
        a_max = max(c["agents"].shape[1] for c in cs)
        m = cs[0]["agents"].shape[2]
        agents = np.stack([np.concatenate([c["agents"][0], np.stack([S.absent(m)] * (a_max - c["agents"].shape[1]))]) if a_max > c["agents"].shape[1]
                           else c["agents"][0] for c in cs]) if a_max else np.zeros((len(cs), 0, m, 6))
        n = cs[0]["paths"].shape[1]
        batches.append((names, dict(paths=np.concatenate([c["paths"] for c in cs]), profile=np.concatenate([c["profile"] for c in cs]),
                                    v_start=np.concatenate([c["v_start"] for c in cs]), agents=agents, prm=cs[0]["prm"], m=cs[0].get("m"),
                                    n_of=np.array([c["n_of"][0] if c.get("n_of") is not None else n for c in cs], np.int32),
                                    a_of=np.array([(c["a_of"][0] if c.get("a_of") is not None else c["agents"].shape[1]) for c in cs], np.int32),
                                    scene_of=np.arange(len(cs), dtype=np.int32))))
    return batches


# ---- the hand cases --------------------------------------------------------------------------------------------------------------------
def test_the_hand_cases_through_both_forms(handle):
    car = capi.car_default_geometry(**S.HAND_CAR)
    seen = 0
    for names, c in _hand_batch():
        want = S.run_case(c, circles(True))
        each = [S.run_case(S.hand_cases()[nm], circles(True)) for nm in names]
        for b, one in enumerate(each):                       # in a batch as alone
            for k in EXACT + ("cost", "traj"):
                assert same_bits(np.asarray(want[k][b], dtype=np.float64), np.asarray(one[k][0], dtype=np.float64)), (names[b], k)
        got = _host(handle, c, car=car)
        _same(got, want, names)
        rc, dev, _ = _device(handle, c, car=car)
        assert rc == 0, handle.lib.pqp_last_error()
        _same(dev, want, names)
        seen += len(names)
    assert seen == len(S.hand_cases()) >= 14


# ---- the seeded shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SEEDED)
def test_shapes_against_the_restatement(handle, name):
    c, want = _reference(name)
    assert want["margins"]["clear"] >= S.CLEAR_MARGIN and min(want["margins"]["cost_gap"], want["margins"]["end_gap"]) >= S.COST_MARGIN
    got = _host(handle, c)
    _same(got, want, name)
    rc, dev, frames = _device(handle, c)
    assert rc == 0, handle.lib.pqp_last_error()
    _same(dev, want, name)
    fr = A.frames(c["agents"])
    assert same_bits(frames[..., [0, 1, 4, 5, 6, 7]], fr[..., [0, 1, 4, 5, 6, 7]]) and float(np.abs(frames[..., 2:4] - fr[..., 2:4]).max()) <= 1e-15
    print(f"{name}: reached {got['reached'].tolist()} flags {got['flags'].tolist()} cost {got['cost'].tolist()}")


def test_one_state_more_than_the_cap_is_refused_with_nothing_written(handle):
    c, _ = _reference("cap")
    assert c["prm"]["stations"] * (c["prm"]["q_max"] + 1) == S.MAX_STATES == capi.SEARCH_MAX_STATES
    over = dict(c, prm=dict(c["prm"], stations=65))
    rc, out, frames = _device(handle, over)
    assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_speed_search:")
    assert all(o.untouched() for o in out.values()) and frames.untouched()
    with pytest.raises(capi.PqpError, match="pqp_speed_search:"):
        _host(handle, over)


def test_the_steps_of_the_long_case_cross_the_words_edges():
    _, want = _reference("long")
    crossed = set()
    for steps, r in zip(want["steps"], want["reached"]):
        for k in range(1, r):
            crossed |= {e for e in (32, 64, 96) if steps[k - 1][0] < e <= steps[k][0]}
    assert crossed == {32, 64, 96}
    _, tiles = _reference("tiles")
    cells = S.unpack(tiles["blocked"], 70)
    assert (cells[..., 31] & cells[..., 32]).any() and (cells[..., 63] & cells[..., 64]).any()


# ---- what is not a number, what is empty, and where a path stands in the batch ----------------------------------------------------------
def test_not_finite_and_empty_paths_leave_their_neighbours_alone(handle):
    c, want = _reference("tiles")
    paths, profile, v_start = c["paths"].copy(), c["profile"].copy(), c["v_start"].copy()
    n_of = np.full(5, paths.shape[1], np.int32)
    paths[1, 40, 2] = math.nan                               # path 1: a heading below c
    n_of[3] = 0                                              # path 3: empty
    got = _host(handle, dict(c, paths=paths, profile=profile, v_start=v_start, n_of=n_of))
    for b in (0, 2, 4):
        for k in EXACT + ("cost", "traj"):
            assert same_bits(np.asarray(got[k][b], dtype=np.float64), np.asarray(want[k][b], dtype=np.float64)), (b, k)
    assert got["flags"][1] == S.NOT_FINITE and got["reached"][1] == 0 and math.isnan(got["cost"][1]) and np.isnan(got["traj"][1]).all()
    assert got["flags"][3] == S.EMPTY and got["reached"][3] == 0 and got["cost"][3] == math.inf and (got["traj"][3] == 0).all()
    for b in (1, 3):
        assert (got["steps"][b] == -1).all() and (got["blocked"][b] == 0).all()
    v_bad = v_start.copy()
    v_bad[0], v_bad[2] = -1.0, math.inf
    got = _host(handle, dict(c, v_start=v_bad))
    assert got["flags"][[0, 2]].tolist() == [S.NOT_FINITE] * 2 and same_bits(got["traj"][[1, 3, 4]], want["traj"][[1, 3, 4]])
    ref = S.run_case(dict(c, paths=paths, n_of=n_of), circles())
    assert np.array_equal(ref["flags"][[1, 3]], [S.NOT_FINITE, S.EMPTY])


def test_same_bits_at_any_position_in_any_batch_from_either_form(handle):
    c, want = _reference("long")
    src = 1
    for B, at in ((1, 0), (6, 5), (9, 3)):
        rng = np.random.default_rng(B)
        other = S.seeded("long")
        pick = rng.integers(0, 4, B)
        pick[at] = src
        d = dict(c, paths=other["paths"][pick], profile=other["profile"][pick], v_start=other["v_start"][pick], n_of=other["n_of"][pick],
                 stop_before=other["stop_before"][pick], scene_of=other["scene_of"][pick])
        got = _host(handle, d)
        rc, dev, _ = _device(handle, d)
        assert rc == 0
        for k in EXACT + ("cost", "traj"):
            assert same_bits(np.asarray(got[k][at], dtype=np.float64), np.asarray(want[k][src], dtype=np.float64)), (B, at, k)
            assert same_bits(np.asarray(dev[k], dtype=np.float64), np.asarray(got[k], dtype=np.float64)), (B, at, k)


# ---- the broad phase -------------------------------------------------------------------------------------------------------------------
def test_discs_riding_at_the_broad_phases_radius_do_not_show(handle):
    """discs at the broad phase's radius around every station's bounding centre and 1e-7 of it to either side, as test_gpu_agents_check.py
    places them: none comes within the margin - by the slack at least - so `blocked` is what it is without them"""
    c, want = _reference("tiles")
    cs, m, margin = circles(), c["m"], c["prm"]["margin"]
    rb = A.bounding_reach(cs)
    agents = np.concatenate([c["agents"], np.stack([np.stack([S.absent(m)] * 3)] * 2)], axis=1)
    for s, b in ((0, 0), (1, 1)):
        pose = S.stations(c["paths"][b], c["profile"][b], c["paths"].shape[1], c["prm"])[2]
        for a, scale in ((3, 1.0 - 1e-7), (4, 1.0 + 1e-7), (5, 1.0)):
            for k in range(m):
                x, y, h = pose[(11 * k + 7 * a) % len(pose), :3]
                bx, by = cs[6][0] * math.cos(h) - cs[6][1] * math.sin(h) + x, cs[6][0] * math.sin(h) + cs[6][1] * math.cos(h) + y
                far = rb + 0.5 + margin + A.SLACK + A.SLACK_REL * (abs(bx) + abs(by)) * 2
                phi = 0.9 * k + a
                agents[s, a, k] = [bx + scale * far * math.cos(phi), by + scale * far * math.sin(phi), 0.3, 0.0, 0.0, 0.5]
    d = dict(c, agents=agents, a_of=np.array([6, 6], np.int32))
    ref = S.run_case(dict(c, agents=agents, a_of=np.array([6, 6], np.int32)), cs)
    got = _host(handle, d)
    assert np.array_equal(got["blocked"], ref["blocked"])
    assert ref["margins"]["clear"] >= S.CLEAR_MARGIN


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(handle):
    c, _ = _reference("cap")
    bad = [dict(prm=dict(c["prm"], **kw)) for kw in (dict(dt=0.0), dict(ds=math.nan), dict(w_slow=-1.0), dict(w_accel=math.inf), dict(margin=-0.5),
                                                    dict(stations=0), dict(q_max=64), dict(q_max=-1), dict(q_up=-1), dict(q_down=-1))]
    for kw in bad:
        rc, out, frames = _device(handle, dict(c, **kw))
        assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_speed_search:"), kw
        assert all(o.untouched() for o in out.values()) and frames.untouched(), kw
    with pytest.raises(capi.PqpError, match="pqp_speed_search: scene_of outside"):
        _host(handle, dict(c, scene_of=np.array([0, 1], np.int32)))
    rc, dev, _ = _device(handle, dict(c, scene_of=np.array([-3, 9], np.int32)))            # the device form clamps
    assert rc == 0 and np.array_equal(dev["steps"], _reference("cap")[1]["steps"])


# ---- through the layers ----------------------------------------------------------------------------------------------------------------
def test_the_search_behind_the_chain(hip_lib):
    """optimize_path(..., speed=, agents=, search=) = the chain, the speed profile and pqp_speed_search one after the other: what it adds
    equals the stand-alone host call on the `out` and `profile` it returns - on every candidate, without a sampler, and with select and a
    sampler on the winners, where the sampler's check runs as well"""
    import chain_util
    B, m = 16, 8
    sc = chain_util.scenarios(B)
    gs = np.array([0, 8, 16], np.int32)
    sp = capi.speed_default_params(v_max=8.0)
    se = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    se.stations, se.w_accel, se.margin = 96, 0.25, 0.2
    agents = np.zeros((2, 2, m, 6))
    for s in range(2):                                       # agent 0 crosses candidate 8 s's line near its middle during layers 2 .. 4, agent 1 stands far away
        st, tg = sc["start"][8 * s], sc["target"][8 * s]
        agents[s, 0, :] = [0.5 * (st[0] + tg[0]), 0.5 * (st[1] + tg[1]), st[2] + 1.5, 2.2, 0.9, 0.1]
        agents[s, 0, [0, 1, 5, 6, 7], 3] = -1.0
        agents[s, 1, :] = [st[0] + 500.0, st[1] - 300.0, 0.0, 0.0, 0.0, 0.4]
    scene_all, scene_grp = (np.arange(B) // 8).astype(np.int32), np.array([1, 0], np.int32)
    runs = {}
    for name, kw in (("all", dict(speed=sp, v_start=np.linspace(0.0, 6.0, B), agents=agents, scene_of=scene_all, search=se)),
                     ("select", dict(select=gs, speed=sp, v_start=np.array([2.0, 5.0]), sample=capi.sample_default_params(dt=1.0), samples=m,
                                     agents=agents, scene_of=scene_grp, search=se))):
        h, hs = chain_util.handles(B)
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **kw)
        h.close(); hs.close()
    every, sel = runs["all"], runs["select"]
    assert list(every)[-5:] == ["search_steps", "search_traj", "search_cost", "search_reached", "search_flags"] and "first_hit" not in every
    assert "first_hit" in sel and sel["search_steps"].shape == (2, m, 2) and every["search_traj"].shape == (B, m, 8)
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    for res, paths, n_of, v0, scene in ((every, every["out"], every["n_out"], np.linspace(0.0, 6.0, B), scene_all),
                                        (sel, sel["best_paths"], sel["best_n"], np.array([2.0, 5.0]), scene_grp)):
        want = h.speed_search(paths, res["profile"], v0, agents, n_of=n_of, scene_of=scene, prm=se)
        for k in ("steps", "traj", "cost", "reached", "flags"):
            assert same_bits(np.asarray(res["search_" + k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)), k
    h.close()
    print(f"behind the chain: reached {every['search_reached'].tolist()} flags {every['search_flags'].tolist()}")
    assert (every["search_reached"] > 0).any()


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_searcher_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("search_demo")
    c, want = _reference("tiles")
    path = tmp_path / "case.bin"
    S.write_case(path, c)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5
    for b, line in enumerate(lines):
        v = [int(t) for t in line.split()[1:]]
        assert line.split()[0] == "path" and v[0] == b and v[1] == want["reached"][b] and v[2] == want["flags"][b], line
        assert v[3:] == want["steps"][b].ravel().tolist(), b
