"""pqp_speed_search restated in numpy float64 and Python integers (include/pqp.h states the definition): the stations and their poses, the
envelope, the occupancy of the path-time plane, the layered dynamic program with its parents, the outputs and the flags - one path at a
time, operation by operation in the stated order.  The circle test is agents_util's, the interpolation is pqp_sample_trajectory's with e
given (sample_util's constrain_angle).  Every operation is a correctly rounded IEEE one and numpy fuses none: steps, reached, flags, cost
and traj agree with the device bit for bit; `blocked` passes through the device's sincos, a few ulp from libm's, so it agrees exactly where
no |clear - margin| is within reach of that (the decision margins search() reports say where)."""
import itertools
import math

import numpy as np

import agents_util as A
import sample_util as T
import speed_util as V

NO_PLAN, START_BLOCKED, GRID_SHORT, ARRIVED, EMPTY, NOT_FINITE = 1, 2, 4, 8, 16, 32
DEFAULTS = dict(dt=1.0, ds=0.5, w_slow=1.0, w_accel=1.0, margin=0.0, stations=128, q_max=20, q_up=3, q_down=6)
MAX_STATES = 4096
INF = math.inf


def params(**over):
    return dict(DEFAULTS, **over)


def from_speed(sp, dt, ds):
    """pqp_search_params_from_speed; None where it refuses"""
    q = math.floor(sp["v_max"] * dt / ds)
    if not 0 <= q <= 63:
        return None
    return params(dt=dt, ds=ds, q_max=q, q_up=min(max(1, math.floor(sp["a_max"] * (dt * dt) / ds)), 63),
                  q_down=min(max(1, math.floor(sp["d_max"] * (dt * dt) / ds)), 63))


def words(S):
    return (S + 31) // 32


def pack(cells):
    """bool [m][S] -> int32 [m][W]: bit j & 31 of word j >> 5"""
    m, S = cells.shape
    out = np.zeros((m, words(S)), np.uint32)
    for j in range(S):
        out[:, j >> 5] |= cells[:, j].astype(np.uint32) << np.uint32(j & 31)
    return out.view(np.int32)


def unpack(blocked, S):
    """int32 [..][W] -> bool [..][S]"""
    w = np.asarray(blocked).view(np.uint32)
    return np.stack([(w[..., j >> 5] >> np.uint32(j & 31)) & 1 for j in range(S)], axis=-1).astype(bool)


def stations(path, profile, c, prm):
    """the stations on the path and what stands there: (J, grid_short, pose [J][4] = x, y, heading, k, venv [J], qenv [J])"""
    S, Q, ds, dt = prm["stations"], prm["q_max"], np.float64(prm["ds"]), np.float64(prm["dt"])
    x, y, h, k = (path[:c, q] for q in (0, 1, 2, 5))
    s, v, a = (profile[:c, q] for q in range(3))
    M = np.maximum.accumulate(s)
    sigma = np.arange(S).astype(np.float64) * ds
    J = int((sigma <= M[c - 1]).sum())
    assert (sigma[:J] <= M[c - 1]).all()                     # a prefix: sigma ascends
    sg = sigma[:J]
    with np.errstate(all="ignore"):
        i = np.maximum(np.searchsorted(M, sg, side="right") - 1, 0)          # #{ i' < c : M_i' <= sigma } - 1
        inside = i < c - 1
        pose = np.zeros((J, 4))
        w = np.zeros(J)
        pose[~inside] = [x[c - 1], y[c - 1], h[c - 1], k[c - 1]]
        w[~inside] = v[c - 1] * v[c - 1]
        if inside.any():
            i0 = i[inside]
            i1 = i0 + 1
            dx, dy = x[i1] - x[i0], y[i1] - y[i0]
            d = np.sqrt(dx * dx + dy * dy)
            e = np.fmin(np.fmax(sg[inside] - s[i0], 0.0), d)
            lam = np.where(d > 0.0, e / np.where(d > 0.0, d, 1.0), 0.0)
            r = np.zeros((len(i0), 4))
            r[:, 0] = x[i0] + lam * dx
            r[:, 1] = y[i0] + lam * dy
            r[:, 2] = T.constrain_angle(h[i0] + lam * T.constrain_angle(h[i1] - h[i0]))
            r[:, 3] = k[i0] + lam * (k[i1] - k[i0])
            pose[inside] = r
            w[inside] = v[i0] * v[i0] + (2.0 * a[i0]) * e
        venv = np.sqrt(np.fmax(w, 0.0))
        qenv = np.fmin(np.floor(venv * dt / ds), np.float64(Q)).astype(np.int64)
    return J, bool(M[c - 1] > sigma[S - 1]), pose, venv, qenv


def occupancy(pose, fr, circles, margin):
    """pose [J][>= 3], fr [A][m][8] (the scene's frames, its agent count applied) -> (cells bool [m][J], clear [m][J][A])"""
    J, (A_, m) = pose.shape[0], fr.shape[:2]
    cells, clear = np.zeros((m, J), bool), np.full((m, J, A_), INF)
    finite = np.isfinite(pose[:, :3]).all(axis=1)
    for k in range(m):
        bad_row = bool(np.isnan(fr[:, k, 7]).any())
        if J and A_:
            fk = np.repeat(fr[:, k:k + 1], int(finite.sum()), axis=1)         # every station against the agents of step k
            clear[k][finite] = A.clear_matrix(pose[finite], fk, circles)
        cells[k] = (clear[k] < margin).any(axis=1) | ~finite | bad_row
    return cells, clear


def reference_steps(qenv, J, Q):
    """qref_j: the largest step the envelope admits from station j, max over r in 1 .. min(Q, j_last - j) of min(r, max(qenv_j, qenv_{j+r}))"""
    return [max([min(r, max(int(qenv[j]), int(qenv[j + r]))) for r in range(1, min(Q, J - 1 - j) + 1)], default=0) for j in range(J)]


def _gap(values):
    """the least difference between the best and the others that is not a tie"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    d = v[1:] - v[0]
    d = d[d > 0]
    return float(d[0]) if d.size else INF


def dp(cells, qenv, J, q0, prm, swept=True):
    """the layered search on cells bool [m][>= J]: (reached, steps [reached][2], cost, margins dict(cost_gap, end_gap), parents, qref).
    parents: per living layer k the map state (j, q) -> the step q' of its parent (layer 0: empty; a layer's keys are its living states);
    qref [J]: reference_steps"""
    m = cells.shape[0]
    Q, q_up, q_down = prm["q_max"], prm["q_up"], prm["q_down"]
    w_slow, w_accel = np.float64(prm["w_slow"]), np.float64(prm["w_accel"])
    layers, parents = [], []
    qref = reference_steps(qenv, J, Q)
    cost_gap = INF
    first = {}
    if J > 0 and not cells[0, 0]:
        first[(0, q0)] = np.float64(0.0)
    layers.append(first)
    parents.append({})
    for k in range(1, m):
        prev, cur, par = layers[-1], {}, {}
        if not prev:
            break
        for j in range(min(J, max(jq[0] for jq in prev) + Q + 1)):           # beyond: j - q lies behind every living state of the layer before
            for q in range(min(Q, j) + 1):
                jp = j - q
                qe = max(int(qenv[jp]), int(qenv[j]))
                if q > qe:
                    continue
                if swept and (cells[k - 1, jp:j + 1].any() or cells[k, jp:j + 1].any()):
                    continue
                if not swept and (cells[k - 1, jp] or cells[k, j]):          # the mistake test (d) must see: only the two ends are tested
                    continue
                slow = w_slow * np.float64(qref[jp] - q)
                cands = []
                for qp in range(max(q - q_up, 0), min(q + q_down, Q) + 1):
                    cp = prev.get((jp, qp))
                    if cp is None:
                        continue
                    dq = q - qp
                    with np.errstate(over="ignore"):
                        cands.append((cp + (w_accel * np.float64(dq * dq) + slow), qp))
                cands = [cq for cq in cands if cq[0] < INF]
                if not cands:
                    continue
                best = min(cands, key=lambda cq: (cq[0], cq[1]))             # the lowest q' wins a tie
                cur[(j, q)], par[(j, q)] = best
                cost_gap = min(cost_gap, _gap([cq[0] for cq in cands]))
        if not cur:
            break
        layers.append(cur)
        parents.append(par)
    if not layers[0]:
        return 0, np.zeros((0, 2), np.int32), INF, dict(cost_gap=cost_gap, end_gap=INF), [{}], qref
    last = layers[-1]
    end = min(last, key=lambda jq: (last[jq], -jq[0], jq[1]))
    steps = [end]
    for k in range(len(layers) - 1, 0, -1):
        j, q = steps[-1]
        steps.append((j - q, parents[k][(j, q)]))
    steps.reverse()
    return len(layers), np.array(steps, np.int32), float(last[end]), dict(cost_gap=cost_gap, end_gap=_gap(list(last.values()))), parents, qref


def search(path, profile, v_start, fr, circles, m, n_of=None, stop_before=None, prm=None, swept=True, cells=None):
    """one path [n][stride >= 6] with its profile [n][4] against its scene's frames fr [A][m][8] ->
    dict(steps [m][2], traj [m][8], cost, reached, flags, blocked [m][W], margins dict(clear, cost_gap, end_gap), qenv, J, q0, parents, qref):
    parents and qref as dp() gives them - the whole table, not the winning plan alone; q0 is the start's step.
    swept=False takes the swept-range rule out; cells: a bool [m][S] to search in place of the occupancy (the brute-force cases)"""
    prm = params(**(prm or {}))
    path, profile = np.asarray(path, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    S, Q = prm["stations"], prm["q_max"]
    ds, dt = np.float64(prm["ds"]), np.float64(prm["dt"])
    c = T.driven(path.shape[0], n_of, stop_before)
    out = dict(steps=np.full((m, 2), -1, np.int32), traj=np.zeros((m, 8)), cost=INF, reached=0, flags=0, blocked=np.zeros((m, words(S)), np.int32),
               margins=dict(clear=INF, cost_gap=INF, end_gap=INF), qenv=np.zeros(0, np.int64), J=0, q0=0, parents=[{}], qref=[])
    if c == 0:
        out["flags"] = EMPTY
        return out
    v0 = np.float64(v_start)
    if not (np.isfinite(path[:c][:, [0, 1, 2, 5]]).all() and np.isfinite(profile[:c, :3]).all() and np.isfinite(v0) and v0 >= 0.0):
        out["traj"][:] = math.nan
        out["cost"], out["flags"] = math.nan, NOT_FINITE
        return out
    J, grid_short, pose, venv, qenv = stations(path, profile, c, prm)
    full = np.zeros((m, S), bool)
    if cells is None:
        got, clear = occupancy(pose, fr, circles, np.float64(prm["margin"]))
        full[:, :J] = got
        fin = clear[np.isfinite(clear)]
        out["margins"]["clear"] = float(np.abs(fin - prm["margin"]).min()) if fin.size else INF
    else:
        full[:, :J] = np.asarray(cells, bool)[:, :J]
    out["blocked"], out["qenv"], out["J"] = pack(full), qenv, J
    with np.errstate(all="ignore"):
        q0 = int(np.fmin(np.fmax(np.rint(v0 * dt / ds), 0.0), np.float64(Q)))
    reached, steps, cost, margins, out["parents"], out["qref"] = dp(full, qenv, J, q0, prm, swept)
    out["margins"].update(margins)
    out["q0"] = q0
    out["reached"], out["cost"] = reached, cost
    out["steps"][:reached] = steps
    for k in range(reached):
        j, q = (int(v) for v in steps[k])
        dq = int(steps[k + 1][1]) - q if k + 1 < reached else 0
        out["traj"][k] = [pose[j, 0], pose[j, 1], pose[j, 2], pose[j, 3], np.float64(j) * ds, np.float64(q) * ds / dt,
                          np.float64(dq) * ds / (dt * dt), np.float64(k) * dt]
    out["flags"] = (NO_PLAN if reached < m else 0) | (START_BLOCKED if reached == 0 else 0) | (GRID_SHORT if grid_short else 0) | \
                   (ARRIVED if reached > 0 and int(steps[-1][0]) == J - 1 and not grid_short else 0)
    return out


def search_batch(paths, profile, v_start, agents, circles, m=None, n_of=None, stop_before=None, a_of=None, scene_of=None, prm=None, frames_in=None,
                 swept=True):
    """the whole entry point: paths [B][n][stride], profile [B][n][4], agents [n_scenes][a_max][m][6] -> dict of stacked outputs and
    `margins`, the least of every decision margin over the batch.  scene_of is clamped as the device form clamps it; frames_in: frames to
    take in place of agents_util.frames(agents)"""
    agents = np.asarray(agents, dtype=np.float64)
    n_scenes, a_max = agents.shape[:2]
    m = agents.shape[2] if m is None else m
    fr = A.frames(agents) if frames_in is None else np.asarray(frames_in, dtype=np.float64)
    pick = lambda a, b: None if a is None else a[b]
    got = []
    for b in range(len(paths)):
        s = 0 if scene_of is None else min(max(int(scene_of[b]), 0), n_scenes - 1)
        A_ = a_max if a_of is None else min(max(int(a_of[s]), 0), a_max)
        got.append(search(paths[b], profile[b], v_start[b], fr[s, :A_].reshape(A_, m, 8), circles, m, pick(n_of, b), pick(stop_before, b), prm, swept))
    res = {k: np.stack([np.asarray(g[k]) for g in got]) for k in ("steps", "traj", "cost", "reached", "flags", "blocked")}
    res["reached"], res["flags"] = res["reached"].astype(np.int32), res["flags"].astype(np.int32)
    res["margins"] = {k: min(g["margins"][k] for g in got) for k in ("clear", "cost_gap", "end_gap")}
    res["each"] = got
    return res


def enumerate_plans(cells, qenv, J, q0, prm):
    """every admissible step sequence by brute force, layer by layer: (reached, [(cost, [(j, q), ...]), ...]), the sequences that get to
    the deepest layer any of them gets to.  The cost of a sequence is the sum of its edges in order - the additions search() makes"""
    m = cells.shape[0]
    Q, q_up, q_down = prm["q_max"], prm["q_up"], prm["q_down"]
    w_slow, w_accel = np.float64(prm["w_slow"]), np.float64(prm["w_accel"])
    qref = reference_steps(qenv, J, Q)
    if J == 0 or cells[0, 0]:
        return 0, []
    level = [(np.float64(0.0), [(0, q0)])]
    for k in range(1, m):
        nxt = []
        for cost, seq in level:
            jp, qp = seq[-1]
            for q in range(max(qp - q_down, 0), min(qp + q_up, Q) + 1):
                j = jp + q
                if j > J - 1:
                    continue
                qe = max(int(qenv[jp]), int(qenv[j]))
                if q > qe or cells[k - 1, jp:j + 1].any() or cells[k, jp:j + 1].any():
                    continue
                edge = w_accel * np.float64((q - qp) * (q - qp)) + w_slow * np.float64(qref[jp] - q)
                nxt.append((cost + edge, seq + [(j, q)]))
        if not nxt:
            return k, level
        level = nxt
    return m, level


def first_plan(plans):
    """the enumeration's first plan under the rules: the least cost, then the largest last j, then the smallest last q, then - among
    sequences that end in the same state at the same cost - the lowest q' at every step from the back (the parent rule)"""
    def key(cs):
        cost, seq = cs
        return (cost, -seq[-1][0], seq[-1][1], tuple(q for _, q in reversed(seq)))
    return min(plans, key=key)


# ---- paths and profiles for the cases --------------------------------------------------------------------------------------------------
HAND_CAR = A.HAND_CAR


def straight(n, step=0.5, stride=7):
    """[n][stride]: along x at heading 0, `step` between waypoints, no curvature"""
    p = np.zeros((n, stride))
    p[:, 0] = step * np.arange(n)
    return p


def profile_of(path, v_start, n_of=None, stop_before=None, v_end=None, prm=None):
    """[n][4] by the speed profile's restatement (speed_util.profile)"""
    rows, _ = V.profile(path, v_start, n_of=n_of, stop_before=stop_before, v_end=v_end, prm=prm)
    return rows


def agent_rows(m, x, y, hl, hw, radius=0.0, heading=0.0):
    """[m][6]: an agent that stands still"""
    return np.tile(np.array([x, y, heading, hl, hw, radius], dtype=np.float64), (m, 1))


def absent(m):
    r = np.zeros((m, 6))
    r[:, 3] = -1.0
    return r


HAND_N, HAND_M = 41, 8                                       # 20 m of road, eight layers


def hand_cases():
    """name -> dict(paths [1][n][7], profile [1][n][4], v_start [1], agents [1][A][m][6], prm[, n_of, stop_before, m]).  A straight road
    along x at heading 0 with 0.5 m between waypoints, the hand car (circles at x = -0.5 .. 3.5 + r, see agents_util), dt = 1, ds = 0.5: a
    station is a waypoint.  tests/test_speed_search.py states the answers"""
    m = HAND_M
    road = straight(HAND_N)
    free = profile_of(road, 0.0, v_end=0.0)
    quick = params(stations=48, w_accel=2.0 ** -6)           # a change of step costs next to nothing: the plan runs along the limits
    base = dict(paths=road[None], profile=free[None], v_start=np.array([0.0]), prm=quick)
    rolling = dict(base, v_start=np.array([2.0]), profile=profile_of(road, 2.0, v_end=0.0)[None])
    none = np.zeros((1, 0, m, 6))
    cases = {"free_road": dict(base, agents=none)}
    # (b) a box across the road from x = 12 to 14: the front small circles reach x = 3.5 + 0.25 + sqrt(0.5) ahead of the station
    cases["parked_box"] = dict(base, agents=agent_rows(m, 13.0, 0.0, 1.0, 3.0)[None, None])
    # (c) a pedestrian disc of 0.5 m that stands at x = 9.25 (the footprints of stations 10 .. 21 reach it) during layers 2 and 3 only
    walk = absent(m)
    walk[2:4] = [9.25, 0.0, 0.0, 0.0, 0.0, 0.5]
    cases["crossing_wait"] = dict(base, agents=walk[None, None], prm=params(stations=48, w_accel=1.0))
    later = absent(m)
    later[5:7] = [9.25, 0.0, 0.0, 0.0, 0.0, 0.5]
    cases["crossing_pass"] = dict(rolling, agents=later[None, None])
    # (d) the same disc during layers 1 and 2, when the rolling car would step into its stations
    early = absent(m)
    early[1:3] = [9.25, 0.0, 0.0, 0.0, 0.0, 0.5]
    cases["jump"] = dict(rolling, agents=early[None, None])
    # (e) a box that drives along the road into the car standing at station 0 (v_end = 0 at waypoint 0: c = 1)
    come = np.stack([[20.0 - 3.0 * k, 0.0, 0.0, 2.0, 1.0, 0.0] for k in range(m)])
    cases["driven_into"] = dict(base, agents=come[None, None], n_of=np.array([1], np.int32), profile=profile_of(road, 0.0, n_of=1)[None])
    cases["start_blocked"] = dict(base, agents=agent_rows(m, 2.0, 0.0, 2.0, 1.0)[None, None])
    # (f)
    cases["empty"] = dict(base, agents=none, n_of=np.array([0], np.int32))
    cases["one_waypoint"] = dict(base, agents=none, n_of=np.array([1], np.int32), profile=profile_of(road, 0.0, n_of=1)[None])
    cases["one_layer"] = dict(base, agents=np.zeros((1, 0, 1, 6)), m=1)
    cases["a_of_zero"] = dict(base, agents=agent_rows(m, 2.0, 0.0, 2.0, 1.0)[None, None], a_of=np.array([0], np.int32))
    gone = agent_rows(m, 2.0, 0.0, 2.0, 1.0)
    gone[:, 4] = -1.0
    cases["absent_row"] = dict(base, agents=gone[None, None])
    bad = absent(m)
    bad[2] = [500.0, 0.0, math.inf, 1.0, 1.0, 0.0]
    cases["bad_row"] = dict(base, agents=bad[None, None])
    cases["grid_short"] = dict(base, agents=none, prm=params(stations=24))
    return cases


# ---- the seeded cases of tests/test_gpu_speed_search.py ---------------------------------------------------------------------------------
CLEAR_MARGIN, COST_MARGIN = 1e-6, 1e-9                      # test_gpu_agents_check.py's and dp_cases.py's
FAST = dict(v_max=40.0, a_max=20.0, d_max=20.0, a_lat_max=math.inf)     # a speed profile under which steps of 63 cells are inside the envelope


def synth_paths(B, n, first=0):
    """[B][n][7]: the curved reference lines of path_optimizer_2_amd.synth (varied spacing 0.15 .. 0.3 m) as plain paths, solved nowhere,
    each somewhere else on the plane"""
    from path_optimizer_2_amd.synth import make_batch
    ref = make_batch(B, n, "varied", first_qp=first)["ref"]             # s, k, heading, x, y
    p = np.zeros((B, n, 7))
    b = np.arange(B)[:, None]
    p[:, :, 0], p[:, :, 1] = ref[:, :, 3] + 37.0 * b - 50.0, ref[:, :, 4] - 23.0 * b + 11.0
    p[:, :, 2], p[:, :, 5] = T.constrain_angle(ref[:, :, 2]), ref[:, :, 1]
    return p


def _profiles(paths, v_start, n_of=None, stop_before=None, prm=None):
    pick = lambda a, b: None if a is None else int(a[b])
    return np.stack([profile_of(paths[b], float(v_start[b]), n_of=pick(n_of, b), stop_before=pick(stop_before, b), prm=prm) for b in range(len(paths))])


def _at_station(case, b, j, layers, shape, side=0.0, ahead=0.0):
    """agent rows [m][6]: absent but at `layers`, where it stands at station j of path b, `ahead` m along its heading and `side` m beside"""
    m = case["m"]
    c = T.driven(case["paths"].shape[1], None if case.get("n_of") is None else case["n_of"][b],
                 None if case.get("stop_before") is None else case["stop_before"][b])
    pose = stations(case["paths"][b], case["profile"][b], c, case["prm"])[2]
    x, y, h = pose[min(j, len(pose) - 1), :3]
    rows = absent(m)
    rows[list(layers)] = [x + ahead * math.cos(h) - side * math.sin(h), y + ahead * math.sin(h) + side * math.cos(h), h + 0.3, *shape]
    return rows


def seeded(name):
    """dict(paths, profile, v_start, agents, a_of, scene_of, n_of, stop_before, prm, m) of one case of the GPU test.  The weights are
    dyadic, so every cost is exact and a gap between two candidates is a multiple of 2^-4 or a tie.  Every plan of these three gets
    through; family() below has the cases whose plans die, with more layers, other steps and weights, and q_max = 0"""
    if name == "tiles":                                      # a second station tile; words 0 / 1 / 2 with runs across 31 / 32 and 63 / 64
        B, n, m = 5, 160, 6
        prm = params(stations=70, q_max=5, q_up=2, q_down=3, w_accel=0.25, margin=0.25)
        c = dict(paths=synth_paths(B, n), v_start=np.array([0.0, 1.0, 2.5, 0.5, 2.0]), prm=prm, m=m, n_of=None, stop_before=None)
        c["profile"] = _profiles(c["paths"], c["v_start"])
        c["scene_of"], c["a_of"] = np.array([0, 1, 0, 1, 0], np.int32), np.array([3, 1], np.int32)
        agents = np.stack([np.stack([absent(m)] * 3)] * 2)
        agents[0, 0] = _at_station(c, 0, 31, (1, 2, 3), (0.0, 0.0, 0.4), side=0.3)
        agents[0, 1] = _at_station(c, 2, 64, (0, 4, 5), (1.5, 0.7, 0.1), side=-0.8)
        agents[0, 2] = _at_station(c, 4, 6, (2, 3), (0.0, 0.0, 0.5), ahead=3.0, side=0.2)
        agents[1, 0] = _at_station(c, 1, 33, (0, 1, 2, 3, 4, 5), (2.0, 1.0, 0.0), side=2.6)
        agents[1, 1] = _at_station(c, 3, 2, (0, 1, 2), (2.0, 1.0, 0.0))            # beyond a_of: not there
        c["agents"] = agents
        return c
    if name == "cap":                                        # the widest step and window at 4096 states exactly
        B, n, m = 2, 160, 3
        prm = params(stations=64, q_max=63, q_up=63, q_down=63, w_accel=2.0 ** -4)
        c = dict(paths=synth_paths(B, n, first=7), v_start=np.array([20.0, 4.0]), prm=prm, m=m, n_of=None, stop_before=None)
        c["profile"] = _profiles(c["paths"], c["v_start"], prm=FAST)
        c["scene_of"], c["a_of"] = np.array([0, 0], np.int32), None
        c["agents"] = np.stack([_at_station(c, 0, 30, (1,), (0.0, 0.0, 0.3), side=0.4), _at_station(c, 1, 20, (2,), (1.0, 0.5, 0.2), side=-0.5)])[None]
        return c
    if name == "long":                                       # states beyond the workgroup's threads, several waypoint tiles, m beyond 8
        B, n, m = 4, 300, 12
        prm = params(stations=200, q_max=19, q_up=3, q_down=6, w_accel=0.5)
        n_of, stop = np.array([300, 257, 300, 129], np.int32), np.array([300, 300, 190, 64], np.int32)
        c = dict(paths=synth_paths(B, n, first=3), v_start=np.array([0.0, 3.0, 6.0, 1.0]), prm=prm, m=m, n_of=n_of, stop_before=stop)
        c["profile"] = _profiles(c["paths"], c["v_start"], n_of, stop)
        c["scene_of"], c["a_of"] = np.array([0, 1, 1, 0], np.int32), np.array([2, 3], np.int32)
        agents = np.stack([np.stack([absent(m)] * 3)] * 2)
        agents[0, 0] = _at_station(c, 0, 30, (2, 3, 4, 5), (0.0, 0.0, 0.45), side=0.1)
        agents[0, 1] = _at_station(c, 3, 12, (6, 7, 8, 9, 10, 11), (2.2, 0.9, 0.1), side=0.5)
        agents[1, 0] = _at_station(c, 1, 66, (3, 4, 5, 6), (0.0, 0.0, 0.5), side=-0.2)
        agents[1, 1] = _at_station(c, 2, 97, (7, 8), (1.0, 1.0, 0.3), side=0.9)
        agents[1, 2] = _at_station(c, 2, 40, (0, 1, 2), (0.0, 0.0, 0.4), side=2.9)
        c["agents"] = agents
        return c
    raise KeyError(name)


SEEDED = ("tiles", "cap", "long")


# ---- the families of tests/test_gpu_speed_search_table.py -------------------------------------------------------------------------------
SLOW = dict(v_max=2.0, a_max=0.5, d_max=1.0)                 # a speed profile whose envelope stays below five cells of 0.5 m a second


def _bad_row(m, layer, heading):
    """agent rows [m][6]: absent but at `layer`, where its heading is no number - which blocks every station of that layer"""
    rows = absent(m)
    rows[layer] = [500.0, 0.0, heading, 1.0, 1.0, 0.0]
    return rows


def _scenes(m, rows):
    """agents [n_scenes][a_max][m][6] and a_of from a list, per scene, of agent rows; absent agents fill up to a_max"""
    a_max = max(len(r) for r in rows)
    agents = np.stack([np.stack(list(r) + [absent(m)] * (a_max - len(r))) if a_max else np.zeros((0, m, 6)) for r in rows])
    return agents, np.array([len(r) for r in rows], np.int32)


def family(name):
    """one batch, as seeded() gives one, of a family of cases that the three seeded shapes leave out.  tests/test_speed_search.py asserts
    on the restatement what each is there for (who dies where, which wavefronts hold living states, which flags occur) and the margins.
      "dead"        S = 200, Q = 19, m = 12, n = 300: plans that die late, at full-table size.  Path 0: an agent row with heading = inf at
                    layer 8 (from rest); 1: heading = nan at layer 5 (from 3 m/s); 2: a wall of discs across every station in reach at
                    layer 5; 3: a start far above a slow envelope (q0 clamped to Q, q_down = 6: layer 1 is empty); 4: gets through
      "ties"        the same batch with w_slow = w_accel = 0: every cost is 0, the terminal rule and the parent rule decide everything
      "horizon70",  S = 24, Q = 3, m = 70 and 260: few states and many layers, an agent that stands on the path for most of them, and an
      "horizon260"  empty and a non-finite path between the ordinary ones.  Path 0 ends on the grid (ARRIVED), 2 and 4 run past it
                    (GRID_SHORT)
      "steps"       dt = 0.8, ds = 0.3, w_slow = 0.75, w_accel = 0.5, q_up = 5 > q_down = 2, margin = 0.1, S = 150, Q = 12, m = 10, paths of
                    stride 9 whose columns 7 and 8 hold 1e9; path 2 starts above the grid's fastest step
      "standing"    q_max = 0, S = 130 (three station tiles, five words): a car that can only stand; one is driven into, one starts blocked
      "wide"        q_max = 0, S = 4096, ds = 0.02, m = 3: 64 station tiles, 128 words a layer; path 1 has n_of = 150, so its stations end
                    inside a tile and whole tiles behind hold nothing; agents beyond tile 15 and beyond tile 31
      "thin"        S = 1365, Q = 2 (4095 states), ds = 0.05, m = 40: many station tiles under a plan that moves for 39 layers; path 0 waits
                    and gets through, 1 and 2 die at layers 10 and 20"""
    if name in ("dead", "ties"):
        B, n, m = 5, 300, 12
        prm = params(stations=200, q_max=19, q_up=3, q_down=6, w_accel=0.5)
        if name == "ties":
            prm = dict(prm, w_slow=0.0, w_accel=0.0)
        c = dict(paths=synth_paths(B, n, first=11), v_start=np.array([0.0, 3.0, 0.0, 30.0, 1.0]), prm=prm, m=m, n_of=None, stop_before=None)
        c["profile"] = _profiles(c["paths"], c["v_start"])
        c["profile"][3] = profile_of(c["paths"][3], 1.0, prm=SLOW)                  # the profile of a slower car than the one that starts at 30 m/s
        c["scene_of"] = np.arange(B, dtype=np.int32)
        wall = [_at_station(c, 2, j, (5,), (0.0, 0.0, 0.5)) for j in range(0, 80, 8)]
        c["agents"], c["a_of"] = _scenes(m, [[_bad_row(m, 8, math.inf)], [_bad_row(m, 5, math.nan)], wall, [],
                                             [_at_station(c, 4, 14, (1, 2, 3, 4), (0.0, 0.0, 0.45), side=0.2)]])
        return c
    if name in ("horizon70", "horizon260"):
        B, n, m = 5, 80, 70 if name == "horizon70" else 260
        prm = params(stations=24, q_max=3, q_up=1, q_down=2, w_accel=0.25)
        paths = synth_paths(B, n, first=5)
        paths[3, 17, 1] = math.nan                           # path 3 is not finite, path 1 is empty
        n_of = np.array([30, 0, n, n, n], np.int32)
        c = dict(paths=paths, v_start=np.array([0.0, 0.0, 0.5, 0.0, 1.5]), prm=prm, m=m, n_of=n_of, stop_before=None)
        fin = paths.copy()
        fin[3, 17, 1] = 0.0
        c["profile"] = _profiles(fin, c["v_start"], n_of)
        c["scene_of"] = np.array([0, 0, 1, 1, 2], np.int32)
        wait = range(0, m - 20)
        c["agents"], c["a_of"] = _scenes(m, [[_at_station(c, 0, 12, wait, (0.0, 0.0, 0.3), ahead=3.5)],
                                             [_at_station(c, 2, 14, wait, (1.0, 0.5, 0.1), ahead=3.5, side=0.3)],
                                             [_at_station(c, 4, 9, range(3, m - 30), (0.0, 0.0, 0.4), ahead=3.5, side=-0.2)]])
        return c
    if name == "steps":
        B, n, m = 3, 220, 10
        prm = params(dt=0.8, ds=0.3, w_slow=0.75, w_accel=0.5, margin=0.1, stations=150, q_max=12, q_up=5, q_down=2)
        paths = np.full((B, n, 9), 1e9)
        paths[:, :, :7] = synth_paths(B, n, first=13)
        c = dict(paths=paths, v_start=np.array([0.0, 2.0, 6.0]), prm=prm, m=m, n_of=np.array([n, 171, n], np.int32), stop_before=None)
        c["profile"] = _profiles(paths, c["v_start"], c["n_of"])
        c["scene_of"], c["a_of"] = np.array([0, 1, 1], np.int32), np.array([1, 2], np.int32)
        c["agents"] = _scenes(m, [[_at_station(c, 0, 20, (3, 4, 5), (0.0, 0.0, 0.4), side=0.3)],
                                  [_at_station(c, 1, 45, (4, 5, 6), (1.5, 0.7, 0.1), side=-0.6), _at_station(c, 2, 70, (5, 6), (0.0, 0.0, 0.5), side=0.1)]])[0]
        return c
    if name == "standing":
        B, n, m = 3, 300, 6
        prm = params(stations=130, q_max=0, margin=0.25)
        c = dict(paths=synth_paths(B, n, first=17), v_start=np.array([0.0, 2.0, 0.0]), prm=prm, m=m, n_of=None, stop_before=None)
        c["profile"] = _profiles(c["paths"], c["v_start"])
        c["scene_of"] = np.arange(B, dtype=np.int32)
        c["agents"], c["a_of"] = _scenes(m, [[_at_station(c, 0, 31, (1, 2, 3), (0.0, 0.0, 0.4), side=0.3), _at_station(c, 0, 100, (0, 4, 5), (2.0, 1.0, 0.0), side=1.0)],
                                             [_at_station(c, 1, 2, (3, 4, 5), (0.0, 0.0, 0.5)), _at_station(c, 1, 64, (0, 1, 2), (1.5, 0.7, 0.1), side=-0.8)],
                                             [_at_station(c, 2, 0, (0, 1), (0.0, 0.0, 0.3), ahead=1.0), _at_station(c, 2, 127, (2,), (0.0, 0.0, 0.5))]])
        return c
    if name == "wide":
        B, n, m = 2, 400, 3
        prm = params(ds=0.02, stations=4096, q_max=0, margin=0.2)
        c = dict(paths=synth_paths(B, n, first=19), v_start=np.array([1.0, 0.0]), prm=prm, m=m, n_of=np.array([n, 150], np.int32), stop_before=None)
        c["profile"] = _profiles(c["paths"], c["v_start"], c["n_of"])
        c["scene_of"], c["a_of"] = np.array([0, 1], np.int32), None
        c["agents"], _ = _scenes(m, [[_at_station(c, 0, 1100, (0, 2), (0.0, 0.0, 0.4), side=0.3), _at_station(c, 0, 2500, (1,), (1.5, 0.7, 0.1), side=-0.6)],
                                     [_at_station(c, 1, 1300, (1, 2), (0.0, 0.0, 0.5), side=0.2), _at_station(c, 1, 2100, (0,), (2.0, 1.0, 0.0), side=0.9)]])
        return c
    if name == "thin":
        B, n, m = 3, 300, 40
        prm = params(ds=0.05, stations=1365, q_max=2, q_up=1, q_down=1, w_accel=0.25, margin=0.1)
        c = dict(paths=synth_paths(B, n, first=23), v_start=np.array([0.0, 0.05, 0.1]), prm=prm, m=m, n_of=None, stop_before=None)
        c["profile"] = _profiles(c["paths"], np.array([0.5, 0.5, 0.5]))
        c["scene_of"], c["a_of"] = np.arange(B, dtype=np.int32), None
        c["agents"], _ = _scenes(m, [[_at_station(c, 0, 20, range(4, 16), (0.0, 0.0, 0.3), ahead=4.5)],
                                     [_at_station(c, 1, 10, range(10, m), (0.0, 0.0, 0.5), ahead=1.5)],
                                     [_at_station(c, 2, 20, range(20, m), (0.0, 0.0, 0.5), ahead=1.5)]])
        return c
    raise KeyError(name)


DEAD_ENDS = ("dead", "ties")
HORIZONS = ("horizon70", "horizon260")
FAMILIES = DEAD_ENDS + HORIZONS + ("steps", "standing", "wide", "thin")


def last_lanes(one, prm):
    """of one path's result: (the lanes e mod 256 of the states that live in its last living layer, e = j (Q + 1) + q; the winner's lane)"""
    if one["reached"] == 0:
        return [], None
    Q1 = prm["q_max"] + 1
    last = list(one["parents"][one["reached"] - 1]) if one["reached"] > 1 else [(0, one["q0"])]
    j, q = (int(v) for v in one["steps"][one["reached"] - 1])
    return [(j_ * Q1 + q_) % 256 for j_, q_ in last], (j * Q1 + q) % 256


def run_case(c, circles, **kw):
    return search_batch(c["paths"], c["profile"], c["v_start"], c["agents"], circles, m=c.get("m"), n_of=c.get("n_of"), stop_before=c.get("stop_before"),
                        a_of=c.get("a_of"), scene_of=c.get("scene_of"), prm=c["prm"], **kw)


def write_case(path, c):
    """the file tests/cpp/search_demo.cpp reads: int32 B, n, m, n_scenes, a_max, stations, q_max, q_up, q_down; double dt, ds, w_slow, w_accel,
    margin; int32 n_of [B], stop_before [B], a_of [n_scenes], scene_of [B]; double v_start [B]; double rows [B][n][8] = x, y, heading, k, s, v, a, t;
    double agents [n_scenes][a_max][m][6]"""
    paths, profile, agents = (np.asarray(c[k], dtype=np.float64) for k in ("paths", "profile", "agents"))
    B, n = paths.shape[:2]
    n_scenes, a_max, m = agents.shape[:3]
    p = c["prm"]
    i32 = lambda a, size, fill: np.full(size, fill, np.int32) if a is None else np.asarray(a, np.int32)
    with open(path, "wb") as f:
        f.write(np.array([B, n, m, n_scenes, a_max, p["stations"], p["q_max"], p["q_up"], p["q_down"]], np.int32).tobytes())
        f.write(np.array([p["dt"], p["ds"], p["w_slow"], p["w_accel"], p["margin"]], np.float64).tobytes())
        f.write(i32(c.get("n_of"), B, n).tobytes())
        f.write(i32(c.get("stop_before"), B, n).tobytes())
        f.write(i32(c.get("a_of"), n_scenes, a_max).tobytes())
        f.write(i32(c.get("scene_of"), B, 0).tobytes())
        f.write(np.asarray(c["v_start"], np.float64).tobytes())
        f.write(np.ascontiguousarray(np.concatenate([paths[:, :, [0, 1, 2, 5]], profile], axis=2)).tobytes())
        f.write(np.ascontiguousarray(agents).tobytes())
