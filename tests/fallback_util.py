"""Test helper: pqp_fallback_rows and pqp_fallback_pick restated in numpy float64 (one rounding per operation) from include/pqp.h,
operation by operation, with predict_util's free-model functions on the arc; the margin of every comparison a flag or a segment hangs on
and that is not a comparison of identical bits; a plain per-sample Python loop of the same definitions that shares no array expression
with the restatement; a numerical integration of the braking law; and the plans, states and cases that tests/test_fallback.py and
tests/test_gpu_fallback.py share."""
import itertools
import math

import numpy as np

import corridor_oracle as K
import predict_util as PR
import sample_util as SU
import stitch_util as ST

BAD, ARC, BAD_PLAN, PATH_SHORT, HORIZON, TAKEN, NOT_CLEAR = (1 << k for k in range(7))
LEVELS = ((1.5, 2.5), (3.0, 5.0), (6.0, 15.0))             # pqp_fallback_default_params
A_CAP = 1.5
# the columns of `margins`: how far each comparison was from going the other way, +inf where it was not made or was one of equal bits
M_T1, M_T, M_TS, M_SIGMA = range(4)
MARGIN_NAMES = ("t against t1", "t against T", "ts against t1", "sigma against a row's s")


def times(dt, r, m):
    """the instants of the M = (m - 1) r + 1 rows: pqp_sample_plan's expression"""
    f = np.arange((m - 1) * r + 1)
    return (f // r).astype(np.float64) * np.float64(dt) + ((f % r).astype(np.float64) * np.float64(dt)) / np.float64(r)


def _gap(a, b):
    """the least |a - b| over the entries that are not equal (equal bits compare equal on any machine), +inf when there is none"""
    g = np.abs(np.asarray(a, dtype=np.float64) - b)
    g = g[np.isfinite(g) & (g > 0.0)]
    return float(g.min()) if g.size else math.inf


def law_constants(v0, a_in, d, j, a_cap):
    """a0, t1, ts, in_ramp, v1, s1, T, eT of include/pqp.h, in its operation order"""
    v0, a_in, d, j, a_cap = (np.float64(q) for q in (v0, a_in, d, j, a_cap))
    a0 = min(max(a_in, -d), a_cap)
    t1 = (a0 + d) / j
    ts = (a0 + np.sqrt(a0 * a0 + (2.0 * j) * v0)) / j
    in_ramp = bool(ts <= t1)
    v1 = max(v0 + (a0 - (0.5 * j) * t1) * t1, np.float64(0.0))
    s1 = (v0 + (0.5 * a0 - (j * t1) / 6.0) * t1) * t1
    u1 = v1 / d
    T = ts if in_ramp else t1 + u1
    eT = max((v0 + (0.5 * a0 - (j * ts) / 6.0) * ts) * ts if in_ramp else s1 + (v1 - (0.5 * d) * u1) * u1, np.float64(0.0))
    return a0, t1, ts, in_ramp, v1, s1, T, eT


def plan_rows(state, level, a_cap, dt, r, m, prev=None, stitch_flags=None):
    """one group and one level: state [8], level (d, j), prev [Mp][>= 5] (the plan's own rows, already cut to its count) or None ->
    dict(rows [M][8], stop [2], stop_row, flags, margins [4])"""
    state = np.asarray(state, dtype=np.float64)
    t = times(dt, r, m)
    M = t.size
    margins = np.full(4, math.inf)
    out = dict(rows=np.zeros((M, 8)), stop=np.zeros(2), stop_row=0, flags=BAD, margins=margins)
    sf = ST.STITCHED if stitch_flags is None else int(stitch_flags)
    if not np.isfinite(state[:7]).all() or state[5] < 0.0 or sf & ST.BAD:
        return out
    x0, y0, h0, k0, s_st, v0, a_in = state[:7]
    d, j = np.float64(level[0]), np.float64(level[1])
    a0, t1, ts, in_ramp, v1, s1, T, eT = law_constants(v0, a_in, d, j, a_cap)
    margins[M_TS] = _gap(ts, t1)
    margins[M_T] = _gap(t, T)
    with np.errstate(invalid="ignore", over="ignore"):
        rest, ramp = t >= T, t < t1
        margins[M_T1] = _gap(t[~rest], t1)
        u = t - t1
        e = np.where(rest, eT, np.where(ramp, (v0 + (0.5 * a0 - (j * t) / 6.0) * t) * t, s1 + (v1 - (0.5 * d) * u) * u))
        v = np.where(rest, 0.0, np.where(ramp, v0 + (a0 - (0.5 * j) * t) * t, v1 - d * u))
        acc = np.where(rest, 0.0, np.where(ramp, a0 - j * t, -d))
    e = np.minimum(np.maximum(e, 0.0), eT)
    v = np.maximum(v, 0.0)
    rows = out["rows"]
    rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = e, v, acc, t
    flags = 0
    Mp = 0 if prev is None else len(prev)
    arc = not (sf & ST.STITCHED) or Mp < 2
    if not arc:
        prev = np.asarray(prev, dtype=np.float64)
        if not np.isfinite(prev[:, :5]).all():
            arc, flags = True, flags | BAD_PLAN
    if arc:
        flags |= ARC
        sh0, ch0 = math.sin(h0), math.cos(h0)
        for f in range(M):
            th = k0 * e[f]
            sinc, cosc, _, _ = PR.ctra_functions(float(th))
            p, q = e[f] * sinc, e[f] * cosc
            rows[f, 0] = x0 + (p * ch0 - q * sh0)
            rows[f, 1] = y0 + (p * sh0 + q * ch0)
            rows[f, 2] = K.constrain_angle(float(h0 + th))
            rows[f, 3] = k0
    else:
        s = prev[:, 4]
        S = np.maximum.accumulate(s)
        sigma = s_st + e
        cnt = (S[None, :] <= sigma[:, None]).sum(axis=1)
        margins[M_SIGMA] = _gap((S[None, :] - sigma[:, None]).ravel(), 0.0)
        i = np.maximum(cnt - 1, 0)
        on = i < Mp - 1
        i0 = np.minimum(i, Mp - 2)
        r0, r1 = prev[i0], prev[i0 + 1]
        ds = r1[:, 4] - r0[:, 4]
        with np.errstate(invalid="ignore", divide="ignore"):
            lam = np.where(ds > 0.0, np.minimum(np.maximum((sigma - r0[:, 4]) / ds, 0.0), 1.0), 0.0)
        x = r0[:, 0] + lam * (r1[:, 0] - r0[:, 0])
        y = r0[:, 1] + lam * (r1[:, 1] - r0[:, 1])
        hd = SU.constrain_angle(r0[:, 2] + lam * SU.constrain_angle(r1[:, 2] - r0[:, 2]))
        kk = r0[:, 3] + lam * (r1[:, 3] - r0[:, 3])
        last = prev[Mp - 1]
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = (np.where(on, x, last[0]), np.where(on, y, last[1]), np.where(on, hd, last[2]),
                                                          np.where(on, kk, last[3]))
        if (~on & (sigma > S[-1])).any():
            flags |= PATH_SHORT
    stop_row = int((t < T).sum())
    if stop_row == M:
        flags |= HORIZON
    out.update(stop=np.array([T, eT]), stop_row=stop_row, flags=flags)
    return out


def fallback_rows(state, levels, a_cap, dt, r, m, prev=None, prev_m=None, stitch_flags=None):
    """pqp_fallback_rows: state [G][8], levels [L][2], prev [G][mp][stride >= 8] or None -> dict(rows [G][L][M][8], stop [G][L][2],
    stop_row [G][L], flags [G][L], margins [G][L][4])"""
    state = np.asarray(state, dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64).reshape(-1, 2)
    G, L, M = state.shape[0], levels.shape[0], (m - 1) * r + 1
    res = dict(rows=np.zeros((G, L, M, 8)), stop=np.zeros((G, L, 2)), stop_row=np.zeros((G, L), np.int32), flags=np.zeros((G, L), np.int32),
               margins=np.full((G, L, 4), math.inf))
    for g in range(G):
        rows = None
        if prev is not None:
            mp = prev.shape[1]
            Mp = mp if prev_m is None else min(max(int(prev_m[g]), 0), mp)
            rows = prev[g, :Mp]
        for l in range(L):
            one = plan_rows(state[g], levels[l], a_cap, dt, r, m, rows, None if stitch_flags is None else stitch_flags[g])
            for k in res:
                res[k][g, l] = one[k]
    return res


def fallback_pick(rows, row_flags, best=None, best_traj=None, best_m=None, first_hit=None, first_collision=None):
    """pqp_fallback_pick -> dict(final_traj [G][M][8], final_m [G], level [G], flags [G])"""
    rows = np.asarray(rows, dtype=np.float64)
    G, L, M = rows.shape[:3]
    rf = np.asarray(row_flags).reshape(G, L)
    hit = np.full((G, L), M) if first_hit is None else np.asarray(first_hit).reshape(G, L)
    col = np.full((G, L), M) if first_collision is None else np.asarray(first_collision).reshape(G, L)
    res = dict(final_traj=np.zeros((G, M, 8)), final_m=np.zeros(G, np.int32), level=np.full(G, -1, np.int32), flags=np.zeros(G, np.int32))
    usable = ((rf & (BAD | PATH_SHORT)) == 0) & (hit == M) & (col == M)
    contact = np.minimum(hit, col)
    for g in range(G):
        if best is not None and best[g] >= 0:
            if best_traj is not None:
                res["final_traj"][g], res["final_m"][g] = best_traj[g], best_m[g]
            continue
        if (rf[g] & BAD).any():
            res["flags"][g] = BAD
            continue
        if usable[g].any():
            lv, extra = int(np.argmax(usable[g])), TAKEN
        else:
            lv, extra = L - 1 - int(np.argmax(contact[g][::-1])), TAKEN | NOT_CLEAR          # the latest contact, among equal ones the highest level
        res["final_traj"][g], res["final_m"][g], res["level"][g], res["flags"][g] = rows[g, lv], M, lv, int(rf[g, lv]) | extra
    return res


# ---- the same definitions as plain loops: Python floats, no array expression --------------------------------------------------------------------
def plan_rows_loop(state, level, a_cap, dt, r, m, prev=None, stitch_flags=None):
    """(rows, (T, eT), stop_row, flags) of one group and one level, sample by sample"""
    st = [float(q) for q in state]
    M = (m - 1) * r + 1
    sf = ST.STITCHED if stitch_flags is None else int(stitch_flags)
    if not all(math.isfinite(q) for q in st[:7]) or st[5] < 0.0 or sf & ST.BAD:
        return [[0.0] * 8 for _ in range(M)], (0.0, 0.0), 0, BAD
    x0, y0, h0, k0, s_st, v0, a_in = st[:7]
    d, j, a_cap = float(level[0]), float(level[1]), float(a_cap)
    a0 = min(max(a_in, -d), a_cap)
    t1 = (a0 + d) / j
    ts = (a0 + math.sqrt(a0 * a0 + (2.0 * j) * v0)) / j
    E = lambda t: (v0 + (0.5 * a0 - (j * t) / 6.0) * t) * t
    v1 = max(v0 + (a0 - (0.5 * j) * t1) * t1, 0.0)
    s1 = E(t1)
    u1 = v1 / d
    if ts <= t1:
        T, eT = ts, max(E(ts), 0.0)
    else:
        T, eT = t1 + u1, max(s1 + (v1 - (0.5 * d) * u1) * u1, 0.0)
    P = [] if prev is None else [[float(q) for q in row[:5]] for row in prev]
    flags = 0
    arc = not (sf & ST.STITCHED) or len(P) < 2
    if not arc and not all(math.isfinite(q) for row in P for q in row):
        arc, flags = True, BAD_PLAN
    if arc:
        flags |= ARC
    rows, stop_row = [], 0
    for f in range(M):
        t = float(f // r) * dt + (float(f % r) * dt) / float(r)
        if t >= T:
            e, v, acc = eT, 0.0, 0.0
        elif t < t1:
            e, v, acc = E(t), v0 + (a0 - (0.5 * j) * t) * t, a0 - j * t
        else:
            u = t - t1
            e, v, acc = s1 + (v1 - (0.5 * d) * u) * u, v1 - d * u, -d
        e, v = min(max(e, 0.0), eT), max(v, 0.0)
        if t < T:
            stop_row += 1
        if arc:
            th = k0 * e
            sinc, cosc, _, _ = PR.ctra_functions(th)
            p, q = e * sinc, e * cosc
            pose = [x0 + (p * math.cos(h0) - q * math.sin(h0)), y0 + (p * math.sin(h0) + q * math.cos(h0)), K.constrain_angle(h0 + th), k0]
        else:
            sigma = s_st + e
            top, cnt = -math.inf, 0
            for row in P:
                top = max(top, row[4])
                if top <= sigma:
                    cnt += 1
            i = max(cnt - 1, 0)
            if i < len(P) - 1:
                a, b = P[i], P[i + 1]
                ds = b[4] - a[4]
                lam = min(max((sigma - a[4]) / ds, 0.0), 1.0) if ds > 0.0 else 0.0
                pose = [a[0] + lam * (b[0] - a[0]), a[1] + lam * (b[1] - a[1]), K.constrain_angle(a[2] + lam * K.constrain_angle(b[2] - a[2])),
                        a[3] + lam * (b[3] - a[3])]
            else:
                pose = P[-1][:4]
                if sigma > top:
                    flags |= PATH_SHORT
        rows.append(pose + [e, v, acc, t])
    if stop_row == M:
        flags |= HORIZON
    return rows, (T, eT), stop_row, flags


def pick_loop(L, M, rf, hit, col):
    """(level, flags) of one group that falls back: rf, hit, col are the levels' flags, first hits and first collisions"""
    if any(f & BAD for f in rf):
        return -1, BAD
    for l in range(L):
        if not rf[l] & (BAD | PATH_SHORT) and hit[l] == M and col[l] == M:
            return l, rf[l] | TAKEN
    lv, latest = -1, -math.inf
    for l in range(L):
        c = min(hit[l], col[l])
        if c >= latest:
            lv, latest = l, c
    return lv, rf[lv] | TAKEN | NOT_CLEAR


# ---- the law by numerical integration -------------------------------------------------------------------------------------------------------------
def integrate(v0, a0, d, j, at, h):
    """(e, v, a) at the ascending instants `at` of a' = -j clamped at -d, v' = a, e' = v, stopped for good at v = 0, by Heun's rule
    (explicit trapezoid, second order) on steps of h from t = 0 - a last shorter step lands on each instant.  Nothing of the closed form
    enters: the end of the ramp and the stop are found by the steps themselves, each to one step's accuracy"""
    out = []
    t, e, v, a = 0.0, 0.0, float(v0), float(a0)
    standing = v == 0.0 and a <= 0.0
    if standing:
        a = 0.0
    for target in at:
        while t < target and not standing:
            step = min(h, target - t)
            a_next = max(a - j * step, -d)
            v_next = v + 0.5 * (a + a_next) * step
            if v_next <= 0.0 and v_next < v:
                part = v / (v - v_next)                            # where the speed's chord crosses 0 inside the step
                e += 0.5 * v * (part * step)
                v, a, standing = 0.0, 0.0, True
                break
            e += 0.5 * (v + v_next) * step
            v, a, t = v_next, a_next, t + step
        out.append((e, v, a))
    return np.array(out)


# ---- plans, states and the cases the device is held to ---------------------------------------------------------------------------------------------
def state_on(plan, row, v=None, a=0.0, lam=0.0):
    """a stitch state row on `plan`: row `row` (lam = 0: its own bits), or the point lam of the way to the next row"""
    st = plan[row, :8].copy() if lam == 0.0 else plan[row, :8] + lam * (plan[row + 1, :8] - plan[row, :8])
    if v is not None:
        st[5] = v
    st[6] = a
    return st


def seeded_case(G, mp, m, r, seed, L=3, stride=8, dt=0.1, ragged=True, flags=None):
    """G plans of up to mp rows (stitch_util's arcs, |x|, |y| well inside 1000 m) and a state on each, between two of its rows, at a speed
    that stops the car on the plan, beyond it or beyond the horizon; L levels ascending from the default ones.
    dict(name, prev, prev_m, state, stitch_flags, levels, a_cap, dt, r, m)"""
    rng = np.random.default_rng(seed)
    prev = np.zeros((G, mp, stride))
    prev_m = np.full(G, mp, np.int32)
    state = np.zeros((G, 8))
    for g in range(G):
        v = rng.uniform(3.0, 14.0)
        prev[g] = ST.arc_plan(mp, 0.1, v=v, a=rng.choice([-0.5, 0.0, 0.75]), curvature=rng.choice([-0.03, 0.0, 0.0004, 0.01, 0.05]),
                              x0=rng.uniform(-400.0, 400.0), y0=rng.uniform(-400.0, 400.0), h0=rng.uniform(-math.pi, math.pi), t0=rng.uniform(0.0, 5.0),
                              s0=rng.uniform(0.0, 50.0), stride=stride)
        if ragged and mp > 2 and rng.random() < 0.3:
            prev_m[g] = rng.integers(2, mp + 1)
        Mp = int(prev_m[g])
        at = int(rng.integers(0, max(Mp - 2, 1)))
        # (speeds and accelerations off the round values: a stop time that falls on a sample's instant to the last bit has no margin)
        state[g] = state_on(prev[g], at, v=0.0 if rng.random() < 0.15 else rng.uniform(0.2, 13.0), a=-3.0 if rng.random() < 0.1 else rng.uniform(-7.0, 2.5),
                            lam=0.0 if Mp < 2 or rng.random() < 0.3 else rng.uniform(0.2, 0.8))
    base = np.array(LEVELS + ((6.5, 15.0), (7.0, 20.0), (7.5, 20.0), (8.0, 25.0), (9.0, 30.0)))
    levels = base[:1] if L == 1 else base[:L]
    return dict(name=f"G{G}_mp{mp}_m{m}_r{r}_L{L}_s{stride}", prev=prev, prev_m=prev_m, state=state, stitch_flags=flags, levels=levels,
                a_cap=1.37, dt=dt, r=r, m=m)          # (a cap off the default 1.5, which puts t1 = 3 / 2.5 on a sample's instant)


def device_cases():
    """every case of the GPU test, by name: M in {1, 2, 63, 64, 65, 130} through (m, r) pairs with r = 1 and r = 10, mp in {2, 63, 64, 65,
    130}, L in {1, 3, 8}, groups in {1, 5, 67}, stride 8 and 11, ragged prev_m with 0, 1 and 2, NaN rows at and away from the used
    segment, stitch_flags absent, stitched, replanned and bad"""
    cases = []
    # (m, r) -> M: (1, 10) 1, (2, 1) 2, (63, 1) 63, (8, 9) 64, (65, 1) 65, (130, 1) 130; r = 10 reaches M = 10 k + 1 alone: (7, 10) 61
    # and (14, 10) 131 beside them
    shapes = [((1, 10), 2), ((2, 1), 63), ((63, 1), 64), ((8, 9), 65), ((65, 1), 130), ((130, 1), 64), ((7, 10), 130), ((14, 10), 65)]
    for k, ((m, r), mp) in enumerate(shapes):
        G, L, stride = (1, 5, 67)[k % 3], (1, 3, 8)[(k + 1) % 3], (8, 11)[k % 2]
        cases.append(seeded_case(G, mp, m, r, seed=300 + k, L=L, stride=stride, dt=0.1 if r == 1 else 0.5))
    # ragged counts with 0, 1 and 2; stitch flags absent above, here stitched, replanned and bad
    c = seeded_case(9, 65, 8, 10, seed=41, ragged=False, dt=0.5)
    c["prev_m"] = np.array([65, 0, 1, 2, 64, 30, 1, 65, 2], np.int32)
    for g in range(9):
        c["state"][g] = state_on(c["prev"][g], 0, v=4.0 + g, a=-0.5)
    c["name"] = "ragged"
    cases.append(c)
    c = seeded_case(8, 64, 14, 10, seed=42, dt=0.5)
    c["stitch_flags"] = np.array([ST.STITCHED, ST.REPLAN | ST.LATERAL, ST.BAD, ST.STITCHED | ST.PREFIX_CUT, ST.REPLAN | ST.NO_PREVIOUS | ST.STANDING,
                                  ST.STITCHED, ST.BAD, ST.STITCHED], np.int32)
    c["state"][2] = 0.0; c["state"][6] = 0.0                      # what the stitch leaves of a bad group
    c["name"] = "stitch_flags"
    cases.append(c)
    # states that are not numbers or drive backwards, between good neighbours
    c = seeded_case(7, 40, 20, 1, seed=43)
    c["state"][1, 0] = np.nan; c["state"][3, 5] = -0.5; c["state"][5, 6] = np.inf
    c["name"] = "bad_states"
    cases.append(c)
    # rows that are not numbers: at the used segment, away from it, in a column that is not read, and behind prev_m
    c = seeded_case(6, 40, 20, 1, seed=44, ragged=False, stride=11)
    for g in range(6):
        c["state"][g] = state_on(c["prev"][g], 3, v=5.3, a=-0.2, lam=0.5)
    c["prev"][0, 3, 0] = np.nan
    c["prev"][1, 30, 4] = np.inf
    c["prev"][2, 5, 6] = np.nan                                   # column 6 is not read: the plan is used
    c["prev"][3, 35, 2] = np.nan; c["prev_m"][3] = 35             # behind the count: not read
    c["prev"][4, :, 3] = np.nan
    c["name"] = "nan_rows"
    cases.append(c)
    # the arc: k0 = 0, |k0 e| on both sides of 2^-6, a straight heading-0 car
    c = seeded_case(6, 2, 9, 10, seed=45, dt=0.5)
    c["prev"], c["prev_m"] = None, None
    c["state"] = np.array([[10.0, -20.0, 0.0, 0.0, 0.0, 9.0, 0.5, 0.0], [10.0, -20.0, 0.7, 0.0, 3.0, 9.0, -1.0, 0.0], [-300.0, 250.0, 2.5, 0.0004, 0.0, 12.0, 0.0, 0.0],
                           [-300.0, 250.0, -2.5, 0.05, 7.0, 12.0, 0.0, 0.0], [900.0, -900.0, 3.1, -0.2, 0.0, 6.0, 1.0, 0.0], [0.0, 0.0, -0.3, 0.03, 0.0, 0.0, -1.0, 0.0]])
    c["name"] = "arc"
    cases.append(c)
    return cases


def run_case(c):
    """the restatement on a case"""
    return fallback_rows(c["state"], c["levels"], c["a_cap"], c["dt"], c["r"], c["m"], c["prev"], c["prev_m"], c["stitch_flags"])


PICK_KINDS = lambda M: [(0, M, M), (HORIZON, 2, M), (ARC, 4, M), (0, M, 2), (PATH_SHORT, M, M)]          # flags, first hit, first collision


def pick_combinations(L, M):
    """(row_flags, first_hit, first_collision), each [G][L]: every level one of usable, hit at row 2, hit at row 4, collided at row 2,
    flagged short.  L <= 3: all 5^L combinations.  Above: all 3^L of the first three kinds - every pattern of usable and unusable
    levels, with the contact at either of two rows so that ties and every order of the contacts are in - and, for the other two kinds,
    all 5^3 on the first, a middle and the last level while every other level is hit at row 2, and again while every other is short"""
    kinds = PICK_KINDS(M)
    if L <= 3:
        combos = [list(co) for co in itertools.product(range(5), repeat=L)]
    else:
        combos = [list(co) for co in itertools.product(range(3), repeat=L)]
        for rest in (1, 4):
            for co in itertools.product(range(5), repeat=3):
                row = [rest] * L
                row[0], row[L // 2], row[L - 1] = co
                combos.append(row)
    pick = lambda k: np.array([[kinds[c][k] for c in co] for co in combos], np.int32)
    return pick(0), pick(1), pick(2)


def pick_case(G, L, M, seed):
    """rows, flags and verdicts for the pick: every kind of level - usable, hit, collided, both, short - ties in the first contact, groups
    with a winner, and a bad group between two good ones.  dict(rows, row_flags, best, best_traj, best_m, first_hit, first_collision)"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-5.0, 5.0, (G, L, M, 8))
    row_flags = rng.choice([0, 0, ARC, HORIZON, PATH_SHORT, ARC | BAD_PLAN], (G, L)).astype(np.int32)
    hit = np.where(rng.random((G, L)) < 0.5, M, rng.integers(0, max(M, 1), (G, L))).astype(np.int32)
    col = np.where(rng.random((G, L)) < 0.5, M, rng.integers(0, max(M, 1), (G, L))).astype(np.int32)
    if G >= 3:
        row_flags[1], rows[1] = BAD, 0.0
    if G >= 5:
        hit[3], col[3] = min(2, M - 1), M                         # a tie in the first contact over every level
        hit[4], col[4] = M, M
        row_flags[4] = PATH_SHORT                                  # no contact, no usable level
    best = np.where(rng.random(G) < 0.4, rng.integers(0, 4, G), -1).astype(np.int32)
    best[:min(G, 5)] = -1
    best_traj = rng.uniform(-5.0, 5.0, (G, M, 8))
    best_m = rng.integers(0, M + 1, G).astype(np.int32)
    return dict(rows=rows, row_flags=row_flags, best=best, best_traj=best_traj, best_m=best_m, first_hit=hit.ravel(), first_collision=col.ravel())


def write_case(path, prev, prev_m, stitch_flags, state, dt, r, m, first_hit, first_collision):
    """the file tests/cpp/fallback_demo.cpp reads: int32 G, mp, m, r; double dt; int32 prev_m [G], stitch_flags [G]; double state [G][8],
    prev [G][mp][8]; int32 first_hit [G * 3], first_collision [G * 3] (the planner's default levels)"""
    prev = np.ascontiguousarray(np.asarray(prev, dtype=np.float64)[:, :, :8])
    G, mp = prev.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([G, mp, m, r], np.int32).tobytes())
        f.write(np.array([dt], np.float64).tobytes())
        for a, dtype in ((prev_m, np.int32), (stitch_flags, np.int32), (state, np.float64), (prev, np.float64), (first_hit, np.int32),
                         (first_collision, np.int32)):
            f.write(np.ascontiguousarray(a, dtype=dtype).tobytes())
