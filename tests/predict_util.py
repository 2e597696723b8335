"""Test helper: pqp_predict_agents restated in Python floats (fp64, one rounding per operation) from include/pqp.h, operation by
operation; an RK4 integration of the motion the closed forms solve, which shares nothing with them; the lanes, tracks and the demo's
file that tests/test_predict_agents.py and tests/test_gpu_predict_agents.py share."""
import math

import numpy as np

import corridor_oracle as K
import project_util as P

ABSENT, BAD, ON_LANE, LANE_FAR, OFF_LANE, STOPS, CAPPED = 1, 2, 4, 8, 16, 32, 64
V_CAP, GROW, L_MAX = 40.0, 0.0, 3.0                 # pqp_predict_default_params
SMALL_ANGLE = 2.0 ** -6
MAX_LENGTH = 1048576.0
ABSENT_ROW = (0.0, 0.0, 0.0, -1.0, -1.0, 0.0)


def step_time(t0, dt, r, f):
    k, i = f // r, f % r
    return t0 + (float(k) * dt + (float(i) * dt) / float(r))


def taylor(th):
    """sinc, cosc, f1, f2 by their polynomials through th^5"""
    t2 = th * th
    return (1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0)), th * (0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0))),
            0.5 - t2 * (1.0 / 8.0 - t2 * (1.0 / 144.0)), th * (1.0 / 3.0 - t2 * (1.0 / 30.0 - t2 * (1.0 / 840.0))))


def closed(th):
    """sinc, cosc, f1, f2 by their closed forms"""
    t2 = th * th
    sn, cs = math.sin(th), math.cos(th)
    sh = math.sin(0.5 * th)
    hv = 2.0 * (sh * sh)
    return sn / th, hv / th, (th * sn - hv) / t2, (sn - th * cs) / t2


def ctra_functions(th):
    return taylor(th) if abs(th) < SMALL_ANGLE else closed(th)


def speed(v, a, v_cap, tau):
    """(te, ve, the stop is reached, the cap is reached) at time tau"""
    if a < 0.0:
        ts = v / (-a)
        done = tau >= ts
        te = min(tau, ts)
        return te, (0.0 if done else v + a * te), done, False
    if a > 0.0:
        if v >= v_cap:
            return 0.0, v, False, True
        tl = (v_cap - v) / a
        done = tau >= tl
        te = min(tau, tl)
        return te, (v_cap if done else v + a * te), False, done
    if v == 0.0:
        return 0.0, 0.0, True, False
    return tau, v, False, False


def free_pose(x0, y0, h0, v, a, w, te, ve, tc):
    th = w * te
    sinc, cosc, f1, f2 = ctra_functions(th)
    vt, at = v * te, a * (te * te)
    p, q = vt * sinc + at * f1, vt * cosc + at * f2
    h1 = h0 + th
    th2 = w * tc if ve > 0.0 else 0.0
    sinc2, cosc2, _, _ = ctra_functions(th2)
    vt2 = ve * tc
    p2, q2 = vt2 * sinc2, vt2 * cosc2
    s0, c0, s1, c1 = math.sin(h0), math.cos(h0), math.sin(h1), math.cos(h1)
    x = (x0 + (p * c0 - q * s0)) + (p2 * c1 - q2 * s1)
    y = (y0 + (p * s0 + q * c0)) + (p2 * s1 + q2 * c1)
    return x, y, K.constrain_angle(h1 + th2)


def lane_anchor(lane, x0, y0, h0, l_max):
    """(searched, on the lane, (s0, l0, dir, dh)) of a track on lane = dict(sx, sy, length)"""
    length = lane["length"]
    if not (0.0 < length < MAX_LENGTH):
        return False, False, (0.0, 0.0, 0.0, 0.0)
    row, _ = P.project(lane["sx"], lane["sy"], length, x0, y0, h0)
    s0, l0, hp = float(row[0]), float(row[1]), float(row[6])
    on = math.isfinite(l0) and abs(l0) <= l_max
    return True, on, (s0, l0, (1.0 if math.cos(h0 - hp) >= 0.0 else -1.0) if on else 0.0, K.constrain_angle(h0 - hp))


def lane_pose(lane, s0, l0, direction, D):
    sx, sy = lane["sx"], lane["sy"]
    sf = s0 + direction * D
    way = math.atan2(K.spline_deriv(sy, 1, sf), K.spline_deriv(sx, 1, sf))
    x = K.spline_eval(sx, sf) + l0 * math.cos(way + math.pi / 2)
    y = K.spline_eval(sy, sf) + l0 * math.sin(way + math.pi / 2)
    return x, y, (K.constrain_angle(way + math.pi) if direction < 0.0 else way), sf


def predict_track(track, t0, dt, m, r, prm=(V_CAP, GROW, L_MAX), lane=None, lane_far=False, anchor=None):
    """one present slot: (rows [M][6], flags, anchor [4]).  lane: dict(sx, sy, length) or None; lane_far: lane_of was at or above n_lanes;
    anchor: the (s0, l0, dir, ..) to take in place of this restatement's own search (the device's, whose s0 is within the projection's
    bound of it and not bit for bit: libm against ocml)"""
    v_cap, grow, l_max = prm
    x0, y0, h0, v, a, w, hl, hw, radius = (float(t) for t in track)
    M = (m - 1) * r + 1
    rows = np.zeros((M, 6))
    if hl < 0.0 or hw < 0.0:
        rows[:] = ABSENT_ROW
        return rows, ABSENT, np.zeros(4)
    if not all(math.isfinite(t) for t in (x0, y0, h0, v, a, w, hl, hw, radius)) or v < 0.0 or radius < 0.0:
        rows[:, :3] = np.nan
        rows[:, 3:] = (hl, hw, radius)
        return rows, BAD, np.zeros(4)
    flags, anc, on = (LANE_FAR if lane_far else 0), (0.0, 0.0, 0.0, 0.0), False
    if lane is not None:
        searched, on, anc = lane_anchor(lane, x0, y0, h0, l_max)
        if anchor is not None and searched:
            anc = tuple(float(t) for t in anchor)
            on = math.isfinite(anc[1]) and abs(anc[1]) <= l_max
            assert (anc[2] != 0.0) == on, anc
        flags |= ON_LANE if on else LANE_FAR
    for f in range(M):
        tau = step_time(t0, dt, r, f)
        te, ve, stop, cap = speed(v, a, v_cap, tau)
        tc = tau - te
        flags |= (STOPS if stop else 0) | (CAPPED if cap else 0)
        if on:
            D = (v + (0.5 * a) * te) * te + ve * tc
            x, y, h, sf = lane_pose(lane, anc[0], anc[1], anc[2], D)
            if sf < 0.0 or sf > lane["length"]:
                flags |= OFF_LANE
        else:
            x, y, h = free_pose(x0, y0, h0, v, a, w, te, ve, tc)
        rows[f] = (x, y, h, hl, hw, radius + grow * tau)
    return rows, flags, np.array(anc)


def lane_heading(lane, s):
    return math.atan2(K.spline_deriv(lane["sy"], 1, s), K.spline_deriv(lane["sx"], 1, s))


def predict(tracks, t0, dt, m, r, a_of=None, lane_of=None, lanes=(), prm=(V_CAP, GROW, L_MAX), anchors=None):
    """pqp_predict_agents: dict(agents [S][A][M][6], flags [S][A], anchor [S][A][4]); anchors: the device's, see predict_track"""
    tracks = np.asarray(tracks, dtype=np.float64)
    S, A = tracks.shape[:2]
    M = (m - 1) * r + 1
    agents, flags, anchor = np.zeros((S, A, M, 6)), np.zeros((S, A), np.int32), np.zeros((S, A, 4))
    for s in range(S):
        count = A if a_of is None else min(max(int(a_of[s]), 0), A)
        for g in range(A):
            if g >= count:
                agents[s, g] = ABSENT_ROW
                flags[s, g] = ABSENT
                continue
            want = -1 if lane_of is None else int(lane_of[s][g])
            lane = lanes[want] if 0 <= want < len(lanes) else None
            agents[s, g], flags[s, g], anchor[s, g] = predict_track(tracks[s, g], t0, dt, m, r, prm, lane, want >= len(lanes),
                                                                    None if anchors is None else anchors[s, g])
    return dict(agents=agents, flags=flags, anchor=anchor)


# ---- the motion itself, integrated: x' = v cos h, y' = v sin h, h' = w [v > 0], v' = a until the stop or the cap -----------------------------
def _rk4(state, a, w, span, delta):
    """(x, y, h, v) after `span` seconds of constant a and w, in ceil(span / delta) equal RK4 steps"""
    if span <= 0.0:
        return state
    n = max(1, math.ceil(span / delta - 1e-12))
    hstep = span / n
    f = lambda s: (s[3] * math.cos(s[2]), s[3] * math.sin(s[2]), w, a)
    for _ in range(n):
        k1 = f(state)
        k2 = f(tuple(state[j] + 0.5 * hstep * k1[j] for j in range(4)))
        k3 = f(tuple(state[j] + 0.5 * hstep * k2[j] for j in range(4)))
        k4 = f(tuple(state[j] + hstep * k3[j] for j in range(4)))
        state = tuple(state[j] + (hstep * (k1[j] + 2.0 * k2[j] + 2.0 * k3[j] + k4[j])) / 6.0 for j in range(4))
    return state


def integrate(track, times, v_cap, delta):
    """[len(times)][3] x, y, unwrapped heading at the ascending `times`: RK4 at step `delta` on the pieces between the sample times and
    the one event (the stop at v / -a, or the cap at (v_cap - v) / a), behind which the speed is constant"""
    x0, y0, h0, v, a, w = (float(t) for t in track[:6])
    if v == 0.0 and a <= 0.0:                                                  # stands from the start
        return np.array([(x0, y0, h0)] * len(times))
    event = v / (-a) if a < 0.0 else (max(v_cap - v, 0.0) / a if a > 0.0 else math.inf)
    after_v = 0.0 if a < 0.0 else max(v, v_cap)
    state, now, out, past = (x0, y0, h0, v), 0.0, [], False
    for t in times:
        if not past and t >= event:
            state = _rk4(state, a, w, event - now, delta)
            state, now, past = (state[0], state[1], state[2], after_v), event, True
        state, now = _rk4(state, 0.0 if past else a, w if state[3] > 0.0 or not past else 0.0, t - now, delta), t
        out.append(state[:3])
    return np.array(out)


# ---- lanes and tracks --------------------------------------------------------------------------------------------------------------------
def make_lane(x, y):
    """dict(sx, sy, length, tab [9][m], ext [4]) of the natural spline through the points, the knots at the accumulated chord length"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = np.concatenate(([0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))))
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    tab, ext = K.pack_spline(sx, sy)
    return dict(sx=sx, sy=sy, length=float(s[-1]), tab=tab, ext=ext)


LANE_M = 12


def straight_lane():
    """40 m along x from (0, 0): knots 40 / 11 m apart"""
    return make_lane(np.linspace(0.0, 40.0, LANE_M), np.zeros(LANE_M))


def dyadic_lane():
    """44 m along x from (0, 0), knots 4 m apart: every knot, and with them the table, is a dyadic number"""
    return make_lane(np.arange(LANE_M) * 4.0, np.zeros(LANE_M))


def arc_lane():
    """a quarter of a circle of radius 30 m from (5, -20), turning left"""
    phi = np.linspace(0.0, 0.5 * math.pi, LANE_M)
    return make_lane(5.0 + 30.0 * np.sin(phi), -20.0 + 30.0 * (1.0 - np.cos(phi)))


def pack_lanes(lanes):
    """(spline [n][9][m], ext [n][4], length [n]) as Handle.predict_agents takes them"""
    return (np.stack([l["tab"] for l in lanes]), np.stack([l["ext"] for l in lanes]), np.array([l["length"] for l in lanes]))


def on_lane_track(lane, s, off, v, a, oncoming=False, turn=0.1, size=(2.2, 0.9, 0.3)):
    """a track `off` to the left of the lane at s, its heading the lane's turned by `turn` (and by pi when oncoming)"""
    x, y = P.point_at(lane["sx"], lane["sy"], s, off)
    h = K.constrain_angle(lane_heading(lane, s) + turn + (math.pi if oncoming else 0.0))
    return [x, y, h, v, a, 0.2, *size]


def seeded_tracks(S, A, seed, span=500.0):
    """tracks [S][A][9] within the bounds the GPU test's tolerance is worked out for: |x|, |y| <= span, v <= 40, |a| <= 3, the yaw rate 0
    or 0.05 .. 0.5 rad/s of either sign"""
    rng = np.random.default_rng(seed)
    t = np.zeros((S, A, 9))
    t[..., 0:2] = rng.uniform(-span, span, (S, A, 2))
    t[..., 2] = rng.uniform(-math.pi, math.pi, (S, A))
    t[..., 3] = rng.uniform(0.0, 40.0, (S, A))
    t[..., 4] = rng.choice([-3.0, -1.25, 0.0, 0.75, 3.0], (S, A))
    t[..., 5] = rng.choice([-1.0, 0.0, 1.0], (S, A)) * rng.uniform(0.05, 0.5, (S, A))
    t[..., 6] = rng.uniform(0.0, 3.0, (S, A))
    t[..., 7] = rng.uniform(0.0, 1.5, (S, A))
    t[..., 8] = rng.uniform(0.0, 0.5, (S, A))
    return t


def write_case(path, tracks, m, r, dt):
    """the file tests/cpp/predict_demo.cpp reads: one scene of free-model tracks"""
    tracks = np.ascontiguousarray(tracks, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(np.array([tracks.shape[0], m, r], np.int32).tobytes())
        f.write(np.array([dt], np.float64).tobytes())
        f.write(tracks.tobytes())
