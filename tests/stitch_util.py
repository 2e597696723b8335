"""Test helper: pqp_stitch_trajectory restated in numpy float64 (one rounding per operation) from include/pqp.h, operation by operation,
with predict_util's free model; the margin of every comparison a group's flags hang on; a plain per-row loop of the same definition that
shares no array expression with it; and the plans, measurements and the demo's file that tests/test_stitch_trajectory.py and
tests/test_gpu_stitch_trajectory.py share."""
import math

import numpy as np

import corridor_oracle as K
import predict_util as PR

BAD, NO_PREVIOUS, TIME, BAD_PLAN, LATERAL, LONGITUDINAL, HEADING, REPLAN, STITCHED, PREFIX_CUT, STANDING = (1 << k for k in range(11))
REASONS = NO_PREVIOUS | TIME | BAD_PLAN | LATERAL | LONGITUDINAL | HEADING
T_AHEAD, LAT_MAX, LON_MAX, DH_MAX, V_STILL, V_CAP = 0.1, 0.5, 2.5, 0.5, 0.1, math.inf          # pqp_stitch_default_params
DEFAULT = (T_AHEAD, LAT_MAX, LON_MAX, DH_MAX, V_STILL, V_CAP)
KEEP = 20
# the columns of `margins`: how far each comparison a flag hangs on was from going the other way, +inf where it was not made
M_LAT, M_LON, M_DH, M_STILL, M_NOW, M_START = range(6)
MARGIN_NAMES = ("lat_max", "lon_max", "dh_max", "v_still", "t_now", "tq")


def _first(mask):
    at = np.flatnonzero(mask)
    return int(at[0]) if at.size else -1


def _time_margin(t, bound):
    """the least |t_f - bound| over the rows that are not exactly on the bound (equal bits compare equal on any machine: no margin is
    needed there), +inf when there is none"""
    gap = np.abs(t - bound)
    gap = gap[np.isfinite(gap) & (gap > 0.0)]
    return float(gap.min()) if gap.size else math.inf


def replanned_state(meas, t_now, prm):
    """(state row, standing, |ve - v_still|) of a measurement advanced by t_ahead under the free model"""
    t_ahead, v_still, v_cap = prm[0], prm[4], prm[5]
    x, y, hd, v, a, w = (float(q) for q in meas)
    te, ve, stop, cap = PR.speed(v, a, v_cap, t_ahead)
    tc = t_ahead - te
    px, py, ph = PR.free_pose(x, y, hd, v, a, w, te, ve, tc)
    k = w / ve if ve > v_still else 0.0
    return np.array([px, py, ph, k, 0.0, ve, 0.0 if (stop or cap) else a, t_now + t_ahead]), ve == 0.0, abs(ve - v_still)


def stitch_group(rows, meas, t_now, prm=DEFAULT, keep=KEEP, prefix_max=None):
    """one group: rows [M][>= 8] (the plan's own rows, already cut to its count) -> dict(state [8], flags, dev [3], idx [3], prefix
    [prefix_n][8], margins [6]); prefix_max None: nothing is cut"""
    t_ahead, lat_max, lon_max, dh_max = (float(q) for q in prm[:4])
    rows = np.asarray(rows, dtype=np.float64)[:, :8]
    M = rows.shape[0]
    meas = np.asarray(meas, dtype=np.float64)
    t_now = float(t_now)
    margins = np.full(6, math.inf)
    out = dict(state=np.zeros(8), flags=0, dev=np.zeros(3), idx=np.full(3, -1, np.int32), prefix=np.zeros((0, 8)), margins=margins)
    if not (np.isfinite(meas).all() and math.isfinite(t_now)) or meas[3] < 0.0:
        out["flags"] = BAD
        return out
    x, y, hd = (float(q) for q in meas[:3])
    tq = t_now + t_ahead
    flags, i_now, p, i_start = 0, -1, -1, -1
    if M < 2:
        flags |= NO_PREVIOUS
    else:
        t = rows[:, 7]
        with np.errstate(invalid="ignore", over="ignore"):
            i_now, i_start = _first(t >= t_now), _first(t >= tq)
            ex, ey = x - rows[:, 0], y - rows[:, 1]
            d2 = ex * ex + ey * ey
        margins[M_NOW], margins[M_START] = _time_margin(t, t_now), _time_margin(t, tq)
        if t_now < t[0] or i_start < 0:
            flags |= TIME
        d2 = np.where(np.isfinite(d2), d2, math.inf)
        p = int(np.argmin(d2)) if np.isfinite(d2).any() else -1                      # argmin: the lowest index of the least
        used = [f for f in (p, i_now, i_now - 1, i_start) if f >= 0]
        numbers = p >= 0 and all(np.isfinite(rows[f]).all() for f in used)
        if not numbers:
            flags |= BAD_PLAN
        if numbers and i_now >= 0:
            xp, yp, hp, sp = (float(q) for q in rows[p, [0, 1, 2, 4]])
            sh, ch = math.sin(hp), math.cos(hp)
            dx, dy = x - xp, y - yp
            lat = -dx * sh + dy * ch
            s_ref = float(rows[0, 4])
            if i_now > 0:
                s1, t1, s0, t0 = (float(q) for q in (rows[i_now, 4], rows[i_now, 7], rows[i_now - 1, 4], rows[i_now - 1, 7]))
                s_ref = s0 + (s1 - s0) * ((t_now - t0) / (t1 - t0))
            lon = s_ref - (sp + (dx * ch + dy * sh))
            dh = K.constrain_angle(hd - hp)
            flags |= (0 if abs(lat) <= lat_max else LATERAL) | (0 if abs(lon) <= lon_max else LONGITUDINAL) | (0 if abs(dh) <= dh_max else HEADING)
            out["dev"] = np.array([lon, lat, dh])
            margins[M_LAT], margins[M_LON], margins[M_DH] = abs(abs(lat) - lat_max), abs(abs(lon) - lon_max), abs(abs(dh) - dh_max)
    out["idx"] = np.array([i_now, p, i_start], np.int32)
    if flags & REASONS:
        state, standing, margins[M_STILL] = replanned_state(meas, t_now, prm)
        out["flags"] = flags | REPLAN | (STANDING if standing else 0)
        out["state"] = state
        out["prefix"] = state[None].copy()
        out["prefix"][0, 7] = 0.0
        return out
    i0 = max(0, i_now - int(keep))
    if prefix_max is not None and i_start - i0 + 1 > prefix_max:
        i0 = i_start - prefix_max + 1
        flags |= PREFIX_CUT
    piece = rows[i0:i_start + 1].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        piece[:, 4] = piece[:, 4] - rows[i_start, 4]
        piece[:, 7] = piece[:, 7] - rows[i_start, 7]
    out["flags"] = flags | STITCHED
    out["state"] = rows[i_start].copy()
    out["prefix"] = piece
    return out


def group_rows(group_start, g, batch):
    """the candidates of group g as the kernels read a group_start: clamped to [0, batch], a descending pair an empty group"""
    if group_start is None:
        return min(g, batch), min(g + 1, batch)
    return min(max(int(group_start[g]), 0), batch), min(max(int(group_start[g + 1]), 0), batch)


def stitch(prev, meas, t_now, m_of=None, group_start=None, batch=None, prm=DEFAULT, keep=KEEP, prefix_max=None, fill=0.0):
    """pqp_stitch_trajectory: prev [G][m][stride >= 8], meas [G][6], t_now [G] -> dict(state [G][8], flags [G], dev [G][3], idx [G][3],
    prefix [G][prefix_max][8] (prefix_max None: m), prefix_n [G], start [batch][3], start_k [batch], v_start [batch], margins [G][6]).
    Candidates that are in no group keep `fill`."""
    prev = np.asarray(prev, dtype=np.float64)
    G, m = prev.shape[:2]
    cap = m if prefix_max is None else int(prefix_max)
    batch = G if batch is None else int(batch)
    res = dict(state=np.zeros((G, 8)), flags=np.zeros(G, np.int32), dev=np.zeros((G, 3)), idx=np.zeros((G, 3), np.int32),
               prefix=np.zeros((G, cap, 8)), prefix_n=np.zeros(G, np.int32), start=np.full((batch, 3), fill), start_k=np.full(batch, fill),
               v_start=np.full(batch, fill), margins=np.full((G, 6), math.inf))
    for g in range(G):
        M = m if m_of is None else min(max(int(m_of[g]), 0), m)
        one = stitch_group(prev[g, :M], meas[g], t_now[g], prm, keep, cap)
        n = one["prefix"].shape[0]
        res["state"][g], res["flags"][g], res["dev"][g], res["idx"][g], res["margins"][g] = one["state"], one["flags"], one["dev"], one["idx"], one["margins"]
        res["prefix"][g, :n], res["prefix_n"][g] = one["prefix"], n
        lo, hi = group_rows(group_start, g, batch)
        if hi > lo:
            res["start"][lo:hi], res["start_k"][lo:hi], res["v_start"][lo:hi] = one["state"][:3], one["state"][3], one["state"][5]
    return res


# ---- the same definition as a plain loop over the rows: no array expression, no argmin --------------------------------------------------------
def stitch_group_loop(rows, meas, t_now, prm=DEFAULT, keep=KEEP, prefix_max=None):
    """(state [8], flags, dev [3], idx [3], prefix rows) of one group, row by row in Python floats"""
    t_ahead, lat_max, lon_max, dh_max, v_still, v_cap = (float(q) for q in prm)
    R = [[float(q) for q in r[:8]] for r in rows]
    ms = [float(q) for q in meas]
    t_now = float(t_now)
    fin = math.isfinite
    if not all(fin(q) for q in ms + [t_now]) or ms[3] < 0.0:
        return [0.0] * 8, BAD, [0.0] * 3, [-1, -1, -1], []
    x, y, hd, v, a, w = ms
    tq = t_now + t_ahead
    flags, i_now, p, i_start, dev = 0, -1, -1, -1, [0.0, 0.0, 0.0]
    if len(R) < 2:
        flags |= NO_PREVIOUS
    else:
        least = math.inf
        for f, r in enumerate(R):
            if i_now < 0 and r[7] >= t_now:
                i_now = f
            if i_start < 0 and r[7] >= tq:
                i_start = f
            ex, ey = x - r[0], y - r[1]
            try:
                d2 = ex * ex + ey * ey
            except OverflowError:
                d2 = math.inf
            if fin(d2) and d2 < least:
                least, p = d2, f
        if t_now < R[0][7] or i_start < 0:
            flags |= TIME
        numbers = p >= 0
        for f in (p, i_now, i_now - 1, i_start):
            if f >= 0 and not all(fin(q) for q in R[f]):
                numbers = False
        if not numbers:
            flags |= BAD_PLAN
        elif i_now >= 0:
            rp = R[p]
            sh, ch = math.sin(rp[2]), math.cos(rp[2])
            dx, dy = x - rp[0], y - rp[1]
            lat = -dx * sh + dy * ch
            s_ref = R[0][4]
            if i_now > 0:
                r1, r0 = R[i_now], R[i_now - 1]
                s_ref = r0[4] + (r1[4] - r0[4]) * ((t_now - r0[7]) / (r1[7] - r0[7]))
            lon = s_ref - (rp[4] + (dx * ch + dy * sh))
            dh = K.constrain_angle(hd - rp[2])
            if not abs(lat) <= lat_max:
                flags |= LATERAL
            if not abs(lon) <= lon_max:
                flags |= LONGITUDINAL
            if not abs(dh) <= dh_max:
                flags |= HEADING
            dev = [lon, lat, dh]
    idx = [i_now, p, i_start]
    if flags & REASONS:
        te, ve, stop, cap = PR.speed(v, a, v_cap, t_ahead)
        px, py, ph = PR.free_pose(x, y, hd, v, a, w, te, ve, t_ahead - te)
        state = [px, py, ph, (w / ve if ve > v_still else 0.0), 0.0, ve, (0.0 if stop or cap else a), tq]
        return state, flags | REPLAN | (STANDING if ve == 0.0 else 0), dev, idx, [state[:7] + [0.0]]
    i0 = max(0, i_now - int(keep))
    if prefix_max is not None and i_start - i0 + 1 > prefix_max:
        i0, flags = i_start - prefix_max + 1, flags | PREFIX_CUT
    prefix = []
    for f in range(i0, i_start + 1):
        r = list(R[f])
        r[4], r[7] = r[4] - R[i_start][4], r[7] - R[i_start][7]
        prefix.append(r)
    return list(R[i_start]), flags | STITCHED, dev, idx, prefix


# ---- plans and measurements ----------------------------------------------------------------------------------------------------------------------
def arc_plan(m, dt=0.1, v=8.0, a=0.5, curvature=0.02, x0=3.0, y0=-2.0, h0=0.4, t0=0.0, s0=0.0, stride=8):
    """[m][stride] rows of a car on a circular arc (curvature 0: a line) under constant acceleration, t = t0 + f dt; the columns beyond 7
    hold a value no output may show"""
    rows = np.full((m, stride), -777.0)
    for f in range(m):
        tau = f * dt
        s = v * tau + 0.5 * a * tau * tau
        th = curvature * s
        if curvature != 0.0:
            lx, ly = math.sin(th) / curvature, (1.0 - math.cos(th)) / curvature
        else:
            lx, ly = s, 0.0
        rows[f, :8] = (x0 + lx * math.cos(h0) - ly * math.sin(h0), y0 + lx * math.sin(h0) + ly * math.cos(h0), h0 + th, curvature, s0 + s,
                       v + a * tau, a, t0 + tau)
    return rows


def displaced(row, lon, lat, dh, v=None, a=0.0, w=0.0):
    """the measurement of a car that is `lon` behind (positive: the plan is ahead), `lat` to the left of and turned by `dh` against a plan
    row: its deviations from that row are (lon, lat, dh) when the row is both the nearest and the one at t_now"""
    x, y, h = float(row[0]), float(row[1]), float(row[2])
    return np.array([x - lon * math.cos(h) - lat * math.sin(h), y - lon * math.sin(h) + lat * math.cos(h), h + dh,
                     float(row[5]) if v is None else v, a, w])


def seeded_case(G, m, seed, stride=8, replan=0.1, dt=0.1, ragged=True):
    """G plans of up to m rows around the origin (|x|, |y| well inside 1000 m) and a measurement each: beside its plan by a few
    centimetres, or - about `replan` of the groups - by metres or turned away, at a time between two rows.  dict(prev, m_of, meas, t_now)"""
    rng = np.random.default_rng(seed)
    prev = np.zeros((G, m, stride))
    m_of = np.full(G, m, np.int32)
    meas, t_now = np.zeros((G, 6)), np.zeros(G)
    for g in range(G):
        prev[g] = arc_plan(m, dt, v=rng.uniform(2.0, 15.0), a=rng.choice([-0.5, 0.0, 0.75]), curvature=rng.choice([-0.03, 0.0, 0.01, 0.05]),
                           x0=rng.uniform(-400.0, 400.0), y0=rng.uniform(-400.0, 400.0), h0=rng.uniform(-math.pi, math.pi), t0=rng.uniform(0.0, 5.0),
                           s0=rng.uniform(0.0, 50.0), stride=stride)
        if ragged and m > 2 and rng.random() < 0.3:
            m_of[g] = rng.integers(2, m + 1)
        M = int(m_of[g])
        at = int(rng.integers(0, max(M - 2, 1)))
        frac = rng.uniform(0.2, 0.8)
        row = prev[g, at] + frac * (prev[g, min(at + 1, M - 1)] - prev[g, at])
        off = rng.random() < replan
        lon, lat, dh = rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1)
        if off:
            kind = rng.integers(0, 3)
            lon, lat, dh = (lon + 6.0, lat, dh) if kind == 0 else ((lon, lat + rng.choice([-1.5, 1.5]), dh) if kind == 1 else (lon, lat, dh + 1.0))
        meas[g] = displaced(row, lon, lat, dh, a=rng.choice([-1.0, 0.0, 1.0]), w=rng.choice([0.0, 0.001, 0.3, -0.4]))
        t_now[g] = row[7]
    return dict(prev=prev, m_of=m_of, meas=meas, t_now=t_now)


def write_case(path, prev, dt, m_of, meas, t_now):
    """the file tests/cpp/stitch_demo.cpp reads: int32 G, m; double dt; int32 m_of [G]; double meas [G][6]; double t_now [G]; double prev
    [G][m][8] (its column t is not read: state f is at f dt)"""
    prev = np.ascontiguousarray(np.asarray(prev, dtype=np.float64)[:, :, :8])
    G, m = prev.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([G, m], np.int32).tobytes())
        f.write(np.array([dt], np.float64).tobytes())
        f.write(np.ascontiguousarray(m_of, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(meas, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(t_now, dtype=np.float64).tobytes())
        f.write(prev.tobytes())


# ---- the cases the device is held to (tests/test_gpu_stitch_trajectory.py), and whose margins tests/test_stitch_trajectory.py checks -----------
def _case(name, prev, meas, t_now, m_of=None, group_start=None, batch=None, prm=DEFAULT, keep=KEEP, prefix_max=None):
    return dict(name=name, prev=np.ascontiguousarray(prev), meas=np.ascontiguousarray(meas), t_now=np.ascontiguousarray(t_now),
                m_of=None if m_of is None else np.ascontiguousarray(m_of, dtype=np.int32),
                group_start=None if group_start is None else np.ascontiguousarray(group_start, dtype=np.int32), batch=batch, prm=tuple(prm), keep=keep,
                prefix_max=prefix_max)


def timed_plan(G, m, stride=8):
    """G copies of one plan on dyadic times, t = 1 + f / 8, and a measurement 5 cm beside row 3 of each: what the time cases start from"""
    prev = np.stack([arc_plan(m, dt=0.125, t0=1.0, stride=stride)] * G)
    meas = np.stack([displaced(prev[0, 3], 0.0, 0.05, 0.01, a=0.25, w=0.1)] * G)
    return prev, meas


def device_cases():
    """every case of the GPU test, by name; the shapes: m in {2, 63, 64, 65, 130}, G in {1, 5, 67}, keep in {0, 3, 200}, prefix_max in
    {1, 4, m}, stride 8 and 11, ragged m_of with 0 and 1, groups of 0, 1, 64, 65 and 130 candidates and none"""
    cases = []
    shapes = [(m, kp) for m in (2, 63, 64, 65, 130) for kp in ((0, 1), (3, 4), (200, None))]
    for k, (m, (keep, cap)) in enumerate(shapes):
        G, stride = (1, 5, 67)[k % 3], (8, 11)[k % 2]
        c = seeded_case(G, m, seed=100 + k, stride=stride, dt=0.05 if m == 2 else 0.1)
        # (m = 2: rows 0.05 s apart and t_ahead 0.02, so that a start in front of the last row exists)
        prm = (0.02,) + DEFAULT[1:] if m == 2 else DEFAULT
        cases.append(_case(f"m{m}_G{G}_s{stride}_keep{keep}_cap{cap}", c["prev"], c["meas"], c["t_now"], c["m_of"], prm=prm, keep=keep, prefix_max=cap))
    # ragged counts, 0 and 1 among them
    c = seeded_case(9, 65, seed=7, ragged=False)
    m_of = np.array([65, 0, 1, 2, 64, 30, 1, 65, 0], np.int32)
    for g in range(9):                                           # the measurement beside a row the shortened plan still has
        M = max(int(m_of[g]), 2)
        c["meas"][g] = displaced(c["prev"][g, (M - 2) // 2], 0.1, -0.1, 0.02, a=0.5, w=0.2)
        c["t_now"][g] = c["prev"][g, (M - 2) // 2, 7] + 0.03
    cases.append(_case("ragged", c["prev"], c["meas"], c["t_now"], m_of))
    # groups of 0, 1, 64, 65 and 130 candidates
    c = seeded_case(5, 71, seed=8)
    cases.append(_case("group_sizes", c["prev"], c["meas"], c["t_now"], c["m_of"], group_start=[0, 0, 1, 65, 130, 260], batch=260))
    # rows that are not numbers: away from the matched rows (stitched all the same), at p, at i_now - 1, at i_start, and a whole plan
    prev, meas = timed_plan(6, 40)
    t_now = np.full(6, prev[0, 3, 7] + 0.06)                     # between rows 3 and 4: i_now 4, i_start (t_ahead 0.13) 5, p 3
    prev[0, 20, 1] = np.nan; prev[0, 1, 5] = np.inf
    prev[1, 3, 3] = np.nan
    prev[2, 3, 0] = np.nan                                       # (its d2 is +inf: another row is the nearest, and row 3 is still i_now - 1)
    prev[3, 5, 6] = -np.inf
    prev[4, :, 0] = np.nan
    prev[5, 4, 4] = np.nan
    cases.append(_case("nan_rows", prev, meas, t_now, prm=(0.13,) + DEFAULT[1:]))
    # t_now before the first row, between rows, exactly on a row, past the last row, and so late that only the start is past it
    prev, meas = timed_plan(5, 40)
    t = prev[0, :, 7]
    t_now = np.array([t[0] - 0.3, t[3] + 0.06, t[3], t[-1] + 0.4, t[-1] - 0.05])
    meas[3] = displaced(prev[3, -1], 0.0, 0.05, 0.0)
    meas[4] = displaced(prev[4, -1], 0.0, 0.05, 0.0)
    cases.append(_case("times", prev, meas, t_now, prm=(0.13,) + DEFAULT[1:]))
    # replans under every branch of the free model: the turned angle below and above the Taylor switch (2^-6), no turn, a stop inside
    # t_ahead, standing, the cap reached and already exceeded, slow enough for curvature 0
    tracks = [(8.0, 0.5, 0.1), (8.0, 0.5, 0.4), (8.0, -1.0, -0.4), (6.0, 0.0, 0.0), (0.05, -1.0, 0.3), (0.0, 0.0, 0.3), (0.0, -1.0, 0.0), (9.95, 1.0, 0.2),
              (12.0, 1.0, -0.2), (0.06, 0.0, 0.5), (0.3, 0.0, 0.5)]
    prev, _ = timed_plan(len(tracks), 30)
    meas = np.array([displaced(prev[0, 3], 0.0, 1.5, 0.1, v=v, a=a, w=w) for v, a, w in tracks])
    cases.append(_case("replans", prev, meas, np.full(len(tracks), prev[0, 3, 7] + 0.06), prm=(0.1, 0.5, 2.5, 0.5, 0.1, 10.0)))
    # bad measurements between good neighbours
    c = seeded_case(8, 64, seed=9)
    c["meas"][1, 0] = np.nan; c["meas"][3, 3] = -0.5; c["meas"][5, 5] = np.inf; c["t_now"][6] = np.nan
    cases.append(_case("bad_measurements", c["prev"], c["meas"], c["t_now"], c["m_of"], group_start=[0, 1, 3, 3, 6, 7, 9, 10, 12], batch=12))
    # every deviation flag alone and in pairs, from one plan
    offs = [(3.0, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, 0.0, 0.7), (3.0, 0.8, 0.0), (3.0, 0.0, -0.7), (0.0, -0.8, 0.7), (-3.0, -0.8, -0.7), (0.4, 0.3, 0.2)]
    prev, _ = timed_plan(len(offs), 64)
    meas = np.array([displaced(prev[0, 30], lon, lat, dh) for lon, lat, dh in offs])
    cases.append(_case("deviation_flags", prev, meas, np.full(len(offs), prev[0, 30, 7]), prm=(0.13,) + DEFAULT[1:]))
    return cases


def run_case(c):
    """the restatement on a case"""
    return stitch(c["prev"], c["meas"], c["t_now"], c["m_of"], c["group_start"], c["batch"], c["prm"], c["keep"], c["prefix_max"])
