"""pqp_sample_trajectory restated in numpy float64 (include/pqp.h states the definition): one path at a time, operation by operation in
the stated order.  Every operation here is a correctly rounded IEEE one and numpy fuses none of them, so the device agrees with this bit
for bit - that is the bound of tests/test_gpu_sample_trajectory.py, not a tolerance."""
import math

import numpy as np

STRIDE = 8                                                   # x, y, heading, k, s, v, a, t
HORIZON_SHORT, STANDS, ENDS_MOVING, EMPTY, NOT_FINITE = 1, 2, 4, 8, 16
DEFAULTS = dict(dt=0.1, hold_last=0)
PI = 3.14159265358979323846


def driven(n, n_of=None, stop_before=None):
    """the driven count c: pqp_speed_profile's expression"""
    count = n if n_of is None else min(max(int(n_of), 0), n)
    return count if stop_before is None else min(count, max(int(stop_before), 0))


def constrain_angle(a):
    """include/tools/tools.hpp:24-35 as the library has it (csrc/pqp_path_lane.hpp): at most 64 turns"""
    a = np.array(a, dtype=np.float64)
    for _ in range(64):
        up, down = a > PI, a < -PI
        if not (up | down).any():
            break
        a = np.where(up, a - 2 * PI, np.where(down, a + 2 * PI, a))
    return a


def sample(path, profile, m, n_of=None, stop_before=None, t0=None, dt=0.1, hold_last=0):
    """path [n][stride >= 6], profile [n][4] -> (rows [m][8], m_of, flags)"""
    path, profile = np.asarray(path, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    n = path.shape[0]
    c = driven(n, n_of, stop_before)
    rows = np.zeros((m, STRIDE))
    if c == 0:
        return rows, 0, EMPTY
    t0 = np.float64(0.0 if t0 is None else t0)
    dt = np.float64(dt)
    x, y, h, k = (path[:c, q] for q in (0, 1, 2, 5))
    s, v, a, t = (profile[:c, q] for q in range(4))
    ok = all(np.isfinite(col).all() for col in (x, y, h, k, s, v, a)) and bool((t >= 0.0).all()) and bool(t0 >= 0.0) and bool(np.isfinite(t0))
    if not ok:
        rows[:] = math.nan
        return rows, 0, NOT_FINITE
    with np.errstate(all="ignore"):
        tau = t0 + np.arange(m).astype(np.float64) * dt
        T = np.maximum.accumulate(t)
        on = tau <= T[c - 1]
        m_of = int(on.sum())
        assert on[:m_of].all()                               # a prefix: tau ascends
        cnt = np.searchsorted(T, tau, side="right")          # #{ j < c : T_j <= tau }
        i = np.maximum(cnt - 1, 0)
        inside = on & (i < c - 1)
        flags = (HORIZON_SHORT if tau[m - 1] < T[c - 1] else 0) | (ENDS_MOVING if m_of < m and v[c - 1] > 0.0 else 0)
        if inside.any():
            i0 = i[inside]
            i1 = i0 + 1
            if (T[i1] == math.inf).any():
                flags |= STANDS
            tk = tau[inside]
            dx, dy = x[i1] - x[i0], y[i1] - y[i0]
            d = np.sqrt(dx * dx + dy * dy)
            u = tk - t[i0]
            e = np.fmin(np.fmax((v[i0] + (0.5 * a[i0]) * u) * u, 0.0), d)
            lam = np.where(d > 0.0, e / np.where(d > 0.0, d, 1.0), 0.0)
            r = rows[inside]
            r[:, 0] = x[i0] + lam * dx
            r[:, 1] = y[i0] + lam * dy
            r[:, 2] = constrain_angle(h[i0] + lam * constrain_angle(h[i1] - h[i0]))
            r[:, 3] = k[i0] + lam * (k[i1] - k[i0])
            r[:, 4] = s[i0] + e
            r[:, 5] = np.fmax(v[i0] + a[i0] * u, 0.0)
            r[:, 6] = a[i0]
            r[:, 7] = tk
            rows[inside] = r
        at_end = on & ~inside                                # waypoint c - 1 itself
        last = np.array([x[c - 1], y[c - 1], h[c - 1], k[c - 1], s[c - 1], v[c - 1], 0.0, 0.0])
        rows[at_end] = last
        rows[at_end, 7] = tau[at_end]
        if hold_last:
            last[5] = 0.0
            rows[~on] = last
            rows[~on, 7] = tau[~on]
    return rows, m_of, flags


def sample_batch(paths, profile, m, n_of=None, stop_before=None, t0=None, dt=0.1, hold_last=0):
    """the same for [B][n][stride] and [B][n][4]: (traj [B][m][8], m_of [B], flags [B])"""
    B = len(paths)
    pick = lambda a, b: None if a is None else a[b]
    got = [sample(paths[b], profile[b], m, pick(n_of, b), pick(stop_before, b), pick(t0, b), dt, hold_last) for b in range(B)]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.int32), np.array([g[2] for g in got], np.int32)


def seeded_path(rng, c, stride=7, step=(0.15, 1.0)):
    """[c][stride]: a slowly turning path of c waypoints, a chord of 0.15 to 1 m, heading across the +-pi seam, noise in the unused columns"""
    d = rng.uniform(step[0], step[1], c)
    k = 0.08 * np.sin(np.cumsum(d) / 9.0 + rng.uniform(0, 6.28)) + rng.normal(scale=0.004, size=c)
    head = constrain_angle(np.cumsum(k * d) + rng.uniform(-PI, PI))
    p = rng.normal(size=(c, stride))
    p[:, 0], p[:, 1], p[:, 2], p[:, 5] = np.cumsum(d * np.cos(head)), np.cumsum(d * np.sin(head)), head, k
    return p


def seeded_profile(rng, path, v_lo=0.5, v_hi=8.0):
    """[c][4] s, v, a, t from a path and seeded speeds by the profile's own formulas - a sequential sum here, which is as good an input"""
    c = path.shape[0]
    d = np.hypot(np.diff(path[:, 0]), np.diff(path[:, 1]))
    w = rng.uniform(v_lo, v_hi, c) ** 2
    v = np.sqrt(w)
    prof = np.zeros((c, 4))
    prof[:, 1] = v
    if c > 1:
        prof[1:, 0] = np.cumsum(d)
        prof[:-1, 2] = np.where(d > 0, (w[1:] - w[:-1]) / (2.0 * np.where(d > 0, d, 1.0)), 0.0)
        prof[1:, 3] = np.cumsum(np.where(d > 0, 2.0 * d / (v[:-1] + v[1:]), 0.0))
    return prof


def write_case(path, paths, profile, m, n_of, stop_before, t0, dt, hold_last):
    """the file tests/cpp/sample_demo.cpp reads; paths [B][n][stride >= 6], profile [B][n][4]"""
    paths, profile = np.asarray(paths, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(np.array(paths.shape[:2] + (m, hold_last), np.int32).tobytes())
        f.write(np.array([dt], np.float64).tobytes())
        f.write(np.asarray(n_of, np.int32).tobytes())
        f.write(np.asarray(stop_before, np.int32).tobytes())
        f.write(np.asarray(t0, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.concatenate([paths[:, :, [0, 1, 2, 5]], profile], axis=2)).tobytes())
