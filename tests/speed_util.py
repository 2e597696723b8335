"""pqp_speed_profile restated in float64 (include/pqp.h): arc length, speed, acceleration and time of every waypoint of a planned path.

profile() is the definition as a planner would write it: the chords summed one after the other, the forward pass (acceleration) then the
backward pass (braking) over w = v^2, one waypoint at a time.  scan_form() is the closed form the kernel evaluates - a prefix minimum and
a suffix minimum over cumulative sums - in numpy; the two share nothing but the caps and the chords, so each checks the other.

profile() runs its recurrences for s and w on the float64 caps and chords in exact rational arithmetic and rounds each result once.  A
float64 sum of 700 chords one after the other is off by a random walk of its roundings - a few u s_last - and w takes differences of s
times 2 a_max or 2 d_max: that error of the restatement's own would use up the 8 units w_tolerance() allows to whatever is compared
against it (numpy's cumsum in place of prefix_sum() below puts the scan form 8.6 units away).  Rounded once, the bounds are the other
side's.  scan_form() sums in the kernel's order: rows of 16 by Kogge-Stone, the rows' totals across the 64, tiles chained by a carry."""
import math
from fractions import Fraction

import numpy as np

START_TOO_FAST, STOPS_EARLY, NEVER_ARRIVES, EMPTY, NOT_FINITE = 1, 2, 4, 8, 16
STRIDE = 4
DEFAULTS = dict(v_max=10.0, a_max=1.5, d_max=3.0, a_lat_max=2.0)
U = 2.0 ** -53


def driven(n, n_of=None, stop_before=None):
    """(count, c) of one path"""
    count = n if n_of is None else min(max(int(n_of), 0), n)
    c = count if stop_before is None else min(count, max(int(stop_before), 0))
    return count, c


def _speed_ok(v):
    return v >= 0.0 and v < math.inf          # False for NaN


def caps(path, c, early, prm, v_start, v_end=None, v_limit=None):
    """cap_i in v^2 for i < c, or None when a value that is read is not what it must be"""
    x, y, k = path[:c, 0], path[:c, 1], path[:c, 5]
    lim = np.full(c, math.inf) if v_limit is None else np.asarray(v_limit, dtype=np.float64)[:c]
    ve = math.nan if v_end is None else float(v_end)
    if not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(k).all() and (lim >= 0.0).all() and _speed_ok(v_start)):
        return None
    if not early and not math.isnan(ve) and not _speed_ok(ve):
        return None
    cap = np.full(c, prm["v_max"] * prm["v_max"])
    cap = np.minimum(cap, lim * lim)
    curved = k != 0.0
    cap[curved] = np.minimum(cap[curved], prm["a_lat_max"] / np.abs(k[curved]))
    cap[0] = min(cap[0], v_start * v_start)
    if early:
        cap[c - 1] = 0.0
    elif not math.isnan(ve):
        cap[c - 1] = min(cap[c - 1], ve * ve)
    return cap


def chords(path, c):
    dx, dy = np.diff(path[:c, 0]), np.diff(path[:c, 1])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(dx * dx + dy * dy)


def accel_and_time(d, w):
    """a [c], the time of every chord [c - 1] and whether one of them is infinite: the definition's last two lines on given d and w"""
    c = len(w)
    v = np.sqrt(w)
    a = np.zeros(c)
    dt = np.zeros(max(c - 1, 0))
    for i in range(c - 1):
        if d[i] == 0.0:
            continue
        a[i] = (w[i + 1] - w[i]) / (2.0 * d[i])
        vv = v[i] + v[i + 1]
        dt[i] = math.inf if vv == 0.0 else 2.0 * d[i] / vv
    return a, dt, bool(np.isinf(dt).any())


def _finish(n, c, count, s, w, d, v_start):
    rows = np.zeros((n, STRIDE))
    a, dt, never = accel_and_time(d, w)
    t = np.zeros(c)
    for i in range(c - 1):
        t[i + 1] = t[i] + dt[i]
    rows[:c, 0], rows[:c, 1], rows[:c, 2], rows[:c, 3] = s, np.sqrt(w), a, t
    flags = (START_TOO_FAST if w[0] < v_start * v_start else 0) | (STOPS_EARLY if c < count else 0) | (NEVER_ARRIVES if never else 0)
    return rows, flags


def _rounded(q):
    try:
        return float(q)                                      # correctly rounded
    except OverflowError:
        return math.inf


def _not_finite(n, c):
    rows = np.zeros((n, STRIDE))
    rows[:c] = math.nan
    return rows, NOT_FINITE


def profile(path, v_start, n_of=None, stop_before=None, v_limit=None, v_end=None, prm=None):
    """One path [n][stride >= 6] -> (rows [n][4] = s, v, a, t, flags): the sequential forward pass then backward pass."""
    prm = dict(DEFAULTS, **(prm or {}))
    path = np.asarray(path, dtype=np.float64)
    n = path.shape[0]
    count, c = driven(n, n_of, stop_before)
    if c == 0:
        return np.zeros((n, STRIDE)), EMPTY | (STOPS_EARLY if count > 0 else 0)
    cap = caps(path, c, c < count, prm, float(v_start), v_end, v_limit)
    if cap is None:
        return _not_finite(n, c)
    d = chords(path, c)
    if not np.isfinite(d).all():
        return _not_finite(n, c)
    dq = [Fraction(float(v)) for v in d]
    sq = [Fraction(0)]
    for i in range(c - 1):
        sq.append(sq[i] + dq[i])
    s = np.array([_rounded(v) for v in sq])
    if not np.isfinite(s).all():
        return _not_finite(n, c)
    two_a, two_d = 2 * Fraction(prm["a_max"]), 2 * Fraction(prm["d_max"])
    wq = [Fraction(float(v)) for v in cap]
    for i in range(c - 1):                                   # forward: what the acceleration allows
        wq[i + 1] = min(wq[i + 1], wq[i] + two_a * dq[i])
    for i in range(c - 2, -1, -1):                           # backward: what the braking allows
        wq[i] = min(wq[i], wq[i + 1] + two_d * dq[i])
    w = np.array([_rounded(v) for v in wq])
    return _finish(n, c, count, s, w, d, float(v_start))


def prefix_sum(x):
    """inclusive prefix sums of x in the order of the kernel's scan (pqp_wave.hpp wave_prefix_sum, tiles of 64 chained by a carry)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(len(x))
    carry = 0.0
    lane = np.arange(64)
    for lo in range(0, len(x), 64):
        v = np.zeros(64)
        v[:len(x[lo:lo + 64])] = x[lo:lo + 64]
        for sh in (1, 2, 4, 8):                              # row_shr: lanes whose source is outside their row of 16 add 0
            src = np.where(lane % 16 >= sh, np.roll(v, sh), 0.0)
            v = v + src
        v = v + np.where((lane // 16) % 2 == 1, v[(lane // 16) * 16 - 1], 0.0)      # row_bcast:15 onto rows 1 and 3
        v = v + np.where(lane >= 32, v[31], 0.0)                                    # row_bcast:31 onto rows 2 and 3
        v = carry + v
        carry = v[63]
        out[lo:lo + 64] = v[:len(out[lo:lo + 64])]
    return out


def scan_form(path, v_start, n_of=None, stop_before=None, v_limit=None, v_end=None, prm=None):
    """The same by scans: s by prefix_sum, w_i = min(cap_i, min_{j<i} (cap_j - 2 a s_j) + 2 a s_i, min_{j>i} (cap_j + 2 d s_j) - 2 d s_i)."""
    prm = dict(DEFAULTS, **(prm or {}))
    path = np.asarray(path, dtype=np.float64)
    n = path.shape[0]
    count, c = driven(n, n_of, stop_before)
    if c == 0:
        return np.zeros((n, STRIDE)), EMPTY | (STOPS_EARLY if count > 0 else 0)
    cap = caps(path, c, c < count, prm, float(v_start), v_end, v_limit)
    if cap is None:
        return _not_finite(n, c)
    d = chords(path, c)
    with np.errstate(invalid="ignore"):
        s = prefix_sum(np.concatenate([[0.0], d]))
    if not np.isfinite(s).all():
        return _not_finite(n, c)
    two_a, two_d = 2.0 * prm["a_max"], 2.0 * prm["d_max"]
    before = np.concatenate([[math.inf], np.minimum.accumulate(cap - two_a * s)[:-1]])
    behind = np.concatenate([np.minimum.accumulate((cap + two_d * s)[::-1])[::-1][1:], [math.inf]])
    w = np.maximum(np.minimum(cap, np.minimum(before + two_a * s, behind - two_d * s)), 0.0)
    return _finish(n, c, count, s, w, d, float(v_start))


def batch_profile(paths, v_start, n_of=None, stop_before=None, v_limit=None, v_end=None, prm=None, form=profile):
    """paths [B][n][stride] -> (profile [B][n][4], flags [B])"""
    B = len(paths)
    pick = lambda a, b: None if a is None else a[b]
    res = [form(paths[b], v_start[b], pick(n_of, b), pick(stop_before, b), pick(v_limit, b), pick(v_end, b), prm) for b in range(B)]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)


def s_tolerance(c, s_last):
    """|s - restatement|: a sum of c - 1 terms in another order, (c - 1) u, plus the rounding of a chord"""
    return (c + 4) * U * s_last


def w_tolerance(cap, s_last, prm):
    """|v^2 - restatement|"""
    prm = dict(DEFAULTS, **(prm or {}))
    finite = cap[np.isfinite(cap)]
    return 8 * U * ((finite.max() if finite.size else 0.0) + 2.0 * max(prm["a_max"], prm["d_max"]) * s_last)


def seeded_path(rng, n, stride=7):
    """a wandering path: steps of 0.05 .. 1 m, a curvature column of its own (the profile reads k, it does not derive it)"""
    step = rng.uniform(0.05, 1.0, n)
    heading = np.cumsum(rng.normal(0.0, 0.08, n))
    p = np.zeros((n, stride))
    p[:, 0] = np.cumsum(step * np.cos(heading)) + rng.uniform(-50, 50)
    p[:, 1] = np.cumsum(step * np.sin(heading)) + rng.uniform(-50, 50)
    p[:, 5] = rng.normal(0.0, 0.15, n) * (rng.random(n) > 0.2)
    p[:, 2] = heading
    return p


def write_case(path, paths, n_of, stop_before, v_start, v_end):
    """the file tests/cpp/speed_demo.cpp reads; paths [B][n][stride >= 6]"""
    paths = np.asarray(paths, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(np.array(paths.shape[:2], np.int32).tobytes())
        f.write(np.asarray(n_of, np.int32).tobytes())
        f.write(np.asarray(stop_before, np.int32).tobytes())
        f.write(np.asarray(v_start, np.float64).tobytes())
        f.write(np.asarray(v_end, np.float64).tobytes())
        f.write(np.ascontiguousarray(paths[:, :, [0, 1, 5]]).tobytes())
