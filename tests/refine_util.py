"""pqp_speed_refine restated in numpy float64 and Python integers (include/pqp.h states the definition): which paths are refined, the
corridor from the search's occupancy bits, the QP as dense (P, q, A, l, u) in the reference order [s(m) v(m) a(m)] with the rows in the
device's order, the placement of a station s on the path and the rows and the excess that follow from it.  The solve itself is not
restated: tests hand the QP to the banded core's host emulation (banded_util) and to HiGHS (oracle/highs_qp.py).  Every operation of the
corridor and the placement is a correctly rounded IEEE one in the stated order, so `bounds` and - at a given s - x, y, heading, k and
excess agree with the device bit for bit (sqrt is correctly rounded on both sides)."""
import math

import numpy as np

import sample_util as T
import search_util as S

W_REF, W_ACCEL, W_JERK, A_MAX, D_MAX, N_PARAMS = 0, 1, 2, 3, 4, 5
REFINED, KEPT, INFEASIBLE = 1, 2, 4
UNSOLVED, SOLVED, PRIMAL_INFEASIBLE = 0, 1, 4
DEFAULT_PRM, DEFAULT_WINDOW = np.array([1.0, 1.0, 1.0, 1.5, 3.0]), 4
INF = 1e30


def pose_at(path, profile, c, at):
    """the search's "pose at sigma" for any stations `at` [..] on a path with driven count c: (pose [..][4] = x, y, heading, k, w [..] =
    the envelope's v^2 there)"""
    x, y, h, k = (path[:c, q] for q in (0, 1, 2, 5))
    s, v, a = (profile[:c, q] for q in range(3))
    at = np.asarray(at, dtype=np.float64)
    M = np.maximum.accumulate(s)
    with np.errstate(all="ignore"):
        i = np.maximum(np.searchsorted(M, at, side="right") - 1, 0)
        inside = i < c - 1
        pose = np.zeros(at.shape + (4,))
        w = np.zeros(at.shape)
        pose[~inside] = [x[c - 1], y[c - 1], h[c - 1], k[c - 1]]
        w[~inside] = v[c - 1] * v[c - 1]
        if inside.any():
            i0 = i[inside]
            i1 = i0 + 1
            dx, dy = x[i1] - x[i0], y[i1] - y[i0]
            d = np.sqrt(dx * dx + dy * dy)
            e = np.fmin(np.fmax(at[inside] - s[i0], 0.0), d)
            lam = np.where(d > 0.0, e / np.where(d > 0.0, d, 1.0), 0.0)
            r = np.zeros((len(i0), 4))
            r[:, 0] = x[i0] + lam * dx
            r[:, 1] = y[i0] + lam * dy
            r[:, 2] = T.constrain_angle(h[i0] + lam * T.constrain_angle(h[i1] - h[i0]))
            r[:, 3] = k[i0] + lam * (k[i1] - k[i0])
            pose[inside] = r
            w[inside] = v[i0] * v[i0] + (2.0 * a[i0]) * e
    return pose, w


def corridor(cells, j_of, J, venv, window, ds):
    """cells bool [m][S] (search_util.unpack of `blocked`), j_of [m] -> bounds [m][3] = lo, hi, vcap, or None when a j_k is outside the path or
    not free in occ_k (no search wrote such steps).  Also returns the integer runs [m][2]"""
    m, S_ = cells.shape
    win = min(int(window), S_)
    bounds, runs = np.zeros((m, 3)), np.zeros((m, 2), np.int64)
    for k in range(m):
        occ = cells[k] | cells[max(k - 1, 0)] | cells[min(k + 1, m - 1)]
        jk = int(j_of[k])
        if not 0 <= jk < J or occ[jk]:
            return None, None
        low, high = max(jk - win, 0), min(jk + win, J - 1)
        below, above = np.flatnonzero(occ[low:jk + 1]), np.flatnonzero(occ[jk:high + 1])
        jlo = low + int(below[-1]) + 1 if below.size else low
        jhi = jk + int(above[0]) - 1 if above.size else high
        runs[k] = jlo, jhi
        vcap = venv[jlo]
        for j in range(jlo + 1, jhi + 1):
            vcap = np.fmax(vcap, venv[j])
        bounds[k] = [0.0 if k == 0 else np.float64(jlo) * ds, 0.0 if k == 0 else np.float64(jhi) * ds, vcap]
    return bounds, runs


def qp(bounds, sigma, v_start, dt, prm):
    """dense (P, q, A, l, u) of the speed QP in the order [s(m) v(m) a(m)]; rows k, m + k, 2m + k: the boxes; 3m + k, 4m - 1 + k: the dynamics.
    The numbers are the device's (refine_assemble_kernel), operation by operation"""
    m = len(sigma)
    dt = np.float64(dt)
    w_ref, w_accel, w_jerk, a_max, d_max = (np.float64(prm[i]) for i in range(N_PARAMS))
    jerk = w_jerk / (dt * dt)
    nv, nc = 3 * m, 5 * m - 2
    P, q, A = np.zeros((nv, nv)), np.zeros(nv), np.zeros((nc, nv))
    lo, up = np.zeros(nc), np.zeros(nc)
    for k in range(m):
        last = k == m - 1
        P[k, k] = 2.0 * w_ref
        P[2 * m + k, 2 * m + k] = 2.0 * w_accel + np.float64((k > 0) + (0 if last else 1)) * (2.0 * jerk)
        if not last:
            P[2 * m + k, 2 * m + k + 1] = P[2 * m + k + 1, 2 * m + k] = -(2.0 * jerk)
        q[k] = -(2.0 * w_ref) * sigma[k]
        A[k, k] = A[m + k, m + k] = A[2 * m + k, 2 * m + k] = 1.0
        if k == 0:
            lo[0] = up[0] = 0.0
            lo[m] = up[m] = v_start
        else:
            lo[k], up[k] = bounds[k, 0], bounds[k, 1]
            lo[m + k], up[m + k] = 0.0, bounds[k, 2]
        lo[2 * m + k], up[2 * m + k] = (0.0, 0.0) if last else (-d_max, a_max)
        if not last:
            r = 3 * m + k
            A[r, k], A[r, m + k], A[r, 2 * m + k], A[r, k + 1] = -1.0, -dt, -(0.5 * (dt * dt)), 1.0
            r = 4 * m - 1 + k
            A[r, m + k], A[r, 2 * m + k], A[r, m + k + 1] = -1.0, -dt, 1.0
    return P, q, A, lo, up


def objective(x, sigma, dt, prm):
    m = len(sigma)
    s, a = x[:m], x[2 * m:]
    return float(prm[W_REF] * ((s - sigma) ** 2).sum() + prm[W_ACCEL] * (a ** 2).sum() + prm[W_JERK] * ((np.diff(a) / dt) ** 2).sum())


def certificate(P, q, A, lo, up, x, y=None, active_tol=1e-6):
    """the KKT residuals of x for min 1/2 x'Px + q'x, l <= Ax <= u: dict(stationarity, primal, complementarity), infinity norms.  Without
    multipliers they are recovered: on the rows that x holds at a bound to active_tol, the y of the right sign (free on an equality
    row, >= 0 at an upper bound, <= 0 at a lower one) that leaves the least stationarity residual in the 2-norm - a bounded least-squares
    problem (scipy's BVLS); the rows away from their bounds get 0.  Complementarity is then 0 up to active_tol times a multiplier."""
    from scipy.optimize import lsq_linear
    z = A @ x
    if y is None:
        at_lo, at_up = np.abs(z - lo) <= active_tol, np.abs(z - up) <= active_tol
        act = at_lo | at_up
        y = np.zeros(len(lo))
        if act.any():
            lower = np.where(at_lo[act], -np.inf, 0.0)
            upper = np.where(at_up[act], np.inf, 0.0)
            y[act] = lsq_linear(A[act].T, -(P @ x + q), bounds=(lower, upper), method="bvls", tol=1e-15).x
    finite_lo, finite_up = lo > -INF, up < INF
    comp = np.zeros(len(lo))
    comp[finite_up] = np.maximum(y[finite_up], 0.0) * np.abs(up[finite_up] - z[finite_up])
    comp[finite_lo] = np.maximum(comp[finite_lo], np.maximum(-y[finite_lo], 0.0) * np.abs(z[finite_lo] - lo[finite_lo]))
    comp[~finite_up] = np.maximum(comp[~finite_up], np.maximum(y[~finite_up], 0.0))
    comp[~finite_lo] = np.maximum(comp[~finite_lo], np.maximum(-y[~finite_lo], 0.0))
    return dict(stationarity=float(np.abs(P @ x + q + A.T @ y).max()), primal=float(np.maximum(np.maximum(lo - z, z - up), 0.0).max()),
                complementarity=float(comp.max()))


def rows_at(path, profile, c, s, v, a, dt):
    """the refined rows [m][8] and the excess for stations s (clamped already), speeds v (clamped already) and accelerations a"""
    m = len(s)
    pose, w = pose_at(path, profile, c, s)
    rows = np.zeros((m, 8))
    rows[:, :4] = pose
    rows[:, 4], rows[:, 5], rows[:, 6] = s, v, a
    rows[:, 7] = np.arange(m).astype(np.float64) * np.float64(dt)
    with np.errstate(all="ignore"):
        excess = float(np.max(v - np.sqrt(np.fmax(w, 0.0))))
    return rows, excess


def setup(path, profile, v_start, found, m, n_of=None, stop_before=None, grid=None, prm=None, window=None):
    """one path with what the search wrote for it (found: dict(blocked [m][W], steps [m][2], reached, traj [m][8])) ->
    dict(kept, c, bounds [m][3], runs, sigma [m], qp = (P, q, A, l, u) or None)"""
    grid = S.params(**(grid or {}))
    prm = DEFAULT_PRM if prm is None else np.asarray(prm, dtype=np.float64)
    window = DEFAULT_WINDOW if window is None else int(window)
    path, profile = np.asarray(path, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    out = dict(kept=True, c=0, bounds=np.zeros((m, 3)), runs=None, sigma=None, qp=None)
    if m < 2 or int(found["reached"]) != m:
        return out
    c = T.driven(path.shape[0], n_of, stop_before)
    v0 = np.float64(v_start)
    if c == 0 or not (np.isfinite(path[:c][:, [0, 1, 2, 5]]).all() and np.isfinite(profile[:c, :3]).all() and np.isfinite(v0) and v0 >= 0.0):
        return out
    J, _, _, venv, _ = S.stations(path, profile, c, grid)
    if J == 0:
        return out
    cells = S.unpack(np.asarray(found["blocked"]), grid["stations"])
    ds = np.float64(grid["ds"])
    bounds, runs = corridor(cells, np.asarray(found["steps"])[:, 0], J, venv, window, ds)
    if bounds is None:
        return out
    sigma = np.asarray(found["steps"])[:, 0].astype(np.float64) * ds
    return dict(kept=False, c=c, bounds=bounds, runs=runs, sigma=sigma, qp=qp(bounds, sigma, v0, grid["dt"], prm), J=J)


def finish(path, profile, su, found, x, status, dt):
    """what the call writes for one path from its setup `su`, the solver's x in the order [s v a] and its status:
    dict(traj, bounds, excess, status, flags)"""
    m = np.asarray(found["traj"]).shape[0]
    if su["kept"] or status != SOLVED:
        st = UNSOLVED if su["kept"] else status
        return dict(traj=np.array(found["traj"], dtype=np.float64), bounds=np.zeros((m, 3)), excess=math.nan, status=st,
                    flags=KEPT | (INFEASIBLE if st == PRIMAL_INFEASIBLE else 0))
    b = su["bounds"]
    s = np.fmin(np.fmax(x[:m], b[:, 0]), b[:, 1])
    v = np.fmax(x[m:2 * m], 0.0)
    a = np.array(x[2 * m:], dtype=np.float64)
    a[m - 1] = 0.0
    rows, excess = rows_at(np.asarray(path, dtype=np.float64), np.asarray(profile, dtype=np.float64), su["c"], s, v, a, dt)
    return dict(traj=rows, bounds=b, excess=excess, status=SOLVED, flags=REFINED)


def from_interleaved(x3, m):
    """the device's (s, v, a)_k order -> [s(m) v(m) a(m)]"""
    return np.concatenate([x3[0::3][:m], x3[1::3][:m], x3[2::3][:m]])


# ---- the cases of tests/test_speed_refine.py and tests/test_gpu_speed_refine.py ---------------------------------------------------------------
def found_of(res, b):
    """path b of a search_util.search_batch result, as setup() takes it"""
    return dict(blocked=res["blocked"][b], steps=res["steps"][b], reached=int(res["reached"][b]), traj=res["traj"][b])


def hand_rest():
    """from rest on a free road: search_util's hand case free_road under the prices of crossing_wait (a change of step costs as much as a
    slow cell, so the staircase accelerates by a cell per layer, which a_max = 1.5 m/s^2 can follow)"""
    return dict(S.hand_cases()["free_road"], m=S.HAND_M, prm=S.params(stations=48, w_accel=1.0))


def hand_quick():
    """free_road as it is: a change of step costs next to nothing, the staircase grows by q_up = 3 cells a layer and stands at 9 m after
    three layers, where a_max = 1.5 m/s^2 from rest gets to 6.75 m: below the corridor's 7 m.  The QP is infeasible"""
    return dict(S.hand_cases()["free_road"], m=S.HAND_M)


def hand_wait():
    """search_util's crossing_wait - a pedestrian disc of 0.5 m at x = 9.25 during layers 2 and 3 - searched with a margin of 1 m: the disc
    then holds stations 8 .. 23 and the plan waits in front of it.  A free station is clear of the disc by the search's margin, 1 m, so
    the whole corridor is clear of it by more than CHECK_MARGIN + ds, whatever lies between two stations"""
    c = S.hand_cases()["crossing_wait"]
    return dict(c, m=S.HAND_M, prm=dict(c["prm"], margin=1.0))


CHECK_MARGIN = 0.5                                           # pqp_agents_check's margin for the refined waiting plan


def seeded(name):
    """a search case by name -> the dict search_util.run_case takes.  m2 .. m40: seeded scenes on the synthetic paths with one crossing disc
    each"""
    if name in HAND:
        return HAND[name]()
    if name in S.SEEDED:
        return S.seeded(name)
    m = int(name[1:])
    B, n = 3, 200 if m > 12 else 120
    stations = 128 if m <= 12 else 100
    grid = S.params(stations=stations, q_max=6 if m <= 12 else 2, q_up=2, q_down=3, w_accel=0.25, margin=0.25, dt=1.0 if m <= 12 else 0.5)
    c = dict(paths=S.synth_paths(B, n, first=m), v_start=np.array([0.0, 1.5, 3.0]), prm=grid, m=m, n_of=None, stop_before=None)
    c["profile"] = S._profiles(c["paths"], c["v_start"])
    c["scene_of"], c["a_of"] = np.array([0, 1, 0], np.int32), None
    agents = np.stack([np.stack([S.absent(m)])] * 2)
    agents[0, 0] = S._at_station(c, 0, 6, tuple(range(1, min(m, 4))), (0.0, 0.0, 0.4), ahead=3.0, side=0.2)
    agents[1, 0] = S._at_station(c, 1, 12, tuple(range(min(2, m - 1), min(m, 5))), (0.0, 0.0, 0.5), ahead=3.0, side=-0.3)
    c["agents"] = agents
    return c


HAND = dict(rest=hand_rest, quick=hand_quick, wait=hand_wait)
QP_CASES = ("rest", "quick", "wait", "m2", "m3", "m8", "m12", "m40")
GPU_CASES = QP_CASES + ("tiles", "long", "m86", "m193")
INFEASIBLE_CASES = {("quick", 0)}                            # (case, path): the QPs that have no feasible point; every other refined path is solved
CAPACITY_M = 193                                             # the most layers the banded core holds: BqLayout{3m, 5m - 2, 3}.total() * 8 <= 160 KiB


def layout_doubles(m):
    """BqLayout{3m, 5m - 2, 3}.total(false) of pqp_banded_qp.hpp, restated: the doubles of LDS a QP of m layers takes"""
    nv, nc, bw = 3 * m, 5 * m - 2, 3
    nb = (nv + bw - 1) // bw
    nbb = nb * bw
    return nb * 4 * bw + (nb // 2 + 1) * 2 * bw * bw + nv + 4 * nbb + 3 * nv + 12 * nc + 128


def circles_of(name):
    import footprint_util as F
    return F.car_circles(**S.HAND_CAR) if name in HAND else F.car_circles()


_REFERENCE = {}


def reference(name, highs=True):
    """one case through the search's restatement, the setup, the core's host emulation and (highs) HiGHS, computed once and shared;
    nobody writes to it.  dict(case, res, m, each = [dict(su, found, emu, xe, xh, highs)]): xe / xh in the order [s v a], None where the
    path is kept or the solver found the QP infeasible; highs: HiGHS's model status"""
    key = (name, highs)
    if key in _REFERENCE:
        return _REFERENCE[key]
    import scipy.sparse as sp

    import banded_util as B
    import emu_util as E
    import highs_qp as H
    c = seeded(name)
    res = S.run_case(c, circles_of(name))
    m = c.get("m") or c["agents"].shape[2]
    each = []
    for b in range(len(c["paths"])):
        pick = lambda a: None if a is None else a[b]
        found = found_of(res, b)
        su = setup(c["paths"][b], c["profile"][b], c["v_start"][b], found, m, pick(c.get("n_of")), pick(c.get("stop_before")), c["prm"])
        one = dict(su=su, found=found, emu=None, xe=None, xh=None, highs=None)
        if not su["kept"]:
            P, q, A, lo, up = su["qp"]
            one["emu"] = B.emu_solve(E.production(polish=1), B.to_banded(P, q, A, lo, up, B.interleave3(m)))
            if one["emu"]["status"] == SOLVED:
                one["xe"] = from_interleaved(one["emu"]["x"], m)
            if highs:
                try:
                    one["xh"], one["highs"] = H.solve_qp(P, q, A, lo, up)[0], "Optimal"
                except RuntimeError:
                    one["highs"] = H._solve_once(sp.csc_matrix(P), q, sp.csc_matrix(A), lo, up, 1e-9)[2]
        each.append(one)
    _REFERENCE[key] = dict(case=c, res=res, m=m, each=each)
    return _REFERENCE[key]

# what tests/test_speed_refine.py measures over GPU_CASES on the emulation (its docstring has the figures to three digits); the GPU test's
# bounds are 4 x KKT_WORST and 2 x HIGHS_DIST
KKT_WORST = dict(stationarity=3.6e-8, primal=3.0e-8, complementarity=2.6e-7)
HIGHS_DIST = 2.9e-6
