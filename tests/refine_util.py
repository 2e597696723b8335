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


def finished_x(su, x):
    """the (s, v, a) the call writes for a solved path from the solver's x, both in the order [s v a]: finish()'s clamps - s into its
    corridor, v to 0 from below, a[m - 1] = 0"""
    m = len(su["sigma"])
    b = su["bounds"]
    a = np.array(x[2 * m:], dtype=np.float64)
    a[m - 1] = 0.0
    return np.concatenate([np.fmin(np.fmax(x[:m], b[:, 0]), b[:, 1]), np.fmax(x[m:2 * m], 0.0), a])


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


MAX_ITER = 2                                                 # PQP_STATUS_MAX_ITER
HIGHS_TOL = 1e-9                                             # HiGHS's primal and dual feasibility tolerance in every verdict here
HIGHS_SECONDS = 5.0

# ---- the case families of tests/test_speed_refine_fallback.py and tests/test_gpu_speed_refine_fallback.py ------------------------------------
# What the banded core does with polish = 1 after its direct active-set attempt is rejected (equilibration, ADMM, periodic polish
# attempts, the infeasibility certificate) runs for these QPs; the lists were chosen on the host emulation from the grid a_max in
# {0.8, 1.5, 1.6, 2.5} x d_max in {0.5, 3} x window in {1, 4, 12} x w_jerk in {0, 1, 50} and a few weights beside it.
JERKY = ((1.0, 1.0, 50.0, 1.5, 3.0), 1)                     # a heavy jerk weight in a narrow corridor: the fallback solves every path from m = 85 on
_STUCK = ((1.0, 1.0, 50.0, 1.5, 0.5), 1)                     # and with d_max = 0.5: no feasible point; the emulation ends two paths at MAX_ITER
_SLOW = ((1.0, 4.0, 0.0, 0.8, 3.0), 1)                       # w_accel = 4, no jerk term, a_max = 0.8: one path by the fallback, two directly
_EAGER = ((2.0, 1.0, 0.0, 1.5, 3.0), 4)                      # w_ref = 2, no jerk term: every path directly
_HEAVY = ((1.0, 4.0, 1.0, 1.5, 3.0), 4)                      # w_accel = 4: 24 iterations from m = 130 on
_LOOSE = ((0.5, 1.0, 50.0, 1.5, 3.0), 4)                     # w_ref = 0.5
# "params": (search case, refine parameters [w_ref w_accel w_jerk a_max d_max], window)
PARAMS = tuple((name,) + combo for name, combos in (
    ("m8", (_STUCK, _SLOW)), ("m40", (JERKY, _STUCK)), ("m85", (JERKY, _STUCK, _SLOW, _EAGER, _LOOSE)),
    ("m130", (JERKY, _STUCK, _SLOW)), ("m131", (JERKY, _STUCK, _SLOW, _EAGER)), ("m170", (_SLOW, _HEAVY)),
    ("m171", (JERKY, _SLOW)), ("m193", (JERKY, _STUCK, _HEAVY))) for combo in combos)
EDGE_M = (85, 86, 130, 131, 170, 171)                        # both sides of every form edge: under the defaults and under JERKY

# "staircases": name -> (m, seed, draws, the draws kept in their order, refine parameters, window): one batch per (window, w_jerk) of
# {1, 2, 4} x {0, 1, 50} under a_max = d_max = 0.6; kept are the draws the fallback solves, those without a feasible point and the first
# few that are solved directly
_STAIR_PRM = lambda w_jerk: (1.0, 1.0, w_jerk, 0.6, 0.6)
STAIRCASES = {
    "stairs_w1_j0": (8, 100, 200, (0, 1, 2, 3, 4, 5, 6, 7, 8, 36, 44, 83, 113, 128, 154, 160), _STAIR_PRM(0.0), 1),
    "stairs_w1_j1": (12, 101, 200, (0, 1, 2, 3, 4, 5, 6, 16, 24, 36, 48, 61, 81, 125, 141, 165), _STAIR_PRM(1.0), 1),
    "stairs_w1_j50": (8, 102, 200, (0, 1, 2, 3, 4, 5, 30, 104, 105, 110, 111, 126, 135, 193), _STAIR_PRM(50.0), 1),
    "stairs_w2_j0": (12, 103, 200, (0, 1, 2, 3, 4, 5, 22, 40, 59, 61, 68, 75, 122, 127, 138, 163), _STAIR_PRM(0.0), 2),
    "stairs_w2_j1": (8, 104, 200, (0, 1, 2, 3, 4, 5, 36, 97), _STAIR_PRM(1.0), 2),
    "stairs_w2_j50": (12, 105, 200, (0, 1, 2, 3, 4, 5, 8, 18, 58, 185, 193), _STAIR_PRM(50.0), 2),
    "stairs_w4_j0": (8, 106, 200, (0, 1, 2, 3, 4, 5, 6, 7), _STAIR_PRM(0.0), 4),
    "stairs_w4_j1": (12, 107, 200, (0, 1, 2, 3, 4, 5, 88, 90, 104, 112, 148), _STAIR_PRM(1.0), 4),
    "stairs_w4_j50": (8, 108, 200, (0, 1, 2, 3, 4, 5, 6, 37, 108, 138), _STAIR_PRM(50.0), 4),
}
STAIR_CALLS = tuple((name, v[4], v[5]) for name, v in STAIRCASES.items())

# "threshold": the hand case "quick" is infeasible below a_max = THRESHOLD_A_MAX and feasible from it on - bisected on HiGHS's verdict
# (2026-10-20, HIGHS_TOL = 1e-9, the interval left was 8e-13 wide); 1.0047 x 7 / 4.5
THRESHOLD_A_MAX = 1.5629168251338
THRESHOLD_NEAR = (1e-2, 1e-3)                                # these members follow HiGHS's verdict
THRESHOLD_CLOSE = (1e-5, 1e-7)                               # these are within rounding of the edge: only the safety properties
_around = lambda eps, sign: ("quick", (1.0, 1.0, 1.0, THRESHOLD_A_MAX * (1.0 + sign * eps), 3.0), DEFAULT_WINDOW)
THRESHOLD_FOLLOWS = tuple(_around(eps, sign) for eps in THRESHOLD_NEAR for sign in (-1.0, 1.0))
THRESHOLD_LEFT_OUT = tuple(_around(eps, sign) for eps in THRESHOLD_CLOSE for sign in (-1.0, 1.0))
THRESHOLD = THRESHOLD_FOLLOWS + THRESHOLD_LEFT_OUT


def verdict_class(one):
    """the emulation's verdict on one refined path: "direct" (SOLVED at iteration 0), "fallback" (SOLVED later), "infeasible" or "max_iter\""""
    e = one["emu"]
    if e["status"] == SOLVED:
        return "direct" if e["iters"] == 0 else "fallback"
    return {PRIMAL_INFEASIBLE: "infeasible", MAX_ITER: "max_iter"}[e["status"]]


def form_of_case(name):
    return form_of_layers(searched(name)[2])
CHECK_MARGIN = 0.5                                     # pqp_agents_check's margin for the refined waiting plan


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


def refine_shape(m):
    """sm_shape (pqp_smoothers.hip) for kBandedRefine: variables, rows, block size, half-bandwidth of P"""
    return dict(nv=3 * m, nc=5 * m - 2, bw=3, pbw=3)


def form_of_layers(m):
    """(B, MAXT, STAGE) of the kernel sm_solve launches for the refine's QP of m layers, None where the core does not hold it: banded_cases'
    selection on the refine's shape"""
    import banded_cases as BC
    sh = refine_shape(m)
    lay = BC.layout(sh["nv"], sh["nc"], sh["bw"])
    threads = 64 * ((lay["nbb"] + 63) // 64)
    if lay["plain"] * 8 > BC.LDS_PER_CU or threads > 1024:
        return None
    stage = threads <= 512 and lay["staged"] * 8 <= BC.LDS_PER_CU
    if threads <= 256 and stage:
        return (sh["bw"], 256, 1)
    if threads <= 512:
        return (sh["bw"], 512, 1 if stage else 0)
    return (sh["bw"], 1024, 0)


# first m, last m, form: every form the refine's shape selects; one layer more than the last does not fit
FORM_RANGES = ((2, 85, (3, 256, 1)), (86, 130, (3, 512, 1)), (131, 170, (3, 512, 0)), (171, 193, (3, 1024, 0)))
FIRST_PLAIN_M = 131                                          # from here on the device runs a non-staged form: the emulation runs both


# ---- "staircases": many different QPs in one call ---------------------------------------------------------------------------------------------
def staircase_draws(m, seed, count, q_top=6):
    """`count` seeded staircases of m layers on the hand road (hand_rest's path, profile and grid): the step q_k a random walk in 0 .. q_top
    with |q_k+1 - q_k| <= 2, j_k their running sum from j_0 = 0; a draw that leaves the path (j > j_last) is drawn again.  v_start lies
    within 0.2 m/s of q_0 ds / dt.  -> (case, res): what searched() returns for a search case, `blocked` zeros, reached = m, and traj the
    rows search_util.search writes for those steps"""
    base = hand_rest()
    grid = S.params(**base["prm"])
    path, profile = base["paths"][0], base["profile"][0]
    J, _, pose, _, _ = S.stations(path, profile, path.shape[0], grid)
    ds, dt = np.float64(grid["ds"]), np.float64(grid["dt"])
    rng = np.random.default_rng(seed)
    steps, v_start = np.zeros((count, m, 2), np.int32), np.zeros(count)
    got = 0
    while got < count:
        q = np.zeros(m, np.int64)
        q[0] = rng.integers(0, q_top + 1)
        for k in range(1, m):
            q[k] = min(max(q[k - 1] + rng.integers(-2, 3), 0), q_top)
        j = np.concatenate([[0], np.cumsum(q[:-1])])         # layer k + 1 stands q_k cells behind layer k
        v0 = max(0.0, float(q[0]) * float(ds / dt) + rng.uniform(-0.2, 0.2))
        if j[-1] > J - 1:
            continue
        steps[got, :, 0], steps[got, :, 1], v_start[got] = j, q, v0
        got += 1
    traj = np.zeros((count, m, 8))
    for b in range(count):
        for k in range(m):
            j, q = (int(v) for v in steps[b, k])
            dq = int(steps[b, k + 1, 1]) - q if k + 1 < m else 0
            traj[b, k] = [pose[j, 0], pose[j, 1], pose[j, 2], pose[j, 3], np.float64(j) * ds, np.float64(q) * ds / dt, np.float64(dq) * ds / (dt * dt),
                          np.float64(k) * dt]
    case = dict(paths=np.repeat(base["paths"], count, axis=0), profile=np.repeat(base["profile"], count, axis=0), v_start=v_start, prm=grid, m=m,
                n_of=None, stop_before=None)
    res = dict(blocked=np.zeros((count, m, S.words(grid["stations"])), np.int32), steps=steps, reached=np.full(count, m, np.int32), traj=traj)
    return case, res


def staircases(name):
    """the batch `name` of STAIRCASES: the draws listed there, in that order"""
    m, seed, count, keep = STAIRCASES[name][:4]
    c, res = staircase_draws(m, seed, count)
    keep = np.asarray(keep)
    c = {k: (v[keep] if k in ("paths", "profile", "v_start") else v) for k, v in c.items()}
    return c, {k: v[keep] for k, v in res.items()}


def circles_of(name):
    import footprint_util as F
    return F.car_circles(**S.HAND_CAR) if name in HAND or name in STAIRCASES else F.car_circles()


_REFERENCE, _SEARCHED = {}, {}


def searched(name):
    """(case, what the search's restatement writes for it, m) of a case by name, computed once; nobody writes to it"""
    if name not in _SEARCHED:
        if name in STAIRCASES:
            c, res = staircases(name)
        else:
            c = seeded(name)
            res = S.run_case(c, circles_of(name))
        _SEARCHED[name] = (c, res, c.get("m") or c["agents"].shape[2])
    return _SEARCHED[name]


def highs_verdict(P, q, A, lo, up):
    """(x or None, HiGHS's model status).  Its active-set solver cycles on an ordering now and then: each run has HIGHS_SECONDS, after
    which highs_qp.solve_qp hands the QP over in another ordering"""
    import scipy.sparse as sp

    import highs_qp as H
    try:
        return H.solve_qp(P, q, A, lo, up, tol=HIGHS_TOL, time_limit=HIGHS_SECONDS)[0], "Optimal"
    except RuntimeError:
        x, _, status = H._solve_once(sp.csc_matrix(P), q, sp.csc_matrix(A), lo, up, HIGHS_TOL, HIGHS_SECONDS)
        return (None, status) if x is None else (x, "Optimal (rows missed)")


def reference(name, highs=True, prm=None, window=None):
    """one case through the search's restatement, the setup under the refine's parameters (prm [5], window; the defaults when None), the
    core's host emulation and (highs) HiGHS, computed once and shared; nobody writes to it.  dict(case, res, m, prm, window, each =
    [dict(su, found, emu, plain, xe, xh, highs)]): emu: the emulation's staged form, plain: its non-staged form where the device runs one
    (m >= FIRST_PLAIN_M); xe / xh in the order [s v a], None where the path is kept or the solver found the QP infeasible; highs:
    HiGHS's model status"""
    prm = DEFAULT_PRM if prm is None else np.asarray(prm, dtype=np.float64)
    window = DEFAULT_WINDOW if window is None else int(window)
    key = (name, highs, tuple(prm.tolist()), window)
    if key in _REFERENCE:
        return _REFERENCE[key]
    import banded_util as B
    import emu_util as E
    c, res, m = searched(name)
    each = []
    for b in range(len(c["paths"])):
        pick = lambda a: None if a is None else a[b]
        found = found_of(res, b)
        su = setup(c["paths"][b], c["profile"][b], c["v_start"][b], found, m, pick(c.get("n_of")), pick(c.get("stop_before")), c["prm"], prm, window)
        one = dict(su=su, found=found, emu=None, plain=None, xe=None, xh=None, highs=None)
        if not su["kept"]:
            P, q, A, lo, up = su["qp"]
            bd = B.to_banded(P, q, A, lo, up, B.interleave3(m))
            one["emu"] = B.emu_solve(E.production(polish=1), bd)
            if m >= FIRST_PLAIN_M:
                one["plain"] = B.emu_solve(E.production(polish=1), bd, stage=False)
            if one["emu"]["status"] == SOLVED:
                one["xe"] = from_interleaved(one["emu"]["x"], m)
            if highs:
                one["xh"], one["highs"] = highs_verdict(P, q, A, lo, up)
        each.append(one)
    _REFERENCE[key] = dict(case=c, res=res, m=m, prm=prm, window=window, each=each)
    return _REFERENCE[key]


# what tests/test_speed_refine.py measures over GPU_CASES on the emulation (its docstring has the figures to three digits); the GPU test's
# bounds are 4 x KKT_WORST and 2 x HIGHS_DIST
KKT_WORST = dict(stationarity=3.6e-8, primal=3.0e-8, complementarity=2.6e-7)
HIGHS_DIST = 2.9e-6
# the same over the families above, where the core's fallback runs (tests/test_speed_refine_fallback.py measures them over FIGURES_QPS
# solved QPs): the emulation's own multipliers, the multipliers recovered from x alone, the distance to HiGHS.  The complementarity is
# the same figure either way - a multiplier times the distance a row that counts as active is left off its bound - and a hundred times
# KKT_WORST's.  KKT_RETURNED_FALLBACK: the recovered-multiplier figures of what the call returns for the emulation's x, finished_x() - the
# clamps move a variable by what the polish leaves an active row off its bound (up to 6e-8 here: a[m - 1] = 0, s into its corridor),
# and under w_jerk = 50 the jerk term's Hessian entries of 2 w_jerk / dt^2 = 100 turn that into a stationarity residual of 3.5e-6.
# tests/test_gpu_speed_refine_fallback.py certifies the rows the device returns the same way and holds them to 4 x KKT_RETURNED_FALLBACK
# and 2 x the distance
KKT_WORST_FALLBACK = dict(stationarity=1.0e-7, primal=8.7e-8, complementarity=3.1e-5)
KKT_RECOVERED_FALLBACK = dict(stationarity=6.2e-8, primal=8.7e-8, complementarity=3.1e-5)
KKT_RETURNED_FALLBACK = dict(stationarity=3.5e-6, primal=1.6e-7, complementarity=5.5e-5)
HIGHS_DIST_FALLBACK = 4.7e-6
FIGURES_QPS = 173
