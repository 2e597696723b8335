"""pqp_select_plans restated in float64 numpy and Python integers from the contract in include/pqp.h (not from the kernels): the count,
the ten terms with sums in ascending order, eligibility, the lowest-row rule on equal scores, best_traj / best_m and best_paths / best_n.  The addends of
the four sums are formed by whole-array expressions (addends) and, to hold those to account, sample by sample in plain Python floats
(addends_loop): the same addends in the same array give the same sum.  The checker of tests/test_select_plans.py and
tests/test_gpu_select_plans.py.

What a sum may differ by.  The device adds a candidate's addends in another order than total(); the addends themselves are the same
correctly rounded products on both sides.  A float64 sum of n addends in any order is within (n - 1) u S / (1 - (n - 1) u) of the exact
sum, u = 2^-53 and S the sum of their absolute values, so two orders differ by at most twice that; 4 c u S, c the candidate's count,
covers it (select_util states the same bound).  The score is six products and five additions of the entries; every entry passes one
product and at most five additions, so evaluating it on entries that differ by d_j gives scores that differ by at most
sum |w_j| d_j + 2 * 6 u sum |w_j e_j| (to first order; 16 u is taken for the 12 u)."""
import math
from dataclasses import dataclass

import numpy as np

import select_util

PLAN_SCORE_STRIDE, RANK_PARAMS = 10, 7
W_PATH, W_PROGRESS, W_ACCEL, W_JUMP, W_LATERAL, W_CLEARANCE, CLEARANCE_WANT = range(7)
NO_PLAN, EMPTY, NOT_FINITE = 1, 16, 32       # PQP_SEARCH_*
U = 2.0 ** -53                               # unit roundoff of a double
SUMS = (2, 3, 4, 6)                          # the entries that are sums over the samples


@dataclass
class Params:                                # pqp_rank_default_params
    w_path: float = 1.0
    w_progress: float = 1.0
    w_accel: float = 1.0
    w_jump: float = 1.0
    w_lateral: float = 1.0
    w_clearance: float = 0.0
    clearance_want: float = 0.6
    require_free: int = 1

    def array(self):
        return np.array([self.w_path, self.w_progress, self.w_accel, self.w_jump, self.w_lateral, self.w_clearance, self.clearance_want], np.float64)


def counts(traj, m_of):
    B, m = traj.shape[0], traj.shape[1]
    return np.full(B, m, np.int64) if m_of is None else np.clip(np.asarray(m_of, np.int64), 0, m)


def addends(rows, c, clear, want):
    """the addends of entries 2, 3, 4, 6 of one candidate of count c >= 1 (rows [>= c][>= 8], clear: its clearance row or None)"""
    k, v, a, t = (np.ascontiguousarray(rows[:c, j]) for j in (3, 5, 6, 7))
    h = t[1:] - t[:-1]
    jump = a[1:] - a[:-1]
    kvv = k[:-1] * (v[:-1] * v[:-1])
    out = {2: (a[:-1] * a[:-1]) * h, 3: jump * jump, 4: (kvv * kvv) * h, 6: np.zeros(0)}
    if clear is not None:
        short = np.fmax(0.0, np.float64(want) - np.asarray(clear, np.float64)[:c - 1])
        out[6] = (short * short) * h
    return out


def addends_loop(rows, c, clear, want):
    """the same, one sample at a time in Python floats (IEEE doubles, one rounding per operation)"""
    out = {2: [], 3: [], 4: [], 6: []}
    for f in range(c - 1):
        k, v, a, t = (float(rows[f][j]) for j in (3, 5, 6, 7))
        a_next, t_next = float(rows[f + 1][6]), float(rows[f + 1][7])
        h = t_next - t
        out[2].append((a * a) * h)
        d = a_next - a
        out[3].append(d * d)
        kvv = k * (v * v)
        out[4].append((kvv * kvv) * h)
        if clear is not None:
            gap = float(want) - float(clear[f])
            short = 0.0 if (gap != gap or gap < 0.0) else gap            # fmax(0, gap): a NaN gives the other operand
            out[6].append((short * short) * h)
    return {j: np.array(v, np.float64) for j, v in out.items()}


def total(add):
    """the sum in ascending order (ufunc.accumulate adds one element at a time): an addend that is an exact zero changes nothing, so the
    jumps of a plan's m rows and of its fine rows, which are those jumps with zeros between them, have the same sum bit for bit"""
    return np.add.accumulate(add)[-1] if add.size else 0.0


def terms(traj, m_of=None, path_terms=None, search_flags=None, first_hit=None, clearance=None, prm=None, with_bound=False, one=addends):
    """terms [B][10]; with_bound: also bound [B][10] (see the module's text), zero for the entries that are exact"""
    prm = prm or Params()
    traj = np.asarray(traj, np.float64)
    B = traj.shape[0]
    cnt = counts(traj, m_of)
    w = prm.array()
    t, bound = np.zeros((B, PLAN_SCORE_STRIDE)), np.zeros((B, PLAN_SCORE_STRIDE))
    with np.errstate(all="ignore"):
        for b in range(B):
            c = int(cnt[b])
            if c < 1:
                continue
            rows = traj[b]
            clear = None if clearance is None else np.asarray(clearance, np.float64)[b]
            S = {}
            for j, add in one(rows, c, clear, prm.clearance_want).items():
                t[b, j] = total(add)
                S[j] = total(np.abs(add))
                bound[b, j] = 4 * c * U * S[j]
            t[b, 1] = rows[c - 1, 4] - rows[0, 4]
            t[b, 8] = rows[c - 1, 7] - rows[0, 7]
            if clear is not None:
                t[b, 5] = np.min(clear[:c])                              # NaN if any is; +inf if all are
            t[b, 7] = 0.0 if path_terms is None else path_terms[b][0]
            parts = [(w[W_PATH], 7), (w[W_PROGRESS], 1), (w[W_ACCEL], 2), (w[W_JUMP], 3), (w[W_LATERAL], 4), (w[W_CLEARANCE], 6)]
            t[b, 0] = w[W_PATH] * t[b, 7] - w[W_PROGRESS] * t[b, 1] + w[W_ACCEL] * t[b, 2] + w[W_JUMP] * t[b, 3] + w[W_LATERAL] * t[b, 4] + \
                w[W_CLEARANCE] * t[b, 6]
            bound[b, 0] = sum(abs(wj) * bound[b, j] for wj, j in parts) + 16 * U * sum(abs(wj) * (abs(t[b, j]) + bound[b, j]) for wj, j in parts)
            ok = bool(np.isfinite(t[b, 0]))
            ok = ok and (search_flags is None or (int(search_flags[b]) & (NO_PLAN | EMPTY | NOT_FINITE)) == 0)
            ok = ok and (first_hit is None or not prm.require_free or int(first_hit[b]) == c)
            ok = ok and (path_terms is None or path_terms[b][7] != 0.0)
            t[b, 9] = 1.0 if ok else 0.0
    return (t, bound) if with_bound else t


def winners(t, group_start):
    """best [groups] from terms: the eligible candidate with the least score, the lowest row among equal scores, -1 without one; an
    untrusted group_start is read by pqp_select_paths's clamping rule (select_util.group_bounds)"""
    best = []
    for lo, hi in select_util.group_bounds(group_start, t.shape[0]):
        idx = [b for b in range(lo, hi) if t[b, 9] == 1.0]
        if not idx:
            best.append(-1)
            continue
        least = min(t[b, 0] for b in idx)
        best.append(min(b for b in idx if t[b, 0] == least))
    return np.array(best, np.int32).reshape(-1)


def best_rows(traj, m_of, best):
    """best_traj [groups][m][8], best_m [groups] of the winners `best`"""
    traj = np.asarray(traj, np.float64)
    cnt = counts(traj, m_of)
    bt, bm = np.zeros((len(best), traj.shape[1], 8)), np.zeros(len(best), np.int32)
    for g, w in enumerate(best):
        if w >= 0:
            bm[g] = cnt[w]
            bt[g, :cnt[w]] = traj[w, :cnt[w], :8]
    return bt, bm


def select(traj, group_start, m_of=None, path_terms=None, search_flags=None, first_hit=None, clearance=None, paths=None, n_of=None, prm=None):
    t = terms(traj, m_of, path_terms, search_flags, first_hit, clearance, prm)
    best = winners(t, group_start)
    bt, bm = best_rows(traj, m_of, best)
    res = dict(terms=t, best=best, best_traj=bt, best_m=bm)
    if paths is not None:
        res["best_paths"], res["best_n"] = select_util.best_rows(paths, n_of, best)
    return res


# ---- the hand case the call exists for ---------------------------------------------------------------------------------------------------
HAND_DISC = (9.25, -1.5, 0.5)                # x, y, radius of the pedestrian disc, on the road during layers 2 and 3
HAND_K = 0.02                                # B's curvature: an arc of 50 m radius that leaves A's lane to the left


def hand_case():
    """One group of two candidates on one scene, on search_util's hand road (41 waypoints 0.5 m apart, the hand car, dt = 1, ds = 0.5,
    eight layers, from rest).  A is the straight road: no curvature, pqp_select_paths scores it 0.  B is an arc of curvature 0.02 to the
    left over the same arc lengths: pqp_select_paths scores it 20 * 41 * 0.02^2 = 0.328, so it picks A.  A disc of 0.5 m stands at
    (9.25, -1.5) during layers 2 and 3: it reaches into A's footprint and not into B's, which has left to the other side by then, so the
    search makes A wait in front of it and lets B pass.  Returns dict(paths [2][41][7], profile, v_start, agents [1][1][8][6], prm, m,
    group_start)"""
    import search_util as S
    n, m = S.HAND_N, S.HAND_M
    a = S.straight(n)
    s = 0.5 * np.arange(n)
    R = 1.0 / HAND_K
    b = np.zeros((n, 7))
    b[:, 0], b[:, 1], b[:, 2], b[:, 5] = R * np.sin(s / R), R * (1.0 - np.cos(s / R)), s / R, HAND_K
    paths = np.stack([a, b])
    v_start = np.array([0.0, 0.0])
    profile = np.stack([S.profile_of(p, 0.0, v_end=0.0) for p in paths])
    walk = S.absent(m)
    walk[2:4] = [HAND_DISC[0], HAND_DISC[1], 0.0, 0.0, 0.0, HAND_DISC[2]]
    return dict(paths=paths, profile=profile, v_start=v_start, agents=walk[None, None], prm=S.params(stations=48, w_accel=1.0), m=m,
                group_start=np.array([0, 2], np.int32))


def write_case(path, traj, dt, m_of, group_start, path_score=None):
    """the file tests/cpp/rank_demo.cpp reads: int32 batch, m, groups; double dt; int32 group_start [groups + 1]; int32 m_of [batch]; double
    path_score [batch]; double traj [batch][m][8] (the demo takes state f to be at f * dt and does not read column 7)"""
    traj = np.ascontiguousarray(traj, dtype=np.float64)
    B, m = traj.shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([B, m, len(group_start) - 1], np.int32).tobytes())
        f.write(np.array([dt], np.float64).tobytes())
        f.write(np.asarray(group_start, np.int32).tobytes())
        f.write((np.full(B, m, np.int32) if m_of is None else np.asarray(m_of, np.int32)).tobytes())
        f.write((np.zeros(B) if path_score is None else np.asarray(path_score, np.float64)).tobytes())
        f.write(traj[:, :, :8].tobytes())
