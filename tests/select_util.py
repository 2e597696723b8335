"""pqp_select_paths restated in float64 numpy from the contract in include/pqp.h (not from the kernels): eligibility, the eight terms
with np.sum, the score, the lowest-index rule on equal scores, best_paths / best_n.  The checker of tests/test_select_paths.py and
tests/test_gpu_select_paths.py."""
from dataclasses import dataclass

import numpy as np

SOLVED, CHAIN_OK = 1, 0          # PQP_STATUS_SOLVED, PQP_CHAIN_OK
U = 2.0 ** -53                   # unit roundoff of a double


@dataclass
class Params:                    # pqp_select_default_params
    weight_kappa: float = 20.0
    weight_dkappa: float = 100.0
    weight_offset: float = 0.0
    weight_length: float = 0.0
    weight_clearance: float = 0.0
    clearance_want: float = 0.6
    per_waypoint: int = 0
    require_free: int = 1


def counts(paths, n_of):
    B, n = paths.shape[0], paths.shape[1]
    return np.full(B, n, np.int64) if n_of is None else np.clip(np.asarray(n_of, np.int64), 0, n)


def _addends(path, margin, c, prm):
    """the addends of terms 1, 2, 3, 4, 6 of one candidate of count c >= 2 (margin: its row or None)"""
    x, y, l, k, dk = (path[:c, j] for j in (0, 1, 3, 5, 6))
    chord = np.sqrt((x[1:] - x[:-1]) ** 2 + (y[1:] - y[:-1]) ** 2)
    short = np.zeros(0) if margin is None else np.maximum(0.0, prm.clearance_want - margin[:c]) ** 2
    return {1: k * k, 2: dk[:c - 1] ** 2, 3: l * l, 4: chord, 6: short}


def weights(prm):
    return {1: prm.weight_kappa, 2: prm.weight_dkappa, 3: prm.weight_offset, 4: prm.weight_length, 6: prm.weight_clearance}


def terms(paths, n_of=None, status=None, stage=None, first_collision=None, margin=None, prm=None, with_bound=False):
    """terms [B][8]; with_bound: also bound [B][8], 4 count 2^-53 S per term with S the sum of the absolute values of the term's addends
    (for the score: of the weighted addends of the terms it is made of) - what a re-ordered float64 summation of rounded addends may differ by"""
    prm = prm or Params()
    paths = np.asarray(paths, np.float64)
    B = paths.shape[0]
    cnt = counts(paths, n_of)
    t, bound = np.zeros((B, 8)), np.zeros((B, 8))
    with np.errstate(all="ignore"):
        for b in range(B):
            c = int(cnt[b])
            if c < 2:
                continue
            add = _addends(paths[b], None if margin is None else np.asarray(margin, np.float64)[b], c, prm)
            div = float(c) if prm.per_waypoint else 1.0
            S = {}
            for j, a in add.items():
                t[b, j] = np.sum(a) / (div if j != 4 else 1.0)
                S[j] = np.sum(np.abs(a)) / (div if j != 4 else 1.0)
                bound[b, j] = 4 * c * U * S[j]
            if margin is not None:
                t[b, 5] = np.min(np.asarray(margin, np.float64)[b, :c])
            w = weights(prm)
            t[b, 0] = w[1] * t[b, 1] + w[2] * t[b, 2] + w[3] * t[b, 3] + w[4] * t[b, 4] + w[6] * t[b, 6]
            bound[b, 0] = 4 * c * U * sum(abs(w[j]) * S[j] for j in w)
            ok = np.isfinite(t[b, 0])
            ok = ok and (status is None or status[b] == SOLVED) and (stage is None or stage[b] == CHAIN_OK)
            ok = ok and (first_collision is None or not prm.require_free or first_collision[b] == c)
            t[b, 7] = 1.0 if ok else 0.0
    return (t, bound) if with_bound else t


def group_bounds(group_start, batch):
    """the rows of every group as the device form takes an untrusted group_start: boundaries clamped to [0, batch], a descending pair empty"""
    gs = np.clip(np.asarray(group_start, np.int64), 0, batch)
    return [(int(gs[g]), max(int(gs[g]), int(gs[g + 1]))) for g in range(len(gs) - 1)]


def winners(t, group_start):
    """best [groups] from terms: the eligible candidate with the least score, the lowest index among equal scores, -1 without one"""
    best = []
    for lo, hi in group_bounds(group_start, t.shape[0]):
        idx = [b for b in range(lo, hi) if t[b, 7] == 1.0]
        if not idx:
            best.append(-1)
            continue
        least = min(t[b, 0] for b in idx)
        best.append(min(b for b in idx if t[b, 0] == least))
    return np.array(best, np.int32).reshape(-1)


def best_rows(paths, n_of, best):
    """best_paths [groups][n][7], best_n [groups] of the winners `best`"""
    paths = np.asarray(paths, np.float64)
    cnt = counts(paths, n_of)
    bp, bn = np.zeros((len(best), paths.shape[1], 7)), np.zeros(len(best), np.int32)
    for g, w in enumerate(best):
        if w >= 0:
            bn[g] = cnt[w]
            bp[g, :cnt[w]] = paths[w, :cnt[w], :7]
    return bp, bn


def select(paths, group_start, n_of=None, status=None, stage=None, first_collision=None, margin=None, prm=None):
    t = terms(paths, n_of, status, stage, first_collision, margin, prm)
    best = winners(t, group_start)
    bp, bn = best_rows(paths, n_of, best)
    return dict(terms=t, best=best, best_paths=bp, best_n=bn)


def write_candidates(path, candidates, group_start):
    """the file tests/cpp/select_demo.cpp reads"""
    with open(path, "wb") as f:
        f.write(np.array([len(candidates), len(group_start) - 1], np.int32).tobytes())
        f.write(np.asarray(group_start, np.int32).tobytes())
        for c in candidates:
            f.write(np.array([len(c)], np.int32).tobytes())
            f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
