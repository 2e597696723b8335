"""The size matrix of the smoothers' generic banded ADMM core (pqp_banded_qp.hpp, banded_solve_kernel<B, MAXT, STAGE>): case table, input
builders and references shared by test_banded_core_sizes_cpu.py (the host emulation) and test_gpu_banded_core.py (the device).  Plain data
and functions, no fixtures.

A handle in the reference's own setting (OSQP defaults, eps 1e-3, polish = 0) runs S1-S3 on this core, one workgroup per QP and one lane per
(padded) variable.  pqp_smoothers.hip picks one of nine kernel forms by size: the block size B = 4 / 9 / 3 by QP type, 256 / 512 / 1024 lanes by
the padded variable count, and whether the row data of A, the index lists and q are staged in LDS (always at 256 lanes, at 512 while
BqLayout::total(true) fits one compute unit's 160 KB, never at 1024).  Past BqLayout::total(false) > 160 KB (or 1024 lanes) the core no
longer holds the QP and the exact kernels take over (iters = 0).  This file restates that selection (sm_shape, BqLayout, sm_solve,
sm_generic_fits), lists both edges of every form's size range, and builds ragged launches (a count per scenario in the pattern of n_max:
the n_of / m_of branch of the assemble kernels, their decoupled dummies) for every form past 256 lanes.
References: oracle/pqp_oracle.py's assembly of each scenario at its own size, run by its osqp_admm at the handle's own setting - the core is the
same iteration, so the two stop at the same check and agree to round-off (measured on the host emulation: |x - x_oracle| <= 2.9e-10 / 3.8e-8 /
3.4e-13 for S1 / S2 / S3; on an MI355X 3.3e-10 / 2.5e-8 / 1.4e-12), which is what the tests hold the device to."""
import numpy as np
import scipy.sparse as sp

import pqp_oracle as O
from smoother_cases import post_inputs, tension_inputs

S1, S2, S3 = 0, 1, 2                       # SM_TENSION2, SM_TENSION, SM_POST
NAME = {S1: "tension2", S2: "tension", S3: "post"}
MIN_SIZE = {S1: 3, S2: 4, S3: 4}           # tension2_ok / tension_ok / post_smooth_ok
ASSEMBLE_MIN = {S1: 2, S2: 4, S3: 1}       # the assemble kernels' clamp of a count
R_MAX, C_MAX = 4, 6                        # kRMax, kCMax
LDS_PER_CU = 160 * 1024                    # kLdsPerCu (pqp_internal.hpp)
X_BAR = 1e-6                               # device / emulation against the oracle's iterate: test_gpu_smoothers.test_tension2's bar for this comparison


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def sm_shape(t, n):
    """sm_shape (pqp_smoothers.hip): variables, rows, block size, half-bandwidth of P"""
    if t == S1:
        return dict(nv=4 * n - 1, nc=3 * (n - 1) + 2, bw=4, pbw=4)
    if t == S2:
        return dict(nv=3 * n, nc=3 * n, bw=9, pbw=9)
    return dict(nv=3 * n, nc=3 * n - 2, bw=3, pbw=0)


def layout(nv, nc, bw):
    """BqLayout::{nb, nbb, total(false), total(true)} in doubles"""
    nb = (nv + bw - 1) // bw
    nbb = nb * bw
    hm = nb * 4 * bw                                        # pivot rows
    x = hm + (nb // 2 + 1) * 2 * bw * bw                    # D^-1 S_left / D^-1 S_right of a level's blocks
    z = x + nv + 4 * nbb + 3 * nv                           # x | xt rhs pl pr | sig dsc xs
    red = z + 12 * nc                                       # z y zt rv e2 esc lo up act zs ys yp
    plain = red + 128
    staged = plain + 4 * nc + nv + (4 * nc + 12 * nv + 1) // 2      # aval, q, the three int32 index lists
    return dict(nb=nb, nbb=nbb, plain=plain, staged=staged)


def form_of(t, n):
    """(B, MAXT, STAGE) of the kernel sm_solve launches for a QP of n points, None where sm_generic_fits says no (the exact kernels)"""
    sh = sm_shape(t, n)
    lay = layout(sh["nv"], sh["nc"], sh["bw"])
    threads = 64 * ((lay["nbb"] + 63) // 64)
    if lay["plain"] * 8 > LDS_PER_CU or threads > 1024:
        return None
    stage = threads <= 512 and lay["staged"] * 8 <= LDS_PER_CU
    if threads <= 256 and stage:
        return (sh["bw"], 256, 1)
    if threads <= 512:
        return (sh["bw"], 512, 1 if stage else 0)
    return (sh["bw"], 1024, 0)


# ---- the case table -------------------------------------------------------------------------------------------------------------------
# type -> (first size, last size, form) of every reachable form; past the last range the core no longer holds the QP
RANGES = {
    S1: ((3, 64, (4, 256, 1)), (65, 128, (4, 512, 1)), (129, 203, (4, 1024, 0))),
    S2: ((4, 84, (9, 256, 1)), (85, 146, (9, 512, 1)), (147, 168, (9, 512, 0)), (169, 203, (9, 1024, 0))),
    S3: ((4, 85, (3, 256, 1)), (86, 169, (3, 512, 1)), (170, 170, (3, 512, 0)), (171, 251, (3, 1024, 0))),
}
CAPACITY = {t: r[-1][1] for t, r in RANGES.items()}        # 203 / 203 / 251
FORMS = sorted({f for r in RANGES.values() for _, _, f in r})
NEVER = ((4, 512, 0), (3, 256, 0), (4, 256, 0), (9, 256, 0))          # forms no size selects
# both edges of every range (the smallest size a type accepts is the first of them): (type, size, form)
CASES = [(t, n, f) for t in (S1, S2, S3) for a, b, f in RANGES[t] for n in sorted({a, b})]
CASE_BATCH = 3
CASE_SEEDS = (1, 2, 3)
# one ragged launch per form past 256 lanes, n_max inside the form's range: (type, n_max, form, counts) - counts from the type's smallest size
# across a wavefront's edge to n_max
RAGGED = [(t, n_max, f, (n_max, MIN_SIZE[t], 63, 64, 65, n_max - 1))
          for t, sizes in ((S1, (100, 180)), (S2, (120, 160, 190)), (S3, (130, 170, 220)))
          for n_max in sizes for f in [next(f for a, b, f in RANGES[t] if a <= n_max <= b)]]
RAGGED_SEED = 11


def case_id(c):
    t, n, f = c[0], c[1], c[2]
    return f"{NAME[t]}-{n}-B{f[0]}x{f[1]}{'s' if f[2] else 'g'}"


def form_name(f):
    return f"<{f[0]},{f[1]},{'true' if f[2] else 'false'}>"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def scenario(t, n, seed):
    """the input lists of one scenario: (x, y, angle, k, s, clearance) for S1 / S2, (s, lb, ub, l0) for S3"""
    return tension_inputs(n, seed=seed) if t != S3 else post_inputs(n, seed=seed)


def oracle_qp(t, sc):
    """the reference's assembly of a scenario at its own size: dense (P, q, A, lo, up)"""
    if t == S1:
        return O.assemble_tension2(sc[0], sc[1], sc[2], sc[3], sc[4])
    if t == S2:
        return O.assemble_tension(sc[0], sc[1], sc[2], sc[5])
    return O.assemble_post(sc[0], list(zip(sc[1], sc[2])), sc[3])


def case_batch(t, n, seeds=CASE_SEEDS):
    return [scenario(t, n, sd) for sd in seeds]


def ragged_batch(t, counts, seed=RAGGED_SEED):
    return [scenario(t, int(c), seed + b) for b, c in enumerate(counts)]


def device_arrays(t, scs, n_max=None, fill=np.nan):
    """the scenarios as the C ABI's [batch][n_max] lists, the padding filled with `fill` (never read)"""
    n_max = n_max or max(len(sc[0]) for sc in scs)
    keys = {S1: (0, 1, 2, 3, 4), S2: (0, 1, 2, 5), S3: (0, 1, 2)}[t]
    arrs = [np.stack([np.concatenate([sc[k], np.full(n_max - len(sc[k]), fill)]) for sc in scs]) for k in keys]
    if t == S3:
        arrs.append(np.array([sc[3] for sc in scs]))
    return arrs


def launch(h, t, arrs, counts=None):
    """the C ABI's call of a type (the _var entry point with counts); dict with out = [batch][n][1 or 2] (l, or x and y), s (S1, S2), status, iters"""
    if t == S1:
        r = h.smooth_tension2(*arrs) if counts is None else h.smooth_tension2_var(*arrs, counts)
    elif t == S2:
        r = h.smooth_tension(*arrs) if counts is None else h.smooth_tension_var(*arrs, counts)
    else:
        r = h.post_smooth(*arrs) if counts is None else h.post_smooth_var(*arrs, counts)
    out = r["l"][:, :, None] if t == S3 else np.stack([r["x"], r["y"]], axis=2)
    return dict(out=out, s=r.get("s"), status=r["status"], iters=r["iters"])


# ---- references -----------------------------------------------------------------------------------------------------------------------
_cache = {}


def cached(key, make):
    """A reference is computed once per process, shared by the tests that need it and not changed by them."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def oracle_settings(**over):
    kw = dict(eps_abs=1e-3, eps_rel=1e-3)
    kw.update(over)
    return O.OsqpSettings(**kw)


def oracle_run(t, n, seed, **over):
    """osqp_admm on the oracle's assembly of scenario (t, n, seed) at the handle's setting: dict(x: the QP's variables in the reference's order, out
    [n][1 or 2]: what the C ABI returns of them, iters, status)"""
    def make():
        P, q, A, lo, up = oracle_qp(t, scenario(t, n, seed))
        r = O.osqp_admm(sp.csc_matrix(P), q, A, lo, up, oracle_settings(**over))
        out = r["x"][:n, None] if t == S3 else np.stack([r["x"][:n], r["x"][n:2 * n]], axis=1)
        out.setflags(write=False)
        return dict(x=r["x"], out=out, iters=r["iters"], status=r["status"], pri=r["pri_res"], dua=r["dua_res"])
    return cached((t, n, seed, tuple(sorted(over.items()))), make)


def chord(x, y):
    return np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])


# ---- the banded arrays of the core, as the device's assemble kernels and sm_upload_structure lay them out -------------------------------
def var_pos(t, n):
    """the reference's variable order at n points -> the point-interleaved position (the same position in the pattern of any n_max >= n)"""
    pos = np.zeros(sm_shape(t, n)["nv"], dtype=np.int64)
    i = np.arange(n)
    if t == S1:
        pos[i] = 4 * i; pos[n + i] = 4 * i + 1; pos[2 * n + i] = 4 * i + 2; pos[3 * n + i[:-1]] = 4 * i[:-1] + 3
    else:
        pos[i] = 3 * i; pos[n + i] = 3 * i + 1; pos[2 * n + i] = 3 * i + 2
    return pos


def row_pos(t, n, n_pat):
    """the reference's row order at n points -> the row of the pattern of n_pat >= n points"""
    i = np.arange(n)
    if t == S1:
        return np.concatenate([i[:-1], (n_pat - 1) + i[:-1], 2 * (n_pat - 1) + i[:-1], [3 * (n_pat - 1), 3 * (n_pat - 1) + 1]])
    if t == S2:
        return np.concatenate([i, n_pat + i, 2 * n_pat + i])
    return np.concatenate([i, n_pat + i[:-1], 2 * n_pat - 1 + i[:-1]])


def structure(t, n):
    """sm_upload_structure: acol [nc][4], trow / tslot [nv][6] of the pattern of n points"""
    sh = sm_shape(t, n)
    acol = -np.ones((sh["nc"], R_MAX), dtype=np.int32)
    for i in range(n - 1 if t != S2 else n):
        if t == S1:
            acol[i, :3] = (4 * (i + 1), 4 * i, 4 * i + 2)
            acol[n - 1 + i, :3] = (4 * (i + 1) + 1, 4 * i + 1, 4 * i + 2)
            acol[2 * (n - 1) + i, :3] = (4 * (i + 1) + 2, 4 * i + 2, 4 * i + 3)
        elif t == S2:
            acol[i, :2] = (3 * i, 3 * i + 2); acol[n + i, :2] = (3 * i + 1, 3 * i + 2); acol[2 * n + i, 0] = 3 * i + 2
        else:
            acol[n + i, :3] = (3 * (i + 1), 3 * i, 3 * i + 1); acol[2 * n - 1 + i, :3] = (3 * (i + 1) + 1, 3 * i + 1, 3 * i + 2)
    if t == S1:
        acol[3 * (n - 1), 0] = 0; acol[3 * (n - 1) + 1, 0] = 1
    if t == S3:
        acol[np.arange(n), 0] = 3 * np.arange(n)
    trow = -np.ones((sh["nv"], C_MAX), dtype=np.int32); tslot = np.zeros((sh["nv"], C_MAX), dtype=np.int32)
    fill = np.zeros(sh["nv"], dtype=np.int64)
    for r in range(sh["nc"]):
        for s in range(R_MAX):
            c = acol[r, s]
            if c >= 0:
                assert fill[c] < C_MAX
                trow[c, fill[c]] = r; tslot[c, fill[c]] = s; fill[c] += 1
    return acol, trow, tslot


def banded(t, scs, n_pat=None):
    """The core's arguments for a batch of scenarios in the pattern of n_pat points (default: their own, equal, size) from the oracle's assembly of
    each at its own size: a shorter scenario is the same QP padded as the assemble kernels pad it - unit cost and no rows on the variables it
    lacks, zero rows with infinite bounds where its rows would be.  For banded_util.emu_solve."""
    n_pat = n_pat or len(scs[0][0])
    sh = sm_shape(t, n_pat)
    nv, nc, pbw = sh["nv"], sh["nc"], sh["pbw"]
    acol, trow, tslot = structure(t, n_pat)
    B = len(scs)
    pband = np.zeros((B, pbw + 1, nv)); qv = np.zeros((B, nv)); aval = np.zeros((B, nc, R_MAX)); lo = np.full((B, nc), -1e30); up = np.full((B, nc), 1e30)
    for b, sc in enumerate(scs):
        n = len(sc[0])
        P, q, A, l, u = oracle_qp(t, sc)
        vp, rp = var_pos(t, n), row_pos(t, n, n_pat)
        Pp = np.eye(nv); Pp[np.ix_(vp, vp)] = P                      # dummies: unit cost
        Ap = np.zeros((nc, nv)); Ap[np.ix_(rp, vp)] = A
        ii, jj = np.nonzero(Pp)
        assert np.abs(ii - jj).max() <= pbw
        for d in range(pbw + 1):
            pband[b, d, :nv - d] = Pp[np.arange(d, nv), np.arange(nv - d)]
        qv[b, vp] = q
        covered = np.zeros_like(Ap, dtype=bool)
        for s in range(R_MAX):
            ok = acol[:, s] >= 0
            aval[b, ok, s] = Ap[np.nonzero(ok)[0], acol[ok, s]]
            covered[np.nonzero(ok)[0], acol[ok, s]] = True
        assert not (Ap != 0)[~covered].any()                        # every entry of A lies in the pattern
        lo[b, rp] = l; up[b, rp] = u
    r = dict(batch=B, nv=nv, nc=nc, bw=sh["bw"], pbw=pbw, pband=pband, q=qv, acol=acol, aval=aval, trow=trow, tslot=tslot, lo=lo, up=up)
    if any(len(sc[0]) != n_pat for sc in scs):            # as sm_solve hands a ragged launch to the core
        r.update(n_of=np.array([len(sc[0]) for sc in scs], dtype=np.int32), ragged=(n_pat, ASSEMBLE_MIN[t], 4 if t == S1 else 3))
    return r


def emu_out(t, x, n):
    """the first n points of an interleaved solution as the C ABI returns them: [n][2] (x, y) or [n][1] (l)"""
    stride = 4 if t == S1 else 3
    return x[stride * np.arange(n)][:, None] if t == S3 else np.stack([x[stride * np.arange(n)], x[stride * np.arange(n) + 1]], axis=1)
