"""Solver-free answers about a path QP, for the tests of more than one solver: the KKT conditions at a returned path, and the optimum by
a direct solve on the active set.
(pytest does not rewrite the asserts of a helper module: each one here carries its own message.)"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pqp_oracle as O


def kkt_certificate_of_the_last_pass(ref, bounds, scal, first, final):
    """Solver-independent: the returned (l, psi, kappa, kappa') with the slacks and multipliers it implies satisfies the KKT conditions of
    the assembled QP of the LAST pass (oracle assembly around the first pass's optimum, reference numbering)."""
    n = ref.shape[0]
    Pd, A, lo, up, sz = O.assemble_path_qp(ref, first[:, 3:6], bounds, scal)
    o = final
    x = np.zeros(sz["vars"])
    x[0:3 * n:3] = o[:, 3]; x[1:3 * n:3] = o[:, 4]; x[2:3 * n:3] = o[:, 5]; x[3 * n:4 * n - 1] = o[:-1, 6]
    # slacks: what the collision rows need beyond their box
    A = sp.csr_matrix(A)
    rows = A @ x
    for i in range(n):
        for j in range(2):
            r_ = 4 * n + 2 * i + j
            x[4 * n - 1 + 2 * i + j] = np.clip(rows[r_], lo[r_], up[r_]) - rows[r_]
    ax = A @ x
    assert np.maximum(lo - ax, ax - up).max() < 1e-8, ("primal feasibility", np.maximum(lo - ax, ax - up).max())
    # multipliers: slack rows y = -w_s s; the rest from stationarity by least squares on the rows active at x
    g = Pd * x
    act = (np.abs(ax - lo) < 1e-7) | (np.abs(ax - up) < 1e-7)
    At = A[act].T.toarray()
    y_act, *_ = np.linalg.lstsq(At, -g, rcond=None)
    assert np.abs(At @ y_act + g).max() < 1e-6, ("stationarity", np.abs(At @ y_act + g).max())
    y = np.zeros(sz["cons"]); y[act] = y_act
    ineq = act & (up - lo > 1e-9)
    assert (y[ineq & (np.abs(ax - up) < 1e-7)] > -1e-6).all() and (y[ineq & (np.abs(ax - lo) < 1e-7)] < 1e-6).all(), "dual signs"


def direct_active_set_solve(Pd, A, lo, up, x_hint, y_hint, tol=1e-7):
    """A solver-free answer for a path QP: identify the active set from a (converged) primal-dual pair, then solve the
    equality-constrained QP on that set DIRECTLY - one sparse LU of the KKT matrix [[P, A_act'], [A_act, 0]] (scipy splu), no ADMM,
    no iteration - and check that the point it gives is the optimum: inactive rows strictly inside their boxes, multipliers of the
    active rows correctly signed.  Returns (x, y, worst_kkt_violation)."""
    ax = A @ x_hint
    at_lo = (np.abs(ax - lo) <= tol * (1 + np.abs(lo))) & (lo > -1e19)
    at_up = (np.abs(ax - up) <= tol * (1 + np.abs(up))) & (up < 1e19)
    eq = (up - lo) <= 1e-12
    act = eq | (at_lo & (y_hint < -1e-9)) | (at_up & (y_hint > 1e-9))
    b = np.where(eq | (at_lo & ~at_up), lo, up)[act]
    Aa = sp.csr_matrix(A[act])
    nv, na = A.shape[1], int(act.sum())
    K = sp.bmat([[sp.diags(Pd), Aa.T], [Aa, None]], format="csc")
    sol = spla.splu(K).solve(np.r_[np.zeros(nv), b])
    x, lam = sol[:nv], sol[nv:]
    y = np.zeros(A.shape[0]); y[act] = lam
    ax = A @ x
    viol = max(float(np.max(np.maximum(lo - ax, ax - up))), 0.0)                       # primal feasibility of every row
    sign = max(float(np.max(np.where(act & ~eq & at_lo & ~at_up, y, 0.0))), float(np.max(np.where(act & ~eq & at_up & ~at_lo, -y, 0.0))), 0.0)
    stat = float(np.abs(Pd * x + A.T @ y).max())
    return x, y, max(viol, sign, stat)
