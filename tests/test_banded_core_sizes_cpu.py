"""The size matrix of the smoothers' generic banded core (banded_cases.py) without a GPU: the restated form selection against the header's own
layout, and the host emulation of pqp_banded_qp.hpp - in the staged or non-staged form the device would pick for the size - against the oracle's
osqp_admm at the reference's setting (eps 1e-3, no polish).  The two are the same iteration: they stop at the same check and agree to
round-off.  Measured here (worst |x - x_oracle| over the cases and the ragged launches): S1 3.2e-10, S2 3.8e-8, S3 1.1e-12."""
import ctypes as C

import numpy as np
import pytest

import banded_cases as K
import banded_util as BU
import emu_util as E


def _plain(**over):
    return E.params(eps_abs=1e-3, eps_rel=1e-3, **over)


def test_restated_layout_is_the_header_s():
    lib = E.load()
    out = np.zeros(3, dtype=np.int32)
    for t in (K.S1, K.S2, K.S3):
        for n in range(K.MIN_SIZE[t], 261):
            sh = K.sm_shape(t, n)
            lay = K.layout(sh["nv"], sh["nc"], sh["bw"])
            lib.pqp_emu_banded_layout(sh["nv"], sh["nc"], sh["bw"], out.ctypes.data_as(C.c_void_p))
            assert tuple(out) == (lay["nbb"], lay["plain"], lay["staged"]), (t, n)


def test_table_of_forms_is_what_the_selection_gives():
    """every size 3..260: the form RANGES names, none past the capacity; every reachable form has a case, the unreachable ones no size"""
    seen = set()
    for t in (K.S1, K.S2, K.S3):
        for n in range(K.MIN_SIZE[t], 261):
            want = next((f for a, b, f in K.RANGES[t] if a <= n <= b), None)
            assert K.form_of(t, n) == want, (t, n)
            assert (want is None) == (n > K.CAPACITY[t])
            seen.add(want)
    seen.discard(None)
    assert seen == set(K.FORMS) and len(K.FORMS) == 11
    assert {f for _, _, f in K.CASES} == seen
    assert not seen & set(K.NEVER)
    for t, n, f in K.CASES:
        assert K.form_of(t, n) == f
    for t, n_max, f, counts in K.RAGGED:
        assert K.form_of(t, n_max) == f and f[1] > 256 and min(counts) == K.MIN_SIZE[t] and {63, 64, 65, n_max - 1, n_max} <= set(counts)
    assert {f for _, _, f, _ in K.RAGGED} == {f for f in K.FORMS if f[1] > 256}


_worst = {}


def _against_oracle(t, b, sizes, seeds, form, tag):
    """the emulation of a batch in the device's form against the oracle's run of every scenario at its own size; the other form returns the same bits"""
    r = BU.emu_solve(_plain(), b, stage=bool(form[2]))
    other = BU.emu_solve(_plain(), b, stage=not form[2])
    for k in ("x", "y", "status", "iters"):
        assert np.array_equal(r[k], other[k]), (tag, k)
    for q, (n, sd) in enumerate(zip(sizes, seeds)):
        o = K.oracle_run(t, n, sd)
        assert o["status"] == "solved" and r["status"][q] == 1, (tag, q)
        gap = np.abs(K.emu_out(t, r["x"][q], n) - o["out"]).max()
        _worst[t] = max(_worst.get(t, 0.0), gap)
        print(f"{tag} scenario {q} ({n}): iters {r['iters'][q]} / oracle {o['iters']}, |x - x_oracle| {gap:.2e}")
        assert r["iters"][q] > 0 and r["iters"][q] == o["iters"], (tag, q)
        assert gap < K.X_BAR, (tag, q, gap)
    print("worst gap per type so far:", {K.NAME[k]: f"{v:.2e}" for k, v in _worst.items()})


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_emulation_follows_the_oracle_at_every_edge(case):
    t, n, form = case
    _against_oracle(t, K.banded(t, K.case_batch(t, n)), [n] * K.CASE_BATCH, K.CASE_SEEDS, form, K.case_id(case))


@pytest.mark.parametrize("rag", K.RAGGED, ids=K.case_id)
def test_emulation_of_a_ragged_launch_follows_the_oracle_at_each_size(rag):
    """the banded arrays of every scenario padded to the pattern of n_max as the assemble kernels pad them (unit-cost dummies, zero rows with
    infinite bounds), the oracle on the scenario alone.  The dummies are decoupled from the QP but for the mean column norm of the cost
    scaling, which the core therefore takes over the QP's own columns: with the dummies in it the 3-point line of S1 ended 2.1e-4 from
    the oracle's iterate in the patterns of 100 and 180 points (2.4e-14 now)."""
    t, n_max, form, counts = rag
    b = K.banded(t, K.ragged_batch(t, counts), n_max)
    assert b["n_of"].tolist() == list(counts)
    _against_oracle(t, b, counts, [K.RAGGED_SEED + q for q in range(len(counts))], form, "ragged " + K.case_id(rag))


@pytest.mark.parametrize("t,n", [(K.S2, 147), (K.S3, 170)])
def test_polish_2_is_the_plain_run_on_qps_with_inequality_rows(t, n):
    """polish = 2 solves an equality-only QP directly and leaves every other one to the plain ADMM: the same bits and count"""
    b = K.banded(t, K.case_batch(t, n))
    stage = bool(K.form_of(t, n)[2])
    r0, r2 = BU.emu_solve(_plain(), b, stage=stage), BU.emu_solve(_plain(polish=2), b, stage=stage)
    assert (r0["iters"] > 0).all() and np.array_equal(r0["iters"], r2["iters"]) and (r2["info"][:, 4] == 0).all()
    assert np.array_equal(r0["x"], r2["x"]) and np.array_equal(r0["y"], r2["y"])


@pytest.mark.parametrize("t,n", [(K.S1, 129), (K.S2, 147), (K.S3, 86)])
def test_emulation_without_equilibration(t, n):
    """scaling = 0 (the branch of run() that skips ruiz()) against the oracle with scaling = 0"""
    r = BU.emu_solve(_plain(scaling=0), K.banded(t, K.case_batch(t, n)), stage=bool(K.form_of(t, n)[2]))
    for q, sd in enumerate(K.CASE_SEEDS):
        o = K.oracle_run(t, n, sd, scaling=0)
        assert o["status"] == "solved" and r["status"][q] == 1 and r["iters"][q] == o["iters"] > 0
        assert np.abs(K.emu_out(t, r["x"][q], n) - o["out"]).max() < K.X_BAR


def test_emulation_of_an_inverted_box():
    """what test_gpu_banded_core's inverted-box test expects of the device: the oracle's verdict at the oracle's iteration, the neighbours untouched.
    (That verdict is "solved": the projection min(max(v, l), u) of the iteration lands on u where l > u, so the layer is pinned to its upper bound;
    the core does the same.  OSQP itself refuses l > u at setup, and the exact kernel of polish = 1 handles reports PRIMAL_INFEASIBLE.)"""
    import scipy.sparse as sp

    import pqp_oracle as O
    t, n = K.S3, 86
    scs = K.case_batch(t, n)
    clean = BU.emu_solve(_plain(), K.banded(t, scs), stage=True)
    s, lb, ub, l0 = scs[1]
    lb = lb.copy(); lb[40] = ub[40] + 0.1
    bad = [scs[0], (s, lb, ub, l0), scs[2]]
    r = BU.emu_solve(_plain(), K.banded(t, bad), stage=True)
    P, q, A, lo, up = K.oracle_qp(t, bad[1])
    o = O.osqp_admm(sp.csc_matrix(P), q, A, lo, up, K.oracle_settings())
    assert r["status"][1] == {"solved": 1, "max_iter": 2, "primal_infeasible": 4}[o["status"]] and r["iters"][1] == o["iters"]
    assert np.abs(K.emu_out(t, r["x"][1], n)[:, 0] - o["x"][:n]).max() < K.X_BAR
    for q in (0, 2):
        assert r["status"][q] == 1 and np.array_equal(r["x"][q], clean["x"][q])
