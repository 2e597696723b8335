"""The smoothers' generic banded ADMM core on the device, form by form (banded_cases.py): banded_solve_kernel<B, MAXT, STAGE> with B = 4 / 9 / 3
(S1 TensionSmoother2, S2 TensionSmoother, S3 postSmooth), 256 / 512 / 1024 lanes, the row data staged in LDS or read from global memory - what a
handle in the reference's own setting (OSQP defaults, eps 1e-3, polish = 0) runs.  Everything goes through the C ABI: assemble kernel, core,
finish kernel.  The reference is oracle/pqp_oracle.py's assembly of each scenario at its own size run by its osqp_admm at the same setting: the
same iteration, so the device stops at the same check (`iters` equal, and > 0: the core ran, not an exact kernel) and returns the same iterate
to round-off - bar 1e-6, the project's bar for this comparison (test_gpu_smoothers.test_tension2).
Measured on an MI355X, worst |x - x_oracle| per form over the cases, the ragged launches and scaling = 0:
  <4,256,true> 6.4e-11   <4,512,true> 2.2e-10                           <4,1024,false> 3.3e-10      (S1)
  <9,256,true> 7.3e-9    <9,512,true> 5.5e-9    <9,512,false> 2.5e-8    <9,1024,false> 1.5e-8       (S2)
  <3,256,true> 4.5e-13   <3,512,true> 5.0e-13   <3,512,false> 5.0e-13   <3,1024,false> 1.4e-12      (S3)
every count equal to the oracle's.  Observed capacities: the core iterates at 203 / 203 / 251 points and hands over to the exact kernels at 204 /
204 / 252.  Converged (eps 1e-9): S1 at 203 points 2.9e-10 from its KKT solution, S3 KKT violation 6.5e-10 at 170 layers, 4.8e-9 at 251."""
import numpy as np
import pytest

import banded_cases as K
import pqp_oracle as O
from path_optimizer_2_amd import capi
from smoother_cases import post_reduced_kkt

pytestmark = pytest.mark.gpu
STATUS_OF = {"solved": 1, "max_iter": 2, "primal_infeasible": 4}      # the oracle's verdicts as pqp_status


def _plain(**over):
    return capi.default_params(eps_abs=1e-3, eps_rel=1e-3, **over)


def _polished():
    return capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25)


def _run(prm, t, scs, n_max=None, counts=None):
    n_max = n_max or len(scs[0][0])
    h = capi.Handle(prm, max_batch=len(scs), max_n=n_max)
    r = K.launch(h, t, K.device_arrays(t, scs, n_max), None if counts is None else np.asarray(counts, dtype=np.int32))
    h.close()
    return r


_worst = {}


def _check_against_oracle(t, r, sizes, seeds, form, tag, **oracle_over):
    """status, iters > 0 (the generic core ran), iters and iterate equal to the oracle's, s = the chord lengths of the returned points"""
    assert (r["status"] == 1).all(), (tag, r["status"])
    assert (r["iters"] > 0).all(), (tag, r["iters"])
    for q, (n, sd) in enumerate(zip(sizes, seeds)):
        o = K.oracle_run(t, n, sd, **oracle_over)
        gap = np.abs(r["out"][q, :n] - o["out"]).max()
        _worst[form] = max(_worst.get(form, 0.0), gap)
        print(f"{tag} scenario {q} ({n} points): iters {r['iters'][q]} / oracle {o['iters']} (its residuals there: {o['pri']:.3e}, {o['dua']:.3e}), |x - x_oracle| {gap:.2e}")
        assert o["status"] == "solved" and r["iters"][q] == o["iters"], (tag, q, r["iters"][q], o["iters"])
        assert gap < K.X_BAR, (tag, q, gap)
        if t != K.S3:
            assert np.abs(r["s"][q, :n] - K.chord(r["out"][q, :n, 0], r["out"][q, :n, 1])).max() <= 1e-12, (tag, q)
    print("worst |x - x_oracle| per form so far:", {K.form_name(f): f"{v:.2e}" for f, v in sorted(_worst.items())})


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_every_form_follows_the_oracle_at_both_edges_of_its_range(hip_lib, case):
    """three scenarios per launch (the per-QP offsets into pband, q, aval, lo, up) at the first and the last size of every kernel form"""
    t, n, form = case
    r = _run(_plain(), t, K.case_batch(t, n))
    _check_against_oracle(t, r, [n] * K.CASE_BATCH, K.CASE_SEEDS, form, K.case_id(case))


@pytest.mark.parametrize("t", [K.S1, K.S2, K.S3], ids=[K.NAME[t] for t in (K.S1, K.S2, K.S3)])
def test_capacity_boundary(hip_lib, t):
    """The last size the core holds (203 / 203 / 251 points: BqLayout::total(false) in one CU's 160 KB) iterates; one point more and the handle
    gets the exact kernel's result - iters = 0, the bits a handle that asks for exact optima gets."""
    n = K.CAPACITY[t]
    assert K.form_of(t, n) is not None and K.form_of(t, n + 1) is None
    r = _run(_plain(), t, K.case_batch(t, n))
    assert (r["status"] == 1).all() and (r["iters"] > 0).all(), r["iters"]
    scs = K.case_batch(t, n + 1)
    r, want = _run(_plain(), t, scs), _run(_polished(), t, scs)
    assert (r["status"] == 1).all() and (r["iters"] == 0).all(), r["iters"]
    assert (want["status"] == 1).all() and (want["iters"] == 0).all()
    assert np.array_equal(r["out"], want["out"])
    if t != K.S3:
        assert np.array_equal(r["s"], want["s"])


@pytest.mark.parametrize("rag", K.RAGGED, ids=K.case_id)
def test_ragged_launches(hip_lib, rag):
    """The _var entry points on a plain handle: a point count per scenario in the pattern of n_max (the assemble kernels' n_of / m_of branch, their
    decoupled dummies, tension_finish_kernel's repeated tail), the padding NaN.  Every scenario follows the oracle's run at its own size - the
    dummies touch nothing of the QP: the cost scaling's mean column norm runs over its own columns - and its launch alone at its own size."""
    t, n_max, form, counts = rag
    scs = K.ragged_batch(t, counts)
    r = _run(_plain(), t, scs, n_max, counts)
    _check_against_oracle(t, r, counts, [K.RAGGED_SEED + q for q in range(len(counts))], form, "ragged " + K.case_id(rag))
    for q, c in enumerate(counts):
        if t == K.S3:
            assert np.all(r["out"][q, c:] == 0.0), q
        else:
            assert np.all(r["out"][q, c:] == r["out"][q, c - 1]) and np.all(r["s"][q, c:] == r["s"][q, c - 1]), q
    q = counts.index(65)
    one = _run(_plain(), t, [scs[q]])
    assert one["status"][0] == 1 and one["iters"][0] == r["iters"][q]
    assert np.abs(one["out"][0] - r["out"][q, :65]).max() < 1e-6


@pytest.mark.parametrize("t,n", [(K.S1, 203), (K.S3, 170), (K.S3, 251)])
def test_converged_on_the_forms_that_read_global_memory(hip_lib, t, n):
    """eps 1e-9 on the non-staged 512-lane form (S3 has one size of it) and the 1024-lane forms: S1 against the solution of its KKT system (every row
    is an equality) at 1e-7, S3 by the KKT conditions of the oracle's matrices at 5e-7 (the host emulation: 2.9e-10 and 4.8e-9 at the largest
    sizes).  S2 is left out on purpose: its P is singular along flat directions, and its converged point and a polished one were 1.8e-3 apart at
    168 points on the emulation with both certificates below 1e-6 - no bar of this kind separates a right kernel from a wrong one there."""
    assert K.form_of(t, n)[2] == 0
    scs = K.case_batch(t, n)
    r = _run(capi.default_params(eps_abs=1e-9, eps_rel=1e-9, max_iter=200000, adaptive_rho_interval=25), t, scs)
    assert (r["status"] == 1).all() and (r["iters"] > 0).all()
    for q, sc in enumerate(scs):
        if t == K.S1:
            P, qv, A, lo, up = K.oracle_qp(t, sc)
            assert (lo == up).all()
            sol = np.linalg.solve(np.block([[P, A.T], [A, np.zeros((A.shape[0], A.shape[0]))]]), np.r_[-qv, lo])
            gap = np.abs(r["out"][q] - np.stack([sol[:n], sol[n:2 * n]], axis=1)).max()
            print(f"{K.NAME[t]} {n} scenario {q}: iters {r['iters'][q]}, |x - x_kkt| {gap:.2e}")
            assert gap < 1e-7, (q, gap)
        else:
            viol = post_reduced_kkt(sc[0], sc[1], sc[2], sc[3], r["out"][q, :, 0])
            print(f"{K.NAME[t]} {n} scenario {q}: iters {r['iters'][q]}, KKT violation {viol:.2e}")
            assert viol < 5e-7, (q, viol)


@pytest.mark.parametrize("t,n", [(K.S2, 85), (K.S3, 170)])
def test_polish_2_is_the_plain_run_on_qps_with_inequality_rows(hip_lib, t, n):
    """polish = 2 sends S1 (equality rows only) to its exact kernel and leaves S2 / S3 on the core's plain ADMM: the plain handle's bits and count"""
    scs = K.case_batch(t, n)
    r0, r2 = _run(_plain(), t, scs), _run(_plain(polish=2), t, scs)
    assert (r0["status"] == 1).all() and (r0["iters"] > 0).all()
    assert np.array_equal(r0["iters"], r2["iters"]) and np.array_equal(r0["status"], r2["status"]) and np.array_equal(r0["out"], r2["out"])
    if t != K.S3:
        assert np.array_equal(r0["s"], r2["s"])


@pytest.mark.parametrize("t,n", [(K.S1, 129), (K.S2, 147), (K.S3, 86)])
def test_without_equilibration(hip_lib, t, n):
    """scaling = 0 (the branch of run() that skips ruiz()) against the oracle with scaling = 0"""
    r = _run(_plain(scaling=0), t, K.case_batch(t, n))
    _check_against_oracle(t, r, [n] * K.CASE_BATCH, K.CASE_SEEDS, K.form_of(t, n), f"scaling 0 {K.NAME[t]}-{n}", scaling=0)


def test_an_inverted_box_ends_as_the_oracle_says_and_leaves_its_neighbours_alone(hip_lib):
    """one S3 scenario of three with lb > ub at a layer, on the plain handle: the oracle's verdict at the oracle's iteration and its iterate, the two
    other scenarios of the launch bit for bit what the clean launch returns.  (That verdict is "solved": the iteration's projection
    min(max(v, l), u) lands on u where l > u, so the layer is pinned to its upper bound, in the oracle and in the core alike.  OSQP itself refuses
    l > u at setup; the exact kernel of polish = 1 handles reports PRIMAL_INFEASIBLE: test_gpu_smoothers.test_post_smooth_exact_kernel.)"""
    import scipy.sparse as sp
    t, n = K.S3, 86
    scs = K.case_batch(t, n)
    clean = _run(_plain(), t, scs)
    s, lb, ub, l0 = scs[1]
    lb = lb.copy(); lb[40] = ub[40] + 0.1
    bad = [scs[0], (s, lb, ub, l0), scs[2]]
    r = _run(_plain(), t, bad)
    P, q, A, lo, up = K.oracle_qp(t, bad[1])
    o = O.osqp_admm(sp.csc_matrix(P), q, A, lo, up, K.oracle_settings())
    print(f"inverted box: status {r['status'][1]} after {r['iters'][1]} iterations, oracle {o['status']} after {o['iters']}")
    assert r["status"][1] == STATUS_OF[o["status"]] and r["iters"][1] == o["iters"] > 0
    assert np.abs(r["out"][1, :, 0] - o["x"][:n]).max() < K.X_BAR
    for q in (0, 2):
        assert r["status"][q] == 1 and r["iters"][q] == clean["iters"][q] and np.array_equal(r["out"][q], clean["out"][q])
