"""The assemble kernel and both path-QP kernels under car and cost parameters away from the defaults (tests/param_cases.py; the host emulations of the same
sources: tests/test_path_params_cpu.py): the four cost weights, the car's three lengths, getSoftBounds' two numbers, the four numbers of the end rows and
constraint_end_heading, through the C ABI, against the oracle's QP from the same parameters - HiGHS on four QPs per case, the converged C oracle on sixteen.

Every bound is one the suite already has: tests/highs_util.py's, the 1e-13 / 1e-12 of test_gpu_parity.py::test_assemble_matches_oracle, the 50 iterations of
::test_iteration_counts_follow_the_osqp_restatement, and tests/test_gpu_stream.py's against the converged oracle (2e-5; 1e-4 with a median of 1e-6 beyond
96 waypoints) and between the kernels (2e-5, median 1e-7) - or param_cases.L_TOL / L_TOL_BATCH, measured on the oracle alone.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import pqp_oracle as O
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import highs_qp as H
import param_cases as PC

pytestmark = pytest.mark.gpu

KERNELS = ["lane_per_waypoint", "lane_per_qp"]
BATCH = 64
SHAPES = [(case, 60) for case in PC.NAMES] + [("all", 9), ("all", 130)]      # 130: two wavefronts per QP, the kernels with polish_final_refine compiled in


def _handle(kernel, prm, batch, n, store_warm=None):
    from path_optimizer_2_amd import capi
    h = capi.Handle(prm, device=0, max_batch=batch, max_n=n)
    if kernel == "lane_per_qp":
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_STREAM_BATCH, 1)
    else:
        h.set_option(capi.OPT_STREAM_BATCH, 0)
        if store_warm is not None:
            h.set_option(capi.OPT_STORE_WARM, store_warm)
    return h


def _served_by(h, kernel):
    from path_optimizer_2_amd import capi
    return h.last_path_kernel() == (capi.KERNEL_LANE_PER_QP if kernel == "lane_per_qp" else capi.KERNEL_LANE_PER_WAYPOINT)


@functools.lru_cache(maxsize=None)
def _solved(kernel, case, n):
    """BaseSolver::solve alone and the whole of optimizePath, 64 QPs, on a fresh handle created with the case: solved once, read by several tests"""
    from path_optimizer_2_amd import capi
    b = PC.batch(BATCH, n)
    h = _handle(kernel, capi.production_params(**PC.CASES[case]), BATCH, n)
    r0 = h.solve(b["ref"], b["bounds"], b["scal"], passes=0)
    r1 = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    served = _served_by(h, kernel)
    h.close()
    return r0, r1, served


def _against_the_converged_oracle(out, case, n, passes=1, count=16):
    want = PC.converged_oracle(case, count, n, passes)
    err = np.abs(out[:count, :, 3:5] - want[:, :, 3:5]).max(axis=(1, 2))
    print(f"{case} n={n} passes={passes}: |l, d_heading - converged oracle| max {err.max():.2e} median {np.median(err):.2e}")
    assert err.max() < (2e-5 if n <= 96 else 1e-4) and np.median(err) < 1e-6, (err.max(), np.median(err))


@pytest.mark.parametrize("n", [3, 80])
@pytest.mark.parametrize("case", PC.NAMES)
def test_assemble_under_the_cases(hip_lib, case, n):
    from path_optimizer_2_amd import capi
    b = PC.batch(6, n)
    prm = PC.oracle_params(case)
    lin = np.stack([O.first_linearization(b["ref"][q]) for q in range(6)])
    lin[3:] += np.random.default_rng(n).normal(scale=[0.3, 0.05, 0.01], size=(3, n, 3))      # a non-trivial linearisation point
    h = capi.Handle(capi.default_params(**PC.CASES[case]), device=0, max_batch=6, max_n=n)
    rows, colptr, pcols = h.pattern(n)
    orows, _, ocolptr, opcols = O.structural_pattern(n, n, with_l=prm.weight_l != 0.0)      # (P has its l columns once weight_l is not an exact zero)
    assert np.array_equal(rows, orows) and np.array_equal(colptr, ocolptr) and np.array_equal(pcols, opcols)
    assert h.sizes(n)["nnz_p"] == len(pcols) == (5 * n - 1 if prm.weight_l else 4 * n - 1)
    for lin_arg in (None, lin):
        a_val, p_val, lo, up = h.assemble(b["ref"], lin_arg, b["bounds"], b["scal"])
        for q in range(6):
            Pd, A, olo, oup, sz = O.assemble_path_qp(b["ref"][q], lin[q] if lin_arg is not None else O.first_linearization(b["ref"][q]), b["bounds"][q], b["scal"][q], prm)
            Ag = sp.csc_matrix((a_val[q], rows, colptr), shape=(sz["cons"], sz["vars"])).toarray()
            np.testing.assert_allclose(Ag, A, rtol=1e-13, atol=1e-15)
            Pg = np.zeros(sz["vars"]); Pg[pcols] = p_val[q]
            np.testing.assert_array_equal(Pg, Pd)
            np.testing.assert_allclose(lo[q], olo, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(up[q], oup, rtol=1e-12, atol=1e-15)
    h.close()


def test_assemble_under_all_in_rough_constraints_mode(hip_lib):
    """beyond precise_planning_length one row per waypoint on the centre circle's box: getSoftBounds with the case's margin and min_clearance there too"""
    from path_optimizer_2_amd import capi
    n = 60
    b = {k: v.copy() for k, v in PC.batch(4, n).items()}
    b["bounds"][:, :, 4] -= 0.15; b["bounds"][:, :, 5] += 0.1               # a centre box of its own
    prm = PC.oracle_params("all", rough_constraints_far_away=True, precise_planning_length=10.0)
    h = capi.Handle(capi.default_params(rough_constraints_far_away=1, precise_planning_length=10.0, **PC.CASES["all"]), device=0, max_batch=4, max_n=n)
    for q in range(4):          # (the arclengths differ from QP to QP in this profile, and one call shares `precise`)
        one = {k: np.ascontiguousarray(v[q:q + 1]) for k, v in b.items()}
        precise = h.sizes(n, one["ref"][0, :, 0].copy())["precise"]
        assert 0 < precise < n and precise == O.path_qp_sizes(n, one["ref"][0, :, 0], prm)["precise"]
        a_val, p_val, lo, up = h.assemble(one["ref"], None, one["bounds"], one["scal"], precise=precise)
        rows, colptr, pcols = h.pattern(n, precise)
        Pd, A, olo, oup, sz = O.assemble_path_qp(one["ref"][0], O.first_linearization(one["ref"][0]), one["bounds"][0], one["scal"][0], prm)
        np.testing.assert_allclose(sp.csc_matrix((a_val[0], rows, colptr), shape=A.shape).toarray(), A, rtol=1e-13, atol=1e-15)
        Pg = np.zeros(sz["vars"]); Pg[pcols] = p_val[0]
        np.testing.assert_array_equal(Pg, Pd)
        np.testing.assert_allclose(lo[0], olo, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(up[0], oup, rtol=1e-12, atol=1e-15)
    h.close()


@pytest.mark.skipif(not H.available(), reason="this scipy does not bundle the HiGHS QP interface")
@pytest.mark.parametrize("case,n", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_both_passes_of_both_kernels_under_the_cases(hip_lib, kernel, case, n):
    from highs_util import against_highs
    b = PC.batch(BATCH, n)
    r0, r1, served = _solved(kernel, case, n)
    assert served
    assert (r0["status"] == 1).all() and (r1["status"] == 1).all()
    _against_the_converged_oracle(r0["out"], case, n, passes=0)
    _against_the_converged_oracle(r1["out"], case, n, passes=1)
    if n > 60:          # (HiGHS is slow beyond)
        return
    prm = PC.oracle_params(case)
    for q in range(4):
        ref, bounds, scal = b["ref"][q], b["bounds"][q], b["scal"][q]
        against_highs(ref, None, bounds, scal, r0["out"][q], one_sided=True, l_tol=PC.l_tol(case), highs=PC.highs_first_pass(case, n, q))
        against_highs(ref, r0["out"][q][:, 3:6], bounds, scal, r1["out"][q], prm, one_sided=True, l_tol=PC.l_tol(case))


@pytest.mark.parametrize("case,n", SHAPES)
def test_the_two_kernels_agree_under_the_cases(hip_lib, case, n):
    ra, rb = _solved("lane_per_waypoint", case, n)[1], _solved("lane_per_qp", case, n)[1]
    assert (ra["status"] == 1).all() and (rb["status"] == 1).all()
    d = np.abs(ra["out"][:, :, 3:5] - rb["out"][:, :, 3:5]).max(axis=(1, 2))
    dl = np.abs(ra["out"][:, :, 3] - rb["out"][:, :, 3]).max()
    print(f"{case} n={n}: between the kernels |l, d_heading| max {d.max():.2e} median {np.median(d):.2e}, |l| max {dl:.2e}")
    assert d.max() < 2e-5 and np.median(d) < 1e-7, (d.max(), np.median(d))
    if case in PC.L_TOL_BATCH and n == 60:          # weight_l > 0: no flat direction (the bound was measured on these 64 QPs)
        assert dl < PC.L_TOL_BATCH[case], dl


@pytest.mark.parametrize("case", ["weights", "car"])
def test_iteration_counts_follow_the_osqp_restatement_under_the_cases(hip_lib, case):
    """The reference's OSQP setting (eps 2e-3, no polish, 10 Ruiz passes) on the lane-per-waypoint kernel: it stops at the same check as the restatement - where
    an equilibration or a rho that silently assumed the default cost or car would show."""
    from path_optimizer_2_amd import capi
    n = 60
    b = PC.batch(8, n)
    h = _handle("lane_per_waypoint", capi.default_params(**PC.CASES[case]), 8, n)
    r = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    assert _served_by(h, "lane_per_waypoint")
    h.close()
    for q in range(8):
        ref = O.solve_path(b["ref"][q], b["bounds"][q], b["scal"][q], prm=PC.oracle_params(case), st=O.OsqpSettings())
        print(f"{case} QP {q}: {int(r['iters'][q])} iterations, the restatement {[x['iters'] for x in ref]} {[x['status'] for x in ref]}")
        assert (r["status"][q] == 1) == all(x["status"] == "solved" for x in ref)
        assert abs(int(r["iters"][q]) - sum(x["iters"] for x in ref)) <= 50


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_curvature_box_follows_wheel_base(hip_lib, kernel):
    """tan(steer) / wheel_base at wheel_base = 2.9 (the box is 14 % narrower than at 2.5): a start curvature just inside it, one outside by less than OSQP's
    primal tolerance eps_abs + eps_rel * bound - projected onto the box (include/pqp.h) -, one outside by more - PRIMAL_INFEASIBLE.  All three lie inside the
    default car's box; their neighbours are not touched."""
    from path_optimizer_2_amd import capi
    prm = capi.production_params(wheel_base=PC.WHEEL_BASE)
    b, kap = PC.curvature_box_batch(prm)
    plain = PC.batch(len(kap), b["ref"].shape[1])
    h = _handle(kernel, prm, len(kap), b["ref"].shape[1])
    r = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    rp = h.solve(plain["ref"], plain["bounds"], plain["scal"], passes=1)
    assert _served_by(h, kernel)
    h.close()
    PC.check_curvature_box(b, kap, r, rp)


@pytest.mark.parametrize("case", ["weights", "car", "all"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_set_params_on_a_live_handle(hip_lib, kernel, case):
    """pqp_set_params between two solves of one batch: the second solve is the one of a fresh handle created with those parameters, bit for bit; what the
    handle kept from the first - warm state, cost keys, the previous cycle's optima - belongs to QPs of other parameters and must not show in a result."""
    from path_optimizer_2_amd import capi
    n = 60
    b = PC.batch(BATCH, n)
    fresh = _solved(kernel, case, n)[1]
    h = _handle(kernel, capi.production_params(), BATCH, n)
    first = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    assert (first["status"] == 1).all() and not np.array_equal(first["out"], fresh["out"])
    h.set_params(capi.production_params(**PC.CASES[case]))
    live = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    assert _served_by(h, kernel)
    h.close()
    assert np.array_equal(live["status"], fresh["status"]) and np.array_equal(live["out"], fresh["out"]) and np.array_equal(live["iters"], fresh["iters"])
    if kernel == "lane_per_waypoint":
        # warm == 1 without `lin`: from the iterate, equilibration and active set the handle kept - those of the default parameters' QPs
        h = _handle(kernel, capi.production_params(), BATCH, n, store_warm=1)
        h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
        h.set_params(capi.production_params(**PC.CASES[case]))
        warm = h.solve(b["ref"], b["bounds"], b["scal"], passes=1, warm=True)
        assert _served_by(h, kernel)
        h.close()
        assert (warm["status"] == 1).all()
        _against_the_converged_oracle(warm["out"], case, n)
    # a planner's handle: PQP_OPT_CARRY_CYCLES and PQP_OPT_ORDER_BY_COST (iteration counts are not pinned: the starts are poor ones)
    h = _handle(kernel, capi.production_params(), BATCH, n, store_warm=0)
    h.set_option(capi.OPT_CARRY_CYCLES, 1); h.set_option(capi.OPT_ORDER_BY_COST, 1)
    h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
    h.set_params(capi.production_params(**PC.CASES[case]))
    for cycle in range(2):
        carried = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
        assert _served_by(h, kernel) and (carried["status"] == 1).all(), cycle
        _against_the_converged_oracle(carried["out"], case, n)
    h.close()


def test_car_flags_through_the_drop_in(hip_lib):
    """BaseSolver::setParams with the `car` case (the reference reads these from gflags): solve() + updateProblemFormulationAndSolve() give what the same two
    calls of the C ABI give with the same pqp_params."""
    from path_optimizer_2_amd import capi
    import cpp_demo
    exe = cpp_demo.build("shim_demo", hip=False, extra=[cpp_demo.SHIM])
    n = 60
    b = PC.batch(4, n)
    car = PC.CASES["car"]
    r = subprocess.run([exe] + ["%s=%r" % kv for kv in car.items()], input=cpp_demo.shim_scenario_text(b, 0), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([[float(v) for v in ln.split()] for ln in r.stdout.strip().splitlines()])
    one = {k: np.ascontiguousarray(v[:1]) for k, v in b.items()}
    h = capi.Handle(capi.default_params(**car), device=0, max_batch=1, max_n=n)
    r0 = h.solve(one["ref"], one["bounds"], one["scal"], lin=O.first_linearization(one["ref"][0])[None], passes=0)
    r1 = h.solve(one["ref"], one["bounds"], one["scal"], lin=np.ascontiguousarray(r0["out"][:, :, 3:6]), passes=0, warm=True)
    h.close()
    assert r0["status"][0] == 1 and r1["status"][0] == 1
    assert np.array_equal(got, r1["out"][0])
    plain = capi.Handle(capi.default_params(), device=0, max_batch=1, max_n=n)
    rd = plain.solve(one["ref"], one["bounds"], one["scal"], passes=1)
    plain.close()
    assert np.abs(rd["out"][0] - got)[:, 3].max() > 1e-3          # (and the flags matter on this scenario)
