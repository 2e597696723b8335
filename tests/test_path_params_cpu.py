"""Both path solvers' device sources compiled for the host (tests/emu) under car and cost parameters away from the defaults (tests/param_cases.py): every
pqp_params field that decides which QP the path kernels build - the four cost weights, the car's three lengths, the two numbers of getSoftBounds, the four
of the end rows and constraint_end_heading - against HiGHS on the QP the oracle assembles from the same parameters.  What tests/test_gpu_path_params.py
repeats with the HIP kernels.
"""
import os
import sys

import numpy as np
import pytest

import pqp_oracle as O
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import highs_qp as H
import param_cases as PC

pytestmark = pytest.mark.skipif(not H.available(), reason="this scipy does not bundle the HiGHS QP interface (scipy.optimize._highspy._core)")


def _emulation(name, over):
    if name == "lane_per_qp":
        import lq_emu_util as E
        return lambda b, passes: E.solve(b["ref"], b["bounds"], b["scal"], passes=passes, prm=E.production(**over))
    import emu_util as EL
    return lambda b, passes: EL.solve(EL.production(**over), b["ref"], b["bounds"], b["scal"], passes=passes)


@pytest.mark.parametrize("n", [9, 60])
def test_the_cases_reach_what_they_are_meant_to(n):
    """tests/param_cases.py's claims about the first four QPs: getSoftBounds' three outcomes under `car`, the signed end-heading compare under `end`"""
    b = PC.batch(4, n)
    car = PC.oracle_params("car")
    kinds = set()
    for lb, ub in b["bounds"][:, :, 0:2].reshape(-1, 2):
        lo, up = O.soft_bounds(lb, ub, car.expected_safety_margin, car.min_clearance)
        kind = "untouched" if (lo, up) == (lb, ub) else "full" if np.isclose(lo - lb, car.expected_safety_margin) else "clipped"
        assert kind != "clipped" or (np.isclose(up - lo, car.min_clearance) and lo - lb < car.expected_safety_margin)
        kinds.add(kind)
    assert kinds == {"untouched", "full", "clipped"}
    end = PC.oracle_params("end")
    end_psi = np.array([O.constrain_angle(b["scal"][q, 3] - b["ref"][q, -1, 2]) for q in range(4)])
    held = end_psi < end.end_psi_max
    assert held.any() and not held.all() and (end_psi[held] < -end.end_psi_max).any()
    for q in range(4):
        _, _, lo, up, _ = O.assemble_path_qp(b["ref"][q], O.first_linearization(b["ref"][q]), b["bounds"][q], b["scal"][q], end)
        assert (up[-1] - lo[-1] == pytest.approx(2 * end.end_psi_tol)) == held[q] and (lo[-2], up[-2]) == (-end.end_l_bound, end.end_l_bound)


@pytest.mark.parametrize("n", [9, 60])
@pytest.mark.parametrize("case", PC.NAMES)
@pytest.mark.parametrize("emulation", ["lane_per_waypoint", "lane_per_qp"])
def test_both_passes_of_the_emulations_against_highs(emulation, case, n):
    from highs_util import against_highs
    b = PC.batch(4, n)
    run = _emulation(emulation, PC.CASES[case])
    r0, r1 = run(b, 0), run(b, 1)
    assert (r0["status"] == 1).all() and (r1["status"] == 1).all()
    prm = PC.oracle_params(case)
    for q in range(4):
        ref, bounds, scal = b["ref"][q], b["bounds"][q], b["scal"][q]
        against_highs(ref, None, bounds, scal, r0["out"][q], one_sided=True, l_tol=PC.l_tol(case), highs=PC.highs_first_pass(case, n, q))
        against_highs(ref, r0["out"][q][:, 3:6], bounds, scal, r1["out"][q], prm, one_sided=True, l_tol=PC.l_tol(case))


@pytest.mark.parametrize("case", PC.NAMES)
def test_the_converged_c_oracle_follows_the_cases(case):
    """oracle/pqp_oracle_c.py forwards every one of these fields: its converged solve is HiGHS's optimum of the case's QP - it is what the GPU tests compare
    more QPs and longer paths against"""
    from highs_util import against_highs
    b = PC.batch(4, 60)
    want = PC.converged_oracle(case, 4, 60, passes=0)
    for q in range(4):
        against_highs(b["ref"][q], None, b["bounds"][q], b["scal"][q], want[q], one_sided=True, l_tol=PC.l_tol(case), highs=PC.highs_first_pass(case, 60, q))


@pytest.mark.parametrize("n", [35, 130])
@pytest.mark.parametrize("emulation", ["lane_per_waypoint", "lane_per_qp"])
def test_more_qps_and_longer_paths_against_the_converged_oracle(emulation, n):
    """`all` on 16 QPs of 35 and 130 waypoints (HiGHS is slow beyond 60), both passes in one call, to the bound of tests/test_gpu_stream.py"""
    b = PC.batch(16, n)
    r = _emulation(emulation, PC.CASES["all"])(b, 1)
    assert (r["status"] == 1).all()
    want = PC.converged_oracle("all", 16, n)
    assert np.abs(r["out"][:, :, 3:5] - want[:, :, 3:5]).max() < 2e-5


@pytest.mark.parametrize("emulation", ["lane_per_waypoint", "lane_per_qp"])
def test_the_curvature_box_follows_wheel_base(emulation):
    """tan(steer) / wheel_base at wheel_base = 2.9: a start curvature just inside the box, one outside by less than OSQP's primal tolerance - projected -, one
    outside by more - PRIMAL_INFEASIBLE; all three inside the default car's box (tests/param_cases.py)"""
    import emu_util as EL
    b, kap = PC.curvature_box_batch(EL.production(wheel_base=PC.WHEEL_BASE))
    run = _emulation(emulation, dict(wheel_base=PC.WHEEL_BASE))
    PC.check_curvature_box(b, kap, run(b, 1), run(PC.batch(len(kap), b["ref"].shape[1]), 1))


def test_sizes_count_the_l_columns_of_the_cost():
    """BaseSolver::setCost's sparseView (base_solver.cpp:145) drops the l_i columns of P only while weight_l is an exact zero: pqp_path_sizes (a host
    function) counts them otherwise, as the oracle's pattern lists them - what pqp_path_pattern and pqp_path_assemble then fill on the device"""
    import ctypes as C
    from path_optimizer_2_amd import capi
    lib = capi.load_library()
    for case in PC.NAMES:
        prm, n = capi.production_params(**PC.CASES[case]), 80
        sizes = capi.PqpSizes()
        assert lib.pqp_path_sizes(C.byref(prm), n, None, C.byref(sizes)) == 0
        with_l = prm.weight_l != 0.0
        assert with_l == (case in PC.L_TOL)
        pcols = O.structural_pattern(n, n, with_l=with_l)[3]
        assert sizes.nnz_p == len(pcols) == (5 * n - 1 if with_l else 4 * n - 1) and sizes.nnz_a == 17 * n - 5
        assert (np.diff(pcols) > 0).all() and with_l == (0 in pcols)
