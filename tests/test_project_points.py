"""pqp_project_points without a GPU: the symbols and the binding, the constants, the C++ wrapper's build, the kernel's resources, and known
answers for the Python restatement (tests/project_util.py) the GPU tests compare the kernel against."""
import math
import os
import re
import subprocess

import numpy as np

import build_util
import corridor_oracle as K
import cpp_demo
import project_util as P
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_project_points", "pqp_project_points_device")


def _header_constants():
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (PQP_PROJ_STRIDE|PQP_PROJECT_TILE_SAMPLES) (\d+)", txt)}
    consts.update({k: int(v) for k, v in re.findall(r"(PQP_PROJ_[A-Z_]+) = (\d+)", txt)})
    return consts


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES:
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    for fn in (hip_lib.pqp_project_points, hip_lib.pqp_project_points_device):
        assert len(fn.argtypes) == 13
    assert callable(capi.Handle.project_points)


def test_constants_equal_the_headers():
    c = _header_constants()
    assert c == dict(PQP_PROJ_STRIDE=capi.PROJ_STRIDE, PQP_PROJECT_TILE_SAMPLES=capi.PROJECT_TILE_SAMPLES, PQP_PROJ_AT_END=capi.PROJ_AT_END,
                     PQP_PROJ_BEFORE_START=capi.PROJ_BEFORE_START, PQP_PROJ_NOT_CONVERGED=capi.PROJ_NOT_CONVERGED,
                     PQP_PROJ_NOT_FINITE=capi.PROJ_NOT_FINITE)
    assert (capi.PROJ_AT_END, capi.PROJ_BEFORE_START, capi.PROJ_NOT_CONVERGED, capi.PROJ_NOT_FINITE) == (1, 2, 4, 8) == \
           (P.AT_END, P.BEFORE_START, P.NOT_CONVERGED, P.NOT_FINITE)
    assert capi.PROJ_STRIDE == 8


def test_projector_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("project_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    s = np.linspace(0.0, 10.0, 11)
    P.write_case(path, s, s, np.zeros(11), np.array([[2.5, 1.0, 0.1]]))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no projector" in r.stderr


def test_the_kernel_uses_no_scratch_and_one_tile_of_lds(hip_lib):
    r = build_util.find_kernel(build_util.kernel_report(), "project_points_kernel")
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] == 16 * (capi.PROJECT_TILE_SAMPLES + 1), r           # x, y of a tile of coarse samples and of the end sample
    assert r["Occupancy"] >= 4, r


# ---- known answers of the restatement --------------------------------------------------------------------------------------------------
S = np.linspace(0.0, 40.0, 41)


def _straight():
    return K.spline_fit(S, S.copy()), K.spline_fit(S, np.zeros_like(S))


def _arc(R=30.0):
    return K.spline_fit(S, R * np.sin(S / R)), K.spline_fit(S, R * (1 - np.cos(S / R)))


def test_straight_line_by_hand():
    """the line y = 0 along x: s is the point's x, l its y, the foot point (x, 0) with heading 0 and curvature 0"""
    sx, sy = _straight()
    row, flag = P.project(sx, sy, 40.0, 27.3, 1.5, heading=0.25)
    np.testing.assert_allclose(row, [27.3, 1.5, 0.0, 0.25, 27.3, 0.0, 0.0, 0.0], atol=1e-9)
    assert flag == 0
    row, flag = P.project(sx, sy, 40.0, 12.0, -2.0)                          # to the right: negative; no heading: d_heading 0
    np.testing.assert_allclose(row, [12.0, -2.0, 0.0, 0.0, 12.0, 0.0, 0.0, 0.0], atol=1e-9)
    assert flag == 0
    # beyond the end: clipped, t is what sticks out; the heading error wraps
    row, flag = P.project(sx, sy, 40.0, 45.0, 1.0, heading=math.pi + 0.5)
    np.testing.assert_allclose(row, [40.0, 1.0, 5.0, 0.5 - math.pi, 40.0, 0.0, 0.0, 0.0], atol=1e-9)
    assert row[0] == 40.0 and flag == P.AT_END
    # before the start: the spline extrapolates and s goes negative
    row, flag = P.project(sx, sy, 40.0, -2.5, 0.7)
    np.testing.assert_allclose(row, [-2.5, 0.7, 0.0, 0.0, -2.5, 0.0, 0.0, 0.0], atol=1e-9)
    assert flag == P.BEFORE_START
    # a shorter length than the knots reach clips there; a length that is no integer has its end sample behind the grid's last
    row, flag = P.project(sx, sy, 25.5, 30.0, 0.0)
    assert row[0] == 25.5 and abs(row[2] - 4.5) < 1e-9 and flag == P.AT_END


def test_arc_by_hand():
    """the arc of test_reference_length_up_to_the_target: 2 m inside it at s = 22 -> l = +2 (the centre is to the left), k = 1 / R"""
    R = 30.0
    cx, cy = _arc(R)
    phi = 22.0 / R
    row, flag = P.project(cx, cy, 40.0, (R - 2.0) * np.sin(phi), R - (R - 2.0) * np.cos(phi), heading=phi + 0.1)
    assert flag == 0
    assert abs(row[0] - 22.0) < 1e-3                      # the spline through 41 knots is the arc to ~1e-6 m
    np.testing.assert_allclose(row[1:4], [2.0, 0.0, 0.1], atol=1e-4)
    np.testing.assert_allclose(row[4:7], [R * np.sin(phi), R * (1 - np.cos(phi)), phi], atol=1e-4)
    assert abs(row[7] - 1.0 / R) < 1e-4
    row, _ = P.project(cx, cy, 40.0, (R + 1.5) * np.sin(phi), R - (R + 1.5) * np.cos(phi))          # outside: to the right
    assert abs(row[1] + 1.5) < 1e-4 and abs(row[0] - 22.0) < 1e-3


def test_degenerate_lengths_and_points_that_are_not_numbers():
    sx, sy = _straight()
    for length in (0.0, -3.0, math.nan):
        row, flag = P.project(sx, sy, length, 5.0, 2.0, heading=0.3)
        np.testing.assert_allclose(row, [0.0, 2.0, 5.0, 0.3, 0.0, 0.0, 0.0, 0.0], atol=1e-12)
        assert flag == (P.AT_END if length == 0.0 else 0)
    for bad in ((math.nan, 1.0, 0.0), (1.0, math.inf, 0.0), (1.0, 1.0, math.nan)):
        row, flag = P.project(sx, sy, 40.0, bad[0], bad[1], heading=bad[2])
        assert np.isnan(row).all() and flag == P.NOT_FINITE
    row, flag = P.project(sx, sy, 40.0, 1.0, 1.0)                            # the heading is not read: whatever it holds
    assert flag == 0 and np.isfinite(row).all()
    row, flag = P.project(sx, sy, math.inf, 1.0, 1.0)
    assert np.isnan(row).all() and flag == P.NOT_FINITE


def test_the_trace_sees_ties_and_near_ties():
    sx, sy = _straight()
    tr = P.trace(sx, sy, 40.0, 10.5, 3.0)                                    # equidistant from samples 10 and 11: an exact tie, not ambiguous
    c = sorted(tr["coarse"])
    assert c[0] == c[1] and not P.ambiguous(tr) and abs(tr["s"] - 10.5) < 1e-9
    tr = P.trace(sx, sy, 40.0, 10.5 + 1e-11, 3.0)                            # a gap of ~3e-12 between the two: within rounding
    assert P.ambiguous(tr)
    tr = P.trace(sx, sy, 40.0, 10.2, 3.0)
    assert not P.ambiguous(tr) and tr["converged"] and 1 <= len(tr["steps"]) <= 20
    # an integer length: the end sample is the grid's last sample bit for bit - a gap of exactly 0
    tr = P.trace(sx, sy, 40.0, 43.0, 1.0)
    assert tr["end"] == tr["coarse"][-1] == min(tr["coarse"]) and not P.ambiguous(tr)
