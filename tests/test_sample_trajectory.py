"""pqp_sample_trajectory without a GPU: the symbols and the binding, the constants, the refusals, the chain wrapper's argument checks, the
C++ wrapper's build, the kernel's resources, and known answers by hand for the numpy restatement (tests/sample_util.py) the GPU tests
compare the kernel against bit for bit."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import build_util
import cpp_demo
import sample_util as S
import speed_util as V
from path_optimizer_2_amd import capi
from shared_util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_sample_trajectory", "pqp_sample_trajectory_device")
LDS_BYTES = 0                                                # the kernel's choice: the search runs across the lanes, not through LDS


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_sample_default_params",):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    for fn in (hip_lib.pqp_sample_trajectory, hip_lib.pqp_sample_trajectory_device):
        assert len(fn.argtypes) == 14
    assert callable(capi.Handle.sample_trajectory)
    assert list(inspect.signature(capi.Handle.sample_trajectory).parameters) == ["self", "paths", "profile", "m", "n_of", "stop_before", "t0", "prm"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        prm = inspect.signature(fn).parameters
        for k in ("sample", "samples", "t0"):
            assert prm[k].default is None, k


def test_constants_and_defaults_equal_the_headers(hip_lib):
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"(PQP_TRAJ_[A-Z_]+) = (\d+)", txt)}
    consts.update({k: int(v) for k, v in re.findall(r"#define (PQP_TRAJ_STRIDE) (\d+)", txt)})
    assert consts == dict(PQP_TRAJ_STRIDE=capi.TRAJ_STRIDE, PQP_TRAJ_HORIZON_SHORT=capi.TRAJ_HORIZON_SHORT, PQP_TRAJ_STANDS=capi.TRAJ_STANDS,
                          PQP_TRAJ_ENDS_MOVING=capi.TRAJ_ENDS_MOVING, PQP_TRAJ_EMPTY=capi.TRAJ_EMPTY, PQP_TRAJ_NOT_FINITE=capi.TRAJ_NOT_FINITE)
    assert (capi.TRAJ_HORIZON_SHORT, capi.TRAJ_STANDS, capi.TRAJ_ENDS_MOVING, capi.TRAJ_EMPTY, capi.TRAJ_NOT_FINITE) == (1, 2, 4, 8, 16) == \
           (S.HORIZON_SHORT, S.STANDS, S.ENDS_MOVING, S.EMPTY, S.NOT_FINITE)
    assert capi.TRAJ_STRIDE == 8 == S.STRIDE
    assert C.sizeof(capi.PqpSampleParams) == 16              # double, int32, padding: the header's struct
    p = capi.sample_default_params(hip_lib)                  # pure host
    assert {k: getattr(p, k) for k in S.DEFAULTS} == S.DEFAULTS == dict(dt=0.1, hold_last=0)
    assert capi.sample_default_params(hip_lib, dt=0.25, hold_last=1).dt == 0.25
    hip_lib.pqp_sample_default_params(None)                  # a null pointer is ignored, as by the other *_default_params


def test_refused_before_it_touches_a_device(hip_lib):
    """both forms refuse a null handle with the entry point's name in front"""
    prm = capi.sample_default_params(hip_lib)
    for fn in (hip_lib.pqp_sample_trajectory, hip_lib.pqp_sample_trajectory_device):
        assert fn(None, C.byref(prm), 1, 4, 7, None, None, None, None, None, 3, None, None, None) == -1
        assert hip_lib.pqp_last_error().decode().startswith("pqp_sample_trajectory:")


def test_sample_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    sa, sp = capi.sample_default_params(hip_lib), capi.speed_default_params(hip_lib)
    check = lambda *a: capi.Handle._sample(None, *a)         # (sample, samples, t0, speed)
    assert check(None, None, None, sp) is None and check(None, None, None, None) is None
    with pytest.raises(ValueError):
        check(sa, 10, None, None)                            # sample without speed
    with pytest.raises(ValueError):
        check(None, 10, None, sp)                            # samples without sample
    with pytest.raises(ValueError):
        check(None, None, [0.0], sp)                         # t0 without sample
    with pytest.raises(ValueError):
        check(sa, None, None, sp)                            # sample without a count
    with pytest.raises(ValueError):
        check(sa, 0, None, sp)
    got = check(sa, 12, [0.0, 1.5], sp)
    assert got[0] is sa and got[1] == 12 and got[2].tolist() == [0.0, 1.5]
    assert check(sa, 12, None, sp)[2] is None


def test_sampler_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("sample_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    paths = np.zeros((1, 5, 7))
    paths[0, :, 0] = np.arange(5)
    S.write_case(path, paths, np.zeros((1, 5, 4)), 3, [5], [5], [0.0], 0.1, 0)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no sampler" in r.stderr


def test_the_kernel_uses_no_scratch_and_a_constant_lds(hip_lib):
    r = build_util.find_kernel(build_util.kernel_report(), "sample_trajectory_kernel")
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= 4, r
    assert r["LDS Size"] <= LDS_BYTES, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r


# ---- known answers of the restatement --------------------------------------------------------------------------------------------------
def _line(n, step=1.0, stride=7):
    p = np.zeros((n, stride))
    p[:, 0] = step * np.arange(n)
    return p


def test_straight_line_from_rest_by_hand():
    """1 m chords, a_max = 1.5, from rest: s = 0.75 tau^2, v = 1.5 tau, a = 1.5, on the x axis"""
    path = _line(40)
    prof, flags = V.profile(path, 0.0, prm=dict(v_max=100.0, a_max=1.5, d_max=3.0, a_lat_max=math.inf))
    assert flags == 0
    m = 15
    rows, m_of, fl = S.sample(path, prof, m, dt=0.5)
    tau = 0.5 * np.arange(m)
    assert m_of == m and fl == S.HORIZON_SHORT               # 39 m take 7.2 s: the horizon of 7 s ends before
    assert np.array_equal(rows[:, 7], tau)
    np.testing.assert_allclose(rows[:, 4], 0.75 * tau ** 2, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(rows[:, 5], 1.5 * tau, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(rows[1:, 6], 1.5, rtol=1e-13)
    np.testing.assert_allclose(rows[:, 0], rows[:, 4], rtol=1e-13, atol=1e-15)
    assert (rows[:, 1] == 0).all() and (rows[:, 2] == 0).all() and (rows[:, 3] == 0).all()
    # a longer horizon passes the end, where the car still moves
    rows, m_of, fl = S.sample(path, prof, 20, dt=0.5)
    assert m_of == 15 and fl == S.ENDS_MOVING and (rows[15:] == 0).all()
    rows, m_of, fl = S.sample(path, prof, 20, dt=0.5, hold_last=1)
    assert m_of == 15 and fl == S.ENDS_MOVING
    assert (rows[15:, 0] == 39.0).all() and (rows[15:, 4] == prof[39, 0]).all() and (rows[15:, 5:7] == 0).all()
    assert np.array_equal(rows[15:, 7], 0.5 * np.arange(15, 20))


def _steady(n, v=2.0):
    """a quarter circle driven at a constant 2 m/s with times that are dyadic: 1 m of arc length per waypoint by decree"""
    phi = np.linspace(0.0, 1.5, n)
    p = np.zeros((n, 7))
    p[:, 0], p[:, 1], p[:, 2], p[:, 5] = 10 * np.sin(phi), 10 * (1 - np.cos(phi)), phi, 0.1
    prof = np.zeros((n, 4))
    prof[:, 0], prof[:, 1], prof[:, 3] = np.arange(n), v, np.arange(n) / v
    return p, prof


def test_a_sample_at_a_waypoints_time_is_that_waypoint():
    p, prof = _steady(9)
    rows, m_of, fl = S.sample(p, prof, 12, dt=0.5)
    assert m_of == 9 and fl == S.ENDS_MOVING
    want = np.concatenate([p[:, [0, 1, 2, 5]], prof], axis=1)
    want[:, 6] = 0.0
    assert same_bits(rows[:9], want) and (rows[9:] == 0).all()
    # t0 = 1: sample k is waypoint k + 2; a t0 behind the arrival leaves nothing on the path
    rows, m_of, fl = S.sample(p, prof, 12, t0=1.0, dt=0.5)
    assert m_of == 7 and same_bits(rows[:7], want[2:])
    rows, m_of, fl = S.sample(p, prof, 4, t0=4.5, dt=0.5)
    assert m_of == 0 and fl == S.ENDS_MOVING and (rows == 0).all()
    # the arrival time itself is on the path, one ulp later is not
    rows, m_of, fl = S.sample(p, prof, 1, t0=4.0, dt=0.5)
    assert m_of == 1 and fl == 0 and same_bits(rows[0], want[8])
    rows, m_of, fl = S.sample(p, prof, 1, t0=np.nextafter(4.0, 5.0), dt=0.5)
    assert m_of == 0 and fl == S.ENDS_MOVING
    # halfway between two waypoints: halfway along the chord, the heading and curvature in between
    rows, m_of, fl = S.sample(p, prof, 2, t0=0.25, dt=0.5, n_of=9, stop_before=20)
    d = np.hypot(*(p[1, :2] - p[0, :2]))
    lam = 0.5 / d                                            # u = 0.25 s at 2 m/s: 0.5 m of the chord of d m
    np.testing.assert_allclose(rows[0, :2], p[0, :2] + lam * (p[1, :2] - p[0, :2]), rtol=1e-15)
    assert rows[0, 4] == 0.5 and rows[0, 5] == 2.0 and rows[0, 6] == 0.0 and rows[0, 7] == 0.25
    np.testing.assert_allclose(rows[0, 2], lam * p[1, 2], rtol=1e-15)
    # the heading turns the short way across the seam
    q = p.copy()
    q[0, 2], q[1, 2] = 3.1, -3.1
    rows, _, _ = S.sample(q, prof, 1, t0=0.25, dt=0.5)
    assert 3.1 < rows[0, 2] <= S.PI or -S.PI <= rows[0, 2] < -3.1


def test_duplicate_waypoint_and_standing_still_by_hand():
    p, prof = _steady(8)
    p[4:] = p[3:-1].copy()                                   # waypoints 3 and 4 coincide
    prof[4:, 0], prof[4:, 3] = prof[3:-1, 0].copy(), prof[3:-1, 3].copy()
    rows, m_of, fl = S.sample(p, prof, 8, dt=0.5)
    assert m_of == 7 and fl == S.ENDS_MOVING
    assert np.array_equal(rows[3, :2], p[4, :2]) and rows[3, 7] == 1.5 and np.array_equal(rows[4, :2], p[5, :2])
    # the t column steps back by an ulp at the duplicate: the running maximum decides, nothing moves backwards
    prof2 = prof.copy()
    prof2[4, 3] = np.nextafter(prof[3, 3], 0.0)
    rows2, m_of2, fl2 = S.sample(p, prof2, 8, dt=0.5)
    assert (m_of2, fl2) == (m_of, fl) and (np.diff(rows2[:m_of2, 4]) >= 0).all()
    # (sample 3 is in segment 4 as before; u = tau - t_4 is now one ulp of 1.5, 2 m/s of it move s by at most one ulp of 3)
    assert np.abs(rows2[:, 4] - rows[:, 4]).max() <= np.spacing(3.0) and np.array_equal(np.delete(rows2, 3, axis=0), np.delete(rows, 3, axis=0))
    rows3, _, _ = S.sample(p, prof2, 1, t0=float(prof2[4, 3]), dt=0.5)          # between the two stamps: in front of both, in segment 2
    assert prof[2, 0] < rows3[0, 4] <= prof[3, 0] and p[2, 0] < rows3[0, 0] <= p[3, 0] and rows3[0, 7] == prof2[4, 3]
    # both ends at rest over one chord: the car never leaves (the profile's NEVER_ARRIVES)
    path = _line(2)
    pr, pf = V.profile(path, 0.0, v_end=0.0)
    assert pf == V.NEVER_ARRIVES and pr[1, 3] == math.inf
    rows, m_of, fl = S.sample(path, pr, 5, dt=1.0)
    assert m_of == 5 and fl == S.STANDS | S.HORIZON_SHORT
    assert (rows[:, [0, 1, 2, 3, 4, 5, 6]] == 0).all() and np.array_equal(rows[:, 7], np.arange(5.0))


def test_counts_hold_last_and_values_that_are_not_numbers():
    p, prof = _steady(6)
    for kw in (dict(n_of=0), dict(stop_before=-3), dict(n_of=4, stop_before=0)):
        for hold in (0, 1):
            rows, m_of, fl = S.sample(p, prof, 5, hold_last=hold, t0=math.nan, **kw)          # nothing is read, t0 neither
            assert fl == S.EMPTY and m_of == 0 and (rows == 0).all()
    # c = 1: sample 0 is the waypoint, the rest is behind the arrival
    rows, m_of, fl = S.sample(p, prof, 3, n_of=1)
    assert m_of == 1 and fl == S.ENDS_MOVING and rows[0].tolist() == [0.0, 0.0, 0.0, 0.1, 0.0, 2.0, 0.0, 0.0] and (rows[1:] == 0).all()
    rows, m_of, fl = S.sample(p, prof, 3, n_of=1, hold_last=1)
    assert m_of == 1 and rows[2].tolist() == [0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 0.2]
    # c = 2, by stop_before: one segment of 0.5 s
    rows, m_of, fl = S.sample(p, prof, 8, n_of=6, stop_before=2, dt=0.125)
    assert m_of == 5 and fl == S.ENDS_MOVING and np.array_equal(rows[:5, 4], 0.25 * np.arange(5)) and rows[4, 0] == p[1, 0]
    for where, value in (((2, 0), math.nan), ((3, 5), math.inf), ((0, 1), -math.inf), ((1, 2), math.nan)):
        q = p.copy()
        q[where] = value
        rows, m_of, fl = S.sample(q, prof, 4, n_of=5)
        assert fl == S.NOT_FINITE and m_of == 0 and np.isnan(rows).all()
        rows, m_of, fl = S.sample(q, prof, 4, n_of=5, stop_before=where[0])      # not read: not driven
        assert fl & S.NOT_FINITE == 0 and np.isfinite(rows).all()
    for where, value in (((1, 0), math.inf), ((2, 1), math.nan), ((0, 2), -math.inf), ((3, 3), math.nan), ((3, 3), -1.0)):
        q = prof.copy()
        q[where] = value
        rows, m_of, fl = S.sample(p, q, 4)
        assert fl == S.NOT_FINITE and m_of == 0 and np.isnan(rows).all(), (where, value)
    for t0 in (math.nan, math.inf, -0.5):
        rows, m_of, fl = S.sample(p, prof, 4, t0=t0)
        assert fl == S.NOT_FINITE and np.isnan(rows).all()
    q = prof.copy()
    q[4:, 3] = math.inf                                      # +inf is a time: the car stands at waypoint 3
    rows, m_of, fl = S.sample(p, q, 6, dt=0.5)
    assert fl == S.STANDS | S.HORIZON_SHORT and m_of == 6 and np.isfinite(rows).all()
