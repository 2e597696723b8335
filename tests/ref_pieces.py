"""The reference's std-only pieces (tk::spline, constrainAngle, the POD types and VehicleState; oracle/_ref, compiled from the reference's
own sources by oracle/Makefile) as the tests see them: what they computed on fixed inputs, recorded in tests/golden/reference_pieces.npz by
tests/golden/make_golden.py, and - where oracle/_ref has been built - the libraries themselves, which must still agree with the record."""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SPLINE = os.path.join(ROOT, "oracle", "_ref", "libref_spline.so")
REF_TYPES = os.path.join(ROOT, "oracle", "_ref", "libref_types.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_pieces.npz")

SPLINE_CASES = 12
STATE_A7 = (1.5, -2.5, 0.25, 0.125, 7.0, 3.0, -1.0)
VEHICLE_ARGS = ((0.5, 0.75, -0.5, 0.0625), (20.0, 3.0, 0.375, -0.03125), 0.4, -0.1, -0.2, 0.05)
BOUND_ARGS = ((1.75, -2.25), (4.0, 5.0, 0.5))


def spline_cases():
    """(x, y, t): knots, values and the points evaluated at - the knots, interior points and both extrapolations"""
    rng = np.random.default_rng(0)
    cases = []
    for _ in range(SPLINE_CASES):
        n = int(rng.integers(3, 60))
        x = np.cumsum(rng.uniform(0.2, 3.0, n)); y = np.cumsum(rng.normal(size=n))
        cases.append((x, y, np.concatenate([x, rng.uniform(x[0] - 3, x[-1] + 3, 120)])))
    return cases


def angles():
    rng = np.random.default_rng(7)
    pi = math.pi
    edge = [0.0, pi, -pi, np.nextafter(pi, 4.0), np.nextafter(-pi, -4.0), np.nextafter(pi, 0.0), 2 * pi, -2 * pi, 3 * pi, -3 * pi,
            np.nextafter(3 * pi, 10.0), 5 * pi - 1e-12, -7 * pi + 1e-12, 1e-300, -1e-300, 100.0, -100.0]
    return np.concatenate([np.array(edge), rng.uniform(-40.0, 40.0, 4000), rng.uniform(-pi, pi, 1000) + 2 * pi * rng.integers(-5, 6, 1000)])


def built():
    return os.path.exists(REF_SPLINE) and os.path.exists(REF_TYPES)


def record():
    """Everything the tests compare against, computed now by oracle/_ref (which must have been built: `make -C oracle ref`)."""
    sl = C.CDLL(REF_SPLINE)
    sl.ref_spline_new.restype = C.c_void_p; sl.ref_spline_new.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    sl.ref_spline_eval.restype = C.c_double; sl.ref_spline_eval.argtypes = [C.c_void_p, C.c_double]
    sl.ref_spline_deriv.restype = C.c_double; sl.ref_spline_deriv.argtypes = [C.c_void_p, C.c_int, C.c_double]
    sl.ref_spline_free.argtypes = [C.c_void_p]
    out = {}
    for c, (x, y, t) in enumerate(spline_cases()):
        h = sl.ref_spline_new(len(x), x.ctypes.data, y.ctypes.data)
        out[f"spline{c}_x"], out[f"spline{c}_y"], out[f"spline{c}_t"] = x, y, t
        out[f"spline{c}_value"] = np.array([[sl.ref_spline_eval(h, float(v))] + [sl.ref_spline_deriv(h, k, float(v)) for k in (1, 2, 3)] for v in t])
        sl.ref_spline_free(h)
    tl = C.CDLL(REF_TYPES)
    tl.ref_constrain_angle.argtypes = [C.c_double]; tl.ref_constrain_angle.restype = C.c_double
    a = angles()
    out["angle"], out["angle_constrained"] = a, np.array([tl.ref_constrain_angle(float(v)) for v in a])
    buf = (C.c_int * 64)()
    out["layout"] = np.array([int(buf[i]) for i in range(tl.ref_type_layout(buf, 64))], dtype=np.int64)
    o8 = (C.c_double * 8)()
    tl.ref_state_ctor((C.c_double * 7)(*STATE_A7), o8)
    out["state"] = np.array(list(o8))
    o6 = (C.c_double * 6)()
    tl.ref_vehicle_state.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)] + [C.c_double] * 4 + [C.POINTER(C.c_double)]
    s4, t4, *rest = VEHICLE_ARGS
    tl.ref_vehicle_state((C.c_double * 4)(*s4), (C.c_double * 4)(*t4), *rest, o6)
    out["vehicle"] = np.array(list(o6))
    o5 = (C.c_double * 5)()
    tl.ref_single_bound_set((C.c_double * 2)(*BOUND_ARGS[0]), (C.c_double * 3)(*BOUND_ARGS[1]), o5)
    out["single_bound"] = np.array(list(o5))
    return out


def reference():
    """The recorded values; where oracle/_ref is built, first checked bit for bit against what it computes now."""
    want = dict(np.load(GOLDEN))
    if built():
        live = record()
        assert sorted(live) == sorted(want)
        for k in want:
            assert np.array_equal(live[k], want[k]), k
    return want
