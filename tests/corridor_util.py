"""Test helper: scenes for the corridor-bounds step -> oracle objects and the flat ABI arrays; spline-table comparisons and the LDS
budgets of the line-geometry kernels."""
import os

import numpy as np

import corridor_oracle as K
from path_optimizer_2_amd.synth import make_scene


def build(seed, n=40, **kw):
    sc = make_scene(seed=seed, n=n, **kw)
    sx = K.spline_fit(sc["knots_s"], sc["knots_x"])
    sy = K.spline_fit(sc["knots_s"], sc["knots_y"])
    g = K.GridGeom(sc["rows"], sc["cols"], sc["resolution"], sc["length"][0], sc["length"][1], sc["pos"][0], sc["pos"][1])
    ref = np.zeros((n, 5))
    for i in range(n):
        s = i * sc["spacing"]
        dx, dy = K.spline_deriv(sx, 1, s), K.spline_deriv(sy, 1, s)
        ddx, ddy = K.spline_deriv(sx, 2, s), K.spline_deriv(sy, 2, s)
        ref[i] = (s, (dx * ddy - dy * ddx) / (dx * dx + dy * dy) ** 1.5, np.arctan2(dy, dx), K.spline_eval(sx, s), K.spline_eval(sy, s))
    tab, ext = K.pack_spline(sx, sy)
    return dict(scene=sc, sx=sx, sy=sy, geom=g, ref=ref, tab=tab, ext=ext, dist=sc["dist"])


SPLINE_TOL = 1e-13      # of the largest coefficient of a table row: the device solves the moment equations by a Thomas recurrence of its own (FMA
                        # contraction allowed), the reference by a row-normalised band LU - same spline, different round-off (measured: < 1e-15)


def ref_spline_lib():
    """the reference's own tk::spline, compiled from where it lies (oracle/_ref, built by oracle/Makefile; travels to the GPU box prebuilt)"""
    import ctypes as C
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_spline.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.ref_spline_new.restype = C.c_void_p; lib.ref_spline_new.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.ref_spline_deriv.restype = C.c_double; lib.ref_spline_deriv.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.ref_spline_eval.restype = C.c_double; lib.ref_spline_eval.argtypes = [C.c_void_p, C.c_double]
    lib.ref_spline_free.argtypes = [C.c_void_p]
    return lib


def rows_close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max()) / scale
    assert err <= SPLINE_TOL, (what, err)
    return err


def tab_close(tab, ext, want_tab, want_ext=None):
    """a device spline table against a restatement / golden one: knots and values exact, coefficient rows to SPLINE_TOL of the row's largest"""
    assert np.array_equal(np.asarray(tab)[[0, 1, 5]], np.asarray(want_tab)[[0, 1, 5]]), "knots or values of the spline table differ"
    for r in (2, 3, 4, 6, 7, 8):
        rows_close(tab[r], want_tab[r], ("row", r))
    if want_ext is not None:
        assert np.abs(np.asarray(ext) - np.asarray(want_ext)).max() <= SPLINE_TOL * max(1.0, float(np.abs(want_ext).max())), \
            ("spline end coefficients", np.abs(np.asarray(ext) - np.asarray(want_ext)).max())


DP_D_FLAG = 1e-6        # a `d < 1.2` / `d > 1.2` test this close to the threshold may come out either way: > 4 ulp of the float32 threshold


def dp_bounds_agree(lb, ub, want, what=None):
    """lb / ub of one scenario of pqp_dp_corridor against the oracle's result `want` (graph_search_dp) on a scene that was not built to keep
    its decisions away from round-off.  The bounds are sums of 0.6 m samples and 0.2 m steps, equal to round-off unless a distance sample sits
    on the 1.2 m threshold, so
      - at least 95 % of the layers agree in both bounds (as these comparisons always asked), and
      - an entry that does not agree is one the oracle flags - a threshold test that sets that entry directly came within DP_D_FLAG of the
        threshold (want["margin_lb" / "margin_ub"]) - and it is off by whole 0.2 m steps.
    Entries flagged on the scenes this is used on (counted on the CPU, the oracle alone): none on any - the five seeds of
    test_dp_corridor_search, the four grids of test_dp_corridor_search_on_other_grids, the 60 / 130 / 199 m lines of
    test_dp_corridor_long_lines_several_maps, the 900 m and 2.7 km roads of test_dp_corridor_past_the_edge, scene_a and scene_b: 0 of up to
    1805 layers x 2; the smallest margin of any test among them is 7.0e-5 (the 130 m line).  So on all of them every entry is held to 1e-9."""
    k = len(want["lb"])
    lb, ub = np.asarray(lb)[:k], np.asarray(ub)[:k]
    d_lb, d_ub = np.abs(lb - want["lb"]), np.abs(ub - want["ub"])
    same = (d_lb < 1e-9) & (d_ub < 1e-9)
    assert same.mean() > 0.95, (what, same.mean(), lb, want["lb"], ub, want["ub"])
    for side, d, margin in (("lb", d_lb, want["margin_lb"]), ("ub", d_ub, want["margin_ub"])):
        for i in np.nonzero(d >= 1e-9)[0]:
            assert margin[i] < DP_D_FLAG, (what, side, int(i), float(d[i]), float(margin[i]))
            steps = d[i] / 0.2
            assert round(steps) >= 1 and abs(steps - round(steps)) * 0.2 < 1e-9, (what, side, int(i), float(d[i]))
    return int((~same).sum())


def dp_flagged(want):
    """the number of lb / ub entries of an oracle result that dp_bounds_agree would excuse"""
    return int((want["margin_lb"] < DP_D_FLAG).sum() + (want["margin_ub"] < DP_D_FLAG).sum())


# ---- LDS budgets of the line-geometry kernels (pqp_corridor_kernels.inc, launchers in pqp_lines.hip) -----------------------------
LDS_PER_CU = 160 * 1024
# static LDS of each kernel as the compiler reports it ("LDS Size"): its __shared__ variables padded to the 16-byte alignment of the
# dynamic array behind them.  The launchers count it against LDS_PER_CU (tests/test_kernel_resources.py pins these numbers).
STATIC_LDS = {"spline_fit_kernel": 0, "reference_states_kernel": 16, "reference_length_kernel": 0, "offsets_to_points_kernel": 0,
              "bspline_resample_kernel": 16, "dp_corridor_kernel": 0, "corridor_bounds_kernel": 16}


def dp_lateral_samples(rng=10.0, spacing=0.6):
    nlat, c = 0, -rng
    while c <= rng and nlat < 64:
        c += spacing
        nlat += 1
    return nlat


def dp_lds_bytes(m, lmax, nlat):
    """DpBlock<true, true>::total_bytes()"""
    parent = 9 * m + lmax + 2 * 64 * 2 + 8 + lmax + 64 + 8 * lmax + 33 * nlat + 2 * nlat * nlat
    return parent * 8 + ((lmax * nlat + 7) // 8) * 8 + lmax * 4


def dynamic_lds(kernel, **a):
    """dynamic LDS bytes the launcher of `kernel` asks for"""
    if kernel == "spline_fit_kernel":
        return 7 * a["m"] * 8
    if kernel == "reference_states_kernel":
        return (9 * a["m"] + a["n_max"]) * 8
    if kernel == "reference_length_kernel":
        return 9 * a["m"] * 8
    if kernel == "offsets_to_points_kernel":
        return (9 * a["m_spline"] + 2 * a["m"]) * 8
    if kernel == "bspline_resample_kernel":
        return (3 * a["p_max"] + 6 + 3 * a["n_max"]) * 8
    if kernel == "dp_corridor_kernel":
        return dp_lds_bytes(a["m"], a["max_layers"], a["nlat"])
    raise KeyError(kernel)


def fits(kernel, **a):
    return STATIC_LDS[kernel] + dynamic_lds(kernel, **a) <= LDS_PER_CU


def largest(kernel, var, **a):
    """the largest value of argument `var` (the others fixed) whose launch fits one CU's LDS"""
    lo, hi = 1, 1
    while fits(kernel, **{**a, var: hi}):
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(kernel, **{**a, var: mid}) else (lo, mid)
    return lo
