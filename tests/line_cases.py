"""Lines for the line-geometry kernels and the checks of their outputs against oracle/corridor_oracle.py, shared by the tests of the LDS
forms (test_gpu_line_geometry.py), the long forms (test_gpu_long_lines.py) and the DP cases.
(pytest does not rewrite the asserts of a helper module: each one here carries its own message.)"""
import numpy as np

import corridor_oracle as K
import corridor_util as U
from corridor_util import tab_close

REFUSED = -4                              # PQP_ERR_CAPACITY
SEG_KEYS = ("x", "y", "s", "angle", "k")
SPLINE_SIZES = [3, 4, 63, 64, 65, 129, 400, 878, 2925]


# ---- lines ------------------------------------------------------------------------------------------------------------------------
def spacings(rng, m, lo=1e-3, hi=20.0):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), m - 1))


def walk(rng, m, lo=1e-3, hi=20.0):
    """random-walk knots (s, x, y) for the spline fit: spacings log-uniform in [lo, hi] m, values a random walk"""
    s = np.concatenate([[0.0], np.cumsum(spacings(rng, m, lo, hi))])
    return s, np.cumsum(rng.normal(size=m)), np.cumsum(rng.normal(size=m))


def smooth_line(rng, m, length, heading=None, lo=1e-3, hi=20.0):
    """m knots of a smooth curve of parameter length `length` (spacings log-uniform in [lo, hi], scaled to it), starting in direction
    `heading` -> the restatement's splines and the packed table"""
    d = spacings(rng, m, lo, hi)
    s = np.concatenate([[0.0], np.cumsum(d * (length / d.sum()))])
    s[-1] = length
    th = rng.uniform(-np.pi, np.pi) if heading is None else heading
    l1, l2, p1, p2 = rng.uniform(25.0, 60.0), rng.uniform(40.0, 90.0), rng.uniform(0, 6.3), rng.uniform(0, 6.3)
    u = s + 0.3 * l1 * np.sin(s / l1 + p1) - 0.3 * l1 * np.sin(p1)
    v = 0.25 * l2 * (np.sin(s / l2 + p2) - np.sin(p2))
    x, y = 3.0 + u * np.cos(th) - v * np.sin(th), -2.0 + u * np.sin(th) + v * np.cos(th)
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    tab, ext = K.pack_spline(sx, sy)
    return dict(s=s, x=x, y=y, sx=sx, sy=sy, tab=tab, ext=ext, length=float(s[-1]))


def close(got, want, rel, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert float(err.max(initial=0.0)) <= rel, (what, float(err.max()), int(err.argmax()))


def check_spline_table(tab, ext, s, x, y, lib=None):
    """one scenario's table against the restatement (and the reference's own tk::spline when it is built): SPLINE_TOL of a row's largest"""
    want_tab, want_ext = K.pack_spline(K.spline_fit(s, x), K.spline_fit(s, y))
    tab_close(tab, ext, want_tab, want_ext)
    if lib is None:
        return
    m = len(s)
    for vals, r0 in ((x, 1), (y, 5)):
        sq, vq = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(vals, dtype=np.float64)
        hd = lib.ref_spline_new(m, sq.ctypes.data, vq.ctypes.data)
        just_right = np.nextafter(sq[:-1], np.inf)
        dl = just_right - sq[:-1]                # one ulp of the knot: on a line thousands of metres long the cubic term over it is not negligible
        d1, d2, d3 = (np.array([lib.ref_spline_deriv(hd, o, t) for t in just_right]) for o in (1, 2, 3))
        a = d3 / 6.0
        b = (d2 - 6.0 * a * dl) / 2.0
        c = d1 - (3.0 * a * dl + 2.0 * b) * dl
        for r, want in ((1, a), (2, b), (3, c)):
            U.rows_close(tab[r0 + r][:-1], want, ("reference build", r0, r))
        lib.ref_spline_free(hd)


# ---- checks ----------------------------------------------------------------------------------------------------------------------
def _check_states(ref, count, line, max_s, n_max, dynamic=True):
    want = K.build_reference_from_spline(line["sx"], line["sy"], float(max_s), dynamic=dynamic)
    assert count == len(want), (count, len(want))
    k = min(count, n_max)
    close(ref[:k], want[:k], 1e-11, "reference states")


def _check_segment(seg, q, line, max_s, n_max):
    x, y, s, ang, k = K.segment_raw_reference(line["sx"], line["sy"], float(max_s))
    assert seg["count"][q] == len(s), ("segment count", q, int(seg["count"][q]), len(s))
    n = min(len(s), n_max)
    assert np.array_equal(seg["s"][q, :n], s[:n]), ("segment s", q)
    for key, want in (("x", x), ("y", y), ("angle", ang), ("k", k)):
        close(seg[key][q, :n], want[:n], 1e-11, key)


def _degree(pts):
    """ReferencePathSmoother::bSpline's degree by the average point spacing"""
    d = np.diff(np.asarray(pts), axis=0)
    length = 0.0
    for ex, ey in d:
        length += np.sqrt(ex * ex + ey * ey)
    avg = length / (len(pts) - 1)
    return 3 if avg > 10.0 else (4 if avg > 5.0 else 5)


def _check_bspline(r, q, pts):
    if len(pts) <= _degree(pts):                 # tinyspline refuses a degree >= the number of control points: no line
        assert r["count"][q] == 0, ("bspline count of a refused polygon", q, int(r["count"][q]))
        return
    x, y, s = K.bspline_resample(pts)
    assert r["count"][q] == len(x), ("bspline count", q, int(r["count"][q]), len(x))
    n = min(len(x), r["x"].shape[1])
    close(r["x"][q, :n], x[:n], 1e-12, "x"); close(r["y"][q, :n], y[:n], 1e-12, "y")
    np.testing.assert_allclose(r["s"][q, :n], s[:n], rtol=0, atol=1e-11 * max(1.0, s[-1] / 50.0))
