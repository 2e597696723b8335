"""The line-geometry steps of the device chain (pqp_spline_fit[_var], pqp_reference_states, pqp_segment_raw_reference, pqp_reference_length,
pqp_offsets_to_points, pqp_bspline_resample, pqp_dp_corridor) against their float64 restatements in oracle/corridor_oracle.py at the sizes
the chain runs them at: lane-stride loops that go round more than once (> 64 knots, points, samples), the multi-round coarse scan of the
wavefront projection, dynamic LDS above 48 KiB and up to the last size that fits one CU's 160 KiB (static __shared__ variables included),
long lines and batches of 1024 scenarios.

The device forms are called on torch tensors whose outputs lie in a larger allocation filled with a sentinel: whatever a kernel must not
write (the guard band behind [batch][n_max], rows past a scenario's count) has to come back as the sentinel.  Properties that need no
oracle - host form == device form, a permuted batch gives permuted outputs, a padded _var table gives what the exact-size table gives -
are checked bit for bit on every scenario; the oracle on a seeded subset."""
import numpy as np
import pytest

import corridor_oracle as K
import corridor_util as U
from corridor_util import tab_close
from device_form import (d_bounds, d_bspline, d_dp, d_offsets, d_reference_length, d_reference_states, d_segment, d_spline_fit,
                         host_equals_device)
from line_cases import (REFUSED, SEG_KEYS, SPLINE_SIZES, _check_bspline, _check_segment, _check_states, _degree, check_spline_table, close,
                        smooth_line, walk)
from path_optimizer_2_amd import capi
from shared_util import capi_geom, same_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=128)
    yield h
    h.close()


# =====================================================================================================================================
# pqp_spline_fit / pqp_spline_fit_var_device
# =====================================================================================================================================
def test_spline_fit_sizes_cover_the_lds_edges():
    assert U.fits("spline_fit_kernel", m=2925) and not U.fits("spline_fit_kernel", m=2926)
    assert U.dynamic_lds("spline_fit_kernel", m=877) <= 48 * 1024 < U.dynamic_lds("spline_fit_kernel", m=878)
    assert U.largest("spline_fit_kernel", "m") == 2925


@pytest.mark.parametrize("m", SPLINE_SIZES)
def test_spline_fit_against_the_oracle(handle, m):
    """fixed-size fit, host and device forms, at and around the lane stride, above 48 KiB and at the last size under 160 KiB"""
    rng = np.random.default_rng(1000 + m)
    B = 4
    # (the reference build's coefficients are read off its derivatives one ulp right of the knot, which needs spacings well above that ulp:
    #  0.2-3 m as in test_gpu_corridor.py for the scenario checked against it; the restatement takes the full 1e-3-20 m range)
    knots = [walk(rng, m) for _ in range(B - 1)] + [walk(rng, m, 0.2, 3.0)]
    s, x, y = (np.stack([k[i] for k in knots]) for i in range(3))
    rc, tab, ext = d_spline_fit(handle, s, x, y)
    assert rc == 0
    htab, hext = handle.spline_fit(s, x, y)
    assert same_bytes(htab, tab) and same_bytes(hext, ext)
    lib = U.ref_spline_lib()
    for q in range(B):
        check_spline_table(tab[q], ext[q], s[q], x[q], y[q], lib if q == B - 1 else None)


def test_spline_fit_refuses_one_knot_past_the_lds(handle):
    rng = np.random.default_rng(7)
    s, x, y = walk(rng, 2926)
    rc, tab, ext = d_spline_fit(handle, s[None], x[None], y[None])
    assert rc == REFUSED and tab.untouched() and ext.untouched()
    rc, tab, ext = d_spline_fit(handle, s[None], x[None], y[None], m_of=[2000])
    assert rc == REFUSED and tab.untouched() and ext.untouched()
    with pytest.raises(capi.PqpError, match="pqp error -4:"):
        handle.spline_fit(s[None], x[None], y[None])


def _check_var_table(tab, ext, s, x, y, n, stride, fixed_tab=None, fixed_ext=None):
    """one scenario of a _var fit with n real knots in a table of `stride`: real rows = the fixed-size fit of the same knots (bit for bit),
    pad rows = knots x_last + 1e6 j with the last value and zero coefficients; fewer than 3 knots: the constant table of the first point"""
    assert np.all(np.isfinite(tab)) and np.all(np.isfinite(ext))
    if n < 3:
        assert np.array_equal(tab[0], np.arange(stride, dtype=np.float64))
        assert np.all(tab[1] == x[0]) and np.all(tab[5] == y[0])
        assert np.all(tab[[2, 3, 4, 6, 7, 8]] == 0.0) and np.all(ext == 0.0)
        return
    n = min(n, stride)
    assert same_bytes(tab[:, :n], fixed_tab) and same_bytes(ext, fixed_ext)
    j = np.arange(1, stride - n + 1, dtype=np.float64)
    assert same_bytes(tab[0, n:], s[n - 1] + 1e6 * j)
    assert np.all(tab[1, n:] == x[n - 1]) and np.all(tab[5, n:] == y[n - 1])
    assert same_bytes(tab[[2, 3, 4, 6, 7, 8], n:], np.zeros((6, stride - n)))


@pytest.mark.parametrize("m_max", [65, 400])
def test_spline_fit_var_ragged_against_the_fixed_fit_and_the_oracle(handle, m_max):
    """pqp_spline_fit_var_device with m_of 1, 2, 3, 4, around 64 and m_max (and beyond it: clamped) mixed in one batch"""
    rng = np.random.default_rng(m_max)
    m_of = np.array([1, 2, 3, 4, 63, 64, 65, m_max, m_max + 5, 0, m_max - 1, 37], dtype=np.int32)
    B = len(m_of)
    knots = [walk(rng, m_max) for _ in range(B)]
    s, x, y = (np.stack([k[i] for k in knots]) for i in range(3))
    rc, tab, ext = d_spline_fit(handle, s, x, y, m_of=m_of)
    assert rc == 0
    for q in range(B):
        n = int(min(m_of[q], m_max))
        ft = fe = None
        if n >= 3:
            rc1, ft, fe = d_spline_fit(handle, s[q:q + 1, :n], x[q:q + 1, :n], y[q:q + 1, :n])
            assert rc1 == 0
            ft, fe = ft[0], fe[0]
            check_spline_table(ft, fe, s[q, :n], x[q, :n], y[q, :n])
        _check_var_table(tab[q], ext[q], s[q], x[q], y[q], int(m_of[q]), m_max, ft, fe)


def test_spline_fit_var_large_batch(handle):
    """1024 scenarios of up to 400 knots (the chain's size): every scenario's real rows equal the fixed-size fit and its pad rows the
    pattern; a permuted batch gives the permuted tables; the oracle on 16 of them"""
    rng = np.random.default_rng(77)
    B, m_max = 1024, 400
    sizes = np.array([3, 40, 64, 65, 129, 200, 333, 400], dtype=np.int32)
    m_of = sizes[rng.integers(0, len(sizes), B)]
    s = np.cumsum(np.concatenate([np.zeros((B, 1)), np.exp(rng.uniform(np.log(1e-3), np.log(20.0), (B, m_max - 1)))], axis=1), axis=1)
    x, y = np.cumsum(rng.normal(size=(B, m_max)), axis=1), np.cumsum(rng.normal(size=(B, m_max)), axis=1)
    rc, tab, ext = d_spline_fit(handle, s, x, y, m_of=m_of)
    assert rc == 0
    for n in sizes:                      # the fixed-size fit of each group's knots
        idx = np.nonzero(m_of == n)[0]
        rc1, ft, fe = d_spline_fit(handle, s[idx, :n], x[idx, :n], y[idx, :n])
        assert rc1 == 0
        for j, q in enumerate(idx):
            _check_var_table(tab[q], ext[q], s[q], x[q], y[q], int(n), m_max, ft[j], fe[j])
    perm = rng.permutation(B)
    rc, ptab, pext = d_spline_fit(handle, s[perm], x[perm], y[perm], m_of=m_of[perm])
    assert rc == 0 and same_bytes(ptab, tab[perm]) and same_bytes(pext, ext[perm])
    for q in np.random.default_rng(5).choice(B, 16, replace=False):
        n = int(m_of[q])
        want_tab, want_ext = K.pack_spline(K.spline_fit(s[q, :n], x[q, :n]), K.spline_fit(s[q, :n], y[q, :n]))
        tab_close(tab[q][:, :n], ext[q], want_tab, want_ext)


# =====================================================================================================================================
# pqp_reference_states / pqp_segment_raw_reference
# =====================================================================================================================================
@pytest.mark.parametrize("m,length", [(65, 60.0), (129, 300.0), (400, 1200.0), (2000, 3000.0)])
def test_reference_states_on_long_lines(handle, m, length):
    """lines of 60-3000 m on 65-2000 knots, n_max as large as LDS allows: max_s past the last knot, on a knot, below one step; fixed
    spacing; host == device; the same lines through segment_raw_reference"""
    rng = np.random.default_rng(int(length) + m)
    lines = [smooth_line(rng, m, length) for _ in range(3)]
    tab, ext = np.stack([l["tab"] for l in lines]), np.stack([l["ext"] for l in lines])
    n_max = U.largest("reference_states_kernel", "n_max", m=m)
    assert U.dynamic_lds("reference_states_kernel", m=m, n_max=n_max) > 48 * 1024
    knot = float(lines[1]["s"][m // 2])
    max_s = np.array([length + 7.3, knot, 0.1])
    for dynamic in (True, False):
        rc, ref, count, _ = d_reference_states(handle, tab, ext, max_s, n_max, dynamic=dynamic)
        assert rc == 0
        href, hcount, _ = handle.reference_states(tab, ext, max_s, n_max, dynamic=dynamic)
        assert np.array_equal(hcount, count)
        host_equals_device(href, ref, count, n_max)
        for q in range(3):
            _check_states(ref[q], int(count[q]), lines[q], max_s[q], n_max, dynamic)
        assert count[2] == 1
    n_seg = min(n_max, int(length) + 16)
    rc, seg = d_segment(handle, tab, ext, max_s, n_seg)
    assert rc == 0
    hseg = handle.segment_raw_reference(tab, ext, max_s, n_seg)
    assert np.array_equal(hseg["count"], seg["count"])
    for key in SEG_KEYS:
        host_equals_device(hseg[key], seg[key], seg["count"], n_seg)
    for q in range(3):
        _check_segment(seg, q, lines[q], max_s[q], n_seg)


def test_reference_states_count_past_n_max_on_a_long_line(handle):
    """a 3000 m line whose states outnumber n_max several times: count is the loop's, the n_max rows written are the first ones"""
    rng = np.random.default_rng(3)
    line = smooth_line(rng, 300, 3000.0)
    n_max = 4000
    rc, ref, count, _ = d_reference_states(handle, line["tab"][None], line["ext"][None], np.array([3000.0]), n_max)
    assert rc == 0 and count[0] > 2 * n_max
    _check_states(ref[0], int(count[0]), line, 3000.0, n_max)
    rc, seg = d_segment(handle, line["tab"][None], line["ext"][None], np.array([3000.0]), 1000)
    assert rc == 0 and seg["count"][0] == 3001
    _check_segment(seg, 0, line, 3000.0, 1000)


def test_reference_states_step_lands_on_max_s(handle):
    """on a straight line (x = s, y = 0: curvature exactly 0) every step is exactly 0.3 and the walk's abscissae are the restatement's bit
    for bit; max_s set to the 1000th of them keeps that state (tmp_s <= max_s) - a step one ulp long drops it"""
    s = np.arange(0.0, 400.0)
    line = dict(sx=K.spline_fit(s, s), sy=K.spline_fit(s, np.zeros_like(s)))
    tab, ext = K.pack_spline(line["sx"], line["sy"])
    on = 0.0
    for _ in range(1000):
        on += 0.3
    max_s = np.array([on, np.nextafter(on, 0.0), on])
    tabs, exts = np.stack([tab] * 3), np.stack([ext] * 3)
    for dynamic in (True, False):
        rc, ref, count, _ = d_reference_states(handle, tabs, exts, max_s, 1100, dynamic=dynamic)
        assert rc == 0 and list(count) == [1001, 1000, 1001]
        for q in range(3):
            want = K.build_reference_from_spline(line["sx"], line["sy"], float(max_s[q]), dynamic=dynamic)
            assert count[q] == len(want) and np.array_equal(ref[q, :count[q], 0], want[:, 0])
            close(ref[q, :count[q]], want, 1e-11, "straight line")


def test_initial_error_with_headings_near_pi(handle):
    rng = np.random.default_rng(11)
    lines = [smooth_line(rng, 129, 200.0, heading=h) for h in (np.pi - 1e-9, -np.pi + 1e-9, np.pi - 0.02, 0.3)]
    tab, ext = np.stack([l["tab"] for l in lines]), np.stack([l["ext"] for l in lines])
    start = []
    for q, l in enumerate(lines):
        sh = (np.pi - 3e-10, -np.pi + 2e-10, -np.pi + 0.01, np.pi - 1e-7)[q]
        start.append([l["x"][0] + 0.4, l["y"][0] - 0.7, sh])
    start = np.array(start)
    max_s = np.full(4, 150.0)
    rc, ref, count, err = d_reference_states(handle, tab, ext, max_s, 1200, start=start)
    assert rc == 0
    href, hcount, herr = handle.reference_states(tab, ext, max_s, 1200, start=start)
    assert same_bytes(herr, err)
    for q, l in enumerate(lines):
        off, dpsi = K.process_init_state(l["sx"], l["sy"], *start[q])
        assert err[q, 0] == pytest.approx(off, abs=1e-12) and err[q, 1] == pytest.approx(dpsi, abs=1e-12)
        _check_states(ref[q], int(count[q]), l, 150.0, 1200)


# =====================================================================================================================================
# pqp_reference_length: the wavefront projection's coarse scan, one round per 64 m
# =====================================================================================================================================
def _parabola(length, a=1.0, vertex=63.5):
    """x = s, y = a (s - vertex)^2 on integer knots: from (vertex, a / 4 + 1 / (2 a)) the nearest points of the curve are at s = vertex -+ 1/2
    and its samples there are exactly equidistant (y = a / 4 at both), while Newton from either one stays on its own side - the coarse
    scan's tie rule (the first minimum wins) decides the result"""
    s = np.arange(0.0, length + 1.0)
    sx, sy = K.spline_fit(s, s), K.spline_fit(s, a * (s - vertex) ** 2)
    tab, ext = K.pack_spline(sx, sy)
    return dict(sx=sx, sy=sy, tab=tab, ext=ext), (vertex, a / 4 + 1 / (2 * a))


def _target(line, s, off):
    x, y = K.spline_eval(line["sx"], s), K.spline_eval(line["sy"], s)
    h = np.arctan2(K.spline_deriv(line["sy"], 1, s), K.spline_deriv(line["sx"], 1, s))
    return [x - off * np.sin(h), y + off * np.cos(h), h]


@pytest.mark.parametrize("length", [63.0, 64.0, 65.0, 150.0, 300.0])
def test_reference_length_scan_rounds_and_ties(handle, length):
    rng = np.random.default_rng(int(length))
    lines, targets = [], []
    # smooth lines: the coarse minimum in round 1, 2, 3 (where the line is that long), beside the line and at its end; beyond the end
    for s_t, off in ((10.3, 0.0), (40.7, 2.5), (70.2, -1.5), (100.0, 0.8), (140.6, 3.0), (250.4, -0.4), (length - 0.3, 1.0)):
        if s_t < length:
            line = smooth_line(rng, int(length / 2) + 3, length, lo=0.5, hi=4.0)
            lines.append(line); targets.append(_target(line, s_t, off))
    line = smooth_line(rng, 70, length, lo=0.5, hi=4.0)
    end = _target(line, length, 0.0)
    lines.append(line); targets.append([end[0] + 3.0 * np.cos(end[2]), end[1] + 3.0 * np.sin(end[2]), 0.0])
    # exact ties: inside round 1 (31 / 32) and across the boundary of rounds 1 and 2 (63 / 64), 2 and 3 (127 / 128)
    for vertex in (31.5, 63.5, 127.5):
        if vertex + 1.0 < length:
            line, tgt = _parabola(length, vertex=vertex)
            lines.append(line); targets.append([tgt[0], tgt[1], 0.0])
    # ... and on a straight line (x = s, y = 0), where both neighbours lead Newton to the same point
    s = np.arange(0.0, length + 1.0)
    straight = dict(sx=K.spline_fit(s, s), sy=K.spline_fit(s, np.zeros_like(s)))
    straight["tab"], straight["ext"] = K.pack_spline(straight["sx"], straight["sy"])
    for s_t in (31.5, 63.5):
        if s_t < length:
            lines.append(straight); targets.append([s_t, 0.0, 0.0])
    m = max(l["tab"].shape[1] for l in lines)
    # one batch: tables of different widths padded as pqp_spline_fit_var_device pads them
    tab = np.stack([_pad_table(l["tab"], m) for l in lines]); ext = np.stack([l["ext"] for l in lines])
    L = np.full(len(lines), length); target = np.array(targets)
    rc, got = d_reference_length(handle, tab, ext, L, target)
    assert rc == 0
    assert same_bytes(handle.reference_length(tab, ext, L, target), got)
    for q, l in enumerate(lines):
        want = K.reference_length(l["sx"], l["sy"], length, target[q, 0], target[q, 1])
        assert got[q] == pytest.approx(want, abs=1e-9), (q, got[q], want)


def _pad_table(tab, m):
    """a packed table of n knots widened to m as the _var fit pads it: knots x_last + 1e6 j, the last value, zero coefficients"""
    n = tab.shape[1]
    if n == m:
        return tab
    out = np.zeros((9, m))
    out[:, :n] = tab
    out[0, n:] = tab[0, n - 1] + 1e6 * np.arange(1, m - n + 1, dtype=np.float64)
    out[1, n:], out[5, n:] = tab[1, n - 1], tab[5, n - 1]
    return out


def test_reference_length_tie_keeps_the_first_sample(handle):
    """the parabola's tie decided explicitly: the result lies beside the lower of the two equidistant samples"""
    for length, vertex in ((100.0, 31.5), (100.0, 63.5), (200.0, 127.5)):
        line, tgt = _parabola(length, vertex=vertex)
        rc, got = d_reference_length(handle, line["tab"][None], line["ext"][None], np.array([length]), np.array([[tgt[0], tgt[1], 0.0]]))
        assert rc == 0
        want = K.reference_length(line["sx"], line["sy"], length, tgt[0], tgt[1])
        assert want < vertex and abs(want - (vertex - 0.5)) < 0.05, want
        assert got[0] == pytest.approx(want, abs=1e-9)


# =====================================================================================================================================
# pqp_offsets_to_points
# =====================================================================================================================================
@pytest.mark.parametrize("m_spline,m", [(65, 63), (129, 64), (400, 65), (129, 400), (2000, 1240)])
def test_offsets_to_points_against_the_oracle(handle, m_spline, m):
    """offsets |l| <= 10 m at abscissae over the whole line (and past its end), ragged m_of; the device form leaves rows past m_of alone,
    the host form returns zeros there"""
    rng = np.random.default_rng(m_spline * 7 + m)
    B = 4
    length = 1.5 * m_spline
    lines = [smooth_line(rng, m_spline, length) for _ in range(B)]
    tab, ext = np.stack([l["tab"] for l in lines]), np.stack([l["ext"] for l in lines])
    at_s = np.sort(rng.uniform(0.0, length + 5.0, (B, m)), axis=1)
    l = rng.uniform(-10.0, 10.0, (B, m))
    m_of = np.array([m, m - 1, 1, max(m // 2, 2)], dtype=np.int32)
    rc, x, y, s = d_offsets(handle, tab, ext, at_s, l, m_of)
    assert rc == 0
    hx, hy, hs = handle.offsets_to_points(tab, ext, at_s, l, m_of=m_of)
    for h_, d_ in ((hx, x), (hy, y), (hs, s)):
        host_equals_device(h_, d_, m_of, m)
    for q in range(B):
        k = int(m_of[q])
        wx, wy, ws = K.offsets_to_points(lines[q]["sx"], lines[q]["sy"], at_s[q, :k], l[q, :k])
        close(x[q, :k], wx, 1e-11, "x"); close(y[q, :k], wy, 1e-11, "y")
        np.testing.assert_allclose(s[q, :k], ws, rtol=0, atol=1e-10 * max(1.0, ws[-1] / 30.0))


# =====================================================================================================================================
# pqp_bspline_resample
# =====================================================================================================================================
@pytest.mark.parametrize("p", [4, 33, 64, 65, 200])
def test_bspline_resample_degrees_and_sizes(handle, p):
    """all three degrees - average spacing exactly 10.0 (degree 4) and 5.0 (degree 5) from collinear points on integer x, above 10 (3) - and
    jittered points; sample counts past 64"""
    rng = np.random.default_rng(p)
    sets = [np.column_stack([10.0 * np.arange(p), np.zeros(p)]), np.column_stack([5.0 * np.arange(p), np.zeros(p)]),
            np.column_stack([-3.0 - 5.0 * np.arange(p), np.full(p, 7.0)])]
    for spacing in (14.0, 7.0, 2.0):
        sets.append(np.cumsum(np.column_stack([np.full(p, spacing), rng.uniform(-0.4, 0.4, p) * spacing]), axis=0))
    pts = np.stack(sets)
    n_pts = np.full(len(sets), p, dtype=np.int32)
    n_max = int(14.0 * p + 8)
    rc, r = d_bspline(handle, pts, n_pts, n_max)
    assert rc == 0
    h = handle.bspline_resample(pts, n_pts, n_max)
    assert np.array_equal(h["count"], r["count"])
    for key in ("x", "y", "s"):
        host_equals_device(h[key], r[key], r["count"], n_max)
    for q, pq in enumerate(sets):
        _check_bspline(r, q, pq)


def test_bspline_resample_at_the_lds_edge(handle):
    """the largest n_max that fits one CU's LDS (static __shared__ included) for 65 points 100 m apart (6400 samples); one more is refused"""
    rng = np.random.default_rng(4)
    p = 65
    pts = np.cumsum(np.column_stack([np.full(p, 100.0), rng.uniform(-20.0, 20.0, p)]), axis=0)[None]
    n_max = U.largest("bspline_resample_kernel", "n_max", p_max=p)
    rc, r = d_bspline(handle, pts, np.array([p]), n_max)
    assert rc == 0 and 6300 < r["count"][0] <= n_max
    _check_bspline(r, 0, pts[0])
    rc, outs = d_bspline(handle, pts, np.array([p]), n_max + 1)
    assert rc == REFUSED and all(o.untouched() for o in outs)


# =====================================================================================================================================
# pqp_dp_corridor
# =====================================================================================================================================
def _dp_scenes(n_scenes, n, seed0=50):
    """make_scene lines of ~(n - 1) 0.6 m + 8 m on one map geometry long enough for them"""
    length = (0.6 * (n - 1) + 30.0, 120.0)
    return [U.build(seed=seed0 + i, n=n, length=length) for i in range(n_scenes)]


def _check_dp(out, q, c, length, start):
    ls, lb, ub, count, vl = out
    # (a column-major copy of the layer: the restatement reads it through a column-major view)
    want = K.graph_search_dp(c["sx"], c["sy"], float(length), tuple(start), np.asfortranarray(c["dist"]), c["geom"])
    assert vl[q] == pytest.approx(want["vehicle_l"] if want else vl[q], abs=1e-12)
    if want is None:
        assert count[q] == 0
        return
    k = int(count[q])
    assert k == len(want["layers_s"])
    np.testing.assert_allclose(ls[q, :k], want["layers_s"], rtol=0, atol=1e-11)
    U.dp_bounds_agree(lb[q], ub[q], want, q)


def test_dp_corridor_long_lines_several_maps(handle):
    """lines of 60-200 m (several chunks of 32 layers), one map per scenario, max_layers past the 48 KiB point and at the last size under
    160 KiB; host == device; one layer more is refused"""
    cs = _dp_scenes(3, 340)
    g = cs[0]["geom"]
    m = max(c["tab"].shape[1] for c in cs)
    tab = np.stack([_pad_table(c["tab"], m) for c in cs]); ext = np.stack([c["ext"] for c in cs])
    lengths = np.array([60.0, 130.0, 199.0])
    start = np.array([[c["ref"][0, 3] + 0.2, c["ref"][0, 4] - 0.4, c["ref"][0, 2] + 0.05] for c in cs])
    dist = np.stack([c["dist"] for c in cs])
    nlat = U.dp_lateral_samples()
    assert U.dynamic_lds("dp_corridor_kernel", m=m, max_layers=140, nlat=nlat) > 48 * 1024
    top = U.largest("dp_corridor_kernel", "max_layers", m=m, nlat=nlat)
    for max_layers in (140, top):
        rc, *out = d_dp(handle, tab, ext, lengths, start, dist, capi_geom(g), max_layers, map_of=[0, 1, 2])
        assert rc == 0
        assert out[3].min() > 40
        h = handle.dp_corridor(tab, ext, lengths, start, dist, capi_geom(g), max_layers=max_layers, map_of=[0, 1, 2])
        assert np.array_equal(h[3], out[3]) and same_bytes(h[4], out[4])
        for j in range(3):
            host_equals_device(h[j], out[j], out[3], max_layers)
        if max_layers == top:
            for q, c in enumerate(cs):
                _check_dp(out, q, c, lengths[q], start[q])
    rc, outs = d_dp(handle, tab, ext, lengths, start, dist, capi_geom(g), top + 1, map_of=[0, 1, 2])
    assert rc == REFUSED and all(o.untouched() for o in outs)


# =====================================================================================================================================
# the capacity edge of every line kernel: the largest accepted size runs and matches the oracle, one element more is refused
# =====================================================================================================================================
def test_reference_states_and_segment_at_the_lds_edge(handle):
    rng = np.random.default_rng(21)
    m = 65
    line = smooth_line(rng, m, 2900.0)
    n_max = U.largest("reference_states_kernel", "n_max", m=m)
    assert n_max == (U.LDS_PER_CU - 16) // 8 - 9 * m
    tab, ext = line["tab"][None], line["ext"][None]
    rc, ref, count, _ = d_reference_states(handle, tab, ext, np.array([2900.0]), n_max)
    assert rc == 0 and count[0] > 9000
    _check_states(ref[0], int(count[0]), line, 2900.0, n_max)
    rc, seg = d_segment(handle, tab, ext, np.array([2900.0]), n_max)
    assert rc == 0
    _check_segment(seg, 0, line, 2900.0, n_max)
    rc, outs = d_reference_states(handle, tab, ext, np.array([2900.0]), n_max + 1)
    assert rc == REFUSED and all(o.untouched() for o in outs)
    rc, outs = d_segment(handle, tab, ext, np.array([2900.0]), n_max + 1)
    assert rc == REFUSED and all(o.untouched() for o in outs)
    # the most knots with one state
    m_top = U.largest("reference_states_kernel", "m", n_max=1)
    line = smooth_line(rng, m_top, 3000.0)
    rc, ref, count, _ = d_reference_states(handle, line["tab"][None], line["ext"][None], np.array([0.5]), 1)
    assert rc == 0 and count[0] >= 2
    _check_states(ref[0], int(count[0]), line, 0.5, 1)


def test_reference_length_and_offsets_at_the_lds_edge(handle):
    rng = np.random.default_rng(22)
    m = U.largest("reference_length_kernel", "m")
    assert m == 2275
    line = smooth_line(rng, m, 2000.0, lo=0.1, hi=3.0)
    tgt = np.array([_target(line, 1733.3, 1.2)])
    rc, got = d_reference_length(handle, line["tab"][None], line["ext"][None], np.array([2000.0]), tgt)
    assert rc == 0
    assert got[0] == pytest.approx(K.reference_length(line["sx"], line["sy"], 2000.0, tgt[0, 0], tgt[0, 1]), abs=1e-9)
    wide = smooth_line(rng, m + 1, 2000.0)
    rc, out = d_reference_length(handle, wide["tab"][None], wide["ext"][None], np.array([2000.0]), tgt)
    assert rc == REFUSED and out.untouched()
    # offsets: the largest m for a table of 1000 knots, then one more
    ms = 1000
    mp = U.largest("offsets_to_points_kernel", "m", m_spline=ms)
    assert 9 * ms + 2 * mp == U.LDS_PER_CU // 8
    line = smooth_line(rng, ms, 1500.0)
    at_s = np.linspace(0.0, 1500.0, mp)[None]
    l = rng.uniform(-10.0, 10.0, (1, mp))
    rc, x, y, s = d_offsets(handle, line["tab"][None], line["ext"][None], at_s, l)
    assert rc == 0
    wx, wy, ws = K.offsets_to_points(line["sx"], line["sy"], at_s[0], l[0])
    close(x[0], wx, 1e-11, "x"); close(y[0], wy, 1e-11, "y")
    np.testing.assert_allclose(s[0], ws, rtol=0, atol=1e-10 * ws[-1] / 30.0)
    rc, outs = d_offsets(handle, line["tab"][None], line["ext"][None], np.linspace(0.0, 1500.0, mp + 1)[None], np.zeros((1, mp + 1)))
    assert rc == REFUSED and all(o.untouched() for o in outs)


# =====================================================================================================================================
# batches of 1024: host == device, permutation, padded tables == exact tables, oracle on a subset
# =====================================================================================================================================
@pytest.fixture(scope="module")
def var_batch(hip_lib):
    """1024 smooth lines of 20-129 knots fitted in one pqp_spline_fit_var_device call (m_max 129), with their exact-size tables"""
    rng = np.random.default_rng(2024)
    B, m_max = 1024, 129
    proto = [smooth_line(rng, m, 0.8 * m + 20.0, lo=0.05, hi=3.0) for m in (20, 63, 64, 65, 100, 129)]
    pick = rng.integers(0, len(proto), B)
    m_of = np.array([len(proto[i]["s"]) for i in pick], dtype=np.int32)
    s = np.zeros((B, m_max)); x = np.zeros((B, m_max)); y = np.zeros((B, m_max))
    shift = rng.uniform(-5.0, 5.0, (B, 2))
    for q, i in enumerate(pick):
        n = m_of[q]
        s[q, :n], x[q, :n], y[q, :n] = proto[i]["s"], proto[i]["x"] + shift[q, 0], proto[i]["y"] + shift[q, 1]
    h = capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=128)
    rc, tab, ext = d_spline_fit(h, s, x, y, m_of=m_of)
    assert rc == 0
    exact = {}
    for n in sorted(set(m_of.tolist())):
        idx = np.nonzero(m_of == n)[0]
        rc, ft, fe = d_spline_fit(h, s[idx, :n], x[idx, :n], y[idx, :n])
        assert rc == 0
        exact[n] = (idx, ft, fe)
    lines = [dict(length=float(s[q, m_of[q] - 1])) for q in range(B)]
    yield dict(B=B, m_max=m_max, m_of=m_of, s=s, x=x, y=y, tab=tab, ext=ext, exact=exact, lines=lines, rng=rng)
    h.close()


def _oracle_line(vb, q):
    n = int(vb["m_of"][q])
    return dict(sx=K.spline_fit(vb["s"][q, :n], vb["x"][q, :n]), sy=K.spline_fit(vb["s"][q, :n], vb["y"][q, :n]))


SUBSET = np.random.default_rng(99).choice(1024, 16, replace=False)


def test_batch_reference_states_and_segment(handle, var_batch):
    vb = var_batch
    B, tab, ext = vb["B"], vb["tab"], vb["ext"]
    L = np.array([l["length"] for l in vb["lines"]])
    max_s = L * np.random.default_rng(1).uniform(0.3, 1.2, B)
    n_max = 600
    start = np.column_stack([vb["x"][:, 0] + 0.3, vb["y"][:, 0] - 0.2, np.random.default_rng(2).uniform(-np.pi, np.pi, B)])
    rc, ref, count, err = d_reference_states(handle, tab, ext, max_s, n_max, start=start)
    assert rc == 0
    href, hcount, herr = handle.reference_states(tab, ext, max_s, n_max, start=start)
    assert np.array_equal(hcount, count) and same_bytes(herr, err)
    host_equals_device(href, ref, count, n_max)
    perm = np.random.default_rng(3).permutation(B)
    rc, pref, pcount, perr = d_reference_states(handle, tab[perm], ext[perm], max_s[perm], n_max, start=start[perm])
    assert rc == 0 and same_bytes(pref, ref[perm]) and np.array_equal(pcount, count[perm]) and same_bytes(perr, err[perm])
    # the padded tables against the exact-size ones
    for n, (idx, ft, fe) in vb["exact"].items():
        rc, eref, ecount, eerr = d_reference_states(handle, ft, fe, max_s[idx], n_max, start=start[idx])
        assert rc == 0 and np.array_equal(ecount, count[idx]) and same_bytes(eerr, err[idx]) and same_bytes(eref, ref[idx])
    for q in SUBSET:
        line = _oracle_line(vb, q)
        _check_states(ref[q], int(count[q]), line, max_s[q], n_max)
        off, dpsi = K.process_init_state(line["sx"], line["sy"], *start[q])
        assert err[q, 0] == pytest.approx(off, abs=1e-12) and err[q, 1] == pytest.approx(dpsi, abs=1e-12)
    # segment_raw_reference
    n_seg = 200
    rc, seg = d_segment(handle, tab, ext, max_s, n_seg)
    assert rc == 0
    hseg = handle.segment_raw_reference(tab, ext, max_s, n_seg)
    for key in SEG_KEYS:
        host_equals_device(hseg[key], seg[key], seg["count"], n_seg)
    rc, pseg = d_segment(handle, tab[perm], ext[perm], max_s[perm], n_seg)
    assert rc == 0 and all(same_bytes(pseg[k], seg[k][perm]) for k in SEG_KEYS + ("count",))
    for n, (idx, ft, fe) in vb["exact"].items():
        rc, eseg = d_segment(handle, ft, fe, max_s[idx], n_seg)
        assert rc == 0 and all(same_bytes(eseg[k], seg[k][idx]) for k in SEG_KEYS + ("count",))
    for q in SUBSET:
        _check_segment(seg, q, _oracle_line(vb, q), max_s[q], n_seg)


def test_batch_reference_length_and_offsets(handle, var_batch):
    vb = var_batch
    B, tab, ext = vb["B"], vb["tab"], vb["ext"]
    rng = np.random.default_rng(8)
    L = np.array([l["length"] for l in vb["lines"]])
    # targets near the line at a random abscissa (some past the end)
    frac = rng.uniform(0.0, 1.15, B)
    target = np.zeros((B, 3))
    for q in range(B):
        n = int(vb["m_of"][q])
        sq = min(frac[q] * L[q], L[q])
        target[q, 0] = np.interp(sq, vb["s"][q, :n], vb["x"][q, :n]) + rng.uniform(-2, 2) + (5.0 if frac[q] > 1.0 else 0.0)
        target[q, 1] = np.interp(sq, vb["s"][q, :n], vb["y"][q, :n]) + rng.uniform(-2, 2)
    rc, got = d_reference_length(handle, tab, ext, L, target)
    assert rc == 0
    assert same_bytes(handle.reference_length(tab, ext, L, target), got)
    perm = rng.permutation(B)
    rc, pgot = d_reference_length(handle, tab[perm], ext[perm], L[perm], target[perm])
    assert rc == 0 and same_bytes(pgot, got[perm])
    for n, (idx, ft, fe) in vb["exact"].items():
        rc, egot = d_reference_length(handle, ft, fe, L[idx], target[idx])
        assert rc == 0 and same_bytes(egot, got[idx])
    for q in SUBSET:
        line = _oracle_line(vb, q)
        assert got[q] == pytest.approx(K.reference_length(line["sx"], line["sy"], L[q], target[q, 0], target[q, 1]), abs=1e-9)
    # offsets_to_points on the same tables: ragged m_of, abscissae up to 10 m past the end
    m = 96
    at_s = np.sort(rng.uniform(0.0, 1.0, (B, m)), axis=1) * (L[:, None] + 10.0)
    l = rng.uniform(-10.0, 10.0, (B, m))
    m_of = rng.integers(1, m + 1, B).astype(np.int32)
    rc, x, y, s = d_offsets(handle, tab, ext, at_s, l, m_of)
    assert rc == 0
    hx, hy, hs = handle.offsets_to_points(tab, ext, at_s, l, m_of=m_of)
    for h_, d_ in ((hx, x), (hy, y), (hs, s)):
        host_equals_device(h_, d_, m_of, m)
    rc, px, py, ps = d_offsets(handle, tab[perm], ext[perm], at_s[perm], l[perm], m_of[perm])
    assert rc == 0 and same_bytes(px, x[perm]) and same_bytes(py, y[perm]) and same_bytes(ps, s[perm])
    for n, (idx, ft, fe) in vb["exact"].items():
        rc, ex, ey, es = d_offsets(handle, ft, fe, at_s[idx], l[idx], m_of[idx])
        assert rc == 0 and same_bytes(ex, x[idx]) and same_bytes(ey, y[idx]) and same_bytes(es, s[idx])
    for q in SUBSET:
        k = int(m_of[q])
        line = _oracle_line(vb, q)
        wx, wy, ws = K.offsets_to_points(line["sx"], line["sy"], at_s[q, :k], l[q, :k])
        close(x[q, :k], wx, 1e-11, "x"); close(y[q, :k], wy, 1e-11, "y")
        np.testing.assert_allclose(s[q, :k], ws, rtol=0, atol=1e-10 * max(1.0, ws[-1] / 30.0))


def test_batch_bspline_resample(handle):
    rng = np.random.default_rng(31)
    B, p_max, n_max = 1024, 40, 500
    n_pts = rng.integers(2, p_max + 1, B).astype(np.int32)
    spacing = rng.choice([2.0, 4.0, 6.0, 8.0, 12.0, 16.0], B)
    pts = np.cumsum(np.stack([np.column_stack([np.full(p_max, sp), rng.uniform(-0.3, 0.3, p_max) * sp]) for sp in spacing]), axis=1)
    pts += rng.uniform(-50, 50, (B, 1, 2))
    rc, r = d_bspline(handle, pts, n_pts, n_max)
    assert rc == 0
    assert np.all(r["count"][n_pts < 4] == 0) and np.any(r["count"] > n_max)
    assert all(r["count"][q] == 0 for q in range(B) if 4 <= n_pts[q] <= _degree(pts[q, :n_pts[q]]))
    h = handle.bspline_resample(pts, n_pts, n_max)
    assert np.array_equal(h["count"], r["count"])
    for key in ("x", "y", "s"):
        host_equals_device(h[key], r[key], r["count"], n_max)
    perm = rng.permutation(B)
    rc, pr = d_bspline(handle, pts[perm], n_pts[perm], n_max)
    assert rc == 0 and all(same_bytes(pr[k], r[k][perm]) for k in ("x", "y", "s", "count"))
    for q in SUBSET:
        if n_pts[q] >= 4 and r["count"][q] <= n_max:
            _check_bspline(r, q, pts[q, :n_pts[q]])


def test_batch_dp_corridor_and_corridor_bounds_on_padded_tables(handle):
    """1024 DP searches over 4 maps on padded tables against the exact-size ones (and corridor_bounds likewise), permuted, host == device,
    the oracle on a subset"""
    cs = _dp_scenes(4, 200, seed0=70)
    g = cs[0]["geom"]
    dist = np.stack([c["dist"] for c in cs])
    B, rng = 1024, np.random.default_rng(41)
    map_of = rng.integers(0, 4, B).astype(np.int32)
    m_max = max(c["tab"].shape[1] for c in cs) + 17
    tab = np.stack([_pad_table(cs[i]["tab"], m_max) for i in map_of]); ext = np.stack([cs[i]["ext"] for i in map_of])
    lengths = rng.uniform(60.0, 110.0, B)
    start = np.array([[cs[i]["ref"][0, 3] + rng.uniform(-0.5, 0.5), cs[i]["ref"][0, 4] + rng.uniform(-1.0, 1.0), cs[i]["ref"][0, 2] + rng.uniform(-0.1, 0.1)]
                      for i in map_of])
    max_layers = 96
    rc, *out = d_dp(handle, tab, ext, lengths, start, dist, capi_geom(g), max_layers, map_of=map_of)
    assert rc == 0 and np.all(out[3] > 0)
    hout = handle.dp_corridor(tab, ext, lengths, start, dist, capi_geom(g), max_layers=max_layers, map_of=map_of)
    assert np.array_equal(hout[3], out[3]) and same_bytes(hout[4], out[4])
    for j in range(3):
        host_equals_device(hout[j], out[j], out[3], max_layers)
    perm = rng.permutation(B)
    rc, *pout = d_dp(handle, tab[perm], ext[perm], lengths[perm], start[perm], dist, capi_geom(g), max_layers, map_of=map_of[perm])
    assert rc == 0 and all(same_bytes(pout[j], out[j][perm]) for j in range(5))
    for i, c in enumerate(cs):
        idx = np.nonzero(map_of == i)[0]
        rc, *eout = d_dp(handle, np.repeat(c["tab"][None], len(idx), 0), ext[idx], lengths[idx], start[idx], dist, capi_geom(g), max_layers, map_of=map_of[idx])
        assert rc == 0 and all(same_bytes(eout[j], out[j][idx]) for j in range(5))
    for q in SUBSET[:8]:
        _check_dp(out, q, cs[map_of[q]], lengths[q], start[q])
    # corridor_bounds on the same padded / exact tables (reference states of each line first)
    n = 128
    rc, ref, count, _ = d_reference_states(handle, tab, ext, lengths, n)
    assert rc == 0
    n_of = np.minimum(count, n).astype(np.int32)
    b, nv = d_bounds(handle, ref, n_of, tab, ext, dist, capi_geom(g), map_of)
    for i, c in enumerate(cs):
        idx = np.nonzero(map_of == i)[0]
        eb, env = d_bounds(handle, ref[idx], n_of[idx], np.repeat(c["tab"][None], len(idx), 0), ext[idx], dist, capi_geom(g), map_of[idx])
        assert np.array_equal(env, nv[idx]) and same_bytes(eb, b[idx])
