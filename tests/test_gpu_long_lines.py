"""PQP_OPT_LONG_LINES: the line-geometry steps and the chain on lines longer than their LDS kernels take (the long forms of
pqp_corridor_kernels.inc: one source text per kernel, compiled once for the LDS and once for the long form).
Past the LDS edge (option 1) every entry point runs and matches oracle/corridor_oracle.py as the edge tests of test_gpu_line_geometry.py
do; where both forms run, the long form (option 2) gives the LDS form's bits; option 1 below the edge is the LDS launch; option 0 still
refuses.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import corridor_oracle as K
import corridor_util as U
import long_line_util as LL
from chain_util import scenarios, smoother_params, steps_one_by_one
from device_form import (d_bounds, d_bspline, d_dp, d_offsets, d_reference_length, d_reference_states, d_segment, d_spline_fit,
                         host_equals_device)
from line_cases import (REFUSED, SPLINE_SIZES, SEG_KEYS, _check_bspline, _check_segment, _check_states, check_spline_table, close, smooth_line,
                        walk)
from path_optimizer_2_amd import capi
from shared_util import same_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(hip_lib):
    """one handle per option value"""
    hs = {v: LL.with_option(capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=128), v) for v in (0, 1, 2)}
    yield hs
    for h in hs.values():
        h.close()


def _same_all(a, b):
    if isinstance(a, dict):
        return all(same_bytes(a[k], b[k]) for k in a)
    return all(same_bytes(x, y) for x, y in zip(a, b))


# ---- 1 + 4: past the edge and well beyond under option 1; option 0 refuses the same inputs ---------------------------------------------------
@pytest.mark.parametrize("m", [2926, 8800])
def test_spline_fit_past_the_edge(handles, m):
    rng = np.random.default_rng(m)
    knots = [walk(rng, m), walk(rng, m, 0.2, 3.0)]
    s, x, y = (np.stack([k[i] for k in knots]) for i in range(3))
    rc, tab, ext = d_spline_fit(handles[1], s, x, y)
    assert rc == 0
    htab, hext = handles[1].spline_fit(s, x, y)
    assert same_bytes(htab, tab) and same_bytes(hext, ext)
    lib = U.ref_spline_lib()
    for q in range(2):
        check_spline_table(tab[q], ext[q], s[q], x[q], y[q], lib if q == 1 else None)
    # _var on the same knots, padded: the real rows are the fixed fit's
    m_of = np.array([m, m - 700], dtype=np.int32)
    rc, vtab, vext = d_spline_fit(handles[1], s, x, y, m_of=m_of)
    assert rc == 0 and same_bytes(vtab[0], tab[0]) and same_bytes(vext[0], ext[0])
    rc, t1, e1 = d_spline_fit(handles[1], s[1:, :m - 700], x[1:, :m - 700], y[1:, :m - 700])
    assert rc == 0 and same_bytes(vtab[1, :, :m - 700], t1[0]) and same_bytes(vext[1], e1[0])
    rc, t0, e0 = d_spline_fit(handles[0], s, x, y)
    assert rc == REFUSED and t0.untouched() and e0.untouched()


@pytest.mark.parametrize("scale", [1, 3])
def test_reference_states_and_segment_past_the_edge(handles, scale):
    rng = np.random.default_rng(31 + scale)
    m = 65
    line = smooth_line(rng, m, 2900.0 * scale)
    edge = U.largest("reference_states_kernel", "n_max", m=m)
    n_max = edge + 1 if scale == 1 else 3 * edge
    tab, ext, max_s = line["tab"][None], line["ext"][None], np.array([2900.0 * scale])
    h = handles[1]
    rc, ref, count, _ = d_reference_states(h, tab, ext, max_s, n_max)
    assert rc == 0
    href, hcount, _ = h.reference_states(tab, ext, max_s, n_max)
    assert np.array_equal(hcount, count)
    host_equals_device(href, ref, count, n_max)
    _check_states(ref[0], int(count[0]), line, max_s[0], n_max)
    rc, seg = d_segment(h, tab, ext, max_s, n_max)
    assert rc == 0
    hseg = h.segment_raw_reference(tab, ext, max_s, n_max)
    for key in SEG_KEYS:
        host_equals_device(hseg[key], seg[key], seg["count"], n_max)
    _check_segment(seg, 0, line, max_s[0], n_max)
    rc, outs = d_reference_states(handles[0], tab, ext, max_s, n_max)
    assert rc == REFUSED and all(o.untouched() for o in outs)
    rc, outs = d_segment(handles[0], tab, ext, max_s, n_max)
    assert rc == REFUSED and all(o.untouched() for o in outs)
    # knots past the edge with one state
    m_top = U.largest("reference_states_kernel", "m", n_max=1)
    wide = smooth_line(rng, (m_top + 1) * scale, 3000.0 * scale)
    rc, ref, count, _ = d_reference_states(h, wide["tab"][None], wide["ext"][None], np.array([0.5]), 1)
    assert rc == 0
    _check_states(ref[0], int(count[0]), wide, 0.5, 1)


@pytest.mark.parametrize("scale", [1, 3])
def test_reference_length_and_offsets_past_the_edge(handles, scale):
    rng = np.random.default_rng(41 + scale)
    m = (U.largest("reference_length_kernel", "m") + 1) * scale
    line = smooth_line(rng, m, 2000.0 * scale, lo=0.1, hi=3.0)
    tgts = []
    for s_t in (0.4 * line["length"], 0.87 * line["length"]):
        x, y = K.spline_eval(line["sx"], s_t), K.spline_eval(line["sy"], s_t)
        tgts.append([x + 0.7, y - 1.1, 0.0])
    tgt = np.array(tgts)
    tab, ext = np.stack([line["tab"]] * 2), np.stack([line["ext"]] * 2)
    L = np.array([line["length"]] * 2)
    rc, got = d_reference_length(handles[1], tab, ext, L, tgt)
    assert rc == 0
    assert same_bytes(handles[1].reference_length(tab, ext, L, tgt), got)
    for q in range(2):
        assert got[q] == pytest.approx(K.reference_length(line["sx"], line["sy"], L[q], tgt[q, 0], tgt[q, 1]), abs=1e-9)
    rc, out = d_reference_length(handles[0], tab, ext, L, tgt)
    assert rc == REFUSED and out.untouched()
    # offsets: a table of 1000 knots and one point more than the LDS form takes (x scale)
    ms = 1000
    mp = (U.largest("offsets_to_points_kernel", "m", m_spline=ms) + 1) * scale
    line = smooth_line(rng, ms, 1500.0)
    at_s = np.linspace(0.0, 1500.0, mp)[None]
    l = rng.uniform(-10.0, 10.0, (1, mp))
    rc, x, y, s = d_offsets(handles[1], line["tab"][None], line["ext"][None], at_s, l)
    assert rc == 0
    hx, hy, hs = handles[1].offsets_to_points(line["tab"][None], line["ext"][None], at_s, l)
    assert same_bytes(hx, x) and same_bytes(hy, y) and same_bytes(hs, s)
    wx, wy, ws = K.offsets_to_points(line["sx"], line["sy"], at_s[0], l[0])
    close(x[0], wx, 1e-11, "x"); close(y[0], wy, 1e-11, "y")
    np.testing.assert_allclose(s[0], ws, rtol=0, atol=1e-10 * ws[-1] / 30.0)
    rc, outs = d_offsets(handles[0], line["tab"][None], line["ext"][None], at_s, l)
    assert rc == REFUSED and all(o.untouched() for o in outs)


@pytest.mark.parametrize("scale", [1, 3])
def test_bspline_resample_past_the_edge(handles, scale):
    rng = np.random.default_rng(51 + scale)
    p = 65 * scale
    pts = np.cumsum(np.column_stack([np.full(p, 100.0), rng.uniform(-20.0, 20.0, p)]), axis=0)[None]
    n_max = (U.largest("bspline_resample_kernel", "n_max", p_max=p) + 1) * (1 if scale == 1 else 3)
    rc, r = d_bspline(handles[1], pts, np.array([p]), n_max)
    assert rc == 0 and r["count"][0] > 6000 * scale
    hr = handles[1].bspline_resample(pts, np.array([p], dtype=np.int32), n_max)
    for k in ("x", "y", "s"):
        host_equals_device(hr[k], r[k], r["count"], n_max)
    _check_bspline(r, 0, pts[0])
    rc, outs = d_bspline(handles[0], pts, np.array([p]), n_max)
    assert rc == REFUSED and all(o.untouched() for o in outs)


def _road_dp(road, line, start, max_layers, h):
    return d_dp(h, line["tab"][None], line["ext"][None], np.array([line["length"]]), start[None], road["dist"][None], road["geom"], max_layers)


@pytest.mark.parametrize("length", [900.0, 2700.0])
def test_dp_corridor_past_the_edge(handles, length):
    """a smoothed line (1 m knots) of 900 m - just past the LDS form's ~880 m - and of 2.7 km on a map along it, against the oracle"""
    road = LL.long_road(length, seed=int(length))
    line = LL.road_spline(road)
    start = np.array([road["x"][0] + 0.2, road["y"][0] - 0.3, 0.05])
    max_layers = int(length / 1.5) + 8
    nlat = U.dp_lateral_samples()
    assert not U.fits("dp_corridor_kernel", m=line["tab"].shape[1], max_layers=max_layers, nlat=nlat)
    rc, *out = _road_dp(road, line, start, max_layers, handles[1])
    assert rc == 0 and out[3][0] > 0.9 * length / 1.5
    h = handles[1].dp_corridor(line["tab"][None], line["ext"][None], np.array([line["length"]]), start[None], road["dist"][None], road["geom"],
                               max_layers=max_layers)
    assert np.array_equal(h[3], out[3]) and same_bytes(h[4], out[4])
    for j in range(3):
        host_equals_device(h[j], out[j], out[3], max_layers)
    want = K.graph_search_dp(line["sx"], line["sy"], line["length"], tuple(start), np.asfortranarray(road["dist"]), road["kgeom"])
    ls, lb, ub, count, vl = out
    k = int(count[0])
    assert k == len(want["layers_s"])
    np.testing.assert_allclose(ls[0, :k], want["layers_s"], rtol=0, atol=1e-9)
    U.dp_bounds_agree(lb[0], ub[0], want, length)
    rc, outs = _road_dp(road, line, start, max_layers, handles[0])
    assert rc == REFUSED and all(o.untouched() for o in outs)


def _road_ref(road, line, h):
    n_max = int(line["length"] / 0.15) + 8                # (the walk's smallest step: every state fits)
    rc, ref, count, _ = d_reference_states(h, line["tab"][None], line["ext"][None], np.array([line["length"]]), n_max)
    assert rc == 0 and count[0] <= n_max
    return ref, count


@pytest.mark.parametrize("length", [2300.0, 6700.0])
def test_corridor_bounds_past_the_edge(handles, length):
    """corridor bounds along a road whose spline table (1 m knots) is past the LDS form's ~2210 knots, and 3x that; the oracle on every
    97th waypoint (each waypoint's walk is its own)"""
    road = LL.long_road(length, seed=7 + int(length))
    line = LL.road_spline(road)
    assert line["tab"].shape[1] > 2210
    ref, count = _road_ref(road, line, handles[1])
    n = int(count[0])
    ref = ref[:, :n].copy()
    n_of = np.array([n], dtype=np.int32)
    bounds, nv = d_bounds(handles[1], ref, n_of, line["tab"][None], line["ext"][None], road["dist"][None], road["geom"])
    hb, hnv = handles[1].corridor_bounds(ref, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
    assert np.array_equal(hnv, nv) and same_bytes(hb, bounds)
    fdist = np.asfortranarray(road["dist"])              # (the oracle reads the layer through a column-major view)
    k = int(nv[0])
    assert k > 1000
    if k < n:                                            # the waypoint where the road is blocked is the oracle's
        _, n_valid, blocked = K.update_bounds_improved(ref[0, k:k + 1], line["sx"], line["sy"], fdist, road["kgeom"])
        assert n_valid == 0 and blocked is not None
        assert np.abs(bounds[0, k] - np.array(blocked)).max() < 1e-9
    sub = np.arange(0, k, 97)
    want, n_valid, blocked = K.update_bounds_improved(ref[0, sub], line["sx"], line["sy"], fdist, road["kgeom"])
    assert n_valid == len(sub) and blocked is None
    diff = np.abs(bounds[0, sub] - want)
    exact = diff < 1e-9
    assert exact.mean() > 0.99, exact.mean()
    for d in diff[~exact]:
        assert min(abs(d - 0.05 * k) for k in range(1, 8)) < 1e-9 or min(abs(d - 0.3 * k) for k in range(1, 4)) < 1e-9, d
    # on states: d_heading 0 everywhere is the plain walk (front / rear lengths scale by 1 - cos 0 = 0: the centres sit on the states)
    st = np.zeros((1, n, 7))
    st[0, :, 4] = np.random.default_rng(3).uniform(-0.3, 0.3, n)
    b2, nv2 = handles[1].corridor_bounds_on_states(ref, st, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
    b2l, nv2l = handles[2].corridor_bounds_on_states(ref, st, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
    assert same_bytes(b2, b2l) and np.array_equal(nv2, nv2l)
    with pytest.raises(capi.PqpError, match="pqp error -4:"):
        handles[0].corridor_bounds(ref, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
    with pytest.raises(capi.PqpError, match="pqp error -4:"):
        handles[0].corridor_bounds_on_states(ref, st, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)


# ---- 2 + 3: where both forms run, the long form's bits are the LDS form's; option 1 below the edge is the LDS launch -------------------------
@pytest.mark.parametrize("m", SPLINE_SIZES)
def test_spline_fit_long_form_bits(handles, m):
    rng = np.random.default_rng(500 + m)
    knots = [walk(rng, m) for _ in range(3)]
    s, x, y = (np.stack([k[i] for k in knots]) for i in range(3))
    m_of = np.array([m, max(1, m - 2), 2], dtype=np.int32)
    for mo in (None, m_of):
        got = {v: d_spline_fit(handles[v], s, x, y, m_of=mo) for v in (0, 1, 2)}
        assert got[0][0] == got[1][0] == got[2][0] == 0
        assert same_bytes(got[0][1], got[2][1]) and same_bytes(got[0][2], got[2][2])
        assert same_bytes(got[0][1], got[1][1]) and same_bytes(got[0][2], got[1][2])


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_golden_scenes_long_form_bits(handles, name):
    import os
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", f"{name}.npz"))
    tab, ext = f["spline"][None], f["spline_ext"][None]
    g = capi.PqpGridGeometry(*[int(v) if i < 2 else float(v) for i, v in enumerate(f["geom"])])
    start = f["start"][None]
    L = np.array([float(f["length"])])
    res = {}
    for v in (0, 1, 2):
        h = handles[v]
        ref, count, err = h.reference_states(tab, ext, L, 200, start=start)
        n_of = np.minimum(count, 200).astype(np.int32)
        bounds, nv = h.corridor_bounds(ref, tab, ext, f["dist"], g, n_of=n_of)
        dp = h.dp_corridor(tab, ext, L, start, f["dist"], g, max_layers=64)
        seg = h.segment_raw_reference(tab, ext, L, 64)
        rl = h.reference_length(tab, ext, L, np.array([[ref[0, 10, 3], ref[0, 10, 4] + 0.5, 0.0]]))
        res[v] = [ref, count, err, bounds, nv, *dp, *(seg[k] for k in sorted(seg)), rl]
    assert _same_all(res[0], res[2]) and _same_all(res[0], res[1])


def test_batch_of_1024_long_form_bits(handles):
    """1024 ragged lines: padded _var tables, every line kernel, option 2 against option 0 bit for bit"""
    rng = np.random.default_rng(77)
    B, m_max = 1024, 129
    m_of = rng.integers(3, m_max + 1, B).astype(np.int32)
    s = np.zeros((B, m_max)); x = np.zeros((B, m_max)); y = np.zeros((B, m_max))
    for q in range(B):
        n = m_of[q]
        ln = smooth_line(rng, n, 0.8 * n + 20.0, lo=0.05, hi=3.0)
        s[q, :n], x[q, :n], y[q, :n] = ln["s"], ln["x"], ln["y"]
    L = s[np.arange(B), m_of - 1]
    at_s = np.sort(rng.uniform(0.0, 1.0, (B, 100)), axis=1) * L[:, None]
    l = rng.uniform(-3.0, 3.0, (B, 100))
    tgt = np.column_stack([x[np.arange(B), m_of // 2], y[np.arange(B), m_of // 2] + 0.4, np.zeros(B)])
    pts = np.stack([np.column_stack([s[q, :40] * 3.0, x[q, :40]]) for q in range(B)])
    n_pts = np.minimum(m_of, 40).astype(np.int32)
    res = {}
    for v in (0, 2):
        h = handles[v]
        rc, tab, ext = d_spline_fit(h, s, x, y, m_of=m_of)
        assert rc == 0
        rc, ref, count, _ = d_reference_states(h, tab, ext, L * 1.1, 300)
        assert rc == 0
        rc, seg = d_segment(h, tab, ext, L, 200)
        assert rc == 0
        rc, rl = d_reference_length(h, tab, ext, L, tgt)
        assert rc == 0
        rc, ox, oy, os_ = d_offsets(h, tab, ext, at_s, l)
        assert rc == 0
        rc, bs = d_bspline(h, pts, n_pts, 400)
        assert rc == 0
        res[v] = [tab, ext, ref, count, *(seg[k] for k in sorted(seg)), rl, ox, oy, os_, *(bs[k] for k in sorted(bs))]
    assert _same_all(res[0], res[2])


def test_dp_and_corridor_on_states_long_form_bits(handles):
    """the DP and the corridor (plain and on states) on a few hundred metres of road: option 2 == option 0 == option 1"""
    road = LL.long_road(400.0, seed=3)
    line = LL.road_spline(road)
    start = np.array([road["x"][0] + 0.2, road["y"][0] - 0.3, 0.05])
    ref, count = _road_ref(road, line, handles[0])
    n = int(count[0])
    ref = ref[:, :n].copy()
    n_of = np.array([n], dtype=np.int32)
    st = np.zeros((1, n, 7))
    st[0, :, 4] = np.random.default_rng(4).uniform(-0.4, 0.4, n)
    st[0, 5, 4] = np.nan                                  # a non-finite d_heading: NaN front / rear rows, as in the LDS form
    res = {}
    for v in (0, 1, 2):
        rc, *dp = _road_dp(road, line, start, 300, handles[v])
        assert rc == 0
        b1 = handles[v].corridor_bounds(ref, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
        b2 = handles[v].corridor_bounds_on_states(ref, st, line["tab"][None], line["ext"][None], road["dist"], road["geom"], n_of=n_of)
        res[v] = [*dp, *b1, *b2]
    assert _same_all(res[0], res[2]) and _same_all(res[0], res[1])


# ---- 5: the chain on lines of 1.5 - 2.5 km ------------------------------------------------------------------------------------------
def _long_scenarios(B, seed=11):
    """B scenarios of 1.5 - 2.5 km along one 2.5 km road (its map serves all of them): the road's points every 20 m, cut at a random
    length, with a little lateral noise"""
    road = LL.long_road(2500.0, seed=seed + 2)
    rng = np.random.default_rng(seed)
    full, _, _ = LL.road_points(road, 20.0)
    p_max = len(full)
    pts = np.zeros((B, p_max, 2)); n_pts = np.zeros(B, dtype=np.int32); start = np.zeros((B, 3)); target = np.zeros((B, 3))
    for b in range(B):
        k = int(float(rng.uniform(1500.0, 2500.0)) // 20) + 1
        p = full[:k].copy()
        p[:, 1] += rng.normal(scale=0.15, size=k)
        n_pts[b] = k
        pts[b, :k] = p
        start[b] = (p[0, 0] + 0.1, p[0, 1] + 0.1, np.arctan2(p[1, 1] - p[0, 1], p[1, 0] - p[0, 0]) + 0.02)
        target[b] = (p[-1, 0], p[-1, 1], np.arctan2(p[-1, 1] - p[-2, 1], p[-1, 0] - p[-2, 0]))
    return dict(pts=pts, n_pts=n_pts, map_of=np.zeros(B, dtype=np.int32), start=start, target=target, dist=road["dist"][None], geom=road["geom"])


@pytest.mark.parametrize("method", [capi.SMOOTHING_TENSION2, capi.SMOOTHING_TENSION])
def test_chain_on_long_lines(hip_lib, method):
    """the chain under option 1 on 1.5 - 2.5 km lines against the same steps run one scenario at a time, every scenario: the stage it
    stops at and the QP status, and the path where one comes out.  The line steps never stop a scenario; the QPs do at these lengths - the
    TensionSmoother QP of 1500+ samples does not converge, the path QP of 3000-5000 waypoints mostly fails - and the
    one-scenario run must stop at the same step.  (A TensionSmoother QP that fails runs to its iteration limit, ~20 s for one scenario at
    these sizes: two of the scenarios the chain stops there are rerun, every other one is)"""
    B = 10
    sc = _long_scenarios(B)
    h = LL.with_option(capi.Handle(capi.production_params(), max_batch=B, max_n=5200), 1)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=2700)
    cfg = h.chain_config(raw_max=2700, sample_max=2700, layer_max=1800, n_max=5200, output_spacing=1.0, smoothing_method=method)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    assert not (got["stage"] == 9).any(), got["stage"]
    compared = smoother_failed = 0
    for b in range(B):
        if got["stage"][b] == 2:
            smoother_failed += 1
            if smoother_failed > 2:
                continue
        want = steps_one_by_one(h, hs, sc, b, cfg)
        assert got["stage"][b] == want["stage"] and got["status"][b] == want["status"], (b, got["stage"][b], want)
        if want["stage"] == 0:
            nv = want["nv"]
            assert got["n_out"][b] == nv
            assert np.abs(got["out"][b, :nv] - want["out"][:nv]).max() < 2e-5, (b, np.abs(got["out"][b, :nv] - want["out"][:nv]).max())
            assert np.all(got["out"][b, nv:] == 0.0)
            compared += 1
    if method == capi.SMOOTHING_TENSION2:
        assert compared >= 1, got["stage"]                 # at least one open road solved end to end, path compared
    h0 = LL.with_option(capi.Handle(capi.production_params(), max_batch=B, max_n=5200), 0)
    with pytest.raises(capi.PqpError, match="pqp error -4:"):
        h0.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    h.close(); hs.close(); h0.close()


def test_chain_short_lines_option_1_is_option_0(hip_lib):
    B = 16
    sc = scenarios(B)
    outs = []
    for opt in (0, 1):
        for graph in (0, 1):
            h = LL.with_option(capi.Handle(capi.production_params(), max_batch=B, max_n=256), opt)
            h.set_option(capi.OPT_CHAIN_GRAPH, graph)
            hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
            for _ in range(4 if graph else 1):           # plain, plain, capture, replay
                got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs)
            outs.append(got)
            h.close(); hs.close()
    for o in outs[1:]:
        assert all(same_bytes(outs[0][k], o[k]) for k in outs[0])


# ---- 6: a NaN knot and an Inf abscissa in one scenario of a long-form batch ------------------------------------------------------------
def test_hostile_scenario_leaves_its_neighbours_alone(handles):
    rng = np.random.default_rng(66)
    B, m = 4, 3000
    lines = [smooth_line(rng, m, 2500.0, lo=0.2, hi=3.0) for _ in range(B)]
    tab, ext = np.stack([l["tab"] for l in lines]), np.stack([l["ext"] for l in lines])
    s = np.stack([l["s"] for l in lines]); x = np.stack([l["x"] for l in lines]); y = np.stack([l["y"] for l in lines])
    L = np.array([l["length"] for l in lines])
    bad_tab, bad_s, bad_L = tab.copy(), s.copy(), L.copy()
    bad_tab[1, 0, 1500] = np.nan; bad_tab[1, 3, 10] = np.nan
    bad_s[1, 700] = np.nan
    bad_L[1] = np.inf
    h = handles[1]
    clean = [d_spline_fit(h, s, x, y)[1:], d_reference_states(h, tab, ext, L, 20000)[1:3], d_segment(h, tab, ext, L, 3000)[1],
             d_reference_length(h, tab, ext, L, np.zeros((B, 3)))[1]]
    dirty = [d_spline_fit(h, bad_s, x, y), d_reference_states(h, bad_tab, ext, bad_L, 20000), d_segment(h, bad_tab, ext, bad_L, 3000),
             d_reference_length(h, bad_tab, ext, L, np.zeros((B, 3)))]         # (an infinite length would be an endless coarse scan in either form)
    assert all(d[0] == 0 for d in dirty)
    keep = [0, 2, 3]
    assert all(same_bytes(a[keep], b[keep]) for a, b in zip(clean[0], dirty[0][1:]))
    assert all(same_bytes(a[keep], b[keep]) for a, b in zip(clean[1], dirty[1][1:3]))
    assert all(same_bytes(clean[2][k][keep], dirty[2][1][k][keep]) for k in clean[2])
    assert same_bytes(clean[3][keep], dirty[3][1][keep])
