"""pqp_corridor_bounds_on_states (ReferencePath::updateBoundsOnInputStates, reference_path_impl.cpp:118-175) on the GPU against the float64
restatement in tests/corridor_states_util.py, and the chain's second_pass = PQP_SECOND_PASS_BOUNDS_ON_STATES (the lines path_optimizer.cpp:147-151
has commented out) against the same composition done step by step through the public ABI.  Sample positions are the reference's
expressions with FMA contraction off; only sin / cos differ (ocml vs libm), which can move a bound by one whole search step when a sample
sits within round-off of the 0.5 m threshold - the tolerance rule of test_gpu_corridor.py, restated here."""
import ctypes as C
import time

import numpy as np
import pytest

import corridor_oracle as K
import corridor_states_util as S
import corridor_util as U
from path_optimizer_2_amd import capi
from path_optimizer_2_amd.synth import make_scene

pytestmark = pytest.mark.gpu

SENT, SENT_I = -1.2345e300, -777          # what the device outputs are filled with before a call
GUARD = 512                               # elements of sentinel behind every device output


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\n{__name__}: {time.time() - t0:.1f} s wall")


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=64, max_n=256)
    yield h
    h.close()


@pytest.fixture(scope="module")
def solver(hip_lib):
    h = capi.Handle(capi.production_params(), device=0, max_batch=64, max_n=256)
    yield h
    h.close()


def _geom(g):
    return capi.PqpGridGeometry(g.rows, g.cols, g.resolution, g.length_x, g.length_y, g.pos_x, g.pos_y)


def _same(a, b):
    """bit for bit, NaN where NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _compare(got, n_valid_got, ref, dpsi, sx, sy, dist, g, prm=K.CorridorParams()):
    """the rule of test_gpu_corridor._compare: n_valid exact, > 99 % of the entries within 1e-9, any other one off by a whole 0.05 / 0.3 m step"""
    want, n_valid, blocked = S.update_bounds_on_input_states(ref, dpsi, sx, sy, dist, g, prm)
    assert n_valid_got == n_valid, (n_valid_got, n_valid)
    rows = np.vstack([want, np.array(blocked)[None]]) if blocked is not None else want
    g_rows = got[:len(rows)]
    nan = np.isnan(rows)
    assert np.array_equal(nan, np.isnan(g_rows))
    diff = np.abs(g_rows[~nan] - rows[~nan])
    exact = diff < 1e-9
    off = diff[~exact]
    assert exact.mean() > 0.99, (exact.mean(), off)
    for d in off:
        assert min(abs(d - 0.05 * k) for k in range(1, 8)) < 1e-9 or min(abs(d - 0.3 * k) for k in range(1, 4)) < 1e-9, d
    return n_valid


def _first_pass(solver, handle, c, map_of=None):
    """a real first pass: the corridor of the reference states, a cold path solve (BaseSolver::solve) on it -> out [n][7], n_valid"""
    b, nv = handle.corridor_bounds(c["ref"][None], c["tab"][None], c["ext"][None], c["dist"], _geom(c["geom"]))
    n = c["ref"].shape[0]
    scal = np.array([[0.05, 0.01, c["ref"][0, 1], c["ref"][n - 1, 2], 1.0 if nv[0] < n else 0.0, 35.0 * np.pi / 180.0]])
    res = solver.solve_var(nv, c["ref"][None], b, scal, passes=0)
    assert res["status"][0] == 1
    return res["out"][0], int(nv[0])


@pytest.mark.parametrize("seed,n", [(0, 40), (1, 80), (2, 80), (5, 120)])
def test_kernel_matches_the_restatement(handle, solver, seed, n):
    c = U.build(seed=seed, n=n)
    out, nv = _first_pass(solver, handle, c)
    g = _geom(c["geom"])
    # the first pass's own heading errors, on its n_valid states (stride 7: `out` as it is)
    got, got_nv = handle.corridor_bounds_on_states(c["ref"][None], out[None], c["tab"][None], c["ext"][None], c["dist"], g, n_of=[nv])
    _compare(got[0], int(got_nv[0]), c["ref"], out[:nv, 4], c["sx"], c["sy"], c["dist"], c["geom"])
    # random heading errors in +-0.5 rad on every state
    rng = np.random.default_rng(seed)
    dpsi = rng.uniform(-0.5, 0.5, size=n)
    st = np.zeros((1, n, 5)); st[0, :, 4] = dpsi
    got, got_nv = handle.corridor_bounds_on_states(c["ref"][None], st, c["tab"][None], c["ext"][None], c["dist"], g)
    _compare(got[0], int(got_nv[0]), c["ref"], dpsi, c["sx"], c["sy"], c["dist"], c["geom"])


def _wall(c, at):
    g = c["geom"]
    d2 = c["dist"].copy()
    x_wall = c["ref"][at, 3]
    for i in range(g.rows):
        x, _ = K.grid_cell_position(g, i, 0)
        d2[i, :] = np.minimum(d2[i, :], np.float32(abs(x - x_wall)))
    return d2


def test_many_maps_ragged_counts_and_a_blocked_road(handle):
    cs = [U.build(seed=s, n=60) for s in (7, 8, 9)]
    cs[2]["dist"] = _wall(cs[2], 35)                     # scenario 2: a wall across the road at waypoint 35
    rng = np.random.default_rng(4)
    dpsi = rng.uniform(-0.4, 0.4, size=(3, 60))
    st = np.zeros((3, 60, 7)); st[:, :, 4] = dpsi
    n_of = np.array([60, 45, 60], dtype=np.int32)
    got, nv = handle.corridor_bounds_on_states(np.stack([c["ref"] for c in cs]), st, np.stack([c["tab"] for c in cs]), np.stack([c["ext"] for c in cs]),
                                               np.stack([c["dist"] for c in cs]), _geom(cs[0]["geom"]), map_of=[0, 1, 2], n_of=n_of)
    for q, c in enumerate(cs):
        _compare(got[q], int(nv[q]), c["ref"], dpsi[q, :n_of[q]], c["sx"], c["sy"], c["dist"], c["geom"])
    assert nv[0] == 60 and nv[1] == 45 and nv[2] < 35
    assert np.all(got[1, 45:] == 0.0)                    # host form: rows beyond a scenario's states come back as zeros


def test_paths_longer_than_the_lds_go_through_in_tiles(handle):
    """a table of 2150 knots leaves room for 33 waypoints at a time: 80 waypoints in three tiles, with and without a wall in the third"""
    c = U.build(seed=8, n=80)
    s_end = c["scene"]["knots_s"][-1]
    ks = np.linspace(0.0, s_end, 2150)
    dx = K.spline_fit(ks, np.array([K.spline_eval(c["sx"], v) for v in ks]))
    dy = K.spline_fit(ks, np.array([K.spline_eval(c["sy"], v) for v in ks]))
    tab, ext = K.pack_spline(dx, dy)
    dpsi = np.random.default_rng(1).uniform(-0.5, 0.5, size=80)
    st = np.zeros((1, 80, 5)); st[0, :, 4] = dpsi
    nvs = []
    for dist in (c["dist"], _wall(c, 72)):
        got, nv = handle.corridor_bounds_on_states(c["ref"][None], st, tab[None], ext[None], dist, _geom(c["geom"]))
        nvs.append(_compare(got[0], int(nv[0]), c["ref"], dpsi, dx, dy, dist, c["geom"]))
    assert 36 <= nvs[1] < 72


def test_stride_seven_in_place_equals_stride_five(handle):
    c = U.build(seed=3, n=80)
    rng = np.random.default_rng(2)
    out = rng.normal(size=(1, 80, 7))
    out[0, :, 4] = rng.uniform(-0.5, 0.5, size=80)
    five = np.ascontiguousarray(out[:, :, :5])
    g = _geom(c["geom"])
    a = handle.corridor_bounds_on_states(c["ref"][None], out, c["tab"][None], c["ext"][None], c["dist"], g)
    b = handle.corridor_bounds_on_states(c["ref"][None], five, c["tab"][None], c["ext"][None], c["dist"], g)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    # only d_heading is read: the other columns do not matter
    five[0, :, :4] = 0.0
    b = handle.corridor_bounds_on_states(c["ref"][None], five, c["tab"][None], c["ext"][None], c["dist"], g)
    assert _same(a[0], b[0])


# ---- device form: sentinel-filled outputs, host == device, permutation ---------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dt=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(_dev())


class Out:
    def __init__(self, shape, dt=np.float64):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.sent = SENT if dt == np.float64 else SENT_I
        self.t = torch.full((self.n + GUARD,), self.sent, dtype=torch.float64 if dt == np.float64 else torch.int32, device=_dev())

    def get(self):
        a = self.t.cpu().numpy()
        assert np.all(a[self.n:] == self.sent), "the device form wrote behind its output"
        return a[:self.n].reshape(self.shape)


def _call(h, name, *args):
    import torch
    conv = [C.c_void_p(a.t.data_ptr()) if isinstance(a, Out) else C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    torch.cuda.synchronize(_dev())
    rc = getattr(h.lib, name)(h._h, *conv)
    h.sync()
    return rc


def _d_bounds(h, ref, states, tab, ext, dist, geom, map_of=None, n_of=None, prm=None):
    B, n = ref.shape[:2]
    bounds, nv = Out((B, n, 6)), Out((B,), np.int32)
    prm = prm or h.corridor_params()
    rc = _call(h, "pqp_corridor_bounds_on_states_device", B, n, tab.shape[2], _t(ref), None if n_of is None else _t(n_of, np.int32), _t(states),
               states.shape[2], _t(tab), _t(ext), _t(np.transpose(dist, (0, 2, 1)), np.float32), None if map_of is None else _t(map_of, np.int32),
               C.byref(geom), C.byref(prm), bounds, nv)
    assert rc == 0, h.lib.pqp_last_error()
    return bounds.get(), nv.get()


def _batch(B=12, n=70, seed=0):
    cs = [U.build(seed=10 + s, n=n) for s in range(4)]
    cs[3]["dist"] = _wall(cs[3], 50)
    rng = np.random.default_rng(seed)
    mo = (np.arange(B) % 4).astype(np.int32)
    ref = np.stack([cs[k]["ref"] for k in mo]); tab = np.stack([cs[k]["tab"] for k in mo]); ext = np.stack([cs[k]["ext"] for k in mo])
    st = rng.normal(size=(B, n, 7)); st[:, :, 4] = rng.uniform(-0.5, 0.5, size=(B, n))
    n_of = rng.integers(1, n + 1, size=B).astype(np.int32); n_of[0] = n
    return cs, mo, ref, tab, ext, st, n_of, np.stack([c["dist"] for c in cs])


def test_device_form_writes_within_its_extent_and_equals_the_host_form(handle):
    cs, mo, ref, tab, ext, st, n_of, dist = _batch()
    g = _geom(cs[0]["geom"])
    got, nv = _d_bounds(handle, ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    hb, hnv = handle.corridor_bounds_on_states(ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    assert _same(nv, hnv)
    for b in range(len(ref)):
        k = int(n_of[b])
        assert np.all(got[b, k:] == SENT), b                 # rows beyond the scenario's states: not written
        assert np.all(got[b, :k] != SENT), b                 # ... every row of its states is (the blocked one and those behind it too)
        assert _same(got[b, :k], hb[b, :k]) and np.all(hb[b, k:] == 0.0)
        _compare(got[b], int(nv[b]), ref[b], st[b, :k, 4], cs[mo[b]]["sx"], cs[mo[b]]["sy"], cs[mo[b]]["dist"], cs[0]["geom"])
    # a permuted batch gives the permuted outputs, bit for bit
    p = np.random.default_rng(5).permutation(len(ref))
    pb, pnv = _d_bounds(handle, ref[p], st[p], tab[p], ext[p], dist, g, map_of=mo[p], n_of=n_of[p])
    assert _same(pnv, nv[p])
    for i, b in enumerate(p):
        assert _same(pb[i, :n_of[b]], got[b, :n_of[b]])


def test_heading_errors_that_are_not_finite_do_not_disturb_the_batch(handle):
    cs, mo, ref, tab, ext, st, n_of, dist = _batch(B=6, seed=3)
    n_of[:] = ref.shape[1]
    g = _geom(cs[0]["geom"])
    clean, clean_nv = _d_bounds(handle, ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    bad = st.copy()
    bad[2, 5, 4] = np.nan; bad[2, 9, 4] = np.inf; bad[4, 0, 4] = -np.inf
    got, nv = _d_bounds(handle, ref, bad, tab, ext, dist, g, map_of=mo, n_of=n_of)
    for b in (0, 1, 3, 5):
        assert _same(got[b], clean[b]) and nv[b] == clean_nv[b]
    for b, rows in ((2, (5, 9)), (4, (0,))):
        for i in rows:
            if i < nv[b]:
                assert np.isnan(got[b, i, :4]).all() and np.isfinite(got[b, i, 4:]).all()
        _compare(got[b], int(nv[b]), ref[b], bad[b, :, 4], cs[mo[b]]["sx"], cs[mo[b]]["sy"], cs[mo[b]]["dist"], cs[0]["geom"])


def test_argument_errors(handle):
    c = U.build(seed=0, n=8)
    g = _geom(c["geom"])
    st = np.zeros((1, 8, 7))
    args = (c["ref"][None], st, c["tab"][None], c["ext"][None], c["dist"], g)
    with pytest.raises(capi.PqpError, match="pqp error -1:"):
        handle.corridor_bounds_on_states(c["ref"][None], np.zeros((1, 8, 4)), c["tab"][None], c["ext"][None], c["dist"], g)     # stride < 5
    with pytest.raises(capi.PqpError, match="pqp error -1:"):
        handle.corridor_bounds_on_states(*args, map_of=[1])                      # one map only
    with pytest.raises(capi.PqpError, match="pqp error -1:"):
        handle.corridor_bounds_on_states(*args, map_of=[-1])
    with pytest.raises(capi.PqpError, match="pqp error -1:"):
        handle.corridor_bounds_on_states(*args, n_of=[9])                        # more states than reference states (CHECK_LE)
    prm = handle.corridor_params()
    nul = lambda *a: handle.lib.pqp_corridor_bounds_on_states(handle._h, *a)
    ref, tab, ext, dist = (np.ascontiguousarray(x) for x in (c["ref"][None], c["tab"][None], c["ext"][None], c["dist"].T.astype(np.float32)))
    bounds, nv = np.zeros((1, 8, 6)), np.zeros(1, dtype=np.int32)
    p = capi._ptr
    assert nul(1, 8, tab.shape[2], p(ref), None, None, 7, p(tab), p(ext), p(dist), 1, None, C.byref(g), C.byref(prm), p(bounds), p(nv)) == -1   # states NULL
    assert nul(1, 8, tab.shape[2], p(ref), None, p(st), 7, p(tab), p(ext), p(dist), 1, None, C.byref(g), C.byref(prm), None, p(nv)) == -1     # bounds NULL
    # the device form checks pointers and sizes only
    assert _call(handle, "pqp_corridor_bounds_on_states_device", 1, 8, tab.shape[2], _t(ref), None, _t(st), 4, _t(tab), _t(ext),
                 _t(dist, np.float32), None, C.byref(g), C.byref(prm), Out((1, 8, 6)), Out((1,), np.int32)) == -1
    # a launch refused for its LDS (a spline table that leaves no room for the probes) leaves the timing of the previous launch
    fresh = capi.Handle(capi.default_params(), device=0, max_batch=1, max_n=8)
    try:
        s = np.arange(8.0)[None]
        fresh.spline_fit(s, s, np.zeros_like(s))
        ms = fresh.last_kernel_ms()
        big = np.zeros((1, 9, 2400)); big[0, 0] = np.arange(2400.0)
        with pytest.raises(capi.PqpError, match="pqp error -4:"):
            fresh.corridor_bounds_on_states(c["ref"][None], st, big, c["ext"][None], c["dist"], g)
        assert fresh.last_kernel_ms() == ms
        assert fresh.kernel_ms_history(1)[0] == np.float32(ms)
    finally:
        fresh.close()


# ---- the chain's second pass -------------------------------------------------------------------------------------------------------
def _smoother_params():
    return capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25)


def _scenarios(B, n_maps=4, seed=5):
    cs = [make_scene(seed=s, n=40, n_obstacles=25, knots_every=3.05) for s in range(n_maps)]
    rng = np.random.default_rng(seed)
    p_max = len(cs[0]["knots_x"])
    pts = np.zeros((B, p_max, 2)); n_pts = np.zeros(B, dtype=np.int32); map_of = (np.arange(B) % n_maps).astype(np.int32)
    start = np.zeros((B, 3)); target = np.zeros((B, 3))
    for b in range(B):
        c = cs[b % n_maps]
        P = int(rng.integers(7, p_max + 1))
        n_pts[b] = P
        pts[b, :P, 0] = c["knots_x"][:P]; pts[b, :P, 1] = c["knots_y"][:P] + rng.normal(scale=0.15, size=P)
        h0 = np.arctan2(pts[b, 1, 1] - pts[b, 0, 1], pts[b, 1, 0] - pts[b, 0, 0])
        start[b] = (pts[b, 0, 0] + 0.1, pts[b, 0, 1] + 0.1, h0 + 0.03)
        h1 = np.arctan2(pts[b, P - 1, 1] - pts[b, P - 2, 1], pts[b, P - 1, 0] - pts[b, P - 2, 0])
        target[b] = (pts[b, P - 1, 0], pts[b, P - 1, 1], h1)
    c0 = cs[0]
    geom = capi.PqpGridGeometry(c0["rows"], c0["cols"], c0["resolution"], c0["length"][0], c0["length"][1], c0["pos"][0], c0["pos"][1])
    return dict(pts=pts, n_pts=n_pts, map_of=map_of, start=start, target=target, dist=np.stack([c["dist"] for c in cs]), geom=geom)


def _steps(h, hs, sc, cfg):
    """pqp_optimize_path_device's launches up to the first path QP, one public device entry point at a time on the chain's own capacities, then
    the second pass composed by hand: pqp_path_solve_var_device (passes 0) -> pqp_corridor_bounds_on_states_device -> pqp_path_solve_var_device
    around the first path.  Returns the host arrays of every step that matters."""
    import torch
    B, p_max = sc["pts"].shape[:2]
    R, Sm, L, N = cfg.raw_max, cfg.sample_max, cfg.layer_max, cfg.n_max
    dev = _dev()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    zi = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
    clamp = lambda c, hi: c.clamp(0, hi).to(torch.int32).contiguous()
    last = lambda src, cnt, add: (src.gather(1, (cnt.clamp(1, src.shape[1]) - 1).long()[:, None])[:, 0] + add).contiguous()

    def run(hh, name, *a):
        assert _call(hh, name, *a) == 0, hh.lib.pqp_last_error()

    pts, n_pts, start, target = _t(sc["pts"]), _t(sc["n_pts"], np.int32), _t(sc["start"]), _t(sc["target"])
    dist, mo, geom = _t(np.transpose(sc["dist"], (0, 2, 1)), np.float32), _t(sc["map_of"], np.int32), sc["geom"]
    rx, ry, rs, raw_count = z(B, R), z(B, R), z(B, R), zi()
    run(h, "pqp_bspline_resample_device", B, p_max, R, pts, n_pts, rx, ry, rs, raw_count)
    raw_fit = clamp(raw_count, R)
    raw_tab, raw_ext = z(B, 9, R), z(B, 4)
    run(h, "pqp_spline_fit_var_device", B, R, raw_fit, rs, rx, ry, raw_tab, raw_ext)
    raw_len = last(rs, raw_fit, 0.0)
    gx, gy, gs, ga, gk, sample_count = z(B, Sm), z(B, Sm), z(B, Sm), z(B, Sm), z(B, Sm), zi()
    run(h, "pqp_segment_raw_reference_device", B, Sm, R, raw_tab, raw_ext, raw_len, C.c_double(1.0), gx, gy, gs, ga, gk, sample_count)
    sample_fit = clamp(sample_count, Sm)
    sx, sy, ss, sm_status, sm_iters = z(B, Sm), z(B, Sm), z(B, Sm), zi(), zi()
    run(hs, "pqp_smooth_tension2_var_device", B, Sm, sample_fit, gx, gy, ga, gk, gs, sx, sy, ss, sm_status, sm_iters, None)
    sm_tab, sm_ext = z(B, 9, Sm), z(B, 4)
    run(h, "pqp_spline_fit_var_device", B, Sm, sample_fit, ss, sx, sy, sm_tab, sm_ext)
    sm_len = last(ss, sample_fit, cfg.smoothed_length_margin)
    ls, lb, ub, layer_count, vl = z(B, L), z(B, L), z(B, L), zi(), z(B)
    run(h, "pqp_dp_corridor_device", B, Sm, L, sm_tab, sm_ext, sm_len, start, dist, mo, C.byref(geom), C.byref(cfg.dp), ls, lb, ub, layer_count, vl)
    layer_fit = clamp(layer_count, L)
    pl, ps_status, ps_iters = z(B, L), zi(), zi()
    run(hs, "pqp_post_smooth_var_device", B, L, layer_fit, ls, lb, ub, vl, pl, ps_status, ps_iters, None)
    px, py, ps = z(B, L), z(B, L), z(B, L)
    run(h, "pqp_offsets_to_points_device", B, Sm, L, sm_tab, sm_ext, ls, pl, layer_fit, px, py, ps)
    fin_tab, fin_ext = z(B, 9, L), z(B, 4)
    run(h, "pqp_spline_fit_var_device", B, L, layer_fit, ps, px, py, fin_tab, fin_ext)
    fin_len = last(ps, layer_fit, 0.0)
    max_s = z(B)
    run(h, "pqp_reference_length_device", B, L, fin_tab, fin_ext, fin_len, target, max_s)
    ref, ref_count, err = z(B, N, 5), zi(), z(B, 2)
    run(h, "pqp_reference_states_device", B, N, L, fin_tab, fin_ext, max_s, start, C.c_double(cfg.output_spacing / 2.0), C.c_double(cfg.output_spacing),
        1, ref, ref_count, err)
    ref_fit = clamp(ref_count, N)
    bounds, n_valid = z(B, N, 6), zi()
    run(h, "pqp_corridor_bounds_device", B, N, L, ref, ref_fit, fin_tab, fin_ext, dist, mo, C.byref(geom), C.byref(cfg.corridor), bounds, n_valid)
    scal = torch.stack([err[:, 0], err[:, 1], torch.zeros(B, dtype=torch.float64, device=dev), target[:, 2], (n_valid < ref_fit).double(),
                        torch.full((B,), cfg.max_steering_angle, dtype=torch.float64, device=dev)], 1).contiguous()
    # the second pass, by hand
    out1, st1, it1 = z(B, N, 7), zi(), zi()
    run(h, "pqp_path_solve_var_device", B, N, n_valid, ref, None, bounds, scal, 0, 0, out1, st1, it1, None)
    bounds2, nv2 = z(B, N, 6), zi()
    run(h, "pqp_corridor_bounds_on_states_device", B, N, L, ref, n_valid, out1, 7, fin_tab, fin_ext, dist, mo, C.byref(geom), C.byref(cfg.corridor), bounds2, nv2)
    scal2 = scal.clone(); scal2[:, 4] = (nv2 < ref_fit).double()
    lin = out1[:, :, 3:6].contiguous()
    n_of2 = torch.where(st1 == 1, nv2, torch.zeros_like(nv2)).contiguous()
    out2, st2, it2 = out1.clone(), zi(), zi()
    run(h, "pqp_path_solve_var_device", B, N, n_of2, ref, lin, bounds2, scal2, 0, 0, out2, st2, it2, None)
    host = lambda x: x.cpu().numpy()
    return dict(ref=host(ref), n_valid=host(n_valid), out1=host(out1), st1=host(st1), it1=host(it1), bounds2=host(bounds2), nv2=host(nv2), scal2=host(scal2),
                lin=host(lin), out2=host(out2), st2=host(st2), it2=host(it2))


def _cfg(h, mode, **over):
    return h.chain_config(raw_max=64, sample_max=48, layer_max=32, n_max=128, second_pass=mode, **over)


def _check_chain_against_steps(got, want, B):
    ok = 0
    for b in range(B):
        if got["stage"][b] in (0, 7, 8) and want["n_valid"][b] >= 2:
            if want["st1"][b] != 1:
                assert got["stage"][b] == 8 and got["status"][b] == want["st1"][b] and got["n_out"][b] == 0, b
            elif want["nv2"][b] < 2:
                assert got["stage"][b] == 7 and got["status"][b] == 0 and got["n_out"][b] == 0, b
            else:
                nv = int(want["nv2"][b])
                assert got["n_out"][b] == nv and got["status"][b] == want["st2"][b], b
                assert got["stage"][b] == (0 if want["st2"][b] == 1 else 8), b
                assert _same(got["out"][b, :nv], want["out2"][b, :nv]), b
                ok += got["stage"][b] == 0
            assert got["iters"][b] == want["it1"][b] + want["it2"][b], b
    return ok


@pytest.mark.parametrize("lane_per_qp", [False, True])
def test_bounds_on_states_chain_equals_the_steps(hip_lib, lane_per_qp):
    B = 24
    sc = _scenarios(B)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(_smoother_params(), max_batch=B, max_n=128)
    if lane_per_qp:
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_STREAM_BATCH, 1)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    if lane_per_qp:
        assert h.last_path_kernel() == capi.KERNEL_LANE_PER_QP
    want = _steps(h, hs, sc, cfg)
    assert _check_chain_against_steps(got, want, B) >= B // 2
    # the second pass did change something: the bounds follow the path
    moved = [b for b in range(B) if got["stage"][b] == 0 and not _same(want["out1"][b, :got["n_out"][b]], got["out"][b, :got["n_out"][b]])]
    assert len(moved) >= B // 2
    # mode 0 on the same handle is still today's chain: passes = 1 on the first bounds
    plain = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                            cfg=_cfg(h, capi.SECOND_PASS_RELINEARISE))
    for b in range(B):
        if plain["stage"][b] == 0:
            assert plain["n_out"][b] == want["n_valid"][b]
    h.close(); hs.close()


def test_second_qp_agrees_with_highs(hip_lib):
    import highs_qp as H
    if not H.available():
        pytest.skip("this scipy does not bundle the HiGHS QP interface")
    from highs_util import against_highs
    B = 12
    sc = _scenarios(B, seed=7)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(_smoother_params(), max_batch=B, max_n=128)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    want = _steps(h, hs, sc, cfg)
    done = 0
    for b in np.random.default_rng(0).permutation(B):
        if got["stage"][b] != 0 or done >= 4:
            continue
        n = int(got["n_out"][b])
        against_highs(want["ref"][b, :n], want["lin"][b, :n], want["bounds2"][b, :n], want["scal2"][b], got["out"][b, :n])
        done += 1
    assert done == 4
    h.close(); hs.close()


def test_stages_of_the_second_pass(hip_lib):
    B = 8
    sc = _scenarios(B, seed=9)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(_smoother_params(), max_batch=B, max_n=128)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    # scenarios 1 and 3 get maps of their own with a 0.35 m pit on the reference line.  The first pass's circles are 3.9 m ahead of / 1 m
    # behind a state, the second pass's on the states themselves (small heading errors).  Scenario 1, pit at state 0: the first pass is
    # not blocked there, the second one is at once (n_valid2 < 2).  Scenario 3, pit at state 4 (s ~ 1 m, behind every front circle): the
    # first pass is blocked where a rear circle reaches it, the second pass earlier, at the pit
    ref0 = _steps(h, hs, sc, cfg)["ref"]
    g = K.GridGeom(sc["geom"].rows, sc["geom"].cols, sc["geom"].resolution, sc["geom"].length_x, sc["geom"].length_y, sc["geom"].pos_x, sc["geom"].pos_y)
    for b, at in ((1, 0), (3, 4)):
        layer = sc["dist"][sc["map_of"][b]].copy()
        x0, y0 = ref0[b, at, 3:5]
        for i in range(g.rows):
            for j in range(g.cols):
                cx, cy = K.grid_cell_position(g, i, j)
                if (cx - x0) ** 2 + (cy - y0) ** 2 < 0.35 ** 2:
                    layer[i, j] = 0.0
        sc["dist"] = np.concatenate([sc["dist"], layer[None]])
        sc["map_of"][b] = len(sc["dist"]) - 1
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    want = _steps(h, hs, sc, cfg)
    _check_chain_against_steps(got, want, B)
    assert want["n_valid"][1] >= 2 and want["st1"][1] == 1 and want["nv2"][1] < 2
    assert got["stage"][1] == 7 and got["n_out"][1] == 0 and got["status"][1] == 0
    assert want["st1"][3] == 1 and 2 <= want["nv2"][3] < want["n_valid"][3], (want["nv2"][3], want["n_valid"][3])
    assert got["stage"][3] in (0, 8) and got["n_out"][3] in (0, want["nv2"][3])
    assert want["scal2"][3, 4] == 1.0
    # a first pass that fails: no second pass, PATH_QP_FAILED with the first solve's status ("Pre solving failed!")
    hf = capi.Handle(capi.production_params(max_iter=3, polish=0), max_batch=B, max_n=256)
    gf = hf.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    wf = _steps(hf, hs, sc, cfg)
    failed = [b for b in range(B) if wf["n_valid"][b] >= 2 and wf["st1"][b] != 1 and gf["stage"][b] in (0, 7, 8)]
    assert failed
    _check_chain_against_steps(gf, wf, B)
    for b in failed:
        assert gf["stage"][b] == 8 and gf["status"][b] == wf["st1"][b] and gf["iters"][b] == wf["it1"][b]
    hf.close()
    # refused up front: rough_constraints_far_away on the path handle, an unknown mode
    hr = capi.Handle(capi.production_params(rough_constraints_far_away=1), max_batch=B, max_n=256)
    with pytest.raises(capi.PqpError, match="pqp error -1:.*rough_constraints_far_away"):
        hr.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    assert hr.last_path_kernel() == capi.KERNEL_NONE
    with pytest.raises(capi.PqpError, match="pqp error -1:"):
        h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=_cfg(h, 2))
    hr.close(); h.close(); hs.close()


def test_chain_graph_replays_follow_the_mode(hip_lib):
    """PQP_OPT_CHAIN_GRAPH with identical pointers call after call: the key holds second_pass, so flipping it never replays the other mode's
    graph; every call equals a plainly launched chain of the same mode bit for bit"""
    import torch
    B = 24
    sc = _scenarios(B, seed=11)
    dev = _dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    modes = [1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1]
    results = {}
    for graph in (0, 1):
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=256)
        hs = capi.Handle(_smoother_params(), device=0, max_batch=B, max_n=128)
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_ORDER_BY_COST, 1); h.set_option(capi.OPT_CHAIN_GRAPH, graph)
        d_pts, d_np, d_st, d_tg = t(sc["pts"], np.float64), t(sc["n_pts"], np.int32), t(sc["start"], np.float64), t(sc["target"], np.float64)
        d_map, d_dist = t(sc["map_of"], np.int32), t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)
        out = torch.zeros((B, 128, 7), dtype=torch.float64, device=dev)
        n_out, status, stage, iters = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
        got = []
        for mode in modes:
            cfg = _cfg(h, mode)
            torch.cuda.synchronize()
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    C.byref(sc["geom"]), None, p(out), p(n_out), p(status), p(stage), p(iters)))
            h.sync(); hs.sync()
            got.append(tuple(x.cpu().numpy().copy() for x in (n_out, status, stage, iters, out)))
        results[graph] = got
        # and the handle still solves plain batches afterwards
        from path_optimizer_2_amd.synth import make_batch
        mb = make_batch(16, 80)
        assert (h.solve(mb["ref"], mb["bounds"], mb["scal"], passes=1)["status"] == 1).all()
        h.close(); hs.close()
    for k, mode in enumerate(modes):
        a, b = results[0][k], results[1][k]
        for x, y in zip(a[:4], b[:4]):
            assert _same(x, y), (k, mode)
        for q in range(B):
            assert _same(a[4][q, :a[0][q]], b[4][q, :b[0][q]]), (k, q)
    # the two modes do give different paths
    assert any(not _same(results[0][0][4][q, :results[0][0][0][q]], results[0][4][4][q, :results[0][4][0][q]]) for q in range(B))
