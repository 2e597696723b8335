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
import device_form
from chain_util import scenarios, smoother_params, steps_on_device
from device_form import SENT, Out, call, d_bounds_on_states, to_device
from path_optimizer_2_amd import capi
from shared_util import capi_geom, oracle_geom, same_bytes

pytestmark = pytest.mark.gpu


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
    b, nv = handle.corridor_bounds(c["ref"][None], c["tab"][None], c["ext"][None], c["dist"], capi_geom(c["geom"]))
    n = c["ref"].shape[0]
    scal = np.array([[0.05, 0.01, c["ref"][0, 1], c["ref"][n - 1, 2], 1.0 if nv[0] < n else 0.0, 35.0 * np.pi / 180.0]])
    res = solver.solve_var(nv, c["ref"][None], b, scal, passes=0)
    assert res["status"][0] == 1
    return res["out"][0], int(nv[0])


@pytest.mark.parametrize("seed,n", [(0, 40), (1, 80), (2, 80), (5, 120)])
def test_kernel_matches_the_restatement(handle, solver, seed, n):
    c = U.build(seed=seed, n=n)
    out, nv = _first_pass(solver, handle, c)
    g = capi_geom(c["geom"])
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
                                               np.stack([c["dist"] for c in cs]), capi_geom(cs[0]["geom"]), map_of=[0, 1, 2], n_of=n_of)
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
        got, nv = handle.corridor_bounds_on_states(c["ref"][None], st, tab[None], ext[None], dist, capi_geom(c["geom"]))
        nvs.append(_compare(got[0], int(nv[0]), c["ref"], dpsi, dx, dy, dist, c["geom"]))
    assert 36 <= nvs[1] < 72


def test_stride_seven_in_place_equals_stride_five(handle):
    c = U.build(seed=3, n=80)
    rng = np.random.default_rng(2)
    out = rng.normal(size=(1, 80, 7))
    out[0, :, 4] = rng.uniform(-0.5, 0.5, size=80)
    five = np.ascontiguousarray(out[:, :, :5])
    g = capi_geom(c["geom"])
    a = handle.corridor_bounds_on_states(c["ref"][None], out, c["tab"][None], c["ext"][None], c["dist"], g)
    b = handle.corridor_bounds_on_states(c["ref"][None], five, c["tab"][None], c["ext"][None], c["dist"], g)
    assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    # only d_heading is read: the other columns do not matter
    five[0, :, :4] = 0.0
    b = handle.corridor_bounds_on_states(c["ref"][None], five, c["tab"][None], c["ext"][None], c["dist"], g)
    assert same_bytes(a[0], b[0])


# ---- device form: sentinel-filled outputs, host == device, permutation ---------------------------------------------------------------
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
    g = capi_geom(cs[0]["geom"])
    got, nv = d_bounds_on_states(handle, ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    hb, hnv = handle.corridor_bounds_on_states(ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    assert same_bytes(nv, hnv)
    for b in range(len(ref)):
        k = int(n_of[b])
        assert np.all(got[b, k:] == SENT), b                 # rows beyond the scenario's states: not written
        assert np.all(got[b, :k] != SENT), b                 # ... every row of its states is (the blocked one and those behind it too)
        assert same_bytes(got[b, :k], hb[b, :k]) and np.all(hb[b, k:] == 0.0)
        _compare(got[b], int(nv[b]), ref[b], st[b, :k, 4], cs[mo[b]]["sx"], cs[mo[b]]["sy"], cs[mo[b]]["dist"], cs[0]["geom"])
    # a permuted batch gives the permuted outputs, bit for bit
    p = np.random.default_rng(5).permutation(len(ref))
    pb, pnv = d_bounds_on_states(handle, ref[p], st[p], tab[p], ext[p], dist, g, map_of=mo[p], n_of=n_of[p])
    assert same_bytes(pnv, nv[p])
    for i, b in enumerate(p):
        assert same_bytes(pb[i, :n_of[b]], got[b, :n_of[b]])


def test_heading_errors_that_are_not_finite_do_not_disturb_the_batch(handle):
    cs, mo, ref, tab, ext, st, n_of, dist = _batch(B=6, seed=3)
    n_of[:] = ref.shape[1]
    g = capi_geom(cs[0]["geom"])
    clean, clean_nv = d_bounds_on_states(handle, ref, st, tab, ext, dist, g, map_of=mo, n_of=n_of)
    bad = st.copy()
    bad[2, 5, 4] = np.nan; bad[2, 9, 4] = np.inf; bad[4, 0, 4] = -np.inf
    got, nv = d_bounds_on_states(handle, ref, bad, tab, ext, dist, g, map_of=mo, n_of=n_of)
    for b in (0, 1, 3, 5):
        assert same_bytes(got[b], clean[b]) and nv[b] == clean_nv[b]
    for b, rows in ((2, (5, 9)), (4, (0,))):
        for i in rows:
            if i < nv[b]:
                assert np.isnan(got[b, i, :4]).all() and np.isfinite(got[b, i, 4:]).all()
        _compare(got[b], int(nv[b]), ref[b], bad[b, :, 4], cs[mo[b]]["sx"], cs[mo[b]]["sy"], cs[mo[b]]["dist"], cs[0]["geom"])


def test_argument_errors(handle):
    c = U.build(seed=0, n=8)
    g = capi_geom(c["geom"])
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
    assert call(handle, "pqp_corridor_bounds_on_states_device", 1, 8, tab.shape[2], to_device(ref), None, to_device(st), 4, to_device(tab), to_device(ext),
                to_device(dist, np.float32), None, C.byref(g), C.byref(prm), Out((1, 8, 6)), Out((1,), np.int32)) == -1
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
                assert same_bytes(got["out"][b, :nv], want["out2"][b, :nv]), b
                ok += got["stage"][b] == 0
            assert got["iters"][b] == want["it1"][b] + want["it2"][b], b
    return ok


@pytest.mark.parametrize("lane_per_qp", [False, True])
def test_bounds_on_states_chain_equals_the_steps(hip_lib, lane_per_qp):
    B = 24
    sc = scenarios(B)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
    if lane_per_qp:
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_STREAM_BATCH, 1)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    if lane_per_qp:
        assert h.last_path_kernel() == capi.KERNEL_LANE_PER_QP
    want = steps_on_device(h, hs, sc, cfg)
    assert _check_chain_against_steps(got, want, B) >= B // 2
    # the second pass did change something: the bounds follow the path
    moved = [b for b in range(B) if got["stage"][b] == 0 and not same_bytes(want["out1"][b, :got["n_out"][b]], got["out"][b, :got["n_out"][b]])]
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
    sc = scenarios(B, seed=7)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    want = steps_on_device(h, hs, sc, cfg)
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
    sc = scenarios(B, seed=9)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
    cfg = _cfg(h, capi.SECOND_PASS_BOUNDS_ON_STATES)
    # scenarios 1 and 3 get maps of their own with a 0.35 m pit on the reference line.  The first pass's circles are 3.9 m ahead of / 1 m
    # behind a state, the second pass's on the states themselves (small heading errors).  Scenario 1, pit at state 0: the first pass is
    # not blocked there, the second one is at once (n_valid2 < 2).  Scenario 3, pit at state 4 (s ~ 1 m, behind every front circle): the
    # first pass is blocked where a rear circle reaches it, the second pass earlier, at the pit
    ref0 = steps_on_device(h, hs, sc, cfg)["ref"]
    g = oracle_geom(sc["geom"])
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
    want = steps_on_device(h, hs, sc, cfg)
    _check_chain_against_steps(got, want, B)
    assert want["n_valid"][1] >= 2 and want["st1"][1] == 1 and want["nv2"][1] < 2
    assert got["stage"][1] == 7 and got["n_out"][1] == 0 and got["status"][1] == 0
    assert want["st1"][3] == 1 and 2 <= want["nv2"][3] < want["n_valid"][3], (want["nv2"][3], want["n_valid"][3])
    assert got["stage"][3] in (0, 8) and got["n_out"][3] in (0, want["nv2"][3])
    assert want["scal2"][3, 4] == 1.0
    # a first pass that fails: no second pass, PATH_QP_FAILED with the first solve's status ("Pre solving failed!")
    hf = capi.Handle(capi.production_params(max_iter=3, polish=0), max_batch=B, max_n=256)
    gf = hf.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    wf = steps_on_device(hf, hs, sc, cfg)
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
    sc = scenarios(B, seed=11)
    dev = device_form.dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    modes = [1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1]
    results = {}
    for graph in (0, 1):
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=256)
        hs = capi.Handle(smoother_params(), device=0, max_batch=B, max_n=128)
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
            assert same_bytes(x, y), (k, mode)
        for q in range(B):
            assert same_bytes(a[4][q, :a[0][q]], b[4][q, :b[0][q]]), (k, q)
    # the two modes do give different paths
    assert any(not same_bytes(results[0][0][4][q, :results[0][0][0][q]], results[0][4][4][q, :results[0][4][0][q]]) for q in range(B))
