"""pqp_optimize_path_device: the whole of PathOptimizer::solve (reference src/path_optimizer.cpp:34-71) for a ragged batch as one
device-resident call, against the same twelve steps run one scenario at a time through the per-step entry points (each of which is
checked against its oracle in test_gpu_corridor.py / test_gpu_smoothers.py / test_gpu_parity.py), and the reference's `return false`
sites as stages.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import corridor_oracle as K
from chain_util import scenarios, smoother_params, steps_one_by_one
from path_optimizer_2_amd import capi

pytestmark = pytest.mark.gpu


def test_ragged_batch_equals_the_steps_run_one_scenario_at_a_time(hip_lib):
    B = 24
    sc = scenarios(B)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
    cfg = h.chain_config()
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    assert (got["stage"] == 0).sum() >= B - 2, got["stage"]
    seen = set()
    for b in range(B):
        if got["stage"][b] != 0:
            continue
        want = steps_one_by_one(h, hs, sc, b, cfg)
        assert want["stage"] == 0, (b, want["stage"])
        seen.add((want["n0"], want["n1"], want["layers"], want["nv"]))
        assert got["n_out"][b] == want["nv"] and got["status"][b] == want["status"] == 1
        nv = want["nv"]
        # both sides solve their QPs to the optimum (polish); the padded smoother QPs and the exact-size ones agree to the polish
        # tolerance, and so does everything downstream
        assert np.abs(got["out"][b, :nv] - want["out"][:nv]).max() < 2e-5, (b, np.abs(got["out"][b, :nv] - want["out"][:nv]).max())
        assert np.all(got["out"][b, nv:] == 0.0)
    assert len(seen) >= 6                          # the batch really was ragged
    h.close(); hs.close()


def test_configs0_the_demo_s_single_path(hip_lib):
    """BASELINE configs[0]: one scenario, a line of about 60 waypoints, fixed start and goal on an obstacle map - the reference's demo
    (CPU OSQP).  Here: batch 1 through the device-resident chain, the reference's smoother setting (OSQP defaults) and the production path
    QP; the path against the C restatement of OSQP run to 1e-9 on the reference states and corridor the chain produced - the north_star
    bar: 1e-4 in lateral offset and heading."""
    import pqp_oracle_c as OC
    sc = scenarios(1, n_maps=1, seed=21)
    sc["n_pts"][0] = 9                                             # ~24 m of input polygon -> ~18 m of line after the search: ~60 waypoints
    h = capi.Handle(capi.production_params(), max_batch=1, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=1, max_n=128)
    cfg = h.chain_config()
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    assert got["stage"][0] == 0 and got["status"][0] == 1
    nv = int(got["n_out"][0])
    assert 40 <= nv <= 90, nv
    want = steps_one_by_one(h, hs, sc, 0, cfg)
    assert want["stage"] == 0, (0, want["stage"])
    assert want["nv"] == nv
    ref = OC.solve_batch(OC.params(eps_abs=1e-9, eps_rel=1e-9, max_iter=200000), want["ref"][:, :nv].copy(), want["bounds"][:, :nv].copy(), want["scal"], passes=1)
    assert ref["solved"] == 1
    assert np.abs(got["out"][0, :nv, 3:5] - ref["out"][0, :, 3:5]).max() < 1e-4
    assert np.abs(got["out"][0, :nv, 0:2] - ref["out"][0, :, 0:2]).max() < 1e-4
    h.close(); hs.close()


def test_capacities_beyond_the_register_kernels(hip_lib):
    """pqp_chain_config has no upper bounds (the reference has none): 300 samples are more than TensionSmoother2's generic core holds (203),
    400 layers more than postSmooth's (251), 600 waypoints more than the lane-per-waypoint kernel's (512 - the handle is created for them;
    a line this short still runs there).  Same paths as with the default capacities; a smoother handle in the reference's ADMM setting gets
    the exact kernels where the generic core does not fit instead of PQP_ERR_CAPACITY."""
    sc = scenarios(3, n_maps=2, seed=33)
    h = capi.Handle(capi.production_params(), max_batch=3, max_n=600)
    hs = capi.Handle(smoother_params(), max_batch=3, max_n=400)
    big_cfg = h.chain_config(raw_max=400, sample_max=300, layer_max=400, n_max=600)
    for method in (capi.SMOOTHING_TENSION2, capi.SMOOTHING_TENSION):
        cfg0 = h.chain_config(smoothing_method=method)
        cfg1 = h.chain_config(raw_max=400, sample_max=300, layer_max=400, n_max=600, smoothing_method=method)
        a = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg0)
        b = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg1)
        assert (a["stage"] == 0).all() and (b["stage"] == 0).all() and (b["status"] == 1).all()
        assert np.array_equal(a["n_out"], b["n_out"])
        for q in range(3):
            nv = int(a["n_out"][q])
            assert np.abs(a["out"][q, :nv] - b["out"][q, :nv]).max() < 1e-7, (method, q)
    plain = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3), max_batch=3, max_n=400)       # the reference's smoother setting
    c = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=plain, cfg=big_cfg)
    assert (c["stage"] == 0).all() and (c["status"] == 1).all()
    h.close(); hs.close(); plain.close()


def test_the_tension_smoothing_method(hip_lib):
    """FLAGS_smoothing_method = TENSION (planning_flags.cpp:27, ReferencePathSmoother::create reference_path_smoother.cpp:18-29): the chain
    looks the clearance of the raw line's samples up on the device and runs TensionSmoother's QP (tension_smoother.cpp:49-177) in place of
    TensionSmoother2's; against the steps run one scenario at a time with the clearance from the oracle's grid_map restatement."""
    B = 10
    sc = scenarios(B, seed=11)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=B, max_n=128)
    cfg = h.chain_config(smoothing_method=capi.SMOOTHING_TENSION)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg)
    assert (got["stage"] == 0).sum() >= B - 2, got["stage"]
    base = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs)
    differs = 0
    for b in range(B):
        if got["stage"][b] != 0:
            continue
        want = steps_one_by_one(h, hs, sc, b, cfg)
        assert want["stage"] == 0, (b, want["stage"])
        nv = want["nv"]
        assert got["n_out"][b] == nv and got["status"][b] == want["status"] == 1
        # (TensionSmoother's QP is ill-conditioned - test_tension: both sides sit on a ~1e-5 round-off floor of the smoothed line)
        assert np.abs(got["out"][b, :nv] - want["out"][:nv]).max() < 2e-4, (b, np.abs(got["out"][b, :nv] - want["out"][:nv]).max())
        if base["stage"][b] == 0 and (base["n_out"][b] != nv or np.abs(base["out"][b, :nv] - got["out"][b, :nv]).max() > 1e-3):
            differs += 1
    assert differs >= 1                           # it is another smoother: the paths are not the TENSION2 ones
    with pytest.raises(capi.PqpError):             # "No such smoother!" (reference_path_smoother.cpp:25-28)
        h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=h.chain_config(smoothing_method=7))
    h.close(); hs.close()


def test_chain_carries_the_previous_planning_cycle(hip_lib):
    """PQP_OPT_CARRY_CYCLES through the whole device-resident chain: the vehicle advances a little every cycle (start pose and input points move), so
    the raw line, the layer and waypoint counts of a scenario change from call to call - the path QP's warm state is kept per waypoint, the exact
    smoother kernels start from their slot's previous active set.  Every cycle's paths equal those of handles that start cold (what the carried
    start saves is time: tools/bench_full_chain.py --carry, 892 k -> 989 k scenarios/s)."""
    B = 24
    sc = scenarios(B, seed=21)
    pair = lambda: (capi.Handle(capi.production_params(), max_batch=B, max_n=256), capi.Handle(smoother_params(), max_batch=B, max_n=128))
    h, hs = pair(); hc, hsc = pair()
    for x in (hc, hsc):
        x.set_option(capi.OPT_CARRY_CYCLES, 1)
    rng = np.random.default_rng(3)
    counts = []
    for cycle in range(4):
        pts = sc["pts"].copy(); start = sc["start"].copy()
        if cycle:
            pts[:, :, 1] += rng.normal(scale=0.02, size=pts.shape[:2]) * (pts[:, :, 0] != 0)
            start[:, :2] += rng.normal(scale=0.05, size=(B, 2)); start[:, 2] += rng.normal(scale=0.01, size=B)
        a = (pts, sc["n_pts"], start, sc["target"], sc["dist"], sc["geom"])
        cold = h.optimize_path(*a, map_of=sc["map_of"], smoother=hs)
        got = hc.optimize_path(*a, map_of=sc["map_of"], smoother=hsc)
        np.testing.assert_array_equal(got["stage"], cold["stage"]); np.testing.assert_array_equal(got["n_out"], cold["n_out"])
        np.testing.assert_array_equal(got["status"], cold["status"])
        ok = np.flatnonzero(cold["stage"] == 0)
        assert len(ok) >= B - 4
        for b in ok:
            nv = cold["n_out"][b]
            assert np.abs(got["out"][b, :nv] - cold["out"][b, :nv]).max() < 2e-5, (cycle, b, np.abs(got["out"][b, :nv] - cold["out"][b, :nv]).max())
        counts.append(cold["n_out"].copy())
    assert any((counts[k] != counts[0]).any() for k in range(1, 4))          # the waypoint counts did move between the cycles
    for x in (h, hs, hc, hsc):
        x.close()


def test_stages_are_the_reference_s_return_false_sites(hip_lib):
    sc = scenarios(6, seed=9)
    sc["n_pts"][1] = 3                                               # "Few reference points" (reference_path_smoother.cpp:33-36)
    sc["start"][2, :2] += np.array([-np.sin(sc["start"][2, 2]), np.cos(sc["start"][2, 2])]) * 14.0      # 14 m beside the line: graphSearchDp quits
    sc["start"][3, 2] += 1.6                                         # 92 degrees off the line's heading: path_optimizer.cpp:113-116
    h = capi.Handle(capi.production_params(), max_batch=6, max_n=256)
    hs = capi.Handle(smoother_params(), max_batch=6, max_n=128)
    got = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs)
    assert got["stage"][1] == 1 and got["stage"][2] == 3 and got["stage"][3] == 6, got["stage"]
    for b in (1, 2, 3):
        assert got["status"][b] == 0 and got["n_out"][b] == 0
    for b in (0, 4, 5):
        assert got["stage"][b] == 0 and got["status"][b] == 1 and got["n_out"][b] >= 2 and np.isfinite(got["out"][b]).all()
    # one handle for everything (smoother QPs at the path QP's setting) works too
    alone = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"])
    assert list(alone["stage"]) == list(got["stage"])
    h.close(); hs.close()


def _wrapper_call(hip_lib, name, sc, handles=None):
    """configuration `name` of chain_plan_cases through Handle.optimize_path at the cases' shapes: (the plan, the returned dict, the handles)"""
    import chain_plan_cases as cases
    import chain_util
    on_grid, kw = cases.configs(hip_lib, sc["start"], sc["target"])[name]
    assert not on_grid
    h, hs = handles or chain_util.handles(cases.B, max_n=(cases.N_MAX, cases.N_MAX))
    kw = dict(kw, map_of=sc["map_of"], smoother=hs, cfg=h.chain_config(**cases.CHAIN_CONFIG))
    plan = h._chain_plan(points=sc["pts"], n_points=sc["n_pts"], start=sc["start"], target=sc["target"], geom=sc["geom"], **kw)
    return plan, h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], **kw), (h, hs)


@pytest.mark.parametrize("name", ["d", "d_winners", "h", "j", "j_winners", "k"])
def test_the_wrapper_returns_what_its_plan_says(hip_lib, name):
    """the dict Handle.optimize_path returns has exactly the plan's keys, in its order, with its shapes and dtypes (the plan's own table
    is pinned without a device in test_chain_plan.py)"""
    plan, res, (h, hs) = _wrapper_call(hip_lib, name, scenarios(4))
    h.close(); hs.close()
    assert [(k, v.shape, str(v.dtype)) for k, v in res.items()] == plan.result
    assert not set(plan.on_device) & set(res)


def test_the_footprint_check_behind_the_chain_repeats_bit_for_bit(hip_lib):
    """free, first_collision and margin of two calls on one pair of handles are the same bits, and those are Handle.footprint_check's on
    the out / n_out the call returned.  (That their zero-fill stands before the call's one synchronize is Handle._chain's structure: the
    fill is far shorter than the chain in front of the check, so no run can show where it stands.)"""
    sc = scenarios(4)
    _, first, handles = _wrapper_call(hip_lib, "b", sc)
    _, again, (h, hs) = _wrapper_call(hip_lib, "b", sc, handles)
    want = h.footprint_check(again["out"], again["n_out"], sc["dist"], sc["geom"], map_of=sc["map_of"], margin=True)
    h.close(); hs.close()
    for k in ("free", "first_collision", "margin"):
        assert first[k].tobytes() == again[k].tobytes() == want[k].tobytes(), k
        assert first[k].shape == want[k].shape and first[k].dtype == want[k].dtype, k


def test_clearance_lookup_on_the_device(hip_lib):
    """pqp_clearance_device = Map::getObstacleDistance at the raw line's points (tension_smoother.cpp:168), against the restatement of
    grid_map's bilinear lookup in the corridor oracle; its output feeds pqp_smooth_tension."""
    import torch
    sc = scenarios(3, n_maps=3, seed=2)
    h = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3), max_batch=3, max_n=64)
    rng = np.random.default_rng(0)
    n = 40
    x = rng.uniform(-30, 30, size=(3, n)); y = rng.uniform(-18, 18, size=(3, n))
    x[0, 0], y[0, 0] = 1e3, 0.0                                   # outside the map: 0 (Map.cpp:17-21)
    dev = torch.device("cuda", 0)
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_dist = t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)
    d_x, d_y, d_map = t(x), t(y), t(np.arange(3), np.int32)
    out = torch.zeros((3, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p = lambda a: capi.C.c_void_p(a.data_ptr())
    assert h.lib.pqp_clearance_device(h._h, 3, n, p(d_x), p(d_y), p(d_dist), p(d_map), capi.C.byref(sc["geom"]), p(out)) == 0
    h.sync()
    got = out.cpu().numpy()
    for b in range(3):
        for i in range(n):
            assert got[b, i] == K.obstacle_distance(sc["dist"][b], sc["geom"], x[b, i], y[b, i])
    assert got[0, 0] == 0.0
    r = h.smooth_tension(np.cumsum(np.ones((3, n)), axis=1), np.zeros((3, n)), np.zeros((3, n)), got)
    assert (r["status"] == 1).all()
    h.close()


def test_chain_replayed_as_a_hip_graph_is_bit_identical(hip_lib):
    """PQP_OPT_CHAIN_GRAPH: the chain's ~25 launches on two streams captured once per argument set and replayed (csrc/pqp_chain.hip).  Same
    device buffers call after call, their CONTENTS moving like planning cycles: every call's result equals the plainly launched chain's bit for bit -
    through the plain first calls, the two captures (one per parity of the cost-order double buffer) and the replays - and other arguments fall
    back to plain launches."""
    import torch
    B = 40
    sc = scenarios(B, seed=11)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: capi.C.c_void_p(x.data_ptr())
    d_np, d_tg, d_map = t(sc["n_pts"], np.int32), t(sc["target"], np.float64), t(sc["map_of"], np.int32)
    d_dist = t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)
    rng = np.random.default_rng(3)
    cycles = []
    for _ in range(9):
        pv = sc["pts"].copy(); pv[:, :, 1] += rng.normal(scale=0.02, size=pv.shape[:2]) * (pv[:, :, 0] != 0)
        sv = sc["start"].copy(); sv[:, :2] += rng.normal(scale=0.05, size=(B, 2))
        cycles.append((pv, sv))
    results = {}
    for graph in (0, 1, 2):          # 2: replays without the fences against the smoother handle's stream (this test syncs both streams after every call)
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=256)
        hs = capi.Handle(smoother_params(), device=0, max_batch=B, max_n=128)
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_ORDER_BY_COST, 1); h.set_option(capi.OPT_CHAIN_GRAPH, graph)
        cfg = h.chain_config(raw_max=64, sample_max=48, layer_max=32, n_max=128)
        d_pts, d_st = t(cycles[0][0], np.float64), t(cycles[0][1], np.float64)
        out = torch.zeros((B, cfg.n_max, 7), dtype=torch.float64, device=dev)
        n_out, status, stage, iters = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
        got = []
        for pv, sv in cycles:
            d_pts.copy_(torch.from_numpy(pv)); d_st.copy_(torch.from_numpy(sv))
            torch.cuda.synchronize()
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, capi.C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    capi.C.byref(sc["geom"]), None, p(out), p(n_out), p(status), p(stage), p(iters)))
            h.sync(); hs.sync()
            got.append((out.cpu().numpy().copy(), n_out.cpu().numpy().copy(), status.cpu().numpy().copy(), stage.cpu().numpy().copy()))
        if graph:
            # other arguments (another output buffer): not the captured graph's - plain launches, same result as the last cycle's
            out2 = torch.zeros_like(out)
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, capi.C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    capi.C.byref(sc["geom"]), None, p(out2), p(n_out), p(status), p(stage), p(iters)))
            h.sync(); hs.sync()
            o2, no = out2.cpu().numpy(), got[-1][1]
            for b in range(B):          # (rows beyond a scenario's waypoint count are not written: the long-lived buffer keeps older cycles' rows there)
                np.testing.assert_array_equal(o2[b, :no[b]], got[-1][0][b, :no[b]])
            # and the handle still solves plain batches afterwards (the ticket counter of the path kernel was reset inside the graph)
            from path_optimizer_2_amd.synth import make_batch
            b = make_batch(16, 80)
            r = h.solve(b["ref"], b["bounds"], b["scal"], passes=1)
            assert (r["status"] == 1).all()
        results[graph] = got
        h.close(); hs.close()
    assert (results[0][0][3] == 0).sum() >= B // 2          # most scenarios give a path
    for k in range(len(cycles)):
        for g in (1, 2):
            for a, b_ in zip(results[0][k], results[g][k]):
                np.testing.assert_array_equal(a, b_)


@pytest.mark.gpu
def test_chain_graph_on_the_lane_per_qp_kernel_leaves_the_ticket_counter_alone(hip_lib):
    """A captured chain whose path solve runs on path_stream_kernel (PQP_OPT_STREAM_BATCH reached) never touches the lane-per-waypoint kernel's
    ticket counter: plain pqp_path_solve calls on the same handle between two replays keep working (round 4's replay rewound the host's
    ticket base to the value at capture time - the next plain launch then drew only tickets beyond its batch and solved nothing), and the
    replays stay bit-identical to plain launches."""
    import torch
    from path_optimizer_2_amd.synth import make_batch
    B = 24
    sc = scenarios(B, seed=5)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: capi.C.c_void_p(x.data_ptr())
    d_np, d_tg, d_map = t(sc["n_pts"], np.int32), t(sc["target"], np.float64), t(sc["map_of"], np.int32)
    d_dist = t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)
    plain = make_batch(16, 80)
    ref_h = capi.Handle(capi.production_params(), device=0, max_batch=16, max_n=80)
    want = ref_h.solve(plain["ref"], plain["bounds"], plain["scal"], passes=1)
    ref_h.close()
    results = {}
    for graph in (0, 1):
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=256)
        hs = capi.Handle(smoother_params(), device=0, max_batch=B, max_n=128)
        h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_STREAM_BATCH, 1); h.set_option(capi.OPT_CHAIN_GRAPH, graph)
        cfg = h.chain_config(raw_max=64, sample_max=48, layer_max=32, n_max=128)
        d_pts, d_st = t(sc["pts"], np.float64), t(sc["start"], np.float64)
        out = torch.zeros((B, cfg.n_max, 7), dtype=torch.float64, device=dev)
        n_out, status, stage, iters = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4))
        got = []
        for cycle in range(6):
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, capi.C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    capi.C.byref(sc["geom"]), None, p(out), p(n_out), p(status), p(stage), p(iters)))
            h.sync(); hs.sync()
            assert h.last_path_kernel() == capi.KERNEL_LANE_PER_QP
            got.append((out.cpu().numpy().copy(), n_out.cpu().numpy().copy(), status.cpu().numpy().copy()))
            # plain solves on the lane-per-waypoint kernel in between (the option is put back before the next chain call: same key)
            h.set_option(capi.OPT_STREAM_BATCH, 0)
            for _ in range(1 + cycle % 2):
                r = h.solve(plain["ref"], plain["bounds"], plain["scal"], passes=1)
                assert h.last_path_kernel() == capi.KERNEL_LANE_PER_WAYPOINT
                assert (r["status"] == 1).all(), (graph, cycle, r["status"])
                np.testing.assert_array_equal(r["out"], want["out"])
            h.set_option(capi.OPT_STREAM_BATCH, 1)
        results[graph] = got
        h.close(); hs.close()
    assert (results[0][0][2] == 1).sum() >= B // 2          # most scenarios give a path
    for k in range(6):
        for a, b_ in zip(results[0][k], results[1][k]):
            np.testing.assert_array_equal(a, b_)


def test_chain_graph_is_not_replayed_after_the_smoother_handle_reallocates(hip_lib):
    """The library's allocation generation is one counter, whichever translation unit a buffer grows in: a captured chain holds device pointers of
    both handles' workspaces, and a smoother call that makes the smoother handle reallocate (pqp_smoothers.hip) must keep pqp_optimize_path_device
    (pqp_chain.hip) from replaying it.  Replay, grow the smoother handle's buffers, call the chain again: bit for bit a fresh pair's plain chain."""
    import torch
    B = 4
    sc = scenarios(B, seed=7)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: capi.C.c_void_p(x.data_ptr())
    d_pts, d_np, d_st, d_tg, d_map = t(sc["pts"], np.float64), t(sc["n_pts"], np.int32), t(sc["start"], np.float64), t(sc["target"], np.float64), t(sc["map_of"], np.int32)
    d_dist = t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)

    def pair(graph):
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=256)
        hs = capi.Handle(smoother_params(), device=0, max_batch=B, max_n=128)
        h.set_option(capi.OPT_CHAIN_GRAPH, graph); hs.set_option(capi.OPT_CHAIN_GRAPH, graph)
        out = torch.zeros((B, 256, 7), dtype=torch.float64, device=dev)
        ints = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]          # n_out, status, stage, iters
        cfg = h.chain_config()                                                            # default-sized scenarios: n_max = 256

        def run():
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, capi.C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    capi.C.byref(sc["geom"]), None, p(out), *(p(x) for x in ints)))
            h.sync(); hs.sync()
            return [out.cpu().numpy().copy()] + [x.cpu().numpy().copy() for x in ints]
        return h, hs, run

    h0, hs0, run0 = pair(0)
    want = run0()
    h0.close(); hs0.close()
    assert (want[3] == 0).sum() >= B // 2          # most scenarios give a path
    h, hs, run = pair(1)
    # until the chain replays: a call launched as a graph records no timing events (pqp_last_kernel_ms has nothing to report), and of three such
    # calls in a row at most two are captures (one per parity of the path handle's solve count), so the third is a replay
    ms, in_a_row = capi.C.c_float(), 0
    for _ in range(12):
        got = run()
        for a, b_ in zip(want, got):
            np.testing.assert_array_equal(a, b_)
        in_a_row = in_a_row + 1 if h.lib.pqp_last_kernel_ms(h._h, capi.C.byref(ms)) != 0 else 0
        if in_a_row == 3:
            break
    assert in_a_row == 3, "the chain never replayed"
    # the smoother handle reallocates: a batch larger than anything it has seen
    n = 32
    s = np.tile(np.arange(n, dtype=np.float64), (64, 1))
    y = 0.3 * np.sin(0.2 * s) + 0.01 * np.arange(64)[:, None]
    sm = hs.smooth_tension2(s.copy(), y, np.arctan(0.06 * np.cos(0.2 * s)), np.zeros_like(s), s.copy())
    assert (sm["status"] == 1).all(), sm["status"]
    got = run()
    for a, b_ in zip(want, got):
        np.testing.assert_array_equal(a, b_)
    h.close(); hs.close()


def test_chain_graph_is_never_replayed_after_an_option_changed(hip_lib):
    """Every option of both handles is part of the chain's graph key (csrc/pqp_internal.hpp: Options goes in as bytes).  Replay, then for each
    option in turn: set it to another value, call once - the call must be launched plainly (it records timing events: pqp_last_kernel_ms succeeds;
    a capture or a replay records none) and give, bit for bit below each scenario's n_out, what a fresh pair with the same options and the graph
    option off gives - and set it back.  The fresh pair is driven through the same calls and option changes (a replay is bit-identical to plain
    launches, above), so what PQP_OPT_CARRY_CYCLES carries from the earlier calls is the same on both sides.
    (Not seen here: that PQP_OPT_STREAM_STAGED is in the key - both workspace layouts give the same bits and a capture is as silent as a replay.)"""
    import torch
    B = 4
    sc = scenarios(B, seed=7)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: capi.C.c_void_p(x.data_ptr())
    d_pts, d_np, d_st, d_tg, d_map = t(sc["pts"], np.float64), t(sc["n_pts"], np.int32), t(sc["start"], np.float64), t(sc["target"], np.float64), t(sc["map_of"], np.int32)
    d_dist = t(np.transpose(sc["dist"], (0, 2, 1)), np.float32)
    # (handle, option, another value than its default, its default)
    changes = [("path", capi.OPT_STORE_WARM, 0, 1), ("path", capi.OPT_ORDER_BY_COST, 1, 0), ("path", capi.OPT_RESERVE_CUS, 8, 0), ("path", capi.OPT_STREAM_BATCH, 1, -1),
               ("path", capi.OPT_STREAM_STAGED, 1, -1), ("path", capi.OPT_CARRY_CYCLES, 1, 0), ("path", capi.OPT_LONG_LINES, 2, 0),
               ("smoother", capi.OPT_CARRY_CYCLES, 1, 0), ("smoother", capi.OPT_LONG_LINES, 2, 0)]

    def session(graph, warm_up):
        """warm_up None: call until the chain replays; else: that many calls.  Then one call per changed option: (results, launched plainly)."""
        h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=128)
        hs = capi.Handle(smoother_params(), device=0, max_batch=B, max_n=128)
        h.set_option(capi.OPT_CHAIN_GRAPH, graph); hs.set_option(capi.OPT_CHAIN_GRAPH, graph)
        cfg = h.chain_config(raw_max=64, sample_max=48, layer_max=32, n_max=128)
        out = torch.zeros((B, cfg.n_max, 7), dtype=torch.float64, device=dev)
        ints = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]          # n_out, status, stage, iters
        ms = capi.C.c_float()

        def run():
            h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, capi.C.byref(cfg), B, sc["pts"].shape[1], p(d_pts), p(d_np), p(d_st), p(d_tg), p(d_dist), p(d_map),
                                                    capi.C.byref(sc["geom"]), None, p(out), *(p(x) for x in ints)))
            h.sync(); hs.sync()
            return dict(out=out.cpu().numpy().copy(), n_out=ints[0].cpu().numpy().copy(), status=ints[1].cpu().numpy().copy(), stage=ints[2].cpu().numpy().copy())

        calls, in_a_row = 0, 0
        while (calls < 12 and in_a_row < 3) if warm_up is None else calls < warm_up:
            run()
            calls += 1
            # (three calls in a row without timing events: at most two of them are captures, one per parity of the path handle's solve count)
            in_a_row = in_a_row + 1 if h.lib.pqp_last_kernel_ms(h._h, capi.C.byref(ms)) != 0 else 0
        if warm_up is None:
            assert in_a_row == 3, "the chain never replayed"
        got = []
        for which, option, value, default in changes:
            x = h if which == "path" else hs
            x.set_option(option, value)
            r = run()
            got.append((r, h.lib.pqp_last_kernel_ms(h._h, capi.C.byref(ms)) == 0))
            x.set_option(option, default)
        h.close(); hs.close()
        return calls, got

    calls, with_graph = session(1, None)
    _, plain = session(0, calls)
    assert (plain[0][0]["stage"] == 0).sum() >= B // 2          # most scenarios give a path
    for (which, option, value, _), (g, launched_plainly), (w, _) in zip(changes, with_graph, plain):
        assert launched_plainly, (which, option, value)
        for k in ("n_out", "status", "stage"):
            np.testing.assert_array_equal(g[k], w[k], err_msg=str((which, option, k)))
        for b in range(B):
            np.testing.assert_array_equal(g["out"][b, :w["n_out"][b]], w["out"][b, :w["n_out"][b]], err_msg=str((which, option, b)))
