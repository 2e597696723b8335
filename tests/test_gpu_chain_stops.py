"""pqp_optimize_path_device on a batch that mixes healthy scenarios with scenarios stopped at every stop site the chain has
(tests/chain_stops_util.py builds them, tests/test_chain_stops_cpu.py shows with the oracle that they are what they claim): the stage,
status and waypoint count of every scenario against the steps run one scenario at a time, and that a stopped scenario stays contained -
its batch neighbours' rows do not move by a bit, nothing is written outside the output arrays, what the handles ran before does not
matter, a replayed graph gives the same, and the steps behind the chain never pick a stopped candidate.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import chain_stops_util as CS
import chain_util
import sample_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu

C = capi.C
METHODS = [capi.SMOOTHING_TENSION2, capi.SMOOTHING_TENSION]
B = len(CS._PLAN)


@pytest.fixture(scope="module")
def batch(hip_lib):
    return CS.mixed_batch()


def _cfg(h, method=capi.SMOOTHING_TENSION2, **over):
    return h.chain_config(**{**CS.MIXED_CFG, "smoothing_method": method, **over})


def _run(h, hs, sc, cfg, **kw):
    return h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, cfg=cfg,
                           start_k=sc["start_k"], **kw)


def _same_rows(a, b, rows, keys=("out", "n_out", "status", "stage", "iters")):
    for k in keys:
        assert same_bits(a[k][rows], b[k][rows]) if a[k].dtype == np.float64 else np.array_equal(a[k][rows], b[k][rows]), k


def _against_the_steps(got, h, hs, sc, cfg, tol):
    """stage, status and n_out of every scenario against the steps run one by one; the path where one comes out.  Returns the steps' answers."""
    want = [chain_util.steps_one_by_one(h, hs, sc, b, cfg) for b in range(B)]
    for b, w in enumerate(want):
        print(b, sc["kind"][b], "chain:", got["stage"][b], got["status"][b], got["n_out"][b], " steps:", w["stage"], w["status"], w.get("site"), w.get("nv"))
    for b, w in enumerate(want):
        assert got["stage"][b] == w["stage"] and got["status"][b] == w["status"], (b, sc["kind"][b], got["stage"][b], got["status"][b], w["stage"], w["status"])
        if w["stage"] == CS.OK:
            nv = w["nv"]
            assert got["status"][b] == 1 and got["n_out"][b] == nv >= 2
            assert np.isfinite(got["out"][b]).all()
            assert np.abs(got["out"][b, :nv] - w["out"][:nv]).max() < tol, (b, np.abs(got["out"][b, :nv] - w["out"][:nv]).max())
            assert np.all(got["out"][b, nv:] == 0.0)
        else:
            assert got["n_out"][b] == 0
            assert (got["status"][b] not in (0, 1)) if w["stage"] == CS.PATH_QP_FAILED else got["status"][b] == 0
    return want


# ---- a: every site, both smoothing methods -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_every_stop_site(batch, method):
    """Stages reached, each by a scenario (or a handle) built for it: 0, 1 FEW_POINTS (n_points 3, 0, -1; n_points = p_max + 1; 4 and 5 points
    3 m apart), 2 SMOOTHER_FAILED (a smoother handle with max_iter = 2 and no polish: every scenario that gets to the smoother QP), 3, 4, 6,
    7 BLOCKED and 8 PATH_QP_FAILED under the default RELINEARISE pass (8 twice: start_k = NaN in one scenario, status NUMERICAL; and a path
    handle with max_iter = 3 and no polish, status MAX_ITER, for every scenario that gets to the path QP), 9 CAPACITY at each of its five sites
    by a scenario of its own: raw points > raw_max, samples > sample_max, samples below the smoother's minimum, layers > layer_max,
    reference states > n_max.
    Stage 5 POST_SMOOTH_FAILED is reached too, though it sits behind stage 2 on the same handle: with the vehicle 2 m beside the line, a
    smoother handle without polish and with max_iter = 75 solves the tension QP and not postSmooth's, which has to bring the line from the
    vehicle's offset back to the centre.  (Measured, the oracle has no QPs: offsets of 1, 2 and 3 m and limits of 50, 75 and 100 iterations
    all stop the same three of the four healthy polygons there, in the chain and in the steps, with both smoothers; the middle of both is used.)
    A NaN among the input points is no way to stage 2: the raw line then has 2 points, which stops at the sample minimum.
    (TensionSmoother's QP is ill-conditioned: 2e-4 against the steps there, as test_gpu_chain.py has it; 2e-5 for TensionSmoother2.)"""
    sc = batch
    tol = 2e-4 if method == capi.SMOOTHING_TENSION else 2e-5
    h, hs = chain_util.handles(B)
    cfg = _cfg(h, method)
    got = _run(h, hs, sc, cfg)
    want = _against_the_steps(got, h, hs, sc, cfg, tol)
    # every scenario stops where it was built to stop, the five capacity sites each by their own scenario
    for b, kind in enumerate(sc["kind"]):
        assert got["stage"][b] == CS.INTENDED[kind], (b, kind, got["stage"][b])
        if kind.startswith("cap_"):
            assert want[b]["site"] == kind[4:], (b, kind, want[b]["site"])
    assert {want[b]["site"] for b in range(B)} - {None} == set(CS.CAPACITY_SITES)
    assert (got["stage"] == 0).sum() >= 4
    nan_row = sc["kind"].index("qp_nan")
    assert got["status"][nan_row] == 3                                   # PQP_STATUS_NUMERICAL
    seen = set(got["stage"].tolist())
    # a smoother handle that cannot converge: SMOOTHER_FAILED for whoever gets there, the stops before it unchanged
    weak = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, max_iter=2, polish=0), max_batch=B, max_n=128)
    g2 = _run(h, weak, sc, cfg)
    _against_the_steps(g2, h, weak, sc, cfg, tol)
    early = np.isin(got["stage"], (1, 9)) & np.array([k not in ("cap_layer_max", "cap_n_max") for k in sc["kind"]])
    assert np.array_equal(g2["stage"][early], got["stage"][early]) and (g2["stage"][~early] == 2).all(), g2["stage"]
    seen |= set(g2["stage"].tolist())
    weak.close()
    # a path handle that cannot converge: PATH_QP_FAILED with the QP's status for whoever gets there
    hf = capi.Handle(capi.production_params(max_iter=3, polish=0), max_batch=B, max_n=256)
    g3 = _run(hf, hs, sc, cfg)
    _against_the_steps(g3, hf, hs, sc, cfg, tol)
    reached = np.isin(got["stage"], (0, 8))
    assert np.array_equal(g3["stage"][~reached], got["stage"][~reached]) and (g3["stage"][reached] == 8).all(), g3["stage"]
    assert (g3["status"][sc["healthy"]] == 2).all()                      # PQP_STATUS_MAX_ITER
    seen |= set(g3["stage"].tolist())
    # the vehicle 2 m beside the line, a smoother handle that gets through the tension QP and not through postSmooth's
    beside = CS.all_healthy(sc)
    beside["start"][:, :2] += np.stack([-np.sin(beside["start"][:, 2]), np.cos(beside["start"][:, 2])], 1) * 2.0
    slow = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, max_iter=75, polish=0), max_batch=B, max_n=128)
    g5 = _run(h, slow, beside, cfg)
    _against_the_steps(g5, h, slow, beside, cfg, tol)
    assert (g5["stage"] == 5).sum() >= B // 2 and set(g5["stage"].tolist()) <= {0, 5}, g5["stage"]
    seen |= set(g5["stage"].tolist())
    slow.close()
    assert seen == {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, seen
    h.close(); hs.close(); hf.close()


# ---- b: containment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_stopped_scenarios_leave_their_neighbours_alone(batch, method):
    """The mixed batch, then the same call with every stopped scenario replaced by a copy of a healthy one (same batch size, configuration
    and handles): the healthy scenarios' rows of out, n_out, status, stage and iters are the same bits - every kernel of the chain works per
    scenario, none of its results depends on the batch neighbours."""
    sc = batch
    h, hs = chain_util.handles(B)
    cfg = _cfg(h, method)
    mixed = _run(h, hs, sc, cfg)
    clean = _run(h, hs, CS.all_healthy(sc), cfg)
    rows = np.flatnonzero(sc["healthy"])
    assert len(rows) >= 4 and (mixed["stage"][rows] == 0).all() and (clean["stage"] == 0).all() and (clean["status"] == 1).all()
    _same_rows(mixed, clean, rows)
    for b in rows:
        assert np.isfinite(mixed["out"][b]).all() and np.all(mixed["out"][b, mixed["n_out"][b]:] == 0.0)
    assert (mixed["n_out"][~sc["healthy"]] == 0).all()
    h.close(); hs.close()


# ---- c, e: the raw ABI on buffers of the test's own ----------------------------------------------------------------------------------------
F_SENTINEL, I_SENTINEL, PAD = -7.25e300, 0x5A5A5A5A, 64


class _Raw:
    """The mixed call through pqp_optimize_path_device itself.  out, n_out, status, stage and iters lie inside larger buffers filled with a
    sentinel, PAD elements of it before and behind each array."""

    def __init__(self, sc, cfg):
        import torch
        self.torch, self.sc, self.cfg = torch, sc, cfg
        dev = torch.device("cuda", 0)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.inputs = [t(sc["pts"], np.float64), t(sc["n_pts"], np.int32), t(sc["start"], np.float64), t(sc["target"], np.float64),
                       t(np.transpose(sc["dist"], (0, 2, 1)), np.float32), t(sc["map_of"], np.int32)]
        self.start_k = t(sc["start_k"], np.float64)
        self.big = {"out": torch.full((PAD + B * cfg.n_max * 7 + PAD,), F_SENTINEL, dtype=torch.float64, device=dev)}
        for k in ("n_out", "status", "stage", "iters"):
            self.big[k] = torch.full((PAD + B + PAD,), I_SENTINEL, dtype=torch.int32, device=dev)
        self.view = {k: v[PAD:v.numel() - PAD] for k, v in self.big.items()}
        self.view["out"].zero_()
        torch.cuda.synchronize()

    def call(self, h, hs):
        p = lambda x: C.c_void_p(x.data_ptr())
        sc, v = self.sc, self.view
        h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, C.byref(self.cfg), B, sc["pts"].shape[1], *(p(x) for x in self.inputs), C.byref(sc["geom"]),
                                                p(self.start_k), p(v["out"]), p(v["n_out"]), p(v["status"]), p(v["stage"]), p(v["iters"])))
        h.sync(); hs.sync()
        res = {k: x.cpu().numpy().copy() for k, x in v.items()}
        res["out"] = res["out"].reshape(B, self.cfg.n_max, 7)
        return res

    def pads_intact(self):
        for k, v in self.big.items():
            edge = self.torch.cat([v[:PAD], v[v.numel() - PAD:]]).cpu().numpy()
            if not (edge == (F_SENTINEL if k == "out" else I_SENTINEL)).all():
                return False
        return True


@pytest.mark.parametrize("method", METHODS)
def test_nothing_is_written_outside_the_outputs(batch, method):
    sc = batch
    h, hs = chain_util.handles(B)
    cfg = _cfg(h, method)
    want = _run(h, hs, sc, cfg)
    raw = _Raw(sc, cfg)
    got = raw.call(h, hs)
    assert raw.pads_intact()
    assert not (got["n_out"] == I_SENTINEL).any() and not (got["stage"] == I_SENTINEL).any() and not (got["status"] == I_SENTINEL).any()
    _same_rows(got, want, np.arange(B), keys=("n_out", "status", "stage"))
    _same_rows(got, want, np.flatnonzero(want["stage"] == 0))
    assert set(got["stage"].tolist()) == {0, 1, 3, 4, 6, 7, 8, 9}
    h.close(); hs.close()


def test_replayed_graph_gives_the_plain_chain_s_arrays(batch):
    """PQP_OPT_CHAIN_GRAPH = 1 on the mixed batch: five calls on the same buffers - plain, plain (the other parity of the cost-order double
    buffer), capture, capture, replay - each give what the plainly launched chain gives: stage, status and n_out of every scenario, and the
    healthy scenarios' rows of out and iters bit for bit (a stopped scenario's rows of out are unspecified, pqp.h)."""
    sc = batch
    h0, hs0 = chain_util.handles(B)
    cfg = _cfg(h0)
    want = _run(h0, hs0, sc, cfg)
    h0.close(); hs0.close()
    h, hs = chain_util.handles(B)
    h.set_option(capi.OPT_CHAIN_GRAPH, 1)
    raw = _Raw(sc, cfg)
    ms, untimed = C.c_float(), []
    for call in range(5):
        got = raw.call(h, hs)
        _same_rows(got, want, np.arange(B), keys=("n_out", "status", "stage"))
        _same_rows(got, want, np.flatnonzero(want["stage"] == 0))
        untimed.append(h.lib.pqp_last_kernel_ms(h._h, C.byref(ms)) != 0)          # a captured or replayed call records no timing events
    print("calls without timing events:", untimed)
    assert not untimed[0] and untimed[-1] and untimed == sorted(untimed), untimed          # plain first; once captured, never plain again
    assert raw.pads_intact()
    h.close(); hs.close()


# ---- d: what the handles ran before --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_stages_do_not_depend_on_what_the_handles_ran_before(batch, method):
    """The mixed batch on fresh handles; on handles that have just run an all-healthy batch under other capacities, so that the workspace is
    carved differently and every row a stopped scenario's later steps read holds something else; and once more right after itself: stage,
    status and n_out of every scenario are the same, the healthy rows the same bits.  (A scenario without a raw line - n_points above p_max, or
    4 / 5 points 3 m apart - used to get its stage from the sample count of a line whose length was whatever lay in its workspace row.)"""
    sc = batch
    big = dict(raw_max=400, sample_max=300, layer_max=400, n_max=600)
    sizes = (600, 400)
    h, hs = chain_util.handles(B, max_n=sizes)
    cfg = _cfg(h, method)
    fresh = _run(h, hs, sc, cfg)
    h.close(); hs.close()
    h, hs = chain_util.handles(B, max_n=sizes)
    other = _run(h, hs, CS.all_healthy(sc), _cfg(h, method, **big))
    assert (other["stage"] == 0).all()
    after_other = _run(h, hs, sc, cfg)
    again = _run(h, hs, sc, cfg)
    h.close(); hs.close()
    print("fresh", fresh["stage"], "\nafter", after_other["stage"], "\nagain", again["stage"])
    for kind, stage in CS.INTENDED.items():
        rows = [b for b, k in enumerate(sc["kind"]) if k == kind]
        assert (fresh["stage"][rows] == stage).all(), (kind, fresh["stage"][rows])
    for r in (after_other, again):
        _same_rows(r, fresh, np.arange(B), keys=("n_out", "status", "stage"))
        _same_rows(r, fresh, np.flatnonzero(sc["healthy"]))


# ---- f: behind the chain -------------------------------------------------------------------------------------------------------------------
def test_the_steps_behind_the_chain_never_pick_a_stopped_candidate(batch):
    """Footprint check, selection, speed profile and sampler right behind the chain on the mixed batch, in groups that hold stopped and healthy
    candidates and one that holds stopped ones only: the same as the four called one after another on the chain's own outputs; no stopped
    candidate is a group's best; the all-stopped group has best -1, an all-zero best path with best_n 0 (pqp.h) and an EMPTY trajectory."""
    sc = batch
    gs, m = CS.GROUP_START, 12
    groups = len(gs) - 1
    sp, sa = capi.speed_default_params(v_max=8.0), capi.sample_default_params(dt=0.2, hold_last=1)
    vs = np.linspace(1.0, 4.0, groups)
    h, hs = chain_util.handles(B)
    cfg = _cfg(h)
    got = _run(h, hs, sc, cfg, check_footprint=True, select=gs, speed=sp, v_start=vs, sample=sa, samples=m)
    hh = capi.Handle(capi.default_params(), max_batch=B, max_n=cfg.n_max)
    fp = hh.footprint_check(got["out"], got["n_out"], sc["dist"], sc["geom"], map_of=sc["map_of"], margin=True)
    assert np.array_equal(got["free"], fp["free"]) and np.array_equal(got["first_collision"], fp["first_collision"]) and same_bits(got["margin"], fp["margin"])
    sel = hh.select_paths(got["out"], gs, n_of=got["n_out"], status=got["status"], stage=got["stage"], first_collision=got["first_collision"],
                          margin=got["margin"])
    for k in ("terms", "best_paths"):
        assert same_bits(got[k], sel[k]), k
    assert np.array_equal(got["best"], sel["best"]) and np.array_equal(got["best_n"], sel["best_n"])
    prof, flags = hh.speed_profile(got["best_paths"], vs, n_of=got["best_n"], prm=sp)
    assert same_bits(got["profile"], prof) and np.array_equal(got["speed_flags"], flags)
    traj, traj_n, traj_flags = hh.sample_trajectory(got["best_paths"], got["profile"], m, n_of=got["best_n"], prm=sa)
    assert same_bits(got["traj"], traj) and np.array_equal(got["traj_n"], traj_n) and np.array_equal(got["traj_flags"], traj_flags)
    stopped = got["stage"] != 0
    assert np.array_equal(stopped, ~sc["healthy"])
    assert (got["terms"][stopped, 7] == 0.0).all() and (got["terms"][stopped] == 0.0).all()          # count 0: eight zeros, not eligible
    for g in range(groups):
        rows = np.arange(gs[g], gs[g + 1])
        if stopped[rows].all():
            assert g == 1 and got["best"][g] == -1 and got["best_n"][g] == 0 and (got["best_paths"][g] == 0.0).all()
            assert got["traj_flags"][g] == S.EMPTY and got["traj_n"][g] == 0
        else:
            # every healthy candidate here is collision-free or not - the winner, where there is one, is a healthy row of its own group
            eligible = rows[got["terms"][rows, 7] == 1.0]
            assert (got["best"][g] == -1) == (len(eligible) == 0)
            if len(eligible):
                assert got["best"][g] in eligible and not stopped[got["best"][g]]
    assert (got["best"] >= 0).sum() >= 2
    h.close(); hs.close(); hh.close()
