"""The device chain (csrc/pqp_chain.hip) as the tests drive it: its scenarios, its pair of handles, and its steps restated twice -
steps_one_by_one(): one scenario at exact sizes through the host entry points, with every stop site; steps_on_device(): the whole batch
at the chain's own capacities through the `_device` entry points, with the second pass composed by hand.  The two restatements are
independent of each other on purpose; a change of the chain's steps has to visit both, here.
(pytest does not rewrite the asserts of a helper module: each one here carries its own message.)"""
import ctypes as C

import numpy as np

import corridor_oracle as K
from chain_stops_util import (BLOCKED, CAPACITY, FEW_POINTS, HEADING, OK, PATH_QP_FAILED, POST_SMOOTH_FAILED, SEARCH_FAILED, SHORT_REFERENCE,
                              SMOOTHER_FAILED, sample_min)
from device_form import call as _call, dev as _dev, to_device as _t
from path_optimizer_2_amd import capi
from path_optimizer_2_amd.synth import make_scene


def smoother_params():
    # the reference's smoother setting (OSQP default eps 1e-3) + the KKT-verified polish, so that both sides return the QP's optimum
    return capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25)


def scenarios(B, n_maps=4, seed=5):
    cs = [make_scene(seed=s, n=40, n_obstacles=25, knots_every=3.05) for s in range(n_maps)]
    rng = np.random.default_rng(seed)
    p_max = len(cs[0]["knots_x"])
    pts = np.zeros((B, p_max, 2)); n_pts = np.zeros(B, dtype=np.int32); map_of = (np.arange(B) % n_maps).astype(np.int32)
    start = np.zeros((B, 3)); target = np.zeros((B, 3))
    for b in range(B):
        c = cs[b % n_maps]
        P = int(rng.integers(7, p_max + 1))                       # polygons of different length: every count downstream differs
        n_pts[b] = P
        pts[b, :P, 0] = c["knots_x"][:P]; pts[b, :P, 1] = c["knots_y"][:P] + rng.normal(scale=0.15, size=P)
        h0 = np.arctan2(pts[b, 1, 1] - pts[b, 0, 1], pts[b, 1, 0] - pts[b, 0, 0])
        start[b] = (pts[b, 0, 0] + 0.1, pts[b, 0, 1] + 0.1, h0 + 0.03)
        h1 = np.arctan2(pts[b, P - 1, 1] - pts[b, P - 2, 1], pts[b, P - 1, 0] - pts[b, P - 2, 0])
        target[b] = (pts[b, P - 1, 0], pts[b, P - 1, 1], h1)
    c0 = cs[0]
    geom = capi.PqpGridGeometry(c0["rows"], c0["cols"], c0["resolution"], c0["length"][0], c0["length"][1], c0["pos"][0], c0["pos"][1])
    return dict(pts=pts, n_pts=n_pts, map_of=map_of, start=start, target=target, dist=np.stack([c["dist"] for c in cs]), geom=geom)


def handles(B, max_n=(256, 128), path_params=None, smoother_params=None):
    """(path handle, smoother handle) for a batch of B: the production path QP and the reference's smoother setting unless given"""
    return (capi.Handle(path_params or capi.production_params(), max_batch=B, max_n=max_n[0]),
            capi.Handle(smoother_params or _reference_smoother(), max_batch=B, max_n=max_n[1]))


_reference_smoother = smoother_params          # (handles() has an argument of that name)


# ---- the chain, one scenario and one step at a time -------------------------------------------------------------------------------------
def steps_one_by_one(h, hs, sc, b, cfg, p_max=None):
    """The chain for scenario b alone, exact sizes, through the per-step host-pointer entry points (each pinned to its oracle elsewhere),
    and where it stops: dict(stage, status, site) - site names the capacity for stage 9 - plus, where a path QP ran, nv and out, the counts
    of the steps before it (n0 raw points, n1 samples, layers, count reference states) and the QP's inputs (ref, bounds, scal).
    The stop sites in the order of the steps (the reference's `return false` sites and what stands in their way here):
      n_points < 4                                   FEW_POINTS       reference_path_smoother.cpp:33-36
      n_points > p_max, or not above the degree      FEW_POINTS       no raw line: bSpline gives no points (tinyspline refuses the spline)
      raw points > raw_max                           CAPACITY
      samples > sample_max, samples < 3 (TENSION: 4) CAPACITY         (two raw points: a polygon below 1 m, whose 1 m samples are two)
      smoother QP not SOLVED                         SMOOTHER_FAILED
      layers > layer_max                             CAPACITY
      no layer                                       SEARCH_FAILED
      fewer than 4 layers                            SHORT_REFERENCE
      postSmooth QP not SOLVED                       POST_SMOOTH_FAILED
      initial heading error > 75 degrees             HEADING
      reference states > n_max                       CAPACITY
      fewer than 2 waypoints before the road closes  BLOCKED
      path QP not SOLVED                             PATH_QP_FAILED, with its status
    p_max: the width of the batch's point array (None: sc["pts"].shape[1])."""
    P = int(sc["n_pts"][b])
    p_max = sc["pts"].shape[1] if p_max is None else p_max
    mo = sc["map_of"][b:b + 1]
    st, tg = sc["start"][b:b + 1], sc["target"][b:b + 1]
    k0 = float(sc["start_k"][b]) if "start_k" in sc else 0.0
    stop = lambda stage, site=None: dict(stage=stage, status=0, site=site)          # (0: PQP_STATUS_UNSOLVED, the status of a scenario no path QP ran for)
    if P < 4 or P > p_max:
        return stop(FEW_POINTS)
    r = h.bspline_resample(sc["pts"][b:b + 1, :P], np.array([P], dtype=np.int32), cfg.raw_max)
    n0 = int(r["count"][0])
    if n0 == 0:
        return stop(FEW_POINTS)
    if n0 > cfg.raw_max:
        return stop(CAPACITY, "raw_max")
    if n0 < 3:
        # two raw points (t = 0 and t = 1) are what a polygon shorter than 1 m gives: tk::spline takes no such line, and its samples at
        # 0 and 1 m are fewer than any smoother QP takes
        return stop(CAPACITY, "sample_min")
    x0, y0, s0 = (r[k][:, :n0] for k in ("x", "y", "s"))
    tab, ext = h.spline_fit(s0, x0, y0)
    seg = h.segment_raw_reference(tab, ext, s0[:, -1].copy(), cfg.sample_max)
    n1 = int(seg["count"][0])
    if n1 > cfg.sample_max:
        return stop(CAPACITY, "sample_max")
    if n1 < sample_min(cfg.smoothing_method):
        return stop(CAPACITY, "sample_min")
    if cfg.smoothing_method == capi.SMOOTHING_TENSION:
        gx, gy = seg["x"][:, :n1], seg["y"][:, :n1]
        clr = np.array([[K.obstacle_distance(sc["dist"][mo[0]], sc["geom"], gx[0, i], gy[0, i]) for i in range(n1)]])      # Map::getObstacleDistance, the oracle's
        sm = hs.smooth_tension(gx, gy, seg["angle"][:, :n1], clr)
    else:
        sm = hs.smooth_tension2(*(seg[k][:, :n1] for k in ("x", "y", "angle", "k", "s")))
    if sm["status"][0] != 1:
        return stop(SMOOTHER_FAILED)
    tab, ext = h.spline_fit(sm["s"], sm["x"], sm["y"])
    ls, lb, ub, cnt, vl = h.dp_corridor(tab, ext, sm["s"][:, -1] + cfg.smoothed_length_margin, st, sc["dist"], sc["geom"], max_layers=cfg.layer_max, map_of=mo)
    k = int(cnt[0])
    if k < 0:
        return stop(CAPACITY, "layer_max")
    if k == 0:
        return stop(SEARCH_FAILED)
    if k < 4:
        return stop(SHORT_REFERENCE)
    ps = hs.post_smooth(ls[:, :k].copy(), lb[:, :k].copy(), ub[:, :k].copy(), vl)
    if ps["status"][0] != 1:
        return stop(POST_SMOOTH_FAILED)
    x2, y2, s2 = h.offsets_to_points(tab, ext, ls[:, :k].copy(), ps["l"])
    tab, ext = h.spline_fit(s2, x2, y2)
    max_s = h.reference_length(tab, ext, s2[:, -1].copy(), tg)
    ref, count, err = h.reference_states(tab, ext, max_s, cfg.n_max, start=st, ds_small=cfg.output_spacing / 2, ds_large=cfg.output_spacing, dynamic=True)
    if abs(err[0, 1]) > 75.0 * np.pi / 180.0:
        return stop(HEADING)
    if count[0] > cfg.n_max:
        return stop(CAPACITY, "n_max")
    bounds, nv = h.corridor_bounds(ref, tab, ext, sc["dist"], sc["geom"], map_of=mo, n_of=count)
    if nv[0] < 2:
        return stop(BLOCKED)
    scal = np.array([[err[0, 0], err[0, 1], k0, tg[0, 2], 1.0 if nv[0] < count[0] else 0.0, cfg.max_steering_angle]])
    res = h.solve_var(nv, ref, bounds, scal, passes=1)
    status = int(res["status"][0])
    return dict(stage=OK if status == 1 else PATH_QP_FAILED, status=status, site=None, nv=int(nv[0]), out=res["out"][0],
                n0=n0, n1=n1, layers=k, count=int(count[0]), ref=ref, bounds=bounds, scal=scal)


# ---- the chain, the whole batch on the device entry points ---------------------------------------------------------------------------------
def steps_on_device(h, hs, sc, cfg):
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
