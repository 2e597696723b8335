"""The braking fallback on one GPU: device time per call (the handle's HIP events around each entry point's launches, after warm-up,
median of the timed calls with min and max) at 1024 and 8192 groups x 71 rows x 3 levels - eight layers a second apart, ten sub-steps
each - of the four calls the stage makes behind the ranking, separately and as the sum of one pass through all four:
  pqp_fallback_rows_device          every group's previous plan is a trajectory of 71 rows on an arc, its state a row of it
  pqp_agents_check_device           the groups * 3 plans against four discs per scene on the same 71 steps, m_of = NULL, no clearance
  pqp_footprint_check_device        the same plans, stride 8, against an open distance layer
  pqp_fallback_pick_device          no group has a winner: every group copies a level's rows
Beside them, from the same run and the parent's kernels: pqp_sample_plan_device at the same 71 samples for one path per group, and
pqp_stitch_trajectory_device on the same groups and rows; and the algorithmic bytes of the two new calls - the rows read and written
once, the per-plan and per-group records - with what fraction of 8 TB/s they are at the median time.
Usage: python tools/bench_fallback.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402

SHAPES = [(1024, 8, 10), (8192, 8, 10)]          # groups, layers, sub-steps: 71 rows
HBM_BYTES_PER_S = 8e12
SCENES, AGENTS = 16, 4


def make_trajectories(rng, G, M, dt):
    """[G][M][8] = x, y, heading, k, s, v, a, t: a car on an arc under constant acceleration, rows dt apart, inside +-100 m"""
    v0, a, k = rng.uniform(3.0, 8.0, (G, 1)), rng.choice([-0.2, 0.0, 0.3], (G, 1)), rng.choice([-0.03, -0.01, 0.01, 0.04], (G, 1))
    x0, y0, h0 = rng.uniform(-30.0, 30.0, (G, 1)), rng.uniform(-30.0, 30.0, (G, 1)), rng.uniform(-np.pi, np.pi, (G, 1))
    tau = np.arange(M)[None, :] * dt
    s = v0 * tau + 0.5 * a * tau * tau
    th = k * s
    lx, ly = np.sin(th) / k, (1.0 - np.cos(th)) / k
    traj = np.zeros((G, M, capi.TRAJ_STRIDE))
    traj[..., 0], traj[..., 1] = x0 + lx * np.cos(h0) - ly * np.sin(h0), y0 + lx * np.sin(h0) + ly * np.cos(h0)
    traj[..., 2], traj[..., 3], traj[..., 4], traj[..., 5], traj[..., 6], traj[..., 7] = h0 + th, k, s, v0 + a * tau, a, tau
    return traj


def case(h, rng, G, m, r, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)

    def ok(rc):
        assert rc == 0, h.lib.pqp_last_error()

    dt = 1.0
    M = (m - 1) * r + 1
    prm = capi.fallback_default_params(h.lib)
    L, levels = prm.level_rows()
    P = G * L
    prev = make_trajectories(rng, G, M, dt / r)
    state = prev[:, 10].copy()
    d_prev, d_prev_m, d_state, d_sflags = t(prev), t(np.full(G, M, np.int32)), t(state), t(np.full(G, capi.STITCH_STITCHED, np.int32))
    d_rows, d_stop, d_stop_row, d_rflags = f64(G, L, M, 8), f64(G, L, 2), i32(G, L), i32(G, L)
    # four discs per scene, three of them well away and one near the origin, on the same steps
    agents = np.zeros((SCENES, AGENTS, M, capi.AGENT_STRIDE))
    agents[..., 0], agents[..., 1] = rng.uniform(-60.0, 60.0, (SCENES, AGENTS, 1)), rng.uniform(-60.0, 60.0, (SCENES, AGENTS, 1))
    agents[..., 5] = 0.5
    d_agents, d_frames = t(agents), f64(SCENES, AGENTS, M, capi.AGENT_FRAME_STRIDE)
    d_scene_of = t(np.repeat(np.arange(G, dtype=np.int32) % SCENES, L))
    d_hit, d_who = i32(P), i32(P)
    car = capi.car_default_geometry(h.lib)
    geom = capi.PqpGridGeometry(800, 800, 0.25, 200.0, 200.0, 0.0, 0.0)
    d_dist = torch.full((1, 800, 800), 10.0, dtype=torch.float32, device=dev)
    d_free, d_col = torch.empty((P, M), dtype=torch.uint8, device=dev), i32(P)
    d_final, d_final_m, d_level, d_flags = f64(G, M, 8), i32(G), i32(G), i32(G)
    calls = dict(
        rows=lambda: h.lib.pqp_fallback_rows_device(h._h, prm.array(), L, levels, dt, r, m, G, M, 8, d_prev, d_prev_m, d_state, d_sflags, d_rows, d_stop,
                                                    d_stop_row, d_rflags),
        agents_check=lambda: h.lib.pqp_agents_check_device(h._h, 0.0, C.byref(car), P, M, 8, d_rows, None, SCENES, AGENTS, d_agents, None, d_scene_of,
                                                           d_frames, d_hit, d_who, None),
        footprint_check=lambda: h.lib.pqp_footprint_check_device(h._h, P, M, 8, d_rows, None, d_dist, None, C.byref(geom), C.byref(car),
                                                                 capi.FOOTPRINT_CIRCLES, d_free, d_col, None),
        pick=lambda: h.lib.pqp_fallback_pick_device(h._h, G, L, M, None, None, None, d_rows, d_rflags, d_hit, d_col, d_final, d_final_m, d_level, d_flags))
    # ---- the parent's kernels on the same groups: the fine sampler at the same 71 samples, the stitch on the same rows -----------------------------
    n = 96
    paths = np.zeros((G, n, 7))
    paths[..., 0] = np.arange(n)[None, :] * 1.0 + rng.uniform(-30.0, 30.0, (G, 1))
    profile = np.zeros((G, n, capi.SPEED_STRIDE))
    profile[..., 0], profile[..., 1], profile[..., 3] = np.arange(n)[None, :], 8.0, np.arange(n)[None, :] / 8.0
    plan = np.zeros((G, m, 8))
    plan[..., 4], plan[..., 5], plan[..., 7] = 8.0 * np.arange(m)[None, :], 8.0, np.arange(m)[None, :]
    d_paths, d_profile, d_plan = t(paths), t(profile), t(plan)
    d_fine, d_m_of, d_defect, d_excess, d_pflags = f64(G, M, 8), i32(G), f64(G), f64(G), i32(G)
    calls["sample_plan"] = lambda: h.lib.pqp_sample_plan_device(h._h, dt, r, 0, G, n, 7, d_paths, None, None, d_profile, m, d_plan, None, None, d_fine,
                                                                d_m_of, d_defect, d_excess, d_pflags)
    sp = capi.stitch_default_params(h.lib)
    at = prev[:, 10] + 0.4 * (prev[:, 11] - prev[:, 10])
    meas = np.stack([at[:, 0], at[:, 1], prev[:, 10, 2], at[:, 5], prev[:, 10, 6], prev[:, 10, 3] * at[:, 5]], axis=1)
    d_meas, d_t_now = t(meas), t(at[:, 7])
    d_st, d_fl, d_dv, d_ix, d_px, d_pn = f64(G, 8), i32(G), f64(G, 3), i32(G, 3), f64(G, M, 8), i32(G)
    calls["stitch_trajectory"] = lambda: h.lib.pqp_stitch_trajectory_device(h._h, sp.array(), int(sp.keep), M, G, M, 8, d_prev, d_prev_m, d_meas, d_t_now, G,
                                                                            None, d_st, d_fl, d_dv, d_ix, d_px, d_pn, None, None, None)
    torch.cuda.synchronize(dev)
    us = lambda a: dict(us=float(np.median(a)) * 1e3, us_min=float(a.min()) * 1e3, us_max=float(a.max()) * 1e3)
    res = dict(groups=G, rows=M, levels=L)
    for name in ("rows", "agents_check", "footprint_check", "pick", "sample_plan", "stitch_trajectory"):
        for _ in range(warmup + steps):
            ok(calls[name]())
        h.sync()
        res[name] = us(h.kernel_ms_history(steps).astype(np.float64))
    stage = ("rows", "agents_check", "footprint_check", "pick")
    for _ in range(warmup + steps):
        for name in stage:
            ok(calls[name]())
    h.sync()
    res["together"] = us(h.kernel_ms_history(4 * steps).astype(np.float64).reshape(steps, 4).sum(axis=1))
    row = capi.TRAJ_STRIDE * 8
    res["rows_bytes"] = G * M * row + G * (row + 4 + 4) + P * M * row + P * (16 + 4 + 4)
    res["pick_bytes"] = P * (4 + 4 + 4) + 2 * G * M * row + G * 12
    for name in ("rows", "pick"):
        res[name]["fraction_of_8_tb_per_s"] = res[name + "_bytes"] / (res[name]["us"] * 1e-6) / HBM_BYTES_PER_S
    flags, level = d_rflags.cpu().numpy(), d_level.cpu().numpy()
    res["plans_flagged"] = {k: int(((flags & getattr(capi, "FALLBACK_" + k)) != 0).sum()) for k in ("ARC", "PATH_SHORT", "HORIZON", "BAD")}
    res["levels_taken"] = np.bincount(level + 1, minlength=L + 1).tolist()          # index 0: none
    line = ", ".join(f"{name} {res[name]['us']:.1f} us (min {res[name]['us_min']:.1f}, max {res[name]['us_max']:.1f})" for name in stage + ("together",))
    print(f"{G:6d} groups x {M} rows x {L} levels: {line}; rows {res['rows_bytes']} B = {100.0 * res['rows']['fraction_of_8_tb_per_s']:.2f} % of 8 TB/s, "
          f"pick {res['pick_bytes']} B = {100.0 * res['pick']['fraction_of_8_tb_per_s']:.2f} %; pqp_sample_plan {res['sample_plan']['us']:.1f} us (min "
          f"{res['sample_plan']['us_min']:.1f}, max {res['sample_plan']['us_max']:.1f}), pqp_stitch_trajectory {res['stitch_trajectory']['us']:.1f} us (min "
          f"{res['stitch_trajectory']['us_min']:.1f}, max {res['stitch_trajectory']['us_max']:.1f}); plans flagged {res['plans_flagged']}, levels taken "
          f"(none, 0, 1, 2) {res['levels_taken']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fallback: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="fallback_stage_us_1024x71x3", value=out[0]["together"]["us"], stage_us_8192x71x3=out[1]["together"]["us"],
                          rows_us_1024=out[0]["rows"]["us"], rows_us_8192=out[1]["rows"]["us"])))


if __name__ == "__main__":
    main()
