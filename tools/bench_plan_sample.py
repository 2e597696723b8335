"""pqp_sample_plan on one GPU: device time per call (the handle's HIP events around its one launch, after warm-up, median of the timed
calls with min and max) at 1024 paths x 80 waypoints x 8 layers x 8 agents and 8192 x 120 x 8 x 16 (bench_speed_search's shapes), at
r = 10 sub-steps per layer, on what pqp_speed_refine wrote for the batch behind pqp_speed_search (bench_speed_refine's inputs): its traj
and flags and the search's reached.  Beside each time, from the same run:
  pqp_sample_trajectory on the same batch at the same sample count, (m - 1) r + 1, and the ratio to it: the nearest existing kernel - one
  wavefront per path, one sample per lane; it walks the t column where this one walks s;
  pqp_agents_check on the fine rows, against the search's agents held over each layer's sub-steps;
  the share of paths sampled under constant acceleration (refined) and linearly (kept), the samples on the plans, defect and excess.
Usage: python tools/bench_plan_sample.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402
from bench_agents_check import make_agents  # noqa: E402
from bench_speed_profile import make_paths  # noqa: E402
from bench_speed_search import SHAPES  # noqa: E402

R = 10


def case(h, rng, B, n, m, A, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    C = capi.C
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)

    def ok(rc):
        assert rc == 0, h.lib.pqp_last_error()

    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof, d_sflags = f64(B, n, capi.SPEED_STRIDE), i32(B)
    sp, car = capi.speed_default_params(h.lib), capi.car_default_geometry(h.lib)
    torch.cuda.synchronize(dev)
    ok(h.lib.pqp_speed_profile_device(h._h, C.byref(sp), B, n, 7, d_paths, None, None, None, d_vs, None, d_prof, d_sflags))
    grid = capi.search_default_params(h.lib, margin=0.3)
    S, Q1 = grid.stations, grid.q_max + 1
    agents = make_agents(rng, A, m, grid.dt)
    d_agents, d_frames = t(agents), f64(1, A, m, capi.AGENT_FRAME_STRIDE)
    d_blocked, d_parents = i32(B, m, (S + 31) // 32), torch.empty((B, m, S, Q1), dtype=torch.uint8, device=dev)
    d_steps, d_plan, d_cost, d_reached, d_sf = i32(B, m, 2), f64(B, m, capi.TRAJ_STRIDE), f64(B), i32(B), i32(B)
    ok(h.lib.pqp_speed_search_device(h._h, C.byref(grid), C.byref(car), B, n, 7, d_paths, None, None, d_prof, d_vs, m, 1, A, d_agents, None, None,
                                     d_frames, d_blocked, d_parents, d_steps, d_plan, d_cost, d_reached, d_sf))
    prm = capi.refine_default_params(h.lib)
    d_traj, d_bounds, d_rcost, d_rexcess, d_status, d_iters, d_rflags = f64(B, m, capi.TRAJ_STRIDE), f64(B, m, 3), f64(B), f64(B), i32(B), i32(B), i32(B)
    ok(h.lib.pqp_speed_refine_device(h._h, C.byref(grid), prm.array(), int(prm.window), B, n, 7, d_paths, None, None, d_prof, d_vs, m, d_blocked,
                                     d_steps, d_reached, d_plan, d_traj, d_bounds, d_rcost, d_rexcess, d_status, d_iters, d_rflags))
    h.sync()
    # ---- the plans on the fine steps ---------------------------------------------------------------------------------------------------------
    M = (m - 1) * R + 1
    d_fine, d_m_of, d_defect, d_excess, d_flags = f64(B, M, capi.TRAJ_STRIDE), i32(B), f64(B), f64(B), i32(B)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_sample_plan_device(h._h, float(grid.dt), R, 0, B, n, 7, d_paths, None, None, d_prof, m, d_traj, d_reached, d_rflags, d_fine, d_m_of,
                                        d_defect, d_excess, d_flags))
    h.sync()
    plan = h.kernel_ms_history(steps).astype(np.float64)
    # ---- the nearest existing kernel: the speed profile on the same number of samples ----------------------------------------------------------
    sa = capi.sample_default_params(h.lib, dt=float(grid.dt) / R)
    d_samples, d_sn, d_sfl = f64(B, M, capi.TRAJ_STRIDE), i32(B), i32(B)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_sample_trajectory_device(h._h, C.byref(sa), B, n, 7, d_paths, None, None, d_prof, None, M, d_samples, d_sn, d_sfl))
    h.sync()
    sampler = h.kernel_ms_history(steps).astype(np.float64)
    # ---- the fine rows against the agents --------------------------------------------------------------------------------------------------------
    d_fagents, d_fframes = t(agents[:, :, np.arange(M) // R]), f64(1, A, M, capi.AGENT_FRAME_STRIDE)
    d_first, d_who = i32(B), i32(B)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_agents_check_device(h._h, float(grid.margin), C.byref(car), B, M, capi.TRAJ_STRIDE, d_fine, d_m_of, 1, A, d_fagents, None, None,
                                         d_fframes, d_first, d_who, None))
    h.sync()
    check = h.kernel_ms_history(steps).astype(np.float64)
    rflags, flags, m_of = d_rflags.cpu().numpy(), d_flags.cpu().numpy(), d_m_of.cpu().numpy()
    defect, excess, first = d_defect.cpu().numpy(), d_excess.cpu().numpy(), d_first.cpu().numpy()
    refined = int((rflags == capi.REFINE_REFINED).sum())
    med = float(np.median(plan))
    us = lambda a: dict(us=float(np.median(a)) * 1e3, us_min=float(a.min()) * 1e3, us_max=float(a.max()) * 1e3)
    r = dict(paths=B, waypoints=n, layers=m, agents=A, sub_steps=R, samples=M, **us(plan), paths_per_s=B / (med * 1e-3),
             samples_per_s=float(m_of.sum()) / (med * 1e-3), bytes_written=B * M * capi.TRAJ_STRIDE * 8,
             sample_trajectory={**us(sampler), "samples_on_path": int(d_sn.cpu().numpy().sum())}, ratio_to_sample_trajectory=med / float(np.median(sampler)),
             agents_check=us(check), refined=refined, linear=B - refined, samples_on_plan=int(m_of.sum()), empty=int((flags == capi.PLAN_EMPTY).sum()),
             backward=int(((flags & capi.PLAN_BACKWARD) != 0).sum()), defect_max=float(np.nanmax(defect)) if np.isfinite(defect).any() else None,
             excess_max=float(np.nanmax(excess)) if np.isfinite(excess).any() else None, hit_on_fine_rows=int((first < m_of).sum()))
    print(f"{B:6d} paths x {n} waypoints x {m} layers x r = {R} ({M} samples): {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f}); "
          f"pqp_sample_trajectory, same sample count {r['sample_trajectory']['us']:.1f} us (min {r['sample_trajectory']['us_min']:.1f}, max "
          f"{r['sample_trajectory']['us_max']:.1f}): x {r['ratio_to_sample_trajectory']:.2f}; pqp_agents_check on the fine rows, {A} agents "
          f"{r['agents_check']['us']:.1f} us (min {r['agents_check']['us_min']:.1f}, max {r['agents_check']['us_max']:.1f}); refined {refined}, linear "
          f"{B - refined}, {r['samples_on_plan']} samples on the plans, {r['empty']} empty, {r['backward']} backward; largest defect {r['defect_max']}, "
          f"largest excess {r['excess_max']}; hit on the fine rows: {r['hit_on_fine_rows']} paths", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plan_sample: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="plan_sample_paths_per_s_1024x80x8_r10", value=out[0]["paths_per_s"], paths_per_s_8192x120x8_r10=out[1]["paths_per_s"],
                          ratio_to_sample_trajectory_1024=out[0]["ratio_to_sample_trajectory"],
                          ratio_to_sample_trajectory_8192=out[1]["ratio_to_sample_trajectory"])))


if __name__ == "__main__":
    main()
