"""pqp_speed_refine on one GPU: device time per call (the handle's HIP events around its four launches, after warm-up, median of the
timed calls with min and max) at 1024 paths x 80 waypoints x 8 layers x 8 agents and 8192 x 120 x 8 x 16, at the default parameters, on
what pqp_speed_search wrote for the batch (bench_speed_search's paths, profile and agents).  Beside each time, from the same run:
  pqp_speed_search on the same batch, and the ratio to it;
  pqp_post_smooth_device at the same batch and m on a handle in the reference's ADMM setting: the same solve kernel
  (banded_solve_kernel<3, 256, true>) on a QP of the same 3 m variables, there iterating ADMM, here polishing;
  the share of paths refined, kept (the search did not get through) and kept as infeasible.
Usage: python tools/bench_speed_refine.py [--steps K] [--warmup W] [--json PATH]"""
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


def case(h, rng, B, n, m, A, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    C = capi.C
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof, d_sflags = f64(B, n, capi.SPEED_STRIDE), i32(B)
    sp, car = capi.speed_default_params(h.lib), capi.car_default_geometry(h.lib)
    torch.cuda.synchronize(dev)
    rc = h.lib.pqp_speed_profile_device(h._h, C.byref(sp), B, n, 7, d_paths, None, None, None, d_vs, None, d_prof, d_sflags)
    assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    grid = capi.search_default_params(h.lib, margin=0.3)
    S, Q1 = grid.stations, grid.q_max + 1
    d_agents, d_frames = t(make_agents(rng, A, m, grid.dt)), f64(1, A, m, capi.AGENT_FRAME_STRIDE)
    d_blocked, d_parents = i32(B, m, (S + 31) // 32), torch.empty((B, m, S, Q1), dtype=torch.uint8, device=dev)
    d_steps, d_plan, d_cost, d_reached, d_sf = i32(B, m, 2), f64(B, m, capi.TRAJ_STRIDE), f64(B), i32(B), i32(B)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_speed_search_device(h._h, C.byref(grid), C.byref(car), B, n, 7, d_paths, None, None, d_prof, d_vs, m, 1, A, d_agents, None, None,
                                           d_frames, d_blocked, d_parents, d_steps, d_plan, d_cost, d_reached, d_sf)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    search = h.kernel_ms_history(steps).astype(np.float64)
    prm = capi.refine_default_params(h.lib)
    d_traj, d_bounds, d_rcost, d_excess, d_status, d_iters, d_flags = f64(B, m, capi.TRAJ_STRIDE), f64(B, m, 3), f64(B), f64(B), i32(B), i32(B), i32(B)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_speed_refine_device(h._h, C.byref(grid), prm.array(), int(prm.window), B, n, 7, d_paths, None, None, d_prof, d_vs, m, d_blocked,
                                           d_steps, d_reached, d_plan, d_traj, d_bounds, d_rcost, d_excess, d_status, d_iters, d_flags)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    refine = h.kernel_ms_history(steps).astype(np.float64)
    flags, excess, iters = d_flags.cpu().numpy(), d_excess.cpu().numpy(), d_iters.cpu().numpy()
    # the same solve kernel on the postSmooth QP of m layers, on the handle's own (ADMM) setting
    d_ls = t(np.tile(np.arange(m) * 1.5, (B, 1)) + rng.uniform(0.0, 0.2, (B, m)))
    half = rng.uniform(0.5, 1.5, (B, m))
    d_lb, d_ub, d_vl, d_l = t(-half), t(half), t(rng.uniform(-0.2, 0.2, B)), f64(B, m)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_post_smooth_device(h._h, B, m, d_ls, d_lb, d_ub, d_vl, d_l, d_status, d_iters, None)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    post = h.kernel_ms_history(steps).astype(np.float64)
    refined, infeasible = int((flags == capi.REFINE_REFINED).sum()), int(((flags & capi.REFINE_INFEASIBLE) != 0).sum())
    med = float(np.median(refine))
    r = dict(paths=B, waypoints=n, layers=m, agents=A, us=med * 1e3, us_min=float(refine.min()) * 1e3, us_max=float(refine.max()) * 1e3,
             paths_per_s=B / (med * 1e-3), search_us=float(np.median(search)) * 1e3, search_us_min=float(search.min()) * 1e3,
             search_us_max=float(search.max()) * 1e3, ratio_to_search=med / float(np.median(search)), post_smooth_solve_us=float(np.median(post)) * 1e3,
             post_smooth_solve_us_min=float(post.min()) * 1e3, post_smooth_solve_us_max=float(post.max()) * 1e3, refined=refined,
             kept_without_a_plan=B - refined - infeasible, kept_infeasible=infeasible, solved_without_admm=int((iters[flags == capi.REFINE_REFINED] == 0).sum()),
             excess_max=float(np.nanmax(excess)) if refined else None, excess_positive=int((excess > 1e-9).sum()))
    print(f"{B:6d} paths x {n} waypoints x {m} layers x {A:2d} agents: {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f}); "
          f"pqp_speed_search {r['search_us']:.1f} us (min {r['search_us_min']:.1f}, max {r['search_us_max']:.1f}): x {r['ratio_to_search']:.2f}; "
          f"pqp_post_smooth_device's solve, same kernel, ADMM {r['post_smooth_solve_us']:.1f} us (min {r['post_smooth_solve_us_min']:.1f}, max "
          f"{r['post_smooth_solve_us_max']:.1f}); refined {refined} ({100.0 * refined / B:.1f} %), kept without a plan {r['kept_without_a_plan']}, kept as "
          f"infeasible {infeasible} ({100.0 * infeasible / B:.1f} %); {r['solved_without_admm']} of the refined at iters = 0; excess above 1e-9 on "
          f"{r['excess_positive']} paths, largest {r['excess_max']}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_speed_refine: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="speed_refine_paths_per_s_1024x80x8x8", value=out[0]["paths_per_s"], paths_per_s_8192x120x8x16=out[1]["paths_per_s"],
                          ratio_to_search_1024=out[0]["ratio_to_search"], ratio_to_search_8192=out[1]["ratio_to_search"])))


if __name__ == "__main__":
    main()
