"""pqp_select_plans on one GPU: device time per call (the handle's HIP events around its two launches, after warm-up, median of the timed
calls with min and max) at 1024 paths x 71 fine samples in 128 groups of 8 and 8192 x 71 in 1024 groups: bench_plan_sample's batches
(1024 paths x 80 waypoints x 8 layers x 8 agents and 8192 x 120 x 8 x 16, r = 10) through pqp_speed_search, pqp_speed_refine,
pqp_sample_plan and pqp_agents_check with clearance on the fine rows, and pqp_select_paths for the paths' terms.  Beside each time, from
the same run on the same batch:
  pqp_sample_plan, which wrote the rows this call reads, and pqp_select_paths in the same groups, the nearest existing kernels - one
  wavefront per candidate, one per group - and the ratios to them;
  the algorithmic bytes of the call - the rows below every count in full (the five columns read share their 64 bytes with the three that
  are not), their clearances, the per-candidate scalars, the records written and read again, the two gathers in and out - and what
  fraction of 8 TB/s they are at the median time.
Usage: python tools/bench_select_plans.py [--steps K] [--warmup W] [--json PATH]"""
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
GROUP = 8
HBM_BYTES_PER_S = 8e12


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
    # ---- the plans on the fine steps: what the call reads, and the first neighbour's time ------------------------------------------------------
    M = (m - 1) * R + 1
    d_fine, d_m_of, d_defect, d_excess, d_flags = f64(B, M, capi.TRAJ_STRIDE), i32(B), f64(B), f64(B), i32(B)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_sample_plan_device(h._h, float(grid.dt), R, 0, B, n, 7, d_paths, None, None, d_prof, m, d_traj, d_reached, d_rflags, d_fine, d_m_of,
                                        d_defect, d_excess, d_flags))
    h.sync()
    plan = h.kernel_ms_history(steps).astype(np.float64)
    d_fagents, d_fframes = t(agents[:, :, np.arange(M) // R]), f64(1, A, M, capi.AGENT_FRAME_STRIDE)
    d_first, d_who, d_clear = i32(B), i32(B), f64(B, M)
    ok(h.lib.pqp_agents_check_device(h._h, float(grid.margin), C.byref(car), B, M, capi.TRAJ_STRIDE, d_fine, d_m_of, 1, A, d_fagents, None, None,
                                     d_fframes, d_first, d_who, d_clear))
    # ---- the second neighbour: the paths' terms and each group's best path ------------------------------------------------------------------------
    groups = B // GROUP
    d_start = t(np.arange(0, B + 1, GROUP, dtype=np.int32))
    sel = capi.select_default_params(h.lib)
    d_pterms, d_pbest, d_pbest_paths, d_pbest_n = f64(B, capi.SCORE_STRIDE), i32(groups), f64(groups, n, 7), i32(groups)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_select_paths_device(h._h, C.byref(sel), B, n, 7, d_paths, None, None, None, None, None, groups, d_start, d_pterms, d_pbest,
                                         d_pbest_paths, d_pbest_n))
    h.sync()
    select = h.kernel_ms_history(steps).astype(np.float64)
    # ---- the finished trajectories and each group's best ----------------------------------------------------------------------------------------
    rk = capi.rank_default_params(h.lib)
    d_terms, d_best, d_best_traj, d_best_m = f64(B, capi.PLAN_SCORE_STRIDE), i32(groups), f64(groups, M, capi.TRAJ_STRIDE), i32(groups)
    d_best_paths, d_best_n = f64(groups, n, 7), i32(groups)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_select_plans_device(h._h, rk.array(), int(rk.require_free), B, M, capi.TRAJ_STRIDE, d_fine, d_m_of, d_pterms, d_sf, d_first, d_clear,
                                         n, 7, d_paths, None, groups, d_start, d_terms, d_best, d_best_traj, d_best_m, d_best_paths, d_best_n))
    h.sync()
    rank = h.kernel_ms_history(steps).astype(np.float64)
    m_of, best, terms = d_m_of.cpu().numpy(), d_best.cpu().numpy(), d_terms.cpu().numpy()
    rows = int(m_of.sum())
    nbytes = rows * (capi.TRAJ_STRIDE * 8 + 8) + B * (capi.SCORE_STRIDE * 8 + 12) + 2 * B * capi.PLAN_SCORE_STRIDE * 8 + \
        2 * groups * (M * capi.TRAJ_STRIDE * 8 + n * 7 * 8) + 8 * groups
    med = float(np.median(rank))
    us = lambda a: dict(us=float(np.median(a)) * 1e3, us_min=float(a.min()) * 1e3, us_max=float(a.max()) * 1e3)
    r = dict(paths=B, waypoints=n, samples=M, groups=groups, **us(rank), paths_per_s=B / (med * 1e-3), algorithmic_bytes=nbytes,
             fraction_of_8_tb_per_s=nbytes / (med * 1e-3) / HBM_BYTES_PER_S, sample_plan=us(plan), ratio_to_sample_plan=med / float(np.median(plan)),
             select_paths=us(select), ratio_to_select_paths=med / float(np.median(select)), rows_on_the_plans=rows,
             eligible=int((terms[:, 9] == 1.0).sum()), groups_with_a_winner=int((best >= 0).sum()),
             winner_differs_from_select_paths=int((best != d_pbest.cpu().numpy()).sum()))
    print(f"{B:6d} paths x {M} samples in {groups} groups of {GROUP}: {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f}); "
          f"{nbytes} algorithmic bytes, {100.0 * r['fraction_of_8_tb_per_s']:.2f} % of 8 TB/s; pqp_sample_plan {r['sample_plan']['us']:.1f} us (min "
          f"{r['sample_plan']['us_min']:.1f}, max {r['sample_plan']['us_max']:.1f}): x {r['ratio_to_sample_plan']:.2f}; pqp_select_paths "
          f"{r['select_paths']['us']:.1f} us (min {r['select_paths']['us_min']:.1f}, max {r['select_paths']['us_max']:.1f}): x "
          f"{r['ratio_to_select_paths']:.2f}; {r['eligible']} eligible, {r['groups_with_a_winner']} groups with a winner, "
          f"{r['winner_differs_from_select_paths']} where pqp_select_paths picks another", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_select_plans: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="select_plans_paths_per_s_1024x71_groups_of_8", value=out[0]["paths_per_s"], paths_per_s_8192x71=out[1]["paths_per_s"],
                          ratio_to_sample_plan_1024=out[0]["ratio_to_sample_plan"], ratio_to_sample_plan_8192=out[1]["ratio_to_sample_plan"],
                          ratio_to_select_paths_1024=out[0]["ratio_to_select_paths"], ratio_to_select_paths_8192=out[1]["ratio_to_select_paths"])))


if __name__ == "__main__":
    main()
