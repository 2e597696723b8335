"""pqp_speed_search on one GPU: device time per call (the handle's HIP events around its three launches, after warm-up, median of the
timed calls with min and max) at 1024 paths x 80 waypoints x 8 layers x 8 agents and 8192 x 120 x 8 x 16, at the default parameters (128
stations of 0.5 m, steps up to 20 cells, 1 s between layers), on the profile pqp_speed_profile wrote for the batch.  The agents of the one
scene drive straight lines across the disc the paths fan out over (bench_agents_check's).  In the same run, what the search is priced
against: pqp_sample_trajectory + pqp_agents_check (clearance NULL) on the same batch, m samples at the layers' times - the pair that
tells a caller a trajectory is hit, where the search tells it what to drive instead.  Beside each time:
  the same call with q_max = 0, in which the search kernel has one state per station and next to nothing to do: the frames, the occupancy
  kernel and that remainder.  The difference to the full call is taken as the search kernel's time (an estimate by difference, not a
  kernel trace: it leaves the search kernel's fixed part on the other side) and divided by the m - 1 layers it relaxes;
  the occupancy's fp64 operations of the definition, 22 per circle test as in bench_agents_check (B S m A 6 tests, of which the broad
  phase skips most: the rate says how fast the table is decided, not how many operations ran), over the q_max = 0 time.
Usage: python tools/bench_speed_search.py [--steps K] [--warmup W] [--json PATH]"""
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
from bench_agents_check import OPS_PER_CIRCLE_TEST, make_agents  # noqa: E402
from bench_speed_profile import make_paths  # noqa: E402

SHAPES = ((1024, 80, 8, 8), (8192, 120, 8, 16))              # paths, waypoints, layers, agents


def case(h, rng, B, n, m, A, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    C = capi.C
    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof = torch.empty((B, n, capi.SPEED_STRIDE), dtype=torch.float64, device=dev)
    d_sflags = torch.empty(B, dtype=torch.int32, device=dev)
    sp, car = capi.speed_default_params(h.lib), capi.car_default_geometry(h.lib)
    torch.cuda.synchronize(dev)
    rc = h.lib.pqp_speed_profile_device(h._h, C.byref(sp), B, n, 7, d_paths, None, None, None, d_vs, None, d_prof, d_sflags)
    assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    prm = capi.search_default_params(h.lib, margin=0.3)
    S, Q1 = prm.stations, prm.q_max + 1
    d_agents = t(make_agents(rng, A, m, prm.dt))
    d_frames = torch.empty((1, A, m, capi.AGENT_FRAME_STRIDE), dtype=torch.float64, device=dev)
    # the pair the search is priced against
    sa = capi.sample_default_params(h.lib, dt=prm.dt, hold_last=1)
    d_traj = torch.empty((B, m, capi.TRAJ_STRIDE), dtype=torch.float64, device=dev)
    d_m_of = torch.empty(B, dtype=torch.int32, device=dev)
    d_flags = torch.empty(B, dtype=torch.int32, device=dev)
    d_first = torch.empty(B, dtype=torch.int32, device=dev)
    d_who = torch.empty(B, dtype=torch.int32, device=dev)
    pair = []
    for _ in range(warmup + steps):
        rc = h.lib.pqp_sample_trajectory_device(h._h, C.byref(sa), B, n, 7, d_paths, None, None, d_prof, None, m, d_traj, d_m_of, d_flags)
        assert rc == 0, h.lib.pqp_last_error()
        rc = h.lib.pqp_agents_check_device(h._h, prm.margin, C.byref(car), B, m, capi.TRAJ_STRIDE, d_traj, None, 1, A, d_agents, None, None, d_frames,
                                           d_first, d_who, None)
        assert rc == 0, h.lib.pqp_last_error()
        h.sync()
        pair.append(float(h.kernel_ms_history(2).sum()))
    pair = np.array(pair[warmup:])
    hit = int((d_first.cpu().numpy() < m).sum())
    # the search
    d_blocked = torch.empty((B, m, (S + 31) // 32), dtype=torch.int32, device=dev)
    d_parents = torch.empty((B, m, S, Q1), dtype=torch.uint8, device=dev)
    d_steps = torch.empty((B, m, 2), dtype=torch.int32, device=dev)
    d_plan = torch.empty((B, m, capi.TRAJ_STRIDE), dtype=torch.float64, device=dev)
    d_cost = torch.empty(B, dtype=torch.float64, device=dev)
    d_reached = torch.empty(B, dtype=torch.int32, device=dev)
    d_sf = torch.empty(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    times = {}
    for name, p in (("full", prm), ("q_max_0", capi.search_default_params(h.lib, margin=0.3, q_max=0))):
        for _ in range(warmup + steps):
            rc = h.lib.pqp_speed_search_device(h._h, C.byref(p), C.byref(car), B, n, 7, d_paths, None, None, d_prof, d_vs, m, 1, A, d_agents, None, None,
                                               d_frames, d_blocked, d_parents, d_steps, d_plan, d_cost, d_reached, d_sf)
            assert rc == 0, h.lib.pqp_last_error()
        h.sync()
        times[name] = h.kernel_ms_history(steps).astype(np.float64)
        if name == "full":
            reached, flags = d_reached.cpu().numpy(), d_sf.cpu().numpy()
    med, occ = float(np.median(times["full"])), float(np.median(times["q_max_0"]))
    ops = B * S * m * A * 6 * OPS_PER_CIRCLE_TEST
    r = dict(paths=B, waypoints=n, layers=m, agents=A, stations=S, q_max=prm.q_max, us=med * 1e3, us_min=float(times["full"].min()) * 1e3,
             us_max=float(times["full"].max()) * 1e3, paths_per_s=B / (med * 1e-3), frames_and_occupancy_us=occ * 1e3,
             occupancy_fp64_ops=ops, occupancy_fp64_ops_per_s=ops / (occ * 1e-3), search_kernel_us_by_difference=(med - occ) * 1e3,
             search_kernel_us_per_layer=(med - occ) * 1e3 / (m - 1), sample_plus_check_us=float(np.median(pair)) * 1e3,
             sample_plus_check_us_min=float(pair.min()) * 1e3, sample_plus_check_us_max=float(pair.max()) * 1e3,
             times_sample_plus_check=med / float(np.median(pair)), paths_hit_at_profile_speed=hit, plans_through=int((reached == m).sum()),
             plans_arrived=int(((flags & capi.SEARCH_ARRIVED) != 0).sum()), start_blocked=int((reached == 0).sum()))
    print(f"{B:6d} paths x {n} waypoints x {m} layers x {A:2d} agents: {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f}); "
          f"frames + occupancy (q_max = 0) {r['frames_and_occupancy_us']:.1f} us = {r['occupancy_fp64_ops_per_s'] / 1e12:.2f} T/s of {ops / 1e9:.2f} G "
          f"fp64 ops of the definition; search kernel by difference {r['search_kernel_us_by_difference']:.1f} us = {r['search_kernel_us_per_layer']:.1f} "
          f"us/layer; sample + check (clearance NULL) {r['sample_plus_check_us']:.1f} us (min {r['sample_plus_check_us_min']:.1f}, max "
          f"{r['sample_plus_check_us_max']:.1f}): x {r['times_sample_plus_check']:.2f}; {hit} paths hit at the profile's speed, "
          f"{r['plans_through']} plans through, {r['plans_arrived']} arrived, {r['start_blocked']} blocked at the start", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_speed_search: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="speed_search_paths_per_s_1024x80x8x8", value=out[0]["paths_per_s"], paths_per_s_8192x120x8x16=out[1]["paths_per_s"],
                          times_sample_plus_check_1024=out[0]["times_sample_plus_check"], times_sample_plus_check_8192=out[1]["times_sample_plus_check"])))


if __name__ == "__main__":
    main()
