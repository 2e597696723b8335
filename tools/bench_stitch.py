"""pqp_stitch_trajectory on one GPU: device time per call (the handle's HIP events around its one launch, after warm-up, median of the
timed calls with min and max) at 1024 groups x 71 rows x 8 candidates and 8192 x 71 x 8, keep = 20, prefix_max = 71, about a tenth of the
groups replanning: every group's eight candidates are trajectories of 71 rows on arcs, pqp_select_plans picks each group's best into
best_traj, and the stitch reads best_traj / best_m where they lie, with a measurement a few centimetres beside each winner (a tenth of
them 1.5 m beside it).  Beside each time, from the same run on the same rows:
  pqp_select_plans, the stage that wrote the rows this call reads - two launches, one wavefront per candidate, then one per group - and
  the ratio to it;
  the algorithmic bytes of the call - every row below the count once (the three columns the scan reads share their 64 bytes with the five
  it does not), the measurements, the per-group records, the prefix in full (it is written out to prefix_max, zeros behind the piece) and
  the piece read again, the candidates' five doubles - and what fraction of 8 TB/s they are at the median time.
Usage: python tools/bench_stitch.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402

SHAPES = [(1024, 71, 8), (8192, 71, 8)]          # groups, rows, candidates per group
HBM_BYTES_PER_S = 8e12
DT = 0.1


def make_trajectories(rng, B, m):
    """[B][m][8] = x, y, heading, k, s, v, a, t: a car on an arc under constant acceleration, rows DT apart"""
    v0, a, k = rng.uniform(3.0, 12.0, (B, 1)), rng.choice([-0.3, 0.0, 0.6], (B, 1)), rng.choice([-0.03, -0.01, 0.01, 0.04], (B, 1))
    x0, y0, h0 = rng.uniform(-300.0, 300.0, (B, 1)), rng.uniform(-300.0, 300.0, (B, 1)), rng.uniform(-np.pi, np.pi, (B, 1))
    tau = np.arange(m)[None, :] * DT
    s = v0 * tau + 0.5 * a * tau * tau
    th = k * s
    lx, ly = np.sin(th) / k, (1.0 - np.cos(th)) / k
    traj = np.zeros((B, m, capi.TRAJ_STRIDE))
    traj[..., 0], traj[..., 1] = x0 + lx * np.cos(h0) - ly * np.sin(h0), y0 + lx * np.sin(h0) + ly * np.cos(h0)
    traj[..., 2], traj[..., 3], traj[..., 4], traj[..., 5], traj[..., 6], traj[..., 7] = h0 + th, k, s, v0 + a * tau, a, tau
    return traj


def case(h, rng, G, m, per_group, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)

    def ok(rc):
        assert rc == 0, h.lib.pqp_last_error()

    B = G * per_group
    d_traj = t(make_trajectories(rng, B, m))
    d_start_of = t(np.arange(0, B + 1, per_group, dtype=np.int32))
    # ---- the yardstick: the stage that leaves the rows ----------------------------------------------------------------------------------------------
    rk = capi.rank_default_params(h.lib)
    d_terms, d_best, d_best_traj, d_best_m = f64(B, capi.PLAN_SCORE_STRIDE), i32(G), f64(G, m, capi.TRAJ_STRIDE), i32(G)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_select_plans_device(h._h, rk.array(), int(rk.require_free), B, m, capi.TRAJ_STRIDE, d_traj, None, None, None, None, None, 0, 0, None,
                                         None, G, d_start_of, d_terms, d_best, d_best_traj, d_best_m, None, None))
    h.sync()
    rank = h.kernel_ms_history(steps).astype(np.float64)
    # ---- the measurements: 40 % of the way from row 10 to row 11 of each winner, a few centimetres beside it, a tenth of them 1.5 m -------------------
    best = d_best_traj.cpu().numpy()
    r0, r1 = best[:, 10], best[:, 11]
    at = r0 + 0.4 * (r1 - r0)
    lat = rng.uniform(-0.1, 0.1, G) + np.where(rng.random(G) < 0.1, 1.5, 0.0)
    meas = np.stack([at[:, 0] - lat * np.sin(r0[:, 2]), at[:, 1] + lat * np.cos(r0[:, 2]), r0[:, 2] + rng.uniform(-0.05, 0.05, G), at[:, 5], r0[:, 6],
                     r0[:, 3] * at[:, 5]], axis=1)
    d_meas, d_t_now = t(meas), t(at[:, 7])
    # ---- the stitch -----------------------------------------------------------------------------------------------------------------------------------
    prm = capi.stitch_default_params(h.lib)
    d_state, d_flags, d_dev, d_idx = f64(G, capi.TRAJ_STRIDE), i32(G), f64(G, 3), i32(G, 3)
    d_prefix, d_prefix_n, d_start, d_start_k, d_v_start = f64(G, m, capi.TRAJ_STRIDE), i32(G), f64(B, 3), f64(B), f64(B)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        ok(h.lib.pqp_stitch_trajectory_device(h._h, prm.array(), int(prm.keep), m, G, m, capi.TRAJ_STRIDE, d_best_traj, d_best_m, d_meas, d_t_now, B,
                                              d_start_of, d_state, d_flags, d_dev, d_idx, d_prefix, d_prefix_n, d_start, d_start_k, d_v_start))
    h.sync()
    stitch = h.kernel_ms_history(steps).astype(np.float64)
    flags, best_m, prefix_n = d_flags.cpu().numpy(), d_best_m.cpu().numpy(), d_prefix_n.cpu().numpy()
    row = capi.TRAJ_STRIDE * 8
    nbytes = int(best_m.sum()) * row + G * (6 * 8 + 8 + 4) + 4 * (G + 1) + G * (row + 4 + 24 + 12 + 4) + G * m * row + int(prefix_n.sum()) * row + B * 5 * 8
    med = float(np.median(stitch))
    us = lambda a: dict(us=float(np.median(a)) * 1e3, us_min=float(a.min()) * 1e3, us_max=float(a.max()) * 1e3)
    r = dict(groups=G, rows=m, candidates=B, **us(stitch), groups_per_s=G / (med * 1e-3), algorithmic_bytes=nbytes,
             fraction_of_8_tb_per_s=nbytes / (med * 1e-3) / HBM_BYTES_PER_S, select_plans=us(rank), ratio_to_select_plans=med / float(np.median(rank)),
             stitched=int(((flags & capi.STITCH_STITCHED) != 0).sum()), replanned=int(((flags & capi.STITCH_REPLAN) != 0).sum()),
             bad=int(((flags & capi.STITCH_BAD) != 0).sum()), mean_prefix_rows=float(prefix_n.mean()))
    print(f"{G:6d} groups x {m} rows x {per_group} candidates: {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f}); {nbytes} algorithmic "
          f"bytes, {100.0 * r['fraction_of_8_tb_per_s']:.2f} % of 8 TB/s; pqp_select_plans on the same rows {r['select_plans']['us']:.1f} us (min "
          f"{r['select_plans']['us_min']:.1f}, max {r['select_plans']['us_max']:.1f}): x {r['ratio_to_select_plans']:.2f}; {r['stitched']} stitched, "
          f"{r['replanned']} replanned, {r['bad']} bad, {r['mean_prefix_rows']:.1f} prefix rows a group", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stitch: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, *shape, args.steps, args.warmup) for shape in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="stitch_groups_per_s_1024x71x8", value=out[0]["groups_per_s"], groups_per_s_8192x71x8=out[1]["groups_per_s"],
                          ratio_to_select_plans_1024=out[0]["ratio_to_select_plans"], ratio_to_select_plans_8192=out[1]["ratio_to_select_plans"])))


if __name__ == "__main__":
    main()
