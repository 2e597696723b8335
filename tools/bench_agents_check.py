"""pqp_agents_check on one GPU: device time per call (the handle's HIP events around its two launches, after warm-up, median of the timed
calls with min and max) at 1024 paths x 50 samples x 8 agents, 8192 x 50 x 16 and 65 536 x 50 x 32, each with the clearance written and
without it (the broad phase and the early exit), on the traj pqp_sample_trajectory wrote for paths of 80 waypoints, read in place
(stride 8, hold_last, every sample checked).  The agents of the one scene drive straight lines across the disc of 40 m the paths fan
out over, 15 m and more from where they all start, so a few are near any given path and most are not.  Two yardsticks beside each
time: the model - the algorithmic bytes (64 m read per path at stride 8, A m 64 of frames per scene read by every path out of L2 and
counted once, A m 48 + A m 64 for the first launch, 8 per path written, 8 m more with the clearance) over 8 TB/s, and the definition's
fp64 operations (22 per circle test: B m A 6 of them, which the run without clearance mostly skips) - and pqp_sample_trajectory's own
time on the same batch in the same run.
Usage: python tools/bench_agents_check.py [--steps K] [--warmup W] [--json PATH]"""
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
from bench_speed_profile import make_paths  # noqa: E402

SHAPES = ((1024, 50, 8), (8192, 50, 16), (65536, 50, 32))
WAYPOINTS = 80
PEAK_BYTES_PER_S = 8e12
OPS_PER_CIRCLE_TEST = 22           # dx, dy; u and w (3 each); ex, ey; ox, oy; ox*ox + oy*oy (3); sqrt; fmax, fmin; +, -; - r_j; min


def make_agents(rng, A, m, dt):
    """[1][A][m][6]: boxes (cars), rounded boxes and discs (pedestrians) on straight lines at up to 8 m/s.  The paths all leave the origin,
    so an agent there would hit every one of them at sample 0: the agents start 15 to 40 m out and drive across, never inwards"""
    ag = np.zeros((1, A, m, capi.AGENT_STRIDE))
    r0, phi = rng.uniform(15.0, 40.0, A), rng.uniform(-np.pi, np.pi, A)
    p0 = np.stack([r0 * np.cos(phi), r0 * np.sin(phi)], axis=1)
    across, out = rng.uniform(-8.0, 8.0, A), rng.uniform(0.0, 2.0, A)
    v = np.stack([-across * np.sin(phi) + out * np.cos(phi), across * np.cos(phi) + out * np.sin(phi)], axis=1)
    t = dt * np.arange(m)
    ag[0, :, :, 0] = p0[:, :1] + v[:, :1] * t
    ag[0, :, :, 1] = p0[:, 1:] + v[:, 1:] * t
    ag[0, :, :, 2] = np.arctan2(v[:, 1], v[:, 0])[:, None]
    disc = rng.uniform(size=A) < 0.3
    ag[0, :, :, 3] = np.where(disc, 0.0, rng.uniform(1.5, 2.5, A))[:, None]
    ag[0, :, :, 4] = np.where(disc, 0.0, rng.uniform(0.8, 1.0, A))[:, None]
    ag[0, :, :, 5] = np.where(disc, 0.4, rng.uniform(0.0, 0.2, A))[:, None]
    return ag


def case(h, rng, B, m, A, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = WAYPOINTS
    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof = torch.empty((B, n, capi.SPEED_STRIDE), dtype=torch.float64, device=dev)
    d_sflags = torch.empty(B, dtype=torch.int32, device=dev)
    d_traj = torch.empty((B, m, capi.TRAJ_STRIDE), dtype=torch.float64, device=dev)
    d_m_of = torch.empty(B, dtype=torch.int32, device=dev)
    d_flags = torch.empty(B, dtype=torch.int32, device=dev)
    sp = capi.speed_default_params(h.lib)
    torch.cuda.synchronize(dev)
    rc = h.lib.pqp_speed_profile_device(h._h, capi.C.byref(sp), B, n, 7, d_paths, None, None, None, d_vs, None, d_prof, d_sflags)
    assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    arrive = float(np.median(d_prof[:, -1, 3].cpu().numpy()))
    sa = capi.sample_default_params(h.lib, dt=arrive / (m - 1), hold_last=1)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_sample_trajectory_device(h._h, capi.C.byref(sa), B, n, 7, d_paths, None, None, d_prof, None, m, d_traj, d_m_of, d_flags)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    sample_med = float(np.median(h.kernel_ms_history(steps)))
    d_agents = t(make_agents(rng, A, m, sa.dt))
    d_frames = torch.empty((1, A, m, capi.AGENT_FRAME_STRIDE), dtype=torch.float64, device=dev)
    d_first = torch.empty(B, dtype=torch.int32, device=dev)
    d_who = torch.empty(B, dtype=torch.int32, device=dev)
    d_clear = torch.empty((B, m), dtype=torch.float64, device=dev)
    ap, car = capi.agents_default_params(h.lib, margin=0.3), capi.car_default_geometry(h.lib)
    torch.cuda.synchronize(dev)
    out, firsts = [], []
    for with_clearance in (True, False):
        for _ in range(warmup + steps):
            rc = h.lib.pqp_agents_check_device(h._h, ap.margin, capi.C.byref(car), B, m, capi.TRAJ_STRIDE, d_traj, None, 1, A, d_agents, None,
                                               None, d_frames, d_first, d_who, d_clear if with_clearance else None)
            assert rc == 0, h.lib.pqp_last_error()
        h.sync()
        ms = h.kernel_ms_history(steps)
        med = float(np.median(ms))
        first = d_first.cpu().numpy()
        firsts.append((first, d_who.cpu().numpy()))
        nbytes = B * (64 * m + 8 + (8 * m if with_clearance else 0)) + A * m * (64 + 48 + 64)
        ops = B * m * A * 6 * OPS_PER_CIRCLE_TEST
        r = dict(paths=B, samples=m, agents=A, clearance=with_clearance, us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3,
                 paths_per_s=B / (med * 1e-3), circle_tests_per_s=B * m * A * 6 / (med * 1e-3), bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3),
                 fp64_ops=ops, fp64_ops_per_s=ops / (med * 1e-3), sample_trajectory_us=sample_med * 1e3, times_sample_trajectory=med / sample_med,
                 paths_hit=int((first < m).sum()))
        r["fraction_of_8TBps"] = r["bytes_per_s"] / PEAK_BYTES_PER_S
        print(f"{B:6d} paths x {m} samples x {A:2d} agents, clearance {'written' if with_clearance else 'NULL   '}: {r['us']:9.1f} us/call "
              f"(min {r['us_min']:.1f}, max {r['us_max']:.1f})  {nbytes / 2**20:7.1f} MiB = {100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s;  "
              f"{ops / 1e9:6.2f} G fp64 ops of the definition = {r['fp64_ops_per_s'] / 1e12:.2f} T/s;  {r['paths_hit']} paths hit;  "
              f"pqp_sample_trajectory on the same batch {r['sample_trajectory_us']:.1f} us: x {r['times_sample_trajectory']:.2f}", flush=True)
        out.append(r)
    assert np.array_equal(firsts[0][0], firsts[1][0]) and np.array_equal(firsts[0][1], firsts[1][1])     # the shortcuts do not show
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_agents_check: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [r for B, m, A in SHAPES for r in case(h, rng, B, m, A, args.steps, args.warmup)]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="agents_check_paths_per_s_1024x50x8", value=out[0]["paths_per_s"], paths_per_s_8192x50x16=out[2]["paths_per_s"],
                          paths_per_s_65536x50x32=out[4]["paths_per_s"], paths_per_s_65536x50x32_no_clearance=out[5]["paths_per_s"],
                          fp64_ops_per_s_65536x50x32=out[4]["fp64_ops_per_s"])))


if __name__ == "__main__":
    main()
