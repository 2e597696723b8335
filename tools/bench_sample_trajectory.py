"""pqp_sample_trajectory on one GPU: device time per call (the handle's HIP events around its launch, after warm-up, median of the timed
calls with min and max) at 1024 paths x 80 waypoints -> 50 samples, 8192 x 120 -> 50, 65 536 x 80 -> 50 and 100, on an `out` of stride 7
and the profile pqp_speed_profile wrote for it, both read in place.  Two yardsticks beside each time: the algorithmic bytes - per path of
c driven waypoints 88 c read (56 of the stride-7 row, 32 of the profile row) and 64 m + 8 written - as a fraction of 8 TB/s, and
pqp_speed_profile's own time on the same batch in the same run.  dt is chosen per shape so that the horizon ends near the median arrival
time: most samples lie on the path and the whole t column is walked.
Usage: python tools/bench_sample_trajectory.py [--steps K] [--warmup W] [--json PATH]"""
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

SHAPES = ((1024, 80, 50), (8192, 120, 50), (65536, 80, 50), (65536, 80, 100))
PEAK_BYTES_PER_S = 8e12


def case(h, rng, B, n, m, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda v: capi.C.c_void_p(v.data_ptr())
    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof = torch.empty((B, n, capi.SPEED_STRIDE), dtype=torch.float64, device=dev)
    d_sflags = torch.empty(B, dtype=torch.int32, device=dev)
    d_traj = torch.empty((B, m, capi.TRAJ_STRIDE), dtype=torch.float64, device=dev)
    d_m_of = torch.empty(B, dtype=torch.int32, device=dev)
    d_flags = torch.empty(B, dtype=torch.int32, device=dev)
    sp = capi.speed_default_params(h.lib)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_speed_profile_device(h._h, capi.C.byref(sp), B, n, 7, p(d_paths), None, None, None, p(d_vs), None, p(d_prof), p(d_sflags))
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    speed_ms = h.kernel_ms_history(steps)
    arrive = float(np.median(d_prof[:, -1, 3].cpu().numpy()))
    sa = capi.sample_default_params(h.lib, dt=arrive / (m - 1))
    for _ in range(warmup + steps):
        rc = h.lib.pqp_sample_trajectory_device(h._h, capi.C.byref(sa), B, n, 7, p(d_paths), None, None, p(d_prof), None, m, p(d_traj), p(d_m_of),
                                                p(d_flags))
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    ms = h.kernel_ms_history(steps)
    flags, m_of = d_flags.cpu().numpy(), d_m_of.cpu().numpy()
    med, speed_med = float(np.median(ms)), float(np.median(speed_ms))
    nbytes = B * (88 * n + 64 * m + 8)
    r = dict(paths=B, waypoints=n, samples=m, dt=sa.dt, us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3,
             paths_per_s=B / (med * 1e-3), bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3), speed_profile_us=speed_med * 1e3,
             times_speed_profile=med / speed_med, mean_samples_on_path=float(m_of.mean()),
             not_finite=int((flags & capi.TRAJ_NOT_FINITE != 0).sum()), horizon_short=int((flags & capi.TRAJ_HORIZON_SHORT != 0).sum()))
    r["fraction_of_8TBps"] = r["bytes_per_s"] / PEAK_BYTES_PER_S
    print(f"{B:6d} paths x {n:4d} waypoints -> {m:3d} samples (dt {sa.dt:.3f} s, {r['mean_samples_on_path']:.1f} on the path): {r['us']:9.1f} us/call "
          f"(min {r['us_min']:.1f}, max {r['us_max']:.1f})  {nbytes / 2**20:7.1f} MiB read + written, {r['bytes_per_s'] / 1e12:.3f} TB/s = "
          f"{100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s;  pqp_speed_profile on the same batch {r['speed_profile_us']:.1f} us: x {r['times_speed_profile']:.2f}",
          flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sample_trajectory: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, B, n, m, args.steps, args.warmup) for B, n, m in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="sample_trajectory_paths_per_s_1024x80x50", value=out[0]["paths_per_s"], paths_per_s_8192x120x50=out[1]["paths_per_s"],
                          paths_per_s_65536x80x50=out[2]["paths_per_s"], paths_per_s_65536x80x100=out[3]["paths_per_s"],
                          fraction_of_8TBps_65536x80x50=out[2]["fraction_of_8TBps"])))


if __name__ == "__main__":
    main()
