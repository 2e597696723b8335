"""pqp_speed_profile on one GPU: device time per call (the handle's HIP events around its launch, after warm-up, median of the timed
calls) and paths/s at three shapes - 1024 paths x 80 waypoints, 8192 x 120, 65 536 x 80 - on an `out` of stride 7 read in place, beside
the algorithmic bytes: per path of c driven waypoints 56 c read (a stride-7 row is fetched whole: x, y and k lie 40 bytes apart in it)
and 32 c written, and what fraction of 8 TB/s those bytes per second are.  The kernel's own re-reads of the profile rows between its
three sweeps are served by the cache and are not counted.
Usage: python tools/bench_speed_profile.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402

SHAPES = ((1024, 80), (8192, 120), (65536, 80))
PEAK_BYTES_PER_S = 8e12


def make_paths(rng, B, n):
    """[B][n][7] slowly turning paths, a waypoint every 0.3 to 0.5 m, the columns of PQP_OUT_STRIDE"""
    step = rng.uniform(0.3, 0.5, (B, n))
    k = 0.05 * np.sin(np.cumsum(step, axis=1) / 15.0 + rng.uniform(0, 6.28, (B, 1))) + rng.normal(scale=0.005, size=(B, n))
    head = np.cumsum(k * step, axis=1) + rng.uniform(-np.pi, np.pi, (B, 1))
    p = np.zeros((B, n, 7))
    p[:, :, 0] = np.cumsum(step * np.cos(head), axis=1)
    p[:, :, 1] = np.cumsum(step * np.sin(head), axis=1)
    p[:, :, 2], p[:, :, 5] = head, k
    return p


def case(h, rng, B, n, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda v: capi.C.c_void_p(v.data_ptr())
    d_paths, d_vs = t(make_paths(rng, B, n)), t(rng.uniform(0.0, 8.0, B))
    d_prof = torch.empty((B, n, capi.SPEED_STRIDE), dtype=torch.float64, device=dev)
    d_flags = torch.empty(B, dtype=torch.int32, device=dev)
    prm = capi.speed_default_params(h.lib)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_speed_profile_device(h._h, capi.C.byref(prm), B, n, 7, p(d_paths), None, None, None, p(d_vs), None, p(d_prof), p(d_flags))
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    ms = h.kernel_ms_history(steps)
    flags = d_flags.cpu().numpy()
    med = float(np.median(ms))
    nbytes = B * n * (56 + 32)
    r = dict(paths=B, waypoints=n, us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3, paths_per_s=B / (med * 1e-3),
             bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3), start_too_fast=int((flags & capi.SPEED_START_TOO_FAST != 0).sum()),
             other_flags=int((flags & ~capi.SPEED_START_TOO_FAST != 0).sum()))
    r["fraction_of_8TBps"] = r["bytes_per_s"] / PEAK_BYTES_PER_S
    print(f"{B:6d} paths x {n:4d} waypoints: {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f})  {r['paths_per_s'] / 1e6:8.2f} M paths/s  "
          f"{nbytes / 2**20:7.1f} MiB read + written, {r['bytes_per_s'] / 1e12:.3f} TB/s = {100 * r['fraction_of_8TBps']:.1f} % of 8 TB/s", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_speed_profile: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, B, n, args.steps, args.warmup) for B, n in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="speed_profile_paths_per_s_1024x80", value=out[0]["paths_per_s"], paths_per_s_8192x120=out[1]["paths_per_s"],
                          paths_per_s_65536x80=out[2]["paths_per_s"], fraction_of_8TBps_65536x80=out[2]["fraction_of_8TBps"])))


if __name__ == "__main__":
    main()
