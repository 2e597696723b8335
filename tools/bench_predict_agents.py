"""pqp_predict_agents on one GPU: device time per call (the handle's HIP events around its launch, after warm-up, median of the timed
calls with min and max) at 128 scenes x 8 agents x 8 layers and at 1024 x 16 x 8 layers with r = 1 and r = 10 (71 fine steps).  Every
second agent follows one of 64 lanes (arcs of 60 m, 16 knots each), the others run the free model.  Two yardsticks beside each time: the
algorithmic bytes (72 per track read, 48 per step and 4 per slot written; the lanes' tables are read out of L2 and not counted) over
8 TB/s, and pqp_agents_check with one path on the same rows in the same run - its frames launch, the nearest existing kernel with the
same volume (48 bytes read and 64 written per row), plus one wavefront of checks.
Usage: python tools/bench_predict_agents.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402

SHAPES = ((128, 8, 8, 1), (1024, 16, 8, 1), (1024, 16, 8, 10))          # scenes, agents, layers, sub-steps
N_LANES, LANE_M, LANE_LENGTH = 64, 16, 60.0
PEAK_BYTES_PER_S = 8e12


def make_lanes(h, rng):
    """(spline [N_LANES][9][LANE_M], ext, length, the knots' x, y): arcs of LANE_LENGTH m with radii of 40 to 400 m, either way"""
    s = np.tile(np.linspace(0.0, LANE_LENGTH, LANE_M), (N_LANES, 1))
    radius = rng.uniform(40.0, 400.0, N_LANES) * rng.choice([-1.0, 1.0], N_LANES)
    x0, y0, h0 = rng.uniform(-200.0, 200.0, N_LANES), rng.uniform(-200.0, 200.0, N_LANES), rng.uniform(-np.pi, np.pi, N_LANES)
    phi = h0[:, None] + s / radius[:, None]
    x = x0[:, None] + radius[:, None] * (np.sin(phi) - np.sin(h0)[:, None])
    y = y0[:, None] - radius[:, None] * (np.cos(phi) - np.cos(h0)[:, None])
    tab, ext = h.spline_fit(s, x, y)
    return tab, ext, s[:, -1].copy(), x, y, phi


def make_tracks(rng, S, A, lanes):
    """tracks [S][A][9] and lane_of [S][A]: odd slots near a knot of a lane, within a metre of its line and along it; even slots free"""
    x, y, phi = lanes[3:]
    t = np.zeros((S, A, capi.TRACK_STRIDE))
    t[..., 0:2] = rng.uniform(-200.0, 200.0, (S, A, 2))
    t[..., 2] = rng.uniform(-np.pi, np.pi, (S, A))
    t[..., 3] = rng.uniform(0.0, 15.0, (S, A))
    t[..., 4] = rng.uniform(-2.0, 2.0, (S, A))
    t[..., 5] = rng.uniform(-0.3, 0.3, (S, A))
    t[..., 6], t[..., 7], t[..., 8] = rng.uniform(1.5, 2.5, (S, A)), rng.uniform(0.8, 1.0, (S, A)), rng.uniform(0.0, 0.2, (S, A))
    lane_of = np.full((S, A), -1, np.int32)
    which, knot = rng.integers(0, N_LANES, (S, A)), rng.integers(0, LANE_M // 2, (S, A))
    on = (np.arange(A) % 2 == 1)[None, :] & np.ones((S, 1), bool)
    t[on, 0] = x[which, knot][on] + rng.uniform(-0.7, 0.7, on.sum())
    t[on, 1] = y[which, knot][on] + rng.uniform(-0.7, 0.7, on.sum())
    t[on, 2] = phi[which, knot][on]
    lane_of[on] = which[on]
    return t, lane_of


def case(h, rng, lanes, S, A, m, r, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    M = (m - 1) * r + 1
    tracks, lane_of = make_tracks(rng, S, A, lanes)
    d_tracks, d_lane_of = t(tracks), t(lane_of)
    d_spl, d_ext, d_len = t(lanes[0]), t(lanes[1]), t(lanes[2])
    d_rows = torch.empty((S, A, M, capi.AGENT_STRIDE), dtype=torch.float64, device=dev)
    d_flags = torch.empty((S, A), dtype=torch.int32, device=dev)
    prm = capi.predict_default_params(h.lib).array()
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_predict_agents_device(h._h, prm, 0.0, 1.0, m, r, S, A, d_tracks, None, d_lane_of, N_LANES, LANE_M, d_spl, d_ext, d_len, d_rows,
                                             None, d_flags)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    ms = h.kernel_ms_history(steps)
    med = float(np.median(ms))
    flags = d_flags.cpu().numpy()
    # pqp_agents_check with one path on the same rows: its frames launch and one wavefront
    d_traj = torch.zeros((1, M, 3), dtype=torch.float64, device=dev)
    d_frames = torch.empty((S, A, M, capi.AGENT_FRAME_STRIDE), dtype=torch.float64, device=dev)
    d_first, d_who = (torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2))
    car = capi.car_default_geometry(h.lib)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_agents_check_device(h._h, 0.0, capi.C.byref(car), 1, M, 3, d_traj, None, S, A, d_rows, None, None, d_frames, d_first, d_who, None)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    frames_med = float(np.median(h.kernel_ms_history(steps)))
    nbytes = S * A * (8 * capi.TRACK_STRIDE + 4 + 8 * capi.AGENT_STRIDE * M)
    res = dict(scenes=S, agents=A, layers=m, r=r, steps=M, us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3,
               rows_per_s=S * A * M / (med * 1e-3), bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3), on_lane=int(((flags & capi.PREDICT_ON_LANE) != 0).sum()),
               agents_check_one_path_us=frames_med * 1e3, times_agents_check_one_path=med / frames_med)
    res["fraction_of_8TBps"] = res["bytes_per_s"] / PEAK_BYTES_PER_S
    print(f"{S:5d} scenes x {A:2d} agents x {m} layers, r = {r:2d} ({M:2d} steps): {res['us']:8.1f} us/call (min {res['us_min']:.1f}, max {res['us_max']:.1f})  "
          f"{nbytes / 2**20:6.2f} MiB = {100 * res['fraction_of_8TBps']:.2f} % of 8 TB/s;  {res['on_lane']} of {S * A} on a lane;  "
          f"pqp_agents_check with one path on the same rows {res['agents_check_one_path_us']:.1f} us: x {res['times_agents_check_one_path']:.2f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_predict_agents: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    lanes = make_lanes(h, rng)
    out = [case(h, rng, lanes, S, A, m, r, args.steps, args.warmup) for S, A, m, r in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="predict_agents_rows_per_s_1024x16x71", value=out[2]["rows_per_s"], us_128x8x8=out[0]["us"], us_1024x16x8=out[1]["us"],
                          us_1024x16x71=out[2]["us"])))


if __name__ == "__main__":
    main()
