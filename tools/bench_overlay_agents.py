"""pqp_overlay_agents on one GPU: device time per call (the handle's HIP events around its two launches, after warm-up, median of the
timed calls with min and max) at 256 scenes x 8 agents and at 1024 scenes x 16 agents on layers of 350 x 200 cells from 16 base maps -
once with the agents clustered near the obstacles of synthetic scenes (synth.make_scene), where most tiles leave most agents out, and
once on a base without obstacle, where no tile leaves any out.  Two yardsticks beside each time: (a) pqp_distance_layer on as many
occupancy grids as there are scenes in the same run - what stamping the agents into bytes and rebuilding every scene's layer would pay
at least; (b) the streaming model, 4 B read and 4 B written per cell and scene, over 8 TB/s.
Usage: python tools/bench_overlay_agents.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402
from path_optimizer_2_amd.synth import make_scene  # noqa: E402

SHAPES = ((256, 8), (1024, 16))                  # scenes, agents
N_MAPS = 16
PEAK_BYTES_PER_S = 8e12


def make_agents(rng, scenes, S, A, base_of, clustered):
    """[S][A][6]: parked-car sized boxes, clustered - within 1.5 m of an obstacle cell of the scene's base map; else anywhere in the map"""
    c0 = scenes[0]
    cx = 0.5 * c0["length"][0] - 0.5 * c0["resolution"] - c0["resolution"] * np.arange(c0["rows"])
    cy = 0.5 * c0["length"][1] - 0.5 * c0["resolution"] - c0["resolution"] * np.arange(c0["cols"])
    ag = np.zeros((S, A, capi.AGENT_STRIDE))
    for s in range(S):
        if clustered:
            cells = np.argwhere(scenes[base_of[s]]["dist"] == 0)
            pick = cells[rng.integers(0, len(cells), A)]
            ag[s, :, 0], ag[s, :, 1] = cx[pick[:, 0]] + rng.uniform(-1.5, 1.5, A), cy[pick[:, 1]] + rng.uniform(-1.5, 1.5, A)
        else:
            ag[s, :, 0], ag[s, :, 1] = rng.uniform(cx.min(), cx.max(), A), rng.uniform(cy.min(), cy.max(), A)
    ag[..., 2] = rng.uniform(-np.pi, np.pi, (S, A))
    ag[..., 3], ag[..., 4], ag[..., 5] = rng.uniform(1.8, 2.6, (S, A)), rng.uniform(0.8, 1.0, (S, A)), rng.uniform(0.0, 0.2, (S, A))
    return ag


def case(h, rng, scenes, geom, S, A, clustered, steps, warmup):
    dev = torch.device("cuda", h.device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    rows, cols = geom.rows, geom.cols
    if clustered:
        base = np.stack([c["dist"] for c in scenes])
    else:
        base = np.full((N_MAPS, rows, cols), np.float32(np.hypot(rows, cols) * geom.resolution), np.float32)
    base_of = (np.arange(S) % N_MAPS).astype(np.int32)
    agents = make_agents(rng, scenes, S, A, base_of, clustered)
    d_base, d_agents, d_base_of = t(capi._column_major(base, np.float32), np.float32), t(agents, np.float64), t(base_of, np.int32)
    d_frames = torch.empty((S, A, capi.AGENT_FRAME_STRIDE), dtype=torch.float64, device=dev)
    d_out = torch.empty((S, cols, rows), dtype=torch.float32, device=dev)
    d_flags = torch.empty(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_overlay_agents_device(h._h, 0.0, N_MAPS, capi.C.byref(geom), d_base, S, A, d_agents, None, d_base_of, d_frames, d_out, d_flags)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    ms = h.kernel_ms_history(steps)
    med = float(np.median(ms))
    undercut = float((d_out < d_base[torch.from_numpy(base_of).long().to(dev)]).float().mean().item())
    # (a) the layers of S occupancy grids, rebuilt: the obstacles of the scene's base map (the stamped agents would only add zeros)
    grids = np.stack([np.where(c["dist"] == 0, 0, 255).astype(np.uint8) for c in scenes]) if clustered else np.full((N_MAPS, rows, cols), 255, np.uint8)
    d_grid = t(capi._column_major(grids[base_of], np.uint8), np.uint8)
    torch.cuda.synchronize(dev)
    for _ in range(warmup + steps):
        rc = h.lib.pqp_distance_layer_device(h._h, S, capi.C.byref(geom), d_grid, d_out)
        assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    rebuild = float(np.median(h.kernel_ms_history(steps)))
    nbytes = 8 * S * rows * cols
    res = dict(scenes=S, agents=A, rows=rows, cols=cols, clustered=bool(clustered), us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3,
               cells_undercut=undercut, distance_layer_us=rebuild * 1e3, times_distance_layer=med / rebuild, bytes=nbytes,
               fraction_of_8TBps=nbytes / (med * 1e-3) / PEAK_BYTES_PER_S, cell_agents_per_s=S * rows * cols * A / (med * 1e-3))
    print(f"{S:5d} scenes x {rows} x {cols} cells x {A:2d} agents, {'clustered near obstacles' if clustered else 'on a base without obstacle'}: "
          f"{res['us']:8.1f} us/call (min {res['us_min']:.1f}, max {res['us_max']:.1f}), {100 * undercut:.1f} % of the cells undercut;  "
          f"(a) pqp_distance_layer on {S} maps {res['distance_layer_us']:.1f} us: x {res['times_distance_layer']:.2f};  "
          f"(b) {nbytes / 2**20:.0f} MiB streamed = {100 * res['fraction_of_8TBps']:.1f} % of 8 TB/s", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_overlay_agents: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    scenes = [make_scene(seed=s) for s in range(N_MAPS)]
    c0 = scenes[0]
    geom = capi.PqpGridGeometry(c0["rows"], c0["cols"], c0["resolution"], c0["length"][0], c0["length"][1], c0["pos"][0], c0["pos"][1])
    out = [case(h, rng, scenes, geom, S, A, clustered, args.steps, args.warmup) for S, A in SHAPES for clustered in (True, False)]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="overlay_agents_us_1024x350x200x16_clustered", value=out[2]["us"], us_256x8_clustered=out[0]["us"],
                          us_256x8_open=out[1]["us"], us_1024x16_open=out[3]["us"], distance_layer_us_256=out[0]["distance_layer_us"],
                          distance_layer_us_1024=out[2]["distance_layer_us"])))


if __name__ == "__main__":
    main()
