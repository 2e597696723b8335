"""pqp_corridor_bounds_on_states on one GPU, next to pqp_corridor_bounds: device time per launch (the handle's HIP events, median of the
timed launches after warm-up) for batch in {1024, 8192, 65 536} x n = 80 over 8 synth maps, heading errors uniform in +-0.3 rad.  Then the
chain's batch of DESIGN 3.6 (1024 scenarios on 16 synth maps, tools/bench_footprint.py's) in both second-pass modes: wall clock per
optimize_path call and the footprint check's collision count of the SOLVED paths.
Usage: python tools/bench_corridor_on_states.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import scenes  # noqa: E402
from path_optimizer_2_amd import capi  # noqa: E402
from path_optimizer_2_amd.synth import make_scene  # noqa: E402


def kernels(batch, n, n_maps, steps, warmup):
    h = capi.Handle(capi.default_params(), device=0, max_batch=batch, max_n=n)
    sc = scenes.build(h, range(n_maps), n)
    geom = sc["geom"]
    dev = torch.device("cuda", 0)
    rep = lambda key: torch.from_numpy(np.stack([sc[key][b % n_maps] for b in range(batch)])).to(dev)
    ref, tab, ext = rep("ref"), rep("tab"), rep("ext")
    dist = torch.from_numpy(np.ascontiguousarray(np.transpose(sc["dist"], (0, 2, 1)))).to(dev)
    map_of = torch.arange(batch, dtype=torch.int32, device=dev) % n_maps
    states = torch.zeros((batch, n, 7), dtype=torch.float64, device=dev)
    states[:, :, 4] = torch.from_numpy(np.random.default_rng(0).uniform(-0.3, 0.3, size=(batch, n))).to(dev)
    bounds = torch.zeros((batch, n, 6), dtype=torch.float64, device=dev)
    nv = torch.zeros(batch, dtype=torch.int32, device=dev)
    prm = h.corridor_params()
    p = lambda t: capi.C.c_void_p(t.data_ptr())
    m = tab.shape[2]
    calls = {
        "corridor_bounds": lambda: h.lib.pqp_corridor_bounds_device(h._h, batch, n, m, p(ref), None, p(tab), p(ext), p(dist), p(map_of), capi.C.byref(geom),
                                                                    capi.C.byref(prm), p(bounds), p(nv)),
        "corridor_bounds_on_states": lambda: h.lib.pqp_corridor_bounds_on_states_device(h._h, batch, n, m, p(ref), None, p(states), 7, p(tab), p(ext), p(dist),
                                                                                        p(map_of), capi.C.byref(geom), capi.C.byref(prm), p(bounds), p(nv)),
    }
    res = {}
    for _ in range(2):                   # interleaved blocks: the spread between the two blocks of one entry point is the noise
        for name, f in calls.items():
            for _ in range(warmup):
                assert f() == 0
            for _ in range(steps):
                assert f() == 0
            h.sync()
            res.setdefault(name, []).append(float(np.median(h.kernel_ms_history(steps))) * 1e3)
    h.close()
    out = []
    for name, us in res.items():
        r = dict(case=name, batch=batch, n=n, us=float(np.median(us)), block_us=us, waypoints_per_s=batch * n / (np.median(us) * 1e-6))
        print(f"{name:28s} {batch:6d} x {n}: {r['us']:9.1f} us/launch (blocks {', '.join(f'{u:.1f}' for u in us)})  {r['waypoints_per_s'] / 1e6:7.1f} M waypoints/s",
              flush=True)
        out.append(r)
    return out


def chain_inputs(B=1024, n_maps=16):
    """tools/bench_footprint.py's chain batch: B scenarios on n_maps synth maps, full polygons with noise"""
    cs = [make_scene(seed=s, n=40, n_obstacles=25, knots_every=3.05) for s in range(n_maps)]
    rng = np.random.default_rng(5)
    p_max = len(cs[0]["knots_x"])
    pts = np.zeros((B, p_max, 2)); n_pts = np.full(B, p_max, dtype=np.int32); map_of = (np.arange(B) % n_maps).astype(np.int32)
    start = np.zeros((B, 3)); target = np.zeros((B, 3))
    for b in range(B):
        c = cs[b % n_maps]
        pts[b, :, 0] = c["knots_x"]; pts[b, :, 1] = c["knots_y"] + rng.normal(scale=0.15, size=p_max)
        h0 = np.arctan2(pts[b, 1, 1] - pts[b, 0, 1], pts[b, 1, 0] - pts[b, 0, 0])
        start[b] = (pts[b, 0, 0] + 0.1, pts[b, 0, 1] + 0.1, h0 + 0.03)
        h1 = np.arctan2(pts[b, -1, 1] - pts[b, -2, 1], pts[b, -1, 0] - pts[b, -2, 0])
        target[b] = (pts[b, -1, 0], pts[b, -1, 1], h1)
    c0 = cs[0]
    geom = capi.PqpGridGeometry(c0["rows"], c0["cols"], c0["resolution"], c0["length"][0], c0["length"][1], 0.0, 0.0)
    return pts, n_pts, start, target, np.stack([c["dist"] for c in cs]), geom, map_of


def chain(steps):
    pts, n_pts, start, target, dist, geom, map_of = chain_inputs()
    B = len(pts)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25), max_batch=B, max_n=128)
    cfg = {mode: h.chain_config(second_pass=mode) for mode in (capi.SECOND_PASS_RELINEARISE, capi.SECOND_PASS_BOUNDS_ON_STATES)}
    run = lambda mode: h.optimize_path(pts, n_pts, start, target, dist, geom, map_of=map_of, smoother=hs, cfg=cfg[mode], check_footprint=True)
    last, times, blocks = {}, {0: [], 1: []}, []
    run(0); run(1)
    for mode in (0, 1, 0, 1):
        t = []
        for _ in range(steps):
            t0 = time.perf_counter(); last[mode] = run(mode); t.append(time.perf_counter() - t0)
        times[mode] += t
        blocks.append((mode, 1e3 * float(np.median(t))))
    h.close(); hs.close()
    out = []
    for mode, r in last.items():
        solved = (r["stage"] == 0)
        rr = dict(case="chain", second_pass=["RELINEARISE", "BOUNDS_ON_STATES"][mode], batch=B, ms=1e3 * float(np.median(times[mode])),
                  block_ms=[m for k, m in blocks if k == mode], solved=int(solved.sum()),
                  solved_paths_with_a_collision=int((r["first_collision"][solved] < r["n_out"][solved]).sum()),
                  stages={int(s): int((r["stage"] == s).sum()) for s in np.unique(r["stage"])}, waypoints=int(r["n_out"][solved].sum()),
                  mean_iters=float(r["iters"][solved].mean()) if solved.any() else 0.0)
        print(f"chain {rr['second_pass']:16s} {B} scenarios: {rr['ms']:.2f} ms/call (blocks {', '.join(f'{m:.2f}' for m in rr['block_ms'])}); solved "
              f"{rr['solved']} ({rr['waypoints']} waypoints, {rr['mean_iters']:.0f} ADMM iterations each), of which {rr['solved_paths_with_a_collision']} put the "
              f"car into an obstacle; stages {rr['stages']}", flush=True)
        out.append(rr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for batch in (1024, 8192, 65536):
        rows += kernels(batch, 80, 8, a.steps, a.warmup)
    rows += chain(max(3, a.steps // 4))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
