"""pqp_distance_layer on one GPU: device time per call (the handle's HIP events around its two launches, after warm-up, median of the
timed calls), cells/s and the HBM fraction by the byte model below, for the reference's map, the chain's synth map size, large maps and
the worst cases; scipy's exact transform on the host in the same run as a baseline; and the chain end to end from occupancy grids
(optimize_path_on_grid) against scipy + optimize_path on the same batch.
Usage: python tools/bench_distance_layer.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

import distance_util as D  # noqa: E402
from path_optimizer_2_amd import capi  # noqa: E402
from path_optimizer_2_amd.synth import make_scene  # noqa: E402

# byte model: phase A reads 1 B and writes 4 B per cell, phase B reads 4 B and writes 4 B (the envelope stack's traffic, which stays in
# the caches of the lane's own line, is not counted)
BYTES_PER_CELL = 1 + 4 + 4 + 4
HBM_BYTES_PER_S = 6.29e12          # MI355X, measured float4 copy


def device_ms(h, n_maps, geom, d_grid, d_dist, steps, warmup):
    p = lambda x: capi.C.c_void_p(x.data_ptr())
    for _ in range(warmup):
        assert h.lib.pqp_distance_layer_device(h._h, n_maps, capi.C.byref(geom), p(d_grid), p(d_dist)) == 0
    for _ in range(steps):
        assert h.lib.pqp_distance_layer_device(h._h, n_maps, capi.C.byref(geom), p(d_grid), p(d_dist)) == 0
    h.sync()
    return h.kernel_ms_history(steps)


def scipy_ms(maps, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        for g in maps:
            ndimage.distance_transform_edt(g != 0)
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def case(h, name, maps, res, steps, warmup, scipy_maps=None):
    n_maps, rows, cols = maps.shape
    geom = capi.PqpGridGeometry(rows, cols, res, rows * res, cols * res, 0.0, 0.0)
    dev = torch.device("cuda", h.device)
    d_grid = torch.from_numpy(np.ascontiguousarray(np.transpose(maps, (0, 2, 1)))).to(dev)
    d_dist = torch.empty((n_maps, cols, rows), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ms = device_ms(h, n_maps, geom, d_grid, d_dist, steps, warmup)
    got = np.transpose(d_dist.cpu().numpy(), (0, 2, 1))
    check = [0, n_maps - 1]
    exact = all(np.array_equal(got[k].view(np.int32), D.distance_layer(maps[k], res).view(np.int32)) for k in check)
    med = float(np.median(ms))
    cells = n_maps * rows * cols
    r = dict(case=name, n_maps=n_maps, rows=rows, cols=cols, ms=med, ms_min=float(ms.min()), ms_max=float(ms.max()), cells_per_s=cells / med * 1e3,
             hbm_fraction=cells * BYTES_PER_CELL / HBM_BYTES_PER_S / (med * 1e-3), bit_exact_checked_maps=exact)
    if scipy_maps is not None:
        sm = scipy_ms(maps[:scipy_maps], 3)
        r["scipy_ms"] = sm * n_maps / scipy_maps
        r["scipy_maps_timed"] = scipy_maps
    print(f"{name:36s} {n_maps:4d} x {rows:5d} x {cols:5d}: {med * 1e3:9.1f} us/call  (min {ms.min() * 1e3:.1f}, max {ms.max() * 1e3:.1f})  "
          f"{cells / med * 1e3 / 1e9:7.2f} Gcells/s  HBM {100 * r['hbm_fraction']:5.1f} %"
          + (f"  scipy {r['scipy_ms']:9.2f} ms" if "scipy_ms" in r else "") + f"  exact={exact}", flush=True)
    return r


def chain_e2e(steps):
    """the chain's own batch (tests/test_gpu_chain.py's kind of scenarios) from occupancy grids: scipy on the host + optimize_path against
    optimize_path_on_grid, wall clock of the whole call (uploads, launches and the copies back included)"""
    B, n_maps = 1024, 16
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
    occ = np.stack([D.occupancy_of(c["dist"]) for c in cs])
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25), max_batch=B, max_n=128)

    def host_layers():
        return np.stack([(ndimage.distance_transform_edt(g != 0) * c0["resolution"]).astype(np.float32) for g in occ])

    def a():
        return h.optimize_path(pts, n_pts, start, target, host_layers(), geom, map_of=map_of, smoother=hs)

    def b():
        return h.optimize_path_on_grid(pts, n_pts, start, target, occ, geom, map_of=map_of, smoother=hs)
    ta, tb = [], []
    a(); b()
    for _ in range(steps):                   # alternated, so that both see the same host
        t0 = time.perf_counter(); ra = a(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); rb = b(); tb.append(time.perf_counter() - t0)
    h.close(); hs.close()
    r = dict(case="chain end to end", batch=B, n_maps=n_maps, rows=c0["rows"], cols=c0["cols"], scipy_plus_optimize_path_ms=1e3 * float(np.median(ta)),
             optimize_path_on_grid_ms=1e3 * float(np.median(tb)), solved_scipy=int((ra["stage"] == 0).sum()), solved_on_grid=int((rb["stage"] == 0).sum()))
    print(f"chain end to end, {B} scenarios on {n_maps} maps of {c0['rows']} x {c0['cols']}: scipy + optimize_path {r['scipy_plus_optimize_path_ms']:.2f} ms, "
          f"optimize_path_on_grid {r['optimize_path_on_grid_ms']:.2f} ms (wall clock per call, median of {steps}); solved {r['solved_scipy']} / "
          f"{r['solved_on_grid']}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_distance_layer: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    ref, res = D.reference_map()
    synth = np.stack([D.occupancy_of(make_scene(seed=s)["dist"]) for s in range(256)])
    big = np.stack([np.where(rng.uniform(size=(2048, 2048)) < 0.02, 0, 255).astype(np.uint8) for _ in range(16)])
    corner = np.full((16, 2048, 2048), 255, np.uint8); corner[:, 0, 0] = 0
    empty = np.full((16, 2048, 2048), 255, np.uint8)
    chk = np.broadcast_to(np.where(np.indices((2048, 2048)).sum(axis=0) % 2 == 0, 0, 255).astype(np.uint8), (16, 2048, 2048)).copy()
    out = [case(h, "reference map (gridmap.png)", ref[None], res, args.steps, args.warmup, scipy_maps=1),
           case(h, "synth maps (make_scene)", synth, 0.2, args.steps, args.warmup, scipy_maps=16),
           case(h, "2048^2, 2 % obstacles", big, 0.2, args.steps, args.warmup, scipy_maps=1),
           case(h, "2048^2, one obstacle in a corner", corner, 0.2, args.steps, args.warmup, scipy_maps=1),
           case(h, "2048^2, no obstacle", empty, 0.2, args.steps, args.warmup),
           case(h, "2048^2, checkerboard", chk, 0.2, args.steps, args.warmup, scipy_maps=1),
           case(h, "reference map x 256", np.broadcast_to(ref, (256,) + ref.shape).copy(), res, args.steps, args.warmup)]
    h.close()
    out.append(chain_e2e(max(3, args.steps // 10)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="distance_layer_reference_map_us", value=out[0]["ms"] * 1e3, synth_256_us=out[1]["ms"] * 1e3)))


if __name__ == "__main__":
    main()
