"""pqp_footprint_check on one GPU: device time per call (the handle's HIP events around its launch, after warm-up, median of the timed
calls) and states/s for batch in {1024, 8192, 65 536} x n in {80, 256} on the reference's map (tests/golden/gridmap_obstacle.npz -> its
distance layer, built on the device), in both modes; path-like states (0.3 m apart, slowly turning, as the chain returns them) from starts
spread over the map's free cells.  Then the chain's batch (tools/bench_distance_layer.py's: 1024 scenarios on 16 synth maps) with and
without check_footprint: wall clock per optimize_path call, and the check's own device time behind the chain.
Usage: python tools/bench_footprint.py [--steps K] [--warmup W] [--json PATH]"""
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

import distance_util as D  # noqa: E402
from path_optimizer_2_amd import capi  # noqa: E402
from path_optimizer_2_amd.synth import make_scene  # noqa: E402

MODES = {capi.FOOTPRINT_CIRCLES: "CIRCLES", capi.FOOTPRINT_BOUNDING_FIRST: "BOUNDING_FIRST"}


def path_states(rng, occ, dist, geom, B, n, spacing=0.3):
    """[B][n][3] paths: start on a free cell at least 2 m from any obstacle, heading random, curvature a slow random walk"""
    ok = np.argwhere(dist >= 2.0)
    pick = ok[rng.integers(0, len(ok), B)]
    x0 = geom.pos_x + 0.5 * geom.length_x - 0.5 * geom.resolution - geom.resolution * pick[:, 0]
    y0 = geom.pos_y + 0.5 * geom.length_y - 0.5 * geom.resolution - geom.resolution * pick[:, 1]
    k = np.cumsum(rng.normal(scale=0.003, size=(B, n)), axis=1)
    heading = rng.uniform(-np.pi, np.pi, B)[:, None] + np.cumsum(k * spacing, axis=1)
    st = np.zeros((B, n, 3))
    st[:, :, 0] = x0[:, None] + np.cumsum(np.cos(heading) * spacing, axis=1) - np.cos(heading[:, :1]) * spacing
    st[:, :, 1] = y0[:, None] + np.cumsum(np.sin(heading) * spacing, axis=1) - np.sin(heading[:, :1]) * spacing
    st[:, :, 2] = heading
    return st


def device_ms(h, args, steps, warmup):
    for _ in range(warmup):
        assert h.lib.pqp_footprint_check_device(*args) == 0
    for _ in range(steps):
        assert h.lib.pqp_footprint_check_device(*args) == 0
    h.sync()
    return h.kernel_ms_history(steps)


def case(h, d_dist, geom, states, mode, steps, warmup, margin=False):
    B, n, _ = states.shape
    dev = torch.device("cuda", h.device)
    d_st = torch.from_numpy(states).to(dev)
    d_free = torch.empty((B, n), dtype=torch.uint8, device=dev)
    d_first = torch.empty(B, dtype=torch.int32, device=dev)
    d_mg = torch.empty((B, n), dtype=torch.float64, device=dev) if margin else None
    torch.cuda.synchronize(dev)
    p = lambda x: None if x is None else capi.C.c_void_p(x.data_ptr())
    car = capi.car_default_geometry()
    args = (h._h, B, n, 3, p(d_st), None, p(d_dist), None, capi.C.byref(geom), capi.C.byref(car), mode, p(d_free), p(d_first), p(d_mg))
    ms = device_ms(h, args, steps, warmup)
    free = d_free.cpu().numpy()
    med = float(np.median(ms))
    r = dict(case=f"{MODES[mode]}{' + margin' if margin else ''}", batch=B, n=n, mode=MODES[mode], margin=margin, us=med * 1e3,
             us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3, states_per_s=B * n / (med * 1e-3), free_fraction=float(free.mean()),
             paths_clear=float((d_first.cpu().numpy() == n).mean()))
    print(f"{r['case']:24s} {B:6d} x {n:4d}: {r['us']:8.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f})  "
          f"{r['states_per_s'] / 1e9:6.2f} G states/s  free {100 * r['free_fraction']:5.1f} %  clear paths {100 * r['paths_clear']:5.1f} %", flush=True)
    return r


def chain(steps):
    """the chain's batch with and without check_footprint (wall clock per call, in blocks) and the check's device time behind it"""
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
    dist = np.stack([c["dist"] for c in cs])
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25), max_batch=B, max_n=128)
    run = lambda flag: h.optimize_path(pts, n_pts, start, target, dist, geom, map_of=map_of, smoother=hs, check_footprint=flag)
    times, blocks, kern = {False: [], True: []}, [], []
    run(False); run(True)
    for flag in (False, True, False, True):      # blocks of consecutive calls, each variant twice: the spread between blocks is the noise
        t = []
        for _ in range(steps):
            t0 = time.perf_counter(); r = run(flag); t.append(time.perf_counter() - t0)
            if flag:
                kern.append(float(h.kernel_ms_history(1)[0]))          # the last launch of the call: the footprint check
                rb = r
            else:
                ra = r
        times[flag] += t
        blocks.append((flag, 1e3 * float(np.median(t))))
    ta, tb = times[False], times[True]
    h.close(); hs.close()
    same = all(np.array_equal(ra[k], rb[k]) for k in ("out", "n_out", "status", "stage"))
    solved = rb["stage"] == 0
    r = dict(case="chain", batch=B, n_maps=n_maps, n_max=int(rb["out"].shape[1]), optimize_path_ms=1e3 * float(np.median(ta)),
             with_check_footprint_ms=1e3 * float(np.median(tb)), footprint_kernel_us=1e3 * float(np.median(kern)), outputs_identical=same,
             solved=int(solved.sum()), solved_paths_with_a_collision=int((rb["first_collision"][solved] < rb["n_out"][solved]).sum()),
             states_checked=int(rb["n_out"].sum()), block_medians_ms=[dict(check_footprint=f, ms=m) for f, m in blocks])
    print(f"chain, {B} scenarios on {n_maps} maps: optimize_path {r['optimize_path_ms']:.2f} ms, with check_footprint {r['with_check_footprint_ms']:.2f} ms "
          f"(wall clock per call, median of {2 * steps}; blocks in order: {', '.join(f'{m:.2f}' + (' +check' if f else '') for f, m in blocks)}); the check's kernel {r['footprint_kernel_us']:.1f} us for {r['states_checked']} states "
          f"(n_max {r['n_max']}); outputs identical: {same}; solved {r['solved']}, of which {r['solved_paths_with_a_collision']} put the car into an "
          f"obstacle", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_footprint: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    occ, res = D.reference_map()
    geom = capi.PqpGridGeometry(occ.shape[0], occ.shape[1], res, occ.shape[0] * res, occ.shape[1] * res, 0.0, 0.0)
    dist = h.distance_layer(occ, geom)
    d_dist = torch.from_numpy(np.ascontiguousarray(dist.T)).to(torch.device("cuda", 0))        # the ABI's column-major layer
    rng = np.random.default_rng(0)
    out = []
    for B in (1024, 8192, 65536):
        for n in (80, 256):
            states = path_states(rng, occ, dist, geom, B, n)
            for mode in MODES:
                out.append(case(h, d_dist, geom, states, mode, args.steps, args.warmup))
            if B == 65536 and n == 80:
                out.append(case(h, d_dist, geom, states, capi.FOOTPRINT_CIRCLES, args.steps, args.warmup, margin=True))
    h.close()
    out.append(chain(max(3, args.steps // 10)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    pick = {(r["batch"], r["n"], r["mode"]): r["us"] for r in out if r["case"] in MODES.values()}
    print(json.dumps(dict(metric="footprint_check_us_1024x80_circles", value=pick[(1024, 80, "CIRCLES")],
                          bounding_first_us=pick[(1024, 80, "BOUNDING_FIRST")], us_65536x80_circles=pick[(65536, 80, "CIRCLES")])))


if __name__ == "__main__":
    main()
