"""Device time per call of the line-geometry kernels' LDS and long forms (PQP_OPT_LONG_LINES), and the chain on long lines.
  - every line kernel: option 0 (LDS form) against option 2 (long form) at the largest size both accept, then option 1 at 2x, 4x, 8x it
  - pqp_optimize_path_device under option 1 on lines of 0.5, 1, 2, 4 km, batch 64 and 1024
One JSON line per measurement.  Usage: python tools/bench_long_lines.py [--reps 5] [--skip-chain] [--chain-batches 64,1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import corridor_oracle as K          # noqa: E402
import corridor_util as U            # noqa: E402
import long_line_util as LL          # noqa: E402
from path_optimizer_2_amd import capi  # noqa: E402

B = 64


def line(rng, m, length):
    d = np.exp(rng.uniform(np.log(0.2), np.log(3.0), m - 1))
    s = np.concatenate([[0.0], np.cumsum(d * (length / d.sum()))])
    x, y = s * 0.9, 5.0 * np.sin(s / 80.0)
    tab, ext = K.pack_spline(K.spline_fit(s, x), K.spline_fit(s, y))
    return s, x, y, tab, ext


def dp_layers(k):
    """max_layers for a road of k metres along x: its arc length (< 1.01 k) in 1.5 m layers, and a margin"""
    return int(1.01 * k / 1.5) + 16


def cases(rng, helper):
    """kernel -> (edge size, run(h, k) for size k = edge * factor)"""
    def fit(h, k):
        s, x, y, _, _ = line(rng, k, 1.0 * k)
        h.spline_fit(*(np.repeat(a[None], B, 0) for a in (s, x, y)))

    def states(h, k):          # m = 65 knots, k states of 0.15 .. 0.3 m
        _, _, _, tab, ext = line(rng, 65, 0.25 * k)
        h.reference_states(np.repeat(tab[None], B, 0), np.repeat(ext[None], B, 0), np.full(B, 0.2 * k), k)

    def length(h, k):
        _, _, _, tab, ext = line(rng, k, 1.0 * k)
        h.reference_length(np.repeat(tab[None], B, 0), np.repeat(ext[None], B, 0), np.full(B, 1.0 * k), np.tile([0.5 * k, 30.0, 0.0], (B, 1)))

    def offsets(h, k):         # table of 1000 knots, k points
        _, _, _, tab, ext = line(rng, 1000, 1500.0)
        at = np.repeat(np.linspace(0.0, 1500.0, k)[None], B, 0)
        h.offsets_to_points(np.repeat(tab[None], B, 0), np.repeat(ext[None], B, 0), at, np.zeros_like(at))

    def bspline(h, k):         # points 100 m apart, as many as make about k samples (65 at the edge size), k samples
        p = max(65, int(round(65 * k / bsp_edge)))
        pts = np.cumsum(np.column_stack([np.full(p, 100.0), rng.uniform(-20.0, 20.0, p)]), axis=0)
        r = h.bspline_resample(np.repeat(pts[None], B, 0), np.full(B, p, dtype=np.int32), k)
        return dict(samples=int(np.median(r["count"])))

    roads = {}

    def road(k):
        if k not in roads:
            roads[k] = LL.long_road(float(k), seed=k)
        r = roads[k]
        return r, LL.road_spline(r)

    def dp(h, k):              # a road of k metres along x, 1 m knots; layers for its arc length (the winding adds ~0.2 %)
        r, ln = road(k)
        assert ln["length"] < 1.01 * k
        st = np.array([r["x"][0] + 0.2, r["y"][0] - 0.3, 0.05])
        out = h.dp_corridor(np.repeat(ln["tab"][None], B, 0), np.repeat(ln["ext"][None], B, 0), np.full(B, ln["length"]), np.repeat(st[None], B, 0),
                            r["dist"], r["geom"], max_layers=dp_layers(k))
        assert (out[3] > 0).all(), out[3]            # the search ran (-1: more layers than max_layers, 0: nothing reachable)
        return dict(layers=int(np.median(out[3])))

    def corridor(h, k):        # a road of k metres, 1 m knots, waypoints every 0.3 m (first 2000)
        r, ln = road(k)
        ref, cnt, _ = helper.reference_states(ln["tab"][None], ln["ext"][None], np.array([ln["length"]]), 2000)
        ref = np.repeat(ref, B, 0)
        h.corridor_bounds(ref, np.repeat(ln["tab"][None], B, 0), np.repeat(ln["ext"][None], B, 0), r["dist"], r["geom"])

    nlat = U.dp_lateral_samples()
    bsp_edge = U.largest("bspline_resample_kernel", "n_max", p_max=65)
    k = 100                    # (knots and layers both grow with the road)
    while U.fits("dp_corridor_kernel", m=k + 1, max_layers=dp_layers(k), nlat=nlat):
        k += 10
    return {"spline_fit": (U.largest("spline_fit_kernel", "m"), fit),
            "reference_states": (U.largest("reference_states_kernel", "n_max", m=65), states),
            "reference_length": (U.largest("reference_length_kernel", "m"), length),
            "offsets_to_points": (U.largest("offsets_to_points_kernel", "m", m_spline=1000), offsets),
            "bspline_resample": (U.largest("bspline_resample_kernel", "n_max", p_max=65), bspline),
            "dp_corridor": (k - 10, dp),
            "corridor_bounds": (2200, corridor)}


def timed(h, fn, k, reps):
    """median device time of `reps` calls, and what the last call reports of its work (or {})"""
    fn(h, k)                                   # warm-up (allocations, code load)
    ms = []
    for _ in range(reps):
        info = fn(h, k) or {}
        ms.append(h.last_kernel_ms())
    return float(np.median(ms)), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--chain-only", action="store_true")
    ap.add_argument("--chain-batches", default="64,1024")
    ap.add_argument("--chain-km", default="0.5,1,2,4")
    ap.add_argument("--only", default="", help="comma-separated kernels to measure (default: all)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    hs = {v: LL.with_option(capi.Handle(capi.default_params(), device=0, max_batch=B, max_n=128), v) for v in (0, 1, 2)}
    if not a.chain_only:
        for name, (edge, fn) in cases(rng, hs[1]).items():
            if a.only and name not in a.only.split(","):
                continue
            (t0, i0), (t2, _) = timed(hs[0], fn, edge, a.reps), timed(hs[2], fn, edge, a.reps)
            print(json.dumps(dict(kernel=name, size=edge, batch=B, lds_ms=t0, long_ms=t2, ratio=t2 / t0, **i0)), flush=True)
            for f in (2, 4, 8):
                try:
                    t1, i1 = timed(hs[1], fn, edge * f, a.reps)
                    print(json.dumps(dict(kernel=name, size=edge * f, factor=f, batch=B, option1_ms=t1, **i1)), flush=True)
                except capi.PqpError as e:
                    print(json.dumps(dict(kernel=name, size=edge * f, factor=f, batch=B, error=str(e))), flush=True)
    if a.skip_chain:
        return
    for km in (float(v) for v in a.chain_km.split(",")):
        road = LL.long_road(1000.0 * km + 30.0, seed=int(km * 10))
        pts, st, tg = LL.road_points(road, 20.0)
        for batch in (int(v) for v in a.chain_batches.split(",")):
            h = LL.with_option(capi.Handle(capi.production_params(), max_batch=batch, max_n=int(2200 * km) + 200), 1)
            sm = capi.Handle(capi.default_params(eps_abs=1e-3, eps_rel=1e-3, polish=1, polish_every=25, adaptive_rho_interval=25), max_batch=batch,
                             max_n=int(1100 * km) + 100)
            cfg = h.chain_config(raw_max=int(1100 * km) + 100, sample_max=int(1100 * km) + 100, layer_max=int(750 * km) + 50, n_max=int(2200 * km) + 200,
                                 output_spacing=1.0)
            P = np.repeat(pts[None], batch, 0); n_pts = np.full(batch, len(pts), dtype=np.int32)
            S = np.repeat(st[None], batch, 0); T = np.repeat(tg[None], batch, 0)
            try:
                r = h.optimize_path(P, n_pts, S, T, road["dist"], road["geom"], smoother=sm, cfg=cfg)        # warm-up
                t = time.perf_counter()
                r = h.optimize_path(P, n_pts, S, T, road["dist"], road["geom"], smoother=sm, cfg=cfg)
                wall = (time.perf_counter() - t) * 1e3
                stages, counts = np.unique(r["stage"], return_counts=True)
                print(json.dumps(dict(chain_km=km, batch=batch, wall_ms=wall, stages={int(s): int(c) for s, c in zip(stages, counts)},
                                      n_out_median=float(np.median(r["n_out"])))), flush=True)
            except capi.PqpError as e:
                print(json.dumps(dict(chain_km=km, batch=batch, error=str(e))), flush=True)
            h.close(); sm.close()


if __name__ == "__main__":
    main()
