"""pqp_project_points on one GPU: device time per call (the handle's HIP events around its launch, after warm-up, median of the timed
calls) and points/s at three shapes - 1024 lines x 256 points on 30 m lines, 64 x 16 384 on 200 m lines, 1 x 262 144 on a 2 km line -
against the same points through pqp_reference_length_device with one row per point, which is what a caller could do before: every row
carries a copy of its line's 9 x m table, and the answer is a projection only for a point behind the line's end, so the baseline takes the
points that lie behind it (nearly all of them).  Its rows are capped (--baseline-bytes of replicated tables); its rate is per row.
Usage: python tools/bench_project.py [--steps K] [--warmup W] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from path_optimizer_2_amd import capi  # noqa: E402

SHAPES = ((1024, 256, 30.0), (64, 16384, 200.0), (1, 262144, 2000.0))
KNOTS_EVERY = 3.0


def make_lines(rng, B, length):
    """B slowly turning lines of `length` metres as knot lists (s, x, y), a knot every 3 m, and the heading at every knot"""
    s = np.arange(0.0, length + KNOTS_EVERY, KNOTS_EVERY)
    curv = 0.02 * np.sin(s[None] / 40.0 + rng.uniform(0, 6.28, (B, 1))) + rng.normal(scale=0.003, size=(B, s.size))
    head = np.cumsum(curv * KNOTS_EVERY, axis=1) + rng.uniform(-np.pi, np.pi, (B, 1))
    x = np.concatenate([np.zeros((B, 1)), np.cumsum(np.cos(head[:, :-1]) * KNOTS_EVERY, axis=1)], axis=1)
    y = np.concatenate([np.zeros((B, 1)), np.cumsum(np.sin(head[:, :-1]) * KNOTS_EVERY, axis=1)], axis=1)
    return np.broadcast_to(s, (B, s.size)).copy(), x, y, head


def make_points(rng, x, y, head, q, length):
    """[B][q][3] points within 6 m of their line, up to 3 m beyond either end, a random heading"""
    B, m = x.shape
    k = rng.integers(0, min(m, int(length / KNOTS_EVERY) + 1), (B, q))
    along, off = rng.uniform(-3.0, 3.0, (B, q)), rng.uniform(-6.0, 6.0, (B, q))
    rows = np.arange(B)[:, None]
    hx, hy = np.cos(head[rows, k]), np.sin(head[rows, k])
    pts = np.empty((B, q, 3))
    pts[:, :, 0] = x[rows, k] + along * hx - off * hy
    pts[:, :, 1] = y[rows, k] + along * hy + off * hx
    pts[:, :, 2] = rng.uniform(-np.pi, np.pi, (B, q))
    return pts


def timed(h, fn, args, steps, warmup):
    for _ in range(warmup + steps):
        assert fn(*args) == 0, h.lib.pqp_last_error()
    h.sync()
    return h.kernel_ms_history(steps)


def case(h, rng, B, q, length, steps, warmup, baseline_bytes):
    dev = torch.device("cuda", h.device)
    s, x, y, head = make_lines(rng, B, length)
    tab, ext = h.spline_fit(s, x, y)
    m = tab.shape[2]
    pts = make_points(rng, x, y, head, q, length)
    t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda v: capi.C.c_void_p(v.data_ptr())
    d_tab, d_ext, d_len, d_pts = t(tab), t(ext), t(np.full(B, length)), t(pts)
    d_proj = torch.empty((B, q, capi.PROJ_STRIDE), dtype=torch.float64, device=dev)
    d_flags = torch.empty((B, q), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ms = timed(h, h.lib.pqp_project_points_device, (h._h, B, m, p(d_tab), p(d_ext), p(d_len), q, 3, 1, p(d_pts), None, p(d_proj), p(d_flags)),
               steps, warmup)
    proj, flags = d_proj.cpu().numpy(), d_flags.cpu().numpy()
    # the baseline: one row per point, each with its line's table; only points behind the line's end are projected at all
    rows = int(min(B * q, max(1024, baseline_bytes // (9 * m * 8))))
    pick = rng.choice(B * q, rows, replace=False) if rows < B * q else np.arange(B * q)
    line = pick // q
    flat = pts.reshape(B * q, 3)[pick]
    k0 = int(length / KNOTS_EVERY)                 # the line's end: on the chord that leaves knot k0, to the spline's deviation from it
    ex, ey = x[line, k0] + (length - s[0, k0]) * np.cos(head[line, k0]), y[line, k0] + (length - s[0, k0]) * np.sin(head[line, k0])
    local_x = (flat[:, 0] - ex) * np.cos(head[line, k0]) + (flat[:, 1] - ey) * np.sin(head[line, k0])
    keep = local_x < -0.5                          # behind the end's normal with room to spare
    pick, line, flat = pick[keep], line[keep], flat[keep]
    rows = len(pick)
    b_tab, b_ext, b_len, b_tgt = d_tab[t(line, np.int64)].contiguous(), d_ext[t(line, np.int64)].contiguous(), t(np.full(rows, length)), t(flat)
    b_out = torch.empty(rows, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    base_ms = timed(h, h.lib.pqp_reference_length_device, (h._h, rows, m, p(b_tab), p(b_ext), p(b_len), p(b_tgt), p(b_out)), steps, warmup)
    behind = flags.reshape(-1)[pick] & capi.PROJ_NOT_FINITE == 0
    same = bool(np.array_equal(b_out.cpu().numpy()[behind], proj.reshape(-1, capi.PROJ_STRIDE)[pick][behind, 0]))
    med, base_med = float(np.median(ms)), float(np.median(base_ms))
    r = dict(lines=B, points_per_line=q, length_m=length, knots=m, us=med * 1e3, us_min=float(ms.min()) * 1e3, us_max=float(ms.max()) * 1e3,
             points_per_s=B * q / (med * 1e-3), baseline_rows=rows, baseline_us=base_med * 1e3, baseline_points_per_s=rows / (base_med * 1e-3),
             baseline_table_bytes=int(rows) * 9 * m * 8, s_identical_to_baseline=same,
             at_end=float((flags & capi.PROJ_AT_END != 0).mean()), not_converged=int((flags & capi.PROJ_NOT_CONVERGED != 0).sum()))
    r["ratio"] = r["points_per_s"] / r["baseline_points_per_s"]
    print(f"{B:5d} lines x {q:6d} points, {length:6.0f} m ({m} knots): {r['us']:9.1f} us/call (min {r['us_min']:.1f}, max {r['us_max']:.1f})  "
          f"{r['points_per_s'] / 1e6:8.1f} M points/s | one pqp_reference_length row per point ({rows} rows, {r['baseline_table_bytes'] / 2**20:.0f} MiB of tables): "
          f"{r['baseline_us']:9.1f} us  {r['baseline_points_per_s'] / 1e6:7.2f} M points/s | ratio {r['ratio']:.1f}  s identical: {same}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-bytes", type=int, default=1 << 30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_project: no GPU (a host run measures nothing here)")
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=80)
    rng = np.random.default_rng(0)
    out = [case(h, rng, B, q, length, args.steps, args.warmup, args.baseline_bytes) for B, q, length in SHAPES]
    h.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(dict(metric="project_points_per_s_1024x256_30m", value=out[0]["points_per_s"], ratio_to_reference_length=out[0]["ratio"],
                          points_per_s_64x16384_200m=out[1]["points_per_s"], points_per_s_1x262144_2km=out[2]["points_per_s"])))


if __name__ == "__main__":
    main()
