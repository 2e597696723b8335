"""pqp_speed_refine on the GPU where the banded core's direct active-set attempt is rejected: equilibration with pbw = 3, ADMM, periodic
polish attempts, eps_scale, the infeasibility certificate and max_iter - the part of pqp_banded_qp.hpp that only the refine runs on the
device (a smoother handle with polish = 1 goes to the exact kernels).  The cases are refine_util's families "params", "staircases",
"threshold" and the form edges; tests/test_speed_refine_fallback.py checks every one of them on the host emulation against HiGHS first
and measures the bounds used here: no number in this file comes from a device.

Held to HiGHS's verdict: REFINED with status SOLVED where it says Optimal, kept with the search's rows where it says Infeasible
(PRIMAL_INFEASIBLE with the INFEASIBLE flag, or MAX_ITER without it - include/pqp.h documents both).  A refined path: `bounds` and - at
the device's own s - the rows and the excess bit for bit the restatement's, the KKT certificate of its (s, v, a) with recovered
multipliers within 4 x the same certificate of what the call returns for the emulation's solution (refine_util.KKT_RETURNED_FALLBACK:
the rows hold the solver's x after the clamps of the definition, and that is what is certified on both sides), every variable within
2 x HIGHS_DIST_FALLBACK of HiGHS, the cost within 1e-6 relative.  Host form
and device form (sentinel-filled outputs) agree bit for bit.  Per kernel form at least one refined path comes back with iters > 0.

The four "threshold" members within 1e-5 of the feasibility edge get the safety properties only.
The MAX_ITER cases (w_jerk = 50, d_max = 0.5, window = 1, paths 0 and 1 from m = 85 on): test_params_and_form_edges prints what the device
ends them with; either PRIMAL_INFEASIBLE or MAX_ITER passes.

On one MI355X (profiles/r21a_pytest_speed_refine_fallback.log): every verdict is HiGHS's and every refined path is safe; per form the
device refines 10 / 7 / 11 / 10 paths with iters > 0, the emulation's counts, and the first run of <3,512,false> with pbw = 3 agrees
with its staged neighbour; all nine MAX_ITER cases end MAX_ITER after 1000 iterations on the device too (flags KEPT alone); the
threshold members at -1e-5 / +1e-5 / -1e-7 / +1e-7 come back kept (PRIMAL_INFEASIBLE, 608 iterations) / refined / refined / refined,
primal violation at most 8.3e-8.  Worst figures on the device: stationarity 3.48e-6 (bound 1.4e-5), primal violation 1.53e-7 (6.4e-7),
complementarity 5.49e-5 (2.2e-4), distance to HiGHS 4.66e-6 (9.4e-6) - to three digits the emulation's own.  The stationarity is the
clamp's doing, not the solver's: stairs_w1_j50 path 3 (solved directly on both sides) has 4.0e-10 at the solver's x and 3.48e-6 once
a[m - 1], which the polish leaves 5.9e-8 off its bound, is set to 0 - the jerk term's Hessian entry is 100 under w_jerk = 50."""
import ctypes as C
import math

import numpy as np
import pytest

import device_form as D
import refine_util as R
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
KEYS = ("traj", "bounds", "cost", "excess", "status", "iters", "flags")
KKT_BOUND = {k: 4.0 * v for k, v in R.KKT_RETURNED_FALLBACK.items()}
DIST_BOUND = 2.0 * R.HIGHS_DIST_FALLBACK


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _prm(prm, window):
    return capi.refine_default_params(w_ref=prm[R.W_REF], w_accel=prm[R.W_ACCEL], w_jerk=prm[R.W_JERK], a_max=prm[R.A_MAX], d_max=prm[R.D_MAX], window=window)


def _host(handle, c, res, prm, window, pick=None):
    sel = (lambda a: a) if pick is None else (lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[pick]))
    return handle.speed_refine(sel(c["paths"]), sel(c["profile"]), sel(c["v_start"]), sel(res["blocked"]), sel(res["steps"]), sel(res["reached"]),
                               sel(res["traj"]), n_of=sel(c.get("n_of")), stop_before=sel(c.get("stop_before")),
                               grid=capi.search_default_params(**c["prm"]), prm=_prm(prm, window))


def _device(handle, c, res, prm, window):
    paths, profile = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("paths", "profile"))
    B, n, stride = paths.shape
    m = res["traj"].shape[1]
    p = _prm(prm, window)
    opt = lambda k: None if c.get(k) is None else D.to_device(c[k], np.int32)
    out = dict(traj=D.Out((B, m, 8)), bounds=D.Out((B, m, 3)), cost=D.Out((B,)), excess=D.Out((B,)), status=D.Out((B,), np.int32),
               iters=D.Out((B,), np.int32), flags=D.Out((B,), np.int32))
    rc = D.call(handle, "pqp_speed_refine_device", C.byref(capi.search_default_params(**c["prm"])), p.array(), int(p.window), B, n, stride,
                D.to_device(paths), opt("n_of"), opt("stop_before"), D.to_device(profile), D.to_device(c["v_start"]), m,
                D.to_device(res["blocked"], np.int32), D.to_device(res["steps"], np.int32), D.to_device(res["reached"], np.int32), D.to_device(res["traj"]),
                out["traj"], out["bounds"], out["cost"], out["excess"], out["status"], out["iters"], out["flags"])
    assert rc == 0, handle.lib.pqp_last_error()
    return {k: v.get() for k, v in out.items()}


def _safe(where, got, b, su, m):
    """a REFINED path lies inside its corridor and meets the restated QP's rows within the primal bound"""
    rows = got["traj"][b]
    s, v, a = rows[:, 4], rows[:, 5], rows[:, 6]
    assert got["status"][b] == R.SOLVED, (where, b, got["status"][b])
    assert (s >= su["bounds"][:, 0]).all() and (s <= su["bounds"][:, 1]).all() and (v >= 0.0).all() and a[m - 1] == 0.0, (where, b)
    P, q, A, lo, up = su["qp"]
    z = A @ np.concatenate([s, v, a])
    primal = float(np.maximum(np.maximum(lo - z, z - up), 0.0).max())
    assert primal <= KKT_BOUND["primal"], (where, b, primal)
    return primal


def _check_path(where, got, b, one, c, m, prm, worst):
    """one path of a call against HiGHS's verdict; -> "refined" / "kept" """
    su, dt = one["su"], c["prm"]["dt"]
    rows = got["traj"][b]
    if one["highs"] == "Optimal":
        assert got["flags"][b] == R.REFINED and got["status"][b] == R.SOLVED, (where, b, "kept where HiGHS has an optimum", got["flags"][b], got["status"][b])
        _safe(where, got, b, su, m)
        assert same_bits(got["bounds"][b], su["bounds"]), (where, b)
        assert same_bits(rows[:, 7], np.arange(m).astype(np.float64) * np.float64(dt)), (where, b)
        x = np.concatenate([rows[:, 4], rows[:, 5], rows[:, 6]])
        P, q, A, lo, up = su["qp"]
        cert = R.certificate(P, q, A, lo, up, x)
        d = float(np.abs(x - one["xh"]).max())
        print(f"{where} path {b}: m = {m}, iters {got['iters'][b]} (emulation {one['emu']['iters']}), " + ", ".join(f"{k} {val:.2e}" for k, val in cert.items()) +
              f", to HiGHS {d:.2e}, to the emulation {np.abs(x - one['xe']).max():.2e}")
        for k in cert:
            worst[k] = max(worst.get(k, 0.0), cert[k])
        worst["dist"] = max(worst.get("dist", 0.0), d)
        for k in cert:
            assert cert[k] <= KKT_BOUND[k], (where, b, k, cert[k], KKT_BOUND[k])
        assert d <= DIST_BOUND, (where, b, d, DIST_BOUND)
        fin = R.finish(c["paths"][b], c["profile"][b], su, one["found"], x, R.SOLVED, dt)
        assert same_bits(fin["traj"], rows) and same_bits(fin["excess"], got["excess"][b]), (where, b)
        want = R.objective(x, su["sigma"], dt, prm)
        assert abs(got["cost"][b] - want) <= 1e-6 * max(1.0, abs(want)), (where, b, got["cost"][b], want)
        return "refined"
    assert one["highs"] == "Infeasible", (where, b, one["highs"])
    assert got["flags"][b] & R.REFINED == 0 and got["flags"][b] & R.KEPT, (where, b, "REFINED where HiGHS says infeasible", got["flags"][b])
    assert got["status"][b] in (R.PRIMAL_INFEASIBLE, R.MAX_ITER), (where, b, got["status"][b])
    assert got["flags"][b] == R.KEPT | (R.INFEASIBLE if got["status"][b] == R.PRIMAL_INFEASIBLE else 0), (where, b, got["flags"][b], got["status"][b])
    assert same_bits(rows, one["found"]["traj"]) and (got["bounds"][b] == 0.0).all() and math.isnan(got["cost"][b]) and math.isnan(got["excess"][b]), (where, b)
    if one["emu"]["status"] == R.MAX_ITER:
        print(f"{where} path {b}: the emulation ends at MAX_ITER after {one['emu']['iters']} iterations; the device: status {got['status'][b]} after {got['iters'][b]}, "
              f"flags {got['flags'][b]}")
    return "kept"


def _check_call(handle, name, prm, window, worst):
    """one call through both forms -> [(emulation's class, the device's iters, "refined" / "kept")] per path"""
    r = R.reference(name, prm=prm, window=window)
    c, res, m = r["case"], r["res"], r["m"]
    where = f"{name} {tuple(prm)} window {window}"
    got = _host(handle, c, res, prm, window)
    dev = _device(handle, c, res, prm, window)
    for k in KEYS:
        assert same_bits(np.asarray(dev[k], dtype=np.float64), np.asarray(got[k], dtype=np.float64)), (where, k)
    return [(R.verdict_class(one), int(got["iters"][b]), _check_path(where, got, b, one, c, m, prm, worst)) for b, one in enumerate(r["each"])]


def _report(what, worst):
    print(f"{what}: worst on the device " + ", ".join(f"{k} {worst.get(k, 0.0):.2e} (bound {KKT_BOUND[k]:.2e})" for k in KKT_BOUND) +
          f", distance to HiGHS {worst.get('dist', 0.0):.2e} (bound {DIST_BOUND:.2e})")


# ---- "params" and the form edges, kernel form by kernel form --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f for _, _, f in R.FORM_RANGES], ids=lambda f: "B%dx%d%s" % (f[0], f[1], "s" if f[2] else "g"))
def test_params_and_form_edges(handle, form):
    """every call of "params" whose m selects this form, and the form's edges under the default parameters and under the heavy jerk weight:
    the checks of the module docstring, and the fallback really ran - a refined path with iters > 0.  (3, 512, false) with pbw = 3 runs
    nowhere else on the device"""
    default = (tuple(R.DEFAULT_PRM.tolist()), R.DEFAULT_WINDOW)
    calls = [call for call in R.PARAMS if R.form_of_case(call[0]) == form]
    calls += [("m%d" % m,) + combo for m in R.EDGE_M if R.form_of_layers(m) == form for combo in (default, R.JERKY) if ("m%d" % m,) + combo not in calls]
    worst, emu_after, dev_after, seen_max_iter = {}, 0, 0, 0
    for name, prm, window in calls:
        for cls, iters, what in _check_call(handle, name, prm, window, worst):
            emu_after += cls == "fallback"
            dev_after += what == "refined" and iters > 0
            seen_max_iter += cls == "max_iter"
    print(f"form {form}: {len(calls)} calls; refined after the fallback: the emulation {emu_after} paths, the device {dev_after}; {seen_max_iter} paths the emulation "
          "leaves at MAX_ITER")
    _report(f"form {form}", worst)
    assert dev_after >= 1, (form, "no refined path with iters > 0")


# ---- "staircases" ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.STAIRCASES))
def test_staircases_in_one_call(handle, name):
    """a batch of different QPs judged on the device as they are: fallbacks, infeasible ones and directly solved ones side by side"""
    _, prm, window = next(call for call in R.STAIR_CALLS if call[0] == name)
    worst = {}
    got = _check_call(handle, name, prm, window, worst)
    print(f"{name}: the emulation's classes {[g[0] for g in got]}; the device's iters {[g[1] for g in got]}")
    _report(name, worst)


@pytest.mark.parametrize("name,want", (("stairs_w1_j1", "infeasible"), ("stairs_w2_j0", "max_iter")))
def test_a_fallback_and_a_kept_path_between_direct_neighbours(handle, name, want):
    """a path the fallback solves and one without a feasible point, each between directly solved neighbours in a longer batch: every
    path's outputs are bit for bit its outputs alone"""
    _, prm, window = next(call for call in R.STAIR_CALLS if call[0] == name)
    r = R.reference(name, prm=prm, window=window)
    c, res = r["case"], r["res"]
    cls = [R.verdict_class(one) for one in r["each"]]
    direct = [b for b, k in enumerate(cls) if k == "direct"]
    order = np.array([direct[0], cls.index("fallback"), direct[1], cls.index(want), direct[2], direct[0], cls.index("fallback"), direct[3]])
    got = _host(handle, c, res, prm, window, pick=order)
    for at, b in enumerate(order):
        alone = _host(handle, c, res, prm, window, pick=np.array([b]))
        for k in KEYS:
            assert same_bits(np.asarray(got[k][at], dtype=np.float64), np.asarray(alone[k][0], dtype=np.float64)), (name, at, b, k)
    assert got["flags"][1] == R.REFINED == got["flags"][6] and got["iters"][1] > 0 and got["flags"][3] & R.KEPT, (got["flags"], got["iters"])
    assert (got["flags"][[0, 2, 4, 5, 7]] == R.REFINED).all()


# ---- "threshold" ---------------------------------------------------------------------------------------------------------------------------------
def test_around_the_feasibility_threshold(handle):
    """the hand case "quick" with a_max at its feasibility edge times 1 +- {1e-2, 1e-3, 1e-5, 1e-7}: the first two pairs follow HiGHS, the
    closer ones may fall either way - whatever is REFINED is safe"""
    worst = {}
    for call in R.THRESHOLD_FOLLOWS:
        assert [g[2] for g in _check_call(handle, *call, worst)] == ["refined" if call[1][R.A_MAX] > R.THRESHOLD_A_MAX else "kept"]
    _report("threshold", worst)
    for name, prm, window in R.THRESHOLD_LEFT_OUT:
        r = R.reference(name, prm=prm, window=window)
        c, res, m = r["case"], r["res"], r["m"]
        got = _host(handle, c, res, prm, window)
        one = r["each"][0]
        line = f"a_max / edge - 1 = {prm[R.A_MAX] / R.THRESHOLD_A_MAX - 1.0:+.0e}: HiGHS {one['highs']}, the emulation {R.verdict_class(one)}, the device flags {got['flags'][0]} status {got['status'][0]} iters {got['iters'][0]}"
        if got["flags"][0] == R.REFINED:
            line += f", primal violation {_safe(name, got, 0, one['su'], m):.2e} (bound {KKT_BOUND['primal']:.2e})"
        else:
            assert got["flags"][0] & R.KEPT and same_bits(got["traj"][0], res["traj"][0]) and got["status"][0] in (R.PRIMAL_INFEASIBLE, R.MAX_ITER), got["flags"]
        print(line)
