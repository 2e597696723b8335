"""The speed refine's QPs that the banded core does not solve by its direct active-set attempt, without a GPU: the case families of
tests/refine_util.py ("params", "staircases", "threshold" and the form edges) through the core's host emulation under production
parameters with the polish on, against HiGHS.  After a rejected direct attempt the core equilibrates (Ruiz, pbw = 3), runs ADMM with
periodic polish attempts, tightens eps_scale and may end with the primal-infeasibility certificate or at max_iter - the refine is the
only caller that runs this on the device, and tests/test_gpu_speed_refine_fallback.py holds the device to what is measured here.

Measured here (test_the_emulation_agrees_with_highs_on_every_family prints them) over the 173 solved QPs of the three families and the
form edges (32 + 32 + 2 + 6 of them solved after the fallback, iters 8 .. 56):
  the emulation's worst KKT residuals on the restatement's matrices, with its own multipliers:
      stationarity 9.94e-8, primal violation 8.61e-8, complementarity 3.01e-5            -> refine_util.KKT_WORST_FALLBACK
  with multipliers recovered from x alone (refine_util.certificate):
      stationarity 6.17e-8, primal violation 8.61e-8, complementarity 3.01e-5            -> refine_util.KKT_RECOVERED_FALLBACK
      (the complementarity is the same either way: it is not the certificate's active_tol that makes it a hundred times what the
       directly solved cases of tests/test_speed_refine.py show, but a multiplier times what an active row is left off its bound)
  of what the call returns for that x (refine_util.finished_x: s clamped into its corridor, v to 0, a[m - 1] = 0), recovered multipliers:
      stationarity 3.48e-6, primal violation 1.53e-7, complementarity 5.49e-5            -> refine_util.KKT_RETURNED_FALLBACK
      (the clamps move a variable by what the polish leaves an active row off its bound, up to 6e-8; the jerk term's Hessian entries
       of 2 w_jerk / dt^2 = 100 under w_jerk = 50 make 3.48e-6 of it on "stairs_w1_j50" path 3, which has 4.0e-10 before the clamp.
       The GPU test certifies the returned rows, so this is the figure it holds the device to)
  its worst distance to HiGHS in any variable: 4.66e-6                                   -> refine_util.HIGHS_DIST_FALLBACK
The emulation leaves "m85" .. "m193" paths 0 and 1 under w_jerk = 50, d_max = 0.5, window = 1 at PQP_STATUS_MAX_ITER after 1000
iterations where HiGHS says "Infeasible" (include/pqp.h documents that outcome), and one staircase as well.  Of the four "threshold"
members left out of the verdict comparison one differs: at a_max = edge x (1 - 1e-7) the emulation solves directly what HiGHS calls
infeasible (the rows are met to the polish's tolerance)."""
import numpy as np
import pytest

import banded_cases as BC
import refine_util as R

FORMS = tuple(f for _, _, f in R.FORM_RANGES)


def test_the_form_table_of_the_refines_shape():
    """every edge of the table, and the capacity: m = 194 does not fit"""
    for first, last, form in R.FORM_RANGES:
        assert R.form_of_layers(first) == form == R.form_of_layers(last), (first, last, form)
    assert [R.form_of_layers(m) for m in (85, 86, 130, 131, 170, 171, 193, 194)] == \
        [(3, 256, 1), (3, 512, 1), (3, 512, 1), (3, 512, 0), (3, 512, 0), (3, 1024, 0), (3, 1024, 0), None]
    assert all(a[1] + 1 == b[0] for a, b in zip(R.FORM_RANGES, R.FORM_RANGES[1:])) and R.FORM_RANGES[-1][1] == R.CAPACITY_M
    assert R.FIRST_PLAIN_M == next(first for first, _, form in R.FORM_RANGES if form[2] == 0)
    for m in (2, 3, 8, 85, 86, 130, 131, 170, 171, 193, 194):
        sh = R.refine_shape(m)
        assert R.layout_doubles(m) == BC.layout(sh["nv"], sh["nc"], sh["bw"])["plain"], m
    assert set(R.EDGE_M) == {m for a, b in zip(R.FORM_RANGES, R.FORM_RANGES[1:]) for m in (a[1], b[0])}


def test_the_staircases_are_what_a_search_could_have_written():
    """steps within the path, |dq| <= 2, j the running sum, rows the search's; the setup refines every one of them"""
    for name, (m, seed, count, keep, prm, window) in R.STAIRCASES.items():
        c, res, m_ = R.searched(name)
        assert m_ == m and len(c["paths"]) == len(keep) <= 64 and sorted(set(keep)) == list(keep), name
        j, q = res["steps"][:, :, 0].astype(np.int64), res["steps"][:, :, 1].astype(np.int64)
        assert (j[:, 0] == 0).all() and (np.diff(j, axis=1) == q[:, :-1]).all() and (np.abs(np.diff(q, axis=1)) <= 2).all() and q.min() >= 0 and q.max() <= 6
        assert (res["blocked"] == 0).all() and (res["reached"] == m).all()
        assert np.array_equal(res["traj"][:, :, 4], j * c["prm"]["ds"]) and np.array_equal(res["traj"][:, :, 5], q * c["prm"]["ds"] / c["prm"]["dt"])
        assert (np.abs(c["v_start"] - res["traj"][:, 0, 5]) <= 0.2).all() and (c["v_start"] >= 0.0).all()
        r = R.reference(name, highs=False, prm=prm, window=window)
        assert not any(one["su"]["kept"] for one in r["each"]) and all(one["su"]["J"] > j.max() for one in r["each"]), name
    assert {(v[5], v[4][R.W_JERK]) for v in R.STAIRCASES.values()} == {(w, wj) for w in (1, 2, 4) for wj in (0.0, 1.0, 50.0)}
    assert {v[0] for v in R.STAIRCASES.values()} == {8, 12}


def _calls():
    """(family, case, prm, window) of every call of the families and the form edges"""
    edges = [("edges", "m%d" % m, combo[0], combo[1]) for m in R.EDGE_M for combo in ((tuple(R.DEFAULT_PRM.tolist()), R.DEFAULT_WINDOW), R.JERKY)]
    return [("params",) + call for call in R.PARAMS] + [("staircases",) + call for call in R.STAIR_CALLS] + \
           [("threshold",) + call for call in R.THRESHOLD] + edges


def test_the_emulation_agrees_with_highs_on_every_family():
    """every QP of the families: SOLVED <-> Optimal, PRIMAL_INFEASIBLE or MAX_ITER <-> Infeasible - but for the four "threshold" members
    within 1e-5 of the edge; the staged and the non-staged form of the emulation agree in status and iterations wherever the device runs
    a non-staged one; the class counts that the families were chosen for; and the figures of the module docstring"""
    zero = dict(stationarity=0.0, primal=0.0, complementarity=0.0)
    own, rec, fin, dist = dict(zero), dict(zero), dict(zero), 0.0
    counts = {fam: {} for fam in ("params", "staircases", "threshold", "edges")}
    per_form = {f: dict(direct=0, fallback=0, infeasible=0, max_iter=0) for f in FORMS}
    left_out, solved, seen = 0, 0, set()
    for fam, name, prm, window in _calls():
        r = R.reference(name, prm=prm, window=window)
        m, dt = r["m"], r["case"]["prm"]["dt"]
        for b, one in enumerate(r["each"]):
            assert not one["su"]["kept"], (name, b)
            cls = R.verdict_class(one)
            key = (name, tuple(prm), window, b)
            if key not in seen:                              # (a form edge under JERKY may be a call of "params" as well: counted once)
                counts[fam][cls] = counts[fam].get(cls, 0) + 1
                per_form[R.form_of_layers(m)][cls] += fam in ("params", "edges")
            if one["plain"] is not None:
                assert (one["plain"]["status"], one["plain"]["iters"]) == (one["emu"]["status"], one["emu"]["iters"]), (name, prm, window, b)
            assert (one["plain"] is not None) == (m >= R.FIRST_PLAIN_M)
            if (name, prm, window) in R.THRESHOLD_LEFT_OUT:
                left_out += key not in seen
                print(f"threshold a_max / edge - 1 = {prm[R.A_MAX] / R.THRESHOLD_A_MAX - 1.0:+.0e}: the emulation {cls}, iters {one['emu']['iters']}; HiGHS {one['highs']}")
            else:
                want = "Optimal" if cls in ("direct", "fallback") else "Infeasible"
                assert one["highs"] == want, (fam, name, prm, window, b, cls, one["emu"]["iters"], one["highs"])
            if cls in ("infeasible", "max_iter") or key in seen:
                seen.add(key)
                continue
            seen.add(key)
            P, q, A, lo, up = one["su"]["qp"]
            c_own, c_rec = R.certificate(P, q, A, lo, up, one["xe"], one["emu"]["y"]), R.certificate(P, q, A, lo, up, one["xe"])
            # what the call returns is not x but finish()'s clamps of it: the GPU test certifies that, so it is measured as well
            c_fin = R.certificate(P, q, A, lo, up, R.finished_x(one["su"], one["xe"]))
            own, rec, fin = ({k: max(w[k], c[k]) for k in w} for w, c in ((own, c_own), (rec, c_rec), (fin, c_fin)))
            solved += 1
            line = f"{fam} {name} {prm} window {window} path {b}: m = {m}, {cls} iters {one['emu']['iters']}, own " + \
                   ", ".join(f"{k} {v:.2e}" for k, v in c_own.items()) + "; recovered " + ", ".join(f"{k} {v:.2e}" for k, v in c_rec.items()) + \
                   "; as returned " + ", ".join(f"{k} {v:.2e}" for k, v in c_fin.items())
            if one["highs"] == "Optimal":
                d = float(np.abs(one["xe"] - one["xh"]).max())
                dist = max(dist, d)
                ours, theirs = (R.objective(x, one["su"]["sigma"], dt, prm) for x in (one["xe"], one["xh"]))
                # two points that meet the rows to `primal` and to HiGHS's 100 x HIGHS_TOL differ in cost by the multipliers times that much
                slack = float(np.abs(one["emu"]["y"]).sum()) * (c_own["primal"] + 100.0 * R.HIGHS_TOL)
                assert abs(ours - theirs) < 1e-6 * max(1.0, abs(theirs)) + slack, (fam, name, prm, window, b, ours, theirs, slack)
                line += f"; distance to HiGHS {d:.2e}, cost {ours:.9g} against {theirs:.9g}"
            print(line)
    print("worst, own multipliers:", ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    print("worst, recovered multipliers:", ", ".join(f"{k} {v:.2e}" for k, v in rec.items()))
    print("worst, as returned (clamped), recovered multipliers:", ", ".join(f"{k} {v:.2e}" for k, v in fin.items()))
    print(f"worst distance to HiGHS {dist:.2e}; {solved} solved QPs; classes {counts}; per form {per_form}")
    # the conditions the families were chosen for
    assert left_out == 4 == len(R.THRESHOLD_LEFT_OUT) and len(R.THRESHOLD) == 8
    for f in FORMS:
        assert per_form[f]["fallback"] >= 2 and per_form[f]["direct"] >= 2 and per_form[f]["infeasible"] + per_form[f]["max_iter"] >= 1, (f, per_form[f])
    assert counts["params"].get("max_iter", 0) >= 1
    stairs = counts["staircases"]
    assert stairs.get("fallback", 0) >= 8 and stairs.get("direct", 0) >= 8 and stairs.get("infeasible", 0) + stairs.get("max_iter", 0) >= 8, stairs
    combos = {call[1] for call in R.PARAMS}
    assert any(p[R.W_REF] != 1.0 for p in combos) and any(p[R.W_ACCEL] != 1.0 for p in combos) and any(p[R.W_JERK] == 0.0 for p in combos)
    # the stated figures are the measured ones
    assert solved == R.FIGURES_QPS
    for k in own:
        assert 0.5 * R.KKT_WORST_FALLBACK[k] <= own[k] <= R.KKT_WORST_FALLBACK[k], (k, own[k])
        assert 0.5 * R.KKT_RECOVERED_FALLBACK[k] <= rec[k] <= R.KKT_RECOVERED_FALLBACK[k], (k, rec[k])
        assert 0.5 * R.KKT_RETURNED_FALLBACK[k] <= fin[k] <= R.KKT_RETURNED_FALLBACK[k], (k, fin[k])
    assert 0.5 * R.HIGHS_DIST_FALLBACK <= dist <= R.HIGHS_DIST_FALLBACK, dist


def test_the_threshold_is_highs_edge():
    """the stored edge separates HiGHS's verdicts at the two nearest members that follow it, and lies between 1.001 and 1.01 times
    7 / 4.5 (a_max = 14 / 9 reaches the corridor's 7 m after three layers from rest; the jerk term and the later layers ask a little more)"""
    assert 1.001 * 7 / 4.5 < R.THRESHOLD_A_MAX < 1.01 * 7 / 4.5
    verdicts = {call[1][R.A_MAX] > R.THRESHOLD_A_MAX: R.reference(*call[:1], prm=call[1], window=call[2])["each"][0]["highs"]
                for call in R.THRESHOLD_FOLLOWS if abs(abs(call[1][R.A_MAX] / R.THRESHOLD_A_MAX - 1.0) - 1e-3) < 1e-9}
    assert verdicts == {False: "Infeasible", True: "Optimal"}
