"""The width matrix (tests/width_cases.py) through the host emulation of the device source, against the independent references: the inputs the
GPU file (test_gpu_path_widths.py) runs are valid - solvable, polished, inside the bars - and stay so when synth.py or the algorithm change.
The emulation runs lanes one after the other and every QP on a fresh context: barriers, DPP rows, cross-wavefront reductions, register
allocation per width and a workgroup slot's second QP are the GPU file's business.  Every test prints what it measured.  Where the GPU file
compares counts with the emulation, the test here checks that they are counts the two can share (width_cases.unstable_counts)."""
import numpy as np
import pytest

import emu_util as EU
import pqp_oracle as O
import width_cases as W


def say(capsys, text):
    with capsys.disabled():
        print("\n    " + text, end="")


def polished(r, passes, rows=slice(None)):
    return (r["status"][rows] == 1).all() and (r["info"][rows, 4] == passes + 1).all()


@pytest.mark.parametrize("n", W.EDGE_SIZES)
def test_width_edges(n, capsys):
    """A: the first and last waypoint count of every workgroup width, one pass and two"""
    b = W.edge_batch(n)
    ora = W.cached(("edge", n), lambda: W.oracle(b))
    assert ora["solved"].all()
    e0 = W.emulate(EU.production(), b, passes=0)
    e1 = W.emulate(EU.production(), b, passes=1)
    assert polished(e0, 0) and polished(e1, 1), (e0["status"], e0["info"][:, 4], e1["status"], e1["info"][:, 4])
    certs = [W.kkt(b, q, *EU.to_reference_order(e0["wx"][q], e0["wy"][q], e0["wye"][q], n)) for q in range(4)]
    worst = {k: max(c[k] for c in certs) for k in ("pri", "stat", "comp")}
    d = W.off(e1["out"], ora["out"]).max()
    say(capsys, f"A n = {n} (NW = {W.width_of(n)}, seed {W.EDGE_SEED}): emulation - C oracle {d:.1e} (bar {W.bar(n):.0e}); first pass KKT pri {worst['pri']:.1e} "
                f"stat {worst['stat']:.1e} comp {worst['comp']:.1e}; iters {e1['iters'].tolist()}")
    assert d < W.bar(n)
    assert len(W.unstable_counts(EU.production(), b, e0, passes=0)) == 0 and len(W.unstable_counts(EU.production(), b, e1)) == 0
    assert worst["pri"] < W.KKT_PRI and worst["stat"] < W.KKT_STAT and worst["comp"] < W.KKT_COMP, worst


@pytest.mark.parametrize("n", W.CERT_SIZES)
def test_both_infeasibility_forms(n, capsys):
    """B: a start curvature outside its box among three feasible QPs, the certificate variant (default parameters) and the late form"""
    b = W.cert_batch(n)
    prm = EU.params()
    r = W.emulate(prm, b, passes=1)
    assert list(r["status"]) == [1, 1, 4, 1]
    ref = W.cached(("cert-restatement", n), lambda: O.solve_path(b["ref"][2], b["bounds"][2], b["scal"][2]))
    assert [x["status"] for x in ref] == ["primal_infeasible"] and r["iters"][2] == ref[0]["iters"]
    want = W.cached(("cert-oracle", n), lambda: W.oracle_at(prm, b, [0, 1, 3]))
    d = W.off(r["out"][[0, 1, 3]], want).max()
    late = W.emulate(EU.production(), b, passes=1)
    assert list(late["status"]) == [1, 1, 4, 1] and polished(late, 1, [0, 1, 3])
    say(capsys, f"B n = {n} (NW = {W.width_of(n)}): certificate at iteration {r['iters'][2]} (restatement {ref[0]['iters']}), neighbours - C oracle at "
                f"eps {prm.eps_abs:g}: {d:.1e} (bar 1e-4); late form iters {late['iters'].tolist()}")
    assert d < 1e-4
    assert len(W.unstable_counts(EU.production(), b, late)) == 0
    feasible = {k: np.ascontiguousarray(v[[0, 1, 3]]) for k, v in b.items()}
    alone = W.emulate(EU.production(), feasible, passes=1)
    assert np.array_equal(late["out"][[0, 1, 3]], alone["out"])


@pytest.mark.parametrize("n", W.REUSE_SIZES)
def test_slot_reuse_batches_are_solvable(n, capsys):
    """C: the twelve QPs a single workgroup slot draws in turn on the device"""
    b = W.reuse_batch(n)
    ora = W.cached(("reuse", n), lambda: W.oracle(b))
    assert ora["solved"].all()
    e = W.emulate(EU.production(), b, passes=1)
    d = W.off(e["out"], ora["out"]).max()
    say(capsys, f"C n = {n} (NW = {W.width_of(n)}): emulation - C oracle {d:.1e} (bar {W.bar(n):.0e}); reduced solves {e['info'][:, 5].astype(int).tolist()}")
    assert polished(e, 1) and d < W.bar(n)
    assert len(W.unstable_counts(EU.production(), b, e)) == 0


def _ragged(capsys, what, b, counts, ora, seed):
    n_max = b["ref"].shape[1]
    e = W.emulate(EU.production(), b, passes=1, n_of=counts)
    missing = W.ragged_condition(b, counts, e, ora)
    real = counts >= 2
    d = W.off(e["out"], ora["out"])
    say(capsys, f"{what} n_max = {n_max} (NW = {W.width_of(n_max)}, seed {seed}), counts {counts.tolist()}: emulation - C oracle {d[real].max():.1e} "
                f"(bar {W.bar(n_max):.0e}); iters {e['iters'].tolist()}")
    assert len(missing) == 0, (missing, counts[missing], e["status"][missing], e["info"][missing, 4], ora["solved"][missing])
    assert d[real].max() < W.bar(n_max)
    for q, c in enumerate(counts):
        assert np.all(e["out"][q, max(c, 0):] == 0.0)
        if c < 2:
            assert e["status"][q] == 0 and e["iters"][q] == 0 and not e["out"][q].any() and not e["info"][q].any()
    return e


@pytest.mark.parametrize("name", list(W.RAGGED))
def test_ragged_counts_in_wide_workgroups(name, capsys):
    """D: the condition on the chosen seeds (every QP of two and more waypoints is solved by the C oracle on its truncated scenario and polished
    in both passes by the emulation) and what the device test asserts, on the emulation"""
    b, counts = W.ragged_batch(name)
    ora = W.cached(("ragged", name), lambda: W.oracle(b, counts))
    _ragged(capsys, f"D {name}", b, counts, ora, W.RAGGED[name][2])


def test_ragged_cases_cover_the_count_set():
    for n_max in (129, 257, 512):
        have = set()
        for m, counts, _ in W.RAGGED.values():
            if m == n_max:
                have |= set(counts)
        assert have >= {c for c in W.RAGGED_COUNT_SET if c <= n_max} | {n_max, 1, 0}, (n_max, sorted(have))


def test_ragged_slot_reuse_batch_is_solvable(capsys):
    """C at n_max = 512 with counts of its own: a short QP behind a long one in the same slot and a long one behind a short one"""
    b, counts = W.reuse_ragged_batch()
    ora = W.cached(("reuse-ragged",), lambda: W.oracle(b, counts))
    _ragged(capsys, "C ragged", b, counts, ora, W.REUSE_RAGGED_SEED)


@pytest.mark.parametrize("n", W.WARM_SIZES)
def test_warm_and_carried_solves(n, capsys):
    """E: the re-linearised warm solve equals the fused second pass; a carried next cycle ends at the cold solve's optimum with no more work"""
    b = W.warm_batch(n)
    ora = W.cached(("warm", n), lambda: W.oracle(b))
    prm = EU.production()
    first = W.emulate(prm, b, passes=0)
    second = W.emulate(prm, b, passes=0, lin=first["out"][:, :, 3:6], warm_from=first)
    fused = W.emulate(prm, b, passes=1)
    assert polished(first, 0) and polished(second, 0) and polished(fused, 1)
    d_o, d_f = W.off(second["out"], ora["out"]).max(), W.off(second["out"], fused["out"]).max()
    nxt = W.next_cycle(b)
    ora_next = W.cached(("warm-next", n), lambda: W.oracle(nxt))
    assert ora["solved"].all() and ora_next["solved"].all()
    carried = W.emulate(prm, nxt, passes=1, warm_from=second)
    cold = W.emulate(prm, nxt, passes=1)
    d_c = W.off(carried["out"], ora_next["out"]).max()
    say(capsys, f"E n = {n} (NW = {W.width_of(n)}): warm second pass - C oracle {d_o:.1e} (bar {W.bar(n):.0e}), - fused {d_f:.1e} (bar 1e-4); carried cycle - C oracle "
                f"{d_c:.1e}, reduced solves carried {int(carried['info'][:, 5].sum())} cold {int(cold['info'][:, 5].sum())}")
    assert d_o < W.bar(n) and d_f < 1e-4
    assert (carried["status"] == 1).all() and d_c < W.bar(n)
    assert carried["info"][:, 5].sum() <= cold["info"][:, 5].sum()
