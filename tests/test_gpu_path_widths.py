"""The lane-per-waypoint path kernel at every workgroup width (NW = 1 / 2 / 4 / 8), certificate form and plain form, through the C ABI: the
cases of tests/width_cases.py against the C oracle, the KKT certificate, the lane-per-QP kernel and - count by count - the host emulation
(test_path_widths_cpu.py runs the same cases on the emulation alone).  A and C launch path_solve_kernel<NW, false> at four widths, B launches
path_solve_kernel<NW, true> at four widths.  Every handle keeps the lane-per-QP kernel off (PQP_OPT_STREAM_BATCH = 0) and every solve asserts
the kernel that served it.  Each test prints what it measured."""
import numpy as np
import pytest

import emu_util as EU
from emu_util import compare_counts as _compare
import pqp_oracle as O
import width_cases as W
from path_optimizer_2_amd import capi

pytestmark = pytest.mark.gpu


def say(capsys, text):
    with capsys.disabled():
        print("\n    " + text, end="")


def lane_handle(prm, batch, n, **options):
    h = capi.Handle(prm, device=0, max_batch=batch, max_n=n)
    h.set_option(capi.OPT_STREAM_BATCH, 0)
    for k, v in options.items():
        h.set_option(getattr(capi, k), v)
    return h


def lane_solve(h, b, counts=None, **kw):
    r = h.solve(b["ref"], b["bounds"], b["scal"], **kw) if counts is None else h.solve_var(counts, b["ref"], b["bounds"], b["scal"], **kw)
    assert h.last_path_kernel() == capi.KERNEL_LANE_PER_WAYPOINT
    return r


def per_qp_kernel(b, counts=None):
    """the same inputs through the lane-per-QP kernel: no iteration or factorisation shared with the kernel under test"""
    batch, n = b["ref"].shape[:2]
    h = capi.Handle(capi.production_params(), device=0, max_batch=batch, max_n=n)
    h.set_option(capi.OPT_STORE_WARM, 0); h.set_option(capi.OPT_STREAM_BATCH, 1)
    r = h.solve(b["ref"], b["bounds"], b["scal"], passes=1) if counts is None else h.solve_var(counts, b["ref"], b["bounds"], b["scal"], passes=1)
    assert h.last_path_kernel() == capi.KERNEL_LANE_PER_QP
    h.close()
    return r


def same_counts(dev, emu, what):
    _compare(dev, emu, what)
    assert np.array_equal(dev["iters"], emu["iters"]), (what, dev["iters"], emu["iters"])


def polished(r, passes, rows=slice(None)):
    return (r["status"][rows] == 1).all() and (r["info"][rows, 4] == passes + 1).all()


@pytest.mark.parametrize("n", W.EDGE_SIZES)
def test_width_edges(hip_lib, n, capsys):
    """A: the first and last waypoint count of every width, one pass then two on the same handle"""
    b = W.edge_batch(n)
    ora = W.cached(("edge", n), lambda: W.oracle(b))
    assert ora["solved"].all()
    h = lane_handle(capi.production_params(), 4, n)
    r0 = lane_solve(h, b, passes=0)
    x0, y0 = h.get_solution(4, n)
    r1 = lane_solve(h, b, passes=1)
    h.close()
    certs = [W.kkt(b, q, x0[q], y0[q]) for q in range(4)]
    worst = {k: max(c[k] for c in certs) for k in ("pri", "stat", "comp")}
    other = per_qp_kernel(b)
    d, d_other = W.off(r1["out"], ora["out"]).max(), W.off(r1["out"], other["out"]).max()
    say(capsys, f"A n = {n} (NW = {W.width_of(n)}): device - C oracle {d:.1e} (bar {W.bar(n):.0e}), - lane-per-QP kernel {d_other:.1e} (bar 1e-4); first pass KKT pri "
                f"{worst['pri']:.1e} stat {worst['stat']:.1e} comp {worst['comp']:.1e}")
    assert polished(r0, 0) and polished(r1, 1), (r0["status"], r0["info"][:, 4], r1["status"], r1["info"][:, 4])
    assert d < W.bar(n)
    assert worst["pri"] < W.KKT_PRI and worst["stat"] < W.KKT_STAT and worst["comp"] < W.KKT_COMP, worst
    same_counts(r0, W.emulate(EU.production(), b, passes=0), f"A {n} one pass")
    same_counts(r1, W.emulate(EU.production(), b, passes=1), f"A {n} two passes")
    assert (other["status"] == 1).all() and d_other < 1e-4


@pytest.mark.parametrize("n", W.CERT_SIZES)
def test_both_infeasibility_forms(hip_lib, n, capsys):
    """B: path_solve_kernel<NW, true> (default parameters: OSQP's certificate at every check) and the late form of the plain kernel on a QP whose
    start curvature lies outside its box, among three feasible neighbours"""
    b = W.cert_batch(n)
    prm = capi.default_params(hip_lib)
    assert prm.eps_prim_inf > 0 and prm.prim_inf_after == 0
    h = lane_handle(prm, 4, n)
    r = lane_solve(h, b, passes=1)
    h.close()
    assert list(r["status"]) == [1, 1, 4, 1]
    ref = W.cached(("cert-restatement", n), lambda: O.solve_path(b["ref"][2], b["bounds"][2], b["scal"][2]))
    assert [x["status"] for x in ref] == ["primal_infeasible"]
    want = W.cached(("cert-oracle", n), lambda: W.oracle_at(prm, b, [0, 1, 3]))
    d = W.off(r["out"][[0, 1, 3]], want).max()
    say(capsys, f"B n = {n} (NW = {W.width_of(n)}): certificate at iteration {r['iters'][2]} (restatement {ref[0]['iters']}), neighbours - C oracle at eps "
                f"{prm.eps_abs:g}: {d:.1e} (bar 1e-4)")
    assert r["iters"][2] == ref[0]["iters"]
    assert d < 1e-4
    h = lane_handle(capi.production_params(), 4, n)
    late = lane_solve(h, b, passes=1)
    h.close()
    assert list(late["status"]) == [1, 1, 4, 1] and polished(late, 1, [0, 1, 3])
    same_counts(late, W.emulate(EU.production(), b, passes=1), f"B {n} late form")
    feasible = {k: np.ascontiguousarray(v[[0, 1, 3]]) for k, v in b.items()}
    h = lane_handle(capi.production_params(), 3, n)
    alone = lane_solve(h, feasible, passes=1)
    h.close()
    assert np.array_equal(late["out"][[0, 1, 3]], alone["out"])


def _slot_reuse(capsys, what, b, counts, ora):
    """default geometry (a workgroup per QP from NW = 4 on), one CU (a workgroup draws 3 - 12 QPs in turn), one CU with the QPs ordered by cost
    (twice: the second launch reads the order array): bit for bit the same"""
    batch, n = b["ref"].shape[:2]
    everywhere = 1 << 20            # more CUs reserved than there are: the launcher keeps one
    runs = []
    for options, times in (({}, 1), (dict(OPT_RESERVE_CUS=everywhere), 1), (dict(OPT_RESERVE_CUS=everywhere, OPT_ORDER_BY_COST=1), 2)):
        h = lane_handle(capi.production_params(), batch, n, **options)
        runs += [lane_solve(h, b, counts, passes=1) for _ in range(times)]
        h.close()
    first = runs[0]
    real = slice(None) if counts is None else counts >= 2
    d = W.off(first["out"], ora["out"])[real].max()
    say(capsys, f"{what} n = {n} (NW = {W.width_of(n)}): device - C oracle {d:.1e} (bar {W.bar(n):.0e}); reduced solves {first['info'][:, 5].astype(int).tolist()}")
    for k, r in enumerate(runs[1:]):
        assert np.array_equal(r["status"], first["status"]), k
        assert np.array_equal(r["out"], first["out"]), (k, np.nonzero((r["out"] != first["out"]).any(axis=(1, 2)))[0])
        assert np.array_equal(r["iters"], first["iters"]) and np.array_equal(r["info"][:, 5:7], first["info"][:, 5:7]), k
    assert polished(first, 1, real) and d < W.bar(n)
    same_counts(first, W.emulate(EU.production(), b, passes=1, n_of=counts), what)
    return first


@pytest.mark.parametrize("n", W.REUSE_SIZES)
def test_slot_reuse(hip_lib, n, capsys):
    """C: a persistent workgroup that draws QP k + 1 after QP k inherits k's LDS, its save area and its parked scale vectors (global memory per
    slot at NW = 8)"""
    b = W.reuse_batch(n)
    ora = W.cached(("reuse", n), lambda: W.oracle(b))
    assert ora["solved"].all()
    _slot_reuse(capsys, "C", b, None, ora)


def _ragged_checks(r, counts, ora, emu, n_max, what):
    real = counts >= 2
    assert (r["status"][real] == 1).all() and (r["info"][real, 4] == 2).all(), (r["status"], r["info"][:, 4])
    same_counts(r, emu, what)
    assert W.off(r["out"], ora["out"])[real].max() < W.bar(n_max)
    for q, c in enumerate(counts):
        assert np.all(r["out"][q, max(c, 0):] == 0.0), q
        if c < 2:
            assert r["status"][q] == 0 and r["iters"][q] == 0 and not r["out"][q].any() and not r["info"][q].any(), q


def test_slot_reuse_with_ragged_counts(hip_lib, capsys):
    """C at n_max = 512: a 17-waypoint QP behind a 512-waypoint one in the same slot, a 300-waypoint one behind that
    (seed: width_cases.REUSE_RAGGED_SEED - on seed 30 the 65-waypoint QP's count hung on the last bit: 67 reduced solves here in all four launches,
    24 in the emulation, 22 in the emulation built with fused multiply-adds)"""
    b, counts = W.reuse_ragged_batch()
    ora = W.cached(("reuse-ragged",), lambda: W.oracle(b, counts))
    first = _slot_reuse(capsys, "C ragged", b, counts, ora)
    _ragged_checks(first, counts, ora, W.emulate(EU.production(), b, passes=1, n_of=counts), 512, "C ragged")


@pytest.mark.parametrize("name", list(W.RAGGED))
def test_ragged_counts_in_wide_workgroups(hip_lib, name, capsys):
    """D: pqp_path_solve_var where the width follows n_max: a 3-waypoint QP in a 512-lane workgroup has seven wavefronts without a real lane
    and runs with the intervals of n_max.
    The seeds are ones on which no QP's count hangs on the last bit (width_cases.unstable_counts): on seed 1 of "512a" the 257-waypoint QP took 64
    iterations / 122 reduced solves here and 128 / 208 in the emulation - 102 when the emulation is built with fused multiply-adds, 183 .. 632
    when its inputs move by 1e-15 .. 1e-13 - with the same status and path (1.9e-8 apart)."""
    b, counts = W.ragged_batch(name)
    n_max = b["ref"].shape[1]
    ora = W.cached(("ragged", name), lambda: W.oracle(b, counts))
    emu = W.emulate(EU.production(), b, passes=1, n_of=counts)
    assert len(W.ragged_condition(b, counts, emu, ora)) == 0
    h = lane_handle(capi.production_params(), len(counts), n_max)
    r = lane_solve(h, b, counts, passes=1)
    h.close()
    other = per_qp_kernel(b, counts)
    real = counts >= 2
    d, d_other = W.off(r["out"], ora["out"])[real].max(), W.off(r["out"], other["out"])[real].max()
    say(capsys, f"D {name} n_max = {n_max} (NW = {W.width_of(n_max)}), counts {counts.tolist()}: device - C oracle {d:.1e} (bar {W.bar(n_max):.0e}), - lane-per-QP "
                f"kernel {d_other:.1e} (bar 1e-4); iters {r['iters'].tolist()}")
    _ragged_checks(r, counts, ora, emu, n_max, f"D {name}")
    assert (other["status"][real] == 1).all() and d_other < 1e-4


@pytest.mark.parametrize("n", W.WARM_SIZES)
def test_warm_and_carried_solves(hip_lib, n, capsys):
    """E: the warm state of NW = 4 / 8 - the re-linearised warm solve against the second pass, then PQP_OPT_CARRY_CYCLES on the next cycle"""
    b = W.warm_batch(n)
    ora = W.cached(("warm", n), lambda: W.oracle(b))
    nxt = W.next_cycle(b)
    ora_next = W.cached(("warm-next", n), lambda: W.oracle(nxt))
    assert ora["solved"].all() and ora_next["solved"].all()
    h = lane_handle(capi.production_params(), 4, n)
    first = lane_solve(h, b, passes=0)
    second = lane_solve(h, b, passes=0, lin=np.ascontiguousarray(first["out"][:, :, 3:6]), warm=True)
    hf = lane_handle(capi.production_params(), 4, n)
    fused = lane_solve(hf, b, passes=1)
    cold = lane_solve(hf, nxt, passes=1)
    hf.close()
    h.set_option(capi.OPT_CARRY_CYCLES, 1)
    carried = lane_solve(h, nxt, passes=1)
    h.close()
    d_o, d_f, d_c = W.off(second["out"], ora["out"]).max(), W.off(second["out"], fused["out"]).max(), W.off(carried["out"], ora_next["out"]).max()
    say(capsys, f"E n = {n} (NW = {W.width_of(n)}): warm second pass - C oracle {d_o:.1e} (bar {W.bar(n):.0e}), - fused {d_f:.1e} (bar 1e-4); carried cycle - C oracle "
                f"{d_c:.1e}, reduced solves carried {int(carried['info'][:, 5].sum())} cold {int(cold['info'][:, 5].sum())}")
    assert (first["status"] == 1).all() and (second["status"] == 1).all() and (fused["status"] == 1).all()
    assert d_o < W.bar(n) and d_f < 1e-4
    assert (carried["status"] == 1).all() and d_c < W.bar(n)
    assert carried["info"][:, 5].sum() <= cold["info"][:, 5].sum()
