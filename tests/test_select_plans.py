"""pqp_select_plans without a GPU: the symbols and the binding, the enumerators, the prototypes in a C file, the refusals, the chain
wrapper's argument checks, the C++ wrapper's build, the kernels' resources - and the numpy restatement the GPU tests compare the kernels
against (tests/rank_util.py): its whole-array form against the plain loop, the properties the definition promises, and the hand case
the call exists for: the straighter path that waits behind a pedestrian and its curvier neighbour that passes.

The hand case's figures (test_the_straighter_path_waits_and_the_curvier_one_wins prints them), on the search's rows: A's score is -12.25
(progress 15.5 m, effort 2.5, jumps 0.75, path 0), B's -14.452725 (progress 19.5 m, effort 3.5, jumps 1, lateral 0.219275, path 0.328):
B wins by 2.2, 15 % of |score|.  Without the progress term A wins, 3.25 against 5.047275."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import agents_util as A
import build_util
import cpp_demo
import plan_util as P
import rank_util as K
import refine_util as R
import search_util as S
import select_util
from path_optimizer_2_amd import capi
from shared_util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_select_plans", "pqp_select_plans_device")


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_rank_default_params",):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert len(hip_lib.pqp_select_plans_device.argtypes) == 24 == len(hip_lib.pqp_select_plans.argtypes)
    assert hip_lib.pqp_select_plans.argtypes[2:6] == [C.c_int] * 4                 # require_free by value beside the plain doubles: no new struct
    assert list(inspect.signature(capi.Handle.select_plans).parameters) == ["self", "traj", "group_start", "m_of", "path_terms", "search_flags",
                                                                            "first_hit", "clearance", "paths", "n_of", "prm"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        prm = inspect.signature(fn).parameters
        assert prm["rank"].default is None and prm["rank_params"].default is None
        assert list(prm)[-5:] == ["rank", "rank_params", "speed", "v_start", "v_end"]       # the last before the three tests/test_speed_profile.py pins at the end
    d = capi.rank_default_params(hip_lib)
    assert d.array().tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, capi.select_default_params(hip_lib).clearance_want] == K.Params().array().tolist()
    assert d.require_free == 1 == K.Params().require_free and d.clearance_want == 0.6
    assert capi.rank_default_params(hip_lib, w_progress=0.0, require_free=0).array()[capi.RANK_W_PROGRESS] == 0.0
    hip_lib.pqp_rank_default_params(None, None)                                    # a NULL pointer is ignored


def test_the_enumerators_equal_the_header():
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    stated = {k: int(v) for k, v in re.findall(r"(PQP_RANK_[A-Z_]+) = (\d+)", txt)}
    assert stated == dict(PQP_RANK_W_PATH=K.W_PATH, PQP_RANK_W_PROGRESS=K.W_PROGRESS, PQP_RANK_W_ACCEL=K.W_ACCEL, PQP_RANK_W_JUMP=K.W_JUMP,
                          PQP_RANK_W_LATERAL=K.W_LATERAL, PQP_RANK_W_CLEARANCE=K.W_CLEARANCE, PQP_RANK_CLEARANCE_WANT=K.CLEARANCE_WANT)
    assert all(getattr(capi, k[4:]) == v for k, v in stated.items())
    defines = {k: int(v) for k, v in re.findall(r"#define (PQP_PLAN_SCORE_STRIDE|PQP_RANK_PARAMS) (\d+)", txt)}
    assert defines == dict(PQP_PLAN_SCORE_STRIDE=10, PQP_RANK_PARAMS=7)
    assert (capi.PLAN_SCORE_STRIDE, capi.RANK_PARAMS) == (K.PLAN_SCORE_STRIDE, K.RANK_PARAMS) == (10, 7)
    assert (K.NO_PLAN, K.EMPTY, K.NOT_FINITE) == (capi.SEARCH_NO_PLAN, capi.SEARCH_EMPTY, capi.SEARCH_NOT_FINITE)
    assert len(capi.HEADER.structs) == 10 and list(capi.HEADER.included) == ["pqp_search_params"]      # no new struct anywhere


def test_a_c_file_compiles_the_prototypes(tmp_path):
    args = ("pqp_handle*, const double*, int, int, int, int, const double*, const int32_t*, const double*, const int32_t*, const int32_t*,\n"
            "    const double*, int, int, const double*, const int32_t*, int, const int32_t*, double*, int32_t*, double*, int32_t*, double*, int32_t*")
    src = ('#include "pqp.h"\n'
           f"int (*device_form)({args}) = pqp_select_plans_device;\n"
           f"int (*host_form)({args}) = pqp_select_plans;\n"
           "void (*defaults)(double*, int*) = pqp_rank_default_params;\n"
           "double prm[PQP_RANK_PARAMS];\n"
           "double record[PQP_PLAN_SCORE_STRIDE];\n"
           "int last = PQP_RANK_W_PATH + PQP_RANK_W_PROGRESS + PQP_RANK_W_ACCEL + PQP_RANK_W_JUMP + PQP_RANK_W_LATERAL + PQP_RANK_W_CLEARANCE +\n"
           "           PQP_RANK_CLEARANCE_WANT;\n")
    (tmp_path / "proto.c").write_text(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "proto.c", "-o", "proto.o"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]


def test_refused_before_it_touches_a_device(hip_lib):
    """every refusal of the header, in both forms: the arguments are judged before the handle is looked into, so a handle that is only not
    null does for the cases that are bad elsewhere.  The output arrays keep their fill"""
    B, m, n, groups = 4, 5, 3, 2
    fake = C.c_void_p(8)
    prm = K.Params().array()
    traj, paths, gs = np.zeros((B, m, 8)), np.zeros((B, n, 7)), np.array([0, 2, 4], np.int32)
    good = dict(h=fake, prm=prm, require_free=1, batch=B, m=m, stride=8, traj=traj, m_of=None, path_terms=None, search_flags=None, first_hit=None,
                clearance=None, n=n, path_stride=7, paths=paths, n_of=None, groups=groups, group_start=gs)
    outs = ("terms", "best", "best_traj", "best_m", "best_paths", "best_n")

    def weight(i, v):
        w = prm.copy()
        w[i] = v
        return dict(prm=w)

    bad = [dict(h=None), dict(prm=None), dict(traj=None), dict(group_start=None), dict(terms=None), dict(best=None), dict(batch=0), dict(m=0),
           dict(stride=7), dict(n=0), dict(path_stride=6), dict(best_traj=None), dict(best_m=None), dict(best_paths=None), dict(best_n=None),
           dict(paths=None), dict(groups=-1), dict(require_free=2), dict(require_free=-1)]
    bad += [weight(i, v) for i in range(K.RANK_PARAMS) for v in (float("nan"), float("inf"), -float("inf"))]
    host_only = [dict(group_start=np.array(g, np.int32)) for g in ((1, 2, 4), (0, 2, 3), (0, 2, 5), (0, 3, 2))] + [dict(groups=0)]
    for fn, cases in ((hip_lib.pqp_select_plans_device, bad), (hip_lib.pqp_select_plans, bad + host_only)):
        for over in cases:
            out = dict(terms=np.full((B, 10), 7.0), best=np.full(groups, 7, np.int32), best_traj=np.full((groups, m, 8), 7.0),
                       best_m=np.full(groups, 7, np.int32), best_paths=np.full((groups, n, 7), 7.0), best_n=np.full(groups, 7, np.int32))
            a = dict(good, **out)
            a.update(over)
            assert fn(*a.values()) == -1, over
            assert hip_lib.pqp_last_error().decode().startswith("pqp_select_plans:"), over
            assert all((v == 7).all() for v in out.values()), over
    assert list(dict(good, **dict.fromkeys(outs))) == [p.name for p in capi.HEADER.functions["pqp_select_plans"].params]


def test_rank_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    class Stub:
        lib = hip_lib
    se = capi.search_default_params(hip_lib)
    B = 6
    rank = lambda *a: capi.Handle._ranking(Stub, *a)         # (rank, rank_params, winners_only, search, select, batch)
    assert rank(None, None, False, None, None, B) is None and rank(None, None, False, se, [0, B], B) is None
    gs, prm, winners = rank([0, 2, 2, B], None, False, se, None, B)
    assert gs.dtype == np.int32 and gs.tolist() == [0, 2, 2, B] and not winners
    assert prm.array().tolist() == K.Params().array().tolist() and prm.require_free == 1
    mine = capi.rank_default_params(hip_lib, w_progress=0.0)
    got = rank(np.array([0, B]), mine, True, se, None, B)
    assert got[1] is mine and got[2] is True
    for bad in (([0, B], None, False, None, None, B),                # rank without search
                ([0, B], None, False, se, [0, B], B),                # rank with select
                ([0, 3], None, False, se, None, B), ([1, B], None, False, se, None, B), ([0, 4, 3, B], None, False, se, None, B), ([], None, False, se, None, B),
                (None, mine, False, se, None, B),                    # rank_params without rank
                ([0, B], capi.refine_default_params(hip_lib), False, se, None, B)):
        with pytest.raises(ValueError):
            rank(*bad)
    # winners_only without select and without rank is refused as before
    with pytest.raises(ValueError):
        capi.Handle._selection(Stub, None, None, True)


def test_plan_selector_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("rank_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    K.write_case(path, np.zeros((3, 4, 8)), 1.0, None, [0, 1, 3])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no plan selector" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


def test_the_kernels_use_no_scratch_no_lds_and_spill_nothing(hip_lib):
    """what the build gives today: plan_score_kernel 32 VGPRs and plan_group_kernel 16, both whole numbers of the allocation granule of 8,
    8 wavefronts per SIMD.  No LDS, no scratch, no spilled register; no atomic and no shared array: the source has none"""
    report = build_util.kernel_report()
    for name, vgprs in (("plan_score_kernel", 32), ("plan_group_kernel", 16)):
        r = build_util.find_kernel(report, name)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
        assert (r["VGPRs"] + 7) // 8 * 8 == vgprs, (name, r)
    src = open(os.path.join(ROOT, "path_optimizer_2_amd", "csrc", "pqp_rank_kernels.inc")).read()
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower() and "__shared__" not in code and "contract(off)" in src
    assert "group_rows(" in code and "group_least<" in code                         # group_select_kernel's rule, not a copy of it
    assert "wave_sum(" in code and "wave_max(" in code and "__ballot(" in code


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def _refined(names=("rest", "wait", "m3", "m12", "tiles", "long")):
    for name in names:
        p = P.refined_plan(name)
        yield name, p, p["case"]


def test_the_whole_array_form_is_the_loop():
    rng = np.random.default_rng(5)
    B, m = 9, 70
    traj = rng.normal(size=(B, m, 9))
    traj[:, :, 7] = np.cumsum(rng.uniform(0.0, 0.3, (B, m)), axis=1)
    m_of = np.array([0, 1, 2, 3, 63, 64, 65, 70, 90], np.int32)
    clear = rng.uniform(-0.5, 2.0, (B, m))
    clear[4, 7], clear[5, 9], clear[6, 0], clear[7, :] = np.nan, -np.inf, np.inf, np.inf
    pt = rng.uniform(0.0, 3.0, (B, 8))
    for kw in (dict(), dict(clearance=clear, prm=K.Params(w_clearance=2.0, clearance_want=0.9)), dict(path_terms=pt, clearance=clear)):
        a, bound = K.terms(traj, m_of, with_bound=True, **kw)
        b = K.terms(traj, m_of, one=K.addends_loop, **kw)
        assert same_bits(a, b), kw
        assert (a[0] == 0.0).all() and (a[1, [1, 2, 3, 4, 6, 8]] == 0.0).all()       # no rows: ten zeros; one row: no interval
        assert (bound[:, [1, 5, 7, 8, 9]] == 0.0).all()
    assert np.isnan(a[4, 5]) and a[5, 5] == -np.inf and a[7, 5] == np.inf and a[5, 6] == np.inf and a[5, 9] == 0.0    # 0 * inf: no finite score
    # the sum itself: one addend at a time, in ascending order
    add = rng.normal(size=200)
    run = 0.0
    for v in add:
        run = run + float(v)
    assert K.total(add) == run and K.total(np.zeros(0)) == 0.0


def test_progress_and_duration_are_single_subtractions():
    for name, p, c in _refined():
        t = K.terms(p["traj"], p["res"]["reached"])
        for b in range(len(t)):
            L = int(p["res"]["reached"][b])
            if L:
                assert t[b, 1] == p["traj"][b, L - 1, 4] - p["traj"][b, 0, 4] and t[b, 8] == p["traj"][b, L - 1, 7] - p["traj"][b, 0, 7], (name, b)
            else:
                assert (t[b] == 0.0).all()


def test_the_jumps_of_a_refined_plan_are_those_of_its_fine_rows():
    """entry 3 is not divided by time: a refined path has one acceleration per layer, so the differences of its fine rows are the layers'
    jumps with exact zeros between them, and the ascending sum is the same bit for bit at any r"""
    seen = 0
    for name, p, c in _refined():
        coarse = K.terms(p["traj"], p["res"]["reached"])
        for r in (1, 4, 10):
            fine = P.sample_batch(c["paths"], c["profile"], p["traj"], r, c["prm"]["dt"], c.get("n_of"), c.get("stop_before"), p["res"]["reached"],
                                  refine_flags=p["flags"])
            got = K.terms(fine["traj"], fine["m_of"])
            for b in np.flatnonzero(p["flags"] == R.REFINED):
                assert same_bits(got[b, 3], coarse[b, 3]) and coarse[b, 3] > 0.0, (name, r, b)
                a = fine["traj"][b, :fine["m_of"][b], 6]
                inside = np.delete(np.diff(a), np.arange(r - 1, len(a) - 1, r))          # the differences that do not cross a layer
                assert (inside == 0.0).all() and inside.size == (r - 1) * (int(p["res"]["reached"][b]) - 1), (name, r, b)
                assert same_bits(got[b, 1], coarse[b, 1])                                 # and the progress: the same two stations
                seen += 1
    assert seen >= 30


def test_who_is_eligible():
    rng = np.random.default_rng(9)
    B, m = 10, 6
    traj = rng.normal(size=(B, m, 8))
    traj[:, :, 7] = np.arange(m)
    traj[8, 2, 6] = np.nan
    m_of = np.full(B, m, np.int32); m_of[0] = 0
    flags = np.zeros(B, np.int32); flags[1:4] = [K.NO_PLAN | 4, K.EMPTY, K.NOT_FINITE]; flags[9] = 2 | 4 | 8     # START_BLOCKED, GRID_SHORT, ARRIVED: no bar
    first = m_of.copy(); first[5] = 3
    pt = np.ones((B, 8)); pt[6, 7] = 0.0
    t = K.terms(traj, m_of, pt, flags, first)
    assert t[:, 9].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    assert K.terms(traj, m_of, pt, flags, first, prm=K.Params(require_free=0))[:, 9].tolist() == [0, 0, 0, 0, 1, 1, 0, 1, 0, 1]
    assert K.terms(traj, m_of)[:, 9].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0, 1]
    assert K.winners(t, [0, 4, 4, 7, 10]).tolist() == [-1, -1, 4, int(min((7, 9), key=lambda b: (t[b, 0], b)))]
    tie = np.zeros((4, 10)); tie[:, 9] = 1.0; tie[0, 0] = 1.0
    assert K.winners(tie, [0, 4]).tolist() == [1]                                   # the lowest row among equal scores
    got = K.select(traj, [0, 4, 10], m_of, pt, flags, first, paths=np.ones((B, 3, 7)), n_of=np.full(B, 2, np.int32))
    w = got["best"][1]
    assert got["best"][0] == -1 and got["best_m"].tolist() == [0, m] and (got["best_traj"][0] == 0.0).all() and same_bits(got["best_traj"][1], traj[w])
    assert got["best_n"].tolist() == [0, 2] and (got["best_paths"][1, :2] == 1.0).all() and (got["best_paths"][1, 2:] == 0.0).all()


# ---- the hand case: the straighter path waits, its curvier neighbour passes --------------------------------------------------------------------
def test_the_straighter_path_waits_and_the_curvier_one_wins(hip_lib):
    """rank_util.hand_case(): A, the straight road, has the lower pqp_select_paths score and is made to wait by the disc; B, the arc,
    passes.  pqp_select_paths' rule picks A; pqp_select_plans' with the default parameters picks B, by 10 % of |score| or more; without
    the progress term it picks A again"""
    c = K.hand_case()
    circles = capi.car_circles(capi.car_default_geometry(hip_lib, **S.HAND_CAR), hip_lib)
    res = S.run_case(c, circles)
    assert res["reached"].tolist() == [c["m"]] * 2 and res["margins"]["clear"] > S.CLEAR_MARGIN
    sa, sb = res["traj"][0][:, 4], res["traj"][1][:, 4]
    assert (sa[1:] < sb[1:]).all() and sa[4] < K.HAND_DISC[0] - 4.0 < sb[4]          # at layer 4, A's front is still short of the disc; B is past it
    sel = select_util.select(c["paths"], c["group_start"])
    assert sel["best"].tolist() == [0] and sel["terms"][0, 0] == 0.0 < sel["terms"][1, 0]
    hit = A.check(res["traj"], c["agents"], circles, m_of=res["reached"])["first_hit"]
    assert hit.tolist() == [c["m"]] * 2
    kw = dict(m_of=res["reached"], path_terms=sel["terms"], search_flags=res["flags"], first_hit=hit)
    got = K.select(res["traj"], c["group_start"], **kw)
    a, b = got["terms"][0, 0], got["terms"][1, 0]
    print(f"A: score {a!r}, terms {got['terms'][0].tolist()}\nB: score {b!r}, terms {got['terms'][1].tolist()}")
    assert got["best"].tolist() == [1] and (got["terms"][:, 9] == 1.0).all()
    assert a - b >= 0.1 * max(abs(a), abs(b)), (a, b)
    assert got["terms"][1, 4] > 0.0 == got["terms"][0, 4] and got["terms"][1, 1] > got["terms"][0, 1]       # B pays for its curve and is ahead
    assert same_bits(got["best_traj"][0], res["traj"][1]) and got["best_m"].tolist() == [c["m"]]
    slow = K.select(res["traj"], c["group_start"], prm=K.Params(w_progress=0.0), **kw)
    print(f"without progress: A {slow['terms'][0, 0]!r}, B {slow['terms'][1, 0]!r}")
    assert slow["best"].tolist() == [0]
