"""pqp_speed_refine without a GPU: the symbols and the binding, the constants and defaults, the prototypes in a C file, the refusals, the
chain wrapper's argument checks, the C++ wrapper's build, the kernels' resources - and the numpy restatement the GPU tests compare the
kernels against (tests/refine_util.py): the corridor on hand cases against a bit-by-bit loop, and the QP through the banded core's host
emulation (banded_util.to_banded with interleave3, emu_solve under production parameters with the polish on) against HiGHS.

Measured here (test_the_emulation_solves_what_highs_solves prints them) over refine_util.GPU_CASES - the hand cases, the seeded scenes at
m = 2, 3, 8, 12, 40, 86 and 193 and the search's seeds "tiles" and "long", 32 refined paths:
  the emulation's worst KKT residuals on the restatement's matrices, with its own multipliers:
      stationarity 3.56e-8, primal violation 3.00e-8, complementarity 2.59e-7            -> refine_util.KKT_WORST (3.6e-8, 3.0e-8, 2.6e-7)
  its worst distance to HiGHS in any variable: 2.87e-6 (it grows with m; HiGHS's own 1e-7 regularisation is in it)
                                                                                         -> refine_util.HIGHS_DIST (2.9e-6)
Every one of them is solved by the direct active-set attempt (iters = 0).  The one infeasible QP ("quick": the staircase runs ahead of
what a_max admits) ends PQP_STATUS_PRIMAL_INFEASIBLE on the emulation and "Infeasible" in HiGHS.  tests/test_gpu_speed_refine.py holds the
device to 4 x the residuals and 2 x the distance."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import build_util
import cpp_demo
import refine_util as R
import search_util as S
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_speed_refine", "pqp_speed_refine_device")


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_refine_default_params",):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert len(hip_lib.pqp_speed_refine_device.argtypes) == 24 == len(hip_lib.pqp_speed_refine.argtypes)
    assert hip_lib.pqp_speed_refine.argtypes[1] is C.POINTER(capi.SearchParams)           # the grid is the search's struct: no new one
    assert list(inspect.signature(capi.Handle.speed_refine).parameters) == ["self", "paths", "profile", "v_start", "blocked", "steps", "reached",
                                                                            "search_traj", "n_of", "stop_before", "grid", "prm"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        assert inspect.signature(fn).parameters["refine"].default is None


def test_constants_and_defaults_equal_the_headers(hip_lib):
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    stated = {k: int(v) for k, v in re.findall(r"(PQP_REFINE_[A-Z_]+) = (\d+)", txt)}
    assert stated == dict(PQP_REFINE_W_REF=R.W_REF, PQP_REFINE_W_ACCEL=R.W_ACCEL, PQP_REFINE_W_JERK=R.W_JERK, PQP_REFINE_A_MAX=R.A_MAX,
                          PQP_REFINE_D_MAX=R.D_MAX, PQP_REFINE_REFINED=R.REFINED, PQP_REFINE_KEPT=R.KEPT, PQP_REFINE_INFEASIBLE=R.INFEASIBLE)
    assert all(getattr(capi, k[4:]) == v for k, v in stated.items())
    assert capi.REFINE_PARAMS == R.N_PARAMS == 5 == int(re.search(r"#define PQP_REFINE_PARAMS (\d+)", txt).group(1))
    assert (capi.STATUS_UNSOLVED, capi.STATUS_SOLVED, capi.STATUS_PRIMAL_INFEASIBLE) == (R.UNSOLVED, R.SOLVED, R.PRIMAL_INFEASIBLE)
    assert len(capi.HEADER.structs) == 10 and list(capi.HEADER.included) == ["pqp_search_params"]      # no new struct anywhere
    p = capi.refine_default_params(hip_lib)
    sp = capi.speed_default_params(hip_lib)
    assert p.array().tolist() == R.DEFAULT_PRM.tolist() == [1.0, 1.0, 1.0, sp.a_max, sp.d_max] and p.window == R.DEFAULT_WINDOW == 4
    q = capi.refine_default_params(hip_lib, w_jerk=0.5, window=2)
    assert q.array()[capi.REFINE_W_JERK] == 0.5 and q.window == 2
    hip_lib.pqp_refine_default_params(None, None)            # null pointers are ignored, each on its own
    only = C.c_int(-7)
    hip_lib.pqp_refine_default_params(None, C.byref(only))
    values = np.full(5, -1.0)
    hip_lib.pqp_refine_default_params(values, None)
    assert only.value == 4 and values.tolist() == R.DEFAULT_PRM.tolist()
    assert R.layout_doubles(R.CAPACITY_M) * 8 <= 160 * 1024 < R.layout_doubles(R.CAPACITY_M + 1) * 8
    assert "m > %d" % R.CAPACITY_M in re.sub(r"\s+\*\s+", " ", txt)


def test_a_c_file_compiles_the_prototypes(tmp_path):
    src = ('#include "pqp.h"\n'
           "int (*device_form)(pqp_handle*, const pqp_search_params*, const double*, int, int, int, int, const double*, const int32_t*, const int32_t*,\n"
           "                   const double*, const double*, int, const int32_t*, const int32_t*, const int32_t*, const double*, double*, double*, double*,\n"
           "                   double*, int32_t*, int32_t*, int32_t*) = pqp_speed_refine_device;\n"
           "int (*host_form)(pqp_handle*, const pqp_search_params*, const double*, int, int, int, int, const double*, const int32_t*, const int32_t*,\n"
           "                 const double*, const double*, int, const int32_t*, const int32_t*, const int32_t*, const double*, double*, double*, double*,\n"
           "                 double*, int32_t*, int32_t*, int32_t*) = pqp_speed_refine;\n"
           "void (*defaults)(double*, int*) = pqp_refine_default_params;\n"
           "double prm[PQP_REFINE_PARAMS];\n"
           "int index_of_last = PQP_REFINE_D_MAX, flags = PQP_REFINE_REFINED | PQP_REFINE_KEPT | PQP_REFINE_INFEASIBLE;\n")
    (tmp_path / "proto.c").write_text(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "proto.c", "-o", "proto.o"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]


def test_refused_before_it_touches_a_device(hip_lib):
    """both forms refuse a null handle with the entry point's name in front"""
    grid, prm = capi.search_default_params(hip_lib), capi.refine_default_params(hip_lib)
    for fn in (hip_lib.pqp_speed_refine_device, hip_lib.pqp_speed_refine):
        assert fn(None, C.byref(grid), prm.array(), 4, 1, 4, 6, *(None,) * 5, 4, *(None,) * 11) == -1
        assert hip_lib.pqp_last_error().decode().startswith("pqp_speed_refine:")


def test_refine_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    class Stub:
        lib = hip_lib
    se, rf = capi.search_default_params(hip_lib), capi.refine_default_params(hip_lib)
    refine = lambda *a: capi.Handle._refine(Stub, *a)        # (refine, search)
    assert refine(None, None) is None and refine(None, se) is None and refine(rf, se) is rf
    for bad in ((rf, None), (R.DEFAULT_PRM, se)):
        with pytest.raises(ValueError):
            refine(*bad)


def test_refiner_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("refine_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    S.write_case(path, R.seeded("wait"))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no refiner" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


@pytest.mark.parametrize("name,vgprs,occupancy,lds", [("st_corridor_kernel", 40, 2, 32768), ("refine_assemble_kernel", 48, 8, 0),
                                                       ("refine_finish_kernel", 72, 7, 0)])
def test_the_kernels_use_no_scratch_and_spill_nothing(hip_lib, name, vgprs, occupancy, lds):
    """what the build gives today: 34, 48 and 68 VGPRs, each held to the allocation granule of 8 it falls in.  The corridor kernel's
    envelope of up to PQP_SEARCH_MAX_STATES stations is 32 KiB of LDS: a workgroup is one wavefront, so the LDS bounds a CU to five of
    them (the remark counts two per SIMD); the other two hold no LDS.  None takes an atomic: their source has none"""
    r = build_util.find_kernel(build_util.kernel_report(), name)
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size"] == lds, r
    assert r["Occupancy"] >= occupancy, r
    assert r["VGPRs"] <= vgprs <= 128, r
    src = open(os.path.join(ROOT, "path_optimizer_2_amd", "csrc", "pqp_refine_kernels.inc")).read()
    assert "atomic" not in re.sub(r"//.*", "", src).lower()


# ---- the corridor --------------------------------------------------------------------------------------------------------------------------
def _loop(cells, j_of, J, window):
    """jlo_k, jhi_k bit by bit: one station at a time away from j_k while it is free in all three layers"""
    m = cells.shape[0]
    runs = []
    for k in range(m):
        rows = (k, max(k - 1, 0), min(k + 1, m - 1))
        free = lambda j: not any(cells[r, j] for r in rows)
        jk = int(j_of[k])
        assert free(jk)
        jlo = jhi = jk
        while jlo - 1 >= max(jk - window, 0) and free(jlo - 1):
            jlo -= 1
        while jhi + 1 <= min(jk + window, J - 1) and free(jhi + 1):
            jhi += 1
        runs.append((jlo, jhi))
    return runs


def _hand_cells(S_, m, occupied):
    cells = np.zeros((m, S_), bool)
    for k, j0, j1 in occupied:
        cells[k, j0:j1 + 1] = True
    return cells


CORRIDORS = {
    # name: (S, J, window, j_k per layer, [(layer, first, last occupied station)], the runs expected)
    "across_31_32": (70, 70, 8, [30, 33, 36], [(1, 24, 26), (1, 40, 41)], [(27, 38), (27, 39), (28, 39)]),
    "across_63_64": (70, 70, 6, [60, 62, 66], [(0, 57, 57), (2, 69, 69)], [(58, 66), (58, 68), (60, 68)]),
    "cut_at_0_and_j_last": (70, 50, 5, [2, 47, 49], [], [(0, 7), (42, 49), (44, 49)]),
    "window_0": (40, 40, 0, [0, 7, 33], [(1, 8, 8)], [(0, 0), (7, 7), (33, 33)]),
    "only_at_neighbour_layers": (40, 40, 4, [10, 10, 10, 10], [(0, 12, 12), (3, 7, 8)], [(6, 11), (6, 11), (9, 14), (9, 14)]),
    "three_words": (100, 100, 40, [50, 50], [(0, 20, 20), (1, 90, 95)], [(21, 89), (21, 89)]),
}


@pytest.mark.parametrize("name", list(CORRIDORS))
def test_the_corridor_on_hand_cases(name):
    S_, J, window, j_of, occupied, want = CORRIDORS[name]
    cells = _hand_cells(S_, len(j_of), occupied)
    venv = np.sqrt(np.arange(S_).astype(np.float64))         # ascending: vcap is the envelope at jhi
    ds = np.float64(0.5)
    bounds, runs = R.corridor(cells, j_of, J, venv, window, ds)
    assert [tuple(r) for r in runs.tolist()] == want == _loop(cells, j_of, J, window)
    for k, (jlo, jhi) in enumerate(want):
        assert bounds[k].tolist() == ([0.0, 0.0] if k == 0 else [jlo * 0.5, jhi * 0.5]) + [venv[jhi]]
    # the packed words give the same cells back, and a window beyond the grid is the grid
    assert np.array_equal(S.unpack(S.pack(cells), S_), cells)
    assert R.corridor(cells, j_of, J, venv, 10 ** 9, ds)[1].tolist() == R.corridor(cells, j_of, J, venv, S_, ds)[1].tolist()


def test_a_station_that_is_not_free_is_no_searchs_output():
    cells = _hand_cells(40, 3, [(2, 5, 5)])
    assert R.corridor(cells, [0, 5, 9], 40, np.ones(40), 4, 0.5)[0] is None              # occupied at layer k + 1
    assert R.corridor(cells, [0, 4, 40], 40, np.ones(40), 4, 0.5)[0] is None             # outside the path
    assert R.corridor(cells, [0, 4, 9], 40, np.ones(40), 4, 0.5)[0] is not None


@pytest.mark.parametrize("name", R.GPU_CASES)
def test_every_searched_station_is_free_in_its_three_layers(name):
    """the search's swept-range rule: j_k is free at layers k - 1, k and k + 1, so no corridor is empty - over every seeded search output,
    and the restatement's runs are the loop's"""
    r = R.reference(name, highs=False)
    c, res, m = r["case"], r["res"], r["m"]
    for b, one in enumerate(r["each"]):
        if int(res["reached"][b]) != m or m < 2:
            assert one["su"]["kept"]
            continue
        cells = S.unpack(res["blocked"][b], c["prm"]["stations"])
        j_of = res["steps"][b][:, 0]
        for k in range(m):
            assert not (cells[k, j_of[k]] or cells[max(k - 1, 0), j_of[k]] or cells[min(k + 1, m - 1), j_of[k]]), (name, b, k)
        assert not one["su"]["kept"]
        window = R.DEFAULT_WINDOW
        assert [tuple(x) for x in one["su"]["runs"].tolist()] == _loop(cells, j_of, one["su"]["J"], window), (name, b)


# ---- the QP --------------------------------------------------------------------------------------------------------------------------------
def test_the_dense_qp_is_the_stated_objective():
    """1/2 x'Px + q'x + w_ref sum sigma^2 is the stated sum, on random points; the rows are the stated kinematics"""
    rng = np.random.default_rng(5)
    m, dt = 6, 0.5
    prm = np.array([0.7, 1.3, 0.4, 1.5, 3.0])
    sigma = np.sort(rng.uniform(0, 10, m))
    bounds = np.stack([sigma - 1, sigma + 1, np.full(m, 5.0)], axis=1)
    P, q, A, lo, up = R.qp(bounds, sigma, 1.25, dt, prm)
    assert P.shape == (3 * m, 3 * m) and A.shape == (5 * m - 2, 3 * m) and np.array_equal(P, P.T)
    for _ in range(5):
        x = rng.normal(size=3 * m)
        assert abs(0.5 * x @ P @ x + q @ x + prm[0] * (sigma ** 2).sum() - R.objective(x, sigma, dt, prm)) < 1e-11
    # a trajectory of constant acceleration satisfies the dynamics rows exactly
    a = np.append(rng.uniform(-1, 1, m - 1), 0.0)
    v, s = np.zeros(m), np.zeros(m)
    v[0] = 1.25
    for k in range(m - 1):
        v[k + 1] = v[k] + dt * a[k]
        s[k + 1] = s[k] + dt * v[k] + 0.5 * dt * dt * a[k]
    z = A @ np.concatenate([s, v, a])
    assert np.abs(z[3 * m:]).max() < 1e-14 and lo[3 * m:].tolist() == up[3 * m:].tolist() == [0.0] * (2 * m - 2)
    assert (lo[0], up[0], lo[m], up[m], lo[3 * m - 1], up[3 * m - 1]) == (0.0, 0.0, 1.25, 1.25, 0.0, 0.0)
    assert lo[2 * m:3 * m - 1].tolist() == [-3.0] * (m - 1) and up[2 * m:3 * m - 1].tolist() == [1.5] * (m - 1)


def test_the_emulation_solves_what_highs_solves():
    """every case, none left out: a path that is to be refined is solved by the emulation and by HiGHS; one that is to be kept as infeasible
    is infeasible for both.  The worst residuals and the worst distance are printed, and are what the module docstring states"""
    import banded_util as B
    worst, dist, refined, seen_infeasible = dict(stationarity=0.0, primal=0.0, complementarity=0.0), 0.0, 0, set()
    for name in R.GPU_CASES:
        r = R.reference(name)
        m = r["m"]
        for b, one in enumerate(r["each"]):
            if one["su"]["kept"]:
                continue
            P, q, A, lo, up = one["su"]["qp"]
            bd = B.to_banded(P, q, A, lo, up, B.interleave3(m))
            assert (bd["bw"], bd["pbw"]) == (3, 3) and (bd["acol"] >= 0).sum(axis=1).max() <= 4 and (bd["trow"] >= 0).sum(axis=1).max() <= 6
            if (name, b) in R.INFEASIBLE_CASES:
                assert one["emu"]["status"] == R.PRIMAL_INFEASIBLE and one["highs"] == "Infeasible", (name, b, one["emu"]["status"], one["highs"])
                seen_infeasible.add((name, b))
                continue
            assert one["emu"]["status"] == R.SOLVED and one["highs"] == "Optimal", (name, b, one["emu"]["status"], one["highs"])
            assert one["emu"]["iters"] == 0, (name, b)       # the direct active-set attempt
            cert = R.certificate(P, q, A, lo, up, one["xe"], one["emu"]["y"])
            d = float(np.abs(one["xe"] - one["xh"]).max())
            print(f"{name} path {b}: m = {m}, " + ", ".join(f"{k} {v:.2e}" for k, v in cert.items()) + f", distance to HiGHS {d:.2e}")
            worst = {k: max(worst[k], cert[k]) for k in worst}
            dist = max(dist, d)
            refined += 1
            # the multipliers recovered from x alone certify it as well as the emulation's own do
            again = R.certificate(P, q, A, lo, up, one["xe"])
            assert all(again[k] <= 4.0 * R.KKT_WORST[k] for k in again), (name, b, again)
            ours, theirs = (R.objective(x, one["su"]["sigma"], r["case"]["prm"]["dt"], R.DEFAULT_PRM) for x in (one["xe"], one["xh"]))
            assert abs(ours - theirs) < 1e-6 * max(1.0, theirs)
    print("worst:", ", ".join(f"{k} {v:.2e}" for k, v in worst.items()), f"; distance to HiGHS {dist:.2e}; {refined} refined paths")
    assert seen_infeasible == R.INFEASIBLE_CASES and refined == 32
    for k in worst:
        assert 0.5 * R.KKT_WORST[k] <= worst[k] <= R.KKT_WORST[k], (k, worst[k])          # the stated figures are the measured ones
    assert 0.5 * R.HIGHS_DIST <= dist <= R.HIGHS_DIST, dist


def test_from_rest_on_a_free_road():
    """the staircase 0, 2, 6, 12, 19, ... cells becomes a start at a_max that eases off: s_1 = a_max dt^2 / 2 exactly, speeds ascend while it runs up, every
    station within its window, and no jump in a larger than the staircase's ds / dt^2"""
    r = R.reference("rest")
    one, m = r["each"][0], r["m"]
    s, v, a = one["xe"][:m], one["xe"][m:2 * m], one["xe"][2 * m:]
    assert r["res"]["steps"][0][:, 0].tolist() == [0, 2, 6, 12, 19, 26, 33, 40]
    assert abs(a[0] - 1.5) < 1e-7 and abs(s[1] - 0.75) < 1e-7 and abs(v[1] - 1.5) < 1e-7
    assert (np.diff(v[:5]) > 0).all() and (np.diff(s) > 0).all()
    b = one["su"]["bounds"]
    assert (s >= b[:, 0] - 1e-7).all() and (s <= b[:, 1] + 1e-7).all()
    assert np.abs(np.diff(a)).max() < np.abs(np.diff(r["res"]["traj"][0][:, 6])).max()


def test_waiting_for_a_crossing_disc():
    """the waiting case: under the search's margin of 1 m the disc holds stations 8 .. 23 during layers 2 and 3, so with the neighbour layers
    the corridor ends at station 7 from layer 3 to layer 4 - the refined plan is at most at 3.5 m until t = 4 s.  The corridor is clear of
    the disc by more than CHECK_MARGIN + ds at every one of its stations, so the GPU test may hand the refined plan to pqp_agents_check
    under CHECK_MARGIN.  (Clear by more than the SEARCH's margin + ds it cannot be where the occupancy ends the corridor: the clearance is
    1-Lipschitz in the station, and the cell behind the last free one is below the margin.)"""
    import agents_util as A
    r = R.reference("wait")
    one, m, c = r["each"][0], r["m"], r["case"]
    cells = S.unpack(r["res"]["blocked"][0], c["prm"]["stations"])
    assert [np.flatnonzero(cells[k]).tolist() for k in range(m)] == [[], [], list(range(8, 24)), list(range(8, 24)), [], [], [], []]
    assert r["res"]["steps"][0][:, 0].tolist() == [0, 0, 1, 3, 7, 13, 20, 28]
    runs = one["su"]["runs"]
    assert runs.tolist() == [[0, 4], [0, 4], [0, 5], [0, 7], [3, 7], [9, 17], [16, 24], [24, 32]]
    s = one["xe"][:m]
    assert (s[:5] <= 3.5 + 1e-7).all() and abs(s[4] - 3.5) < 1e-6 and s[5] > 4.5
    fr = A.frames(c["agents"])[0]
    pose = S.stations(c["paths"][0], c["profile"][0], c["paths"].shape[1], c["prm"])[2]
    for k in range(m):
        jlo, jhi = (int(x) for x in runs[k])
        clear = A.clear_matrix(pose[jlo:jhi + 1], np.repeat(fr[:, k:k + 1], jhi - jlo + 1, axis=1), R.circles_of("wait"))
        assert clear.min() > R.CHECK_MARGIN + c["prm"]["ds"], (k, clear.min())
