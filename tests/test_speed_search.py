"""pqp_speed_search without a GPU: the symbols and the binding, the constants and defaults, the refusals, the chain wrapper's argument
checks, the C++ wrapper's build, the kernels' resources - and the numpy restatement the GPU tests compare the kernels against
(tests/search_util.py): against every admissible plan by brute force (the plan, and the way back through the parents from every state of
the last living layer), on hand cases with answers worked out on dyadic numbers, and the decision margins of the seeds the GPU tests run:
the three seeded shapes and the hand cases of tests/test_gpu_speed_search.py, and the families of tests/test_gpu_speed_search_table.py
("dead", "ties", "horizon70", "horizon260", "steps", "standing", "wide", "thin") with what each is there for - who dies where, which
wavefronts hold the living states of a last layer, which flags occur."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import agents_util as A
import build_util
import cpp_demo
import footprint_util as F
import search_util as S
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_speed_search", "pqp_speed_search_device")
HAND_CIRCLES = F.car_circles(**S.HAND_CAR)
INF = math.inf


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_search_default_params", "pqp_search_params_from_speed"):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert len(hip_lib.pqp_speed_search_device.argtypes) == 25 and len(hip_lib.pqp_speed_search.argtypes) == 23      # the host form: no frames, no parents
    assert list(inspect.signature(capi.Handle.speed_search).parameters) == ["self", "paths", "profile", "v_start", "agents", "m", "n_of", "stop_before",
                                                                            "a_of", "scene_of", "car", "prm", "blocked"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        assert inspect.signature(fn).parameters["search"].default is None


def test_constants_and_defaults_equal_the_headers(hip_lib):
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"(PQP_SEARCH_[A-Z_]+) = (\d+)", txt)}
    assert flags == dict(PQP_SEARCH_NO_PLAN=S.NO_PLAN, PQP_SEARCH_START_BLOCKED=S.START_BLOCKED, PQP_SEARCH_GRID_SHORT=S.GRID_SHORT,
                         PQP_SEARCH_ARRIVED=S.ARRIVED, PQP_SEARCH_EMPTY=S.EMPTY, PQP_SEARCH_NOT_FINITE=S.NOT_FINITE)
    assert all(getattr(capi, k[4:]) == v for k, v in flags.items()) and sorted(flags.values()) == [1, 2, 4, 8, 16, 32]
    assert capi.SEARCH_MAX_STATES == S.MAX_STATES == 4096 == int(re.search(r"#define PQP_SEARCH_MAX_STATES (\d+)", txt).group(1))
    assert capi.SearchParams is capi.STRUCTS["pqp_search_params"]
    assert [f for f, _ in capi.SearchParams._fields_] == list(S.DEFAULTS)
    # the defaults stand in the header's comments, field by field
    sub = open(os.path.join(ROOT, "include", "pqp_search_params.h")).read()
    assert '#include "pqp_search_params.h"' in txt and list(capi.HEADER.included) == ["pqp_search_params"]
    body = re.search(r"typedef struct pqp_search_params \{(.*?)\} pqp_search_params;", sub, re.S).group(1)
    stated = {k: float(v) for k, v in re.findall(r"(\w+);\s*/\*\s*([0-9.]+)", body)}
    assert stated == {k: float(v) for k, v in S.DEFAULTS.items()}
    p = capi.search_default_params(hip_lib)
    assert {k: getattr(p, k) for k in S.DEFAULTS} == S.DEFAULTS
    assert capi.search_default_params(hip_lib, w_accel=0.25, stations=70).stations == 70
    hip_lib.pqp_search_default_params(None)                  # a null pointer is ignored, as by the other *_default_params
    # from_speed: the defaults are that call on the speed defaults at dt = 1, ds = 0.5
    sp = capi.speed_default_params(hip_lib)
    q = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    assert {k: getattr(q, k) for k in S.DEFAULTS} == S.DEFAULTS == S.from_speed(dict(v_max=10.0, a_max=1.5, d_max=3.0), 1.0, 0.5)
    for sp_kw, dt, ds in ((dict(v_max=8.0, a_max=1.0, d_max=2.5), 0.5, 0.25), (dict(v_max=3.0, a_max=0.2, d_max=0.2), 1.0, 1.0), (dict(v_max=15.75), 2.0, 0.5)):
        sp = capi.speed_default_params(hip_lib, **sp_kw)
        want = S.from_speed({k: getattr(sp, k) for k in ("v_max", "a_max", "d_max")}, dt, ds)
        got = capi.search_params_from_speed(hip_lib, sp, dt, ds)
        assert {k: getattr(got, k) for k in S.DEFAULTS} == want, (sp_kw, dt, ds)
    assert want["q_max"] == 63 and S.from_speed(dict(v_max=16.0, a_max=1.5, d_max=3.0), 2.0, 0.5) is None
    keep = capi.search_default_params(hip_lib, stations=5)
    for sp_kw, dt, ds in ((dict(v_max=16.0), 2.0, 0.5), (dict(), 0.0, 0.5), (dict(), 1.0, math.nan)):
        sp = capi.speed_default_params(hip_lib, **sp_kw)
        assert hip_lib.pqp_search_params_from_speed(C.byref(sp), dt, ds, C.byref(keep)) == -1 and keep.stations == 5
        assert hip_lib.pqp_last_error().decode().startswith("pqp_search_params_from_speed:")


def test_the_structs_layout_agrees_with_the_compiler(tmp_path):
    """pqp_search_params lies in a header of its own that pqp.h includes: sizeof, and offsetof and size of every field, as gcc lays it out
    through pqp.h, against the ctypes class the binding's reader built from it (what tests/test_abi_binding.py does for pqp.h's own)"""
    from path_optimizer_2_amd import pqp_header
    s = capi.HEADER.included["pqp_search_params"]
    assert [t for _, t in s.fields] == ["double"] * 5 + ["int32_t"] * 4 and "pqp_search_params" not in capi.HEADER.structs
    prints = [f'printf("{s.name} %zu\\n", sizeof({s.name}));']
    prints += [f'printf("{s.name}.{f} %zu %zu\\n", offsetof({s.name}, {f}), sizeof((({s.name}*)0)->{f}));' for f, _ in s.fields]
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pqp.h"\nint main(void) {\n' + "\n".join(prints) + "\nreturn 0;\n}\n")
    r = subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "layout.c", "-o", "layout"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]
    got = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    cls = capi.SearchParams
    want = [f"{s.name} {C.sizeof(cls)}"] + [f"{s.name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in s.fields]
    assert got == want and C.sizeof(cls) == 56, (got, want)
    assert hip_lib_prototype_takes_the_struct()
    # the reader takes struct typedefs from an included header and nothing else, and no include it cannot find
    (tmp_path / "pqp_x.h").write_text("#ifndef PQP_X_H_\n#define PQP_X_H_\n#include <stdint.h>\ntypedef struct pqp_x { double a; int32_t n; } pqp_x;\n#endif\n")
    small = ('#ifndef PQP_H_\n#define PQP_H_\n#include <stdint.h>\n#include "pqp_x.h"\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
             "int pqp_f(const pqp_x* x);\n#ifdef __cplusplus\n}\n#endif\n#endif\n")
    h = pqp_header.parse(small, str(tmp_path))
    assert h.included["pqp_x"].fields == (("a", "double"), ("n", "int32_t")) and not h.structs and h.functions["pqp_f"].params[0].type == "const pqp_x*"
    with pytest.raises(pqp_header.HeaderError):
        pqp_header.parse(small)                              # no directory to read the include from
    for bad in ("int pqp_g(int n);", "#define PQP_Y 3", "typedef struct pqp_y { float f; } pqp_y;", "enum { PQP_Z = 1 };"):
        (tmp_path / "pqp_x.h").write_text(f"#ifndef PQP_X_H_\n#define PQP_X_H_\n#include <stdint.h>\n{bad}\n#endif\n")
        with pytest.raises(pqp_header.HeaderError):
            pqp_header.parse(small, str(tmp_path))


def hip_lib_prototype_takes_the_struct():
    lib = capi.load_library()
    return lib.pqp_speed_search.argtypes[1] is C.POINTER(capi.SearchParams) and lib.pqp_search_default_params.argtypes[0] is C.POINTER(capi.SearchParams)


def test_refused_before_it_touches_a_device(hip_lib):
    """both forms refuse a null handle with the entry point's name in front"""
    prm, car = capi.search_default_params(hip_lib), capi.car_default_geometry(hip_lib)
    nothing = (None,) * 5
    assert hip_lib.pqp_speed_search_device(None, C.byref(prm), C.byref(car), 1, 4, 6, None, None, None, None, None, 4, 1, 0, None, None, None, None, None, None,
                                           *nothing) == -1
    assert hip_lib.pqp_last_error().decode().startswith("pqp_speed_search:")
    assert hip_lib.pqp_speed_search(None, C.byref(prm), C.byref(car), 1, 4, 6, None, None, None, None, None, 4, 1, 0, None, None, None, None, *nothing) == -1
    assert hip_lib.pqp_last_error().decode().startswith("pqp_speed_search:")


def test_search_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    sa, sp, se = capi.sample_default_params(hip_lib), capi.speed_default_params(hip_lib), capi.search_default_params(hip_lib)

    class Stub:                                              # _search and _agents read self.lib alone
        lib = hip_lib
    ag = np.zeros((2, 3, 10, 6))
    search = lambda *a: capi.Handle._search(Stub, *a)        # (search, speed, agents)
    assert search(None, None, None) is None and search(None, sp, ag) is None and search(se, sp, ag) is se
    for bad in ((se, None, ag), (se, sp, None), (dict(S.DEFAULTS), sp, ag)):
        with pytest.raises(ValueError):
            search(*bad)
    agents = lambda *a, **kw: capi.Handle._agents(Stub, *a, **kw)      # (agents, agents_of, scene_of, agents_params, sample, samples, car, batch, select)
    with pytest.raises(ValueError):
        agents(ag, None, None, None, None, None, None, 3, None)        # neither sample nor search
    got = agents(ag, [3, 1], [1, 0, 1], None, None, None, None, 3, None, search=se)      # the search alone: the agents' steps are its layers
    assert got[0].shape == ag.shape and got[1].tolist() == [3, 1] and got[2].tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        agents(ag[..., :5], None, None, None, None, None, None, 3, None, search=se)
    with pytest.raises(ValueError):
        agents(ag, None, None, None, sa, 12, None, 3, None, search=se)                   # with sample too, the steps are the samples
    assert agents(ag, None, None, None, sa, 10, None, 3, None, search=se)[0].shape == ag.shape


def test_searcher_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("search_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    S.write_case(path, S.hand_cases()["parked_box"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no searcher" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


@pytest.mark.parametrize("name,vgprs,occupancy,lds", [("st_occupancy_kernel", 88, 5, 0), ("st_search_kernel", 64, 2, 65536)])
def test_the_kernels_use_no_scratch_and_spill_nothing(hip_lib, name, vgprs, occupancy, lds):
    """what the build gives today: 84 VGPRs for the occupancy (the six centres, the bounding centre and the circle test's operands) and 60 for
    the search, each held to the allocation granule of 8 it falls in (88, 64).  The occupancy kernel holds no LDS and keeps five wavefronts
    per SIMD (at least four: a lane state that fits 128 registers); the search kernel's two cost layers are 65 536 bytes exactly, which
    is what bounds it to two workgroups - two wavefronts per SIMD - per CU"""
    r = build_util.find_kernel(build_util.kernel_report(), name)
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size"] == lds <= 65536, r
    assert r["Occupancy"] >= occupancy, r
    assert r["VGPRs"] <= vgprs <= 128, r
    if name == "st_occupancy_kernel":
        assert r["Occupancy"] >= 4


# ---- the restatement against every admissible plan ---------------------------------------------------------------------------------------
BRUTE = [(seed, 6 + seed % 7, 2 + seed % 2, 3 + seed % 3) for seed in range(8)]          # S 6 .. 12, Q 2 .. 3, m 3 .. 5
# the parameter classes of search_util.family(): q_up > q_down, a car that can only stand, a price on slowness alone, other steps of time and arc
BRUTE_MORE = {9: dict(q_up=3, q_down=1), 12: dict(q_up=2, q_down=1), 10: dict(q_max=0), 11: dict(w_slow=0.75, w_accel=0.0), 15: dict(w_slow=2.5, w_accel=0.0),
              13: dict(dt=0.8, ds=0.3), 16: dict(dt=0.8, ds=0.3, q_up=3, q_down=1, w_slow=0.75, w_accel=0.5)}
BRUTE += [(seed, 7 + seed % 5, 0 if seed == 10 else 3, 4 + seed % 2) for seed in BRUTE_MORE]


def _q0(v0, prm):
    return int(min(max(np.rint(np.float64(v0) * np.float64(prm["dt"]) / np.float64(prm["ds"])), 0.0), prm["q_max"]))


def _brute_case(seed, Sn, Q, m, density):
    rng = np.random.default_rng(100 + seed)
    weights = {1: (0.0, 0.0), 2: (0.0, 0.0), 5: (0.0, 1.0)}.get(seed,(0.5, 2.0) if seed % 2 == 0 else (0.3, 1.7))      # dyadic and not; two that tie all over
    prm = S.params(stations=Sn, q_max=Q, q_up=1 + seed % 2, q_down=1 + (seed // 2) % 3, w_accel=weights[0], w_slow=weights[1])
    prm.update(BRUTE_MORE.get(seed, {}))
    n = 2 * Sn + 1 - (seed % 3)                              # waypoints every 0.25 m: the path ends at, before or behind the grid
    path = S.straight(n, step=0.25)
    profile = S.profile_of(path, 1.0 * (seed % 3), v_end=None if seed % 4 else 0.0, prm=dict(v_max=1.75, a_max=0.75))
    cells = rng.uniform(size=(m, Sn)) < density
    cells[0, 0] = seed == 5 and density > 0.3                # one case starts blocked
    return prm, path, profile, 1.0 * (seed % 3), cells


@pytest.mark.parametrize("density", (0.12, 0.45))
@pytest.mark.parametrize("seed,Sn,Q,m", BRUTE)
def test_the_search_finds_what_the_enumeration_finds(seed, Sn, Q, m, density):
    prm, path, profile, v0, cells = _brute_case(seed, Sn, Q, m, density)
    got = S.search(path, profile, v0, np.zeros((0, m, 8)), HAND_CIRCLES, m, prm=prm, cells=cells)
    full = S.unpack(got["blocked"], Sn)
    assert np.array_equal(full[:, :got["J"]], cells[:, :got["J"]]) and not full[:, got["J"]:].any()
    q0 = _q0(v0, prm)
    assert q0 == min(max(int(round(v0 * prm["dt"] / prm["ds"])), 0), Q) == got["q0"]
    reached, plans = S.enumerate_plans(full, got["qenv"], got["J"], q0, prm)
    assert got["reached"] == reached and len(got["parents"]) == max(reached, 1) and list(got["qref"]) == S.reference_steps(got["qenv"], got["J"], Q)
    if reached == 0:
        assert not plans and got["cost"] == INF and got["flags"] & S.START_BLOCKED
        return
    assert len(plans) >= 1
    cost, seq = S.first_plan(plans)
    assert got["cost"] == min(c for c, _ in plans) == cost                   # bit for bit: the same edges added in the same order
    assert got["steps"][:reached].tolist() == [list(jq) for jq in seq]
    assert (got["steps"][reached:] == -1).all() and bool(got["flags"] & S.NO_PLAN) == (reached < m)
    # the table behind the plan: the states of the last living layer are the ends of the enumeration's sequences, and the way back from
    # each of them through the parents is the first, by the parent rule, of the cheapest sequences that end there
    ends = {}
    for cs in plans:
        ends.setdefault(cs[1][-1], []).append(cs)
    assert set(ends) == (set(got["parents"][reached - 1]) if reached > 1 else {(0, q0)})
    for (j, q), group in ends.items():
        cost, seq = S.first_plan(group)
        back = [(j, q)]
        for k in range(reached - 1, 0, -1):
            back.append((back[-1][0] - back[-1][1], got["parents"][k][back[-1]]))
        assert back[::-1] == seq, (j, q)


def test_the_brute_force_cases_hold_plans_dead_ends_and_ties():
    kinds, ties = set(), 0
    for density in (0.12, 0.45):
        for seed, Sn, Q, m in BRUTE:
            prm, path, profile, v0, cells = _brute_case(seed, Sn, Q, m, density)
            got = S.search(path, profile, v0, np.zeros((0, m, 8)), HAND_CIRCLES, m, prm=prm, cells=cells)
            kinds.add("through" if got["reached"] == m else "blocked at the start" if got["reached"] == 0 else "dead end")
            reached, plans = S.enumerate_plans(S.unpack(got["blocked"], Sn), got["qenv"], got["J"], _q0(v0, prm), prm)
            ties += sum(1 for c, _ in plans if c == got["cost"]) > 1
    assert kinds == {"through", "blocked at the start", "dead end"} and ties >= 2


# ---- hand cases on dyadic numbers ------------------------------------------------------------------------------------------------------
def _run(name, **kw):
    c = S.hand_cases()[name]
    r = S.run_case(c, HAND_CIRCLES, **kw)
    return r["steps"][0].tolist(), int(r["reached"][0]), int(r["flags"][0]), float(r["cost"][0]), r


def _hand_sum(steps, qref, w_accel, w_slow=1.0):
    """the edges of a plan added up as the definition adds them, from the step list and the stations' qref"""
    cost = 0.0
    for (jp, qp), (j, q) in zip(steps[:-1], steps[1:]):
        assert j == jp + q
        cost = cost + (w_accel * float((q - qp) ** 2) + w_slow * float(qref[jp] - q))
    return cost


def test_the_hand_roads_envelope():
    """from rest at a_max = 1.5 the profile has v^2 = 3 s: qenv_j = floor(2 sqrt(1.5 j)) up to the cap of 12, which the braking into v_end = 0
    at waypoint 40 (d_max = 3: v^2 = 6 (20 - s)) cuts from station 29 on"""
    r = _run("free_road")[4]["each"][0]
    assert r["J"] == 41
    up = [min(int(math.floor(2.0 * math.sqrt(1.5 * j))), 99) for j in range(41)]
    down = [int(math.floor(2.0 * math.sqrt(3.0 * (40 - j)))) for j in range(41)]
    assert r["qenv"].tolist() == [min(u, d) for u, d in zip(up, down)]
    assert r["qenv"][:5].tolist() == [0, 2, 3, 4, 4] and r["qenv"][-4:].tolist() == [6, 4, 3, 0] and r["qenv"].max() == 12
    qref = S.reference_steps(r["qenv"], 41, 20)
    assert qref[0] == 10 and qref[30:] == list(range(10, -1, -1))       # 20 cells ahead of station 0 the envelope is at 10; the end comes nearer


def test_free_road_from_rest_by_hand():
    """(a) a change of step costs 2^-6 a cell squared against 1 per cell of slowness: the plan takes q_up more per layer - 3, 6, 9 - then
    what the envelope allows at its arrival (11 at station 29), and brakes by at most q_down = 6 into the last station, where it stands"""
    steps, reached, flags, cost, r = _run("free_road")
    assert steps == [[0, 0], [3, 3], [9, 6], [18, 9], [29, 11], [37, 8], [40, 3], [40, 0]]
    assert (reached, flags) == (8, S.ARRIVED)
    e = r["each"][0]
    qref = S.reference_steps(e["qenv"], e["J"], 20)
    assert cost == _hand_sum(steps, qref, 2.0 ** -6) == 19.15625
    # 9 * 4 + 4 + 9 + 25 + 9 = 83 sixty-fourths of acceleration; slowness (10 - 3) + (11 - 6) + (12 - 9) + (11 - 11) + (11 - 8) + (3 - 3) + 0 = 18
    assert cost == 18.0 + (9 + 9 + 9 + 4 + 9 + 25 + 9) / 64.0
    t = r["traj"][0]
    assert t[:, 0].tolist() == t[:, 4].tolist() == [0.0, 1.5, 4.5, 9.0, 14.5, 18.5, 20.0, 20.0] and (t[:, 1:4] == 0).all()
    assert t[:, 5].tolist() == [0.0, 1.5, 3.0, 4.5, 5.5, 4.0, 1.5, 0.0] and t[:, 6].tolist() == [1.5, 1.5, 1.5, 1.0, -1.5, -2.5, -1.5, 0.0]
    assert t[:, 7].tolist() == [float(k) for k in range(8)]


def test_a_box_parked_on_the_path_by_hand():
    """(b) the box fills x = 12 .. 14 across the road: the front corner circles, 3.5 m ahead of the station with radius sqrt(0.5), touch it
    from station 16 (x = 8: 8 + 3.5 + 0.707 > 12) and the rear ones let go behind station 30 (15 - 0.5 - 0.707 < 14 < 15.5 - 1.207): the
    plan ends at station 15, the last one clear of it, and is not ARRIVED"""
    steps, reached, flags, cost, r = _run("parked_box")
    cells = S.unpack(r["blocked"][0], 48)
    assert all(cells[k].nonzero()[0].tolist() == list(range(16, 31)) for k in range(8))
    assert steps[-1] == [15, 7] and (reached, flags) == (8, 0) and max(j for j, _ in steps) == 15
    e = r["each"][0]
    assert cost == _hand_sum(steps, S.reference_steps(e["qenv"], e["J"], 20), 2.0 ** -6)
    assert steps == [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [3, 3], [8, 5], [15, 7]]         # standing at 0 or at 15 costs the same 10 a layer


def test_a_crossing_pedestrian_by_hand():
    """(c) a disc of 0.5 m at x = 9.25 blocks stations 10 .. 21 (the front circles reach it from x = 5: 5 + 3.5 + 0.707 + 0.5 > 9.25; the rear
    ones let go behind x = 10.5: 11 - 0.5 - 0.707 - 0.5 > 9.25) during layers 2 and 3.  With w_accel = 1 the plan from rest builds up slowly
    and is at station 9 at layer 4, before the disc's stations, which it enters in the step to layer 5, the first whose two layers are both
    free.  With w_accel = 2^-6 and the disc there at layers 5 and 6, the car rolling at 2 m/s is through its stations at layer 3 and stands
    at the end of the road when the disc comes"""
    steps, reached, flags, cost, r = _run("crossing_wait")
    cells = S.unpack(r["blocked"][0], 48)
    held = list(range(10, 22))
    assert [cells[k].nonzero()[0].tolist() for k in range(8)] == [[], [], held, held, [], [], [], []]
    assert steps == [[0, 0], [0, 0], [2, 2], [5, 3], [9, 4], [14, 5], [20, 6], [27, 7]] and (reached, flags, cost) == (8, 0, 59.0)
    e = r["each"][0]
    assert cost == _hand_sum(steps, S.reference_steps(e["qenv"], e["J"], 20), 1.0)
    assert max(j for j, _ in steps[:5]) == 9 < 10
    steps, reached, flags, cost, r = _run("crossing_pass")
    assert steps == [[0, 4], [7, 7], [17, 10], [28, 11], [37, 9], [40, 3], [40, 0], [40, 0]] and (reached, flags, cost) == (8, S.ARRIVED, 10.0625)
    assert steps[3][0] > 21 and min(j for j, _ in steps[4:]) > 21 and S.unpack(r["blocked"][0], 48)[5:7, 10:22].all()


def test_the_swept_range_rule_by_hand():
    """(d) the same disc during layers 1 and 2.  Without the swept-range rule - only the two ends of a step tested - the plan steps from
    station 9 at layer 2 to 18 at layer 3: through stations 10 .. 18, which the disc holds at layer 2 and has left at layer 3.  With the rule
    it brakes to a stand at station 0, and starts one layer later"""
    steps, reached, flags, cost, r = _run("jump", swept=False)
    assert steps[:4] == [[0, 4], [3, 3], [9, 6], [18, 9]]
    cells = S.unpack(r["blocked"][0], 48)
    assert cells[2, 10:14].all() and not cells[3].any() and not cells[2, 9] and not cells[3, 18]
    steps, reached, flags, cost, _ = _run("jump")
    assert steps == [[0, 4], [0, 0], [3, 3], [9, 6], [18, 9], [29, 11], [37, 8], [40, 3]] and (reached, flags) == (8, S.ARRIVED)
    for k in range(1, 8):                                    # no step sweeps a station that is blocked at either of its layers
        lo, hi = steps[k - 1][0], steps[k][0]
        assert not cells[k - 1, lo:hi + 1].any() and not cells[k, lo:hi + 1].any()


def test_an_agent_driving_into_the_standing_car_by_hand():
    """(e) one waypoint: the car can only stand at station 0.  A box of half length 2 comes down the road 3 m a layer from x = 20: its front is
    at 18 - 3 k, the car's front circles reach 3.5 + sqrt(0.5) = 4.207: free up to layer 4 (front at 6), hit from layer 5 (front at 3):
    five layers are reached.  Standing at layer 0 already: nothing is"""
    steps, reached, flags, cost, r = _run("driven_into")
    assert steps == [[0, 0]] * 5 + [[-1, -1]] * 3 and (reached, flags, cost) == (5, S.NO_PLAN | S.ARRIVED, 0.0)
    assert S.unpack(r["blocked"][0], 48)[:, 0].tolist() == [False] * 5 + [True] * 3 and (r["traj"][0][5:] == 0).all()
    steps, reached, flags, cost, r = _run("start_blocked")
    assert steps == [[-1, -1]] * 8 and (reached, flags, cost) == (0, S.NO_PLAN | S.START_BLOCKED, INF) and (r["traj"] == 0).all()


def test_counts_layers_absent_and_bad_rows_by_hand():
    """(f)"""
    steps, reached, flags, cost, r = _run("empty")
    assert steps == [[-1, -1]] * 8 and (reached, flags, cost) == (0, S.EMPTY, INF) and (r["traj"] == 0).all() and (r["blocked"] == 0).all()
    steps, reached, flags, cost, _ = _run("one_waypoint")
    assert steps == [[0, 0]] * 8 and (reached, flags, cost) == (8, S.ARRIVED, 0.0)
    steps, reached, flags, cost, _ = _run("one_layer")
    assert steps == [[0, 0]] and (reached, flags, cost) == (1, 0, 0.0)
    free = _run("free_road")
    for name in ("a_of_zero", "absent_row"):                 # the box on the car is not there: the free road's plan
        assert _run(name)[:4] == free[:4], name
    steps, reached, flags, cost, r = _run("bad_row")          # a heading that is no number at layer 2: every station of that layer
    cells = S.unpack(r["blocked"][0], 48)
    assert cells[2, :41].all() and not cells[2, 41:].any() and not np.delete(cells, 2, axis=0).any()
    assert steps == [[0, 0], [3, 3]] + [[-1, -1]] * 6 and (reached, flags) == (2, S.NO_PLAN)
    steps, reached, flags, cost, r = _run("grid_short")      # 24 stations on 20 m of road: the plan runs to the grid's last station
    assert r["each"][0]["J"] == 24 and (reached, flags) == (8, S.GRID_SHORT) and steps[-1][0] == 23
    bad = dict(S.hand_cases()["free_road"])
    for col, where in ((0, "paths"), (2, "profile")):
        c = dict(bad, **{where: bad[where].copy()})
        c[where][0, 7, col] = math.nan
        r = S.run_case(c, HAND_CIRCLES)
        assert r["flags"][0] == S.NOT_FINITE and np.isnan(r["traj"]).all() and math.isnan(r["cost"][0]) and (r["steps"] == -1).all() and (r["blocked"] == 0).all()
    for v in (-0.5, math.inf, math.nan):
        assert S.run_case(dict(bad, v_start=np.array([v])), HAND_CIRCLES)["flags"][0] == S.NOT_FINITE


# ---- the seeds of the GPU test ---------------------------------------------------------------------------------------------------------
def test_seeds_of_the_gpu_test_stay_clear_of_every_decision():
    """every |clear - margin| of every cell is at least 1e-6 m and every gap between a state's best and second-best predecessor, or between
    the two cheapest terminal states, is a tie (exactly 0, decided by the tie rule) or at least 1e-9 - for every case the GPU test runs, none
    left out: the hand cases, the three seeded shapes, and the riders of the broad phase test sit a slack of 2^-10 m away by construction.
    And the cases hold blocked cells, plans that get through, one that arrives, and agents that are absent"""
    circles = F.car_circles()
    for name in S.SEEDED:
        c = S.seeded(name)
        r = S.run_case(c, circles)
        assert r["margins"]["clear"] >= S.CLEAR_MARGIN, (name, r["margins"])
        assert min(r["margins"]["cost_gap"], r["margins"]["end_gap"]) >= S.COST_MARGIN, (name, r["margins"])
        assert (r["blocked"] != 0).any() and (r["reached"] == c["m"]).all(), name
    for name, c in S.hand_cases().items():
        r = S.run_case(c, HAND_CIRCLES)
        assert r["margins"]["clear"] >= S.CLEAR_MARGIN and min(r["margins"]["cost_gap"], r["margins"]["end_gap"]) >= S.COST_MARGIN, (name, r["margins"])


# ---- the families of tests/test_gpu_speed_search_table.py ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(name):
    c = S.family(name)
    return c, S.run_case(c, F.car_circles())


@pytest.mark.parametrize("name", S.FAMILIES)
def test_families_of_the_table_test_stay_clear_of_every_decision(name):
    """the same two margins as the seeds', no family and no path left out (an exact tie has an infinite gap: "ties" has nothing else)"""
    c, r = _family(name)
    assert r["margins"]["clear"] >= S.CLEAR_MARGIN, (name, r["margins"])
    assert min(r["margins"]["cost_gap"], r["margins"]["end_gap"]) >= S.COST_MARGIN, (name, r["margins"])
    assert (r["blocked"] != 0).any() and c["prm"]["stations"] * (c["prm"]["q_max"] + 1) <= S.MAX_STATES
    for w in ("w_slow", "w_accel"):                          # dyadic: a cost gap is a tie or large
        assert (c["prm"][w] * 16.0).is_integer()


def _waves(one, prm):
    lanes, win = S.last_lanes(one, prm)
    return {l // 64 for l in lanes}, win, len(lanes) - len(set(lanes))


@pytest.mark.parametrize("name", S.DEAD_ENDS)
def test_the_dead_ends_die_late_and_in_every_wavefront(name):
    """who dies where: the bad rows at layers 8 and 5, the wall at layer 5, the start above the envelope at layer 1, and path 4 gets through.
    The last living layers of the four that move hold living states in all four wavefronts (e mod 256 in each range of 64) and lanes with
    several living states; at least one winner lies in a wavefront that is neither the first nor the last, so no rule that takes the
    first or the last wavefront's state finds it"""
    c, r = _family(name)
    m, prm = c["m"], c["prm"]
    assert r["reached"].tolist() == [8, 5, 5, 1, m] and r["flags"].tolist() == [S.NO_PLAN] * 4 + [0]
    assert [e["q0"] for e in r["each"]] == [0, 6, 0, prm["q_max"], 2] and r["each"][3]["qenv"].max() < prm["q_max"] - prm["q_down"]
    cells = S.unpack(r["blocked"], prm["stations"])
    for b, k in ((0, 8), (1, 5)):                            # the bad row: every station of the path at that layer, none elsewhere
        J = r["each"][b]["J"]
        assert cells[b, k, :J].all() and not np.delete(cells[b], k, axis=0).any()
    in_reach = max(j for j, _ in r["each"][2]["parents"][4]) + prm["q_max"]
    assert cells[2, 5, :in_reach + 1].all() and not cells[2, 5, r["each"][2]["J"] - 1] and not cells[2, :5].any()            # a wall, not a bad row
    assert not cells[3].any()
    seen = [_waves(r["each"][b], prm) for b in (0, 1, 2, 4)]
    assert all(waves == {0, 1, 2, 3} for waves, _, _ in seen)
    assert sum(win >= 64 for _, win, _ in seen) >= 1 and any(64 <= win < 192 for _, win, _ in seen)
    assert sum(dup >= 1 for _, _, dup in seen) >= 2
    for b in range(5):                                       # behind a dead end
        k = r["reached"][b]
        assert (r["steps"][b, k:] == -1).all() and (r["traj"][b, k:] == 0).all() and r["traj"][b, k - 1, 6] == 0
    if name == "ties":
        assert (r["cost"] == 0).all() and r["margins"]["cost_gap"] == INF == r["margins"]["end_gap"]
        for b in (0, 1, 2, 4):                               # the terminal rule alone: the largest j of the last layer, then the smallest q
            last = list(r["each"][b]["parents"][r["reached"][b] - 1])
            assert tuple(r["steps"][b, r["reached"][b] - 1]) == min(last, key=lambda jq: (-jq[0], jq[1]))
    else:
        assert (r["cost"][[0, 1, 2, 4]] > 0).all()


@pytest.mark.parametrize("name", S.HORIZONS)
def test_the_horizons_wait_and_go_beside_an_empty_and_a_bad_path(name):
    c, r = _family(name)
    m = c["m"]
    assert m in (70, 260) and r["reached"].tolist() == [m, 0, m, 0, m]
    assert r["flags"].tolist() == [S.ARRIVED, S.EMPTY, S.GRID_SHORT, S.NOT_FINITE, S.GRID_SHORT] and r["each"][0]["J"] < c["prm"]["stations"]
    for b in (0, 2, 4):                                      # stands for most of the horizon, then goes to the last station
        j = r["steps"][b, :, 0]
        stand = np.flatnonzero(np.diff(j) == 0)
        assert (np.diff(j) >= 0).all() and j[-1] == r["each"][b]["J"] - 1 and j[m - 25] < j[-1] and len(stand) >= m - 25


def test_the_other_families_hold_what_they_are_there_for():
    c, r = _family("steps")
    assert c["paths"].shape[2] == 9 and (c["paths"][:, :, 7:] == 1e9).all() and c["prm"]["q_up"] > c["prm"]["q_down"]
    assert (r["reached"] == c["m"]).all() and [e["q0"] for e in r["each"]] == [0, 5, 12] and c["v_start"][2] * 0.8 / 0.3 > 12.5
    assert all(_waves(e, c["prm"])[0] == {0, 1, 2, 3} for e in r["each"])
    c, r = _family("standing")
    assert S.words(c["prm"]["stations"]) == 5 and r["reached"].tolist() == [6, 3, 0]
    assert r["flags"].tolist() == [S.GRID_SHORT, S.GRID_SHORT | S.NO_PLAN, S.GRID_SHORT | S.NO_PLAN | S.START_BLOCKED]
    assert (r["steps"][0] == 0).all() and (r["traj"][0, :, 4:7] == 0).all() and r["traj"][0, :, 7].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert (r["blocked"] != 0).any(axis=(0, 1)).all()          # every one of the five words, the third tile's single one too
    c, r = _family("wide")
    J = [e["J"] for e in r["each"]]
    assert J[0] == 4096 and J[1] % 64 != 0 and 2048 < J[1] < 4096 - 64 and r["flags"].tolist() == [S.GRID_SHORT, 0] and (r["reached"] == 3).all()
    cells = S.unpack(r["blocked"], 4096)
    for b in range(2):                                       # agents beyond tile 15 and beyond tile 31; nothing behind the path's last station
        assert cells[b, :, 1024:2048].any() and cells[b, :, 2048:J[b]].any() and not cells[b, :, J[b]:].any()
    c, r = _family("thin")
    assert c["prm"]["stations"] * 3 == S.MAX_STATES - 1 and r["reached"].tolist() == [40, 10, 20]
    j = r["steps"][0, :, 0]
    assert (np.diff(j) == 1)[:11].all() and j[-1] > 64                       # held back by the waiting agent, then at the full step into a second station tile
    # somewhere on a curved path: ARRIVED, GRID_SHORT, and neither with the path ending on the grid
    assert _family("horizon70")[1]["flags"][0] == S.ARRIVED and _family("steps")[1]["flags"][0] == S.GRID_SHORT
    dead = _family("dead")
    assert dead[1]["flags"][4] == 0 and dead[1]["each"][4]["J"] < dead[0]["prm"]["stations"]
