"""pqp_agents_check without a GPU: the symbols and the binding, the constants, the refusals, the chain wrapper's argument checks, the C++
wrapper's build, the kernels' resources, and known answers by hand for the numpy restatement (tests/agents_util.py) the GPU tests compare
the kernels against."""
import ctypes as C
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
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_agents_check", "pqp_agents_check_device")
HAND_CIRCLES = F.car_circles(**A.HAND_CAR)
INF = math.inf


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_agents_default_params",):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert len(hip_lib.pqp_agents_check_device.argtypes) == 17 and len(hip_lib.pqp_agents_check.argtypes) == 16      # the host form: no frames
    assert list(inspect.signature(capi.Handle.agents_check).parameters) == ["self", "traj", "agents", "m_of", "a_of", "scene_of", "car", "prm",
                                                                            "clearance"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        prm = inspect.signature(fn).parameters
        for k in ("agents", "agents_of", "scene_of", "agents_params"):
            assert prm[k].default is None, k


def test_constants_and_defaults_equal_the_headers(hip_lib):
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (PQP_AGENT_[A-Z_]+) (\d+)", txt)}
    assert consts == dict(PQP_AGENT_STRIDE=capi.AGENT_STRIDE, PQP_AGENT_FRAME_STRIDE=capi.AGENT_FRAME_STRIDE)
    assert (capi.AGENT_STRIDE, capi.AGENT_FRAME_STRIDE) == (6, 8) == (A.AGENT_STRIDE, A.FRAME_STRIDE)
    # one parameter: the ABI passes it as a double, second in both forms, and adds no struct for it
    for fn in (hip_lib.pqp_agents_check, hip_lib.pqp_agents_check_device):
        assert fn.argtypes[1] is C.c_double
    assert not any("agents" in s for s in capi.STRUCTS) and capi.AgentsParams.__slots__ == ("margin",)
    raw = C.c_double(-1.0)
    hip_lib.pqp_agents_default_params(C.byref(raw))
    assert raw.value == 0.0
    p = capi.agents_default_params(hip_lib)                  # pure host
    assert {k: getattr(p, k) for k in A.DEFAULTS} == A.DEFAULTS == dict(margin=0.0)
    assert capi.agents_default_params(hip_lib, margin=0.25).margin == 0.25
    hip_lib.pqp_agents_default_params(None)                  # a null pointer is ignored, as by the other *_default_params


def test_refused_before_it_touches_a_device(hip_lib):
    """both forms refuse a null handle with the entry point's name in front"""
    prm, car = capi.agents_default_params(hip_lib), capi.car_default_geometry(hip_lib)
    assert hip_lib.pqp_agents_check_device(None, prm.margin, C.byref(car), 1, 4, 3, None, None, 1, 1, None, None, None, None, None, None, None) == -1
    assert hip_lib.pqp_last_error().decode().startswith("pqp_agents_check:")
    assert hip_lib.pqp_agents_check(None, prm.margin, C.byref(car), 1, 4, 3, None, None, 1, 1, None, None, None, None, None, None) == -1
    assert hip_lib.pqp_last_error().decode().startswith("pqp_agents_check:")


def test_agents_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    sa = capi.sample_default_params(hip_lib)

    class Stub:                                              # _agents reads self.lib alone
        lib = hip_lib
    check = lambda *a: capi.Handle._agents(Stub, *a)         # (agents, agents_of, scene_of, agents_params, sample, samples, car, batch, select)
    ag = np.zeros((2, 3, 10, 6))
    assert check(None, None, None, None, sa, 10, None, 3, None) is None and check(None, None, None, None, None, None, None, 3, None) is None
    with pytest.raises(ValueError):
        check(ag, None, None, None, None, None, None, 3, None)        # agents without sample
    with pytest.raises(ValueError):
        check(None, [3, 3], None, None, sa, 10, None, 3, None)        # agents_of without agents
    with pytest.raises(ValueError):
        check(None, None, [0], None, sa, 10, None, 3, None)           # scene_of without agents
    with pytest.raises(ValueError):
        check(None, None, None, capi.agents_default_params(hip_lib), sa, 10, None, 3, None)
    with pytest.raises(ValueError):
        check(ag, None, None, None, sa, 12, None, 3, None)            # the agents' steps are not the samples
    with pytest.raises(ValueError):
        check(ag[..., :5], None, None, None, sa, 10, None, 3, None)
    with pytest.raises(ValueError):
        check(ag, [3], None, None, sa, 10, None, 3, None)             # agents_of: one per scene
    with pytest.raises(ValueError):
        check(ag, None, [0, 2], None, sa, 10, None, 3, None)          # a scene that is not there
    got = check(ag, [3, 1], [1, 0, 1], None, sa, 10, None, 3, None)
    assert got[0].shape == ag.shape and got[1].tolist() == [3, 1] and got[2].tolist() == [1, 0, 1] and got[3].margin == 0.0 and got[4] is None
    # scene_of has one entry per row the sampler runs on: per candidate, or per group with select
    with pytest.raises(ValueError, match="one entry per candidate"):
        check(ag, None, [1, 0], None, sa, 10, None, 3, None)
    with pytest.raises(ValueError, match="one entry per group"):
        check(ag, None, [1, 0, 1], None, sa, 10, None, 3, np.array([0, 1, 3]))
    assert check(ag, None, [1, 0], None, sa, 10, None, 3, np.array([0, 1, 3]))[2].tolist() == [1, 0]


def test_checker_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("agents_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    c = A.hand_cases()["parked_box"]
    A.write_case(path, c["traj"], c["agents"], c["margin"], [A.HAND_M], [1], [0])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no checker" in r.stderr


@pytest.mark.parametrize("name,tag,vgprs,occupancy", [("agent_frames_kernel", "", 40, 8), ("agents_check_kernel", "ILb1E", 96, 5),
                                                       ("agents_check_kernel", "ILb0E", 112, 4)])
def test_the_kernels_use_no_scratch_and_no_lds(hip_lib, name, tag, vgprs, occupancy):
    """what the build gives today: 38 VGPRs for the frames, 92 with the clearance written and 97 without (the broad phase's operands),
    each held to the allocation granule of 8 it falls in (40, 96, 112) and to the occupancy that follows from it; an occupancy below 4
    would be a lane state that no longer fits 128 registers"""
    r = build_util.find_kernel(build_util.kernel_report(), name, tag)
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["Occupancy"] >= occupancy >= 4, r
    assert r["VGPRs"] <= vgprs <= 128, r


# ---- known answers of the restatement --------------------------------------------------------------------------------------------------
def _run(case):
    r = A.check(case["traj"], case["agents"], HAND_CIRCLES, m_of=case.get("m_of"), margin=case["margin"])
    return int(r["first_hit"][0]), int(r["hit_agent"][0]), r["clearance"][0]


def test_the_hand_cars_circles_are_dyadic_where_it_matters():
    c = HAND_CIRCLES
    assert c[4].tolist() == [2.25, 0.0, 1.25] and c[5].tolist() == [0.75, 0.0, 1.25]
    assert c[:4, :2].tolist() == [[-0.5, -0.5], [-0.5, 0.5], [3.5, -0.5], [3.5, 0.5]] and (c[:4, 2] == math.sqrt(0.5)).all()
    # Rb: the corner circles reach sqrt(2^2 + 0.5^2) + sqrt(0.5) from the bounding centre (1.5, 0) - beyond the reference's own bounding radius
    assert A.bounding_reach(c) == math.hypot(2.0, 0.5) + math.sqrt(0.5) > c[6][2]


def test_frames_by_hand():
    ag = np.array([[1.0, 2.0, 0.0, 3.0, 4.0, 0.5],           # present: reach = 5 + 0.5
                   [1.0, 2.0, 0.0, -1.0, 4.0, 0.5],          # absent by half_length
                   [math.nan, 2.0, 0.0, 3.0, -0.5, 0.5],     # absent by half_width: the NaN is not read
                   [1.0, math.inf, 0.0, 3.0, 4.0, 0.5],      # bad
                   [1.0, 2.0, 0.0, 3.0, 4.0, -0.5],          # bad: a negative radius
                   [1.0, 2.0, 0.0, math.nan, 4.0, 0.5],      # bad: NaN < 0 is false, so it is present, and not finite
                   [7.0, 8.0, 0.0, 0.0, 0.0, 0.25]])         # a disc
    f = A.frames(ag)
    assert f[0].tolist() == [1.0, 2.0, 1.0, 0.0, 3.0, 4.0, 0.5, 5.5]
    assert f[1].tolist() == f[2].tolist() == [0.0] * 7 + [-1.0]
    for q in (3, 4, 5):
        assert f[q, :7].tolist() == [0.0] * 7 and math.isnan(f[q, 7])
    assert f[6].tolist() == [7.0, 8.0, 1.0, 0.0, 0.0, 0.0, 0.25, 0.25]
    h = A.frames(np.array([[0.0, 0.0, math.pi / 2, 1.0, 1.0, 0.0]]))
    assert h[0, 2] == math.cos(math.pi / 2) and h[0, 3] == 1.0


def test_driving_past_a_parked_box_by_hand():
    """the box's near side is 3 m from the axis, the large circles' radius is 1.25: 1.75 m while one of them is beside the box (steps 0-10),
    more behind it; the small circles are 2.5 - sqrt(0.5) away"""
    cases = A.hand_cases()
    first, who, cl = _run(cases["parked_box"])
    assert (first, who) == (A.HAND_M, -1)
    assert (cl[:11] == 1.75).all() and (cl[11:] > 1.75).all() and (np.diff(cl[11:]) >= 0).all()
    assert cl[11] == math.sqrt(0.25 * 0.25 + 9.0) - 1.25     # the rear large circle, 0.25 m behind the box's end
    assert cl[12] == cl[13] == 2.5 - math.sqrt(0.5)          # then the rear small circle at y = 0.5, still beside the box
    # the box comes nearer by exactly the gap at step 5: touching is no hit at margin 0, and a hit at any margin above
    first, who, cl = _run(cases["moved_by_the_gap_touching"])
    assert (first, who) == (A.HAND_M, -1) and cl[5] == 0.0 and (np.delete(cl, 5) >= 1.75).all()
    first, who, cl = _run(cases["moved_by_the_gap"])
    assert (first, who) == (5, 0) and cl[5] == 0.0


def test_grazing_at_exactly_the_margin_by_hand():
    cases = A.hand_cases()
    first, who, cl = _run(cases["grazing"])                  # d - r_j == margin: strict, no hit
    assert (first, who) == (A.HAND_M, -1) and cl[0] == 1.75
    first, who, cl = _run(cases["grazing_one_ulp_nearer"])   # the box's y one ulp of 4 nearer; sqrt(oy * oy) == oy: it arrives in the clearance
    assert (first, who) == (0, 0) and cl[0] == 1.75 - 2.0 ** -51


def test_inside_disc_absent_bad_and_ego_by_hand():
    cases = A.hand_cases()
    # the front large circle's centre is the box's: ex = -2, ey = -1, d = fmin(fmax(ex, ey), 0) = -1, minus the radius
    first, who, cl = _run(cases["centre_inside"])
    assert (first, who) == (0, 0) and cl.tolist() == [-2.25]
    # a disc of 0.5 m, 3 m beside the front large circle's centre: 3 - 0.5 - 1.25
    first, who, cl = _run(cases["disc"])
    assert (first, who) == (1, -1) and cl.tolist() == [1.25]
    first, who, cl = _run(cases["absent_for_some_steps"])
    assert (first, who) == (A.HAND_M, -1)
    assert (cl[[3, 4, 5, 9]] == INF).all() and (cl[[0, 1, 2, 6, 7, 10]] == 1.75).all()
    assert cl[8] == 4.0 - 1.25                               # -0 is present: a box of no width on the line y = 4
    first, who, cl = _run(cases["bad_rows"])
    assert (first, who) == (7, 1) and cl[7] == -INF and cl[9] == -INF and (cl[[0, 6, 8, 10]] == 1.75).all()
    first, who, cl = _run(cases["ego_nan"])
    assert (first, who) == (4, -1) and cl[4] == -INF and (cl[:4] == 1.75).all() and cl[5] == 1.75
    first, who, cl = _run(cases["ego_inf_over_a_hit"])       # the agent is on top of the car at step 0, and the sample is still its own hit
    assert (first, who) == (0, -1) and cl[0] == -INF and cl[1] < 0.0


def test_counts_ties_and_empty_scenes_by_hand():
    cases = A.hand_cases()
    first, who, cl = _run(cases["count_zero"])               # first_hit = count = 0, as first_collision with n_of = 0
    assert (first, who) == (0, -1) and (cl == 0.0).all()
    first, who, cl = _run(cases["count_three"])              # the hit at step 5 is not checked
    assert (first, who) == (3, -1) and (cl[:3] == 1.75).all() and (cl[3:] == 0.0).all()
    first, who, cl = _run(cases["two_hit_the_same_sample"])
    assert (first, who) == (5, 1) and cl[5] == 0.0
    first, who, cl = _run(cases["no_agents"])
    assert (first, who) == (A.HAND_M, -1) and (cl == INF).all()


def test_hits_at_the_edge_of_the_broad_phase_would_be_lost_to_a_smaller_radius():
    """agents_util.edge_cases: true hits by 1e-6 m whose centres are as far from the bounding centre as a hitting agent's can be.  The
    restated broad phase (the kernel's expression) keeps every one; with the reference's own bounding radius in place of Rb, with the
    margin forgotten, or with the rounding radius forgotten, it leaves them out and the path's only hit is lost - so the GPU test that
    runs these cases with clearance = NULL sees each of those mistakes"""
    circles = F.car_circles()
    c = A.edge_cases(circles)
    run = lambda **kw: A.check(c["traj"], c["agents"], circles, scene_of=c["scene_of"], margin=c["margin"], **kw)
    exact = run()
    assert np.array_equal(exact["first_hit"], c["want_first"]) and np.array_equal(exact["hit_agent"], c["want_who"])
    assert set(c["want_first"].tolist()) == {5, 63, 64, 66}                  # both tiles, both sides of the tile edge
    for b, cl in enumerate(exact["clear"]):
        k = c["want_first"][b]
        assert abs(cl[k, 1] - (c["margin"] - A.EDGE_EPS)) <= 1e-8 and (cl[:, 0] > c["margin"]).all() and (cl[:, 0] < c["margin"] + 2 * A.EDGE_EPS).all()
    kept = run(broad=dict())                                                 # the kernel's own bound
    assert np.array_equal(kept["first_hit"], exact["first_hit"]) and np.array_equal(kept["hit_agent"], exact["hit_agent"])
    assert circles[6][2] < A.bounding_reach(circles) - 0.05                  # the reference's circle does not hold the corner circles
    radii = np.array([c["agents"][b, 1, c["want_first"][b], 5] for b in range(len(c["want_first"]))])
    for kw, lost in ((dict(rb=circles[6][2]), slice(None)), (dict(with_margin=False), slice(None)), (dict(with_radius=False), radii > 0.0)):
        wrong = run(broad=kw)
        assert (wrong["first_hit"][lost] == A.EDGE_M).all() and (wrong["hit_agent"][lost] == -1).all(), kw
    assert (radii > 0.0).sum() >= 6 and (radii == 0.0).any()


def test_seeds_of_the_gpu_test_stay_clear_of_the_margin():
    """the samples whose hit a few ulp of sin / cos could flip, |clear - margin| <= 1e-9, are at most 0.1 % for every seeded case the GPU
    test runs (essentially none: the placements are continuous) - and the cases do hold hits, near misses and clear paths"""
    circles = F.car_circles()
    kinds = set()
    for case in A.seeded_cases():
        r = A.check(case["traj"], case["agents"], circles, case["m_of"], case["a_of"], case["scene_of"], case["margin"])
        near = A.near_margin(r["clear"], case["margin"])
        checked = sum(n.size for n in near)
        assert sum(int(n.sum()) for n in near) <= 1e-3 * checked, case["id"]
        for b, cl in enumerate(r["clear"]):
            kinds.add("hit" if r["first_hit"][b] < cl.shape[0] else "clear")
    assert kinds == {"hit", "clear"}
