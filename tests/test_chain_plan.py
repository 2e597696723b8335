"""What Handle.optimize_path returns, from its plan alone (capi.Handle._chain_plan: no device, no torch): for every configuration of
tests/chain_plan_cases.py the result's keys in order, each key's shape and dtype, and the keys that winners_only keeps on the device.  The
expected values are written out here, from the wrapper's contract (optimize_path's docstring); test_gpu_chain.py holds the device to the
same plan.

Shapes: 4 candidates in 3 groups, n_max 128, 2 scenes of 1 agent, 3 layers, 2 sub-steps per layer = 5 fine steps, 3 samples, 96 stations
= 3 words of the search's blocked bits."""
import numpy as np
import pytest

import chain_plan_cases as cases
from path_optimizer_2_amd import capi

F, I, U8 = "float64", "int32", "uint8"
# key -> (shape, dtype) where the speed stages run on every candidate (4 rows) ...
PER_CANDIDATE = {
    "out": ((4, 128, 7), F), "n_out": ((4,), I), "status": ((4,), I), "stage": ((4,), I), "iters": ((4,), I),
    "free": ((4, 128), U8), "first_collision": ((4,), I), "margin": ((4, 128), F),
    "terms": ((4, 8), F), "best": ((3,), I), "best_paths": ((3, 128, 7), F), "best_n": ((3,), I),
    "profile": ((4, 128, 4), F), "speed_flags": ((4,), I),
    "traj": ((4, 3, 8), F), "traj_n": ((4,), I), "traj_flags": ((4,), I),
    "first_hit": ((4,), I), "hit_agent": ((4,), I), "agent_clearance": ((4, 3), F),
    "search_steps": ((4, 3, 2), I), "search_traj": ((4, 3, 8), F), "search_cost": ((4,), F), "search_reached": ((4,), I), "search_flags": ((4,), I),
    "search_blocked": ((4, 3, 3), I), "refine_traj": ((4, 3, 8), F), "refine_bounds": ((4, 3, 3), F), "refine_cost": ((4,), F),
    "refine_excess": ((4,), F), "refine_status": ((4,), I), "refine_flags": ((4,), I),
    "plan_traj": ((4, 5, 8), F), "plan_m_of": ((4,), I), "plan_defect": ((4,), F), "plan_excess": ((4,), F), "plan_flags": ((4,), I),
    "plan_first_hit": ((4,), I), "plan_hit_agent": ((4,), I),
    "predict_flags": ((2, 1), I), "predict_anchor": ((2, 1, 4), F),
    "plan_clearance": ((4, 5), F), "rank_terms": ((4, 10), F), "rank_best": ((3,), I), "best_traj": ((3, 5, 8), F), "best_m": ((3,), I),
}
# ... and where they run on the winners of a selection (3 rows)
PER_GROUP = dict(PER_CANDIDATE, **{
    "profile": ((3, 128, 4), F), "speed_flags": ((3,), I),
    "traj": ((3, 3, 8), F), "traj_n": ((3,), I), "traj_flags": ((3,), I),
    "first_hit": ((3,), I), "hit_agent": ((3,), I), "agent_clearance": ((3, 3), F),
    "search_steps": ((3, 3, 2), I), "search_traj": ((3, 3, 8), F), "search_cost": ((3,), F), "search_reached": ((3,), I), "search_flags": ((3,), I),
    "search_blocked": ((3, 3, 3), I), "refine_traj": ((3, 3, 8), F), "refine_bounds": ((3, 3, 3), F), "refine_cost": ((3,), F),
    "refine_excess": ((3,), F), "refine_status": ((3,), I), "refine_flags": ((3,), I),
    "plan_traj": ((3, 5, 8), F), "plan_m_of": ((3,), I), "plan_defect": ((3,), F), "plan_excess": ((3,), F), "plan_flags": ((3,), I),
    "plan_first_hit": ((3,), I), "plan_hit_agent": ((3,), I),
})

# configuration -> (the result's keys in order, the keys that stay on the device, the table their shapes are in)
EXPECTED = {
    "a": (["out", "n_out", "status", "stage", "iters"], [], PER_CANDIDATE),
    "b": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin"], [], PER_CANDIDATE),
    "c": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin"], [], PER_CANDIDATE),
    "d": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "terms", "best", "best_paths", "best_n"], [], PER_GROUP),
    "d_winners": (["n_out", "status", "stage", "iters", "first_collision", "terms", "best", "best_paths", "best_n"], ["out", "free", "margin"], PER_GROUP),
    "e": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "terms", "best", "best_paths", "best_n", "profile",
           "speed_flags", "traj", "traj_n", "traj_flags", "first_hit", "hit_agent", "agent_clearance"], [], PER_GROUP),
    "e_winners": (["n_out", "status", "stage", "iters", "first_collision", "terms", "best", "best_paths", "best_n", "profile", "speed_flags", "traj",
                   "traj_n", "traj_flags", "first_hit", "hit_agent", "agent_clearance"], ["out", "free", "margin"], PER_GROUP),
    "f": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "profile", "speed_flags", "search_steps", "search_traj",
           "search_cost", "search_reached", "search_flags"], [], PER_CANDIDATE),
    "g": (["out", "n_out", "status", "stage", "iters", "profile", "speed_flags", "traj", "traj_n", "traj_flags", "first_hit", "hit_agent",
           "agent_clearance", "search_steps", "search_traj", "search_cost", "search_reached", "search_flags"], [], PER_CANDIDATE),
    "h": (["out", "n_out", "status", "stage", "iters", "terms", "best", "best_paths", "best_n", "profile", "speed_flags", "search_steps",
           "search_traj", "search_cost", "search_reached", "search_flags", "search_blocked", "refine_traj", "refine_bounds", "refine_cost",
           "refine_excess", "refine_status", "refine_flags", "plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags", "plan_first_hit",
           "plan_hit_agent"], [], PER_GROUP),
    "i": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "profile", "speed_flags", "search_steps", "search_traj",
           "search_cost", "search_reached", "search_flags", "plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags"], [], PER_CANDIDATE),
    "j": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "profile", "speed_flags", "search_steps", "search_traj",
           "search_cost", "search_reached", "search_flags", "search_blocked", "refine_traj", "refine_bounds", "refine_cost", "refine_excess",
           "refine_status", "refine_flags", "plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags", "plan_first_hit", "plan_hit_agent",
           "plan_clearance", "terms", "rank_terms", "rank_best", "best_paths", "best_n", "best_traj", "best_m"], [], PER_CANDIDATE),
    "j_winners": (["n_out", "status", "stage", "iters", "first_collision", "speed_flags", "search_steps", "search_cost", "search_reached",
                   "search_flags", "search_blocked", "refine_bounds", "refine_cost", "refine_excess", "refine_status", "refine_flags", "plan_m_of",
                   "plan_defect", "plan_excess", "plan_flags", "plan_first_hit", "plan_hit_agent", "terms", "rank_terms", "rank_best", "best_paths",
                   "best_n", "best_traj", "best_m"],
                  ["out", "free", "margin", "profile", "search_traj", "refine_traj", "plan_traj", "plan_clearance"], PER_CANDIDATE),
    "k": (["out", "n_out", "status", "stage", "iters", "profile", "speed_flags", "search_steps", "search_traj", "search_cost", "search_reached",
           "search_flags", "plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags", "plan_first_hit", "plan_hit_agent", "predict_flags",
           "predict_anchor", "plan_clearance", "terms", "rank_terms", "rank_best", "best_paths", "best_n", "best_traj", "best_m"], [], PER_CANDIDATE),
    "l": (["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "profile", "speed_flags", "search_steps", "search_traj",
           "search_cost", "search_reached", "search_flags"], [], PER_CANDIDATE),
}


def expected(name):
    """[(key, shape, dtype)] in the result's order, and the keys that stay on the device"""
    keys, on_device, table = EXPECTED[name]
    return [(k,) + table[k] for k in keys], on_device


def plan_of(lib, kw):
    h = capi.Handle.__new__(capi.Handle)          # no pqp_create: the plan needs the library's defaults and no device
    h.lib = lib
    cfg = capi._defaults(lib, capi.PqpChainConfig, "pqp_chain_default_config", cases.CHAIN_CONFIG)
    return h._chain_plan(points=np.zeros((cases.B, 9, 2)), cfg=cfg, **kw)


def test_every_configuration_has_its_expectation(hip_lib):
    assert list(cases.configs(hip_lib)) == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_the_plan_s_keys_shapes_and_dtypes(hip_lib, name):
    plan = plan_of(hip_lib, cases.configs(hip_lib)[name][1])
    want, on_device = expected(name)
    assert [k for k, _, _ in plan.result] == [k for k, _, _ in want]
    assert plan.result == want
    assert plan.on_device == on_device


def test_the_speed_stages_rows_and_steps(hip_lib):
    """the context the stages share: rows = groups with select=, else the batch; the layers, fine steps and samples"""
    cf = cases.configs(hip_lib)
    h, j, e, a = (plan_of(hip_lib, cf[k][1]) for k in ("h", "j", "e", "a"))
    assert (h.rows, h.paths, h.layers, h.fine, h.samples) == (3, ("best_paths", "best_n", None), 3, 5, None)
    assert (j.rows, j.paths, j.layers, j.fine, j.samples) == (4, ("out", "n_out", "first_collision"), 3, 5, None)
    assert (e.rows, e.paths, e.layers, e.fine, e.samples) == (3, ("best_paths", "best_n", None), None, None, 3)
    assert (a.rows, a.paths, a.layers, a.fine, a.samples) == (4, ("out", "n_out", None), None, None, None)


def test_one_entry_per_row_or_a_value_error(hip_lib):
    cf = cases.configs(hip_lib)
    per_candidate, per_group = cf["f"][1], cf["e"][1]
    for kw, rows, other, what in ((per_candidate, 4, 3, "candidate"), (per_group, 3, 4, "group")):
        for name in ("v_start", "v_end"):
            with pytest.raises(ValueError, match=rf"^v_start / v_end must have one entry per {what} \({rows}\)$"):
                plan_of(hip_lib, dict(kw, **{name: np.zeros(other)}))
        plan_of(hip_lib, dict(kw, v_end=np.zeros(rows)))
    with pytest.raises(ValueError, match=r"^t0 must have one entry per group \(3\)$"):
        plan_of(hip_lib, dict(per_group, t0=np.zeros(4)))
    with pytest.raises(ValueError, match=r"^t0 must have one entry per candidate \(4\)$"):
        plan_of(hip_lib, dict(cf["g"][1], t0=np.zeros(3)))
    plan_of(hip_lib, dict(per_group, t0=np.zeros(3)))
    with pytest.raises(ValueError, match=r"^group_start must ascend from 0 to the batch \(4\)$"):
        plan_of(hip_lib, dict(cf["d"][1], select=np.array([0, 2, 5], np.int32)))
    with pytest.raises(TypeError, match="no_such_argument"):
        plan_of(hip_lib, dict(no_such_argument=1))
