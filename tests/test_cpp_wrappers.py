"""What the header-only C++ wrappers (include/pqp_*.hpp) have in common.  The rows, ragged batches and agent scenes they share
(include/pqp_wrapper_detail.hpp): tests/cpp/wrapper_rows_check.cpp, a plain C++ program on that header and pqp_types.hpp alone, under
the address and undefined-behaviour sanitizers.  And every wrapper that takes or names a state type against the reference's own State /
SlState (include/data_struct/data_struct.hpp:14-32) with PQP_USE_REFERENCE_TYPES, as a compile check.  No GPU."""
import os
import subprocess

import pytest

import cpp_demo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_shared_rows_batches_and_agent_scenes(tmp_path):
    exe = str(tmp_path / "wrapper_rows_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I" + INCLUDE, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "wrapper_rows_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 ragged batches + 5 layouts (pose, path with and without heading, profile, trajectory) + the timed trajectory there and back
    # + 3 scene sets + the one-step form
    assert r.stdout.strip() == "ok 12", r.stdout


_BOTH = ("const std::vector<std::vector<State>>& a, const std::vector<std::vector<SlState>>& b", "std::vector<std::vector<State>> x; std::vector<std::vector<SlState>> y;")
_SCENES = "const std::vector<double>& v, const std::vector<std::vector<std::vector<PredictedAgent>>>& s"

# per wrapper: what is compiled behind `#include "pqp_<name>.hpp"` - the body of a function that calls every method templated on the state
# type with State and with SlState; None: the header alone, its methods name State / SlState themselves
WRAPPERS = {
    "agent_checker": ("bool f(AgentChecker& c, %s, const std::vector<std::vector<std::vector<PredictedAgent>>>& s, std::vector<int>* o) {\n"
                      "    return c.check(a, s, o, o) && c.check(b, s, o, o); }\n" % _BOTH[0]),
    "speed_searcher": ("bool f(SpeedSearcher& c, %s, %s, std::vector<SpeedSearcher::Plan>* o) {\n"
                       "    %s\n    return c.search(a, v, s, o, &x) && c.search(b, v, s, o, &y); }\n" % (_BOTH[0], _SCENES, _BOTH[1])),
    "speed_profiler": None,
    "trajectory_sampler": ("bool f(TrajectorySampler& t, %s, const std::vector<std::vector<double>>& tt, std::vector<std::vector<State>>* o) {\n"
                           "    return t.sample(a, tt, 5, o) && t.sample(b, tt, 5, o); }\n" % _BOTH[0]),
    "frenet_projector": None,
    "speed_refiner": ("bool f(SpeedRefiner& c, %s, %s, std::vector<SpeedRefiner::Result>* o) {\n"
                      "    %s\n    return c.refine(a, v, s, o, &x) && c.refine(b, v, s, o, &y); }\n" % (_BOTH[0], _SCENES, _BOTH[1])),
    "plan_sampler": ("bool f(PlanSampler& c, %s, %s, std::vector<PlanSampler::Result>* o) {\n"
                     "    %s\n    return c.sample(a, v, s, o, &x) && c.sample(b, v, s, o, &y); }\n" % (_BOTH[0], _SCENES, _BOTH[1])),
    "plan_selector": ("bool f(PlanSelector& c, %s, const std::vector<int>& g, std::vector<int>* o) {\n"
                      "    %s\n    return c.selectBest(a, 0.1, g, o, nullptr, &x) && c.selectBest(b, 0.1, g, o, nullptr, &y); }\n" % _BOTH),
    "trajectory_stitcher": ("bool f(TrajectoryStitcher& c, %s, const std::vector<TrajectoryStitcher::Measured>& m) {\n"
                            "    std::vector<TrajectoryStitcher::Result<State>> x; std::vector<TrajectoryStitcher::Result<SlState>> y;\n"
                            "    return c.stitch(a, 0.1, m, &x) && c.stitch(b, 0.1, m, &y); }\n" % _BOTH[0]),
    "fallback_planner": ("bool f(FallbackPlanner& c, %s, const std::vector<FallbackPlanner::Start>& st, FallbackPlanner::Plans* p) {\n"
                         "    std::vector<FallbackPlanner::Result<State>> x; std::vector<FallbackPlanner::Result<SlState>> y;\n"
                         "    return c.brake(a, st, 0.1, 2, 5, p) && c.brake(b, st, 0.1, 2, 5, p) && c.pick(*p, nullptr, nullptr, &x) && c.pick(*p, nullptr, nullptr, &y); }\n"
                         % _BOTH[0]),
    "path_selector": None,
    "footprint_checker": None,          # over the HIP runtime API as well
}


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_compiles_against_the_reference_headers(name):
    """with PQP_USE_REFERENCE_TYPES a wrapper reads, fills and returns the reference's own State / SlState"""
    if not os.path.isdir(cpp_demo.REF_INCLUDE):
        pytest.skip("the reference tree is not on this box")
    src = "#include \"pqp_%s.hpp\"\nusing namespace PathOptimizationNS;\n%s" % (name, WRAPPERS[name] or "")
    hip = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] if name == "footprint_checker" else []          # no other wrapper may need them
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-DPQP_USE_REFERENCE_TYPES", *hip, "-I" + cpp_demo.REF_INCLUDE, "-I" + INCLUDE,
           "-include", "data_struct/data_struct.hpp", "-"]
    r = subprocess.run(cmd, input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "error" not in r.stderr
