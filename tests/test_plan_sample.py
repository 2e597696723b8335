"""pqp_sample_plan without a GPU: the symbols and the binding, the enumerators, the prototypes in a C file, the refusals, the chain
wrapper's argument checks, the C++ wrapper's build, the kernel's resources - and the numpy restatement the GPU tests compare the kernel
against (tests/plan_util.py): its vectorised form against the plain loop, the properties the definition promises, and the hand case the
call exists for, a disc that crosses the lane between two layers.

Measured here (test_a_refined_plan_follows_its_own_kinematics prints them) over refine_util.QP_CASES' refined paths, plans finished from
the banded core's host emulation: the worst defect is 3.2e-8 m where plan_util.defect_bound allows 1.4e-7 (dt = 1) - the bound is derived
from refine_util.KKT_WORST's primal residual, not from these figures."""
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
import refine_util as R
import search_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_sample_plan", "pqp_sample_plan_device")
KEYS = ("traj", "m_of", "defect", "excess", "flags")


def _same(a, b, where):
    for k in KEYS:
        assert same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), (where, k)


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES:
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert len(hip_lib.pqp_sample_plan_device.argtypes) == 20 == len(hip_lib.pqp_sample_plan.argtypes)
    assert hip_lib.pqp_sample_plan.argtypes[1:4] == [C.c_double, C.c_int, C.c_int]         # dt, r, linear by value: no new struct
    assert list(inspect.signature(capi.Handle.sample_plan).parameters) == ["self", "paths", "profile", "plan", "r", "dt", "n_of", "stop_before",
                                                                           "count_of", "refine_flags", "linear"]
    for fn in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        prm = inspect.signature(fn).parameters
        assert prm["plan_samples"].default is None and prm["plan_agents"].default is None


def test_the_enumerators_equal_the_header():
    txt = open(os.path.join(ROOT, "include", "pqp.h")).read()
    stated = {k: int(v) for k, v in re.findall(r"(PQP_PLAN_[A-Z_]+) = (\d+)", txt)}
    assert stated == dict(PQP_PLAN_EMPTY=P.EMPTY, PQP_PLAN_NOT_FINITE=P.NOT_FINITE, PQP_PLAN_BACKWARD=P.BACKWARD)
    assert all(getattr(capi, k[4:]) == v for k, v in stated.items())
    assert P.REFINED == capi.REFINE_REFINED
    assert len(capi.HEADER.structs) == 10 and list(capi.HEADER.included) == ["pqp_search_params"]      # no new struct anywhere


def test_a_c_file_compiles_the_prototypes(tmp_path):
    src = ('#include "pqp.h"\n'
           "int (*device_form)(pqp_handle*, double, int, int, int, int, int, const double*, const int32_t*, const int32_t*, const double*, int,\n"
           "                   const double*, const int32_t*, const int32_t*, double*, int32_t*, double*, double*, int32_t*) = pqp_sample_plan_device;\n"
           "int (*host_form)(pqp_handle*, double, int, int, int, int, int, const double*, const int32_t*, const int32_t*, const double*, int,\n"
           "                 const double*, const int32_t*, const int32_t*, double*, int32_t*, double*, double*, int32_t*) = pqp_sample_plan;\n"
           "int flags = PQP_PLAN_EMPTY | PQP_PLAN_NOT_FINITE | PQP_PLAN_BACKWARD;\n")
    (tmp_path / "proto.c").write_text(src)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "proto.c", "-o", "proto.o"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:4000]


def test_refused_before_it_touches_a_device(hip_lib):
    """every refusal of the header, in both forms: the arguments are judged before the handle is looked into, so a handle that is only not
    null does for the cases that are bad elsewhere.  The output arrays keep their fill"""
    B, n, m, r = 2, 4, 3, 5
    fake = C.c_void_p(8)
    paths, profile, plan = np.zeros((B, n, 6)), np.zeros((B, n, 4)), np.zeros((B, m, 8))
    good = dict(h=fake, dt=1.0, r=r, linear=0, batch=B, n=n, stride=6, paths=paths, n_of=None, stop_before=None, profile=profile, m=m, plan=plan,
                count_of=None, refine_flags=None)
    bad = [dict(h=None), dict(paths=None), dict(profile=None), dict(plan=None), dict(fine=None), dict(m_of=None), dict(flags=None), dict(batch=0),
           dict(n=0), dict(m=0), dict(r=0), dict(r=-3), dict(stride=5), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")),
           dict(linear=2), dict(linear=-1), dict(m=2 ** 16 + 1, r=2 ** 15)]
    for fn in (hip_lib.pqp_sample_plan_device, hip_lib.pqp_sample_plan):
        for over in bad:
            out = dict(fine=np.full((B, P.fine_count(m, r), 8), 7.0), m_of=np.full(B, 7, np.int32), defect=np.full(B, 7.0), excess=np.full(B, 7.0),
                       flags=np.full(B, 7, np.int32))
            a = dict(good, **out)
            a.update(over)
            assert fn(*a.values()) == -1, over
            assert hip_lib.pqp_last_error().decode().startswith("pqp_sample_plan:"), over
            assert all((v == 7).all() for v in out.values()), over


def test_plan_arguments_of_the_chain_wrapper_are_checked_on_the_host(hip_lib):
    class Stub:
        lib = hip_lib
    se = capi.search_default_params(hip_lib)
    m, r = 8, 10
    agents, fine = np.zeros((2, 3, m, 6)), np.zeros((2, 3, P.fine_count(m, r), 6))
    plan = lambda *a: capi.Handle._plan(Stub, *a)            # (plan_samples, plan_agents, search, agents)
    assert plan(None, None, None, None) is None and plan(None, None, se, agents) is None
    got = plan(r, None, se, agents)
    assert got == (r, None)
    got = plan(np.int64(r), fine, se, agents)
    assert got[0] == r and got[1].shape == fine.shape and got[1].dtype == np.float64
    assert plan(1, np.zeros((2, 3, m, 6)), se, agents)[0] == 1
    for bad in ((None, fine, se, agents), (r, None, None, agents), (0, None, se, agents), (-1, None, se, agents), (2.5, None, se, agents),
                (True, None, se, agents), (r, fine[:1], se, agents), (r, fine[:, :2], se, agents), (r, fine[:, :, :-1], se, agents),
                (r, fine[..., :5], se, agents), (r, agents, se, agents), (2 ** 30, None, se, agents)):
        with pytest.raises(ValueError):
            plan(*bad)


def test_plan_sampler_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("plan_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    S.write_case(path, R.seeded("wait"))
    r = subprocess.run([exe, str(path), "10"], capture_output=True, text=True)
    assert r.returncode == 1 and "no plan sampler" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin"), "10"], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


def test_the_kernel_uses_no_scratch_no_lds_and_spills_nothing(hip_lib):
    """what the build gives today: 64 VGPRs, which is a whole number of the allocation granule of 8, and 8 wavefronts per SIMD.  No LDS, no
    scratch, no spilled register; no atomic: the source has none"""
    r = build_util.find_kernel(build_util.kernel_report(), "plan_sample_kernel")
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size"] == 0, r
    assert r["VGPRs"] <= 64, r
    src = open(os.path.join(ROOT, "path_optimizer_2_amd", "csrc", "pqp_plan_kernels.inc")).read()
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower() and "__shared__" not in code
    assert "st_count(" in code and "st_pose(" in code and "contract(off)" in src        # the search's walk and placement, not a copy of them


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_the_placement_is_the_searchs_pose_at_sigma():
    """refine_util.pose_at, which plan_util places with, gives search_util.stations' poses and envelope on the grid's own stations"""
    for name in ("rest", "tiles", "long"):
        c = R.seeded(name)
        for b in range(len(c["paths"])):
            pick = lambda a: None if a is None else a[b]
            cnt = P.T.driven(c["paths"].shape[1], pick(c.get("n_of")), pick(c.get("stop_before")))
            J, _, pose, venv, _ = S.stations(c["paths"][b], c["profile"][b], cnt, S.params(**c["prm"]))
            got, w = R.pose_at(c["paths"][b], c["profile"][b], cnt, np.arange(J).astype(np.float64) * np.float64(c["prm"]["ds"]))
            assert J > 0 and same_bits(got, pose) and same_bits(np.sqrt(np.fmax(w, 0.0)), venv), (name, b)


def _cases():
    """(name, paths, profile, plan, dt, n_of, stop_before, count_of, refine_flags): refined plans with kept ones among them, and the search's
    staircases with their reached counts"""
    out = []
    for name in ("rest", "quick", "wait", "m3", "m12", "tiles", "long"):
        p = P.refined_plan(name)
        c = p["case"]
        out.append((name, c["paths"], c["profile"], p["traj"], c["prm"]["dt"], c.get("n_of"), c.get("stop_before"), p["res"]["reached"], p["flags"]))
    return out


@pytest.mark.parametrize("r", (1, 3, 10))
def test_the_vectorised_form_is_the_loop(r):
    seen = set()
    for name, paths, profile, plan, dt, n_of, stop, reached, flags in _cases():
        for kw in (dict(refine_flags=flags), dict(linear=False), dict(linear=True)):
            a = P.sample_batch(paths, profile, plan, r, dt, n_of, stop, reached, **kw)
            b = P.sample_batch(paths, profile, plan, r, dt, n_of, stop, reached, one=P.sample_loop, **kw)
            _same(a, b, (name, r, kw))
            assert a["traj"].shape == (len(paths), P.fine_count(plan.shape[1], r), 8)
            seen |= set(a["flags"].tolist())
    assert 0 in seen


def test_the_vectorised_form_is_the_loop_on_the_gpu_tests_synthetic_plans():
    """plan_util.synthetic as tests/test_gpu_plan_sample.py draws it: ragged counts, a stop inside a tile, empty paths, clamped layer counts"""
    n_of = np.array([130, 123, 130, 0, 66, 130], np.int32)
    stop = np.array([130, 130, 86, 130, 40, 0], np.int32)
    count = np.array([5, 1, 2, 5, -3, 9], np.int32)
    c = P.synthetic(6, 130, 5, seed=3, n_of=n_of, stop_before=stop)
    mixed = np.array([R.REFINED, R.KEPT, R.REFINED, R.KEPT | R.INFEASIBLE, 0, R.REFINED], np.int32)
    for kw in (dict(linear=False), dict(linear=True), dict(refine_flags=mixed)):
        a = P.sample_batch(c["paths"], c["profile"], c["plan"], 13, c["dt"], n_of, stop, count, **kw)
        _same(a, P.sample_batch(c["paths"], c["profile"], c["plan"], 13, c["dt"], n_of, stop, count, one=P.sample_loop, **kw), kw)
        assert a["flags"].tolist() == [0, 0, 0, P.EMPTY, P.EMPTY, P.EMPTY] and a["m_of"].tolist() == [53, 1, 14, 0, 0, 0]
    assert a["traj"][0, 52, 4] > c["profile"][0, 129, 0] and same_bits(a["traj"][0, 52, :4], c["paths"][0, 129][[0, 1, 2, 5]])     # past the end: the last waypoint


def test_rows_on_the_layers_are_the_plans_rows():
    """i = 0: x, y, heading, k, s and t of the plan's own row bit for bit, whatever the kinematics; rows behind m_of are zeros"""
    for name, paths, profile, plan, dt, n_of, stop, reached, flags in _cases():
        for r in (1, 7):
            for kw in (dict(refine_flags=flags), dict(linear=True), dict(linear=False)):
                got = P.sample_batch(paths, profile, plan, r, dt, n_of, stop, reached, **kw)
                for b in range(len(paths)):
                    L = int(reached[b])
                    if L == 0:
                        assert got["flags"][b] == P.EMPTY and got["m_of"][b] == 0 and (got["traj"][b] == 0.0).all()
                        continue
                    assert got["m_of"][b] == P.fine_count(L, r)
                    on = got["traj"][b][:got["m_of"][b]:r]
                    assert same_bits(on[:, [0, 1, 2, 3, 4, 7]], plan[b][:L][:, [0, 1, 2, 3, 4, 7]]), (name, b, r, kw)
                    assert (got["traj"][b][got["m_of"][b]:] == 0.0).all()


def test_one_sub_step_returns_a_refined_plan():
    """r = 1 under constant acceleration: all eight columns of a refined plan"""
    count = 0
    for name, paths, profile, plan, dt, n_of, stop, reached, flags in _cases():
        got = P.sample_batch(paths, profile, plan, 1, dt, n_of, stop, reached, refine_flags=flags)
        for b in np.flatnonzero(flags == R.REFINED):
            assert np.array_equal(got["traj"][b], plan[b]), (name, b)
            count += 1
    assert count >= 10


def test_a_refined_plan_follows_its_own_kinematics():
    """the defect of every refined plan finished from the emulation's x is below plan_util.defect_bound, which follows from
    refine_util.KKT_WORST's primal residual; the samples between two layers lie between their stations, speeds are not negative"""
    worst = 0.0
    for name in R.QP_CASES:
        p = P.refined_plan(name)
        c = p["case"]
        dt = c["prm"]["dt"]
        got = P.sample_batch(c["paths"], c["profile"], p["traj"], 10, dt, c.get("n_of"), c.get("stop_before"), p["res"]["reached"], refine_flags=p["flags"])
        for b in np.flatnonzero(p["flags"] == R.REFINED):
            bound = P.defect_bound(dt, p["traj"][b][:, 4].max())
            print(f"{name} path {b}: m = {p['m']}, defect {got['defect'][b]:.3e} (bound {bound:.3e}), excess {got['excess'][b]:.3e}")
            assert 0.0 <= got["defect"][b] <= bound, (name, b, got["defect"][b], bound)
            worst = max(worst, float(got["defect"][b]))
            s = got["traj"][b][:, 4]
            assert (np.diff(s) >= 0.0).all() and (got["traj"][b][:, 5] >= 0.0).all() and got["flags"][b] == 0, (name, b)
            assert got["excess"][b] >= R.rows_at(c["paths"][b], c["profile"][b], R.T.driven(c["paths"].shape[1], None if c.get("n_of") is None else c["n_of"][b],
                                                 None if c.get("stop_before") is None else c["stop_before"][b]), p["traj"][b][:, 4], p["traj"][b][:, 5],
                                                 p["traj"][b][:, 6], dt)[1], (name, b)        # the layers are among the samples
    print(f"worst defect {worst:.3e}")
    assert worst > 0.0


def test_a_staircase_is_linear_and_not_of_constant_acceleration():
    """the search's rows: s_{k+1} - s_k = q_{k+1} ds while the constant-acceleration row predicts (q_k + q_{k+1}) ds / 2, so the defect is
    max |q_{k+1} - q_k| ds / 2 - exactly, on the hand road's dyadic grid.  Linearly the defect is 0 and every sample lies in [s_k, s_{k+1}]"""
    c, res, m = R.searched("rest")
    ds, dt = c["prm"]["ds"], c["prm"]["dt"]
    plan, q = res["traj"], res["steps"][0][:, 1]
    assert int(res["reached"][0]) == m
    cacc = P.sample_batch(c["paths"], c["profile"], plan, 10, dt, linear=False)
    assert cacc["defect"][0] == 0.5 * np.abs(np.diff(q)).max() * ds > 0.0
    lin = P.sample_batch(c["paths"], c["profile"], plan, 10, dt, linear=True)
    assert lin["defect"][0] == 0.0 and lin["flags"][0] == 0 and lin["m_of"][0] == P.fine_count(m, 10)
    s = lin["traj"][0][:, 4]
    for f in range(P.fine_count(m, 10) - 1):
        k = f // 10
        assert plan[0, k, 4] <= s[f] <= plan[0, k + 1, 4] and lin["traj"][0][f, 5] == (plan[0, k + 1, 4] - plan[0, k, 4]) / dt and lin["traj"][0][f, 6] == 0.0
    # given the refine's flags, a kept path is sampled linearly and a refined one is not
    p = P.refined_plan("quick")
    assert p["flags"].tolist() == [R.KEPT | R.INFEASIBLE]
    c = p["case"]
    kept = P.sample_batch(c["paths"], c["profile"], p["traj"], 4, dt, refine_flags=p["flags"])
    _same(kept, P.sample_batch(c["paths"], c["profile"], p["traj"], 4, dt, linear=True), "kept")


def test_empty_not_finite_and_backward():
    c, res, m = R.searched("rest")
    path, profile, plan, dt = c["paths"][0], c["profile"][0], res["traj"][0], c["prm"]["dt"]
    M = P.fine_count(m, 3)
    for kw in (dict(n_of=0), dict(stop_before=0), dict(count=0), dict(count=-4)):
        got = P.sample(path, profile, plan, 3, dt, **kw)
        assert got["flags"] == P.EMPTY and got["m_of"] == 0 and (got["traj"] == 0.0).all() and np.isnan(got["defect"]) and np.isnan(got["excess"])
    one = P.sample(path, profile, plan, 3, dt, count=1)
    assert one["flags"] == 0 and one["m_of"] == 1 and one["defect"] == 0.0 and same_bits(one["traj"][0], plan[0]) and (one["traj"][1:] == 0.0).all()
    for where, col in (("path", 1), ("path", 5), ("profile", 2), ("plan", 4), ("plan", 5), ("plan", 6)):
        arrays = dict(path=path.copy(), profile=profile.copy(), plan=plan.copy())
        arrays[where][2, col] = np.inf
        got = P.sample(arrays["path"], arrays["profile"], arrays["plan"], 3, dt)
        assert got["flags"] == P.NOT_FINITE and got["m_of"] == 0 and np.isnan(got["traj"]).all() and got["traj"].shape == (M, 8), (where, col)
        assert P.sample(arrays["path"], arrays["profile"], arrays["plan"], 3, dt, n_of=2, count=2)["flags"] == 0        # behind the counts: not read
    arrays = dict(path=path.copy(), plan=plan.copy())
    arrays["path"][2, 3], arrays["path"][2, 4], arrays["plan"][2, 0], arrays["plan"][2, 7] = np.nan, np.nan, np.nan, np.nan       # columns nobody reads
    _same(P.sample(arrays["path"], profile, arrays["plan"], 3, dt), P.sample(path, profile, plan, 3, dt), "unread columns")
    back = plan.copy()
    back[4, 4] = back[3, 4] - 1.0
    for linear in (False, True):
        got = P.sample(path, profile, back, 3, dt, linear=linear)
        assert got["flags"] == P.BACKWARD and (got["traj"][9:12, 4] == back[3, 4]).all() and got["m_of"] == M
        assert P.sample(path, profile, back, 3, dt, count=4, linear=linear)["flags"] == 0


# ---- the hand case: a disc that crosses the lane between two layers ------------------------------------------------------------------------------
def test_a_disc_crossing_between_two_layers_is_seen_on_the_fine_steps_only():
    """refine_util's road at heading 0 (sin and cos are exact), the refined plan from rest, plan_util.crossing()'s disc.  The m rows pass
    agents_util's check against the disc at the layers; the fine rows at r = 10 against the disc on the fine steps are hit first at sample
    34.  No |clear - margin| of any sample is below 1e-6, so the device's sincos cannot move either verdict"""
    x = P.crossing()
    c, m, r = x["case"], x["m"], P.CROSS_R
    assert x["flags"].tolist() == [R.REFINED] and (c["paths"][0][:, 2] == 0.0).all()
    circles = R.circles_of("rest")
    coarse = A.check(x["plan"], x["coarse_agents"], circles)
    assert coarse["first_hit"].tolist() == [m] and coarse["hit_agent"].tolist() == [-1]
    fine = P.sample_batch(c["paths"], c["profile"], x["plan"], r, c["prm"]["dt"], refine_flags=x["flags"])
    assert fine["m_of"].tolist() == [P.fine_count(m, r)] == [71] and (fine["traj"][0][:, 2] == 0.0).all()
    assert same_bits(x["coarse_agents"][0, 0], x["fine_agents"][0, 0, ::r])
    got = A.check(fine["traj"], x["fine_agents"], circles, m_of=fine["m_of"])
    assert got["first_hit"].tolist() == [P.CROSS_FIRST_HIT] and got["hit_agent"].tolist() == [0]
    hits = np.flatnonzero(got["clear"][0][:, 0] < 0.0)
    assert hits.tolist() == [34, 35, 36]                     # t = 3.4 .. 3.6 s: between layers 3 and 4
    every = np.concatenate([coarse["clear"][0].ravel(), got["clear"][0].ravel()])
    assert every.size == m + 71 and np.isfinite(every).all() and np.abs(every - 0.0).min() >= 1e-6, np.abs(every).min()
    # the same plan sampled linearly, as a kept path would be, is hit too: the verdict does not hang on the kinematics here
    lin = P.sample_batch(c["paths"], c["profile"], x["plan"], r, c["prm"]["dt"], linear=True)
    assert A.check(lin["traj"], x["fine_agents"], circles, m_of=lin["m_of"])["first_hit"].tolist() == [P.CROSS_FIRST_HIT]
