"""pqp_stitch_trajectory without a device: the restatement of tests/stitch_util.py held against a plain per-row loop and against what a
stitch must do by construction (the state row is a row of the plan, the prefix is the plan re-based, the deviations of a car displaced
from a known arc come back), the margins of every case the GPU test runs, the binding, every refusal, the chain's plan with previous=,
the header-only TrajectoryStitcher and the kernel's resources."""
import ctypes as C
import inspect
import math
import subprocess

import numpy as np
import pytest

import build_util
import chain_plan_cases as cases
import cpp_demo
import stitch_util as U
from path_optimizer_2_amd import capi
from shared_util import same_bits

NAMES = ("pqp_stitch_trajectory", "pqp_stitch_trajectory_device")
CASES = U.device_cases()


def _against_the_loop(c):
    got = U.run_case(c)
    G, m = c["prev"].shape[:2]
    cap = m if c["prefix_max"] is None else c["prefix_max"]
    for g in range(G):
        M = m if c["m_of"] is None else min(max(int(c["m_of"][g]), 0), m)
        state, flags, dev, idx, prefix = U.stitch_group_loop(c["prev"][g, :M], c["meas"][g], c["t_now"][g], c["prm"], c["keep"], cap)
        assert flags == got["flags"][g] and idx == got["idx"][g].tolist(), (c["name"], g, flags, got["flags"][g], idx)
        assert same_bits(np.array(state), got["state"][g]) and same_bits(np.array(dev), got["dev"][g]), (c["name"], g)
        assert len(prefix) == got["prefix_n"][g]
        assert same_bits(np.array(prefix).reshape(-1, 8), got["prefix"][g, :len(prefix)]) and not got["prefix"][g, len(prefix):].any()
    return got


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_against_a_plain_loop(c):
    _against_the_loop(c)


def test_hand_cases_one_per_flag_and_pairs_of_reasons():
    plan = U.arc_plan(40, dt=0.125, t0=1.0)
    on = lambda lon=0.0, lat=0.0, dh=0.0, **kw: U.displaced(plan[8], lon, lat, dh, **kw)
    t8 = plan[8, 7]
    prm = (0.13,) + U.DEFAULT[1:]
    one = lambda rows, meas, t, **kw: U.stitch_group(rows, meas, t, kw.pop("prm", prm), **kw)
    R, S = U.REPLAN, U.STITCHED
    nan_meas = on(); nan_meas[4] = math.nan
    hole = plan.copy(); hole[8, 2] = math.nan
    flat = plan.copy(); flat[:, :2] = math.nan
    assert one(plan, on(0.1, 0.1, 0.1), t8)["flags"] == S
    assert one(plan, on(), t8, keep=2, prefix_max=3)["flags"] == S | U.PREFIX_CUT
    assert one(plan, nan_meas, t8)["flags"] == U.BAD
    assert one(plan, on(v=-1.0), t8)["flags"] == U.BAD
    assert one(plan, on(), math.inf)["flags"] == U.BAD
    assert one(plan[:1], on(), t8)["flags"] == U.NO_PREVIOUS | R
    assert one(plan[:0], on(), t8)["flags"] == U.NO_PREVIOUS | R
    assert one(plan, U.displaced(plan[0], 0.0, 0.0, 0.0), plan[0, 7] - 0.5)["flags"] == U.TIME | R
    assert one(plan, U.displaced(plan[-1], 0.0, 0.0, 0.0), plan[-1, 7])["flags"] == U.TIME | R          # no row at t_now + t_ahead
    assert one(hole, on(), t8)["flags"] == U.BAD_PLAN | R
    assert one(flat, on(), t8)["flags"] == U.BAD_PLAN | R and one(flat, on(), t8)["idx"][1] == -1
    assert one(plan, on(lat=0.6), t8)["flags"] == U.LATERAL | R
    assert one(plan, on(lon=2.6), t8)["flags"] == U.LONGITUDINAL | R
    assert one(plan, on(dh=-0.6), t8)["flags"] == U.HEADING | R
    assert one(plan, on(lat=-0.6, dh=0.6), t8)["flags"] == U.LATERAL | U.HEADING | R
    assert one(plan, on(lon=-2.6, lat=0.6), t8)["flags"] == U.LONGITUDINAL | U.LATERAL | R
    assert one(plan, U.displaced(plan[0], 0.0, 0.6, 0.0), plan[0, 7] - 0.5)["flags"] == U.TIME | U.LATERAL | R
    assert one(plan, on(lat=0.6), plan[0, 7] - 0.5)["flags"] == U.TIME | U.LATERAL | U.LONGITUDINAL | R      # s_ref is s_0, the car is at row 8
    assert one(hole, on(), plan[-1, 7] + 1.0)["flags"] == U.TIME | U.BAD_PLAN | R
    assert one(plan, on(lat=0.6, v=0.0), t8)["flags"] == U.LATERAL | R | U.STANDING
    assert one(plan, on(lat=0.6, v=0.1, a=-2.0), t8)["flags"] == U.LATERAL | R | U.STANDING            # stops inside t_ahead
    # the replanned state row: x, y, heading by the free model, k = w / ve above v_still and 0 at or below it, a_e, the instant
    r = one(plan, on(lat=0.6, v=4.0, a=0.5, w=0.2), t8)
    ve = 4.0 + 0.5 * 0.13
    assert r["state"][3:].tolist() == [0.2 / ve, 0.0, ve, 0.5, t8 + 0.13] and r["prefix"].tolist() == [r["state"][:7].tolist() + [0.0]]
    assert one(plan, on(lat=0.6, v=0.1, w=0.2), t8)["state"][3] == 0.0 and one(plan, on(lat=0.6, v=0.11, w=0.2), t8)["state"][3] == 0.2 / 0.11
    capped = one(plan, on(lat=0.6, v=4.0, a=0.5), t8, prm=prm[:5] + (4.01,))
    assert capped["state"][5] == 4.01 and capped["state"][6] == 0.0
    straight = one(plan, U.displaced(np.array([1.0, 2.0, 0.0, 0, 0, 0, 0, 0]), 0.0, 0.0, 0.0, v=2.0), 50.0)      # past the plan: from (1, 2) along x
    assert straight["flags"] == U.TIME | R and not straight["dev"].any() and straight["idx"].tolist()[0::2] == [-1, -1]      # no i_now: no deviations
    assert straight["state"][:3].tolist() == [1.0 + 2.0 * 0.13, 2.0, 0.0]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_a_stitched_state_is_a_row_of_the_plan_and_the_prefix_is_the_plan_rebased(c):
    got = U.run_case(c)
    stitched = np.flatnonzero(got["flags"] & U.STITCHED)
    for g in stitched:
        i_now, _, i_start = got["idx"][g]
        n = got["prefix_n"][g]
        rows, piece = c["prev"][g, :, :8], got["prefix"][g, :n]
        assert same_bits(got["state"][g], rows[i_start])
        i0 = i_start - n + 1
        assert n >= 1 and i0 >= 0 and (i0 == max(0, i_now - c["keep"]) or got["flags"][g] & U.PREFIX_CUT)
        assert piece[-1, 4] == 0.0 and piece[-1, 7] == 0.0
        assert same_bits(piece[:, [0, 1, 2, 3, 5, 6]], rows[i0:i_start + 1][:, [0, 1, 2, 3, 5, 6]])
        assert same_bits(piece[:, 4], rows[i0:i_start + 1, 4] - rows[i_start, 4]) and same_bits(piece[:, 7], rows[i0:i_start + 1, 7] - rows[i_start, 7])
        assert not got["prefix"][g, n:].any()
        assert got["state"][g, 7] >= c["t_now"][g] + c["prm"][0]
    replanned = np.flatnonzero(got["flags"] & U.REPLAN)
    assert (got["prefix_n"][replanned] == 1).all() and (got["state"][replanned, 4] == 0.0).all()
    assert same_bits(got["state"][replanned, 7], c["t_now"][replanned] + c["prm"][0])
    bad = np.flatnonzero(got["flags"] & U.BAD)
    assert (got["flags"][bad] == U.BAD).all() and not got["state"][bad].any() and not got["prefix_n"][bad].any()
    assert not ((got["flags"] & U.STITCHED != 0) & (got["flags"] & (U.REPLAN | U.BAD) != 0)).any()
    assert np.isfinite(got["start"]).all() and np.isfinite(got["start_k"]).all() and np.isfinite(got["v_start"]).all()      # no NaN goes on to the chain


def test_every_device_case_keeps_its_margins():
    """every comparison a flag hangs on, in every case the GPU test runs, none left out, is at least 1e-6 from going the other way: the
    device's sincos (1e-9 m at these coordinates) cannot move a flag, so the GPU test may ask for the flags' bits.  A time that lies
    exactly on a row's is a comparison of equal bits and needs no margin; tq is one addition of the same two doubles on both sides."""
    seen = 0
    for c in CASES:
        margins = U.run_case(c)["margins"]
        assert margins.shape == (c["prev"].shape[0], 6)
        assert (margins >= 1e-6).all(), (c["name"], margins.min(axis=0))
        seen += int(np.isfinite(margins).sum())
    assert seen > 1000


@pytest.mark.parametrize("curvature", [0.02, -0.05, 0.0])
def test_known_deviations_from_a_known_arc_come_back(curvature):
    """a car `lon` behind where the plan wants it at t_now, `lat` to the left of the arc and turned by `dh` against its tangent.  The
    kernel measures in the frame of the nearest row, an arc length d <= half a row spacing h from the car's foot point, so the frame is
    turned by theta = |k| d against the tangent there:  |lat error| <= (1 - cos theta)(1 / |k| + |lat|) <= |k| d^2 / 2 (1 + |k lat|),
    |lon error| <= (d - sin theta / |k|) + |lat| sin theta + a dt^2 / 8 (s_ref is a chord of s(t)) <= k^2 d^3 / 6 + |k lat| d + a dt^2 / 8,
    |dh error| = theta = |k| d."""
    v, a, dt, m = 8.0, 0.5, 0.1, 71
    plan = U.arc_plan(m, dt, v=v, a=a, curvature=curvature)
    h = float(np.diff(plan[:, 4]).max())
    d = 0.5 * h * 1.05
    k = abs(curvature)
    for lon, lat, dh in ((0.0, 0.0, 0.0), (0.3, 0.2, 0.1), (-1.7, -0.4, -0.3), (2.2, 0.45, 0.4)):
        for t_now in (plan[20, 7], plan[20, 7] + 0.037, plan[33, 7] + 0.08):
            tau = t_now - plan[0, 7]
            s_car = v * tau + 0.5 * a * tau * tau - lon                                  # where the car's foot point is on the arc
            tau_c = (-v + math.sqrt(v * v + 2.0 * a * s_car)) / a
            foot = U.arc_plan(2, tau_c, v=v, a=a, curvature=curvature)[1]                # the arc's own point at that length
            meas = U.displaced(foot, 0.0, lat, dh)
            got = U.stitch_group(plan, meas, t_now)
            assert got["flags"] == U.STITCHED, (lon, lat, dh, got["flags"])
            e_lon, e_lat, e_dh = np.abs(got["dev"] - (lon, lat, dh))
            assert e_lat <= 0.5 * k * d * d * (1.0 + k * abs(lat)) + 1e-9, (e_lat, lon, lat, dh)
            assert e_lon <= k * k * d ** 3 / 6.0 + k * abs(lat) * d + a * dt * dt / 8.0 + 1e-9, (e_lon, lon, lat, dh)
            assert e_dh <= k * d + 1e-9, (e_dh, lon, lat, dh)


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
PARAMS = ["h", "prm", "keep", "prefix_max", "groups", "m", "stride", "prev", "m_of", "meas", "t_now", "batch", "group_start", "state", "flags", "dev",
          "idx", "prefix", "prefix_n", "start", "start_k", "v_start"]


def test_symbols_constants_and_defaults(hip_lib):
    assert set(NAMES + ("pqp_stitch_default_params",)) <= set(capi.EXPORTS) and all(hasattr(hip_lib, n) for n in NAMES)
    for name in NAMES:
        assert [q.name for q in capi.HEADER.functions[name].params] == PARAMS
    assert not any(s.startswith("pqp_stitch") for s in capi.HEADER.structs)              # six plain doubles, no struct
    assert capi.STITCH_PARAMS == 6
    assert [getattr(capi, "STITCH_" + n) for n in ("T_AHEAD", "LAT_MAX", "LON_MAX", "DH_MAX", "V_STILL", "V_CAP")] == list(range(6))
    names = ("BAD", "NO_PREVIOUS", "TIME", "BAD_PLAN", "LATERAL", "LONGITUDINAL", "HEADING", "REPLAN", "STITCHED", "PREFIX_CUT", "STANDING")
    assert [getattr(capi, "STITCH_" + n) for n in names] == [getattr(U, n) for n in names] == [1 << k for k in range(11)]
    p = capi.stitch_default_params(hip_lib)
    assert p.array().tolist() == list(U.DEFAULT) == [0.1, 0.5, 2.5, 0.5, 0.1, math.inf] and p.keep == U.KEEP == 20
    q = capi.stitch_default_params(hip_lib, lat_max=0.25, keep=3)
    assert q.array().tolist() == [0.1, 0.25, 2.5, 0.5, 0.1, math.inf] and q.keep == 3
    hip_lib.pqp_stitch_default_params(None, None)                                        # NULL pointers are ignored
    assert list(inspect.signature(capi.Handle.stitch_trajectory).parameters) == \
        ["self", "prev", "meas", "t_now", "m_of", "group_start", "batch", "prm", "prefix_max"]
    for f in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        names = list(inspect.signature(f).parameters)
        assert names[-7:-4] == ["previous", "parked", "rank"] and names[3] == "start"          # in front of rank, and of parked, which a test pins there


def _call(lib, form, handle, **over):
    """one call with a single argument changed from a set the library would accept; never sent with none changed: `h` is not a handle"""
    G, m, B = 3, 4, 5
    a = dict(prm=np.array(U.DEFAULT), keep=2, prefix_max=m, groups=G, m=m, stride=8, prev=np.zeros((G, m, 8)), m_of=np.full(G, m, np.int32),
             meas=np.zeros((G, 6)), t_now=np.zeros(G), batch=B, group_start=np.array([0, 2, 2, 5], np.int32), state=np.full((G, 8), 7.0),
             flags=np.full(G, 7, np.int32), dev=np.full((G, 3), 7.0), idx=np.full((G, 3), 7, np.int32), prefix=np.full((G, m, 8), 7.0),
             prefix_n=np.full(G, 7, np.int32), start=np.full((B, 3), 7.0), start_k=np.full(B, 7.0), v_start=np.full(B, 7.0))
    assert over and set(over) <= set(a) | {"h"}
    a.update(over)
    rc = getattr(lib, form)(over.get("h", handle), *[a[k] for k in PARAMS[1:]])
    untouched = all((a[k] == 7).all() for k in ("state", "flags", "dev", "idx", "prefix", "prefix_n", "start", "start_k", "v_start") if a[k] is not None)
    return rc, untouched, lib.pqp_last_error().decode()


REFUSALS = [dict(h=None), dict(prm=None), dict(prev=None), dict(meas=None), dict(t_now=None), dict(state=None), dict(flags=None), dict(dev=None),
            dict(idx=None), dict(prefix_n=None), dict(groups=0), dict(m=0), dict(stride=7), dict(batch=-1), dict(keep=-1), dict(prefix_max=0),
            dict(group_start=None), dict(group_start=None, batch=4, v_start=None, start_k=None)] + \
           [dict(prm=np.array(U.DEFAULT[:k] + (bad,) + U.DEFAULT[k + 1:])) for k in range(6) for bad in (-0.5, math.nan)] + \
           [dict(prm=np.array((math.inf,) + U.DEFAULT[1:])), dict(prm=np.array(U.DEFAULT[:4] + (math.inf, math.inf)))]
HOST_REFUSALS = [dict(group_start=np.array([1, 2, 2, 5], np.int32)), dict(group_start=np.array([0, 2, 2, 4], np.int32)),
                 dict(group_start=np.array([0, 3, 2, 5], np.int32))]


def test_every_refusal_comes_before_the_device(hip_lib):
    """both forms check everything before they look into the handle, so a pointer that is no handle shows the refusals here"""
    no_handle = C.create_string_buffer(4096)
    for form in NAMES:
        for over in REFUSALS:
            rc, untouched, msg = _call(hip_lib, form, no_handle, **over)
            assert rc == -1 and untouched and msg.startswith("pqp_stitch_trajectory:"), (form, over, rc, msg)
    for over in HOST_REFUSALS:
        rc, untouched, msg = _call(hip_lib, NAMES[0], no_handle, **over)
        assert rc == -1 and untouched and msg.startswith("pqp_stitch_trajectory: group_start"), (over, rc, msg)


def test_the_wrapper_s_own_refusals(hip_lib):
    h = object.__new__(capi.Handle)
    h.lib = hip_lib
    prev, meas, t = np.zeros((3, 4, 8)), np.zeros((3, 6)), np.zeros(3)
    for args, kw, what in (((prev[0], meas, t), {}, r"prev must be \[G\]\[m\]\[stride\]"), ((prev, meas[:2], t), {}, "meas must be"),
                           ((prev, meas, t[:2]), {}, "t_now must have 3"), ((prev, meas, t), dict(m_of=[1, 2]), "m_of must have 3"),
                           ((prev, meas, t), dict(group_start=[0, 1, 2, 3]), "needs batch"),
                           ((prev, meas, t), dict(group_start=[0, 3], batch=3), "needs batch and 4 entries"),
                           ((prev, meas, t), dict(group_start=[0, 1, 2, 4], batch=3), "must ascend from 0 to the batch")):
        with pytest.raises(ValueError, match=what):
            h.stitch_trajectory(*args, **kw)
    with pytest.raises(C.ArgumentError, match="wants a C-contiguous float64 array"):
        hip_lib.pqp_stitch_trajectory(None, np.zeros(6, np.float32), 0, 1, 1, 2, 8, None, None, None, None, 1, None, None, None, None, None, None,
                                      None, None, None, None)


# ---- the chain's plan ---------------------------------------------------------------------------------------------------------------------------
def _plan(lib, kw):
    h = capi.Handle.__new__(capi.Handle)
    h.lib = lib
    cfg = capi._defaults(lib, capi.PqpChainConfig, "pqp_chain_default_config", cases.CHAIN_CONFIG)
    return h._chain_plan(points=np.zeros((cases.B, 9, 2)), cfg=cfg, **kw)


def _previous(groups, m=6, prm=None):
    return (np.zeros((groups, m, 8)), np.full(groups, m, np.int32), np.zeros((groups, 6)), np.zeros(groups), prm)


STITCH_KEYS = [("stitch_state", (3, 8), "float64"), ("stitch_flags", (3,), "int32"), ("stitch_dev", (3, 3), "float64"),
               ("stitch_prefix", (3, 6, 8), "float64"), ("stitch_prefix_n", (3,), "int32")]


def test_the_chain_s_plan_with_previous(hip_lib):
    cf = cases.configs(hip_lib)
    without = lambda kw, *names: {k: v for k, v in kw.items() if k not in names}
    # rank=: the groups are the ranking's, v_start a row per candidate; the keys stand behind every existing key
    j = without(cf["j"][1], "v_start")
    base, plan = _plan(hip_lib, cf["j"][1]), _plan(hip_lib, dict(j, previous=_previous(cases.GROUPS)))
    assert plan.result == base.result + STITCH_KEYS and plan.on_device == base.on_device
    stage = plan.stages[0]
    assert [s[:3] for s in stage.scratch] == [("stitch_idx", (3, 3), "int32"), ("start", (4, 3), "float64"), ("start_k", (4,), "float64"),
                                              ("v_start", (4,), "float64")]
    assert [u[0] for u in stage.uploads] == ["stitch_prev", "stitch_prev_m", "stitch_meas", "stitch_t_now", "stitch_group_start"]
    assert stage.uploads[4][1].tolist() == cases.GROUP_START and plan.previous[4].keep == 20
    # select= with speed=: the profile runs on the winners, v_start is a row per group
    hcase = without(cf["h"][1], "v_start")
    plan = _plan(hip_lib, dict(hcase, previous=_previous(cases.GROUPS, prm=capi.stitch_default_params(hip_lib, keep=2))))
    assert plan.stages[0].scratch[3][:3] == ("v_start", (3,), "float64") and plan.previous[4].keep == 2
    assert plan.result == _plan(hip_lib, cf["h"][1]).result + STITCH_KEYS
    # neither: one group per candidate, no group_start, and without speed= no v_start
    plan = _plan(hip_lib, dict(previous=_previous(cases.B)))
    assert [k for k, _, _ in plan.result][-5:] == [k for k, _, _ in STITCH_KEYS] and plan.result[-5][1] == (4, 8)
    assert plan.stages[0].uploads[4][1] is None and [s[0] for s in plan.stages[0].scratch] == ["stitch_idx", "start", "start_k"]
    # parked= keeps its place in front, and its key in front of the stitch's
    parked = (np.zeros((2, 1, 6)), None, None)
    geom = capi.PqpGridGeometry()
    plan = _plan(hip_lib, dict(previous=_previous(cases.B), parked=parked, geom=geom))
    assert [k for k, _, _ in plan.result][-6] == "parked_flags" and plan.stages[1] is not None and plan.stages[1].scratch[0][0] == "stitch_idx"
    # a call without previous= is what it was
    assert base.previous is None and not any(k.startswith("stitch") for k, _, _ in base.result)


def test_the_chain_s_refusals_with_previous(hip_lib):
    cf = cases.configs(hip_lib)
    j = {k: v for k, v in cf["j"][1].items() if k != "v_start"}
    for extra, what in ((dict(start=np.zeros((4, 3))), "refused together with start"), (dict(start_k=np.zeros(4)), "refused together with start"),
                        (dict(v_start=np.zeros(4)), "refused together with start")):
        with pytest.raises(ValueError, match=what):
            _plan(hip_lib, dict(j, previous=_previous(cases.GROUPS), **extra))
    for previous, what in ((_previous(cases.GROUPS)[:4], "previous must be"), (_previous(cases.B), r"prev must be \[3\]"),
                           ((np.zeros((3, 6, 7)),) + _previous(3)[1:], "stride >= 8"), (_previous(3)[:1] + (np.zeros(2, np.int32),) + _previous(3)[2:], "one per group"),
                           (_previous(3)[:2] + (np.zeros((3, 5)),) + _previous(3)[3:], "one per group"), (_previous(3)[:3] + (np.zeros(4), None), "one per group"),
                           (_previous(3)[:4] + ("params",), "must be a StitchParams")):
        with pytest.raises(ValueError, match=what):
            _plan(hip_lib, dict(j, previous=previous))
    with pytest.raises(ValueError, match=r"prev must be \[4\].*a plan per candidate"):
        _plan(hip_lib, dict(previous=_previous(3)))
    with pytest.raises(ValueError, match="speed needs v_start"):
        _plan(hip_lib, j)                                                              # without previous= the speed profile still needs its v_start


# ---- the C++ class, the kernel -------------------------------------------------------------------------------------------------------------------
def test_stitcher_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("stitch_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    c = U.seeded_case(2, 5, seed=3)
    U.write_case(path, c["prev"], 0.1, c["m_of"], c["meas"], c["t_now"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no trajectory stitcher" in r.stderr
    (tmp_path / "short.bin").write_bytes(open(path, "rb").read()[:100])
    r = subprocess.run([exe, str(tmp_path / "short.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "short or bad file" in r.stderr


def test_the_kernel_uses_no_scratch_and_no_lds(hip_lib):
    """one wavefront per group: the measurement, the matches and the state row live in registers - 107 VGPRs as the build stands, read
    here and not pinned (most of them are the free model's, which only a replanned group runs) - and the matches meet through ballots and
    DPP, so there is no LDS; no register is spilled to memory and nothing sizes a stack"""
    r = build_util.find_kernel(build_util.kernel_report(), "stitch_trajectory_kernel")
    print("stitch_trajectory_kernel:", r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert 0 < r["VGPRs"] <= 512
