"""pqp_predict_agents without a GPU: the restatement of include/pqp.h's definition (tests/predict_util.py) against an RK4 integration of
the motion, hand cases on dyadic numbers, the time grid, the struct-free ABI and the binding's argument checks."""
import math
import subprocess

import numpy as np
import pytest

import cpp_demo
import predict_util as U
from path_optimizer_2_amd import capi

HORIZON_M = 14                     # layers a second apart: 13 s

# free-model tracks (x, y, heading, v, a, yaw rate) and what each one is there for
RK4_CASES = {
    "brakes_to_a_stop_at_6s": (1.0, 2.0, 0.3, 12.0, -2.0, 0.1),
    "reaches_the_cap_at_4s": (-3.0, 4.0, -1.0, 34.0, 1.5, -0.05),
    "constant_speed_on_a_circle": (0.0, 0.0, 2.0, 10.0, 0.0, 0.2),
    "accelerates_turning_left": (5.0, -5.0, 0.5, 5.0, 1.0, 0.3),
    "accelerates_turning_right": (5.0, -5.0, 0.5, 5.0, 1.0, -0.3),
    "straight_braking_dyadic": (2.0, 1.0, 0.0, 8.0, -2.0, 0.0),
    "straight_constant_dyadic": (2.0, 1.0, 0.0, 4.0, 0.0, 0.0),
    # te = 1 s from the first layer on (38 -> 40 m/s at 2 m/s^2), so |w te| is just below and just above the switch at every later step
    "below_the_switch": (0.0, 0.0, 0.25, 38.0, 2.0, 2.0 ** -6 * (1.0 - 2.0 ** -20)),
    "above_the_switch": (0.0, 0.0, 0.25, 38.0, 2.0, 2.0 ** -6 * (1.0 + 2.0 ** -20)),
    "above_the_switch_right": (0.0, 0.0, 0.25, 38.0, 2.0, -(2.0 ** -6) * (1.0 + 2.0 ** -20)),
}


def _estimate(track, times, delta):
    coarse, fine = U.integrate(track, times, U.V_CAP, delta), U.integrate(track, times, U.V_CAP, 0.5 * delta)
    return fine, float(np.hypot(fine[:, 0] - coarse[:, 0], fine[:, 1] - coarse[:, 1]).max())


@pytest.mark.parametrize("name", sorted(RK4_CASES))
def test_restatement_against_rk4(name):
    """The closed forms against x' = v cos h, y' = v sin h, h' = w [v > 0], v' = a until the stop or the cap, integrated by RK4 at step
    sizes delta and delta / 2 on the pieces between the sample times and the event.  The difference of the two integrations is the
    integrator's own error estimate; the restatement must lie within 4 x that estimate of the finer one, at every step.  delta is, per
    case, the first of 1, 1/2, 1/4, ... s whose estimate is below 1e-9 m: coarse on purpose, so that the estimate is the integrator's
    truncation and not fp64 noise.  (The two straight cases run on dyadic numbers at heading 0, where RK4 is exact in fp64 and so is the
    restatement: estimate 0, difference 0.)  Largest estimate over the cases: 8.4e-10 m (the three at the switch, delta 1/2 s); largest
    restatement-to-RK4 distance 5.6e-11 m.  The heading is linear in time, which RK4 integrates exactly: it is held to 1e-13 rad, a few
    roundings of a value below 8 rad."""
    track = RK4_CASES[name] + (2.0, 1.0, 0.25)
    times = [U.step_time(0.0, 1.0, 1, f) for f in range(HORIZON_M)]
    delta = 1.0
    while True:
        fine, est = _estimate(track, times, delta)
        if est < 1e-9:
            break
        delta *= 0.5
    rows, flags, _ = U.predict_track(track, 0.0, 1.0, HORIZON_M, 1)
    off = float(np.hypot(rows[:, 0] - fine[:, 0], rows[:, 1] - fine[:, 1]).max())
    print(f"{name}: delta {delta} s, estimate {est:.3e} m, restatement to RK4 {off:.3e} m")
    assert off <= 4.0 * est, (name, delta, est, off)
    wrapped = np.array([capi_free_angle(h) for h in fine[:, 2]])
    assert np.abs(np.angle(np.exp(1j * (rows[:, 2] - wrapped)))).max() < 1e-13
    assert bool(flags & U.STOPS) == (name in ("brakes_to_a_stop_at_6s", "straight_braking_dyadic"))
    assert bool(flags & U.CAPPED) == ("cap" in name or "switch" in name)


def capi_free_angle(a):
    import corridor_oracle as K
    return K.constrain_angle(a)


def test_the_two_forms_of_each_function_agree_at_the_switch():
    """sinc, cosc, f1 and f2 by their closed forms and by their polynomials at |th| = 2^-6 and one ulp below, both signs.  The bound:
    the first term the polynomial leaves out (th^6 / 5040 = 2.9e-15 for sinc, th^6 / 5760 for f1, th^7 / 40320 and th^7 / 45360 for
    the odd pair) plus the closed form's rounding, largest for f2, whose numerator sin th - th cos th loses th^2 to cancellation:
    3 ulp(2^-6) / 2^-12 = 4.3e-14.  Measured gaps: sinc 2.9e-15, cosc 4.3e-18, f1 2.6e-15, f2 2.6e-15."""
    gaps = np.zeros(4)
    for th in (2.0 ** -6, np.nextafter(2.0 ** -6, 0.0), -(2.0 ** -6), -np.nextafter(2.0 ** -6, 0.0)):
        gaps = np.maximum(gaps, np.abs(np.array(U.closed(float(th))) - np.array(U.taylor(float(th)))))
    print("gaps at the switch: sinc %.2e cosc %.2e f1 %.2e f2 %.2e" % tuple(gaps))
    assert (gaps <= 5e-14).all(), gaps
    assert U.ctra_functions(np.nextafter(2.0 ** -6, 0.0)) == U.taylor(np.nextafter(2.0 ** -6, 0.0))
    assert U.ctra_functions(2.0 ** -6) == U.closed(2.0 ** -6)
    assert U.ctra_functions(0.0) == (1.0, 0.0, 0.5, 0.0)


def test_hand_cases_on_dyadic_numbers():
    size = (2.0, 1.0, 0.5)
    # straight at heading 0: x = 3 + 4 tau
    rows, flags, _ = U.predict_track((3.0, -2.0, 0.0, 4.0, 0.0, 0.0) + size, 0.0, 0.5, 5, 1)
    assert rows[:, 0].tolist() == [3.0, 5.0, 7.0, 9.0, 11.0] and (rows[:, 1] == -2.0).all() and (rows[:, 2] == 0.0).all() and flags == 0
    assert (rows[:, 3:] == size).all()
    # braking 8 m/s at 2 m/s^2: stops after 4 s and 16 m; x = 8 tau - tau^2 before
    rows, flags, _ = U.predict_track((0.0, 0.0, 0.0, 8.0, -2.0, 0.0) + size, 0.0, 1.0, 7, 1)
    assert rows[:, 0].tolist() == [0.0, 7.0, 12.0, 15.0, 16.0, 16.0, 16.0] and (rows[:, 1:3] == 0.0).all() and flags == U.STOPS
    rows, flags, _ = U.predict_track((0.0, 0.0, 0.0, 8.0, -2.0, 0.25) + size, 0.0, 1.0, 7, 1)
    assert (rows[4:] == rows[4]).all() and flags == U.STOPS                              # a stopped agent neither moves nor turns
    assert rows[4, 2] == 1.0                                                             # it turned for its 4 s at 0.25 rad/s
    # the cap: 38 -> 40 m/s at 2 m/s^2 takes 1 s and 39 m, then 40 m/s
    rows, flags, _ = U.predict_track((0.0, 0.0, 0.0, 38.0, 2.0, 0.0) + size, 0.0, 1.0, 4, 1)
    assert rows[:, 0].tolist() == [0.0, 39.0, 79.0, 119.0] and flags == U.CAPPED
    # a track that is already faster keeps its speed: the cap ends an acceleration and slows nobody down
    rows, flags, _ = U.predict_track((0.0, 0.0, 0.0, 48.0, 2.0, 0.0) + size, 0.0, 1.0, 3, 1)
    assert rows[:, 0].tolist() == [0.0, 48.0, 96.0] and flags == U.CAPPED
    # standing with a yaw rate: neither moves nor turns
    rows, flags, _ = U.predict_track((1.0, 1.0, 0.5, 0.0, 0.0, 0.3) + size, 0.0, 1.0, 3, 1)
    assert (rows[:, :3] == (1.0, 1.0, 0.5)).all() and flags == U.STOPS
    # the radius grows with the time of the step
    rows, _, _ = U.predict_track((0.0, 0.0, 0.0, 1.0, 0.0, 0.0) + size, 2.0, 1.0, 3, 2, prm=(40.0, 0.25, 3.0))
    assert rows[:, 5].tolist() == [1.0, 1.125, 1.25, 1.375, 1.5]
    # absent and bad
    rows, flags, _ = U.predict_track((1.0, 1.0, 0.5, 1.0, 0.0, 0.3, -1.0, 1.0, 0.5), 0.0, 1.0, 3, 1)
    assert (rows == U.ABSENT_ROW).all() and flags == U.ABSENT
    rows, flags, _ = U.predict_track((1.0, math.inf, 0.5, 1.0, 0.0, 0.3) + size, 0.0, 1.0, 3, 1)
    assert np.isnan(rows[:, :3]).all() and (rows[:, 3:] == size).all() and flags == U.BAD


def test_hand_cases_of_the_lane_model():
    """a straight lane along x whose table is dyadic: forward and oncoming, half a metre to its left"""
    lane = U.dyadic_lane()
    size = (2.0, 1.0, 0.5)
    rows, flags, anchor = U.predict_track((10.0, 0.5, 0.125, 4.0, 0.0, 0.3) + size, 0.0, 1.0, 4, 1, lane=lane)
    assert anchor.tolist() == [10.0, 0.5, 1.0, 0.125] and flags == U.ON_LANE
    assert rows[:, 0].tolist() == [10.0, 14.0, 18.0, 22.0] and (rows[:, 1] == 0.5).all() and (rows[:, 2] == 0.0).all()     # the lane's heading, not the track's
    rows, flags, anchor = U.predict_track((10.0, 0.5, math.pi, 4.0, 0.0, 0.3) + size, 0.0, 1.0, 5, 1, lane=lane)
    assert anchor[:3].tolist() == [10.0, 0.5, -1.0] and flags == U.ON_LANE | U.OFF_LANE                                    # s = -6 at the last step
    assert rows[:, 0].tolist() == [10.0, 6.0, 2.0, -2.0, -6.0] and (rows[:, 1] == 0.5).all() and (rows[:, 2] == math.pi).all()
    # four metres off the line: not on that lane, the free model under the track's own heading and yaw rate
    far, flags, anchor = U.predict_track((10.0, 4.0, 0.0, 4.0, 0.0, 0.0) + size, 0.0, 1.0, 3, 1, lane=lane)
    free, _, _ = U.predict_track((10.0, 4.0, 0.0, 4.0, 0.0, 0.0) + size, 0.0, 1.0, 3, 1)
    assert (far == free).all() and flags == U.LANE_FAR and anchor.tolist() == [10.0, 4.0, 0.0, 0.0]


@pytest.mark.parametrize("t0", [0.0, 0.3])
def test_rows_of_r1_are_rows_kr_of_r3(t0):
    lanes = [U.straight_lane(), U.arc_lane()]
    tracks = U.seeded_tracks(1, 6, seed=3)
    tracks[0, 4] = U.on_lane_track(lanes[0], 5.0, 0.7, 6.0, 0.75)
    tracks[0, 5] = U.on_lane_track(lanes[1], 30.0, -1.1, 9.0, -1.25, oncoming=True)
    lane_of = np.array([[-1, -1, -1, -1, 0, 1]])
    coarse = U.predict(tracks, t0, 0.7, 9, 1, lane_of=lane_of, lanes=lanes)
    fine = U.predict(tracks, t0, 0.7, 9, 3, lane_of=lane_of, lanes=lanes)
    assert coarse["agents"].tobytes() == fine["agents"][:, :, ::3].tobytes()
    assert (coarse["flags"] == fine["flags"]).all() and (coarse["flags"][0, 4:] & U.ON_LANE).all()


def test_struct_free_abi_and_defaults(hip_lib):
    assert (capi.PREDICT_PARAMS, capi.TRACK_STRIDE, capi.ANCHOR_STRIDE) == (3, 9, 4)
    assert (capi.PREDICT_V_CAP, capi.PREDICT_GROW, capi.PREDICT_L_MAX) == (0, 1, 2)
    assert [getattr(capi, "PREDICT_" + n) for n in ("ABSENT", "BAD", "ON_LANE", "LANE_FAR", "OFF_LANE", "STOPS", "CAPPED")] == \
        [U.ABSENT, U.BAD, U.ON_LANE, U.LANE_FAR, U.OFF_LANE, U.STOPS, U.CAPPED]
    p = capi.predict_default_params(hip_lib)
    assert (p.v_cap, p.grow, p.l_max) == (U.V_CAP, U.GROW, U.L_MAX) and p.array().tolist() == [40.0, 0.0, 3.0]
    assert capi.predict_default_params(hip_lib, grow=0.1).array().tolist() == [40.0, 0.1, 3.0]
    hip_lib.pqp_predict_default_params(None)                                             # a NULL pointer is ignored
    assert not any(s.startswith("pqp_predict") for s in capi.HEADER.structs)
    for name in ("pqp_predict_agents", "pqp_predict_agents_device"):
        assert [q.name for q in capi.HEADER.functions[name].params] == \
            ["h", "prm", "t0", "dt", "m", "r", "n_scenes", "a_max", "tracks", "a_of", "lane_of", "n_lanes", "lane_m", "lane_spline", "lane_ext",
             "lane_length", "agents", "anchor", "flags"]
    # refused for its arguments before it touches a device
    assert hip_lib.pqp_predict_agents_device(None, p.array(), 0.0, 1.0, 1, 1, 1, 1, None, None, None, 0, 0, None, None, None, None, None, None) == -1
    assert hip_lib.pqp_last_error().decode().startswith("pqp_predict_agents:")


def test_chain_keywords_are_checked_before_the_device(hip_lib):
    h = object.__new__(capi.Handle)
    h.lib = hip_lib
    tr = U.seeded_tracks(2, 3, seed=1)
    search = capi.search_default_params(hip_lib)
    args = lambda **kw: h._tracks(kw.get("tracks", (tr, None, None, None)), kw.get("layers", 6), kw.get("anchor", False), kw.get("search", search),
                                  kw.get("agents"), kw.get("plan_agents"), kw.get("plan_samples"))
    with pytest.raises(ValueError, match="refused together with agents"):
        args(agents=np.zeros((2, 3, 6, 6)))
    with pytest.raises(ValueError, match="refused together with agents"):
        args(plan_agents=np.zeros((2, 3, 16, 6)), plan_samples=3)
    with pytest.raises(ValueError, match="needs search"):
        args(search=None)
    with pytest.raises(ValueError, match="layers=m"):
        args(layers=None)
    with pytest.raises(ValueError, match="at or above"):
        args(tracks=(tr, np.zeros((2, 3), np.int32), None, None))
    with pytest.raises(ValueError, match="need tracks"):
        h._tracks(None, 6, False, search, None, None, None)
    predicting, agents, fine = args(plan_samples=3, anchor=True)
    assert agents.shape == (2, 3, 6, 6) and fine.shape == (2, 3, 16, 6) and agents.ndim == 4 and agents.size == 216 and predicting[4] is True
    assert h._tracks(None, None, False, search, "a", "b", 3) == (None, "a", "b")       # without tracks= nothing changes
    # the stand-ins pass the checks agents= and plan_agents= go through
    got = h._agents(agents, [3, 1], None, None, None, None, None, 4, None, search)
    assert got[0] is agents and got[1].tolist() == [3, 1]
    assert h._plan(3, fine, search, agents) == (3, fine)


def test_predictor_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("predict_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "case.bin"
    U.write_case(path, U.seeded_tracks(1, 2, seed=2)[0], 4, 2, 0.5)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no predictor" in r.stderr
