"""pqp_predict_agents on the device against tests/predict_util.py's restatement of include/pqp.h: shapes around the 64-step tile, both
models, the time grid, both forms, hostile tracks, every refusal, the chain's tracks= and the C++ predictor.

The bound on a pose, TOL = 1e-9 m, is tests/test_gpu_agents_check.py's.  Device and restatement run the same operations; they differ in
sin / cos / sincos / atan2 (ocml against libm), each within a few ulp.  On the seeds here - |x|, |y| <= 500 m, v <= 40 m/s, |a| <= 3 m/s^2,
a horizon of 8 s, a yaw rate of 0 or 0.05 .. 0.5 rad/s - the lever of such an ulp is v tau + a tau^2 <= 320 + 192 = 512 m (the free
model multiplies v te and a te^2 by functions of the angle): 4 ulp x 512 m = 2.3e-13 m.  The sums onto a coordinate below 820 m round
to 1.1e-13 m each, two of them.  f2's numerator sin th - th cos th loses th^2 to cancellation, an error of 2 ulp(th) / th^2 = 4.4e-16 / th
on f2, times a te^2: 4.4e-16 a te / w <= 4.4e-16 x 3 x 8 / 0.05 = 2.1e-13 m.  Together 6.7e-13 m, three orders below the bound.  (The
seeds keep the yaw rate away from 0 < |w| < 0.05 rad/s for that last term; the angles at the switch are test_predict_agents.py's
and the hand cases' here.)  On the lane model the lever of an ulp in atan2, cos and sin is |l0| <= 3 m.  Largest difference seen on one
MI355X over the shapes below: 5.7e-14 m."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import cpp_demo
import predict_util as U
import project_util as P
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-9
HORIZON = 8.0
SIZE = (2.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def lanes():
    return (U.straight_lane(), U.arc_lane())


@functools.lru_cache(maxsize=None)
def packed():
    return U.pack_lanes(lanes())


def _scene(S, A, seed):
    """tracks [S][A][9], lane_of [S][A], a_of [S]: seeded free tracks, every third slot on a lane (forward on the line, oncoming on the arc),
    ragged counts that include 0 where there is more than one scene"""
    tracks = U.seeded_tracks(S, A, seed)
    lane_of = np.full((S, A), -1, np.int32)
    for s in range(S):
        for g in range(A):
            if (s + g) % 3 == 1:
                which = (s + g) % 2
                lane = lanes()[which]
                tracks[s, g] = U.on_lane_track(lane, 4.0 + 3.0 * g, 0.6 * (g - 1), 3.0 + g, (-1.25, 0.75)[which], oncoming=bool(which))
                lane_of[s, g] = which
    a_of = np.array([A if s == 0 else (0 if s == 1 else A - 1) for s in range(S)], np.int32)
    return tracks, lane_of, a_of


def _host(h, tracks, m, r, dt, t0=0.0, a_of=None, lane_of=None, prm=None):
    return h.predict_agents(tracks, t0=t0, dt=dt, m=m, r=r, a_of=a_of, lane_of=lane_of, lanes=packed(), prm=prm, anchor=True)


def _device(h, tracks, m, r, dt, t0=0.0, a_of=None, lane_of=None, prm=None, n_lanes=2):
    """the device form on outputs prefilled with -7: every element must have been overwritten"""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a, dt_: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt_)).to(dev)
    S, A = tracks.shape[:2]
    M = (m - 1) * r + 1
    spl, ext, length = packed()
    d_agents = torch.full((S, A, M, 6), -7.0, dtype=torch.float64, device=dev)
    d_anchor = torch.full((S, A, 4), -7.0, dtype=torch.float64, device=dev)
    d_flags = torch.full((S, A), -7, dtype=torch.int32, device=dev)
    ins = (t(tracks, np.float64), t(a_of, np.int32), t(lane_of, np.int32), t(spl, np.float64), t(ext, np.float64), t(length, np.float64))
    torch.cuda.synchronize(dev)
    prm = prm if prm is not None else capi.predict_default_params()
    rc = h.lib.pqp_predict_agents_device(h._h, prm.array(), float(t0), float(dt), m, r, S, A, ins[0], ins[1], ins[2], n_lanes, spl.shape[2], ins[3], ins[4],
                                         ins[5], d_agents, d_anchor, d_flags)
    assert rc == 0, h.lib.pqp_last_error()
    h.sync()
    res = dict(agents=d_agents.cpu().numpy(), anchor=d_anchor.cpu().numpy(), flags=d_flags.cpu().numpy())
    assert not (res["agents"] == -7.0).any() and not (res["anchor"] == -7.0).any() and not (res["flags"] == -7).any()
    return res


def _same(a, b):
    return all(same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)) for k in ("agents", "anchor", "flags"))


def _angle_gap(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def _against_restatement(h, got, tracks, m, r, dt, t0, a_of, lane_of, prm=None, who=""):
    """flags, sizes and absent rows bit for bit; the free model's heading bit for bit (no library function enters it); every pose within
    TOL of the restatement at the device's own anchor; that anchor's s0 bit for bit Handle.project_points', its s0 and l0 within project_util's
    bound of the restatement's own search.  Returns the largest pose difference."""
    p = (prm.v_cap, prm.grow, prm.l_max) if prm is not None else (U.V_CAP, U.GROW, U.L_MAX)
    want = U.predict(tracks, t0, dt, m, r, a_of=a_of, lane_of=lane_of, lanes=lanes(), prm=p, anchors=got["anchor"])
    own = U.predict(tracks, t0, dt, 1, 1, a_of=a_of, lane_of=lane_of, lanes=lanes(), prm=p)
    assert np.array_equal(got["flags"], want["flags"]), (who, got["flags"], want["flags"])
    assert same_bits(got["agents"][..., 3:], want["agents"][..., 3:]), who
    gone = (want["flags"] & (U.ABSENT | U.BAD)) != 0
    assert same_bits(got["agents"][gone], want["agents"][gone]), who
    free = ((want["flags"] & (U.ABSENT | U.BAD | U.ON_LANE)) == 0)
    assert same_bits(got["agents"][free][..., 2], want["agents"][free][..., 2]), who
    live = ~gone
    worst = 0.0
    if live.any():
        worst = float(np.abs(got["agents"][live][..., :2] - want["agents"][live][..., :2]).max())
        assert worst < TOL, (who, worst)
        assert _angle_gap(got["agents"][live][..., 2], want["agents"][live][..., 2]).max() < TOL, who
    searched = (want["flags"] & (U.ON_LANE | U.LANE_FAR)) != 0
    if lane_of is not None:
        searched &= np.asarray(lane_of) < len(lanes())
    spl, ext, length = packed()
    for s, g in zip(*np.nonzero(searched)):
        k = int(lane_of[s][g])
        proj, _ = h.project_points(spl[k:k + 1], ext[k:k + 1], length[k:k + 1], tracks[s, g][None, None, :3])
        assert same_bits(got["anchor"][s, g, 0], proj[0, 0, 0]), (who, s, g)
        assert np.abs(got["anchor"][s, g, :2] - own["anchor"][s, g, :2]).max() < P.PROJECT_TOL, (who, s, g)
        assert got["anchor"][s, g, 2] == own["anchor"][s, g, 2], (who, s, g)
    assert not got["anchor"][~searched].any(), who
    return worst


SHAPES = [(1, 1, 1, 1), (63, 1, 1, 4), (64, 1, 1, 5), (22, 3, 2, 3), (65, 1, 2, 3), (44, 3, 1, 5), (130, 1, 3, 4)]     # m, r, S, A: M = 1, 63, 64, 64, 65, 130, 130


@pytest.mark.parametrize("m,r,S,A", SHAPES)
def test_shapes_against_the_restatement(handle, m, r, S, A):
    tracks, lane_of, a_of = _scene(S, A, seed=10 * m + A)
    dt = HORIZON / (m - 1) if m > 1 else 1.0
    got = _host(handle, tracks, m, r, dt, a_of=a_of, lane_of=lane_of)
    assert got["agents"].shape == (S, A, (m - 1) * r + 1, 6)
    worst = _against_restatement(handle, got, tracks, m, r, dt, 0.0, a_of, lane_of, who=(m, r, S, A))
    print(f"m {m} r {r} scenes {S} agents {A}: flags {got['flags'].tolist()}, max |pose - restatement| = {worst:.3e} m")
    assert _same(got, _device(handle, tracks, m, r, dt, a_of=a_of, lane_of=lane_of)), "host and device form differ"
    if A >= 3:
        assert (got["flags"] & U.ON_LANE).any()


def test_no_agents_and_every_optional_array_absent(handle):
    got = handle.predict_agents(np.zeros((2, 0, 9)), m=5, r=2)
    assert got["agents"].shape == (2, 0, 9, 6) and got["flags"].shape == (2, 0)
    assert handle.lib.pqp_predict_agents_device(handle._h, capi.predict_default_params().array(), 0.0, 1.0, 5, 2, 2, 0, None, None, None, 0, 0, None, None,
                                                None, None, None, None) == 0
    tracks = U.seeded_tracks(1, 3, seed=4)
    got = handle.predict_agents(tracks, dt=0.5, m=9)                    # no a_of, no lane_of, no lanes, no anchor
    want = U.predict(tracks, 0.0, 0.5, 9, 1)
    assert sorted(got) == ["agents", "flags"] and np.array_equal(got["flags"], want["flags"])
    assert np.abs(got["agents"][..., :2] - want["agents"][..., :2]).max() < TOL and same_bits(got["agents"][..., 2:], want["agents"][..., 2:])


def test_the_hand_cases_bit_for_bit(handle):
    """heading 0 and dyadic numbers: no library function returns anything but 0 or 1, so the free model, and the lane model on a lane
    whose table is dyadic, agree with the restatement in every bit"""
    lane = U.dyadic_lane()
    spl = U.pack_lanes([lane])
    tracks = np.array([[(3.0, -2.0, 0.0, 4.0, 0.0, 0.0) + SIZE, (0.0, 0.0, 0.0, 8.0, -2.0, 0.0) + SIZE, (0.0, 0.0, 0.0, 38.0, 2.0, 0.0) + SIZE,
                        (1.0, 1.0, 0.5, 0.0, 0.0, 0.3) + SIZE, (10.0, 0.5, 0.125, 4.0, 0.0, 0.3) + SIZE, (10.0, 0.5, math.pi, 4.0, 0.0, 0.3) + SIZE,
                        (10.0, 4.0, 0.0, 4.0, 0.0, 0.0) + SIZE]])
    lane_of = np.array([[-1, -1, -1, -1, 0, 0, 0]], np.int32)
    prm = capi.predict_default_params(grow=0.25)
    got = handle.predict_agents(tracks, t0=0.0, dt=1.0, m=7, r=2, lane_of=lane_of, lanes=spl, prm=prm, anchor=True)
    want = U.predict(tracks, 0.0, 1.0, 7, 2, lane_of=lane_of, lanes=[lane], prm=(40.0, 0.25, 3.0))
    assert _same(got, want), (got["anchor"], want["anchor"])
    assert got["flags"].tolist() == [[0, U.STOPS, U.CAPPED, U.STOPS, U.ON_LANE, U.ON_LANE | U.OFF_LANE, U.LANE_FAR]]
    assert got["agents"][0, 0, :, 0].tolist() == [3.0 + 2.0 * f for f in range(13)]
    assert got["agents"][0, 5, ::2, 0].tolist() == [10.0, 6.0, 2.0, -2.0, -6.0, -10.0, -14.0] and (got["agents"][0, 5, :, 2] == math.pi).all()
    assert got["anchor"][0, 4].tolist() == [10.0, 0.5, 1.0, 0.125] and got["anchor"][0, 5, :3].tolist() == [10.0, 0.5, -1.0]


@pytest.mark.parametrize("t0", [0.0, 0.3])
def test_layer_rows_are_every_third_fine_row(handle, t0):
    tracks, lane_of, a_of = _scene(2, 5, seed=7)
    a_of[:] = 5
    coarse = _host(handle, tracks, 9, 1, 0.7, t0=t0, a_of=a_of, lane_of=lane_of)
    fine = _host(handle, tracks, 9, 3, 0.7, t0=t0, a_of=a_of, lane_of=lane_of)
    assert same_bits(coarse["agents"], fine["agents"][:, :, ::3]) and same_bits(coarse["anchor"], fine["anchor"])
    assert np.array_equal(coarse["flags"], fine["flags"])


def test_same_bits_at_any_position_in_any_batch(handle):
    tracks, lane_of, _ = _scene(1, 5, seed=9)
    alone = [_host(handle, tracks[:, g:g + 1], 22, 3, 0.4, lane_of=lane_of[:, g:g + 1]) for g in range(5)]
    big = np.zeros((3, 7, 9))
    big[..., 6] = -1.0
    big_lane = np.full((3, 7), -1, np.int32)
    where = [(0, 6), (2, 0), (1, 3), (2, 6), (0, 0)]
    for g, (s, q) in enumerate(where):
        big[s, q], big_lane[s, q] = tracks[0, g], lane_of[0, g]
    big[1, 4], big_lane[1, 4] = tracks[0, 1], lane_of[0, 1]              # the same track a second time
    got = _device(handle, big, 22, 3, 0.4, lane_of=big_lane)
    for g, (s, q) in enumerate(where):
        for k in ("agents", "anchor", "flags"):
            assert same_bits(np.asarray(got[k][s, q], dtype=np.float64), np.asarray(alone[g][k][0, 0], dtype=np.float64)), (g, k)
    assert same_bits(got["agents"][1, 4], got["agents"][2, 0]) and got["flags"][1, 4] == got["flags"][2, 0]
    rest = np.ones((3, 7), bool)
    rest[tuple(zip(*where))] = False
    rest[1, 4] = False
    assert (got["flags"][rest] == U.ABSENT).all() and (got["agents"][rest] == U.ABSENT_ROW).all()


def test_lanes_far_oncoming_and_the_flags(handle):
    line, arc = lanes()
    far = U.on_lane_track(line, 12.0, 3.5, 6.0, 0.75)                    # 3.5 m off the line: beyond l_max = 3
    near = U.on_lane_track(line, 12.0, 2.5, 6.0, 0.75)
    onc = U.on_lane_track(arc, 30.0, -1.0, 5.0, 0.0, oncoming=True)
    stops = U.on_lane_track(line, 2.0, 0.0, 6.0, -3.0)                   # stands after 2 s and 6 m
    caps = [0.0, 0.0, 0.3, 39.0, 2.0, 0.1, *SIZE]
    tracks = np.array([[far, near, onc, stops, caps, far]])
    lane_of = np.array([[0, 0, 1, 0, -1, -1]], np.int32)
    got = _host(handle, tracks, 9, 3, 1.0, lane_of=lane_of)
    _against_restatement(handle, got, tracks, 9, 3, 1.0, 0.0, None, lane_of, who="behaviour")
    F = got["flags"][0]
    assert F.tolist() == [U.LANE_FAR, U.ON_LANE | U.OFF_LANE, U.ON_LANE | U.OFF_LANE, U.ON_LANE | U.STOPS, U.CAPPED, 0], F
    # a track that is not on its lane gets the free model's rows bit for bit
    assert same_bits(got["agents"][0, 0], got["agents"][0, 5]) and got["anchor"][0, 0, 2] == 0.0 and abs(got["anchor"][0, 0, 1]) > 3.0
    # so does one whose lane is not there, through the device form; the host form refuses it
    beyond = np.array([[2, 0, 1, 0, -1, 7]], np.int32)
    dev = _device(handle, tracks, 9, 3, 1.0, lane_of=beyond)
    assert same_bits(dev["agents"][0, 0], got["agents"][0, 0]) and same_bits(dev["agents"][0, 1:], got["agents"][0, 1:])
    assert dev["flags"][0].tolist() == [F[0], F[1], F[2], F[3], F[4], F[5] | U.LANE_FAR] and not dev["anchor"][0, 0].any()
    with pytest.raises(capi.PqpError, match="lane_of at or above n_lanes"):
        _host(handle, tracks, 9, 3, 1.0, lane_of=beyond)
    # oncoming: towards decreasing s, heading the lane's + pi
    assert got["anchor"][0, 2, 2] == -1.0 and abs(abs(got["anchor"][0, 2, 3]) - math.pi) < 0.2
    spl, ext, length = packed()
    proj, _ = handle.project_points(spl[1:2], ext[1:2], length[1:2], got["agents"][0:1, 2, :, :3])
    on = proj[0, :, 0] > 0.0
    assert on[:10].all() and (np.diff(proj[0, on, 0]) < 0.0).all()
    assert _angle_gap(got["agents"][0, 2, on, 2], proj[0, on, 6] + math.pi).max() < 1e-6 and np.abs(proj[0, on, 1] + 1.0).max() < 1e-6
    # a stopped agent's rows repeat bit for bit
    assert (got["agents"][0, 3, 6:] == got["agents"][0, 3, 6]).all() and not (got["agents"][0, 3, 5] == got["agents"][0, 3, 6]).all()


HOSTILE = [(c, v) for c in range(9) for v in (math.nan, math.inf)] + [(3, -0.5), (8, -0.1), (0, -math.inf), (4, -math.inf)]


def test_tracks_that_are_not_numbers_stay_in_their_slot(handle):
    """NaN or Inf in each column, a negative speed, a negative radius: PQP_PREDICT_BAD alone, NaN poses, the sizes kept, every neighbour
    bit for bit what it is without the bad track - and pqp_agents_check reads such rows as a hit at sample 0 for every path of the scene"""
    tracks, lane_of, _ = _scene(2, 3, seed=11)
    m, r, dt = 22, 3, 0.25
    clean = _host(handle, tracks, m, r, dt, lane_of=lane_of)
    assert not (clean["flags"] & U.BAD).any()
    M = (m - 1) * r + 1
    traj = np.zeros((3, M, 3))
    traj[..., 0] = 5000.0 + np.arange(3)[:, None] * 50.0                 # three parked cars far from everything
    for slot, (col, value) in enumerate(HOSTILE):
        s, g = slot % 2, (slot // 2) % 3
        bad = tracks.copy()
        bad[s, g, col] = value
        got = _host(handle, bad, m, r, dt, lane_of=lane_of)
        assert got["flags"][s, g] == U.BAD and np.isnan(got["agents"][s, g, :, :3]).all(), (col, value)
        assert same_bits(got["agents"][s, g, :, 3:], np.broadcast_to(bad[s, g, 6:], (M, 3))), (col, value)
        others = np.ones((2, 3), bool)
        others[s, g] = False
        for k in ("agents", "anchor", "flags"):
            assert same_bits(np.asarray(got[k][others], dtype=np.float64), np.asarray(clean[k][others], dtype=np.float64)), (col, value, k)
        if slot % 4 == 0:
            chk = handle.agents_check(traj, got["agents"], scene_of=np.array([s, s, 1 - s], np.int32))
            assert chk["first_hit"].tolist() == [0, 0, M] and chk["hit_agent"].tolist()[:2] == [g, g], (col, value, chk)
    # a size below zero, -inf included, is an absent slot, as in pqp_agents_check's rows
    gone = tracks.copy()
    gone[0, 1, 6] = -math.inf
    got = _host(handle, gone, m, r, dt, lane_of=lane_of)
    assert got["flags"][0, 1] == U.ABSENT and (got["agents"][0, 1] == U.ABSENT_ROW).all()


def test_refusals_leave_the_outputs_alone(handle):
    tracks, lane_of, a_of = _scene(2, 3, seed=12)
    spl, ext, length = packed()
    m, r = 5, 2
    agents, anchor, flags = np.full((2, 3, 9, 6), -7.0), np.full((2, 3, 4), -7.0), np.full((2, 3), -7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(form="pqp_predict_agents", prm=None, t0=0.0, dt=1.0, m_=m, r_=r, S=2, A=3, n_lanes=2, lane_m=spl.shape[2], drop=(), no_handle=False,
             lane_of_=lane_of):
        prm = prm if prm is not None else capi.predict_default_params().array()
        a = dict(prm=prm, tracks=tracks, spl=spl, ext=ext, length=length, agents=agents, flags=flags)
        for k in drop:
            a[k] = None
        rc = getattr(handle.lib, form)(None if no_handle else handle._h, p(a["prm"]), t0, dt, m_, r_, S, A, p(a["tracks"]), p(a_of), p(lane_of_), n_lanes,
                                       lane_m, p(a["spl"]), p(a["ext"]), p(a["length"]), p(a["agents"]), p(anchor), p(a["flags"]))
        return rc, bool((agents == -7.0).all() and (anchor == -7.0).all() and (flags == -7).all()), handle.lib.pqp_last_error().decode()

    bad = [dict(no_handle=True), dict(S=0), dict(S=-1), dict(A=-1), dict(m_=0), dict(r_=0), dict(m_=2 ** 30, r_=4), dict(S=2 ** 20, A=2 ** 19),
           dict(S=2 ** 15, A=2 ** 15, m_=2 ** 9), dict(n_lanes=-1), dict(lane_m=1), dict(lane_m=0)]
    bad += [dict(drop=(k,)) for k in ("prm", "tracks", "spl", "ext", "length", "agents", "flags")]
    bad += [dict(dt=v) for v in (0.0, -1.0, math.nan, math.inf)] + [dict(t0=v) for v in (-0.5, math.nan, math.inf)]
    for k in range(3):
        for v in (-1.0, math.nan, math.inf):
            q = capi.predict_default_params().array()
            q[k] = v
            bad.append(dict(prm=q))
    for form in ("pqp_predict_agents", "pqp_predict_agents_device"):                # (the device form is refused before it reads a pointer)
        for kw in bad:
            rc, untouched, msg = call(form=form, **kw)
            assert rc == -1 and untouched and msg.startswith("pqp_predict_agents:"), (form, kw, rc, msg)
    rc, untouched, msg = call(lane_of_=np.array([[0, 1, 2], [0, 0, 0]], np.int32))
    assert rc == -1 and untouched and "lane_of" in msg
    rc, untouched, _ = call()
    assert rc == 0 and not untouched and not (agents == -7.0).any() and not (flags == -7).any() and not (anchor == -7.0).any()
    want = _host(handle, tracks, m, r, 1.0, a_of=a_of, lane_of=lane_of)
    assert same_bits(agents, want["agents"]) and same_bits(anchor, want["anchor"]) and np.array_equal(flags, want["flags"])


# ---- through the layers ----------------------------------------------------------------------------------------------------------------
def test_tracks_behind_the_chain(hip_lib):
    """optimize_path(..., tracks=, layers=, search=, plan_samples=3) gives bit for bit what the same call gives with agents= and plan_agents=
    set to the predictions it downloaded itself"""
    import chain_util
    B, m, r = 4, 8, 3
    sc = chain_util.scenarios(B)
    sp = capi.speed_default_params(v_max=8.0)
    se = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    se.stations, se.margin = 96, 0.2
    st, tg = sc["start"][0], sc["target"][0]
    mid = (0.5 * (st[0] + tg[0]), 0.5 * (st[1] + tg[1]))
    line = U.make_lane(np.linspace(mid[0] - 20.0 * math.cos(st[2] + 1.5), mid[0] + 20.0 * math.cos(st[2] + 1.5), U.LANE_M),
                       np.linspace(mid[1] - 20.0 * math.sin(st[2] + 1.5), mid[1] + 20.0 * math.sin(st[2] + 1.5), U.LANE_M))
    crossing = U.on_lane_track(line, 8.0, 0.4, 4.0, -0.5)                # along a lane that crosses candidate 0's line near its middle
    free = [tg[0], tg[1], tg[2] + math.pi, 3.0, 0.5, 0.05, 2.2, 0.9, 0.1]  # from the target back towards the start
    tracks = np.array([[crossing, free, [0.0] * 6 + [-1.0, 1.0, 0.0]]])
    lane_of = np.array([[0, -1, -1]], np.int32)
    lanes_ = U.pack_lanes([line])
    prm = capi.predict_default_params(hip_lib, grow=0.05)
    ap = capi.agents_default_params(hip_lib, margin=0.3)
    base = dict(speed=sp, v_start=np.linspace(0.0, 3.0, B), search=se, refine=capi.refine_default_params(hip_lib), plan_samples=r, agents_params=ap,
                agents_of=np.array([3], np.int32))
    h2 = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    coarse = h2.predict_agents(tracks, dt=se.dt, m=m, lane_of=lane_of, lanes=lanes_, prm=prm, anchor=True)
    fine = h2.predict_agents(tracks, dt=se.dt, m=m, r=r, lane_of=lane_of, lanes=lanes_, prm=prm)
    h2.close()
    assert coarse["flags"][0].tolist() == [U.ON_LANE, 0, U.ABSENT]
    runs = []
    for kw in (dict(tracks=(tracks, lane_of, lanes_, prm), layers=m, predict_anchor=True), dict(agents=coarse["agents"], plan_agents=fine["agents"])):
        h, hs = chain_util.handles(B)
        runs.append(h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **base, **kw))
        if "tracks" in kw:
            with pytest.raises(ValueError, match="refused together with agents"):
                h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **base, **kw,
                                agents=coarse["agents"])
        h.close(); hs.close()
    with_tracks, with_arrays = runs
    assert list(with_tracks) == list(with_arrays) + ["predict_flags", "predict_anchor"]
    for k in with_arrays:
        assert same_bits(np.asarray(with_tracks[k], dtype=np.float64), np.asarray(with_arrays[k], dtype=np.float64)), k
    assert np.array_equal(with_tracks["predict_flags"], coarse["flags"]) and same_bits(with_tracks["predict_anchor"], coarse["anchor"])
    print(f"behind the chain: predict flags {with_tracks['predict_flags'].tolist()}, search flags {with_tracks['search_flags'].tolist()}, "
          f"plan first hit {with_tracks['plan_first_hit'].tolist()}")


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_predictor_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("predict_demo")
    tracks = U.seeded_tracks(1, 2, seed=2)
    path = tmp_path / "case.bin"
    U.write_case(path, tracks[0], 4, 2, 0.5)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = handle.predict_agents(tracks, dt=0.5, m=4, r=2)
    lines = iter(r.stdout.strip().splitlines())
    for a in range(2):
        head = next(lines).split()
        assert head[0] == "agent" and [int(v) for v in head[1:]] == [a, want["flags"][0, a], 7], head
        got = np.array([[float(v) for v in next(lines).split()] for _ in range(7)])
        assert same_bits(got, want["agents"][0, a]), a
    assert next(lines, None) is None
