"""pqp_stitch_trajectory on the device, held to the restatement of tests/stitch_util.py over the cases of stitch_util.device_cases().

What is asked bit for bit: flags, idx, prefix_n of every group; the state row, the prefix and the candidates' start, start_k and v_start of
every stitched group (copies and one subtraction); of a replanned group the columns no sincos enters (k, s, v, a, t); zeros of a bad one.
What is asked to 1e-9 m or rad: dev and a replanned group's pose, for coordinates within +-1000 m - DESIGN 3.13's and 3.18's bound for
this expression class, the device's sincos against libm's.  tests/test_stitch_trajectory.py shows that every comparison a flag hangs on
keeps a margin of 1e-6 in every case here, so that bound cannot move a flag."""
import subprocess

import numpy as np
import pytest

import chain_plan_cases as cases
import chain_util
import cpp_demo
import device_form as D
import stitch_util as U
from path_optimizer_2_amd import capi
from shared_util import same_bits, same_bytes

pytestmark = pytest.mark.gpu
CASES = U.device_cases()
BY_NAME = {c["name"]: c for c in CASES}
TOL = 1e-9
KEYS = ("state", "flags", "dev", "idx", "prefix", "prefix_n", "start", "start_k", "v_start")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def restated():
    """every case's restatement, computed once and left unchanged"""
    return {c["name"]: U.run_case(c) for c in CASES}


def _prm(c):
    return capi.StitchParams(c["prm"], c["keep"])


def _host(h, c, **over):
    a = dict(c, **over)
    return h.stitch_trajectory(a["prev"], a["meas"], a["t_now"], m_of=a["m_of"], group_start=a["group_start"], batch=a["batch"], prm=_prm(a),
                               prefix_max=a["prefix_max"])


def _held_to(got, want, c):
    """the device's result against the restatement's, as the module's docstring says"""
    name = c["name"]
    assert np.array_equal(got["flags"], want["flags"]) and np.array_equal(got["idx"], want["idx"]), (name, got["flags"], want["flags"], got["idx"], want["idx"])
    assert np.array_equal(got["prefix_n"], want["prefix_n"]), name
    stitched, replanned, bad = ((want["flags"] & f) != 0 for f in (U.STITCHED, U.REPLAN, U.BAD))
    assert (stitched.astype(int) + replanned + bad == 1).all()
    err = float(np.abs(got["dev"] - want["dev"]).max())
    assert err <= TOL, (name, err)
    assert same_bits(got["state"][stitched], want["state"][stitched]) and same_bits(got["prefix"][stitched], want["prefix"][stitched]), name
    assert same_bits(got["state"][replanned][:, 3:], want["state"][replanned][:, 3:]) and same_bits(got["prefix"][replanned][:, :, 3:], want["prefix"][replanned][:, :, 3:]), name
    if replanned.any():
        pose = float(np.abs(got["state"][replanned][:, :3] - want["state"][replanned][:, :3]).max())
        assert pose <= TOL and float(np.abs(got["prefix"][replanned][:, :, :3] - want["prefix"][replanned][:, :, :3]).max()) <= TOL, (name, pose)
        assert same_bits(got["prefix"][replanned][:, 0, :7], got["state"][replanned][:, :7])           # the one row is the state row
    for k in ("state", "dev", "prefix"):
        assert not got[k][bad].any(), (name, k)
    # the candidates: their group's state row, in the device's own bits - and so, for a stitched group, the restatement's
    G, batch = len(want["flags"]), len(want["start_k"])
    seen = np.zeros(batch, bool)
    for g in range(G):
        lo, hi = U.group_rows(c["group_start"], g, batch)
        seen[lo:hi] = True
        assert same_bits(got["start"][lo:hi], np.broadcast_to(got["state"][g, :3], (max(hi - lo, 0), 3))), (name, g)
        assert same_bits(got["start_k"][lo:hi], np.full(max(hi - lo, 0), got["state"][g, 3])) and same_bits(got["v_start"][lo:hi], np.full(max(hi - lo, 0), got["state"][g, 5]))
        if stitched[g]:
            assert same_bits(got["start"][lo:hi], want["start"][lo:hi]) and same_bits(got["start_k"][lo:hi], want["start_k"][lo:hi]) and \
                same_bits(got["v_start"][lo:hi], want["v_start"][lo:hi]), (name, g)
    assert seen.all() and np.isfinite(got["start"]).all() and np.isfinite(got["start_k"]).all() and np.isfinite(got["v_start"]).all()
    assert same_bits(got["start_k"], want["start_k"]) and same_bits(got["v_start"], want["v_start"]), name          # (no sincos enters k or v)
    return err


@pytest.mark.parametrize("name", list(BY_NAME))
def test_the_host_form_against_the_restatement(handle, restated, name):
    c = BY_NAME[name]
    got = _host(handle, c)
    err = _held_to(got, restated[name], c)
    print(f"{name}: flags {sorted(set(got['flags'].tolist()))}, dev within {err:.2e}")


def test_a_bad_group_leaves_its_neighbours_bits(handle):
    c = BY_NAME["bad_measurements"]
    got = _host(handle, c)
    bad = np.flatnonzero(got["flags"] == U.BAD)
    assert bad.tolist() == [1, 3, 5, 6]
    meas, t_now = c["meas"].copy(), c["t_now"].copy()
    meas[bad], t_now[bad] = meas[0], t_now[0]
    other = _host(handle, c, meas=meas, t_now=t_now)
    good = np.setdiff1d(np.arange(len(t_now)), bad)
    assert not (other["flags"][bad] & U.BAD).any()
    for k in ("state", "flags", "dev", "idx", "prefix", "prefix_n"):
        assert same_bytes(got[k][good], other[k][good]), k
    mine = np.concatenate([np.arange(*U.group_rows(c["group_start"], g, c["batch"])) for g in good])
    for k in ("start", "start_k", "v_start"):
        assert same_bytes(got[k][mine], other[k][mine]), k


@pytest.mark.parametrize("name", ["m65_G67_s11_keep200_capNone", "replans", "times"])
def test_the_same_group_elsewhere_in_a_larger_batch_has_the_same_bits(handle, name):
    c = BY_NAME[name]
    got = _host(handle, c, group_start=None, batch=None)
    G, m, stride = c["prev"].shape
    rng = np.random.default_rng(11)
    big = U.seeded_case(2 * G + 3, m, seed=12, stride=stride)
    at = rng.permutation(2 * G + 3)[:G]
    big["prev"][at], big["meas"][at], big["t_now"][at] = c["prev"], c["meas"], c["t_now"]
    big["m_of"][at] = m if c["m_of"] is None else c["m_of"]
    other = _host(handle, dict(c, **big), group_start=None, batch=None)
    for k in KEYS:
        assert same_bytes(got[k], other[k][at]), (name, k)


def _device_form(h, c, group_start, batch, outs=None):
    G, m, stride = c["prev"].shape
    cap = m if c["prefix_max"] is None else c["prefix_max"]
    o = outs or dict(state=D.Out((G, 8)), flags=D.Out((G,), np.int32), dev=D.Out((G, 3)), idx=D.Out((G, 3), np.int32), prefix=D.Out((G, cap, 8)),
                     prefix_n=D.Out((G,), np.int32), start=D.Out((batch, 3)), start_k=D.Out((batch,)), v_start=D.Out((batch,)))
    opt = lambda a: None if a is None else D.to_device(a, np.int32)
    rc = D.call(h, "pqp_stitch_trajectory_device", _prm(c).array(), c["keep"], cap, G, m, stride, D.to_device(c["prev"]), opt(c["m_of"]),
                D.to_device(c["meas"]), D.to_device(c["t_now"]), batch, opt(group_start), *(o[k] for k in KEYS))
    return rc, o


@pytest.mark.parametrize("name", ["m130_G67_s8_keep200_capNone", "m64_G5_s11_keep3_cap4", "ragged", "group_sizes", "nan_rows", "bad_measurements"])
def test_the_device_form_on_guarded_buffers_gives_the_host_form_s_bits(handle, name):
    c = BY_NAME[name]
    host = _host(handle, c)
    rc, o = _device_form(handle, c, c["group_start"], len(host["start_k"]))
    assert rc == 0, handle.lib.pqp_last_error()
    for k in KEYS:
        assert same_bytes(o[k].get(), host[k]), (name, k)


def test_the_device_form_reads_a_damaged_group_start_inside_its_batch(handle, restated):
    """what the host form refuses: boundaries outside [0, batch], a descending pair, candidates in no group - those keep what they held"""
    c = BY_NAME["group_sizes"]
    starts, batch = np.array([-4, 2, 5, 5, 300, 11], np.int32), 12          # groups [0, 2) [2, 5) empty [5, 12) empty (a descending pair)
    rc, o = _device_form(handle, c, starts, batch)
    assert rc == 0, handle.lib.pqp_last_error()
    state, start, start_k, v_start = o["state"].get(), o["start"].get(), o["start_k"].get(), o["v_start"].get()
    assert same_bytes(state, _host(handle, c)["state"])
    for b, g in enumerate([0, 0, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3]):
        assert same_bytes(start[b], state[g, :3]) and start_k[b] == state[g, 3] and v_start[b] == state[g, 5], b
    # candidates in no group: one group of two in a batch of five
    one = dict(c, prev=c["prev"][:1], meas=c["meas"][:1], t_now=c["t_now"][:1], m_of=c["m_of"][:1])
    rc, o = _device_form(handle, one, np.array([1, 3], np.int32), 5)
    assert rc == 0
    start_k = o["start_k"].get()
    assert (start_k[[0, 3, 4]] == D.SENT).all() and (start_k[1:3] == o["state"].get()[0, 3]).all()
    assert (o["start"].get()[[0, 3, 4]] == D.SENT).all() and (o["v_start"].get()[[0, 3, 4]] == D.SENT).all()


def test_optional_outputs_and_refusals_on_the_device(handle):
    c = BY_NAME["ragged"]
    G, m, _ = c["prev"].shape
    host = _host(handle, c)
    # without prefix, start, start_k: nothing is cut, prefix_n is the count, v_start alone is written
    o = dict(state=D.Out((G, 8)), flags=D.Out((G,), np.int32), dev=D.Out((G, 3)), idx=D.Out((G, 3), np.int32), prefix=None,
             prefix_n=D.Out((G,), np.int32), start=None, start_k=None, v_start=D.Out((G,)))
    rc, _ = _device_form(handle, dict(c, prefix_max=1), None, G, o)
    assert rc == 0, handle.lib.pqp_last_error()
    assert same_bytes(o["prefix_n"].get(), host["prefix_n"]) and same_bytes(o["flags"].get(), host["flags"]) and same_bytes(o["v_start"].get(), host["v_start"])
    # refused: nothing is launched, every output keeps what it held
    for over, batch in ((dict(keep=-1), G), (dict(prefix_max=0), G), (dict(prm=(0.1, -1.0) + U.DEFAULT[2:]), G), (dict(prm=(np.nan,) + U.DEFAULT[1:]), G),
                        ({}, G + 1)):
        rc, o = _device_form(handle, dict(c, **over), None, batch)
        assert rc == ERR_INVALID and handle.lib.pqp_last_error().decode().startswith("pqp_stitch_trajectory:"), over
        assert all(v.untouched() for v in o.values()), over
    # the host form also refuses a group_start that does not run from 0 to batch (the wrapper would refuse it first: the raw call)
    out = dict(state=np.full((G, 8), 7.0), flags=np.full(G, 7, np.int32), dev=np.full((G, 3), 7.0), idx=np.full((G, 3), 7, np.int32),
               prefix=np.full((G, m, 8), 7.0), prefix_n=np.full(G, 7, np.int32), start=np.full((G, 3), 7.0), start_k=np.full(G, 7.0), v_start=np.full(G, 7.0))
    starts = np.arange(G + 1, dtype=np.int32)
    starts[-1] -= 1
    rc = handle.lib.pqp_stitch_trajectory(handle._h, _prm(c).array(), c["keep"], m, G, m, c["prev"].shape[2], c["prev"], c["m_of"], c["meas"], c["t_now"], G,
                                          starts, *(out[k] for k in KEYS))
    assert rc == ERR_INVALID and handle.lib.pqp_last_error().decode().startswith("pqp_stitch_trajectory: group_start must")
    assert all((v == 7).all() for v in out.values())


def test_stitcher_gives_the_wrapper_s_bits(handle, tmp_path):
    exe = cpp_demo.build("stitch_demo")
    m, dt = 71, 0.1
    c = U.seeded_case(7, m, seed=21, dt=dt, ragged=False)
    c["prev"][:, :, 7] = np.arange(m).astype(np.float64) * np.float64(dt)            # state f at f dt, as the stitcher takes it
    c["m_of"][2], c["m_of"][5] = 1, 0
    for g in range(7):
        c["t_now"][g] = c["prev"][g, min(4 + g, max(int(c["m_of"][g]) - 2, 0)), 7] + 0.04
        c["meas"][g] = U.displaced(c["prev"][g, min(4 + g, max(int(c["m_of"][g]) - 2, 0))], 0.3, 0.1 if g != 3 else 0.9, 0.02, a=0.5, w=0.2)
    path = tmp_path / "case.bin"
    U.write_case(path, c["prev"], dt, c["m_of"], c["meas"], c["t_now"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = handle.stitch_trajectory(c["prev"], c["meas"], c["t_now"], m_of=c["m_of"])
    assert {U.STITCHED, U.LATERAL | U.REPLAN, U.NO_PREVIOUS | U.REPLAN} <= set(want["flags"].tolist())
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    at = 0
    for g in range(7):
        n = int(want["prefix_n"][g])
        assert lines[at][0] == "group" and [int(v) for v in lines[at][1:]] == [want["flags"][g], n]
        assert lines[at + 1][0] == "state" and same_bits(np.array([float(v) for v in lines[at + 1][1:]]), want["state"][g])
        assert lines[at + 2][0] == "dev" and same_bits(np.array([float(v) for v in lines[at + 2][1:]]), want["dev"][g])
        rows = lines[at + 3:at + 3 + n]
        assert all(l[0] == "prefix" for l in rows) and same_bits(np.array([[float(v) for v in l[1:]] for l in rows]).reshape(n, 8), want["prefix"][g, :n])
        at += 3 + n
    assert at == len(lines)


# ---- two cycles through the chain ---------------------------------------------------------------------------------------------------------------
def _measured_beside(best_traj, best_m, lat):
    """per group a car 40 % of the way from row 0 to row 1 of its plan, `lat` m to its left, at that time (a group without a plan: zeros)"""
    G = len(best_m)
    meas, t_now = np.zeros((G, 6)), np.zeros(G)
    for g in range(G):
        if best_m[g] >= 2:
            r0, r1 = best_traj[g, 0], best_traj[g, 1]
            at = r0 + 0.4 * (r1 - r0)
            at[2] = r0[2]
            meas[g], t_now[g] = U.displaced(at, 0.0, lat, 0.0), at[7]
    return meas, t_now


def _same_results(stitched, by_hand):
    assert [k for k in stitched if not k.startswith("stitch_")] == list(by_hand)
    for k, v in by_hand.items():
        assert same_bytes(stitched[k], v), k


def test_two_cycles_through_the_chain(hip_lib):
    """cycle 1 plans, ranks and samples its winners; cycle 2 starts on them through previous= and is, bit for bit in every key the two
    share, cycle 2 called with the restatement's start, start_k and v_start by hand.  A measurement 1 m beside the plan replans: that
    cycle starts from the advanced measurement.  Then the same with select= and speed=, where v_start is a row per group"""
    sc = chain_util.scenarios(4)
    h, hs = chain_util.handles(cases.B, max_n=(cases.N_MAX, cases.N_MAX))
    cf = cases.configs(hip_lib, sc["start"], sc["target"])
    common = dict(map_of=sc["map_of"], smoother=hs, cfg=h.chain_config(**cases.CHAIN_CONFIG))
    run = lambda start, kw: h.optimize_path(sc["pts"], sc["n_pts"], start, sc["target"], sc["dist"], sc["geom"], **dict(kw, **common))
    k = dict(cf["k"][1], rank_params=capi.rank_default_params(hip_lib, require_free=0))
    first = run(sc["start"], k)
    best_traj, best_m, gs = first["best_traj"], first["best_m"], np.array(cases.GROUP_START)
    assert best_traj.shape == (cases.GROUPS, cases.FINE, 8) and (best_m[[0, 2]] >= 2).all() and best_m[1] == 0, best_m
    again = {key: v for key, v in k.items() if key != "v_start"}
    spread = lambda rows: np.concatenate([np.repeat(rows[g:g + 1], gs[g + 1] - gs[g], axis=0) for g in range(cases.GROUPS)])

    meas, t_now = _measured_beside(best_traj, best_m, 0.1)
    want = U.stitch(best_traj, meas, t_now, m_of=best_m, group_start=gs, batch=cases.B)
    assert (want["flags"][[0, 2]] == U.STITCHED).all() and want["flags"][1] == U.NO_PREVIOUS | U.REPLAN | U.STANDING, want["flags"]
    assert (want["margins"] >= 1e-6).all(), want["margins"]
    second = run(None, dict(again, previous=(best_traj, best_m, meas, t_now, None)))
    assert list(second)[-5:] == ["stitch_state", "stitch_flags", "stitch_dev", "stitch_prefix", "stitch_prefix_n"]
    assert np.array_equal(second["stitch_flags"], want["flags"]) and np.array_equal(second["stitch_prefix_n"], want["prefix_n"])
    assert same_bits(second["stitch_state"][[0, 2]], want["state"][[0, 2]]) and same_bits(second["stitch_prefix"][[0, 2]], want["prefix"][[0, 2]])
    assert float(np.abs(second["stitch_dev"] - want["dev"]).max()) <= TOL and abs(abs(second["stitch_dev"][0, 1]) - 0.1) < 0.05
    _same_results(second, run(want["start"], dict(again, start_k=want["start_k"], v_start=want["v_start"])))

    meas, t_now = _measured_beside(best_traj, best_m, 1.0)
    want = U.stitch(best_traj, meas, t_now, m_of=best_m, group_start=gs, batch=cases.B)
    assert (want["flags"][[0, 2]] & ~U.STANDING == U.LATERAL | U.REPLAN).all() and (want["margins"] >= 1e-6).all(), (want["flags"], want["margins"])
    third = run(None, dict(again, previous=(best_traj, best_m, meas, t_now, None)))
    state = third["stitch_state"]
    assert np.array_equal(third["stitch_flags"], want["flags"]) and float(np.abs(state[:, :3] - want["state"][:, :3]).max()) <= TOL
    assert same_bits(state[:, 3:], want["state"][:, 3:]) and (third["stitch_prefix_n"] == 1).all()
    assert float(np.hypot(*(state[[0, 2], :2] - meas[[0, 2], :2]).T).max()) <= 0.1 * float(meas[:, 3].max()) + 0.5 * 0.5 * 0.01 + TOL      # v t + a t^2 / 2 away
    _same_results(third, run(spread(state[:, :3]), dict(again, start_k=spread(state[:, 3]), v_start=spread(state[:, 5]))))

    # select= with speed=: start and start_k a row per candidate, v_start a row per group
    hk = {key: v for key, v in cf["h"][1].items() if key != "v_start"}
    meas, t_now = _measured_beside(best_traj, best_m, 0.1)
    want = U.stitch(best_traj, meas, t_now, m_of=best_m, group_start=gs, batch=cases.B)
    fourth = run(None, dict(hk, previous=(best_traj, best_m, meas, t_now, None)))
    assert np.array_equal(fourth["stitch_flags"], want["flags"]) and same_bits(fourth["stitch_state"][:, 3:], want["state"][:, 3:])
    _same_results(fourth, run(want["start"], dict(hk, start_k=want["start_k"], v_start=want["state"][:, 5])))
    h.close(); hs.close()
