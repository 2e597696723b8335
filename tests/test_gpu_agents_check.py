"""pqp_agents_check on the GPU against the numpy restatement (tests/agents_util.py, known answers in tests/test_agents_check.py).

The frames' x, y, half_length, half_width, radius and reach are compared bit for bit, their cos and sin to 1e-15 (a few ulp of 1: what the
device's sincos may differ from libm's).  Clearances are compared to 1e-9 m: a few ulp in sin / cos times a lever arm below 10 m, plus
the rounding of coordinates up to 1e3 m, is below 1e-12 m, so 1e-9 leaves three orders of margin.  Hits are compared exactly except at
samples where some |clear(k, a) - margin| <= 1e-9 (tests/test_agents_check.py holds the seeds to at most 0.1 % of such samples), and
with heading 0 on dyadic numbers - the hand cases - everything is bit for bit, the grazing case included.

Shapes: the tile edges of m (1, 63, 64, 65, 130), the workgroup edge of the batch (1, 4, 5), 0, 1 and 3 agents with ragged counts, two
scenes, ragged m_of with 0, strides 3 and 8.  Then clearance = NULL against clearance given (the broad phase and the early exit must not
show; true hits at the very edge of the broad phase), position independence, hostile input, the refusals, the check behind the device chain and from C++."""
import ctypes as C
import functools
import math
import subprocess

import numpy as np
import pytest

import agents_util as A
import chain_util
import cpp_demo
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-9
MS, BATCHES, AGENTS = A.MS, A.BATCHES, A.AGENTS


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def circles():
    return capi.car_circles()


@functools.lru_cache(maxsize=None)
def _reference(m, B, a_max):
    """computed once per shape and shared; nobody writes to it"""
    c = A.seeded(m, B, a_max)
    return c, A.check(c["traj"], c["agents"], circles(), c["m_of"], c["a_of"], c["scene_of"], c["margin"])


def _host(handle, c, clearance=True, car=None):
    return handle.agents_check(c["traj"], c["agents"], m_of=c.get("m_of"), a_of=c.get("a_of"), scene_of=c.get("scene_of"), car=car,
                               prm=capi.agents_default_params(margin=c["margin"]), clearance=clearance)


def _device(handle, c, clearance=True, fill=-7.0, car=None):
    """the device form on outputs and a workspace that held `fill`: (frames, first_hit, hit_agent, clearance)"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    traj, agents = up(c["traj"], np.float64), up(c["agents"], np.float64)
    m_of, a_of, scene_of = (up(c.get(k), np.int32) for k in ("m_of", "a_of", "scene_of"))
    B, m, stride = c["traj"].shape
    n_scenes, a_max = c["agents"].shape[:2]
    frames = torch.full((n_scenes, a_max, m, 8), fill, dtype=torch.float64, device=dev)
    first = torch.full((B,), -7, dtype=torch.int32, device=dev)
    who = torch.full((B,), -7, dtype=torch.int32, device=dev)
    cl = torch.full((B, m), fill, dtype=torch.float64, device=dev) if clearance else None
    torch.cuda.synchronize(dev)
    prm = capi.agents_default_params(margin=c["margin"])
    car = car if car is not None else capi.car_default_geometry()
    handle._check(handle.lib.pqp_agents_check_device(handle._h, prm.margin, C.byref(car), B, m, stride, traj, m_of, n_scenes, a_max,
                                                     agents if a_max else None, a_of, scene_of, frames if a_max else None, first, who, cl))
    handle.sync()
    return frames.cpu().numpy(), first.cpu().numpy(), who.cpu().numpy(), None if cl is None else cl.cpu().numpy()


def _compare(got_first, got_who, got_clear, c, want, where=""):
    """first_hit / hit_agent / clearance of a launch against the restatement: clearances to TOL, hits exactly where no sample of the
    path is within TOL of the margin; returns the largest clearance difference seen"""
    near = A.near_margin(want["clear"], c["margin"], TOL)
    worst = 0.0
    for b in range(c["traj"].shape[0]):
        if got_clear is not None:
            w, g = want["clearance"][b], got_clear[b]
            fin = np.isfinite(w)
            assert np.array_equal(g[~fin], w[~fin]), (where, b)                                  # +inf, -inf and the zeros behind the count
            if fin.any():
                worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
            count = want["clear"][b].shape[0]
            below = np.nonzero(g[:count] < c["margin"])[0]                                       # the launch's own clearance decides its first_hit
            assert got_first[b] == (below[0] if below.size else count), (where, b)
        if not near[b].any():
            assert (got_first[b], got_who[b]) == (want["first_hit"][b], want["hit_agent"][b]), (where, b)
    assert worst <= TOL, (where, worst)
    return worst


# ---- the frames ------------------------------------------------------------------------------------------------------------------------
def test_frames_against_the_restatement(handle):
    rng = np.random.default_rng(7)
    traj, agents = A.seeded_case(rng, 2, 70, 3, 4, near=0.3)
    for at in ((0, 1, 5), (1, 2, 9), (2, 0, 11), (2, 3, 13), (0, 0, 30)):
        agents[at][3:5] = [1.0, 0.5]                         # present, whatever the seed said
    agents[0, 1, 5, 0] = math.nan                            # bad rows
    agents[1, 2, 9, 5] = -0.5
    agents[2, 0, 11, 2] = math.inf
    agents[2, 3, 13, 3] = math.nan
    agents[1, 0, 20, 4] = -1.0                               # absent, with what is then not read not a number
    agents[1, 0, 20, 1] = math.nan
    agents[0, 0, 30, 2] = 1e6                                # a heading of many turns
    c = dict(traj=traj, agents=agents, margin=0.0)
    got = _device(handle, c)[0]
    want = A.frames(agents)
    assert got.shape == want.shape == (3, 4, 70, 8)
    assert same_bits(got[..., [0, 1, 4, 5, 6, 7]], want[..., [0, 1, 4, 5, 6, 7]])
    d = float(np.abs(got[..., 2:4] - want[..., 2:4]).max())
    print(f"frames: max |cos, sin - libm| = {d:.3e}")
    assert d <= 1e-15
    absent, bad = want[..., 7] == -1.0, np.isnan(want[..., 7])
    assert absent.sum() >= 50 and bad.sum() == 4
    assert (got[absent][:, :7] == 0).all() and (got[bad][:, :7] == 0).all()


# ---- against the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_max", AGENTS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("m", MS)
def test_shapes_against_the_restatement(handle, m, B, a_max):
    c, want = _reference(m, B, a_max)
    got = _host(handle, c, clearance=True)
    worst = _compare(got["first_hit"], got["hit_agent"], got["clearance"], c, want, c["id"])
    print(f"{c['id']}: max |clearance - restatement| = {worst:.3e} m")
    quick = _host(handle, c, clearance=False)                # the broad phase and the early exit: the same answer
    assert np.array_equal(quick["first_hit"], got["first_hit"]) and np.array_equal(quick["hit_agent"], got["hit_agent"]), c["id"]
    _compare(quick["first_hit"], quick["hit_agent"], None, c, want, c["id"])


def test_every_optional_array_may_be_absent(handle):
    c, _ = _reference(65, 5, 3)
    for absent in (("m_of",), ("a_of",), ("scene_of",), ("m_of", "a_of", "scene_of")):
        d = {k: v for k, v in c.items() if k not in absent}
        want = A.check(d["traj"], d["agents"], circles(), d.get("m_of"), d.get("a_of"), d.get("scene_of"), d["margin"])
        got = _host(handle, d)
        _compare(got["first_hit"], got["hit_agent"], got["clearance"], d, want, absent)


# ---- the hand cases: bit for bit -------------------------------------------------------------------------------------------------------
def test_the_hand_cases_bit_for_bit(handle):
    import footprint_util as F
    car = capi.car_default_geometry(**A.HAND_CAR)
    hand = capi.car_circles(car)
    assert same_bits(hand, F.car_circles(**A.HAND_CAR))
    for name, c in A.hand_cases().items():
        want = A.check(c["traj"], c["agents"], hand, m_of=c.get("m_of"), margin=c["margin"])
        for clearance in (True, False):
            got = _host(handle, c, clearance=clearance, car=car)
            assert (got["first_hit"][0], got["hit_agent"][0]) == (want["first_hit"][0], want["hit_agent"][0]), (name, clearance)
            if clearance:
                assert same_bits(got["clearance"], want["clearance"]), name
    # the grazing pair, spelled out: exactly the margin is no hit, one ulp of the box's coordinate nearer is
    cases = A.hand_cases()
    assert _host(handle, cases["grazing"], car=car)["first_hit"][0] == A.HAND_M
    assert _host(handle, cases["grazing_one_ulp_nearer"], car=car)["first_hit"][0] == 0


# ---- clearance = NULL against clearance given ------------------------------------------------------------------------------------------
def test_the_shortcuts_do_not_show(handle):
    """agents that ride along just inside and just outside the broad phase's radius, and hits in the first tile with more behind it, in
    the second tile only, and nowhere"""
    rng = np.random.default_rng(99)
    B, m, a_max, margin = 6, 200, 6, 0.25
    traj, agents = A.seeded_case(rng, B, m, B, a_max, near=0.0)              # one scene per path; the seeded agents are far away
    cs = circles()
    rb = A.bounding_reach(cs)
    k = np.arange(m)
    for b in range(B):
        x, y, h = traj[b, :, 0], traj[b, :, 1], traj[b, :, 2]
        bx = cs[6][0] * np.cos(h) - cs[6][1] * np.sin(h) + x
        by = cs[6][0] * np.sin(h) + cs[6][1] * np.cos(h) + y
        for a, scale in ((0, 1.0 - 1e-7), (1, 1.0 + 1e-7), (2, 1.0)):         # discs at the radius itself and a hair to either side
            radius = 0.5
            far = rb + radius + margin + A.SLACK + A.SLACK_REL * (np.abs(bx) + np.abs(by)) * 2
            phi = 0.05 * k + a
            agents[b, a, :, 0], agents[b, a, :, 1] = bx + scale * far * np.cos(phi), by + scale * far * np.sin(phi)
            agents[b, a, :, 2:] = [0.3, 0.0, 0.0, radius]
        hit_at = {0: (10, 100, 150), 1: (70,), 2: (), 3: (63, 64), 4: (199,), 5: (0,)}[b]
        for a in (3, 4):                                                      # two boxes that sit on the car at those steps: the lower index wins
            agents[b, a, :, 3] = -1.0
            for at in hit_at:
                agents[b, a, at] = [x[at] + 1.0, y[at], h[at] + 0.2, 1.0, 0.5, 0.1]
    c = dict(traj=traj, agents=agents, margin=margin, scene_of=np.arange(B, dtype=np.int32))
    want = A.check(traj, agents, cs, scene_of=c["scene_of"], margin=margin)
    assert want["first_hit"].tolist() == [10, 70, m, 63, 199, 0] and want["hit_agent"].tolist() == [3, 3, -1, 3, 3, 3]
    full, quick = _host(handle, c, clearance=True), _host(handle, c, clearance=False)
    _compare(full["first_hit"], full["hit_agent"], full["clearance"], c, want, "full")
    assert np.array_equal(quick["first_hit"], full["first_hit"]) and np.array_equal(quick["hit_agent"], full["hit_agent"])
    assert quick["first_hit"].tolist() == want["first_hit"].tolist() and quick["hit_agent"].tolist() == want["hit_agent"].tolist()
    # the riders never come within the margin - by the slack at least - so leaving them out or not cannot show
    riders = np.stack([cl[:, :3] for cl in want["clear"]])
    assert (riders > margin + 0.5 * A.SLACK).all() and (riders < margin + 2.0 * rb).all()


def test_hits_at_the_edge_of_the_broad_phase_are_kept(handle):
    """true hits by 1e-6 m whose centres are as far from the bounding centre as a hitting agent's can be (agents_util.edge_cases): a
    broad phase with the reference's bounding radius for Rb, or without the margin or the rounding radius in its bound, would leave them
    out and lose each path's only hit (tests/test_agents_check.py shows that on the restatement)"""
    c = A.edge_cases(circles())
    want = A.check(c["traj"], c["agents"], circles(), scene_of=c["scene_of"], margin=c["margin"])
    assert np.array_equal(want["first_hit"], c["want_first"]) and np.array_equal(want["hit_agent"], c["want_who"])
    assert not any(n.any() for n in A.near_margin(want["clear"], c["margin"], TOL))      # 1e-6 from the margin: a thousand times the tolerance
    for clearance in (False, True):
        got = _host(handle, c, clearance=clearance)
        assert got["first_hit"].tolist() == c["want_first"].tolist() and got["hit_agent"].tolist() == c["want_who"].tolist(), clearance
    _compare(got["first_hit"], got["hit_agent"], got["clearance"], c, want, "edge")
    dev = _device(handle, c, clearance=False)
    assert dev[1].tolist() == c["want_first"].tolist() and dev[2].tolist() == c["want_who"].tolist()


# ---- position independence -------------------------------------------------------------------------------------------------------------
def test_same_bits_at_any_position_in_any_batch_from_either_form(handle):
    c, _ = _reference(130, 5, 3)
    first = _host(handle, c)
    rng = np.random.default_rng(5)
    src = 2                                                  # path 2 of scene 0
    for B, at in ((1, 0), (9, 7), (13, 4)):
        traj, agents = A.seeded_case(rng, B, 130, 3, 3, stride=c["traj"].shape[2])
        agents[1] = c["agents"][0]                           # its scene moves too
        traj[at] = c["traj"][src]
        m_of = rng.integers(0, 131, B).astype(np.int32)
        m_of[at] = c["m_of"][src]
        scene_of = rng.integers(0, 3, B).astype(np.int32)
        scene_of[at] = 1
        d = dict(traj=traj, agents=agents, m_of=m_of, a_of=np.array([2, c["a_of"][0], 3], np.int32), scene_of=scene_of, margin=c["margin"])
        got = _host(handle, d)
        assert got["first_hit"][at] == first["first_hit"][src] and got["hit_agent"][at] == first["hit_agent"][src], (B, at)
        assert same_bits(got["clearance"][at], first["clearance"][src]), (B, at)
        fr, f, w, cl = _device(handle, d)                    # outputs and a workspace that held -7: fully overwritten
        assert np.array_equal(f, got["first_hit"]) and np.array_equal(w, got["hit_agent"]) and same_bits(cl, got["clearance"]), (B, at)
        assert not (fr == -7.0).any()
        f2, w2 = _device(handle, d, clearance=False)[1:3]
        assert np.array_equal(f2, f) and np.array_equal(w2, w)


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def test_values_that_are_not_numbers_stay_in_their_path_and_scene(handle):
    c, _ = _reference(130, 5, 3)
    bad = dict(c, traj=c["traj"].copy(), agents=c["agents"].copy(), m_of=np.full(5, 130, np.int32))
    clean = _host(handle, dict(c, m_of=bad["m_of"]))
    bad["agents"][1, 0, 17, 3:5] = bad["agents"][1, 1, 5, 3:5] = [1.0, 0.5]             # present, whatever the seed said
    bad["traj"][2, 40, 0] = math.nan                         # path 2 (scene 0)
    bad["traj"][2, 90, 2] = -math.inf
    bad["agents"][1, 0, 17, 1] = math.inf                    # scene 1 (paths 1 and 3), agent 0
    bad["agents"][1, 1, 5, 5] = math.nan
    got = _host(handle, bad)
    want = A.check(bad["traj"], bad["agents"], circles(), bad["m_of"], bad["a_of"], bad["scene_of"], bad["margin"])
    _compare(got["first_hit"], got["hit_agent"], got["clearance"], bad, want, "hostile")
    for b in (0, 4):                                         # scene 0, their own rows clean: the same bits as before
        assert got["first_hit"][b] == clean["first_hit"][b] and got["hit_agent"][b] == clean["hit_agent"][b]
        assert same_bits(got["clearance"][b], clean["clearance"][b])
    assert got["clearance"][2, 40] == -math.inf and got["clearance"][2, 90] == -math.inf
    others = np.delete(np.arange(130), [40, 90])
    assert same_bits(got["clearance"][2, others], clean["clearance"][2, others])
    assert got["first_hit"][2] == min(40, clean["first_hit"][2])
    for b in (1, 3):
        assert got["clearance"][b, 5] == -math.inf and got["clearance"][b, 17] == -math.inf
        assert got["first_hit"][b] == min(5, clean["first_hit"][b])
        assert got["hit_agent"][b] == (1 if clean["first_hit"][b] > 5 else clean["hit_agent"][b])
    quick = _host(handle, bad, clearance=False)
    assert np.array_equal(quick["first_hit"], got["first_hit"]) and np.array_equal(quick["hit_agent"], got["hit_agent"])


def test_a_scene_outside_the_range_is_clamped_by_the_device_form(handle):
    """the device form cannot refuse what it does not read on the host: it clamps, and the answer is the clamped call's"""
    c, _ = _reference(65, 5, 3)
    wild = dict(c, scene_of=np.array([-5, 7, 2 ** 31 - 1, -2 ** 31, 1], np.int32))
    tame = dict(c, scene_of=np.array([0, 1, 1, 0, 1], np.int32))
    got, ref = _device(handle, wild), _device(handle, tame)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and same_bits(got[3], ref[3])
    want = A.check(wild["traj"], wild["agents"], circles(), wild["m_of"], wild["a_of"], wild["scene_of"], wild["margin"])
    _compare(got[1], got[2], got[3], wild, want, "clamped")
    with pytest.raises(capi.PqpError, match="pqp_agents_check: scene_of outside"):
        _host(handle, wild)                                  # the host form refuses them


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(handle):
    c, _ = _reference(63, 4, 1)
    traj, agents = np.ascontiguousarray(c["traj"]), np.ascontiguousarray(c["agents"])
    B, m, stride = traj.shape
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(batch=B, m_=m, stride_=stride, n_scenes=2, a_max=1, prm=None, car=None, drop=(), no_car=False, no_handle=False):
        first, who, cl = np.full(B, -7, np.int32), np.full(B, -7, np.int32), np.full((B, m), -7.0)
        args = dict(traj=p(traj), agents=p(agents), first=p(first), who=p(who))
        for k in drop:
            args[k] = None
        prm = prm or capi.agents_default_params()
        car = car or capi.car_default_geometry()
        rc = handle.lib.pqp_agents_check(None if no_handle else handle._h, prm.margin, None if no_car else C.byref(car), batch,
                                         m_, stride_, args["traj"], None, n_scenes, a_max, args["agents"], None, None, args["first"], args["who"], p(cl))
        return rc, (first == -7).all() and (who == -7).all() and (cl == -7.0).all(), handle.lib.pqp_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    bad = [dict(batch=0), dict(batch=-1), dict(m_=0), dict(stride_=2), dict(n_scenes=0), dict(a_max=-1), dict(n_scenes=2 ** 20, a_max=2 ** 20), dict(no_car=True),
           dict(no_handle=True)]
    bad += [dict(drop=(k,)) for k in ("traj", "agents", "first", "who")]
    bad += [dict(prm=capi.agents_default_params(margin=v)) for v in (-0.1, math.nan, math.inf)]
    bad += [dict(car=capi.car_default_geometry(width=math.nan)), dict(car=capi.car_default_geometry(front_length=math.inf))]
    for kw in bad:
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and msg.startswith("pqp_agents_check:"), (kw, rc, msg)
    # the device form refuses the same before it launches anything, and a missing workspace too
    import torch
    dev = torch.device("cuda", 0)
    d_traj, d_agents = torch.from_numpy(traj).to(dev), torch.from_numpy(agents).to(dev)
    d_frames = torch.full((2, 1, m, 8), -7.0, dtype=torch.float64, device=dev)
    d_first = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_who = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    car = capi.car_default_geometry()
    for kw in (dict(stride=2), dict(batch=0), dict(m=0), dict(n_scenes=0), dict(a_max=-1), dict(prm=capi.agents_default_params(margin=-1.0)),
               dict(frames=None), dict(agents=None)):
        prm = kw.get("prm") or capi.agents_default_params()
        rc = handle.lib.pqp_agents_check_device(handle._h, prm.margin, C.byref(car), kw.get("batch", B), kw.get("m", m), kw.get("stride", stride), d_traj,
                                                None, kw.get("n_scenes", 2), kw.get("a_max", 1), kw.get("agents", d_agents), None, None,
                                                kw.get("frames", d_frames), d_first, d_who, None)
        assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_agents_check:"), kw
    handle.sync()
    assert (d_frames.cpu().numpy() == -7.0).all() and (d_first.cpu().numpy() == -7).all() and (d_who.cpu().numpy() == -7).all()


# ---- through the layers ----------------------------------------------------------------------------------------------------------------
def test_the_check_behind_the_chain(hip_lib):
    """optimize_path(..., speed=, sample=, samples=, agents=) = the chain, the speed profile, the sampler and pqp_agents_check one after the
    other: what it adds equals the stand-alone host call on the traj it returns - on every candidate's samples, the parked car's included
    with hold_last, and with select on the winners' samples that lie on the path"""
    B, m = 16, 40
    sc = chain_util.scenarios(B)
    gs = np.array([0, 8, 16], np.int32)
    sp = capi.speed_default_params(v_max=8.0)
    # scene s: agent 0 drives from candidate s's target back to its start, agent 1 stands beside that start, agent 2 is a pedestrian far away
    lam = np.linspace(0.0, 1.0, m)
    agents = np.zeros((2, 3, m, 6))
    for s in range(2):
        st, tg = sc["start"][8 * s], sc["target"][8 * s]
        agents[s, 0, :, 0], agents[s, 0, :, 1] = tg[0] + lam * (st[0] - tg[0]), tg[1] + lam * (st[1] - tg[1])
        agents[s, 0, :, 2:] = [tg[2] + math.pi, 2.2, 0.9, 0.1]
        agents[s, 1, :] = [st[0] - 4.0 * math.sin(st[2]), st[1] + 4.0 * math.cos(st[2]), st[2], 2.0, 1.0, 0.0]
        agents[s, 2, :] = [st[0] + 500.0, st[1] - 300.0, 0.0, 0.0, 0.0, 0.4]
    agents[1, 1, ::7, 3] = -1.0
    ap = capi.agents_default_params(margin=0.2)
    a_of = np.array([3, 2], np.int32)
    scene_all, scene_grp = (np.arange(B) // 8).astype(np.int32), np.array([1, 0], np.int32)
    runs = {}
    for name, kw in (("all", dict(speed=sp, v_start=np.linspace(0.0, 6.0, B), sample=capi.sample_default_params(dt=0.2, hold_last=1), samples=m,
                                  agents=agents, agents_of=a_of, scene_of=scene_all, agents_params=ap)),
                     ("select", dict(select=gs, speed=sp, v_start=np.array([2.0, 5.0]), sample=capi.sample_default_params(dt=0.2), samples=m,
                                     agents=agents, agents_of=a_of, scene_of=scene_grp, agents_params=ap))):
        h, hs = chain_util.handles(B)
        if name == "all":
            with pytest.raises(ValueError, match="scene_of must have one entry per candidate"):
                h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                                **dict(kw, scene_of=scene_grp))
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **kw)
        h.close(); hs.close()
    every, sel = runs["all"], runs["select"]
    assert list(every)[-6:] == ["traj", "traj_n", "traj_flags", "first_hit", "hit_agent", "agent_clearance"]
    assert every["agent_clearance"].shape == (B, m) and sel["agent_clearance"].shape == (2, m)
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    want = h.agents_check(every["traj"], agents, m_of=None, a_of=a_of, scene_of=scene_all, prm=ap, clearance=True)
    assert np.array_equal(every["first_hit"], want["first_hit"]) and np.array_equal(every["hit_agent"], want["hit_agent"])
    assert same_bits(every["agent_clearance"], want["clearance"])
    want = h.agents_check(sel["traj"], agents, m_of=sel["traj_n"], a_of=a_of, scene_of=scene_grp, prm=ap, clearance=True)
    assert np.array_equal(sel["first_hit"], want["first_hit"]) and np.array_equal(sel["hit_agent"], want["hit_agent"])
    assert same_bits(sel["agent_clearance"], want["clearance"])
    h.close()
    ref = A.check(every["traj"], agents, circles(), None, a_of, scene_all, 0.2)
    worst = _compare(every["first_hit"], every["hit_agent"], every["agent_clearance"], dict(traj=every["traj"], margin=0.2), ref, "chain")
    print(f"behind the chain: max |clearance - restatement| = {worst:.3e} m; first_hit {every['first_hit'].tolist()}")
    assert np.isfinite(every["agent_clearance"]).all()


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_checker_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("agents_demo")
    c, _ = _reference(65, 5, 3)
    path = tmp_path / "case.bin"
    A.write_case(path, c["traj"], c["agents"], c["margin"], c["m_of"], c["a_of"], c["scene_of"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = _host(handle, dict(c, traj=np.ascontiguousarray(c["traj"][:, :, :3])))
    lines = iter(r.stdout.strip().splitlines())
    for b in range(5):
        head = next(lines).split()
        rows = int(c["m_of"][b])
        assert head[0] == "path" and [int(v) for v in head[1:]] == [b, want["first_hit"][b], want["hit_agent"][b], rows], (b, head)
        got = np.array([float(next(lines)) for _ in range(rows)])
        assert same_bits(got, want["clearance"][b, :rows]), b
    assert next(lines, None) is None
