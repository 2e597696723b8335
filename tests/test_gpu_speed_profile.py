"""pqp_speed_profile on the GPU against the restatement (tests/speed_util.py, known answers and the scan form in tests/test_speed_profile.py):
ragged batches at the counts where the kernel's tiles of 64 can go wrong, the tightest cap / a duplicate waypoint / a zero curvature /
the early stop on both sides of a tile edge, every optional pointer absent and present, hostile input, determinism, the refusals, and
the profile behind a path solve, behind the device chain and from C++.

What is compared with what (include/pqp.h states the definition):
  s      against the restatement within (c + 4) 2^-53 s_last: the re-ordered summation's (c - 1) u plus the rounding of a chord
  v      through v^2 against the restatement within 8 2^-53 (largest cap + 2 max(a_max, d_max) s_last)
  a, t   against the definition applied to the device's own s and v columns, within the same bounds (a: that of v^2 divided by d_i);
         and -d_max <= a_i <= a_max up to that
  flags  exactly: v_start is kept 1e-6 relative (or more) away from the limit at waypoint 0"""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import chain_util
import cpp_demo
import speed_util as V
from path_optimizer_2_amd import capi
from shared_util import same_bytes

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 700)
PLACES = (0, 63, 64, 65, -1)                                 # -1: c - 1
PRM = dict(v_max=12.0, a_max=1.2, d_max=2.5, a_lat_max=2.0)


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _cprm(prm=None):
    return capi.speed_default_params(**dict(V.DEFAULTS, **(prm or {})))


def _safe_v_start(path, want, **kw):
    """`want`, moved 1 % down when it sits within 1e-6 of what waypoint 0 allows - START_TOO_FAST is then no rounding question"""
    rows, flags = V.profile(path, 1e6, **kw)
    if flags & (V.EMPTY | V.NOT_FINITE):
        return want
    limit = rows[0, 1]
    return want * 0.99 if abs(want - limit) <= 2e-6 * limit else want


class Case:
    """paths of one launch: every per-path input, absent ones as None"""

    def __init__(self, n, stride, prm=None):
        self.n, self.stride, self.prm = n, stride, dict(PRM, **(prm or {}))
        self.paths, self.n_of, self.stop, self.lim, self.vs, self.ve = [], [], [], [], [], []

    def add(self, rng, count, stop=None, mark=None, v_end=math.nan, v_start=None):
        """a seeded path of `count` waypoints; mark(path, limit) edits it; the rows beyond count are noise"""
        p = rng.normal(size=(self.n, self.stride))
        if count > 0:
            p[:count] = V.seeded_path(rng, count, self.stride)
        lim = np.where(rng.random(self.n) < 0.1, rng.uniform(1.0, 8.0, self.n), math.inf)
        if mark is not None:
            mark(p, lim)
        stop = count if stop is None else stop
        want = float(rng.uniform(0.0, 9.0)) if v_start is None else v_start
        self.paths.append(p); self.n_of.append(count); self.stop.append(stop); self.lim.append(lim); self.ve.append(v_end)
        self.vs.append(_safe_v_start(p, want, n_of=count, stop_before=stop, v_limit=lim, v_end=v_end, prm=self.prm))
        return len(self.paths) - 1

    def arrays(self, absent=()):
        a = dict(paths=np.stack(self.paths), n_of=np.array(self.n_of, np.int32), stop_before=np.array(self.stop, np.int32),
                 v_limit=np.stack(self.lim), v_start=np.array(self.vs), v_end=np.array(self.ve))
        for k in absent:
            a[k] = None
        return a


def _run(handle, a, prm):
    return handle.speed_profile(a["paths"], a["v_start"], n_of=a["n_of"], stop_before=a["stop_before"], v_limit=a["v_limit"], v_end=a["v_end"],
                                prm=_cprm(prm))


def _check(got, a, prm):
    """every row of a launch against the restatement and the definition; returns the worst v^2 error in units of its bound / 8"""
    prof, flags = got
    prm = dict(V.DEFAULTS, **prm)
    B, n = a["paths"].shape[:2]
    pick = lambda k, b: None if a[k] is None else a[k][b]
    worst = 0.0
    for b in range(B):
        path = a["paths"][b]
        kw = dict(n_of=pick("n_of", b), stop_before=pick("stop_before", b), v_limit=pick("v_limit", b), v_end=pick("v_end", b), prm=prm)
        want, wf = V.profile(path, a["v_start"][b], **kw)
        count, c = V.driven(n, kw["n_of"], kw["stop_before"])
        rows = prof[b]
        assert flags[b] == wf, (b, c, flags[b], wf)
        assert (rows[c:] == 0.0).all() and not np.signbit(rows[c:]).any(), (b, c)
        if wf & V.NOT_FINITE:
            assert np.isnan(rows[:c]).all(), b
            continue
        if c == 0:
            continue
        assert np.isfinite(rows[:c, :3]).all(), (b, c)
        s_last = want[c - 1, 0]
        assert np.abs(rows[:c, 0] - want[:c, 0]).max() <= V.s_tolerance(c, s_last), (b, c)
        assert rows[0, 0] == 0.0 and rows[0, 3] == 0.0
        cap = V.caps(path, c, c < count, prm, a["v_start"][b], kw["v_end"], kw["v_limit"])
        tol = V.w_tolerance(cap, s_last, prm)
        err = np.abs(rows[:c, 1] ** 2 - want[:c, 1] ** 2).max()
        print(f"path {b}: c = {c}, |v^2 - restatement| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (b, c, err, tol)
        if tol > 0.0:
            worst = max(worst, err / (tol / 8))
        assert (rows[:c, 1] ** 2 <= cap + tol).all(), (b, c)
        # a and t: the definition on the device's own columns
        d = V.chords(path, c)
        a_def, dt, never = V.accel_and_time(d, rows[:c, 1] ** 2)
        moving = d > 0.0
        slack = np.zeros(c)
        slack[:c - 1][moving] = tol / d[moving]
        assert (np.abs(rows[:c, 2] - a_def) <= slack).all(), (b, c, np.abs(rows[:c, 2] - a_def).max())
        assert (rows[:c, 2] <= prm["a_max"] + slack).all() and (rows[:c, 2] >= -prm["d_max"] - slack).all(), (b, c)
        assert rows[c - 1, 2] == 0.0 and (rows[:c - 1, 2][~moving] == 0.0).all()
        t_def = np.concatenate([[0.0], np.cumsum(dt)])
        assert never == bool(wf & V.NEVER_ARRIVES)
        there = np.isfinite(t_def)
        assert np.array_equal(np.isinf(rows[:c, 3]), ~there) and (rows[:c, 3] >= 0).all(), (b, c)
        if there.any():
            t_last = t_def[there][-1]
            assert np.abs(rows[:c, 3][there] - t_def[there]).max() <= V.s_tolerance(c, t_last), (b, c)
        if there.all():
            assert (np.diff(rows[:c, 3])[~moving] == 0.0).all(), (b, c)
    return worst


# ---- the counts and the places ---------------------------------------------------------------------------------------------------------
def _ragged_case(stride):
    """every count with and without an early stop behind it, and the tightest cap of the path at every place around a tile edge"""
    rng = np.random.default_rng(101 + stride)
    case = Case(max(COUNTS) + 2, stride)
    for c in COUNTS:
        case.add(rng, c, v_end=[math.nan, 0.0, 3.0][c % 3])
        case.add(rng, c + 2, stop=c)                         # two more waypoints, not driven: the profile ends at rest at c - 1
    for c in (129, 200, 700):
        for at in PLACES:
            def tightest(p, lim, at=at % c):
                lim[at] = 0.4                                # far below every other cap: both passes start here
            case.add(rng, c, mark=tightest, v_end=2.0)
    return case


def _edge_case(stride):
    """a duplicate waypoint, a zero curvature among curved waypoints and the early stop at every place around a tile edge; stop_before 0, 1, c"""
    rng = np.random.default_rng(211 + stride)
    case = Case(max(COUNTS) + 2, stride)
    for c in (129, 200, 700):
        for at in PLACES:
            at = at % c

            def duplicate(p, lim, at=at, c=c):
                a, b = (at, at + 1) if at + 1 < c else (at - 1, at)
                p[b:c, 0:2] -= p[b, 0:2] - p[a, 0:2]         # waypoints a and b coincide, the rest of the path follows

            def straight(p, lim, at=at, c=c):
                p[:c, 5] = np.where(np.abs(p[:c, 5]) < 0.05, 0.08, p[:c, 5])       # every waypoint curved: v^2 <= 25 ...
                p[at, 5] = 0.0                                                      # ... but this one
                lim[:] = math.inf

            case.add(rng, c, mark=duplicate)
            case.add(rng, c, mark=straight, v_start=4.0)
    for at in (0, 63, 64, 65):
        case.add(rng, 200, stop=at + 1)                      # the stop itself at `at`: the backward carry starts there
    for stop in (0, 1, 200, 201, -3):
        case.add(rng, 200, stop=stop)
    case.add(rng, 2, v_start=0.0, v_end=0.0)                 # NEVER_ARRIVES
    return case


@pytest.mark.parametrize("stride", [6, 7])
@pytest.mark.parametrize("which", ["ragged", "edges"])
def test_counts_and_places_against_the_restatement(handle, which, stride):
    case = (_ragged_case if which == "ragged" else _edge_case)(stride)
    a = case.arrays()
    assert len(a["paths"]) <= 64
    got = _run(handle, a, case.prm)
    worst = _check(got, a, case.prm)
    print(f"{which}, stride {stride}: worst |v^2 - restatement| = {worst:.2f} units of 2^-53 (cap + 2 max(a, d) s); the bound is 8")
    flags = got[1]
    if which == "ragged":
        assert flags[0] == V.EMPTY and flags[1] == V.EMPTY | V.STOPS_EARLY
        assert all(flags[2 * i + 1] & V.STOPS_EARLY for i in range(len(COUNTS)))
    else:
        assert flags[-1] == V.NEVER_ARRIVES and flags[-2] == V.EMPTY | V.STOPS_EARLY == flags[-6]          # both ends at rest; stop_before -3, 0
        assert flags[-3] & V.STOPS_EARLY == 0 and flags[-4] & V.STOPS_EARLY == 0 and flags[-5] & V.STOPS_EARLY       # 201, 200 = c; 1


@pytest.mark.parametrize("absent", [(), ("n_of",), ("stop_before",), ("v_limit",), ("v_end",), ("n_of", "stop_before", "v_limit", "v_end")])
def test_every_optional_array_may_be_absent(handle, absent):
    rng = np.random.default_rng(307)
    case = Case(130, 7)
    for c, stop in ((130, 130), (130, 70), (64, 64), (130, 1), (1, 1), (130, 129)):
        case.add(rng, c, stop=stop, v_end=[math.nan, 1.5][c % 2])
    a = case.arrays(absent)
    _check(_run(handle, a, case.prm), a, case.prm)


def test_default_parameters_and_an_unbounded_lateral_acceleration(handle):
    rng = np.random.default_rng(311)
    for prm in ({}, dict(a_lat_max=math.inf), dict(v_max=0.0)):
        case = Case(90, 7, prm=dict(V.DEFAULTS, **prm))
        for c in (90, 66, 3):
            case.add(rng, c)
        a = case.arrays()
        got = handle.speed_profile(a["paths"], a["v_start"], n_of=a["n_of"], stop_before=a["stop_before"], v_limit=a["v_limit"], v_end=a["v_end"],
                                   prm=None if not prm else _cprm(case.prm))
        _check(got, a, case.prm)


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def test_values_that_are_not_numbers_stay_in_their_path(handle):
    rng = np.random.default_rng(401)
    case = Case(140, 7)
    for _ in range(9):
        case.add(rng, 140 - int(rng.integers(0, 12)))
    clean = case.arrays()
    want = _run(handle, clean, case.prm)
    assert (want[1] & V.NOT_FINITE == 0).all()
    bad = {k: (None if v is None else v.copy()) for k, v in clean.items()}
    bad["paths"][1, 64, 0] = math.nan                        # a NaN x
    bad["paths"][4, 3, 5] = math.inf                         # an Inf k
    bad["v_start"][7] = math.nan                             # a NaN v_start
    got = _run(handle, bad, case.prm)
    for b in range(9):
        c = int(clean["n_of"][b])
        if b in (1, 4, 7):
            assert got[1][b] == V.NOT_FINITE and np.isnan(got[0][b, :c]).all() and (got[0][b, c:] == 0).all(), b
        else:
            assert got[1][b] == want[1][b] and same_bytes(got[0][b], want[0][b]), b
    _check(got, bad, case.prm)
    # what is not read does no harm: behind the driven range, and a v_end of a path that stops early
    bad = {k: (None if v is None else v.copy()) for k, v in clean.items()}
    bad["stop_before"][:] = 60
    bad["paths"][:, 60:, :] = math.nan
    bad["v_limit"][:, 60:] = -1.0
    bad["v_end"][:] = -math.inf
    got = _run(handle, bad, case.prm)
    assert (got[1] & V.NOT_FINITE == 0).all() and (got[1] & V.STOPS_EARLY != 0).all() and np.isfinite(got[0]).all()
    _check(got, bad, case.prm)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def _device_form(handle, a, prm, fill=None):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d = {k: up(v) for k, v in a.items()}
    B, n, stride = a["paths"].shape
    prof = torch.full((B, n, 4), -7.0 if fill is None else fill, dtype=torch.float64, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    cp = _cprm(prm)
    handle._check(handle.lib.pqp_speed_profile_device(handle._h, C.byref(cp), B, n, stride, p(d["paths"]), p(d["n_of"]), p(d["stop_before"]),
                                                      p(d["v_limit"]), p(d["v_start"]), p(d["v_end"]), p(prof), p(flags)))
    handle.sync()
    return prof.cpu().numpy(), flags.cpu().numpy()


def test_same_bits_in_any_batch_and_from_either_form(handle):
    rng = np.random.default_rng(503)
    n = 210
    one = Case(n, 7)
    one.add(rng, 200, stop=190, v_end=1.0)
    alone = one.arrays()
    first = _run(handle, alone, one.prm)
    _check(first, alone, one.prm)
    for B, at in ((1, 0), (30, 17), (64, 63), (64, 0)):
        case = Case(n, 7)
        for b in range(B):
            case.add(rng, int(rng.integers(0, n + 1)))
        for lst, src in ((case.paths, one.paths), (case.n_of, one.n_of), (case.stop, one.stop), (case.lim, one.lim), (case.vs, one.vs),
                         (case.ve, one.ve)):
            lst[at] = src[0]
        a = case.arrays()
        got = _run(handle, a, case.prm)
        assert got[1][at] == first[1][0] and same_bytes(got[0][at], first[0][0]), (B, at)
        dev = _device_form(handle, a, case.prm)                      # outputs that held -7: fully overwritten
        assert same_bytes(dev[0], got[0]) and np.array_equal(dev[1], got[1]), (B, at)
        again = _run(handle, a, case.prm)
        assert same_bytes(again[0], got[0])
    # n is no part of the sums: the same path in a shorter row
    short = {k: (None if v is None else v.copy()) for k, v in alone.items()}
    short["paths"], short["v_limit"] = alone["paths"][:, :200], alone["v_limit"][:, :200]
    got = _run(handle, short, one.prm)
    assert same_bytes(got[0][0], first[0][0, :200]) and (first[0][0, 190:] == 0).all()


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(handle):
    rng = np.random.default_rng(601)
    B, n = 4, 20
    paths = np.stack([V.seeded_path(rng, n) for _ in range(B)])
    v_start = np.ones(B)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(batch=B, n_=n, stride=7, prm=None, drop=(), no_prm=False, no_handle=False):
        prof, flags = np.full((B, n, 4), -7.0), np.full(B, -7, np.int32)
        args = dict(paths=p(paths), v_start=p(v_start), profile=p(prof), flags=p(flags))
        for k in drop:
            args[k] = None
        prm = prm or capi.speed_default_params()
        rc = handle.lib.pqp_speed_profile(None if no_handle else handle._h, None if no_prm else C.byref(prm), batch, n_, stride, args["paths"], None,
                                          None, None, args["v_start"], None, args["profile"], args["flags"])
        return rc, (prof == -7.0).all() and (flags == -7).all(), handle.lib.pqp_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    bad = [dict(batch=0), dict(batch=-1), dict(n_=0), dict(stride=5), dict(no_prm=True), dict(no_handle=True)]
    bad += [dict(drop=(k,)) for k in ("paths", "v_start", "profile", "flags")]
    bad += [dict(prm=capi.speed_default_params(v_max=v)) for v in (math.nan, math.inf, -1.0)]
    bad += [dict(prm=capi.speed_default_params(**{k: v})) for k in ("a_max", "d_max") for v in (0.0, -1.0, math.inf, math.nan)]
    bad += [dict(prm=capi.speed_default_params(a_lat_max=v)) for v in (0.0, -1.0, math.nan)]
    for kw in bad:
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and msg.startswith("pqp_speed_profile:"), (kw, rc, msg)
    # the device form refuses the same before it launches anything
    import torch
    dev = torch.device("cuda", 0)
    d_paths, d_vs = torch.from_numpy(paths).to(dev), torch.from_numpy(v_start).to(dev)
    d_prof = torch.full((B, n, 4), -7.0, dtype=torch.float64, device=dev)
    d_flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    q = lambda x: C.c_void_p(x.data_ptr())
    for kw in (dict(stride=5), dict(batch=0), dict(n=0), dict(prm=capi.speed_default_params(d_max=0.0)), dict(v_start=None)):
        prm = kw.get("prm") or capi.speed_default_params()
        rc = handle.lib.pqp_speed_profile_device(handle._h, C.byref(prm), kw.get("batch", B), kw.get("n", n), kw.get("stride", 7), q(d_paths), None,
                                                 None, None, None if "v_start" in kw else q(d_vs), None, q(d_prof), q(d_flags))
        assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_speed_profile:"), kw
    handle.sync()
    assert (d_prof.cpu().numpy() == -7.0).all() and (d_flags.cpu().numpy() == -7).all()


# ---- through the layers ----------------------------------------------------------------------------------------------------------------
def test_a_path_solve_s_out_profiled_in_place(hip_lib):
    """8 QPs of N = 80: the solve writes `out` on the device, the profile reads it there (stride 7) - the same bits as from a host copy"""
    import torch
    from path_optimizer_2_amd.synth import make_batch
    dev = torch.device("cuda", 0)
    B, n = 8, 80
    b = make_batch(B, n)
    h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_ref, d_bounds, d_scal = up(b["ref"]), up(b["bounds"]), up(b["scal"])
    out = torch.zeros((B, n, 7), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    v_start = np.linspace(0.0, 7.0, B)
    d_vs = up(v_start)
    prof = torch.zeros((B, n, 4), dtype=torch.float64, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    h.solve_device(B, n, d_ref, d_bounds, d_scal, out, status=status)
    prm = capi.speed_default_params()
    q = lambda x: C.c_void_p(x.data_ptr())
    h._check(h.lib.pqp_speed_profile_device(h._h, C.byref(prm), B, n, 7, q(out), None, None, None, q(d_vs), None, q(prof), q(flags)))
    h.sync()
    paths = out.cpu().numpy()
    assert (status.cpu().numpy() == 1).all()
    got = prof.cpu().numpy(), flags.cpu().numpy()
    copy = h.speed_profile(paths.copy(), v_start)
    h.close()
    assert same_bytes(got[0], copy[0]) and np.array_equal(got[1], copy[1])
    a = dict(paths=paths, n_of=None, stop_before=None, v_limit=None, v_start=v_start, v_end=None)
    _check(got, a, V.DEFAULTS)
    assert (got[0][:, -1, 0] > 0).all() and (got[0][:, -1, 3] > 0).all()         # paths of some length, and time passes


def test_speed_behind_the_chain(hip_lib):
    """optimize_path(check_footprint=True, speed=...) = the chain, pqp_footprint_check and pqp_speed_profile one after the other; with select
    the winners' rows of best_paths are what is profiled"""
    B = 16
    sc = chain_util.scenarios(B)
    gs = np.array([0, 8, 16], np.int32)
    sp = capi.speed_default_params(v_max=8.0)
    vs_all, ve_all = np.linspace(0.0, 6.0, B), np.where(np.arange(B) % 2 == 0, 0.0, math.nan)
    vs_grp, ve_grp = np.array([2.0, 5.0]), np.array([math.nan, 0.0])
    runs = {}
    for name, kw in (("plain", dict()), ("all", dict(speed=sp, v_start=vs_all, v_end=ve_all)),
                     ("winners", dict(select=gs, winners_only=True, speed=sp, v_start=vs_grp, v_end=ve_grp))):
        h, hs = chain_util.handles(B)
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                                     check_footprint=True, **kw)
        h.close(); hs.close()
    plain, every, win = runs["plain"], runs["all"], runs["winners"]
    assert list(every) == list(plain) + ["profile", "speed_flags"]
    for k in plain:                                          # speed=None: as before; with it: the same paths
        assert same_bytes(plain[k], every[k]), k
    assert every["profile"].shape == every["out"].shape[:2] + (4,) and every["speed_flags"].shape == (B,)
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    fp = h.footprint_check(every["out"], every["n_out"], sc["dist"], sc["geom"], map_of=sc["map_of"])
    assert np.array_equal(fp["first_collision"], every["first_collision"])
    want = h.speed_profile(every["out"], vs_all, n_of=every["n_out"], stop_before=fp["first_collision"], v_end=ve_all, prm=sp)
    assert same_bytes(every["profile"], want[0]) and np.array_equal(every["speed_flags"], want[1])
    a = dict(paths=every["out"], n_of=every["n_out"], stop_before=every["first_collision"], v_limit=None, v_start=vs_all, v_end=ve_all)
    _check((every["profile"], every["speed_flags"]), a, dict(V.DEFAULTS, v_max=8.0))
    assert (every["speed_flags"] & V.NOT_FINITE == 0).all() and (every["profile"][:, :, 0].max(axis=1) > 0).any()
    assert np.array_equal((every["speed_flags"] & V.STOPS_EARLY) != 0, every["first_collision"] < every["n_out"])
    # the winners
    assert sorted(win) == sorted(["n_out", "status", "stage", "iters", "first_collision", "terms", "best", "best_paths", "best_n", "profile",
                                  "speed_flags"])
    assert win["profile"].shape == (2,) + every["out"].shape[1:2] + (4,) and (win["best"] >= 0).any()
    want = h.speed_profile(win["best_paths"], vs_grp, n_of=win["best_n"], v_end=ve_grp, prm=sp)
    h.close()
    assert same_bytes(win["profile"], want[0]) and np.array_equal(win["speed_flags"], want[1])
    for g in range(2):
        assert (win["speed_flags"][g] == V.EMPTY) == (win["best"][g] < 0)
        if win["best"][g] >= 0:                              # an eligible winner is collision-free: its whole path is driven
            assert same_bytes(win["best_paths"][g], every["out"][win["best"][g]]) and win["speed_flags"][g] & V.STOPS_EARLY == 0


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_profiler_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("speed_demo")
    rng = np.random.default_rng(701)
    counts = [30, 1, 64, 65, 0, 130]
    stops = [30, 1, 40, 65, 0, 129]
    n = max(counts)
    paths = np.zeros((len(counts), n, 7))
    for b, c in enumerate(counts):
        if c:
            paths[b, :c] = V.seeded_path(rng, c)
    v_start, v_end = rng.uniform(0.0, 5.0, len(counts)), np.array([math.nan, 0.5, math.nan, 0.0, 1.0, math.nan])
    path = tmp_path / "paths.bin"
    V.write_case(path, paths, counts, stops, v_start, v_end)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = handle.speed_profile(paths, v_start, n_of=counts, stop_before=stops, v_end=v_end)
    lines = iter(r.stdout.strip().splitlines())
    for b, c in enumerate(counts):
        head = next(lines).split()
        assert head[0] == "path" and int(head[1]) == b and int(head[2]) == want[1][b]
        rows = np.array([[float(v) for v in next(lines).split()] for _ in range(c)]).reshape(c, 4)
        driven = min(c, stops[b])
        assert same_bytes(rows[:driven], want[0][b, :driven]), b
        assert (rows[driven:] == 0.0).all()                  # states behind the stop keep the zeros they came with
    assert next(lines, None) is None
