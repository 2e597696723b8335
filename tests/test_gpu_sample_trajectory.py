"""pqp_sample_trajectory on the GPU against the numpy restatement (tests/sample_util.py, known answers in tests/test_sample_trajectory.py),
bit for bit: every operation of the definition (include/pqp.h) is a correctly rounded IEEE one on both sides, so there is no tolerance -
traj, m_of and the flags are compared exactly (NaN rows as NaN rows).

Ragged batches at the counts and sample counts where the kernel's tiles of 64 can go wrong, three regimes of dt (many samples in a
segment, about one, many waypoints between two samples), three strides, synthetic profiles and the device's own pqp_speed_profile output,
sample tiles that start on a waypoint-tile edge, t0 in every form, the arrival time to the ulp, a t column that steps back, a +inf tail,
stop_before around index 64, every optional pointer, hostile input, determinism, the refusals, and the samples behind a path solve,
behind the device chain and from C++."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import chain_util
import cpp_demo
import sample_util as S
import speed_util as V
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 2, 3, 63, 64, 65, 128, 129, 200, 700)
SAMPLES = (1, 2, 63, 64, 65, 130, 300)
# seconds per sample: a chord of 0.15 to 1 m at 0.5 to 8 m/s takes about 0.17 s
REGIMES = dict(fine=0.01, one_per_segment=0.17, coarse=40.0)


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _cprm(dt, hold_last=0):
    return capi.sample_default_params(dt=dt, hold_last=hold_last)


class Case:
    """paths of one launch: rows behind a path's count are noise"""

    def __init__(self, n, stride):
        self.n, self.stride = n, stride
        self.paths, self.prof, self.n_of, self.stop, self.t0 = [], [], [], [], []

    def add(self, rng, count, stop=None, t0=0.0, mark=None, profile=None):
        p, o = rng.normal(size=(self.n, self.stride)), rng.normal(size=(self.n, 4))
        if count > 0:
            p[:count] = S.seeded_path(rng, count, self.stride)
            o[:count] = S.seeded_profile(rng, p[:count]) if profile is None else profile(p[:count])
        if mark is not None:
            mark(p, o)
        self.paths.append(p); self.prof.append(o); self.n_of.append(count); self.stop.append(count if stop is None else stop); self.t0.append(t0)
        return len(self.paths) - 1

    def arrays(self, absent=()):
        a = dict(paths=np.stack(self.paths), profile=np.stack(self.prof), n_of=np.array(self.n_of, np.int32),
                 stop_before=np.array(self.stop, np.int32), t0=np.array(self.t0, np.float64))
        for k in absent:
            a[k] = None
        return a


def _run(handle, a, m, dt, hold_last=0):
    return handle.sample_trajectory(a["paths"], a["profile"], m, n_of=a["n_of"], stop_before=a["stop_before"], t0=a["t0"], prm=_cprm(dt, hold_last))


def _check(got, a, m, dt, hold_last=0):
    """every path of a launch against the restatement, bit for bit"""
    traj, m_of, flags = got
    want = S.sample_batch(a["paths"], a["profile"], m, a["n_of"], a["stop_before"], a["t0"], dt, hold_last)
    assert traj.shape == (len(a["paths"]), m, 8)
    for b in range(len(a["paths"])):
        assert flags[b] == want[2][b] and m_of[b] == want[1][b], (b, flags[b], want[2][b], m_of[b], want[1][b])
        if not same_bits(traj[b], want[0][b]):
            diff = np.argwhere(traj[b].view(np.uint64) != want[0][b].view(np.uint64))
            k, col = diff[0]
            raise AssertionError(f"path {b}: {len(diff)} cells differ, first at sample {k} column {col}: {traj[b, k, col]!r} != {want[0][b, k, col]!r}")
    return want


# ---- the counts, the sample counts, the strides and the regimes ---------------------------------------------------------------------------
def _ragged(rng, stride, dt):
    case = Case(max(COUNTS) + 2, stride)
    for c in COUNTS:
        case.add(rng, c, t0=[0.0, 0.0, 0.37, 3.0 * dt][c % 4])
    case.add(rng, 202, stop=200, t0=0.0)
    case.add(rng, 702, stop=64, t0=1.0)
    return case


@pytest.mark.parametrize("stride", [6, 7, 9])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_counts_and_sample_counts_against_the_restatement(handle, regime, stride):
    dt = REGIMES[regime]
    rng = np.random.default_rng(1000 + 10 * stride + list(REGIMES).index(regime))
    a = _ragged(rng, stride, dt).arrays()
    seen = 0
    for m in SAMPLES:
        for hold in ((0, 1) if m in (2, 65, 300) else (0,)):
            want = _check(_run(handle, a, m, dt, hold), a, m, dt, hold)
            seen |= int(np.bitwise_or.reduce(want[2]))
            assert want[2][0] == S.EMPTY
    assert seen & S.ENDS_MOVING and seen & S.HORIZON_SHORT and seen & S.EMPTY
    if regime == "coarse":                                   # c = 700, m = 3: one sample tile walks over several waypoint tiles
        T = a["profile"][10, :700, 3].max()
        assert 40.0 > a["profile"][10, 64, 3] and 80.0 > a["profile"][10, 192, 3] and T > 80.0


def test_on_the_device_s_own_speed_profile(handle):
    rng = np.random.default_rng(1101)
    n = 702
    counts = COUNTS + (702, 300)
    stops = list(counts[:-2]) + [640, 65]
    paths = rng.normal(size=(len(counts), n, 7))
    for b, c in enumerate(counts):
        if c:
            paths[b, :c] = V.seeded_path(rng, c)
            paths[b, :c, 2] = S.constrain_angle(np.cumsum(paths[b, :c, 5] * 0.5) + 3.0)
    v_start = rng.uniform(0.0, 2.0, len(counts))
    v_end = np.where(np.arange(len(counts)) % 2 == 0, 0.0, math.nan)
    prof, sf = handle.speed_profile(paths, v_start, n_of=counts, stop_before=stops, v_end=v_end)
    assert (sf & V.NOT_FINITE == 0).all()
    a = dict(paths=paths, profile=prof, n_of=np.array(counts, np.int32), stop_before=np.array(stops, np.int32), t0=None)
    flags = 0
    for m, dt, hold in ((130, 0.01, 0), (300, 0.5, 1), (65, 2.0, 0), (3, 60.0, 0), (64, 0.1, 1)):
        want = _check(_run(handle, a, m, dt, hold), a, m, dt, hold)
        flags |= int(np.bitwise_or.reduce(want[2]))
        assert (want[1][1:] > 0).all()                       # t_0 = 0: sample 0 is always on the path
    assert flags & S.HORIZON_SHORT


def _dyadic(n, per_second=4):
    """a path whose waypoint i is reached at i / per_second exactly, at 2 m/s with s = i / 2 by decree"""
    phi = np.linspace(0.0, 2.5, n)
    p = np.zeros((n, 7))
    p[:, 0], p[:, 1], p[:, 2], p[:, 5] = 40 * np.sin(phi), 40 * (1 - np.cos(phi)), phi, 0.025
    o = np.zeros((n, 4))
    o[:, 0], o[:, 1], o[:, 3] = np.arange(n) * 2.0 / per_second, 2.0, np.arange(n) / per_second
    return p, o


def test_sample_tiles_that_start_on_a_waypoint_tile_edge(handle):
    n = 200
    p, o = _dyadic(n)
    rows = np.concatenate([p[:, [0, 1, 2, 5]], o], axis=1)
    rows[:, 6] = 0.0
    a = dict(paths=p[None], profile=o[None], n_of=None, stop_before=None, t0=None)
    traj, m_of, flags = _run(handle, a, 130, 0.25)           # sample k = waypoint k: sample 64 opens the second tile on waypoint 64
    _check((traj, m_of, flags), a, 130, 0.25)
    assert m_of[0] == 130 and flags[0] == S.HORIZON_SHORT and same_bits(traj[0], rows[:130])
    traj, m_of, flags = _run(handle, a, 130, 0.5)            # sample k = waypoint 2 k: sample 64 on waypoint 128, sample 99 on the last
    _check((traj, m_of, flags), a, 130, 0.5)
    assert m_of[0] == 100 and flags[0] == S.ENDS_MOVING and same_bits(traj[0, :100], rows[::2]) and (traj[0, 100:] == 0).all()
    for t0 in (16.0, 15.75, 32.0, 49.75):                    # sample 0 itself on waypoints 64, 63, 128 and the last
        a["t0"] = np.array([t0])
        traj, m_of, flags = _run(handle, a, 66, 0.25)
        _check((traj, m_of, flags), a, 66, 0.25)
        k = int(t0 * 4)
        assert m_of[0] == min(66, n - k) and same_bits(traj[0, :m_of[0]], rows[k:k + 66])


# ---- t0, the arrival, the t column ----------------------------------------------------------------------------------------------------
def test_t0_absent_zero_positive_and_behind_the_arrival(handle):
    rng = np.random.default_rng(1201)
    case = Case(131, 7)
    for c in (130, 64, 3, 131):
        case.add(rng, c)
    a = case.arrays()
    zero = _run(handle, a, 70, 0.1)
    _check(zero, a, 70, 0.1)
    absent = _run(handle, dict(a, t0=None), 70, 0.1)
    assert all(same_bits(x, y) for x, y in zip(zero, absent))
    arrive = np.array([a["profile"][b, :c, 3].max() for b, c in enumerate((130, 64, 3, 131))])
    a["t0"] = np.array([0.4, 2.0, arrive[2] + 1.0, np.nextafter(arrive[3], math.inf)])
    got = _run(handle, a, 70, 0.1, 1)
    _check(got, a, 70, 0.1, 1)
    assert got[1][2] == 0 and got[1][3] == 0 and got[1][0] > 0
    assert np.array_equal(got[0][3, :, 7], a["t0"][3] + np.arange(70.0) * 0.1) and (got[0][3, :, 5] == 0).all()      # held at rest


def test_the_arrival_time_to_the_ulp(handle):
    rng = np.random.default_rng(1301)
    dt, m = 0.3, 40
    tau = np.arange(m).astype(np.float64) * dt
    case = Case(90, 7)
    for c, k in ((90, 17), (65, 39), (2, 1)):
        for less in (False, True):
            def arrive_at(p, o, c=c, k=k, less=less):
                o[:c, 3] *= tau[k] / o[c - 1, 3]             # the arrival lands near tau_k ...
                o[c - 1, 3] = np.nextafter(tau[k], 0.0) if less else tau[k]      # ... then on it, or one ulp in front
                o[:c - 1, 3] = np.minimum(o[:c - 1, 3], o[c - 1, 3])
            case.add(rng, c, mark=arrive_at)
    a = case.arrays()
    got = _run(handle, a, m, dt)
    _check(got, a, m, dt)
    assert got[1].tolist() == [18, 17, 40, 39, 2, 1]
    assert (got[2][[2]] == 0).all() and got[2][3] == S.ENDS_MOVING          # arriving on the last sample exactly is inside the horizon


def test_a_t_column_that_steps_back_and_a_tail_of_inf(handle):
    rng = np.random.default_rng(1401)
    case = Case(140, 7)
    for at in (5, 63, 64, 100):
        def duplicate(p, o, at=at):
            p[at + 1:140] = p[at:139].copy()                 # waypoints at and at + 1 coincide, the rest follows
            o[at + 1:140] = o[at:139].copy()
            o[at + 1, 3] = np.nextafter(o[at, 3], 0.0)       # ... and the scan's t steps back by an ulp there
            o[at, 2] = 0.0
        case.add(rng, 140, mark=duplicate)
    for at in (1, 64, 65, 139):
        def tail(p, o, at=at):
            o[at:, 3] = math.inf                             # the car stands at waypoint at - 1
            o[at - 1:, 1] = 0.0
            o[at - 1:, 2] = 0.0
        case.add(rng, 140, mark=tail)
    a = case.arrays()
    for m, dt in ((300, 0.1), (65, 0.5)):                    # 30 s: behind waypoint 138's time
        got = _run(handle, a, m, dt)
        _check(got, a, m, dt)
        for b in range(4):
            on = got[0][b, :got[1][b]]
            assert (np.diff(on[:, 4]) >= -1e-12).all()                           # nothing moves backwards at the step
        assert (got[2][4:] == S.STANDS | S.HORIZON_SHORT).all() and (got[1][4:] == m).all()
    # a sample between the two stamps of the duplicate is in front of both: the running maximum decides
    at = 63
    a1 = {k: (None if v is None else v[1:2].copy()) for k, v in a.items()}
    a1["t0"] = np.array([a["profile"][1, at + 1, 3]])
    got = _run(handle, a1, 1, 0.1)
    _check(got, a1, 1, 0.1)
    assert a["profile"][1, at - 1, 0] < got[0][0, 0, 4] <= a["profile"][1, at, 0] and got[0][0, 0, 6] == a["profile"][1, at - 1, 2]


def test_stop_before_on_both_sides_of_a_tile_edge(handle):
    rng = np.random.default_rng(1501)
    case = Case(130, 7)
    for stop in (63, 64, 65, 0, -2, 1, 130, 131):
        case.add(rng, 130, stop=stop)
    a = case.arrays()
    for m, dt in ((130, 0.2), (64, 0.5)):
        got = _run(handle, a, m, dt, 1)
        want = _check(got, a, m, dt, 1)
        assert (want[2][[3, 4]] == S.EMPTY).all()
        for b, stop in enumerate((63, 64, 65)):              # held at waypoint stop - 1 behind its arrival
            assert got[1][b] < m and np.array_equal(got[0][b, -1, :2], a["paths"][b, stop - 1, :2])


@pytest.mark.parametrize("absent", [(), ("n_of",), ("stop_before",), ("t0",), ("n_of", "stop_before", "t0")])
def test_every_optional_array_may_be_absent(handle, absent):
    rng = np.random.default_rng(1601)
    case = Case(130, 9)
    for c, stop, t0 in ((130, 130, 0.0), (130, 70, 0.5), (64, 64, 0.0), (130, 1, 0.25), (1, 1, 0.0), (100, 129, 2.0)):
        case.add(rng, c, stop=stop, t0=t0)
    a = case.arrays(absent)
    if "n_of" in absent:                                     # then every row up to n is read: no noise behind the counts
        for b in range(len(case.paths)):
            a["paths"][b] = S.seeded_path(rng, 130, 9)
            a["profile"][b] = S.seeded_profile(rng, a["paths"][b])
    _check(_run(handle, a, 65, 0.2), a, 65, 0.2)
    got = handle.sample_trajectory(a["paths"], a["profile"], 12, n_of=a["n_of"], stop_before=a["stop_before"], t0=a["t0"])       # prm absent: the defaults
    _check(got, a, 12, 0.1, 0)


# ---- hostile input ---------------------------------------------------------------------------------------------------------------------
def test_values_that_are_not_numbers_stay_in_their_path(handle):
    rng = np.random.default_rng(1701)
    case = Case(140, 7)
    for b in range(13):
        case.add(rng, 140 - int(rng.integers(0, 12)), t0=0.1 * b)
    clean = case.arrays()
    m, dt = 130, 0.15
    want = _run(handle, clean, m, dt)
    assert (want[2] & S.NOT_FINITE == 0).all()
    bad = {k: v.copy() for k, v in clean.items()}
    hostile = {0: ("paths", (64, 0), math.nan), 1: ("paths", (3, 1), math.inf), 2: ("paths", (127, 2), -math.inf), 3: ("paths", (0, 5), math.nan),
               5: ("profile", (65, 0), math.inf), 6: ("profile", (2, 1), math.nan), 7: ("profile", (63, 2), math.inf),
               8: ("profile", (100, 3), math.nan), 9: ("profile", (1, 3), -1e-300), 11: ("t0", (), math.nan), 12: ("t0", (), -1.0)}
    for b, (k, where, value) in hostile.items():
        bad[k][(b,) + where] = value
    got = _run(handle, bad, m, dt)
    _check(got, bad, m, dt)
    for b in range(13):
        if b in hostile:
            assert got[2][b] == S.NOT_FINITE and got[1][b] == 0 and np.isnan(got[0][b]).all(), b
        else:
            assert got[2][b] == want[2][b] and got[1][b] == want[1][b] and same_bits(got[0][b], want[0][b]), b
    # a launch without the hostile paths: the neighbours' bits are the same
    keep = [b for b in range(13) if b not in hostile]
    alone = _run(handle, {k: v[keep] for k, v in clean.items()}, m, dt)
    assert same_bits(alone[0], got[0][keep]) and np.array_equal(alone[1], got[1][keep]) and np.array_equal(alone[2], got[2][keep])
    inf_t0 = dict(clean, t0=np.where(np.arange(13) == 4, math.inf, clean["t0"]))
    got = _run(handle, inf_t0, m, dt)
    assert got[2][4] == S.NOT_FINITE and same_bits(got[0][keep[1:]], want[0][keep[1:]])
    # what is not read does no harm: behind the driven range
    bad = {k: v.copy() for k, v in clean.items()}
    bad["stop_before"][:] = 60
    bad["paths"][:, 60:, :] = math.nan
    bad["profile"][:, 60:, :] = -math.inf
    got = _run(handle, bad, m, dt)
    assert (got[2] & S.NOT_FINITE == 0).all() and np.isfinite(got[0]).all()
    _check(got, bad, m, dt)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def _device_form(handle, a, m, dt, hold_last=0, fill=-7.0):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d = {k: up(v) for k, v in a.items()}
    B, n, stride = a["paths"].shape
    traj = torch.full((B, m, 8), fill, dtype=torch.float64, device=dev)
    m_of = torch.full((B,), -7, dtype=torch.int32, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    cp = _cprm(dt, hold_last)
    handle._check(handle.lib.pqp_sample_trajectory_device(handle._h, C.byref(cp), B, n, stride, p(d["paths"]), p(d["n_of"]), p(d["stop_before"]),
                                                          p(d["profile"]), p(d["t0"]), m, p(traj), p(m_of), p(flags)))
    handle.sync()
    return traj.cpu().numpy(), m_of.cpu().numpy(), flags.cpu().numpy()


def test_same_bits_in_any_batch_for_any_n_and_m_and_from_either_form(handle):
    rng = np.random.default_rng(1801)
    n, m, dt = 210, 130, 0.12
    one = Case(n, 7)
    one.add(rng, 200, stop=190, t0=0.7)
    alone = one.arrays()
    first = _run(handle, alone, m, dt)
    _check(first, alone, m, dt)
    for B, at in ((1, 0), (30, 17), (33, 32), (33, 0)):
        case = Case(n, 7)
        for b in range(B):
            case.add(rng, int(rng.integers(0, n + 1)), t0=float(rng.uniform(0, 3)))
        for lst, src in ((case.paths, one.paths), (case.prof, one.prof), (case.n_of, one.n_of), (case.stop, one.stop), (case.t0, one.t0)):
            lst[at] = src[0]
        a = case.arrays()
        got = _run(handle, a, m, dt)
        assert got[2][at] == first[2][0] and got[1][at] == first[1][0] and same_bits(got[0][at], first[0][0]), (B, at)
        dev = _device_form(handle, a, m, dt)                 # outputs that held -7: fully overwritten
        assert same_bits(dev[0], got[0]) and np.array_equal(dev[1], got[1]) and np.array_equal(dev[2], got[2]), (B, at)
    # n is no part of a sample: the same path in a shorter row; nor is m: a longer horizon shares the prefix
    short = dict(alone, paths=alone["paths"][:, :195], profile=alone["profile"][:, :195])
    got = _run(handle, short, m, dt)
    assert same_bits(got[0], first[0]) and got[1][0] == first[1][0]
    for m2 in (131, 300):
        got = _run(handle, alone, m2, dt)
        assert same_bits(got[0][:, :m], first[0]) and got[1][0] >= first[1][0]


# ---- what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(handle):
    rng = np.random.default_rng(1901)
    B, n, m = 4, 20, 9
    paths = np.stack([S.seeded_path(rng, n) for _ in range(B)])
    prof = np.stack([S.seeded_profile(rng, paths[b]) for b in range(B)])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(batch=B, n_=n, stride=7, m_=m, prm=None, drop=(), no_prm=False, no_handle=False):
        traj, m_of, flags = np.full((B, m, 8), -7.0), np.full(B, -7, np.int32), np.full(B, -7, np.int32)
        args = dict(paths=p(paths), profile=p(prof), traj=p(traj), m_of=p(m_of), flags=p(flags))
        for k in drop:
            args[k] = None
        prm = prm or capi.sample_default_params()
        rc = handle.lib.pqp_sample_trajectory(None if no_handle else handle._h, None if no_prm else C.byref(prm), batch, n_, stride, args["paths"],
                                              None, None, args["profile"], None, m_, args["traj"], args["m_of"], args["flags"])
        return rc, (traj == -7.0).all() and (m_of == -7).all() and (flags == -7).all(), handle.lib.pqp_last_error().decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched
    bad = [dict(batch=0), dict(batch=-1), dict(n_=0), dict(m_=0), dict(m_=-3), dict(stride=5), dict(no_prm=True), dict(no_handle=True)]
    bad += [dict(drop=(k,)) for k in ("paths", "profile", "traj", "m_of", "flags")]
    bad += [dict(prm=capi.sample_default_params(dt=v)) for v in (0.0, -0.1, math.nan, math.inf)]
    bad += [dict(prm=capi.sample_default_params(hold_last=v)) for v in (2, -1)]
    for kw in bad:
        rc, untouched, msg = call(**kw)
        assert rc == -1 and untouched and msg.startswith("pqp_sample_trajectory:"), (kw, rc, msg)
    # the device form refuses the same before it launches anything
    import torch
    dev = torch.device("cuda", 0)
    d_paths, d_prof = torch.from_numpy(paths).to(dev), torch.from_numpy(prof).to(dev)
    d_traj = torch.full((B, m, 8), -7.0, dtype=torch.float64, device=dev)
    d_m_of = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    q = lambda x: C.c_void_p(x.data_ptr())
    for kw in (dict(stride=5), dict(batch=0), dict(n=0), dict(m=0), dict(prm=capi.sample_default_params(dt=0.0)),
               dict(prm=capi.sample_default_params(hold_last=3)), dict(profile=None)):
        prm = kw.get("prm") or capi.sample_default_params()
        rc = handle.lib.pqp_sample_trajectory_device(handle._h, C.byref(prm), kw.get("batch", B), kw.get("n", n), kw.get("stride", 7), q(d_paths),
                                                     None, None, None if "profile" in kw else q(d_prof), None, kw.get("m", m), q(d_traj),
                                                     q(d_m_of), q(d_flags))
        assert rc == -1 and handle.lib.pqp_last_error().decode().startswith("pqp_sample_trajectory:"), kw
    handle.sync()
    assert (d_traj.cpu().numpy() == -7.0).all() and (d_m_of.cpu().numpy() == -7).all() and (d_flags.cpu().numpy() == -7).all()


# ---- through the layers ----------------------------------------------------------------------------------------------------------------
def test_a_path_solve_s_out_sampled_in_place(hip_lib):
    """8 QPs of N = 80: the solve writes `out` on the device, the profile and the samples read it there (stride 7) - the same bits as
    from host copies, and the restatement's"""
    import torch
    from path_optimizer_2_amd.synth import make_batch
    dev = torch.device("cuda", 0)
    B, n, m = 8, 80, 50
    b = make_batch(B, n)
    h = capi.Handle(capi.production_params(), device=0, max_batch=B, max_n=n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_ref, d_bounds, d_scal = up(b["ref"]), up(b["bounds"]), up(b["scal"])
    out = torch.zeros((B, n, 7), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    v_start = np.linspace(0.0, 7.0, B)
    d_vs = up(v_start)
    prof = torch.zeros((B, n, 4), dtype=torch.float64, device=dev)
    sflags = torch.zeros(B, dtype=torch.int32, device=dev)
    traj = torch.zeros((B, m, 8), dtype=torch.float64, device=dev)
    m_of = torch.zeros(B, dtype=torch.int32, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    h.solve_device(B, n, d_ref, d_bounds, d_scal, out, status=status)
    sp, sa = capi.speed_default_params(), capi.sample_default_params()
    q = lambda x: C.c_void_p(x.data_ptr())
    h._check(h.lib.pqp_speed_profile_device(h._h, C.byref(sp), B, n, 7, q(out), None, None, None, q(d_vs), None, q(prof), q(sflags)))
    h._check(h.lib.pqp_sample_trajectory_device(h._h, C.byref(sa), B, n, 7, q(out), None, None, q(prof), None, m, q(traj), q(m_of), q(flags)))
    h.sync()
    assert (status.cpu().numpy() == 1).all()
    paths, profile = out.cpu().numpy(), prof.cpu().numpy()
    got = traj.cpu().numpy(), m_of.cpu().numpy(), flags.cpu().numpy()
    copy = h.sample_trajectory(paths.copy(), profile.copy(), m)
    h.close()
    assert same_bits(got[0], copy[0]) and np.array_equal(got[1], copy[1]) and np.array_equal(got[2], copy[2])
    _check(got, dict(paths=paths, profile=profile, n_of=None, stop_before=None, t0=None), m, 0.1)
    assert (got[1] > 0).all() and (got[0][:, 1, 4] >= 0).all()


def test_samples_behind_the_chain(hip_lib):
    """optimize_path(check_footprint=True, speed=..., sample=...) = the chain, pqp_footprint_check, pqp_speed_profile and
    pqp_sample_trajectory one after the other; with select the winners' rows of best_paths are what is sampled"""
    B, m = 16, 40
    sc = chain_util.scenarios(B)
    gs = np.array([0, 8, 16], np.int32)
    sp, sa = capi.speed_default_params(v_max=8.0), capi.sample_default_params(dt=0.2, hold_last=1)
    vs_all, vs_grp = np.linspace(0.0, 6.0, B), np.array([2.0, 5.0])
    t0_all, t0_grp = np.linspace(0.0, 1.5, B), np.array([0.0, 0.3])
    runs = {}
    for name, kw in (("speed", dict(speed=sp, v_start=vs_all)),
                     ("all", dict(speed=sp, v_start=vs_all, sample=sa, samples=m, t0=t0_all)),
                     ("select", dict(select=gs, speed=sp, v_start=vs_grp, sample=sa, samples=m)),
                     ("winners", dict(select=gs, winners_only=True, speed=sp, v_start=vs_grp, sample=sa, samples=m, t0=t0_grp))):
        h, hs = chain_util.handles(B)
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                                     check_footprint=True, **kw)
        h.close(); hs.close()
    before, every, sel, win = runs["speed"], runs["all"], runs["select"], runs["winners"]
    assert list(every) == list(before) + ["traj", "traj_n", "traj_flags"]
    for k in before:                                         # sample=None: as before; with it: the same paths and profiles
        assert same_bits(before[k], every[k]) if before[k].dtype == np.float64 else np.array_equal(before[k], every[k]), k
    assert every["traj"].shape == (B, m, 8) and every["traj_n"].shape == (B,) and every["traj_flags"].shape == (B,)
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    want = h.sample_trajectory(every["out"], every["profile"], m, n_of=every["n_out"], stop_before=every["first_collision"], t0=t0_all, prm=sa)
    assert same_bits(every["traj"], want[0]) and np.array_equal(every["traj_n"], want[1]) and np.array_equal(every["traj_flags"], want[2])
    a = dict(paths=every["out"], profile=every["profile"], n_of=every["n_out"], stop_before=every["first_collision"], t0=t0_all)
    _check((every["traj"], every["traj_n"], every["traj_flags"]), a, m, 0.2, 1)
    assert (every["traj_flags"] & S.NOT_FINITE == 0).all() and (every["traj_n"] > 0).any()
    # the winners, with and without the candidates' arrays crossing to the host
    assert sorted(win) == sorted(["n_out", "status", "stage", "iters", "first_collision", "terms", "best", "best_paths", "best_n", "profile",
                                  "speed_flags", "traj", "traj_n", "traj_flags"])
    assert "out" in sel and sel["traj"].shape == (2, m, 8) == win["traj"].shape and (win["best"] >= 0).any()
    for res, t0 in ((sel, None), (win, t0_grp)):
        want = h.sample_trajectory(res["best_paths"], res["profile"], m, n_of=res["best_n"], t0=t0, prm=sa)
        assert same_bits(res["traj"], want[0]) and np.array_equal(res["traj_n"], want[1]) and np.array_equal(res["traj_flags"], want[2])
        for g in range(2):
            assert (res["traj_flags"][g] == S.EMPTY) == (res["best"][g] < 0)
    h.close()
    assert same_bits(sel["best_paths"], win["best_paths"]) and same_bits(sel["profile"], win["profile"])


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_sampler_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("sample_demo")
    rng = np.random.default_rng(2001)
    counts = [30, 1, 64, 65, 0, 130]
    stops = [30, 1, 40, 65, 0, 129]
    t0 = [0.0, 0.0, 0.3, 1.0, 0.0, 2.5]
    n, m, dt = max(counts), 70, 0.15
    paths, prof = np.zeros((len(counts), n, 7)), np.zeros((len(counts), n, 4))
    for b, c in enumerate(counts):
        if c:
            paths[b, :c] = S.seeded_path(rng, c)
            prof[b, :c] = S.seeded_profile(rng, paths[b, :c])
    for hold in (0, 1):
        path = tmp_path / f"paths{hold}.bin"
        S.write_case(path, paths, prof, m, counts, stops, t0, dt, hold)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want = handle.sample_trajectory(paths, prof, m, n_of=counts, stop_before=stops, t0=t0, prm=_cprm(dt, hold))
        lines = iter(r.stdout.strip().splitlines())
        for b, c in enumerate(counts):
            head = next(lines).split()
            rows_want = 0 if c == 0 else (m if hold else int(want[1][b]))
            assert head[0] == "path" and int(head[1]) == b and int(head[2]) == want[2][b] and int(head[3]) == rows_want, (b, head)
            rows = np.array([[float(v) for v in next(lines).split()] for _ in range(rows_want)]).reshape(rows_want, 8)
            assert same_bits(rows, want[0][b, :rows_want]), b
        assert next(lines, None) is None
