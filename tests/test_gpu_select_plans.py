"""pqp_select_plans on the GPU against its float64 numpy restatement (tests/rank_util.py; tests/test_select_plans.py holds it against a
plain loop and checks the hand case on the CPU first): the ten terms of ragged batches, the winners and their rows, every optional array
absent, the eligibility clauses one by one, bit-for-bit reproducibility and independence of a candidate from its batch, its group and the
form, an untrusted group_start on the device form, the host form's refusals, the device's own search-refine-sample-check output, the stage
behind the device chain, and the C++ wrapper.  Run with -m gpu on an MI355X.

Tolerances.  Entries 1, 7, 8 and 9 and the gathered rows are exact, entry 5 too (a NaN is a NaN).  Entries 2, 3, 4 and 6 are sums the
device adds in another order than the restatement: they hold within rank_util's 4 c 2^-53 S, and the score within the bound that follows
from those (rank_util's text derives both).  `best` is exact against the restatement's group rule applied to the device's own terms.
The generated cases have no two eligible scores of a group within twice the sum of their bounds of each other (checked on the
restatement when a case is made), apart from deliberate ties - equal rows - where the lowest row wins; so `best` equals the
restatement's own winners as well.

The shapes are the smallest at which the kernels can go wrong: counts 0, 1, 2, 63, 64, 65, 128, 129 and 200 in one batch (the lane
stride's edges and the i + 1 neighbour at a stride edge), strides 8 and 11, groups of 0, 1, 2, 63, 64, 65 and 130 candidates, n = 9 and
m = 200 (7 n and 8 m are no multiples of 64)."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import cpp_demo
import device_form as D
import plan_util as P
import rank_util as K
import refine_util as R
import search_util as S
import select_util
from path_optimizer_2_amd import capi
from shared_util import same_bits

pytestmark = pytest.mark.gpu
COUNTS = [0, 1, 2, 63, 64, 65, 128, 129, 200]
GROUP_SIZES = [2, 0, 63, 1, 64, 130, 65]
OPTIONAL = ("m_of", "path_terms", "search_flags", "first_hit", "clearance", "paths", "n_of")
FIELDS = ("w_path", "w_progress", "w_accel", "w_jump", "w_lateral", "w_clearance", "clearance_want", "require_free")
PRMS = [K.Params(),
        K.Params(w_path=0.5, w_progress=2.0, w_accel=0.25, w_jump=3.0, w_lateral=1.5, w_clearance=4.0, clearance_want=0.9, require_free=0)]
ERR_INVALID = -1


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _cprm(prm):
    return capi.rank_default_params(**{k: getattr(prm, k) for k in FIELDS})


def _random_case(seed, counts, m, stride=8, n=9, path_stride=7):
    """trajectories of a car's size: k about 0.1 / m, v up to 6 m/s, a in -3 .. 1.5 m/s^2, uneven time steps from a start time of its own;
    every column beyond the eight, and the columns nobody reads, are noise"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    B = len(counts)
    traj = rng.normal(size=(B, m, stride))
    traj[:, :, 3] *= 0.1
    traj[:, :, 4] = np.cumsum(rng.uniform(0.0, 1.0, (B, m)), axis=1) + rng.uniform(-20, 20, (B, 1))
    traj[:, :, 5] = rng.uniform(0.0, 6.0, (B, m))
    traj[:, :, 6] = rng.uniform(-3.0, 1.5, (B, m))
    traj[:, :, 7] = np.cumsum(rng.uniform(0.05, 0.15, (B, m)), axis=1) + rng.uniform(-5, 5, (B, 1))
    path_terms = rng.uniform(0.0, 50.0, (B, 8))
    path_terms[:, 7] = rng.choice([1.0, 1.0, 1.0, 0.0], B)
    clearance = rng.uniform(-0.4, 2.0, (B, m))
    clearance[rng.random(B) < 0.1] = np.inf                  # no agent near
    first = np.where(rng.random(B) < 0.25, (counts * rng.random(B)).astype(np.int32), counts).astype(np.int32)
    return dict(traj=traj, m_of=counts, path_terms=path_terms, search_flags=rng.choice([0, 0, 0, 0, 8, 4, 2, 12, 1, 16, 32], B).astype(np.int32),
                first_hit=first, clearance=clearance, paths=rng.normal(size=(B, n, path_stride)), n_of=rng.integers(0, n + 1, B).astype(np.int32))


def _tie(case, at, like):
    """row `at` becomes row `like` in every array: a deliberate exact tie"""
    for k in ("traj",) + OPTIONAL:
        if case.get(k) is not None:
            case[k][at] = case[k][like]


def _restated(case, prm):
    return K.terms(case["traj"], case.get("m_of"), case.get("path_terms"), case.get("search_flags"), case.get("first_hit"), case.get("clearance"), prm,
                   with_bound=True)


def _no_near_ties(case, gs, prm):
    """what the module's text promises of a generated case: within a group two eligible scores are those of equal rows, or further apart
    than twice the sum of their bounds"""
    want, bound = _restated(case, prm)
    for lo, hi in select_util.group_bounds(gs, len(want)):
        idx = [b for b in range(lo, hi) if want[b, 9] == 1.0]
        for i, a in enumerate(idx):
            for b in idx[i + 1:]:
                if not same_bits(want[a], want[b]):
                    assert abs(want[a, 0] - want[b, 0]) > 2.0 * (bound[a, 0] + bound[b, 0]), (a, b, want[a, 0], want[b, 0])


def _host(handle, case, gs, prm):
    return handle.select_plans(case["traj"], gs, **{k: case.get(k) for k in OPTIONAL}, prm=_cprm(prm))


def _device(handle, case, gs, prm, batch=None, groups=None, want_traj=True, want_paths=True):
    """the device form through device_form: the outputs lie in sentinel-filled allocations with a guard band behind them.  batch: the rows
    to rank when the arrays hold more"""
    traj = np.ascontiguousarray(case["traj"], dtype=np.float64)
    rows, m, stride = traj.shape
    B = rows if batch is None else batch
    paths = case.get("paths")
    n, path_stride = (0, 0) if paths is None else paths.shape[1:]
    G = len(gs) - 1 if groups is None else groups
    f64 = lambda k: None if case.get(k) is None else D.to_device(case[k])
    i32 = lambda k: None if case.get(k) is None else D.to_device(case[k], np.int32)
    out = dict(terms=D.Out((rows, 10)), best=D.Out((len(gs) - 1,), np.int32))
    out.update(best_traj=D.Out((len(gs) - 1, m, 8)), best_m=D.Out((len(gs) - 1,), np.int32)) if want_traj else out.update(best_traj=None, best_m=None)
    if want_paths and paths is not None:
        out.update(best_paths=D.Out((len(gs) - 1, n, 7)), best_n=D.Out((len(gs) - 1,), np.int32))
    else:
        out.update(best_paths=None, best_n=None)
    rc = D.call(handle, "pqp_select_plans_device", prm.array(), int(prm.require_free), B, m, stride, D.to_device(traj), i32("m_of"), f64("path_terms"),
                i32("search_flags"), i32("first_hit"), f64("clearance"), n, path_stride, f64("paths"), i32("n_of"), G, D.to_device(gs, np.int32),
                *out.values())
    return rc, out


def _check(got, case, gs, prm, where=""):
    """everything section by section: terms against the restatement, winners against the device's own scores and against the restatement's,
    the winners' rows"""
    want, bound = _restated(case, prm)
    t = got["terms"]
    for j in (1, 7, 8, 9):
        assert same_bits(t[:, j], want[:, j]), (where, j)
    assert np.array_equal(t[:, 5], want[:, 5], equal_nan=True), where
    with np.errstate(all="ignore"):
        for j in (2, 3, 4, 6, 0):
            same = (t[:, j] == want[:, j]) | (np.isnan(t[:, j]) & np.isnan(want[:, j]))          # (inf and NaN: the same on both sides)
            err = np.where(same, 0.0, np.abs(t[:, j] - want[:, j]))
            part = np.where(bound[:, j] > 0, err / bound[:, j], np.where(err > 0, np.inf, 0.0))
            print(f"{where} term {j}: worst error = {err.max():.3e}, worst error / bound = {part.max():.3f}")
            bad = ~(err <= bound[:, j]) & ~same
            assert not bad.any(), (where, j, np.flatnonzero(bad)[:8], t[bad, j][:8], want[bad, j][:8], bound[bad, j][:8])
    best = got["best"]
    assert np.array_equal(best, K.winners(t, gs)), (where, best, K.winners(t, gs))           # by the device's own terms: exact
    assert np.array_equal(best, K.winners(want, gs)), (where, best, K.winners(want, gs))     # no near ties in a generated case
    if "best_traj" in got:
        bt, bm = K.best_rows(case["traj"], case.get("m_of"), best)
        assert np.array_equal(got["best_m"], bm) and same_bits(got["best_traj"], bt), where
    if "best_paths" in got:
        bp, bn = select_util.best_rows(case["paths"], case.get("n_of"), best)
        assert np.array_equal(got["best_n"], bn) and same_bits(got["best_paths"], bp), where
    return want


def _ragged(seed, stride):
    rng = np.random.default_rng(seed)
    B = sum(GROUP_SIZES)
    counts = rng.permutation((COUNTS * 4 + list(rng.integers(2, 201, B)))[:B])
    gs = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int32)
    case = _random_case(seed + 1, counts, 200, stride, n=9, path_stride=7 if stride == 8 else 10)
    for at, like in ((1, 0), (70, 66), (325 - 60, 325 - 65)):
        _tie(case, at, like)
    return case, gs


# ---- terms and winners -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [8, 11])
@pytest.mark.parametrize("which", range(len(PRMS)))
def test_terms_and_winners_of_ragged_batches(handle, stride, which):
    prm = PRMS[which]
    case, gs = _ragged(100 * which + stride, stride)
    assert set(COUNTS) <= set(case["m_of"].tolist()) and np.diff(gs).tolist() == GROUP_SIZES
    _no_near_ties(case, gs, prm)
    got = _host(handle, case, gs, prm)
    want = _check(got, case, gs, prm, (stride, which))
    assert 0 < want[:, 9].sum() < len(want) and (got["best"] >= 0).sum() >= 4 and got["best"][1] == -1


@pytest.mark.parametrize("absent", ["m_of", "path_terms", "search_flags", "first_hit", "clearance", "paths", "all"])
def test_every_optional_array_may_be_absent(handle, absent):
    rng = np.random.default_rng(7)
    counts = rng.permutation(COUNTS[:-3] + [130, 130, 97, 3, 2, 130])
    case = _random_case(31, counts, 130)
    if absent in ("m_of", "all"):
        case["first_hit"] = np.where(case["first_hit"] == case["m_of"], 130, case["first_hit"]).astype(np.int32)
    for k in (OPTIONAL if absent == "all" else ("paths", "n_of") if absent == "paths" else (absent,)):
        case[k] = None
    prm = PRMS[1] if absent != "first_hit" else K.Params(w_clearance=1.0)
    gs = np.array([0, 4, 4, 9, len(counts)], np.int32)
    _no_near_ties(case, gs, prm)
    got = _host(handle, case, gs, prm)
    _check(got, case, gs, prm, absent)
    assert ("best_paths" in got) == (case["paths"] is not None)
    if case["clearance"] is None:
        assert (got["terms"][:, 5] == 0).all() and (got["terms"][:, 6] == 0).all()
    if case["path_terms"] is None:
        assert (got["terms"][:, 7] == 0).all()
    if absent != "all":
        return
    # the device form alone: groups = 0 only scores, and best_paths may be asked for without best_traj
    case = _random_case(33, counts, 130)
    rc, out = _device(handle, case, gs, prm, groups=0)
    assert rc == 0, handle.lib.pqp_last_error()
    assert same_bits(out["terms"].get(), _host(handle, case, gs, prm)["terms"])
    assert all(out[k].untouched() for k in ("best", "best_traj", "best_m", "best_paths", "best_n"))
    rc, out = _device(handle, case, gs, prm, want_traj=False)
    assert rc == 0, handle.lib.pqp_last_error()
    _check({k: v.get() for k, v in out.items() if v is not None}, case, gs, prm, "paths without traj")


# ---- edge rules ------------------------------------------------------------------------------------------------------------------------
def test_who_can_win(handle):
    """every eligibility clause on its own: each group holds the cheapest candidate by far - barred by one clause - and an ordinary one"""
    m = 70
    base = _random_case(5, [m], m)["traj"][0]
    cheap = base.copy(); cheap[:, 4] *= 40.0                 # forty times the progress: the least score by far
    nan = cheap.copy(); nan[40, 6] = np.nan
    # groups of two: NO_PLAN, EMPTY, NOT_FINITE, hit, path not eligible, a NaN in a, a clearance of -inf, no rows, nobody eligible, a tie
    cands = [cheap, base] * 5 + [nan, base] + [cheap, base] * 2 + [cheap, nan] + [base, base]
    traj = np.stack(cands)
    B = len(cands)
    gs = np.arange(0, B + 1, 2).astype(np.int32)
    m_of = np.full(B, m, np.int32); m_of[14] = 0
    flags = np.zeros(B, np.int32); flags[0], flags[2], flags[4] = K.NO_PLAN | 4, K.EMPTY, K.NOT_FINITE | 2
    flags[1] = 2 | 4 | 8                                     # START_BLOCKED, GRID_SHORT, ARRIVED bar nobody
    first = m_of.copy(); first[6] = 12; first[16] = 0
    pt = np.ones((B, 8)); pt[:, 0] = 0.25; pt[8, 7] = 0.0
    clear = np.full((B, m), 1.0); clear[12, 5] = -np.inf
    case = dict(traj=traj, m_of=m_of, path_terms=pt, search_flags=flags, first_hit=first, clearance=clear)
    got = _host(handle, case, gs, K.Params())
    _check(got, case, gs, K.Params(), "who can win")
    assert got["best"].tolist() == [1, 3, 5, 7, 9, 11, 13, 15, -1, 18]
    assert got["terms"][:, 9].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1]
    assert np.isnan(got["terms"][10, 0]) and got["terms"][12, 5] == -np.inf and got["terms"][12, 6] == np.inf and (got["terms"][14] == 0).all()
    assert same_bits(got["terms"][18], got["terms"][19])
    assert got["best_m"].tolist() == [m] * 8 + [0, m] and (got["best_traj"][8] == 0).all() and same_bits(got["best_traj"][3], base)
    # require_free = 0: the hit candidates may win (6 and 16; 17 holds a NaN)
    free_or_not = _host(handle, case, gs, K.Params(require_free=0))
    assert free_or_not["best"].tolist() == [1, 3, 5, 6, 9, 11, 13, 15, 16, 18]
    # a clearance of -inf with a weight on the shortfall: the score is +inf, not finite either
    assert _host(handle, case, gs, K.Params(w_clearance=1.0))["terms"][12, 0] == np.inf


# ---- reproducible, and a candidate's terms are its own ---------------------------------------------------------------------------------
def test_same_bits_every_run_at_any_position_and_from_either_form(handle):
    rng = np.random.default_rng(41)
    B, m = 200, 130
    counts = rng.integers(1, m + 1, B).astype(np.int32)
    counts[[5, 97, 199]] = [130, 65, 129]
    case = _random_case(43, counts, m, stride=9)
    gs = np.arange(0, B + 1, 8, dtype=np.int32)
    prm = PRMS[1]
    a, b = _host(handle, case, gs, prm), _host(handle, case, gs, prm)
    rc, out = _device(handle, case, gs, prm)
    assert rc == 0, handle.lib.pqp_last_error()
    dev = {k: v.get() for k, v in out.items()}
    for k in a:
        assert same_bits(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)), k
        assert same_bits(np.asarray(a[k], np.float64), np.asarray(dev[k], np.float64)), k
    # the batch back to front in groups of five: every candidate at another position, in another group
    back = {k: np.ascontiguousarray(v[::-1]) for k, v in case.items()}
    turned = _host(handle, back, np.arange(0, B + 1, 5, dtype=np.int32), prm)
    assert same_bits(turned["terms"][::-1], a["terms"])
    for at in (5, 97, 199, 77):
        c = int(counts[at])                                  # and alone in a shorter row: m is no part of the sums
        one = dict(case, traj=case["traj"][at:at + 1, :c], clearance=case["clearance"][at:at + 1, :c],
                   **{k: case[k][at:at + 1] for k in ("m_of", "path_terms", "search_flags", "first_hit", "paths", "n_of")})
        assert same_bits(_host(handle, one, [0, 1], prm)["terms"][0], a["terms"][at]), at


# ---- the device form and a group_start nobody checked ----------------------------------------------------------------------------------
def test_untrusted_group_start_on_the_device_form(handle):
    """include/pqp.h: the kernel clamps every boundary to [0, batch] and takes a descending pair for an empty group.  So of the groups
    around a value above `batch`, the one that starts there is empty and the one that ends there runs to the last row; a negative
    boundary counts as 0; the group of a descending pair is empty.  32 spare rows lie behind the batch, inside the allocation, and would
    win every group that reached them: nothing is read outside an array either way"""
    alloc, B, m = 96, 64, 40
    counts = np.random.default_rng(57).integers(2, m + 1, alloc).astype(np.int32)
    case = _random_case(59, counts, m)
    case["traj"][B:, :, 4] *= 100.0                          # the spare rows' progress
    case["search_flags"][:] = 0; case["path_terms"][:, 7] = 1.0; case["first_hit"][:] = counts
    case["first_hit"][1:B:2] = 0                             # every other candidate of the batch is hit
    gs = np.array([-5, 8, 16, 24, 90, 32, 40, 36, 48, 56, 64], np.int32)          # -5 < 0; 90 > batch (inside the allocation); 40 > 36 descends
    prm = K.Params()
    rc, out = _device(handle, case, gs, prm, batch=B)
    assert rc == 0, handle.lib.pqp_last_error()
    got = {k: v.get() for k, v in out.items()}
    assert (got["terms"][B:] == D.SENT).all()                # rows beyond the batch: not scored
    inside = {k: v[:B] for k, v in case.items()}
    got["terms"] = got["terms"][:B]
    _check(got, inside, gs, prm, "untrusted")                # select_util.group_bounds: the documented reading of such an array
    t = got["terms"]
    assert (got["best"] < B).all() and got["best"][4] == -1 and got["best"][6] == -1          # starts above the batch; descends
    rows = {0: (0, 8), 1: (8, 16), 2: (16, 24), 3: (24, B), 5: (32, 40), 7: (36, 48), 8: (48, 56), 9: (56, 64)}
    for g, (lo, hi) in rows.items():
        assert got["best"][g] == K.winners(t, [lo, hi])[0] >= 0, g
    assert (got["best_m"][[4, 6]] == 0).all() and (got["best_traj"][[4, 6]] == 0).all() and (got["best_paths"][[4, 6]] == 0).all()


# ---- what the host form refuses --------------------------------------------------------------------------------------------------------
def test_host_form_refuses_and_leaves_the_outputs_alone(handle):
    B, m, n = 6, 10, 4
    case = _random_case(61, [m] * B, m, n=n)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(stride=8, path_stride=7, groups=2, gs=(0, 3, 6), prm=None, require_free=1, want=("terms", "best", "best_traj", "best_m", "best_paths", "best_n"),
             paths=True, m_=m, n_=n, batch=B):
        G = max(groups, 1)
        out = dict(terms=np.full((B, 10), -7.0), best=np.full(G, -7, np.int32), best_traj=np.full((G, m, 8), -7.0), best_m=np.full(G, -7, np.int32),
                   best_paths=np.full((G, n, 7), -7.0), best_n=np.full(G, -7, np.int32))
        prm = K.Params().array() if prm is None else prm
        rc = handle.lib.pqp_select_plans(handle._h, prm, require_free, batch, m_, stride, p(case["traj"]), None, None, None, None, None, n_, path_stride,
                                         p(case["paths"]) if paths else None, None, groups, p(np.array(gs, np.int32)),
                                         *(p(out[k]) if k in want else None for k in out))
        return rc, all((a == -7).all() for a in out.values())

    rc, untouched = call()
    assert rc == 0 and not untouched
    every = ("terms", "best", "best_traj", "best_m", "best_paths", "best_n")
    bad = [dict(stride=7), dict(path_stride=6), dict(groups=-1), dict(groups=0), dict(gs=(1, 3, 6)), dict(gs=(0, 3, 5)), dict(gs=(0, 3, 7)), dict(gs=(0, 4, 3)),
           dict(groups=3, gs=(0, 4, 2, 6)), dict(batch=0), dict(m_=0), dict(n_=0), dict(require_free=2), dict(paths=False)]
    bad += [dict(want=tuple(k for k in every if k != gone)) for gone in every]
    for i in range(K.RANK_PARAMS):
        for v in (np.nan, np.inf):
            w = K.Params().array(); w[i] = v
            bad.append(dict(prm=w))
    for kw in bad:
        rc, untouched = call(**kw)
        assert rc == ERR_INVALID and untouched, kw
        assert handle.lib.pqp_last_error().decode().startswith("pqp_select_plans:"), kw
    with pytest.raises(ValueError):
        handle.select_plans(case["traj"], [0, 4, 3, B])


# ---- the device's own plans ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finished(name, r=10):
    """a case through pqp_speed_search, pqp_speed_refine, pqp_sample_plan at r sub-steps and pqp_agents_check with clearance on the device,
    every layer's agents held for its sub-steps, and pqp_select_paths for the paths' terms: the arrays pqp_select_plans reads"""
    c = K.hand_case() if name == "hand" else R.seeded(name)
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    car = capi.car_default_geometry(**S.HAND_CAR) if name == "hand" or name in R.HAND else None
    grid = capi.search_default_params(**c["prm"])
    opt = dict(n_of=c.get("n_of"), stop_before=c.get("stop_before"))
    se = h.speed_search(c["paths"], c["profile"], c["v_start"], c["agents"], m=c.get("m"), a_of=c.get("a_of"), scene_of=c.get("scene_of"), car=car,
                        prm=grid, blocked=True, **opt)
    rf = h.speed_refine(c["paths"], c["profile"], c["v_start"], se["blocked"], se["steps"], se["reached"], se["traj"], grid=grid, **opt)
    fine = h.sample_plan(c["paths"], c["profile"], rf["traj"], r, dt=c["prm"]["dt"], count_of=se["reached"], refine_flags=rf["flags"], **opt)
    M = fine["traj"].shape[1]
    fine_agents = np.ascontiguousarray(c["agents"][:, :, np.arange(M) // r])
    chk = h.agents_check(fine["traj"], fine_agents, m_of=fine["m_of"], a_of=c.get("a_of"), scene_of=c.get("scene_of"), car=car, clearance=True)
    B = len(c["paths"])
    gs = c.get("group_start", np.array([0, B // 2, B], np.int32))
    sel = h.select_paths(c["paths"], gs, n_of=c.get("n_of"))
    h.close()
    case = dict(traj=fine["traj"], m_of=fine["m_of"], path_terms=sel["terms"], search_flags=se["flags"], first_hit=chk["first_hit"],
                clearance=chk["clearance"], paths=c["paths"], n_of=c.get("n_of"))
    return case, gs, dict(search=se, refine=rf, select=sel, coarse=rf["traj"])


@pytest.mark.parametrize("name", ("rest", "wait", "m12", "tiles", "long"))
def test_the_devices_own_plans_against_the_restatement(handle, name):
    case, gs, made = _finished(name)
    for prm in (K.Params(), K.Params(w_clearance=2.0, require_free=0)):
        got = _host(handle, case, gs, prm)
        want = _check(got, case, gs, prm, name)
    print(f"{name}: refine flags {made['refine']['flags'].tolist()} first hit {case['first_hit'].tolist()} m_of {case['m_of'].tolist()} "
          f"scores {got['terms'][:, 0].tolist()} eligible {got['terms'][:, 9].tolist()} best {got['best'].tolist()}")
    # the jumps of a refined path: its m rows give what its fine rows give, within the two sums' bounds (the restatement: bit for bit)
    coarse = _host(handle, dict(traj=made["coarse"], m_of=made["search"]["reached"]), gs, K.Params())
    _, bound = _restated(case, K.Params())
    for b in np.flatnonzero(made["refine"]["flags"] == R.REFINED):
        assert abs(coarse["terms"][b, 3] - got["terms"][b, 3]) <= 2.0 * bound[b, 3], (name, b)
        assert same_bits(coarse["terms"][b, 1], got["terms"][b, 1])


def test_the_curvier_path_that_passes_wins_on_the_device(handle):
    """rank_util.hand_case() through the device's own stages: pqp_select_paths picks A, the straight road; pqp_select_plans picks B, the
    arc that passes the disc A waits for; without the progress term it picks A again"""
    case, gs, made = _finished("hand")
    assert made["select"]["best"].tolist() == [0]
    assert made["search"]["reached"].tolist() == [S.HAND_M] * 2 and case["first_hit"].tolist() == case["m_of"].tolist() == [71, 71]
    got = _host(handle, case, gs, K.Params())
    _check(got, case, gs, K.Params(), "hand")
    a, b = got["terms"][0, 0], got["terms"][1, 0]
    print(f"A: score {a!r}, terms {got['terms'][0].tolist()}\nB: score {b!r}, terms {got['terms'][1].tolist()}; refine flags {made['refine']['flags'].tolist()}")
    assert got["best"].tolist() == [1] and b < a and got["terms"][1, 1] > got["terms"][0, 1]
    assert same_bits(got["best_traj"][0], case["traj"][1]) and same_bits(got["best_paths"][0], case["paths"][1])
    assert _host(handle, case, gs, K.Params(w_progress=0.0))["best"].tolist() == [0]


# ---- through the layers ----------------------------------------------------------------------------------------------------------------------
def test_rank_behind_the_chain(hip_lib):
    """optimize_path(..., search=, refine=, plan_samples=4, plan_agents=, rank=group_start): what it adds equals the same steps called one by
    one through the public entry points on the arrays it returns; winners_only returns the same winners without the per-candidate arrays;
    the same call without rank= returns its other keys, bit for bit"""
    import chain_util
    B, m, r = 16, 8, 4
    M = P.fine_count(m, r)
    sc = chain_util.scenarios(B)
    gs = np.array([0, 5, 5, 16], np.int32)
    sp = capi.speed_default_params(v_max=8.0)
    se = capi.search_params_from_speed(hip_lib, sp, 1.0, 0.5)
    se.stations, se.w_accel, se.margin = 96, 1.0, 0.2
    rf = capi.refine_default_params(hip_lib, w_jerk=0.5, window=6)
    agents = np.zeros((2, 1, m, 6))
    for s in range(2):                                       # crosses candidate 8 s's line near its middle during layers 2 .. 4
        st, tg = sc["start"][8 * s], sc["target"][8 * s]
        agents[s, 0, :] = [0.5 * (st[0] + tg[0]), 0.5 * (st[1] + tg[1]), st[2] + 1.5, 2.2, 0.9, 0.1]
        agents[s, 0, [0, 1, 5, 6, 7], 3] = -1.0
    fine_agents = np.ascontiguousarray(agents[:, :, np.arange(M) // r])
    scene = (np.arange(B) // 8).astype(np.int32)
    ap = capi.agents_default_params(hip_lib, margin=0.3)
    rk = capi.rank_default_params(hip_lib, w_clearance=0.5)
    kw = dict(check_footprint=True, speed=sp, agents=agents, agents_params=ap, search=se, v_start=np.linspace(0.0, 3.0, B), scene_of=scene, refine=rf,
              plan_samples=r, plan_agents=fine_agents)
    runs = {}
    for name, new in (("rank", dict(rank=gs, rank_params=rk)), ("winners", dict(rank=gs, rank_params=rk, winners_only=True)), ("plain", {})):
        h, hs = chain_util.handles(B)
        runs[name] = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs, **kw, **new)
        h.close(); hs.close()
    res, win, plain = runs["rank"], runs["winners"], runs["plain"]
    before = ["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin", "profile", "speed_flags", "search_steps", "search_traj",
              "search_cost", "search_reached", "search_flags", "search_blocked", "refine_traj", "refine_bounds", "refine_cost", "refine_excess",
              "refine_status", "refine_flags", "plan_traj", "plan_m_of", "plan_defect", "plan_excess", "plan_flags", "plan_first_hit", "plan_hit_agent"]
    added = ["plan_clearance", "terms", "rank_terms", "rank_best", "best_paths", "best_n", "best_traj", "best_m"]
    assert list(plain) == before and list(res) == before + added
    for k in plain:
        assert same_bits(np.asarray(res[k], dtype=np.float64), np.asarray(plain[k], dtype=np.float64)), k
    # the same steps one by one
    h2 = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    chk = h2.agents_check(res["plan_traj"], fine_agents, m_of=res["plan_m_of"], scene_of=scene, prm=ap, clearance=True)
    assert same_bits(res["plan_first_hit"], chk["first_hit"]) and same_bits(res["plan_clearance"], chk["clearance"])
    sel = h2.select_paths(res["out"], gs, res["n_out"], res["status"], res["stage"], res["first_collision"], res["margin"])
    assert same_bits(res["terms"], sel["terms"])
    one = h2.select_plans(res["plan_traj"], gs, m_of=res["plan_m_of"], path_terms=sel["terms"], search_flags=res["search_flags"],
                          first_hit=chk["first_hit"], clearance=chk["clearance"], paths=res["out"], n_of=res["n_out"], prm=rk)
    h2.close()
    for k, mine in (("rank_terms", "terms"), ("rank_best", "best"), ("best_paths", "best_paths"), ("best_n", "best_n"), ("best_traj", "best_traj"),
                    ("best_m", "best_m")):
        assert same_bits(np.asarray(res[k], dtype=np.float64), np.asarray(one[mine], dtype=np.float64)), k
    case = dict(traj=res["plan_traj"], m_of=res["plan_m_of"], path_terms=res["terms"], search_flags=res["search_flags"], first_hit=res["plan_first_hit"],
                clearance=res["plan_clearance"], paths=res["out"], n_of=res["n_out"])
    prm = K.Params(w_clearance=0.5)
    want, _ = _restated(case, prm)
    assert np.array_equal(res["rank_best"], K.winners(res["rank_terms"], gs)) and np.array_equal(res["rank_terms"][:, 9], want[:, 9])
    print(f"rank_best {res['rank_best'].tolist()} eligible {res['rank_terms'][:, 9].tolist()} scores {res['rank_terms'][:, 0].tolist()}")
    assert res["rank_best"][1] == -1 and res["rank_terms"].shape == (B, 10) and res["best_traj"].shape == (3, M, 8)
    for g, w in enumerate(res["rank_best"]):
        if w >= 0:
            assert same_bits(res["best_paths"][g], res["out"][w]) and same_bits(res["best_traj"][g], res["plan_traj"][w])
            assert res["best_n"][g] == res["n_out"][w] and res["best_m"][g] == res["plan_m_of"][w]
    # winners only: the same winners, and none of the per-candidate arrays
    gone = ("out", "free", "margin", "profile", "search_traj", "refine_traj", "plan_traj", "plan_clearance")
    assert list(win) == [k for k in list(res) if k not in gone]
    for k in win:
        assert same_bits(np.asarray(win[k], dtype=np.float64), np.asarray(res[k], dtype=np.float64)), k
    # and on the plan's m rows, without the fine step: the refine's traj with the search's reached
    h, hs = chain_util.handles(B)
    coarse = h.optimize_path(sc["pts"], sc["n_pts"], sc["start"], sc["target"], sc["dist"], sc["geom"], map_of=sc["map_of"], smoother=hs,
                             **{k: v for k, v in kw.items() if not k.startswith("plan_")}, rank=gs)
    h.close(); hs.close()
    assert "plan_clearance" not in coarse and coarse["best_traj"].shape == (3, m, 8)
    case = dict(traj=coarse["refine_traj"], m_of=coarse["search_reached"], path_terms=coarse["terms"], search_flags=coarse["search_flags"])
    want, _ = _restated(case, K.Params())
    assert np.array_equal(coarse["rank_best"], K.winners(coarse["rank_terms"], gs)) and np.array_equal(coarse["rank_terms"][:, [1, 7, 8, 9]], want[:, [1, 7, 8, 9]])


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------------
def test_plan_selector_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("rank_demo")
    counts = np.array([30, 1, 12, 64, 65, 0, 5, 5, 90], np.int32)
    m, dt = 90, 0.1
    case = _random_case(71, counts, m)
    case["traj"][:, :, 7] = np.arange(m).astype(np.float64) * np.float64(dt)        # state f at f dt, as the selector takes it
    _tie(case, 7, 6)
    gs = [0, 3, 3, 6, 9]
    score = case["path_terms"][:, 0]
    path = tmp_path / "case.bin"
    K.write_case(path, case["traj"], dt, counts, gs, score)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    pt = np.zeros((len(counts), 8)); pt[:, 0], pt[:, 7] = score, 1.0
    want = handle.select_plans(case["traj"], gs, m_of=counts, path_terms=pt)
    assert [l.split()[0] for l in lines] == ["best"] * 4 + ["terms"] * len(counts)
    assert [int(l.split()[1]) for l in lines[:4]] == want["best"].tolist() and [int(l.split()[2]) for l in lines[:4]] == want["best_m"].tolist()
    assert same_bits(np.array([[float(v) for v in l.split()[1:]] for l in lines[4:]]), want["terms"])
    assert want["best"][1] == -1 and want["best"][3] == 6
