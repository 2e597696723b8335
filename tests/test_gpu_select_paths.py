"""pqp_select_paths on the GPU against its float64 numpy restatement (tests/select_util.py): the eight terms of ragged random batches, the
winners and their rows, the edge rules, bit-for-bit reproducibility and independence of a candidate from its batch, an untrusted
group_start on the device form, the host form's refusals, the selection behind the device chain, and the C++ wrapper.  Run with -m gpu
on an MI355X.

Tolerances.  The device adds a candidate's addends in another order than np.sum, and a few addends (the chords' square roots, the
per-waypoint division) carry a rounding of their own: a term may differ from numpy's by 4 count 2^-53 S, S the sum of the absolute values
of its addends (select_util.terms(with_bound=True)).  The least margin (term 5) and eligibility (term 7) are exact.  `best` is exact
against the device's own scores.  Against the restatement's scores a near tie may go either way: with w the device's winner and m the
restatement's, device(w) <= device(m), so restated(w) <= restated(m) + bound(w) + bound(m).

An untrusted group_start: include/pqp.h says the kernel clamps every boundary to [0, batch] and takes a descending pair for an empty group.
So of the groups around a value above `batch`, the one that starts there is empty (-1) and the one that ends there runs to the last row;
the group of a descending pair is empty (-1)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import chain_util
import cpp_demo
import select_util as S
from path_optimizer_2_amd import capi
from shared_util import same_bytes

pytestmark = pytest.mark.gpu
COUNTS = [0, 1, 2, 63, 64, 65, 80, 500, 2000]
FIELDS = ("weight_kappa", "weight_dkappa", "weight_offset", "weight_length", "weight_clearance", "clearance_want", "per_waypoint", "require_free")


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), device=0, max_batch=8, max_n=16)
    yield h
    h.close()


def _cprm(prm):
    return capi.select_default_params(**{k: getattr(prm, k) for k in FIELDS})


def _random_paths(rng, counts, n, stride=7):
    """smooth-ish paths: a random walk in x, y; l, k, dk of the sizes the chain produces; every column beyond the seven is noise"""
    B = len(counts)
    p = rng.normal(size=(B, n, stride))
    p[:, :, 0] = np.cumsum(rng.uniform(0.2, 0.6, (B, n)), axis=1) + rng.uniform(-50, 50, (B, 1))
    p[:, :, 1] = np.cumsum(rng.normal(scale=0.1, size=(B, n)), axis=1) + rng.uniform(-50, 50, (B, 1))
    p[:, :, 3] *= 0.8
    p[:, :, 5] *= 0.1
    p[:, :, 6] *= 0.02
    return p


def _random_case(seed, counts, n, stride=7):
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    B = len(counts)
    first = np.where(rng.random(B) < 0.3, (counts * rng.random(B)).astype(np.int32), counts).astype(np.int32)
    return dict(paths=_random_paths(rng, counts, n, stride), n_of=counts, status=rng.choice([1, 1, 1, 1, 2, 0, 4], B).astype(np.int32),
                stage=rng.choice([0, 0, 0, 0, 3, 7], B).astype(np.int32), first_collision=first, margin=rng.uniform(-0.4, 2.0, (B, n)))


def _random_groups(rng, B, groups):
    cuts = np.sort(rng.integers(0, B + 1, groups - 1))
    return np.concatenate([[0], cuts, [B]]).astype(np.int32)


def _check(got, case, group_start, prm):
    """everything section by section: terms against the restatement, winners against the device's own scores and against the restatement's,
    the winners' rows"""
    opt = {k: case.get(k) for k in ("n_of", "status", "stage", "first_collision", "margin")}
    want, bound = S.terms(case["paths"], prm=prm, with_bound=True, **opt)
    t = got["terms"]
    with np.errstate(all="ignore"):
        for j in (0, 1, 2, 3, 4, 6):
            same = (t[:, j] == want[:, j]) | (np.isnan(t[:, j]) & np.isnan(want[:, j]))          # (inf and NaN: the same on both sides)
            err = np.where(same, 0.0, np.abs(t[:, j] - want[:, j]))
            part = np.where(bound[:, j] > 0, err / bound[:, j], np.where(err > 0, np.inf, 0.0))
            print(f"term {j}: worst error = {err.max():.3e}, worst error / bound = {part.max():.3f}")
            bad = ~(err <= bound[:, j]) & ~same
            assert not bad.any(), (j, np.flatnonzero(bad)[:8], t[bad, j][:8], want[bad, j][:8], bound[bad, j][:8])
    assert np.array_equal(t[:, 5], want[:, 5], equal_nan=True) and np.array_equal(t[:, 7], want[:, 7])
    # the winner by the device's own scores: exact
    best = got["best"]
    assert np.array_equal(best, S.winners(t, group_start)), (best, S.winners(t, group_start))
    # and by the restatement's: the same groups have one, and a different one only on a near tie
    ref = S.winners(want, group_start)
    assert np.array_equal(best >= 0, ref >= 0)
    for g in np.flatnonzero(best >= 0):
        w, m = best[g], ref[g]             # two scores, each within its own bound of the device's: the sum is the tight consequence
        assert want[w, 7] == 1.0 and want[w, 0] <= want[m, 0] + bound[w, 0] + bound[m, 0], (g, w, m)
    bp, bn = S.best_rows(case["paths"], case.get("n_of"), best)
    assert np.array_equal(got["best_n"], bn) and same_bytes(got["best_paths"], bp)
    return want


# ---- terms and winners -----------------------------------------------------------------------------------------------------------------
PRMS = [S.Params(),
        S.Params(weight_kappa=3.5, weight_dkappa=41.0, weight_offset=0.7, weight_length=0.25, weight_clearance=12.0, clearance_want=0.9),
        S.Params(weight_kappa=1.0, weight_dkappa=7.0, weight_offset=2.0, weight_length=1.5, weight_clearance=3.0, per_waypoint=1),
        S.Params(weight_length=1.0, weight_kappa=0.0, weight_dkappa=0.0, per_waypoint=1, require_free=0)]


@pytest.mark.parametrize("stride", [7, 9])
@pytest.mark.parametrize("which", range(len(PRMS)))
def test_terms_and_winners_of_ragged_batches(handle, stride, which):
    prm = PRMS[which]
    rng = np.random.default_rng(100 + which)
    counts = COUNTS + list(rng.integers(2, 2001, 27)) + [80] * 12
    case = _random_case(10 * which + stride, rng.permutation(counts), 2000, stride)
    gs = _random_groups(rng, len(counts), 9)
    got = handle.select_paths(case["paths"], gs, case["n_of"], case["status"], case["stage"], case["first_collision"], case["margin"], prm=_cprm(prm))
    want = _check(got, case, gs, prm)
    assert 0 < want[:, 7].sum() < len(counts) and (got["best"] >= 0).any()


@pytest.mark.parametrize("absent", ["n_of", "status", "stage", "first_collision", "margin", "all"])
def test_every_optional_array_may_be_absent(handle, absent):
    rng = np.random.default_rng(7)
    counts = rng.permutation(COUNTS[:-2] + [150, 150, 97, 3, 2, 150])
    case = _random_case(31, counts, 150)
    if absent == "n_of":
        case["first_collision"] = np.where(case["first_collision"] == case["n_of"], 150, case["first_collision"]).astype(np.int32)
    for k in (["n_of", "status", "stage", "first_collision", "margin"] if absent == "all" else [absent]):
        case[k] = None
    prm = PRMS[1]
    gs = np.array([0, 4, 4, 9, len(counts)], np.int32)
    got = handle.select_paths(case["paths"], gs, case["n_of"], case["status"], case["stage"], case["first_collision"], case["margin"], prm=_cprm(prm))
    _check(got, case, gs, prm)
    if case["margin"] is None:
        assert (got["terms"][:, 5] == 0).all() and (got["terms"][:, 6] == 0).all()


# ---- edge rules ------------------------------------------------------------------------------------------------------------------------
def test_who_can_win(handle):
    rng = np.random.default_rng(3)
    n = 70
    base = _random_paths(rng, [n] * 1, n)[0]
    cheap = base.copy(); cheap[:, 5:7] *= 0.1               # a tenth of the curvature: the cheapest by far
    mid = base.copy(); mid[:, 5:7] *= 0.5
    nan = cheap.copy(); nan[40, 6] = math.nan
    inf = cheap.copy(); inf[69, 1] = math.inf                # the length is not finite: 0 * inf
    # group 0: duplicates tie, the lower index wins.  group 1: the cheapest collides.  group 2: unsolved, stopped, short, NaN, inf; then mid.
    # group 3: empty.  group 4: nobody eligible.
    cands = [base, mid, mid, base,      cheap, mid, base,      cheap, cheap, cheap, nan, inf, mid,      cheap, cheap]
    paths = np.stack(cands)
    B = len(cands)
    n_of = np.full(B, n, np.int32); n_of[9] = 1
    status = np.ones(B, np.int32); status[7] = 2; status[13] = 0
    stage = np.zeros(B, np.int32); stage[8] = 5
    first = n_of.copy(); first[4] = 12; first[14] = 0
    gs = np.array([0, 4, 7, 13, 13, 15], np.int32)
    got = handle.select_paths(paths, gs, n_of, status, stage, first)
    assert got["best"].tolist() == [1, 5, 12, -1, -1]
    assert got["terms"][:, 7].tolist() == [1, 1, 1, 1,  0, 1, 1,  0, 0, 0, 0, 0, 1,  0, 0]
    assert same_bytes(got["terms"][1], got["terms"][2]) and (got["terms"][9] == 0).all()
    assert math.isnan(got["terms"][10, 0]) and not math.isfinite(got["terms"][11, 0])
    assert got["best_n"].tolist() == [n, n, n, 0, 0] and (got["best_paths"][3:] == 0).all()
    assert same_bytes(got["best_paths"][2], mid)
    _check(got, dict(paths=paths, n_of=n_of, status=status, stage=stage, first_collision=first), gs, S.Params())
    # require_free = 0: the colliding candidates may win (14 collides and is solved; 13 is not solved)
    free_or_not = handle.select_paths(paths, gs, n_of, status, stage, first, prm=capi.select_default_params(require_free=0))
    assert free_or_not["best"].tolist() == [1, 4, 12, -1, 14]


def test_one_group_of_65536_and_a_group_per_candidate(handle):
    rng = np.random.default_rng(23)
    B, n = 65536, 12
    counts = rng.integers(0, n + 1, B).astype(np.int32)
    case = dict(paths=_random_paths(rng, counts, n), n_of=counts, status=rng.choice([1, 1, 1, 2], B).astype(np.int32))
    least = 40000 + int(np.argmax(counts[40000:] == n))
    case["paths"][least, :, 5:7] = 0.0                       # score 0, twice: the lower index wins
    case["paths"][least + 9] = case["paths"][least]; counts[least + 9] = n
    case["status"][[least, least + 9]] = 1
    got = handle.select_paths(case["paths"], [0, B], case["n_of"], case["status"])
    assert got["best"].tolist() == [least] and got["terms"][least, 0] == 0.0
    _check(got, case, [0, B], S.Params())
    gs = np.arange(B + 1, dtype=np.int32)
    got = handle.select_paths(case["paths"], gs, case["n_of"], case["status"])
    assert np.array_equal(got["best"], np.where(got["terms"][:, 7] == 1.0, np.arange(B), -1))
    assert np.array_equal(got["best_n"], np.where(got["best"] >= 0, counts, 0))
    bp, _ = S.best_rows(case["paths"], counts, got["best"])
    assert same_bytes(got["best_paths"], bp)


# ---- reproducible, and a candidate's terms are its own ---------------------------------------------------------------------------------
def test_same_bits_every_run_and_in_any_batch(handle):
    rng = np.random.default_rng(41)
    B, n = 8192, 200
    counts = rng.integers(2, n + 1, B).astype(np.int32)
    counts[[5, 4097, 8191]] = [200, 65, 129]
    case = _random_case(43, counts, n)
    gs = np.arange(0, B + 1, 8, dtype=np.int32)
    prm = _cprm(PRMS[2])
    args = (case["paths"], gs, case["n_of"], case["status"], case["stage"], case["first_collision"], case["margin"])
    a, b = handle.select_paths(*args, prm=prm), handle.select_paths(*args, prm=prm)
    for k in a:
        assert same_bytes(a[k], b[k]), k
    for at in (5, 4097, 8191, 77):
        one = handle.select_paths(case["paths"][at:at + 1], [0, 1], *(case[k][at:at + 1] for k in ("n_of", "status", "stage", "first_collision", "margin")),
                                  prm=prm)
        assert same_bytes(one["terms"][0], a["terms"][at]), at
        # and alone in a shorter row: n is no part of the sums
        c = int(counts[at])
        one = handle.select_paths(case["paths"][at:at + 1, :c], [0, 1], *(case[k][at:at + 1] for k in ("n_of", "status", "stage", "first_collision")),
                                  margin=case["margin"][at:at + 1, :c], prm=prm)
        assert same_bytes(one["terms"][0], a["terms"][at]), at


# ---- the device form and a group_start nobody checked ----------------------------------------------------------------------------------
def test_untrusted_group_start_on_the_device_form(handle):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(57)
    alloc, B, n = 96, 64, 40                                 # 32 spare rows behind the batch: nothing reads outside an allocation, clamp or not
    counts = rng.integers(2, n + 1, alloc).astype(np.int32)
    case = _random_case(59, counts, n)
    case["paths"][B:, :, 5:7] = 0.0                          # the spare rows would win every group that reached them
    case["status"][B:] = 1; case["stage"][B:] = 0; case["first_collision"][B:] = counts[B:]
    case["status"][:B:2] = 1; case["stage"][:B:2] = 0       # enough eligible candidates for every group to have one
    gs = np.array([0, 8, 16, 24, 90, 32, 40, 36, 48, 56, 64], np.int32)          # 90 > batch (inside the allocation); 40 > 36 descends
    groups = gs.size - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: up(case[k]) for k in ("paths", "n_of", "status", "stage", "first_collision", "margin")}
    d_gs = up(gs)
    terms = torch.full((alloc, 8), -7.0, dtype=torch.float64, device=dev)
    best = torch.full((groups,), -7, dtype=torch.int32, device=dev)
    best_paths = torch.full((groups, n, 7), -7.0, dtype=torch.float64, device=dev)
    best_n = torch.full((groups,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    prm = capi.select_default_params()
    handle._check(handle.lib.pqp_select_paths_device(handle._h, C.byref(prm), B, n, 7, p(d["paths"]), p(d["n_of"]), p(d["status"]), p(d["stage"]),
                                                     p(d["first_collision"]), p(d["margin"]), groups, p(d_gs), p(terms), p(best), p(best_paths), p(best_n)))
    handle.sync()
    got = dict(terms=terms.cpu().numpy(), best=best.cpu().numpy(), best_paths=best_paths.cpu().numpy(), best_n=best_n.cpu().numpy())
    assert (got["terms"][B:] == -7.0).all()                  # rows beyond the batch: not scored
    inside = {k: (v[:B] if v is not None else None) for k, v in case.items()}
    got["terms"] = got["terms"][:B]
    _check(got, inside, gs, S.Params())                      # select_util.group_bounds: the documented reading of such an array
    t = got["terms"]
    assert (got["best"] < B).all()
    assert got["best"][4] == -1 and got["best"][6] == -1     # starts above the batch; descends
    # 3 ends above the batch: it runs to the last row; 5 and 7, around the descending pair, are what their own boundaries say
    rows = {0: (0, 8), 1: (8, 16), 2: (16, 24), 3: (24, B), 5: (32, 40), 7: (36, 48), 8: (48, 56), 9: (56, 64)}
    for g, (lo, hi) in rows.items():
        assert got["best"][g] == S.winners(t, [lo, hi])[0], g
    assert (got["best"] >= 0).sum() >= 6


# ---- what the host form refuses --------------------------------------------------------------------------------------------------------
def test_host_form_refuses_and_leaves_the_outputs_alone(handle):
    rng = np.random.default_rng(61)
    B, n = 6, 10
    paths = _random_paths(rng, [n] * B, n, stride=7)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(stride=7, groups=2, gs=(0, 3, 6), prm=None, want_paths=True, want_n=True):
        terms, best = np.full((B, 8), -7.0), np.full(max(groups, 1), -7, np.int32)
        bp, bn = np.full((max(groups, 1), n, 7), -7.0), np.full(max(groups, 1), -7, np.int32)
        prm = prm or capi.select_default_params()
        rc = handle.lib.pqp_select_paths(handle._h, C.byref(prm), B, n, stride, p(paths), None, None, None, None, None, groups,
                                         p(np.array(gs, np.int32)), p(terms), p(best), p(bp) if want_paths else None, p(bn) if want_n else None)
        return rc, all((a == -7).all() for a in (terms, best, bp, bn))

    rc, untouched = call()
    assert rc == 0 and not untouched
    bad = [dict(stride=6), dict(groups=-1), dict(gs=(1, 3, 6)), dict(gs=(0, 3, 5)), dict(gs=(0, 3, 7)), dict(gs=(0, 4, 3)),
           dict(groups=3, gs=(0, 4, 2, 6)), dict(want_paths=False), dict(want_n=False)]
    bad += [dict(prm=capi.select_default_params(**{k: v})) for k in FIELDS[:6] for v in (math.nan, math.inf)]
    for kw in bad:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
    assert b"pqp_select_paths" in handle.lib.pqp_last_error()


# ---- behind the device chain -----------------------------------------------------------------------------------------------------------
def _restated(res, gs, prm=None):
    return S.select(res["out"], gs, res["n_out"], res["status"], res["stage"], res.get("first_collision"), res.get("margin"), prm)


@pytest.mark.parametrize("on_grid", [False, True])
def test_select_behind_the_chain(hip_lib, on_grid):
    import distance_util as D
    B = 24 if not on_grid else 16
    sc = chain_util.scenarios(B)
    gs = np.arange(0, B + 1, 8, dtype=np.int32)
    layers = np.stack([D.occupancy_of(d) for d in sc["dist"]]) if on_grid else sc["dist"]
    runs = {}
    for name, kw in (("plain", dict()), ("select", dict(select=gs)), ("winners", dict(select=gs, winners_only=True)),
                     ("no_check", dict(select=gs, check_footprint=False))):
        h, hs = chain_util.handles(B)                            # fresh handles for each: nothing carried from one call to the other
        run = h.optimize_path_on_grid if on_grid else h.optimize_path
        runs[name] = run(sc["pts"], sc["n_pts"], sc["start"], sc["target"], layers, sc["geom"], map_of=sc["map_of"], smoother=hs,
                         **{"check_footprint": True, **kw})
        h.close(); hs.close()
    plain, sel, win, no_check = (runs[k] for k in ("plain", "select", "winners", "no_check"))
    assert list(plain) == ["out", "n_out", "status", "stage", "iters", "free", "first_collision", "margin"]        # select=None: as before
    assert list(sel) == list(plain) + ["terms", "best", "best_paths", "best_n"]
    for k in plain:
        assert same_bytes(plain[k], sel[k]), k
    want = _restated(sel, gs)
    assert np.array_equal(sel["best"], want["best"]) and (sel["best"] >= 0).any()
    assert np.array_equal(sel["best_n"], want["best_n"]) and same_bytes(sel["best_paths"], want["best_paths"])
    _check(sel, dict(paths=sel["out"], n_of=sel["n_out"], status=sel["status"], stage=sel["stage"], first_collision=sel["first_collision"],
                     margin=sel["margin"]), gs, S.Params())
    # winners only: the same answer, and neither the paths nor the per-waypoint arrays
    assert sorted(win) == sorted(["n_out", "status", "stage", "iters", "first_collision", "terms", "best", "best_paths", "best_n"])
    for k in ("best", "best_paths", "best_n", "terms", "n_out", "status", "stage", "first_collision"):
        assert same_bytes(win[k], sel[k]), k
    # without the footprint check the selection reads neither first_collision nor margin
    assert "first_collision" not in no_check and np.array_equal(no_check["best"], _restated(no_check, gs)["best"])
    assert (no_check["terms"][:, 5:7] == 0).all()


def test_selection_arguments_without_select_are_refused(hip_lib):
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    with pytest.raises(ValueError):
        h._selection(None, None, True)
    with pytest.raises(ValueError):
        capi._check_group_start(np.array([0, 5, 4, 8]), 8)
    h.close()


# ---- C++ -------------------------------------------------------------------------------------------------------------------------------
def test_selector_agrees_with_the_python_call(handle, tmp_path):
    exe = cpp_demo.build("select_demo")
    rng = np.random.default_rng(71)
    counts = [30, 1, 12, 64, 65, 0, 5, 5, 90]
    n = max(counts)
    paths = _random_paths(rng, counts, n)
    paths[7] = paths[6]                                      # a tie
    gs = [0, 3, 3, 6, 9]
    path = tmp_path / "candidates.bin"
    S.write_candidates(path, [paths[b, :c] for b, c in enumerate(counts)], gs)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    want = handle.select_paths(paths, gs, np.array(counts, np.int32))
    assert [int(l.split()[1]) for l in lines[:4]] == want["best"].tolist()
    assert [l.split()[0] for l in lines] == ["best"] * 4 + ["score"] * len(counts)
    assert np.array_equal(np.array([float(l.split()[1]) for l in lines[4:]]), want["terms"][:, 0])
    assert want["best"][1] == -1 and want["best"][3] == 6
