"""pqp_speed_search on the GPU where tests/test_gpu_speed_search.py does not take it: plans that die late at full-table size, more layers
than a wavefront or a workgroup has lanes, other steps of time and arc length, other weights, q_up > q_down, a wider path stride,
q_max = 0 on up to 64 station tiles - and, for every case old and new, the whole table of parents behind the winning plan.

The cases are search_util.family()'s (tests/test_speed_search.py asserts on the restatement what each is there for and holds every one to
the margins of the seeded shapes: |clear - margin| >= 1e-6 m, a cost gap a tie or >= 1e-9).  Every family goes through both forms:
blocked, steps, reached and flags equal the numpy restatement's, cost and traj bit for bit, frames under test_gpu_agents_check.py's bounds.

The table.  include/pqp.h leaves the contents of `parents` unspecified to callers.  This file pins the kernels' present layout, as the
header comment of csrc/pqp_search_kernels.inc states it, and changes together with that layout; it promises callers nothing.  Layer 0 holds
qenv_j in bytes [0, J) and, where q_max >= 1, qref_j in bytes [S, S + J).  In layers k >= 1 the byte at [k][j][q] of a state that lives in
the restatement is the restatement's parent - every living state's, not the winning plan's alone: a wrong cost in a state beside the plan,
or one that a cost layer kept from two layers back, shows as a wrong or a surplus parent - and every other byte is 255 (visited, dead) or
the allocation's fill (not visited).  Nothing is asserted about the table of an empty or non-finite path."""
import functools

import numpy as np
import pytest

import agents_util as A
import refine_util as R
import search_util as S
import test_gpu_speed_search as G
from path_optimizer_2_amd import capi
from shared_util import same_bits
from test_gpu_speed_search import handle                     # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu
DEAD, FILL = 255, G.TABLE_SENTINEL


@functools.lru_cache(maxsize=None)
def _family(name):
    """computed once per family and shared; nobody writes to it"""
    c = S.family(name)
    return c, S.run_case(c, G.circles())


def _table_equals(table, c, want, where):
    """the device form's `parents` [B][m][S][Q + 1] against the restatement's table, path by path"""
    B, m, Sn, Q1 = table.shape
    assert (Sn, Q1) == (c["prm"]["stations"], c["prm"]["q_max"] + 1) and B == len(want["each"])
    for b, one in enumerate(want["each"]):
        if one["flags"] & (S.EMPTY | S.NOT_FINITE):
            continue
        J, reached = one["J"], one["reached"]
        first = table[b, 0].ravel()
        assert np.array_equal(first[:J], one["qenv"]), (where, b, "qenv")
        if Q1 > 1:
            assert np.array_equal(first[Sn:Sn + J], one["qref"]), (where, b, "qref")
        for k in range(1, m):
            lives = one["parents"][k] if k < reached else {}
            expect = np.full((Sn, Q1), DEAD, np.uint8)
            for (j, q), parent in lives.items():
                expect[j, q] = parent
            got = table[b, k]
            alive = expect != DEAD
            assert np.array_equal(got[alive], expect[alive]), (where, b, k, "a living state's parent", np.argwhere(alive & (got != expect))[:4].tolist())
            rest = got[~alive]
            assert ((rest == DEAD) | (rest == FILL)).all(), (where, b, k, "a parent where no state lives", np.argwhere(~alive & (got != DEAD) & (got != FILL))[:4].tolist())
        assert len(one["parents"]) == max(reached, 1)


def _both_forms(handle, c, want, where, car=None, frames=True):
    """host and device form against the restatement, then the device form's table; returns the host form's outputs"""
    got = G._host(handle, c, car=car)
    G._same(got, want, where)
    table = []
    rc, dev, fr = G._device(handle, c, car=car, table=table)
    assert rc == 0, handle.lib.pqp_last_error()
    G._same(dev, want, where)
    if frames and fr is not None:
        ref = A.frames(c["agents"])
        fin = np.isfinite(np.asarray(c["agents"])[..., 2])                      # (a row whose heading is no number has no frame to compare: its reach is nan)
        assert np.isnan(fr[~fin][:, 7]).all() and np.isnan(ref[~fin][:, 7]).all()
        assert same_bits(fr[fin][:, [0, 1, 4, 5, 6, 7]], ref[fin][:, [0, 1, 4, 5, 6, 7]]) and float(np.abs(fr[fin][:, 2:4] - ref[fin][:, 2:4]).max(initial=0.0)) <= 1e-15
    _table_equals(table[0], c, want, where)
    return got


# ---- the table of the cases tests/test_gpu_speed_search.py runs ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SEEDED)
def test_the_seeded_shapes_table(handle, name):
    c, want = G._reference(name)
    table = []
    rc, dev, _ = G._device(handle, c, table=table)
    assert rc == 0, handle.lib.pqp_last_error()
    G._same(dev, want, name)
    _table_equals(table[0], c, want, name)


def test_the_hand_batches_table(handle):
    car = capi.car_default_geometry(**S.HAND_CAR)
    for names, c in G._hand_batch():
        want = S.run_case(c, G.circles(True))
        table = []
        rc, dev, _ = G._device(handle, c, car=car, table=table)
        assert rc == 0, handle.lib.pqp_last_error()
        G._same(dev, want, names)
        _table_equals(table[0], c, want, names)


# ---- plans that die late, and plans that only the rules decide ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.DEAD_ENDS)
def test_dead_ends_at_full_table_size(handle, name):
    """S = 200, Q = 19, m = 12: four plans die at layers 8, 5, 5 and 1 with living states in every wavefront of their last layer, several
    to a lane, and winners outside the first wavefront (tests/test_speed_search.py holds that).  "ties": every cost is 0"""
    c, want = _family(name)
    got = _both_forms(handle, c, want, name)
    m = c["m"]
    assert got["reached"].tolist() == [8, 5, 5, 1, m]
    for b, reached in enumerate(got["reached"]):            # the rows behind a dead end
        assert (got["steps"][b, reached:] == -1).all() and (got["traj"][b, reached:] == 0).all() and got["traj"][b, reached - 1, 6] == 0, b
        if reached < m:
            assert got["flags"][b] & S.NO_PLAN and not got["flags"][b] & S.ARRIVED, b
    print(f"{name}: reached {got['reached'].tolist()} flags {got['flags'].tolist()} cost {got['cost'].tolist()}")


def test_the_refine_keeps_the_rows_of_plans_that_die_late(handle):
    """pqp_speed_refine behind the search on "dead": a path without a full plan keeps the searched rows bit for bit"""
    c, want = _family("dead")
    res = G._host(handle, c)
    G._same(res, want, "dead")
    got = handle.speed_refine(c["paths"], c["profile"], c["v_start"], res["blocked"], res["steps"], res["reached"], res["traj"], n_of=c.get("n_of"),
                              stop_before=c.get("stop_before"), grid=capi.search_default_params(**c["prm"]))
    for b in range(4):
        assert 0 < res["reached"][b] < c["m"] and got["flags"][b] == R.KEPT and got["status"][b] == R.UNSOLVED, (b, got["flags"][b], got["status"][b])
        assert same_bits(got["traj"][b], res["traj"][b]) and (got["bounds"][b] == 0.0).all() and np.isnan(got["cost"][b]) and np.isnan(got["excess"][b]), b
    assert res["reached"][4] == c["m"] and got["flags"][4] & (R.REFINED | R.KEPT)
    if got["flags"][4] & R.KEPT:
        assert same_bits(got["traj"][4], res["traj"][4])
    else:                                                    # the refined neighbour: on its path's stations still, at the layers' times
        assert same_bits(got["traj"][4][:, 7], res["traj"][4][:, 7]) and (got["traj"][4][:, 5] >= 0.0).all()


# ---- more layers than lanes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.HORIZONS)
def test_horizons_beyond_a_wavefront_and_a_workgroup(handle, name):
    """m = 70 and m = 260 on S = 24, Q = 3: the rows are written by a second wavefront and in a second turn of the workgroup, and an empty
    and a non-finite path between the ordinary ones have more rows to fill than a wavefront (blocked) or the workgroup (traj, steps) has
    lanes.  The ordinary paths are bit for bit what they are in a batch of their own"""
    c, want = _family(name)
    got = _both_forms(handle, c, want, name)
    m = c["m"]
    assert got["flags"].tolist() == [S.ARRIVED, S.EMPTY, S.GRID_SHORT, S.NOT_FINITE, S.GRID_SHORT] and got["reached"].tolist() == [m, 0, m, 0, m]
    assert (got["traj"][1] == 0).all() and np.isnan(got["traj"][3]).all() and (got["steps"][[1, 3]] == -1).all() and (got["blocked"][[1, 3]] == 0).all()
    assert got["cost"][1] == np.inf and np.isnan(got["cost"][3])
    keep = np.array([0, 2, 4])
    alone = dict(c, paths=c["paths"][keep], profile=c["profile"][keep], v_start=c["v_start"][keep], n_of=c["n_of"][keep], scene_of=c["scene_of"][keep])
    one = G._host(handle, alone)
    for k in G.EXACT + ("cost", "traj"):
        assert same_bits(np.asarray(one[k], dtype=np.float64), np.asarray(got[k][keep], dtype=np.float64)), (name, k)


# ---- other steps, weights, window and stride; a car that can only stand; many station tiles ----------------------------------------------------
@pytest.mark.parametrize("name", ("steps", "standing", "wide", "thin"))
def test_the_other_families_against_the_restatement(handle, name):
    c, want = _family(name)
    got = _both_forms(handle, c, want, name)
    if c["prm"]["q_max"] == 0:                               # the stationary plan: at station 0 in every row that is planned
        for b, reached in enumerate(got["reached"]):
            assert (got["steps"][b, :reached] == 0).all() and (got["traj"][b, :reached, 4:7] == 0).all(), b
    print(f"{name}: reached {got['reached'].tolist()} flags {got['flags'].tolist()} cost {got['cost'].tolist()}")
