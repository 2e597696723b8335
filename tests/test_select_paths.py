"""pqp_select_paths without a GPU: the symbols and the binding, the default parameters, the C++ wrapper's build, and known answers
written out by hand for the numpy restatement (tests/select_util.py) the GPU tests compare the kernels against."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import build_util
import cpp_demo
import select_util as S
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_select_default_params", "pqp_select_paths", "pqp_select_paths_device")


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES:
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    assert capi.SCORE_STRIDE == 8 and C.sizeof(capi.PqpSelectParams) == 6 * 8 + 2 * 4
    for fn in (hip_lib.pqp_select_paths, hip_lib.pqp_select_paths_device):
        assert len(fn.argtypes) == 17
    assert callable(capi.Handle.select_paths)


def test_default_params_are_the_path_qps_weights(hip_lib):
    p = capi.select_default_params(hip_lib)
    got = (p.weight_kappa, p.weight_dkappa, p.weight_offset, p.weight_length, p.weight_clearance, p.clearance_want, p.per_waypoint, p.require_free)
    assert got == (20.0, 100.0, 0.0, 0.0, 0.0, 0.6, 0, 1)
    q = capi.default_params(hip_lib)
    assert (p.weight_kappa, p.weight_dkappa) == (q.weight_kappa, q.weight_dkappa)
    assert capi.select_default_params(hip_lib, weight_length=2.5, require_free=0).weight_length == 2.5
    d = S.Params()
    assert got == (d.weight_kappa, d.weight_dkappa, d.weight_offset, d.weight_length, d.weight_clearance, d.clearance_want, d.per_waypoint,
                   d.require_free)


def test_selector_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("select_demo")
    import torch
    if torch.cuda.is_available():
        return
    path = tmp_path / "candidates.bin"
    S.write_candidates(path, [np.zeros((3, 7)), np.ones((2, 7))], [0, 2])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no selector" in r.stderr


def test_both_kernels_use_no_scratch_and_no_lds(hip_lib):
    kernels = build_util.kernel_report()
    for name in ("path_score_kernel", "group_select_kernel"):
        r = build_util.find_kernel(kernels, name)
        assert r["ScratchSize"] == 0 and r["LDS Size"] == 0 and r["Occupancy"] >= 8, (name, r)


# ---- known answers of the restatement --------------------------------------------------------------------------------------------------
def _row(x, y, l, k, dk, heading=0.0, d_heading=0.0):
    return [x, y, heading, l, d_heading, k, dk]


def _batch(cands, n=None):
    n = n or max(len(c) for c in cands)
    paths = np.zeros((len(cands), n, 7))
    for b, c in enumerate(cands):
        paths[b, :len(c)] = np.reshape(c, (len(c), 7))
    return paths, np.array([len(c) for c in cands], np.int32)


THREE = [_row(0.0, 0.0, 0.5, 0.1, 0.02), _row(3.0, 4.0, -1.0, 0.2, -0.03), _row(3.0, 10.0, 2.0, -0.3, 7.0)]


def test_three_waypoints_by_hand():
    """k: .01 + .04 + .09; dk without the last: .0004 + .0009; l: .25 + 1 + 4; chords 5 and 6; margins .1, .7, .4 against .6: .25 + 0 + .04"""
    paths, n_of = _batch([THREE], n=5)
    paths[0, 3:] = 99.0                                    # beyond the count: not read
    margin = np.array([[0.1, 0.7, 0.4, -5.0, -5.0]])
    prm = S.Params(weight_kappa=2.0, weight_dkappa=1000.0, weight_offset=1.0, weight_length=0.5, weight_clearance=10.0)
    t = S.terms(paths, n_of, margin=margin, prm=prm)[0]
    np.testing.assert_allclose(t[1:7], [0.14, 0.0013, 5.25, 11.0, 0.1, 0.29], rtol=1e-14)
    np.testing.assert_allclose(t[0], 2 * 0.14 + 1000 * 0.0013 + 5.25 + 5.5 + 2.9, rtol=1e-14)
    assert t[7] == 1.0
    # per waypoint: the three sums over waypoints and the clearance sum by the count, the length as it is
    prm.per_waypoint = 1
    t = S.terms(paths, n_of, margin=margin, prm=prm)[0]
    np.testing.assert_allclose(t[1:7], [0.14 / 3, 0.0013 / 3, 1.75, 11.0, 0.1, 0.29 / 3], rtol=1e-14)
    # the defaults: twice the QP's objective; no margin given: terms 5 and 6 are 0
    t = S.terms(paths, n_of)[0]
    np.testing.assert_allclose(t[0], 20 * 0.14 + 100 * 0.0013, rtol=1e-14)
    assert t[5] == 0.0 and t[6] == 0.0
    r = S.select(paths, [0, 1], n_of)
    assert r["best"].tolist() == [0] and r["best_n"].tolist() == [3]
    assert np.array_equal(r["best_paths"][0, :3], np.array(THREE)) and (r["best_paths"][0, 3:] == 0).all()


def test_a_tie_goes_to_the_lower_index():
    worse = [_row(0, 0, 0, 0.5, 0), _row(1, 0, 0, 0.5, 0)]
    paths, n_of = _batch([worse, THREE, THREE, worse])
    r = S.select(paths, [0, 4], n_of)
    assert r["terms"][1, 0] == r["terms"][2, 0] < r["terms"][0, 0]
    assert r["best"].tolist() == [1]
    assert S.select(paths[::-1].copy(), [0, 4], n_of[::-1].copy())["best"].tolist() == [1]


def test_the_cheapest_candidate_collides():
    cheap = [_row(0, 0, 0, 0.01, 0), _row(1, 0, 0, 0.01, 0), _row(2, 0, 0, 0.01, 0)]
    paths, n_of = _batch([THREE, cheap])
    first = np.array([3, 1], np.int32)                     # candidate 1 collides at its waypoint 1
    assert S.select(paths, [0, 2], n_of, first_collision=first)["best"].tolist() == [0]
    r = S.select(paths, [0, 2], n_of, first_collision=first, prm=S.Params(require_free=0))
    assert r["best"].tolist() == [1] and r["terms"][:, 7].tolist() == [1.0, 1.0]
    assert S.select(paths, [0, 2], n_of)["best"].tolist() == [1]


def test_empty_groups_and_groups_without_an_eligible_candidate():
    short = [_row(0, 0, 0, 0, 0)]
    paths, n_of = _batch([THREE, short, THREE, THREE, []])
    status = np.array([1, 1, 2, 1, 1], np.int32)           # candidate 2 ran out of iterations
    stage = np.array([0, 0, 0, 3, 0], np.int32)            # candidate 3 stopped in the chain
    r = S.select(paths, [0, 0, 1, 1, 5, 5], n_of, status=status, stage=stage)
    assert r["best"].tolist() == [-1, 0, -1, -1, -1]
    assert r["terms"][:, 7].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert (r["terms"][1] == 0).all() and (r["terms"][4] == 0).all()          # a count below 2: zeros
    assert r["terms"][2, 0] == r["terms"][0, 0]                                 # not eligible, its terms all the same
    assert r["best_n"].tolist() == [0, 3, 0, 0, 0] and (r["best_paths"][[0, 2, 3, 4]] == 0).all()


def test_a_path_that_is_not_a_number_cannot_win():
    bad = [list(r) for r in THREE]
    bad[1][5] = math.nan
    far = [list(r) for r in THREE]
    far[2][0] = math.inf                                   # an infinite length under weight 0: 0 * inf is not finite either
    paths, n_of = _batch([bad, far, THREE])
    r = S.select(paths, [0, 3], n_of)
    assert r["best"].tolist() == [2] and r["terms"][:, 7].tolist() == [0.0, 0.0, 1.0]
    assert math.isnan(r["terms"][0, 0]) and math.isnan(r["terms"][1, 0])
    assert S.select(paths[:2], [0, 2], n_of[:2])["best"].tolist() == [-1]


def test_group_boundaries_as_the_device_form_reads_them():
    assert S.group_bounds([0, 3, 99, 5, 2, 8], 8) == [(0, 3), (3, 8), (8, 8), (5, 5), (2, 8)]
    assert S.group_bounds([-4, 2], 8) == [(0, 2)]
