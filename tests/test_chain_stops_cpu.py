"""The scenarios of chain_stops_util.mixed_batch() are what they claim to be: with oracle/corridor_oracle.py alone (no library, no GPU),
every count a stop depends on lies on the intended side of its threshold by 2 or more, so a count that differs by one between the device
and the oracle cannot move a scenario to another stage.

The oracle has no smoother QPs.  Here the raw line's 1 m samples stand in for the smoothed line and the search's centre of each layer's
bounds for postSmooth's offsets: the QPs move the points by decimetres at most on these roads, which moves a count of 1 m samples, 1.5 m
layers or 0.3 m waypoints by one at most.  Where a margin of 2 cannot exist - a count that is bounded below by 2 has to be below 3, a layer
count has to lie in 1 .. 3 - the test pins the continuous quantity behind the count to the middle of its interval instead and says so."""
import math

import numpy as np
import pytest

import chain_stops_util as CS
import corridor_oracle as K
from shared_util import oracle_geom

R, S, L, N = (CS.MIXED_CFG[k] for k in ("raw_max", "sample_max", "layer_max", "n_max"))
MARGIN = 2
SAMPLE_MIN = 4                     # the larger of the two smoothers' minima (TensionSmoother)


@pytest.fixture(scope="module")
def batch():
    return CS.mixed_batch()


def _counts(sc, b, upto="all", map_of=None):
    """the oracle's counts of scenario b, as far as they exist: raw, samples, layers_needed (what the line asks of layer_max), layers (what the
    search keeps), vehicle_l, heading_err, ref_count, n_valid"""
    P = int(sc["n_pts"][b])
    p = sc["pts"][b, :P]
    g = oracle_geom(sc["geom"])
    dist = sc["dist"][(sc["map_of"] if map_of is None else map_of)[b]]
    out = {}
    x, y, s = K.bspline_resample(p)
    out["raw"], out["raw_len"] = len(x), s[-1]
    if len(x) < 3 or upto == "raw":
        return out
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    gx, gy, gs, _, _ = K.segment_raw_reference(sx, sy, s[-1])
    out["samples"] = len(gs)
    if upto == "samples":
        return out
    # the smoothed line: through the samples, abscissa = accumulated chord length, declared 3 m longer than its last point
    ss = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(gx), np.diff(gy)))])
    mx, my = K.spline_fit(ss, gx), K.spline_fit(ss, gy)
    length = ss[-1] + 3.0
    start = sc["start"][b]
    s0 = K.projection(mx, my, start[0], start[1], length)
    ds = 1.5 if length > 6 else 0.5
    out["layers_needed"] = int(math.ceil((length - s0) / ds - 1e-12)) + 1
    out["s0"], out["length"] = s0, length
    ph = math.atan2(K.spline_deriv(my, 1, s0), K.spline_deriv(mx, 1, s0))
    out["vehicle_l"] = K.global2local_y(K.spline_eval(mx, s0), K.spline_eval(my, s0), ph, start[0], start[1])
    if upto == "layers_needed" or abs(out["vehicle_l"]) > 10.0:
        return out
    dp = K.graph_search_dp(mx, my, length, start, dist, g)
    out["layers"] = 0 if dp is None else len(dp["layers_s"])
    assert dp is None or dp["n_layers_sampled"] == out["layers_needed"]
    if out["layers"] < 4:
        return out
    l = np.clip(0.0, dp["lb"], dp["ub"]); l[0] = dp["vehicle_l"]
    fx, fy, fs = K.offsets_to_points(mx, my, dp["layers_s"], l)
    qx, qy = K.spline_fit(fs, fx), K.spline_fit(fs, fy)
    max_s = K.reference_length(qx, qy, fs[-1], sc["target"][b, 0], sc["target"][b, 1])
    out["heading_err"] = K.process_init_state(qx, qy, *start)[1]
    ref = K.build_reference_from_spline(qx, qy, max_s)
    out["ref_count"] = len(ref)
    if upto == "ref_count":
        return out
    out["n_valid"] = K.update_bounds_improved(ref[:N], qx, qy, dist, g)[1]
    return out


def _fits(c, upto):
    """every count up to `upto` fits its capacity and its minimum with the margin"""
    order = ["raw", "samples", "layers", "ref_count", "n_valid"]
    for k in order[:order.index(upto) + 1]:
        if k == "raw":
            assert 3 + MARGIN <= c["raw"] <= R - MARGIN, c
        if k == "samples":
            assert SAMPLE_MIN + MARGIN <= c["samples"] <= S - MARGIN, c
        if k == "layers":
            assert abs(c["vehicle_l"]) < 8.0 and c["layers_needed"] <= L - MARGIN and c["layers"] >= 4 + MARGIN, c
        if k == "ref_count":
            assert abs(c["heading_err"]) < math.radians(75 - 20) and c["ref_count"] <= N - MARGIN, c
        if k == "n_valid":
            assert c["n_valid"] >= 2 + MARGIN, c


def test_the_plan_covers_every_site(batch):
    kinds = set(batch["kind"])
    assert {"cap_" + s for s in CS.CAPACITY_SITES} <= kinds
    assert set(CS.INTENDED[k] for k in kinds) == {0, 1, 3, 4, 6, 7, 8, 9}          # (2 and 5 come from the smoother handle, not from inputs)
    assert batch["healthy"].sum() >= 4
    assert sorted(batch["n_pts"][[b for b, k in enumerate(batch["kind"]) if k == "few_points"]]) == [-1, 0, 3]
    # the groups of the selection: each holds a healthy candidate except group 1, which holds stopped ones only
    gs = CS.GROUP_START
    assert gs[0] == 0 and gs[-1] == len(batch["kind"])
    for g in range(len(gs) - 1):
        assert batch["healthy"][gs[g]:gs[g + 1]].any() == (g != 1)
    # the rows of a scenario that is to stop for its count alone are filled like a healthy one's
    assert all(np.abs(batch["pts"][b, :4]).sum() > 0 for b in range(len(batch["kind"])))


def test_healthy_scenarios_fit_every_capacity(batch):
    seen = set()
    for b in np.flatnonzero(batch["healthy"]):
        c = _counts(batch, b)
        _fits(c, "n_valid")
        seen.add((c["raw"], c["layers"], c["ref_count"]))
    assert len(seen) >= 3                                   # a ragged batch


def test_no_raw_line(batch):
    """n_points above p_max; 4 and 5 points about 3 m apart: degree 5, which is not below the number of control points"""
    p_max = batch["pts"].shape[1]
    for b, k in enumerate(batch["kind"]):
        P = int(batch["n_pts"][b])
        if k == "no_line_p_max":
            assert P == p_max + 1
        if k == "no_line_degree":
            p = batch["pts"][b, :P]
            mean = np.hypot(np.diff(p[:, 0]), np.diff(p[:, 1])).sum() / (P - 1)
            assert 4 <= P <= 5 and 2.0 < mean < 4.0 and CS.bspline_degree(p) == 5 and not P > CS.bspline_degree(p)
    assert sorted(batch["n_pts"][b] for b, k in enumerate(batch["kind"]) if k == "no_line_degree") == [4, 5]


def test_capacity_sites(batch):
    at = {k: b for b, k in enumerate(batch["kind"])}
    c = _counts(batch, at["cap_raw_max"], "raw")
    assert c["raw"] >= R + MARGIN, c
    c = _counts(batch, at["cap_sample_max"], "samples")
    _fits(c, "raw")
    assert c["samples"] >= S + MARGIN, c
    # fewer than 3 samples means 2 - the samples at 0 and at the first abscissa >= the length are always there - so no margin of 2 exists:
    # what is pinned is the length, 0.6 m, in the middle of (0, 1), where the raw line has its 2 points (t = 0, t = 1) and 2 samples
    c = _counts(batch, at["cap_sample_min"], "raw")
    assert c["raw"] == 2 and 0.4 < c["raw_len"] < 0.8, c
    c = _counts(batch, at["cap_layer_max"], "layers_needed")
    _fits(c, "samples")
    assert abs(c["vehicle_l"]) < 8.0 and c["layers_needed"] >= L + MARGIN, c
    c = _counts(batch, at["cap_n_max"], "ref_count")
    _fits(c, "layers")
    assert abs(c["heading_err"]) < math.radians(55) and c["ref_count"] >= N + MARGIN, c


def test_search_heading_short_and_blocked(batch):
    at = {k: b for b, k in enumerate(batch["kind"])}
    c = _counts(batch, at["search_failed"], "layers_needed")
    _fits(c, "samples")
    assert abs(c["vehicle_l"]) > 10.0 + MARGIN, c              # lateral range 10 m: graphSearchDp returns false
    c = _counts(batch, at["heading"], "ref_count")
    _fits(c, "layers")
    assert abs(c["heading_err"]) > math.radians(75 + 10), c
    # 1 .. 3 layers leave no margin of 2 on either side: the line is declared 8 m long (> 6 m: layers 1.5 m apart) and the vehicle stands
    # 0.75 m before its end, in the middle of the (0, 1.5] m that give exactly 2 layers
    c = _counts(batch, at["short_reference"])
    _fits(c, "samples")
    assert c["length"] > 7.0 and 0.4 < c["length"] - c["s0"] < 1.1 and c["layers_needed"] == 2 and 1 <= c["layers"] <= 2, c
    # the pit closes the road at the first waypoint; on the map without it the same scenario is healthy
    b = at["blocked"]
    c = _counts(batch, b)
    _fits(c, "ref_count")
    assert c["n_valid"] == 0, c
    _fits(_counts(batch, b, map_of=batch["open_map"]), "n_valid")
    # the NaN start curvature reaches nothing before the path QP: healthy up to there
    _fits(_counts(batch, at["qp_nan"]), "n_valid")
    assert np.isnan(batch["start_k"][at["qp_nan"]]) and np.isfinite(np.delete(batch["start_k"], at["qp_nan"])).all()
