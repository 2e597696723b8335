"""The scenes of tests/dp_cases.py, from the oracle alone (no GPU): every scene keeps the margins that make the device comparison of
tests/test_gpu_dp_cases.py exact, covers what its name says, and - the mutation table - each of seven defects of the cost model or the parent
choice changes the bounds or the layer count of at least one scene, so a kernel with that defect fails the comparison."""
import numpy as np
import pytest

import corridor_oracle as K
import corridor_util as U
import dp_cases as D


@pytest.mark.parametrize("name", D.NAMES)
def test_scene_keeps_its_margins(name):
    e = D.expected(name)
    assert e is not None
    print(f"{name}: layers {len(e['lb'])} of {e['n_layers_sampled']}, distinct indices {len(set(e['path']))}, margin_cost {e['margin_cost']:.3e}, "
          f"ties {e['n_ties']} ({e['ties_on_path']} on the path), margin_d {e['margin_d']:.3e}")
    assert e["margin_cost"] >= D.COST_MARGIN
    assert e["margin_d"] >= D.D_MARGIN
    assert min(e["margin_lb"].min(), e["margin_ub"].min()) >= e["margin_d"]
    assert len(set(e["path"])) >= D.MIN_DISTINCT
    assert len(e["path"]) == len(e["lb"]) == e["max_layer"] + 1
    if name == "tie":
        assert e["ties_on_path"] >= 1
    else:
        assert e["n_ties"] == 0
    # the path is a path: consecutive nodes are admissible (|dl| <= ds)
    sc = D.scenes()[name]
    dl = np.abs(np.diff(e["path"])) * sc["prm"].lateral_spacing
    assert np.all(dl <= np.diff(e["layers_s"]) + 1e-12)


def test_scene_sizes():
    sc = D.scenes()
    for name in D.NAMES:
        g = sc[name]["geom"]
        assert sc[name]["tab"].shape == (9, D.KNOTS)
        assert g.rows * g.cols <= 300 * 150 and sc[name]["dist"].dtype == np.float32
        n = D.expected(name)["n_layers_sampled"]
        assert 66 <= n <= 80 if name == "long" else 20 <= n <= 45, (name, n)
    assert len(D.NAMES) <= 14 and set(D.BATCHABLE) <= set(D.NAMES)
    for name in D.BATCHABLE:                   # one launch takes them all: one geometry, one knot count, one lateral grid
        assert sc[name]["geom"] == D.GEOM and sc[name]["prm"] == K.DpParams()


def _window(sc, ds):
    """(R, nlat) of pqp_dp_body.inc for a layer `ds` behind its predecessor"""
    prm = sc["prm"]
    return int(ds / prm.lateral_spacing) + 1, U.dp_lateral_samples(prm.lateral_range, prm.lateral_spacing)


def test_what_the_named_scenes_cover():
    sc = D.scenes()
    # several feasible runs per layer where the obstacles are: the bounds name the run
    for name in D.NAMES:
        if name.startswith(("discs", "lanes")):
            e = D.expected(name)
            assert len(e["lb"]) == e["n_layers_sampled"]
            assert len(set(zip(np.round(e["lb"][1:], 6), np.round(e["ub"][1:], 6)))) >= 3
    # the long scene: the index changes into and out of the first layer of the second and of the third chunk of 32 prepared layers, whose
    # slots in the ring of 33 are 32, 0 and 31, 32
    p = D.expected("long")["path"]
    assert len(p) >= 66
    for i in (32, 64):
        assert p[i - 1] != p[i] and p[i] != p[i + 1], (i, p[i - 1:i + 2])
    # the window: a strict subset, the whole layer, and a last layer with a window of its own
    R, nlat = _window(sc["narrow"], 1.5)
    assert 2 * R + 1 < nlat and sc["narrow"]["prm"] != K.DpParams()
    R, nlat = _window(sc["full"], 2.4)
    assert 2 * R + 1 >= nlat and sc["full"]["prm"] != K.DpParams()
    ds = np.diff(D.expected("short_last")["layers_s"])
    assert _window(sc["short_last"], ds[-1])[0] == 1 and all(_window(sc["short_last"], v)[0] == 3 for v in ds[:-1])
    # the wall: stopped midway, well behind the start
    e = D.expected("wall")
    assert 8 <= len(e["lb"]) < e["n_layers_sampled"] - 3


def _differs(a, b):
    if len(a["lb"]) != len(b["lb"]):
        return "count"
    k = int(((np.abs(a["lb"] - b["lb"]) >= 1e-9) | (np.abs(a["ub"] - b["ub"]) >= 1e-9)).sum())
    return k or None


def test_mutation_table():
    """each defect, as a setting of the oracle's knobs, changes at least one lb / ub entry by >= 1e-9, or the count, in at least one scene"""
    table = {}
    for mut, knobs in D.MUTATIONS.items():
        table[mut] = {name: _differs(D.expected(name), D.expected(name, knobs)) for name in D.NAMES}
        caught = {n: v for n, v in table[mut].items() if v}
        print(f"{mut:42s} caught by " + (", ".join(f"{n} ({v})" for n, v in caught.items()) or "NOTHING"))
    for mut in D.MUTATIONS:
        assert any(table[mut].values()), mut
    # where the issue names the scene: the narrowed window on the strict-subset grid, the tie rule on the tie scene
    assert table["window ds -> ds / 2"]["narrow"]
    assert table["last wins on ties"]["tie"]


def test_default_knobs_are_the_reference_cost_model():
    """the knobs at their defaults change nothing, bit for bit (tests/test_corridor_oracle.py holds the goldens)"""
    sc = D.scenes()["discs_0"]
    a = D.expected("discs_0")
    b = K.graph_search_dp(sc["sx"], sc["sy"], sc["length"], sc["start"], sc["dist"], sc["geom"], prm=sc["prm"], knobs=K.DpCostKnobs())
    assert a["path"] == b["path"] and np.array_equal(a["lb"], b["lb"]) and np.array_equal(a["ub"], b["ub"])
    assert (K.DpCostKnobs().w_prev_dir, K.DpCostKnobs().w_heading, K.DpCostKnobs().w_dist, K.DpCostKnobs().w_lateral) == (16.0, 0.5, 0.5, 1.0)


def test_the_shared_comparison_excuses_only_flagged_entries_off_by_whole_steps():
    """corridor_util.dp_bounds_agree, the comparison of the older DP tests, on made-up disagreements"""
    n = 40
    want = dict(lb=np.full(n, -2.2), ub=np.full(n, 3.4), margin_lb=np.full(n, 1e-3), margin_ub=np.full(n, 1e-3))
    assert U.dp_bounds_agree(want["lb"].copy(), want["ub"].copy(), want) == 0 and U.dp_flagged(want) == 0
    lb = want["lb"].copy()
    lb[7] += 0.4
    with pytest.raises(AssertionError):                     # off by two steps, but no test near the threshold
        U.dp_bounds_agree(lb, want["ub"], want)
    flagged = dict(want, margin_lb=want["margin_lb"].copy())
    flagged["margin_lb"][7] = 3e-8
    assert U.dp_bounds_agree(lb, want["ub"], flagged) == 1 and U.dp_flagged(flagged) == 1
    with pytest.raises(AssertionError):                     # the other side of the flagged layer is not excused
        U.dp_bounds_agree(want["lb"], np.where(np.arange(n) == 7, 3.6, want["ub"]), flagged)
    lb[7] = want["lb"][7] + 0.13
    with pytest.raises(AssertionError):                     # flagged, but not a whole number of 0.2 m steps
        U.dp_bounds_agree(lb, want["ub"], flagged)
    many = dict(want, margin_lb=np.full(n, 3e-8))
    with pytest.raises(AssertionError):                     # flagged and whole steps, but more than 5 % of the layers
        U.dp_bounds_agree(want["lb"] + np.where(np.arange(n) < 3, 0.2, 0.0), want["ub"], many)


def test_batch_scenarios_cover_the_three_ways_out():
    b = D.batch()
    want = [D.batch_expected(q) for q in range(len(b["names"]))]
    assert len(want) >= 6 and len(set(b["map_of"])) >= 3
    counts = [D.batch_count(w, b["max_layers"]) for w in want]
    assert 0 in counts and -1 in counts
    stopped = [q for q, w in enumerate(want) if w is not None and 0 < len(w["lb"]) < w["n_layers_sampled"] <= b["max_layers"]]
    assert stopped
    assert sum(c > 0 for c in counts) >= 4
