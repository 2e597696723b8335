"""pqp_overlay_agents without a GPU: the numpy restatement (tests/overlay_util.py) against an independent check of the distance and against
distance_util's layers, standing_rows, the symbols and the binding, the refusals, the chain wrapper's plan with parked=, the C++
wrapper's build and the kernel's resources."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

import build_util
import cpp_demo
import distance_util
import overlay_util as V
from path_optimizer_2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqp_overlay_agents", "pqp_overlay_agents_device")


@pytest.fixture(scope="module")
def kernels():
    return build_util.kernel_report()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _boundary(agent, step=1e-3):
    """points on the boundary of a rounded rectangle (x, y, heading, hl, hw, radius), at most `step` apart: the four sides pushed out by
    the radius and the four quarter circles round the corners"""
    x, y, h, hl, hw, r = agent
    pts = []
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        half = hw if sx else hl
        t = np.linspace(-half, half, int(2 * half / step) + 2)
        pts.append(np.stack([sx * (hl + r) + 0 * t, t], 1) if sx else np.stack([t, sy * (hw + r) + 0 * t], 1))
    if r > 0.0:
        a = np.linspace(0.0, 0.5 * math.pi, int(0.5 * math.pi * r / step) + 2)
        for q, (cx, cy) in enumerate(((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))):
            pts.append(np.stack([cx + r * np.cos(a + q * 0.5 * math.pi), cy + r * np.sin(a + q * 0.5 * math.pi)], 1))
    p = np.concatenate(pts)
    c, s = math.cos(h), math.sin(h)
    return np.stack([x + p[:, 0] * c - p[:, 1] * s, y + p[:, 0] * s + p[:, 1] * c], 1)


def _inside(agent, px, py):
    """the shape as a union of two rectangles and four discs, in the agent's frame"""
    x, y, h, hl, hw, r = agent
    c, s = math.cos(h), math.sin(h)
    u, w = np.abs((px - x) * c + (py - y) * s), np.abs((py - y) * c - (px - x) * s)
    return ((u <= hl + r) & (w <= hw)) | ((u <= hl) & (w <= hw + r)) | ((u - hl) ** 2 + (w - hw) ** 2 <= r * r)


def test_the_restated_distance_against_the_nearest_boundary_sample():
    """random rounded rectangles, the boundary sampled every 1e-3 m: the cell is 0 when its centre lies inside the shape, else the
    distance to the nearest sample - to within 2e-3 m (the sample spacing; the brute-force minimum is never below the true distance by
    more than rounding, and above it by less than half a step's chord)"""
    rng = np.random.default_rng(11)
    geom = V.geometry(23, 17, 0.3, 1.5, -2.0)
    cx, cy = V.cell_centres(geom)
    px, py = np.meshgrid(cx, cy, indexing="ij")
    for k in range(12):
        agent = [rng.uniform(cx.min(), cx.max()), rng.uniform(cy.min(), cy.max()), rng.uniform(-math.pi, math.pi),
                 (0.0, rng.uniform(0.1, 2.0))[k % 3 > 0], (0.0, rng.uniform(0.1, 1.0))[k % 3 > 0], (rng.uniform(0.05, 0.5), 0.0)[k % 4 == 1]]
        if k == 5:
            agent[3:] = [0.0, 0.0, 0.0]                                           # a point
        got, bad = V.agents_distance(geom, np.array([agent]))
        assert not bad
        if agent[3] == agent[4] == agent[5] == 0.0:
            want = np.hypot(px - agent[0], py - agent[1])
        else:
            b = _boundary(agent)
            want = np.sqrt(((px[..., None] - b[:, 0]) ** 2 + (py[..., None] - b[:, 1]) ** 2).min(axis=2))
            want[_inside(agent, px, py)] = 0.0
        assert np.abs(got - want).max() <= 2e-3, (k, agent)


def test_the_overlay_equals_the_layer_of_the_occupancy_with_the_covered_cells_set():
    """cell-aligned boxes, heading 0, no radius, on maps with obstacles: the overlay is distance_util.distance_layer of the occupancy
    with the covered cells set to 0, to within one cell diagonal (the box's edge against the covered cells' centres), and never above
    the base"""
    rng = np.random.default_rng(3)
    res = 0.2
    for rows, cols in ((30, 21), (17, 40)):
        geom = V.geometry(rows, cols, res, 0.7, -1.1)
        cx, cy = V.cell_centres(geom)
        grid = np.where(rng.uniform(size=(rows, cols)) < 0.03, 0, 255).astype(np.uint8)
        grid[1, 1] = 0
        base = distance_util.distance_layer(grid, res)
        agents, covered = [], grid.copy()
        for _ in range(3):
            i0, j0 = int(rng.integers(0, rows - 4)), int(rng.integers(0, cols - 4))
            ni, nj = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            # the box from the outer edge of cell i0 to that of cell i0 + ni - 1: it covers those cells' centres and no others
            xs, ys = cx[i0:i0 + ni], cy[j0:j0 + nj]
            agents.append([0.5 * (xs[0] + xs[-1]), 0.5 * (ys[0] + ys[-1]), 0.0, 0.5 * ni * res, 0.5 * nj * res, 0.0])
            covered[i0:i0 + ni, j0:j0 + nj] = 0
        out, flags, _ = V.overlay(base, geom, np.array([agents]))
        want = distance_util.distance_layer(covered, res)
        assert flags.tolist() == [0]
        assert (out[0] <= base).all()
        assert np.array_equal(out[0] == 0.0, covered == 0)
        assert np.abs(out[0].astype(np.float64) - want).max() <= res * math.sqrt(2.0) + 1e-6


def test_bad_none_and_nan_by_hand():
    geom = V.geometry(4, 3, 0.5)
    base = np.arange(12, dtype=np.float32).reshape(1, 4, 3)
    base[0, 2, 1] = math.nan
    box = [0.0, 0.0, 0.0, 0.25, 0.25, 0.0]
    agents = np.array([[box, V.ABSENT], [V.ABSENT, V.ABSENT], [box, [0.0, math.inf, 0.0, 1.0, 1.0, 0.0]], [box, [0.0, 0.0, 0.0, 1.0, 1.0, -1.0]]])
    out, flags, decided = V.overlay(base, geom, agents)
    assert flags.tolist() == [0, V.OVERLAY_NONE, V.OVERLAY_BAD, V.OVERLAY_BAD]
    assert out[1].tobytes() == base[0].tobytes() and not decided[1].any()
    assert (out[2] == 0.0).all() and (out[3] == 0.0).all()
    assert math.isnan(out[0, 2, 1]) and not decided[0, 2, 1]                          # a NaN base value stays
    assert out[0, 0, 0] == 0.0 and (out[0] <= base[0])[~np.isnan(base[0])].all()
    # the count applies before anything is read: the bad row behind it is not there
    out, flags, _ = V.overlay(base, geom, agents[2:3], a_of=[1])
    assert flags.tolist() == [0]
    # base_of picks the layer, clamped; inflate moves the shape out and never below 0
    two = np.stack([base[0], base[0] + 1.0])
    out, _, _ = V.overlay(two, geom, np.array([[V.ABSENT]] * 3), base_of=[1, 0, 7])
    assert out[0].tobytes() == two[1].tobytes() and out[1].tobytes() == two[0].tobytes() and out[2].tobytes() == two[1].tobytes()
    d0, _ = V.agents_distance(geom, np.array([box]))
    d1, _ = V.agents_distance(geom, np.array([box]), inflate=0.3)
    assert np.array_equal(d1, np.fmax(d0 - 0.3, 0.0)) and (d1 >= 0.0).all()
    cx, cy = V.cell_centres(geom)
    assert cx.tolist() == [0.75, 0.25, -0.25, -0.75] and cy.tolist() == [0.5, 0.0, -0.5]


def test_the_tolerance_rule_holds_the_restatement_and_sees_a_wrong_cell():
    c = V.seeded_scenes(5, 20, 11, 0.2, ("empty", "dense"), 2, 3)
    out, _, decided = V.overlay(c["dist"], c["geom"], c["agents"])
    assert V.within_tolerance(out, c["dist"], c["geom"], c["agents"]) >= int(decided.sum()) > 0
    wrong = out.copy()
    i = tuple(np.argwhere(decided & (out > 0.0))[0])
    wrong[i] = np.nextafter(np.nextafter(wrong[i], np.float32(np.inf)), np.float32(np.inf)) + np.float32(1e-6)
    with pytest.raises(AssertionError):
        V.within_tolerance(wrong, c["dist"], c["geom"], c["agents"])
    wrong = out.copy()
    j = tuple(np.argwhere(~decided[1])[0])
    wrong[(1,) + j] = np.nextafter(wrong[(1,) + j], np.float32(np.inf))
    with pytest.raises(AssertionError):
        V.within_tolerance(wrong, c["dist"], c["geom"], c["agents"])


# ---- standing_rows ------------------------------------------------------------------------------------------------------------------
def test_standing_rows():
    size = [2.2, 0.9, 0.1]
    t = np.zeros((2, 4, 9))
    t[0, 0] = [1.0, 2.0, 0.3, 0.0, 0.0, 0.2] + size                 # stands (its yaw rate does not matter)
    t[0, 1] = [1.0, 2.0, 0.3, 0.5, 0.0, 0.0] + size                 # moves
    t[0, 2] = [1.0, 2.0, 0.3, 0.0, 0.5, 0.0] + size                 # stands now and is about to start: the speed stages'
    t[0, 3] = [1.0, 2.0, 0.3, 0.0, -1.0, 0.0] + size                # stands and brakes
    t[1, 0] = [1.0, math.nan, 0.3, 0.0, 0.0, 0.0] + size            # not finite: bad
    t[1, 1] = [1.0, 2.0, 0.3, math.inf, 0.0, 0.0] + size            # a speed that is no number: bad, though its pose is fine
    t[1, 2] = [math.nan, 2.0, 0.3, 0.0, 0.0, 0.0, -1.0, 0.9, 0.1]   # absent: the NaN is not read
    t[1, 3] = [1.0, 2.0, 0.3, 0.4, 0.0, 0.0] + size
    r = capi.standing_rows(t)
    assert r.shape == (2, 4, 6) and r.dtype == np.float64
    stand = [1.0, 2.0, 0.3] + size
    assert r[0, 0].tolist() == stand and r[0, 3].tolist() == stand
    assert r[0, 1].tolist() == r[0, 2].tolist() == r[1, 2].tolist() == r[1, 3].tolist() == list(V.ABSENT)
    for a in (0, 1):
        assert np.isnan(r[1, a, :3]).all() and r[1, a, 3:].tolist() == size
    f = V.frames(r)                                                  # and the overlay reads them so: bad stays bad, absent absent
    assert np.isnan(f[1, :2, 7]).all() and (f[0, 1:3, 7] == -1.0).all() and (f[0, [0, 3], 7] > 0).all()
    assert capi.standing_rows(t, v_still=0.45)[1, 3].tolist() == stand and capi.standing_rows(t, v_still=0.45)[0, 1].tolist() == list(V.ABSENT)
    assert capi.standing_rows(np.zeros((3, 0, 9))).shape == (3, 0, 6)
    with pytest.raises(ValueError):
        capi.standing_rows(np.zeros((2, 4, 6)))


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(hip_lib):
    for nm in NAMES + ("pqp_overlay_default_params",):
        assert nm in capi.EXPORTS and hasattr(hip_lib, nm), nm
    assert set(build_util.declared()) == set(capi.EXPORTS)
    fn = capi.HEADER.functions
    names = lambda f: [p.name for p in fn[f].params]
    assert names("pqp_overlay_agents_device") == ["h", "inflate", "n_maps", "geom", "dist", "n_scenes", "a_max", "agents", "a_of", "base_of", "frames",
                                                  "dist_out", "flags"]
    assert names("pqp_overlay_agents") == [n for n in names("pqp_overlay_agents_device") if n != "frames"]          # the host form: no frames
    types = {p.name: p.type for p in fn["pqp_overlay_agents_device"].params}
    assert types == dict(h="pqp_handle*", inflate="double", n_maps="int", geom="const pqp_grid_geometry*", dist="const float*", n_scenes="int",
                         a_max="int", agents="const double*", a_of="const int32_t*", base_of="const int32_t*", frames="double*", dist_out="float*",
                         flags="int32_t*")
    assert hip_lib.pqp_overlay_agents.argtypes[1] is C.c_double and len(hip_lib.pqp_overlay_agents_device.argtypes) == 13
    assert (capi.OVERLAY_BAD, capi.OVERLAY_NONE) == (1, 2) == (V.OVERLAY_BAD, V.OVERLAY_NONE)
    assert len(capi.HEADER.structs) == 10 and not any("overlay" in s for s in capi.STRUCTS)                 # no new struct
    assert list(inspect.signature(capi.Handle.overlay_agents).parameters) == ["self", "dist", "geom", "agents", "a_of", "base_of", "inflate"]
    for f in (capi.Handle.optimize_path, capi.Handle.optimize_path_on_grid):
        prm = inspect.signature(f).parameters
        assert prm["parked"].default is None
        assert list(prm)[-5:] == ["rank", "rank_params", "speed", "v_start", "v_end"] and list(prm)[-6] == "parked"
    raw = C.c_double(-1.0)
    hip_lib.pqp_overlay_default_params(C.byref(raw))
    assert raw.value == 0.0 == capi.overlay_default_params(hip_lib).inflate
    assert capi.overlay_default_params(hip_lib, inflate=0.25).inflate == 0.25
    hip_lib.pqp_overlay_default_params(None)


def test_refused_before_it_touches_a_device(hip_lib):
    """every refusal of the header through both forms; the handle is NULL throughout, so nothing can be launched and the arrays - host
    memory - come back untouched"""
    geom = V.geometry(4, 3, 0.5)
    dist, out = np.ones((2, 3, 4), np.float32), np.full((2, 3, 4), 7.0, np.float32)
    agents, frames, flags = np.zeros((2, 1, 6)), np.zeros((2, 1, 8)), np.full(2, 7, np.int32)
    good = dict(inflate=0.0, n_maps=2, geom=geom, dist=dist, n_scenes=2, a_max=1, agents=agents, a_of=None, base_of=None, frames=frames, dist_out=out,
                flags=flags)

    def bad_geom(**kw):
        g = V.geometry(4, 3, 0.5)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    refused = [dict(dist=None), dict(dist_out=None), dict(flags=None), dict(agents=None), dict(geom=None), dict(n_maps=0), dict(n_scenes=0),
               dict(a_max=-1), dict(geom=bad_geom(rows=1)), dict(geom=bad_geom(resolution=0.0)), dict(geom=bad_geom(resolution=math.nan)),
               dict(geom=bad_geom(length_x=math.inf)), dict(geom=bad_geom(length_y=math.nan)), dict(geom=bad_geom(pos_x=math.nan)),
               dict(geom=bad_geom(pos_y=-math.inf)), dict(geom=bad_geom(rows=1 << 15, cols=1 << 15)), dict(inflate=-0.1), dict(inflate=math.nan),
               dict(inflate=math.inf), dict(geom=bad_geom(rows=1 << 14, cols=1 << 14), n_scenes=(1 << 10) + 1, n_maps=1),
               dict(n_scenes=3), dict(dist_out=dist, base_of=np.zeros(2, np.int32)), dict(dist_out=dist, n_maps=1), dict({})]
    for over in refused:
        a = dict(good, **over)
        g = None if a["geom"] is None else C.byref(a["geom"])
        for name in NAMES:
            tail = (a["frames"],) if name.endswith("_device") else ()
            rc = getattr(hip_lib, name)(None, a["inflate"], a["n_maps"], g, a["dist"], a["n_scenes"], a["a_max"], a["agents"], a["a_of"], a["base_of"],
                                        *tail, a["dist_out"], a["flags"])
            assert rc == -1 == capi.ERR_INVALID, (over, name)
            assert hip_lib.pqp_last_error().decode().startswith("pqp_overlay_agents:"), (over, name)
    assert (out == 7.0).all() and (flags == 7).all() and (dist == 1.0).all()


def test_parked_in_the_chains_plan(hip_lib):
    import test_chain_plan as P
    import chain_plan_cases as cases
    geom = V.geometry(40, 30, 0.5)
    rows = np.zeros((3, 2, 6))
    base = cases.configs(hip_lib)["b"][1]
    plan = P.plan_of(hip_lib, dict(base, geom=geom, parked=(rows, [1, 0, 1], None), map_of=[0, 1, 2, 2]))
    want, on_device = P.expected("b")
    assert plan.result == want + [("parked_flags", (3,), "int32")] and plan.on_device == on_device          # the added key, behind the others
    assert plan.parked[0].shape == (3, 2, 6) and plan.parked[1].tolist() == [1, 0, 1] and plan.parked[2] == 0.0
    # the overlay is the first launch, and what it lays out under the name every later stage reads its layer by is the scenes' layers
    first = plan.stages[0]
    assert [o[0] for o in first.outputs] == ["parked_flags"]
    assert ("dist", (3, 30, 40), "float32", "empty") in first.scratch
    assert not any(name == "dist" for s in plan.stages[1:] for name, *_ in s.scratch + s.outputs + s.uploads)
    assert len(plan.stages) == len(P.plan_of(hip_lib, base).stages) + 1
    # a call without parked keeps its plan
    assert P.plan_of(hip_lib, dict(base, geom=geom)).result == want and P.plan_of(hip_lib, dict(base, geom=geom)).parked is None
    assert P.plan_of(hip_lib, dict(base, geom=geom, parked=(rows, None, 0.25))).parked[1:] == (None, 0.25)
    assert P.plan_of(hip_lib, dict(base, geom=geom, parked=(np.zeros((3, 0, 6)), None, None))).parked[0].shape == (3, 0, 6)
    for kw, text in ((dict(map_of=[0, 1, 2, 3]), r"map_of outside \[0, 3\)"), (dict(map_of=[0, -1, 2, 2]), r"map_of outside \[0, 3\)"),
                     (dict(parked=(rows, [0, 1], None)), "base_of"), (dict(parked=(rows, [0, -1, 0], None)), "base_of"),
                     (dict(parked=(rows[..., :5], None, None)), "agents must be"), (dict(parked=(rows[0], None, None)), "agents must be"),
                     (dict(parked=(rows, None, -1.0)), "inflate"), (dict(parked=(rows, None, math.nan)), "inflate"), (dict(parked=rows), "parked must be"),
                     (dict(geom=None), "geom")):
        with pytest.raises(ValueError, match=text):
            P.plan_of(hip_lib, dict(dict(base, geom=geom, parked=(rows, None, None)), **kw))


def test_overlay_builds_and_fails_cleanly_without_gpu(hip_lib, tmp_path):
    exe = cpp_demo.build("overlay_demo")
    import torch
    if torch.cuda.is_available():
        return
    c = V.seeded_scenes(1, 6, 5, 0.2, ("empty",), 1, 1)
    path = tmp_path / "case.bin"
    V.write_case(path, c["dist"], c["geom"], c["agents"], [0], 0.0)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "no overlay" in r.stderr


def test_the_kernel_uses_no_scratch_and_no_lds(kernels):
    r = build_util.find_kernel(kernels, "overlay_kernel")
    assert r["ScratchSize"] == 0, r
    assert r["LDS Size"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["Occupancy"] >= 4, r


def test_the_chains_scene_is_decided_well_away_from_the_last_digits():
    """the scene of tests/test_gpu_overlay_agents.py's chain test, on the CPU: the oracle's corridor bounds and path QP on the straight
    reference drive through the parked agent on the base layer (an overlap of 0.535 m) and clear it on the restated overlay (by 0.656 m) -
    both at least 0.1 m, so the device's outcome does not hang on the last digits of a solve"""
    without, with_overlay = V.parked_paths_on_the_cpu()
    assert without <= -0.1 and with_overlay >= 0.1
    assert abs(without + 0.535) < 5e-3 and abs(with_overlay - 0.656) < 5e-3
