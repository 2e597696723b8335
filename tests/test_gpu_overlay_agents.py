"""pqp_overlay_agents on the device against the numpy restatement (tests/overlay_util.py).

The tolerance rule: the device's sincos and numpy's may differ in the last place, so a cell an agent decides need not round to the same
float.  With d the restatement's double of the cell, the device's value lies in [fl32(d - 1e-9), fl32(d + 1e-9)] after the same minimum
with the base - 1e-9 m is the bound tests/test_gpu_agents_check.py holds this expression to with coordinates within +-1000 m, and every
coordinate here is far inside that.  No cell is left out; cells the base decides, scenes without agents and scenes with a bad agent
are bit for bit, and with every heading exactly 0 the whole layer is."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import cpp_demo
import overlay_util as V
from device_form import call, to_device
from path_optimizer_2_amd import capi
from shared_util import same_bytes

pytestmark = pytest.mark.gpu

ROWS = (2, 63, 64, 65, 130)
COLS = (2, V.TILE_COLS - 1, V.TILE_COLS, V.TILE_COLS + 1, 37)
KINDS = (("empty", "dense"), ("dense", "blocked"), ("nan", "empty"), ("blocked", "nan"), ("dense", "empty"))


@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(capi.production_params(), max_batch=4, max_n=128)
    yield h
    h.close()


@pytest.fixture(scope="module")
def chain_handles():
    import chain_util
    h, hs = chain_util.handles(2)
    yield h, hs
    h.close()
    hs.close()


def _case(rows, cols, a_max=5, exact_heading=False):
    """two base layers, three scenes on them, pos != 0, resolution 0.2 or 0.3 by the shape"""
    k = ROWS.index(rows) + COLS.index(cols)
    res = (0.2, 0.3)[k % 2]
    c = V.seeded_scenes(1000 * rows + cols, rows, cols, res, KINDS[k % len(KINDS)], 3, a_max, pos=(12.5, -7.25), exact_heading=exact_heading)
    c.update(base_of=np.array([1, 0, 1], np.int32), a_of=np.array([a_max, max(a_max - 2, 0), a_max], np.int32))
    return c


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_every_shape_against_the_restatement(handle, rows, cols):
    """n_maps = 2, n_scenes = 3, base_of = [1, 0, 1], five agents a scene - in the map, across its border, outside it, a disc, a point,
    absent rows - one a_of below a_max, on every pair of base layers"""
    c = _case(rows, cols)
    got, flags = handle.overlay_agents(c["dist"], c["geom"], c["agents"], a_of=c["a_of"], base_of=c["base_of"])
    want, want_flags, _ = V.overlay(c["dist"], c["geom"], c["agents"], c["a_of"], c["base_of"])
    assert flags.tolist() == want_flags.tolist() == [0, 0, 0]
    decided = V.within_tolerance(got, c["dist"], c["geom"], c["agents"], c["a_of"], c["base_of"])
    if "empty" in KINDS[(ROWS.index(rows) + COLS.index(cols)) % len(KINDS)]:
        assert decided >= rows * cols                        # on the layer without obstacle the agents decide every cell: nothing was skipped


@pytest.mark.parametrize("rows,cols", [(65, 9), (130, 37), (2, 2)])
def test_headings_of_exactly_zero_are_bit_for_bit(handle, rows, cols):
    c = _case(rows, cols, exact_heading=True)
    for inflate in (0.0, 0.35):
        got, flags = handle.overlay_agents(c["dist"], c["geom"], c["agents"], a_of=c["a_of"], base_of=c["base_of"], inflate=inflate)
        want, want_flags, decided = V.overlay(c["dist"], c["geom"], c["agents"], c["a_of"], c["base_of"], inflate)
        assert same_bytes(got, want) and flags.tolist() == want_flags.tolist() and decided.any()


@pytest.mark.parametrize("a_max", [0, 1, 5])
def test_agent_counts_one_base_layer_and_no_base_of(handle, a_max):
    """a_max in {0, 1, 5}; base_of = NULL with n_maps = 1: every scene starts from layer 0"""
    c = _case(65, 9, a_max=a_max)
    dist = c["dist"][:1]
    got, flags = handle.overlay_agents(dist, c["geom"], c["agents"], a_of=c["a_of"])
    want, want_flags, _ = V.overlay(dist, c["geom"], c["agents"], c["a_of"])
    assert flags.tolist() == want_flags.tolist()
    assert flags.tolist() == ([V.OVERLAY_NONE] * 3 if a_max == 0 else [0, V.OVERLAY_NONE, 0] if a_max == 1 else [0, 0, 0])
    V.within_tolerance(got, dist, c["geom"], c["agents"], c["a_of"])
    for s in np.nonzero(flags == V.OVERLAY_NONE)[0]:
        assert same_bytes(got[s], dist[0])


def test_a_bad_row_closes_its_scene_and_leaves_the_neighbours(handle):
    c = _case(130, 9)
    clean, _ = handle.overlay_agents(c["dist"], c["geom"], c["agents"], base_of=c["base_of"])
    for bad_row in ([1.0, math.nan, 0.0, 1.0, 1.0, 0.0], [1.0, 2.0, 0.0, 1.0, 1.0, -0.5], [math.inf, 2.0, 0.0, 0.0, 0.0, 0.0]):
        ag = c["agents"].copy()
        ag[1, 4] = bad_row                                   # the last row: every skip and every good agent stands in front of it
        got, flags = handle.overlay_agents(c["dist"], c["geom"], ag, base_of=c["base_of"])
        assert flags.tolist() == [0, V.OVERLAY_BAD, 0]
        assert same_bytes(got[1], np.zeros_like(got[1])) and same_bytes(got[0], clean[0]) and same_bytes(got[2], clean[2])
        got, flags = handle.overlay_agents(c["dist"], c["geom"], ag, a_of=[5, 4, 5], base_of=c["base_of"])          # behind the count: not there
        assert flags.tolist() == [0, 0, 0] and same_bytes(got[0], clean[0])


def test_the_same_scene_elsewhere_in_a_larger_batch_has_the_same_bits(handle):
    c = _case(130, 37)
    got, _ = handle.overlay_agents(c["dist"], c["geom"], c["agents"], a_of=c["a_of"], base_of=c["base_of"])
    order = [2, 0, 1, 1, 2, 0, 0]
    big, flags = handle.overlay_agents(c["dist"], c["geom"], c["agents"][order], a_of=c["a_of"][order], base_of=c["base_of"][order])
    for k, s in enumerate(order):
        assert same_bytes(big[k], got[s]), (k, s)
    assert flags.tolist() == [0] * 7


def _device_form(h, c, dist_t, out_t, base_of=True, guard=0):
    """pqp_overlay_agents_device on torch buffers; -> (layers as the device has them [n_scenes][cols][rows], flags, frames)"""
    import torch
    n_scenes, a_max = c["agents"].shape[:2]
    frames = torch.full((n_scenes, a_max, 8), -7.0, dtype=torch.float64, device=dist_t.device)
    flags = torch.full((n_scenes,), -7, dtype=torch.int32, device=dist_t.device)
    rc = call(h, "pqp_overlay_agents_device", 0.0, dist_t.shape[0], C.byref(c["geom"]), dist_t, n_scenes, a_max, to_device(c["agents"]),
              to_device(c["a_of"], np.int32), to_device(c["base_of"], np.int32) if base_of else None, frames, out_t, flags)
    assert rc == 0, h.lib.pqp_last_error()
    return out_t.cpu().numpy(), flags.cpu().numpy(), frames.cpu().numpy()


def test_the_device_form_gives_the_host_forms_bits_and_writes_nothing_else(handle):
    import torch
    c = _case(65, 9)
    host, host_flags = handle.overlay_agents(c["dist"], c["geom"], c["agents"], a_of=c["a_of"], base_of=c["base_of"])
    dist_t = to_device(capi._column_major(c["dist"], np.float32), np.float32)
    cells = 65 * 9
    out_t = torch.full((3 * cells + 512,), -7.0, dtype=torch.float32, device=dist_t.device)
    got, flags, frames = _device_form(handle, c, dist_t, out_t)
    assert (got[3 * cells:] == -7.0).all()                   # nothing behind the scenes' layers
    assert same_bytes(np.transpose(got[:3 * cells].reshape(3, 9, 65), (0, 2, 1)), host) and flags.tolist() == host_flags.tolist()
    # the frames are fully written, and they are pqp_agents_check's: everything but the sincos bit for bit
    want = V.frames(c["agents"])
    assert same_bytes(frames[..., [0, 1, 4, 5, 6, 7]], want[..., [0, 1, 4, 5, 6, 7]]) and np.abs(frames[..., 2:4] - want[..., 2:4]).max() <= 1e-15


def test_in_place_with_one_layer_a_scene(handle):
    """dist_out = dist with base_of = NULL and n_scenes = n_maps: every scene overlays its own layer where it lies; and every other
    aliasing is refused with the outputs untouched"""
    import torch
    c = _case(130, 9)
    dist = np.stack([c["dist"][0], c["dist"][1], c["dist"][0]])
    host, host_flags = handle.overlay_agents(dist, c["geom"], c["agents"], a_of=c["a_of"])
    want, _, _ = V.overlay(dist, c["geom"], c["agents"], c["a_of"])
    V.within_tolerance(host, dist, c["geom"], c["agents"], c["a_of"])
    dist_t = to_device(capi._column_major(dist, np.float32), np.float32)
    got, flags, _ = _device_form(handle, c, dist_t, dist_t, base_of=False)
    assert same_bytes(np.transpose(got, (0, 2, 1)), host) and flags.tolist() == host_flags.tolist()
    before = dist_t.clone()
    flags_t = torch.full((3,), -7, dtype=torch.int32, device=dist_t.device)
    frames = torch.zeros((3, 5, 8), dtype=torch.float64, device=dist_t.device)
    rc = call(handle, "pqp_overlay_agents_device", 0.0, 3, C.byref(c["geom"]), dist_t, 3, 5, to_device(c["agents"]), None,
              to_device(np.arange(3), np.int32), frames, dist_t, flags_t)
    assert rc == capi.ERR_INVALID and handle.lib.pqp_last_error().decode().startswith("pqp_overlay_agents:")
    assert torch.equal(dist_t.view(torch.int32), before.view(torch.int32)) and (flags_t == -7).all()          # (bits: the layer has NaN cells)
    # the host form: base_of outside [0, n_maps) is refused
    with pytest.raises(capi.PqpError, match="base_of outside"):
        handle.overlay_agents(dist, c["geom"], c["agents"], base_of=[0, 3, 1])


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def _plan(h, hs, sc, **kw):
    import distance_util
    grid = distance_util.occupancy_of(sc["dist"])            # no obstacle: the layer built on the device has no zero either
    return h.optimize_path_on_grid(sc["pts"], sc["n_pts"], sc["start"], sc["target"], grid, sc["geom"], smoother=hs, **kw)


def test_the_path_goes_round_a_parked_agent(chain_handles):
    """One straight, obstacle-free scenario and a parked rectangle whose near side is 0.7 m beside the line (overlay_util.parked_scene).
    Without parked= the chain drives the line and pqp_agents_check (margin 0, on `out` with stride 7 and n_out) reports a hit; with
    parked= the path is solved and the check reports none.
    Chosen on the CPU first (overlay_util.parked_paths_on_the_cpu: the oracle's corridor bounds and path QP on the straight reference,
    without the smoothers and the DP search): the footprint's clearance to the agent is -0.535 m without the overlay - an overlap of
    0.535 m - and +0.656 m with it, both beyond the 0.1 m that keeps the outcome off the last digits of a solve."""
    h, hs = chain_handles
    sc = V.parked_scene()
    res = {}
    for name, kw in (("without", {}), ("with", dict(parked=(sc["agents"], None, None)))):
        r = _plan(h, hs, sc, **kw)
        assert r["status"].tolist() == [1] and r["stage"].tolist() == [0], (name, r["status"], r["stage"])
        n = int(r["n_out"][0])
        hit = h.agents_check(r["out"][:, :, :], sc["agents"][:, :, None, :].repeat(r["out"].shape[1], axis=2), m_of=r["n_out"])
        res[name] = (int(hit["first_hit"][0]), n, V.path_clearance(r["out"][0], n, V.PARKED_AGENT), r)
        print(f"{name} parked=: first_hit {res[name][0]} of n_out {n}, clearance {res[name][2]:+.3f} m")
    assert res["without"][0] < res["without"][1] and res["without"][2] <= -0.1
    assert res["with"][0] == res["with"][1] and res["with"][2] >= 0.1
    assert res["with"][3]["parked_flags"].tolist() == [0] and "parked_flags" not in res["without"][3]
    assert list(res["with"][3])[:-1] == list(res["without"][3])


def test_the_chains_footprint_check_reads_the_scenes_layers(chain_handles):
    """check_footprint=True under parked= against pqp_footprint_check on the scenes' layers from overlay_agents: two scenes on one grid,
    the parked agent in the first, a much larger one across the line in the second"""
    import distance_util
    h, hs = chain_handles
    sc = V.parked_scene()
    two = lambda a: np.concatenate([a, a])
    agents = np.array([[V.PARKED_AGENT], [(-8.0, 0.0, 0.3, 2.2, 0.9, 0.2)]])
    grid = distance_util.occupancy_of(sc["dist"])
    r = h.optimize_path_on_grid(two(sc["pts"]), two(sc["n_pts"]), two(sc["start"]), two(sc["target"]), grid, sc["geom"], smoother=hs,
                                map_of=np.array([0, 1], np.int32), check_footprint=True, parked=(agents, np.zeros(2, np.int32), None))
    base = h.distance_layer(grid, sc["geom"])
    layers, flags = h.overlay_agents(base, sc["geom"], agents, base_of=[0, 0])
    assert flags.tolist() == r["parked_flags"].tolist() == [0, 0]
    fp = h.footprint_check(r["out"], r["n_out"], layers, sc["geom"], map_of=[0, 1], margin=True)
    on_path = np.arange(r["out"].shape[1])[None, :] < r["n_out"][:, None]
    assert np.array_equal(fp["first_collision"], r["first_collision"])
    assert np.array_equal(fp["free"][on_path], r["free"][on_path]) and same_bytes(fp["margin"][on_path], r["margin"][on_path])
    assert r["status"][0] == 1 and r["first_collision"][0] == r["n_out"][0]
    # the scenes differ: the second's road is closed by the agent across it, or its path leaves the line further than the first's
    assert r["stage"][1] != 0 or np.abs(r["out"][1, :r["n_out"][1], 1]).max() > np.abs(r["out"][0, :r["n_out"][0], 1]).max()
    with pytest.raises(ValueError, match="map_of outside"):
        h.optimize_path_on_grid(two(sc["pts"]), two(sc["n_pts"]), two(sc["start"]), two(sc["target"]), grid, sc["geom"], smoother=hs,
                                map_of=np.array([0, 2], np.int32), parked=(agents, np.zeros(2, np.int32), None))
    with pytest.raises(ValueError, match="base_of outside"):
        h.optimize_path_on_grid(two(sc["pts"]), two(sc["n_pts"]), two(sc["start"]), two(sc["target"]), grid, sc["geom"], smoother=hs,
                                map_of=np.array([0, 1], np.int32), parked=(agents, np.array([0, 1], np.int32), None))


def test_the_cpp_overlay_gives_the_wrappers_bits(handle, tmp_path):
    exe = cpp_demo.build("overlay_demo")
    c = _case(65, 9)
    want, want_flags = handle.overlay_agents(c["dist"], c["geom"], c["agents"], base_of=c["base_of"], inflate=0.125)
    path = tmp_path / "case.bin"
    V.write_case(path, c["dist"], c["geom"], c["agents"], c["base_of"], 0.125)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    cells = 65 * 9
    for s in range(3):
        head = lines[s * (cells + 1)].split()
        assert head == ["scene", str(s), str(int(want_flags[s]))]
        bits = np.array([int(v, 16) for v in lines[s * (cells + 1) + 1:(s + 1) * (cells + 1)]], np.uint32)
        assert np.array_equal(bits.reshape(9, 65).T, want[s].view(np.uint32))
