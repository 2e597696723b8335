"""pqp_distance_layer without a GPU: the restatement (tests/distance_util.py) against the definition, the host build of the kernels'
per-line routines (tests/emu/edt_emu.cpp) against the restatement bit for bit, the edge cases of the integer and float arithmetic
against closed forms, and the library's symbols and register budget."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import distance_util as D
import edt_emu_util as E
from path_optimizer_2_amd import capi


@pytest.fixture(scope="module")
def small_maps():
    return D.random_maps(np.random.default_rng(2024))


def test_restatement_is_the_definition(small_maps):
    for g in small_maps:
        assert np.array_equal(D.d2_exact(g), D.d2_brute(g)), g.shape


def test_host_build_equals_the_restatement(small_maps):
    for g in small_maps:
        for res in (0.2, 0.05, 1.0):
            got, want = E.distance_layer(g, res), D.distance_layer(g, res)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (g.shape, res)


def test_host_build_several_maps_in_one_call(small_maps):
    rng = np.random.default_rng(3)
    maps = np.stack([np.where(rng.uniform(size=(23, 31)) < d, 0, 255).astype(np.uint8) for d in (0.0, 0.01, 0.3, 0.9, 1.0)])
    got = E.distance_layer(maps, 0.2)
    for k in range(len(maps)):
        assert np.array_equal(got[k].view(np.int32), E.distance_layer(maps[k], 0.2).view(np.int32))
        assert np.array_equal(got[k].view(np.int32), D.distance_layer(maps[k], 0.2).view(np.int32))


def test_host_build_on_the_reference_map():
    g, res = D.reference_map()
    assert g.shape == (701, 710)
    want = D.distance_layer(g, res)
    assert np.array_equal(E.distance_layer(g, res).view(np.int32), want.view(np.int32))
    assert want.max() == np.float32(np.float32(77.0) * np.float32(0.2))        # 77 cells, 15.4 m


def test_no_obstacle_gets_the_diagonal():
    for rows, cols in ((2, 2), (7, 3), (40, 37)):
        got = E.distance_layer(np.full((rows, cols), 255, np.uint8), 0.2)
        want = np.float32(np.sqrt(np.float64(rows * rows + cols * cols))) * np.float32(0.2)
        assert (got.view(np.int32) == want.view(np.int32)).all()


def test_squared_distances_beyond_2_31_take_64_bits():
    """60 000 x 3, obstacles on the first row only: d2 = r^2 reaches 3.6e9"""
    rows, cols = 60000, 3
    assert E.wide(rows, cols) and not E.wide(701, 710)
    g = np.full((rows, cols), 255, np.uint8)
    g[0, :] = 0
    got = E.distance_layer(g, 0.2)
    r = np.arange(rows, dtype=np.float32)[:, None]
    want = np.broadcast_to(r * np.float32(0.2), (rows, cols))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_squared_distances_beyond_2_24_round_like_float():
    """5000 x 8, one obstacle in a corner: d2 = r^2 + c^2 up to 2.5e7, where a float no longer holds every integer"""
    rows, cols = 5000, 8
    g = np.full((rows, cols), 255, np.uint8)
    g[0, 0] = 0
    got = E.distance_layer(g, 0.2)
    r, c = np.indices((rows, cols))
    want = np.sqrt((r * r + c * c).astype(np.float64)).astype(np.float32) * np.float32(0.2)
    assert (r * r + c * c).max() > 2 ** 24
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def _sqrt_rn_exact(d2):
    """the float nearest to sqrt(d2), ties to even, by exact comparison with the midpoints"""
    f = np.float32(np.sqrt(np.float64(d2)))
    for _ in range(3):
        up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(0))
        hi, lo = (Fraction(float(f)) + Fraction(float(up))) / 2, (Fraction(float(f)) + Fraction(float(dn))) / 2
        odd = int(f.view(np.int32)) & 1
        if d2 > hi * hi or (d2 == hi * hi and odd):
            f = up
        elif d2 < lo * lo or (d2 == lo * lo and odd):
            f = dn
        else:
            return f
    raise AssertionError(d2)


def test_sqrt_is_correctly_rounded_up_to_2_60():
    rng = np.random.default_rng(7)
    cases = [int(x) for x in rng.integers(1, 2 ** 60, size=3000)] + [int(x) for x in rng.integers(1, 2 ** 52, size=1000)]
    for m in [int(x) for x in rng.integers(2 ** 25, 2 ** 30, size=500)]:          # squares of float midpoints and their neighbours
        f = np.float32(m)
        mid = (int(f) + int(np.nextafter(f, np.float32(np.inf)))) // 2
        cases += [mid * mid - 1, mid * mid, mid * mid + 1]
    for d2 in cases:
        assert E.sqrt_rn(d2).view(np.int32) == _sqrt_rn_exact(d2).view(np.int32), d2


def test_symbols_are_exported(hip_lib):
    for name in ("pqp_distance_layer", "pqp_distance_layer_device"):
        assert name in capi.EXPORTS and hasattr(hip_lib, name)


def test_distance_kernels_use_no_scratch(hip_lib):
    import __graft_entry__ as g
    kernels, cur = {}, None
    for line in open(g.RESOURCES):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[\w/]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    found = {k: v for k, v in kernels.items() if "distance_lines_kernel" in k or "distance_envelope_kernel" in k}
    assert len(found) == 3, list(found)           # phase A + phase B in 32- and 64-bit arithmetic
    for k, v in found.items():
        assert v["ScratchSize"] == 0, (k, v)


def test_bool_grids_are_refused():
    h = capi.Handle.__new__(capi.Handle)          # the check comes before any library call
    with pytest.raises(TypeError):
        capi.Handle.distance_layer(h, np.ones((4, 4), dtype=bool), None)
