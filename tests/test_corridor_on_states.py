"""updateBoundsOnInputStates (reference_path_impl.cpp:118-175) on the CPU: the float64 restatement in tests/corridor_states_util.py on
hand-made scenes whose answer is known, and the host-side parts of the C ABI that need no GPU (argument checks, the chain's default)."""
import ctypes as C
import math

import numpy as np
import pytest

import corridor_oracle as K
import corridor_states_util as S
from path_optimizer_2_amd import capi


@pytest.fixture(scope="module")
def straight():
    return S.straight_scene()


def test_zero_heading_error_puts_both_circles_on_the_state(straight):
    """d_heading = 0: front_length_new = rear_length_new = 0, so the front and rear centres are the reference state itself and their
    projection on the line is the state again: each front and rear interval is the waypoint's centre interval"""
    ref, sx, sy, dist, g = straight
    rows, n_valid, blocked = S.update_bounds_on_input_states(ref, np.zeros(len(ref)), sx, sy, dist, g)
    assert n_valid == len(ref) and blocked is None
    np.testing.assert_allclose(rows[:, 0:2], rows[:, 4:6], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rows[:, 2:4], rows[:, 4:6], rtol=0, atol=1e-9)
    # walls at +3 and -2.5: the strict clearance walk, 1 m car width, 0.3 m margin
    for i in (0, 10, len(ref) - 1):
        lb, ub = rows[i, 4], rows[i, 5]
        assert (ub, lb) == K.clearance_strict(ref[i, 3], ref[i, 4], ref[i, 2], dist, g)
        assert 1.5 < ub < 2.5 and -2.0 < lb < -1.0


def test_heading_error_moves_the_circles_along_the_line(straight):
    """on a straight line the centres stay on it: the front one moves L (1 - cos dpsi) ahead, the rear one behind; where the walls are
    parallel to the line the intervals do not change, the offset of the projection is zero"""
    ref, sx, sy, dist, g = straight
    dpsi = np.full(len(ref), 0.4)
    rows, n_valid, _ = S.update_bounds_on_input_states(ref, dpsi, sx, sy, dist, g)
    base, _, _ = S.update_bounds_on_input_states(ref, np.zeros(len(ref)), sx, sy, dist, g)
    assert n_valid == len(ref)
    np.testing.assert_allclose(rows, base, rtol=0, atol=1e-9)
    # ... and against updateBoundsImproved (centres at the full lengths): the same intervals on this road, other centres
    imp, nv_imp, _ = K.update_bounds_improved(ref, sx, sy, dist, g)
    assert nv_imp == n_valid
    np.testing.assert_allclose(rows[:, 4:6], imp[:, 4:6], rtol=0, atol=0)


def test_a_wall_across_the_road_truncates_at_the_first_blocked_waypoint():
    ref, sx, sy, dist, g = S.straight_scene(wall_x=12.2)
    dpsi = np.zeros(len(ref))
    rows, n_valid, blocked = S.update_bounds_on_input_states(ref, dpsi, sx, sy, dist, g)
    # at dpsi = 0 the probes sit on the states: the first state closer than 0.5 m to the wall has no clearance (both bounds 0)
    first = int(np.argmax(np.abs(ref[:, 3] - 12.2) < 0.5))
    assert n_valid == first == 24 and blocked is not None
    assert blocked[0] == blocked[1] == 0.0 and len(rows) == n_valid
    # with a heading error the front circle moves ahead and reaches the wall earlier
    rows2, n_valid2, _ = S.update_bounds_on_input_states(ref, np.full(len(ref), 0.9), sx, sy, dist, g)
    assert n_valid2 < n_valid
    # fewer input states than reference states: the loop runs over the states (CHECK_LE), the walls never reached
    rows3, n_valid3, blocked3 = S.update_bounds_on_input_states(ref, dpsi[:10], sx, sy, dist, g)
    assert n_valid3 == 10 and blocked3 is None
    np.testing.assert_array_equal(rows3, rows[:10])
    with pytest.raises(AssertionError):
        S.update_bounds_on_input_states(ref, np.zeros(len(ref) + 1), sx, sy, dist, g)


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_heading_error_that_is_not_finite_gives_nan_rows_and_no_exception(straight, bad):
    ref, sx, sy, dist, g = straight
    dpsi = np.zeros(len(ref))
    dpsi[7] = bad
    rows, n_valid, blocked = S.update_bounds_on_input_states(ref, dpsi, sx, sy, dist, g)
    base, _, _ = S.update_bounds_on_input_states(ref, np.zeros(len(ref)), sx, sy, dist, g)
    assert n_valid == len(ref) and blocked is None          # NaN intervals are not "equal": never blocked
    assert np.isnan(rows[7, :4]).all() and np.isfinite(rows[7, 4:]).all()
    mask = np.ones(len(ref), dtype=bool)
    mask[7] = False
    np.testing.assert_array_equal(rows[mask], base[mask])


def test_chain_config_default_and_layout():
    """pqp_chain_default_config (pure host): the re-linearised second pass, as optimizePath runs today; the field sits at the end"""
    lib = capi.load_library(with_torch=False)
    c = capi.PqpChainConfig()
    c.second_pass = 7
    lib.pqp_chain_default_config(C.byref(c))
    assert c.second_pass == capi.SECOND_PASS_RELINEARISE == 0 and capi.SECOND_PASS_BOUNDS_ON_STATES == 1
    assert capi.PqpChainConfig._fields_[-1][0] == "second_pass"
    assert capi.PqpChainConfig.second_pass.offset == C.sizeof(capi.PqpChainConfig) - 4


def test_entry_points_refuse_a_null_handle_without_a_device():
    lib = capi.load_library(with_torch=False)
    g = capi.PqpGridGeometry(4, 4, 0.5, 2.0, 2.0, 0.0, 0.0)
    prm = capi.PqpCorridorParams()
    lib.pqp_corridor_default_params(C.byref(prm))
    for name in ("pqp_corridor_bounds_on_states_device",):
        assert getattr(lib, name)(None, 1, 4, 4, None, None, None, 7, None, None, None, None, C.byref(g), C.byref(prm), None, None) == -1
    assert lib.pqp_corridor_bounds_on_states(None, 1, 4, 4, None, None, None, 7, None, None, None, 1, None, C.byref(g), C.byref(prm), None, None) == -1
