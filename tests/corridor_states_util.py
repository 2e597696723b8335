"""Test helper: ReferencePathImpl::updateBoundsOnInputStates (reference src/data_struct/reference_path_impl.cpp:118-175) restated in
float64 from the corridor oracle's pieces, in the reference's expression order - the checker of pqp_corridor_bounds_on_states."""
import math

import numpy as np

import corridor_oracle as K


def _cos(v):
    # std::cos of a value that is not finite is NaN; math.cos raises for an infinity
    return math.cos(v) if math.isfinite(v) else math.nan


def update_bounds_on_input_states(ref, d_heading, sx, sy, dist, g, prm=K.CorridorParams()):
    """ref [n][5] = (s, k, heading, x, y) of the reference states, d_heading [k <= n] of the input states.  Returns (bounds [n_valid][6]
    in the ABI order f_lb f_ub r_lb r_ub c_lb c_ub, n_valid, blocked row or None), as K.update_bounds_improved does for updateBoundsImproved."""
    assert len(d_heading) <= len(ref)                 # CHECK_LE (:119)
    out = []
    blocked = None
    for i in range(len(d_heading)):
        s, _, heading, x, y = (float(v) for v in ref[i])
        dpsi = float(d_heading[i])
        front_length_new = prm.front_length - prm.front_length * _cos(dpsi)
        rear_length_new = prm.rear_length - prm.rear_length * _cos(dpsi)
        fcx = x + front_length_new * math.cos(heading)
        fcy = y + front_length_new * math.sin(heading)
        rcx = x + rear_length_new * math.cos(heading)
        rcy = y + rear_length_new * math.sin(heading)
        # the Newton guess keeps the flag's length (:139-150)
        fpx, fpy, _ = K.directional_projection_newton(sx, sy, fcx, fcy, heading + math.pi / 2, s + prm.projection_window, s + prm.front_length)
        rpx, rpy, _ = K.directional_projection_newton(sx, sy, rcx, rcy, heading + math.pi / 2, s + prm.projection_window, s + prm.rear_length)
        f_ub, f_lb = K.clearance_strict(fpx, fpy, heading, dist, g, prm)
        off = K.global2local_y(fcx, fcy, heading, fpx, fpy)
        f_ub += off; f_lb += off
        r_ub, r_lb = K.clearance_strict(rpx, rpy, heading, dist, g, prm)
        off = K.global2local_y(rcx, rcy, heading, rpx, rpy)
        r_ub += off; r_lb += off
        c_ub, c_lb = K.clearance_strict(x, y, heading, dist, g, prm)
        row = [f_lb, f_ub, r_lb, r_ub, c_lb, c_ub]
        if abs(f_ub - f_lb) < prm.epsilon or abs(r_ub - r_lb) < prm.epsilon:
            blocked = row
            break
        out.append(row)
    return np.array(out).reshape(-1, 6), len(out), blocked


def straight_scene(length=40.0, left=3.0, right=-2.5, wall_x=None, resolution=0.1):
    """A straight reference line along +x from (0, 0), walls at y = left and y = right, optionally a wall across the road at x = wall_x:
    (ref [n][5] at 0.5 m spacing, sx, sy, dist [rows][cols] float32, GridGeom).  The map covers [-10, 50] x [-10, 10]."""
    g = K.GridGeom.make(60.0, 20.0, resolution, pos=(20.0, 0.0))
    dist = np.zeros((g.rows, g.cols), dtype=np.float32)
    for ix in range(g.rows):
        for iy in range(g.cols):
            px, py = K.grid_cell_position(g, ix, iy)
            d = min(abs(py - left), abs(py - right))
            if wall_x is not None:
                d = min(d, abs(px - wall_x))
            dist[ix, iy] = np.float32(max(d, 0.0))
    ks = np.linspace(0.0, length + 10.0, 13)
    sx = K.spline_fit(ks, ks.copy())
    sy = K.spline_fit(ks, np.zeros_like(ks))
    s = np.arange(0.0, length, 0.5)
    ref = np.stack([s, np.zeros_like(s), np.zeros_like(s), s, np.zeros_like(s)], axis=1)
    return ref, sx, sy, dist, g
