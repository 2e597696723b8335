"""The look fused into a polish solve (PathQp::iterate(true) + look_after_solve()) against residuals(), on the host emulation of pqp_path_lane.hpp.
The emulation's context has kDpp = false, so this is the fused form with LDS neighbours.  tests/emu/look_emu.cpp arms run()'s look hook: after EVERY
polish solve it calls residuals() on the same state and compares bit for bit - the six values of a full look, and the lazy look's four against the
corresponding four of the six.  Bit equality is the bar: the per-lane arithmetic is one helper for both, and a maximum does not depend on order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_util as EU
from path_optimizer_2_amd.synth import make_batch

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "look_emu.cpp")
LIB = os.path.join(HERE, "emu", "liblook_emu.so")
_lib = None


def _load():
    global _lib
    if _lib is None:
        deps = [SRC] + EU._DEPS
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC], check=True)
        _lib = C.CDLL(LIB)
    return _lib


def _solve_checked(prm, b, n_of=None, wave_order=1):
    """-> (result, looks[2], mismatches[2], first mismatch) of one batch through the hooked emulation"""
    lib = _load()
    B, n = b["ref"].shape[0], b["ref"].shape[1]
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ref, bounds, scal = (np.ascontiguousarray(b[k]) for k in ("ref", "bounds", "scal"))
    n_of_c = None if n_of is None else np.ascontiguousarray(n_of, dtype=np.int32)
    out = np.zeros((B, n, 7)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32); info = np.zeros((B, 8))
    wx = np.zeros((B, n, 6)); wy = np.zeros((B, n, 6)); wye = np.zeros((B, 2)); wrho = np.zeros(B)
    looks = (C.c_longlong * 2)(); bad = (C.c_longlong * 2)(); first = (C.c_double * 12)()
    lib.pqp_emu_look_counts(looks, bad, first, 1)
    lib.pqp_emu_set_wave_order(wave_order)
    lib.pqp_emu_set_counts(vp(n_of_c))
    lib.pqp_emu_path_solve(C.byref(prm), B, n, vp(ref), None, vp(bounds), vp(scal), 1, 0, vp(out), vp(st), vp(it), vp(info), vp(wx), vp(wy), vp(wye), vp(wrho))
    lib.pqp_emu_set_counts(None)
    lib.pqp_emu_set_wave_order(1)
    lib.pqp_emu_look_counts(looks, bad, first, 1)
    return dict(out=out, status=st, info=info), list(looks), list(bad), list(first)


CASES = [(17, "uniform", 48, False), (64, "uniform", 48, False), (80, "uniform", 64, False), (80, "varied", 48, False), (120, "varied", 48, False),
         (200, "uniform", 32, False), (80, "uniform", 32, True)]


@pytest.mark.parametrize("n,profile,batch,rough", CASES)
def test_fused_look_equals_residuals_bit_for_bit(n, profile, batch, rough):
    b = make_batch(batch, n, profile, seed=71 + n)
    over = dict(rough_constraints_far_away=1, precise_planning_length=10.0) if rough else {}
    prm = EU.production(**over)
    n_of = None
    if n >= 64 and not rough:          # ragged counts too: the last real lane away from a row's / a wavefront's end, and on it
        n_of = np.full(batch, n, dtype=np.int32)
        n_of[::5] = n - 13; n_of[1::7] = 65 if n > 65 else 33; n_of[2::9] = 64 if n >= 64 else n
        b["scal"][n_of < n, 4] = 1.0
    for order in (1, 0):
        r, looks, bad, first = _solve_checked(prm, b, n_of, wave_order=order)
        print(f"n {n} {profile} rough {rough} wave order {order}: lazy looks {looks[0]} (mismatches {bad[0]}), full looks {looks[1]} (mismatches {bad[1]}), "
              f"solved {(r['status'] == 1).sum()} of {batch}")
        assert looks[0] > batch // 2 and looks[1] > batch // 2, looks          # both kinds of look really ran
        assert bad == [0, 0], (bad, first[:6], first[6:])
        assert (r["status"] == 1).mean() > 0.9
    # the hook changes nothing: the plain emulation gives the same records
    plain = EU.solve(EU.production(**over), b["ref"], b["bounds"], b["scal"], n_of=n_of)
    assert (plain["status"] == r["status"]).all() and (plain["info"] == r["info"]).all() and (plain["out"] == r["out"]).all()
