"""Build + drive tests/emu/libedt_emu.so: the per-line routines of pqp_distance_layer (csrc/pqp_distance_layer.hpp) compiled for the host
(test infrastructure)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu", "edt_emu.cpp")
LIB = os.path.join(HERE, "emu", "libedt_emu.so")
_DEPS = [SRC, os.path.join(ROOT, "path_optimizer_2_amd", "csrc", "pqp_distance_layer.hpp")]
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in _DEPS):
            subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC], check=True)
        lib = C.CDLL(LIB)
        lib.pqp_emu_distance_layer.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.pqp_emu_distance_wide.argtypes = [C.c_int, C.c_int]
        lib.pqp_emu_sqrt_rn.argtypes = [C.c_uint64]
        lib.pqp_emu_sqrt_rn.restype = C.c_float
        _lib = lib
    return _lib


def distance_layer(grid, resolution):
    """grid [n_maps][rows][cols] (or 2-D) uint8, 0 = obstacle, numpy orientation -> float32 layer in the same orientation"""
    g = np.asarray(grid, dtype=np.uint8)
    two_d = g.ndim == 2
    if two_d:
        g = g[None]
    n_maps, rows, cols = g.shape
    cm = np.ascontiguousarray(np.transpose(g, (0, 2, 1)))          # the ABI's [n_maps][cols][rows]
    out = np.empty(cm.shape, dtype=np.float32)
    rc = load().pqp_emu_distance_layer(n_maps, rows, cols, resolution, cm.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    out = np.transpose(out, (0, 2, 1))
    return out[0] if two_d else out


def wide(rows, cols):
    return bool(load().pqp_emu_distance_wide(rows, cols))


def sqrt_rn(d2):
    return np.float32(load().pqp_emu_sqrt_rn(int(d2)))
