"""ctypes binding of the C ABI in include/pqp.h (libpqp_hip.so).

Python is plumbing here (tests, bench, smoke); the product is the shared library.  There is no CPU
fallback: if the library or a HIP device is missing, loading / pqp_create fails loudly.

Nothing of the ABI is restated here: the Structure classes (pqp_grid_geometry -> PqpGridGeometry), the constants (PQP_OPT_STORE_WARM ->
OPT_STORE_WARM), EXPORTS and every function's argtypes / restype are built from what pqp_header reads in include/pqp.h.
"""
import collections
import ctypes as C
import inspect
import os
import types

import numpy as np

from . import pqp_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpqp_hip.so")

HEADER = pqp_header.read()
EXPORTS = list(HEADER.functions)
globals().update({k[len("PQP_"):]: v for k, v in HEADER.constants.items()})      # OPT_*, KERNEL_*, FOOTPRINT_*, *_STRIDE, PROJ_*, SPEED_*, TRAJ_*, ...

_FIELD = {"double": C.c_double, "int32_t": C.c_int32}
STRUCTS = {}                                                   # header name -> Structure class, in the header's order
for _s in list(HEADER.structs.values()) + list(HEADER.included.values()):       # pqp.h's own, then those of the headers it includes
    STRUCTS[_s.name] = type(pqp_header.class_name(_s.name), (C.Structure,),
                            {"_fields_": [(f, _FIELD.get(t) or STRUCTS[t]) for f, t in _s.fields], "__module__": __name__})
globals().update({c.__name__: c for c in STRUCTS.values()})    # PqpParams, PqpSizes, PqpGridGeometry, ...

_DTYPE = {"double": "float64", "float": "float32", "int32_t": "int32", "int": "int32", "uint8_t": "uint8"}      # pointee -> numpy / torch name
_PASS = (C.c_void_p, C.Array, C._Pointer, type(C.byref(C.c_int())))


class _DataPointer:
    """argtype of one data-pointer parameter (const double* ref, int32_t* status, ...).  None, an int, a c_void_p and a ctypes array,
    pointer or byref go through unchecked (device pointers look like that); a numpy array or an object with data_ptr() (a torch tensor)
    must hold the pointee's element type, an array must be C-contiguous.  Anything else is a TypeError before the library is entered."""
    __slots__ = ("where", "dtype")

    def __init__(self, function, param):
        self.where = f"{function}: {param.name} ({param.type})"
        self.dtype = _DTYPE[pqp_header.pointee(param.type)[0]]

    def from_param(self, v):
        if v is None or isinstance(v, _PASS):
            return v
        if isinstance(v, np.ndarray):
            if v.dtype.name != self.dtype or not v.flags["C_CONTIGUOUS"]:
                raise TypeError(f"{self.where} wants a C-contiguous {self.dtype} array, not {v.dtype.name}"
                                f"{'' if v.flags['C_CONTIGUOUS'] else ' (not contiguous)'}")
            return C.c_void_p(v.ctypes.data)
        if hasattr(v, "data_ptr"):
            if str(v.dtype) != "torch." + self.dtype:
                raise TypeError(f"{self.where} wants a {self.dtype} tensor, not {v.dtype}")
            return C.c_void_p(v.data_ptr())
        if isinstance(v, (int, np.integer)):
            return C.c_void_p(int(v))
        raise TypeError(f"{self.where} wants None, an address, a ctypes pointer, a numpy array or a tensor, not {type(v).__name__}")


_RESTYPE = {"int": C.c_int, "void": None, "const char*": C.c_char_p, "pqp_handle*": C.c_void_p}


def _argtype(function, param):
    base, stars = pqp_header.pointee(param.type)
    if stars == 0:
        return {"int": C.c_int, "double": C.c_double}[base]
    if stars == 2:
        return C.POINTER(C.c_void_p)                           # pqp_handle**, pqp_multi**, void**, double* const*
    if base in STRUCTS:
        return C.POINTER(STRUCTS[base])
    if base == "void" or base in HEADER.opaque:
        return C.c_void_p
    return _DataPointer(function, param)


_lib = None


def load_library(path=None, with_torch=None):
    """dlopen libpqp_hip.so and give every function of the header its argtypes and restype.  Raises OSError if the library was not built
    or lacks a function the header declares.
    with_torch: import torch BEFORE the library is mapped (see below).  None = yes unless PQP_CAPI_TORCH=0: the safe default for a process that
    may use torch later; a torch-free user of the C ABI passes False (or sets PQP_CAPI_TORCH=0) and skips torch's multi-second import."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("PQP_LIB") or LIB_PATH        # PQP_LIB: an alternative build of the library (experiments)
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # A process that also uses torch must load torch's HIP runtime FIRST: the wheel bundles its own libamdhip64 under the soname this library needs
    # too, and whichever copy is mapped first serves both - with /opt/rocm's mapped first, torch finds no device ("No HIP GPUs are available").
    # (The device-resident entry points of this binding use torch as memory plumbing; the library itself does not depend on it.)
    import sys
    if with_torch is None:
        with_torch = os.environ.get("PQP_CAPI_TORCH", "1") != "0"
    if with_torch or "torch" in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(path)
    for f in HEADER.functions.values():
        try:
            fn = getattr(lib, f.name)
        except AttributeError:
            raise OSError(f"{path} lacks {f.name}, which include/pqp.h declares: rebuild the library") from None
        fn.argtypes = [_argtype(f.name, p) for p in f.params]
        fn.restype = _RESTYPE[f.ret]
    if path == LIB_PATH:
        _lib = lib
    return lib


class PqpError(RuntimeError):
    pass


def _raise_on(lib, rc):
    if rc != 0:
        raise PqpError(f"pqp error {rc}: {lib.pqp_last_error().decode()}")


def _defaults(lib, struct, function, over):
    """struct filled by the library's `function` (pqp_*_default_*), with `over` applied"""
    lib = lib or load_library()
    p = struct()
    getattr(lib, function)(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_params(lib=None, **over):
    return _defaults(lib, PqpParams, "pqp_default_params", over)


def production_params(lib=None, **over):
    """pqp_production_params: the defaults + the engine's production solver setting (1e-4 + KKT-verified polish)."""
    return _defaults(lib, PqpParams, "pqp_production_params", over)


def car_default_geometry(lib=None, **over):
    """pqp_car_default_geometry: the reference's flags (car_width 2.0, rear_length -1.0, front_length 3.9), with `over` applied."""
    return _defaults(lib, PqpCarGeometry, "pqp_car_default_geometry", over)


def select_default_params(lib=None, **over):
    """pqp_select_default_params: the path QP's own weights on k and dk (20, 100), nothing else weighted, clearance_want 0.6,
    require_free 1, with `over` applied."""
    return _defaults(lib, PqpSelectParams, "pqp_select_default_params", over)


def speed_default_params(lib=None, **over):
    """pqp_speed_default_params: v_max 10 m/s, a_max 1.5, d_max 3 and a_lat_max 2 m/s^2 - this library's choice, the reference has no such
    flags - with `over` applied."""
    return _defaults(lib, PqpSpeedParams, "pqp_speed_default_params", over)


def sample_default_params(lib=None, **over):
    """pqp_sample_default_params: dt 0.1 s, hold_last 0 - this library's choice - with `over` applied."""
    return _defaults(lib, PqpSampleParams, "pqp_sample_default_params", over)


class AgentsParams:
    """what pqp_agents_check takes besides its arrays and the car: the margin alone, which the C ABI therefore passes as a double and not
    in a struct.  Here it keeps the shape of the other parameter sets (agents_default_params(margin=...), prm=, agents_params=)."""
    __slots__ = ("margin",)

    def __init__(self, margin):
        self.margin = float(margin)


def agents_default_params(lib=None, **over):
    """pqp_agents_default_params: margin 0 m (touching is no hit) - this library's choice - with `over` applied."""
    lib = lib or load_library()
    margin = C.c_double(-1.0)
    lib.pqp_agents_default_params(C.byref(margin))
    p = AgentsParams(margin.value)
    for k, v in over.items():
        setattr(p, k, v)
    return p


SearchParams = PqpSearchParams                                 # pqp_search_params under the name the other parameter sets go by here


def search_default_params(lib=None, **over):
    """pqp_search_default_params: dt 1 s, ds 0.5 m, both weights 1, margin 0, 128 stations, steps up to 20 cells that grow by at most 3 and
    shrink by at most 6 per layer - pqp_search_params_from_speed on the speed defaults - with `over` applied."""
    return _defaults(lib, SearchParams, "pqp_search_default_params", over)


def search_params_from_speed(lib, speed_prm, dt, ds):
    """pqp_search_params_from_speed (pure host): the defaults with q_max, q_up and q_down from the speed limits of `speed_prm` at the grid
    dt, ds.  PqpError when floor(v_max dt / ds) > 63."""
    lib = lib or load_library()
    p = SearchParams()
    _raise_on(lib, lib.pqp_search_params_from_speed(C.byref(speed_prm), float(dt), float(ds), C.byref(p)))
    return p


class RefineParams:
    """what pqp_speed_refine takes besides its arrays and the search's grid: the REFINE_PARAMS doubles the C ABI passes as a plain array
    (w_ref, w_accel, w_jerk, a_max, d_max, at REFINE_W_REF .. REFINE_D_MAX) and the window beside them, under the names of the header's
    enumerators.  refine_default_params(w_jerk=...) as for the other parameter sets."""
    __slots__ = ("w_ref", "w_accel", "w_jerk", "a_max", "d_max", "window")
    _INDEX = (("w_ref", REFINE_W_REF), ("w_accel", REFINE_W_ACCEL), ("w_jerk", REFINE_W_JERK), ("a_max", REFINE_A_MAX), ("d_max", REFINE_D_MAX))

    def __init__(self, values, window):
        for name, i in self._INDEX:
            setattr(self, name, float(values[i]))
        self.window = int(window)

    def array(self):
        out = np.zeros(REFINE_PARAMS)
        for name, i in self._INDEX:
            out[i] = getattr(self, name)
        return out


def refine_default_params(lib=None, **over):
    """pqp_refine_default_params: the weights 1, 1, 1, the speed defaults' a_max 1.5 and d_max 3 m/s^2, window 4 - with `over` applied."""
    lib = lib or load_library()
    values, window = np.full(REFINE_PARAMS, -1.0), C.c_int(-1)
    lib.pqp_refine_default_params(values, C.byref(window))
    p = RefineParams(values, window.value)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class RankParams:
    """what pqp_select_plans takes besides its arrays: the RANK_PARAMS doubles the C ABI passes as a plain array (w_path, w_progress,
    w_accel, w_jump, w_lateral, w_clearance, clearance_want, at RANK_W_PATH .. RANK_CLEARANCE_WANT) and require_free beside them, under
    the names of the header's enumerators.  rank_default_params(w_progress=...) as for the other parameter sets."""
    __slots__ = ("w_path", "w_progress", "w_accel", "w_jump", "w_lateral", "w_clearance", "clearance_want", "require_free")
    _INDEX = (("w_path", RANK_W_PATH), ("w_progress", RANK_W_PROGRESS), ("w_accel", RANK_W_ACCEL), ("w_jump", RANK_W_JUMP),
              ("w_lateral", RANK_W_LATERAL), ("w_clearance", RANK_W_CLEARANCE), ("clearance_want", RANK_CLEARANCE_WANT))

    def __init__(self, values, require_free):
        for name, i in self._INDEX:
            setattr(self, name, float(values[i]))
        self.require_free = int(require_free)

    def array(self):
        out = np.zeros(RANK_PARAMS)
        for name, i in self._INDEX:
            out[i] = getattr(self, name)
        return out


def rank_default_params(lib=None, **over):
    """pqp_rank_default_params: the weights 1, 1, 1, 1, 1, 0, the selection's clearance_want 0.6, require_free 1 - with `over` applied."""
    lib = lib or load_library()
    values, require_free = np.full(RANK_PARAMS, -1.0), C.c_int(-1)
    lib.pqp_rank_default_params(values, C.byref(require_free))
    p = RankParams(values, require_free.value)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class PredictParams:
    """what pqp_predict_agents takes besides its arrays and the time grid: the PREDICT_PARAMS doubles the C ABI passes as a plain array
    (v_cap, grow, l_max, at PREDICT_V_CAP .. PREDICT_L_MAX), under the names of the header's enumerators.
    predict_default_params(grow=...) as for the other parameter sets."""
    __slots__ = ("v_cap", "grow", "l_max")
    _INDEX = (("v_cap", PREDICT_V_CAP), ("grow", PREDICT_GROW), ("l_max", PREDICT_L_MAX))

    def __init__(self, values):
        for name, i in self._INDEX:
            setattr(self, name, float(values[i]))

    def array(self):
        out = np.zeros(PREDICT_PARAMS)
        for name, i in self._INDEX:
            out[i] = getattr(self, name)
        return out


def predict_default_params(lib=None, **over):
    """pqp_predict_default_params: v_cap 40 m/s, grow 0 m/s, l_max 3 m - this library's choice - with `over` applied."""
    lib = lib or load_library()
    values = np.full(PREDICT_PARAMS, -1.0)
    lib.pqp_predict_default_params(values)
    p = PredictParams(values)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class OverlayParams:
    """what pqp_overlay_agents takes besides its arrays: inflate alone, which the C ABI therefore passes as a double and not in a struct
    (AgentsParams' case)."""
    __slots__ = ("inflate",)

    def __init__(self, inflate):
        self.inflate = float(inflate)


def overlay_default_params(lib=None, **over):
    """pqp_overlay_default_params: inflate 0 m (the corridor and the footprint check add the car's circles and the safety margin
    themselves) - this library's choice - with `over` applied."""
    lib = lib or load_library()
    inflate = C.c_double(-1.0)
    lib.pqp_overlay_default_params(C.byref(inflate))
    p = OverlayParams(inflate.value)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class StitchParams:
    """what pqp_stitch_trajectory takes besides its arrays: the STITCH_PARAMS doubles the C ABI passes as a plain array (t_ahead, lat_max,
    lon_max, dh_max, v_still, v_cap, at STITCH_T_AHEAD .. STITCH_V_CAP) and keep beside them, under the names of the header's
    enumerators.  stitch_default_params(lat_max=...) as for the other parameter sets."""
    __slots__ = ("t_ahead", "lat_max", "lon_max", "dh_max", "v_still", "v_cap", "keep")
    _INDEX = (("t_ahead", STITCH_T_AHEAD), ("lat_max", STITCH_LAT_MAX), ("lon_max", STITCH_LON_MAX), ("dh_max", STITCH_DH_MAX),
              ("v_still", STITCH_V_STILL), ("v_cap", STITCH_V_CAP))

    def __init__(self, values, keep):
        for name, i in self._INDEX:
            setattr(self, name, float(values[i]))
        self.keep = int(keep)

    def array(self):
        out = np.zeros(STITCH_PARAMS)
        for name, i in self._INDEX:
            out[i] = getattr(self, name)
        return out


def stitch_default_params(lib=None, **over):
    """pqp_stitch_default_params: t_ahead 0.1 s, lat_max 0.5 m, lon_max 2.5 m, dh_max 0.5 rad, v_still 0.1 m/s, v_cap +inf, keep 20 - this
    library's choice - with `over` applied."""
    lib = lib or load_library()
    values, keep = np.full(STITCH_PARAMS, -1.0), C.c_int(-1)
    lib.pqp_stitch_default_params(values, C.byref(keep))
    p = StitchParams(values, keep.value)
    for k, v in over.items():
        setattr(p, k, v)
    return p


class FallbackParams:
    """what pqp_fallback_rows takes besides its arrays: levels [L][2] = (braking d, jerk j) per level, d ascending, 1 <= L <=
    FALLBACK_MAX_LEVELS, and a_cap, the cap on the acceleration the braking starts from (prm[FALLBACK_A_CAP] of the C ABI).
    fallback_default_params(a_cap=...) as for the other parameter sets."""
    __slots__ = ("levels", "a_cap")

    def __init__(self, levels, a_cap):
        self.levels = np.array(levels, dtype=np.float64).reshape(-1, 2)
        self.a_cap = float(a_cap)

    def array(self):
        out = np.zeros(FALLBACK_PARAMS)
        out[FALLBACK_A_CAP] = self.a_cap
        return out

    def level_rows(self):
        """(L, levels as the contiguous [L][2] float64 array the C ABI reads)"""
        levels = np.ascontiguousarray(self.levels, dtype=np.float64).reshape(-1, 2)
        return levels.shape[0], levels


def _check_fallback_params(who, prm):
    """what pqp_fallback_rows refuses of its parameters, for a caller that wants it refused before anything is launched"""
    levels = np.asarray(prm.levels, dtype=np.float64)
    if levels.ndim != 2 or levels.shape[1] != 2 or not 1 <= levels.shape[0] <= FALLBACK_MAX_LEVELS:
        raise ValueError(f"{who}: levels must be [L][2] = (d, j) with 1 <= L <= {FALLBACK_MAX_LEVELS}, not {levels.shape}")
    if not (np.isfinite(levels).all() and (levels > 0.0).all() and (np.diff(levels[:, 0]) >= 0.0).all()):
        raise ValueError(f"{who}: every level's d and j must be finite and > 0, and d must ascend")
    if not prm.a_cap >= 0.0:
        raise ValueError(f"{who}: a_cap must be >= 0, not {prm.a_cap}")


def fallback_default_params(lib=None, **over):
    """pqp_fallback_default_params: levels (1.5, 2.5), (3.0, 5.0), (6.0, 15.0) in m/s^2 and m/s^3 around the speed profile's d_max, a_cap
    1.5 m/s^2 = its a_max - this library's choice - with `over` applied."""
    lib = lib or load_library()
    prm, levels, count = np.full(FALLBACK_PARAMS, -1.0), np.full((FALLBACK_DEFAULT_LEVELS, 2), -1.0), C.c_int(-1)
    lib.pqp_fallback_default_params(prm, levels, C.byref(count))
    p = FallbackParams(levels[:count.value], prm[FALLBACK_A_CAP])
    for k, v in over.items():
        setattr(p, k, np.array(v, dtype=np.float64).reshape(-1, 2) if k == "levels" else v)
    return p


def standing_rows(tracks, v_still=0.0):
    """tracks [n_scenes][a_max][9] = x, y, heading, v, a, yaw_rate, half_length, half_width, radius (predict_agents' input) -> the rows
    [n_scenes][a_max][6] = x, y, heading, half_length, half_width, radius that overlay_agents and parked= take: of a track that stands
    (v <= v_still and a <= 0) the pose and the size, copied; of a present track with a value that is not finite a bad row (its pose NaN:
    it must not vanish, the overlay then closes the scene); of every other track - absent, or moving: the speed stages' - the absent
    row (0, 0, 0, -1, -1, 0).  Host numpy."""
    tracks = np.asarray(tracks, dtype=np.float64)
    if tracks.ndim != 3 or tracks.shape[2] != TRACK_STRIDE:
        raise ValueError(f"standing_rows: tracks must be [n_scenes][a_max][{TRACK_STRIDE}], not {tracks.shape}")
    absent = (tracks[..., 6] < 0.0) | (tracks[..., 7] < 0.0)
    bad = ~absent & ~np.isfinite(tracks).all(axis=2)
    with np.errstate(invalid="ignore"):
        stands = ~absent & ~bad & (tracks[..., 3] <= float(v_still)) & (tracks[..., 4] <= 0.0)
    rows = np.empty(tracks.shape[:2] + (AGENT_STRIDE,))
    rows[...] = [0.0, 0.0, 0.0, -1.0, -1.0, 0.0]
    rows[stands] = tracks[stands][:, [0, 1, 2, 6, 7, 8]]
    rows[bad] = tracks[bad][:, [0, 1, 2, 6, 7, 8]]
    rows[bad, :3] = np.nan
    return rows


class _PredictedAgents:
    """the shape of an agents array that a prediction fills on the device (optimize_path's tracks=): what the checks of agents= and
    plan_agents= read of a host array, without the array"""
    __slots__ = ("shape",)

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)

    @property
    def size(self):
        return int(np.prod(self.shape))

    @property
    def ndim(self):
        return len(self.shape)


def _lanes(lanes, who):
    """lanes = (spline [n_lanes][9][lane_m], spline_ext [n_lanes][4], length [n_lanes]) or None -> (n_lanes, lane_m, the three arrays)"""
    if lanes is None:
        return 0, 0, None, None, None
    spl, ext, length = (np.ascontiguousarray(a, dtype=np.float64) for a in lanes)
    if spl.ndim != 3 or spl.shape[1] != 9 or ext.shape != (spl.shape[0], 4) or length.shape != (spl.shape[0],):
        raise ValueError(f"{who}: lanes must be (spline [n_lanes][9][lane_m], spline_ext [n_lanes][4], length [n_lanes]), not "
                         f"{spl.shape}, {ext.shape}, {length.shape}")
    if spl.shape[0] == 0:
        return 0, 0, None, None, None
    return spl.shape[0], spl.shape[2], spl, ext, length


def car_circles(car=None, lib=None):
    """pqp_car_circles (pure host): [7][3] x, y, r in the vehicle frame of rr, rl, fr, fl, fm, rm and the bounding circle."""
    lib = lib or load_library()
    car = car if car is not None else car_default_geometry(lib)
    out = np.zeros((7, 3))
    _raise_on(lib, lib.pqp_car_circles(C.byref(car), out))
    return out


def _ptr(a):
    """c_void_p of a host array or a raw address: what the typed argtypes let through unchecked (raw calls in tests and tools)"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))      # raw device pointer (e.g. torch.Tensor.data_ptr())


def _dp(x):
    """c_void_p of a device pointer: an int, or an object with data_ptr() (a torch tensor), unchecked"""
    if x is None:
        return None
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))


def stream_batch_default(n, lib=None):
    """pqp_stream_batch_default: from how many QPs of n waypoints on a cold call runs on the lane-per-QP kernel (PQP_OPT_STREAM_BATCH's default)."""
    lib = lib or load_library()
    return int(lib.pqp_stream_batch_default(int(n)))


def path_interval(value, n):
    """What pqp_params.adaptive_rho_interval / check_termination / polish_every mean for paths of n waypoints: negative values (the production
    setting) stand for "by path length" (csrc/pqp_defaults.hpp path_interval: 5 iterations up to 90 waypoints, 8 beyond)."""
    return value if value >= 0 else (5 if n <= 90 else 8)


class MultiHandle:
    """pqp_multi: one handle + one host thread per shard of the batch (several GPUs of one node; devices may repeat)."""

    def __init__(self, params=None, devices=(0,), max_batch_per_shard=1024, max_n=128):
        self.lib = load_library(with_torch=True)
        self.params = params or default_params(self.lib)
        self._m = C.c_void_p()
        devs = (C.c_int32 * len(devices))(*devices)
        _raise_on(self.lib, self.lib.pqp_multi_create(C.byref(self._m), C.byref(self.params), len(devices), devs, max_batch_per_shard, max_n))

    def close(self):
        if self._m:
            self.lib.pqp_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        _raise_on(self.lib, self.lib.pqp_multi_set_option(self._m, int(option), int(value)))

    def solve(self, ref, bounds, scal, lin=None, passes=1, n_of=None):
        ref = np.ascontiguousarray(ref, dtype=np.float64); bounds = np.ascontiguousarray(bounds, dtype=np.float64)
        scal = np.ascontiguousarray(scal, dtype=np.float64)
        lin = None if lin is None else np.ascontiguousarray(lin, dtype=np.float64)
        counts = None if n_of is None else np.ascontiguousarray(n_of, dtype=np.int32)
        batch, n = ref.shape[0], ref.shape[1]
        out = np.zeros((batch, n, 7)); status = np.zeros(batch, dtype=np.int32); iters = np.zeros(batch, dtype=np.int32); info = np.zeros((batch, 8))
        _raise_on(self.lib, self.lib.pqp_multi_path_solve(self._m, batch, n, counts, ref, lin, bounds, scal, passes, out, status, iters, info))
        self._last = (batch, n)
        return dict(out=out, status=status, iters=iters, info=info)

    def gather_paths(self, devices):
        """pqp_multi_gather_paths after solve(): one torch tensor [batch][n][7] per shard, on the shard's GPU (`devices`: the list given at creation),
        every one holding the whole batch - gathered over RCCL, nothing through the host."""
        import torch
        batch, n = self._last
        outs = [torch.zeros((batch, n, 7), dtype=torch.float64, device=torch.device("cuda", int(d))) for d in devices]
        for d in devices:
            torch.cuda.synchronize(int(d))
        ptrs = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        _raise_on(self.lib, self.lib.pqp_multi_gather_paths(self._m, batch, n, ptrs))
        return outs

    def gather_ranks(self):
        """ncclCommCount of the gather's communicator (0 before the first gather_paths)."""
        return int(self.lib.pqp_multi_gather_ranks(self._m))


def _occupancy(grid, who):
    """uint8 occupancy grids [n_maps][rows][cols] (0 = obstacle).  A bool mask is refused: which of its values would mean obstacle is easy
    to get backwards."""
    grid = np.asarray(grid)
    if grid.dtype != np.uint8:
        raise TypeError(f"{who}: grid must be uint8 with 0 = obstacle, not {grid.dtype}")
    return grid[None] if grid.ndim == 2 else grid


def _check_group_start(group_start, batch):
    """what pqp_select_paths refuses on the host and the device form cannot see"""
    gs = np.asarray(group_start)
    if gs.ndim != 1 or gs.size < 1 or gs[0] != 0 or gs[-1] != batch or (np.diff(gs) < 0).any():
        raise ValueError(f"group_start must ascend from 0 to the batch ({batch})")


def _column_major(maps, dtype):
    """one map [rows][cols] or many [n_maps][rows][cols] -> the ABI's column-major [n_maps][cols][rows], contiguous, as dtype"""
    maps = np.asarray(maps, dtype=dtype)
    if maps.ndim == 2:
        maps = maps[None]
    return np.ascontiguousarray(np.transpose(maps, (0, 2, 1)))


_i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
_f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _check_sizes(who, *named):
    """(name, array or None, entries) of a host-array method's optional arrays"""
    for name, a, size in named:
        if a is not None and a.size != size:
            raise ValueError(f"{who}: {name} must have {size} entries, not {a.size}")


def _paths_with_profile(who, paths, profile):
    """paths [B][n][stride] and their profile [B][n][4] as float64 arrays, and (B, n, stride)"""
    paths = _f64(paths)
    B, n, stride = paths.shape
    profile = _f64(profile)
    if profile.shape != (B, n, SPEED_STRIDE):
        raise ValueError(f"{who}: profile must be {(B, n, SPEED_STRIDE)}, not {profile.shape}")
    return paths, profile, (B, n, stride)


# ---- the steps of Handle.optimize_path, one record each ----------------------------------------------------------------------------------
# A stage function takes the call's context c (Handle._chain_plan) and returns its record; _STAGES below says which calls have the step:
#   outputs  (result key, shape, dtype, per_candidate): a zero-filled device buffer of that name, downloaded under that key - unless
#            per_candidate (a row per candidate, not per winner) and winners_only, which keep it on the device
#   scratch  (name, shape, dtype[, "empty"]): device buffers nothing downloads, zero-filled unless "empty"
#   uploads  (name, host array or None, dtype)
#   launch   launch(h, c, d): the step's library calls on handle h, d = the call's device buffers by name (a name may hold None, and
#            d.get(name) is None too where no stage of this call made the buffer)
# Every buffer exists before the call's one torch.cuda.synchronize, which orders torch's uploads and fills before the launches on the
# handle's non-blocking stream: a launch allocates nothing.
_Stage = collections.namedtuple("_Stage", "outputs scratch uploads launch")
_F, _I, _U8 = "float64", "int32", "uint8"
_per_row = lambda rows, dtype, *keys: tuple((k, (rows,), dtype, False) for k in keys)
_paths = lambda c, d: (d[c.paths[0]], d[c.paths[1]], d.get(c.paths[2]))         # paths, n_of, stop_before of the speed stages


def _agent_rows(c, d, rows="agents", frames="agent_frames"):
    """n_scenes, a_max, the agents' rows, agents_of, scene_of, the frames: what every reader of the agents takes (a_max = 0: no rows)"""
    shape, some = c.moving[0].shape, c.moving[0].size > 0
    return shape[0], shape[1], d[rows] if some else None, d["agents_of"], d["scene_of"], d[frames] if some else None


def _stage_overlay(c):
    """in front of the chain: the scenes' layers from the base layers (d["base"]: uploaded, or built from the grid) and the standing
    agents.  Its scratch is named dist, so every later reader of d["dist"] - the chain, the footprint check - reads the scenes' layers"""
    ag, base_of, inflate = c.parked
    g, some = c.args.geom, ag.size > 0
    launch = lambda h, c, d: h._check(h.lib.pqp_overlay_agents_device(
        h._h, inflate, d["base"].shape[0], C.byref(g), d["base"], ag.shape[0], ag.shape[1], d["parked_agents"] if some else None, None,
        d["parked_base_of"], d["parked_frames"] if some else None, d["dist"], d["parked_flags"]))
    return _Stage((("parked_flags", (ag.shape[0],), _I, False),),
                  (("dist", (ag.shape[0], g.cols, g.rows), "float32", "empty"), ("parked_frames", ag.shape[:2] + (AGENT_FRAME_STRIDE,), _F, "empty")),
                  (("parked_agents", ag, _F), ("parked_base_of", base_of, _I)), launch)


def _stage_stitch(c):
    """in front of the chain, beside the overlay: the start of this cycle from the previous cycle's plan.  Its scratch is named start,
    start_k and v_start, so the chain and the speed profile read what it wrote: start and start_k a row per candidate, v_start a row per
    row of the speed stages - per candidate, or with select= per group, which a second launch over the groups alone writes (the
    per-group column of the state row, contiguous as pqp_speed_profile takes it)"""
    prev, prev_m, meas, t_now, prm, group_start = c.previous
    G, m, stride = prev.shape
    per_group = c.speed is not None and not c.per_candidate

    def launch(h, c, d):
        call = lambda batch, starts, start, start_k, v_start: h._check(h.lib.pqp_stitch_trajectory_device(
            h._h, prm.array(), int(prm.keep), m, G, m, stride, d["stitch_prev"], d["stitch_prev_m"], d["stitch_meas"], d["stitch_t_now"], batch, starts,
            d["stitch_state"], d["stitch_flags"], d["stitch_dev"], d["stitch_idx"], d["stitch_prefix"], d["stitch_prefix_n"], start, start_k, v_start))
        call(c.B, d["stitch_group_start"], d["start"], d["start_k"], None if per_group else d.get("v_start"))
        if per_group:
            call(G, None, None, None, d["v_start"])
    return _Stage((("stitch_state", (G, TRAJ_STRIDE), _F, False), ("stitch_flags", (G,), _I, False), ("stitch_dev", (G, 3), _F, False),
                   ("stitch_prefix", (G, m, TRAJ_STRIDE), _F, False), ("stitch_prefix_n", (G,), _I, False)),
                  (("stitch_idx", (G, 3), _I), ("start", (c.B, 3), _F), ("start_k", (c.B,), _F)) + ((("v_start", (c.rows,), _F),) if c.speed is not None else ()),
                  (("stitch_prev", prev, _F), ("stitch_prev_m", prev_m, _I), ("stitch_meas", meas, _F), ("stitch_t_now", t_now, _F),
                   ("stitch_group_start", group_start, _I)), launch)


def _stage_chain(c):
    """pqp_optimize_path_device itself, in the same form"""
    a = c.args
    launch = lambda h, c, d: h._check(h.lib.pqp_optimize_path_device(
        h._h, a.smoother._h if a.smoother is not None else None, C.byref(c.cfg), c.B, np.shape(a.points)[1], d["points"], d["n_points"], d["start"],
        d["target"], d["dist"], d["map_of"], C.byref(a.geom), d["start_k"], d["out"], d["n_out"], d["status"], d["stage"], d["iters"]))
    return _Stage((("out", (c.B, c.n_max, 7), _F, True),) + _per_row(c.B, _I, "n_out", "status", "stage", "iters"), (),
                  (("points", a.points, _F), ("n_points", a.n_points, _I), ("start", a.start, _F), ("target", a.target, _F), ("map_of", a.map_of, _I),
                   ("start_k", a.start_k, _F)), launch)


def _stage_footprint(c):
    """behind the chain: reads out / n_out where they are"""
    launch = lambda h, c, d: h._check(h.lib.pqp_footprint_check_device(
        h._h, c.B, c.n_max, 7, d["out"], d["n_out"], d["dist"], d["map_of"], C.byref(c.args.geom), C.byref(c.car), c.footprint, d["free"],
        d["first_collision"], d["margin"]))
    return _Stage((("free", (c.B, c.n_max), _U8, True), ("first_collision", (c.B,), _I, False), ("margin", (c.B, c.n_max), _F, True)), (), (), launch)


def _stage_selection(c):
    """behind both: reads out, n_out, status, stage (and first_collision, margin) where they are"""
    launch = lambda h, c, d: h._check(h.lib.pqp_select_paths_device(
        h._h, C.byref(c.selection[1]), c.B, c.n_max, 7, d["out"], d["n_out"], d["status"], d["stage"], d.get("first_collision"), d.get("margin"),
        c.groups, d["group_start"], d["terms"], d["best"], d["best_paths"], d["best_n"]))
    return _Stage((("terms", (c.B, SCORE_STRIDE), _F, False), ("best", (c.groups,), _I, False), ("best_paths", (c.groups, c.n_max, 7), _F, False),
                   ("best_n", (c.groups,), _I, False)), (), (("group_start", c.selection[0], _I),), launch)


def _stage_speed(c):
    """behind all of them, on c.paths: the winners where the selection left them (an eligible winner is collision-free: require_free), or
    every candidate in `out` up to its first collision"""
    launch = lambda h, c, d: h._check(h.lib.pqp_speed_profile_device(
        h._h, C.byref(c.speed[0]), c.rows, c.n_max, 7, *_paths(c, d), None, d["v_start"], d["v_end"], d["profile"], d["speed_flags"]))
    return _Stage((("profile", (c.rows, c.n_max, SPEED_STRIDE), _F, c.per_candidate), ("speed_flags", (c.rows,), _I, False)), (),
                  (("v_start", c.speed[1], _F), ("v_end", c.speed[2], _F)), launch)


def _stage_sampling(c):
    """behind the speed profile, on the arrays it ran on"""
    prm, m, t0 = c.sampling
    launch = lambda h, c, d: h._check(h.lib.pqp_sample_trajectory_device(
        h._h, C.byref(prm), c.rows, c.n_max, 7, *_paths(c, d), d["profile"], d["t0"], m, d["traj"], d["traj_n"], d["traj_flags"]))
    return _Stage((("traj", (c.rows, m, TRAJ_STRIDE), _F, False),) + _per_row(c.rows, _I, "traj_n", "traj_flags"), (), (("t0", t0, _F),), launch)


def _stage_predicting(c):
    """the agents' rows on the device, for every step that reads them: uploaded, or with tracks= predicted where the search reads them - at
    the layers' times, and on the fine steps the plan is checked at - so that only the tracks cross to the device"""
    ag, agents_of, scene_of = c.moving[:3]
    uploads = (("agents_of", agents_of, _I), ("scene_of", scene_of, _I))
    frames = (("agent_frames", ag.shape[:3] + (AGENT_FRAME_STRIDE,), _F),)
    if c.predicting is None:
        return _Stage((), frames, uploads + (("agents", ag, _F),), lambda h, c, d: None)
    tracks, lane_of, (n_lanes, lane_m, spl, ext, length), prm, want_anchor = c.predicting

    def launch(h, c, d):
        predict = lambda r, rows, anchor, flags: h._check(h.lib.pqp_predict_agents_device(
            h._h, prm.array(), 0.0, float(c.searching.dt), ag.shape[2], r, ag.shape[0], ag.shape[1], d["tracks"], d["agents_of"], d["lane_of"], n_lanes,
            lane_m, d["lane_spline"], d["lane_ext"], d["lane_length"], rows, anchor, flags))
        predict(1, d["agents"], d.get("predict_anchor"), d["predict_flags"])
        if d.get("plan_agents") is not None:
            predict(c.planning, d["plan_agents"], None, d["predict_fine_flags"])          # (written, never returned)
    return _Stage((("predict_flags", ag.shape[:2], _I, False),) + ((("predict_anchor", ag.shape[:2] + (ANCHOR_STRIDE,), _F, False),) if want_anchor else ()),
                  frames + (("agents", ag.shape, _F, "empty"), ("predict_fine_flags", ag.shape[:2], _I)),
                  uploads + (("tracks", tracks, _F), ("lane_of", lane_of, _I), ("lane_spline", spl, _F), ("lane_ext", ext, _F), ("lane_length", length, _F)),
                  launch)


def _stage_agents(c):
    """behind the sampler, on its samples: all of them with hold_last (the parked car), else those on the path"""
    launch = lambda h, c, d: h._check(h.lib.pqp_agents_check_device(
        h._h, float(c.moving[3].margin), C.byref(c.car), c.rows, c.samples, TRAJ_STRIDE, d["traj"], None if c.sampling[0].hold_last else d["traj_n"],
        *_agent_rows(c, d), d["first_hit"], d["hit_agent"], d["agent_clearance"]))
    return _Stage(_per_row(c.rows, _I, "first_hit", "hit_agent") + (("agent_clearance", (c.rows, c.samples), _F, False),), (), (), launch)


def _stage_searching(c):
    """behind the speed profile, on the rows it ran on and under its envelope; its blocked bits are the refine's to read and to report"""
    se, n, m = c.searching, c.rows, c.layers
    launch = lambda h, c, d: h._check(h.lib.pqp_speed_search_device(
        h._h, C.byref(se), C.byref(c.car), n, c.n_max, 7, *_paths(c, d), d["profile"], d["v_start"], m, *_agent_rows(c, d), d["search_blocked"],
        d["search_parents"], d["search_steps"], d["search_traj"], d["search_cost"], d["search_reached"], d["search_flags"]))
    stations = max(int(se.stations), 0)
    blocked = ("search_blocked", (n, m, (stations + 31) // 32), _I, False)
    return _Stage((("search_steps", (n, m, 2), _I, False), ("search_traj", (n, m, TRAJ_STRIDE), _F, c.per_candidate), ("search_cost", (n,), _F, False))
                  + _per_row(n, _I, "search_reached", "search_flags") + ((blocked,) if c.refining is not None else ()),
                  (("search_parents", (n, m, stations, max(int(se.q_max) + 1, 1)), _U8),) + ((blocked[:3],) if c.refining is None else ()), (), launch)


def _stage_refining(c):
    """behind the search, on the rows it ran on and on what it wrote"""
    rf, n, m = c.refining, c.rows, c.layers
    launch = lambda h, c, d: h._check(h.lib.pqp_speed_refine_device(
        h._h, C.byref(c.searching), rf.array(), int(rf.window), n, c.n_max, 7, *_paths(c, d), d["profile"], d["v_start"], m, d["search_blocked"],
        d["search_steps"], d["search_reached"], d["search_traj"], d["refine_traj"], d["refine_bounds"], d["refine_cost"], d["refine_excess"],
        d["refine_status"], d["refine_iters"], d["refine_flags"]))
    return _Stage((("refine_traj", (n, m, TRAJ_STRIDE), _F, c.per_candidate), ("refine_bounds", (n, m, 3), _F, False))
                  + _per_row(n, _F, "refine_cost", "refine_excess") + _per_row(n, _I, "refine_status", "refine_flags"),
                  (("refine_iters", (n,), _I),), (), launch)


def _stage_planning(c):
    """behind the refine (or the search alone), on the rows they ran on and on the plan they wrote: a refined path under constant
    acceleration, the search's or a kept one linearly"""
    n, refined = c.rows, c.refining is not None
    launch = lambda h, c, d: h._check(h.lib.pqp_sample_plan_device(
        h._h, float(c.searching.dt), c.planning, 0 if refined else 1, n, c.n_max, 7, *_paths(c, d), d["profile"], c.layers,
        d["refine_traj" if refined else "search_traj"], d["search_reached"], d.get("refine_flags"), d["plan_traj"], d["plan_m_of"], d["plan_defect"],
        d["plan_excess"], d["plan_flags"]))
    return _Stage((("plan_traj", (n, c.fine, TRAJ_STRIDE), _F, c.per_candidate), ("plan_m_of", (n,), _I, False))
                  + _per_row(n, _F, "plan_defect", "plan_excess") + _per_row(n, _I, "plan_flags"), (), (), launch)


def _stage_plan_agents(c):
    """behind that, on the fine rows that are on the plan - uploaded, or with tracks= filled by the prediction; with rank= the check also
    writes the clearance the ranking reads"""
    fine = c.plan_agents
    launch = lambda h, c, d: h._check(h.lib.pqp_agents_check_device(
        h._h, float(c.moving[3].margin), C.byref(c.car), c.rows, c.fine, TRAJ_STRIDE, d["plan_traj"], d["plan_m_of"],
        *_agent_rows(c, d, "plan_agents", "plan_frames"), d["plan_first_hit"], d["plan_hit_agent"], d.get("plan_clearance")))
    frames = (("plan_frames", fine.shape[:3] + (AGENT_FRAME_STRIDE,), _F),)
    rows = (("plan_agents", fine.shape, _F, "empty"),) if c.predicting is not None else ()          # predicted: no upload
    return _Stage(_per_row(c.rows, _I, "plan_first_hit", "plan_hit_agent"), frames + rows, () if rows else (("plan_agents", fine, _F),), launch)


def _stage_ranking(c):
    """behind everything (no selection: the rows are the B candidates): the paths' terms, then the finished trajectories - the fine rows,
    else the refine's, else the search's - and each group's best"""
    group_start, prm = c.ranking[:2]
    groups, steps = group_start.size - 1, c.fine if c.planning is not None else c.layers
    traj, m_of = ("plan_traj", "plan_m_of") if c.planning is not None else ("refine_traj" if c.refining is not None else "search_traj", "search_reached")
    clearance = c.plan_agents is not None          # the fine check ran: its first hits and clearance go in

    def launch(h, c, d):
        h._check(h.lib.pqp_select_paths_device(h._h, C.byref(select_default_params(h.lib)), c.B, c.n_max, 7, d["out"], d["n_out"], d["status"], d["stage"],
                                               d.get("first_collision"), d.get("margin"), 0, d["rank_start"], d["terms"], d["rank_best"], None, None))
        h._check(h.lib.pqp_select_plans_device(h._h, prm.array(), int(prm.require_free), c.B, steps, TRAJ_STRIDE, d[traj], d[m_of], d["terms"],
                                               d["search_flags"], d["plan_first_hit"] if clearance else None, d.get("plan_clearance"), c.n_max, 7,
                                               d["out"], d["n_out"], groups, d["rank_start"], d["rank_terms"], d["rank_best"], d["best_traj"],
                                               d["best_m"], d["best_paths"], d["best_n"]))
    return _Stage(((("plan_clearance", (c.B, c.fine), _F, True),) if clearance else ())
                  + (("terms", (c.B, SCORE_STRIDE), _F, False), ("rank_terms", (c.B, PLAN_SCORE_STRIDE), _F, False), ("rank_best", (groups,), _I, False),
                     ("best_paths", (groups, c.n_max, 7), _F, False), ("best_n", (groups,), _I, False),
                     ("best_traj", (groups, steps, TRAJ_STRIDE), _F, False), ("best_m", (groups,), _I, False)),
                  (), (("rank_start", group_start, _I),), launch)


def _stage_fallback(c):
    """behind the ranking: a braking plan per group and level along the plan the stitch read, from the state it wrote; the agent check
    (every row: the car is checked while it stands) and the footprint check on those G * L plans as the batch of trajectories they are,
    against the agents' rows of the finest check the call has - whose frames lie in their workspace already - and the scenes' layers; then
    one trajectory per group: the winner's, or the gentlest level that passed both"""
    prm, scene_of, map_of = c.fallback
    G, mp, stride = c.previous[0].shape
    L, levels = prm.level_rows()
    fine = c.planning is not None
    M, r = (c.fine, c.planning) if fine else (c.layers, 1)
    rows, frames = ("plan_agents", "plan_frames") if fine else ("agents", "agent_frames")
    mode = c.footprint if c.footprint is not None else FOOTPRINT_CIRCLES

    def launch(h, c, d):
        h._check(h.lib.pqp_fallback_rows_device(
            h._h, prm.array(), L, levels, float(c.searching.dt), r, c.layers, G, mp, stride, d["stitch_prev"], d["stitch_prev_m"], d["stitch_state"],
            d["stitch_flags"], d["fallback_rows"], d["fallback_stop"], d["fallback_stop_row"], d["fallback_row_flags"]))
        n_scenes, a_max, agents, agents_of, _, fr = _agent_rows(c, d, rows, frames)
        h._check(h.lib.pqp_agents_check_device(
            h._h, float(c.moving[3].margin), C.byref(c.car), G * L, M, TRAJ_STRIDE, d["fallback_rows"], None, n_scenes, a_max, agents, agents_of,
            d["fallback_scene_of"], fr, d["fallback_first_hit"], d["fallback_hit_agent"], None))
        h._check(h.lib.pqp_footprint_check_device(
            h._h, G * L, M, TRAJ_STRIDE, d["fallback_rows"], None, d["dist"], d["fallback_map_of"], C.byref(c.args.geom), C.byref(c.car), mode,
            d["fallback_free"], d["fallback_first_collision"], None))
        h._check(h.lib.pqp_fallback_pick_device(
            h._h, G, L, M, d["rank_best"], d["best_traj"], d["best_m"], d["fallback_rows"], d["fallback_row_flags"], d["fallback_first_hit"],
            d["fallback_first_collision"], d["final_traj"], d["final_m"], d["fallback_level"], d["fallback_flags"]))
    return _Stage((("final_traj", (G, M, TRAJ_STRIDE), _F, False), ("final_m", (G,), _I, False), ("fallback_level", (G,), _I, False),
                   ("fallback_flags", (G,), _I, False), ("fallback_rows", (G, L, M, TRAJ_STRIDE), _F, False), ("fallback_first_hit", (G * L,), _I, False),
                   ("fallback_first_collision", (G * L,), _I, False)),
                  (("fallback_stop", (G, L, 2), _F), ("fallback_stop_row", (G, L), _I), ("fallback_row_flags", (G, L), _I),
                   ("fallback_hit_agent", (G * L,), _I), ("fallback_free", (G * L, M), _U8)),
                  (("fallback_scene_of", scene_of, _I), ("fallback_map_of", map_of, _I)), launch)


# (stage, the fields of the context it needs: the call has the step when none of them is None), in launch order; the result's keys come
# in the same order, except that the prediction's stand behind the fine plan's, the overlay's and the stitch's behind everything else,
# and the fallback's behind those
_STAGES = ((_stage_overlay, ("parked",)), (_stage_stitch, ("previous",)), (_stage_chain, ()), (_stage_footprint, ("footprint",)), (_stage_selection, ("selection",)), (_stage_speed, ("speed",)),
           (_stage_sampling, ("sampling",)), (_stage_predicting, ("moving",)), (_stage_agents, ("moving", "sampling")),
           (_stage_searching, ("searching",)), (_stage_refining, ("refining",)), (_stage_planning, ("planning",)),
           (_stage_plan_agents, ("plan_agents",)), (_stage_ranking, ("ranking",)), (_stage_fallback, ("fallback",)))
_RESULT_ORDER = [f for f, _ in _STAGES if f not in (_stage_predicting, _stage_overlay, _stage_stitch, _stage_fallback)]
_RESULT_ORDER.insert(_RESULT_ORDER.index(_stage_ranking), _stage_predicting)
_RESULT_ORDER += [_stage_overlay, _stage_stitch, _stage_fallback]


class Handle:
    """Thin RAII wrapper over pqp_handle (one per GPU)."""

    def __init__(self, params=None, device=0, max_batch=1024, max_n=128):
        self.lib = load_library(with_torch=True)
        self.params = params or default_params(self.lib)
        self._h = C.c_void_p()
        self.device = int(device)          # the torch helpers below allocate and synchronise on the handle's own GPU
        self._check(self.lib.pqp_create(C.byref(self._h), C.byref(self.params), device, max_batch, max_n))

    def _check(self, rc):
        _raise_on(self.lib, rc)

    def close(self):
        if self._h:
            self.lib.pqp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        self.params = params
        self._check(self.lib.pqp_set_params(self._h, C.byref(params)))

    def sync(self):
        self._check(self.lib.pqp_sync(self._h))

    def set_option(self, option, value):
        """PQP_OPT_STORE_WARM = 1, PQP_OPT_ORDER_BY_COST = 2 (include/pqp.h)."""
        self._check(self.lib.pqp_set_option(self._h, int(option), int(value)))

    def mark(self, slot):
        self._check(self.lib.pqp_mark(self._h, slot))

    def constrain_angle(self, angles):
        """pqp_constrain_angle_device on a host array (torch as the memory plumbing)."""
        import torch
        dev = torch.device("cuda", self.device)
        a = torch.from_numpy(np.ascontiguousarray(angles, dtype=np.float64).ravel()).to(dev)
        o = torch.empty_like(a)
        torch.cuda.synchronize(dev)
        self._check(self.lib.pqp_constrain_angle_device(self._h, a.numel(), a, o))
        self.sync()
        return o.cpu().numpy().reshape(np.shape(angles))

    def wait_mark(self, other, slot):
        """Everything enqueued on this handle from now on waits for `other`'s mark `slot` (pqp_wait_mark)."""
        self._check(self.lib.pqp_wait_mark(self._h, other._h, slot))

    def wait_stream(self, hip_stream=None):
        """Order the handle's coming launches after what is enqueued on `hip_stream` now (None: the default stream; for torch tensors
        pass torch.cuda.current_stream().cuda_stream)."""
        self._check(self.lib.pqp_stream_wait(self._h, C.c_void_p(hip_stream or 0)))

    def stream(self):
        s = C.c_void_p()
        self._check(self.lib.pqp_get_stream(self._h, C.byref(s)))
        return s.value

    def chain_config(self, **over):
        return _defaults(self.lib, PqpChainConfig, "pqp_chain_default_config", over)

    def optimize_path(self, points, n_points, start, target, dist, geom, map_of=None, smoother=None, cfg=None, start_k=None, check_footprint=False,
                      car=None, footprint_mode=FOOTPRINT_CIRCLES, select=None, select_params=None, winners_only=False, search=None, refine=None,
                      plan_samples=None, plan_agents=None, agents=None, agents_of=None, scene_of=None, agents_params=None, sample=None, samples=None,
                      t0=None, tracks=None, layers=None, predict_anchor=False, fallback=None, previous=None, parked=None, rank=None, rank_params=None, speed=None, v_start=None, v_end=None):
        """pqp_optimize_path_device with torch as the memory plumbing: host arrays in, device-resident chain, host arrays out.
        points [B][p_max][2], n_points [B], start / target [B][3], dist [n_maps][rows][cols] float32.  smoother: the handle the two
        smoother QPs run on (None: this one).  cfg: PqpChainConfig (None: chain_config()); chain_config(second_pass=SECOND_PASS_BOUNDS_ON_STATES)
        runs the reference's commented-out second pass (corridor bounds on the first path's states, then a solve around it) in place of the
        re-linearised one.  Returns dict(out [B][n_max][7], n_out, status, stage, iters).
        check_footprint: pqp_footprint_check_device right behind the chain on the same stream, on its `out` (stride 7) and `n_out` and the same
        layers (car: PqpCarGeometry, None: the reference's; footprint_mode: pqp_footprint_mode); adds free [B][n_max], first_collision [B]
        and margin [B][n_max] to the dict.
        select: group_start [groups + 1] - pqp_select_paths_device behind the chain (and behind the footprint check, whose first_collision
        and margin it then reads) on the same stream; adds terms [B][8], best [groups], best_paths [groups][n_max][7] and best_n [groups]
        (select_params: PqpSelectParams, None: select_default_params()).  winners_only (with select): out, free and margin stay on the
        device and are not in the dict - only per-candidate scalars and the winners cross to the host.
        speed: PqpSpeedParams - pqp_speed_profile_device behind all of these on the same stream; adds profile [..][n_max][4] = s, v, a, t and
        speed_flags.  Without select it runs on out / n_out for every candidate, v_start (and v_end, optional) [B], stopping before
        first_collision when the footprint was checked.  With select it runs on best_paths / best_n, so only the winners become
        trajectories, v_start (and v_end) [groups]; a winner's collision index is not at hand, so select_params.require_free = 0 together
        with check_footprint is refused.  The winners' profile crosses to the host with winners_only too.
        sample: PqpSampleParams (needs speed) - pqp_sample_trajectory_device behind the speed profile on the same stream, on the arrays it ran
        on: `samples` rows per path at t0 + k dt (t0 [B], or [groups] with select; None: all 0); adds traj [..][samples][8] = x, y, heading,
        k, s, v, a, t, traj_n (the samples on the path) and traj_flags.  The winners' samples cross to the host with winners_only too.
        agents: [n_scenes][a_max][samples][6] = x, y, heading, half_length, half_width, radius of predicted agents at the samples' time steps
        (needs sample) - pqp_agents_check_device behind the sampler on the same stream, on its traj and traj_n, or on all `samples` rows
        with sample.hold_last (the parked car is checked too); agents_of [n_scenes]: agents per scene (None: all), scene_of: the scene of
        every row the sampler ran on ([B], or [groups] with select; None: scene 0), agents_params: AgentsParams (None: agents_default_params()),
        car: the footprint.  Adds first_hit, hit_agent and agent_clearance [..][samples].
        search: SearchParams (needs speed and agents; not sample) - pqp_speed_search_device behind the speed profile on the same stream, on
        the rows it ran on, with its v_start: the agents' step count is the number of layers m (with sample too, that is `samples`, and
        both run).  Adds search_steps [..][m][2], search_traj [..][m][8], search_cost, search_reached and search_flags.
        refine: RefineParams (needs search) - pqp_speed_refine_device behind the search on the same stream, on the rows the search ran on and
        on what it wrote.  Adds search_blocked [..][m][W] (what the refine read), refine_traj [..][m][8], refine_bounds [..][m][3], refine_cost, refine_excess, refine_status and refine_flags.
        plan_samples: r >= 1 (needs search) - pqp_sample_plan_device behind the refine on the same stream, r sub-steps per layer of the grid's
        dt: with refine on its traj and flags (a refined path under constant acceleration, a kept one linearly) and the search's reached,
        without refine on the search's traj, linearly.  Adds plan_traj [..][(m - 1) r + 1][8], plan_m_of, plan_defect, plan_excess and
        plan_flags.  plan_agents: [n_scenes][a_max][(m - 1) r + 1][6], the agents of `agents` on the fine steps - pqp_agents_check_device behind
        that on plan_traj and plan_m_of, under agents_params' margin and the same agents_of / scene_of; adds plan_first_hit and
        plan_hit_agent.
        rank: group_start [groups + 1] (needs search; not select: the speed stages run on every candidate) - behind everything else on the
        same stream, pqp_select_paths_device with groups = 0 for the paths' terms (select_default_params(); first_collision and margin
        when the footprint was checked), then pqp_select_plans_device on the fine rows (plan_traj, plan_m_of) when plan_samples is given,
        else on the refine's traj, else the search's, with search_reached; with plan_agents the fine check also writes its clearance,
        and plan_first_hit and that clearance go in.  rank_params: RankParams (None: rank_default_params()).  Adds terms [B][8],
        rank_terms [B][10], rank_best [groups], best_paths [groups][n_max][7], best_n, best_traj [groups][rows][8], best_m (and
        plan_clearance with plan_agents).  winners_only (with rank): out, free, margin, profile, search_traj, refine_traj, plan_traj and
        plan_clearance stay on the device and are not in the dict.
        tracks: (tracks [n_scenes][a_max][9], lane_of [n_scenes][a_max] or None, lanes = (spline, spline_ext, length) or None, PredictParams or
        None) with layers=m (needs search; refused together with agents= or plan_agents=) - pqp_predict_agents_device on the same stream
        in place of both uploads: with r = 1 at the search's dt into the rows the search reads, and with plan_samples=r into the rows the
        fine check reads, so only the tracks cross to the device and the two agree at the layers.  agents_of / scene_of / agents_params
        apply as with agents=.  Adds predict_flags [n_scenes][a_max] of PREDICT_* (and predict_anchor [n_scenes][a_max][4] with
        predict_anchor=True).  (tracks, layers, predict_anchor, previous and parked stand in front of rank: tests pin the last five names
        of the signature, and parked in front of them.)
        parked: (agents [n_scenes][a_max][6] = x, y, heading, half_length, half_width, radius of the scenes' standing agents (standing_rows
        makes them from tracks), base_of [n_scenes] or None: the layer of `dist` a scene starts from (None: layer 0 of one, else layer s of
        n_scenes), inflate in m or None: overlay_default_params()) - pqp_overlay_agents_device behind the layers' upload (or build) and in
        front of the chain on the same stream: layer(scene) = min(base layer, distance to the scene's standing agents), and every later
        reader of the layers - the chain, the footprint check, the second pass - reads those.  map_of then indexes scenes: it is refused
        outside [0, n_scenes), and None means scene 0.  Adds parked_flags [n_scenes] of OVERLAY_*, behind every other key.  Moving agents are
        not overlaid: they are the speed stages'.  A standing agent may be given both here and to the speed stages (agents= / tracks=): the
        path then goes round it and the checks still see it.
        previous: (prev [groups][m][stride >= 8], prev_m [groups] or None, meas [groups][6], t_now [groups], StitchParams or None:
        stitch_default_params()) - pqp_stitch_trajectory_device in front of the chain on the same stream: the previous cycle's best_traj /
        best_m (or any rows x, y, heading, k, s, v, a, t), the measured x, y, heading, v, a, yaw rate and its time in that plan's time base
        give the start, start_k and v_start of this cycle's candidates, on the device.  The groups are rank='s or select='s, without either one
        group per candidate; with select= and speed= the profile runs on the winners and v_start is written per group.  start (positional:
        pass None), start_k and v_start must be None.  Adds stitch_state [groups][8] (column 7: where this cycle's t = 0 lies in the old
        time base), stitch_flags [groups] of STITCH_*, stitch_dev [groups][3] = lon, lat, heading deviation, stitch_prefix [groups][m][8] (the
        re-based piece of the old plan up to the start) and stitch_prefix_n, behind every other key.  A group flagged STITCH_BAD plans from
        the zero start: its results are to be ignored.
        fallback: True (fallback_default_params()) or a FallbackParams (needs previous= and rank=) - behind the ranking on the same stream,
        pqp_fallback_rows_device along the plan the stitch read, from the state it wrote: L braking plans per group, M rows each, M and the
        agents' rows being the fine check's (plan_samples= with plan_agents= or tracks=) where the call has one, else the layers'; then
        pqp_agents_check_device (every row: the car is checked while it stands) and pqp_footprint_check_device on those groups * L plans -
        each under its group's first candidate's scene_of and map_of, so a group without candidates is refused - and
        pqp_fallback_pick_device.  Adds final_traj [groups][M][8] and final_m (a group's winner where it has one, else the gentlest braking
        plan that passed both checks: what the next cycle passes as prev and prev_m), fallback_level [groups] (-1: the winner, or a bad
        state), fallback_flags [groups] of FALLBACK_*, fallback_rows [groups][L][M][8], fallback_first_hit and fallback_first_collision
        [groups * L], behind every other key.  (fallback stands in front of previous for the reason previous stands in front of parked.)
        Every step behind the chain is one record of _STAGES above (its outputs, its uploads, its calls); _chain_plan checks the arguments and
        lays the call out from them without a device, _chain runs it."""
        a = dict(locals())                  # the arguments by name, as _chain_plan takes them: no statement may stand above this one
        del a["self"], a["dist"]
        return self._chain(self._chain_plan(**a), dist, np.float32, None)

    def optimize_path_on_grid(self, points, n_points, start, target, grid, geom, map_of=None, smoother=None, cfg=None, start_k=None,
                              check_footprint=False, car=None, footprint_mode=FOOTPRINT_CIRCLES, select=None, select_params=None,
                              winners_only=False, search=None, refine=None, plan_samples=None, plan_agents=None, agents=None, agents_of=None,
                              scene_of=None, agents_params=None, sample=None, samples=None, t0=None, tracks=None, layers=None, predict_anchor=False,
                              fallback=None, previous=None, parked=None, rank=None, rank_params=None, speed=None, v_start=None, v_end=None):
        """optimize_path with occupancy grids in place of distance layers: grid [n_maps][rows][cols] (or 2-D) uint8, 0 = obstacle, goes to the
        device as bytes, pqp_distance_layer_device builds the layers there and pqp_optimize_path_device reads them, on the same stream with
        no host round trip between the two.  Returns what optimize_path returns (check_footprint: against the layers built on the device;
        select / select_params / winners_only / speed / v_start / v_end / sample / samples / t0 / agents / agents_of / scene_of /
        agents_params / search / refine / plan_samples / plan_agents / rank / rank_params / tracks / layers / predict_anchor: as for
        optimize_path; parked: as for optimize_path, over the layers built on the device, base_of indexing the grids.  Moving agents are not
        overlaid; a standing agent may be given both to parked= and to the speed stages; previous, fallback: as for optimize_path)."""
        a = dict(locals())                  # the arguments by name, as _chain_plan takes them: no statement may stand above this one
        del a["self"], a["grid"]
        plan = self._chain_plan(**a)
        grid = _occupancy(grid, "optimize_path_on_grid")
        build = lambda d_grid, d_base: self._check(self.lib.pqp_distance_layer_device(self._h, grid.shape[0], C.byref(geom), d_grid, d_base))
        return self._chain(plan, grid, np.uint8, build)

    def _tracks(self, tracks, layers, predict_anchor, search, agents, plan_agents, plan_samples):
        """tracks= of optimize_path: (what _chain predicts from, or None; agents; plan_agents) - with tracks the two arrays are the shapes
        of what the prediction fills on the device"""
        if tracks is None:
            if layers is not None or predict_anchor:
                raise ValueError("layers / predict_anchor need tracks=")
            return None, agents, plan_agents
        if agents is not None or plan_agents is not None:
            raise ValueError("tracks is refused together with agents= or plan_agents=: the prediction fills both on the device")
        if not isinstance(search, SearchParams):
            raise ValueError("tracks needs search=SearchParams: the agents are predicted at its layers' times")
        if len(tracks) != 4:
            raise ValueError("tracks must be (tracks, lane_of or None, lanes or None, PredictParams or None)")
        tr, lane_of, lanes, prm = tracks
        tr = np.ascontiguousarray(tr, dtype=np.float64)
        if tr.ndim != 3 or tr.shape[0] < 1 or tr.shape[2] != TRACK_STRIDE:
            raise ValueError(f"tracks must be [n_scenes >= 1][a_max][{TRACK_STRIDE}], not {tr.shape}")
        if layers is None or isinstance(layers, bool) or int(layers) != layers or int(layers) < 1:
            raise ValueError("tracks needs layers=m >= 1, the layers of the search")
        layers = int(layers)
        if lane_of is not None:
            lane_of = np.ascontiguousarray(lane_of, dtype=np.int32)
            if lane_of.shape != tr.shape[:2]:
                raise ValueError(f"tracks: lane_of must be {tr.shape[:2]}, not {lane_of.shape}")
        lanes = _lanes(lanes, "tracks")
        if lane_of is not None and (lane_of >= lanes[0]).any():
            raise ValueError(f"tracks: lane_of at or above the {lanes[0]} lanes given")
        if prm is not None and not isinstance(prm, PredictParams):
            raise ValueError("tracks: the parameters must be a PredictParams")
        prm = prm if prm is not None else predict_default_params(self.lib)
        fine = None
        if plan_samples is not None and not isinstance(plan_samples, bool) and int(plan_samples) == plan_samples and int(plan_samples) >= 1:
            fine = _PredictedAgents(tr.shape[:2] + ((layers - 1) * int(plan_samples) + 1, AGENT_STRIDE))
        return (tr, lane_of, lanes, prm, bool(predict_anchor)), _PredictedAgents(tr.shape[:2] + (layers, AGENT_STRIDE)), fine

    def _speed(self, speed, v_start, v_end, check_footprint, select, select_params, previous=None):
        if speed is None:
            if v_start is not None or v_end is not None:
                raise ValueError("v_start / v_end need speed=PqpSpeedParams")
            return None
        if v_start is None and previous is None:
            raise ValueError("speed needs v_start")
        if select is not None and check_footprint and select_params is not None and not select_params.require_free:
            raise ValueError("speed with select and check_footprint needs select_params.require_free: a winner's collision index is not at hand")
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel()
        return (speed, f64(v_start), f64(v_end))

    def _sample(self, sample, samples, t0, speed):
        if sample is None:
            if samples is not None or t0 is not None:
                raise ValueError("samples / t0 need sample=PqpSampleParams")
            return None
        if speed is None:
            raise ValueError("sample needs speed=PqpSpeedParams: the samples are taken from its profile")
        if samples is None or int(samples) < 1:
            raise ValueError("sample needs samples >= 1")
        return (sample, int(samples), None if t0 is None else np.ascontiguousarray(t0, dtype=np.float64).ravel())

    def _search(self, search, speed, agents):
        if search is None:
            return None
        if not isinstance(search, SearchParams):
            raise ValueError("search must be a SearchParams")
        if speed is None:
            raise ValueError("search needs speed=PqpSpeedParams: the search runs under its profile's envelope")
        if agents is None:
            raise ValueError("search needs agents=: the predicted agents at the layers' times")
        return search

    def _refine(self, refine, search):
        if refine is None:
            return None
        if not isinstance(refine, RefineParams):
            raise ValueError("refine must be a RefineParams")
        if search is None:
            raise ValueError("refine needs search=SearchParams: it refines the plan the search wrote")
        return refine

    def _plan(self, plan_samples, plan_agents, search, agents):
        if plan_samples is None:
            if plan_agents is not None:
                raise ValueError("plan_agents needs plan_samples=r: the agents are given at the fine steps")
            return None
        if search is None:
            raise ValueError("plan_samples needs search=SearchParams: the plan it samples is the search's or the refine's")
        if isinstance(plan_samples, bool) or int(plan_samples) != plan_samples or int(plan_samples) < 1:
            raise ValueError("plan_samples must be a whole number of sub-steps per layer, >= 1")
        r = int(plan_samples)
        layers = np.shape(agents)[2]                                   # (search needs agents: _search has checked that they are there)
        fine = (layers - 1) * r + 1
        if fine > 2 ** 31 - 1:
            raise ValueError(f"plan_samples: (m - 1) r + 1 = {fine} samples per path do not fit an int")
        if plan_agents is not None:
            if not isinstance(plan_agents, _PredictedAgents):
                plan_agents = np.ascontiguousarray(plan_agents, dtype=np.float64)
            want = tuple(np.shape(agents)[:2]) + (fine, AGENT_STRIDE)
            if plan_agents.shape != want:
                raise ValueError(f"plan_agents must be [n_scenes][a_max][(m - 1) r + 1][{AGENT_STRIDE}] = {want}, the scenes and agents of agents=, "
                                 f"not {plan_agents.shape}")
        return (r, plan_agents)

    def _ranking(self, rank, rank_params, winners_only, search, select, batch):
        if rank is None:
            if rank_params is not None:
                raise ValueError("rank_params needs rank=group_start")
            return None
        if search is None:
            raise ValueError("rank needs search=SearchParams: it ranks the trajectories the speed stages finished")
        if select is not None:
            raise ValueError("rank is refused together with select: the speed stages must run on every candidate")
        if rank_params is not None and not isinstance(rank_params, RankParams):
            raise ValueError("rank_params must be a RankParams")
        group_start = np.ascontiguousarray(rank, dtype=np.int32).ravel()
        _check_group_start(group_start, batch)
        return (group_start, rank_params if rank_params is not None else rank_default_params(self.lib), bool(winners_only))

    def _agents(self, agents, agents_of, scene_of, agents_params, sample, samples, car, batch, select, search=None):
        if agents is None:
            if agents_of is not None or scene_of is not None or agents_params is not None:
                raise ValueError("agents_of / scene_of / agents_params need agents=")
            return None
        if sample is None and search is None:
            raise ValueError("agents needs sample=PqpSampleParams: the agents are given at the samples' time steps")
        if not isinstance(agents, _PredictedAgents):
            agents = np.ascontiguousarray(agents, dtype=np.float64)
        if sample is None:                                             # the search alone: the agents' steps are its layers
            if agents.ndim != 4 or agents.shape[0] < 1 or agents.shape[2] < 1 or agents.shape[3] != AGENT_STRIDE:
                raise ValueError(f"agents must be [n_scenes >= 1][a_max][m >= 1][{AGENT_STRIDE}], not {agents.shape}")
        elif agents.ndim != 4 or agents.shape[0] < 1 or agents.shape[2] != int(samples) or agents.shape[3] != AGENT_STRIDE:
            raise ValueError(f"agents must be [n_scenes >= 1][a_max][{int(samples)}][{AGENT_STRIDE}], not {agents.shape}")
        n_scenes = agents.shape[0]
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ravel()
        agents_of, scene_of = i32(agents_of), i32(scene_of)
        if agents_of is not None and agents_of.size != n_scenes:
            raise ValueError(f"agents_of must have one entry per scene ({n_scenes})")
        if scene_of is not None and ((scene_of < 0) | (scene_of >= n_scenes)).any():
            raise ValueError(f"scene_of outside [0, {n_scenes})")
        rows = batch if select is None else np.size(select) - 1          # the rows the sampler runs on
        if scene_of is not None and scene_of.size != rows:
            raise ValueError(f"scene_of must have one entry per {'candidate' if select is None else 'group'} ({rows})")
        return (agents, agents_of, scene_of, agents_params if agents_params is not None else agents_default_params(self.lib), car)

    def _parked(self, parked, map_of, geom):
        """parked= of optimize_path: (agents [n_scenes][a_max][6], base_of or None, inflate) checked, or None"""
        if parked is None:
            return None
        if not isinstance(parked, (tuple, list)) or len(parked) != 3:
            raise ValueError("parked must be (agents, base_of or None, inflate or None)")
        agents, base_of, inflate = parked
        agents = np.ascontiguousarray(agents, dtype=np.float64)
        if agents.ndim != 3 or agents.shape[0] < 1 or agents.shape[2] != AGENT_STRIDE:
            raise ValueError(f"parked: agents must be [n_scenes >= 1][a_max][{AGENT_STRIDE}], not {agents.shape}")
        n_scenes = agents.shape[0]
        if geom is None:
            raise ValueError("parked needs geom: the scenes' layers have its cells")
        base_of = None if base_of is None else np.ascontiguousarray(base_of, dtype=np.int32).ravel()
        if base_of is not None and (base_of.size != n_scenes or (base_of < 0).any()):
            raise ValueError(f"parked: base_of must have one entry >= 0 per scene ({n_scenes})")
        inflate = overlay_default_params(self.lib).inflate if inflate is None else float(inflate)
        if not (np.isfinite(inflate) and inflate >= 0.0):
            raise ValueError(f"parked: inflate must be finite and >= 0, not {inflate}")
        if map_of is not None:
            map_of = np.asarray(map_of)
            if ((map_of < 0) | (map_of >= n_scenes)).any():
                raise ValueError(f"map_of outside [0, {n_scenes}): with parked it indexes the scenes")
        return (agents, base_of, inflate)

    def _previous(self, previous, start, start_k, v_start, batch, select, rank):
        """previous= of optimize_path: (prev, prev_m or None, meas, t_now, StitchParams, group_start or None) checked, or None"""
        if previous is None:
            return None
        if start is not None or start_k is not None or v_start is not None:
            raise ValueError("previous is refused together with start, start_k or v_start: the stitch writes all three on the device")
        if not isinstance(previous, (tuple, list)) or len(previous) != 5:
            raise ValueError("previous must be (prev, prev_m or None, meas, t_now, StitchParams or None)")
        prev, prev_m, meas, t_now, prm = previous
        starts = rank if rank is not None else select
        starts = None if starts is None else np.ascontiguousarray(starts, dtype=np.int32).ravel()
        if starts is not None:
            _check_group_start(starts, batch)
        G, per = (batch, "candidate") if starts is None else (starts.size - 1, "group")
        prev = np.ascontiguousarray(prev, dtype=np.float64)
        if prev.ndim != 3 or prev.shape[0] != G or prev.shape[1] < 1 or prev.shape[2] < TRAJ_STRIDE:
            raise ValueError(f"previous: prev must be [{G}][m >= 1][stride >= {TRAJ_STRIDE}], a plan per {per}, not {prev.shape}")
        prev_m = None if prev_m is None else np.ascontiguousarray(prev_m, dtype=np.int32).ravel()
        meas = np.ascontiguousarray(meas, dtype=np.float64)
        t_now = np.ascontiguousarray(t_now, dtype=np.float64).ravel()
        if (prev_m is not None and prev_m.size != G) or meas.shape != (G, 6) or t_now.size != G:
            raise ValueError(f"previous: prev_m, meas and t_now must be [{G}], [{G}][6] and [{G}], one per {per}")
        if prm is not None and not isinstance(prm, StitchParams):
            raise ValueError("previous: the parameters must be a StitchParams")
        return (prev, prev_m, meas, t_now, prm if prm is not None else stitch_default_params(self.lib), starts)

    def _fallback(self, fallback, previous, ranking, planning, scene_of, map_of):
        """fallback= of optimize_path: (FallbackParams, the plans' scene_of, the plans' map_of or None) checked, or None.  previous,
        ranking and planning are those arguments as checked"""
        if fallback is None or fallback is False:
            return None
        if fallback is not True and not isinstance(fallback, FallbackParams):
            raise ValueError("fallback must be True or a FallbackParams")
        if previous is None or ranking is None:
            raise ValueError("fallback needs previous= and rank=: it brakes along the previous plan, in the groups that end without a winner")
        if planning is not None and planning[1] is None:
            raise ValueError("fallback with plan_samples= needs plan_agents= (or tracks=): its plans are checked on the fine steps")
        prm = fallback_default_params(self.lib) if fallback is True else fallback
        L = prm.level_rows()[0]
        _check_fallback_params("fallback", prm)
        group_start = ranking[0]
        empty = np.flatnonzero(np.diff(group_start) == 0)
        if empty.size:
            raise ValueError(f"fallback: group {int(empty[0])} is empty, so it has no scene to check a braking plan in")
        first = group_start[:-1]
        per_plan = lambda of: None if of is None else np.repeat(np.ascontiguousarray(of, dtype=np.int32).ravel()[first], L)
        plans_scene = per_plan(scene_of)
        return (prm, plans_scene if plans_scene is not None else np.zeros(first.size * L, np.int32), per_plan(map_of))

    def _selection(self, select, select_params, winners_only):
        if select is None:
            if winners_only or select_params is not None:
                raise ValueError("select_params / winners_only need select=group_start")
            return None
        return (np.ascontiguousarray(select, dtype=np.int32), select_params if select_params is not None else select_default_params(self.lib),
                bool(winners_only))

    def _chain_plan(self, **a):
        """optimize_path's arguments by name (what is not given has the signature's default) -> the call laid out, without a device: every
        argument check - the one place the validators above are called from - and then the context c that the stage records read:
          c.args, c.cfg, c.B, c.n_max    the arguments, the chain's configuration, the batch and the waypoints per path
          c.footprint .. c.predicting    each step's checked parameters (planning: r, plan_agents beside it), or None where the call has no such step
          c.parked                       (standing agents' rows, base_of, inflate) of the overlay in front of the chain, or None
          c.previous                     (prev, prev_m, meas, t_now, StitchParams, group_start or None) of the stitch in front of the chain, or None
          c.fallback                     (FallbackParams, scene_of [groups * L], map_of [groups * L] or None) of the braking plans behind the ranking, or None
          c.car                          the footprint of the footprint check and of every check against agents
          c.groups, c.rows, c.paths      the rows of the speed stages - `groups` with select=, else B - and the buffers they run on as (paths,
                                         n_of, stop_before): the winners' best_paths / best_n and no stop, or out / n_out and first_collision
          c.per_candidate                whether those rows are the candidates', which winners_only keeps on the device
          c.samples, c.layers, c.fine    the step counts: the sampler's, the search's m and the fine plan's (m - 1) r + 1
          c.stages                       the records of the call's steps, in launch order
          c.result, c.on_device          (key, shape, dtype) of the returned dict in its order, and the keys winners_only keeps on the device"""
        if not a.keys() <= _CHAIN_ARGS.keys():
            raise TypeError(f"optimize_path has no argument {', '.join(sorted(a.keys() - _CHAIN_ARGS.keys()))}")
        a = types.SimpleNamespace(**{**_CHAIN_ARGS, **a})
        B = np.shape(a.points)[0]
        predicting, agents, plan_agents = self._tracks(a.tracks, a.layers, a.predict_anchor, a.search, a.agents, a.plan_agents, a.plan_samples)
        c = types.SimpleNamespace(
            args=a, B=B, predicting=predicting, footprint=int(a.footprint_mode) if a.check_footprint else None,
            selection=self._selection(a.select, a.select_params, a.winners_only and a.rank is None),
            speed=self._speed(a.speed, a.v_start, a.v_end, a.check_footprint, a.select, a.select_params, a.previous),
            previous=self._previous(a.previous, a.start, a.start_k, a.v_start, B, a.select, a.rank),
            sampling=self._sample(a.sample, a.samples, a.t0, a.speed),
            moving=self._agents(agents, a.agents_of, a.scene_of, a.agents_params, a.sample, a.samples, a.car, B, a.select, a.search),
            searching=self._search(a.search, a.speed, agents), refining=self._refine(a.refine, a.search),
            planning=self._plan(a.plan_samples, plan_agents, a.search, agents),
            ranking=self._ranking(a.rank, a.rank_params, a.winners_only, a.search, a.select, B),
            parked=self._parked(a.parked, a.map_of, a.geom))
        c.fallback = self._fallback(a.fallback, c.previous, c.ranking, c.planning, a.scene_of, a.map_of)
        c.planning, c.plan_agents = c.planning or (None, None)         # r, and the agents' fine rows or their shape
        c.cfg = a.cfg or _defaults(self.lib, PqpChainConfig, "pqp_chain_default_config", {})
        c.n_max = c.cfg.n_max
        if c.selection is not None:
            _check_group_start(c.selection[0], B)
        c.groups = None if c.selection is None else c.selection[0].size - 1          # (one or more: group_start runs from 0 to B)
        c.per_candidate = c.selection is None
        c.rows, per = (B, "candidate") if c.per_candidate else (c.groups, "group")
        c.paths = ("out", "n_out", None if c.footprint is None else "first_collision") if c.per_candidate else ("best_paths", "best_n", None)
        if c.speed is not None and ((c.speed[1] is not None and c.speed[1].size != c.rows) or (c.speed[2] is not None and c.speed[2].size != c.rows)):
            raise ValueError(f"v_start / v_end must have one entry per {per} ({c.rows})")
        if c.sampling is not None and c.sampling[2] is not None and c.sampling[2].size != c.rows:
            raise ValueError(f"t0 must have one entry per {per} ({c.rows})")
        needs_car = c.footprint is not None or c.moving is not None
        c.car = car_default_geometry(self.lib) if needs_car and a.car is None else a.car
        c.samples = None if c.sampling is None else c.sampling[1]
        c.layers = None if c.searching is None else c.moving[0].shape[2]
        c.fine = None if c.planning is None else (c.layers - 1) * c.planning + 1
        have = vars(c)
        records = {f: f(c) for f, needs in _STAGES if all(have[n] is not None for n in needs)}
        c.stages = list(records.values())
        outputs = [o for f in _RESULT_ORDER if f in records for o in records[f].outputs]
        winners = bool(a.winners_only)
        c.result = [o[:3] for o in outputs if not (winners and o[3])]
        c.on_device = [o[0] for o in outputs if winners and o[3]]
        return c

    def _chain(self, c, maps, layer_dtype, build):
        """runs the call _chain_plan laid out.  maps: [n_maps][rows][cols] (or 2-D), uploaded in the ABI's column-major order as layer_dtype;
        build(d_grid, d_dist): enqueues the float layer from them on the handle's stream (None: they are the layer)"""
        import torch
        dev = torch.device("cuda", self.device)
        t = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
        d = dict(layer=t(_column_major(maps, layer_dtype), layer_dtype))
        if c.parked is not None:            # what pqp_overlay_agents refuses and the plan, which has no maps, cannot see
            n_maps, (ag, base_of, _) = d["layer"].shape[0], c.parked
            if base_of is None and n_maps != 1 and n_maps != ag.shape[0]:
                raise ValueError(f"parked: base_of=None needs one map or one per scene ({ag.shape[0]}), not {n_maps}")
            if base_of is not None and (base_of >= n_maps).any():
                raise ValueError(f"parked: base_of outside [0, {n_maps})")
        # base: the layers as uploaded or built; dist: what the chain and the footprint check read - the same, or with parked= the
        # scenes' layers, which the overlay's record lays out under that name
        d["dist"] = d["base"] = d["layer"] if build is None else torch.empty(d["layer"].shape, dtype=torch.float32, device=dev)
        for s in c.stages:
            for name, x, dt in s.uploads:
                if x is not None or name not in d:          # nothing to upload: what an earlier stage laid out under that name stays
                    d[name] = t(x, dt)
            for name, shape, dtype, _ in s.outputs:
                d[name] = torch.zeros(shape, dtype=getattr(torch, dtype), device=dev)
            for name, shape, dtype, *how in s.scratch:
                d[name] = (torch.empty if how else torch.zeros)(shape, dtype=getattr(torch, dtype), device=dev)
        torch.cuda.synchronize(dev)         # the one fence between torch's stream and the handle's: nothing is created after it
        if build is not None:
            build(d["layer"], d["base"])
        for s in c.stages:
            s.launch(self, c, d)
        self.sync()
        if c.args.smoother is not None:
            c.args.smoother.sync()
        return {key: d[key].cpu().numpy() for key, _, _ in c.result}

    def distance_layer(self, grid, geom):
        """pqp_distance_layer (host arrays): grid [n_maps][rows][cols] (or 2-D) uint8, 0 = obstacle, in the orientation corridor_bounds takes
        its layer -> the float32 distance layer [n_maps][rows][cols] (2-D in, 2-D out)."""
        two_d = np.ndim(grid) == 2
        cm = _column_major(_occupancy(grid, "distance_layer"), np.uint8)
        out = np.empty(cm.shape, dtype=np.float32)
        self._check(self.lib.pqp_distance_layer(self._h, cm.shape[0], C.byref(geom), cm, out))
        out = np.transpose(out, (0, 2, 1))
        return out[0] if two_d else out

    def overlay_agents(self, dist, geom, agents, a_of=None, base_of=None, inflate=None):
        """pqp_overlay_agents (host arrays): dist [n_maps][rows][cols] (or 2-D) float32, the base layers in distance_layer's orientation,
        geom = PqpGridGeometry, agents [n_scenes][a_max][6] = x, y, heading, half_length, half_width, radius of the scenes' standing agents
        (half_length or half_width < 0: absent), and optionally a_of [n_scenes] (agents per scene), base_of [n_scenes] (the layer a scene
        starts from; None: layer 0 of one, else layer s of n_scenes), inflate in m (None: overlay_default_params()).  Returns (layers
        [n_scenes][rows][cols] float32 = min(base layer, distance to the scene's agents), flags [n_scenes] of OVERLAY_*)."""
        cm = _column_major(dist, np.float32)
        agents = np.ascontiguousarray(agents, dtype=np.float64)
        if agents.ndim != 3 or agents.shape[2] != AGENT_STRIDE:
            raise ValueError(f"overlay_agents: agents must be [n_scenes][a_max][{AGENT_STRIDE}], not {agents.shape}")
        n_scenes, a_max = agents.shape[:2]
        ao, bo = _i32(a_of), _i32(base_of)
        _check_sizes("overlay_agents", ("a_of", ao, n_scenes), ("base_of", bo, n_scenes))
        inflate = overlay_default_params(self.lib).inflate if inflate is None else float(inflate)
        out = np.empty((n_scenes,) + cm.shape[1:], dtype=np.float32)
        flags = np.zeros(n_scenes, dtype=np.int32)
        self._check(self.lib.pqp_overlay_agents(self._h, inflate, cm.shape[0], C.byref(geom), cm, n_scenes, a_max, agents if agents.size else None,
                                                ao, bo, out, flags))
        return np.transpose(out, (0, 2, 1)), flags

    def footprint_check(self, states, n_of, dist, geom, map_of=None, car=None, mode=FOOTPRINT_CIRCLES, margin=False):
        """pqp_footprint_check (host arrays): states [B][n][stride >= 3] (x, y, heading first; the chain's `out` as it is), n_of [B] or None,
        dist [n_maps][rows][cols] float32 (converted to the ABI's column-major order here), geom = PqpGridGeometry, car = PqpCarGeometry
        (None: the reference's), mode = FOOTPRINT_CIRCLES / FOOTPRINT_BOUNDING_FIRST.  Returns dict(free [B][n] uint8, first_collision [B]
        [, margin [B][n]])."""
        states = np.ascontiguousarray(states, dtype=np.float64)
        dist_cm = _column_major(dist, np.float32)
        B, n, stride = states.shape
        no, mo = _i32(n_of), _i32(map_of)
        car = car if car is not None else car_default_geometry(self.lib)
        free = np.zeros((B, n), dtype=np.uint8)
        first = np.zeros(B, dtype=np.int32)
        mg = np.zeros((B, n)) if margin else None
        self._check(self.lib.pqp_footprint_check(self._h, B, n, stride, states, no, dist_cm, dist_cm.shape[0], mo, C.byref(geom),
                                                 C.byref(car), int(mode), free, first, mg))
        res = dict(free=free, first_collision=first)
        if margin:
            res["margin"] = mg
        return res

    def select_paths(self, paths, group_start, n_of=None, status=None, stage=None, first_collision=None, margin=None, prm=None):
        """pqp_select_paths (host arrays): paths [B][n][stride >= 7] (the chain's `out` as it is), group_start [groups + 1] (ascending, 0 ..
        B), the optional per-candidate arrays the chain and the footprint check wrote, prm = PqpSelectParams (None: the defaults).  Returns
        dict(terms [B][8], best [groups], best_paths [groups][n][7], best_n [groups])."""
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        B, n, stride = paths.shape
        gs = np.ascontiguousarray(group_start, dtype=np.int32).ravel()
        _check_group_start(gs, B)
        groups = gs.size - 1
        no, stt, stg, fc = _i32(n_of), _i32(status), _i32(stage), _i32(first_collision)
        mg = _f64(margin)
        prm = prm if prm is not None else select_default_params(self.lib)
        terms = np.zeros((B, SCORE_STRIDE))
        best = np.zeros(groups, dtype=np.int32)
        best_paths = np.zeros((groups, n, 7))
        best_n = np.zeros(groups, dtype=np.int32)
        self._check(self.lib.pqp_select_paths(self._h, C.byref(prm), B, n, stride, paths, no, stt, stg, fc, mg,
                                              groups, gs, terms, best, best_paths, best_n))
        return dict(terms=terms, best=best, best_paths=best_paths, best_n=best_n)

    def speed_profile(self, paths, v_start, n_of=None, stop_before=None, v_limit=None, v_end=None, prm=None):
        """pqp_speed_profile (host arrays): paths [B][n][stride >= 6] (x, y first, k at offset 5; the chain's `out` or best_paths as they are),
        v_start [B], and optionally n_of [B], stop_before [B] (e.g. first_collision), v_limit [B][n], v_end [B] (NaN: free); prm =
        PqpSpeedParams (None: the defaults).  Returns (profile [B][n][4] = s, v, a, t, flags [B] of SPEED_*)."""
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        B, n, stride = paths.shape
        no, sb, vl, vs, ve = _i32(n_of), _i32(stop_before), _f64(v_limit), _f64(v_start), _f64(v_end)
        _check_sizes("speed_profile", ("n_of", no, B), ("stop_before", sb, B), ("v_limit", vl, B * n), ("v_start", vs, B), ("v_end", ve, B))
        prm = prm if prm is not None else speed_default_params(self.lib)
        profile = np.zeros((B, n, SPEED_STRIDE))
        flags = np.zeros(B, dtype=np.int32)
        self._check(self.lib.pqp_speed_profile(self._h, C.byref(prm), B, n, stride, paths, no, sb, vl, vs, ve,
                                               profile, flags))
        return profile, flags

    def sample_trajectory(self, paths, profile, m, n_of=None, stop_before=None, t0=None, prm=None):
        """pqp_sample_trajectory (host arrays): paths [B][n][stride >= 6] (x, y, heading first, k at offset 5; the chain's `out` or best_paths
        as they are), profile [B][n][4] = s, v, a, t (speed_profile's), m samples per path at t0 + k dt, and optionally n_of [B], stop_before
        [B] (the two speed_profile got), t0 [B] (None: all 0); prm = PqpSampleParams (None: the defaults).  Returns (traj [B][m][8] = x, y,
        heading, k, s, v, a, t, m_of [B]: the samples on the path, flags [B] of TRAJ_*)."""
        paths, profile, (B, n, stride) = _paths_with_profile("sample_trajectory", paths, profile)
        m = int(m)
        no, sb, tt = _i32(n_of), _i32(stop_before), _f64(t0)
        _check_sizes("sample_trajectory", ("n_of", no, B), ("stop_before", sb, B), ("t0", tt, B))
        prm = prm if prm is not None else sample_default_params(self.lib)
        traj = np.zeros((B, max(m, 0), TRAJ_STRIDE))
        m_of = np.zeros(B, dtype=np.int32)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self.lib.pqp_sample_trajectory(self._h, C.byref(prm), B, n, stride, paths, no, sb, profile, tt, m,
                                                   traj, m_of, flags))
        return traj, m_of, flags

    def agents_check(self, traj, agents, m_of=None, a_of=None, scene_of=None, car=None, prm=None, clearance=False):
        """pqp_agents_check (host arrays): traj [B][m][stride >= 3] (x, y, heading first; sample_trajectory's traj as it is), agents
        [n_scenes][a_max][m][6] = x, y, heading, half_length, half_width, radius at the same m time steps (half_length or half_width < 0:
        absent at that step), and optionally m_of [B] (the samples to check; None: all), a_of [n_scenes] (agents per scene), scene_of [B]
        (None: scene 0); car = PqpCarGeometry (None: the reference's), prm = AgentsParams (None: agents_default_params()).  Returns
        dict(first_hit [B], hit_agent [B][, clearance [B][m]])."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        B, m, stride = traj.shape
        agents = np.ascontiguousarray(agents, dtype=np.float64)
        if agents.ndim != 4 or agents.shape[2:] != (m, AGENT_STRIDE):
            raise ValueError(f"agents_check: agents must be [n_scenes][a_max][{m}][{AGENT_STRIDE}], not {agents.shape}")
        n_scenes, a_max = agents.shape[:2]
        mo, ao, so = _i32(m_of), _i32(a_of), _i32(scene_of)
        _check_sizes("agents_check", ("m_of", mo, B), ("a_of", ao, n_scenes), ("scene_of", so, B))
        car = car if car is not None else car_default_geometry(self.lib)
        prm = prm if prm is not None else agents_default_params(self.lib)
        first = np.zeros(B, dtype=np.int32)
        who = np.zeros(B, dtype=np.int32)
        cl = np.zeros((B, m)) if clearance else None
        self._check(self.lib.pqp_agents_check(self._h, float(prm.margin), C.byref(car), B, m, stride, traj, mo, n_scenes, a_max,
                                              agents if agents.size else None, ao, so, first, who, cl))
        res = dict(first_hit=first, hit_agent=who)
        if clearance:
            res["clearance"] = cl
        return res

    def predict_agents(self, tracks, t0=0.0, dt=1.0, m=1, r=1, a_of=None, lane_of=None, lanes=None, prm=None, anchor=False):
        """pqp_predict_agents (host arrays): tracks [n_scenes][a_max][9] = x, y, heading, v, a, yaw_rate, half_length, half_width, radius
        -> the agents' rows at m layers dt apart from t0 on, r sub-steps per layer; optionally a_of [n_scenes] (agents per scene), lane_of
        [n_scenes][a_max] (the lane a track follows; < 0 or None: the free model) with lanes = (spline [n_lanes][9][lane_m], spline_ext
        [n_lanes][4], length [n_lanes]) as spline_fit returns and project_points takes them; prm = PredictParams (None:
        predict_default_params()).  Returns dict(agents [n_scenes][a_max][(m - 1) r + 1][6], flags [n_scenes][a_max] of PREDICT_*[, anchor
        [n_scenes][a_max][4] = s0, l0, dir, heading error])."""
        tracks = np.ascontiguousarray(tracks, dtype=np.float64)
        if tracks.ndim != 3 or tracks.shape[2] != TRACK_STRIDE:
            raise ValueError(f"predict_agents: tracks must be [n_scenes][a_max][{TRACK_STRIDE}], not {tracks.shape}")
        n_scenes, a_max = tracks.shape[:2]
        ao, lo = _i32(a_of), _i32(lane_of)
        _check_sizes("predict_agents", ("a_of", ao, n_scenes), ("lane_of", lo, n_scenes * a_max))
        n_lanes, lane_m, spl, ext, length = _lanes(lanes, "predict_agents")
        prm = prm if prm is not None else predict_default_params(self.lib)
        m, r = int(m), int(r)
        M = max(m - 1, 0) * max(r, 0) + 1
        if M > 2 ** 31 - 1:
            raise ValueError(f"predict_agents: (m - 1) r + 1 = {M} steps do not fit an int")
        agents = np.zeros((n_scenes, a_max, M, AGENT_STRIDE))
        flags = np.zeros((n_scenes, a_max), dtype=np.int32)
        anc = np.zeros((n_scenes, a_max, ANCHOR_STRIDE)) if anchor else None
        self._check(self.lib.pqp_predict_agents(self._h, prm.array(), float(t0), float(dt), m, r, n_scenes, a_max, tracks, ao, lo, n_lanes, lane_m,
                                                spl, ext, length, agents, anc, flags))
        res = dict(agents=agents, flags=flags)
        if anchor:
            res["anchor"] = anc
        return res

    def speed_search(self, paths, profile, v_start, agents, m=None, n_of=None, stop_before=None, a_of=None, scene_of=None, car=None, prm=None,
                     blocked=False):
        """pqp_speed_search (host arrays): paths [B][n][stride >= 6] (the chain's `out` or best_paths as they are), profile [B][n][4] = s, v,
        a, t (speed_profile's), v_start [B], agents [n_scenes][a_max][m][6] at the m layers' times k dt (m=None: the agents' step count;
        without agents, a_max = 0, m must be given), and optionally n_of [B], stop_before [B] (the two speed_profile got), a_of [n_scenes],
        scene_of [B] (None: scene 0); car = PqpCarGeometry (None: the reference's), prm = SearchParams (None: search_default_params()).
        Returns dict(steps [B][m][2] = j, q, traj [B][m][8], cost [B], reached [B], flags [B] of SEARCH_*[, blocked [B][m][W] int32])."""
        paths, profile, (B, n, stride) = _paths_with_profile("speed_search", paths, profile)
        agents = np.ascontiguousarray(agents, dtype=np.float64)
        if agents.ndim != 4 or agents.shape[3] != AGENT_STRIDE or (m is not None and agents.shape[2] != int(m)):
            raise ValueError(f"speed_search: agents must be [n_scenes][a_max][{'m' if m is None else int(m)}][{AGENT_STRIDE}], not {agents.shape}")
        m = agents.shape[2] if m is None else int(m)
        n_scenes, a_max = agents.shape[:2]
        no, sb, ao, so = _i32(n_of), _i32(stop_before), _i32(a_of), _i32(scene_of)
        vs = np.ascontiguousarray(v_start, dtype=np.float64)
        _check_sizes("speed_search", ("n_of", no, B), ("stop_before", sb, B), ("v_start", vs, B), ("a_of", ao, n_scenes), ("scene_of", so, B))
        car = car if car is not None else car_default_geometry(self.lib)
        prm = prm if prm is not None else search_default_params(self.lib)
        rows = max(m, 0)
        steps = np.zeros((B, rows, 2), dtype=np.int32)
        traj = np.zeros((B, rows, TRAJ_STRIDE))
        cost = np.zeros(B)
        reached = np.zeros(B, dtype=np.int32)
        flags = np.zeros(B, dtype=np.int32)
        blk = np.zeros((B, rows, (max(int(prm.stations), 0) + 31) // 32), dtype=np.int32) if blocked else None
        self._check(self.lib.pqp_speed_search(self._h, C.byref(prm), C.byref(car), B, n, stride, paths, no, sb, profile, vs, m, n_scenes, a_max,
                                              agents if agents.size else None, ao, so, blk, steps, traj, cost, reached, flags))
        res = dict(steps=steps, traj=traj, cost=cost, reached=reached, flags=flags)
        if blocked:
            res["blocked"] = blk
        return res

    def speed_refine(self, paths, profile, v_start, blocked, steps, reached, search_traj, n_of=None, stop_before=None, grid=None, prm=None):
        """pqp_speed_refine (host arrays): paths [B][n][stride >= 6], profile [B][n][4], v_start [B] and optionally n_of [B], stop_before [B]
        as speed_search got them; blocked [B][m][W], steps [B][m][2], reached [B] and search_traj [B][m][8] as it returned them (its
        blocked=True); grid = the search's SearchParams (None: search_default_params()), prm = RefineParams (None:
        refine_default_params()).  Returns dict(traj [B][m][8], bounds [B][m][3] = lo, hi, vcap, cost [B], excess [B], status [B], iters
        [B], flags [B] of REFINE_*)."""
        paths, profile, (B, n, stride) = _paths_with_profile("speed_refine", paths, profile)
        grid = grid if grid is not None else search_default_params(self.lib)
        prm = prm if prm is not None else refine_default_params(self.lib)
        search_traj = np.ascontiguousarray(search_traj, dtype=np.float64)
        if search_traj.ndim != 3 or search_traj.shape[0] != B or search_traj.shape[2] != TRAJ_STRIDE:
            raise ValueError(f"speed_refine: search_traj must be [{B}][m][{TRAJ_STRIDE}], not {search_traj.shape}")
        m = search_traj.shape[1]
        no, sb, blk, stp, rch = _i32(n_of), _i32(stop_before), _i32(blocked), _i32(steps), _i32(reached)
        vs = np.ascontiguousarray(v_start, dtype=np.float64)
        words = (max(int(grid.stations), 0) + 31) // 32
        _check_sizes("speed_refine", ("n_of", no, B), ("stop_before", sb, B), ("v_start", vs, B), ("blocked", blk, B * m * words), ("steps", stp, B * m * 2),
                     ("reached", rch, B))
        traj = np.zeros((B, m, TRAJ_STRIDE))
        bounds = np.zeros((B, m, 3))
        cost, excess = np.zeros(B), np.zeros(B)
        status, iters, flags = (np.zeros(B, dtype=np.int32) for _ in range(3))
        self._check(self.lib.pqp_speed_refine(self._h, C.byref(grid), prm.array(), int(prm.window), B, n, stride, paths, no, sb, profile, vs, m, blk,
                                              stp, rch, search_traj, traj, bounds, cost, excess, status, iters, flags))
        return dict(traj=traj, bounds=bounds, cost=cost, excess=excess, status=status, iters=iters, flags=flags)

    def sample_plan(self, paths, profile, plan, r, dt=1.0, n_of=None, stop_before=None, count_of=None, refine_flags=None, linear=False):
        """pqp_sample_plan (host arrays): paths [B][n][stride >= 6], profile [B][n][4] and optionally n_of [B], stop_before [B] as
        speed_search and speed_refine got them; plan [B][m][8]: the traj either of them returned, dt the grid's; r sub-steps per layer;
        count_of [B]: the planned layers (the search's reached; None: m); refine_flags [B]: speed_refine's flags - a REFINED path is sampled
        under constant acceleration, every other path linearly (None: every path by `linear`).  Returns dict(traj [B][(m - 1) r + 1][8],
        m_of [B]: the samples on the plan, defect [B], excess [B], flags [B] of PLAN_*)."""
        paths, profile, (B, n, stride) = _paths_with_profile("sample_plan", paths, profile)
        plan = np.ascontiguousarray(plan, dtype=np.float64)
        if plan.ndim != 3 or plan.shape[0] != B or plan.shape[2] != TRAJ_STRIDE:
            raise ValueError(f"sample_plan: plan must be [{B}][m][{TRAJ_STRIDE}], not {plan.shape}")
        m, r = plan.shape[1], int(r)
        no, sb, co, rfl = _i32(n_of), _i32(stop_before), _i32(count_of), _i32(refine_flags)
        _check_sizes("sample_plan", ("n_of", no, B), ("stop_before", sb, B), ("count_of", co, B), ("refine_flags", rfl, B))
        M = max(m - 1, 0) * max(r, 0) + 1
        if M > 2 ** 31 - 1:
            raise ValueError(f"sample_plan: (m - 1) r + 1 = {M} samples per path do not fit an int")
        traj = np.zeros((B, M, TRAJ_STRIDE))
        m_of, flags = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        defect, excess = np.zeros(B), np.zeros(B)
        self._check(self.lib.pqp_sample_plan(self._h, float(dt), r, int(linear), B, n, stride, paths, no, sb, profile, m, plan, co, rfl, traj, m_of,
                                             defect, excess, flags))
        return dict(traj=traj, m_of=m_of, defect=defect, excess=excess, flags=flags)

    def select_plans(self, traj, group_start, m_of=None, path_terms=None, search_flags=None, first_hit=None, clearance=None, paths=None, n_of=None,
                     prm=None):
        """pqp_select_plans (host arrays): traj [B][m][stride >= 8] (sample_plan's, speed_refine's or speed_search's traj as it is),
        group_start [groups + 1] (ascending, 0 .. B), and optionally m_of [B] (the rows of each: sample_plan's m_of or the search's reached),
        path_terms [B][8] (select_paths' terms), search_flags [B], first_hit [B] and clearance [B][m] (agents_check's on these rows), paths
        [B][n][path_stride >= 7] with n_of [B] (the waypoints to gather for the winners); prm = RankParams (None: rank_default_params()).
        Returns dict(terms [B][10], best [groups], best_traj [groups][m][8], best_m [groups][, best_paths [groups][n][7], best_n [groups]])."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        if traj.ndim != 3:
            raise ValueError(f"select_plans: traj must be [B][m][stride], not {traj.shape}")
        B, m, stride = traj.shape
        gs = np.ascontiguousarray(group_start, dtype=np.int32).ravel()
        _check_group_start(gs, B)
        groups = gs.size - 1
        mo, sf, fh, no, pt, cl, pa = _i32(m_of), _i32(search_flags), _i32(first_hit), _i32(n_of), _f64(path_terms), _f64(clearance), _f64(paths)
        if pa is not None and pa.ndim != 3:
            raise ValueError(f"select_plans: paths must be [B][n][path_stride], not {pa.shape}")
        n, path_stride = (0, 0) if pa is None else pa.shape[1:]
        if no is not None and pa is None:
            raise ValueError("select_plans: n_of needs paths")
        _check_sizes("select_plans", ("m_of", mo, B), ("search_flags", sf, B), ("first_hit", fh, B), ("n_of", no, B), ("path_terms", pt, B * SCORE_STRIDE),
                     ("clearance", cl, B * m), ("paths", pa, B * n * path_stride))
        prm = prm if prm is not None else rank_default_params(self.lib)
        terms = np.zeros((B, PLAN_SCORE_STRIDE))
        best, best_m = np.zeros(groups, dtype=np.int32), np.zeros(groups, dtype=np.int32)
        best_traj = np.zeros((groups, m, TRAJ_STRIDE))
        best_paths = None if pa is None else np.zeros((groups, n, 7))
        best_n = None if pa is None else np.zeros(groups, dtype=np.int32)
        self._check(self.lib.pqp_select_plans(self._h, prm.array(), int(prm.require_free), B, m, stride, traj, mo, pt, sf, fh, cl, n, path_stride,
                                              pa, no, groups, gs, terms, best, best_traj, best_m, best_paths, best_n))
        res = dict(terms=terms, best=best, best_traj=best_traj, best_m=best_m)
        if pa is not None:
            res.update(best_paths=best_paths, best_n=best_n)
        return res

    def stitch_trajectory(self, prev, meas, t_now, m_of=None, group_start=None, batch=None, prm=None, prefix_max=None):
        """pqp_stitch_trajectory (host arrays): prev [G][m][stride >= 8] = x, y, heading, k, s, v, a, t (select_plans' best_traj, sample_plan's
        or sample_trajectory's rows as they are), meas [G][6] = x, y, heading, v, a, yaw rate, t_now [G] in the plan's time base, and
        optionally m_of [G] (the rows of each plan: best_m), group_start [groups + 1] with batch (the candidates of each group; None: one
        candidate per group), prm = StitchParams (None: stitch_default_params()), prefix_max (the rows of prefix; None: m).  Returns
        dict(state [G][8], flags [G] of STITCH_*, dev [G][3] = lon, lat, dh, idx [G][3] = i_now, p, i_start, prefix [G][prefix_max][8],
        prefix_n [G], start [batch][3], start_k [batch], v_start [batch])."""
        prev = np.ascontiguousarray(prev, dtype=np.float64)
        if prev.ndim != 3:
            raise ValueError(f"stitch_trajectory: prev must be [G][m][stride], not {prev.shape}")
        G, m, stride = prev.shape
        meas, tn, mo = _f64(meas), _f64(t_now), _i32(m_of)
        if meas.shape != (G, 6):
            raise ValueError(f"stitch_trajectory: meas must be {(G, 6)}, not {meas.shape}")
        _check_sizes("stitch_trajectory", ("t_now", tn, G), ("m_of", mo, G))
        gs = None
        if group_start is not None:
            gs = np.ascontiguousarray(group_start, dtype=np.int32).ravel()
            if batch is None or gs.size != G + 1:
                raise ValueError(f"stitch_trajectory: group_start needs batch and {G + 1} entries")
            _check_group_start(gs, int(batch))
        batch = G if batch is None else int(batch)
        prm = prm if prm is not None else stitch_default_params(self.lib)
        prefix_max = m if prefix_max is None else int(prefix_max)
        res = dict(state=np.zeros((G, TRAJ_STRIDE)), flags=np.zeros(G, dtype=np.int32), dev=np.zeros((G, 3)), idx=np.zeros((G, 3), dtype=np.int32),
                   prefix=np.zeros((G, max(prefix_max, 0), TRAJ_STRIDE)), prefix_n=np.zeros(G, dtype=np.int32), start=np.zeros((batch, 3)),
                   start_k=np.zeros(batch), v_start=np.zeros(batch))
        self._check(self.lib.pqp_stitch_trajectory(self._h, prm.array(), int(prm.keep), prefix_max, G, m, stride, prev, mo, meas, tn, batch, gs,
                                                   res["state"], res["flags"], res["dev"], res["idx"], res["prefix"], res["prefix_n"], res["start"],
                                                   res["start_k"], res["v_start"]))
        return res

    def fallback_rows(self, state, m, dt=1.0, r=1, prev=None, prev_m=None, stitch_flags=None, prm=None):
        """pqp_fallback_rows (host arrays): state [G][8] (stitch_trajectory's state), m layers of dt with r sub-steps each (M = (m - 1) r + 1
        rows per plan), and optionally prev [G][mp][stride >= 8] with prev_m [G] (the plan the stitch read; None: every group brakes on its
        arc), stitch_flags [G] (the stitch's; None: all stitched), prm = FallbackParams (None: fallback_default_params()).  Returns
        dict(rows [G][L][M][8], stop [G][L][2] = T, e(T), stop_row [G][L], flags [G][L] of FALLBACK_*)."""
        state = _f64(state)
        if state.ndim != 2 or state.shape[1] != TRAJ_STRIDE:
            raise ValueError(f"fallback_rows: state must be [G][{TRAJ_STRIDE}], not {state.shape}")
        G = state.shape[0]
        prev, pm, sf = _f64(prev), _i32(prev_m), _i32(stitch_flags)
        if prev is not None and (prev.ndim != 3 or prev.shape[0] != G):
            raise ValueError(f"fallback_rows: prev must be [{G}][mp][stride], not {prev.shape}")
        if prev is None and pm is not None:
            raise ValueError("fallback_rows: prev_m needs prev")
        _check_sizes("fallback_rows", ("prev_m", pm, G), ("stitch_flags", sf, G))
        mp, stride = (0, 0) if prev is None else prev.shape[1:]
        prm = prm if prm is not None else fallback_default_params(self.lib)
        L, levels = prm.level_rows()
        m, r = int(m), int(r)
        M = max(m - 1, 0) * max(r, 0) + 1
        if M > 2 ** 31 - 1 - 64:
            raise ValueError(f"fallback_rows: (m - 1) r + 1 = {M} rows per plan do not fit an int (less a tile of 64)")
        res = dict(rows=np.zeros((G, L, M, TRAJ_STRIDE)), stop=np.zeros((G, L, 2)), stop_row=np.zeros((G, L), dtype=np.int32),
                   flags=np.zeros((G, L), dtype=np.int32))
        self._check(self.lib.pqp_fallback_rows(self._h, prm.array(), L, levels, float(dt), r, m, G, mp, stride, prev, pm, state, sf, res["rows"],
                                               res["stop"], res["stop_row"], res["flags"]))
        return res

    def fallback_pick(self, rows, row_flags, best=None, best_traj=None, best_m=None, first_hit=None, first_collision=None):
        """pqp_fallback_pick (host arrays): rows [G][L][M][8] and row_flags [G][L] as fallback_rows returned them, and optionally best [G]
        (select_plans' winners; None: every group falls back), best_traj [G][M][8] with best_m [G] (both or neither), first_hit [G * L]
        and first_collision [G * L] (agents_check's and footprint_check's verdicts on the G * L plans; None: not checked).  Returns
        dict(final_traj [G][M][8], final_m [G], level [G], flags [G] of FALLBACK_*): what the next cycle passes as prev and prev_m."""
        rows = _f64(rows)
        if rows.ndim != 4 or rows.shape[3] != TRAJ_STRIDE:
            raise ValueError(f"fallback_pick: rows must be [G][L][M][{TRAJ_STRIDE}], not {rows.shape}")
        G, L, M = rows.shape[:3]
        rf, b, bt, bm, fh, fc = _i32(row_flags), _i32(best), _f64(best_traj), _i32(best_m), _i32(first_hit), _i32(first_collision)
        if (bt is None) != (bm is None):
            raise ValueError("fallback_pick: best_traj and best_m go together")
        _check_sizes("fallback_pick", ("row_flags", rf, G * L), ("best", b, G), ("best_traj", bt, G * M * TRAJ_STRIDE), ("best_m", bm, G),
                     ("first_hit", fh, G * L), ("first_collision", fc, G * L))
        res = dict(final_traj=np.zeros((G, M, TRAJ_STRIDE)), final_m=np.zeros(G, dtype=np.int32), level=np.zeros(G, dtype=np.int32),
                   flags=np.zeros(G, dtype=np.int32))
        self._check(self.lib.pqp_fallback_pick(self._h, G, L, M, b, bt, bm, rows, rf, fh, fc, res["final_traj"], res["final_m"], res["level"],
                                               res["flags"]))
        return res

    def corridor_params(self, **over):
        return _defaults(self.lib, PqpCorridorParams, "pqp_corridor_default_params", over)

    def dp_corridor(self, spline, spline_ext, length, start, dist, geom, max_layers=128, map_of=None, prm=None):
        """pqp_dp_corridor (host arrays) -> (layers_s [B][max_layers], lb, ub, count [B], vehicle_l [B])."""
        spline = np.ascontiguousarray(spline, dtype=np.float64); spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        length = np.ascontiguousarray(length, dtype=np.float64); start = np.ascontiguousarray(start, dtype=np.float64)
        dist_cm = _column_major(dist, np.float32)
        B, m = spline.shape[0], spline.shape[2]
        ls = np.zeros((B, max_layers)); lb = np.zeros((B, max_layers)); ub = np.zeros((B, max_layers))
        count = np.zeros(B, dtype=np.int32); vl = np.zeros(B)
        mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
        if prm is None:
            prm = _defaults(self.lib, PqpDpParams, "pqp_dp_default_params", {})
        self._check(self.lib.pqp_dp_corridor(self._h, B, m, max_layers, spline, spline_ext, length, start, dist_cm,
                                             dist_cm.shape[0], mo, C.byref(geom), C.byref(prm), ls, lb, ub, count, vl))
        return ls, lb, ub, count, vl

    def spline_fit(self, s, x, y):
        """pqp_spline_fit (host arrays [B][m]) -> (spline [B][9][m], spline_ext [B][4])."""
        s = np.ascontiguousarray(s, dtype=np.float64); x = np.ascontiguousarray(x, dtype=np.float64); y = np.ascontiguousarray(y, dtype=np.float64)
        B, m = s.shape
        tab = np.zeros((B, 9, m)); ext = np.zeros((B, 4))
        self._check(self.lib.pqp_spline_fit(self._h, B, m, s, x, y, tab, ext))
        return tab, ext

    def reference_states(self, spline, spline_ext, max_s, n_max, start=None, ds_small=0.15, ds_large=0.3, dynamic=True):
        """pqp_reference_states (host arrays): spline [B][9][m], spline_ext [B][4], max_s [B], start [B][3] or None.
        Returns (ref [B][n_max][5], count [B], init_err [B][2] or None)."""
        spline = np.ascontiguousarray(spline, dtype=np.float64)
        spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        max_s = np.ascontiguousarray(max_s, dtype=np.float64)
        B, m = spline.shape[0], spline.shape[2]
        st = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
        ref = np.zeros((B, n_max, 5)); count = np.zeros(B, dtype=np.int32)
        err = None if start is None else np.zeros((B, 2))
        self._check(self.lib.pqp_reference_states(self._h, B, n_max, m, spline, spline_ext, max_s, st, ds_small,
                                                  ds_large, 1 if dynamic else 0, ref, count, err))
        return ref, count, err

    def offsets_to_points(self, spline, spline_ext, at_s, l, m_of=None):
        """pqp_offsets_to_points (host arrays): spline [B][9][m_spline], at_s, l [B][m], m_of [B] or None -> (x, y, s) [B][m]."""
        spline = np.ascontiguousarray(spline, dtype=np.float64); spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        at_s = np.ascontiguousarray(at_s, dtype=np.float64); l = np.ascontiguousarray(l, dtype=np.float64)
        mo = None if m_of is None else np.ascontiguousarray(m_of, dtype=np.int32)
        B, ms, m = spline.shape[0], spline.shape[2], at_s.shape[1]
        x = np.zeros((B, m)); y = np.zeros((B, m)); s = np.zeros((B, m))
        self._check(self.lib.pqp_offsets_to_points(self._h, B, ms, m, spline, spline_ext, at_s, l, mo, x, y, s))
        return x, y, s

    def reference_length(self, spline, spline_ext, length, target):
        """pqp_reference_length (host arrays): spline [B][9][m], spline_ext [B][4], length [B], target [B][3] -> length_out [B]."""
        spline = np.ascontiguousarray(spline, dtype=np.float64); spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        length = np.ascontiguousarray(length, dtype=np.float64); target = np.ascontiguousarray(target, dtype=np.float64)
        B, m = spline.shape[0], spline.shape[2]
        out = np.zeros(B)
        self._check(self.lib.pqp_reference_length(self._h, B, m, spline, spline_ext, length, target, out))
        return out

    def project_points(self, spline, spline_ext, length, points, q_of=None, has_heading=None):
        """pqp_project_points (host arrays): spline [B][9][m], spline_ext [B][4], length [B], points [B][q_max][stride] with x, y (and a heading
        when has_heading; None: stride >= 3) in front, q_of [B] or None -> (proj [B][q_max][8] = s, l, t, d_heading, x_p, y_p, heading_p, k_p,
        flags [B][q_max] of PROJ_*)."""
        spline = np.ascontiguousarray(spline, dtype=np.float64); spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        length = np.ascontiguousarray(length, dtype=np.float64); points = np.ascontiguousarray(points, dtype=np.float64)
        qo = None if q_of is None else np.ascontiguousarray(q_of, dtype=np.int32)
        B, m = spline.shape[0], spline.shape[2]
        q_max, stride = points.shape[1], points.shape[2]
        if has_heading is None:
            has_heading = stride >= 3
        proj = np.zeros((B, q_max, PROJ_STRIDE)); flags = np.zeros((B, q_max), dtype=np.int32)
        self._check(self.lib.pqp_project_points(self._h, B, m, spline, spline_ext, length, q_max, stride, 1 if has_heading else 0,
                                                points, qo, proj, flags))
        return proj, flags

    def bspline_resample(self, points, n_points, n_max):
        """pqp_bspline_resample (host arrays): points [B][p_max][2], n_points [B].  Returns dict(x, y, s: [B][n_max], count [B])."""
        points = np.ascontiguousarray(points, dtype=np.float64)
        n_points = np.ascontiguousarray(n_points, dtype=np.int32)
        B, p_max = points.shape[0], points.shape[1]
        o = {k: np.zeros((B, n_max)) for k in ("x", "y", "s")}
        count = np.zeros(B, dtype=np.int32)
        self._check(self.lib.pqp_bspline_resample(self._h, B, p_max, n_max, points, n_points, o["x"], o["y"], o["s"],
                                                  count))
        o["count"] = count
        return o

    def segment_raw_reference(self, spline, spline_ext, max_s, n_max, delta_s=1.0):
        """pqp_segment_raw_reference (host arrays): spline [B][9][m], spline_ext [B][4], max_s [B].
        Returns dict(x, y, s, angle, k: [B][n_max], count [B]) - the smoother QPs' input lists."""
        spline = np.ascontiguousarray(spline, dtype=np.float64)
        spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        max_s = np.ascontiguousarray(max_s, dtype=np.float64)
        B, m = spline.shape[0], spline.shape[2]
        o = {k: np.zeros((B, n_max)) for k in ("x", "y", "s", "angle", "k")}
        count = np.zeros(B, dtype=np.int32)
        self._check(self.lib.pqp_segment_raw_reference(self._h, B, n_max, m, spline, spline_ext, max_s, delta_s,
                                                       o["x"], o["y"], o["s"], o["angle"], o["k"], count))
        o["count"] = count
        return o

    def corridor_bounds(self, ref, spline, spline_ext, dist, geom, map_of=None, prm=None, n_of=None):
        """pqp_corridor_bounds (host arrays): ref [B][n][5], spline [B][9][m], spline_ext [B][4], dist [n_maps][rows][cols] float32
        (converted to the ABI's column-major order here), geom = PqpGridGeometry.  Returns (bounds [B][n][6], n_valid [B])."""
        ref = np.ascontiguousarray(ref, dtype=np.float64)
        spline = np.ascontiguousarray(spline, dtype=np.float64)
        spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        dist_cm = _column_major(dist, np.float32)
        B, n = ref.shape[0], ref.shape[1]
        m = spline.shape[2]
        bounds = np.zeros((B, n, 6))
        n_valid = np.zeros(B, dtype=np.int32)
        mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
        prm = prm or self.corridor_params()
        no = None if n_of is None else np.ascontiguousarray(n_of, dtype=np.int32)
        self._check(self.lib.pqp_corridor_bounds(self._h, B, n, m, ref, no, spline, spline_ext, dist_cm, dist_cm.shape[0],
                                                 mo, C.byref(geom), C.byref(prm), bounds, n_valid))
        return bounds, n_valid

    def corridor_bounds_on_states(self, ref, states, spline, spline_ext, dist, geom, map_of=None, prm=None, n_of=None):
        """pqp_corridor_bounds_on_states (host arrays): ReferencePath::updateBoundsOnInputStates.  ref [B][n][5] (the reference states),
        states [B][n][stride >= 5] with d_heading at offset 4 (a solve's `out` as it is), n_of [B] states per scenario (<= n) or None;
        spline, spline_ext, dist, geom, map_of, prm as for corridor_bounds.  Returns (bounds [B][n][6], n_valid [B])."""
        ref = np.ascontiguousarray(ref, dtype=np.float64)
        states = np.ascontiguousarray(states, dtype=np.float64)
        spline = np.ascontiguousarray(spline, dtype=np.float64)
        spline_ext = np.ascontiguousarray(spline_ext, dtype=np.float64)
        dist_cm = _column_major(dist, np.float32)
        B, n = ref.shape[0], ref.shape[1]
        if states.ndim != 3 or states.shape[:2] != (B, n):
            raise ValueError(f"states must be [{B}][{n}][stride], got {states.shape}")
        m = spline.shape[2]
        bounds = np.zeros((B, n, 6))
        n_valid = np.zeros(B, dtype=np.int32)
        mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
        prm = prm or self.corridor_params()
        no = None if n_of is None else np.ascontiguousarray(n_of, dtype=np.int32)
        self._check(self.lib.pqp_corridor_bounds_on_states(self._h, B, n, m, ref, no, states, states.shape[2], spline, spline_ext,
                                                           dist_cm, dist_cm.shape[0], mo, C.byref(geom), C.byref(prm), bounds, n_valid))
        return bounds, n_valid

    def sizes(self, n, s=None):
        out = PqpSizes()
        self._check(self.lib.pqp_path_sizes(C.byref(self.params), n, s, C.byref(out)))
        return {k: getattr(out, k) for k, _ in PqpSizes._fields_}

    def _nnz_p(self, n, precise):
        """pqp_sizes.nnz_p: the diagonal of P has the l columns too once weight_l is not zero"""
        return (2 * n if self.params.weight_l != 0.0 else n) + n - 1 + precise + n

    def pattern(self, n, precise=None):
        precise = n if precise is None else precise
        nv = 3 * n + n - 1 + precise + n
        nnz_a = 3 * n + 7 * (n - 1) + n + 6 * precise + 2 * (n - precise) + 2
        rows = np.zeros(nnz_a, dtype=np.int32)
        colptr = np.zeros(nv + 1, dtype=np.int32)
        pcols = np.zeros(self._nnz_p(n, precise), dtype=np.int32)
        self._check(self.lib.pqp_path_pattern(self._h, n, precise, rows, colptr, pcols))
        return rows, colptr, pcols

    def assemble(self, ref, lin, bounds, scal, precise=None):
        batch, n = ref.shape[0], ref.shape[1]
        precise = n if precise is None else precise
        nnz_a = 3 * n + 7 * (n - 1) + n + 6 * precise + 2 * (n - precise) + 2
        nnz_p = self._nnz_p(n, precise)
        cons = 4 * n + precise + n + 2
        a_val = np.zeros((batch, nnz_a)); p_val = np.zeros((batch, nnz_p))
        lo = np.zeros((batch, cons)); up = np.zeros((batch, cons))
        self._check(self.lib.pqp_path_assemble(self._h, batch, n, precise, ref, lin, bounds,
                                               scal, a_val, p_val, lo, up))
        return a_val, p_val, lo, up

    def solve(self, ref, bounds, scal, lin=None, passes=1, warm=False):
        """Host-array convenience: returns dict(out, status, iters, info)."""
        batch, n = ref.shape[0], ref.shape[1]
        out = np.zeros((batch, n, 7)); status = np.zeros(batch, dtype=np.int32)
        iters = np.zeros(batch, dtype=np.int32); info = np.zeros((batch, 8))
        self._check(self.lib.pqp_path_solve(self._h, batch, n, ref, lin, bounds, scal,
                                            passes, 1 if warm else 0, out, status, iters, info))
        return dict(out=out, status=status, iters=iters, info=info)

    def solve_var(self, n_of, ref, bounds, scal, lin=None, passes=1, warm=False):
        """pqp_path_solve_var (host arrays): a waypoint count per QP, arrays of stride n_max = ref.shape[1]."""
        batch, n = ref.shape[0], ref.shape[1]
        counts = np.ascontiguousarray(n_of, dtype=np.int32)
        out = np.zeros((batch, n, 7)); status = np.zeros(batch, dtype=np.int32)
        iters = np.zeros(batch, dtype=np.int32); info = np.zeros((batch, 8))
        self._check(self.lib.pqp_path_solve_var(self._h, batch, n, counts, ref, lin, bounds, scal,
                                                passes, 1 if warm else 0, out, status, iters, info))
        return dict(out=out, status=status, iters=iters, info=info)

    def solve_device(self, batch, n, ref, bounds, scal, out, lin=None, passes=1, warm=False, status=None,
                     iters=None, info=None):
        """Device pointers (ints or objects with data_ptr()); asynchronous on the handle's stream."""
        self._check(self.lib.pqp_path_solve_device(self._h, batch, n, _dp(ref), _dp(lin), _dp(bounds), _dp(scal), passes,
                                                   1 if warm else 0, _dp(out), _dp(status), _dp(iters), _dp(info)))

    def solve_var_device(self, batch, n_max, n_of, ref, bounds, scal, out, lin=None, passes=1, warm=False, status=None, iters=None, info=None):
        """pqp_path_solve_var_device: like solve_device with a waypoint count per QP (n_of: device int32 [batch])."""
        self._check(self.lib.pqp_path_solve_var_device(self._h, batch, n_max, _dp(n_of), _dp(ref), _dp(lin), _dp(bounds), _dp(scal), passes,
                                                       1 if warm else 0, _dp(out), _dp(status), _dp(iters), _dp(info)))

    def get_solution(self, batch, n, precise=None):
        precise = n if precise is None else precise
        nv = 3 * n + n - 1 + precise + n
        nc = 4 * n + precise + n + 2
        x = np.zeros((batch, nv)); y = np.zeros((batch, nc))
        self._check(self.lib.pqp_path_get_solution(self._h, batch, n, precise, x, y))
        return x, y

    # ---- smoother QPs (host arrays [batch][n]) ----
    def smooth_tension2(self, x, y, angle, k, s):
        B, n = x.shape
        ox = np.zeros((B, n)); oy = np.zeros((B, n)); os_ = np.zeros((B, n)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
        c = np.ascontiguousarray
        self._check(self.lib.pqp_smooth_tension2(self._h, B, n, c(x), c(y), c(angle), c(k), c(s), ox, oy,
                                                 os_, st, it))
        return dict(x=ox, y=oy, s=os_, status=st, iters=it)

    def smooth_tension(self, x, y, angle, clearance, info=False):
        B, n = x.shape
        ox = np.zeros((B, n)); oy = np.zeros((B, n)); os_ = np.zeros((B, n)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
        c = np.ascontiguousarray
        if not info:
            self._check(self.lib.pqp_smooth_tension(self._h, B, n, c(x), c(y), c(angle), c(clearance), ox, oy,
                                                    os_, st, it))
            return dict(x=ox, y=oy, s=os_, status=st, iters=it)
        # with the info rows (factorisations in [5]): the device entry point
        return self._on_device(self.lib.pqp_smooth_tension_device, (x, y, angle, clearance), None, ("x", "y", "s"), True, True)

    def _on_device(self, function, lists, count, outs, info_rows=False, info=False):
        """A smoother's `_device` entry point on host arrays, torch as the memory plumbing: uploads `lists` ([B][n] each, the last may be
        [B]) and `count` [B] (None: the entry point takes none), zeroes the [B][n] outputs named in `outs`, status, iters and - with
        info_rows - the info rows [B][8], synchronises, calls, waits and downloads.  The entry point gets the info rows only with `info`."""
        import torch
        dev = torch.device("cuda", self.device)
        B, n = lists[0].shape
        t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        d = [t(a) for a in lists]
        d_count = [] if count is None else [t(count, np.int32)]
        o = [torch.zeros((B, n), dtype=torch.float64, device=dev) for _ in outs]
        st, it = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        inf = torch.zeros((B, 8), dtype=torch.float64, device=dev) if info_rows else None
        torch.cuda.synchronize(dev)
        self._check(function(self._h, B, n, *d_count, *d, *o, st, it, inf if info else None))
        self.sync()
        r = {k: a.cpu().numpy() for k, a in zip(outs + ("status", "iters"), o + [st, it])}
        if info:
            r["info"] = inf.cpu().numpy()
        return r

    def smooth_tension2_var(self, x, y, angle, k, s, n_of):
        """pqp_smooth_tension2_var_device (torch as the memory plumbing): lists [B][n_max], n_of [B] points per scenario."""
        return self._on_device(self.lib.pqp_smooth_tension2_var_device, (x, y, angle, k, s), n_of, ("x", "y", "s"))

    def smooth_tension_var(self, x, y, angle, clearance, n_of):
        """pqp_smooth_tension_var_device (torch as the memory plumbing): lists [B][n_max], n_of [B] points per scenario."""
        return self._on_device(self.lib.pqp_smooth_tension_var_device, (x, y, angle, clearance), n_of, ("x", "y", "s"))

    def post_smooth(self, layers_s, lb, ub, vehicle_l):
        B, m = layers_s.shape
        ol = np.zeros((B, m)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
        c = np.ascontiguousarray
        self._check(self.lib.pqp_post_smooth(self._h, B, m, c(layers_s), c(lb), c(ub), c(vehicle_l), ol, st, it))
        return dict(l=ol, status=st, iters=it)

    def post_smooth_var(self, layers_s, lb, ub, vehicle_l, m_of, info=False):
        """pqp_post_smooth_var_device (torch as the memory plumbing): lists [B][m_max], m_of [B] layers per scenario."""
        return self._on_device(self.lib.pqp_post_smooth_var_device, (layers_s, lb, ub, vehicle_l), m_of, ("l",), True, info)

    def kernel_ms_history(self, count):
        """HIP-event durations of the last `count` launches of this handle (oldest first)."""
        ms = np.zeros(count, dtype=np.float32)
        self._check(self.lib.pqp_kernel_ms_history(self._h, ms, count))
        return ms

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(self.lib.pqp_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_path_kernel(self):
        """pqp_last_path_kernel: 1 = lane-per-waypoint kernel, 2 = lane-per-QP kernel served the last solve (0: none yet)."""
        return int(self.lib.pqp_last_path_kernel(self._h))


# optimize_path's arguments by name with the signature's defaults (None where it has none): what Handle._chain_plan takes
_CHAIN_ARGS = {k: None if p.default is p.empty else p.default for k, p in inspect.signature(Handle.optimize_path).parameters.items()
               if k not in ("self", "dist")}
