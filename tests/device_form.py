"""The `_device` entry points called on torch tensors whose outputs lie in a larger allocation filled with a sentinel: whatever a kernel
must not write (the guard band behind [batch][n_max], rows past a scenario's count) has to come back as the sentinel.  The wrappers of
the line family (d_*) return host arrays, or the untouched Out objects when the call was refused.
(pytest does not rewrite the asserts of a helper module: each one here carries its own message.)"""
import ctypes as C

import numpy as np

from line_cases import SEG_KEYS
from path_optimizer_2_amd import capi
from shared_util import same_bytes

SENT, SENT_I = -1.2345e300, -777          # what the device outputs are filled with before a call
GUARD = 512                               # elements of sentinel behind every device output


def dev():
    import torch
    return torch.device("cuda", 0)


def to_device(a, dt=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


class Out:
    """a device output of `shape` at the start of an allocation GUARD elements longer, all of it filled with the sentinel"""

    def __init__(self, shape, dt=np.float64):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.sent = SENT if dt == np.float64 else SENT_I
        self.t = torch.full((self.n + GUARD,), self.sent, dtype=torch.float64 if dt == np.float64 else torch.int32, device=dev())

    def get(self):
        a = self.t.cpu().numpy()
        assert np.all(a[self.n:] == self.sent), "the device form wrote behind its output"
        return a[:self.n].reshape(self.shape)

    def untouched(self):
        return bool(np.all(self.t.cpu().numpy() == self.sent))


def call(h, name, *args):
    import torch
    conv = [C.c_void_p(a.t.data_ptr()) if isinstance(a, Out) else C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    torch.cuda.synchronize(dev())
    rc = getattr(h.lib, name)(h._h, *conv)
    h.sync()
    return rc


def rows_after(count, n):
    """mask [B][n]: True on the rows at and past each scenario's count"""
    return np.arange(n)[None, :] >= np.minimum(np.maximum(np.asarray(count), 0), n)[:, None]


def host_equals_device(host, dev, count, n):
    """the host form's rows up to count equal the device form's bit for bit; past count the host form has zeros, the device form
    wrote nothing (the sentinel)"""
    past = rows_after(count, n)
    past = past.reshape(past.shape + (1,) * (np.ndim(host) - 2))
    past = np.broadcast_to(past, np.shape(host))
    assert same_bytes(np.where(past, 0.0, dev), np.where(past, 0.0, host)), "host and device form differ in the rows up to count"
    assert np.all(np.asarray(host)[past] == 0.0), "the host form has something other than zeros past count"
    assert np.all(np.asarray(dev)[past] == SENT), "the device form wrote past count"


# ---- the line family -----------------------------------------------------------------------------------------------------------------
def d_spline_fit(h, s, x, y, m_of=None):
    B, m = np.shape(s)
    tab, ext = Out((B, 9, m)), Out((B, 4))
    if m_of is None:
        rc = call(h, "pqp_spline_fit_device", B, m, to_device(s), to_device(x), to_device(y), tab, ext)
    else:
        rc = call(h, "pqp_spline_fit_var_device", B, m, to_device(m_of, np.int32), to_device(s), to_device(x), to_device(y), tab, ext)
    return (rc, tab, ext) if rc else (rc, tab.get(), ext.get())


def d_reference_states(h, tab, ext, max_s, n_max, start=None, dynamic=True):
    B, m = tab.shape[0], tab.shape[2]
    ref, cnt = Out((B, n_max, 5)), Out((B,), np.int32)
    err = Out((B, 2)) if start is not None else None
    rc = call(h, "pqp_reference_states_device", B, n_max, m, to_device(tab), to_device(ext), to_device(max_s), None if start is None else to_device(start),
              0.15, 0.3, 1 if dynamic else 0, ref, cnt, err)
    if rc:
        return rc, (ref, cnt)
    return rc, ref.get(), cnt.get(), None if err is None else err.get()


def d_segment(h, tab, ext, max_s, n_max):
    B, m = tab.shape[0], tab.shape[2]
    o = {k: Out((B, n_max)) for k in SEG_KEYS}
    cnt = Out((B,), np.int32)
    rc = call(h, "pqp_segment_raw_reference_device", B, n_max, m, to_device(tab), to_device(ext), to_device(max_s), 1.0, *(o[k] for k in SEG_KEYS), cnt)
    if rc:
        return rc, list(o.values()) + [cnt]
    r = {k: v.get() for k, v in o.items()}
    r["count"] = cnt.get()
    return rc, r


def d_reference_length(h, tab, ext, length, target):
    B, m = tab.shape[0], tab.shape[2]
    out = Out((B,))
    rc = call(h, "pqp_reference_length_device", B, m, to_device(tab), to_device(ext), to_device(length), to_device(target), out)
    return (rc, out) if rc else (rc, out.get())


def d_offsets(h, tab, ext, at_s, l, m_of=None):
    B, ms, m = tab.shape[0], tab.shape[2], at_s.shape[1]
    x, y, s = Out((B, m)), Out((B, m)), Out((B, m))
    rc = call(h, "pqp_offsets_to_points_device", B, ms, m, to_device(tab), to_device(ext), to_device(at_s), to_device(l),
              None if m_of is None else to_device(m_of, np.int32), x, y, s)
    return (rc, [x, y, s]) if rc else (rc, x.get(), y.get(), s.get())


def d_bspline(h, pts, n_pts, n_max):
    B, p_max = pts.shape[0], pts.shape[1]
    o = {k: Out((B, n_max)) for k in ("x", "y", "s")}
    cnt = Out((B,), np.int32)
    rc = call(h, "pqp_bspline_resample_device", B, p_max, n_max, to_device(pts), to_device(n_pts, np.int32), o["x"], o["y"], o["s"], cnt)
    if rc:
        return rc, list(o.values()) + [cnt]
    r = {k: v.get() for k, v in o.items()}
    r["count"] = cnt.get()
    return rc, r


def d_dp(h, tab, ext, length, start, dist, geom, max_layers, map_of=None, prm=None):
    B, m = tab.shape[0], tab.shape[2]
    if prm is None:
        prm = capi.PqpDpParams()
        h.lib.pqp_dp_default_params(C.byref(prm))
    ls, lb, ub, vl = Out((B, max_layers)), Out((B, max_layers)), Out((B, max_layers)), Out((B,))
    cnt = Out((B,), np.int32)
    rc = call(h, "pqp_dp_corridor_device", B, m, max_layers, to_device(tab), to_device(ext), to_device(length), to_device(start),
              to_device(capi._column_major(dist, np.float32), np.float32), None if map_of is None else to_device(map_of, np.int32), C.byref(geom), C.byref(prm),
              ls, lb, ub, cnt, vl)
    if rc:
        return rc, [ls, lb, ub, cnt, vl]
    return rc, ls.get(), lb.get(), ub.get(), cnt.get(), vl.get()


def d_bounds(h, ref, n_of, tab, ext, dist, geom, map_of=None):
    B, n, m = ref.shape[0], ref.shape[1], tab.shape[2]
    bounds, nv = Out((B, n, 6)), Out((B,), np.int32)
    rc = call(h, "pqp_corridor_bounds_device", B, n, m, to_device(ref), to_device(n_of, np.int32), to_device(tab), to_device(ext),
              to_device(capi._column_major(dist, np.float32), np.float32), None if map_of is None else to_device(map_of, np.int32), C.byref(geom),
              C.byref(h.corridor_params()), bounds, nv)
    assert rc == 0, h.lib.pqp_last_error()
    return bounds.get(), nv.get()


def d_bounds_on_states(h, ref, states, tab, ext, dist, geom, map_of=None, n_of=None, prm=None):
    B, n = ref.shape[:2]
    bounds, nv = Out((B, n, 6)), Out((B,), np.int32)
    prm = prm or h.corridor_params()
    rc = call(h, "pqp_corridor_bounds_on_states_device", B, n, tab.shape[2], to_device(ref), None if n_of is None else to_device(n_of, np.int32), to_device(states),
              states.shape[2], to_device(tab), to_device(ext), to_device(np.transpose(dist, (0, 2, 1)), np.float32),
              None if map_of is None else to_device(map_of, np.int32), C.byref(geom), C.byref(prm), bounds, nv)
    assert rc == 0, h.lib.pqp_last_error()
    return bounds.get(), nv.get()
