"""pqp_sample_plan restated in numpy float64 (include/pqp.h states the definition): the m rows of a speed plan on r sub-steps per layer
under constant acceleration or linearly, the clamp between the two layers' stations, the placement on the path, defect, excess and the
flags - one path at a time, operation by operation in the stated order.  The placement is not restated here: it is the search's "pose at
sigma" at any station, which refine_util.pose_at holds for the refine's restatement (tests/test_plan_sample.py holds it against
search_util.stations on the grid's own stations).  Every operation is a correctly rounded IEEE one and numpy fuses none, sqrt included:
every output agrees with the device bit for bit.  sample() is the vectorised form the tests compare the device against; sample_loop() is
the same definition one sample at a time in a plain Python loop, which the CPU tests hold sample() against."""
import math

import numpy as np

import refine_util as R
import sample_util as T

EMPTY, NOT_FINITE, BACKWARD = 1, 2, 4
REFINED = R.REFINED


def fine_count(m, r):
    """M = (m - 1) r + 1"""
    return (m - 1) * r + 1


def _judge(path, profile, plan, n_of, stop_before, count):
    """(c, L, what the call writes when the path has no samples, or None)"""
    m = plan.shape[0]
    c = T.driven(path.shape[0], n_of, stop_before)
    L = m if count is None else min(max(int(count), 0), m)
    if c == 0 or L == 0:
        return c, L, EMPTY
    if not (np.isfinite(path[:c][:, [0, 1, 2, 5]]).all() and np.isfinite(profile[:c, :3]).all() and np.isfinite(plan[:L, 4:7]).all()):
        return c, L, NOT_FINITE
    return c, L, None


def _nothing(M, why):
    return dict(traj=np.full((M, 8), math.nan if why == NOT_FINITE else 0.0), m_of=0, defect=math.nan, excess=math.nan, flags=why)


def sample(path, profile, plan, r, dt, n_of=None, stop_before=None, count=None, linear=False):
    """one path [n][stride >= 6] with its profile [n][4] and its plan [m][8] -> dict(traj [M][8], m_of, defect, excess, flags)"""
    path, profile, plan = (np.asarray(a, dtype=np.float64) for a in (path, profile, plan))
    m, r = plan.shape[0], int(r)
    M = fine_count(m, r)
    c, L, why = _judge(path, profile, plan, n_of, stop_before, count)
    if why is not None:
        return _nothing(M, why)
    dt, rr = np.float64(dt), np.float64(r)
    m_of = fine_count(L, r)
    f = np.arange(m_of - 1)
    k, i = f // r, f % r
    sk, vk, ak, sn = plan[k, 4], plan[k, 5], plan[k, 6], plan[k + 1, 4]
    fi = i.astype(np.float64)
    with np.errstate(all="ignore"):
        u = (fi * dt) / rr
        if linear:
            at = sk + ((sn - sk) * fi) / rr
            v = (sn - sk) / dt
            a = np.zeros(len(f))
        else:
            at = sk + (vk + (0.5 * ak) * u) * u
            v = np.fmax(vk + ak * u, 0.0)
            a = ak
        s = np.fmin(np.fmax(at, sk), np.fmax(sn, sk))
        t = k.astype(np.float64) * dt + u
        rows = np.zeros((M, 8))
        rows[:m_of - 1, 4], rows[:m_of - 1, 5], rows[:m_of - 1, 6], rows[:m_of - 1, 7] = s, v, a, t
        rows[m_of - 1, 4:] = [plan[L - 1, 4], np.fmax(plan[L - 1, 5], 0.0), plan[L - 1, 6], np.float64(L - 1) * dt]
        pose, w = R.pose_at(path, profile, c, rows[:m_of, 4])
        rows[:m_of, :4] = pose
        excess = float(np.fmax.reduce(rows[:m_of, 5] - np.sqrt(np.fmax(w, 0.0)), initial=-math.inf))
        defect = 0.0
        if not linear and L > 1:
            s0, v0, a0 = plan[:L - 1, 4], plan[:L - 1, 5], plan[:L - 1, 6]
            defect = float(np.fmax.reduce(np.fabs((s0 + (v0 + (0.5 * a0) * dt) * dt) - plan[1:L, 4]), initial=0.0))
    flags = BACKWARD if (plan[1:L, 4] < plan[:L - 1, 4]).any() else 0
    return dict(traj=rows, m_of=m_of, defect=defect, excess=excess, flags=flags)


def sample_loop(path, profile, plan, r, dt, n_of=None, stop_before=None, count=None, linear=False):
    """sample(), one sample at a time: the definition read top to bottom"""
    path, profile, plan = (np.asarray(a, dtype=np.float64) for a in (path, profile, plan))
    m, r = plan.shape[0], int(r)
    M = fine_count(m, r)
    c, L, why = _judge(path, profile, plan, n_of, stop_before, count)
    if why is not None:
        return _nothing(M, why)
    dt = np.float64(dt)
    m_of = fine_count(L, r)
    rows = np.zeros((M, 8))
    defect, excess, flags = np.float64(0.0), np.float64(-math.inf), 0
    with np.errstate(all="ignore"):
        for f in range(m_of):
            if f < m_of - 1:
                k, i = divmod(f, r)
                sk, vk, ak, sn = (np.float64(x) for x in (plan[k, 4], plan[k, 5], plan[k, 6], plan[k + 1, 4]))
                u = (np.float64(i) * dt) / np.float64(r)
                if linear:
                    at = sk + ((sn - sk) * np.float64(i)) / np.float64(r)
                    v, a = (sn - sk) / dt, np.float64(0.0)
                else:
                    at = sk + (vk + (0.5 * ak) * u) * u
                    v, a = np.fmax(vk + ak * u, 0.0), ak
                    if i == 0:
                        defect = np.fmax(defect, np.fabs((sk + (vk + (0.5 * ak) * dt) * dt) - sn))
                s = np.fmin(np.fmax(at, sk), np.fmax(sn, sk))
                t = np.float64(k) * dt + u
                if sn < sk:
                    flags |= BACKWARD
            else:
                s, v, a, t = plan[L - 1, 4], np.fmax(plan[L - 1, 5], 0.0), plan[L - 1, 6], np.float64(L - 1) * dt
            pose, w = R.pose_at(path, profile, c, np.array([s]))
            rows[f] = [pose[0, 0], pose[0, 1], pose[0, 2], pose[0, 3], s, v, a, t]
            excess = np.fmax(excess, v - np.sqrt(np.fmax(w[0], 0.0)))
    return dict(traj=rows, m_of=m_of, defect=float(defect), excess=float(excess), flags=flags)


def sample_batch(paths, profile, plan, r, dt, n_of=None, stop_before=None, count_of=None, refine_flags=None, linear=False, one=sample):
    """the whole entry point: paths [B][n][stride], profile [B][n][4], plan [B][m][8] -> dict of stacked outputs.  refine_flags given: a
    path with REFINED set is sampled under constant acceleration, every other path linearly, and `linear` is not read"""
    pick = lambda a, b: None if a is None else a[b]
    got = []
    for b in range(len(paths)):
        lin = bool(linear) if refine_flags is None else not (int(refine_flags[b]) & REFINED)
        got.append(one(paths[b], profile[b], plan[b], r, dt, pick(n_of, b), pick(stop_before, b), pick(count_of, b), lin))
    res = {k: np.stack([np.asarray(g[k]) for g in got]) for k in ("traj", "m_of", "defect", "excess", "flags")}
    res["m_of"], res["flags"] = res["m_of"].astype(np.int32), res["flags"].astype(np.int32)
    return res


# ---- the plans of the cases ----------------------------------------------------------------------------------------------------------------
def defect_bound(dt, s_top):
    """what the defect of a plan pqp_speed_refine returns is bounded by, from refine_util.KKT_WORST's primal residual p (the worst violation
    of any row of the QP at the emulation's x, 3.0e-8): the dynamics row s_{k+1} - s_k - dt v_k - (dt^2 / 2) a_k is off 0 by at most p, and
    the call's clamps (s into its corridor, v to 0 from below, a_{m-1} = 0) move each of the row's four variables by at most p, since
    the boxes are rows of the QP too - together p times (1 + the row's 1-norm, 2 + dt + dt^2 / 2).  The defect's own expression rounds
    five times at the size of the plan's largest station."""
    return R.KKT_WORST["primal"] * (3.0 + dt + 0.5 * dt * dt) + 8.0 * np.finfo(np.float64).eps * max(float(s_top), 1.0)


_REFINED = {}


def refined_plan(name):
    """a case of refine_util by name through the search's restatement and the banded core's host emulation (refine_util.reference without
    HiGHS), finished as the call finishes it: dict(case, res, m, traj [B][m][8], flags [B]); computed once, nobody writes to it"""
    if name not in _REFINED:
        r = R.reference(name, highs=False)
        c, dt = r["case"], r["case"]["prm"]["dt"]
        fins = []
        for b, one in enumerate(r["each"]):
            e = one["emu"]
            x = None if e is None or e["status"] != R.SOLVED else one["xe"]
            fins.append(R.finish(c["paths"][b], c["profile"][b], one["su"], one["found"], x, R.SOLVED if x is not None else (R.UNSOLVED if e is None else e["status"]), dt))
        _REFINED[name] = dict(case=c, res=r["res"], m=r["m"], traj=np.stack([f["traj"] for f in fins]), flags=np.array([f["flags"] for f in fins], np.int32))
    return _REFINED[name]


def synthetic(B, n, m, seed, n_of=None, stop_before=None):
    """plan rows from numpy on search_util's curved synthetic paths (0.15 .. 0.3 m between waypoints) under their own speed profiles:
    dict(paths [B][n][7], profile [B][n][4], plan [B][m][8], n_of, stop_before, dt).  Stations ascend by steps that take the last layers
    of most plans past the end of the driven path (where the pose is the last waypoint's), speeds and accelerations are anything of a
    car's size, negative speeds included; the columns nobody reads (x, y, heading, k, t) hold noise"""
    import search_util as S
    rng = np.random.default_rng(seed)
    paths = S.synth_paths(B, n, first=seed)
    v_start = rng.uniform(0.0, 4.0, B)
    plan = rng.normal(size=(B, m, 8))
    profile = np.zeros((B, n, 4))
    for b in range(B):
        c = T.driven(n, None if n_of is None else n_of[b], None if stop_before is None else stop_before[b])
        if c:                                                # (an empty path's profile is not read: zeros)
            profile[b] = S.profile_of(paths[b], float(v_start[b]), n_of=None if n_of is None else int(n_of[b]),
                                      stop_before=None if stop_before is None else int(stop_before[b]))
        length = float(profile[b, c - 1, 0]) if c else 1.0
        step = rng.uniform(0.0, 1.0, m) * (2.0 * length / m)
        step[rng.uniform(size=m) < 0.2] = 0.0                 # the car stands for a layer now and then
        s = np.concatenate([[0.0], np.cumsum(step[1:])])
        if b == 0 and m > 1:                                  # path 0 always ends past its path
            s = s * (1.25 * length / s[-1]) if s[-1] > 0.0 else np.concatenate([s[:-1], [1.25 * length]])
        plan[b, :, 4] = s
        plan[b, :, 5] = rng.uniform(-0.5, 6.0, m)
        plan[b, :, 6] = rng.uniform(-3.0, 1.5, m)
    return dict(paths=paths, profile=profile, plan=plan, n_of=n_of, stop_before=stop_before, dt=0.5)


# ---- the hand case: a disc that crosses the lane between two layers -----------------------------------------------------------------------------
CROSS_R = 10                                                 # sub-steps per layer
CROSS_AT = 35                                                # the fine step at which the disc is on the car's axis: t = 3.5 s, between layers 3 and 4
CROSS_STEP = 1.25                                            # m the disc moves across the road per fine step (12.5 m/s)
CROSS_RADIUS = 0.5
CROSS_FIRST_HIT = 34


def crossing():
    """refine_util's hand road ("rest": from rest on a free road at heading 0, the hand car), its refined plan, and a pedestrian disc of
    0.5 m that crosses the road at right angles, 1.25 m per fine step of 0.1 s, through the car's axis at fine step 35 (t = 3.5 s), 1.5 m
    in front of the rear axle's station there.  The hand car's large circles (radius 1.25 at 0.75 and 2.25 m in front of the rear axle)
    reach 1.75 m to the side with the disc's radius: at fine steps 34, 35 and 36 the disc is 1.25, 0 and 1.25 m beside the axis - hits -
    and at step 33 it is 2.5 m beside it, clear by 0.75 m or more.  At the layers (steps 30 and 40) it is 6.25 m away.  So the m rows are
    clear and the fine rows are hit first at sample 34.
    -> dict(case, plan [1][m][8], flags [1], m, fine_agents [1][1][M][6], coarse_agents [1][1][m][6])"""
    p = refined_plan("rest")
    c, m = p["case"], p["m"]
    M = fine_count(m, CROSS_R)
    got = sample(c["paths"][0], c["profile"][0], p["traj"][0], CROSS_R, c["prm"]["dt"])
    x = float(got["traj"][CROSS_AT, 0]) + 1.5
    fine = np.zeros((1, 1, M, 6))
    fine[0, 0, :, 0] = x
    fine[0, 0, :, 1] = CROSS_STEP * (CROSS_AT - np.arange(M)).astype(np.float64)
    fine[0, 0, :, 5] = CROSS_RADIUS
    return dict(case=c, plan=p["traj"], flags=p["flags"], m=m, fine_agents=fine, coarse_agents=np.ascontiguousarray(fine[:, :, ::CROSS_R]))
