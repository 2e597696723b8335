"""pqp_agents_check restated in numpy float64 (include/pqp.h states the definition): both launches, operation by operation in the stated
order.  Every operation here is a correctly rounded IEEE one and numpy fuses none of them; what the device may differ by is its sincos,
a few ulp of 1 from libm's - so the frames' cos and sin are compared to 1e-15 and the clearances to 1e-9 m, everything else bit for bit
(tests/test_gpu_agents_check.py), and with heading 0, where both are exact, the whole answer is."""
import math

import numpy as np

AGENT_STRIDE, FRAME_STRIDE = 6, 8
DEFAULTS = dict(margin=0.0)
SLACK, SLACK_REL = 2.0 ** -10, 2.0 ** -30                    # the broad phase's (csrc/pqp_agent_frames.hpp)


def frames(agents):
    """agents [...][6] = x, y, heading, half_length, half_width, radius -> [...][8] = x, y, cos, sin, hl, hw, radius, reach.
    Absent (hl < 0 or hw < 0, tested first): zeros with reach -1.  Bad (a value not finite, radius < 0): zeros with reach NaN."""
    ag = np.asarray(agents, dtype=np.float64)
    out = np.zeros(ag.shape[:-1] + (FRAME_STRIDE,))
    x, y, h, hl, hw, rad = (ag[..., q] for q in range(AGENT_STRIDE))
    absent = (hl < 0.0) | (hw < 0.0)
    bad = ~absent & ~(np.isfinite(ag).all(axis=-1) & (rad >= 0.0))
    ok = ~absent & ~bad
    with np.errstate(all="ignore"):
        reach = np.sqrt(hl * hl + hw * hw) + rad
        cos, sin = np.cos(np.where(ok, h, 0.0)), np.sin(np.where(ok, h, 0.0))
    for q, col in enumerate((x, y, cos, sin, hl, hw, rad, reach)):
        out[..., q] = np.where(ok, col, 0.0)
    out[..., 7] = np.where(absent, -1.0, np.where(bad, math.nan, out[..., 7]))
    return out


def bounding_reach(circles):
    """Rb = max_j (|c_j - c_6| + r_j): the six circles lie within Rb of the bounding circle's centre (the host's std::hypot is libm's)"""
    return max(math.hypot(cx - circles[6][0], cy - circles[6][1]) + r for cx, cy, r in circles[:6])


def clear_matrix(rows, fr, circles):
    """rows [c][>= 3] (x, y, heading; all finite), fr [A][c][8] -> clear(k, a) [c][A]: +inf for an absent agent, -inf for a bad one"""
    c = rows.shape[0]
    A = fr.shape[0]
    out = np.full((c, A), math.inf)
    if c == 0 or A == 0:
        return out
    x, y, h = rows[:, 0], rows[:, 1], rows[:, 2]
    with np.errstate(all="ignore"):
        sh, ch = np.sin(h), np.cos(h)
        for j in range(6):
            cx, cy, r = (np.float64(v) for v in circles[j])
            gx = cx * ch - cy * sh + x
            gy = cx * sh + cy * ch + y
            for a in range(A):
                ax, ay, cs, sn, hl, hw, rad = (fr[a, :, q] for q in range(7))
                dx, dy = gx - ax, gy - ay
                u = dx * cs + dy * sn
                w = dy * cs - dx * sn
                ex, ey = np.fabs(u) - hl, np.fabs(w) - hw
                ox, oy = np.fmax(ex, 0.0), np.fmax(ey, 0.0)
                d = np.sqrt(ox * ox + oy * oy) + np.fmin(np.fmax(ex, ey), 0.0) - rad
                out[:, a] = np.fmin(out[:, a], d - r)
    reach = fr[:, :, 7].T
    out = np.where(reach < 0.0, math.inf, out)
    return np.where(np.isnan(reach), -math.inf, out)


def broad_phase_skips(rows, fr, circles, margin, rb=None, with_margin=True, with_radius=True):
    """rows [c][>= 3] (finite), fr [A][c][8] -> bool [c][A]: the agents agents_check_kernel<false> leaves out, by its own expression
    (csrc/pqp_agents_kernels.inc).  rb: the radius around the bounding centre c_6 taken to hold the six circles (None: bounding_reach);
    with_margin / with_radius = False leave the margin / the agent's rounding radius out of the bound.  The defaults are the kernel; the
    others are the mistakes the tests must be able to see (tests/test_agents_check.py)."""
    rb = bounding_reach(circles) if rb is None else rb
    x, y, h = rows[:, 0], rows[:, 1], rows[:, 2]
    cx, cy = np.float64(circles[6][0]), np.float64(circles[6][1])
    with np.errstate(all="ignore"):
        sh, ch = np.sin(h), np.cos(h)
        bx, by = (cx * ch - cy * sh + x)[:, None], (cx * sh + cy * ch + y)[:, None]
        ax, ay, reach = fr[:, :, 0].T, fr[:, :, 1].T, fr[:, :, 7].T
        if not with_radius:
            reach = reach - fr[:, :, 6].T
        ux, uy = bx - ax, by - ay
        far = rb + reach + (margin if with_margin else 0.0) + SLACK + SLACK_REL * (np.fabs(bx) + np.fabs(by) + np.fabs(ax) + np.fabs(ay))
        return (reach >= 0.0) & (ux * ux + uy * uy > far * far)          # (absent and bad rows never get here)


def check_path(rows, fr, circles, margin=0.0, count=None, broad=None):
    """one path: rows [m][>= 3], fr [A][m][8] (its scene's frames, the scene's agent count applied) ->
    (first_hit, hit_agent, clearance [m], clear [count][A]: the matrix the answer was taken from, NaN rows at ego samples not finite).
    broad: keywords of broad_phase_skips - the agents it leaves out count as clear (+inf), as with clearance = NULL"""
    rows = np.asarray(rows, dtype=np.float64)
    m = rows.shape[0]
    c = m if count is None else min(max(int(count), 0), m)
    A = fr.shape[0]
    finite = np.isfinite(rows[:c, :3]).all(axis=1)
    clear = np.full((c, A), math.nan)
    clear[finite] = clear_matrix(rows[:c][finite], fr[:, :c][:, finite], circles)
    if broad is not None and A:
        clear[finite] = np.where(broad_phase_skips(rows[:c][finite], fr[:, :c][:, finite], circles, margin, **broad), math.inf, clear[finite])
    clearance = np.zeros(m)
    first, who = c, -1
    for k in range(c):
        if not finite[k]:
            clearance[k] = -math.inf
            hits = None
        else:
            clearance[k] = np.fmin.reduce(clear[k], initial=math.inf) if A else math.inf
            hits = np.nonzero(clear[k] < margin)[0]
        if first == c and (hits is None or hits.size):
            first, who = k, (-1 if hits is None else int(hits[0]))
    return first, who, clearance, clear


def check(traj, agents, circles, m_of=None, a_of=None, scene_of=None, margin=0.0, frames_in=None, broad=None):
    """the whole entry point: traj [B][m][stride], agents [n_scenes][a_max][m][6] -> dict(first_hit [B], hit_agent [B], clearance [B][m],
    clear: one [count][A] matrix per path).  scene_of is clamped as the device form clamps it; frames_in: frames to take in place of
    frames(agents) (the device's own, to leave its sincos out of a comparison); broad: see check_path."""
    traj = np.asarray(traj, dtype=np.float64)
    agents = np.asarray(agents, dtype=np.float64)
    B, m = traj.shape[:2]
    n_scenes, a_max = agents.shape[:2]
    fr = frames(agents) if frames_in is None else np.asarray(frames_in, dtype=np.float64)
    first, who, clearance, clears = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, m)), []
    for b in range(B):
        s = 0 if scene_of is None else min(max(int(scene_of[b]), 0), n_scenes - 1)
        A = a_max if a_of is None else min(max(int(a_of[s]), 0), a_max)
        first[b], who[b], clearance[b], cl = check_path(traj[b], fr[s, :A], circles, margin, None if m_of is None else m_of[b], broad)
        clears.append(cl)
    return dict(first_hit=first, hit_agent=who, clearance=clearance, clear=clears)


def near_margin(clears, margin, tol=1e-9):
    """per path a bool [count]: some |clear(k, a) - margin| <= tol - where a few ulp of sin / cos may flip the comparison"""
    return [(np.abs(cl - margin) <= tol).any(axis=1) if cl.size else np.zeros(cl.shape[0], bool) for cl in clears]


def seeded_case(rng, B, m, n_scenes, a_max, stride=3, span=1000.0, near=0.7):
    """traj [B][m][stride], agents [n_scenes][a_max][m][6]: cars that drive 0.2 to 1.5 m per step somewhere within +-span, and agents
    of which a share `near` is placed along one of the scene's paths (some into it, some beside it) and the rest anywhere; noise in the
    unused columns, agents absent at a tenth of the steps"""
    traj = rng.normal(size=(B, m, stride))
    for b in range(B):
        h0 = rng.uniform(-math.pi, math.pi)
        head = h0 + np.cumsum(rng.normal(scale=0.03, size=m))
        step = rng.uniform(0.2, 1.5)
        traj[b, :, 0] = rng.uniform(-span, span) + np.cumsum(step * np.cos(head))
        traj[b, :, 1] = rng.uniform(-span, span) + np.cumsum(step * np.sin(head))
        traj[b, :, 2] = head
    agents = np.zeros((n_scenes, a_max, m, AGENT_STRIDE))
    for s in range(n_scenes):
        for a in range(a_max):
            if rng.uniform() < near:
                b = int(rng.integers(B))
                k = int(rng.integers(m))
                off = rng.uniform(-8.0, 8.0, 2) * (0.25 if rng.uniform() < 0.5 else 1.0)
                v = rng.uniform(-1.0, 1.0, 2)
                agents[s, a, :, 0] = traj[b, k, 0] + off[0] + v[0] * (np.arange(m) - k)
                agents[s, a, :, 1] = traj[b, k, 1] + off[1] + v[1] * (np.arange(m) - k)
            else:
                agents[s, a, :, 0] = rng.uniform(-span, span) + rng.uniform(-1, 1) * np.arange(m)
                agents[s, a, :, 1] = rng.uniform(-span, span) + rng.uniform(-1, 1) * np.arange(m)
            agents[s, a, :, 2] = rng.uniform(-math.pi, math.pi) + np.cumsum(rng.normal(scale=0.05, size=m))
            kind = rng.integers(3)
            agents[s, a, :, 3] = 0.0 if kind == 0 else rng.uniform(0.2, 3.0)
            agents[s, a, :, 4] = 0.0 if kind == 0 else rng.uniform(0.2, 1.2)
            agents[s, a, :, 5] = rng.uniform(0.2, 0.6) if kind == 0 else (0.0 if kind == 1 else rng.uniform(0.0, 0.4))
            gone = rng.uniform(size=m) < 0.1
            agents[s, a, gone, 3 + int(rng.integers(2))] = -1.0
    return traj, agents


# ---- cases with answers known by hand (tests/test_agents_check.py states them; the device must give the same bits) -------------------------
# A car 2 m wide from 1 m behind the rear axle to 4 m in front of it: the two large circles sit at (0.75, 0) and (2.25, 0) with the dyadic
# radius 1.25, the four small ones at (-0.5, +-0.5) and (3.5, +-0.5) with radius sqrt(0.5).  Heading 0 everywhere: sin and cos are exact.
HAND_CAR = dict(width=2.0, rear_length=-1.0, front_length=4.0)
HAND_M = 16


def _drive(m=HAND_M, step=0.5):
    """[1][m][3]: along the x axis, 0.5 m per step"""
    t = np.zeros((1, m, 3))
    t[0, :, 0] = step * np.arange(m)
    return t


def _agent(x, y, hl, hw, radius=0.0, heading=0.0, m=HAND_M):
    return np.tile(np.array([x, y, heading, hl, hw, radius], dtype=np.float64), (m, 1))


def hand_cases():
    """name -> dict(traj, agents [1][A][m][6], margin[, m_of])"""
    box = _agent(4.0, 4.0, 2.0, 1.0)                         # x in [2, 6], y in [3, 5]: 3 m beside the axis, 1.75 m beside the large circles
    cases = {"parked_box": dict(traj=_drive(), agents=box[None, None], margin=1.5)}
    moved = box.copy()
    moved[5, 1] = 4.0 - 1.75                                 # at step 5 the box has come nearer by exactly the gap: touching
    cases["moved_by_the_gap_touching"] = dict(traj=_drive(), agents=moved[None, None], margin=0.0)
    cases["moved_by_the_gap"] = dict(traj=_drive(), agents=moved[None, None], margin=2.0 ** -20)
    cases["grazing"] = dict(traj=_drive(), agents=box[None, None], margin=1.75)
    nearer = box.copy()
    nearer[:, 1] = np.nextafter(4.0, 0.0)
    cases["grazing_one_ulp_nearer"] = dict(traj=_drive(), agents=nearer[None, None], margin=1.75)
    cases["centre_inside"] = dict(traj=_drive(m=1), agents=_agent(2.25, 0.0, 2.0, 1.0, m=1)[None, None], margin=0.0)
    cases["disc"] = dict(traj=_drive(m=1), agents=_agent(2.25, 3.0, 0.0, 0.0, radius=0.5, m=1)[None, None], margin=0.0)
    away = box.copy()
    away[3:6, 3] = -1.0                                      # absent by half_length
    away[8, 4] = -0.0                                        # -0 is not < 0: present, a box of no width
    away[9, 4] = -2.0                                        # absent by half_width, with a NaN in what is then not read
    away[9, 0] = math.nan
    cases["absent_for_some_steps"] = dict(traj=_drive(), agents=away[None, None], margin=1.5)
    bad = np.stack([box, box])
    bad[1, 7, 5] = -0.25                                     # agent 1: a negative radius at step 7
    bad[0, 9, 1] = math.inf                                  # agent 0: a y that is no number at step 9
    cases["bad_rows"] = dict(traj=_drive(), agents=bad[None], margin=0.0)
    ego = _drive()
    ego[0, 4, 2] = math.nan
    close = _agent(2.25, 0.0, 2.0, 1.0)                      # on top of the car at step 0 ... and the NaN sample is still the ego's own hit
    cases["ego_nan"] = dict(traj=ego, agents=box[None, None], margin=0.0)
    ego2 = ego.copy()
    ego2[0, 0, 0] = math.inf
    cases["ego_inf_over_a_hit"] = dict(traj=ego2, agents=close[None, None], margin=0.0)
    cases["count_zero"] = dict(traj=_drive(), agents=close[None, None], margin=0.0, m_of=[0])
    cases["count_three"] = dict(traj=_drive(), agents=moved[None, None], margin=1.0, m_of=[3])
    two = np.stack([box, moved, moved])                      # agents 1 and 2 both hit at step 5
    cases["two_hit_the_same_sample"] = dict(traj=_drive(), agents=two[None], margin=0.5)
    cases["no_agents"] = dict(traj=_drive(), agents=np.zeros((1, 0, HAND_M, AGENT_STRIDE)), margin=0.0)
    return cases


# ---- hits at the very edge of the broad phase ----------------------------------------------------------------------------------------------
EDGE_M, EDGE_MARGIN, EDGE_EPS = 70, 0.3, 1e-6


def edge_cases(circles, margin=EDGE_MARGIN, eps=EDGE_EPS):
    """dict(traj [B][70][3], agents [B][2][70][6], scene_of, margin, want_first, want_who): one scene per path, and in it one true hit, by
    eps: an agent whose centre is as far from the footprint's bounding centre c_6 as a hitting agent's can be, Rb + reach + margin - eps.
    It lies beyond a corner circle j in the direction c_6 -> c_j (all four corners attain Rb), which leaves clear = margin - eps to that
    circle and more to the others.  Discs, and rounded boxes whose own corner points at the car (their reach then counts in full).  A
    broad phase with a smaller radius - the reference's own bounding circle, a forgotten margin or rounding radius - leaves these out and
    loses the path's only hit.  The hit is agent 1 at one sample, in the first tile or the second; agent 0 is the same agent moved out by
    2 eps at every sample, a miss by eps."""
    circles = np.asarray(circles, dtype=np.float64)
    shapes = [(0.0, 0.0, 0.5), (2.0, 1.0, 0.25), (0.0, 0.0, 0.4), (1.5, 0.5, 0.0), (0.7, 0.7, 0.35)]          # hl, hw, radius
    combos = [(h, j) for h in (0.0, 0.7, -2.1, 3.0) for j in (2, 3)] + [(1.3, 0), (-0.4, 1)]
    B = len(combos)
    traj, agents = np.zeros((B, EDGE_M, 3)), np.zeros((B, 2, EDGE_M, AGENT_STRIDE))
    want_first = np.zeros(B, np.int32)
    for b, (h, j) in enumerate(combos):
        hl, hw, radius = shapes[b % len(shapes)]
        k_hit = (5, 66, 63, 64)[b % 4]
        k = np.arange(EDGE_M)
        x, y = 30.0 * b - 100.0 + 0.6 * k * math.cos(h), 17.0 * b - 60.0 + 0.6 * k * math.sin(h)
        traj[b, :, 0], traj[b, :, 1], traj[b, :, 2] = x, y, h
        vx, vy = circles[j][0] - circles[6][0], circles[j][1] - circles[6][1]
        vn = math.hypot(vx, vy)
        ex, ey = (vx * math.cos(h) - vy * math.sin(h)) / vn, (vx * math.sin(h) + vy * math.cos(h)) / vn       # c_6 -> c_j in the world
        gx = circles[j][0] * math.cos(h) - circles[j][1] * math.sin(h) + x
        gy = circles[j][0] * math.sin(h) + circles[j][1] * math.cos(h) + y
        reach = math.hypot(hl, hw) + radius
        heading = math.atan2(-ey, -ex) - math.atan2(hw, hl)                  # the box's (+, +) corner points back at the car
        for a, off in ((0, +eps), (1, -eps)):
            dist = circles[j][2] + reach + margin + off
            agents[b, a, :, 0], agents[b, a, :, 1] = gx + dist * ex, gy + dist * ey
            agents[b, a, :, 2:] = [heading, hl, hw, radius]
        agents[b, 1, :, 3] = -1.0                                            # the hit: there at one sample alone
        agents[b, 1, k_hit, 3] = hl
        want_first[b] = k_hit
    return dict(traj=traj, agents=agents, scene_of=np.arange(B, dtype=np.int32), margin=margin, want_first=want_first,
                want_who=np.ones(B, np.int32))


# the shapes of the seeded cases: trajectory lengths around the wavefront, batches, agents per scene
MS = (1, 63, 64, 65, 130)
BATCHES = (1, 4, 5)
AGENTS = (0, 1, 3)


def seeded(m, B, a_max):
    """one case per shape, the seed from the shape: two scenes, ragged a_of and m_of (a 0 among them when the batch allows), stride 3 or 8"""
    rng = np.random.default_rng(1000 * m + 10 * B + a_max)
    stride = 3 if (m + B + a_max) % 2 else 8
    traj, agents = seeded_case(rng, B, m, 2, a_max, stride=stride)
    m_of = rng.integers(0, m + 1, B).astype(np.int32)
    m_of[0] = m
    if B > 1:
        m_of[1] = 0
    a_of = np.array([a_max, max(a_max - 1, 0)], np.int32)
    scene_of = (np.arange(B) % 2).astype(np.int32)
    return dict(id=f"m{m}-B{B}-A{a_max}", traj=traj, agents=agents, m_of=m_of, a_of=a_of, scene_of=scene_of, margin=0.3 if a_max == 3 else 0.0)


def seeded_cases():
    return [seeded(m, B, a) for m in MS for B in BATCHES for a in AGENTS]


def write_case(path, traj, agents, margin, m_of, a_of, scene_of):
    """the file tests/cpp/agents_demo.cpp reads; traj [B][m][stride >= 3], agents [n_scenes][a_max][m][6]"""
    traj, agents = np.asarray(traj, dtype=np.float64), np.asarray(agents, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(np.array(traj.shape[:2] + agents.shape[:2], np.int32).tobytes())
        f.write(np.array([margin], np.float64).tobytes())
        for a in (m_of, a_of, scene_of):
            f.write(np.asarray(a, np.int32).tobytes())
        f.write(np.ascontiguousarray(traj[:, :, :3]).tobytes())
        f.write(np.ascontiguousarray(agents).tobytes())
