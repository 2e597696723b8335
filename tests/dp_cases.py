"""Scenes that pin the costs and the parent choice of the DP corridor search (tests/test_dp_cases_cpu.py, tests/test_gpu_dp_cases.py).

The search (oracle/corridor_oracle.py::graph_search_dp, pqp_dp_body.inc on the device) returns bounds only: the chosen lateral index is seen
through the feasible run of samples the chosen node lies in.  These scenes are built so that the run depends on the costs, and so that no
decision of the search is within round-off of going the other way:

  margin_cost >= COST_MARGIN   one edge cost is a few operations on values <= 32, a few ulp = 1e-14; a node's total sums <= 140 of them,
                               <= 1e-12.  ocml's atan2 against libm's moves a total by that much and no more, so a gap of 1e-9 between the best
                               predecessor and the runner-up (three orders above) cannot flip.  Exact ties (gap 0) are counted apart: only the
                               tie scene has any, and there both sides compute the same bits.
  margin_d >= D_MARGIN         the distance is a float32 (bilinear sample, rounded); 1e-6 is more than 4 ulp of the threshold 1.2 (ulp 1.2e-7),
                               so no `d < 1.2` / `d > 1.2` test can come out differently: no bound entry is excusable.
  >= 5 distinct lateral indices on the chosen path.

Every scene is seeded numpy: a map of 300 x 150 cells of 0.2 m (the tie scene: 240 x 128 of 0.25 m, exact in binary), a spline of 18 knots, 20-45
layers (`long`: 73).  The distance layer is an input array and need not be a distance transform: `lanes` and `channel` write the values they want.
All scenes but `tie` share one map geometry and one knot count, so they batch into one launch.

  discs_*       round obstacles of radius 0.2-0.8 m within 3 m of a gently curved line, road edges 7.5 m off it: several feasible runs per
                layer, left or right decided by the costs
  lanes_*       lanes 1.2 m apart along the road - every other lateral sample is a divider - with blocked stretches and gaps in the dividers
  narrow        lateral grid 3.0 / 0.2: 31 samples, window of 17 predecessors (a strict subset), a winding channel
  full          lateral grid 2.4 / 0.6 with layers 2.4 m apart: 9 samples, the window covers the whole layer
  long          layers 0.7 m apart, 73 of them: the channel winds across the chunk boundaries and the wrap of the ring of 33 prepared layers
                (layers 32 / 33 and 64 / 65)
  short_last    the last layer 0.3 m behind the one before it: a window of 1 + 1 + 1 there, 3 + 1 + 3 elsewhere
  wall          a wall across the road: the search stops midway, count = last reachable layer + 1
  tie           straight line along x, symmetric map, an obstacle dead ahead: left and right cost the same bits, the first one wins
"""
import functools
import math

import numpy as np

import corridor_oracle as K

COST_MARGIN = 1e-9
D_MARGIN = 1e-6
MIN_DISTINCT = 5
KNOTS = 18

GEOM = K.GridGeom.make(60.0, 30.0, 0.2, pos=(30.0, 0.0))           # x in [0, 60], y in [-15, 15]
TIE_GEOM = K.GridGeom.make(60.0, 32.0, 0.25, pos=(30.0, 0.0))


def cell_centres(g):
    """x of every row and y of every column (grid_map: index 0 is the largest coordinate)"""
    cx = (g.pos_x + 0.5 * g.length_x - 0.5 * g.resolution) - g.resolution * np.arange(g.rows)
    cy = (g.pos_y + 0.5 * g.length_y - 0.5 * g.resolution) - g.resolution * np.arange(g.cols)
    return cx, cy


def _line(amp, period, phase, x0=4.0, x1=56.0):
    """18 knots along x on y = amp sin(2 pi x / period + phase), abscissa = chord length"""
    x = np.linspace(x0, x1, KNOTS)
    y = amp * np.sin(2.0 * np.pi * x / period + phase) if amp else np.zeros(KNOTS)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    tab, ext = K.pack_spline(sx, sy)
    centre = (lambda q: amp * np.sin(2.0 * np.pi * q / period + phase)) if amp else (lambda q: np.zeros_like(q))
    return dict(sx=sx, sy=sy, tab=tab, ext=ext, s_end=float(s[-1]), centre=centre, x0=x0)


def _scene(name, line, dist, length, start_off=(0.2, 0.3, 0.03), prm=None, geom=GEOM):
    sx, sy = line["sx"], line["sy"]
    h0 = math.atan2(K.spline_deriv(sy, 1, 0.0), K.spline_deriv(sx, 1, 0.0))
    start = (K.spline_eval(sx, 0.0) + start_off[0], K.spline_eval(sy, 0.0) + start_off[1], h0 + start_off[2])
    assert length <= line["s_end"]
    return dict(name=name, sx=sx, sy=sy, tab=line["tab"], ext=line["ext"], length=float(length), start=start,
                dist=np.asfortranarray(dist, dtype=np.float32), geom=geom, prm=prm or K.DpParams())


def _discs(seed, length=40.0):
    rng = np.random.default_rng(seed)
    line = _line(rng.uniform(0.5, 2.0), rng.uniform(50.0, 90.0), rng.uniform(0.0, 6.0))
    cx, cy = cell_centres(GEOM)
    X, Y = np.meshgrid(cx, cy, indexing="ij")
    d = 7.5 - np.abs(Y - line["centre"](X))                       # road edges
    for ox in np.arange(9.0, 48.0, 3.0):
        ox = ox + rng.uniform(-1.0, 1.0)
        oy = float(line["centre"](np.array(ox))) + rng.uniform(-3.0, 3.0)
        d = np.minimum(d, np.hypot(X - ox, Y - oy) - rng.uniform(0.2, 0.8))
    return _scene(f"discs_{seed}", line, np.clip(d, 0.0, 5.0), length)


def _lanes(seed, length=40.0):
    """lane centres at l = -10 + 1.2 k (the even lateral samples of the default grid on a line along y = 0), free value 2.0 ... 2.42 by lane
    (under 3: the distance term tells the lanes apart), dividers and blocked stretches 0.6; every few metres a stretch of two to five lanes is
    blocked and a divider is open (1.9)"""
    rng = np.random.default_rng(seed)
    line = _line(0.0, 1.0, 0.0)
    cx, cy = cell_centres(GEOM)
    X, Y = np.meshgrid(cx, cy, indexing="ij")
    lane = np.floor((Y + 10.0 + 0.3) / 1.2)                       # lane k covers l in [1.2 k - 0.3, 1.2 k + 0.3) about its centre; the rest is divider
    in_lane = (Y + 10.0 + 0.3) - 1.2 * lane < 0.6
    d = np.where(in_lane & (np.abs(Y) < 6.5), 2.0 + 0.07 * ((lane * 5) % 7), 0.6)
    for ox in np.arange(8.0, 52.0, 3.0):
        x_lo = ox + rng.uniform(-1.0, 1.0)
        k_lo = rng.integers(3, 11)
        blocked = (X > x_lo) & (X < x_lo + rng.uniform(1.5, 4.0)) & (lane >= k_lo) & (lane < k_lo + rng.integers(2, 6))
        d = np.where(blocked, 0.6, d)
    for ox in np.arange(6.0, 54.0, 2.0):
        x_lo = ox + rng.uniform(-1.0, 1.0)
        k = rng.integers(2, 13)
        gap = (X > x_lo) & (X < x_lo + rng.uniform(2.0, 5.0)) & (Y + 10.0 > 1.2 * k - 0.1) & (Y + 10.0 < 1.2 * (k + 1) + 0.1)
        d = np.where(gap, np.maximum(d, 1.9), d)
    return _scene(f"lanes_{seed}", line, d, length, start_off=(0.2, -0.4 + 1.2 * (seed % 3 - 1), 0.02))


def _channel(name, seed, length, prm, half_width, swing, period, harm=0.3, line_amp=1.0, wall_at=None):
    """a free channel of `half_width` about a centre that starts on the line and swings `swing` to either side of it every `period` metres;
    inside it the value falls from ~3.2 at the centre to 1.3 at the edge (so the own cost of a node depends on where in the channel it
    is), outside it is 0.4"""
    rng = np.random.default_rng(seed)
    line = _line(line_amp, rng.uniform(60.0, 90.0), rng.uniform(0.0, 6.0))
    cx, cy = cell_centres(GEOM)
    X, Y = np.meshgrid(cx, cy, indexing="ij")
    u = 2.0 * np.pi * (X - line["x0"]) / period
    off = np.abs(Y - line["centre"](X) - swing * np.sin(u) - harm * swing * np.sin(u / 0.37))
    d = np.where(off < half_width, 1.3 + 1.9 * (1.0 - off / half_width), 0.4)
    d = d + np.where(off < half_width, 0.2 * np.sin(3.1 * X + 1.7 * Y), 0.0)          # (ripples: no two nodes with the same own cost)
    if wall_at is not None:
        d = np.where(np.abs(X - wall_at) < 1.0, 0.4, d)
    return _scene(name, line, d, length, prm=prm, start_off=(0.2, 0.1, 0.02))


def _tie():
    """Straight line along x from x = 8 (from there on |l| cos(pi / 2) = 8 x 6e-17 is under half an ulp of x: a sample's x is the line's,
    for l and -l alike), y = 0 exactly, lateral grid 8 / 0.5 and cells of 0.25 m: every lateral offset, cell centre and interpolation weight is
    exact, so the samples at l and -l read mirrored cells with the same weights.  Free cells are 3.5 (>= 3: no distance term), obstacles 0: a
    block dead ahead, a wider one further on, then a funnel that leaves only l = 0 - the path has to come back to the line, and the node it
    comes back to has a left and a right predecessor of the same cost to the bit.  (atan2(-y, x) = -atan2(y, x) bit for bit in libm, and - the
    device test passes on this scene - in ocml.)"""
    g = TIE_GEOM
    line = _line(0.0, 1.0, 0.0, x0=8.0, x1=59.0)
    cx, cy = cell_centres(g)
    X, Y = np.meshgrid(cx, cy, indexing="ij")
    d = np.full(X.shape, 3.5)
    for x_lo, x_hi, half in ((16.0, 19.0, 1.6), (30.0, 34.0, 2.6)):
        d = np.where((X > x_lo) & (X < x_hi) & (np.abs(Y) < half), 0.0, d)
    d = np.where(np.abs(Y) > 7.0, 0.0, d)
    d = np.where((X > 42.0) & (np.abs(Y) > 0.3), 0.0, d)         # the road ends in a funnel one sample wide: the path comes back to l = 0
    assert np.array_equal(d, d[:, ::-1])
    prm = K.DpParams(lateral_range=8.0, lateral_spacing=0.5)
    return _scene("tie", line, d, 40.0, start_off=(0.0, 0.0, 0.0), prm=prm, geom=g)


DISC_SEEDS = (0, 8, 25, 43)
LANE_SEEDS = (13, 27, 59)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene, built once per process"""
    out = [_discs(seed) for seed in DISC_SEEDS] + [_lanes(seed) for seed in LANE_SEEDS]
    out.append(_channel("narrow", 11, 33.0, K.DpParams(lateral_range=3.0, lateral_spacing=0.2), half_width=0.9, swing=1.6, period=11.0))
    out.append(_channel("full", 12, 50.0, K.DpParams(lateral_range=2.4, longitudinal_spacing=2.4, lateral_spacing=0.6), half_width=0.8, swing=1.5, period=31.0))
    out.append(_channel("long", 13, 50.0, K.DpParams(longitudinal_spacing=0.7), half_width=0.8, swing=2.8, period=22.4, harm=0.0))
    out.append(_channel("short_last", 14, 0.2 + 1.5 * 24 + 0.3, K.DpParams(), half_width=1.5, swing=2.5, period=30.0, harm=0.15))
    out.append(_channel("wall", 15, 40.0, K.DpParams(), half_width=1.5, swing=2.5, period=30.0, harm=0.15, wall_at=30.0))
    out.append(_tie())
    return {sc["name"]: sc for sc in out}


NAMES = [f"discs_{s}" for s in DISC_SEEDS] + [f"lanes_{s}" for s in LANE_SEEDS] + ["narrow", "full", "long", "short_last", "wall", "tie"]
BATCHABLE = [n for n in NAMES if n.startswith(("discs", "lanes")) or n in ("short_last", "wall")]        # default lateral grid and layer spacing


@functools.lru_cache(maxsize=None)
def expected(name, knobs=None):
    """the oracle's result for a scene (shared, not to be modified); `knobs`: a tuple of (field, value) pairs of K.DpCostKnobs"""
    sc = scenes()[name]
    kn = K.DpCostKnobs(**dict(knobs)) if knobs else None
    return K.graph_search_dp(sc["sx"], sc["sy"], sc["length"], sc["start"], sc["dist"], sc["geom"], prm=sc["prm"], knobs=kn)


# the seven defects of the search that the scenes must tell from the reference's, as knob settings
MUTATIONS = {
    "w_prev_dir 16 -> 8": (("w_prev_dir", 8.0),),
    "w_heading 0.5 -> 0": (("w_heading", 0.0),),
    "last wins on ties": (("tie_first", False),),
    "no distance term": (("w_dist", 0.0),),
    "no |l| term": (("w_lateral", 0.0),),
    "window ds -> ds / 2": (("window_factor", 0.5),),
    "layer heading for the incoming direction": (("use_prev_dir", False),),
}


# ---- one launch of several scenarios on several maps -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch():
    """Seven scenarios on four maps (map_of), one launch: four that run through, the stopped one, one whose vehicle is 12 m off its line
    (count 0) and one whose line needs more layers than max_layers (count -1).  Returns the flat arrays of the C ABI and, per scenario, what
    the oracle is to be run on."""
    sc = scenes()
    maps = ["discs_0", "lanes_27", "short_last", "wall"]
    rows = [("discs_0", "discs_0", None, None), ("lanes_27", "lanes_27", None, None), ("far", "discs_0", "far", None), ("short_last", "short_last", None, None),
            ("wall", "wall", None, None), ("too_long", "lanes_27", None, 50.0), ("discs_on_lanes", "lanes_27", "discs_0", None)]
    names, lines, starts, lengths, map_of = [], [], [], [], []
    for name, map_name, line_name, length in rows:
        line = sc["discs_0" if line_name in ("far", "discs_0") else map_name]
        start = line["start"]
        if line_name == "far":
            start = (start[0], start[1] + 12.0, start[2])
        names.append(name); lines.append(line); starts.append(start); map_of.append(maps.index(map_name))
        lengths.append(line["length"] if length is None else length)
    return dict(names=names, lines=lines, map_of=map_of, max_layers=30,
                tab=np.stack([l["tab"] for l in lines]), ext=np.stack([l["ext"] for l in lines]), length=np.array(lengths), start=np.array(starts),
                dist=np.stack([np.ascontiguousarray(sc[m]["dist"]) for m in maps]))


@functools.lru_cache(maxsize=None)
def batch_expected(q):
    b = batch()
    line = b["lines"][q]
    return K.graph_search_dp(line["sx"], line["sy"], float(b["length"][q]), tuple(b["start"][q]), np.asfortranarray(b["dist"][b["map_of"][q]]), GEOM)


def batch_count(want, max_layers):
    """the count the device reports for an oracle result: 0 when the reference returns false, -1 when the layers do not fit"""
    if want is None:
        return 0
    return -1 if want["n_layers_sampled"] > max_layers else len(want["lb"])
