"""pqp_project_points on the GPU: many points onto their reference lines (getProjection + global2Local, src/tools/tools.cpp:57-126) against
the Python restatement (tests/project_util.py over oracle/corridor_oracle.py), bit for bit against the projection pqp_reference_length
already ships, round trips through pqp_offsets_to_points, the shapes and edges where the kernel can go wrong, and behind the chain.
Run with -m gpu on an MI355X."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import chain_util
import corridor_oracle as K
import corridor_util as U
import cpp_demo
import project_util as P
from path_optimizer_2_amd import capi

pytestmark = pytest.mark.gpu

TOL = P.PROJECT_TOL
LENGTHS = (30.0, 30.0, 25.5, 28.0)
TILE = capi.PROJECT_TILE_SAMPLES


@pytest.fixture(scope="module")
def handle(hip_lib):
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def lines():
    """the four lines of test_reference_length_up_to_the_target with 300 seeded points each and the oracle's rows for them (computed once)"""
    cs = [U.build(seed=s, n=10) for s in (40, 41, 42, 43)]
    pts = np.stack([P.scattered_points(c, L, 300, seed=400 + q) for q, (c, L) in enumerate(zip(cs, LENGTHS))])
    want = [P.project_many(c["sx"], c["sy"], L, p) for c, L, p in zip(cs, LENGTHS, pts)]
    return dict(cs=cs, tab=np.stack([c["tab"] for c in cs]), ext=np.stack([c["ext"] for c in cs]), length=np.array(LENGTHS), pts=pts,
                proj=np.stack([w[0] for w in want]), flags=np.stack([w[1] for w in want]), amb=np.stack([w[2] for w in want]))


def _close(got, want, what=None):
    np.testing.assert_allclose(got, want, rtol=0, atol=TOL, err_msg=str(what))


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------------
def test_scattered_points_against_the_oracle(handle, lines):
    proj, flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], lines["pts"])
    amb = lines["amb"]
    clipped = int((lines["flags"] & P.AT_END != 0).sum())
    print(f"ambiguous {int(amb.sum())} of {amb.size}; not converged {int((lines['flags'] & P.NOT_CONVERGED != 0).sum())}; at the end {clipped}; "
          f"before the start {int((lines['flags'] & P.BEFORE_START != 0).sum())}; worst |error| {np.abs(proj - lines['proj'])[~amb].max():.2e}")
    assert amb.sum() <= 0.01 * amb.size
    # the oracle's own count on exactly these 1200 points, so that a drift of the generator or of the restatement shows: no decision within
    # rounding, every Newton run converged, 101 points clipped at the end, 98 left of the start
    assert amb.sum() == 0 and (lines["flags"] & P.NOT_CONVERGED != 0).sum() == 0
    assert clipped == 101 and (lines["flags"] & P.BEFORE_START != 0).sum() == 98
    ok = ~amb
    _close(proj[ok], lines["proj"][ok])
    assert np.array_equal(flags[ok], lines["flags"][ok])
    # the exact tie of the integer-length lines - the end sample is the grid's last sample bit for bit - is not left out
    for q in (0, 1):
        c = lines["cs"][q]
        tie = [i for i in range(300) if lines["flags"][q, i] & P.AT_END and not amb[q, i]]
        assert tie, q
        assert all(proj[q, i, 0] == LENGTHS[q] for i in tie)
        tr = P.trace(c["sx"], c["sy"], LENGTHS[q], *lines["pts"][q, tie[0], :2])
        assert tr["end"] == tr["coarse"][-1]


# ---- 2. bit-identity with the projection the library already ships -----------------------------------------------------------------------
@pytest.mark.parametrize("long_lines", [0, 2])
def test_s_is_bit_for_bit_what_reference_length_returns(hip_lib, lines, long_lines):
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    h.set_option(capi.OPT_LONG_LINES, long_lines)
    proj, _ = h.project_points(lines["tab"], lines["ext"], lines["length"], lines["pts"])
    rows, tabs, exts, lens, tgts = [], [], [], [], []
    for q, (c, L) in enumerate(zip(lines["cs"], LENGTHS)):
        ex, ey, eh, _ = P.state_at(c["sx"], c["sy"], L)
        for i, p in enumerate(lines["pts"][q]):
            local_x = (p[0] - ex) * math.cos(eh) + (p[1] - ey) * math.sin(eh)          # setReferencePathLength projects only behind the end
            if local_x < -1e-9:
                rows.append((q, i)); tabs.append(lines["tab"][q]); exts.append(lines["ext"][q]); lens.append(L); tgts.append(p)
    assert len(rows) > 900
    got = h.reference_length(np.stack(tabs), np.stack(exts), np.array(lens), np.stack(tgts))
    h.close()
    np.testing.assert_array_equal(np.array([proj[q, i, 0] for q, i in rows]), got)


# ---- 3. round trip through pqp_offsets_to_points -------------------------------------------------------------------------------------------
def test_round_trip_through_offsets_to_points(handle, lines):
    rng = np.random.default_rng(77)
    n = 64
    at_s = np.stack([np.sort(rng.uniform(0.0, L, n)) for L in LENGTHS])
    l = rng.uniform(-2.0, 2.0, (4, n))
    x, y, _ = handle.offsets_to_points(lines["tab"], lines["ext"], at_s, l)
    pts = np.stack([x, y], axis=2)
    proj, flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], pts)
    for q, (c, L) in enumerate(zip(lines["cs"], LENGTHS)):
        want, wflags, amb = P.project_many(c["sx"], c["sy"], L, pts[q])
        ok = ~amb
        assert ok.sum() >= n - 1
        _close(proj[q][ok], want[ok], q)
        assert np.array_equal(flags[q][ok], wflags[ok])
        # what comes back is (s, l) to the Newton stop's own error, which the oracle shows on the same points
        # (a point within a metre of a line's end may be clipped there - the end sample wins the scan and Newton is skipped: its s is
        #  off by up to the distance to the end, in the oracle as on the device; where Newton ran, its last step was below 1e-5)
        newton = ok & (wflags & P.AT_END == 0)
        assert newton.sum() >= n - 8 and np.abs(want[newton, 0] - at_s[q][newton]).max() < 1e-5
        for col, src in ((0, at_s[q]), (1, l[q])):
            bound = np.abs(want[ok, col] - src[ok]).max()
            assert np.abs(proj[q][ok, col] - src[ok]).max() <= bound + TOL
        assert (proj[q][ok, 3] == 0.0).all()                             # no heading given


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_max", [1, 63, 64, 65, 256, 257])
def test_point_counts_around_the_wavefront_and_the_workgroup(handle, lines, q_max):
    """batch 5 (line 0 twice) with ragged counts, 0 among them; rows beyond a line's count are zeros with flag 0; batch 1 gives the same bits"""
    idx = [0, 1, 2, 3, 0]
    q_of = np.array([q_max, 0, q_max // 2, max(q_max - 1, 0), min(q_max, 3)], np.int32)
    pts = np.ascontiguousarray(lines["pts"][idx, :q_max])
    proj, flags = handle.project_points(lines["tab"][idx], lines["ext"][idx], lines["length"][idx], pts, q_of=q_of)
    for b, q in enumerate(idx):
        k = int(q_of[b])
        ok = ~lines["amb"][q, :k]
        _close(proj[b, :k][ok], lines["proj"][q, :k][ok], (b, q))
        assert np.array_equal(flags[b, :k][ok], lines["flags"][q, :k][ok])
        assert (proj[b, k:] == 0.0).all() and (flags[b, k:] == 0).all()
    one, one_flags = handle.project_points(lines["tab"][:1], lines["ext"][:1], lines["length"][:1], pts[:1])
    assert np.array_equal(one[0], proj[0]) and np.array_equal(one_flags[0], flags[0])
    k = int(q_of[4])
    assert np.array_equal(proj[4, :k], proj[0, :k])                      # the same line and points in another row of the batch
    # counts beyond q_max and below 0 are clamped
    wild, wild_flags = handle.project_points(lines["tab"][:2], lines["ext"][:2], lines["length"][:2], pts[:2], q_of=np.array([q_max + 9, -4], np.int32))
    assert np.array_equal(wild[0], proj[0]) and (wild[1] == 0.0).all() and (wild_flags[1] == 0).all()


def test_strides_give_the_same_bits(handle, lines):
    q_max = 70
    p3 = np.ascontiguousarray(lines["pts"][:, :q_max])
    p7 = np.full((4, q_max, 7), 123.0); p7[:, :, :3] = p3
    p2 = np.ascontiguousarray(p3[:, :, :2])
    base, base_flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], p3)
    got7, flags7 = handle.project_points(lines["tab"], lines["ext"], lines["length"], p7)
    got2, flags2 = handle.project_points(lines["tab"], lines["ext"], lines["length"], p2)
    assert np.array_equal(got7, base) and np.array_equal(flags7, base_flags)
    cols = [0, 1, 2, 4, 5, 6, 7]
    assert np.array_equal(got2[:, :, cols], base[:, :, cols]) and np.array_equal(flags2, base_flags) and (got2[:, :, 3] == 0.0).all()
    assert np.abs(base[:, :, 3]).max() > 0.1
    # a heading that is there but not asked for is not read
    p3n = p3.copy(); p3n[:, :, 2] = np.nan
    got, _ = handle.project_points(lines["tab"], lines["ext"], lines["length"], p3n, has_heading=False)
    assert np.array_equal(got, got2)


def test_the_same_point_at_every_position_of_a_tile(handle, lines):
    q_max = 256 + 64
    pts = np.repeat(lines["pts"][:, 5:6], q_max, axis=1)
    proj, flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], pts)
    assert (proj == proj[:, :1]).all() and (flags == flags[:, :1]).all()
    assert np.array_equal(proj[:, 0], handle.project_points(lines["tab"], lines["ext"], lines["length"], lines["pts"])[0][:, 5])


# ---- 5. the border between two tiles of coarse samples -------------------------------------------------------------------------------------
def test_minimum_carried_across_the_tile_border(handle):
    """One straight line of TILE + 70 m with knots every 0.375 m: more knots than the kernels that stage the table in LDS take, so there is
    no cap.  Knots and values are multiples of 1/8, so the spline is x = s exactly and a point above s = TILE - 0.5 is exactly equidistant
    from the last sample of tile 0 and the first of tile 1.  (On a straight line Newton lands on the same abscissa from either sample, so
    what the tie shows is the oracle's s, bit for bit; test_rival_minima_in_two_tiles is where the start sample decides.)"""
    L = float(TILE + 70)
    s = np.arange(0.0, L + 0.375, 0.375)
    assert 9 * len(s) * 8 > U.LDS_PER_CU
    sx, sy = K.spline_fit(s, s.copy()), K.spline_fit(s, np.zeros_like(s))
    tab, ext = K.pack_spline(sx, sy)
    xs = [TILE - 1.2, TILE - 0.7, TILE - 0.5, TILE - 0.3, TILE + 0.2, TILE + 0.5, TILE + 1.4, 0.2, 500.25, TILE + 35.5, L - 0.25, L + 2.0, -1.5,
          TILE / 2 - 0.5, 2.0 * TILE, TILE - 1.0]
    pts = np.array([[x, 3.0 if i % 2 else -1.25, 0.1 * i] for i, x in enumerate(xs)])
    tr = P.trace(sx, sy, L, TILE - 0.5, -1.25)
    assert tr["coarse"][TILE - 1] == tr["coarse"][TILE] == min(tr["coarse"])          # the exact tie across the border
    want, wflags, amb = P.project_many(sx, sy, L, pts)
    assert not amb.any()
    proj, flags = handle.project_points(tab[None], ext[None], np.array([L]), pts[None])
    _close(proj[0], want)
    assert np.array_equal(flags[0], wflags)
    inside = [i for i, x in enumerate(xs) if 0.0 <= x <= L]
    assert np.array_equal(proj[0, inside, 0], np.array(xs)[inside])          # x = s exactly: Newton's one step lands on it
    assert proj[0, 2, 0] == TILE - 0.5 and flags[0, 11] == P.AT_END and flags[0, 12] == P.BEFORE_START and flags[0, 14] == P.AT_END


def _hairpin(leg=540.0, R=20.0):
    """a line that folds back: `leg` metres out along y = 0, a half circle of radius R, `leg` metres back along y = 2 R; a knot per metre of
    arc.  1142.8 m: the return leg crosses the tile border at x = 118.8, and a point between the legs has a local minimum in either tile"""
    L = 2 * leg + math.pi * R
    s = np.append(np.arange(0.0, L, 1.0), L)
    back = leg + math.pi * R
    x = np.where(s <= leg, s, np.where(s >= back, leg - (s - back), leg + R * np.sin((s - leg) / R)))
    y = np.where(s <= leg, 0.0, np.where(s >= back, 2 * R, R - R * np.cos((s - leg) / R)))
    return s, x, y, L


def test_rival_minima_in_two_tiles(hip_lib):
    """Where the start sample decides the answer: on the hairpin a point near one leg has a second local minimum on the other leg, hundreds
    of metres of arc away and - for x below 118.8 - in the other tile.  A minimum that is not carried from tile 0 to tile 1, a sample index
    without its tile's base, or a tile overwritten while it is still being scanned all end on the wrong leg.  16 points against the
    oracle; 512 points (two workgroups) bit for bit against reference_length's projection on a PQP_OPT_LONG_LINES handle."""
    s, x, y, L = _hairpin()
    assert TILE < L < 2 * TILE
    sx, sy = K.spline_fit(s, x), K.spline_fit(s, y)
    tab, ext = K.pack_spline(sx, sy)
    bx = 540.0 - (TILE - 540.0 - math.pi * 20.0)                 # the return leg's x at s = TILE
    near = [(60.3, 8.0), (100.7, -3.0), (118.2, 12.5), (300.4, 6.0),          # nearest on the outward leg (tile 0), the return leg above them a rival
            (60.3, 31.0), (100.7, 44.0), (30.6, 27.5), (5.2, 38.0),           # nearest on the return leg beyond the border (tile 1)
            (bx + 0.4, 33.0), (bx - 0.6, 33.0), (bx + 1.5, 41.0), (bx - 1.5, 29.0),          # the return leg right at the border
            (300.4, 30.0), (555.0, 21.0), (570.0, 5.0), (-4.0, 36.0)]         # return leg within tile 0, inside and outside the turn, past the end
    pts = np.array([[a, b, 0.1 * i] for i, (a, b) in enumerate(near)])
    want, wflags, amb = P.project_many(sx, sy, L, pts)
    assert not amb.any()
    # the oracle's own scan says that these points do what they are here for
    coarse = [np.array(P.trace(sx, sy, L, a, b)["coarse"]) for a, b in near]
    first = [int(np.argmin(c)) for c in coarse]
    in_tile0, in_tile1 = [int(np.argmin(c[:TILE])) for c in coarse], [int(np.argmin(c[TILE:])) + TILE for c in coarse]
    for i in range(4):          # the answer is in tile 0 and tile 1's own minimum, hundreds of metres of arc away, must not replace it
        assert first[i] == in_tile0[i] and abs(want[i, 0] - near[i][0]) < 1e-6 and abs(want[i, 0] - in_tile1[i]) > 500.0
    for i in range(4, 8):       # the answer is in tile 1: tile 0's minimum must give way, and the sample's index needs its tile's base
        assert first[i] == in_tile1[i] and abs(want[i, 0] - first[i]) < 1.0 and abs(want[i, 0] - in_tile0[i]) > 10.0
        assert abs(want[i, 0] - (first[i] - TILE)) > 500.0
    assert sorted(first[8:12]) == [TILE - 2, TILE, TILE + 1, TILE + 1]
    h = capi.Handle(capi.default_params(), max_batch=8, max_n=16)
    proj, flags = h.project_points(tab[None], ext[None], np.array([L]), pts[None])
    _close(proj[0], want)
    assert np.array_equal(flags[0], wflags) and flags[0, 15] == P.AT_END
    rng = np.random.default_rng(9)
    many = np.column_stack([rng.uniform(2.0, 575.0, 512), rng.uniform(-6.0, 46.0, 512)])          # all behind the line's end: it heads towards -x at x = 0
    proj, flags = h.project_points(tab[None], ext[None], np.array([L]), many[None], has_heading=False)
    h.set_option(capi.OPT_LONG_LINES, 2)
    got = h.reference_length(np.repeat(tab[None], 512, axis=0), np.repeat(ext[None], 512, axis=0), np.full(512, L),
                             np.column_stack([many, np.zeros(512)]))
    h.close()
    np.testing.assert_array_equal(proj[0, :, 0], got)
    assert (flags[0] & ~P.AT_END == 0).all()
    assert ((proj[0, :, 0] < TILE - 1).sum() > 100) and ((proj[0, :, 0] > TILE + 1).sum() > 40)          # both tiles hold answers


# ---- 6. edges --------------------------------------------------------------------------------------------------------------------------------
def test_lengths_that_are_no_lengths(handle, lines):
    pts = np.ascontiguousarray(lines["pts"][:3, :40])
    length = np.array([0.0, -2.0, math.nan])
    proj, flags = handle.project_points(lines["tab"][:3], lines["ext"][:3], length, pts)
    for q in range(3):
        want, wflags, _ = P.project_many(lines["cs"][q]["sx"], lines["cs"][q]["sy"], float(length[q]), pts[q])
        _close(proj[q], want, q)
        assert np.array_equal(flags[q], wflags)
        assert (proj[q, :, 0] == 0.0).all() and (flags[q] == (P.AT_END if q == 0 else 0)).all()
    # a length without an end: the scan would not stop - refused like a point that is not finite
    proj, flags = handle.project_points(lines["tab"][:2], lines["ext"][:2], np.array([math.inf, 2.0 ** 20]), pts[:2])
    assert np.isnan(proj).all() and (flags == P.NOT_FINITE).all()


def test_points_that_are_not_numbers_leave_their_neighbours_alone(handle, lines):
    pts = np.ascontiguousarray(lines["pts"][:, :130])
    base, base_flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], pts)
    bad = pts.copy()
    where = [(0, 0, 0, math.nan), (0, 64, 1, math.inf), (1, 63, 0, -math.inf), (2, 129, 2, math.nan), (3, 65, 1, math.nan), (3, 66, 2, math.inf)]
    for q, i, col, v in where:
        bad[q, i, col] = v
    proj, flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], bad)
    hit = np.zeros(flags.shape, bool)
    for q, i, _, _ in where:
        hit[q, i] = True
    assert np.isnan(proj[hit]).all() and (flags[hit] == P.NOT_FINITE).all()
    assert np.array_equal(proj[~hit], base[~hit]) and np.array_equal(flags[~hit], base_flags[~hit])


def test_a_point_far_to_the_left_of_the_start(handle, lines):
    pts = np.zeros((4, 3, 3))
    for q, c in enumerate(lines["cs"]):
        for i, (s0, off) in enumerate(((-8.0, 1.0), (-2.5, -3.0), (-15.0, 0.0))):
            pts[q, i, :2] = P.point_at(c["sx"], c["sy"], s0, off)
    proj, flags = handle.project_points(lines["tab"], lines["ext"], lines["length"], pts)
    for q, (c, L) in enumerate(zip(lines["cs"], LENGTHS)):
        want, wflags, amb = P.project_many(c["sx"], c["sy"], L, pts[q])
        assert not amb.any() and (want[:, 0] < 0.0).all() and (wflags & P.BEFORE_START).all()
        _close(proj[q], want, q)
        assert np.array_equal(flags[q], wflags)


def test_bad_arguments_are_refused_with_the_outputs_untouched(handle, lines):
    lib = handle.lib
    tab, ext, length = (np.ascontiguousarray(lines[k][:2]) for k in ("tab", "ext", "length"))
    pts = np.ascontiguousarray(lines["pts"][:2, :8])
    proj = np.full((2, 8, 8), 7.0); flags = np.full((2, 8), 7, np.int32)
    p = capi._ptr
    good = dict(batch=2, m=tab.shape[2], spline=p(tab), ext=p(ext), length=p(length), q_max=8, stride=3, has_heading=1, points=p(pts), proj=p(proj),
                flags=p(flags))
    def call(**over):
        a = {**good, **over}
        return lib.pqp_project_points(handle._h, a["batch"], a["m"], a["spline"], a["ext"], a["length"], a["q_max"], a["stride"], a["has_heading"],
                                      a["points"], None, a["proj"], a["flags"])
    for over in (dict(batch=0), dict(m=1), dict(q_max=0), dict(stride=1, has_heading=0), dict(stride=2), dict(spline=None), dict(ext=None),
                 dict(length=None), dict(points=None), dict(proj=None), dict(flags=None), dict(q_max=256 * 65535 + 1)):
        assert call(**over) == -1, over                                   # PQP_ERR_INVALID
        assert b"pqp_project_points" in lib.pqp_last_error()
        assert (proj == 7.0).all() and (flags == 7).all()
    assert lib.pqp_project_points_device(handle._h, 0, 6, None, None, None, 8, 3, 1, None, None, None, None) == -1
    assert call() == 0 and (flags != 7).all()
    assert call(stride=2, has_heading=0, points=p(np.ascontiguousarray(pts[:, :, :2]))) == 0


# ---- 7. behind the chain, and from C++ ----------------------------------------------------------------------------------------------------------
def test_a_planned_path_projects_onto_the_line_through_its_own_points(hip_lib):
    """pqp_optimize_path_device leaves `out` on the device; on the same stream: chord-length abscissae of its waypoints, pqp_spline_fit_var_device
    through them, pqp_project_points_device of the waypoints (stride 7, with heading) onto that line.  No host copy until all three ran."""
    import torch
    B = 4
    sc = chain_util.scenarios(B)
    h = capi.Handle(capi.production_params(), max_batch=B, max_n=256)
    hs = capi.Handle(chain_util.smoother_params(), max_batch=B, max_n=128)
    cfg = h.chain_config()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    n = cfg.n_max
    d_in = [t(sc["pts"], np.float64), t(sc["n_pts"], np.int32), t(sc["start"], np.float64), t(sc["target"], np.float64),
            t(np.ascontiguousarray(np.transpose(sc["dist"], (0, 2, 1))), np.float32), t(sc["map_of"], np.int32)]
    out = torch.zeros((B, n, 7), dtype=torch.float64, device=dev)
    ints = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
    tab = torch.zeros((B, 9, n), dtype=torch.float64, device=dev); ext = torch.zeros((B, 4), dtype=torch.float64, device=dev)
    proj = torch.full((B, n, 8), 7.0, dtype=torch.float64, device=dev); flags = torch.full((B, n), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    h._check(h.lib.pqp_optimize_path_device(h._h, hs._h, C.byref(cfg), B, sc["pts"].shape[1], p(d_in[0]), p(d_in[1]), p(d_in[2]), p(d_in[3]), p(d_in[4]),
                                            p(d_in[5]), C.byref(sc["geom"]), None, p(out), p(ints[0]), p(ints[1]), p(ints[2]), p(ints[3])))
    with torch.cuda.stream(torch.cuda.ExternalStream(h.stream(), device=dev)):
        x, y = out[:, :, 0].contiguous(), out[:, :, 1].contiguous()
        s = torch.zeros((B, n), dtype=torch.float64, device=dev)
        s[:, 1:] = torch.cumsum(torch.sqrt((x[:, 1:] - x[:, :-1]) ** 2 + (y[:, 1:] - y[:, :-1]) ** 2), dim=1)
        count = torch.where(ints[2] == 0, ints[0], torch.zeros_like(ints[0]))          # the paths that came through the chain
        # the line runs 2 m past its last knot (tk::spline extrapolates): getProjection hands a point to the end sample, without Newton,
        # when that is strictly closer than every 1 m grid sample - on a line that ended at the last waypoint it would clip the waypoints
        # of its last metre there
        length = (torch.gather(s, 1, (count.long() - 1).clamp(min=0)[:, None])[:, 0] + 2.0).contiguous()
        h._check(h.lib.pqp_spline_fit_var_device(h._h, B, n, p(count), p(s), p(x), p(y), p(tab), p(ext)))
        h._check(h.lib.pqp_project_points_device(h._h, B, n, p(tab), p(ext), p(length), n, 7, 1, p(out), p(count), p(proj), p(flags)))
    h.sync(); hs.sync()
    count, proj, flags, path, s = count.cpu().numpy(), proj.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy(), s.cpu().numpy()
    h.close(); hs.close()
    assert (count >= 20).sum() >= B - 1, count
    for b in range(B):
        k = int(count[b])
        assert (proj[b, k:] == 0.0).all() and (flags[b, k:] == 0).all()
        if k == 0:
            continue
        assert np.abs(proj[b, :k, 1]).max() < 1e-6                           # the waypoints are the line's knots
        assert (np.diff(proj[b, :k, 0]) > 0.0).all()
        assert np.abs(proj[b, :k, 0] - s[b, :k]).max() < 1e-4 and np.abs(proj[b, :k, 4:6] - path[b, :k, :2]).max() < 1e-6
        assert (flags[b, :k] == 0).all()


def test_the_cpp_projector_agrees_with_the_python_call(handle, lines, tmp_path):
    exe = cpp_demo.build("project_demo")
    sc = lines["cs"][2]["scene"]
    pts = lines["pts"][2, :40]
    path = tmp_path / "case.bin"
    P.write_case(path, sc["knots_s"], sc["knots_x"], sc["knots_y"], pts)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([[float(v) for v in ln.split()] for ln in r.stdout.strip().splitlines()])
    length = float(sc["knots_s"][-1])                                     # FrenetProjector::setLine: the line ends at its last knot
    tab, ext = handle.spline_fit(sc["knots_s"][None], sc["knots_x"][None], sc["knots_y"][None])
    proj, flags = handle.project_points(tab, ext, np.array([length]), pts[None])
    assert np.array_equal(got[:, :8], proj[0][:, [0, 1, 3, 4, 5, 6, 7, 2]]) and np.array_equal(got[:, 8].astype(np.int32), flags[0])
