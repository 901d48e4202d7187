"""The geodesic field kernel and the goal controller (csrc/cagym_ig_geodesic.h) at their structural edges: long chains, the seams
between the field kernel's four register strips, the diagonal rule, the tile's halo, and every branch of the controller - each met
by construction on the hand-made worlds of tests/geodesic_worlds.py and on fabricated fields, not by the luck of a generated world.

The unmarked tests assert, on ig.geodesic_spec / ig.goal_action_spec alone, what every world and every controller row was built
for, and on a numpy twin of the kernel's layout that each slip the layout invites changes a field the gpu test compares; the gpu
tests then hold InfoGain.geodesic and InfoGain.goal_actions to the same specifications bit for bit.  One env of
6 worlds x 5 slots with 2 robots per test; world 5 has its robots in slots 1 and 3 (rank differs from slot).

The closed loop runs in a serpentine of its own: the env's wall-collision test reads the raster with Map's y-flip and the distance
field reads it without, so a gap of the field's serpentine is a wall of the collision raster unless the raster is its
own y-flip - serpentine(transposed=True, phase=14) is."""
import heapq
import importlib
import math

import numpy as np
import pytest

import geodesic_worlds as gw
from oracle import oracle as orc
from test_ig_goals import _b32, _bits, _cell, _choice_of

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
igm = importlib.import_module("gym-exploration-2d_amd.ig")

N, M, R, K = 6, 5, 2, 24
INF = np.float32(np.inf)
ORTHO, DIAG = igm.GEO_ORTHO, igm.GEO_DIAG
Y_SERP, X_SERP, STAIRS, MIRROR, POCKET, OPEN = range(N)
WORLDS = (gw.serpentine(False), gw.serpentine(True), gw.staircase(missing=(7,)), gw.staircase(mirrored=True), gw.sealed_pocket(),
          gw.open_map())
SLOTS = ((0, 1),) * 5 + ((1, 3),)  # the robots' slots, world by world
BLOCKED_SOURCE = (19, 22)          # a cell of the pocket's west wall band with the pocket's (20, 22) next to it
OFF_MAP, NAN_POINT = (20.3, 3.1), (np.nan, 1.0)

# the sources [world][robot] of the three launches of the field test, as cells (i, j) - their centres are the points - or a point.
# A: corners everywhere, inside and outside the pocket.  B: written into A's tensors; a seam-row cell of either serpentine, a source
# in a blocked cell, the lonely cell.  C: the masked launch (C_MASK); the strip ends of the open map.  The staircases' B and C sources
# are cells of refused diagonals that straddle a seam or touch the border (STAIR_SOURCES says which): a wrong diagonal bit in a
# strip's first or last row changes only fields whose shortest ways cross the seam diagonally, from that side.
SRC_A = (((0, 0), (59, 59)), ((0, 0), (29, 30)), ((0, 59), (59, 0)), ((0, 0), (59, 59)), ((21, 22), (5, 50)), ((0, 0), (59, 59)))
SRC_B = (((30, 29), (0, 0)), ((59, 59), (0, 0)), ((31, 30), (9, 14)), ((46, 14), (35, 29)), (BLOCKED_SOURCE, gw.LONELY), ((59, 0), (0, 59)))
SRC_C = (((0, 0), (59, 59)), ((0, 0), (59, 59)), ((43, 44), (0, 3)), ((13, 45), (59, 3)), ((19, 19), OFF_MAP), ((29, 14), (30, 15)))
C_MASK = np.array([[0, 1], [1, 0], [1, 1], [5, 0], [1, 1], [1, 1]], dtype=np.uint8)
# where the robots stand (the field test does not care; goal_distance reads the field there): in a corridor and inside a wall
# band of the y-serpentine, off the map and in a corridor of the x-serpentine, anywhere in the other worlds
STAND = (((6, 20), (7, 20)), (OFF_MAP, (20, 9)), ((2, 30), (50, 8)), ((5, 5), (50, 50)), ((21, 21), (10, 40)), ((12, 12), (47, 31)))


def _point(src):
    return gw.centre(*src) if isinstance(src[0], (int, np.integer)) else src


def _points(table):
    return np.array([[_point(table[w][r]) for r in range(R)] for w in range(N)], dtype=np.float64)


def _ruleless(edf, point, radius):
    """ig.geodesic_spec without the diagonal rule - a mutant of the specification: every diagonal between two free cells is taken."""
    free = np.asarray(edf)[2::5, 2::5] > float(radius) + 0.1
    si, sj = _cell(point[0]), _cell(point[1])
    free = free.copy()
    free[sj, si] = True
    field = np.full((60, 60), np.inf, dtype=np.float32)
    field[sj, si] = 0.0
    heap = [(0.0, sj, si)]
    while heap:
        d, j, i = heapq.heappop(heap)
        if d > field[j, i]:
            continue
        for k, (di, dj) in enumerate(igm.GEO_NEIGHBOURS):
            ni, nj = i + di, j + dj
            if not (0 <= ni < 60 and 0 <= nj < 60 and free[nj, ni]):
                continue
            nd = np.float32(field[j, i] + (ORTHO if k < 4 else DIAG))
            if nd < field[nj, ni]:
                field[nj, ni] = nd
                heapq.heappush(heap, (float(nd), nj, ni))
    return field


def _spec(edf, src):
    return igm.geodesic_spec(edf, _point(src), 0.5)


# ---- 1. the worlds, on the specification alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
def test_the_serpentine_is_one_long_chain_of_one_cell_corridors(transposed):
    rects = gw.serpentine(transposed)
    assert rects.shape == (19, 4) and np.allclose(np.minimum(rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]), 0.1)
    free = gw.free_mask(rects)
    along = free.T if transposed else free  # [position along the corridors, across them]
    # one-cell-wide corridors: between the end gaps a cell is free iff its column is a corridor's, or beyond the last wall
    across = np.arange(60)
    want = (across % 3 == 0) | (across >= 57)
    assert (along[2:58] == want[None, :]).all()
    for k in range(19):  # the gap of wall k: both cells, two rows deep, at alternating ends and nowhere else
        ends = along[:, 3 * k + 1:3 * k + 3]
        assert ends[58:].all() and not ends[:58].any() if k % 2 == 0 else ends[:2].all() and not ends[2:].any()
    assert int(free.sum()) == 1396
    if not transposed:  # every corridor crosses the three strip seams
        for s in gw.SEAMS:
            assert free[s - 1:s + 1, 0:58:3].all() and not free[s - 1:s + 1, 1:57:3].any() and not free[s - 1:s + 1, 2:57:3].any()
    edf = gw.edf_of(rects)
    seam_source = (29, 30) if transposed else (30, 29)
    assert free[seam_source[1], seam_source[0]] and seam_source[1] + (0 if transposed else 1) in gw.SEAMS
    longest = {}
    for src in ((0, 0), (59, 59), seam_source):
        field, fr, cell = _spec(edf, src)
        assert cell == src and np.array_equal(fr, free)
        assert np.isfinite(field[free]).all() and (field[~free] == INF).all()  # every free cell is reached
        longest[src] = float(field[free].max())
    print("serpentine %s: longest ways %s" % ("x" if transposed else "y", {k: round(v, 1) for k, v in longest.items()}))
    assert longest[(0, 0)] > 500.0 and longest[(59, 59)] > 500.0 and longest[seam_source] > 250.0
    assert abs(longest[(0, 0)] - 599.9) < 0.1 and abs(longest[(59, 59)] - 571.7) < 0.1


@pytest.mark.parametrize("mirrored, missing", [(False, ()), (True, ()), (False, (7,)), (True, (7,))])
def test_the_staircase_puts_refused_diagonals_on_every_seam_and_on_the_border(mirrored, missing):
    rects = gw.staircase(mirrored=mirrored, missing=missing)
    assert len(rects) == 20 - len(missing) <= K
    free = gw.free_mask(rects)
    rd = gw.refused_diagonals(free)
    one, both = rd[:, 4] == 1, rd[:, 4] == 2
    counts = {s: (int((gw.on_seam(rd, s) & one).sum()), int((gw.on_seam(rd, s) & both).sum())) for s in gw.SEAMS}
    border = (int((gw.on_border(rd) & one).sum()), int((gw.on_border(rd) & both).sum()))
    print("staircase mirrored=%s missing=%s: %d refused with one orthogonal cell blocked, %d with both; on the seams %s, on the border %s"
          % (mirrored, missing, one.sum(), both.sum(), counts, border))
    for s in gw.SEAMS:
        assert counts[s][0] >= 1 and counts[s][1] >= 1, s
    assert border[0] >= 1 and border[1] >= 1
    # which diagonal bits: the NE-SW chain's corner touches refuse NW and SE moves, the mirrored chain's NE and SW ones
    dirs = {(int(a), int(b)) for a, b in rd[both][:, 2:4]}
    assert dirs == ({(1, 1), (-1, -1)} if mirrored else {(-1, 1), (1, -1)})
    # ... and along the blobs' flanks the other two are refused with one orthogonal cell blocked: the two chains cover all four bits
    # (round the hole a missing square leaves, all four)
    assert {(int(a), int(b)) for a, b in rd[one][:, 2:4]} == (set(gw.DIAGONALS) if missing else set(gw.DIAGONALS) - dirs)
    # without the rule the field differs on every seam, from a corner source
    edf = gw.edf_of(rects)
    src = (0, 0) if mirrored else (0, 59)
    field, fr, _ = _spec(edf, src)
    mutant = _ruleless(edf, _point(src), 0.5)
    differ = _bits(field) != _bits(mutant)
    print("    without the rule %d cells of the field from %s change" % (differ.sum(), src))
    for s in gw.SEAMS:
        assert differ[s - 1].any() and differ[s].any(), s
    assert differ[:, [0, 59]].any() or differ[[0, 59]].any()
    if not missing:  # the chain is closed: two free regions that touch at 19 corners and stay unconnected
        other = (59, 59) if mirrored else (59, 0)
        assert free[other[1], other[0]] and field[other[1], other[0]] == INF and np.isfinite(mutant[other[1], other[0]])
        back = _spec(edf, other)[0]
        assert ((field < INF) ^ (back < INF))[free].all()
    else:
        assert np.isfinite(field[free]).all()


# (world, source): (the seam's first row or "border", orthogonal cells blocked, the source is the upper or the lower cell of the pair)
STAIR_SOURCES = {(STAIRS, (31, 30)): (30, 1, "upper"), (STAIRS, (9, 14)): (15, 1, "lower"), (STAIRS, (43, 44)): (45, 2, "lower"),
                 (STAIRS, (0, 3)): ("border", 2, "upper"), (MIRROR, (46, 14)): (15, 2, "lower"), (MIRROR, (35, 29)): (30, 1, "lower"),
                 (MIRROR, (13, 45)): (45, 1, "upper"), (MIRROR, (59, 3)): ("border", 2, "upper")}


def test_the_chosen_staircase_sources_sit_on_refused_diagonals():
    """The B and C sources of the two staircase worlds are cells of a refused diagonal on the seam (or on the border) they were
    chosen for: the field's first relaxation step already meets the rule there, from either side of every seam between them."""
    assert {k for k in STAIR_SOURCES} == {(w, src) for w in (STAIRS, MIRROR) for src in SRC_B[w] + SRC_C[w]}
    for (w, src), (where, blocked, side) in STAIR_SOURCES.items():
        free = gw.free_mask(WORLDS[w])
        rd = gw.refused_diagonals(free)
        mine = rd[(rd[:, 0] == src[0]) & (rd[:, 1] == src[1]) & (rd[:, 4] == blocked)]
        assert free[src[1], src[0]] and len(mine) >= 1, (w, src)
        assert gw.on_border(mine).all() if where == "border" else gw.on_seam(mine, where).all(), (w, src)
        assert (mine[:, 3] == (-1 if side == "upper" else 1)).all(), (w, src)
    seams = {(w, where, side) for (w, _), (where, _, side) in STAIR_SOURCES.items()}
    assert {(STAIRS, 30, "upper"), (STAIRS, 15, "lower"), (MIRROR, 45, "upper"), (MIRROR, 30, "lower")} <= seams


def test_the_pocket_is_sealed_and_the_lonely_cell_has_no_way_out():
    rects = gw.sealed_pocket()
    free, edf = gw.free_mask(rects), gw.edf_of(rects)
    lo, hi = gw.POCKET
    inside = np.zeros((60, 60), dtype=bool)
    inside[lo:hi, lo:hi] = True
    assert free[inside].all() and not free[lo - 2:hi + 2, lo - 2:hi + 2][~inside[lo - 2:hi + 2, lo - 2:hi + 2]].any()
    li, lj = gw.LONELY
    lonely = np.zeros((60, 60), dtype=bool)
    lonely[lj, li] = True
    # from inside: the pocket and nothing else; from outside: everything but the pocket and the lonely cell
    field = _spec(edf, SRC_A[POCKET][0])[0]
    assert np.array_equal(field < INF, inside)
    field = _spec(edf, SRC_A[POCKET][1])[0]
    assert np.array_equal(field < INF, free & ~inside & ~lonely)
    # the lonely cell: free, E N W S blocked, NW and SE free - its only exits are refused diagonals, the field is the single zero
    assert free[lj, li] and not (free[lj, li + 1] or free[lj + 1, li] or free[lj, li - 1] or free[lj - 1, li])
    assert free[lj + 1, li - 1] and free[lj - 1, li + 1]
    field = _spec(edf, gw.LONELY)[0]
    assert np.array_equal(field < INF, lonely) and field[lj, li] == 0
    assert np.isfinite(_ruleless(edf, gw.centre(li, lj), 0.5)[free & ~inside]).all()
    # a source in a blocked cell of the west wall band: the source is free, its blocked neighbours are not, and the field leaves it
    # into the pocket alone (the band is two cells thick)
    bi, bj = BLOCKED_SOURCE
    assert not free[bj, bi] and free[bj, bi + 1] and not free[bj, bi - 1] and not free[bj + 1, bi] and not free[bj - 1, bi]
    field, fr, cell = _spec(edf, BLOCKED_SOURCE)
    assert cell == BLOCKED_SOURCE and fr[bj, bi] and field[bj, bi] == 0 and field[bj, bi + 1] == ORTHO
    assert field[bj + 1, bi + 1] > DIAG  # (the diagonal past the blocked (bi, bj + 1) is closed)
    assert np.array_equal(field < INF, inside | (np.arange(60)[None, :] == bi) & (np.arange(60)[:, None] == bj))
    # ... and one in the band's corner: E, N, W, S blocked, and the diagonal into the pocket's corner passes between two of them
    field = _spec(edf, SRC_C[POCKET][0])[0]
    assert int((field < INF).sum()) == 1
    assert _spec(edf, OFF_MAP)[2] is None and _spec(edf, NAN_POINT)[2] is None


def test_the_open_map_is_the_octile_distance():
    """No rectangle: d2 is the convention 2 * 300^2 everywhere, every cell is free, and the field is the octile distance - to the
    rounding of at most 59 fp32 additions (each within half an ulp of a sum below 64: 59 * 2^-19 m)."""
    edf = gw.edf_of(WORLDS[OPEN])
    assert gw.free_mask(WORLDS[OPEN]).all() and (edf == np.sqrt(2.0 * 300 * 300) * 0.1).all()
    for src in [s for table in (SRC_A, SRC_B, SRC_C) for s in table[OPEN]] + [(59, 0)]:
        field, _, cell = _spec(edf, src)
        assert cell == src and np.abs(field.astype(np.float64) - gw.octile(*src)).max() <= 59 * 2.0 ** -19, src
        # the straight lines of the field are exact: multiples of 0.5
        assert np.array_equal(field[src[1], :], (np.abs(np.arange(60) - src[0]) * 0.5).astype(np.float32))
        assert np.array_equal(field[:, src[0]], (np.abs(np.arange(60) - src[1]) * 0.5).astype(np.float32))
    assert {(0, 0), (59, 59), (0, 59), (59, 0), (29, 14), (30, 15)} == {s for table in (SRC_A, SRC_B, SRC_C) for s in table[OPEN]}


# ---- the kernel's layout on the CPU, and what the worlds catch -----------------------------------------------------------------------
MUTANTS = ("above", "below", "seam_north", "seam_south", "or_rule", "no_halo", "missed_store", "mirrored_bits")


def _kernel_twin(free, src, mutant=None, cap=3600):
    """k_ig_geodesic's data layout and one legal order of its sweeps, in numpy: a 62 x 62 tile with an infinite halo, the free mask
    with a halo of zeros, four strips of 15 rows per column; a sweep reads the two neighbour columns and the cells beyond a strip's
    ends as the last sweep left them and relaxes the strip upwards on its own new values; it ends on the sweep in which no thread
    stored.  Returns (field, sweeps).  mutant: one of MUTANTS - a slip of the kind the layout invites:
      above / below   a strip's last (first) cell takes its own value for the cell beyond the strip's end
      seam_north      the diagonal bits of a strip's last row take the cell to the north for free: it changes only fields whose
                      shortest ways cross a seam diagonally from above (seam_south: a strip's first row, the cell to the south)
      or_rule         a diagonal is allowed when ONE of its orthogonal cells is free
      no_halo         the tile has no halo columns: west of column 0 lies the last cell of the row below
      missed_store    the store of one thread (column 40, rows 15 .. 29) does not reach the workgroup's OR
      mirrored_bits   the NE and NW bits read each other's column"""
    si, sj = src
    fr = free.copy()
    fr[sj, si] = True
    F = np.pad(fr, 1)
    e, w, n, s = F[1:61, 2:62].copy(), F[1:61, 0:60].copy(), F[2:62, 1:61].copy(), F[0:60, 1:61].copy()
    if mutant == "seam_north":
        n[14::15] = True
    if mutant == "seam_south":
        s[15::15] = True
    both = (lambda a, b: a | b) if mutant == "or_rule" else (lambda a, b: a & b)
    ne, nw, sw, se = both(e, n), both(w, n), both(w, s), both(e, s)
    work = fr.copy()
    work[sj, si] = False
    tile = np.full((62, 62), INF, dtype=np.float32)
    tile[sj + 1, si + 1] = 0.0
    cur = tile[1:61, 1:61]  # (a view: a strip's registers and its cells of the tile hold the same values between two sweeps)
    inf = np.full((4, 60), INF, dtype=np.float32)
    for trip in range(cap):
        P = tile.copy()
        if mutant == "no_halo":
            P[1:, 0] = P[:-1, 60]
        changed = False
        for k in range(15):
            rows = np.arange(4) * 15 + k
            south = P[rows, 1:61] if k == 0 else cur[rows - 1]
            north = P[rows + 2, 1:61] if k == 14 else cur[rows + 1]
            if mutant == "below" and k == 0 or mutant == "above" and k == 14:
                south, north = (cur[rows], north) if k == 0 else (south, cur[rows])
            o = np.minimum(np.minimum(P[rows + 1, 2:62], P[rows + 1, 0:60]), np.minimum(north, south)) + ORTHO
            up_e, up_w = P[rows + 2, 2:62], P[rows + 2, 0:60]
            if mutant == "mirrored_bits":
                up_e, up_w = up_w, up_e
            d = np.minimum(np.minimum(np.where(ne[rows], up_e, inf), np.where(nw[rows], up_w, inf)),
                           np.minimum(np.where(sw[rows], P[rows, 0:60], inf), np.where(se[rows], P[rows, 2:62], inf))) + DIAG
            nv = np.minimum(o, d)
            assert nv.dtype == np.float32
            better = work[rows] & (nv < cur[rows])
            cur[rows] = np.where(better, nv, cur[rows])
            if mutant == "missed_store":
                better[1, 40] = False
            changed |= bool(better.any())
        if not changed:
            return cur.copy(), trip + 1
    return cur.copy(), cap + 1


def test_the_kernels_layout_on_the_cpu_equals_the_specification_and_its_slips_show():
    """The twin equals geodesic_spec bit for bit on a source of every world (its sweep counts are printed: the device's own order of
    reads may differ).  Every slip of MUTANTS changes some field of the gpu test's (world, source) pairs - named here per slip;
    how many of them an open map from its centre would let through is printed."""
    free = [gw.free_mask(x) for x in WORLDS]
    edf = [gw.edf_of(x) for x in WORLDS]
    sweeps = {}
    for w, src in ((Y_SERP, SRC_A[Y_SERP][1]), (X_SERP, SRC_A[X_SERP][0]), (STAIRS, SRC_B[STAIRS][0]), (MIRROR, SRC_C[MIRROR][1]),
                   (POCKET, BLOCKED_SOURCE), (POCKET, gw.LONELY), (OPEN, (59, 0))):
        field, n = _kernel_twin(free[w], src)
        assert np.array_equal(_bits(field), _bits(_spec(edf[w], src)[0])), (w, src)
        sweeps[(w, src)] = n
    print("sweeps of the twin: %s" % sweeps)
    assert max(sweeps.values()) <= 3600 and sweeps[(X_SERP, (0, 0))] > 1000 and sweeps[(POCKET, gw.LONELY)] == 1
    caught_by = {"above": [(Y_SERP, (59, 59))], "below": [(Y_SERP, (0, 0))], "seam_north": [(STAIRS, (31, 30)), (MIRROR, (13, 45))],
                 "seam_south": [(STAIRS, (9, 14)), (MIRROR, (35, 29))], "or_rule": [(MIRROR, (46, 14)), (POCKET, BLOCKED_SOURCE)],
                 "no_halo": [(OPEN, (59, 0)), (MIRROR, (59, 3))], "missed_store": [(X_SERP, (0, 0))],
                 "mirrored_bits": [(STAIRS, (0, 3)), (MIRROR, (13, 45))]}
    assert set(caught_by) == set(MUTANTS)
    hidden = 0
    for mutant, pairs in caught_by.items():
        for w, src in pairs:
            assert src in SRC_A[w] + SRC_B[w] + SRC_C[w]
            field, _ = _kernel_twin(free[w], src, mutant)
            differ = int((_bits(field) != _bits(_spec(edf[w], src)[0])).sum())
            print("    %-13s changes %4d cells of world %d from %s" % (mutant, differ, w, src))
            assert differ > 0, (mutant, w, src)
        plain, _ = _kernel_twin(free[OPEN], (30, 30), mutant)
        hidden += int(np.array_equal(_bits(plain), _bits(_spec(edf[OPEN], (30, 30))[0])))
    print("    %d of the %d slips leave the open map's field from its centre as it is" % (hidden, len(MUTANTS)))


# ---- the env of the gpu tests ------------------------------------------------------------------------------------------------------
def _env():
    B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
    a6 = np.zeros((N, M, 6))
    a6[:, :, 4], a6[:, :, 5] = 1.0, 0.2
    pol = np.full((N, M), scen.POLICY_STATIC, dtype=np.int32)
    h0 = np.zeros((N, M))
    for w in range(N):
        a6[w, :, 0], a6[w, :, 1] = 12.0 - 2.0 * np.arange(M), -13.9 + 0.3 * w  # the other agents: a row of static targets
        a6[w, :, 2:4] = a6[w, :, 0:2]
        for r, slot in enumerate(SLOTS[w]):
            pol[w, slot] = scen.POLICY_IGMCTS
            a6[w, slot] = [*_point(STAND[w][r]), 0.0, 0.0, 1.0, 0.5]
            h0[w, slot] = 0.3 * (w + 1) * (-1) ** r
    obst = np.zeros((N, K, 4))
    for w in range(N):
        obst[w, :len(WORLDS[w])] = WORLDS[w]
    env = B(N, M, max_obstacles=K, game_over_mode="agent0")
    env.set_scenarios(a6, pol, scen.DYN_FIRSTORDER, heading0=h0, n_agents=[M] * N, obstacles=obst, n_obst=[len(x) for x in WORLDS])
    env.reset()
    return env


def _poses(env):
    """positions [N, M, 2] and headings [N, M], read back"""
    import torch
    torch.cuda.synchronize()
    st = env.state()
    return np.stack([st["pos_x"].cpu().numpy(), st["pos_y"].cpu().numpy()], -1).reshape(N, M, 2), st["heading"].cpu().numpy().reshape(N, M)


def _edf(ig):
    """the read-back distance fields of the worlds' slots (no world has restarted: world w is on slot w), which are the CPU's
    (oracle.rasterize, oracle.edt) of the builders' rectangles"""
    edf = ig.edf().cpu().numpy()
    assert edf.shape == (N, 300, 300) and edf.dtype == np.float64
    for w in range(N):
        assert np.array_equal(edf[w], gw.edf_of(WORLDS[w])), w
    return edf


def _np(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _hold_to_spec(got, edf, table, pairs, what):
    """field, active and goal_xy of the (world, robot) pairs against geodesic_spec from the table's sources; sweeps within their bounds"""
    pts = _points(table)
    for w, r in pairs:
        want, _, cell = _spec(edf[w], table[w][r])
        assert got["active"][w, r] == (cell is not None), (what, w, r)
        bad = np.argwhere(_bits(got["field"][w, r]) != _bits(want))
        assert len(bad) == 0, (what, w, r, len(bad), bad[:5].tolist())
        assert np.array_equal(got["goal_xy"][w, r].view(np.uint64), pts[w, r].view(np.uint64)), (what, w, r)
        assert (1 <= got["sweeps"][w, r] <= 3600) if cell is not None else got["sweeps"][w, r] == 0, (what, w, r, got["sweeps"][w, r])
    print("sweeps %s: %s" % (what, got["sweeps"].tolist()))


# ---- 2. the field against the specification ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_field_equals_the_specification_on_every_hand_made_world():
    """One launch for the 12 (world, robot) pairs (A), a second into the same tensors with other sources (B: nothing of A survives),
    a third with a mask into tensors of a known pattern (C: a skipped pair keeps every byte next to serpentine pairs of 600 to 1100
    sweeps).  The sweep counts are printed and only bounded: reads across threads inside a sweep are unordered by design."""
    import torch
    env = _env()
    ig = igm.InfoGain(env)
    edf = _edf(ig)
    every = [(w, r) for w in range(N) for r in range(R)]
    out = ig.geodesic(points=_points(SRC_A), radius=0.5)
    a = _np(out)
    assert a["field"].shape == (N, R, 60, 60) and a["field"].dtype == np.float32 and a["sweeps"].dtype == np.int32
    _hold_to_spec(a, edf, SRC_A, every, "A")
    assert a["active"].all()
    again = ig.geodesic(points=_points(SRC_B), radius=0.5, out=out)
    assert again is out
    b = _np(out)
    _hold_to_spec(b, edf, SRC_B, every, "B")
    for w, r in every:  # (the specification's fields of A and B differ for every pair: a survivor of A would show)
        assert (_bits(a["field"][w, r]) != _bits(b["field"][w, r])).any(), (w, r)
    keep = {"field": torch.full((N, R, 60, 60), -7.0, dtype=torch.float32, device=env.device),
            "goal_xy": torch.full((N, R, 2), -7.0, dtype=torch.float64, device=env.device),
            "active": torch.full((N, R), 77, dtype=torch.uint8, device=env.device),
            "sweeps": torch.full((N, R), -3, dtype=torch.int32, device=env.device)}
    before = _np(keep)
    ig.geodesic(points=_points(SRC_C), mask=C_MASK, radius=0.5, out=keep)
    c = _np(keep)
    on = C_MASK != 0
    _hold_to_spec(c, edf, SRC_C, [p for p in every if on[p]], "C")
    for k in before:
        assert np.array_equal(c[k][~on].view(np.uint8), before[k][~on].view(np.uint8)), k
    assert not c["active"][POCKET, 1] and (c["field"][POCKET, 1] == INF).all()  # the point off the map: no source, all +inf
    env.close()


@pytest.mark.gpu
def test_goal_distance_is_the_field_at_the_robots_own_cell():
    """attach_ig_goals / ig_set_goals with the A sources: goal_distance is bit for bit the specification's field at the robot's cell,
    +inf for the robot that stands inside a wall band of the y-serpentine (a blocked cell) and for the one off the map.  Then goals
    given as window cells, which the kernel resolves through the robots' slots."""
    env = _env()
    env.attach_ig_learner(window=24, rotate=False)
    env.attach_ig_goals()
    env.reset()
    pos, _ = _poses(env)
    edf = _edf(env._igm.ig)
    env.ig_set_goals(_points(SRC_A))
    got = _np(env.ig_goals())
    finite = 0
    for w in range(N):
        for r, slot in enumerate(SLOTS[w]):
            assert np.array_equal(pos[w, slot], np.array(_point(STAND[w][r]))), (w, r)
            want = _spec(edf[w], SRC_A[w][r])[0]
            assert np.array_equal(_bits(got["field"][w, r]), _bits(want)), (w, r)
            ci, cj = _cell(pos[w, slot, 0]), _cell(pos[w, slot, 1])
            d = want[cj, ci] if 0 <= ci < 60 and 0 <= cj < 60 else INF
            assert _b32(got["goal_distance"][w, r]) == _b32(d), (w, r, got["goal_distance"][w, r], d)
            finite += int(np.isfinite(d))
    free = gw.free_mask(WORLDS[Y_SERP])
    (i0, j0), (i1, j1) = STAND[Y_SERP]
    assert free[j0, i0] and not free[j1, i1]
    assert np.isfinite(got["goal_distance"][Y_SERP, 0]) and got["goal_distance"][Y_SERP, 0] > 50.0  # two corridors away
    assert got["goal_distance"][Y_SERP, 1] == INF and got["goal_distance"][X_SERP, 0] == INF and finite >= 8
    assert got["active"].all() and not got["goal_reached"].any()
    # frame="window" finds each robot's pose by its RANK among the world's robots (world 5: slots 1 and 3): with rotate=False cell
    # (a, b) is the point pose + ((a - 11.5) / 2, (b - 11.5) / 2), one rounding per coordinate
    cells = np.array([[(14 + w, 9 + 3 * r) for r in range(R)] for w in range(N)], dtype=np.int32)
    env.ig_set_goals(cells, frame="window")
    got = _np(env.ig_goals())
    for w in range(N):
        for r, slot in enumerate(SLOTS[w]):
            q = pos[w, slot] + (cells[w, r] - 11.5) * 0.5
            assert np.array_equal(got["goal_xy"][w, r], q), (w, r, got["goal_xy"][w, r], q)
            want, _, cell = igm.geodesic_spec(edf[w], q, 0.5)
            assert got["active"][w, r] == (cell is not None) and np.array_equal(_bits(got["field"][w, r]), _bits(want)), (w, r)
    assert got["active"].sum() == N * R - 1 and not got["active"][X_SERP, 0]  # (the robot off the map: so is its window's cell)
    env.close()


# ---- 3. the controller on hand-made fields -----------------------------------------------------------------------------------------
CTL = dict(v_max=2.0, w_max=20.0, align_tol=np.pi / 4, goal_tol=0.01)
DT = 0.1
HOME = (30, 30)                      # the cell most rows stand in: x and y in 0 .. 0.5
HX, HY = gw.centre(*HOME)
FAR = gw.centre(5, 5)
RANGES = (2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66)  # igg_atan_pos: below each bound in turn, then at least 2^66


def _f32(x):
    return np.float32(x)


def _field_of(cells):
    f = np.full((60, 60), INF, dtype=np.float32)
    for (i, j), v in cells.items():
        f[j, i] = v
    return f


def _nb(k, at=HOME):
    return (at[0] + igm.GEO_NEIGHBOURS[k][0], at[1] + igm.GEO_NEIGHBOURS[k][1])


def _equal_key_diagonal():
    """an fp32 value d with fl32(d + GEO_DIAG) == fl32(1 + GEO_ORTHO) = 1.5"""
    d = _f32(_f32(1.5) - DIAG)
    for cand in (d, np.nextafter(d, INF), np.nextafter(d, -INF)):
        if _f32(cand + DIAG) == _f32(1.5):
            return cand
    raise AssertionError("no fp32 value whose diagonal key rounds to 1.5")


def _rounded_ties():
    """Two pairs (diagonal value, orthogonal value) whose fp32 keys are equal while the exact sums are not: in the first the
    diagonal's exact sum is the smaller, in the second the orthogonal's.  (The sum of two fp32 numbers is exact in fp64.)"""
    rng = np.random.default_rng(17)
    found = {}
    while len(found) < 2:
        o = _f32(rng.uniform(1.0, 60.0))
        key = _f32(o + ORTHO)
        d = _f32(key - DIAG)
        for cand in (d, np.nextafter(d, INF), np.nextafter(d, -INF)):
            exact_d, exact_o = float(cand) + float(DIAG), float(o) + float(ORTHO)
            if _f32(cand + DIAG) == key and exact_d != exact_o:
                found.setdefault(exact_d < exact_o, (cand, o))
    return found[True], found[False]


def _v_of(th, east):
    return igm.goal_action_spec(east, (HX, HY, th), FAR, dt=DT, **CTL)[0]


def _alignment_edge(sign, east):
    """The two adjacent doubles th between which the specification's v flips, for a robot in HOME that aims due east (atan2 = +0,
    err = wrap(-th)) and turns at the clamp: |rem| = |err| - w_max dt against align_tol.  sign: of err.  Returns (th with v = v_max,
    th with v = 0)."""
    inner, outer = -sign * (2.0 + np.pi / 4 - 1e-3), -sign * (2.0 + np.pi / 4 + 1e-3)
    assert _v_of(inner, east) == CTL["v_max"] and _v_of(outer, east) == 0.0
    while np.nextafter(inner, outer) != outer:
        mid = 0.5 * (inner + outer)
        if _v_of(mid, east) == 0.0:
            outer = mid
        else:
            inner = mid
    return inner, outer


def _controller_cases():
    """Every row of the controller test: dict(name, kind, pose (x, y, heading), goal (x, y), field [60, 60] f32, active)."""
    cases = []

    def add(name, kind, pose, goal, cells, active=1):
        cases.append(dict(name=name, kind=kind, pose=tuple(float(v) for v in pose), goal=tuple(float(v) for v in goal),
                          field=_field_of(cells), active=active))

    home = (HX + 0.05, HY - 0.1, 0.4)
    # equal keys: k = 0 .. 3 with a finite own cell (E, N, W, S open in turn), k = 4 .. 7 with an infinite one (every diagonal open)
    d_eq = _equal_key_diagonal()
    for k in range(8):
        cells = {_nb(n): (_f32(1.0) if n < 4 else d_eq) for n in range(k, 8)}
        if k < 4:
            cells[HOME] = _f32(2.0)
        add("equal keys from %d" % k, "equal", home, FAR, cells)
    for n, (d, o) in enumerate(_rounded_ties()):  # S (3) against NE (4), own cell infinite: the diagonal is open
        add("rounded tie %d" % n, "tie", home, FAR, {_nb(3): o, _nb(4): d})
    gate = {_nb(4): _f32(1.0), _nb(0): _f32(3.0), _nb(2): _f32(4.0)}  # NE smallest, N infinite
    add("diagonal refused", "gate", home, FAR, {**gate, HOME: _f32(5.0)})
    add("diagonal open", "gate", home, FAR, gate)
    add("no way out", "none", home, FAR, {HOME: _f32(1.0)})
    # the map's corners, in this order and in consecutive rows: a neighbour index that is not checked would read the row before or
    # behind, in this field or in the one stored next to it - the small values wait there
    decoy = _f32(0.125)
    add("corner (0, 59)", "corner", (*gw.centre(0, 59), 1.0), FAR, {(1, 59): 3.0, (0, 58): 3.0, (59, 58): decoy, (59, 59): decoy, (0, 59): decoy})
    add("corner (0, 0)", "corner", (*gw.centre(0, 0), 2.0), gw.centre(50, 50), {(1, 0): 3.0, (0, 1): 2.0, (0, 0): 9.0, (59, 0): decoy})
    add("corner (59, 59)", "corner", (*gw.centre(59, 59), -1.0), FAR, {(58, 59): 4.0, (59, 58): 4.0, (59, 59): decoy, (0, 59): decoy})
    add("corner (59, 0)", "corner", (*gw.centre(59, 0), 0.5), FAR, {(58, 0): 3.0, (59, 1): 2.5, (0, 1): decoy, (0, 2): decoy, (0, 0): decoy,
                                                                   (59, 0): decoy})
    add("off the map", "off", (15.3, 0.2, 0.1), FAR, {(59, 30): 1.0, (0, 30): 1.0, (0, 31): 1.0})
    add("off the map, below", "off", (0.2, -15.2, 0.1), FAR, {(30, 0): 1.0, (30, 59): 1.0})
    gx, gy = HX + 0.07, HY + 0.05
    add("goal in the own cell, slow", "own", (HX - 0.02, HY - 0.02, math.atan2(0.07, 0.09)), (gx, gy), {HOME: 0.0})
    add("at the goal", "reached", (gx - 0.004, gy + 0.005, 0.3), (gx, gy), {HOME: 0.0, _nb(0): 0.5})
    add("at the goal from the next cell", "reached", (0.5 - 0.004, HY, 0.3), (0.5 + 0.004, HY), {_nb(0): 0.0, HOME: 0.5})
    add("no active goal", "inactive", home, FAR, {_nb(0): 1.0}, active=0)
    # atan2: the aim is the goal point in the robot's own cell, (dy, dx) is free; the heading a little off the aim: not clipped
    shapes = ((1e-10, 0.2), (0.05, 0.2), (0.11, 0.2), (0.18, 0.2), (0.2, 0.11), (0.2, 0.02), (0.3, 1e-25))
    n = 0
    for ady, adx in shapes:
        for sx in (1, -1):
            for sy in (1, -1):
                if adx == 1e-25:  # |dy / dx| >= 2^66 near the origin: x = 1e-25 and 2e-25 lie in the same cell
                    x, gx = (1e-25, 2e-25) if sx > 0 else (2e-25, 1e-25)
                    y, gy = (0.1, 0.4) if sy > 0 else (0.4, 0.1)
                else:
                    x, y, gx, gy = HX, HY, HX + sx * adx, HY + sy * ady
                th = igm.atan2_spec(gy - y, gx - x) - 0.05 * (1 + n % 3) * (-1) ** n
                add("atan2 %g / %g (%+d, %+d)" % (ady, adx, sy, sx), "atan2", (x, y, th), (gx, gy), {HOME: 0.0})
                n += 1
    for dx, dy in ((0.0, 0.2), (0.0, -0.2), (0.2, 0.0), (-0.2, 0.0)):
        th = igm.atan2_spec(dy, dx) + 0.07
        add("atan2 axis (%g, %g)" % (dy, dx), "atan2", (HX, HY, th), (HX + dx, HY + dy), {HOME: 0.0})
    # the wrap: aim due east from the cell's centre (atan2 = +0), err = wrap(-heading); these turns are clipped, in both senses
    east = {_nb(0): _f32(1.0), HOME: _f32(1.5)}
    for base in (np.pi, -np.pi):  # the heading at +-pi, then one and two ulps inside (towards 0) and one and two outside
        one_in, one_out = np.nextafter(base, 0.0), np.nextafter(base, 2.0 * base)
        for th in (base, one_in, np.nextafter(one_in, 0.0), one_out, np.nextafter(one_out, 2.0 * base)):
            add("wrap %r" % th, "wrap", (HX, HY, th), FAR, east)
    for sign in (1, -1):
        for th in _alignment_edge(sign, _field_of(east)):
            add("alignment %r" % th, "align", (HX, HY, th), FAR, east)
    return cases


def _atan2_class(case):
    """(range of |dy / dx| in igg_atan_pos, or the axis) and the quadrant m of igg_atan2, for a row whose aim is its goal point"""
    dy, dx = case["goal"][1] - case["pose"][1], case["goal"][0] - case["pose"][0]
    m = (1 if math.copysign(1.0, dy) < 0 else 0) + (2 if math.copysign(1.0, dx) < 0 else 0)
    if dy == 0.0:
        return "dy == 0", m
    if dx == 0.0:
        return "dx == 0", m
    q = abs(dy / dx)
    return sum(q >= b for b in RANGES), m


def _specs_of(cases):
    out = []
    for c in cases:
        v, om, cell, reached = igm.goal_action_spec(c["field"], c["pose"], c["goal"], dt=DT, **CTL)
        out.append((v, om, _choice_of(cell, _cell(c["pose"][0]), _cell(c["pose"][1])), reached))
    return out


def test_every_controller_branch_is_met_by_construction():
    cases = _controller_cases()
    spec = _specs_of(cases)
    by = lambda kind: [(c, s) for c, s in zip(cases, spec) if c["kind"] == kind]
    # equal keys: the candidate order, one by one
    d_eq = _equal_key_diagonal()
    assert _f32(d_eq + DIAG) == _f32(_f32(1.0) + ORTHO)
    assert [s[2] for _, s in by("equal")] == list(range(8))
    # rounded ties: equal fp32 keys, unequal exact sums, the orthogonal cell - first in order - wins both
    (d0, o0), (d1, o1) = _rounded_ties()
    assert _f32(d0 + DIAG) == _f32(o0 + ORTHO) and float(d0) + float(DIAG) < float(o0) + float(ORTHO)
    assert _f32(d1 + DIAG) == _f32(o1 + ORTHO) and float(d1) + float(DIAG) > float(o1) + float(ORTHO)
    assert [s[2] for _, s in by("tie")] == [3, 3]
    assert [s[2] for _, s in by("gate")] == [0, 4]
    assert [s[:3] for _, s in by("none")] == [(0.0, 0.0, 255)]
    assert [s[2] for _, s in by("corner")] == [0, 1, 2, 1]
    assert [s for _, s in by("off")] == [(0.0, 0.0, 255, False)] * 2
    (_, own), = by("own")
    assert own[2] == 8 and CTL["goal_tol"] / DT < own[0] < CTL["v_max"] and abs(own[1]) < 1e-9
    assert [s for _, s in by("reached")] == [(0.0, 0.0, 255, True)] * 2
    # atan2: every range in every quadrant, both axes with both signs
    classes = {}
    for c, s in by("atan2"):
        assert s[2] == 8 and abs(s[1]) < CTL["w_max"] and s[1] != 0.0, c["name"]
        classes[_atan2_class(c)] = classes.get(_atan2_class(c), 0) + 1
    print("atan2 rows per (range, quadrant): %s" % sorted(classes.items(), key=str))
    want = {(rng, m) for rng in range(7) for m in range(4)} | {("dx == 0", 0), ("dx == 0", 1), ("dy == 0", 0), ("dy == 0", 2)}
    assert set(classes) == want
    # the wrap: a = atan2 - heading at -pi, just inside and just outside it, and the same at +pi; clipped turns of both senses
    a = [0.0 - c["pose"][2] for c, _ in by("wrap")]
    err = [s[1] for _, s in by("wrap")]
    assert a[0] == -np.pi and -np.pi < a[1] < a[2] < -3.14159 and -3.14160 < a[4] < a[3] < -np.pi
    assert a[5] == np.pi and np.pi > a[6] > a[7] > 3.14159 and 3.14160 > a[9] > a[8] > np.pi
    w = CTL["w_max"]
    # at -pi and inside it the turn is negative, outside it wraps to +pi; at +pi the sum a + pi is 2 pi and wraps to -pi, and so
    # does the double one ulp inside (a + pi rounds to 2 pi: ties to even); two ulps inside the turn is positive
    assert err == [-w, -w, -w, w, w, -w, -w, w, -w, -w] and all(s[0] == 0.0 and s[2] == 0 for _, s in by("wrap"))
    # the alignment threshold: adjacent doubles, v_max on one side and 0 on the other, for either sense of the turn
    al = by("align")
    for k in (0, 2):
        assert np.nextafter(al[k][0]["pose"][2], al[k + 1][0]["pose"][2]) == al[k + 1][0]["pose"][2]
        assert al[k][1][0] == CTL["v_max"] and al[k + 1][1][0] == 0.0 and abs(al[k][1][1]) == w
    assert al[0][1][1] == w and al[2][1][1] == -w
    counts = {}
    for c in cases:
        counts[c["kind"]] = counts.get(c["kind"], 0) + 1
    print("controller rows per class: %s (%d rows)" % (counts, len(cases)))
    first = [c["name"] for c in cases].index("corner (0, 59)")
    assert first % (N * R) >= 1 and first % (N * R) + 4 < N * R  # the four corner rows have a row before and behind them in their batch


@pytest.mark.gpu
def test_the_controller_equals_the_specification_on_every_branch():
    """Batches of 12 rows (6 worlds x 2 robots; world 5's robots in slots 1 and 3): the poses are written into the state, field,
    goal_xy and active are fabricated, the action table holds a pattern.  choice is exact, v bit for bit, omega bit for bit (float)
    of the specification's double on the read-back poses; every row of a non-robot or of a robot without an active goal is the
    caller's bit for bit."""
    import torch
    cases = _controller_cases()
    env = _env()
    ig = igm.InfoGain(env)
    P = ig.goal_params(R, radius=0.5, **CTL)
    st = env.state()
    pad = dict(cases[-1], name="padding", kind="pad")
    rng = np.random.default_rng(23)
    per = N * R
    differ = {"choice": 0, "v": 0, "omega": 0, "kept": 0}
    for b0 in range(0, len(cases), per):
        batch = (cases[b0:b0 + per] + [pad] * per)[:per]
        pos, th = _poses(env)
        for n, c in enumerate(batch):
            w, slot = n // R, SLOTS[n // R][n % R]
            pos[w, slot], th[w, slot] = c["pose"][:2], c["pose"][2]
        for key, val in (("pos_x", pos[:, :, 0]), ("pos_y", pos[:, :, 1]), ("heading", th)):
            st[key].copy_(torch.as_tensor(np.ascontiguousarray(val), device=env.device).reshape(st[key].shape))
        pos, th = _poses(env)  # read back
        goals = {"field": torch.as_tensor(np.stack([c["field"] for c in batch]).reshape(N, R, 60, 60), device=env.device),
                 "goal_xy": torch.as_tensor(np.array([c["goal"] for c in batch]).reshape(N, R, 2), device=env.device),
                 "active": torch.as_tensor(np.array([c["active"] for c in batch], dtype=np.uint8).reshape(N, R), device=env.device)}
        caller = rng.uniform(-3.0, 3.0, (N, M, 2)).astype(np.float32)
        table = torch.as_tensor(caller, device=env.device)
        choice = torch.full((N, R), 99, dtype=torch.uint8, device=env.device)
        ig.goal_actions(P, goals, table, choice)
        torch.cuda.synchronize()
        table, choice = table.cpu().numpy(), choice.cpu().numpy()
        robot_rows = set()
        for n, c in enumerate(batch):
            w, r, slot = n // R, n % R, SLOTS[n // R][n % R]
            robot_rows.add((w, slot))
            assert (pos[w, slot, 0], pos[w, slot, 1], th[w, slot]) == c["pose"], c["name"]
            if not c["active"]:
                differ["kept"] += int(not np.array_equal(_bits(table[w, slot]), _bits(caller[w, slot])) or choice[w, r] != 255)
                continue
            v, om, cell, _ = igm.goal_action_spec(c["field"], (pos[w, slot, 0], pos[w, slot, 1], th[w, slot]), c["goal"], dt=DT, **CTL)
            want = _choice_of(cell, _cell(pos[w, slot, 0]), _cell(pos[w, slot, 1]))
            bad = (choice[w, r] != want, _b32(table[w, slot, 0]) != _b32(v), _b32(table[w, slot, 1]) != _b32(np.float32(om)))
            if any(bad):
                print("row %r: choice %d (specification %d), v %r (%r), omega %r (%r)"
                      % (c["name"], choice[w, r], want, table[w, slot, 0], v, table[w, slot, 1], np.float32(om)))
            for key, flag in zip(("choice", "v", "omega"), bad):
                differ[key] += int(flag)
        for w in range(N):
            for k in range(M):
                if (w, k) not in robot_rows:
                    differ["kept"] += int(not np.array_equal(_bits(table[w, k]), _bits(caller[w, k])))
    print("controller: %d rows; rows that differ from the specification: %s" % (len(cases), differ))
    assert differ == {"choice": 0, "v": 0, "omega": 0, "kept": 0}
    env.close()


# ---- 4. closed loop through two gaps of a serpentine ------------------------------------------------------------------------------
LOOP_WORLD = gw.serpentine(transposed=True, phase=14)  # corridors along x in the rows 3 k + 1; its raster is its own y-flip
LOOP_CTL = dict(v_max=2.0, w_max=np.pi, align_tol=np.pi / 4, goal_tol=0.25)
# (start cell, heading, goal cell, the corridor rows on the way): west along row 4, up through wall 1's gap at the low end, east along
# row 7, up through wall 2's gap at the high end, west along row 10 - and the mirror image of it three rows higher
LOOPS = (((6, 4), np.pi, (52, 10), (4, 7, 10)), ((53, 7), 0.0, (7, 13), (7, 10, 13)))
LN, LM, LR = len(LOOPS), 3, 1


def _loop_scenario():
    a6 = np.zeros((LN, LM, 6))
    pol = np.full((LN, LM), scen.POLICY_STATIC, dtype=np.int32)
    h0 = np.zeros((LN, LM))
    for w, (start, th, _, _) in enumerate(LOOPS):
        a6[w, 0] = [*gw.centre(*start), *gw.centre(30, 55), 0.2, 0.5]  # (its scenario goal is far away and its time limit long)
        pol[w, 0], h0[w, 0] = scen.POLICY_IGMCTS, th
        for k in (1, 2):  # two static targets, out of the way
            a6[w, k] = [*gw.centre(20 * k, 40), *gw.centre(20 * k, 40), 1.0, 0.2]
    obst = np.zeros((LN, K, 4))
    obst[:, :len(LOOP_WORLD)] = LOOP_WORLD
    goals = np.array([[gw.centre(*goal)] for _, _, goal, _ in LOOPS])
    return dict(a6=a6, pol=pol, h0=h0, obst=obst, goals=goals,
                args=dict(heading0=h0, n_agents=[LM] * LN, obstacles=obst, n_obst=[len(LOOP_WORLD)] * LN))


def _loop_twin(max_steps=600):
    """The robots on the CPU: the oracle env, geodesic_spec's fields and goal_action_spec's actions as fp32 rows.  Returns, step by
    step until both have arrived, what the device must choose: (choice, v) [T, LN], the cells stood in, and the smallest distance of
    a robot from a cell border (a device pose differs from the twin's by rounding alone: that far from a border it is in the same cell)."""
    sc = _loop_scenario()
    env = orc.OracleEnv(LN, LM, max_obstacles=K, game_over_mode=orc.GO_AGENT0)
    env.set_scenario(sc["a6"], sc["pol"], scen.DYN_FIRSTORDER, **sc["args"])
    env.reset()
    edf = gw.edf_of(LOOP_WORLD)
    fields = [igm.geodesic_spec(edf, sc["goals"][w, 0], 0.5)[0] for w in range(LN)]
    rows, cells, margin, arrived = [], [], np.inf, np.full(LN, -1)
    for t in range(max_steps):
        pos, th = env.f("pos"), env.f("heading")
        acts = np.zeros((LN, LM, 2), dtype=np.float32)
        row = []
        for w in range(LN):
            x, y = pos[w, 0]
            v, om, cell, reached = igm.goal_action_spec(fields[w], (x, y, th[w, 0]), sc["goals"][w, 0], dt=DT, **LOOP_CTL)
            acts[w, 0] = v, om
            row.append((_choice_of(cell, _cell(x), _cell(y)), _b32(v)))
            for u in ((x + 15.0) * 2.0, (y + 15.0) * 2.0):
                margin = min(margin, abs(u - round(u)) * 0.5)
            if reached and arrived[w] < 0:
                arrived[w] = t
        rows.append(row)
        cells.append([(_cell(pos[w, 0, 0]), _cell(pos[w, 0, 1])) for w in range(LN)])
        if (arrived >= 0).all():
            break
        env.step(acts.astype(np.float64))
        assert not (env.u("in_collision")[:, 0] | env.u("ran_out_of_time")[:, 0] | env.u("is_at_goal")[:, 0]).any(), t
    return sc, fields, np.array(rows), cells, margin, arrived


def test_the_loop_world_is_its_own_flip_and_the_twin_passes_two_gaps():
    raster = gw.raster_of(LOOP_WORLD)
    assert np.array_equal(raster, raster[::-1]) and raster.any()
    free = gw.free_mask(LOOP_WORLD)
    assert free[0].all() and free[59].all()  # (the open rows beside the first and the last corridor)
    for j in range(1, 59):
        if j % 3 == 1:
            assert free[j].all(), j
        else:  # between two corridors: the wall's band, free only in the two cells of its gap
            k = (j - 2) // 3
            assert np.array_equal(np.flatnonzero(free[j]), [58, 59] if k % 2 == 0 else [0, 1]), j
    sc, fields, rows, cells, margin, arrived = _loop_twin()
    print("loop twin: arrived after %s steps, %.3g m from a cell border at the closest; choices %s"
          % (arrived.tolist(), margin, {int(c): int((rows[:, :, 0] == c).sum()) for c in np.unique(rows[:, :, 0])}))
    assert (arrived > 100).all() and margin > 1e-6
    for w, (start, _, goal, corridors) in enumerate(LOOPS):
        way = [c[w] for c in cells]
        assert way[0] == start and way[-1] == goal
        seen = [j for n, (i, j) in enumerate(way) if n == 0 or way[n - 1][1] != j]
        assert [j for j in seen if j in corridors] == list(corridors), seen       # the three corridors, in order
        gaps = {j for j in seen if j % 3 != 1}
        assert len(gaps) == 4 and all(i in (0, 1, 58, 59) for i, j in way if j % 3 != 1)  # both cells of two gaps, at the map's ends
    turning = int(((rows[:, :, 1] == _b32(0.0)) & (rows[:, :, 0] != 255)).sum())
    assert turning >= 4 * LN  # the turns at the gaps are made on the spot


@pytest.mark.gpu
def test_a_goal_driven_robot_threads_the_serpentine_as_on_the_cpu():
    """One robot per world with attach_ig_goals, through two gaps of a one-cell-wide serpentine: the device's choice and v equal the
    twin's at every step (the twin's poses stay 1e-6 m clear of every cell border, asserted on the CPU), and it arrives with it."""
    import torch
    B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
    sc, fields, rows, cells, margin, arrived = _loop_twin()
    env = B(LN, LM, max_obstacles=K, game_over_mode="agent0")
    env.set_scenarios(sc["a6"], sc["pol"], scen.DYN_FIRSTORDER, **sc["args"])
    env.reset()
    env.attach_ig_learner(window=24)
    env.attach_ig_goals(**LOOP_CTL)
    env.reset()
    env.ig_set_goals(sc["goals"])
    got = _np(env.ig_goals())
    for w in range(LN):
        assert np.array_equal(_bits(got["field"][w, 0]), _bits(fields[w])), w
    caller = torch.zeros((LN, LM, 2), dtype=torch.float32, device=env.device)
    differ, first = 0, np.full(LN, -1)
    for t in range(len(rows)):
        _, _, _, info = env.step(caller)
        torch.cuda.synchronize()
        choice, table = env._goals.choice.cpu().numpy(), env._act.cpu().numpy()
        for w in range(LN):
            bad = choice[w, 0] != rows[t, w, 0] or _b32(table[w, 0, 0]) != rows[t, w, 1]
            if bad and differ < 5:
                print("step %d world %d: choice %d v %r, the twin's %d %r" % (t, w, choice[w, 0], table[w, 0, 0], rows[t, w, 0],
                                                                             np.array([rows[t, w, 1]], dtype=np.uint32).view(np.float32)[0]))
            differ += int(bad)
        reached = info["goal_reached"].cpu().numpy()[:, 0]
        first = np.where((first < 0) & (reached != 0), t + 1, first)
    print("loop: %d steps, %d rows differ from the twin's; arrived after %s steps (twin %s)" % (len(rows), differ, first.tolist(), arrived.tolist()))
    assert differ == 0 and np.array_equal(first, arrived)
    assert not (env.flags.cpu().numpy()[:, 0] & (importlib.import_module("gym-exploration-2d_amd._lib").FLAG_IN_COLLISION)).any()
    env.close()
