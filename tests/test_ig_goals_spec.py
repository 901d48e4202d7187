"""CPU: ig.geodesic_spec and ig.goal_action_spec, the numpy statements that tests/test_ig_goals.py holds cagym_ig_geodesic and
cagym_ig_goal_actions to, the layout of their parameter block and their prototype rows.  The Dijkstra of geodesic_spec is compared,
bit for bit, with a plain Jacobi iteration of the same fp32 relaxation run to its fixed point - the order of relaxation does not
matter - on hand-made masks and on stage-2 worlds from the exploration twin."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np

import exploration_twin as xt
from oracle import oracle as orc
from test_abi import ROOT, _c_compiler

igm = importlib.import_module("gym-exploration-2d_amd.ig")
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
INF = np.float32(np.inf)
ORTHO, DIAG = np.float32(0.5), np.float32(0.5 * np.sqrt(2.0))
CTL = dict(dt=0.1, v_max=2.0, w_max=np.pi, align_tol=np.pi / 4, goal_tol=0.25)


def _edf_of(free):
    """a [300, 300] distance field whose every raster cell of a free belief cell passes EDF > 0.6 and of a blocked one fails"""
    return np.kron(np.where(free, 5.0, 0.0), np.ones((5, 5)))


def _centre(i, j):
    return (i * 0.5 - 15.0 + 0.25, j * 0.5 - 15.0 + 0.25)


def _jacobi(free, si, sj):
    """Jacobi sweeps of field[v] = min over allowed u of fl32(field[u] + cost) from field[source] = 0, to the fixed point.  Returns
    (field, sweeps)."""
    free = free.copy()
    free[sj, si] = True
    f = np.full((60, 60), INF, dtype=np.float32)
    f[sj, si] = 0.0
    FP = np.pad(free, 1, constant_values=False)
    for sweep in range(1, 3601):
        P = np.pad(f, 1, constant_values=INF)
        new = f.copy()
        for k, (di, dj) in enumerate(igm.GEO_NEIGHBOURS):
            cand = P[1 + dj:61 + dj, 1 + di:61 + di] + (ORTHO if k < 4 else DIAG)
            assert cand.dtype == np.float32
            if k >= 4:
                cand = np.where(FP[1:61, 1 + di:61 + di] & FP[1 + dj:61 + dj, 1:61], cand, INF)
            new = np.minimum(new, cand)
        new = np.where(free, new, INF)
        new[sj, si] = 0.0
        if np.array_equal(new, f):
            return f, sweep
        f = new
    raise AssertionError("no fixed point within 3600 sweeps")


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _wall_with_a_gap():
    free = np.ones((60, 60), dtype=bool)
    free[:, 30] = False   # a wall along y at column 30 ...
    free[50, 30] = True   # ... with one gap near the top
    return free


def test_dijkstra_equals_jacobi_on_hand_made_masks():
    rng = np.random.default_rng(3)
    masks = [np.ones((60, 60), dtype=bool), _wall_with_a_gap(), rng.random((60, 60)) > 0.3, rng.random((60, 60)) > 0.45]
    for n, free in enumerate(masks):
        for (si, sj) in ((10, 10), (0, 0), (59, 31), (45, 50)):
            field, fr, src = igm.geodesic_spec(_edf_of(free), _centre(si, sj), 0.5)
            want, sweeps = _jacobi(free, si, sj)
            assert src == (si, sj) and fr[sj, si] and _same(field, want), (n, si, sj)
            assert field[sj, si] == 0 and (field[~fr] == INF).all()
    assert sweeps > 1


def test_dijkstra_equals_jacobi_on_stage_2_worlds():
    """8 twin-generated stage-2 worlds, the two robots' start points as sources: equal bit for bit, the sweep counts printed."""
    S, M, K, R, T = 8, 5, 16, 2, 3
    pool = xt.generate(S, M, K, scen.GEN_STAGE_2, 0, R, T, n_obst=(6, 16), target_radius=0.2, robot_pref_speed=0.2)
    assert pool["n_failed"] == 0
    counts, reach, blocked_sources = [], [], 0
    for s in range(S):
        edf = orc.edt(orc.rasterize(pool["obstacles"][s, :int(pool["n_obst"][s])]))[0]
        for r in range(R):
            p = pool["agents6"][s, r, :2]
            field, free, src = igm.geodesic_spec(edf, p, 0.5)
            si, sj = src
            assert (si, sj) == (math.floor((p[0] + 15) / 0.5), math.floor((p[1] + 15) / 0.5))
            raw = edf[2::5, 2::5] > 0.5 + 0.1
            blocked_sources += int(not raw[sj, si])
            want, sweeps = _jacobi(raw, si, sj)
            assert _same(field, want), (s, r)
            assert np.array_equal(free, raw | ((np.arange(60)[None, :] == si) & (np.arange(60)[:, None] == sj)))
            assert (field[~free] == INF).all()
            counts.append(sweeps)
            reach.append(int(np.isfinite(field).sum()))
    print("jacobi sweeps %d..%d, %d sources in cells that fail the clearance test" % (min(counts), max(counts), blocked_sources))
    assert max(reach) > 1000 and sorted(reach)[len(reach) // 2] > 500  # (a start walled in by the clearance band reaches little)
    assert blocked_sources > 0  # (the rule 'the source cell always counts as free' is exercised)


def test_a_wall_with_one_gap_makes_the_way_longer_than_the_line():
    free = _wall_with_a_gap()
    field, _, _ = igm.geodesic_spec(_edf_of(free), _centre(25, 10), 0.5)
    line = math.hypot(35 - 25, 0) * 0.5
    assert np.isfinite(field[10, 35]) and field[10, 35] > line + 15.0  # up to row 50 and down again
    assert field[10, 20] == np.float32(2.5)                            # the same side: five orthogonal moves
    assert (field[:, 30][np.arange(60) != 50] == INF).all() and np.isfinite(field[50, 30])
    # through the gap every move is orthogonal: both diagonals into and out of it pass a wall cell
    assert field[50, 31] == np.float32(field[50, 30] + ORTHO) and field[50, 30] == np.float32(field[50, 29] + ORTHO)


def test_a_diagonal_squeezed_between_two_blocked_cells_is_not_taken():
    free = np.ones((60, 60), dtype=bool)
    free[21, 20] = free[20, 21] = False  # N and E of (20, 20): the NE diagonal passes between them
    field, _, _ = igm.geodesic_spec(_edf_of(free), _centre(20, 20), 0.5)
    assert field[21, 21] > DIAG and np.isfinite(field[21, 21])
    assert field[19, 19] == DIAG and field[19, 21] > DIAG and field[21, 19] > DIAG  # SW is open; SE and NW touch one blocked cell
    one = np.ones((60, 60), dtype=bool)
    one[21, 20] = False  # one blocked orthogonal cell is enough
    assert igm.geodesic_spec(_edf_of(one), _centre(20, 20), 0.5)[0][21, 21] > DIAG


def test_an_enclosed_source_reaches_nothing_and_a_blocked_source_is_free():
    free = np.ones((60, 60), dtype=bool)
    free[9:12, 9:12] = False
    free[10, 10] = True
    field, fr, src = igm.geodesic_spec(_edf_of(free), _centre(10, 10), 0.5)
    assert src == (10, 10) and np.isfinite(field).sum() == 1 and field[10, 10] == 0
    # a source in a blocked cell counts as free: the field leaves it through its free neighbours
    free = np.ones((60, 60), dtype=bool)
    free[10, 10] = free[10, 11] = False
    field, fr, src = igm.geodesic_spec(_edf_of(free), _centre(10, 10), 0.5)
    assert fr[10, 10] and not fr[10, 11] and field[10, 10] == 0 and field[10, 9] == ORTHO and field[10, 11] == INF
    assert field[11, 11] > DIAG  # (the diagonal past the blocked (11, 10) is closed)
    # no source cell: outside the map, NaN, infinite
    for p in ((15.0, 0.0), (-15.01, 0.0), (0.0, 40.0), (np.nan, 0.0), (0.0, np.inf)):
        field, fr, src = igm.geodesic_spec(_edf_of(free), p, 0.5)
        assert src is None and (field == INF).all() and field.dtype == np.float32, p
    assert igm.geodesic_spec(_edf_of(free), (14.999, -15.0), 0.5)[2] == (59, 0)


# ---- the controller ------------------------------------------------------------------------------------------------------------------
def _open_field(goal=(20, 20)):
    return igm.geodesic_spec(_edf_of(np.ones((60, 60), dtype=bool)), _centre(*goal), 0.5)[0]


def test_ties_go_to_the_first_candidate_in_order():
    field = np.full((60, 60), INF, dtype=np.float32)
    x, y = _centre(30, 30)
    field[30, 31] = field[31, 30] = field[30, 29] = field[29, 30] = 1.0  # E, N, W, S all equal: E
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(5, 5), **CTL)[2] == (31, 30)
    field[30, 31] = 1.5
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(5, 5), **CTL)[2] == (30, 31)  # N
    field[31, 30] = 1.5
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(5, 5), **CTL)[2] == (29, 30)  # W
    # an orthogonal candidate wins a tie of KEYS against a diagonal one: key(E) = 1.5 + 0.5 = key(SW) when ...
    field[:] = INF
    field[30, 31] = 1.5
    field[29, 29] = np.float32(2.0) - DIAG
    assert np.float32(field[29, 29] + DIAG) == np.float32(2.0)
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(5, 5), **CTL)[2] == (31, 30)
    field[29, 29] = np.float32(1.0)  # ... and a smaller key wins wherever it stands in the order
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(5, 5), **CTL)[2] == (29, 29)


def test_an_infinite_own_cell_drops_the_diagonal_rule():
    field = np.full((60, 60), INF, dtype=np.float32)
    x, y = _centre(30, 30)
    field[31, 31] = 1.0  # NE finite, its two orthogonal cells infinite
    v, om, cell, reached = igm.goal_action_spec(field, (x, y, 0.0), _centre(40, 40), **CTL)
    assert cell == (31, 31) and not reached  # the robot stands inside the clearance band: any finite neighbour will do
    field[30, 30] = 2.0   # with a finite own value the squeezed diagonal is closed: no candidate, no motion
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(40, 40), **CTL) == (0.0, 0.0, None, False)
    field[30, 31] = field[31, 30] = 1.6  # both orthogonal cells finite: open again, and the smaller key
    assert igm.goal_action_spec(field, (x, y, 0.0), _centre(40, 40), **CTL)[2] == (31, 31)


def test_in_the_goal_cell_the_aim_is_the_goal_point_and_the_speed_is_capped():
    field = _open_field()
    cx, cy = _centre(20, 20)
    goal = (cx + 0.2, cy + 0.1)
    pose = (cx - 0.2, cy - 0.2, math.atan2(0.3, 0.4))  # heading straight at the goal, 0.5 m away
    v, om, cell, reached = igm.goal_action_spec(field, pose, goal, **CTL)
    assert cell == (20, 20) and not reached and abs(om) < 1e-12 and v == 2.0  # min(2.0, 0.5 / 0.1)
    v, om, cell, reached = igm.goal_action_spec(field, pose, goal, **dict(CTL, goal_tol=0.05, v_max=8.0))
    dx, dy = goal[0] - pose[0], goal[1] - pose[1]
    assert v == math.sqrt(dx * dx + dy * dy) / 0.1 and 4.9 < v < 5.1  # one step lands on the point
    # reached: within goal_tol, nothing moves; the bound is inclusive
    assert igm.goal_action_spec(field, (goal[0] - 0.25, goal[1], 1.0), goal, **CTL) == (0.0, 0.0, None, True)
    assert igm.goal_action_spec(field, (goal[0] - 0.2500001, goal[1], 1.0), goal, **CTL)[3] is False
    # reached counts even in a neighbouring cell
    assert igm.goal_action_spec(field, (cx - 0.3, cy, 0.0), (cx - 0.2, cy, 0.0), **CTL)[3] is True


def test_outside_the_map_and_without_a_candidate_nothing_moves():
    field = _open_field()
    assert igm.goal_action_spec(field, (15.2, 0.0, 0.0), _centre(20, 20), **CTL) == (0.0, 0.0, None, False)
    assert igm.goal_action_spec(field, (0.0, -15.5, 0.0), _centre(20, 20), **CTL) == (0.0, 0.0, None, False)
    none = np.full((60, 60), INF, dtype=np.float32)
    assert igm.goal_action_spec(none, (0.1, 0.1, 0.0), _centre(20, 20), **CTL) == (0.0, 0.0, None, False)
    # at the map's edge the candidates outside it do not exist
    edge = np.full((60, 60), INF, dtype=np.float32)
    edge[0, 1] = 1.0
    assert igm.goal_action_spec(edge, (*_centre(0, 0), 0.0), _centre(20, 20), **CTL)[2] == (1, 0)


def test_the_turn_is_clamped_and_the_speed_waits_for_alignment():
    field = _open_field((40, 30))  # the goal due east of the robot: it aims at the E neighbour's centre, err = -heading
    x, y = _centre(30, 30)
    for th, om_want, v_want in ((0.0, 0.0, 2.0), (0.2, -2.0, 2.0), (-0.3, 3.0, 2.0),       # err / dt within the clamp: aligned in one step
                                (1.0, -np.pi, 2.0),                                       # clamped; rem = -1 + pi / 10 = -0.686 > -pi / 4
                                (1.2, -np.pi, 0.0), (-1.2, np.pi, 0.0), (3.0, -np.pi, 0.0)):  # |rem| > pi / 4: turn on the spot
        v, om, cell, reached = igm.goal_action_spec(field, (x, y, th), _centre(40, 30), **CTL)
        assert cell == (31, 30) and v == v_want and abs(om - om_want) < 1e-12, th
    # the gate sits at |rem| == align_tol, inclusive
    th = np.pi / 4 + np.pi * 0.1
    assert igm.goal_action_spec(field, (x, y, th * (1 - 1e-9)), _centre(40, 30), **CTL)[0] == 2.0
    assert igm.goal_action_spec(field, (x, y, th * (1 + 1e-9)), _centre(40, 30), **CTL)[0] == 0.0
    # wrap: a heading just past -pi turns through pi, not round the long way
    west = _open_field((20, 30))
    v, om, cell, _ = igm.goal_action_spec(west, (x, y, -3.1), _centre(20, 30), **dict(CTL, w_max=100.0))
    assert cell == (29, 30) and abs(om * 0.1 + (np.pi - 3.1)) < 1e-12 and v == 2.0  # atan2 = pi, err = 2 pi - 3.1 - pi wrapped


def test_atan2_spec_is_within_an_ulp_of_the_c_library():
    """ig.atan2_spec restates fdlibm's atan2 in plain fp64 operations: 0 or 1 ulp from math.atan2 over all four quadrants and
    twelve decades of |y / x|, and equal to it on the axes, signed zeros included."""
    rng = np.random.default_rng(0)
    bits = lambda v: np.array([v], dtype=np.float64).view(np.int64)[0]
    worst = 0
    for scale in (1.0, 1e-3, 1e3, 1e-9, 1e9, 30.0):
        for _ in range(4000):
            y, x = rng.normal() * scale, rng.normal()
            worst = max(worst, abs(int(bits(igm.atan2_spec(y, x))) - int(bits(math.atan2(y, x)))))
    print("worst difference %d ulp" % worst)
    assert worst <= 1
    for y, x in ((0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (1e-300, 1.0), (1.0, 1e-300),
                 (1.0, -1e300), (-1e-20, -1.0), (0.25, 0.25), (-0.25, 0.25), (0.0, -0.5), (3.0, -0.0)):
        assert bits(igm.atan2_spec(y, x)) == bits(math.atan2(y, x)), (y, x)


def test_parameter_block_mirror_matches_the_header(tmp_path):
    S = _lib.IgGoalParams
    fields = [f[0] for f in S._fields_]
    assert fields == ["n_robots", "window", "rotate", "flags", "radius", "v_max", "w_max", "align_tol", "goal_tol", "dt"]
    lines = ['printf("size %d\\n", (int)sizeof(struct cagym_ig_goal_params));']
    lines += ['printf("%s %%d\\n", (int)offsetof(struct cagym_ig_goal_params, %s));' % (f, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cagym_ig_goals.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([_c_compiler(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert ctypes.sizeof(S) == int(got["size"]) == 64
    for f in fields:
        assert getattr(S, f).offset == int(got[f]), f


def test_prototype_rows():
    rows = {"cagym_ig_geodesic": 10, "cagym_ig_goal_actions": 8, "cagym_ig_goal_status": 9}
    for name, n in rows.items():
        row = _lib._ARGTYPES[name]
        assert len(row) == n and row[1] is ctypes.POINTER(_lib.IgGoalParams), name
    header = open(os.path.join(ROOT, "include", "cagym.h")).read()
    assert "typedef struct cagym_ig_goal_params cagym_ig_goal_params;" in header
    assert "struct cagym_ig_goal_params {" not in header  # (defined in a header of its own)
    assert float(igm.GEO_DIAG) == float(np.float32(0.5 * math.sqrt(2.0))) and igm.GEO_ORTHO == 0.5
