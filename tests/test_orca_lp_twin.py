"""CPU: the fp32 twin of the ORCA linear programs (orca_lp_twin.py) against the oracle, and what the LP pools of lp_worlds.py reach.

(1) The twin's result equals the oracle's new_vel bit for bit on every RVO solve of random pools, of every LP pool and of every
    hand-made scene: the branch counters and margins it reports describe the oracle's own solve.
(2) Coverage: for every shape the kernel matrix runs (test_kernel_matrix.shape_for), without and with rectangles, the accepted
    pool reaches each rare branch at least MIN_REACHED times, the line beyond the lanes of an 8-lane group for M = 10, second-slot
    lines (i >= 17) for M = 20 and 32, and linearProgram3 at all for the generic kernels' M = 7 and 13.  The test prints the
    counts (pytest -s); DESIGN.md section 2 quotes them.
(3) The tie rejection of lp_worlds.build_pool replaces at most a quarter of its candidates.
(4) lp3_inner_failed - the inner program of linearProgram3 fails and the result is restored - "should in principle not happen"
    (RVO2).  It does: a seeded search over 20 000 boxed-in solves (egos of pref_speed 0.125 .. 0.5, coop 1, 3 to 6 neighbours at
    1.005 .. 1.14 m on a 1/1024 m grid, half of them beside walls inside the inflated band) found 6, all of one kind: two nearly
    anti-parallel half-planes of deeply overlapping neighbours meet far outside a small speed disc, the projected line misses
    the disc, the inner program fails on it.  (Where such a far line does cut the disc by rounding - disc = dot * dot + r * r -
    |p|^2 cancels catastrophically - the chord's ends lie outside the disc: RVO2's own fp32 behaviour, which the device has to
    repeat operation for operation.)  Three of the six are the scenes trap_a .. trap_c of lp_worlds.SCENES and fall under the
    coverage rule; no comparison of their solves is near its threshold."""
import importlib

import numpy as np
import pytest

import lp_worlds as lw
import orca_lp_twin as twin
from test_kernel_matrix import _cases, _n_worlds

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")

MIN_REACHED = 3
SHAPES = sorted({(M, _n_worlds(M, wp)) for _, _, wp, M, _ in _cases()})  # the two M = 10 rows share one pool
BRANCHES = ["lp1_parallel_inside", "lp1_parallel_outside", "lp1_disc_negative_original", "lp3_parallel_opposite",
            "lp3_parallel_same", "neighbour_distance_ties", "lp3_outer_2inner", "lp3_inner_failed"]
POOLS = [pytest.param(M, N, rects, id="M%d-%s" % (M, "obst" if rects else "free")) for M, N in SHAPES for rects in (False, True)]


def required(M, rects):
    """{counter: smallest count} the accepted pool of a shape must reach"""
    need = {k: MIN_REACHED for k in BRANCHES}
    if rects:
        need["lp3_with_obstacle_lines"] = MIN_REACHED
    if M == 10:  # the ninth line of M = 10: one beyond the lanes of a GW = 8 group, its chord computed on the fly
        need["lp2_line:8"] = need["lp3_outer_line:8"] = 1
    if M in (7, 13):
        need["lp3_solves"] = 1
    return need


def test_shapes_are_those_of_the_kernel_matrix():
    assert [M for M, _ in SHAPES] == [4, 7, 10, 13, 20, 32]


@pytest.mark.parametrize("M", [4, 7, 10, 13, 20, 32])
def test_twin_equals_oracle_on_random_pools(M):
    """all-RVO random crowds, in a square small enough for linearProgram3 to run"""
    N, T = (6, 20) if M <= 13 else (3, 12)
    a6 = scen.random_worlds_fast(N, M, seed=300 + M, side=3.0 if M <= 10 else 4.0 if M <= 20 else 5.5)
    pool = dict(agents6=a6, policy_id=np.full((N, M), scen.POLICY_RVO, dtype=np.int32), dynamics_id=scen.DYN_UNICYCLE,
                n_agents=np.full(N, M, dtype=np.int32), coop=np.full((N, M), 0.5), obstacles=None, n_obst=None)
    tr = lw.trace(pool, M, False, T)
    solves, bad, c = sum(t[2] for t in tr), sum(t[3] for t in tr), lw._total(tr)
    print("random M=%d: %d solves, %d in linearProgram3" % (M, solves, c.get("lp3_solves", 0)))
    assert solves == N * T * M and bad == 0
    assert c.get("lp3_solves", 0) > 0 or M < 10


@pytest.mark.parametrize("M,N,rects", POOLS)
def test_lp_pool_twin_coverage_and_rejection_rate(M, N, rects):
    pool, info = lw.build_pool(M, N, rects)
    c = info["counters"]
    need = required(M, rects)
    print("M=%d N=%d %s: %d solves, %d candidates, %d rejected (%.0f %%), scene steps %s" % (
        M, N, "obst" if rects else "free", info["solves"], info["candidates"], info["rejected"], 100 * info["rate"],
        info["scene_steps"]))
    print("   ", {k: c.get(k, 0) for k in list(need) + ["lp3_solves", "lp3_inner_failed", "lp1_disc_negative_projected",
                                                        "max_lp2_line", "max_lp3_outer_line", "max_lp3_inner_line"]})
    assert len(pool["agents6"]) == N and info["n_scenes"] == len(lw.scene_names(M, rects))
    assert info["mismatches"] == 0 and info["solves"] > 0  # (1)
    assert min(t[0] for t in info["traces"]) >= twin.TIE_MARGIN  # every world of the pool passed the tie rejection
    for k, n in need.items():  # (2)
        assert c.get(k, 0) >= n, (k, c.get(k, 0), n)
    if M in (20, 32):  # lanes project their second-slot lines
        assert c["max_lp3_outer_line"] >= 17, c["max_lp3_outer_line"]
    assert info["rate"] <= lw.MAX_REJECTED, (info["rejected"], info["candidates"])  # (3)


@pytest.mark.parametrize("M,maxnb", [(10, 3), (20, 10)])
def test_max_neighbours_pools_cut_off_at_tied_distances(M, maxnb):
    """the pools of the rvo_max_neighbors device test: exactly tied distances AT the cut decide which neighbours are kept"""
    pool, info = lw.build_pool(M, _n_worlds(M, 0 if M != 20 else 2), False, maxnb, scenes=False)
    print("M=%d max_neighbors=%d: %d solves, %d candidates, %d rejected" % (M, maxnb, info["solves"], info["candidates"],
                                                                          info["rejected"]))
    assert info["mismatches"] == 0 and info["rate"] <= lw.MAX_REJECTED
    at_cut = 0
    for w in range(len(pool["agents6"])):  # reset state: positions are the scenario's
        for ego in np.nonzero(pool["policy_id"][w] == scen.POLICY_RVO)[0]:
            _, dsq, cut = twin.kept_neighbours(pool["agents6"][w, :, 0:2], int(ego), maxnb)
            at_cut += int(cut is not None and cut == dsq[-1])
    assert at_cut >= MIN_REACHED and info["counters"]["neighbour_distance_ties"] >= MIN_REACHED


@pytest.mark.parametrize("name", sorted(lw.SCENES))
def test_scenes_reach_their_branches(name):
    """every hand-made scene, unperturbed and at the perturbation step the pools use: twin == oracle, and the accepted one
    reaches the branches it is there for"""
    rects = bool(lw.SCENES[name][5])
    M = max(6, len(lw.SCENES[name][0]))
    info = dict(candidates=0, rejected=0, scene_steps={})
    _, tr = lw._accepted_scene(name, M, rects, 0, lw.T_STEPS, info)
    raw = lw.trace(lw.as_pool([lw.scene_world(name, M, 0)], rects), M, rects)[0]
    print(name, "perturbation step", info["scene_steps"][name], {k: v for k, v in tr[1].items() if v > 0 and ":" not in k})
    assert tr[3] == 0 and raw[3] == 0 and tr[2] == lw.T_STEPS
    for k in lw.SCENES[name][6]:
        assert tr[1].get(k, 0) > 0, k


def test_file_scenes_are_what_reaches_the_same_direction_hole():
    """without the two file scenes the M = 4 pool would not reach lp3_parallel_same: the coverage rule notices a missing scene"""
    _, info = lw.build_pool(4, _n_worlds(4, 0), False)
    names = lw.scene_names(4, False)
    others = [t for k, t in zip(names, info["traces"]) if not k.startswith("file")] + info["traces"][len(names):-1]
    assert not names[(4 + 0) % len(names)].startswith("file")  # the last world repeats another scene
    assert lw._total(others).get("lp3_parallel_same", 0) < MIN_REACHED <= info["counters"]["lp3_parallel_same"]


def test_margin_counts_decisions_only():
    """two lines through the preferred velocity's neighbourhood: a line violated by 1e-5 is no decision (either way the result
    moves by 1e-5), the end of a line parallel to the objective is"""
    r, c, m = twin.classify(np.array([[0.0, 0.5 - 1e-5, 1.0, 0.0]], dtype=np.float32), 0, 1.0, (0.0, 0.5))
    assert c.raw_margin < twin.TIE_MARGIN <= m and c["lp2_rounds"] == 0
    lines = np.array([[0.0, -0.2, -1.0, 0.0], [0.0, 0.2, 1.0, 0.0], [0.5, 0.0, 0.0, 1.0]], dtype=np.float32)  # v.y <= -0.2, >= 0.2
    r, c, m = twin.classify(lines, 0, 1.0, (0.3, 0.0))
    assert c["lp3_solves"] == 1 and c["lp3_parallel_opposite"] == 1
    # the third line (v.x <= 0.5) is satisfied; had it come into linearProgram3, its projected lines would meet the objective
    # at a real angle: the margin of this solve is set by decisions far from their thresholds
    assert m >= twin.TIE_MARGIN
    wall = np.array([[0.0, 0.0, 0.0, 1.0], [0.05, 0.0, 0.0, -1.0]], dtype=np.float32)  # v.x <= 0 protected, v.x >= 0.05
    r, c, m = twin.classify(wall, 1, 0.25, (0.25, 0.0))
    assert c["lp3_with_obstacle_lines"] == 1 and m == 0.0 and c.what == "dot > 0 (dir_opt)"
