"""CPU: ig.assign_goals_spec, the numpy statement that tests/test_ig_assign.py holds cagym_ig_assign_goals to - the sequential-greedy
allocation of coverage over the robots' candidate goals - on stage-2 worlds from the exploration twin with the oracle's distance
field: cell sets from ig.view_gain_spec (a robot turning on the spot) and oracle.visible_cells (a cone), priced by oracle.mi_reward
on a non-uniform belief.  Also the parameter block's layout and the prototype row."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import exploration_twin as xt
from oracle import oracle as orc

igm = importlib.import_module("gym-exploration-2d_amd.ig")
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
S, M, K, R, T = 4, 6, 16, 3, 3
KC = 4  # candidates per robot
RANGE, RADIUS, D0 = 5.0, 0.5, 1.0
CENTRES = np.arange(60) * 0.5 - 15.0 + 0.25


def _reward(belief):
    return lambda cells: orc.mi_reward(belief, igm.cells_to_words(cells))


@pytest.fixture(scope="module")
def worlds():
    """Per world: cell sets [R, KC, 60, 60] of candidates that all lie round robot 0's start, so that the robots compete (even
    candidates turning on the spot, odd ones a cone looking past that start), valid [R, KC], distance [R, KC] f32 from each robot's
    own start, a belief, and a seed set: what a robot standing at robot 0's start sees."""
    pool = xt.generate(S, M, K, scen.GEN_STAGE_2, 0, R, T, n_obst=(6, 16), target_radius=0.2, robot_pref_speed=0.2)
    assert pool["n_failed"] == 0
    rng = np.random.default_rng(3)
    out = []
    for s in range(S):
        edf = orc.edt(orc.rasterize(pool["obstacles"][s, :int(pool["n_obst"][s])]))[0]
        belief = rng.uniform(0.3, 3.0, (60, 60))
        mi = igm.cell_mi(belief)
        free = np.argwhere(igm.edf_at_spec(edf, CENTRES[None, :].repeat(60, 0), CENTRES[:, None].repeat(60, 1)) > RADIUS + 0.1)
        masks = np.zeros((R, KC, 60, 60), dtype=bool)
        valid = np.zeros((R, KC), dtype=bool)
        dist = np.zeros((R, KC), dtype=np.float32)
        for r in range(R):
            here = pool["agents6"][s, r, :2]
            hub = pool["agents6"][s, 0, :2]  # every robot's candidates lie round robot 0's start: the teams' cell sets overlap
            near = free[np.argsort(np.hypot(CENTRES[free[:, 1]] - hub[0], CENTRES[free[:, 0]] - hub[1]), kind="stable")]
            for c in range(KC):
                j, i = near[2 + 9 * c + 3 * r]  # free cell centres a little apart, nearest first
                p = (CENTRES[i], CENTRES[j])
                if c % 2 == 0:
                    _, _, valid[r, c], masks[r, c], _ = igm.view_gain_spec(edf, mi, p, RADIUS, RANGE)
                else:
                    th = math.atan2(hub[1] - p[1], hub[0] - p[0]) + 0.3
                    masks[r, c] = igm.words_to_cells(orc.visible_cells(edf, np.array([p[0], p[1], th]), rng=RANGE))
                    valid[r, c] = True
                dist[r, c] = np.float32(math.hypot(p[0] - here[0], p[1] - here[1]))
        seed = igm.view_gain_spec(edf, mi, pool["agents6"][s, 0, :2], RADIUS, RANGE)[3]
        out.append(dict(masks=masks, valid=valid, dist=dist, belief=belief, seed=seed))
    return out


def test_words_and_cells_round_trip():
    rng = np.random.default_rng(0)
    cells = rng.random((3, 60, 60)) < 0.3
    words = igm.cells_to_words(cells)
    assert words.dtype == np.uint64 and words.shape == (3, 60)
    assert bool((words[1, 7] >> np.uint64(59)) & np.uint64(1)) == bool(cells[1, 7, 59]) and int(words.max()) < 1 << 60
    assert np.array_equal(igm.words_to_cells(words), cells) and np.array_equal(igm.words_to_cells(words.view(np.int64)), cells)


def test_the_worlds_have_overlapping_candidates(worlds):
    """what the seed was chosen for: candidates that see something, robots whose candidates overlap a teammate's, a seed that matters"""
    pops = np.array([w["masks"].sum(axis=(2, 3)) for w in worlds])
    print("cells per candidate: min %d, median %d, max %d" % (pops.min(), np.median(pops), pops.max()))
    assert all(w["valid"].all() for w in worlds) and (pops > 10).all()
    assert all((w["masks"][0].any(0) & w["masks"][1].any(0)).any() and (w["masks"][1].any(0) & w["masks"][2].any(0)).any() for w in worlds)
    assert all((w["masks"][0].any(0) & w["seed"]).any() for w in worlds)


def test_one_open_robot_takes_the_arg_max_with_the_tie_rule(worlds):  # (a)
    for w in worlds:
        rew = _reward(w["belief"])
        for mode in ("slot", "best"):
            for r in range(R):
                got = igm.assign_goals_spec(w["masks"], np.zeros((60, 60), bool), w["dist"], w["valid"], rew, mode, D0, [r])
                u = [rew(w["masks"][r, c]) / (float(w["dist"][r, c]) + D0) for c in range(KC)]
                assert got["choice"][r] == int(np.argmax(u)) and got["utility"][r] == max(u) and got["order"][r] == 0
                assert got["marginal"][r] == rew(w["masks"][r, got["choice"][r]])
                assert (np.delete(got["choice"], r) == -1).all() and np.isnan(got["round_gain"][1:]).all()
                assert np.array_equal(got["claimed"], w["masks"][r, got["choice"][r]])
    # equal utilities: the smaller index
    w = worlds[0]
    masks, dist = w["masks"].copy(), w["dist"].copy()
    best = int(igm.assign_goals_spec(masks, np.zeros((60, 60), bool), dist, w["valid"], _reward(w["belief"]), "best", D0, [1])["choice"][1])
    other = (best + 2) % KC
    masks[1, other], dist[1, other] = masks[1, best], dist[1, best]
    got = igm.assign_goals_spec(masks, np.zeros((60, 60), bool), dist, w["valid"], _reward(w["belief"]), "best", D0, [1])
    assert got["choice"][1] == min(best, other)


@pytest.mark.parametrize("mode", ["slot", "best"])
def test_what_each_robot_adds_is_disjoint_and_adds_up(worlds, mode):  # (b)
    for w in worlds:
        got = igm.assign_goals_spec(w["masks"], w["seed"], w["dist"], w["valid"], _reward(w["belief"]), mode, D0, [0, 1, 2])
        assert (got["choice"] >= 0).all() and sorted(got["order"]) == [0, 1, 2]
        claimed, added = w["seed"].copy(), []
        for r in np.argsort(got["order"]):
            new = w["masks"][r, got["choice"][r]] & ~claimed
            assert not (new & w["seed"]).any() and all(not (new & a).any() for a in added)
            assert got["marginal"][r] == _reward(w["belief"])(new) and got["marginal"][r] > 0
            added.append(new)
            claimed |= w["masks"][r, got["choice"][r]]
        assert np.array_equal(claimed, got["claimed"])
        assert int(got["claimed"].sum()) == int(w["seed"].sum()) + sum(int(a.sum()) for a in added)


@pytest.mark.parametrize("mode", ["slot", "best"])
def test_two_robots_with_the_same_single_candidate(worlds, mode):  # (c)
    w = worlds[1]
    masks = np.stack([w["masks"][0, :1], w["masks"][0, :1]])
    dist = np.array([[1.0], [3.0]], dtype=np.float32)
    got = igm.assign_goals_spec(masks, np.zeros((60, 60), bool), dist, np.ones((2, 1), bool), _reward(w["belief"]), mode, D0, [0, 1])
    assert got["choice"].tolist() == [0, -1] and got["order"].tolist() == [0, -1] and got["marginal"][1] == 0 and got["utility"][1] == 0
    assert got["round_gain"][1, 1, 0] == 0.0 and np.array_equal(got["claimed"], masks[0, 0])  # (priced at nothing, hence not eligible)


def test_best_first_does_not_depend_on_the_slots_and_slot_order_does(worlds):  # (d)
    perm = [2, 0, 1]  # new slot n holds old robot perm[n]
    for w in worlds:
        rew = _reward(w["belief"])
        a = igm.assign_goals_spec(w["masks"], w["seed"], w["dist"], w["valid"], rew, "best", D0, [0, 1, 2])
        for t in range(R):  # every utility of every round is distinct: no tie for the slots to break
            g = a["round_gain"][t]
            u = (g / (w["dist"].astype(np.float64) + D0))[np.isfinite(g) & (g > 0)]
            assert len(np.unique(u)) == len(u)
        b = igm.assign_goals_spec(w["masks"][perm], w["seed"], w["dist"][perm], w["valid"][perm], rew, "best", D0, [0, 1, 2])
        for n in ("choice", "order", "marginal", "utility"):
            assert np.array_equal(b[n], a[n][perm]), n
        assert np.array_equal(a["claimed"], b["claimed"]) and np.array_equal(b["round_gain"], a["round_gain"][:, perm], equal_nan=True)
    # an input on which the two modes differ, and slot order depends on the slots: robot 1's wide candidate covers robot 0's
    blk = lambda j0, j1: np.pad(np.ones((j1 - j0, 60), bool), ((j0, 60 - j1), (0, 0)))
    masks = np.zeros((2, 2, 60, 60), dtype=bool)
    masks[0, 0], masks[0, 1] = blk(0, 10), blk(30, 38)
    masks[1, 0], masks[1, 1] = blk(0, 20), blk(50, 55)
    args = (np.zeros((60, 60), bool), np.zeros((2, 2), np.float32), np.ones((2, 2), bool), _reward(np.ones((60, 60))))
    slot = igm.assign_goals_spec(masks, *args, "slot", D0, [0, 1])
    best = igm.assign_goals_spec(masks, *args, "best", D0, [0, 1])
    assert slot["choice"].tolist() == [0, 0] and slot["order"].tolist() == [0, 1] and slot["marginal"][1] == _reward(np.ones((60, 60)))(blk(10, 20))
    assert best["choice"].tolist() == [1, 0] and best["order"].tolist() == [1, 0]
    swapped = igm.assign_goals_spec(masks[::-1], *args, "slot", D0, [0, 1])
    assert swapped["choice"].tolist() == [0, 1]  # robot 1 first takes the wide one: robot 0 is left its second candidate
    assert int(best["claimed"].sum()) > int(slot["claimed"].sum())


@pytest.mark.parametrize("mode", ["slot", "best"])
def test_what_makes_a_candidate_ineligible(worlds, mode):  # (e)
    w = worlds[2]
    rew = _reward(w["belief"])
    masks, seed = w["masks"][:1, :2].copy(), np.zeros((60, 60), bool)
    small = np.zeros((60, 60), bool)
    small[5, 5] = True
    masks[0, 1] = small  # candidate 0 is worth far more than candidate 1, unless it is ineligible
    ok, dist = np.ones((1, 2), bool), np.array([[2.0, 2.0]], dtype=np.float32)
    run = lambda **kw: igm.assign_goals_spec(kw.get("masks", masks), kw.get("seed", seed), kw.get("dist", dist), kw.get("ok", ok), rew, mode, D0, [0])
    assert run()["choice"][0] == 0
    cases = {"invalid": dict(ok=np.array([[False, True]])), "nan": dict(dist=np.array([[np.nan, 2.0]], dtype=np.float32)),
             "inf": dict(dist=np.array([[np.inf, 2.0]], dtype=np.float32)), "zero": dict(seed=masks[0, 0] & ~small)}
    for name, kw in cases.items():
        got = run(**kw)
        assert got["choice"][0] == 1 and got["marginal"][0] == rew(small), name
        assert np.isnan(got["round_gain"][0, 0, 0]) == (name != "zero") and (name != "zero" or got["round_gain"][0, 0, 0] == 0.0), name
        alone = run(masks=masks[:, :1], dist=kw.get("dist", dist)[:, :1], ok=kw.get("ok", ok)[:, :1], seed=kw.get("seed", seed))
        assert alone["choice"][0] == -1 and alone["order"][0] == -1 and alone["marginal"][0] == 0 and alone["utility"][0] == 0, name
        assert np.array_equal(alone["claimed"], kw.get("seed", seed)), name
    with pytest.raises(ValueError):
        igm.assign_goals_spec(masks, seed, dist, ok, rew, mode, D0, [1])


def test_marginal_gains_do_not_grow_from_round_to_round(worlds):  # (f)
    shrank = 0
    for w in worlds:
        got = igm.assign_goals_spec(w["masks"], w["seed"], w["dist"], w["valid"], _reward(w["belief"]), "best", D0, [0, 1, 2])
        g = got["round_gain"]
        both = np.isfinite(g[1:]) & np.isfinite(g[:-1])
        assert both.sum() >= KC * 3 and (g[1:][both] <= g[:-1][both]).all()
        shrank += int((g[1:][both] < g[:-1][both]).sum())
        assert np.isfinite(g[0]).all() and np.isnan(g[1, np.argmin(got["order"])]).all()  # round 0 prices everybody, its winner is closed
    assert shrank >= 1


def test_parameter_block_and_prototype_row():
    P = _lib.IgAssignParams
    assert [f[0] for f in P._fields_] == ["n_robots", "k", "mode", "flags", "radius", "range", "d0", "fov"]
    assert ctypes.sizeof(P) == 48 and P.radius.offset == 16 and P.fov.offset == 40
    assert _lib.IG_ASSIGN_MODES == {"slot": 0, "best": 1}
    row = _lib._ARGTYPES["cagym_ig_assign_goals"]
    assert len(row) == 17 and row[1] == ctypes.POINTER(P) and all(t is ctypes.c_void_p for t in row[2:])
    header = open(importlib.import_module("test_abi").ROOT + "/include/cagym_ig_assign.h").read()
    for name, _ in P._fields_:
        assert (" %s;" % name) in header, name
