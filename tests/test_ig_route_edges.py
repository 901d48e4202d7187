"""GPU: cagym_ig_route_gains (csrc/cagym_ig_route.h) on the hand-made fields of tests/test_ig_route_edges_spec.py - equal and rounded
keys, gated diagonals, moves that do not descend, NaN, -inf and values below zero, the map's corners and borders, corridors of
exact length at eight strides, all eight directions - and on the device's own geodesic fields of the hand-made worlds of
tests/geodesic_worlds.py, a serpentine's 1100 moves among them.  n_path, n_way, truncated, way_cells and way_dir are held to
ig.route_spec, the masks to cagym_ig_visible_cells and cagym_ig_assign_goals, the gains to cagym_ig_mi_reward, utility and best to
ig.route_gains_spec - all bit for bit, as tests/test_ig_route.py holds them on generated worlds.  What every field was built for is
asserted on the CPU, in the spec module.

The gadget fields are the same in all six worlds (the walks are, the cell sets are not): stage-2 worlds after ten learner steps."""
import importlib
import math

import numpy as np
import pytest

import geodesic_worlds as gw
import test_ig_route_edges_spec as S
from test_ig_assign import _np, _team, _words
from test_ig_goals_edges import MIRROR, POCKET, STAIRS, X_SERP, Y_SERP, _env, _points
from test_ig_route import OUT_KEYS, _centres, _sentinels, _untouched
from test_ig_viewpoints import N, RADIUS, _bits, _steps

pytestmark = pytest.mark.gpu
igm = importlib.import_module("gym-exploration-2d_amd.ig")
R, K = S.R, S.K
MASK = np.ones((N, R), dtype=np.uint8)
MASK[3], MASK[4] = (1, 0, 1, 0, 0, 1, 0, 1), 0  # world 3: five of the eight robots ask; world 4: nobody does


def hold_route(ig, field_dev, field, cells, hd, stride, mask=None, exclude=None, radius=RADIUS, d0=1.0, dev=None, same_worlds=False,
               rules=True):
    """One launch of route_gains into tensors of a known pattern, held to the specification as tests/test_ig_route.py holds it:
    the walks to route_spec, route_masks to the OR of visible_cells over the way-point poses, total_masks to that OR'd with
    assign_goals' set of the candidate, the gains to mi_reward and (rules) utility and best to route_gains_spec.  field: the
    read-back [n, R, 60, 60]; same_worlds: every world holds the same fields (the walks are specified once).  Returns the read-back
    outputs, rows outside the mask included as they were left."""
    n_worlds, n_robots, k = cells.shape[:3]
    mask = np.ones((n_worlds, n_robots), dtype=np.uint8) if mask is None else mask
    on = mask != 0
    asg = _np(ig.assign_goals(_centres(cells), np.ones((n_worlds, n_robots, k), dtype=np.float32), cand_heading=hd, mode="slot", radius=radius,
                              want_rounds=False))
    terminal = _words(asg["masks"])
    ex_words = np.zeros((n_worlds, 60), dtype=np.uint64) if exclude is None else _words(exclude)
    out = _sentinels(dev, n_robots, k)
    got = ig.route_gains(field_dev, cells, cand_heading=hd, mask=mask, exclude=exclude, stride=stride, radius=radius, d0=d0, out=out,
                         want_waypoints=True)
    assert got is out
    got = _np(out)
    for name in OUT_KEYS:  # rows of robots outside the mask, and the worlds nobody asks in, keep every byte
        assert _untouched(name, got[name][~on]).all(), name
    for name in ("n_path", "n_way", "truncated", "best", "route_gain", "total_gain", "utility", "way_dir"):
        assert not _untouched(name, got[name][on]).any(), name
    poses, owner, memo = [], [], {}
    for w, r in np.argwhere(on):
        for c in range(k):
            key = (r, c) if same_worlds else (w, r, c)
            if key not in memo:
                memo[key] = igm.route_spec(field[w, r], cells[w, r, c], min(stride, 3601))  # (a stride beyond the walk's cap: no way-point)
            n, wc, wd, trunc = memo[key]
            at = (w, r, c)
            assert got["n_path"][at] == n and got["n_way"][at] == len(wd) and got["truncated"][at] == int(trunc), (at, n, got["n_path"][at], got["n_way"][at])
            assert np.array_equal(got["way_cells"][at][:len(wd)], wc) and np.array_equal(got["way_dir"][at][:len(wd)], wd), at
            assert (got["way_cells"][at][len(wd):] == -1).all() and (got["way_dir"][at][len(wd):] == -1).all(), at
            for (i, j), d in zip(wc, wd):
                poses.append((i * 0.5 - 15.0 + 0.25, j * 0.5 - 15.0 + 0.25, igm.route_heading(d)))
                owner.append(at)
    want_route = np.zeros((n_worlds, n_robots, k, 60), dtype=np.uint64)
    if poses:
        vis = _words(ig.visible_cells(np.array(poses), np.array([o[0] for o in owner], dtype=np.int32)))
        for o, m in zip(owner, vis):
            want_route[o] |= m
    route = _words(np.where(on[..., None, None], got["route_masks"], 0))
    total = _words(np.where(on[..., None, None], got["total_masks"], 0))
    assert np.array_equal(route[on], want_route[on]), np.argwhere((route != want_route).any(-1) & on[..., None])[:5]
    has = (got["n_path"] >= 0) & on[..., None]
    want_total = np.where(has[..., None], want_route | terminal, np.uint64(0))
    assert np.array_equal(total[on], want_total[on]), np.argwhere((total != want_total).any(-1) & on[..., None])[:5]
    assert int(total.max()) < 1 << 60
    world = np.broadcast_to(np.arange(n_worlds, dtype=np.int32)[:, None, None], (n_worlds, n_robots, k))
    for name, sets in (("route_gain", route), ("total_gain", total)):
        priced = ig.mi_reward((sets & ~ex_words[:, None, None, :])[on].reshape(-1, 60).view(np.int64), world[on].ravel().copy()).cpu().numpy()
        assert np.array_equal(_bits(got[name][on].ravel()), _bits(priced)), name
    if rules:
        ex_cells = igm.words_to_cells(ex_words)
        for w, r in np.argwhere(on):
            dist = np.array([field[w, r][c[1], c[0]] if (0 <= c[0] < 60 and 0 <= c[1] < 60) else np.inf for c in cells[w, r]], dtype=np.float32)
            # (the prices are the device's own, held to mi_reward above: the rule is what is compared here)
            prices = {}
            for c in range(k):
                prices[igm.cells_to_words(igm.words_to_cells(route[w, r, c]) & ~ex_cells[w]).tobytes()] = got["route_gain"][w, r, c]
                prices[igm.cells_to_words(igm.words_to_cells(total[w, r, c]) & ~ex_cells[w]).tobytes()] = got["total_gain"][w, r, c]
            reward = lambda cells_, prices=prices: prices[igm.cells_to_words(cells_).tobytes()]
            want = igm.route_gains_spec(igm.words_to_cells(want_route[w, r]), igm.words_to_cells(terminal[w, r]), dist, got["n_path"][w, r] >= 0,
                                        reward, d0, ex_cells[w])
            assert got["best"][w, r] == want["best"], (w, r, got["best"][w, r], want["best"])
            for name in ("route_gain", "total_gain", "utility"):
                assert np.array_equal(_bits(got[name][w, r]), _bits(want[name])), (w, r, name)
    return got


@pytest.fixture(scope="module")
def scene():
    import torch
    env = _team(3)
    _steps(env, 10, seed=5)
    bank = S.build()
    fields = np.ascontiguousarray(np.broadcast_to(bank.fields()[None], (N, R, 60, 60)))
    cells = np.ascontiguousarray(np.broadcast_to(S.candidates(bank)[None], (N, R, K, 2)))
    rng = np.random.default_rng(3)
    hd = rng.uniform(-math.pi, math.pi, (N, R, K))
    hd[:, :, 1::2] = np.nan
    hd[:, S.B_TURNS, 1], hd[:, S.B_NONE, 13] = hd[:, S.B_TURNS, 0], hd[:, S.B_NONE, 9]  # the repeated candidates: the same pose
    hd[:, S.B_MIRROR] = hd[:, S.B_RULE, ::-1]
    yield dict(env=env, ig=env._igm.ig, bank=bank, field=fields, field_dev=torch.as_tensor(fields, device=env.device), cells=cells, hd=hd)
    env.close()


def _by_name(bank):
    return {(g["r"], g["name"]): g for g in bank.gadgets}


@pytest.mark.parametrize("stride", S.STRIDES)
def test_the_gadget_walks_sets_and_prices_are_the_rules(scene, stride):
    ig, bank = scene["ig"], scene["bank"]
    got = hold_route(ig, scene["field_dev"], scene["field"], scene["cells"], scene["hd"], stride, mask=MASK, dev=scene["env"].device,
                     same_worlds=True, rules=stride <= 3)
    on = MASK != 0
    print("stride %d: %d candidates with a route, %d without, %d way-points, %d truncated"
          % (stride, (got["n_path"][on] >= 0).sum(), (got["n_path"][on] < 0).sum(), got["n_way"][on].sum(), (got["truncated"][on] == 1).sum()))
    for g in bank.gadgets:  # what the CPU test asserted of the specification, of the device
        at = (slice(None), g["r"], g["c"])
        asked = on[:, g["r"]]
        assert (got["n_path"][at][asked] == g["n"]).all(), g["name"]
        if g["n"] < 0:  # no route: nothing is left behind
            for name in ("route_gain", "total_gain", "utility", "n_way", "truncated"):
                assert (got[name][at][asked] == 0).all(), (g["name"], name)
            assert (got["route_masks"][at][asked] == 0).all() and (got["total_masks"][at][asked] == 0).all(), g["name"]
            assert (got["way_cells"][at][asked] == -1).all() and (got["way_dir"][at][asked] == -1).all(), g["name"]
        if g["first"] is not None and stride == 1:  # the neighbour taken is the single way-point
            assert (got["n_way"][at][asked] == 1).all() and (got["way_cells"][at][asked][:, 0] == g["first"]).all(), g["name"]
    by = _by_name(bank)
    if stride == 1:
        turns = by[(S.B_TURNS, "all eight directions")]
        dirs = got["way_dir"][0, turns["r"], turns["c"]]
        assert sorted(set(dirs[:15].tolist())) == list(range(8)) and dirs[15] == -1
        assert (got["truncated"][on] == 1).sum() >= N  # the borders' and the long corridors' candidates
    # the same cell with the same heading twice in a robot's list: equal bits, and the smaller index wins
    for r, a, b in ((S.B_TURNS, 0, 1), (S.B_NONE, 9, 13)):
        for name in ("utility", "total_gain", "route_gain", "n_path"):
            assert np.array_equal(_bits(got[name][:, r, a][on[:, r]]), _bits(got[name][:, r, b][on[:, r]])), (r, name)
        assert (got["best"][:, r][on[:, r]] != b).all()
    # the own cell: no move, an empty route, and the candidate's own set priced over d0 alone
    own = by[(S.B_RULE, "own cell")]
    at = (slice(None), own["r"], own["c"])
    asked = on[:, own["r"]]
    assert (got["n_path"][at][asked] == 0).all() and (got["route_masks"][at][asked] == 0).all() and (got["route_gain"][at][asked] == 0).all()
    assert np.array_equal(_bits(got["utility"][at][asked]), _bits(got["total_gain"][at][asked] / np.float64(1.0)))
    # B_MIRROR holds B_RULE's candidates in reverse order: the same bytes
    for name in ("route_masks", "total_masks", "route_gain", "total_gain", "utility", "n_path", "n_way"):
        both = on[:, S.B_RULE] & on[:, S.B_MIRROR]
        assert np.array_equal(_bits(got[name][both][:, S.B_MIRROR]), _bits(got[name][both][:, S.B_RULE, ::-1])), name


def test_prices_and_choice_at_their_edges(scene):
    import torch
    ig, dev = scene["ig"], scene["env"].device
    field_dev, field, cells, hd = scene["field_dev"], scene["field"], scene["cells"], scene["hd"]
    plain = hold_route(ig, field_dev, field, cells, hd, 2, dev=dev, same_worlds=True, d0=0.7)
    routed = plain["n_path"] >= 0
    assert (plain["best"] >= 0).sum() >= N * 4 and (plain["total_gain"][routed] > 0).sum() > routed.sum() // 4
    # the own cell again, with a d0 that shows: utility = total_gain / (0 + d0), bit for bit
    own = _by_name(scene["bank"])[(S.B_RULE, "own cell")]
    u, tg = plain["utility"][:, own["r"], own["c"]], plain["total_gain"][:, own["r"], own["c"]]
    assert np.array_equal(_bits(u), _bits(tg / (np.float64(np.float32(0.0)) + np.float64(0.7)))) and (tg > 0).any()
    # every cell spoken for: every gain 0, nobody has a best candidate, the walks are as they were
    everything = torch.full((N, 60), -1, dtype=torch.int64, device=dev)
    none = hold_route(ig, field_dev, field, cells, hd, 2, exclude=everything, dev=dev, same_worlds=True, d0=0.7)
    for name in ("route_gain", "total_gain", "utility"):
        assert (none[name] == 0).all(), name
    assert (none["best"] == -1).all() and np.array_equal(none["n_path"], plain["n_path"]) and (none["n_path"] >= 0).any()
    for name in ("route_masks", "total_masks", "n_way", "truncated", "way_cells", "way_dir"):
        assert np.array_equal(none[name], plain[name]), name
    # a radius beyond the distance field's largest value, 42.5 m: igv_point fails where the field is finite - the route alone is priced
    wide = hold_route(ig, field_dev, field, cells, hd, 2, radius=45.0, dev=dev, same_worlds=True, d0=0.7)
    assert np.array_equal(wide["total_masks"], wide["route_masks"]) and np.array_equal(_bits(wide["total_gain"]), _bits(wide["route_gain"]))
    assert np.array_equal(wide["route_masks"], plain["route_masks"]) and np.array_equal(wide["n_path"], plain["n_path"])
    assert (wide["route_gain"] > 0).any() and (wide["best"] >= 0).any() and (plain["total_masks"] != plain["route_masks"]).any()


@pytest.mark.parametrize("k", [1, 2])
def test_one_robot_with_one_candidate_and_with_the_same_candidate_twice(scene, k):
    import torch
    ig, dev, bank = scene["ig"], scene["env"].device, scene["bank"]
    turns = _by_name(bank)[(S.B_TURNS, "all eight directions")]
    field = np.ascontiguousarray(scene["field"][:, S.B_TURNS:S.B_TURNS + 1])
    cells = np.ascontiguousarray(np.broadcast_to(np.array(turns["cell"], dtype=np.int32), (N, 1, k, 2)))
    hd = np.full((N, 1, k), 0.9)
    got = hold_route(ig, torch.as_tensor(field, device=dev), field, cells, hd, 3, dev=dev, same_worlds=True)
    assert (got["n_path"] == 16).all() and (got["n_way"] == 5).all() and (got["truncated"] == 0).all()
    sees = got["total_gain"][:, 0, 0] > 0
    assert sees.any() and np.array_equal(got["best"][:, 0], np.where(sees, 0, -1))  # (k = 2: equal utilities, the smaller index)
    if k == 2:
        assert np.array_equal(_bits(got["utility"][:, 0, 0]), _bits(got["utility"][:, 0, 1]))


# ---- the device's own fields of the hand-made worlds --------------------------------------------------------------------------------
# the sources [world][robot], cells whose centres are the points: corners of the serpentines, the staircases' far corners, the pocket
# from inside and from outside, the open map's corner and middle
SOURCES = (((0, 0), (59, 59)), ((0, 0), (59, 59)), ((0, 59), (31, 30)), ((0, 0), (46, 14)), ((21, 22), (5, 50)), ((59, 0), (29, 14)))
# four candidates per robot besides the farthest cell: seam cells of the staircases' refused diagonals, the pocket's and the lonely
# cell (no route from outside), corners
CANDS = (((59, 59), (30, 29), (0, 59), (3, 40)), ((59, 59), (29, 30), (59, 0), (40, 3)), ((31, 30), (9, 14), (43, 44), (0, 3)),
         ((46, 14), (35, 29), (13, 45), (59, 3)), ((22, 23), gw.LONELY, (19, 22), (50, 5)), ((0, 59), (59, 59), (30, 15), (0, 0)))


def test_long_walks_on_the_hand_made_worlds():
    import torch
    env = _env()
    ig = igm.InfoGain(env)
    geo = ig.geodesic(points=_points(SOURCES), radius=0.5)
    torch.cuda.synchronize()
    field = geo["field"].cpu().numpy()
    assert geo["active"].cpu().numpy().all()
    k = 5
    cells = np.zeros((N, 2, k, 2), dtype=np.int32)
    for w in range(N):
        for r in range(2):
            f = np.where(np.isfinite(field[w, r]), field[w, r], -1.0)
            j, i = np.unravel_index(int(np.argmax(f)), f.shape)
            cells[w, r, 0] = (i, j)  # the far end
            cells[w, r, 1:] = CANDS[w]
    # what the worlds are here for, on the specification alone
    far = [[igm.route_spec(field[w, r], cells[w, r, 0], 1)[0] for r in range(2)] for w in range(N)]
    print("moves to the far end: %s" % far)
    n_long = far[Y_SERP][0]
    assert n_long > 1000 and far[X_SERP][0] > 1000 and far[Y_SERP][1] > 1000
    first_whole = -(-n_long // 17)  # the first stride whose way-points are not truncated
    assert igm.route_spec(field[Y_SERP, 0], cells[Y_SERP, 0, 0], first_whole)[3] is False
    assert igm.route_spec(field[Y_SERP, 0], cells[Y_SERP, 0, 0], first_whole - 1)[3] is True
    spec1 = [[[igm.route_spec(field[w, r], cells[w, r, c], 1)[0] for c in range(k)] for r in range(2)] for w in range(N)]
    lonely = CANDS[POCKET].index(gw.LONELY) + 1
    assert spec1[POCKET][1][1] == -1 and spec1[POCKET][1][lonely] == -1 and spec1[POCKET][0][1] >= 1 and spec1[POCKET][0][4] == -1
    # the seam cells of the refused diagonals: reached in the open staircase; the closed one has two regions, a robot in each
    assert all(spec1[STAIRS][r][c] >= 1 for r in range(2) for c in range(1, k) if tuple(cells[STAIRS, r, c]) != SOURCES[STAIRS][r])
    assert all(sorted(spec1[MIRROR][r][c] >= 0 for c in range(1, k)) == [False, False, True, True] for r in range(2)), spec1[MIRROR]
    hd = np.full((N, 2, k), np.nan)
    hd[:, :, ::2] = 0.4
    for stride in (1, 64, first_whole):
        got = hold_route(ig, geo["field"], field, cells, hd, stride, dev=env.device, rules=stride == 64)
        assert got["n_path"][Y_SERP, 0, 0] == n_long and got["truncated"][Y_SERP, 0, 0] == int(stride < first_whole)
        assert got["n_way"][Y_SERP, 0, 0] == 16
        assert (got["route_masks"][Y_SERP, 0, 0] != 0).any() and got["route_gain"][Y_SERP, 0, 0] > 0
    env.close()
