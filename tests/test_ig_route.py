"""GPU: cagym_ig_route_gains (csrc/cagym_ig_route.h), its binding InfoGain.route_gains and the env's ig_route_gains, held to
ig.route_spec for the walks and the way-points, to cagym_ig_visible_cells and cagym_ig_assign_goals for the cell sets (device against
device), to cagym_ig_mi_reward for every gain and to ig.route_gains_spec for the utilities and the choice - all bit for bit.

The worlds are those of tests/test_ig_viewpoints.py - 6 worlds x 5 agents of train_stage_2 with 6 to 16 rectangles, window 24, after
ten learner steps - with 2 or 3 robots.  The raw call gets hand-picked candidate cells read from the device field, not proposals;
what they were picked for is asserted before anything is compared."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from test_ig_assign import _np, _team, _words
from test_ig_viewpoints import E_INVALID, E_STATE, K, M, N, RADIUS, SEED, _B, _bits, _steps

pytestmark = pytest.mark.gpu
igm = importlib.import_module("gym-exploration-2d_amd.ig")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
D0 = 1.0
KINDS = ("far", "diagonal", "beside", "own", "infinite", "outside", "near")  # candidates 0..6 of every robot; the rest: any finite cell
OUT_KEYS = ("route_masks", "total_masks", "route_gain", "total_gain", "utility", "n_path", "n_way", "truncated", "best", "way_cells", "way_dir")


def _centres(cells):
    return cells.astype(np.float64) * 0.5 - 15.0 + 0.25  # (a cell outside the map: a point outside it)


def _beside(field, path):
    """a cell of the path has a blocked (non-finite) cell of the map as an orthogonal neighbour"""
    for (i, j, _) in path:
        for di, dj in igm.GEO_NEIGHBOURS[:4]:
            if 0 <= i + di < 60 and 0 <= j + dj < 60 and not np.isfinite(field[j + dj, i + di]):
                return True
    return False


def _pick(field, rng):
    """16 candidate cells (i, j) of one robot in the order of KINDS, then any finite cells"""
    fin = np.argwhere(np.isfinite(field))
    own = np.argwhere(field == 0)
    assert len(own) == 1
    oj, oi = own[0]
    if len(fin) < 500:  # a robot that stands walled in, within radius + 0.1 of a rectangle: its own cell, and cells it cannot reach
        blocked = np.argwhere(~np.isfinite(field))[rng.permutation((~np.isfinite(field)).sum())[:16]][:, ::-1]
        blocked[[KINDS.index(n) for n in KINDS if n not in ("infinite", "outside")]] = (oi, oj)
        blocked[KINDS.index("outside")] = (-1, 7)
        return blocked.astype(np.int32), False
    j, i = fin[np.argmax(field[fin[:, 0], fin[:, 1]])]
    cells = {"far": (i, j), "own": (oi, oj), "outside": (-1, int(rng.integers(0, 60)))}
    j, i = np.argwhere(~np.isfinite(field))[int(rng.integers(0, (~np.isfinite(field)).sum()))]
    cells["infinite"] = (i, j)
    near = [(oi + di, oj + dj) for di, dj in igm.GEO_NEIGHBOURS[:4] if 0 <= oi + di < 60 and 0 <= oj + dj < 60 and np.isfinite(field[oj + dj, oi + di])]
    cells["near"] = near[0] if near else (oi, oj)
    order = fin[rng.permutation(len(fin))]
    rest = []
    for j, i in order[:200]:
        path = igm.route_path_spec(field, (i, j))
        if "diagonal" not in cells and any(m is not None and m >= 4 for _, _, m in path) and len(path) > 6:
            cells["diagonal"] = (i, j)
        elif "beside" not in cells and _beside(field, path) and len(path) > 6:
            cells["beside"] = (i, j)
        elif len(rest) < 16 - len(KINDS):
            rest.append((i, j))
        if len(cells) == len(KINDS) and len(rest) == 16 - len(KINDS):
            break
    for n in ("diagonal", "beside"):
        cells.setdefault(n, rest[0])
    return np.array([cells[n] for n in KINDS] + rest, dtype=np.int32), True


@pytest.fixture(scope="module", params=[2, 3])
def scene(request):
    """one env per team size: ten learner steps, every robot's own field read back, 16 hand-picked candidate cells per robot"""
    import torch
    R = request.param
    env = _team(R)
    _steps(env, 10, seed=5)
    ig = env._igm.ig
    st = env.state()
    here = torch.stack((st["pos_x"][:, :R], st["pos_y"][:, :R]), dim=-1).contiguous()
    geo = ig.geodesic(points=here, radius=RADIUS)
    torch.cuda.synchronize()
    field = geo["field"].cpu().numpy()
    rng = np.random.default_rng(17)
    cells, roomy = np.zeros((N, R, 16, 2), dtype=np.int32), np.zeros((N, R), dtype=bool)
    for w in range(N):
        for r in range(R):
            cells[w, r], roomy[w, r] = _pick(field[w, r], rng)
    assert roomy.sum() >= N * R - 2 and roomy.any(axis=1).all()  # (every world has a robot with room to drive)
    # what the candidates were picked for
    spec1 = [[[igm.route_spec(field[w, r], cells[w, r, c], 1) for c in range(16)] for r in range(R)] for w in range(N)]
    paths = [[[igm.route_path_spec(field[w, r], cells[w, r, c]) for c in range(16)] for r in range(R)] for w in range(N)]
    at = lambda n: KINDS.index(n)
    for w in range(N):
        for r in range(R):
            s = spec1[w][r]
            assert s[at("own")][0] == 0 and s[at("infinite")][0] == -1 and s[at("outside")][0] == -1 and (cells[w, r, at("outside")] == -1).any()
            assert not np.isfinite(field[w, r][cells[w, r, at("infinite"), 1], cells[w, r, at("infinite"), 0]])
    far = np.array([[spec1[w][r][at("far")][0] for r in range(R)] for w in range(N)])[roomy]
    assert (far >= 18).all() and all(spec1[w][r][at("far")][3] for w, r in np.argwhere(roomy))  # n >= 18 at stride 1: truncated
    n_diag = sum(any(m is not None and m >= 4 for _, _, m in paths[w][r][at("diagonal")]) for w in range(N) for r in range(R))
    n_beside = sum(_beside(field[w, r], paths[w][r][at("beside")]) for w in range(N) for r in range(R))
    n_near = sum(1 <= spec1[w][r][at("near")][0] < 4 for w in range(N) for r in range(R))
    print("R %d: far n %d .. %d, %d diagonal, %d beside, %d near of %d robots with room" % (R, far.min(), far.max(), n_diag, n_beside, n_near, roomy.sum()))
    assert n_diag >= N and n_beside >= N and n_near >= N  # (stride 4 and 7 exceed a near candidate's n: no way-points)
    yield dict(env=env, ig=ig, R=R, field_dev=geo["field"], field=field, cells=cells)
    env.close()


def _sentinels(dev, R, k):
    import torch
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)
    return {"route_masks": full((N, R, k, 60), -7, torch.int64), "total_masks": full((N, R, k, 60), -7, torch.int64),
            "route_gain": full((N, R, k), -7.0, torch.float64), "total_gain": full((N, R, k), -7.0, torch.float64),
            "utility": full((N, R, k), -7.0, torch.float64), "n_path": full((N, R, k), -7, torch.int32), "n_way": full((N, R, k), -7, torch.int32),
            "truncated": full((N, R, k), 7, torch.uint8), "best": full((N, R), -7, torch.int32),
            "way_cells": full((N, R, k, 16, 2), -7, torch.int32), "way_dir": full((N, R, k, 16), -7, torch.int8)}


def _untouched(name, a):
    return a == (7 if name == "truncated" else -7)


def _reward_of(ig, w):
    return lambda cells: float(ig.mi_reward(igm.cells_to_words(cells).view(np.int64), [w]).cpu().numpy()[0])


@pytest.mark.parametrize("k,stride,headed,excluded", [(16, 1, True, True), (16, 4, False, False), (8, 7, True, False), (1, 4, False, True),
                                                      (8, 1, False, True), (16, 7, True, True), (8, 4, True, True)])
def test_routes_sets_prices_and_choices_are_the_rules(scene, k, stride, headed, excluded):
    import torch
    ig, R, field = scene["ig"], scene["R"], scene["field"]
    cells = np.ascontiguousarray(scene["cells"][:, :, :k])
    rng = np.random.default_rng(100 * k + stride)
    hd = None
    if headed:  # a heading for the candidates of even index, NaN - turning on the spot - for the others
        hd = rng.uniform(-math.pi, math.pi, (N, R, k))
        hd[:, :, 1::2] = np.nan
    mask = np.ones((N, R), dtype=np.uint8)
    mask[1, 0], mask[2], mask[4, R - 1] = 0, 0, 0  # worlds 1 and 4: one robot does not ask; world 2: nobody does
    on = mask != 0
    xy = _centres(cells)
    # the candidates' own sets as cagym_ig_assign_goals builds them, and (excluded) what a team assignment on them claimed
    asg = _np(ig.assign_goals(xy, np.ones((N, R, k), dtype=np.float32), cand_heading=hd, mode="best", radius=RADIUS, d0=D0, want_rounds=False))
    terminal = _words(asg["masks"])
    exclude = asg["claimed"] if excluded else None
    ex_words = _words(asg["claimed"]) if excluded else np.zeros((N, 60), dtype=np.uint64)
    if excluded:
        assert (ex_words != 0).any(axis=1).all()
    out = _sentinels(scene["env"].device, R, k)
    got = ig.route_gains(scene["field_dev"], cells, cand_heading=hd, mask=mask, exclude=exclude, stride=stride, radius=RADIUS, d0=D0, out=out,
                         want_waypoints=True)
    assert got is out and sorted(got) == sorted(OUT_KEYS)
    got = _np(out)
    # ---- 5. rows of robots outside the mask, and the world nobody asks in, keep every byte
    for n in OUT_KEYS:
        assert _untouched(n, got[n][~on]).all(), n
    for n in ("n_path", "n_way", "truncated", "best", "route_gain", "total_gain", "utility"):
        assert not _untouched(n, got[n][on]).any(), n
    assert not _untouched("route_masks", got["route_masks"][on]).any() and not _untouched("way_dir", got["way_dir"][on]).any()
    # ---- 1. the walks and the way-points
    poses, owner = [], []
    for w, r in np.argwhere(on):
        for c in range(k):
            n, wc, wd, trunc = igm.route_spec(field[w, r], cells[w, r, c], stride)
            at = (w, r, c)
            assert got["n_path"][at] == n and got["n_way"][at] == len(wd) and got["truncated"][at] == int(trunc), (at, n, got["n_path"][at])
            assert np.array_equal(got["way_cells"][at][:len(wd)], wc) and np.array_equal(got["way_dir"][at][:len(wd)], wd), at
            assert (got["way_cells"][at][len(wd):] == -1).all() and (got["way_dir"][at][len(wd):] == -1).all(), at
            for (i, j), d in zip(wc, wd):
                poses.append((i * 0.5 - 15.0 + 0.25, j * 0.5 - 15.0 + 0.25, igm.route_heading(d)))
                owner.append(at)
    n_way, n_path = got["n_way"][on], got["n_path"][on]
    print("R %d k %d stride %d: %d candidates, %d without a route, %d way-points, %d truncated" %
          (R, k, stride, n_path.size, (n_path < 0).sum(), n_way.sum(), (got["truncated"][on] == 1).sum()))
    assert (n_way > 0).any() and ((got["truncated"][on] == 1).any() or stride > 1)  # (the far candidates: n >= 18)
    if k >= 8:
        assert (n_path < 0).sum() >= 2 * on.sum() and (n_path == 0).sum() >= on.sum() and ((n_path > 0) & (n_way == 0)).any()
    # ---- 2. route_masks: the OR of cagym_ig_visible_cells over the way-point poses
    want_route = np.zeros((N, R, k, 60), dtype=np.uint64)
    vis = _words(ig.visible_cells(np.array(poses), np.array([o[0] for o in owner], dtype=np.int32)))
    for o, m in zip(owner, vis):
        want_route[o] |= m
    route, total = _words(np.where(on[..., None, None], got["route_masks"], 0)), _words(np.where(on[..., None, None], got["total_masks"], 0))
    assert np.array_equal(route[on], want_route[on]), np.argwhere((route != want_route).any(-1) & on[..., None])[:5]
    assert int(route.max()) < 1 << 60 and (route[on] != 0).any()
    # ---- 3. total_masks: route | the candidate's own set (a candidate without a route: empty)
    has = (got["n_path"] >= 0) & on[..., None]
    want_total = np.where(has[..., None], want_route | terminal, np.uint64(0))
    assert np.array_equal(total[on], want_total[on]), np.argwhere((total != want_total).any(-1) & on[..., None])[:5]
    assert (terminal[has] != 0).any() and ((want_total != want_route) & has[..., None]).any()
    # ---- 4. every gain is cagym_ig_mi_reward's double; utility and best are the specification's
    world = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None, None], (N, R, k))
    for name, sets in (("route_gain", route), ("total_gain", total)):
        priced = ig.mi_reward((sets & ~ex_words[:, None, None, :])[on].reshape(-1, 60).view(np.int64), world[on].ravel().copy()).cpu().numpy()
        assert np.array_equal(_bits(got[name][on].ravel()), _bits(priced)), name
    assert (got["total_gain"][on] >= got["route_gain"][on]).all() and (got["route_gain"][on] > 0).any()
    ex_cells = igm.words_to_cells(ex_words)
    n_best = 0
    for w, r in np.argwhere(on):
        dist = np.array([field[w, r][c[1], c[0]] if (0 <= c[0] < 60 and 0 <= c[1] < 60) else np.inf for c in cells[w, r]], dtype=np.float32)
        want = igm.route_gains_spec(igm.words_to_cells(want_route[w, r]), igm.words_to_cells(terminal[w, r]), dist, got["n_path"][w, r] >= 0,
                                    _reward_of(ig, w), D0, ex_cells[w])
        assert got["best"][w, r] == want["best"], (w, r, got["best"][w, r], want["best"])
        for name in ("route_gain", "total_gain", "utility"):
            assert np.array_equal(_bits(got[name][w, r]), _bits(want[name])), (w, r, name)
        n_best += int(want["best"] >= 0)
    assert n_best >= (on.sum() // 2 if k >= 8 else 1)
    # ---- 5. two launches give the same bytes; a call without the way-point outputs gives the same other outputs
    again = _sentinels(scene["env"].device, R, k)
    ig.route_gains(scene["field_dev"], cells, cand_heading=hd, mask=mask, exclude=exclude, stride=stride, radius=RADIUS, d0=D0, out=again,
                   want_waypoints=True)
    bare = {n: v for n, v in _sentinels(scene["env"].device, R, k).items() if not n.startswith("way_")}
    res = ig.route_gains(scene["field_dev"], cells, cand_heading=hd, mask=mask, exclude=exclude, stride=stride, radius=RADIUS, d0=D0, out=bare)
    assert sorted(res) == sorted(n for n in OUT_KEYS if not n.startswith("way_"))
    again, bare = _np(again), _np(bare)
    for n in OUT_KEYS:
        assert np.array_equal(_bits(got[n]), _bits(again[n])), n
        if n in bare:
            assert np.array_equal(_bits(got[n]), _bits(bare[n])), n


def test_eight_robots_with_sixteen_candidates_each(scene):
    """the entry's limits: 128 candidates per world on the scene's fields, repeated to eight robots, against the specification"""
    import torch
    ig, R0, k = scene["ig"], scene["R"], 16
    reps = [r % R0 for r in range(8)]
    field_dev = scene["field_dev"][:, reps].contiguous()
    field = scene["field"][:, reps]
    cells = np.ascontiguousarray(scene["cells"][:, reps])
    cells[:, R0:] = cells[:, R0:, ::-1]  # the repeated robots hold their candidates in reverse order
    got = _np(ig.route_gains(field_dev, cells, stride=4, radius=RADIUS, d0=D0, want_waypoints=True))
    for w in range(N):
        for r in range(8):
            for c in range(k):
                n, wc, wd, trunc = igm.route_spec(field[w, r], cells[w, r, c], 4)
                assert got["n_path"][w, r, c] == n and got["n_way"][w, r, c] == len(wd) and got["truncated"][w, r, c] == int(trunc)
                assert np.array_equal(got["way_cells"][w, r, c][:len(wd)], wc) and np.array_equal(got["way_dir"][w, r, c][:len(wd)], wd)
    for n in ("route_masks", "total_masks", "route_gain", "total_gain", "utility", "n_path"):
        assert np.array_equal(_bits(got[n][:, R0:2 * R0]), _bits(got[n][:, :R0, ::-1])), n  # the same candidate, the same bytes
    assert (got["best"] >= 0).mean() > 0.9


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def _P(**kw):
    p = dict(n_robots=2, k=4, stride=4, flags=0, radius=RADIUS, range=5.0, fov=math.pi / 3, d0=1.0)
    p.update(kw)
    return _lib.IgRouteParams(*[p[f[0]] for f in _lib.IgRouteParams._fields_])


def test_the_entry_refuses_and_touches_nothing():
    import torch
    R, k = 2, 4
    env = _B()(N, M, max_obstacles=K, game_over_mode="agent0")
    assert env.generate_exploration_worlds(kinds="train_stage_2", seed=SEED, n_robots=R, n_targets=M - R, n_obst=(6, 16), target_radius=0.2,
                                           robot_pref_speed=0.2) == 0
    env.reset()
    dev = env.device
    t = _sentinels(dev, R, k)
    field = torch.full((N, R, 60, 60), float("inf"), dtype=torch.float32, device=dev)
    field[:, :, 30, 30], field[:, :, 30, 31] = 0.0, 0.5
    cells = torch.zeros((N, R, k, 2), dtype=torch.int32, device=dev)
    cells[..., 0], cells[..., 1] = 31, 30
    L, h, s, p = env.L, env.h, env._stream, _lib.ptr

    def call(P, **kw):
        a = dict(t, field=field, cand_cells=cells)
        a.update(kw)
        return L.cagym_ig_route_gains(h, None if P is None else C.byref(P), None, p(a["field"]), p(a["cand_cells"]), None, None,
                                      *[p(a[n]) for n in OUT_KEYS], s())

    assert call(_P()) == E_STATE and b"cagym_ig_route_gains before cagym_ig_init" in L.cagym_last_error(h)
    ig = igm.InfoGain(env)  # (cagym_ig_init)
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_robots=0), dict(n_robots=9), dict(n_robots=-1), dict(k=0), dict(k=17), dict(k=-3), dict(stride=0), dict(stride=-4), dict(flags=1)]
    for f in ("radius", "range", "fov", "d0"):
        bad += [{f: 0.0}, {f: -1.0}, {f: nan}, {f: inf}]
    for kw in bad:
        assert call(_P(**kw)) == E_INVALID and b"cagym_ig_route_gains" in L.cagym_last_error(h), kw
    assert call(None) == E_INVALID
    for missing in ("field", "cand_cells") + OUT_KEYS[:9]:
        assert call(_P(), **{missing: None}) == E_INVALID, missing
    torch.cuda.synchronize()
    for n, v in t.items():
        assert _untouched(n, v).all(), n  # nothing was launched
    assert call(_P(), way_cells=None, way_dir=None) == 0  # the way-point outputs are optional
    torch.cuda.synchronize()
    assert _untouched("way_cells", t["way_cells"]).all() and _untouched("way_dir", t["way_dir"]).all()
    assert (t["n_path"] == 1).all() and (t["n_way"] == 0).all() and (t["truncated"] == 0).all() and (t["route_masks"] == 0).all()
    sees = (t["total_masks"] != 0).any(-1).any(-1)  # one move east of the source: no way-point, the own view where a robot can stand
    assert sees.any() and (t["best"] == torch.where(sees, 0, -1)).all()
    assert call(_P(stride=2 ** 31 - 1)) == 0  # (any stride >= 1)
    torch.cuda.synchronize()
    assert (t["n_path"] == 1).all() and (t["way_dir"] == -1).all()
    with pytest.raises(ValueError, match="must be \\[N, R, k, 2\\]"):
        ig.route_gains(field, cells[0])
    with pytest.raises(ValueError, match="field must be"):
        ig.route_gains(field[:, :1], cells)
    env.close()


# ---- 7. through the env -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("headings", [None, 8])
def test_the_env_prices_the_last_proposals_and_sends_the_team(headings):
    import torch
    R = 2
    env = _team(R)
    _steps(env, 10, seed=5)
    with pytest.raises(RuntimeError, match="needs an earlier ig_propose_goals"):
        env.ig_route_gains()
    assert env._goals.route is None  # a refused call allocated nothing
    prop = env.ig_propose_goals(k=8, min_sep=2.0, d0=0.5, headings=headings)
    with pytest.raises(ValueError, match="stride must be at least 1"):
        env.ig_route_gains(stride=0)
    with pytest.raises(ValueError, match="d0 must be finite and positive"):
        env.ig_route_gains(d0=0.0)
    assert env._goals.route is None
    prop["cells"][2, 1] = -1  # a robot whose proposals are gone: no route, nothing to choose
    mask = np.array([[1, 1], [1, 0], [1, 1], [0, 1], [1, 1], [0, 0]], dtype=np.uint8)
    on = mask != 0
    env.ig_set_goals(np.zeros((N, R, 2)) + 100.0)  # nobody has an active goal (outside the map)
    assert not _np(env.ig_goals())["active"].any()
    a = _np(env.ig_route_gains(mask=mask, stride=4, set_goals=True))
    assert sorted(a) == sorted(OUT_KEYS[:9] + ("xy", "heading"))
    ig = env._igm.ig
    raw = _np(ig.route_gains(env._goals.own["field"], prop["cells"], cand_heading=prop["heading"] if headings else None, mask=mask, stride=4,
                             radius=RADIUS, d0=0.5))  # (d0 is the proposal call's)
    for n in raw:
        assert np.array_equal(_bits(a[n][on]), _bits(raw[n][on])), n
    took = on & (a["best"] >= 0)
    assert a["best"][2, 1] == -1 and (a["n_path"][2, 1] == -1).all() and took.sum() >= 5 and (a["n_way"][on] > 0).any()
    pxy, idx = prop["xy"].cpu().numpy(), np.clip(a["best"], 0, None)
    want_xy = np.take_along_axis(pxy, idx[:, :, None, None].repeat(2, -1), 2)[:, :, 0]
    assert np.array_equal(_bits(a["xy"][took]), _bits(want_xy[took])) and np.isnan(a["xy"][~took]).all()
    g = _np(env.ig_goals())
    assert np.array_equal(g["active"][on], took[on].astype(np.uint8)) and g["active"][2, 1] == 0 and not g["active"][~on].any()
    assert np.array_equal(_bits(g["goal_xy"][took]), _bits(a["xy"][took]))
    if headings is None:
        assert np.isnan(a["heading"]).all() and "goal_heading" not in g
    else:
        ph = np.take_along_axis(prop["heading"].cpu().numpy(), idx[:, :, None], 2)[:, :, 0]
        assert np.isfinite(a["heading"][took]).all() and np.array_equal(_bits(a["heading"][took]), _bits(ph[took])) and np.isnan(a["heading"][~took]).all()
        assert np.array_equal(_bits(g["goal_heading"][took]), _bits(a["heading"][took]))
    # exclude = what a team assignment claimed: no mask shrinks or grows, no gain rises
    claimed = env.ig_assign_goals(mode="best", mask=mask, set_goals=False)["claimed"]
    b = _np(env.ig_route_gains(mask=mask, stride=4, exclude=claimed))
    for n in ("route_masks", "total_masks", "n_path", "n_way", "truncated"):
        assert np.array_equal(_bits(a[n][on]), _bits(b[n][on])), n
    assert (b["route_gain"][on] <= a["route_gain"][on]).all() and (b["total_gain"][on] <= a["total_gain"][on]).all()
    assert (b["total_gain"][on] < a["total_gain"][on]).any()
    assert sorted(env.step()[3]) == sorted(["belief_window", "flags", "gain", "goal_distance", "goal_reached", "observed"] +
                                           (["goal_facing"] if headings else []))  # step() gains nothing
    env.close()


def test_a_twin_that_never_prices_routes_steps_and_proposes_the_same_bits():
    import torch
    envs = [_team(2), _team(2)]
    outs = [[], []]
    for n, env in enumerate(envs):
        rng = np.random.default_rng(4)
        for t in range(6):
            a = np.stack([rng.uniform(0.0, 1.5, (N, M)), rng.uniform(-2.0, 2.0, (N, M))], axis=-1).astype(np.float32)
            obs, rew, go, info = env.step(torch.as_tensor(a, device=env.device))
            prop = env.ig_propose_goals(k=4)
            if n == 0:
                env.ig_route_gains(stride=1 + t)
            torch.cuda.synchronize()
            keep = [rew, go, info["flags"], info["belief_window"], info["gain"], info["observed"], info["goal_distance"]]
            keep += [obs[key] for key in sorted(obs)] if isinstance(obs, dict) else [obs]
            keep += [prop[key] for key in sorted(prop)]
            outs[n].append([v.cpu().numpy().copy() for v in keep])
    for t in range(6):
        assert len(outs[0][t]) == len(outs[1][t])
        for x, y in zip(outs[0][t], outs[1][t]):
            assert np.array_equal(_bits(x), _bits(y)), t
    for env in envs:
        env.close()


def test_the_env_refuses_without_goals():
    env = _B()(N, M, max_obstacles=K, game_over_mode="agent0")
    assert env.generate_exploration_worlds(kinds="train_stage_2", seed=SEED, n_robots=2, n_targets=3, n_obst=(6, 16), target_radius=0.2,
                                           robot_pref_speed=0.2) == 0
    env.reset()
    env.attach_ig_learner()
    with pytest.raises(RuntimeError, match="needs attach_ig_goals"):
        env.ig_route_gains()
    env.close()
