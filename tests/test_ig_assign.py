"""GPU: cagym_ig_assign_goals (csrc/cagym_ig_assign.h), its binding InfoGain.assign_goals and the env's ig_assign_goals, held to
cagym_ig_visible_cells / cagym_ig_view_gain for the cell sets, to cagym_ig_mi_reward for every marginal gain and to
ig.assign_goals_spec for the selection, all bit for bit.

The worlds are those of tests/test_ig_viewpoints.py - 6 worlds x 5 agents of train_stage_2 with 6 to 16 rectangles, window 24, after
ten learner steps, so the belief is not uniform - with 2 or 3 robots.  What the seeds and the candidates were chosen for is asserted
before anything is compared.  A cell exactly on a cone edge or on the range circle is decided by the last bit of sine and cosine, so
the cell sets are compared with the host specification on cell-centre candidates at range 4.9 and headings h 2 pi / 8, whose margins
are asserted first; everywhere else the comparison is device against device."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from test_ig_headings_spec import margins
from test_ig_viewpoints import CENTRES, E_INVALID, E_STATE, K, M, N, RADIUS, SEED, _B, _bits, _points_of, _state, _steps

pytestmark = pytest.mark.gpu
igm = importlib.import_module("gym-exploration-2d_amd.ig")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
D0 = 1.0


def _team(R, seed=SEED, stream=False, pref=0.2):
    env = _B()(N, M, n_scenarios=2 * N if stream else N, max_obstacles=K, game_over_mode="agent0")
    fill = env.stream_exploration_worlds if stream else env.generate_exploration_worlds
    assert fill(kinds="train_stage_2", seed=seed, n_robots=R, n_targets=M - R, n_obst=(6, 16), target_radius=0.2, robot_pref_speed=pref) == 0
    env.reset()
    env.attach_ig_learner(window=24, rotate=True)
    env.attach_ig_goals(radius=RADIUS)
    env.reset()
    return env


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _words(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint64)


def _pop(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1).sum(axis=-1)


@pytest.fixture(scope="module", params=[2, 3])
def scene(request):
    """one env per team size: ten learner steps, 64 labelled points per world, the read-back fields and cell MI"""
    R = request.param
    env = _team(R)
    _steps(env, 10, seed=5)
    pos, edf, mi, _ = _state(env)
    assert np.ptp(mi) > 1e-3  # the belief, and with it the MI, is no longer uniform
    ob = env.obstacles()
    rects, n_obst = ob["obstacles"].cpu().numpy(), ob["n_obst"].cpu().numpy()
    rng = np.random.default_rng(9)
    points, kinds = np.zeros((N, 64, 2)), []
    for w in range(N):
        points[w], kd = _points_of(w, pos, edf[w], rects[w], n_obst[w], rng)
        kinds.append(kd)
    yield dict(env=env, ig=env._igm.ig, R=R, pos=pos, edf=edf, mi=mi, points=points, kinds=kinds)
    env.close()


def _candidates(sc, R, k, seed, centres=False, bad_distances=True):
    """R k of each world's 64 labelled points (beside and inside rectangles, map corners and edges, outside, NaN, the clearance
    band, off-centre) dealt to R robots, and their distance from robot r's place as f32 - a few of them NaN or infinite.  centres:
    every finite point inside the map moves to the centre of its cell."""
    rng = np.random.default_rng(seed)
    xy, dist, kinds = np.zeros((N, R, k, 2)), np.zeros((N, R, k), dtype=np.float32), []
    for w in range(N):
        must = [sc["kinds"][w].index(n) for n in ("outside", "nan", "inside", "edge", "beside")] if R * k >= 8 else []  # (k = 1: any points)
        rest = [p for p in rng.permutation(64) if p not in must]
        pick = np.array((must + rest)[:R * k])[rng.permutation(R * k)]
        xy[w] = sc["points"][w][pick].reshape(R, k, 2)
        kinds.append([sc["kinds"][w][p] for p in pick])
    if centres:
        inside = np.isfinite(xy).all(-1, keepdims=True) & (np.abs(xy) < 15.0).all(-1, keepdims=True)
        with np.errstate(invalid="ignore"):
            snapped = CENTRES[np.clip(np.floor((np.nan_to_num(xy) + 15.0) / 0.5), 0, 59).astype(int)]
        xy = np.where(inside, snapped, xy)
    with np.errstate(invalid="ignore"):
        d = np.hypot(xy[..., 0] - sc["pos"][:, :R, None, 0], xy[..., 1] - sc["pos"][:, :R, None, 1])
    dist[:] = np.where(np.isfinite(d), d, 3.0).astype(np.float32)
    if bad_distances and k >= 8:
        dist[:, :, 2] = np.nan
        dist[:, 0, 5] = np.inf
    return xy, dist, kinds


def _headings(xy, seed, lattice=False):
    """a heading for the candidates of even index (any angle, or h 2 pi / 8), NaN - turning on the spot - for the others"""
    rng = np.random.default_rng(seed)
    hd = rng.integers(0, 8, xy.shape[:3]) * (2.0 * math.pi / 8) if lattice else rng.uniform(-math.pi, math.pi, xy.shape[:3])
    hd[:, :, 1::2] = np.nan
    return hd


# ---- 1. the cell sets -------------------------------------------------------------------------------------------------------------------
def test_cell_sets_are_those_of_visible_cells_and_view_gain(scene):
    ig, R, k = scene["ig"], scene["R"], 16
    xy, dist, kinds = _candidates(scene, R, k, seed=1)
    hd = _headings(xy, seed=2)
    got = _np(ig.assign_goals(xy, dist, cand_heading=hd, mode="best", radius=RADIUS, d0=D0, want_rounds=False))
    assert sorted(got) == ["choice", "claimed", "marginal", "masks", "order", "utility"] and got["masks"].shape == (N, R, k, 60)
    masks = _words(got["masks"])
    view = _np(ig.view_gain(points=xy.reshape(N, R * k, 2), radius=RADIUS))
    valid, n_vis = view["valid"].reshape(N, R, k) != 0, view["n_visible"].reshape(N, R, k)
    headed = np.isfinite(hd)
    flat = [n for kd in kinds for n in kd]
    by_kind = {n: (int(np.sum([valid.ravel()[q] for q in range(len(flat)) if flat[q] == n])), flat.count(n)) for n in sorted(set(flat))}
    print("candidates valid / all by kind: %s; headed and valid %d, turning and valid %d" % (by_kind, (headed & valid).sum(), (~headed & valid).sum()))
    # what the candidates were chosen for
    assert by_kind["outside"] == (0, N) and by_kind["nan"] == (0, N) and by_kind["inside"][0] == 0 and by_kind["inside"][1] >= N
    assert by_kind["beside"][0] >= N // 2 and by_kind["edge"][0] >= N // 2 and by_kind["off-centre"][0] >= N
    assert (headed & valid).sum() >= N * R * k // 4 and (~headed & valid).sum() >= N * R * k // 4 and (~valid & headed).any() and (~valid & ~headed).any()
    assert (_pop(masks)[~valid] == 0).all()  # an invalid point: the empty set, with or without a heading
    poses = np.concatenate([np.where(valid[..., None], xy, 0.0), np.where(headed, hd, 0.0)[..., None]], axis=-1)
    world = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None, None], (N, R, k)).copy()
    cone = _words(ig.visible_cells(poses.reshape(-1, 3), world.ravel())).reshape(N, R, k, 60)
    sel = headed & valid
    assert np.array_equal(masks[sel], cone[sel]), np.argwhere((masks != cone).any(-1) & sel)[:5]  # every one of them, bit for bit
    sel = ~headed & valid
    assert np.array_equal(_pop(masks)[sel], n_vis[sel]), np.argwhere((_pop(masks) != n_vis) & sel)[:5]
    assert (_pop(masks)[headed & valid] < _pop(masks)[sel].max()).all() and _pop(masks)[sel].max() > 100
    assert int(masks.max()) < 1 << 60


def test_cell_sets_equal_the_specification_on_the_lattice(scene):
    ig, R, k, rng = scene["ig"], scene["R"], 8, 4.9
    xy, dist, kinds = _candidates(scene, R, k, seed=3, centres=True)
    hd = _headings(xy, seed=4, lattice=True)
    edf, mi = scene["edf"], scene["mi"]
    want = np.zeros((N, R, k, 60, 60), dtype=bool)
    n_valid = n_headed = occluded = 0
    for w in range(N):
        for r in range(R):
            for c in range(k):
                p, phi = xy[w, r, c], hd[w, r, c]
                if np.isfinite(phi):
                    s = igm.view_gain_headings_spec(edf[w], mi[w], p, [phi], RADIUS, ig.fov, rng)
                    want[w, r, c], ok = s["masks"][0], s["valid"]
                    free = igm.view_gain_headings_spec(np.full((300, 300), 50.0), mi[w], p, [phi], RADIUS, ig.fov, rng)["masks"][0]
                else:
                    _, _, ok, want[w, r, c], inr = igm.view_gain_spec(edf[w], mi[w], p, RADIUS, rng)
                    free = inr
                if ok:  # the margins of the input: no cell within 1e-6 of the range circle or (with a heading) of a cone edge
                    a, rad = margins(p[0], p[1], [phi] if np.isfinite(phi) else [], ig.fov, rng)
                    assert rad > 1e-6 and a > 1e-6, (w, r, c, p, phi, a, rad)
                    n_valid, n_headed, occluded = n_valid + 1, n_headed + int(np.isfinite(phi)), occluded + int(want[w, r, c].sum() < free.sum())
                else:
                    assert not want[w, r, c].any()
    print("%d valid candidates of %d, %d with a heading, %d with an occluded cell" % (n_valid, N * R * k, n_headed, occluded))
    assert n_valid >= N * R * k // 2 and n_valid < N * R * k and n_headed >= n_valid // 4 and n_headed < n_valid and 4 * occluded >= n_valid
    got = ig.assign_goals(xy, dist, cand_heading=hd, mode="slot", radius=RADIUS, range=rng, d0=D0, want_rounds=False)
    cells = igm.words_to_cells(_words(got["masks"]))
    assert np.array_equal(cells, want), np.argwhere((cells != want).any(axis=(-1, -2)))[:5]  # every mask, none left out


# ---- 2. and 3. pricing and selection ------------------------------------------------------------------------------------------------------
def _device_sets(ig, xy, hd):
    """the cell sets of N x P poses (P <= 8) as the entry itself builds them: candidates of P robots with one candidate each"""
    P = xy.shape[1]
    out = ig.assign_goals(xy.reshape(N, P, 1, 2), np.ones((N, P, 1), dtype=np.float32), cand_heading=hd.reshape(N, P, 1), mode="slot",
                          radius=RADIUS, want_rounds=False)
    return igm.words_to_cells(_words(out["masks"]))[:, :, 0]


def _reward_of(ig, w):
    return lambda cells: float(ig.mi_reward(igm.cells_to_words(cells).view(np.int64), [w]).cpu().numpy()[0])


def _check_against_rule(ig, got, dist, valid, mask, seed_cells, mode, d0):
    """got: the entry's read-back outputs for [N, R, k] candidates; seed_cells [N, 60, 60] bool.  The pricing: every finite
    round_gain is mi_reward of masks & ~(what was claimed before that round, rebuilt from masks, choice and order), bit for bit, and
    marginal the chosen entry's bits.  The selection: choice, order, claimed, utility, marginal and round_gain are assign_goals_spec's
    on the read-back masks with reward = mi_reward."""
    R, k = dist.shape[1:]
    cells = igm.words_to_cells(_words(got["masks"]))
    rg, choice, order = got["round_gain"], got["choice"], got["order"]
    q_words, q_world, q_at = [], [], []
    for w in range(N):
        on = np.flatnonzero(mask[w])
        if not len(on):
            continue
        for t in range(R):
            before = seed_cells[w].copy()
            for r in on:
                if 0 <= order[w, r] < t:
                    before |= cells[w, r, choice[w, r]]
            for r, c in np.argwhere(np.isfinite(rg[w, t])):
                q_words.append(igm.cells_to_words(cells[w, r, c] & ~before))
                q_world.append(w)
                q_at.append((w, t, r, c))
    assert len(q_at) >= (N if k >= 8 else 1)  # something was priced
    priced = ig.mi_reward(np.array(q_words).view(np.int64), np.array(q_world, dtype=np.int32)).cpu().numpy()
    at = tuple(np.array(q_at).T)
    assert np.array_equal(_bits(rg[at]), _bits(priced)), np.array(q_at)[_bits(rg[at]) != _bits(priced)][:5]
    for w in range(N):
        on = np.flatnonzero(mask[w])
        if not len(on):
            continue
        want = igm.assign_goals_spec(cells[w], seed_cells[w], dist[w], valid[w], _reward_of(ig, w), mode, d0, on)
        assert np.array_equal(choice[w, on], want["choice"][on]) and np.array_equal(order[w, on], want["order"][on]), (w, choice[w], want["choice"])
        assert np.array_equal(igm.words_to_cells(_words(got["claimed"]))[w], want["claimed"]), w
        for n in ("utility", "marginal"):
            assert np.array_equal(_bits(got[n][w, on]), _bits(want[n][on])), (w, n)
        assert np.array_equal(np.isnan(rg[w]), np.isnan(want["round_gain"])), w
        fin = np.isfinite(rg[w])
        assert np.array_equal(_bits(rg[w][fin]), _bits(want["round_gain"][fin])), w
        for r in on:
            if choice[w, r] >= 0:
                assert _bits(got["marginal"][w, r:r + 1])[0] == _bits(rg[w, order[w, r], r, choice[w, r]:choice[w, r] + 1])[0]
            else:
                assert order[w, r] == -1 and got["marginal"][w, r] == 0 and got["utility"][w, r] == 0


@pytest.mark.parametrize("mode", ["slot", "best"])
@pytest.mark.parametrize("k", [1, 8, 16])
def test_prices_and_choices_are_the_rules(scene, k, mode):
    import torch
    ig, R = scene["ig"], scene["R"]
    xy, dist, _ = _candidates(scene, R, k, seed=10 + k)
    hd = _headings(xy, seed=20 + k)
    if k >= 8:  # robots that share candidates: what one takes, the other is not credited again
        xy[:, 1, :4], hd[:, 1, :4], dist[3:, 1, :4] = xy[:, 0, :4], hd[:, 0, :4], dist[3:, 0, :4]
    else:
        xy[::2, 1], hd[::2, 1] = xy[::2, 0], hd[::2, 0]
    mask = np.ones((N, R), dtype=np.uint8)
    mask[1, 0], mask[2], mask[4, R - 1] = 0, 0, 0  # world 1 and 4: a teammate under way; world 2: nobody chooses
    claim = np.zeros((N, R), dtype=np.uint8)
    claim[1, 0], claim[2, 0], claim[0, 0] = 1, 1, 1  # (world 0's robot 0 is masked: its claim byte is ignored)
    seen = _np(ig.view_gain(radius=RADIUS))["n_visible"].reshape(N, 3600).argmax(axis=1)  # per world the cell centre that sees most
    claim_xy = np.broadcast_to(np.stack([CENTRES[seen % 60], CENTRES[seen // 60]], -1)[:, None, :], (N, R, 2)).copy()
    claim_hd = np.full((N, R), np.nan)
    claim_hd[1, 0] = 0.7
    view = _np(ig.view_gain(points=xy.reshape(N, R * k, 2), radius=RADIUS))
    valid = view["valid"].reshape(N, R, k) != 0
    seeds = _device_sets(ig, claim_xy, claim_hd)
    seed_cells = np.zeros((N, 60, 60), dtype=bool)
    seed_cells[1] = seeds[1, 0]
    assert seed_cells[1].sum() > 5  # (world 4's unmasked robot has no claim byte: no seed)
    dev = scene["env"].device
    out = {"choice": torch.full((N, R), -7, dtype=torch.int32, device=dev), "order": torch.full((N, R), -7, dtype=torch.int32, device=dev),
           "marginal": torch.full((N, R), -7.0, dtype=torch.float64, device=dev), "utility": torch.full((N, R), -7.0, dtype=torch.float64, device=dev),
           "claimed": torch.full((N, 60), -7, dtype=torch.int64, device=dev), "masks": torch.full((N, R, k, 60), -7, dtype=torch.int64, device=dev),
           "round_gain": torch.full((N, R, R, k), -7.0, dtype=torch.float64, device=dev)}
    assert ig.assign_goals(xy, dist, cand_heading=hd, mask=mask, claim=claim, claim_xy=claim_xy, claim_heading=claim_hd, mode=mode,
                           radius=RADIUS, d0=D0, out=out) is out
    got = _np(out)
    on = mask != 0
    # rows of robots outside the mask, and the world nobody chooses in, keep every byte - claimed and round_gain included
    for n in ("choice", "order", "marginal", "utility", "masks"):
        assert (got[n][~on] == -7).all() and (got[n][on] != -7).all(), n
    assert (got["claimed"][2] == -7).all() and (got["round_gain"][2] == -7.0).all() and (np.delete(got["claimed"], 2, 0) != -7).all()
    assigned = got["choice"][on] >= 0
    print("R %d k %d %s: %d of %d masked robots assigned, %d priced entries" % (R, k, mode, assigned.sum(), on.sum(), np.isfinite(np.delete(got["round_gain"], 2, 0)).sum()))
    # (about half the candidates are valid: of 8 or 16 one is eligible almost surely, of a single one often none)
    assert assigned.sum() >= (on.sum() // 2 if k >= 8 else 1)
    if k == 1:
        assert not assigned.all()  # the robots with the same single candidate: the second finds nothing left
    sub = {n: (np.where((on if got[n].ndim == 2 else on[..., None, None]), got[n], 0) if n in ("choice", "order", "marginal", "utility", "masks") else got[n]) for n in got}
    sub["round_gain"], sub["claimed"] = got["round_gain"].copy(), got["claimed"].copy()
    sub["round_gain"][2], sub["claimed"][2] = np.nan, 0
    _check_against_rule(ig, sub, dist, valid, mask, seed_cells, mode, D0)
    claimed = igm.words_to_cells(_words(sub["claimed"]))
    assert (claimed[1] & seed_cells[1]).sum() == seed_cells[1].sum()  # the seed is in the final union
    # two launches: the same bytes
    again = _np(ig.assign_goals(xy, dist, cand_heading=hd, mask=mask, claim=claim, claim_xy=claim_xy, claim_heading=claim_hd, mode=mode,
                                radius=RADIUS, d0=D0, out={n: v.clone() for n, v in out.items()}))
    for n in got:
        assert np.array_equal(_bits(got[n]), _bits(again[n])), n


@pytest.mark.parametrize("mode", ["slot", "best"])
def test_eight_robots_with_sixteen_candidates_each(mode):
    """the entry's limits on synthetic candidate lists: 128 candidates per world, places all over the map, a third with a heading"""
    env = _team(2)
    _steps(env, 10, seed=5)
    ig, R, k = env._igm.ig, 8, 16
    rng = np.random.default_rng(31)
    xy = rng.uniform(-14.5, 14.5, (N, R, k, 2))
    xy[:, 4:] = xy[:, :4] + rng.uniform(-1.0, 1.0, (N, 4, k, 2))  # robots 4..7 look at nearly what robots 0..3 look at
    hd = np.where(rng.random((N, R, k)) < 0.33, rng.uniform(-math.pi, math.pi, (N, R, k)), np.nan)
    dist = rng.uniform(0.0, 20.0, (N, R, k)).astype(np.float32)
    valid = _np(ig.view_gain(points=xy.reshape(N, R * k, 2), radius=RADIUS))["valid"].reshape(N, R, k) != 0
    assert valid.mean() > 0.4 and not valid.all()
    got = _np(ig.assign_goals(xy, dist, cand_heading=hd, mode=mode, radius=RADIUS, d0=D0))
    assert got["round_gain"].shape == (N, R, R, k) and (got["choice"] >= 0).mean() >= 0.9
    _check_against_rule(ig, got, dist, valid, np.ones((N, R), dtype=np.uint8), np.zeros((N, 60, 60), dtype=bool), mode, D0)
    if mode == "best":  # submodular: what a candidate is worth never grows from one round to the next
        g = got["round_gain"]
        both = np.isfinite(g[:, 1:]) & np.isfinite(g[:, :-1])
        assert (g[:, 1:][both] <= g[:, :-1][both]).all() and (g[:, 1:][both] < g[:, :-1][both]).any()
    env.close()


# ---- 4. claims and masks, through the env ------------------------------------------------------------------------------------------------
def test_teammates_under_way_keep_their_cells():
    import torch
    R = 3
    env = _team(R)
    _steps(env, 10, seed=5)
    ig = env._igm.ig
    prop = env.ig_propose_goals(k=8, min_sep=2.0, d0=D0)
    # robot 2 is under way to ITS best proposal; robots 0 and 1 get robot 2's proposals as their first four: they overlap its claim
    env.ig_set_goals(prop["xy"][:, :, 0])
    prop["xy"][:, :2, :4] = prop["xy"][:, 2:3, :4]
    goals = _np(env.ig_goals())
    # what the seed was chosen for: worlds whose three robots have their eight proposals each (world 3 is the one nobody chooses in)
    ws = [w for w in (0, 1, 2, 4, 5) if (prop["n_found"][w] == 8).all() and goals["active"][w, 2]]
    assert len(ws) >= 3, ws
    mask = np.ones((N, R), dtype=np.uint8)
    mask[:, 2], mask[3] = 0, 0
    for n, v in env.ig_assign_goals(mask=mask, set_goals=False).items():
        if n not in ("xy", "heading"):
            v.fill_(-7)  # the env's buffers, poisoned: the next call writes the masked robots' rows alone
    a = _np(env.ig_assign_goals(mode="best", mask=mask, set_goals=False))
    on = mask != 0
    for n in ("choice", "order", "marginal", "utility", "masks"):
        assert (a[n][~on] == -7).all() and (a[n][on] != -7).all(), n
    assert (a["claimed"][3] == -7).all() and (a["round_gain"][3] == -7.0).all() and np.isnan(a["xy"][~on]).all()
    seed = _device_sets(ig, goals["goal_xy"], np.full((N, R), np.nan))[:, 2]
    claimed, cells = igm.words_to_cells(_words(np.where(a["claimed"] == -7, 0, a["claimed"]))), igm.words_to_cells(_words(np.where(a["masks"] == -7, 0, a["masks"])))
    world = np.arange(N, dtype=np.int32)
    for w in ws:
        assert seed[w].sum() > 20 and (claimed[w] & seed[w]).sum() == seed[w].sum()  # the teammate's set is in claimed ...
        first = int(np.flatnonzero(a["order"][w] == 0)[0])
        new = cells[w, first, a["choice"][w, first]] & ~seed[w]
        got = ig.mi_reward(igm.cells_to_words(new).view(np.int64), [w]).cpu().numpy()
        assert _bits(got)[0] == _bits(a["marginal"][w, first:first + 1])[0]  # ... and nobody is credited its cells
        assert np.isnan(a["round_gain"][w, :, 2]).all() and np.isfinite(a["round_gain"][w, 0, :2]).all()
    assert all((cells[w, :2, :4] & seed[w]).any() for w in ws)
    # the same call without the claims prices those cells
    b = _np(env.ig_assign_goals(mode="best", mask=mask, claim_active=False, set_goals=False))
    full = ig.mi_reward(a["masks"][on].reshape(-1, 60), np.repeat(world, on.sum(axis=1) * 8)).cpu().numpy().reshape(-1, 8)
    with_claims, without = a["round_gain"][:, 0][on], b["round_gain"][:, 0][on]
    fin = np.isfinite(without)
    assert np.array_equal(fin, np.isfinite(with_claims)) and fin.sum() >= len(ws) * 16
    assert np.array_equal(_bits(without[fin]), _bits(full[fin]))
    assert (without[fin] >= with_claims[fin]).all() and (without[fin] > with_claims[fin]).any()
    # a masked robot's own active goal is no seed: with every robot masked by an explicit mask the claims change nothing
    ones = np.ones((N, R), dtype=np.uint8)
    c = _np(env.ig_assign_goals(mode="slot", mask=ones, set_goals=False))
    d = _np(env.ig_assign_goals(mode="slot", mask=ones, claim_active=False, set_goals=False))
    e = _np(env.ig_assign_goals(mode="slot", set_goals=False))
    for n in c:
        assert np.array_equal(_bits(c[n]), _bits(d[n])) and np.array_equal(_bits(c[n]), _bits(e[n])), n
    union = np.zeros((N, 60, 60), dtype=bool)
    cc = igm.words_to_cells(_words(c["masks"]))
    for w in range(N):
        for r in range(R):
            if c["choice"][w, r] >= 0:
                union[w] |= cc[w, r, c["choice"][w, r]]
    assert np.array_equal(igm.words_to_cells(_words(c["claimed"])), union)
    env.close()


# ---- 5. the env ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("headings", [None, 8])
def test_the_env_sends_the_team_to_what_it_assigned(headings):
    import torch
    R = 2
    env = _team(R)
    _steps(env, 10, seed=5)
    with pytest.raises(RuntimeError, match="needs an earlier ig_propose_goals"):
        env.ig_assign_goals()
    prop = env.ig_propose_goals(k=8, min_sep=2.0, d0=0.5, headings=headings)
    prop["xy"][2, 1] = float("nan")  # a robot whose proposals are gone: nothing is left for it to see
    mask = np.array([[1, 1], [1, 0], [1, 1], [0, 1], [1, 1], [0, 0]], dtype=np.uint8)
    env.ig_set_goals(np.zeros((N, R, 2)) + 100.0)  # nobody has an active goal (outside the map)
    before = _np(env.ig_goals())
    assert not before["active"].any()
    a = _np(env.ig_assign_goals(mode="best", mask=mask))
    assert sorted(a) == ["choice", "claimed", "heading", "marginal", "masks", "order", "round_gain", "utility", "xy"]
    on = mask != 0
    assert a["choice"][2, 1] == -1 and a["order"][2, 1] == -1 and (a["choice"][on] >= 0).sum() >= 5  # (of the 7 other masked robots)
    pxy, idx = prop["xy"].cpu().numpy(), np.clip(a["choice"], 0, None)
    took = on & (a["choice"] >= 0)
    want_xy = np.take_along_axis(pxy, idx[:, :, None, None].repeat(2, -1), 2)[:, :, 0]
    assert np.array_equal(_bits(a["xy"][took]), _bits(want_xy[took])) and np.isnan(a["xy"][~took]).all()
    g = _np(env.ig_goals())
    assert np.array_equal(g["active"][on], took[on].astype(np.uint8)) and g["active"][2, 1] == 0 and not g["active"][~on].any()
    assert np.array_equal(_bits(g["goal_xy"][took]), _bits(a["xy"][took]))
    if headings is None:
        assert np.isnan(a["heading"]).all() and "goal_heading" not in g
        util = a["marginal"][took] / (np.take_along_axis(prop["distance"].cpu().numpy().astype(np.float64), idx[:, :, None], 2)[:, :, 0][took] + 0.5)
        assert np.array_equal(_bits(a["utility"][took]), _bits(util))  # d0 is the proposal call's
    else:
        ph = np.take_along_axis(prop["heading"].cpu().numpy(), idx[:, :, None], 2)[:, :, 0]
        assert np.isfinite(a["heading"][took]).all() and np.array_equal(_bits(a["heading"][took]), _bits(ph[took])) and np.isnan(a["heading"][~took]).all()
        assert np.array_equal(_bits(g["goal_heading"][took]), _bits(a["heading"][took]))
        # the cones are what was claimed: every chosen mask is visible_cells of the chosen pose
        poses = np.concatenate([a["xy"][took], a["heading"][took][:, None]], axis=1)
        cone = _words(env._igm.ig.visible_cells(poses, np.nonzero(took)[0].astype(np.int32)))
        chosen = np.take_along_axis(_words(a["masks"]), idx[:, :, None, None].repeat(60, -1).astype(np.int64), 2)[:, :, 0]
        assert np.array_equal(chosen[took], cone)
    # the robots drive to what they were assigned
    caller = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)
    d_before = env.ig_goals()["goal_distance"].clone()
    for _ in range(20):
        _, _, _, info = env.step(caller)
    moved = ((info["goal_distance"] < d_before) | (info["goal_reached"] != 0))[torch.as_tensor(took, device=env.device)]
    assert moved.any()
    env.close()


def test_a_twin_that_never_assigns_steps_and_proposes_the_same_bits():
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
                env.ig_assign_goals(mode="best" if t % 2 else "slot", set_goals=False)
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


def test_after_an_auto_reset_the_assignment_is_on_the_new_slots_field():
    """Streamed worlds with a short time limit (pref_speed 30): once every world has restarted, the assignment of a world that runs
    on a fresh slot is the specification's on THAT slot's field - proposals are cell centres and the range is 5.0, where the host's
    and the device's range test agree exactly - and not the one on the field it left."""
    R = 2
    env = _team(R, seed=3, stream=True, pref=30.0)
    first = env._igm.ig.edf()[:N].cpu().numpy()
    restarted = _steps(env, 48, seed=8, auto_reset=True)
    pos, edf, mi, slots = _state(env)
    print("restarted worlds: %s, slots now %s" % (np.flatnonzero(restarted).tolist(), slots.tolist()))
    assert restarted.all()
    fresh = [w for w in range(N) if not np.array_equal(edf[w], first[w])]
    assert fresh
    w = fresh[0]
    prop = env.ig_propose_goals(k=8)
    a = _np(env.ig_assign_goals(mode="best", set_goals=False))
    pxy, dist = prop["xy"].cpu().numpy(), prop["distance"].cpu().numpy()
    ig = env._igm.ig
    want = np.zeros((R, 8, 60, 60), dtype=bool)
    old = np.zeros((R, 8, 60, 60), dtype=bool)
    valid = np.zeros((R, 8), dtype=bool)
    for r in range(R):
        for c in range(8):
            _, _, valid[r, c], want[r, c], _ = igm.view_gain_spec(edf[w], mi[w], pxy[w, r, c], RADIUS, 5.0)
            old[r, c] = igm.view_gain_spec(first[w], mi[w], pxy[w, r, c], RADIUS, 5.0)[3]
    assert valid.sum() >= 8 and not np.array_equal(want, old)
    assert np.array_equal(igm.words_to_cells(_words(a["masks"]))[w], want)
    spec = igm.assign_goals_spec(want, np.zeros((60, 60), bool), dist[w], valid, _reward_of(ig, w), "best", 1.0, [0, 1])
    assert np.array_equal(a["choice"][w], spec["choice"]) and np.array_equal(a["order"][w], spec["order"])
    assert np.array_equal(igm.words_to_cells(_words(a["claimed"]))[w], spec["claimed"])
    assert np.array_equal(_bits(a["utility"][w]), _bits(spec["utility"])) and np.array_equal(_bits(a["marginal"][w]), _bits(spec["marginal"]))
    env.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def _P(**kw):
    p = dict(n_robots=2, k=4, mode=1, flags=0, radius=RADIUS, range=5.0, d0=1.0, fov=math.pi / 3)
    p.update(kw)
    return _lib.IgAssignParams(*[p[f[0]] for f in _lib.IgAssignParams._fields_])


def test_the_entry_refuses_and_touches_nothing():
    import torch
    R, k = 2, 4
    env = _B()(N, M, max_obstacles=K, game_over_mode="agent0")
    assert env.generate_exploration_worlds(kinds="train_stage_2", seed=SEED, n_robots=R, n_targets=M - R, n_obst=(6, 16), target_radius=0.2,
                                           robot_pref_speed=0.2) == 0
    env.reset()
    dev = env.device
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)
    t = dict(choice=full((N, R), -7, torch.int32), order=full((N, R), -7, torch.int32), marginal=full((N, R), -7.0, torch.float64),
             utility=full((N, R), -7.0, torch.float64), claimed=full((N, 60), -7, torch.int64), masks=full((N, R, k, 60), -7, torch.int64),
             round_gain=full((N, R, R, k), -7.0, torch.float64))
    xy = torch.zeros((N, R, k, 2), dtype=torch.float64, device=dev)
    dist = torch.ones((N, R, k), dtype=torch.float32, device=dev)
    claim = torch.ones((N, R), dtype=torch.uint8, device=dev)
    L, h, s, p = env.L, env.h, env._stream, _lib.ptr

    def call(P, claim=None, claim_xy=None, **kw):
        a = dict(t, cand_xy=xy, cand_distance=dist)
        a.update(kw)
        return L.cagym_ig_assign_goals(h, None if P is None else C.byref(P), None, p(a["cand_xy"]), None, p(a["cand_distance"]), p(claim),
                                       p(claim_xy), None, p(a["choice"]), p(a["order"]), p(a["marginal"]), p(a["utility"]), p(a["claimed"]),
                                       p(a["masks"]), p(a["round_gain"]), s())

    assert call(_P()) == E_STATE and b"cagym_ig_assign_goals before cagym_ig_init" in L.cagym_last_error(h)
    ig = igm.InfoGain(env)  # (cagym_ig_init)
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_robots=0), dict(n_robots=9), dict(n_robots=-1), dict(k=0), dict(k=17), dict(k=-3), dict(mode=2), dict(mode=-1), dict(flags=1)]
    for f in ("radius", "range", "d0", "fov"):
        bad += [{f: 0.0}, {f: -1.0}, {f: nan}, {f: inf}]
    for kw in bad:
        assert call(_P(**kw)) == E_INVALID and b"cagym_ig_assign_goals" in L.cagym_last_error(h), kw
    assert call(None) == E_INVALID
    for missing in ("cand_xy", "cand_distance", "choice", "order", "marginal", "utility", "claimed", "masks"):
        assert call(_P(), **{missing: None}) == E_INVALID, missing
    assert call(_P(), claim=claim) == E_INVALID and b"claim needs claim_xy" in L.cagym_last_error(h)
    torch.cuda.synchronize()
    for n, v in t.items():
        assert (v == -7).all(), n  # nothing was launched
    assert call(_P(), round_gain=None) == 0  # round_gain is optional
    torch.cuda.synchronize()
    assert (t["round_gain"] == -7.0).all() and (t["choice"] != -7).all() and (t["masks"] != -7).all() and (t["claimed"] != -7).all()
    assert call(_P(), claim=claim, claim_xy=xy) == 0
    torch.cuda.synchronize()
    assert (t["round_gain"] != -7.0).all()
    with pytest.raises(ValueError, match="mode must be"):
        ig.assign_goals(xy, dist, mode="greedy")
    with pytest.raises(ValueError, match="must be \\[N, R, k\\]"):
        ig.assign_goals(xy, dist[0])
    with pytest.raises(ValueError, match="claim needs claim_xy"):
        ig.assign_goals(xy, dist, claim=claim)
    env.close()


def test_the_env_refuses_out_of_order_calls():
    env = _B()(N, M, max_obstacles=K, game_over_mode="agent0")
    assert env.generate_exploration_worlds(kinds="train_stage_2", seed=SEED, n_robots=2, n_targets=3, n_obst=(6, 16), target_radius=0.2,
                                           robot_pref_speed=0.2) == 0
    env.reset()
    env.attach_ig_learner()
    with pytest.raises(RuntimeError, match="needs attach_ig_goals"):
        env.ig_assign_goals()
    env.attach_ig_goals()
    env.reset()
    with pytest.raises(RuntimeError, match="needs an earlier ig_propose_goals"):
        env.ig_assign_goals()
    assert env._goals.assign is None  # a refused call allocated nothing
    env.ig_propose_goals(k=4)
    with pytest.raises(ValueError, match="mode must be"):
        env.ig_assign_goals(mode="greedy")
    with pytest.raises(ValueError, match="d0 must be finite and positive"):
        env.ig_assign_goals(d0=0.0)
    assert env._goals.assign is None
    assert sorted(env.step()[3]) == ["belief_window", "flags", "gain", "goal_distance", "goal_reached", "observed"]  # step() gains nothing
    env.close()
