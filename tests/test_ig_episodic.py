"""Dec-MCTS robots under auto-reset: attach_ig_mcts(episodic=True), cagym_ig_episode_boundary and the per-world accumulators.

The restart scenario: game_over_mode "agent0" with agent 0 a robot whose goal lies 1.25 + 0.1 (s % 8) m BEHIND it (pref_speed 3:
a time limit of 0.5 .. 1.2 s, 5 to 13 steps, and no way to turn round in that time), so every world's episodes end at its own
time; a pool of S = 2 N scenarios whose second half stands among other rectangles.  Every test that leans on restarts asserts from
the device's game_over history that they happened as intended (_preconditions)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_dmcts import OBST, OracleBackend, _ig_world

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
igm = importlib.import_module("gym-exploration-2d_amd.ig")
dm = importlib.import_module("gym-exploration-2d_amd.dmcts")
vec = importlib.import_module("gym-exploration-2d_amd.vecenv")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBST2 = [(3, 3, 10, 10), (-10, 3, -3, 10), (3, -10, 10, -3), (-10, -10, -3, -3)]  # the pool's second half
SLOTS = [0, 4, 7]
N, M, K, T = 8, 10, 9, 32
BUDGET = dict(Ntree=5, Nsims=3, Ncycles=2)
KW = dict(radius=0.5, horizon=4, c_p=1.0, gamma=0.95)


def _B():
    return importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def _env(same_limit=False, n=N):
    S = 2 * n
    a6 = np.zeros((S, M, 6))
    a6[..., 4], a6[..., 5], a6[..., 0] = 1.0, 0.1, 1e3 + np.arange(M)
    pol = np.full((S, M), scen.POLICY_STATIC, dtype=np.int32)
    tgt = [[6, 12, 0, 0, 1, .2], [-6, -12, 0, 0, 1, .2], [1.5, 2.5, 0, 0, 1, .2], [12, -6, 0, 0, 1, .2], [-12, 6, 0, 0, 1, .2]]
    for s in range(S):
        d = 1.25 if same_limit else 1.25 + 0.1 * (s % 8)
        a6[s, 0] = [-5, 0, -5 - d, 0, 3.0, .5]
        a6[s, 4] = [0, 0, 16, 0, 1, .5]
        a6[s, 7] = [5, 0, 16, 0, 1, .5]
        for slot, r in zip([q for q in range(8) if q not in SLOTS], tgt):
            a6[s, slot] = r
    pol[:, SLOTS] = scen.POLICY_IGMCTS
    obst = np.array([OBST] * n + [OBST2] * n, dtype=np.float64)
    env = _B()(n, M, n_scenarios=S, max_obstacles=4, game_over_mode="agent0")
    env.set_scenarios(a6, pol, scen.DYN_FIRSTORDER, heading0=np.zeros((S, M)), n_agents=[8] * S, obstacles=obst, n_obst=[4] * S)
    env.reset()
    return env


def _attach(env, parallel=False, seed=3, episodic=True, **kw):
    b = dict(BUDGET)
    b.update(kw)
    return env.attach_ig_mcts(detect_fov=60.0, detect_range=5.0, xdt=5, mcts_cp=1.0, mcts_horizon=4, mcts_gamma=0.95,
                              parallelize_agents=parallel, radius=0.5, seed=seed, episodic=episodic, **b)


def _front(b, ig, world):
    """The explicit front end of test_ig_mcts_internal_step_equals_explicit_composition: poses, detections, belief update, reward."""
    import torch
    slots = torch.tensor(SLOTS, device=b.device)
    st = b.state()
    poses = torch.stack([st["pos_x"][:, slots], st["pos_y"][:, slots], st["heading"][:, slots]], dim=2)
    mask, off = igm.find_targets_in_obs(b.obs_oas[:, slots], 5.0)
    order = torch.argsort((~mask).to(torch.int8), dim=2, stable=True)
    det = torch.gather(off.double() + poses[:, :, None, :2], 2, order[..., None].expand(b.N, 3, K, 2)).contiguous()
    nd = mask.sum(dim=2).to(torch.int32)
    observed = ig.update_belief(poses, det, nd)
    return poses, ig.mi_reward(observed, world)


def _preconditions(go_hist, episode, n=N):
    """go_hist [T, N] game_over of every step; episode [N] the worlds' episode counters at the end."""
    go = np.asarray(go_hist).astype(bool)
    assert (go.sum(axis=0) >= 2).all(), go.sum(axis=0)               # every world restarted at least twice
    assert len(np.nonzero(go.any(axis=1))[0]) >= 3                   # on at least 3 distinct step indices
    # world w stands on scenario (w + restarts * n) % 2n: after an odd number of restarts on the second half of the pool
    assert (np.cumsum(go, axis=0)[:-1] % 2 == 1).any()               # ... and at least one world took steps there
    assert (np.asarray(episode) == go.sum(axis=0)).all()


def _same(a, b, what):
    import torch
    for k, x, y in (("oas", a.obs_oas, b.obs_oas), ("ego", a.obs_ego, b.obs_ego), ("reward", a.reward, b.reward),
                    ("flags", a.flags, b.flags), ("game_over", a.game_over, b.game_over)):
        assert torch.equal(x, y), (what, k)


# ---- CPU: the specification the GPU tests lean on (passes on the parent commit too) ----------------------------------------
def test_host_planner_reset_of_one_world_changes_that_world_alone():
    """DecMCTSPlanner.reset(worlds=[w]) with the CPU-oracle backend: world w's next planning step no longer hears the previous
    plans (its trees' statistics change), every other world's is identical to an undisturbed run.  Passes on the parent commit:
    it pins the host specification, not the new device code."""
    from oracle import oracle as orc
    orc.build()
    edf = _ig_world()
    n = 3
    p0 = np.array([[[-5, 0, 0], [0, 0, 0], [5, 0, 0]], [[-6, 0.5, 0.3], [0.5, -5, 1.6], [0, 6, -1.5]],
                   [[-12, 0, 0], [12, 1, 3.0], [0, -12, 1.5]]], dtype=np.float64)
    p1 = p0 + np.array([0.2, 0.0, 0.0])

    def run(reset_world):
        pl = dm.DecMCTSPlanner(OracleBackend([edf] * n, [np.ones((60, 60))] * n), n, 3, seed=11, Ntree=6, Nsims=4, Ncycles=2, **KW)
        pl.plan(p0)
        if reset_world is not None:
            pl.reset(worlds=[reset_world])
        acts, paths = pl.plan(p1)
        stats = np.array([[(pl.trees[r][w].root.mu, pl.trees[r][w].root.N, len(pl.trees[r][w].nodes)) for r in range(3)] for w in range(n)])
        return acts, paths, stats

    a0, q0, s0 = run(None)
    a1, q1, s1 = run(1)
    for w in (0, 2):
        assert np.array_equal(a0[w], a1[w]) and q0[w] == q1[w] and np.array_equal(s0[w], s1[w]), w
    assert q0[1] != q1[1] or not np.array_equal(s0[1], s1[1])


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("parallel", [False, True])
def test_episodic_step_equals_the_host_specification_world_by_world(parallel):
    """1. Env A (episodic attach, auto-reset) against the explicit composition over the HOST planner, restarted per world with
    reset_belief(game_over) and DecMCTSPlanner.reset(worlds=...): bit-equal every step, accumulators included."""
    import torch
    a, b = _env(), _env()
    _attach(a, parallel)
    ig = igm.InfoGain(b)
    host = dm.DecMCTSPlanner(igm.InfoGainBackend(ig), N, 3, seed=3, parallelize_agents=parallel, **BUDGET, **KW)
    world = torch.arange(N, dtype=torch.int32, device=b.device)
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=b.device)
    run, tot, last, eps = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32)
    hist = []
    for t in range(T):
        a.step(None, auto_reset=True)
        poses, reward = _front(b, ig, world)
        actions, _ = host.plan(poses.cpu().numpy())
        actions = torch.as_tensor(actions, device=b.device)
        ext[:, SLOTS] = actions.float()
        b.step(ext, auto_reset=True)
        ig.reset_belief(b.game_over)
        torch.cuda.synchronize()
        go = b.game_over.cpu().numpy().astype(bool)
        host.reset(worlds=np.nonzero(go)[0])
        hist.append(go)
        assert torch.equal(a._igm.planner.actions, actions), t
        assert torch.equal(a.team_reward, reward), t
        assert torch.equal(a._igm.ig.belief, ig.belief), t
        assert torch.equal(a.state()["action"], b.state()["action"]), t
        _same(a, b, t)
        rw = reward.cpu().numpy()
        for w in range(N):  # the host loop the accumulators restate: fp64 sums in step order
            run[w] += rw[w]
            if go[w]:
                tot[w] += run[w]
                last[w] = run[w]
                eps[w] += 1
                run[w] = 0.0
        st = {k: v.cpu().numpy() for k, v in a.ig_episode_stats().items()}
        assert np.array_equal(st["running"], run) and np.array_equal(st["sum"], tot) and np.array_equal(st["last"], last), t
        assert np.array_equal(st["episodes"], eps), t
    _preconditions(hist, a.state()["episode"].cpu().numpy())
    assert (tot > 0).all()
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("parallel", [False, True])
def test_all_worlds_restart_equals_reset_advance_episode(parallel):
    """2. One time limit everywhere: all worlds restart on the same step.  A: episodic + auto-reset.  B: the default attach
    stepped with step(None) and reset(advance_episode=True) when every world is over - the public path that existed before."""
    import torch
    a, b = _env(same_limit=True), _env(same_limit=True)
    _attach(a, parallel)
    _attach(b, parallel, episodic=False)
    restarts = 0
    for t in range(20):
        a.step(None, auto_reset=True)
        b.step(None)
        torch.cuda.synchronize()
        go = b.game_over.cpu().numpy().astype(bool)
        assert go.all() or not go.any(), (t, go)
        assert torch.equal(a.game_over, b.game_over), t
        assert torch.equal(a.team_reward, b.team_reward), t
        assert torch.equal(a._igm.planner.actions, b._igm.planner.actions), t
        assert torch.equal(a.reward, b.reward) and torch.equal(a.flags, b.flags), t
        if go.all():
            b.reset(advance_episode=True)
            restarts += 1
            torch.cuda.synchronize()
        assert torch.equal(a.obs_oas, b.obs_oas) and torch.equal(a.obs_ego, b.obs_ego), t
        assert torch.equal(a._igm.ig.belief, b._igm.ig.belief), t
        assert torch.equal(a.state()["episode"], b.state()["episode"]), t
    assert restarts >= 2  # episode 1 ran on the second-half scenarios (w + N), episode 2 on the first half again
    assert (a.ig_episode_stats()["episodes"].cpu().numpy() == restarts).all()
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("parallel", [False, True])
def test_a_world_is_not_disturbed_by_other_worlds_restarts(parallel):
    """3a. C: same pool and seed, default attach, no auto-reset.  Every world of A equals C up to and including its first terminal
    step, while other worlds of A have already restarted."""
    import torch
    a, c = _env(), _env()
    pa, pc = _attach(a, parallel), _attach(c, parallel, episodic=False)
    done = np.zeros(N, dtype=bool)
    hist = []
    overlap = 0
    for t in range(T):
        a.step(None, auto_reset=True)
        c.step(None)
        torch.cuda.synchronize()
        go = a.game_over.cpu().numpy().astype(bool)
        live = torch.as_tensor(~done, device=a.device)  # worlds still in their first episode when this step began
        overlap += int(done.any() and (~done).any())
        for x, y, k in ((pa.actions, pc.actions, "plan"), (pa.paths, pc.paths, "paths"), (a.team_reward, c.team_reward, "team_reward"),
                        (a.reward, c.reward, "reward"), (a.flags, c.flags, "flags"), (a.game_over, c.game_over, "game_over")):
            assert torch.equal(x[live], y[live]), (t, k)
        done |= go
        still = torch.as_tensor(~done, device=a.device)  # (a restarted world's observation, action and belief are the new episode's)
        assert torch.equal(a.obs_oas[still], c.obs_oas[still]) and torch.equal(a._igm.ig.belief[still], c._igm.ig.belief[still]), t
        assert torch.equal(a.state()["action"][still], c.state()["action"][still]), t
        hist.append(go)
    _preconditions(hist, a.state()["episode"].cpu().numpy())
    assert overlap >= 3  # steps on which first-episode worlds ran beside restarted ones
    a.close()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ncycles", [2, 3])
def test_first_plan_after_a_restart_equals_a_fresh_handle(ncycles):
    """3b. Agent-parallel mode, even and odd Ncycles (the first cycle reads the first publication buffer or its copy): the first
    plan of a restarted world equals the plan of a fresh handle with reset_comms set and the same call_base."""
    import torch
    a = _env()
    pa = _attach(a, True, Ncycles=ncycles)
    for t in range(T):
        a.step(None, auto_reset=True)
        torch.cuda.synchronize()
        if a.game_over.any() and t >= 6:
            break
    restarted = a.game_over.bool().clone()
    assert restarted.any() and not restarted.all()
    calls = pa.calls
    a.step(None, auto_reset=True)
    torch.cuda.synchronize()
    g = a._igm
    episode = a.state()["episode"].cpu().numpy()
    f = _env()
    for k in range(int(episode.max())):  # the fresh handle's worlds onto the scenarios A's worlds stand on
        f.reset(world_mask=(episode > k).astype(np.uint8), advance_episode=True)
    ig = igm.InfoGain(f)
    ig.update_belief(g.poses, g.det, g.n_det)
    pf = dm.DeviceDecMCTSPlanner(ig, 3, seed=3, parallelize_agents=True, Ntree=BUDGET["Ntree"], Nsims=BUDGET["Nsims"], Ncycles=ncycles, **KW)
    assert pf.P.reset_comms == 1
    pf.calls = calls
    pf.plan(g.poses)
    torch.cuda.synchronize()
    assert torch.equal(ig.belief[restarted], g.ig.belief[restarted])
    for x, y in ((pf.actions, pa.actions), (pf.paths, pa.paths), (pf.stats, pa.stats)):
        assert torch.equal(x[restarted], y[restarted])
    # (the other worlds heard their previous plans: the comparison above is not vacuous)
    assert not torch.equal(pf.stats[~restarted], pa.stats[~restarted])
    a.close()
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("start_parallel", [False, True])
def test_mode_switch_on_the_step_after_a_restart(start_parallel):
    """4. sequential <-> agent-parallel on every step that follows a restart: still the host planner's decisions."""
    import torch
    a, b = _env(), _env()
    pa = _attach(a, start_parallel)
    ig = igm.InfoGain(b)
    host = dm.DecMCTSPlanner(igm.InfoGainBackend(ig), N, 3, seed=3, parallelize_agents=start_parallel, **BUDGET, **KW)
    world = torch.arange(N, dtype=torch.int32, device=b.device)
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=b.device)
    hist, switches = [], 0
    for t in range(T):
        a.step(None, auto_reset=True)
        poses, reward = _front(b, ig, world)
        actions, _ = host.plan(poses.cpu().numpy())
        actions = torch.as_tensor(actions, device=b.device)
        ext[:, SLOTS] = actions.float()
        b.step(ext, auto_reset=True)
        ig.reset_belief(b.game_over)
        torch.cuda.synchronize()
        go = b.game_over.cpu().numpy().astype(bool)
        host.reset(worlds=np.nonzero(go)[0])
        hist.append(go)
        assert torch.equal(pa.actions, actions), t
        assert torch.equal(a.team_reward, reward) and torch.equal(a._igm.ig.belief, ig.belief), t
        assert torch.equal(a.game_over, b.game_over), t
        if go.any():
            host.parallelize_agents = not host.parallelize_agents
            pa.parallelize_agents = host.parallelize_agents
            switches += 1
    _preconditions(hist, a.state()["episode"].cpu().numpy())
    assert switches >= 3
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("parallel", [False, True])
def test_rollout_equals_steps(parallel):
    """5. rollout(T, auto_reset=True) == T step(auto_reset=True), every slice, team_reward included."""
    import torch
    a, b = _env(), _env()
    _attach(a, parallel)
    _attach(b, parallel)
    want = a.alloc_rollout(T)
    assert want["team_reward"].shape == (T, N) and want["team_reward"].dtype == torch.float64
    pairs = (("other_agents_states", "obs_oas"), ("ego", "obs_ego"), ("reward", "reward"), ("flags", "flags"), ("game_over", "game_over"),
             ("team_reward", "team_reward"))
    for t in range(T):
        a.step(None, auto_reset=True)
        for k, attr in pairs:
            want[k][t].copy_(getattr(a, attr))
    got = b.rollout(T, auto_reset=True)
    torch.cuda.synchronize()
    for k, _ in pairs:
        assert torch.equal(got[k], want[k]), k
    for k, v in a.ig_episode_stats().items():
        assert torch.equal(v, b.ig_episode_stats()[k]), k
    assert torch.equal(a._igm.ig.belief, b._igm.ig.belief)
    _preconditions(got["game_over"].cpu().numpy(), b.state()["episode"].cpu().numpy())
    # the env's own observation table holds the last step's rows: a step() behind the rollout continues it
    a.step(None, auto_reset=True)
    b.step(None, auto_reset=True)
    torch.cuda.synchronize()
    assert torch.equal(a.team_reward, b.team_reward) and torch.equal(a._igm.planner.actions, b._igm.planner.actions)
    _same(a, b, "step behind the rollout")
    # ... and so does a rollout without observation slices (the robots' detector still sees every step's table)
    more = b.rollout(4, auto_reset=True, out=b.alloc_rollout(4, obs=False))
    for t in range(4):
        a.step(None, auto_reset=True)
        torch.cuda.synchronize()
        assert torch.equal(more["team_reward"][t], a.team_reward) and torch.equal(more["reward"][t], a.reward), t
    torch.cuda.synchronize()
    assert torch.equal(a.obs_oas, b.obs_oas) and torch.equal(a._igm.ig.belief, b._igm.ig.belief)
    # without auto-reset the chain still accumulates the running return
    c = _env()
    _attach(c, parallel)
    out = c.rollout(3, auto_reset=False)
    torch.cuda.synchronize()
    assert torch.equal(c.ig_episode_stats()["running"], out["team_reward"][0] + out["team_reward"][1] + out["team_reward"][2])
    assert int(c.ig_episode_stats()["episodes"].sum()) == 0
    for e in (a, b, c):
        e.close()


@pytest.mark.gpu
def test_vecenv_steps_across_restarts_and_returns_team_reward():
    """6. CagymVecEnv.step (always auto-reset) over an episodic attach."""
    import torch
    a = _env()
    _attach(a)
    v = vec.CagymVecEnv(a, ["dist_to_goal", "other_agents_states"], single_agent=True)
    obs = v.reset()
    dones_total = torch.zeros(N, dtype=torch.int64, device=a.device)
    ret = torch.zeros(N, dtype=torch.float64, device=a.device)
    hist = []
    for t in range(T):
        obs, rews, dones, infos = v.step([None])
        assert obs.shape == (N, v.flat.size) and rews.shape == (N,) and dones.dtype == torch.bool
        assert infos["team_reward"].dtype == torch.float64 and infos["team_reward"].shape == (N,)
        assert torch.equal(infos["team_reward"], a.team_reward)
        ret += infos["team_reward"]
        dones_total += dones
        hist.append(dones.cpu().numpy())
    st = a.ig_episode_stats()
    _preconditions(hist, a.state()["episode"].cpu().numpy())
    assert torch.equal(st["episodes"].long(), dones_total)
    assert torch.allclose(st["sum"] + st["running"], ret, rtol=1e-12, atol=0)  # (another summation order: not bitwise)
    # nothing changes without ig attached
    e = _env()
    _, _, _, infos = vec.CagymVecEnv(e, ["dist_to_goal"]).step([None])
    assert sorted(infos) == ["flags"]
    e.close()
    v.close()


@pytest.mark.gpu
def test_manual_reset_of_some_worlds():
    """7. reset(world_mask=m) with an episodic attach restarts the masked worlds alone: the unmasked worlds plan as in a run
    without that reset, and no episode is counted."""
    import torch
    a, b = _env(), _env()
    pa, pb = _attach(a), _attach(b)
    for t in range(3):
        a.step(None)
        b.step(None)
    m = torch.zeros(N, dtype=torch.uint8, device=a.device)
    m[[1, 3]] = 1
    keep = ~m.bool()
    a.reset(world_mask=m)
    torch.cuda.synchronize()
    st = a.ig_episode_stats()
    assert (a._igm.ig.belief[m.bool()] == 1.0).all()
    assert torch.equal(a._igm.ig.belief[keep], b._igm.ig.belief[keep])
    assert (st["running"][m.bool()] == 0).all() and torch.equal(st["running"][keep], b.ig_episode_stats()["running"][keep])
    assert (st["running"][keep] > 0).all()
    assert int(st["episodes"].sum()) == 0 and float(st["sum"].sum()) == 0.0 and float(st["last"].sum()) == 0.0
    for t in range(2):
        a.step(None)
        b.step(None)
        torch.cuda.synchronize()
        for x, y in ((pa.actions, pb.actions), (pa.paths, pb.paths), (pa.stats, pb.stats), (a.team_reward, b.team_reward)):
            assert torch.equal(x[keep], y[keep]), t
        assert not torch.equal(pa.stats[m.bool()], pb.stats[m.bool()])
    assert int(a.ig_episode_stats()["episodes"].sum()) == 0
    # the planner's own per-world reset forgets plans only: beliefs and accumulators stay
    before = {k: v.clone() for k, v in a.ig_episode_stats().items()}
    bel = a._igm.ig.belief.clone()
    pa.reset(world_mask=m)
    torch.cuda.synchronize()
    assert torch.equal(a._igm.ig.belief, bel)
    for k, v in a.ig_episode_stats().items():
        assert torch.equal(v, before[k]), k
    # reset() with no mask: everything restarts, every running return is zeroed
    a.reset()
    torch.cuda.synchronize()
    assert (a.ig_episode_stats()["running"] == 0).all() and (a._igm.ig.belief == 1.0).all()
    a.close()
    b.close()


@pytest.mark.gpu
def test_episodic_refusals_and_abi_checks():
    """8. The split step stays refused, rollout() refuses a capturing stream; the C entry's argument checks."""
    import ctypes
    import torch
    a = _env()
    pa = _attach(a)
    for call in (lambda: a.step_begin(), lambda: a.step_finish(None), lambda: a.step_overlapped(lambda x: None, None)):
        with pytest.raises(RuntimeError, match="split step"):
            call()
    x = torch.zeros(4, device=a.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.add_(1)
        with pytest.raises(RuntimeError, match="captured"):
            a.rollout(2)
    L, ws = a.L, pa.workspace
    call = lambda P, nbytes, flags=1: L.cagym_ig_episode_boundary(a.h, ctypes.byref(P), None, None, flags, ws.data_ptr(), nbytes, a._stream())
    assert call(pa.P, ws.numel()) == 0
    assert call(pa.P, ws.numel() - 1) == -1 and b"workspace too small" in L.cagym_last_error(a.h)
    assert call(pa.P, ws.numel(), 4) == -1
    bad = dm.DmctsParams.from_buffer_copy(pa.P)
    bad.n_robots = 9
    assert call(bad, ws.numel()) == -1
    bad = dm.DmctsParams.from_buffer_copy(pa.P)
    bad.parallel_agents = 2
    assert call(bad, ws.numel()) == -1
    a.close()
    # before cagym_ig_init: CAGYM_E_STATE
    e = _env()
    assert e.L.cagym_ig_episode_boundary(e.h, ctypes.byref(pa.P), None, None, 1, ws.data_ptr(), ws.numel(), e._stream()) == -5
    e.close()


@pytest.mark.gpu
def test_continuous_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dmcts_continuous.py"), "--worlds", "8", "--steps", "30", "--Ntree", "4",
                        "--Nsims", "3", "--Ncycles", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "finished episodes" in r.stdout and "mean team return per episode" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
