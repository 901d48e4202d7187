"""Pools and twins shared by tests/test_terminal_keep.py and tests/test_trajectory_ring.py.

The pool: N = 7 worlds (the last wave of every launch holds a partial set of worlds), M = 4 or 7 agent slots, S = 3 N scenarios, some
with n_agents < M.  Every agent has a lane of its own 3 m from the next one and a goal 1.25 - 2.0 m from its start at pref_speed 1,
so the time limit 3 (d - 0.75) / v is 1.5 - 3.75 s and a NonCooperative agent arrives after (d - 0.75) / (v dt) <= 12.5 steps:
agent 0 is NonCooperative or RVO everywhere except in the scenarios where it is Static with d = 1.25 (a time-out after 15 steps), and
the Static agents elsewhere have d = 1.25 too, so under both game_over rules every episode is over after 15 steps or so.  One
scenario in five starts with a head-on pair 1.2 m apart (radius 0.5): a collision in the first step.  The distances differ from
scenario to scenario, so the worlds drift apart and most steps finish some worlds and not others."""
import importlib

import numpy as np

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
N_WORLDS = 7
STEPS = 60
OUT = ("obs_oas", "obs_ego", "obs_laser", "reward", "flags", "game_over")


def B():
    return importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def pool(M, seed=0, S=3 * N_WORLDS, ga3c=False):
    """(agents6 [S, M, 6], policy [S, M], n_agents [S], coop [S, M])"""
    rng = np.random.default_rng(seed)
    a6 = np.zeros((S, M, 6))
    pol = np.zeros((S, M), dtype=np.int32)
    n_agents = rng.integers(2, M + 1, S).astype(np.int32)
    n_agents[0], n_agents[1], n_agents[S - 1] = M, 2, 2
    for s in range(S):
        for j in range(M):
            p = [scen.POLICY_NONCOOP, scen.POLICY_RVO, scen.POLICY_STATIC][int(rng.integers(0, 3))]
            if j == 0:
                p = scen.POLICY_STATIC if s % 6 == 4 else [scen.POLICY_NONCOOP, scen.POLICY_RVO][s % 2]
            d = 1.25 if p == scen.POLICY_STATIC else 1.25 + 0.25 * int(rng.integers(0, 4))
            d *= 1 if j % 2 == 0 else -1
            a6[s, j] = [0.1 * (s % 3), 3.0 * j, 0.1 * (s % 3) + d, 3.0 * j, 1.0, 0.5]
            pol[s, j] = p
        if s % 5 == 1:  # a head-on pair: both in collision after the first step
            a6[s, 0] = [0.0, 0.0, 1.5, 0.0, 1.0, 0.5]
            a6[s, 1] = [1.2, 0.0, -0.3, 0.0, 1.0, 0.5]
            pol[s, 0] = pol[s, 1] = scen.POLICY_NONCOOP
        if ga3c:
            pol[s, 0] = scen.POLICY_GA3C
    coop = 0.5 + 0.5 * rng.random((S, M))
    return a6, pol, n_agents, coop


def rectangles(S):
    """two rectangles per scenario, clear of the lanes (y = 0, 3, 6, 9 between x = -2.5 and 2.5) but inside the laser's range"""
    ob = np.zeros((S, 2, 4))
    for s in range(S):
        ob[s, 0] = [-1.0 + 0.2 * (s % 4), -2.5, 0.5 + 0.2 * (s % 4), -1.5]
        ob[s, 1] = [3.5, 1.0 + 0.3 * (s % 3), 4.5, 2.0 + 0.3 * (s % 3)]
    return ob, np.full((S,), 2, dtype=np.int32)


def make_env(M, mode="agent0", laser=False, the_pool=None, N=N_WORLDS, S=None, reset=True):
    the_pool = pool(M) if the_pool is None else the_pool
    a6, pol, n_agents, coop = the_pool
    S = a6.shape[0] if S is None else S
    kw = dict(max_obstacles=2, laserscan=True) if laser else {}
    env = B()(N, M, n_scenarios=S, game_over_mode=mode, **kw)
    ob, no = rectangles(S) if laser else (None, None)
    env.set_scenarios(a6, pol, scen.DYN_UNICYCLE, n_agents=n_agents, coop=coop, obstacles=ob, n_obst=no)
    if reset:
        env.reset()
    return env


def outputs(env):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(env, k).cpu().numpy().copy() for k in OUT if getattr(env, k) is not None}


def state(env):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in env.state().items() if k != "map_bits"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def assert_same_dicts(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert same(a[k], b[k]), (what, k)


def assert_restarts(game_over_history, n=N_WORLDS):
    """the precondition of every test here: at least N restarts, and a step in which some but not all worlds finish"""
    G = np.asarray(game_over_history).astype(bool)
    assert G.sum() >= n, G.sum()
    per_step = G.sum(axis=1)
    assert ((per_step > 0) & (per_step < G.shape[1])).any(), per_step
