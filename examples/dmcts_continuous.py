#!/usr/bin/env python3
"""IG_agent_crossing (3 ig_mcts robots + 2 static targets, test_cases.py:3209-3239) run CONTINUOUSLY in many worlds: a VecEnv
over an env with attach_ig_mcts(episodic=True).  Robot 0's time limit is staggered over the worlds (game_over_mode "agent0"), so
the worlds finish at their own times; each one restarts inside the step launch - next scenario, prior belief, no communicated
plans - and the team's return per episode is kept on the device (ig_episode_stats()): no host synchronisation per step.

usage: python examples/dmcts_continuous.py [--worlds 64] [--steps 200] [--Ntree 30] [--Nsims 10] [--Ncycles 5]
                                           [--parallelize-agents]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
vec = importlib.import_module("gym-exploration-2d_amd.vecenv")

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=64)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--Ntree", type=int, default=30)
ap.add_argument("--Nsims", type=int, default=10)
ap.add_argument("--Ncycles", type=int, default=5)
ap.add_argument("--parallelize-agents", action="store_true", help="ig_mcts.set_param(..., parallelize_agents=True)")
args = ap.parse_args()

N, M = args.worlds, 10
OBST = [(2, 2, 10, 10), (-10, 2, -2, 10), (2, -10, 10, -2), (-10, -10, -2, -2)]  # test_cases.py:3219-3222
a6 = np.zeros((N, M, 6))
a6[..., 4], a6[..., 5], a6[..., 0] = 1.0, 0.1, 1e3 + np.arange(M)
a6[:, 0], a6[:, 1], a6[:, 2] = [-5, 0, 16, 0, 1, .5], [0, 0, 16, 0, 1, .5], [5, 0, 16, 0, 1, .5]   # test_cases.py:3226-3232
a6[:, 3], a6[:, 4] = [6, 12, 0, 0, 1, .2], [-6, -12, 0, 0, 1, .2]                                   # static targets
# staggered time limits: robot 0's goal 2.25 .. 4 m away at pref_speed 3 gives it 1.5 .. 3.25 s (15 .. 33 steps)
a6[:, 0, 2] = -5 + 2.25 + 0.25 * (np.arange(N) % 8)
a6[:, 0, 4] = 3.0
pol = np.zeros((N, M), dtype=np.int32)
pol[:, :3] = scen.POLICY_IGMCTS
env = B(N, M, max_obstacles=4, game_over_mode="agent0")
env.set_scenarios(a6, pol, scen.DYN_FIRSTORDER, heading0=np.zeros((N, M)), n_agents=[5] * N,
                  obstacles=np.tile(np.array(OBST, dtype=np.float64)[None], (N, 1, 1)), n_obst=[4] * N)
env.attach_ig_mcts(Ntree=args.Ntree, Nsims=args.Nsims, Ncycles=args.Ncycles, parallelize_agents=args.parallelize_agents,
                   episodic=True)                                  # detect_fov 60 deg, range 5 m, xdt 5 (dmcts.py:74-78)
v = vec.CagymVecEnv(env, ["dist_to_goal", "other_agents_states"])
v.reset()
total = torch.zeros(N, dtype=torch.float64, device=env.device)
for t in range(args.steps):
    obs, rews, dones, infos = v.step([None])                       # finished worlds restart inside the launch
    total += infos["team_reward"]
st = {k: x.cpu().numpy() for k, x in env.ig_episode_stats().items()}  # the only device-to-host copy
n = int(st["episodes"].sum())
mean = st["sum"].sum() / n if n else float("nan")
print("worlds %d, steps %d: finished episodes %d (per world %d .. %d), mean team return per episode %.3f, last %.3f .. %.3f, in progress %.3f"
      % (N, args.steps, n, st["episodes"].min(), st["episodes"].max(), mean, st["last"].min(), st["last"].max(), st["running"].mean()))
assert abs(float(total.sum()) - (st["sum"].sum() + st["running"].sum())) < 1e-6 * max(1.0, float(total.sum()))
v.close()
