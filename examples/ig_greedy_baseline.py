#!/usr/bin/env python3
"""The greedy baseline next to examples/dmcts_experiment.py: the same worlds (IG_agent_crossing, 3 robots + 2 static targets,
MANY worlds at once) driven by the one-step greedy information-gain policy (policies/ig_greedy.py), every robot on its own and
with coordinate=True (the team chooses in slot order without the cells its earlier robots chose), and by the Dec-MCTS planner;
prints the cumulative team reward of each.  Every policy is attached to its own handle and runs inside step().

usage: python examples/ig_greedy_baseline.py [--worlds 256] [--steps 30] [--Ntree 30] [--Ncycles 5] [--no-planner]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=256)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--Ntree", type=int, default=30)
ap.add_argument("--Ncycles", type=int, default=5)
ap.add_argument("--Nsims", type=int, default=10)
ap.add_argument("--no-planner", action="store_true", help="skip the Dec-MCTS run (most of the time)")
args = ap.parse_args()

N, M = args.worlds, 10
OBST = [(2, 2, 10, 10), (-10, 2, -2, 10), (2, -10, 10, -2), (-10, -10, -2, -2)]  # test_cases.py:3219-3222
a6 = np.zeros((M, 6))
a6[:, 4], a6[:, 5], a6[:, 0] = 1.0, 0.1, 1e3 + np.arange(M)
a6[0], a6[1], a6[2] = [-5, 0, 16, 0, 1, .5], [0, 0, 16, 0, 1, .5], [5, 0, 16, 0, 1, .5]   # test_cases.py:3226-3232
a6[3], a6[4] = [6, 12, 0, 0, 1, .2], [-6, -12, 0, 0, 1, .2]                               # static targets
pol = np.zeros(M, dtype=np.int32)
pol[:3] = scen.POLICY_IGMCTS


def run(attach):
    env = B(N, M, max_obstacles=4, game_over_mode="agent0")
    env.set_scenarios(np.tile(a6[None], (N, 1, 1)), np.tile(pol[None], (N, 1)), scen.DYN_FIRSTORDER, heading0=np.zeros((N, M)),
                      n_agents=[5] * N, obstacles=np.tile(np.array(OBST, dtype=np.float64)[None], (N, 1, 1)), n_obst=[4] * N)
    env.reset()
    attach(env)
    cum = torch.zeros(N, dtype=torch.float64, device=env.device)
    for t in range(args.steps):
        env.step(None)
        cum += env.team_reward                                     # policy.team_reward (experiments/src/dmcts.py:90)
    torch.cuda.synchronize()
    env.close()
    return cum.cpu().numpy()


rows = [("ig_greedy", lambda e: e.attach_ig_greedy(detect_fov=60.0, detect_range=5.0, radius=0.5)),
        ("ig_greedy, coordinate=True", lambda e: e.attach_ig_greedy(detect_fov=60.0, detect_range=5.0, radius=0.5, coordinate=True))]
if not args.no_planner:
    rows.append(("ig_mcts (Dec-MCTS)", lambda e: e.attach_ig_mcts(detect_fov=60.0, detect_range=5.0, xdt=5, Ntree=args.Ntree,
                                                                 Nsims=args.Nsims, mcts_cp=1.0, mcts_horizon=4, mcts_gamma=0.95,
                                                                 Ncycles=args.Ncycles, radius=0.5, seed=0)))
print("worlds %d, steps %d: cumulative team reward" % (N, args.steps))
for name, attach in rows:
    c = run(attach)
    print("  %-28s mean %.3f, std %.3f, min %.3f, max %.3f" % (name, c.mean(), c.std(), c.min(), c.max()))
