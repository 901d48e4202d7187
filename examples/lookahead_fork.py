#!/usr/bin/env python3
"""One-step look-ahead over the real env dynamics with env.fork(): agent 0 of every source world is external (the CARRL action
table, 11 headings at preferred speed) among RVO agents.  At every decision each source world is forked into 11 siblings, one
per table row; the siblings hold their row for H steps without auto-reset, agent 0's summed reward is compared, and the best
first action is applied in the source world - which a subset snapshot / restore keeps where it was while the siblings look ahead.

Layout: world 12 k is source k, worlds 12 k + 1 .. 12 k + 11 are its siblings; n_scenarios = n_worlds, so every world owns its
scenario slot (fork copies the source's scenario over the sibling's).

usage: python examples/lookahead_fork.py [--worlds 8] [--horizon 5] [--decisions 20] [--agents 6] [--seed 3]"""
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
ap.add_argument("--worlds", type=int, default=8, help="source worlds")
ap.add_argument("--horizon", type=int, default=5)
ap.add_argument("--decisions", type=int, default=20)
ap.add_argument("--agents", type=int, default=6)
ap.add_argument("--seed", type=int, default=3)
args = ap.parse_args()

ROWS = 11  # CARRLPolicy.py:5-15
W, H, M = args.worlds, args.horizon, args.agents
N = W * (1 + ROWS)
pol = np.full((N, M), scen.POLICY_RVO, dtype=np.int32)
pol[:, 0] = scen.POLICY_CARRL
env = B(N, M, game_over_mode="agent0")
env.set_scenarios(scen.random_worlds_fast(N, M, seed=args.seed), pol, scen.DYN_UNICYCLE, coop=np.full((N, M), 0.5))
env.reset()
dev = env.device

sources = torch.arange(W, device=dev) * (1 + ROWS)
siblings = (sources[:, None] + 1 + torch.arange(ROWS, device=dev)[None, :]).reshape(-1)  # [W * 11], family-major
src_list = sources.repeat_interleave(ROWS)
source_mask = torch.zeros(N, dtype=torch.uint8, device=dev)
source_mask[sources] = 1
rows = torch.arange(ROWS, dtype=torch.float32, device=dev).repeat(W)
ext = torch.zeros((N, M, 2), dtype=torch.float32, device=dev)
ret = torch.zeros(W, dtype=torch.float64, device=dev)
outcomes = torch.zeros(3, dtype=torch.int64, device=dev)  # agent 0 at goal / in collision / out of time
gain = 0.0

for d in range(args.decisions):
    here = env.snapshot(sources)
    env.fork(src_list, siblings)
    ext.zero_()
    ext[siblings, 0, 0] = rows
    score = torch.zeros(W * ROWS, dtype=torch.float64, device=dev)
    for h in range(H):
        env.step(ext, auto_reset=False)
        score += env.reward[siblings, 0].double()
    score = score.view(W, ROWS)
    best = score.argmax(dim=1)
    gain += float((score.max(dim=1).values - score[:, ROWS // 2]).mean())  # against "straight ahead"
    env.restore(here)  # the sources stepped along: back to the decision point
    ext.zero_()
    ext[sources, 0, 0] = best.float()
    env.step(ext, auto_reset=False)
    ret += env.reward[sources, 0].double()
    over = env.game_over[sources].bool()
    f0 = env.flags[sources, 0]
    for k, bit in enumerate((1, 2, 4)):  # CAGYM_FLAG_AT_GOAL / IN_COLLISION / RAN_OUT_OF_TIME
        outcomes[k] += (over & ((f0 & bit) != 0)).sum()
    env.reset(world_mask=source_mask & env.game_over)  # finished sources start over

torch.cuda.synchronize()
o = outcomes.tolist()
print("lookahead_fork: %d worlds x %d siblings, H = %d, %d decisions: mean return %.3f, at goal %d, collisions %d, timed out %d, "
      "mean look-ahead gain over straight ahead %.3f" % (W, ROWS, H, args.decisions, float(ret.mean()), o[0], o[1], o[2], gain / args.decisions))
env.close()
