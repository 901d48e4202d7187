#!/usr/bin/env python3
"""What the episode recorder (attach_episode_records, csrc/cagym_episode_records.h) costs at the flagship size: 4096 worlds x 10
RVO agents + OtherAgentsStates, scenario pool of 2 x worlds, game over when all agents are done, auto-reset.  Four configurations
on ONE build, each timed as --blocks blocks between two device synchronisations (wall clock around each block; the median
and the spread of the blocks are reported, after --warmup untimed blocks):
  step            a step(auto_reset=True) loop, --steps launches per block
  step+records    the same loop with records attached (one cagym_episode_records_update launch behind every step)
  rollout         rollout(--roll) launches, --steps steps per block
  rollout+records the same with records attached (one update launch over the T slices behind every rollout)
The unattached loops run code this feature does not touch: they are the baseline.  Prints one JSON line.
usage: python tools/episode_records_cost.py [--worlds 4096] [--agents 10] [--steps 512] [--roll 512] [--blocks 9] [--warmup 2]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--roll", type=int, default=512)
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--pool-factor", type=int, default=2)
args = ap.parse_args()

N, M, S = args.worlds, args.agents, args.pool_factor * args.worlds
a6 = scen.random_worlds_fast(S, M, seed=1234)


def measure(rollout, records):
    env = B(N, M, n_scenarios=S, game_over_mode="all")
    env.set_scenarios(a6, scen.POLICY_RVO, scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5))
    env.reset()
    if records:
        env.attach_episode_records(keep="first")
    roll = max(1, min(args.roll, args.steps))
    traj = env.alloc_rollout(roll) if rollout else None

    def block():
        if rollout:
            for _ in range(args.steps // roll):
                env.rollout(roll, auto_reset=True, out=traj)
        else:
            for _ in range(args.steps):
                env.step(auto_reset=True)

    times = []
    for b in range(args.warmup + args.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        block()
        torch.cuda.synchronize()
        if b >= args.warmup:
            times.append(time.perf_counter() - t0)
    steps = (args.steps // roll) * roll if rollout else args.steps
    rate = [N * steps / t for t in times]
    res = {"env_steps_per_s_median": statistics.median(rate), "min": min(rate), "max": max(rate),
           "us_per_step_median": 1e6 * statistics.median(times) / steps}
    if records:
        rec = env.episode_records()  # raises on desync
        res["episodes_recorded"] = int(rec["count"].sum())
        res["cases_with_a_record"] = int((rec["count"] > 0).sum())
    env.close()
    return res


out = {"worlds": N, "agents": M, "scenarios": S, "steps_per_block": args.steps, "roll": args.roll, "blocks": args.blocks}
for name, rollout, records in (("step", False, False), ("step+records", False, True), ("rollout", True, False),
                               ("rollout+records", True, True)):
    out[name] = measure(rollout, records)
for a, b in (("step", "step+records"), ("rollout", "rollout+records")):
    out[b]["overhead_vs_%s" % a] = out[a]["env_steps_per_s_median"] / out[b]["env_steps_per_s_median"] - 1.0
print(json.dumps(out))
