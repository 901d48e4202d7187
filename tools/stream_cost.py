#!/usr/bin/env python3
"""What streamed scenarios (csrc/cagym_stream.h) cost at the flagship size: microseconds per env.step(auto_reset=True) on a fixed
pool and on the same handle shape while it streams (one cagym_stream_refill launch behind every step), and the refill launch alone
when no world finished an episode (its idle path: two loads per world).  Two shapes, both 4096 worlds x 10 agents with a ring of
--depth slots per world:
  free_space   train_agents_swap_circle, every agent RVO
  stage_2      train_stage_2 (2..10 rectangles), RVO agents, LaserScan
Each figure is the median over --blocks blocks of --reps calls between two HIP events (after --warmup untimed blocks), in
microseconds per call, with the fastest and slowest block beside it; fixed and streaming blocks alternate, on handles built from the
same arguments.  Prints one JSON line per shape.
usage: python tools/stream_cost.py [--worlds 4096] [--agents 10] [--depth 2] [--reps 5000] [--blocks 9] [--warmup 2]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--depth", type=int, default=2)
ap.add_argument("--reps", type=int, default=5000)
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
N, M = args.worlds, args.agents


def block(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.reps


def summary(us):
    return {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def measure(name, K, laser, gen):
    envs = {}
    for mode in ("fixed", "streaming"):
        env = B(N, M, n_scenarios=args.depth * N, max_obstacles=K, laserscan=laser, game_over_mode="agent0")
        failed = (env.stream_reference_scenarios if mode == "streaming" else env.generate_reference_scenarios)(**gen)
        env.reset()
        envs[mode] = env
    us = {"fixed": [], "streaming": []}
    for b in range(args.warmup + args.blocks):
        for mode, env in envs.items():  # alternated: both see the same drift of the machine
            t = block(lambda: env.step(auto_reset=True))
            if b >= args.warmup:
                us[mode].append(t)
    env = envs["streaming"]
    idle = [block(env._refill) for _ in range(args.warmup + args.blocks)][args.warmup:]  # nothing stepped: every wave is idle
    st = env.stream_stats()
    steps = (args.warmup + args.blocks) * args.reps
    res = {"shape": name, "worlds": N, "agents": M, "depth": args.depth, "max_obstacles": K, "laserscan": bool(laser), "reps": args.reps,
           "blocks": args.blocks, "n_failed_first_fill": failed, "step_fixed": summary(us["fixed"]), "step_streaming": summary(us["streaming"]),
           "refill_idle": summary(idle), "slots_refilled_per_step": round((st["generated"] - env.S) / steps, 2),
           "n_failed": st["n_failed"], "n_lapped": st["n_lapped"]}
    for env in envs.values():
        env.close()
    return res


print(json.dumps(measure("free_space", 0, False, dict(kinds="train_agents_swap_circle", seed=1, other_policies=scen.POLICY_RVO))), flush=True)
print(json.dumps(measure("stage_2", 10, True, dict(kinds="train_stage_2", seed=2))), flush=True)
