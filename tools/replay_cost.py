#!/usr/bin/env python3
"""What replay of failed scenarios (csrc/cagym_replay.h) costs: microseconds per env.step(auto_reset=True) at 4096 worlds x 10 agents
on a streaming handle with an episode log (RVO agents in free space, train_agents_swap_circle, a ring of depth 2), on handles built
from the same arguments:
  plain_a, plain_b  stream + log, replay never armed: step, log update (scan, write), k_stream_refill - the launches of a tree without
                    replay, so the same script run there gives the yardstick, and the difference between the two is the spread of
                    two runs on one machine;
  armed             attach_replay(p = --p, outcomes = collision + stuck): one k_replay_harvest launch (a single workgroup) between
                    the log update and the refill, which is k_stream_refill_replay.
Each figure is the median over --blocks blocks of calls between two HIP events (after --warmup untimed blocks), with the fastest and
slowest block beside it; the handles alternate block by block, so all see the same drift of the machine.  On a tree without
attach_replay the armed handle is left out.  Prints one JSON line.
usage: python tools/replay_cost.py [--worlds 4096] [--agents 10] [--reps 1000] [--blocks 7] [--warmup 2] [--p 0.25] [--capacity 4096]"""
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
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--p", type=float, default=0.25)
ap.add_argument("--capacity", type=int, default=4096)
args = ap.parse_args()
N, M = args.worlds, args.agents
MODES = ("plain_a", "plain_b") + (("armed",) if hasattr(B, "attach_replay") else ())


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def summary(us):
    return {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


envs = {}
for mode in MODES:
    env = B(N, M, n_scenarios=2 * N, game_over_mode="agent0")
    env.stream_reference_scenarios("train_agents_swap_circle", seed=1, other_policies=scen.POLICY_RVO)
    env.attach_episode_log(65536)
    if mode == "armed":
        env.attach_replay(capacity=args.capacity, p=args.p)
    env.reset()
    envs[mode] = env
us = {mode: [] for mode in MODES}
for b in range(args.warmup + args.blocks):
    for mode, env in envs.items():
        t = block(lambda: env.step(auto_reset=True), args.reps)
        if b >= args.warmup:
            us[mode].append(t)
res = {"worlds": N, "agents": M, "blocks": args.blocks, "reps": args.reps, "step": {mode: summary(v) for mode, v in us.items()}}
res["step"]["plain_spread_us"] = round(abs(res["step"]["plain_a"]["us_median"] - res["step"]["plain_b"]["us_median"]), 2)
if "armed" in envs:
    res["step"]["armed_added_us"] = round(res["step"]["armed"]["us_median"] - min(res["step"]["plain_a"]["us_median"], res["step"]["plain_b"]["us_median"]), 2)
    res["replay"] = envs["armed"].replay_stats()
res["episodes_finished"] = {mode: int(env.state()["stat_episodes"].sum().item()) for mode, env in envs.items()}
res["stream"] = {mode: env.stream_stats() for mode, env in envs.items()}
for env in envs.values():
    env.close()
print(json.dumps(res), flush=True)
