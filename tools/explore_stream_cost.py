#!/usr/bin/env python3
"""What an exploration stream (csrc/cagym_explore.h) costs at the cfg5 shape, 2048 worlds x a ring of depth 2, between HIP events:
  step_fixed / step_streaming   microseconds per env.step(auto_reset=True) of an episodic ig_greedy team on a fixed pool of
                                exploration worlds (what the parent commit can run) and on the same shape while it streams (the
                                refill and the field refresh behind every step); blocks alternate between the two handles
  refill_idle                   cagym_stream_refill when no world finished: the refill's idle waves plus the three refresh launches
                                that find an empty work list
  refill_all                    cagym_stream_refill after every world finished one episode (reset(advance_episode=True), untimed):
                                N slots regenerated, rasterised and their distance fields rebuilt; per_slot = that time / N
Each figure is the median over --blocks blocks (after --warmup untimed ones) with the fastest and slowest beside it.  One JSON line.
--dump-pool FILE writes the fixed handle's pool as an .npz; --fixed-pool FILE measures step_fixed alone on that pool, uploaded
through set_scenarios - the form that runs on a commit from before the exploration sampler (the parent-to-tree comparison).
usage: python tools/explore_stream_cost.py [--worlds 2048] [--depth 2] [--robots 3] [--targets 5] [--reps 200] [--blocks 7] [--warmup 2]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=2048)
ap.add_argument("--depth", type=int, default=2)
ap.add_argument("--robots", type=int, default=3)
ap.add_argument("--targets", type=int, default=5)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dump-pool", default=None)
ap.add_argument("--fixed-pool", default=None)
args = ap.parse_args()
N, M = args.worlds, args.robots + args.targets
GEN = dict(kinds="train_stage_1", seed=1, n_robots=args.robots, n_targets=args.targets, n_obst=(1, 4), robot_pref_speed=10.0)


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


def handle(mode):
    env = B(N, M, n_scenarios=args.depth * N, max_obstacles=4, game_over_mode="agent0")
    if mode == "uploaded":
        p = np.load(args.fixed_pool)
        env.set_scenarios(p["agents6"], p["policy"], p["dynamics"], n_agents=p["n_agents"], coop=p["coop"], obstacles=p["obstacles"],
                          n_obst=p["n_obst"])
    else:
        (env.stream_exploration_worlds if mode == "streaming" else env.generate_exploration_worlds)(**GEN)
    env.reset()
    env.attach_ig_greedy(episodic=True)
    return env


if args.fixed_pool:
    env = handle("uploaded")
    us = [block(lambda: env.step(auto_reset=True), args.reps) for _ in range(args.warmup + args.blocks)][args.warmup:]
    print(json.dumps({"shape": "uploaded_fixed_pool", "worlds": N, "agents": M, "depth": args.depth, "reps": args.reps,
                      "blocks": args.blocks, "step_fixed": summary(us)}), flush=True)
    env.close()
    sys.exit(0)
envs = {mode: handle(mode) for mode in ("fixed", "streaming")}
if args.dump_pool:
    e = envs["fixed"]
    np.savez(args.dump_pool, **{k: t.cpu().numpy() for k, t in dict(e.scenarios(), **e.obstacles()).items()})
us = {mode: [] for mode in envs}
for b in range(args.warmup + args.blocks):
    for mode, env in envs.items():  # alternated: both see the same drift of the machine
        t = block(lambda: env.step(auto_reset=True), args.reps)
        if b >= args.warmup:
            us[mode].append(t)
env = envs["streaming"]
steps = (args.warmup + args.blocks) * args.reps
built_per_step = env.exploration_stream_stats()["fields_built"] / steps
idle = [block(env._refill, args.reps) for _ in range(args.warmup + args.blocks)][args.warmup:]  # nothing stepped: empty work list
full = []
for b in range(args.warmup + args.blocks):
    env._streaming = False  # every world advances one episode, and the refill that reset() would enqueue is left to the timed call
    env.reset(advance_episode=True)
    env._streaming = True
    before = env.exploration_stream_stats()["fields_built"]
    t = block(env._refill, 1)
    assert env.exploration_stream_stats()["fields_built"] - before == N
    if b >= args.warmup:
        full.append(t)
st = env.stream_stats()
res = {"shape": "exploration_stage_1", "worlds": N, "agents": M, "robots": args.robots, "depth": args.depth, "reps": args.reps,
       "blocks": args.blocks, "step_fixed": summary(us["fixed"]), "step_streaming": summary(us["streaming"]),
       "streaming_over_fixed": round(statistics.median(us["streaming"]) / statistics.median(us["fixed"]), 4),
       "fields_rebuilt_per_step": round(built_per_step, 2), "refill_idle": summary(idle), "refill_all": summary(full),
       "per_slot_us": round(statistics.median(full) / N, 2), "n_failed": st["n_failed"], "n_lapped": st["n_lapped"]}
for env in envs.values():
    env.close()
print(json.dumps(res), flush=True)
