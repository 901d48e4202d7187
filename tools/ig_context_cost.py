#!/usr/bin/env python3
"""What the learner's context window costs (csrc/cagym_ig_context.h): microseconds per auto-resetting learner step of --agents
agents, 3 of them IG robots driven at a constant (v, omega), 2 static targets and NonCooperative walkers among rectangles (the cfg5
pool of tools/ig_learner_cost.py), at 2048 and at 256 worlds, on two handles built from the same arguments:
  learner  attach_ig_learner(window, context=False): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the path
           as it was before the context window existed, the yardstick, re-measured in the same run;
  context  attach_ig_learner(window, context=True): the same + ONE cagym_ig_context_window behind the observe launch.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time, after --warmup untimed blocks;
the handles alternate block by block, so both see the same drift of the machine.  Prints ONE JSON line.
usage: python tools/ig_context_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 2] [--seconds 2.0]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", default="2048,256")
ap.add_argument("--agents", type=int, default=20)
ap.add_argument("--window", type=int, default=24)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--seconds", type=float, default=2.0)
args = ap.parse_args()
M, R, KOBS = args.agents, 3, 8
MODES = ("learner", "context")


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


def handle(N, mode):
    a6, ob, nob, _ = scen.obstacle_worlds(N, M, KOBS, seed=1234)
    pol = np.full((N, M), scen.POLICY_NONCOOP, dtype=np.int32)
    pol[:, :R], pol[:, R:R + 2] = scen.POLICY_IGMCTS, scen.POLICY_STATIC
    dyn = np.full((N, M), scen.DYN_UNICYCLE, dtype=np.int32)
    dyn[:, :R] = scen.DYN_FIRSTORDER
    env = B(N, M, n_scenarios=N, max_obstacles=KOBS, game_over_mode="all")
    env.set_scenarios(a6, pol, dyn, obstacles=ob, n_obst=nob)
    env.reset()
    env.attach_ig_learner(window=args.window, rotate=True, context=(mode == "context"))
    env.reset()
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    return env, lambda: env.step(ext, auto_reset=True)


def measure(N):
    made = {mode: handle(N, mode) for mode in MODES}
    # calibration: the faster handle's call time decides the block length for both, so that each figure covers --seconds
    for _, fn in made.values():
        block(fn, 50)  # (first launches load code objects)
    per_call = min(block(fn, 50) for _, fn in made.values())
    reps = max(20, int(args.seconds * 1e6 / (args.blocks * per_call)) + 1)
    us = {mode: [] for mode in MODES}
    for b in range(args.warmup + args.blocks):
        for mode, (_, fn) in made.items():
            t = block(fn, reps)
            if b >= args.warmup:
                us[mode].append(t)
    res = {mode: summary(v) for mode, v in us.items()}
    ctx = made["context"][0]._igm.context_window
    res.update(worlds=N, calls_per_block=reps, timed_seconds={mode: round(sum(v) * reps * 1e-6, 2) for mode, v in us.items()},
               context_added_us=round(res["context"]["us_median"] - res["learner"]["us_median"], 2),
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2),
               context_bytes=ctx.numel() * 4, mean_clearance=round(float(ctx[:, :, 0].mean()), 4),
               agent_cells=int((ctx[:, :, 1] > 0).sum()), seen_share=round(float(ctx[:, :, 2].mean()), 4),
               episodes_finished={mode: int(env.state()["stat_episodes"].sum().item()) for mode, (env, _) in made.items()})
    for env, _ in made.values():
        env.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks,
       "window_bytes_per_world": R * 3 * args.window * args.window * 4,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
