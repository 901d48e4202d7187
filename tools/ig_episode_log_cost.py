#!/usr/bin/env python3
"""What the IG team's episode log costs (csrc/cagym_ig_episode_log.h): microseconds per auto-resetting env step of the cfg5 pool
of tools/ig_learner_cost.py (--agents agents: 3 IG robots driven at a constant (v, omega), 2 static targets, NonCooperative walkers
among rectangles; window 24) under attach_ig_learner, at 2048 and at 256 worlds, on two handles built from the same arguments:
  nolog  step(auto_reset=True) = cagym_step_autoreset + cagym_ig_observe - the parent's chain, the yardstick, re-measured here;
  log    the same with attach_ig_episode_log: two more launches per step (the single-workgroup scan, one workgroup per world).
and in three regimes:
  rare   game_over_mode "all" and the last walker's pref_speed divided by 1000: it does not arrive and its time limit does not end,
         so worlds finish four times more rarely than in `quiet` - at 256 worlds nine steps in ten finish no world at all: what
         the log costs on a step where every workgroup leaves behind its target check;
  quiet  game_over_mode "all", the pool as it is: episodes last hundreds of steps, two worlds in a thousand finish per step;
  busy   game_over_mode "agent0" and robot 0's pref_speed times 30: its time limit ends an episode every ten-odd steps, so a
         share of the worlds (printed per block) writes a row with its three sums over 3600 cells in every step.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time, after --warmup untimed blocks;
the handles alternate block by block, so both see the same drift of the machine.  Prints ONE JSON line.
usage: python tools/ig_episode_log_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 2] [--seconds 2.0]"""
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
MODES = ("nolog", "log")


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


def handle(N, mode, regime):
    a6, ob, nob, _ = scen.obstacle_worlds(N, M, KOBS, seed=1234)
    busy = regime == "busy"
    if busy:
        a6[:, 0, 4] *= 30.0
    if regime == "rare":
        a6[:, M - 1, 4] *= 1e-3
    pol = np.full((N, M), scen.POLICY_NONCOOP, dtype=np.int32)
    pol[:, :R], pol[:, R:R + 2] = scen.POLICY_IGMCTS, scen.POLICY_STATIC
    dyn = np.full((N, M), scen.DYN_UNICYCLE, dtype=np.int32)
    dyn[:, :R] = scen.DYN_FIRSTORDER
    env = B(N, M, n_scenarios=N, max_obstacles=KOBS, game_over_mode="agent0" if busy else "all")
    env.set_scenarios(a6, pol, dyn, obstacles=ob, n_obst=nob)
    env.reset()
    env.attach_ig_learner(window=args.window)
    if mode == "log":
        env.attach_ig_episode_log(capacity=65536)
    env.reset()
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    return env, lambda: env.step(ext, auto_reset=True)


def finished(env):
    return int(env.ig_episode_stats()["episodes"].sum().item())


def measure(N, regime):
    made = {mode: handle(N, mode, regime) for mode in MODES}
    for _, fn in made.values():
        block(fn, 50)  # (first launches load code objects)
    per_call = min(block(fn, 50) for _, fn in made.values())
    reps = max(20, int(args.seconds * 1e6 / (args.blocks * per_call)) + 1)
    us, share = {mode: [] for mode in MODES}, {mode: [] for mode in MODES}
    for b in range(args.warmup + args.blocks):
        for mode, (env, fn) in made.items():
            n0 = finished(env)
            t = block(fn, reps)
            if b >= args.warmup:
                us[mode].append(t)
                share[mode].append(round((finished(env) - n0) / float(reps * N), 5))
    res = {mode: summary(v) for mode, v in us.items()}
    rows = made["log"][0].ig_episode_log_views()
    res.update(worlds=N, regime=regime, calls_per_block=reps,
               timed_seconds={mode: round(sum(v) * reps * 1e-6, 2) for mode, v in us.items()},
               finished_share_per_block=share,
               log_added_us=round(res["log"]["us_median"] - res["nolog"]["us_median"], 2),
               nolog_spread_us=round(res["nolog"]["us_max"] - res["nolog"]["us_min"], 2),
               rows_appended=int(rows["head"].item()), desync=int(rows["desync"].item()))
    for env, _ in made.values():
        env.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks,
       "shapes": [measure(int(n), regime) for n in args.worlds.split(",") for regime in ("rare", "quiet", "busy")]}
print(json.dumps(out), flush=True)
