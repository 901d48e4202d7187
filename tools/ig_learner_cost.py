#!/usr/bin/env python3
"""What the learner's observation costs (csrc/cagym_ig_observe.h): microseconds per auto-resetting env step of --agents agents, 3 of
them IG robots driven at a constant (v, omega), 2 static targets and NonCooperative walkers among rectangles (the cfg5 pool of
bench.py), at 2048 and at 256 worlds, on four handles built from the same arguments:
  step    (a) cagym_step_autoreset alone - the parent's launch, the yardstick;
  fused   (b) the step + ONE cagym_ig_observe (restart mask = the step's game_over, FOLD, windows of --window cells written);
  nowin   (b') the same with a NULL belief_window: what the launch costs without its window phase;
  chain   (c) the step + the four launches that did the same before, without any window: cagym_ig_robot_inputs,
          cagym_ig_update_belief, cagym_ig_mi_reward, cagym_ig_episode_boundary (FOLD, the same restart mask).
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time, after --warmup untimed blocks;
the handles alternate block by block, so all see the same drift of the machine.  Prints ONE JSON line.
usage: python tools/ig_learner_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 2] [--seconds 2.0]"""
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
igm = importlib.import_module("gym-exploration-2d_amd.ig")
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
MODES = ("step", "fused", "nowin", "chain")


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
    dev = env.device
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=dev)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    if mode == "step":
        return env, lambda: env.step(ext, auto_reset=True)
    ig = igm.InfoGain(env)
    reward = torch.zeros((N,), dtype=torch.float64, device=dev)
    if mode in ("fused", "nowin"):
        gain, observed = torch.zeros_like(reward), torch.zeros((N, 60), dtype=torch.int64, device=dev)
        window = torch.zeros((N, R, 3, args.window, args.window), dtype=torch.float32, device=dev) if mode == "fused" else None

        def fused():
            env.step(ext, auto_reset=True)
            ig.observe(R, 5.0, env.obs_oas, args.window, True, env.game_over, igm.EPISODE_FOLD, reward, gain, observed, window)
        return env, fused
    planner = igm.GreedyPlanner(ig, R)  # (its parameter block and workspace are what the boundary launch asks for)
    poses = torch.zeros((N, R, 3), dtype=torch.float64, device=dev)
    det = torch.zeros((N, R, M - 1, 2), dtype=torch.float64, device=dev)
    n_det = torch.zeros((N, R), dtype=torch.int32, device=dev)
    world = torch.arange(N, dtype=torch.int32, device=dev)

    def chain():
        env.step(ext, auto_reset=True)
        ig.robot_inputs(R, 5.0, env.obs_oas, poses, det, n_det)
        ig.mi_reward(ig.update_belief(poses, det, n_det), world, out=reward)
        ig.episode_boundary(planner.P, planner.workspace, reward, env.game_over, igm.EPISODE_FOLD)
    return env, chain


def measure(N):
    made = {mode: handle(N, mode) for mode in MODES}
    # calibration: the fastest mode's call time decides the block length for all three, so that each covers --seconds
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
    res.update(worlds=N, calls_per_block=reps, timed_seconds={mode: round(sum(v) * reps * 1e-6, 2) for mode, v in us.items()},
               fused_added_us=round(res["fused"]["us_median"] - res["step"]["us_median"], 2),
               chain_added_us=round(res["chain"]["us_median"] - res["step"]["us_median"], 2),
               window_phase_us=round(res["fused"]["us_median"] - res["nowin"]["us_median"], 2),
               fused_minus_chain_us=round(res["fused"]["us_median"] - res["chain"]["us_median"], 2),
               chain_spread_us=round(res["chain"]["us_max"] - res["chain"]["us_min"], 2),
               episodes_finished={mode: int(env.state()["stat_episodes"].sum().item()) for mode, (env, _) in made.items()})
    for env, _ in made.values():
        env.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks,
       "window_bytes_per_world": R * 3 * args.window * args.window * 4,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
