#!/usr/bin/env python3
"""What heading-resolved view gains and goal headings cost (csrc/cagym_ig_headings.h): microseconds, on the pool of
tools/ig_viewpoints_cost.py (--agents agents, 3 of them IG robots, 2 static targets and NonCooperative walkers among 8 rectangles)
at 2048 and at 256 worlds.
  learner        attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the yardstick;
  goals          the same step with attach_ig_goals and every robot under way to a goal (two more launches) - the other yardstick;
  goals_face     that step once the goals carry headings: cagym_ig_goal_face_actions and cagym_ig_goal_face_status behind them;
  map            ONE cagym_ig_view_gain launch in map mode (the robot turning on the spot) - the yardstick of the maps below;
  hmap8, hmap16  ONE cagym_ig_view_gain_headings launch in map mode with H = 8 and H = 16, all outputs;
  hmap8_best     H = 8 without the two [.., H] tensors (want_rows=False), as env.ig_propose_goals(headings=8) launches it;
  points64       cagym_ig_view_gain on 64 caller's points per world, drawn uniformly over the map;
  hpoints64      cagym_ig_view_gain_headings, H = 8, on the same points.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time (one call per block where a call
is longer than that), after --warmup untimed blocks; the figures alternate block by block, so all see the same drift of the machine.
Prints ONE JSON line.
usage: python tools/ig_headings_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 1] [--seconds 2.0]"""
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
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--seconds", type=float, default=2.0)
args = ap.parse_args()
M, R, KOBS = args.agents, 3, 8
MODES = ("learner", "goals", "goals_face", "map", "hmap8", "hmap16", "hmap8_best", "points64", "hpoints64")


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


def handle(N, goals):
    a6, ob, nob, _ = scen.obstacle_worlds(N, M, KOBS, seed=1234)
    pol = np.full((N, M), scen.POLICY_NONCOOP, dtype=np.int32)
    pol[:, :R], pol[:, R:R + 2] = scen.POLICY_IGMCTS, scen.POLICY_STATIC
    dyn = np.full((N, M), scen.DYN_UNICYCLE, dtype=np.int32)
    dyn[:, :R] = scen.DYN_FIRSTORDER
    env = B(N, M, n_scenarios=N, max_obstacles=KOBS, game_over_mode="all")
    env.set_scenarios(a6, pol, dyn, obstacles=ob, n_obst=nob)
    env.reset()
    env.attach_ig_learner(window=args.window, rotate=True)
    if goals:
        env.attach_ig_goals()
    env.reset()
    return env


def measure(N):
    rng = np.random.default_rng(7)
    plain, goal, face = handle(N, False), handle(N, True), handle(N, True)
    dev = goal.device
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=dev)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    for _ in range(10):  # a belief that is no longer the prior's, as a policy would meet it
        goal.step(ext, auto_reset=True)
    ig = goal._igm.ig
    points = torch.as_tensor(rng.uniform(-14.9, 14.9, (N, 64, 2)), device=dev)
    there = torch.as_tensor(rng.uniform(-14.0, 14.0, (N, R, 2)), device=dev)
    facing = torch.as_tensor(rng.uniform(-3.0, 3.0, (N, R)), device=dev)

    def step_with_goals(env, headings):
        env.ig_set_goals(there, headings=headings)  # (a world that restarts loses its goals, in both handles alike; the launches
        return lambda: env.step(ext, auto_reset=True)  # run whatever the flags say, and the share still active is reported)

    view = ig.view_gain()
    h8 = ig.view_gain_headings(headings=8)
    h16 = ig.view_gain_headings(headings=16)
    h8b = ig.view_gain_headings(headings=8, want_rows=False)
    pts = ig.view_gain(points=points)
    hpts = ig.view_gain_headings(points=points, headings=8)
    fns = {"learner": lambda: plain.step(ext, auto_reset=True),
           "goals": step_with_goals(goal, None),
           "goals_face": step_with_goals(face, facing),
           "map": lambda: ig.view_gain(out=view),
           "hmap8": lambda: ig.view_gain_headings(headings=8, out=h8),
           "hmap16": lambda: ig.view_gain_headings(headings=16, out=h16),
           "hmap8_best": lambda: ig.view_gain_headings(headings=8, out=h8b, want_rows=False),
           "points64": lambda: ig.view_gain(points=points, out=pts),
           "hpoints64": lambda: ig.view_gain_headings(points=points, headings=8, out=hpts)}
    per_call = {}
    for k, fn in fns.items():
        block(fn, 1)  # (first launches load code objects)
        t = block(fn, 1)
        per_call[k] = block(fn, min(50, max(1, int(5e4 / t))))
    reps = {k: max(1, int(args.seconds * 1e6 / (args.blocks * t)) + 1) for k, t in per_call.items()}
    us = {mode: [] for mode in MODES}
    for b in range(args.warmup + args.blocks):
        for mode in MODES:
            t = block(fns[mode], reps[mode])
            if b >= args.warmup:
                us[mode].append(t)
    res = {mode: summary(v) for mode, v in us.items()}
    m = res["map"]["us_median"]
    res.update(worlds=N, calls_per_block=reps,
               hmap8_over_map=round(res["hmap8"]["us_median"] / m, 3), hmap16_over_map=round(res["hmap16"]["us_median"] / m, 3),
               hmap8_best_over_map=round(res["hmap8_best"]["us_median"] / m, 3),
               hpoints64_over_points64=round(res["hpoints64"]["us_median"] / res["points64"]["us_median"], 3),
               face_launches_us=round(res["goals_face"]["us_median"] - res["goals"]["us_median"], 2),
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2),
               goals_active_share=round(float((goal.ig_goals()["active"] != 0).double().mean()), 3),
               face_active_share=round(float((face.ig_goals()["active"] != 0).double().mean()), 3),
               valid_share=round(float((view["valid"] != 0).double().mean()), 4))
    for e in (plain, goal, face):
        e.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
