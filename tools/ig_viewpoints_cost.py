#!/usr/bin/env python3
"""What view gains and goal proposals cost (csrc/cagym_ig_viewpoints.h): microseconds, on the pool of tools/ig_goals_cost.py
(--agents agents, 3 of them IG robots, 2 static targets and NonCooperative walkers among 8 rectangles) at 2048 and at 256 worlds.
  learner        attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the yardstick,
                 re-measured in the same run;
  geodesic_all   ONE cagym_ig_geodesic launch for all N x 3 robots from their own places - the other yardstick;
  map            ONE cagym_ig_view_gain launch in map mode: the 3600 cell centres of every world;
  map_16th       the same launch with one world in sixteen flagged in its mask;
  points64       the same kernel on 64 caller's points per world, drawn uniformly over the map;
  propose        ONE cagym_ig_propose_goals launch, k = 8, on the map and the fields the two launches above left;
  propose_goals  env.ig_propose_goals(k=8) as a whole: the map, the geodesic launch from the robots' places, the proposals.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time (one call per block where a call
is longer than that), after --warmup untimed blocks; the figures alternate block by block, so all see the same drift of the machine.
Also reported: the (viewpoint, cell) pairs a map launch traces, the share it finds visible and the pairs per second.  Prints ONE JSON
line.
usage: python tools/ig_viewpoints_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 1] [--seconds 2.0]"""
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
M, R, KOBS, KPROP = args.agents, 3, 8, 8
MODES = ("learner", "geodesic_all", "map", "map_16th", "points64", "propose", "propose_goals")


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
    plain, goal = handle(N, False), handle(N, True)
    dev = goal.device
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=dev)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    for _ in range(10):  # a belief that is no longer the prior's, as a policy would meet it
        goal.step(ext, auto_reset=True)
    ig = goal._igm.ig
    st = goal.state()
    here = torch.stack((st["pos_x"][:, :R], st["pos_y"][:, :R]), dim=-1).contiguous()
    points = torch.as_tensor(rng.uniform(-14.9, 14.9, (N, 64, 2)), device=dev)
    some = np.zeros(N, dtype=np.uint8)
    some[rng.choice(N, size=max(N // 16, 1), replace=False)] = 1  # (drawn, not every sixteenth: workgroups go round the XCDs in order)
    some = torch.as_tensor(some, device=dev)
    view = ig.view_gain()
    view_some = {k: v.clone() for k, v in view.items()}
    pts_out = ig.view_gain(points=points)
    own = ig.geodesic(points=here)
    prop = ig.propose_goals(view["gain"], view["valid"], own["field"], KPROP, 2.0, 1.0)
    fns = {"learner": lambda: plain.step(ext, auto_reset=True),
           "geodesic_all": lambda: ig.geodesic(points=here, out=own),
           "map": lambda: ig.view_gain(out=view),
           "map_16th": lambda: ig.view_gain(world_mask=some, out=view_some),
           "points64": lambda: ig.view_gain(points=points, out=pts_out),
           "propose": lambda: ig.propose_goals(view["gain"], view["valid"], own["field"], KPROP, 2.0, 1.0, out=prop),
           "propose_goals": lambda: goal.ig_propose_goals(k=KPROP)}
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
    # the pairs a map launch traces: every valid centre's in-range cells inside the map
    n = int(np.floor(ig.range / 0.5)) + 1
    a = torch.arange(-n, n + 1, device=dev, dtype=torch.float64)
    disc = ((a[:, None] ** 2 + a[None, :] ** 2) * 0.25 < ig.range * ig.range).double()[None, None]
    cand = torch.nn.functional.conv2d(torch.ones((1, 1, 60, 60), dtype=torch.float64, device=dev), disc, padding=n)[0, 0]
    pairs = float((cand[None] * (view["valid"] != 0).double()).sum())
    visible = float(view["n_visible"].double().sum())
    res.update(worlds=N, calls_per_block=reps, pairs_per_map_launch=pairs, visible_share=round(visible / max(pairs, 1.0), 4),
               valid_share=round(float((view["valid"] != 0).double().mean()), 4),
               pairs_per_second=round(pairs / (res["map"]["us_median"] * 1e-6), 0),
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2),
               proposals_found_mean=round(float(prop["n_found"].double().mean()), 3))
    plain.close()
    goal.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks, "k": KPROP,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
