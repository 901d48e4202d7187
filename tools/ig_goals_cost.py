#!/usr/bin/env python3
"""What goal actions cost (csrc/cagym_ig_geodesic.h): microseconds, on the pool of tools/ig_context_cost.py (--agents agents, 3 of
them IG robots, 2 static targets and NonCooperative walkers among 8 rectangles) at 2048 and at 256 worlds.
  learner       attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the yardstick,
                re-measured in the same run;
  goals         the same handle kind with attach_ig_goals and a goal on every robot: + cagym_ig_goal_actions in front of the step
                (on a copy of the caller's table) + cagym_ig_goal_status behind the observe launch (a restarted world loses its
                goals; the loop hands the flags back every 16th step and reports the share of robots that held one at a block's end);
  geodesic_all  ONE cagym_ig_geodesic launch for all N x 3 robots (ig_set_goals' launch, without its status launch), goals drawn
                uniformly over the map;
  geodesic_16th the same launch with one robot in sixteen flagged in its mask - what a loop that re-targets robots as they arrive
                pays per step.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time, after --warmup untimed blocks;
the four alternate block by block, so all see the same drift of the machine.  Also reported: the relaxation sweeps per field
(min, median, max) and the share of goals with a source cell.  Prints ONE JSON line.
usage: python tools/ig_goals_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 2] [--seconds 2.0]"""
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
MODES = ("learner", "goals", "geodesic_all", "geodesic_16th")


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
    points = torch.as_tensor(rng.uniform(-14.0, 14.0, (N, R, 2)), device=dev)
    some = np.zeros(N * R, dtype=np.uint8)
    some[rng.choice(N * R, size=N * R // 16, replace=False)] = 1  # (drawn, not every sixteenth: workgroups go round the XCDs in order)
    some = torch.as_tensor(some.reshape(N, R), device=dev)
    ig = goal._igm.ig
    out = dict(goal._goals.out, sweeps=torch.zeros((N, R), dtype=torch.int32, device=dev))

    goal.ig_set_goals(points)
    saved, count = goal._goals.out["active"].clone(), [0]

    def stepped():
        # auto-reset takes a finished world's goals away; every 16th call hands the flags back (one 6 KB copy, on fields of the
        # world's last map: the cost of the two launches is the same), so that the controller has work in nearly every world
        count[0] += 1
        if count[0] % 16 == 0:
            goal._goals.out["active"].copy_(saved)
        goal.step(ext, auto_reset=True)

    fns = {"learner": lambda: plain.step(ext, auto_reset=True), "goals": stepped,
           "geodesic_all": lambda: ig.geodesic(points=points, out=out), "geodesic_16th": lambda: ig.geodesic(points=points, mask=some, out=out)}
    for fn in fns.values():
        block(fn, 50)  # (first launches load code objects)
    per_call = {k: block(fn, 50) for k, fn in fns.items()}
    reps = {k: max(20, int(args.seconds * 1e6 / (args.blocks * t)) + 1) for k, t in per_call.items()}
    us = {mode: [] for mode in MODES}
    active_share = []
    for b in range(args.warmup + args.blocks):
        for mode in MODES:
            if mode == "goals":
                goal.ig_set_goals(points)  # (untimed: every robot of every world holds a goal when the block starts)
            t = block(fns[mode], reps[mode])
            if mode == "goals":
                active_share.append(float((goal.ig_goals()["active"] != 0).float().mean()))
            if b >= args.warmup:
                us[mode].append(t)
    res = {mode: summary(v) for mode, v in us.items()}
    ig.geodesic(points=points, out=out)
    torch.cuda.synchronize()
    sw = out["sweeps"].cpu().numpy().ravel()
    sw = sw[out["active"].cpu().numpy().ravel() != 0]
    res.update(worlds=N, calls_per_block=reps, goals_added_us=round(res["goals"]["us_median"] - res["learner"]["us_median"], 2),
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2),
               goals_active_share_at_block_end=round(min(active_share), 3),
               sweeps={"min": int(sw.min()), "median": float(np.median(sw)), "max": int(sw.max())},
               source_share=round(float((out["active"] != 0).float().mean()), 3), field_bytes=out["field"].numel() * 4)
    plain.close()
    goal.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
