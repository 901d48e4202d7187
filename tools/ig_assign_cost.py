#!/usr/bin/env python3
"""What the team's goal assignment costs (csrc/cagym_ig_assign.h): microseconds, on the pool of tools/ig_goals_cost.py (--agents
agents, 3 of them IG robots, 2 static targets and NonCooperative walkers among 8 rectangles) at 2048 and at 256 worlds.
  learner        attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the yardstick,
                 re-measured in the same run;
  propose        ONE cagym_ig_propose_goals launch, k = 8, on a view-gain map and the fields from the robots' places - the other
                 yardstick;
  slot / best    ONE cagym_ig_assign_goals launch on those proposals (3 robots x 8 candidates, turning on the spot), every robot
                 choosing, round_gain written, in slot order and best first;
  slot_h / best_h  the same with the proposals of ig_propose_goals(headings=8): every candidate's cell set is a sensor cone;
  cells_only     the same launch as best with k = 8 and ONE robot masked per world: 8 cell sets, one round - next to best it tells
                 what the traces of phase 1 cost and what the rounds of phase 2;
  assign_goals   env.ig_assign_goals(mode="best") as a whole: the launch, the gathers and ig_set_goals' two launches.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time (one call per block where a call
is longer than that), after --warmup untimed blocks; the figures alternate block by block, so all see the same drift of the machine.
Also reported: the cells per candidate mask and the share of robots assigned.  Prints ONE JSON line.
usage: python tools/ig_assign_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 1] [--seconds 2.0]"""
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
MODES = ("learner", "propose", "slot", "best", "slot_h", "best_h", "cells_only", "assign_goals")


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
    plain, goal = handle(N, False), handle(N, True)
    dev = goal.device
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=dev)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    for _ in range(10):  # a belief that is no longer the prior's, as a policy would meet it
        goal.step(ext, auto_reset=True)
    ig = goal._igm.ig
    st = goal.state()
    here = torch.stack((st["pos_x"][:, :R], st["pos_y"][:, :R]), dim=-1).contiguous()
    view = ig.view_gain()
    own = ig.geodesic(points=here)
    prop = ig.propose_goals(view["gain"], view["valid"], own["field"], KPROP, 2.0, 1.0)
    headed = {k: v.clone() for k, v in goal.ig_propose_goals(k=KPROP, headings=8).items() if k in ("xy", "distance", "heading")}
    one = torch.zeros((N, R), dtype=torch.uint8, device=dev)
    one[:, 0] = 1
    outs = {m: None for m in ("slot", "best", "slot_h", "best_h", "cells_only")}

    def assign(name, mode, cand, mask=None):
        outs[name] = ig.assign_goals(cand["xy"], cand["distance"], cand_heading=cand.get("heading"), mask=mask, mode=mode, out=outs[name])

    fns = {"learner": lambda: plain.step(ext, auto_reset=True),
           "propose": lambda: ig.propose_goals(view["gain"], view["valid"], own["field"], KPROP, 2.0, 1.0, out=prop),
           "slot": lambda: assign("slot", "slot", prop), "best": lambda: assign("best", "best", prop),
           "slot_h": lambda: assign("slot_h", "slot", headed), "best_h": lambda: assign("best_h", "best", headed),
           "cells_only": lambda: assign("cells_only", "best", prop, one),
           "assign_goals": lambda: goal.ig_assign_goals(mode="best")}
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
    pop = lambda o: float(np.unpackbits(o["masks"].cpu().numpy().view(np.uint8), axis=-1).sum(axis=-1).mean())
    res.update(worlds=N, calls_per_block=reps, cells_per_mask=round(pop(outs["best"]), 1), cells_per_cone=round(pop(outs["best_h"]), 1),
               assigned_share={m: round(float((outs[m]["choice"] >= 0).double().mean()), 4) for m in ("slot", "best", "slot_h", "best_h")},
               team_gain_mean={m: round(float(outs[m]["marginal"].sum(dim=1).mean()), 4) for m in ("slot", "best", "slot_h", "best_h")},
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2))
    plain.close()
    goal.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks, "k": KPROP,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
