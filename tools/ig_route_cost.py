#!/usr/bin/env python3
"""What the route gains cost (csrc/cagym_ig_route.h): microseconds, on the pool of tools/ig_assign_cost.py (--agents agents, 3 of
them IG robots, 2 static targets and NonCooperative walkers among 8 rectangles) at 2048 and at 256 worlds.
  learner        attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the yardstick,
                 re-measured in the same run;
  propose_goals  env.ig_propose_goals(k = 8) as a whole: the view-gain map, the fields from the robots' places, the proposals;
  assign         ONE cagym_ig_assign_goals launch (best first) on those proposals, 3 robots x 8 candidates turning on the spot;
  route_s4 / route_s1      ONE cagym_ig_route_gains launch on the same proposals and the robots' own fields, stride 4 and stride 1;
  route_s4_h / route_s1_h  the same on the proposals of ig_propose_goals(headings=8): the candidate's own set is a sensor cone;
  views_only     the stride-4 launch with candidates that are all the robots' own cells (n = 0): no walk, no way-point - next to
                 route_s4 it tells what the staging, the 24 own views (a robot turning on the spot) and their prices cost;
  route_gains    env.ig_route_gains(stride=4) as a whole: the launch and the gathers.
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time (one call per block where a call
is longer than that), after --warmup untimed blocks; the figures alternate block by block, so all see the same drift of the machine.
Also reported: path moves and way-points per candidate, the truncated share, the cells per route mask, and how often the route-priced
best is not the first proposal.  Prints ONE JSON line.
usage: python tools/ig_route_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 1] [--seconds 2.0]"""
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
ROUTES = ("route_s4", "route_s1", "route_s4_h", "route_s1_h")
MODES = ("learner", "propose_goals", "assign") + ROUTES + ("views_only", "route_gains")


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
    keep = ("cells", "xy", "distance", "heading")
    headed = {k: v.clone() for k, v in goal.ig_propose_goals(k=KPROP, headings=8).items() if k in keep}
    plainp = {k: v.clone() for k, v in goal.ig_propose_goals(k=KPROP).items() if k in keep}  # (the last call: route_gains prices these)
    field = goal._goals.own["field"]
    st = goal.state()
    own_cells = torch.stack((torch.floor((st["pos_x"][:, :R] + 15.0) / 0.5), torch.floor((st["pos_y"][:, :R] + 15.0) / 0.5)), dim=-1)
    own_cells = own_cells.to(torch.int32)[:, :, None, :].expand(N, R, KPROP, 2).contiguous()
    outs = {m: None for m in ROUTES + ("views_only", "assign")}

    def route(name, cand, stride, cells=None):
        outs[name] = ig.route_gains(field, cand["cells"] if cells is None else cells, cand_heading=cand.get("heading"), stride=stride, out=outs[name])

    def assign():
        outs["assign"] = ig.assign_goals(plainp["xy"], plainp["distance"], mode="best", out=outs["assign"])

    fns = {"learner": lambda: plain.step(ext, auto_reset=True),
           "propose_goals": lambda: goal.ig_propose_goals(k=KPROP),
           "assign": assign,
           "route_s4": lambda: route("route_s4", plainp, 4), "route_s1": lambda: route("route_s1", plainp, 1),
           "route_s4_h": lambda: route("route_s4_h", headed, 4), "route_s1_h": lambda: route("route_s1_h", headed, 1),
           "views_only": lambda: route("views_only", plainp, 4, own_cells),
           "route_gains": lambda: goal.ig_route_gains(stride=4)}
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
    pop = lambda t: float(np.unpackbits(t.cpu().numpy().view(np.uint8), axis=-1).sum(axis=-1).mean())
    shape = {}
    for m in ROUTES:
        o = outs[m]
        ok = o["n_path"] >= 0
        shape[m] = {"routes_share": round(float(ok.double().mean()), 4), "moves_mean": round(float(o["n_path"][ok].double().mean()), 2),
                    "waypoints_mean": round(float(o["n_way"][ok].double().mean()), 2),
                    "truncated_share": round(float((o["truncated"][ok] != 0).double().mean()), 4),
                    "cells_per_route": round(pop(o["route_masks"]), 1), "cells_per_total": round(pop(o["total_masks"]), 1),
                    "best_not_first_share": round(float((o["best"] > 0).double().mean()), 4),
                    "no_best_share": round(float((o["best"] < 0).double().mean()), 4)}
    res.update(worlds=N, calls_per_block=reps, routes=shape, learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2))
    plain.close()
    goal.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks, "k": KPROP,
       "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
