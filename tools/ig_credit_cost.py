#!/usr/bin/env python3
"""What the per-robot credit costs (csrc/cagym_ig_credit.h): microseconds per auto-resetting learner step of --agents agents, 3 of
them IG robots driven at a constant (v, omega), 2 static targets and NonCooperative walkers among rectangles (the cfg5 pool of
tools/ig_learner_cost.py), at 2048 and at 256 worlds, on two handles built from the same arguments:
  learner  attach_ig_learner(window): step(auto_reset=True) = the step launch + ONE cagym_ig_observe - the path as it was before
           the credit existed, the yardstick, re-measured in the same run;
  credit   the same + attach_ig_credit(): ONE cagym_ig_credit behind the observe launch;
and, on the credit handle's state, the launches alone, back to back in blocks of their own:
  observe_alone    InfoGain.observe with NULL outputs but the window (the belief moves on: one more observation per call);
  credit_alone     InfoGain.robot_credit into the env's tensors (it writes nothing of the handle);
  credit_skeleton  the same launch with a sensing range of a micrometre: every cell set is empty, what remains is the robot
                   inputs, the barriers and the 3R + 1 reduction trees;
  traces_alone     the R visibility traces as N * R single queries of cagym_ig_visible_cells (128 threads each).
Each figure is the median over --blocks blocks of calls between two HIP events, with the fastest and slowest block beside it; the
block length is calibrated so that a figure's timed blocks cover at least --seconds of device time, after --warmup untimed blocks;
the handles alternate block by block, so both see the same drift of the machine.  Prints ONE JSON line.
usage: python tools/ig_credit_cost.py [--worlds 2048,256] [--agents 20] [--window 24] [--blocks 7] [--warmup 2] [--seconds 2.0]"""
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
MODES = ("learner", "credit")


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
    env.attach_ig_learner(window=args.window, rotate=True)
    if mode == "credit":
        env.attach_ig_credit()
    env.reset()
    ext = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)
    ext[:, :R, 0], ext[:, :R, 1] = 1.0, 0.5
    return env, lambda: env.step(ext, auto_reset=True)


def timed(fns, per_call):
    """{name: [us per block]} of the callables, alternating block by block"""
    reps = max(20, int(args.seconds * 1e6 / (args.blocks * per_call)) + 1)
    us = {name: [] for name in fns}
    for b in range(args.warmup + args.blocks):
        for name, fn in fns.items():
            t = block(fn, reps)
            if b >= args.warmup:
                us[name].append(t)
    return us, reps


def measure(N):
    made = {mode: handle(N, mode) for mode in MODES}
    for _, fn in made.values():
        block(fn, 50)  # (first launches load code objects)
    per_call = min(block(fn, 50) for _, fn in made.values())
    us, reps = timed({mode: fn for mode, (_, fn) in made.items()}, per_call)
    res = {mode: summary(v) for mode, v in us.items()}
    res.update(worlds=N, calls_per_block=reps, timed_seconds={mode: round(sum(v) * reps * 1e-6, 2) for mode, v in us.items()},
               credit_added_us=round(res["credit"]["us_median"] - res["learner"]["us_median"], 2),
               learner_spread_us=round(res["learner"]["us_max"] - res["learner"]["us_min"], 2),
               episodes_finished={mode: int(env.state()["stat_episodes"].sum().item()) for mode, (env, _) in made.items()})
    # the two launches alone, on the state the credit handle stands in
    env = made["credit"][0]
    g, q = env._igm, env._credit
    # where the launch's time goes: the same launch with a sensing range of a micrometre (every cell set empty: the robot inputs,
    # the barriers and the 3R + 1 reduction trees remain), and the R traces as N * R single queries of cagym_ig_visible_cells
    total = float(q.out["gain"].sum())  # (of the last step: the alone runs below wear the belief out)
    share = {"%s_share" % k: round(float(q.out["credit"][:, :, c].sum()) / total, 4) if total > 0 else None
             for c, k in enumerate(("own", "exclusive", "difference"))}  # the robots' credit over the team's gain, summed over the worlds
    scratch = {k: torch.zeros_like(v) for k, v in q.out.items()}
    st = env.state()
    poses = torch.stack([st["pos_x"][:, :R], st["pos_y"][:, :R], st["heading"][:, :R]], dim=2).reshape(-1, 3).contiguous()
    world = torch.arange(N, dtype=torch.int32, device=env.device).repeat_interleave(R)
    alone = {"observe_alone": lambda: g.ig.observe(g.R, g.range, env.obs_oas, g.window, g.rotate, belief_window=g.belief_window),
             "credit_alone": lambda: g.ig.robot_credit(g.R, g.range, env.obs_oas, None, 0, q.out, None),
             "credit_skeleton": lambda: g.ig.robot_credit(g.R, g.range, env.obs_oas, None, 0, scratch, None, range=1e-6),
             "traces_alone": lambda: g.ig.visible_cells(poses, world)}
    for fn in alone.values():
        block(fn, 20)
    us2, reps2 = timed(alone, min(block(fn, 20) for fn in alone.values()))
    res.update({name: summary(v) for name, v in us2.items()})
    res.update(calls_per_block_alone=reps2, **share)
    for e, _ in made.values():
        e.close()
    return res


out = {"agents": M, "robots": R, "window": args.window, "blocks": args.blocks, "shapes": [measure(int(n)) for n in args.worlds.split(",")]}
print(json.dumps(out), flush=True)
