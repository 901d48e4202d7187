#!/usr/bin/env python3
"""What a planning step of the greedy information-gain policy costs at 2048 worlds x 3 robots (the scene of tools/ig_episode_cost.py:
cfg5's composition), two ways on one handle and one belief:
  fused     one cagym_ig_greedy_plan launch (InfoGain.greedy_plan);
  composed  the same plan from the entry points that existed before it: torch next-pose arithmetic and feasibility on the distance
            field, cagym_ig_visible_cells on the N x R x 9 candidates, cagym_ig_mi_reward, torch arg-max (independent mode only:
            the coordinated mode needs the robots in sequence, three times this chain).
The belief is made non-uniform by --warm env steps with the policy attached.  The two are timed alternately, --reps windows of
--iters plans each between device events, after a warm-up of both; the medians and the spread over the windows are printed as one
JSON line, with a check that both paths chose the same candidates.
usage: python tools/ig_greedy_cost.py [--worlds 2048] [--warm 8] [--reps 7] [--iters 200] [--coordinate 0]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=2048)
ap.add_argument("--warm", type=int, default=8)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--coordinate", type=int, default=0)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
igm = importlib.import_module("gym-exploration-2d_amd.ig")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

if not torch.cuda.is_available():
    raise SystemExit("ig_greedy_cost.py times kernels: it needs the GPU")
N, M, K, R = args.worlds, 20, 8, 3
a6, ob, nob, _ = scen.obstacle_worlds(N, M, K, seed=1234)
pol = np.full((N, M), scen.POLICY_NONCOOP, dtype=np.int32)
pol[:, :3] = scen.POLICY_IGMCTS
pol[:, 3:5] = scen.POLICY_STATIC
dyn = np.full((N, M), scen.DYN_UNICYCLE, dtype=np.int32)
dyn[:, :3] = scen.DYN_FIRSTORDER
env = B(N, M, max_obstacles=K, game_over_mode="all")
env.set_scenarios(a6, pol, dyn, obstacles=ob, n_obst=nob)
env.reset()
planner = env.attach_ig_greedy(coordinate=bool(args.coordinate))
for _ in range(args.warm):
    env.step(None)
g = env._igm
ig, dev = g.ig, env.device
ig.robot_inputs(R, g.range, env.obs_oas, g.poses, g.det, g.n_det)
poses = g.poses.clone()
torch.cuda.synchronize()

cand = torch.tensor([[v, w] for v in igm.GREEDY_V for w in igm.GREEDY_W], dtype=torch.float64, device=dev)  # [9,2]
world_q = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(R * 9)
d2 = ig.edf_d2  # [S,300,300] squared cell distances; S = N and no episode has ended: world w stands on scenario w
widx = torch.arange(N, device=dev)[:, None, None]


def composed():
    th = poses[..., 2:3]
    step = torch.stack([torch.cos(th) * cand[:, 0], torch.sin(th) * cand[:, 0], cand[:, 1].expand(N, R, 9)], dim=-1) * ig.dt
    nxt = poses[:, :, None, :] + step                                        # [N,R,9,3]
    idx = torch.floor((nxt[..., :2] + 15.0) / 0.1)
    inside = ((idx >= 0) & (idx < 300)).all(dim=-1)
    ci = idx.clamp(0, 299).long()
    edf = d2[widx, ci[..., 1], ci[..., 0]].double().sqrt() * 0.1
    ok = inside & (edf > planner.radius + 0.1)
    masks = ig.visible_cells(torch.where(ok[..., None], nxt, poses[:, :, None, :]).reshape(-1, 3), world_q)
    mi = torch.where(ok, ig.mi_reward(masks, world_q).reshape(N, R, 9), torch.full((), -1.0, dtype=torch.float64, device=dev))
    best, choice = mi.max(dim=-1)
    choice = torch.where(best > -1.0, choice, torch.full_like(choice, 255))
    actions = torch.where((best > -1.0)[..., None], cand[choice.clamp(max=8)], torch.zeros((), dtype=torch.float64, device=dev))
    return actions, choice, mi


out = None


def fused():
    global out
    out = ig.greedy_plan(poses, coordinate=bool(args.coordinate), radius=planner.radius, out=out)
    return out


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.iters  # ms per plan


for _ in range(3):
    fused()
    composed()
torch.cuda.synchronize()
tf, tc = [], []
for _ in range(args.reps):
    tf.append(window(fused))
    tc.append(window(composed))
res = {"worlds": N, "robots": R, "coordinate": args.coordinate, "iters": args.iters, "reps": args.reps,
       "fused_ms_median": statistics.median(tf), "fused_ms_min_max": [min(tf), max(tf)],
       "composed_ms_median": statistics.median(tc), "composed_ms_min_max": [min(tc), max(tc)],
       "feasible_share": float((fused()["mi"] >= 0).double().mean())}
if not args.coordinate:
    a, c, mi = composed()
    # torch.max returns one maximiser, not necessarily the first: compare rewards everywhere and choices where the maximum is unique
    unique = ((mi == mi.max(dim=-1, keepdim=True).values).sum(dim=-1) == 1)
    res["same_mi"] = bool(torch.equal(mi, out["mi"]))
    res["same_choice_where_unique"] = bool(torch.equal(c[unique], out["choice"].long()[unique]))
print(json.dumps(res), flush=True)
env.close()
