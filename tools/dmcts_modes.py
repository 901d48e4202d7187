#!/usr/bin/env python3
"""The Dec-MCTS planning step of cfg5 (3 robots, Ntree 30, Nsims 10, horizon 4, Ncycles 5) in both planning modes: sequential
(k_dmcts_plan, one workgroup per world) and agent-parallel (k_dmcts_plan_cycle, one workgroup per world and robot, one launch per
cycle).  Prints one JSON line per mode with the wall time of a planning step by HIP events (median of --reps); run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own times (tools/dmcts_modes.sh).
usage: python tools/dmcts_modes.py [--worlds 2048] [--reps 5] [--modes seq,par]   (CAGYM_LIB selects another library build)"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
IG = importlib.import_module("gym-exploration-2d_amd.ig").InfoGain
dmm = importlib.import_module("gym-exploration-2d_amd.dmcts")

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=2048)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--modes", default="seq,par")
args = ap.parse_args()

N, M, K, R = args.worlds, 20, 8, 3  # the scene of tools/dmcts_phases.py (cfg5's composition)
S = 2 * N
a6, ob, nob, _ = scen.obstacle_worlds(S, M, K, seed=1234)
pol = np.full((S, M), scen.POLICY_NONCOOP, dtype=np.int32)
pol[:, :3] = scen.POLICY_IGMCTS
pol[:, 3:5] = scen.POLICY_STATIC
dyn = np.full((S, M), scen.DYN_UNICYCLE, dtype=np.int32)
dyn[:, :3] = scen.DYN_FIRSTORDER
env = B(N, M, n_scenarios=S, max_obstacles=K, game_over_mode="all")
env.set_scenarios(a6, pol, dyn, obstacles=ob, n_obst=nob)
env.reset()
ig = IG(env)
st = env.state()
poses = torch.stack([st["pos_x"][:, :R], st["pos_y"][:, :R], st["heading"][:, :R]], dim=2).contiguous()
for mode in args.modes.split(","):
    planner = dmm.DeviceDecMCTSPlanner(ig, R, radius=0.5, Ntree=30, Nsims=10, horizon=4, c_p=1.0, gamma=0.95, Ncycles=5, seed=1,
                                       parallelize_agents=(mode == "par"))
    planner.plan(poses)  # warm-up (and the previous step's plans for the timed ones)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        planner.plan(poses)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"mode": mode, "worlds": N, "robots": R, "plan_ms_median": float(np.median(ms)), "plan_ms": ms,
                      "lib": os.environ.get("CAGYM_LIB", "default")}), flush=True)
    del planner
env.close()
