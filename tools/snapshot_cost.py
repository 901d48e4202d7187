#!/usr/bin/env python3
"""What snapshot, restore and fork (csrc/cagym_snapshot.h) cost at the flagship size, next to the same handle's one-step launch:
4096 worlds x 10 RVO agents, in free space and with 10 rectangles + LaserScan.  Timed per configuration:
  step            env.step(auto_reset=True), the one-step launch
  snapshot_abi    cagym_snapshot of every world into a preallocated blob (the copy kernel alone)
  restore_abi     cagym_restore of every row of that blob
  fork_abi        cagym_fork, every 12th world into its 11 successors (two launches: state rows, pool rows)
  snapshot / restore / fork   the Python methods: the ABI call plus the rows of the env-owned output tensors (fork: device
                  lists with check=False, i.e. masked output-row copies; fork_host_lists: numpy lists, validated on the host)
Each figure is the median over --blocks blocks of --reps calls between two HIP events (after --warmup untimed blocks), in
microseconds per call, with the fastest and slowest block beside it.  Prints one JSON line per configuration.
usage: python tools/snapshot_cost.py [--worlds 4096] [--agents 10] [--reps 200] [--blocks 9] [--warmup 2]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
_lib = importlib.import_module("gym-exploration-2d_amd._lib")

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
N, M = args.worlds, args.agents


def timed(fn):
    us = []
    for b in range(args.warmup + args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        if b >= args.warmup:
            us.append(1e3 * e0.elapsed_time(e1) / args.reps)
    return {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def measure(K, laser):
    env = B(N, M, n_scenarios=N, max_obstacles=K, laserscan=laser, game_over_mode="all")
    if K:
        a6, obst, n_obst, _ = scen.obstacle_worlds(N, M, K, seed=1234)
    else:
        a6, obst, n_obst = scen.random_worlds_fast(N, M, seed=1234), None, None
    env.set_scenarios(a6, scen.POLICY_RVO, scen.DYN_UNICYCLE, coop=np.full((N, M), 0.5), obstacles=obst, n_obst=n_obst)
    env.reset()
    for _ in range(50):
        env.step(auto_reset=True)
    heads = torch.arange(0, N - 11, 12, device=env.device)
    src = heads.repeat_interleave(11).to(torch.int32)
    dst = (heads[:, None] + 1 + torch.arange(11, device=env.device)[None, :]).reshape(-1).to(torch.int32)
    snap = env.snapshot()
    L, h, st = env.L, env.h, env._stream
    res = {"worlds": N, "agents": M, "max_obstacles": K, "laserscan": bool(laser), "row_bytes": int(snap.layout.row_bytes),
           "blob_mb": round(snap.blob.numel() / 1e6, 2), "fork_pairs": int(src.numel()), "reps": args.reps, "blocks": args.blocks}
    res["step"] = timed(lambda: env.step(auto_reset=True))
    res["snapshot_abi"] = timed(lambda: _lib.call(L, h, "cagym_snapshot", None, N, snap.blob.data_ptr(), st()))
    res["restore_abi"] = timed(lambda: _lib.call(L, h, "cagym_restore", snap.layout, snap.blob.data_ptr(), None, N, st()))
    res["fork_abi"] = timed(lambda: _lib.call(L, h, "cagym_fork", src.data_ptr(), dst.data_ptr(), src.numel(), st()))
    res["snapshot"] = timed(lambda: env.snapshot())
    res["restore"] = timed(lambda: env.restore(snap))
    res["fork"] = timed(lambda: env.fork(src, dst, check=False))
    hs, hd = src.cpu().numpy(), dst.cpu().numpy()
    res["fork_host_lists"] = timed(lambda: env.fork(hs, hd))
    env.close()
    return res


for K, laser in ((0, False), (10, True)):
    print(json.dumps(measure(K, laser)), flush=True)
