#!/usr/bin/env python3
"""What a whole-env checkpoint (csrc/cagym_checkpoint.h) costs at the flagship size, next to the same handle's one-step launch:
4096 worlds x 10 agents on a scenario stream of depth 3 with an episode log (65536 rows) and a replay buffer (4096 keys), in free
space and with up to 10 rectangles + LaserScan.  Timed per configuration:
  step         env.step(auto_reset=True): the one-step launch with the log update, the harvest and the refill behind it
  save_abi     cagym_checkpoint_save into preallocated buffers (three copy launches)
  load_abi     cagym_checkpoint_load of those buffers into the same handle (the three copies plus the raster launch)
  checkpoint / load_checkpoint   the Python methods: the ABI call plus the blob's allocation and the env-owned output tensors
Each figure is the median over --blocks blocks of --reps calls between two HIP events (after --warmup untimed blocks), in
microseconds per call, with the fastest and slowest block beside it.  Prints one JSON line per configuration.
usage: python tools/checkpoint_cost.py [--worlds 4096] [--agents 10] [--depth 3] [--reps 100] [--blocks 9] [--warmup 2]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
_lib = importlib.import_module("gym-exploration-2d_amd._lib")

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--depth", type=int, default=3)
ap.add_argument("--reps", type=int, default=100)
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
    env = B(N, M, n_scenarios=args.depth * N, max_obstacles=K, laserscan=laser, game_over_mode="agent0")
    kinds = ["train_stage_1", "train_stage_2"] if K else ["train_agents_swap_circle", "train_agents_pairwise_swap", "train_agents_random_positions"]
    env.stream_reference_scenarios(kinds, 1234, n_obst=(-1, K) if K else None, check=False)
    env.attach_episode_log(65536)
    env.attach_replay(capacity=4096, p=0.25, outcomes=("collision", "stuck"), seed=1)
    env.reset()
    for _ in range(50):
        env.step(auto_reset=True)
    ckpt = env.checkpoint()
    L, h, st = env.L, env.h, env._stream
    hp, hn, bp, bn = ckpt.header.data_ptr(), ckpt.header.numel(), ckpt.blob.data_ptr(), ckpt.blob.numel()
    res = {"worlds": N, "agents": M, "depth": args.depth, "max_obstacles": K, "laserscan": bool(laser),
           "section_bytes": dict(zip(_lib.CKPT_SECTIONS, ckpt.sizes)), "blob_mb": round(bn / 1e6, 2), "reps": args.reps, "blocks": args.blocks}
    res["step"] = timed(lambda: env.step(auto_reset=True))
    res["save_abi"] = timed(lambda: _lib.call(L, h, "cagym_checkpoint_save", hp, hn, bp, bn, st()))
    res["load_abi"] = timed(lambda: _lib.call(L, h, "cagym_checkpoint_load", hp, hn, bp, bn, st()))
    res["checkpoint"] = timed(lambda: env.checkpoint())
    res["load_checkpoint"] = timed(lambda: env.load_checkpoint(ckpt))
    env.close()
    return res


for K, laser in ((0, False), (10, True)):
    print(json.dumps(measure(K, laser)), flush=True)
