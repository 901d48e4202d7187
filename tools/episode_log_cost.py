#!/usr/bin/env python3
"""What the append-only episode log (csrc/cagym_episode_log.h) costs at the flagship size, 4096 worlds x 10 agents in free space
(train_agents_swap_circle, every agent RVO): microseconds per env.step(auto_reset=True) and per env.rollout(--rollout) call with
the log attached and detached, on a fixed pool and while streaming (ring of --depth slots per world).  The attached call adds the
log's launches behind the step(s): scan + write for a one-step call, count + scan + write for a roll-out.
Each figure is the median over --blocks blocks of calls between two HIP events (after --warmup untimed blocks), with the fastest and
slowest block beside it; attached and detached blocks alternate, on two handles built from the same arguments.  The detached handle
runs exactly the parent's launches (the step, roll-out and refill kernels are unchanged: tools/kernel_asm_diff.py), so it is the
yardstick.  `update_alone` times cagym_episode_log_update by itself on one slice in which nothing finished.  Prints one JSON line per pool.
usage: python tools/episode_log_cost.py [--worlds 4096] [--agents 10] [--depth 4] [--rollout 512] [--reps 2000] [--rollout-reps 16]
                                        [--blocks 7] [--warmup 2] [--capacity 65536]"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=4096)
ap.add_argument("--agents", type=int, default=10)
ap.add_argument("--depth", type=int, default=4)
ap.add_argument("--rollout", type=int, default=512)
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--rollout-reps", type=int, default=16)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--capacity", type=int, default=65536)
args = ap.parse_args()
N, M = args.worlds, args.agents


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


def measure(pool):
    gen = dict(kinds="train_agents_swap_circle", seed=1, other_policies=scen.POLICY_RVO)
    envs = {}
    for mode in ("detached", "attached"):
        env = B(N, M, n_scenarios=args.depth * N, game_over_mode="agent0")
        (env.stream_reference_scenarios if pool == "streaming" else env.generate_reference_scenarios)(**gen)
        env.reset()
        if mode == "attached":
            env.attach_episode_log(args.capacity)
        envs[mode] = env
    res = {"pool": pool, "worlds": N, "agents": M, "depth": args.depth, "capacity": args.capacity, "blocks": args.blocks}
    bufs = {mode: env.alloc_rollout(args.rollout, obs=False) for mode, env in envs.items()}
    calls = (("step", args.reps, lambda env, mode: env.step(auto_reset=True)),
             ("rollout%d" % args.rollout, args.rollout_reps, lambda env, mode: env.rollout(args.rollout, auto_reset=True, out=bufs[mode])))
    for name, reps, fn in calls:
        us = {"detached": [], "attached": []}
        for b in range(args.warmup + args.blocks):
            for mode, env in envs.items():  # alternated: both see the same drift of the machine
                t = block(lambda: fn(env, mode), reps)
                if b >= args.warmup:
                    us[mode].append(t)
        res[name] = {mode: summary(v) for mode, v in us.items()}
        res[name]["added_us"] = round(res[name]["attached"]["us_median"] - res[name]["detached"]["us_median"], 2)
    env = envs["attached"]
    head = int(env.episode_log_views()["head"])
    res["episodes_logged"] = head
    # the update by itself, one slice with no finished episode (restart first: the feed is out of step on purpose, nothing is read back)
    quiet = torch.zeros((N,), dtype=torch.uint8, device=env.device)
    one = lambda: env._log_fn(env.h, env.flags.data_ptr(), env.reward.data_ptr(), quiet.data_ptr(), 1, env._stream())  # noqa: E731
    res["update_alone"] = summary([block(one, args.reps) for _ in range(args.warmup + args.blocks)][args.warmup:])
    if pool == "streaming":
        res["n_lapped"] = env.stream_stats()["n_lapped"]
    for env in envs.values():
        env.close()
    return res


for pool in ("fixed", "streaming"):
    print(json.dumps(measure(pool)), flush=True)
