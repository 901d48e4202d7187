"""Time a fresh stage-2 scenario pool: on the device (cagym_generate_reference_scenarios, HIP events) against the host sampler
scenarios.obstacle_worlds + set_scenarios (wall clock, upload and prep rows included).  S = 8192, M = 10, K = 10 by default.

    python tools/gen_time.py [--S 8192] [--M 10] [--K 10] [--reps 20] [--host-reps 2] [--max-tries 1000] [--out FILE.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=8192)
    ap.add_argument("--M", type=int, default=10)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--max-tries", type=int, default=1000)  # generate_reference_scenarios' default
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    env = B(a.S, a.M, n_scenarios=a.S, max_obstacles=a.K)
    kw = dict(ego_policy=scen.POLICY_GA3C, other_policies=(scen.POLICY_RVO, scen.POLICY_NONCOOP), p_b=0.2, max_tries=a.max_tries)
    failed = env.generate_reference_scenarios("train_stage_2", 0, **kw)  # warm-up (module load, first launch)
    dev_ms = []
    for r in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        env.generate_reference_scenarios("train_stage_2", r + 1, check=False, **kw)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    failed_last = env.generate_reference_scenarios("train_stage_2", a.reps, **kw)
    n_obst = env.obstacles()["n_obst"].cpu().numpy()
    host_ms, sample_ms = [], []
    for r in range(a.host_reps):
        t0 = time.perf_counter()
        a6, obst, nob, na = scen.obstacle_worlds(a.S, a.M, a.K, seed=r)
        t1 = time.perf_counter()
        pol = np.full((a.S, a.M), scen.POLICY_RVO, np.int32)
        env.set_scenarios(a6, pol, scen.DYN_UNICYCLE, n_agents=na, obstacles=obst, n_obst=nob)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sample_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t0) * 1e3)
    res = {"S": a.S, "M": a.M, "K": a.K, "kind": "train_stage_2", "max_tries": a.max_tries, "device": torch.cuda.get_device_name(),
           "device_ms_median": float(np.median(dev_ms)), "device_ms_min": float(np.min(dev_ms)), "device_ms_max": float(np.max(dev_ms)),
           "device_reps": a.reps, "n_failed": [failed, failed_last], "mean_n_obst": float(n_obst.mean()),
           "host_obstacle_worlds_ms": sample_ms, "host_total_ms": host_ms,
           "host_note": "scenarios.obstacle_worlds + set_scenarios (upload, host prep rows, raster), wall clock"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
