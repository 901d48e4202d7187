#!/usr/bin/env python3
"""Diagnostic (never the shipped library): who arrives last at the step's barrier X - wave 0 with S1, or a row wave with the
OtherAgentsStates rows of the step before (-DCAGYM_XTRACE: two stamps per wave and step, 8 workgroups, the 512 steps of a launch of
the headline shape).  Prints, over all traced steps, the share of steps in which a row wave is last, the gap between the last row
wave and wave 0 (positive: the rows are later), and how long wave 0 stands at the barrier.
usage: python tools/barrier_x.py [launches]        (XT_DEFS: further -D flags for the diagnostic unit)"""
import ctypes, importlib, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
b = importlib.import_module("gym-exploration-2d_amd.build")
import torch
if "--child" not in sys.argv:
    LIB = b.build_variant("xtrace", ["-DCAGYM_XTRACE"] + os.environ.get("XT_DEFS", "").split())
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], env=dict(os.environ, CAGYM_LIB=LIB)))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
args = [a for a in sys.argv[1:] if a != "--child"]
N, M, T, WGS, LAUNCHES = 4096, 10, 512, 8, int(args[0]) if args else 6
env = B(N, M, n_scenarios=8 * N, game_over_mode="all")
env.set_scenarios(scen.random_worlds_fast(8 * N, M, seed=1234), scen.POLICY_RVO, scen.DYN_UNICYCLE, coop=np.full((8 * N, M), 0.5))
env.reset()
traj = env.alloc_rollout(T)
for _ in range(2):
    env.rollout(T, out=traj)
acc = []
for rep in range(LAUNCHES):
    env.rollout(T, out=traj)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (WGS * T * 8))()
    env.L.cagym_debug_xtrace(buf)
    acc.append(np.frombuffer(buf, dtype=np.uint64).reshape(WGS, T, 8).astype(np.int64)[:, 1:, :5])  # step 0 has no rows to write
X = np.concatenate(acc, axis=1)  # [workgroup, step, (wave 0: S1 done, waves 1-3: rows done, wave 0 behind X)]
s1, rows, behind = X[:, :, 0], X[:, :, 1:4].max(axis=2), X[:, :, 4]
gap = rows - s1
print("%d worlds x %d agents, %d launches of %d steps, workgroups 0, 128, .., 896; s_memtime ticks" % (N, M, LAUNCHES, T))
print("%-10s %8s %16s %12s %12s %12s %14s" % ("workgroup", "steps", "row wave last %", "gap median", "gap p10", "gap p90", "w0 at X median"))
for w in list(range(WGS)) + [None]:
    g, wt = (gap[w], (behind - s1)[w]) if w is not None else (gap.ravel(), (behind - s1).ravel())
    print("%-10s %8d %16.1f %12.0f %12.0f %12.0f %14.0f" % ("all" if w is None else 128 * w, g.size, 100.0 * (g > 0).mean(), np.median(g),
                                                         np.percentile(g, 10), np.percentile(g, 90), np.median(wt)))
late = gap[gap > 0]
print("steps with a row wave last: median lateness %.0f ticks; steps with wave 0 last: median slack of the rows %.0f ticks"
      % (np.median(late) if late.size else 0.0, -np.median(gap[gap <= 0]) if (gap <= 0).any() else 0.0))
