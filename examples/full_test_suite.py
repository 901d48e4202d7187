#!/usr/bin/env python3
"""The reference's test suite (experiments/src/run_full_test_suite.py + process_full_test_suite_pickles.py) on the device: ONE pool
of test cases (random positions, radius 0.2, pref_speed 1: the suite's vpref1.0_r0.2-0.2 setting) run under NonCooperative, RVO
and - if its weights load - GA3C-CADRL, every agent of a case running the policy under test (homogeneous testing, game over when
all agents are done).  Each policy steps its worlds with auto-reset and episode records attached (keep="first") until every case
has a record, then stats.suite_statistics turns the table into the two lines the reference prints per policy:
    <pct collision + pct stuck> (<pct collision> / <pct stuck>)
    <50th> / <75th> / <90th> percentile of the mean extra time to goal
the percentiles over the cases NO policy collided or got stuck in (the intersection of their clean rows), as the reference takes
them.  The goal radius is the kernels' 0.75 m (the reference's suite script sets 0.8).

usage: python examples/full_test_suite.py [--worlds 256] [--cases 500] [--agents 4] [--seed 1] [--block 32]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
stats = importlib.import_module("gym-exploration-2d_amd.stats")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=256)
ap.add_argument("--cases", type=int, default=500)
ap.add_argument("--agents", type=int, default=4)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--block", type=int, default=32, help="steps per rollout between two looks at the table")
args = ap.parse_args()

N, S, M = args.worlds, max(args.cases, args.worlds), args.agents
a6 = scen.random_worlds_fast(S, M, seed=args.seed, radius=0.2)


def run(policy, dynamics, ga3c=False):
    env = B(N, M, n_scenarios=S, game_over_mode="all")
    env.set_scenarios(a6, policy, dynamics)
    if ga3c:
        env.attach_ga3c()
    env.reset()
    env.attach_episode_records(keep="first")
    out = env.alloc_rollout(args.block, obs=False)
    steps = 0
    while True:
        env.rollout(args.block, auto_reset=True, out=out)
        steps += args.block
        rec = env.episode_records()
        if int(rec["count"].min()) >= 1:
            break
        if steps > 100000:
            raise RuntimeError("the suite did not complete: %d cases without a record" % int((rec["count"] == 0).sum()))
    table = {k: v.clone() for k, v in rec.items()}
    env.close()
    return table, steps


policies = [("NonCooperative", scen.POLICY_NONCOOP, scen.DYN_UNICYCLE, False), ("RVO", scen.POLICY_RVO, scen.DYN_UNICYCLE, False)]
try:
    ga3c_dir = os.path.dirname(importlib.import_module("gym-exploration-2d_amd.ga3c").__file__)
    assert np.load(os.path.join(ga3c_dir, "weights", "ga3c_cadrl_iros18.npz")).files
    policies.append(("GA3C-CADRL", scen.POLICY_GA3C, scen.DYN_UNICYCLE, True))
except Exception as exc:  # the suite runs without the learned policy
    print("GA3C-CADRL skipped: %s" % exc)

tables = {}
for name, pol, dyn, ga3c in policies:
    tables[name], steps = run(pol, dyn, ga3c)
    print("%s: %d cases x %d agents recorded in %d steps of %d worlds" % (name, S, M, steps, N))
clean = None
for name in tables:
    c = stats.suite_statistics(tables[name])["clean"]
    clean = c if clean is None else clean & c
print("cases every policy finished without collision or stuck agent: %d of %d" % (int(clean.sum()), S))
for name in tables:
    st = stats.suite_statistics(tables[name], include=clean)
    print("---\nPolicy: %s" % name)
    print("{:.2f} ({:.2f} / {:.2f})".format(st["pct_collision"] + st["pct_stuck"], st["pct_collision"], st["pct_stuck"]))
    print(" / ".join("%.2f" % float(v) for v in st["extra_time_pctls"].cpu()))
