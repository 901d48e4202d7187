#!/usr/bin/env python3
"""Fixture of the reference's own training samplers (this container only; needs /root/reference).

Run:  python tests/golden/make_golden_samplers.py        (a few seconds)
Output: tests/golden/scenario_samplers.npz (the scenario_ prefix keeps it out of golden_util's episode groups) -- data only: 400 scenarios drawn by each of train_agents_swap_circle,
train_agents_pairwise_swap (number_of_agents=8), train_stage_1 (4) and train_stage_2 (10) of test_cases.py, executed unmodified
through ref_harness.py under fixed np.random / random seeds (unseeded branch: the counts are drawn).  Per sampler <name>:
  <name>__rows     [W, 10, 4] start x, y, goal x, y per agent (zero beyond n_agents)
  <name>__n_agents [W]        <name>__policy [W, 10] policy id (include/cagym.h), <name>__dynamics [W, 10], <name>__coop [W, 10]
  <name>__rects    [W, 10, 4] xl, yl, xu, yu per rectangle     <name>__n_obst [W]
tests/test_reference_samplers.py regenerates it into a scratch directory and compares bytes.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

OUT = os.environ.get("CAGYM_GOLDEN_OUT") or HERE
W, MAXA, MAXK = 400, 10, 10
SAMPLERS = [("train_agents_swap_circle", 8, 101), ("train_agents_pairwise_swap", 8, 202), ("train_stage_1", 4, 303),
            ("train_stage_2", 10, 404)]
POLICY_IDS = {"RVOPolicy": 5, "NonCooperativePolicy": 1, "StaticPolicy": 0}
DYNAMICS_IDS = {"UnicycleDynamics": 0, "UnicycleDynamicsMaxTurnRate": 1, "UnicycleDynamicsMaxAcc": 2, "FirstOrderDynamics": 4}


def main():
    rh.install_standins()
    from gym_collision_avoidance.envs import test_cases as tc

    class PyRVOSimulator(object):  # RVOPolicy.__init__ builds one (RVOPolicy.py:25-28); nothing of it is exercised
        def __init__(self, *a, **k):
            pass
    sys.modules["rvo2"].PyRVOSimulator = PyRVOSimulator
    arrays = {}
    for name, n_agents, seed in SAMPLERS:
        np.random.seed(seed)
        random.seed(seed)
        rows, pol, dyn = np.zeros((W, MAXA, 4)), np.zeros((W, MAXA), np.int8), np.zeros((W, MAXA), np.int8)
        coop, rects = np.zeros((W, MAXA)), np.zeros((W, MAXK, 4))
        na, no = np.zeros(W, np.int8), np.zeros(W, np.int8)
        for w in range(W):
            with rh.quiet():
                agents, obst = getattr(tc, name)(number_of_agents=n_agents, ego_agent_policy=tc.RVOPolicy,
                                                 other_agents_policy=tc.RVOPolicy)
            na[w], no[w] = len(agents), len(obst)
            for i, a in enumerate(agents):
                rows[w, i] = [a.pos_global_frame[0], a.pos_global_frame[1], a.goal_global_frame[0], a.goal_global_frame[1]]
                pol[w, i] = POLICY_IDS[type(a.policy).__name__]
                dyn[w, i] = DYNAMICS_IDS[type(a.dynamics_model).__name__]
                coop[w, i] = a.cooperation_coef
            for k, c in enumerate(obst):  # corners (xu, yu), (xl, yu), (xl, yl), (xu, yl)
                rects[w, k] = [c[2][0], c[2][1], c[0][0], c[0][1]]
        for key, v in (("rows", rows), ("n_agents", na), ("policy", pol), ("dynamics", dyn), ("coop", coop), ("rects", rects),
                       ("n_obst", no)):
            arrays[name + "__" + key] = v
    path = os.path.join(OUT, "scenario_samplers.npz")
    np.savez_compressed(path, **arrays)
    print("%-28s          %8.1f KB" % ("scenario_samplers", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
