"""Train-style driver loop on STREAMED scenarios (cagym_stream_scenarios / cagym_stream_refill): the reference draws a fresh world
at every reset() from the scenario functions of its curriculum (collision_avoidance_env.py:403-441).  Here the pool is a ring of
--depth slots per world that one small launch refills behind every auto-resetting step, so world w's episode e runs on the scenario
the samplers draw for key w + e * N: no scenario is ever replayed, no pool is regenerated, and no running episode is cut (compare
examples/curriculum_pools.py, which redraws the whole pool between roll-outs).  The curriculum's sampler set is switched with
set_stream_params as the step count passes the reference's thresholds; a world meets the new set depth - 1 episodes later.
Trains nothing: it steps, switches and prints the stream's counters.

    python examples/streaming_curriculum.py [--worlds 1024] [--depth 4] [--steps 4096] [--check 256] [--start 0] [--stages]

--stages adds train_stage_1 / train_stage_2 to the scenario list (obstacle worlds from 5e6 steps on).  RVO agents among rectangles
take at most 9 of them at max_agents 8 (include/cagym.h), so stage 2's up-to-10 rectangles are capped at 9 here.
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=4, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=4096, help="env steps per world")
    ap.add_argument("--check", type=int, default=256, help="env steps between two looks at the curriculum")
    ap.add_argument("--start", type=float, default=0.0, help="total env steps already trained (selects the curriculum stage)")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    names = scen.TRAINING_SCENARIOS + (("train_stage_1", "train_stage_2") if a.stages else ())
    n_obst = (-1, 9) if a.stages else None
    env = B(a.worlds, 8, n_scenarios=a.depth * a.worlds, max_obstacles=9 if a.stages else 0, game_over_mode="agent0")
    total, t, seed = a.start, 0, 0
    current = scen.reference_curriculum(total, names)
    env.stream_reference_scenarios(current[0], seed, number_of_agents=current[1], n_obst=n_obst)
    env.reset()
    while t < a.steps:
        for _ in range(min(a.check, a.steps - t)):
            env.step(auto_reset=True)  # one refill launch rides behind each step
        t += a.check
        total += a.check * a.worlds
        st, ep = env.stream_stats(), env.episode_stats()
        print("steps %8d  kinds %-12s agents %d  generated %d  failed %d  lapped %d  episodes %d" % (
            total, ",".join(str(k) for k in current[0]), current[1], st["generated"], st["n_failed"], st["n_lapped"],
            int(ep["stat_episodes"].sum())))
        nxt = scen.reference_curriculum(total, names)
        if nxt != current:  # the reference's switch: later refills draw from the new sampler set
            current, seed = nxt, seed + 1
            env.set_stream_params(current[0], seed, number_of_agents=current[1], n_obst=n_obst)
    torch.cuda.synchronize()
    print("streaming done")
    env.close()


if __name__ == "__main__":
    main()
