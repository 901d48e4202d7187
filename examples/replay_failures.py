"""Hard-case replay inside the scenario stream (cagym_stream_replay_*): a crowd of NonCooperative agents on streamed
train_agents_random_positions worlds, an episode log, and attach_replay() - from then on the key of every episode that ends in a
collision or stuck goes into a device buffer (one harvest launch behind the log's update), and the refill generates a share p of its
slots from keys of that buffer instead of fresh ones.  The log's key column names the scenario each episode really ran, so the two
populations can be told apart afterwards: a row whose key is its own w + e * N ran a fresh scenario, any other a replayed one.
Trains nothing - the agents do not learn, so a replayed failure fails again, which is what the printed rates show: replay spends
the chosen share of the episodes on scenarios that are known to fail.  No host synchronisation inside the loop.

    python examples/replay_failures.py [--worlds 1024] [--agents 4] [--depth 2] [--steps 1024] [--p 0.25] [--capacity 4096] [--seed 11]
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
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--depth", type=int, default=2, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=1024, help="env steps per world")
    ap.add_argument("--p", type=float, default=0.25, help="share of the refilled slots drawn from the replay buffer")
    ap.add_argument("--capacity", type=int, default=4096, help="keys the replay buffer holds")
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    N = a.worlds
    env = B(N, a.agents, n_scenarios=a.depth * N, game_over_mode="agent0")
    env.stream_reference_scenarios("train_agents_random_positions", a.seed, number_of_agents=a.agents, fixed_count=True,
                                   ego_policy=scen.POLICY_NONCOOP, ego_dynamics=scen.DYN_UNICYCLE, other_policies=scen.POLICY_NONCOOP)
    env.attach_episode_log(1 << 20)
    env.attach_replay(capacity=a.capacity, p=a.p, outcomes=("collision", "stuck"), seed=a.seed)
    env.reset()
    for _ in range(a.steps):
        env.step(auto_reset=True)  # behind each step: log update, replay harvest, refill
    rows, st = env.episode_log(), env.replay_stats()
    own = rows["world"].to(torch.int64) + rows["episode"].to(torch.int64) * N
    replayed = rows["key"] != (own & 0xFFFFFFFF)
    failed = (rows["outcome"] & 5) != 0
    for name, sel in (("fresh", ~replayed), ("replayed", replayed)):
        n = int(sel.sum())
        print("%-8s %6d episodes, %5.1f %% end in a collision or stuck" % (name, n, 100.0 * int((failed & sel).sum()) / max(n, 1)))
    print("buffer: %d keys harvested, %d live of %d; %d slots generated from it; missed %d stale %d" % (
        st["harvested"], st["live"], st["capacity"], st["replayed"], st["n_missed"], st["n_stale"]))
    print("replay done")
    env.close()


if __name__ == "__main__":
    main()
