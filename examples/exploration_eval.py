"""Evaluate exploration policies episode by episode (attach_ig_episode_log): three handles run on ONE stream_exploration_worlds
seed, hence on the same never-repeating sequence of worlds - a "learner" that draws (v, omega) at random (the place of a policy
network), the built-in ig_greedy, and Dec-MCTS (ig_mcts) at a small budget.  Each keeps the IG team's episode log: one row per
finished team episode with its return, which targets the belief localised and at which step, and the entropy of the belief it ended
on.  The script prints stats.exploration_statistics per policy and, by stats.paired_by_key, the return difference on the worlds two
policies both finished - the comparison by stream key, not of two means over different worlds.

    python examples/exploration_eval.py [--worlds 64] [--depth 2] [--steps 128] [--robots 2] [--targets 3] [--p-found 0.75]
"""
import argparse
import importlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
stats = importlib.import_module("gym-exploration-2d_amd.stats")


def make(a):
    M = a.robots + a.targets
    env = B(a.worlds, M, n_scenarios=a.depth * a.worlds, max_obstacles=4, game_over_mode="agent0")
    env.stream_exploration_worlds("train_stage_1", n_obst=(1, 4), seed=a.seed, n_robots=a.robots, n_targets=a.targets,
                                  target_radius=0.2, robot_pref_speed=a.pref_speed)
    env.reset()
    return env, M


def run(a, name):
    env, M = make(a)
    if name == "random":
        env.attach_ig_learner(window=4)
    elif name == "ig_greedy":
        env.attach_ig_greedy(episodic=True)
    else:
        env.attach_ig_mcts(Ntree=a.ntree, Nsims=4, Ncycles=2, mcts_horizon=3, seed=a.seed, episodic=True)
    env.attach_ig_episode_log(capacity=a.capacity, p_found=a.p_found)
    env.reset()
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    actions = torch.zeros((a.worlds, M, 2), dtype=torch.float32, device=env.device) if name == "random" else None
    for _ in range(a.steps):
        if actions is not None:  # a policy would map the observation and info["belief_window"] to the robots' rows here
            actions[..., 0] = 4.0 * torch.rand((a.worlds, M), generator=gen, device=env.device)
            actions[..., 1] = math.pi * (2.0 * torch.rand((a.worlds, M), generator=gen, device=env.device) - 1.0)
        env.step(actions, auto_reset=True)
    rows = env.ig_episode_log()  # (one synchronisation)
    s = stats.exploration_statistics(rows)
    print("%-10s episodes %4d  return mean %.3f median %.3f  found %.3f of targets, all in %.3f of episodes  found_at p50/p75/p90 %s  "
          "entropy %.1f nats  touched %.3f" % (name, s["episodes"], s["mean_return"], s["median_return"], s["found_share"],
                                              s["all_found_share"], "/".join("%.1f" % x for x in s["found_at_pctls"].tolist()),
                                              s["mean_entropy"], s["mean_touched"]))
    env.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--depth", type=int, default=2, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--robots", type=int, default=2)
    ap.add_argument("--targets", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ntree", type=int, default=4, help="Dec-MCTS tree iterations per cycle (a small budget)")
    ap.add_argument("--capacity", type=int, default=65536, help="rows of each episode log")
    ap.add_argument("--p-found", type=float, default=0.75, help="a target counts as found once P(occupied) of its cell reaches this")
    ap.add_argument("--pref-speed", type=float, default=10.0, help="sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed")
    a = ap.parse_args()
    logs = {name: run(a, name) for name in ("random", "ig_greedy", "ig_mcts")}
    for x, y in (("ig_greedy", "random"), ("ig_mcts", "random"), ("ig_mcts", "ig_greedy")):
        ix, iy = stats.paired_by_key(logs[x], logs[y])
        d = logs[x]["ret"][ix] - logs[y]["ret"][iy]
        n = int(d.numel())
        print("%-9s - %-9s on %4d shared worlds: mean return difference %+.3f, better on %.3f of them" % (
            x, y, n, float(d.mean()) if n else float("nan"), float((d > 0).double().mean()) if n else float("nan")))
    torch.cuda.synchronize()
    print("exploration eval done")


if __name__ == "__main__":
    main()
