"""Goal actions on streamed exploration worlds (attach_ig_learner + attach_ig_goals): instead of a (v, omega) per step the "policy"
names a PLACE for each robot - a cell of the belief window the env hands out - and the env drives there round the obstacles: one
geodesic launch per goal (ig_set_goals), then one controller launch in front of every step and one status launch behind it.

The place-picking rule stands where a policy network would: every --every steps, or as soon as a robot has reached its goal or
lost it (its world restarted, or the goal cannot be reached), the robot's goal becomes the cell of its belief window with the
largest mutual-information channel (frame="window"); a robot whose last goal turned out unreachable draws a random window cell
instead.  Everything stays on the device; the script prints the mean team return beside the random (v, omega) learner of
examples/exploration_learner.py and the built-in ig_greedy on the same seed, hence the same sequence of worlds.

    python examples/exploration_goals.py [--worlds 64] [--depth 2] [--steps 128] [--robots 2] [--targets 3] [--window 24] [--every 8]
"""
import argparse
import importlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
vec = importlib.import_module("gym-exploration-2d_amd.vecenv")


def make(a):
    M = a.robots + a.targets
    env = B(a.worlds, M, n_scenarios=a.depth * a.worlds, max_obstacles=4, game_over_mode="agent0")
    env.stream_exploration_worlds("train_stage_1", n_obst=(1, 4), seed=a.seed, n_robots=a.robots, n_targets=a.targets,
                                  target_radius=0.2, robot_pref_speed=a.pref_speed)
    return env, M


def report(name, env):
    ig = env.ig_episode_stats()
    n = int(ig["episodes"].sum())
    print("%-10s episodes %d  mean team return %.4f  last %s" % (
        name, n, float(ig["sum"].sum()) / max(n, 1), " ".join("%.3f" % v for v in ig["last"][:4].tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--depth", type=int, default=2, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--robots", type=int, default=2)
    ap.add_argument("--targets", type=int, default=3)
    ap.add_argument("--window", type=int, default=24, help="cells per side of a robot's belief window (even, 4..64)")
    ap.add_argument("--every", type=int, default=8, help="steps after which every robot gets a new goal")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pref-speed", type=float, default=10.0, help="sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed")
    a = ap.parse_args()
    N, R, G = a.worlds, a.robots, a.window

    # goals: the env drives, the loop only names places
    env, M = make(a)
    env.attach_ig_learner(window=G, rotate=True)
    env.attach_ig_goals()
    v = vec.CagymVecEnv(env, ["dist_to_goal", "heading_ego_frame", "other_agents_states"])
    v.reset()
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    actions = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)  # rows of robots without a goal: stand still
    goals, infos = env.ig_goals(), None
    unreachable = torch.zeros((N, R), dtype=torch.bool, device=env.device)
    n_set = n_reached = 0
    for t in range(a.steps):
        if infos is not None:  # (the first step has no window yet: the robots stand still)
            idle = (goals["active"] == 0) | (goals["goal_reached"] != 0) | unreachable
            need = idle if t % a.every else torch.ones_like(idle)
            best = infos["belief_window"][:, :, 1].reshape(N, R, G * G).argmax(dim=-1)  # the window cell with the most information left
            rand = torch.randint(0, G * G, (N, R), generator=gen, device=env.device)
            pick = torch.where(unreachable, rand, best)
            cells = torch.stack([pick // G, pick % G], dim=-1).to(torch.int32)
            env.ig_set_goals(cells, mask=need.to(torch.uint8), frame="window")
            unreachable = (goals["active"] != 0) & torch.isinf(goals["goal_distance"])
            n_set += int(need.sum())  # (host reads per step: an example's bookkeeping, not a training loop's)
        _, _, _, infos = v.step(actions)
        n_reached += int(infos["goal_reached"].sum())
    print("goals      set %d  robot-steps at a goal %d  active now %d of %d  mean metres to go %.2f" % (
        n_set, n_reached, int(goals["active"].sum()), N * R,
        float(goals["goal_distance"][torch.isfinite(goals["goal_distance"])].mean()) if torch.isfinite(goals["goal_distance"]).any() else 0.0))
    report("goals", env)
    env.close()

    # the random (v, omega) learner on the same worlds
    env, M = make(a)
    env.attach_ig_learner(window=G, rotate=True)
    env.reset()
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    for _ in range(a.steps):
        actions[..., 0] = 4.0 * torch.rand((N, M), generator=gen, device=env.device)
        actions[..., 1] = math.pi * (2.0 * torch.rand((N, M), generator=gen, device=env.device) - 1.0)
        env.step(actions, auto_reset=True)
    report("random", env)
    env.close()

    # the built-in greedy baseline on the same worlds
    env, M = make(a)
    env.reset()
    env.attach_ig_greedy(episodic=True)
    for _ in range(a.steps):
        env.step(auto_reset=True)
    report("ig_greedy", env)
    torch.cuda.synchronize()
    env.close()
    print("exploration goals done")


if __name__ == "__main__":
    main()
