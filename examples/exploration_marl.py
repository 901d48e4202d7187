"""A team of robots as N * R environments with a reward of their own (attach_ig_credit, CagymRobotVecEnv): every world holds
--robots IG robots and --targets static targets on a fresh map per episode (stream_exploration_worlds).  The team reward is one
number per world; the credit launch behind every observation tells it apart per robot:
  own         the information in the robot's own cone,
  exclusive   the part of it no teammate's cone covered as well,
  difference  the team's gain minus what the gain would have been had this robot not looked (the difference reward).
CagymRobotVecEnv presents robot r of world w as environment w * R + r - observation: its belief window [3, G, G]; action: its
(v, omega); reward: the chosen kind - the shape a shared-parameter multi-agent learner trains on.

The policy here is fixed and hand-written, the place where a network would stand: drive at --speed and turn towards the half of the
window that holds more mutual information.  The script prints each robot's mean episode return for the three kinds next to the
team's (ig_robot_episode_stats() beside ig_episode_stats()).

    python examples/exploration_marl.py [--worlds 64] [--depth 2] [--steps 128] [--robots 3] [--targets 3] [--window 24]
                                        [--reward difference|own|exclusive|team]
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
vec = importlib.import_module("gym-exploration-2d_amd.vecenv")


def policy(obs, speed, turn):
    """obs [E, 3, G, G]: rows forward, columns to the robot's left.  Turn towards the half with more cell MI (channel 1)."""
    G = obs.shape[-1]
    mi = obs[:, 1]
    left, right = mi[:, :, G // 2:].sum(dim=(1, 2)), mi[:, :, :G // 2].sum(dim=(1, 2))
    act = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=obs.device)
    act[:, 0] = speed
    act[:, 1] = turn * torch.sign(left - right)
    return act


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--depth", type=int, default=2, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--robots", type=int, default=3)
    ap.add_argument("--targets", type=int, default=3)
    ap.add_argument("--window", type=int, default=24, help="cells per side of a robot's belief window (even, 4..64)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pref-speed", type=float, default=30.0, help="sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed")
    ap.add_argument("--speed", type=float, default=2.0)
    ap.add_argument("--turn", type=float, default=1.0)
    ap.add_argument("--reward", default="difference", choices=["difference", "own", "exclusive", "team"])
    a = ap.parse_args()

    N, R, M = a.worlds, a.robots, a.robots + a.targets
    env = B(N, M, n_scenarios=a.depth * N, max_obstacles=4, game_over_mode="agent0")
    env.stream_exploration_worlds("train_stage_1", n_obst=(1, 4), seed=a.seed, n_robots=R, n_targets=a.targets, target_radius=0.2,
                                  robot_pref_speed=a.pref_speed)
    env.attach_ig_learner(window=a.window, rotate=True)
    env.attach_ig_credit()
    v = vec.CagymRobotVecEnv(env, reward=a.reward)
    obs = v.reset()
    seen = torch.zeros((), dtype=torch.float64, device=env.device)
    for _ in range(a.steps):
        obs, rews, dones, infos = v.step(policy(obs, a.speed, a.turn))
        seen += rews.sum()
    torch.cuda.synchronize()
    print("marl       envs %d = %d worlds x %d robots  obs %s  reward %r  reward seen %.3f" % (
        v.num_envs, N, R, tuple(obs.shape), a.reward, float(seen)))
    team, rob = env.ig_episode_stats(), env.ig_robot_episode_stats()
    n = int(team["episodes"].sum())
    assert torch.equal(team["episodes"], rob["episodes"])
    print("team       episodes %d  mean return %.4f" % (n, float(team["sum"].sum()) / max(n, 1)))
    per = rob["sum"].sum(dim=0) / max(n, 1)  # [R, 3]
    for r in range(R):
        print("robot %d    mean return  own %.4f  exclusive %.4f  difference %.4f" % (r, float(per[r, 0]), float(per[r, 1]), float(per[r, 2])))
    print("sum over robots          own %.4f  exclusive %.4f  difference %.4f" % tuple(float(x) for x in per.sum(dim=0)))
    env.close()
    print("exploration marl done")


if __name__ == "__main__":
    main()
