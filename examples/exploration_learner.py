"""A learner's loop on streamed exploration worlds (attach_ig_learner): every world holds --robots IG robots and --targets static
targets on a fresh map per episode (stream_exploration_worlds), the caller moves the robots through step()'s action table, and
the env keeps the belief, the team's information-gain reward and each robot's ego-centred belief window around them
(infos["belief_window"] [N, R, 3, G, G]: P(occupied), cell mutual information, inside-the-map) - one fused launch behind every step.

Two handles run on the same seed, hence on the same sequence of worlds: a "learner" that draws (v, omega) at random - the place
where a policy network would read the flat observation and the window - and the built-in ig_greedy baseline.  The script prints
both mean episode returns from ig_episode_stats().

--context adds the second image in the same frame, infos["context_window"] [N, R, 3, G, G]: obstacle clearance (what the built-in
planners' feasibility test reads), the other moving agents and the cells the team's sensors covered in this update.

    python examples/exploration_learner.py [--worlds 64] [--depth 2] [--steps 128] [--robots 2] [--targets 3] [--window 24] [--context]
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
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pref-speed", type=float, default=10.0, help="sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed")
    ap.add_argument("--context", action="store_true", help="also keep infos['context_window']: clearance, agents, seen-now")
    a = ap.parse_args()

    # the learner: a VecEnv whose infos carry the windows beside the flat observation
    env, M = make(a)
    env.attach_ig_learner(window=a.window, rotate=True, context=a.context)
    v = vec.CagymVecEnv(env, ["dist_to_goal", "heading_ego_frame", "other_agents_states"])
    obs = v.reset()
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    actions = torch.zeros((a.worlds, M, 2), dtype=torch.float32, device=env.device)
    seen = 0.0
    for _ in range(a.steps):
        # a policy would map (obs, infos["belief_window"]) to the robots' rows here; rows of internally driven agents are ignored
        actions[..., 0] = 4.0 * torch.rand((a.worlds, M), generator=gen, device=env.device)
        actions[..., 1] = math.pi * (2.0 * torch.rand((a.worlds, M), generator=gen, device=env.device) - 1.0)
        obs, rews, dones, infos = v.step(actions)
        seen += float(infos["team_reward"].sum())  # (a host read per step: an example's bookkeeping, not a training loop's)
    win = infos["belief_window"]
    print("learner    obs %s  belief_window %s  inside-map share %.3f  reward seen %.3f" % (
        tuple(obs.shape), tuple(win.shape), float(win[:, :, 2].mean()), seen))
    if a.context:
        ctx = infos["context_window"]
        print("learner    context_window %s  mean clearance %.3f  seen-now share %.3f" % (
            tuple(ctx.shape), float(ctx[:, :, 0].mean()), float(ctx[:, :, 2].mean())))
    report("random", env)
    env.close()

    # the baseline on the same worlds
    env, M = make(a)
    env.reset()
    env.attach_ig_greedy(episodic=True)
    for _ in range(a.steps):
        env.step(auto_reset=True)
    report("ig_greedy", env)
    torch.cuda.synchronize()
    env.close()
    print("exploration learner done")


if __name__ == "__main__":
    main()
