"""Trajectory datasets from a STREAMING env, as the reference's run_trajectory_dataset_creator.py writes them - without stopping the
auto-resetting loop and without one env.state() snapshot per step (dataset.record_episode).  The env streams
train_agents_swap_circle worlds (no scenario is ever replayed), the episode log names every finished episode by (world, episode),
and the trajectory ring keeps the reference's global_state_history row of every agent and step, the terminal row included
(attach_trajectory_ring: one capture launch between the step and the restart of the finished worlds).  Every --every steps the
episodes the log has appended since the last look, and that are still whole in the ring, are written as one reference-schema pickle
(dataset.export_ring); at the end the trajectory of the last logged collision is dumped as an array.
The ring holds --every + --margin slices: an episode is exported whole if it is no longer than the margin.

    python examples/trajectory_dataset.py [--worlds 256] [--agents 8] [--steps 1024] [--every 128] [--margin 384] [--out DIR]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
dataset = importlib.import_module("gym-exploration-2d_amd.dataset")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=256)
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4, help="streamed pool slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--every", type=int, default=128, help="env steps between two exports")
    ap.add_argument("--margin", type=int, default=384, help="ring slices on top of --every: the longest episode exported whole")
    ap.add_argument("--out", default="trajectory_dataset")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    N, M = a.worlds, a.agents
    env = B(N, M, n_scenarios=a.depth * N, game_over_mode="agent0")
    env.stream_reference_scenarios("train_agents_swap_circle", seed=0)
    env.reset()
    env.attach_episode_log(capacity=max(4096, 4 * N))
    env.attach_trajectory_ring(a.every + a.margin)
    coop = np.full((M,), 0.5)  # the sampler's rule (train_agents_swap_circle): the ego 1.0, every other agent 0.5
    coop[0] = 1.0
    seen, t, files, collision = 0, 0, [], None
    while t < a.steps:
        for _ in range(min(a.every, a.steps - t)):
            env.step(auto_reset=True)  # step, capture, restart of the finished worlds; log update and refill ride behind
        t += a.every
        head = int(env.episode_log_views()["head"].item())
        rows = env.episode_log(last=head - seen)  # the episodes appended since the last look, oldest first
        seen = head
        world, episode = rows["world"].cpu().numpy(), rows["episode"].cpu().numpy()
        hit = np.nonzero(rows["outcome"].cpu().numpy() & 1)[0]
        if hit.size:
            collision = (int(world[hit[-1]]), int(episode[hit[-1]]))
        path = os.path.join(a.out, "trajectories_%06d.pkl" % t)
        n = dataset.export_ring(env, path, zip(world, episode), n_agents=rows["n_agents"].cpu().numpy(), coop=np.tile(coop, (len(world), 1)))
        files.append(path)
        print("steps %6d  episodes logged %5d  agent trajectories written %6d  -> %s" % (t, len(world), n, path))
    if collision is not None:
        tr = env.trajectory(*collision)
        path = os.path.join(a.out, "collision_world%d_episode%d.npz" % collision)
        np.savez(path, history=tr["history"], moved=tr["moved"], complete=tr["complete"], columns=np.asarray(importlib.import_module(
            "gym-exploration-2d_amd._lib").TRAJ_COLUMNS))
        print("last logged collision: world %d episode %d, %d steps in the ring (complete: %s) -> %s" % (
            collision + (tr["history"].shape[0], tr["complete"], path)))
    torch.cuda.synchronize()
    print("stream: %s" % env.stream_stats())
    env.close()
    return files


if __name__ == "__main__":
    main()
