"""Checkpoint and resume of a streaming run (cagym_checkpoint_*): a crowd of NonCooperative agents on streamed worlds with a
curriculum switch, an episode log and hard-case replay - the configuration a long training job runs in.  Half way through the env is
saved to a file (env.checkpoint() -> EnvCheckpoint.state_dict() -> torch.save); the run goes on, and a FRESH env of the same shape
loads the file (torch.load -> EnvCheckpoint.from_state_dict -> env.load_checkpoint()) and goes on the same way.  The two
continuations agree bit for bit: rewards, game_over, the episode log, the replay buffer's counters and the stream's.

    python examples/checkpoint_resume.py [--worlds 1024] [--agents 4] [--depth 3] [--steps 1024] [--file checkpoint.pt] [--seed 11]
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
benv = importlib.import_module("gym-exploration-2d_amd.batched_env")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--depth", type=int, default=3, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=1024, help="env steps per world, half before the checkpoint and half after")
    ap.add_argument("--file", default="checkpoint.pt")
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    N, half = a.worlds, max(a.steps // 2, 2)
    make = lambda: benv.BatchedCollisionAvoidanceEnv(N, a.agents, n_scenarios=a.depth * N, game_over_mode="agent0")
    crowd = dict(number_of_agents=a.agents, fixed_count=True, ego_policy=scen.POLICY_NONCOOP, ego_dynamics=scen.DYN_UNICYCLE,
                 other_policies=scen.POLICY_NONCOOP)
    env = make()
    env.stream_reference_scenarios("train_agents_random_positions", a.seed, **crowd)
    env.attach_episode_log(4096)
    env.attach_replay(capacity=256, p=0.25, outcomes=("collision", "stuck"), seed=a.seed)
    env.reset()
    env.rollout(half // 2, auto_reset=True)
    env.set_stream_params("train_agents_swap_circle", a.seed + 1, **crowd)  # the curriculum moves on
    env.rollout(half - half // 2, auto_reset=True)

    ckpt = env.checkpoint()
    torch.save(ckpt.state_dict(), a.file)
    print("saved %s: %d bytes of header, sections %s" % (a.file, ckpt.sizes[0], dict(zip(("state", "pool", "stream", "log", "replay"), ckpt.sizes[1:]))))

    def go_on(e):
        out = e.rollout(half, auto_reset=True)
        return [out["reward"], out["game_over"]] + [e.episode_log()[k] for k in ("key", "world", "episode", "ret", "outcome")], \
            (e.replay_stats(), e.stream_stats())

    want, want_stats = go_on(env)

    fresh = make()  # no pool, no stream, no log: the checkpoint brings them
    fresh.load_checkpoint(benv.EnvCheckpoint.from_state_dict(torch.load(a.file), fresh.device))
    got, got_stats = go_on(fresh)
    same = got_stats == want_stats and all(torch.equal(x, y) for x, y in zip(got, want))
    st, ss = got_stats
    print("after the resume: %d episodes logged, %d slots generated (%d from the replay buffer), %d keys harvested" % (
        int(fresh.episode_log_views()["head"].item()), ss["generated"], st["replayed"], st["harvested"]))
    print("resumed run equals the uninterrupted one: %s" % same)
    print("resume done")
    env.close()
    fresh.close()


if __name__ == "__main__":
    main()
