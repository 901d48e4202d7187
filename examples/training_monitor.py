"""A curriculum driven by SUCCESS RATE on streamed scenarios.  The reference's curriculum (collision_avoidance_env.py:419-438)
switches stages on step counts alone, because that is all a training loop on fresh worlds can see.  With the append-only episode
log (attach_episode_log) a streaming env keeps one row per finished episode, so the loop below reads the collision rate of the
newest --window episodes every --check steps and moves to the next stage - one more agent on the swap circle - once that rate falls
below --bound percent (and the window has filled with episodes of the current stage).  A logged failure is reproducible: its `key`
is the stream key its scenario was drawn for.  Trains nothing: the agents are the samplers' own RVO / NonCooperative policies.

    python examples/training_monitor.py [--worlds 256] [--depth 4] [--steps 2048] [--check 128] [--bound 25.0] [--window 256] [--agents 2]
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
stats = importlib.import_module("gym-exploration-2d_amd.stats")
B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=256)
    ap.add_argument("--depth", type=int, default=4, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=2048, help="env steps per world")
    ap.add_argument("--check", type=int, default=128, help="env steps between two looks at the log")
    ap.add_argument("--bound", type=float, default=25.0, help="collision rate of the window, in percent, below which the stage ends")
    ap.add_argument("--window", type=int, default=256, help="newest episodes the rate is taken over")
    ap.add_argument("--agents", type=int, default=2, help="agents on the circle in the first stage")
    ap.add_argument("--max-agents", type=int, default=8)
    a = ap.parse_args()
    env = B(a.worlds, a.max_agents, n_scenarios=a.depth * a.worlds, game_over_mode="agent0")
    stage, agents, seed = 0, a.agents, 0
    env.stream_reference_scenarios("train_agents_swap_circle", seed, number_of_agents=agents, fixed_count=True)
    env.reset()
    env.attach_episode_log(max(a.window, 4 * a.worlds))
    t, since, rate = 0, 0, float("nan")  # since: episodes logged when the stage began
    while t < a.steps:
        for _ in range(min(a.check, a.steps - t)):
            env.step(auto_reset=True)  # step, log update, refill: in this order on the stream
        t += a.check
        log = env.episode_log(last=a.window)
        n = int(log["count"].numel())
        if n == 0:
            continue
        rate = stats.suite_statistics(log)["pct_collision"]
        # the window holds the current stage's episodes only once every row in it has this stage's agent count
        settled = n == a.window and bool((log["n_agents"] == agents).all())
        if settled and rate < a.bound and agents < a.max_agents:
            head = int(env.episode_log_views()["head"])
            stage, agents, seed = stage + 1, agents + 1, seed + 1
            env.set_stream_params("train_agents_swap_circle", seed, number_of_agents=agents, fixed_count=True)
            print("step %6d: collision rate %.1f %% over %d episodes (%d since the last switch) -> stage %d, %d agents" % (
                t, rate, n, head - since, stage, agents))
            since = head
    torch.cuda.synchronize()
    st = env.stream_stats()
    print("monitor done: stage %d, %d agents, %d episodes logged, last collision rate %.1f %%, lapped %d" % (
        stage, agents, int(env.episode_log_views()["head"]), rate, st["n_lapped"]))
    env.close()


if __name__ == "__main__":
    main()
