"""The best-viewpoint baseline on streamed exploration worlds (attach_ig_learner + attach_ig_goals + ig_propose_goals): every robot
drives to the place from which it would see the most mutual information, weighed against the way there.  ig_propose_goals hands
each robot its k best places - view gain / (geodesic distance + d0), at least min_sep apart - and the "policy", which stands where
a goal-level network would pick one of k, takes the best one that is not within min_sep of a teammate's target; ig_set_goals sends
the robot there.  The view gain is what a robot TURNING ON THE SPOT would cover, and the robots' sensors see a 60 degree cone: a
robot that has arrived gives its goal up and turns once round (--spin steps of the caller's row (0, pi)), then asks for the next
place - by then the belief round it is settled and the proposals lie elsewhere.  A robot whose world restarted starts over, with
a look round, as every robot does at the start.  Everything stays on the device.

--headings H (default 0: the loop above) scores POSES instead: ig_propose_goals(headings=H) ranks every place by the best of H sensor
cones there and hands the cone's heading back, ig_set_goals(..., headings=) makes the robot turn to it on arrival, and the robot
gives its goal up once info["goal_facing"] says "there, and facing it" - there is no look round, at the start or anywhere else.

--assign team (default apart: the pick above) leaves the choice to the env: ig_assign_goals prices every proposal by the mutual
information of the cells no teammate - under way or just assigned - is already going to see, through the walls and inside the sensor's
range (and cone, with --headings), and sends the robots that choose now to complementary viewpoints in one launch.

--rank route (default utility: one of the picks above) prices the WAY as well: ig_route_gains walks every proposal's shortest path on
the robot's own geodesic field, takes the sensor cone every --stride cells along it - what the robot will see while it drives - and
sends each robot that chooses now to the proposal whose route and view together are worth most per metre, in one launch; --assign is
not consulted then.

The same seed, hence the same never-repeating sequence of worlds, is then run by the built-in ig_greedy; both keep the IG team's
episode log, and stats.paired_by_key compares the two episode by episode on the worlds both finished.

    python examples/exploration_viewpoints.py [--worlds 64] [--depth 2] [--steps 128] [--robots 2] [--targets 3] [--k 8] [--spin 20] [--headings 0] [--assign apart]
                                             [--rank utility] [--stride 4]
"""
import argparse
import importlib
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


def report(name, env):
    rows = env.ig_episode_log()  # (one synchronisation)
    s = stats.exploration_statistics(rows)
    print("%-10s episodes %4d  return mean %.3f median %.3f  found %.3f of targets  entropy %.1f nats  touched %.3f" % (
        name, s["episodes"], s["mean_return"], s["median_return"], s["found_share"], s["mean_entropy"], s["mean_touched"]))
    return rows


def pick_apart(prop, target, need, min_sep):
    """One of k per robot, on the device: the best proposal that is not within min_sep of a teammate's target.  prop:
    ig_propose_goals' dict; target [N, R, 2]: every robot's current target (NaN: none); need [N, R] bool: the robots that choose
    now, in slot order, each seeing the choices made before it.  Returns (target with the new choices, rank [N, R] chosen)."""
    xy, n_found = prop["xy"], prop["n_found"]
    N, R, k, _ = xy.shape
    found = torch.arange(k, device=xy.device)[None, None, :] < n_found[:, :, None]  # [N, R, k]
    target = target.clone()
    rank = torch.zeros((N, R), dtype=torch.int64, device=xy.device)
    for r in range(R):  # (R is small; every line is an expression over [N, k])
        mates = torch.cat([target[:, :r], target[:, r + 1:]], dim=1)                          # [N, R - 1, 2]
        d = (xy[:, r, :, None, :] - mates[:, None, :, :]).norm(dim=-1)                         # [N, k, R - 1]; NaN: no target there
        free = found[:, r] & ~(d < min_sep).any(dim=-1)
        first = torch.where(free.any(dim=-1), free.float().argmax(dim=-1), torch.zeros_like(rank[:, r]))  # (none free: the best)
        rank[:, r] = first
        chosen = xy[:, r].gather(1, first[:, None, None].expand(N, 1, 2))[:, 0]
        target[:, r] = torch.where(need[:, r, None], chosen, target[:, r])
    return target, rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--depth", type=int, default=2, help="ring slots per world (>= 2)")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--robots", type=int, default=2)
    ap.add_argument("--targets", type=int, default=3)
    ap.add_argument("--window", type=int, default=4, help="cells per side of a robot's belief window (unused by this policy)")
    ap.add_argument("--k", type=int, default=8, help="proposals per robot (1..16)")
    ap.add_argument("--min-sep", type=float, default=2.0, help="metres between two proposals, and between two robots' targets")
    ap.add_argument("--d0", type=float, default=1.0, help="metres added to the distance in gain / (distance + d0)")
    ap.add_argument("--spin", type=int, default=20, help="steps a robot turns on the spot after it has arrived (20 x 0.1 s x pi rad/s: once round)")
    ap.add_argument("--headings", type=int, default=0, help="H > 0: proposals and goals carry the best of H headings; no look round")
    ap.add_argument("--assign", choices=("apart", "team"), default="apart",
                    help="apart: the best proposal min_sep from the teammates' targets; team: ig_assign_goals, marginal view gains")
    ap.add_argument("--rank", choices=("utility", "route"), default="utility",
                    help="utility: the pick of --assign on the proposals' own view gains; route: ig_route_gains' best, the way there priced too")
    ap.add_argument("--stride", type=int, default=4, help="--rank route: path cells between two way-points")
    ap.add_argument("--turn", type=float, default=3.141592653589793, help="rad/s of that turn")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--capacity", type=int, default=65536, help="rows of each episode log")
    ap.add_argument("--p-found", type=float, default=0.75, help="a target counts as found once P(occupied) of its cell reaches this")
    ap.add_argument("--pref-speed", type=float, default=10.0, help="sets the robots' time limit 3 (|p - g| - 0.75) / pref_speed")
    a = ap.parse_args()
    N, R = a.worlds, a.robots
    look = 0 if a.headings > 0 else a.spin  # steps of a look round: none when the goals carry a heading

    # best viewpoints: the env scores places and drives, the loop only picks one of k
    env, M = make(a)
    env.attach_ig_learner(window=a.window)
    env.attach_ig_goals()
    env.attach_ig_episode_log(capacity=a.capacity, p_found=a.p_found)
    env.reset()
    actions = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)  # rows of robots without a target: the caller's
    nan = torch.full((N, R, 2), float("nan"), dtype=torch.float64, device=env.device)
    if a.headings > 0:  # (no goal yet, but from here on the goals carry headings: ig_goals() and info hold goal_facing)
        env.ig_set_goals(nan, headings=nan[:, :, 0])
    goals = env.ig_goals()
    spin = torch.full((N, R), look, dtype=torch.int64, device=env.device)  # steps of the look round still to go
    n_set = n_shifted = 0
    for t in range(a.steps):
        active = goals["active"] != 0
        arrived = active & (goals["goal_facing" if a.headings > 0 else "goal_reached"] != 0)
        env.ig_clear_goals(mask=arrived.to(torch.uint8))  # (a proposal is a place the robot can reach: nobody gets stuck)
        spin = torch.where(arrived, torch.full_like(spin, look), spin)
        active = goals["active"] != 0
        need = ~active & (spin == 0)
        prop = env.ig_propose_goals(k=a.k, min_sep=a.min_sep, d0=a.d0, mask=need.to(torch.uint8), headings=a.headings if a.headings > 0 else None)
        if a.rank == "route":  # one launch: every proposal's route and view priced, the goals (and headings) set for the robots that choose now
            rank = env.ig_route_gains(mask=need.to(torch.uint8), stride=a.stride, set_goals=True)["best"]  # (-1: no route or nothing to see, no goal)
        elif a.assign == "team":  # one launch: the team's marginal gains, the goals (and headings) set for the robots that choose now
            rank = env.ig_assign_goals(mode="best", mask=need.to(torch.uint8))["choice"]  # (-1: nothing left to see, no goal)
        else:
            target = torch.where(active[:, :, None], goals["goal_xy"], nan)  # what the robots that keep their target aim at
            target, rank = pick_apart(prop, target, need, a.min_sep)
            if a.headings > 0:  # the chosen proposal's best cone: the robot turns to it once it is there
                env.ig_set_goals(target, mask=need.to(torch.uint8), headings=prop["heading"].gather(2, rank[:, :, None])[:, :, 0])
            else:
                env.ig_set_goals(target, mask=need.to(torch.uint8))
        n_set += int(need.sum())  # (host reads per step: an example's bookkeeping, not a training loop's)
        n_shifted += int((need & (rank > 0)).sum())
        actions[:, :R, 1] = torch.where(spin > 0, a.turn, 0.0).to(torch.float32)  # (read only by robots without a target)
        spin = (spin - 1).clamp(min=0)
        _, _, over, _ = env.step(actions, auto_reset=True)
        spin = torch.where((over != 0)[:, None], torch.full_like(spin, look), spin)  # a new world: look round first
    print("viewpoints targets set %d  moved off a teammate's %d  active now %d of %d" % (n_set, n_shifted, int(goals["active"].sum()), N * R))
    logs = {"viewpoints": report("viewpoints", env)}
    env.close()

    # the built-in greedy baseline on the same worlds
    env, M = make(a)
    env.attach_ig_greedy(episodic=True)
    env.attach_ig_episode_log(capacity=a.capacity, p_found=a.p_found)
    env.reset()
    for _ in range(a.steps):
        env.step(auto_reset=True)
    logs["ig_greedy"] = report("ig_greedy", env)
    env.close()

    ix, iy = stats.paired_by_key(logs["viewpoints"], logs["ig_greedy"])
    d = logs["viewpoints"]["ret"][ix] - logs["ig_greedy"]["ret"][iy]
    n = int(d.numel())
    print("viewpoints - ig_greedy on %4d shared worlds: mean return difference %+.3f, better on %.3f of them" % (
        n, float(d.mean()) if n else float("nan"), float((d > 0).double().mean()) if n else float("nan")))
    torch.cuda.synchronize()
    print("exploration viewpoints done")


if __name__ == "__main__":
    main()
