#!/usr/bin/env python3
"""The main loop of the reference's experiments/src/dmcts.py, line for line, on the gym-style facade: IG_agent_crossing
(test_cases.py:3209-3239: 3 ig_mcts robots with FirstOrderDynamics, 2 static targets, 4 rectangles), set_param on every
robot, then env.step({}) - the env plans the robots itself (device belief update, team MI reward, Dec-MCTS) - and the team
reward read from agent 0's policy.  Prints the cumulative team reward.

usage: python examples/dmcts_reference_loop.py [--steps 30] [--Ntree 30] [--Nsims 10] [--Ncycles 5] [--cp 1.0]
                                               [--parallelize-agents] [--seed 0]"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
E = importlib.import_module("gym-exploration-2d_amd.env")
Config = E.Config

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)  # the reference runs up to 300 (dmcts.py:83)
ap.add_argument("--Ntree", type=int, default=30)
ap.add_argument("--Nsims", type=int, default=10)
ap.add_argument("--Ncycles", type=int, default=5)
ap.add_argument("--cp", type=float, default=1.0)
ap.add_argument("--parallelize-agents", action="store_true")
ap.add_argument("--seed", type=int, default=0, help="the planner's random streams (the reference draws from np.random)")
args = ap.parse_args()
Ntree, Nsims, Ncycles, mcts_cp = args.Ntree, args.Nsims, args.Ncycles, args.cp


def ig_agent_crossing():
    """tc.IG_agent_crossing (test_cases.py:3209-3239)."""
    robots = [E.Agent(x, 0, 16, 0, 0.5, 1.0, 0.0, E.ig_mcts, E.FirstOrderDynamics, [E.OtherAgentsStatesSensor], i)
              for i, x in enumerate((-5, 0, 5))]
    targets = [E.Agent(x, y, 0, 0, 0.2, 1.0, 0.0, E.StaticPolicy, E.FirstOrderDynamics, [E.OtherAgentsStatesSensor], 3 + i)
               for i, (x, y) in enumerate(((6, 12), (-6, -12)))]
    obstacles = [(2, 2, 10, 10), (-10, 2, -2, 10), (2, -10, 10, -2), (-10, -10, -2, -2)]  # xl, yl, xu, yu (:3219-3222)
    return robots + targets, obstacles


env = E.CollisionAvoidanceEnv()
env.planner_seed = args.seed
env.set_agents(ig_agent_crossing())

obs = env.reset()  # Get agents' initial observations

dmcts_agents = [0, 1, 2]

cum_reward = [0.0]

for i in dmcts_agents:
    env.agents[i].policy.set_param(ego_agent=env.agents[i], occ_map=env.map,
                                   map_size=(Config.MAP_WIDTH, Config.MAP_HEIGHT), detect_fov=60.0,
                                   map_res=Config.SUBMAP_RESOLUTION, detect_range=5.0,
                                   Ntree=Ntree, Nsims=Nsims, parallelize_sims=False, mcts_cp=mcts_cp, mcts_horizon=4,
                                   parallelize_agents=args.parallelize_agents, dt=0.1, xdt=5, mcts_gamma=0.95,
                                   Ncycles=Ncycles)

# Repeatedly send actions to the environment based on agents' observations
num_steps = args.steps
for i in range(num_steps):
    actions = {}
    # Run a simulation step (check for collisions, move sim agents)
    obs, rewards, game_over, which_agents_done = env.step(actions)

    cum_reward.append(env.agents[0].policy.team_reward + cum_reward[-1])

    if game_over:
        print("All agents finished!")
        break
env.reset()
env.close()

print("steps %d: cumulative team reward %.6f" % (len(cum_reward) - 1, cum_reward[-1]))
