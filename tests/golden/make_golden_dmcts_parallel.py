#!/usr/bin/env python3
"""Generate tests/golden/ig_dmcts_reference_parallel.npz by EXECUTING the reference's Dec-MCTS loop in its
agent-parallel mode (ig_mcts.set_param(..., parallelize_agents=True)) on the scenario and budget of
make_golden.dmcts_reference (IG_agent_crossing; Ntree 5, Nsims 3, horizon 4, Ncycles 2).

Run:  python tests/golden/make_golden_dmcts_parallel.py   (needs the reference; ~1 min)

The reference runs each robot of a cycle in its own process on a pickled copy of env.agents and writes the robots'
policy objects back once all of them have planned (collision_avoidance_env.py:342-379).  Here the processes are
replaced by an in-process pickle round trip with the same effect: for every cycle, each robot plans on its own
pickle copy of env.agents taken before any robot of the cycle has planned, and only then are the robots' policy
objects written back.  (The reference's child processes draw from freshly seeded np.random streams; here every
robot draws from the one global stream seeded per run, which keeps the fixture reproducible.)  The planner is
random, so the fixture pins statistics: the cumulative team reward, plus every robot's own team_reward per step
(the one-belief-per-world deviation in this mode).
"""
import os
import pickle

import numpy as np

import make_golden as mg

rh, Config = mg.rh, mg.Config


def _take_action_dmcts_parallel(env, dmcts_agents):
    """One planning step of the agent-parallel mode without processes."""
    actions = {}
    new_step = True
    for _ in range(env.agents[dmcts_agents[0]].policy.Ncycles):
        planned = {}
        for k in dmcts_agents:
            agents = pickle.loads(pickle.dumps(env.agents))  # this robot's view: the cycle's starting state
            obs = pickle.loads(pickle.dumps(env.observation[k]))
            actions[k] = agents[k].policy.find_next_action(obs, agents, k, env.obstacles, new_step)
            planned[k] = agents[k].policy
        for k in dmcts_agents:  # written back after every robot of the cycle has planned
            env.agents[k].policy = planned[k]
        new_step = False
    return actions


def dmcts_reference_parallel(n_seeds=12, n_steps=6):
    from gym_collision_avoidance.envs.collision_avoidance_env import CollisionAvoidanceEnv
    Config.EVALUATE_MODE = True
    Config.HOMOGENEOUS_TESTING = False
    Config.TRAIN_SINGLE_AGENT = False
    mg.set_max_agents(10)
    Config.STATES_IN_OBS = ['radius', 'heading_global_frame', 'pos_global_frame', 'pref_speed', 'other_agents_states']
    out = {"cum_reward": [], "first_actions": [], "pos": [], "team_reward": []}
    for seed in range(n_seeds):
        np.random.seed(seed)
        with rh.quiet():
            env = CollisionAvoidanceEnv()
            env.reset()
            for i in range(3):
                env.agents[i].policy.set_param(ego_agent=env.agents[i], occ_map=env.map, map_size=(30, 30),
                                               detect_fov=60.0, map_res=0.1, detect_range=5.0, Ntree=5, Nsims=3,
                                               parallelize_sims=False, mcts_cp=1., mcts_horizon=4,
                                               parallelize_agents=True, dt=0.1, xdt=5, mcts_gamma=0.95, Ncycles=2)
        env._take_action_dmcts = lambda agents, env=env: _take_action_dmcts_parallel(env, agents)
        cum, acts, pos, team = [0.0], [], [], []
        for t in range(n_steps):
            with rh.quiet():
                env.step({})
            cum.append(cum[-1] + env.agents[0].policy.team_reward)
            team.append([a.policy.team_reward for a in env.agents[:3]])
            acts.append([np.asarray(a.past_actions[0]) for a in env.agents[:3]])
            pos.append([np.append(a.pos_global_frame, a.heading_global_frame) for a in env.agents[:3]])
        out["cum_reward"].append(cum)
        out["first_actions"].append(acts)
        out["pos"].append(pos)
        out["team_reward"].append(team)
    Config.STATES_IN_OBS = list(mg.OBS_KEYS)
    path = os.path.join(mg.OUT, "ig_dmcts_reference_parallel.npz")
    np.savez_compressed(path, **{k: np.array(v, dtype=np.float64) for k, v in out.items()})
    print("%-28s          %8.1f KB" % ("ig_dmcts_reference_parallel", os.path.getsize(path) / 1024))
    print(np.array(out["cum_reward"])[:, -1])


if __name__ == "__main__":
    dmcts_reference_parallel()
