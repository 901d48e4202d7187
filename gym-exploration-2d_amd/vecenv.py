"""Flat-observation / VecEnv adapter on device tensors.

Byte layout of the reference's MultiagentFlattenDictWrapper (envs/wrappers.py:8-46): for agent 0..M-1, for
key in dict_keys (Config.STATES_IN_OBS order): the raveled value -- one float32 row of M * obs_len per world.
VecEnv convention of stable-baselines' DummyVecEnv as the reference uses it (experiments/src/env_utils.py:29-62):
step(actions) -> (obs[n_envs, D], rews[n_envs], dones[n_envs], infos), finished envs restart and return the
first observation of the new episode.  Everything stays on the GPU; no host round trip per step.
"""
import numpy as np
import torch

# (source tensor, first column, width) of every in-scope key (config.py:104-215)
_EGO = {"dist_to_goal": (0, 1), "rel_goal": (1, 2), "radius": (3, 1), "heading_ego_frame": (4, 1),
        "heading_global_frame": (5, 1), "pos_global_frame": (6, 2), "pref_speed": (8, 1), "num_other_agents": (9, 1),
        "use_ppo": (10, 1)}


def key_width(key, M):
    if key in _EGO:
        return _EGO[key][1]
    if key == "other_agents_states":
        return (M - 1) * 10
    if key == "other_agent_states":
        return 10
    if key == "laserscan":
        return 16
    raise KeyError("observation key %r is outside the hot-path scope (SURVEY.md 8(a))" % key)


def observation_indices(dict_keys, M):
    """Same bookkeeping as MultiagentFlattenDictWrapper.__init__ (wrappers.py:17-31)."""
    idx, size = {}, 0
    for agent in range(M):
        idx[agent] = {}
        lo = size
        for key in dict_keys:
            w = key_width(key, M)
            idx[agent][key] = [size, size + w]
            size += w
        idx[agent]["BOUNDS"] = [lo, size]
    return idx, size


class FlatObservation(object):
    def __init__(self, benv, dict_keys):
        self.b, self.keys = benv, list(dict_keys)
        self.indices, self.size = observation_indices(self.keys, benv.M)
        self.agent_size = self.size // benv.M

    def __call__(self, obs=None):
        """The flat rows of the env's current observation tensors, or of `obs`: a dict of tensors of the same shapes under the
        keys "other_agents_states", "ego" and "laserscan" (e.g. step()'s info["terminal"])."""
        b = self.b
        oas, ego, laser = (b.obs_oas, b.obs_ego, b.obs_laser) if obs is None else (obs["other_agents_states"], obs["ego"], obs.get("laserscan"))
        parts = []
        for key in self.keys:
            if key in _EGO:
                c, w = _EGO[key]
                parts.append(ego[:, :, c:c + w])
            elif key == "other_agents_states":
                parts.append(oas.reshape(b.N, b.M, -1))
            elif key == "other_agent_states":
                parts.append(oas[:, :, 0, :])
            elif key == "laserscan":
                parts.append(laser)
        return torch.cat(parts, dim=2).reshape(b.N, self.size)

    def array_to_dict(self, row):
        """observationArrayToDict (wrappers.py:48-57) for one world's flat row."""
        row = np.asarray(row)
        return {a: {k: row[self.indices[a][k][0]:self.indices[a][k][1]] for k in self.keys} for a in range(self.b.M)}


class CagymVecEnv(object):
    """n_envs = N worlds.  rews: agent 0's reward when single_agent (Config.TRAIN_SINGLE_AGENT, env.py:565-566)
    else [N, M].  terminal_observation=True: infos["terminal_observation"] is the [N, D] flat observation every world that
    finished on this step ENDED on (DummyVecEnv's infos[i]["terminal_observation"]; the returned obs is the first one of its new
    episode); rows are valid where dones.  It switches the env's keep_terminal_observations() on."""

    def __init__(self, benv, dict_keys, single_agent=True, terminal_observation=False):
        self.b = benv
        self.num_envs = benv.N
        self.flat = FlatObservation(benv, dict_keys)
        self.single_agent = single_agent
        self._actions = None
        self.terminal_observation = bool(terminal_observation)
        if self.terminal_observation:
            benv.keep_terminal_observations()

    def reset(self):
        self.b.reset()
        return self.flat()

    def step_async(self, actions):
        self._actions = actions

    @staticmethod
    def _external(actions):
        """None, or a list / tuple of None (the reference's env.step([None])), means no external actions."""
        if actions is None or (isinstance(actions, (list, tuple)) and all(a is None for a in actions)):
            return None
        return actions

    def step_wait(self):
        b = self.b
        # DummyVecEnv auto-reset inside the launch; an attached GA3C policy or (episodic) ig_mcts team fills its agents' rows and
        # restarts with its worlds (BatchedCollisionAvoidanceEnv.step); attached episode records and the episode log are fed there too
        _, rew, go, info = b.step(self._external(self._actions), auto_reset=True)
        rews = rew[:, 0] if self.single_agent else rew
        infos = {"flags": info["flags"]}
        if getattr(b, "_igm", None) is not None:  # an episodic attach_ig_mcts: the team's MI reward of this step, [N] f64
            infos["team_reward"] = b.team_reward
            if "belief_window" in info:  # attach_ig_learner: the robots' belief windows, an image beside the flat observation
                infos["belief_window"], infos["gain"] = info["belief_window"], info["gain"]
                if "context_window" in info:  # attach_ig_learner(context=True): the second image, same frame
                    infos["context_window"] = info["context_window"]
                if "goal_distance" in info:  # attach_ig_goals: metres to go along the grid, and goal reached
                    infos["goal_distance"], infos["goal_reached"] = info["goal_distance"], info["goal_reached"]
                if "robot_reward" in info:  # attach_ig_credit: the team reward told apart per robot, [N, R, 3] f64
                    infos["robot_reward"] = info["robot_reward"]
        if self.terminal_observation:
            infos["terminal_observation"] = self.flat(info["terminal"])
        return self.flat(), rews, go.bool(), infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.b.close()


ROBOT_REWARDS = {"own": 0, "exclusive": 1, "difference": 2}  # the columns of info["robot_reward"] (attach_ig_credit)


class CagymRobotVecEnv(object):
    """The learner's robots as the N * R environments a standard training loop wants: env index w * R + r is robot r (slot order)
    of world w.  Needs attach_ig_learner; attach_ig_credit is switched on here when a per-robot reward is asked for and the env does
    not have it yet.
      obs  [N*R, 3, G, G] f32: each robot's belief window; [N*R, 6, G, G] with attach_ig_learner(context=True), the context window's
           three channels behind the belief's.
      step(actions [N*R, 2]): the robots' (v, omega).  They go into the robots' rows of a table [N, M, 2] this object owns, whose
           other rows stay zero (cagym_ig_robot_actions, on the device), and benv.step(table, auto_reset=True) runs; a robot that
           holds a goal (attach_ig_goals) still follows the controller.
      rews [N*R] f64: reward="difference" | "own" | "exclusive" - that column of info["robot_reward"]; "team" - team_reward, the
           same number for every robot of a world.
      dones [N*R] bool: the world's game_over, repeated per robot.
      infos: "team_reward" [N] and, with the credit attached, "credit" [N, R, 3]; the goal keys where present.
    Everything stays on the GPU; nothing synchronises."""

    def __init__(self, benv, reward="difference"):
        g = getattr(benv, "_igm", None)
        if g is None or g.kind != "ig_learner":
            raise RuntimeError("CagymRobotVecEnv needs attach_ig_learner: its environments are the learner's robots")
        if reward != "team" and reward not in ROBOT_REWARDS:
            raise ValueError("CagymRobotVecEnv: reward must be one of 'difference', 'own', 'exclusive', 'team', got %r" % (reward,))
        if reward != "team" and benv._credit is None:
            benv.attach_ig_credit()
        self.b, self.reward, self.R = benv, reward, g.R
        self.num_envs = benv.N * g.R
        self._table = torch.zeros((benv.N, benv.M, 2), dtype=torch.float32, device=benv.device)
        self._actions = None

    def _obs(self):
        g = self.b._igm
        w = g.belief_window if g.context_window is None else torch.cat([g.belief_window, g.context_window], dim=2)
        return w.reshape(self.num_envs, w.shape[2], g.window, g.window)

    def reset(self):
        self.b.reset()
        return self._obs()

    def step_async(self, actions):
        self._actions = actions

    def step_wait(self):
        b, R = self.b, self.R
        planned = torch.as_tensor(self._actions, device=b.device).to(torch.float64).reshape(b.N, R, 2).contiguous()
        self._table.zero_()  # (a streamed world may come back with its robots in other slots)
        b._igm.ig.robot_actions(R, planned, self._table)
        _, _, go, info = b.step(self._table, auto_reset=True)
        if self.reward == "team":
            rews = b.team_reward.repeat_interleave(R)
        else:
            rews = info["robot_reward"][:, :, ROBOT_REWARDS[self.reward]].reshape(self.num_envs)
        infos = {"team_reward": b.team_reward}
        for k in ("credit", "goal_distance", "goal_reached", "goal_facing"):
            if k in info:
                infos[k] = info[k]
        return self._obs(), rews, go.bool().repeat_interleave(R), infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.b.close()
