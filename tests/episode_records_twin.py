"""numpy twin of the episode recorder (csrc/cagym_episode_records.h: cagym_episode_records_update).

Same inputs as the kernel - flags [T, N, M] u8, reward [T, N, M], game_over [T, N] - plus what the kernel reads from the handle:
the episode index every world was on when recording started (episode0 [N]), the scenario pool (agents6 [S, M, 6], n_agents [S])
and dt.  Slices are walked in order and, inside a slice, worlds in ascending order: with keep="first" the first episode that ends
on a scenario owns its row, with keep="last" the newest one does; every finished episode counts.
"""
import numpy as np

AT_GOAL, IN_COLLISION = 1, 2
OUT_COLLISION, OUT_ALL_AT_GOAL, OUT_STUCK = 1, 2, 4


def straight_line_time(agents6):
    """(|start - goal| - 0.75) / pref_speed (agent.py:59 with the kernels' NEAR_GOAL_THRESHOLD) of rows [..., 6]."""
    a = np.asarray(agents6, dtype=np.float64)
    dx, dy = a[..., 0] - a[..., 2], a[..., 1] - a[..., 3]
    return (np.sqrt(dx * dx + dy * dy) - 0.75) / a[..., 4]


class EpisodeRecordsTwin(object):
    def __init__(self, N, M, agents6, n_agents, dt, episode0=None, keep="first"):
        self.N, self.M = int(N), int(M)
        self.a6 = np.asarray(agents6, dtype=np.float64).reshape(-1, self.M, 6)
        self.S = self.a6.shape[0]
        self.n_agents = np.asarray(n_agents, dtype=np.int64).reshape(self.S)
        self.dt = float(dt)
        assert keep in ("first", "last")
        self.keep = keep
        S, M = self.S, self.M
        self.t = np.zeros((S, M))
        self.extra_t = np.zeros((S, M))
        self.flags = np.zeros((S, M), dtype=np.uint8)
        self.ret = np.zeros(S)
        self.steps = np.zeros(S, dtype=np.int32)
        self.outcome = np.zeros(S, dtype=np.int32)
        self.count = np.zeros(S, dtype=np.int32)
        self.restart(episode0=episode0)

    def restart(self, mask=None, episode0=None):
        """The masked worlds (None = all) forget the episode in progress; episode0: the handle's episode index of every world."""
        N, M = self.N, self.M
        if mask is None:
            mask = np.ones(N, dtype=bool)
        mask = np.asarray(mask).astype(bool)
        if not hasattr(self, "t_run"):
            self.t_run = np.zeros((N, M))
            self.ret_run = np.zeros(N)
            self.steps_run = np.zeros(N, dtype=np.int32)
            self.atgoal_run = np.zeros((N, M), dtype=bool)
            self.cursor = np.zeros(N, dtype=np.int64)
        self.t_run[mask] = 0.0
        self.ret_run[mask] = 0.0
        self.steps_run[mask] = 0
        self.atgoal_run[mask] = False
        if episode0 is not None:
            self.cursor[mask] = np.asarray(episode0, dtype=np.int64).reshape(N)[mask]
        else:
            self.cursor[mask] = 0

    def update(self, flags, reward, game_over):
        flags = np.asarray(flags)
        T = flags.shape[0]
        flags = flags.reshape(T, self.N, self.M).astype(np.uint8)
        reward = np.asarray(reward).reshape(T, self.N, self.M).astype(np.float64)  # fp32 -> fp64 is exact
        game_over = np.asarray(game_over).reshape(T, self.N)
        for t in range(T):
            f = flags[t]
            self.t_run = np.where(self.atgoal_run, self.t_run, self.t_run + self.dt)
            self.atgoal_run = (f & AT_GOAL) != 0
            self.steps_run += 1
            self.ret_run = self.ret_run + reward[t, :, 0]
            for w in np.nonzero(game_over[t])[0]:
                self._finish(int(w), f[w])

    def _finish(self, w, f):
        s = int((w + int(self.cursor[w]) * self.N) % self.S)
        if self.keep == "last" or self.count[s] == 0:
            n = int(self.n_agents[s])
            act = np.arange(self.M) < n
            t = np.where(act, self.t_run[w], 0.0)
            self.t[s] = t
            sl = np.zeros(self.M)
            sl[:n] = straight_line_time(self.a6[s, :n])
            self.extra_t[s] = np.where(act, t - sl, 0.0)
            self.flags[s] = np.where(act, f, 0).astype(np.uint8)
            self.ret[s] = self.ret_run[w]
            self.steps[s] = self.steps_run[w]
            coll, goal = (f[:n] & IN_COLLISION) != 0, (f[:n] & AT_GOAL) != 0
            self.outcome[s] = (OUT_COLLISION if coll.any() else 0) | (OUT_ALL_AT_GOAL if goal.all() else 0) | \
                              (OUT_STUCK if (~coll & ~goal).any() else 0)
        self.count[s] += 1
        self.t_run[w] = 0.0
        self.ret_run[w] = 0.0
        self.steps_run[w] = 0
        self.atgoal_run[w] = False
        self.cursor[w] += 1

    def table(self):
        return {k: getattr(self, k) for k in ("t", "extra_t", "flags", "ret", "steps", "outcome", "count")}
