"""numpy twin of the append-only episode log (csrc/cagym_episode_log.h: cagym_episode_log_update).

The arithmetic is EpisodeRecordsTwin's (tests/episode_records_twin.py, keep="last"): every finished episode writes its pool slot's
row of that table, and the log copies the row out at that moment.  What the log adds is the order and the ring rule: the rows of one
update are appended world-major (ascending world, inside a world ascending slice), updates append in call order, row number i lives
at ring index i % capacity, and an update that finishes n > capacity episodes writes its last `capacity` rows only while head grows
by n.
"""
import numpy as np

from episode_records_twin import EpisodeRecordsTwin

ROW_COLUMNS = ("key", "world", "episode", "slice", "steps", "ret", "outcome", "n_agents", "n_obst", "t", "extra_t", "flags")


class _Recorder(EpisodeRecordsTwin):
    """The table twin, telling its owner of every finished episode."""

    def _finish(self, w, f):
        e = int(self.cursor[w])
        s = int((w + e * self.N) % self.S)
        EpisodeRecordsTwin._finish(self, w, f)
        self.finished.append((w, e, s, {k: np.array(v[s]) for k, v in self.table().items()}))


class EpisodeLogTwin(object):
    def __init__(self, N, M, agents6, n_agents, dt, capacity, n_obst=None, episode0=None):
        self.N, self.M, self.L, self.dt = int(N), int(M), int(capacity), float(dt)
        L = self.L
        self.ring = {"key": np.zeros(L, dtype=np.int64), "world": np.zeros(L, dtype=np.int32), "episode": np.zeros(L, dtype=np.int32),
                     "slice": np.zeros(L, dtype=np.int64), "steps": np.zeros(L, dtype=np.int32), "ret": np.zeros(L),
                     "outcome": np.zeros(L, dtype=np.int32), "n_agents": np.zeros(L, dtype=np.int32),
                     "n_obst": np.zeros(L, dtype=np.int32), "t": np.zeros((L, self.M)), "extra_t": np.zeros((L, self.M)),
                     "flags": np.zeros((L, self.M), dtype=np.uint8)}
        self.written = np.zeros(L, dtype=bool)  # ring indices ever stored to
        self.head = 0
        self.seq = 0
        self.rec = None
        self.set_pool(agents6, n_agents, n_obst, episode0)

    def set_pool(self, agents6, n_agents, n_obst=None, episode0=None):
        """A new pool: the rows stay, the running values are cleared and take the handle's episode indices."""
        self.rec = _Recorder(self.N, self.M, agents6, n_agents, self.dt, episode0=episode0, keep="last")
        self.n_obst = np.zeros(self.rec.S, dtype=np.int32) if n_obst is None else np.asarray(n_obst, dtype=np.int32).reshape(self.rec.S)

    def restart(self, mask=None, episode0=None):
        self.rec.restart(mask, episode0)

    def update(self, flags, reward, game_over):
        T = np.asarray(flags).shape[0]
        rec = self.rec
        rows = []
        for t in range(T):  # slice by slice, to know which slice ended an episode
            rec.finished = []
            rec.update(np.asarray(flags)[t:t + 1], np.asarray(reward)[t:t + 1], np.asarray(game_over)[t:t + 1])
            rows += [(w, self.seq + t, e, s, row) for (w, e, s, row) in rec.finished]
        rows.sort(key=lambda r: (r[0], r[1]))  # world-major
        n = len(rows)
        for j, (w, sl, e, s, row) in enumerate(rows):
            if n - j > self.L:
                continue  # not among the update's last L rows: skipped
            i = (self.head + j) % self.L
            R = self.ring
            R["key"][i] = (w + e * self.N) & 0xFFFFFFFF
            R["world"][i], R["episode"][i], R["slice"][i] = w, e, sl
            R["steps"][i], R["ret"][i], R["outcome"][i] = row["steps"], row["ret"], row["outcome"]
            R["n_agents"][i], R["n_obst"][i] = rec.n_agents[s], self.n_obst[s]
            R["t"][i], R["extra_t"][i], R["flags"][i] = row["t"], row["extra_t"], row["flags"]
            self.written[i] = True
        self.head += n
        self.seq += T
        return n

    def rows(self, last=None, sort=False):
        """The valid rows in append order, oldest first; last: the newest K; sort: by (slice, world)."""
        n = min(self.head, self.L)
        if last is not None:
            n = min(n, max(int(last), 0))
        idx = np.arange(self.head - n, self.head) % self.L
        out = {k: v[idx] for k, v in self.ring.items()}
        if sort:
            order = np.lexsort((out["world"], out["slice"]))
            out = {k: v[order] for k, v in out.items()}
        return out

    def running(self):
        r = self.rec
        atgoal = (r.atgoal_run.astype(np.int64) << np.arange(self.M)[None, :]).sum(axis=1)
        return {"t_run": r.t_run, "ret_run": r.ret_run, "steps_run": r.steps_run, "atgoal_run": atgoal, "cursor": r.cursor}
