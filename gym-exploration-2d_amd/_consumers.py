"""The consumers of BatchedCollisionAvoidanceEnv's step outputs - per-scenario episode records, the append-only episode log, the
trajectory ring, the IG team's episode log - and the terminal observations.  They share one contract (include/cagym.h): fed by
auto-reset stepping only, every step once and in order, a desync word that counts what went past them, a restart with reset()."""
import collections

import torch

from . import _lib

# One row per consumer.  attr: the env's field that is not None while it is attached; noun: how its messages name it; detach: the
# method that stops feeding it; fed: why it needs auto-reset stepping; timeline: why restore() / fork() refuse beside it (None: only
# the library does); desync: what a non-zero desync word (%d) means.  The messages are put together from these when they are raised.
_Consumer = collections.namedtuple("_Consumer", "attr noun detach fed timeline desync")
_RING = _Consumer(
    "_traj", "a trajectory ring", "detach_trajectory_ring", "the ring is fed by cagym_step_autoreset_keep only",
    "its running values would describe another timeline (the library refuses as long as the ring is initialised)",
    "the trajectory ring is out of step with the env (desync: %d agent-steps went past it): the env was stepped through another "
    "entry than step(auto_reset=True) / rollout(auto_reset=True)")
_LOG = _Consumer(
    "_log", "an episode log", "detach_episode_log", "cagym_episode_log_update takes the outputs of auto-reset stepping only",
    "its running rows would describe another timeline (the library refuses as long as the log is initialised)",
    "the episode log is out of step with the env in %d world-launches (desync): the recorder was fed a step twice, skipped one, "
    "or saw a step without auto-reset")
_REC = _Consumer(
    "_rec", "episode records", "detach_episode_records", "cagym_episode_records_update takes the outputs of auto-reset stepping only",
    None,
    "episode records are out of step with the env in %d world-launches (desync): the recorder was fed a step twice, skipped one, "
    "or saw a step without auto-reset")
_IGLOG = _Consumer(
    "_iglog", "an IG episode log", "detach_ig_episode_log", "cagym_ig_episode_log_update goes behind the auto-resetting step only",
    None,
    "the IG episode log is out of step with the env in %d world-launches (desync): it was fed a step twice, skipped one, or saw a "
    "step without auto-reset")
_CONSUMERS = (_RING, _LOG, _REC, _IGLOG)  # the order in which their auto_reset=False refusals compete


class _ConsumersMixin(object):
    def _init_consumers(self):
        L = self.L  # (the calls inside per-step loops, resolved once)
        self._records_fn, self._log_fn, self._keep_fn = L.cagym_episode_records_update, L.cagym_episode_log_update, L.cagym_step_autoreset_keep
        self._rec = None          # keep mode of attach_episode_records, None while detached
        self._rec_views = None
        self._rec_priv = {}       # rollout buffers of a caller whose `out` lacks reward / flags / game_over
        self._log = None          # capacity of attach_episode_log, None while detached
        self._log_views = None
        self._term = None         # keep_terminal_observations: {"other_agents_states", "ego", "laserscan"} env-owned tensors
        self._term_c = None       # ... as the cagym_terminal_outputs step() passes
        self._traj = None         # n_slices of attach_trajectory_ring, None while detached
        self._traj_views = None
        self._iglog_fn = L.cagym_ig_episode_log_update
        self._iglog = None        # capacity of attach_ig_episode_log, None while detached
        self._iglog_views = None

    def _records_contract(self, auto_reset, what):
        if not auto_reset and any(getattr(self, c.attr) is not None for c in _CONSUMERS):
            c = next(c for c in _CONSUMERS if getattr(self, c.attr) is not None)
            raise RuntimeError("%s(auto_reset=False) with %s attached: %s, every step exactly once and in order (include/cagym.h); "
                               "%s() first" % (what, c.noun, c.fed, c.detach))

    def _refuse_without(self, what, c):
        if getattr(self, c.attr) is None:
            raise RuntimeError("%s() without %s: %s() first" % (what, c.noun, c.detach.replace("detach", "attach", 1)))

    @staticmethod
    def _check_desync(c, d, check=True):
        if check and d:
            raise RuntimeError((c.desync + "; %s() again to clear") % (d, c.detach.replace("detach", "attach", 1)))

    def _after_steps(self, auto_reset, flags, reward, game_over, T):
        """What follows the step launch(es) of one call on the stream, in this order: the episode log's update (it reads the pool
        slot of the episode that ended, which the refill regenerates next), the replay harvest (attach_replay with outcomes: it reads
        the rows the update appended and the key table of the same slots), the stream's refill, the records' update."""
        if self._log is not None:
            rc = self._log_fn(self.h, flags.data_ptr(), reward.data_ptr(), game_over.data_ptr(), int(T), self._stream())
            if rc:
                _lib.check(self.L, self.h, rc, "cagym_episode_log_update")
            if self._replay is not None and self._replay["mask"]:
                self._harvest()
        if self._streaming and auto_reset:
            self._refill()
        if self._rec is not None:
            self._records_update(flags, reward, game_over, T)

    # ---- per-scenario episode records (include/cagym.h: cagym_episode_records_*) ---------------------------------------------
    def attach_episode_records(self, keep="first"):
        """From now on every auto-resetting step is followed, on the same stream, by ONE cagym_episode_records_update launch
        that rebuilds from the step's outputs what the reference reads from prev_episode_agents at the end of an episode
        (experiments/src/env_utils.py:41-62): per scenario of the pool the agents' t and extra time to goal, terminal flags,
        agent 0's return, the step count and the outcome bits.  step / step_finish / step_overlapped with auto_reset=True and
        rollout(auto_reset=True) (single launch, GA3C chain and episodic IG chain) feed it; CagymVecEnv inherits it through
        step().  keep="first": a row is written by the first episode that ends on its scenario (a suite's table is complete
        once episode_records()["count"].min() >= 1); keep="last": the newest finished episode overwrites it (training
        monitors).  The recorder takes every step exactly once and in order, so step(auto_reset=False) and
        rollout(auto_reset=False) are refused while attached.  Attaching again clears the table.  Needs a scenario pool."""
        if keep not in _lib.EPREC_KEEP:
            raise ValueError("attach_episode_records: keep must be 'first' or 'last', got %r" % (keep,))
        self._refuse_streaming("attach_episode_records", "the records table has one row per pool slot, and a streamed pool reuses its slots")
        _lib.call(self.L, self.h, "cagym_episode_records_init", _lib.EPREC_KEEP[keep], self._stream())
        self._rec = keep
        return self

    def detach_episode_records(self):
        """Stop feeding the recorder (its table stays readable through the C ABI; attach again to clear and resume)."""
        self._rec = None

    def _records_update(self, flags, reward, game_over, T):
        rc = self._records_fn(self.h, flags.data_ptr(), reward.data_ptr(), game_over.data_ptr(), int(T), self._stream())
        if rc:
            _lib.check(self.L, self.h, rc, "cagym_episode_records_update")

    def _records_out(self, out, n_steps):
        """reward / flags / game_over slices for the recorder: the caller's, or private ones where `out` has none."""
        if self._rec is None and self._log is None:
            return out
        T = int(n_steps)
        shapes = {"reward": ((T, self.N, self.M), torch.float32), "flags": ((T, self.N, self.M), torch.uint8),
                  "game_over": ((T, self.N), torch.uint8)}
        full = dict(out)
        for k, (shape, dt) in shapes.items():
            if full.get(k) is None:
                buf = self._rec_priv.get(k)
                if buf is None or tuple(buf.shape) != shape:
                    buf = self._rec_priv[k] = torch.empty(shape, dtype=dt, device=self.device)
                full[k] = buf
        return full

    def restart_episode_records(self, world_mask=None, clear_table=False):
        """The masked worlds (None = all) forget the episode in progress; clear_table also empties the table and desync."""
        m = self._mask(world_mask)
        _lib.call(self.L, self.h, "cagym_episode_records_restart", _lib.ptr(m), int(bool(clear_table)), self._stream())

    def episode_records(self, check=True):
        """Zero-copy device views of the recorder: the table t / extra_t [S, M] f64, flags [S, M] u8, ret [S] f64, steps /
        outcome / count [S] i32, the running t_run [N, M], ret_run, steps_run, atgoal_run, cursor [N], and desync [1].  Raises
        RuntimeError when the recorder saw a skipped, doubled or non-auto-reset step (desync != 0; this synchronises).  The pool's
        n_agents [S] rides along for stats.suite_statistics."""
        if self._rec_views is None:
            v = self._get_views("cagym_episode_records_get", _lib.CagymEpisodeRecordPtrs(), _lib.EPREC_FIELDS)
            v["n_agents"] = self.scenarios()["n_agents"]
            self._rec_views = v
        if check:
            self._check_desync(_REC, int(self._rec_views["desync"].item()))
        return dict(self._rec_views)

    # ---- append-only episode log (include/cagym.h: cagym_episode_log_*) --------------------------------------------------------
    def attach_episode_log(self, capacity=65536):
        """From now on every auto-resetting step / rollout is followed, on the same stream, by one cagym_episode_log_update: ONE ROW
        PER FINISHED EPISODE in a device ring of `capacity` rows (the newest overwrite the oldest).  Unlike the per-scenario
        records it is not keyed by pool slot, so it works on any pool and under stream_reference_scenarios: a row names its
        episode by key = (uint32)(world + episode * N), the stream key its scenario was drawn for, and carries world, episode,
        slice, steps, ret, outcome, n_agents, n_obst, t / extra_t / flags [M].  The same paths feed it as the records (step,
        step_finish, step_overlapped, rollout in its three forms, CagymVecEnv.step), in the order step(s), log update, stream
        refill, records update; step(auto_reset=False) and rollout(auto_reset=False) are refused while attached, and so are
        restore() and fork() (snapshot() is not).  Records and log may be attached together on a fixed pool.  A world that lapped
        its ring inside a rollout logs the scenario that actually ran under the key of the one it should have met:
        stream_stats()["n_lapped"] tells.  Attaching again clears the log and may change the capacity.  Needs a scenario pool."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("attach_episode_log: capacity must be >= 1, got %d" % capacity)
        _lib.call(self.L, self.h, "cagym_episode_log_init", capacity, self._stream())
        self._log, self._log_views = capacity, None
        return self

    def detach_episode_log(self):
        """Stop feeding the log (the library keeps it, and keeps refusing restore / fork; attach again to clear and resume)."""
        self._log = None

    def clear_episode_log(self):
        """Empty the log: every row, head, the slice counter and desync; every world forgets the episode in progress."""
        self._refuse_without("clear_episode_log", _LOG)
        _lib.call(self.L, self.h, "cagym_episode_log_restart", None, 1, self._stream())

    def episode_log_views(self):
        """Zero-copy device views of the ring and its words, no synchronisation: key (u32 bits as int32), world, episode, steps,
        outcome, n_agents, n_obst [L] i32, slice [L] i64, ret [L] f64, t / extra_t [L, M] f64, flags [L, M] u8, the running t_run
        [N, M], ret_run, steps_run, atgoal_run, cursor [N], head [1] i64 (rows ever appended; row i lives at index i % L) and
        desync [1]."""
        self._refuse_without("episode_log_views", _LOG)
        if self._log_views is None:
            self._log_views = self._get_views("cagym_episode_log_get", _lib.CagymEpisodeLogPtrs(), _lib.EPLOG_FIELDS, "capacity")
        return dict(self._log_views)

    def episode_log(self, last=None, sort=False, check=True):
        """The valid rows in append order, oldest first, as device tensors (copies): the columns of episode_log_views() with key
        as int64 in [0, 2^32), plus count (int32 ones) so that stats.suite_statistics(env.episode_log(last=K)) works on a window.
        One synchronisation, to read head.  last=K: the newest K rows only; sort=True: ordered by (slice, world) instead;
        check: raise RuntimeError when the log saw a skipped, doubled or non-auto-reset step (desync != 0)."""
        v = self.episode_log_views()
        L = self._log
        head, d = torch.cat([v["head"], v["desync"].to(torch.int64)]).tolist()
        self._check_desync(_LOG, d, check)
        n = min(head, L)
        if last is not None:
            n = min(n, max(int(last), 0))
        idx = (torch.arange(head - n, head, dtype=torch.int64, device=self.device) % L)
        rows = {k: v[k].index_select(0, idx) for k, _, shape in _lib.EPLOG_FIELDS if shape in ("L", "LM")}
        rows["key"] = rows["key"].to(torch.int64) & 0xFFFFFFFF
        if sort and n:
            order = torch.argsort(rows["slice"] * self.N + rows["world"].to(torch.int64), stable=True)
            rows = {k: t.index_select(0, order) for k, t in rows.items()}
        rows["count"] = torch.ones((n,), dtype=torch.int32, device=self.device)
        return rows

    # ---- the IG team's episode log (include/cagym.h: cagym_ig_episode_log_*) ---------------------------------------------------
    def attach_ig_episode_log(self, capacity=65536, p_found=0.75):
        """From now on every auto-resetting step of an IG team is followed, on the same stream and BEFORE the launch that restarts a
        finished world's belief, by one cagym_ig_episode_log_update: ONE ROW PER FINISHED TEAM EPISODE in a device ring of
        `capacity` rows (the newest overwrite the oldest), with what a target search is judged by.  A row names its episode by
        key = (uint32)(world + episode * N), the stream key its world was drawn for - the same key on every handle of the same
        stream seed, whatever policy drives it (stats.paired_by_key) - and carries world, episode, slice, steps, ret (the team
        return, bit for bit ig_episode_stats()["last"]), n_targets, n_found, found_at [M] (-2: the slot is no target, -1: a target
        never found, else the 1-based step at which the odds of its belief cell first reached p_found / (1 - p_found)), entropy
        (nats, over the 3600 cells), residual_mi (the MI still to be gained) and n_touched (cells off the prior), all of the
        belief the episode ended on.  The targets are the STATIC agents of the episode's pool slot.  ig.episode_log_spec states
        the belief columns in numpy, stats.exploration_statistics summarises a log.
        Needs an IG attach that restarts per world - attach_ig_learner, or attach_ig_mcts / attach_ig_greedy with episodic=True -
        and stays attached when one such attach replaces another.  step() and rollout() feed it through the same chain;
        CagymVecEnv inherits it.  reset() restarts every world's running values (rows kept), reset(world_mask=m) the masked
        worlds'.  step(auto_reset=False) and rollout(auto_reset=False) are refused while attached; the library refuses restore /
        fork while the log is initialised.  A world that lapped its ring inside a rollout logs the scenario that actually ran
        under the key of the one it should have met: stream_stats()["n_lapped"] tells.  Attaching again clears the log and may
        change capacity and p_found."""
        capacity, p_found = int(capacity), float(p_found)
        if capacity < 1:
            raise ValueError("attach_ig_episode_log: capacity must be >= 1, got %d" % capacity)
        if not 0.0 < p_found < 1.0:
            raise ValueError("attach_ig_episode_log: p_found must lie inside (0, 1), got %r" % (p_found,))
        if self._igm is None or not self._igm.episodic:
            raise RuntimeError("attach_ig_episode_log() needs an IG attach that restarts per world: attach_ig_learner(), or "
                               "attach_ig_mcts / attach_ig_greedy with episodic=True")
        _lib.call(self.L, self.h, "cagym_ig_episode_log_init", capacity, p_found / (1.0 - p_found), self._stream())
        self._iglog, self._iglog_views = capacity, None
        return self

    def detach_ig_episode_log(self):
        """Stop feeding the log (the library keeps it, and keeps refusing restore / fork; attach again to clear and resume)."""
        self._iglog = None

    def clear_ig_episode_log(self):
        """Empty the log: every row, head, the call counter and desync; every world forgets the episode in progress."""
        self._refuse_without("clear_ig_episode_log", _IGLOG)
        _lib.call(self.L, self.h, "cagym_ig_episode_log_restart", None, 1, self._stream())

    def _ig_log_update(self, game_over, team_reward):
        """Behind the step launch that wrote game_over, before the team's boundary / observe launch; team_reward: what that
        boundary launch is given (None behind a learner's step)."""
        rc = self._iglog_fn(self.h, game_over.data_ptr(), _lib.ptr(team_reward), self._stream())
        if rc:
            _lib.check(self.L, self.h, rc, "cagym_ig_episode_log_update")

    def ig_episode_log_views(self):
        """Zero-copy device views of the ring and its words, no synchronisation: key (u32 bits as int32), world, episode, steps,
        n_targets, n_found, n_touched [L] i32, slice [L] i64, ret, entropy, residual_mi [L] f64, found_at [L, M] i32, the running
        steps_run, cursor [N], found_run [N, M] i32, head [1] i64 (rows ever appended; row i lives at index i % L), desync [1]."""
        self._refuse_without("ig_episode_log_views", _IGLOG)
        if self._iglog_views is None:
            self._iglog_views = self._get_views("cagym_ig_episode_log_get", _lib.CagymIgEpisodeLogPtrs(), _lib.IGLOG_FIELDS, "capacity")
        return dict(self._iglog_views)

    def ig_episode_log(self, last=None, check=True):
        """The valid rows in append order, oldest first, as device tensors (copies): the ring columns of ig_episode_log_views()
        with key as int64 in [0, 2^32).  One synchronisation, to read head.  last=K: the newest K rows only; check: raise
        RuntimeError when the log saw a skipped, doubled or non-auto-reset step (desync != 0)."""
        v = self.ig_episode_log_views()
        L = self._iglog
        head, d = torch.cat([v["head"], v["desync"].to(torch.int64)]).tolist()
        self._check_desync(_IGLOG, d, check)
        n = min(head, L)
        if last is not None:
            n = min(n, max(int(last), 0))
        idx = (torch.arange(head - n, head, dtype=torch.int64, device=self.device) % L)
        rows = {k: v[k].index_select(0, idx) for k, _, shape in _lib.IGLOG_FIELDS if shape in ("L", "LM")}
        rows["key"] = rows["key"].to(torch.int64) & 0xFFFFFFFF
        return rows

    # ---- terminal observations and the trajectory ring (include/cagym.h: cagym_step_autoreset_keep, cagym_trajectory_*) ---------
    def _refuse_keep(self, what, why):
        if self._term is not None or self._traj is not None:
            on = "a trajectory ring attached" if self._traj is not None else "keep_terminal_observations() on"
            raise RuntimeError("%s() with %s: %s" % (what, on, why))

    def _refuse_keep_with_planner(self, what):
        if self._igm is not None:
            raise RuntimeError("%s() with %s attached: an attached IG planner's per-world restart reads the game_over of the "
                               "auto-resetting launch; the three-launch step has not been taken through it; detach_ig_mcts() first"
                               % (what, self._igm.kind))

    def _refuse_split_keep(self, auto_reset, what):
        if auto_reset:
            self._refuse_keep("%s(auto_reset=True)" % what, "the split step ends in the auto-resetting launch, which overwrites the "
                              "terminal observation and the terminal state; use step(auto_reset=True)")

    def keep_terminal_observations(self, on=True):
        """From now on step(auto_reset=True) keeps the observation every finished world ENDED on, which the auto-reset overwrites with
        the first one of the new episode: info["terminal"] = {"other_agents_states" [N, M, M-1, 10], "ego" [N, M, 12], "laserscan"
        [N, M, 16] (with a LaserScan sensor), "valid": game_over}.  The tensors are the env's own and are rewritten in place; a
        world's rows are meaningful where `valid` is set and otherwise hold what its last finished episode left (zeros before
        the first).  The step then runs as three launches with the same results, bit for bit (cagym_step_autoreset_keep: step,
        capture, reset of the finished worlds).  step_finish / step_overlapped with auto_reset=True and an attached IG planner are
        refused while it is on; rollout() stays the single launch and returns no terminal observations.  on=False switches back."""
        if not on:
            self._term = self._term_c = None
            return self
        self._refuse_keep_with_planner("keep_terminal_observations")
        t = {"other_agents_states": torch.zeros_like(self.obs_oas), "ego": torch.zeros_like(self.obs_ego)}
        if self.laserscan:
            t["laserscan"] = torch.zeros_like(self.obs_laser)
        self._term = t
        self._term_c = _lib.CagymTerminalOutputs(t["other_agents_states"].data_ptr(), t["ego"].data_ptr(), _lib.ptr(t.get("laserscan")))
        return self

    def attach_trajectory_ring(self, n_slices):
        """From now on every step(auto_reset=True) adds one slice to a device ring of n_slices steps: per agent that moved, the
        reference's global_state_history row [t_before, px, py, gx, gy, radius, pref_speed, vx, vy, speed, heading, a0, a1]
        (agent.py:198-201: the state AFTER the move, the time stamp of before it), the terminal row of every episode included,
        plus the world's episode index and game_over.  trajectory(world, episode) reads an episode back, dataset.export_ring
        writes the reference's trajectory pickle.  The step runs as three launches with the same results (see
        keep_terminal_observations), and rollout(auto_reset=True) as the chain of such steps (see rollout).  The ring takes every
        step exactly once and in order: step(auto_reset=False), rollout(auto_reset=False), step_finish / step_overlapped with
        auto_reset=True, restore(), fork() and an attached IG planner are refused while attached.  A ring attached in mid-episode
        starts there.  Attaching again clears the ring and may change n_slices.  Needs a scenario pool."""
        n_slices = int(n_slices)
        if n_slices < 1:
            raise ValueError("attach_trajectory_ring: n_slices must be >= 1, got %d" % n_slices)
        self._refuse_keep_with_planner("attach_trajectory_ring")
        _lib.call(self.L, self.h, "cagym_trajectory_init", n_slices, self._stream())
        self._traj, self._traj_views = n_slices, None
        return self

    def detach_trajectory_ring(self):
        """Stop feeding the ring (the library keeps it, and keeps refusing restore / fork; attach again to clear and resume)."""
        self._traj = None

    def trajectory_views(self):
        """Zero-copy device views of the ring, no synchronisation: rows [L, 13, N, M] f64 (column planes, _lib.TRAJ_COLUMNS),
        moved [L, N, M] u8, episode [L, N] i32, last [L, N] u8, head [1] i64 (slices ever written; slice i lives at index i % L),
        desync [1] i32, and the ring's running t_prev [N, M] f64, seen [N, M] i32."""
        self._refuse_without("trajectory_views", _RING)
        if self._traj_views is None:
            self._traj_views = self._get_views("cagym_trajectory_get", _lib.CagymTrajectoryPtrs(), _lib.TRAJ_FIELDS, "n_slices")
        return dict(self._traj_views)

    def trajectory(self, world, episode, check=True):
        """The slices of episode `episode` of world `world` that are still in the ring, oldest first, as host arrays: "history"
        [T, M, 13] (a row is meaningful where `moved`), "moved" [T, M] bool, "complete": the episode's first row and its `last`
        slice (the step that set game_over) are both present.  One synchronisation.  check: raise RuntimeError when a step went
        past the ring (desync != 0)."""
        from . import dataset
        v = self.trajectory_views()
        w = int(world)
        if not 0 <= w < self.N:
            raise ValueError("trajectory: world must lie in [0, %d), got %d" % (self.N, w))
        head, d = torch.cat([v["head"], v["desync"].to(torch.int64)]).tolist()
        self._check_desync(_RING, d, check)
        planes = {"rows": v["rows"][:, :, w:w + 1].cpu().numpy(), "moved": v["moved"][:, w:w + 1].cpu().numpy(),
                  "episode": v["episode"][:, w:w + 1].cpu().numpy(), "last": v["last"][:, w:w + 1].cpu().numpy(), "head": head}
        H, mv, complete = dataset.ring_slices(planes, 0, int(episode))
        return {"history": H, "moved": mv, "complete": complete}
