"""The scenario pool of BatchedCollisionAvoidanceEnv: setters, on-device generators, both streams and their stats."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import scenarios as sc


def _kinds_obst(kinds, n_obst):
    """(the sampler kinds as a list, their kinds_mask, n_obst_min, n_obst_max) of a generator's `kinds` and `n_obst` arguments."""
    ks = [kinds] if isinstance(kinds, (str, int, np.integer)) else list(kinds)
    mask = sum(1 << k for k in {sc.sampler_kind(k) for k in ks})
    lo, hi = (-1, -1) if n_obst is None else (n_obst, n_obst) if np.isscalar(n_obst) else n_obst
    return ks, mask, int(lo), int(hi)


class _PoolMixin(object):
    def _init_pool(self):
        self._refill_fn = self.L.cagym_stream_refill  # (called inside per-step loops: resolved once)
        self._pool_policies = set()  # what the pool holds
        self._n_ig = None         # IG robots per scenario (-1: the scenarios differ; None: a generated pool)
        self._streaming = False   # stream_reference_scenarios: one cagym_stream_refill behind every episode-advancing call
        self._stream_views = None
        self._explore_views = None
        self._replay = None       # attach_replay: {"capacity", "p", "mask"} while the stream's replay is armed
        self._replay_views = None
        self._harvest_fn = self.L.cagym_stream_replay_harvest

    def _pool_committed(self, streaming, policies, n_ig):
        """Host state after a pool was committed (as the library: a new pool ends the stream unless it starts one).  An attached IG
        team is detached when the team size is unknown (a generated pool's robot count is not known on the host) or the planner was
        sized for another team; else it gets fresh beliefs on the new rasters' fields (cagym_ig_init; on a stream it arms the refresh)."""
        self._streaming, self._pool_policies, self._n_ig = streaming, policies, n_ig
        self._replay = None  # (a new stream starts un-armed)
        if n_ig is None or (self._igm is not None and n_ig != self._igm.R):
            self.detach_ig_mcts()
        if self._igm is not None:
            _lib.call(self.L, self.h, "cagym_ig_init", self._stream())

    def _generate(self, fn, P, pols, n_ig, streaming, check=True):
        """One generator call of the C ABI and the pool's commit; returns n_failed when check."""
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, fn, C.byref(P), C.byref(nf) if check else None, self._stream())
        self._pool_committed(streaming, pols, n_ig)
        return int(nf.value) if check else None

    # ---- scenarios (set_agents / _init_agents / _init_static_map) ---------------------------------
    def set_scenarios(self, agents6, policy_id, dynamics_id, heading0=None, n_agents=None, coop=None,
                      obstacles=None, n_obst=None):
        S, M = self.S, self.M
        a6 = np.ascontiguousarray(np.asarray(agents6, dtype=np.float64).reshape(S, M, 6))
        pol = np.ascontiguousarray(np.broadcast_to(np.asarray(policy_id, dtype=np.int32), (S, M)))
        dyn = np.ascontiguousarray(np.broadcast_to(np.asarray(dynamics_id, dtype=np.int32), (S, M)))
        opt = lambda x, dt, shape: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dt).reshape(shape))
        h0 = opt(heading0, np.float64, (S, M))
        na = opt(n_agents, np.int32, (S,))
        co = opt(coop, np.float64, (S, M))
        ob = no = None
        if obstacles is not None and self.Kobs:
            o = np.asarray(obstacles, dtype=np.float64).reshape(S, -1, 4)
            ob = np.zeros((S, self.Kobs, 4), dtype=np.float64)
            ob[:, :o.shape[1]] = o
            no = np.ascontiguousarray(np.asarray(n_obst, dtype=np.int32).reshape(S))
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        _lib.call(self.L, self.h, "cagym_set_scenarios", p(a6), p(h0), p(pol), p(dyn), p(na), p(co), p(ob), p(no), self._stream())
        live = np.arange(M)[None, :] < (na if na is not None else np.full(S, M))[:, None]
        counts = ((pol == sc.POLICY_IGMCTS) & live).sum(axis=1)
        self._pool_committed(False, set(np.unique(pol[live]).tolist()), int(counts[0]) if (counts == counts[0]).all() else -1)

    def generate_scenarios(self, seed, n_agents=None, ego_policy=5, ego_dynamics=0, other_policies=(5, 1), p_b=0.5,
                           other_dynamics=0, side=7.5, min_travel=4.0, min_sep=1.5, radius=0.5, pref_speed=1.0,
                           coop=0.5, max_tries=100000, check=True):
        """Fill the scenario pool ON DEVICE with the rule of train_agents_random_positions (test_cases.py:1362-1463):
        no host sampling, no upload.  n_agents = int or (min, max); agent 0 gets (ego_policy, ego_dynamics), every
        other agent other_policies[1] with probability p_b else other_policies[0].  Returns the number of agents
        whose rejection loop hit max_tries (0 in any sane configuration) when check=True."""
        if n_agents is None:
            n_agents = self.M
        n_min, n_max = (n_agents, n_agents) if np.isscalar(n_agents) else n_agents
        P = _lib.CagymGenParams(int(seed), int(n_min), int(n_max), int(ego_policy), int(ego_dynamics),
                                int(other_policies[0]), int(other_policies[1]), int(other_dynamics), int(max_tries),
                                float(p_b), float(side), float(min_travel), float(min_sep), float(radius),
                                float(pref_speed), float(coop))
        return self._generate("cagym_generate_scenarios", P, {int(ego_policy), int(other_policies[0]), int(other_policies[1])},
                              None, False, check)

    def generate_reference_scenarios(self, kinds, seed, number_of_agents=None, fixed_count=False, ego_policy=5, ego_dynamics=4,
                                     other_policies=None, p_b=None, other_dynamics=0, n_obst=None, max_tries=1000, check=True):
        """Fill the scenario pool ON DEVICE with the reference's own training samplers (cagym_generate_reference_scenarios):
        kinds = one test_cases.py sampler name or scenarios.GEN_* id, or several (every scenario then draws one uniformly, as
        _init_agents' np.random.randint stage does; scenarios.reference_curriculum gives the set of a training step).
        number_of_agents: the samplers' argument (default max_agents); fixed_count takes the top of its range (the seeded branch).
        ego_dynamics / other_dynamics default to the samplers' FirstOrder / Unicycle; a GA3C ego of the swap and random-position
        samplers gets UnicycleDynamicsMaxAcc as there.  other_policies=None keeps each sampler's rule (80/20 RVO / NonCooperative,
        50/50 for random positions, RVO only among rectangles); a pair (a, b) with p_b gives every non-ego agent b with
        probability p_b else a, a single id all of them.  n_obst=(min, max) narrows the stage samplers' rectangle counts
        ((0, 4) / (2, 10); None or a negative bound: none): n_obst=(-1, 6) caps stage 2 at 6 and leaves stage 1 at 0..4.  A count
        that can exceed max_obstacles is refused.  max_tries bounds every rejection loop: the reference's loops are unbounded,
        and a world that leaves no room for an agent (ten agents among ten stage-2 rectangles can) spins its lane to the bound -
        1000 keeps a pool of 8192 stage-2 worlds near 10 ms, 100000 takes about 0.3 s.  Returns the number of agents and
        rectangles whose rejection loop hit max_tries (they keep their last draw) when check=True."""
        P, pols = self._gen2_params(kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                                    other_dynamics, n_obst, max_tries)
        return self._generate("cagym_generate_reference_scenarios", P, pols, None, False, check)

    def _gen2_params(self, kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                     other_dynamics, n_obst, max_tries):
        """generate_reference_scenarios' arguments as (cagym_gen2_params, the policies the scenarios may hold)."""
        ks, mask, lo, hi = _kinds_obst(kinds, n_obst)
        if number_of_agents is None:
            number_of_agents = self.M
        own = other_policies is not None
        if not own:
            pa, pb, pp = sc.POLICY_RVO, sc.POLICY_NONCOOP, 0.0
        elif np.isscalar(other_policies):
            pa = pb = int(other_policies)
            pp = 0.0
        else:
            pa, pb = int(other_policies[0]), int(other_policies[1])
            pp = 0.5 if p_b is None else float(p_b)
        P = _lib.CagymGen2Params(int(seed), mask, int(number_of_agents), int(bool(fixed_count)), int(ego_policy),
                                 int(ego_dynamics), int(own), pa, pb, int(other_dynamics), lo, hi, int(max_tries), pp)
        # the policies the pool may hold
        pols = {int(ego_policy)}
        for k in {sc.sampler_kind(k) for k in ks}:
            if own:
                pols |= {pa} if pp < 1.0 else set()
                pols |= {pb} if pp > 0.0 else set()
            else:
                pols |= {sc.POLICY_RVO} if k >= sc.GEN_STAGE_1 else {sc.POLICY_RVO, sc.POLICY_NONCOOP}
        return P, pols

    # ---- streamed scenarios (include/cagym.h: cagym_stream_*) -------------------------------------------------------------------
    def stream_reference_scenarios(self, kinds, seed, number_of_agents=None, fixed_count=False, ego_policy=5, ego_dynamics=4,
                                   other_policies=None, p_b=None, other_dynamics=0, n_obst=None, max_tries=1000, check=True):
        """generate_reference_scenarios (same arguments, same pool), and from now on the pool is a ring of depth
        k = n_scenarios / n_worlds per world that is refilled behind the stepping calls: world w's episode e runs on the scenario
        the samplers draw for key w + e * N - row w + e * N of a plain pool generated with the same arguments, however large e
        gets - instead of replaying the pool after k episodes (the reference draws a fresh world at every reset()).  One
        cagym_stream_refill launch is enqueued on the current stream behind every call that can advance an episode counter:
        step / step_finish / step_overlapped with auto_reset=True, rollout(auto_reset=True) (once, behind its last step) and
        reset(advance_episode=True); CagymVecEnv inherits it through step().  A world that finished nothing costs the launch two
        loads.  Needs n_scenarios to be a multiple of n_worlds and >= 2 * n_worlds; refused on handles with information-gain
        state, for IG_MCTS agents and while episode records are attached.  While streaming, restore(), fork() and
        attach_episode_records() raise.  set_scenarios / generate_* / stop_streaming() end it.  Returns n_failed as
        generate_reference_scenarios does when check=True."""
        P, pols = self._gen2_params(kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                                    other_dynamics, n_obst, max_tries)
        return self._generate("cagym_stream_scenarios", P, pols, None, True, check)

    def set_stream_params(self, kinds, seed, number_of_agents=None, fixed_count=False, ego_policy=5, ego_dynamics=4,
                          other_policies=None, p_b=None, other_dynamics=0, n_obst=None, max_tries=1000):
        """The reference's curriculum switch (collision_avoidance_env.py:419-438) on a streaming env: the slots that later refills
        generate come from this sampler set (scenarios.reference_curriculum gives the set of a training step); the seed may change
        too.  Scenarios already in the ring stay, so a world meets the new set n_scenarios / n_worlds - 1 episodes later."""
        P, pols = self._gen2_params(kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                                    other_dynamics, n_obst, max_tries)
        _lib.call(self.L, self.h, "cagym_stream_set_params", C.byref(P))
        self._pool_policies = self._pool_policies | pols

    def _refuse_streaming(self, what, why):
        if self._streaming:
            raise RuntimeError("%s() on a streaming env: %s; stop_streaming() first" % (what, why))

    def stop_streaming(self):
        """End the stream: the pool stays as it is and is replayed from here on, as a fixed pool is."""
        _lib.call(self.L, self.h, "cagym_stream_stop")
        self._streaming = False
        self._replay = None

    def stream_stats(self):
        """Host integers of the stream (this synchronises): generated (slots generated since stream_reference_scenarios, its first
        fill included), n_failed (rejection loops that hit max_tries), n_lapped (times a world started an episode on a slot that
        had not been refilled: only a rollout in which a world finishes more than depth - 1 episodes does that), depth."""
        if self._stream_views is None:
            self._stream_views = self._get_views("cagym_stream_get", _lib.CagymStreamPtrs(), _lib.STREAM_FIELDS)
        v = self._stream_views
        return {"generated": int(v["generated"].item()), "n_failed": int(v["n_failed"].item()), "n_lapped": int(v["n_lapped"].item()),
                "depth": self.S // self.N}

    def stream_next_episode(self):
        """Zero-copy device view of next_episode [N] i32: the first episode of each world whose slot has not been generated."""
        self.stream_stats()
        return self._stream_views["next_episode"]

    # ---- replay of failed scenarios (include/cagym.h: cagym_stream_replay_*) ------------------------------------------------------
    @staticmethod
    def _outcome_mask(outcomes):
        names = [outcomes] if isinstance(outcomes, str) else list(outcomes or ())
        bad = [n for n in names if n not in _lib.REPLAY_OUTCOMES]
        if bad:
            raise ValueError("replay outcomes must be among %s, got %r" % (", ".join(sorted(_lib.REPLAY_OUTCOMES)), bad[0]))
        return sum({_lib.REPLAY_OUTCOMES[n] for n in names})

    def attach_replay(self, capacity=4096, p=0.25, outcomes=("collision", "stuck"), seed=0):
        """Hard-case replay on a stream_reference_scenarios stream: a device buffer of `capacity` stream keys, filled from the
        attached episode log - one harvest launch behind every log update appends the key of each finished episode whose outcome is
        among `outcomes` ("collision", "goal", "stuck") - or by replay_push(); from now on the refill generates each slot from a key
        sampled from the buffer with probability p (with replacement; a key that fails again is appended again and so weighs more)
        and from its fresh key w + e * N otherwise.  The draw is a pure function of (seed, w + e * N, p, buffer):
        scenarios.replay_choice states it.  The log's key column and stream_keys() then name the scenario each episode really ran,
        and a logged failure stays reproducible from its key.  outcomes=None: push-only (no harvest launch).  The buffer holds for
        one parameter set: set_stream_params() empties it at the next harvest or push.  There is no detach - set_replay(p=0)
        pauses -; stop_streaming() and every pool setter end it, and a new stream starts un-armed.  Attaching again clears the
        buffer and may change the capacity.  Raises RuntimeError when not streaming, on an exploration stream, or with outcomes
        but no attached episode log."""
        mask = self._outcome_mask(outcomes)
        if mask and self._streaming and self._log is None:
            raise RuntimeError("attach_replay(outcomes=%r) without an episode log: the buffer is harvested from the log's rows; "
                               "attach_episode_log() first, or outcomes=None to push keys yourself" % (outcomes,))
        _lib.call(self.L, self.h, "cagym_stream_replay_init", int(capacity), int(seed) & 0xFFFFFFFFFFFFFFFF, self._stream())
        self._replay, self._replay_views = {"capacity": int(capacity), "p": 0.0, "mask": 0}, None
        _lib.call(self.L, self.h, "cagym_stream_replay_set", float(p), mask)
        self._replay.update(p=float(p), mask=mask)
        return self

    def _refuse_without_replay(self, what):
        if self._replay is None:
            raise RuntimeError("%s() without replay: attach_replay() first" % what)

    def set_replay(self, p=None, outcomes=None):
        """Change the replay probability and / or the harvested outcomes (None: as it is); takes effect at the next launch.
        p=0 is the pause: the per-slot key tables stay maintained and the harvest goes on."""
        self._refuse_without_replay("set_replay")
        mask = self._replay["mask"] if outcomes is None else self._outcome_mask(outcomes)
        if mask and self._log is None:
            raise RuntimeError("set_replay(outcomes=%r) without an episode log: attach_episode_log() first" % (outcomes,))
        p = self._replay["p"] if p is None else float(p)
        _lib.call(self.L, self.h, "cagym_stream_replay_set", p, mask)
        self._replay.update(p=p, mask=mask)

    def replay_push(self, keys):
        """Append stream keys (any integer sequence or tensor; taken mod 2^32) to the replay buffer, in order, on the current stream."""
        self._refuse_without_replay("replay_push")
        k = torch.as_tensor(keys, device=self.device).to(torch.int64).bitwise_and(0xFFFFFFFF).flatten()
        k = torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32).contiguous()  # the u32 bits
        _lib.call(self.L, self.h, "cagym_stream_replay_push", k.data_ptr(), int(k.numel()), self._stream())

    def replay_views(self):
        """Zero-copy device views of the replay state, no synchronisation: buf_key [capacity] (u32 bits as int32; entry i since the
        last clear lives at i % capacity), words [6] i64 (_lib.REPLAY_WORDS: count, harvested, pushed, replayed, n_missed,
        n_stale), slot_key [S] (u32 bits as int32) and slot_gen [S] i32."""
        if self._replay_views is None:
            a = [C.c_void_p() for _ in _lib.REPLAY_FIELDS]
            q = C.c_int(0)
            _lib.call(self.L, self.h, "cagym_stream_replay_get", *([C.byref(x) for x in a] + [C.byref(q)]))
            self._replay_views = _lib.views({f[0]: x.value for f, x in zip(_lib.REPLAY_FIELDS, a)}, _lib.REPLAY_FIELDS, self.device,
                                            S=self.S, Q=int(q.value))
        return dict(self._replay_views)

    def replay_stats(self):
        """Host integers of the replay buffer (this synchronises): count (keys appended since the last clear), harvested, pushed,
        replayed (slots generated from a buffered key), n_missed (log rows overwritten before the harvest saw them), n_stale
        (rows of slots generated under an earlier parameter set), live = min(count, capacity), capacity, p."""
        self._refuse_without_replay("replay_stats")
        st = dict(zip(_lib.REPLAY_WORDS, self.replay_views()["words"].tolist()))
        st.update(live=min(st["count"], self._replay["capacity"]), capacity=self._replay["capacity"], p=self._replay["p"])
        return st

    def stream_keys(self):
        """Zero-copy device view of slot_key [S] (u32 bits as int32): the stream key each pool slot was generated from."""
        self._refuse_without_replay("stream_keys")
        return self.replay_views()["slot_key"]

    def _harvest(self):
        rc = self._harvest_fn(self.h, self._stream())
        if rc:
            _lib.check(self.L, self.h, rc, "cagym_stream_replay_harvest")

    # ---- exploration worlds (include/cagym.h: cagym_generate_exploration_scenarios, cagym_stream_exploration_*) -----------------
    def _explore_params(self, kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries):
        _, mask, lo, hi = _kinds_obst(kinds, n_obst)
        return _lib.CagymExploreParams(int(seed), mask, int(n_robots), int(n_targets), lo, hi, int(max_tries),
                                       float(target_radius), float(robot_pref_speed))

    def generate_exploration_worlds(self, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0,
                                    max_tries=1000):
        """Fill the scenario pool ON DEVICE with exploration worlds (cagym_generate_exploration_scenarios): n_robots IG robots
        (slots 0..n_robots-1, FirstOrder) and n_targets static targets of radius target_radius among the rectangles of
        kinds = "train_stage_1" and / or "train_stage_2" (names or scenarios.GEN_* ids); starts, goals and rectangles are the
        stage samplers' own draws for number_of_agents = n_robots + n_targets.  n_obst and max_tries: as
        generate_reference_scenarios.  robot_pref_speed only sets the robots' time limit.  The team size is known afterwards:
        attach_ig_mcts() / attach_ig_greedy() work on the generated pool.  Returns n_failed."""
        P = self._explore_params(kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries)
        return self._generate("cagym_generate_exploration_scenarios", P, {sc.POLICY_IGMCTS, sc.POLICY_STATIC}, int(n_robots), False)

    def stream_exploration_worlds(self, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0,
                                  max_tries=1000):
        """generate_exploration_worlds (same arguments, same pool), and from now on the pool is stream_reference_scenarios' ring:
        world w's episode e runs on the world of key w + e * N, refilled behind every episode-advancing call.  With an IG team
        attached (before or after this call) the same refill rebuilds the distance field of every slot it regenerated, so
        attach_ig_mcts(episodic=True) / attach_ig_greedy(episodic=True) run under auto-reset, rollout() and CagymVecEnv on worlds
        that never repeat; the default attach keeps refusing auto-reset.  Needs n_scenarios % n_worlds == 0 and >= 2 * n_worlds;
        restore(), fork() and attach_episode_records() raise while it runs.  Returns n_failed."""
        P = self._explore_params(kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries)
        return self._generate("cagym_stream_exploration_scenarios", P, {sc.POLICY_IGMCTS, sc.POLICY_STATIC}, int(n_robots), True)

    def set_exploration_stream_params(self, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0,
                                      max_tries=1000):
        """The curriculum switch of an exploration stream (set_stream_params' counterpart): later refills generate from these
        arguments; worlds already in the ring stay.  n_robots must be the stream's."""
        P = self._explore_params(kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries)
        _lib.call(self.L, self.h, "cagym_stream_set_exploration_params", C.byref(P))

    def exploration_stream_stats(self):
        """Host integers of the exploration stream's field refresh (this synchronises): fields_built (distance fields rebuilt
        behind refills since the stream started), depth."""
        if self._explore_views is None:
            self._explore_views = self._address_views("cagym_explore_stream_get", _lib.EXPLORE_STREAM_FIELDS)
        return {"fields_built": int(self._explore_views["fields_built"].item()), "depth": self.S // self.N}

    def exploration_field_next(self):
        """Zero-copy device view of field_next [N] i32: the first episode of each world whose slot's field has not been rebuilt."""
        self.exploration_stream_stats()
        return self._explore_views["field_next"]

    def _refill(self):
        rc = self._refill_fn(self.h, self._stream())
        if rc:
            _lib.check(self.L, self.h, rc, "cagym_stream_refill")

    def obstacles(self):
        """Zero-copy device views of the pool's rectangles: obstacles [S, max_obstacles, 4] (xl, yl, xu, yu), n_obst [S]."""
        o, n = C.c_void_p(), C.c_void_p()
        _lib.call(self.L, self.h, "cagym_get_obstacles", C.byref(o), C.byref(n))
        if not self.Kobs:
            return {"obstacles": torch.zeros((self.S, 0, 4), dtype=torch.float64, device=self.device),
                    "n_obst": torch.zeros((self.S,), dtype=torch.int32, device=self.device)}
        return self._views({"obstacles": o.value, "n_obst": n.value}, _lib.OBSTACLE_FIELDS)

    def scenarios(self):
        """Zero-copy device views of the scenario pool: agents6 [S,M,6], policy / dynamics [S,M], n_agents [S], coop."""
        return self._get_views("cagym_get_scenarios", _lib.CagymScenarioPtrs(), _lib.SCENARIO_FIELDS)
