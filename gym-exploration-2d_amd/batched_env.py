"""BatchedCollisionAvoidanceEnv: N worlds x M agents of the reference's CollisionAvoidanceEnv
(gym_collision_avoidance/envs/collision_avoidance_env.py) stepped by hand-written HIP kernels.

Vectorised convention of the reference's DummyVecEnv use (experiments/src/env_utils.py:29-31,
envs/wrappers.py:101-106): step(actions[N, M, 2]) -> (obs, rewards[N, M], game_over[N], info);
observations and outputs are PyTorch-ROCm tensors that the kernels write in place (zero-copy).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import scenarios as sc
from .dmcts import DeviceDecMCTSPlanner
from .ga3c import GA3CCADRLPolicy
from .ig import EPISODE_FOLD, GreedyPlanner, InfoGain

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (device index) -> hipStream_t as an int

_TORCH_DT = {"f8": torch.float64, "f4": torch.float32, "u4": torch.int32, "i4": torch.int32}


class _DevArray(object):
    """Minimal __cuda_array_interface__ holder: zero-copy torch view of a raw device pointer."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<" + typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class _IgState(object):
    """What step() needs of an attached IG policy, whichever it is: the primitives, the planner and the robots' input buffers."""
    __slots__ = ("kind", "ig", "R", "range", "episodic", "poses", "det", "n_det", "world", "planner")


_OUT_KEYS = ("other_agents_states", "ego", "laserscan", "reward", "flags", "game_over")  # a rollout's buffers in CagymOutputs order
GAME_OVER_MODES = {"agent0": _lib.GO_AGENT0, "all": _lib.GO_ALL, "learning": _lib.GO_LEARNING}


_SNAP_OUT = ("obs_oas", "obs_ego", "obs_laser", "reward", "flags", "game_over")  # the env-owned output tensors a snapshot carries rows of


class EnvSnapshot(object):
    """What BatchedCollisionAvoidanceEnv.snapshot() returns and restore() takes: `layout` (cagym_snapshot_layout), `blob`
    [n, row_bytes] u8 on the device (cagym_snapshot's rows), `worlds` [n] i32 device tensor of the origin world ids, and
    `outputs`: clones of the same worlds' rows of the env's output tensors - nothing in the C ABI recomputes an observation
    without stepping, and a policy needs the restored state's observation.  The scenario pool is not part of it."""

    def __init__(self, layout, blob, worlds, outputs, all_worlds=False, trusted=True):
        self.layout, self.blob, self.worlds, self.outputs = layout, blob, worlds, outputs
        self.all_worlds = bool(all_worlds)  # rows 0..N-1 are worlds 0..N-1 (snapshot() without a list)
        self.trusted = bool(trusted)        # the world ids were validated on the host
        self.n = int(blob.shape[0])

    def state_dict(self):
        """A plain dict of CPU tensors and ints: torch.save / torch.load of it give checkpoint and resume."""
        return {"layout": {k: int(getattr(self.layout, k)) for k, _ in _lib.CagymSnapshotLayout._fields_},
                "blob": self.blob.cpu(), "worlds": self.worlds.cpu(), "all_worlds": self.all_worlds,
                "outputs": {k: v.cpu() for k, v in self.outputs.items()}}

    @classmethod
    def from_state_dict(cls, d, device):
        layout = _lib.CagymSnapshotLayout(**{k: int(v) for k, v in d["layout"].items()})
        worlds = torch.as_tensor(d["worlds"]).to(torch.int32).reshape(-1)
        ids = worlds.numpy()
        if ids.size != int(d["blob"].shape[0]) or (ids.size and (ids.min() < 0 or ids.max() >= layout.n_worlds)) or np.unique(ids).size != ids.size:
            raise ValueError("EnvSnapshot.from_state_dict: `worlds` must name one distinct world of [0, %d) per blob row" % layout.n_worlds)
        dev = torch.device(device)
        return cls(layout, torch.as_tensor(d["blob"]).to(torch.uint8).to(dev).contiguous(), worlds.to(dev),
                   {k: torch.as_tensor(v).to(dev).contiguous() for k, v in d["outputs"].items()}, d.get("all_worlds", False), True)


class BatchedCollisionAvoidanceEnv(object):
    def __init__(self, n_worlds, max_agents=10, n_scenarios=None, max_obstacles=0, game_over_mode="agent0",
                 collide_with_static=False, laserscan=False, device="cuda:0", dt=0.1, rvo_max_neighbors=0):
        self.L = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BatchedCollisionAvoidanceEnv runs on a ROCm device only (got %s)" % device)
        self.N, self.M, self.K = int(n_worlds), int(max_agents), int(max_agents) - 1
        self.S = int(n_scenarios) if n_scenarios else self.N
        self.Kobs = int(max_obstacles)
        self.laserscan = bool(laserscan)
        if isinstance(game_over_mode, str):
            game_over_mode = GAME_OVER_MODES[game_over_mode]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._dev_index = int(idx)
        self.cfg = _lib.CagymConfig(self.N, self.M, self.S, self.Kobs, int(game_over_mode),
                                    int(bool(collide_with_static)), int(self.laserscan), int(idx), float(dt),
                                    int(rvo_max_neighbors), 0)  # rvo_max_neighbors 0 = max_agents (RVOPolicy.py:15)
        self.h = C.c_void_p()
        _lib.check(self.L, None, self.L.cagym_create(C.byref(self.cfg), C.byref(self.h)), "cagym_create")
        # the calls inside per-step loops, resolved once
        self._step_fn = (self.L.cagym_step, self.L.cagym_step_autoreset)
        self._rollout_fn, self._records_fn = self.L.cagym_rollout, self.L.cagym_episode_records_update
        self._refill_fn, self._log_fn = self.L.cagym_stream_refill, self.L.cagym_episode_log_update
        self._keep_fn = self.L.cagym_step_autoreset_keep
        N, M, K = self.N, self.M, self.K
        dev = self.device
        self.obs_oas = torch.zeros((N, M, K, 10), dtype=torch.float32, device=dev)
        self.obs_ego = torch.zeros((N, M, _lib.EGO_WIDTH), dtype=torch.float32, device=dev)
        self.obs_laser = torch.zeros((N, M, 16), dtype=torch.float32, device=dev) if self.laserscan else None
        self.reward = torch.zeros((N, M), dtype=torch.float32, device=dev)
        self.flags = torch.zeros((N, M), dtype=torch.uint8, device=dev)
        self.game_over = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self._out = self._outputs(self.obs_oas, self.obs_ego, self.obs_laser, self.reward, self.flags, self.game_over)
        self._state = None
        self._side = None  # side stream of step_overlapped (created on first use)
        # policies the env drives itself inside step() (attach_ga3c / attach_ig_mcts) and what the pool holds
        self._ga3c = None
        self._igm = None
        self._act = None          # [N, M, 2] f32 action table of an internal step (the caller's buffer is only read)
        self._pool_policies = set()
        self._n_ig = None         # IG robots per scenario (-1: the scenarios differ; None: a generated pool)
        self.team_reward = None   # [N] f64: the team's MI reward of the last step with ig_mcts attached (policy.team_reward)
        self._rec = None          # keep mode of attach_episode_records, None while detached
        self._rec_views = None
        self._rec_priv = {}       # rollout buffers of a caller whose `out` lacks reward / flags / game_over
        self._log = None          # capacity of attach_episode_log, None while detached
        self._log_views = None
        self._streaming = False   # stream_reference_scenarios: one cagym_stream_refill behind every episode-advancing call
        self._stream_views = None
        self._explore_views = None
        self._term = None         # keep_terminal_observations: {"other_agents_states", "ego", "laserscan"} env-owned tensors
        self._term_c = None       # ... as the cagym_terminal_outputs step() passes
        self._traj = None         # n_slices of attach_trajectory_ring, None while detached
        self._traj_views = None

    # ---- plumbing ------------------------------------------------------------------------------
    @staticmethod
    def _outputs(oas, ego, laser, reward, flags, go):
        p = _lib.ptr
        return _lib.CagymOutputs(p(oas), p(ego), p(laser), p(reward), p(flags), p(go))

    def _actions(self, actions):
        """The caller's actions as a contiguous f32 [N, M, 2] device tensor, or None."""
        if actions is None:
            return None
        return torch.as_tensor(actions, device=self.device).to(torch.float32).reshape(self.N, self.M, 2).contiguous()

    def _mask(self, world_mask):
        """A world mask as a contiguous u8 device tensor, or None (= every world)."""
        if world_mask is None:
            return None
        return torch.as_tensor(world_mask, device=self.device).to(torch.uint8).contiguous()

    def _stream(self):
        # torch's current stream of the handle's device (the raw-handle accessor costs 0.3 us, the Stream object 2 us per launch)
        if _raw_stream is not None:
            return C.c_void_p(_raw_stream(self._dev_index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            torch.cuda.synchronize(self.device)
            self.L.cagym_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        self._streaming = False  # as the library: a new pool ends the stream
        live = np.arange(M)[None, :] < (na if na is not None else np.full(S, M))[:, None]
        self._pool_policies = set(np.unique(pol[live]).tolist())
        counts = ((pol == sc.POLICY_IGMCTS) & live).sum(axis=1)
        self._n_ig = int(counts[0]) if (counts == counts[0]).all() else -1
        if self._igm is not None and self._n_ig != self._igm.R:  # the attached planner was sized for another team
            self.detach_ig_mcts()
        if self._igm is not None:  # new rasters: their distance fields and fresh beliefs (cagym_ig_init)
            _lib.call(self.L, self.h, "cagym_ig_init", self._stream())

    def sense_occupancy_grid(self, out=None):
        """'local_grid' observation of every agent (OccupancyGridSensor.sense): uint8 [N, M, 60, 60], 1 = occupied.
        Parity unpinned (cv2.warpAffine is restated, OpenCV is not installed): see include/cagym.h."""
        if out is None:
            out = torch.empty((self.N, self.M, 60, 60), dtype=torch.uint8, device=self.device)
        _lib.call(self.L, self.h, "cagym_occupancy_grid", out.data_ptr(), self._stream())
        return out

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
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, "cagym_generate_scenarios", C.byref(P), C.byref(nf) if check else None, self._stream())
        self._streaming = False
        self._pool_policies = {int(ego_policy), int(other_policies[0]), int(other_policies[1])}
        self._n_ig = None
        self.detach_ig_mcts()  # the generated pool's robot count is not known on the host
        return int(nf.value) if check else None

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
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, "cagym_generate_reference_scenarios", C.byref(P), C.byref(nf) if check else None, self._stream())
        self._streaming = False
        self._pool_policies = pols
        self._n_ig = None
        self.detach_ig_mcts()  # the generated pool's robot count is not known on the host
        return int(nf.value) if check else None

    def _gen2_params(self, kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                     other_dynamics, n_obst, max_tries):
        """generate_reference_scenarios' arguments as (cagym_gen2_params, the policies the scenarios may hold)."""
        ks = [kinds] if isinstance(kinds, (str, int, np.integer)) else list(kinds)
        mask = 0
        for k in ks:
            mask |= 1 << sc.sampler_kind(k)
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
        lo, hi = (-1, -1) if n_obst is None else (n_obst, n_obst) if np.isscalar(n_obst) else n_obst
        P = _lib.CagymGen2Params(int(seed), mask, int(number_of_agents), int(bool(fixed_count)), int(ego_policy),
                                 int(ego_dynamics), int(own), pa, pb, int(other_dynamics), int(lo), int(hi), int(max_tries), pp)
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
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, "cagym_stream_scenarios", C.byref(P), C.byref(nf) if check else None, self._stream())
        self._streaming = True
        self._pool_policies = pols
        self._n_ig = None
        self.detach_ig_mcts()
        return int(nf.value) if check else None

    def set_stream_params(self, kinds, seed, number_of_agents=None, fixed_count=False, ego_policy=5, ego_dynamics=4,
                          other_policies=None, p_b=None, other_dynamics=0, n_obst=None, max_tries=1000):
        """The reference's curriculum switch (collision_avoidance_env.py:419-438) on a streaming env: the slots that later refills
        generate come from this sampler set (scenarios.reference_curriculum gives the set of a training step); the seed may change
        too.  Scenarios already in the ring stay, so a world meets the new set n_scenarios / n_worlds - 1 episodes later."""
        P, pols = self._gen2_params(kinds, seed, number_of_agents, fixed_count, ego_policy, ego_dynamics, other_policies, p_b,
                                    other_dynamics, n_obst, max_tries)
        _lib.call(self.L, self.h, "cagym_stream_set_params", C.byref(P))
        self._pool_policies = self._pool_policies | pols

    def stop_streaming(self):
        """End the stream: the pool stays as it is and is replayed from here on, as a fixed pool is."""
        _lib.call(self.L, self.h, "cagym_stream_stop")
        self._streaming = False

    def stream_stats(self):
        """Host integers of the stream (this synchronises): generated (slots generated since stream_reference_scenarios, its first
        fill included), n_failed (rejection loops that hit max_tries), n_lapped (times a world started an episode on a slot that
        had not been refilled: only a rollout in which a world finishes more than depth - 1 episodes does that), depth."""
        if self._stream_views is None:
            sp = _lib.CagymStreamPtrs()
            _lib.call(self.L, self.h, "cagym_stream_get", C.byref(sp))
            spec = {"next_episode": ((self.N,), "i4"), "generated": ((1,), "i8"), "n_failed": ((1,), "i4"), "n_lapped": ((1,), "i4")}
            self._stream_views = {k: torch.as_tensor(_DevArray(getattr(sp, k), shp, ts), device=self.device) for k, (shp, ts) in spec.items()}
        v = self._stream_views
        return {"generated": int(v["generated"].item()), "n_failed": int(v["n_failed"].item()), "n_lapped": int(v["n_lapped"].item()),
                "depth": self.S // self.N}

    def stream_next_episode(self):
        """Zero-copy device view of next_episode [N] i32: the first episode of each world whose slot has not been generated."""
        self.stream_stats()
        return self._stream_views["next_episode"]

    # ---- exploration worlds (include/cagym.h: cagym_generate_exploration_scenarios, cagym_stream_exploration_*) -----------------
    def _explore_params(self, kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries):
        ks = [kinds] if isinstance(kinds, (str, int, np.integer)) else list(kinds)
        mask = 0
        for k in ks:
            mask |= 1 << sc.sampler_kind(k)
        lo, hi = (-1, -1) if n_obst is None else (n_obst, n_obst) if np.isscalar(n_obst) else n_obst
        return _lib.CagymExploreParams(int(seed), mask, int(n_robots), int(n_targets), int(lo), int(hi), int(max_tries),
                                       float(target_radius), float(robot_pref_speed))

    def _explore_pool(self, n_robots, streaming):
        """Host state after an exploration pool was committed: the team size is known, and an attached team of that size stays."""
        self._streaming = streaming
        self._pool_policies = {sc.POLICY_IGMCTS, sc.POLICY_STATIC}
        self._n_ig = int(n_robots)
        if self._igm is not None and self._n_ig != self._igm.R:  # the attached planner was sized for another team
            self.detach_ig_mcts()
        if self._igm is not None:  # as set_scenarios: fresh beliefs on the new rasters' fields (on a stream it arms the refresh)
            _lib.call(self.L, self.h, "cagym_ig_init", self._stream())

    def generate_exploration_worlds(self, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0,
                                    max_tries=1000):
        """Fill the scenario pool ON DEVICE with exploration worlds (cagym_generate_exploration_scenarios): n_robots IG robots
        (slots 0..n_robots-1, FirstOrder) and n_targets static targets of radius target_radius among the rectangles of
        kinds = "train_stage_1" and / or "train_stage_2" (names or scenarios.GEN_* ids); starts, goals and rectangles are the
        stage samplers' own draws for number_of_agents = n_robots + n_targets.  n_obst and max_tries: as
        generate_reference_scenarios.  robot_pref_speed only sets the robots' time limit.  The team size is known afterwards:
        attach_ig_mcts() / attach_ig_greedy() work on the generated pool.  Returns n_failed."""
        P = self._explore_params(kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries)
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, "cagym_generate_exploration_scenarios", C.byref(P), C.byref(nf), self._stream())
        self._explore_pool(n_robots, False)
        return int(nf.value)

    def stream_exploration_worlds(self, kinds, seed, n_robots, n_targets, n_obst=None, target_radius=0.2, robot_pref_speed=1.0,
                                  max_tries=1000):
        """generate_exploration_worlds (same arguments, same pool), and from now on the pool is stream_reference_scenarios' ring:
        world w's episode e runs on the world of key w + e * N, refilled behind every episode-advancing call.  With an IG team
        attached (before or after this call) the same refill rebuilds the distance field of every slot it regenerated, so
        attach_ig_mcts(episodic=True) / attach_ig_greedy(episodic=True) run under auto-reset, rollout() and CagymVecEnv on worlds
        that never repeat; the default attach keeps refusing auto-reset.  Needs n_scenarios % n_worlds == 0 and >= 2 * n_worlds;
        restore(), fork() and attach_episode_records() raise while it runs.  Returns n_failed."""
        P = self._explore_params(kinds, seed, n_robots, n_targets, n_obst, target_radius, robot_pref_speed, max_tries)
        nf = C.c_int32(0)
        _lib.call(self.L, self.h, "cagym_stream_exploration_scenarios", C.byref(P), C.byref(nf), self._stream())
        self._explore_pool(n_robots, True)
        return int(nf.value)

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
            fn, fb = C.c_void_p(), C.c_void_p()
            _lib.call(self.L, self.h, "cagym_explore_stream_get", C.byref(fn), C.byref(fb))
            self._explore_views = {"field_next": torch.as_tensor(_DevArray(fn.value, (self.N,), "i4"), device=self.device),
                                   "fields_built": torch.as_tensor(_DevArray(fb.value, (1,), "i8"), device=self.device)}
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
        return {"obstacles": torch.as_tensor(_DevArray(o.value, (self.S, self.Kobs, 4), "f8"), device=self.device),
                "n_obst": torch.as_tensor(_DevArray(n.value, (self.S,), "i4"), device=self.device)}

    def scenarios(self):
        """Zero-copy device views of the scenario pool: agents6 [S,M,6], policy / dynamics [S,M], n_agents [S], coop."""
        sp = _lib.CagymScenarioPtrs()
        _lib.call(self.L, self.h, "cagym_get_scenarios", C.byref(sp))
        S, M = self.S, self.M
        spec = {"agents6": ((S, M, 6), "f8"), "policy": ((S, M), "i4"), "dynamics": ((S, M), "i4"),
                "n_agents": ((S,), "i4"), "coop": ((S, M), "f8")}
        return {k: torch.as_tensor(_DevArray(getattr(sp, k), shp, ts), device=self.device) for k, (shp, ts) in spec.items()}

    # ---- gym surface ----------------------------------------------------------------------------
    def _obs(self):
        obs = {"other_agents_states": self.obs_oas, "ego": self.obs_ego}
        if self.laserscan:
            obs["laserscan"] = self.obs_laser
        return obs

    def reset(self, world_mask=None, advance_episode=False):
        m = self._mask(world_mask)
        _lib.call(self.L, self.h, "cagym_reset", _lib.ptr(m), int(bool(advance_episode)), C.byref(self._out), self._stream())
        if self._streaming and advance_episode:
            self._refill()
        g = self._igm
        if g is not None and g.episodic and m is not None:
            # a manual restart of the masked worlds only: prior belief, no communicated plans, running team return zeroed; it is
            # not a finished episode, so nothing is folded into the episode statistics (cagym_ig_episode_boundary without FOLD)
            g.ig.episode_boundary(g.planner.P, g.planner.workspace, None, m, 0)
        elif g is not None:  # a new episode: prior beliefs (of the masked worlds) and no communicated plans (of any world)
            g.ig.reset_belief(m)
            g.planner.reset()
            if g.episodic:
                g.ig.episode_stats["running"].zero_()
        return self._obs()

    # ---- policies driven inside step(): GA3C-CADRL (collision_avoidance_env.py:287-340) and ig_mcts (:342-379) ------------------
    def attach_ga3c(self, checkpoint="iros18", max_observed=None):
        """From now on step() and rollout() compute the action of every active GA3C agent themselves
        (GA3CCADRLPolicy.find_next_action): one cagym_ga3c_act_merge launch writes the whole action table - the network's action
        for the GA3C agents, the caller's rows for every other slot - into a buffer of the env, and the step reads that.  The env
        keeps the policy (and its weight blob, which the handle caches by address) for as long as it is attached."""
        self._ga3c = GA3CCADRLPolicy(self, checkpoint=checkpoint, max_observed=max_observed)
        self._alloc_act()
        return self._ga3c

    def attach_ig_mcts(self, detect_fov=60.0, detect_range=5.0, xdt=5, Ntree=30, Nsims=10, mcts_cp=1.0, mcts_horizon=4,
                       mcts_gamma=0.95, Ncycles=5, parallelize_agents=False, radius=0.5, seed=0, episodic=False):
        """From now on step() plans the (v, omega) of every IG robot itself (ig_mcts.set_param + find_next_action, the Dec-MCTS
        cycles of collision_avoidance_env.py:342-379): robot poses and detections (cagym_ig_robot_inputs), belief update, the
        team's MI reward into self.team_reward, Dec-MCTS plan (seeded counter-based streams), the robots' rows of the action
        table (cagym_ig_robot_actions), then the step.  One belief per world, shared by its robots.  Every scenario of the pool
        must hold the same number of IG robots.
        episodic=False (default): one team episode per handle, as the reference's experiment loop runs it; step(auto_reset=True)
        and rollout() are refused, and reset(world_mask=...) forgets the plans of every world.
        episodic=True: every step ends with one cagym_ig_episode_boundary launch.  It adds the step's team reward to the
        world's running return (ig_episode_stats()) and, under auto_reset, restarts the planner and the belief of exactly the
        worlds whose game_over the step just set: the terminal step's reward belongs to the episode that ends, the next step's
        belief update is the first observation of the new episode on the new scenario's distance field, and its first planning
        cycle hears nothing (DummyVecEnv's reset() builds new ig_mcts objects).  rollout() chains such steps; CagymVecEnv works.
        reset(world_mask=m) restarts the masked worlds alone and zeroes their running return without counting an episode;
        reset() restarts everything and zeroes every running return."""
        return self._attach_ig("ig_mcts", detect_fov, detect_range, xdt, episodic, lambda g: DeviceDecMCTSPlanner(
            g.ig, g.R, radius=radius, Ntree=Ntree, Nsims=Nsims, horizon=mcts_horizon, c_p=mcts_cp, gamma=mcts_gamma, Ncycles=Ncycles,
            seed=seed, parallelize_agents=parallelize_agents))

    def _attach_ig(self, kind, detect_fov, detect_range, xdt, episodic, make_planner):
        """Attach an IG policy, whichever it is: the primitives, the robots' input buffers, then its planner."""
        self._refuse_keep("attach_%s" % kind, "an attached IG planner's per-world restart reads the game_over of the auto-resetting launch; "
                          "the three-launch step has not been taken through it")
        R = self._n_ig if self._n_ig is not None else 0
        self._igm = None
        ig = InfoGain(self, fov_rad=detect_fov * np.pi / 180, sens_range=detect_range, xdt=xdt, dt=self.cfg.dt)
        N, K, dev = self.N, self.K, self.device
        g = _IgState()
        g.kind, g.ig, g.R, g.range, g.episodic = kind, ig, R, float(detect_range), bool(episodic)
        g.poses = torch.zeros((N, max(R, 1), 3), dtype=torch.float64, device=dev)
        g.det = torch.zeros((N, max(R, 1), K, 2), dtype=torch.float64, device=dev)
        g.n_det = torch.zeros((N, max(R, 1)), dtype=torch.int32, device=dev)
        g.world = torch.arange(N, dtype=torch.int32, device=dev)
        ig.robot_inputs(R, g.range, self.obs_oas, g.poses, g.det, g.n_det)  # refuses a pool without R robots in every scenario
        g.planner = make_planner(g)
        self._igm = g
        self._alloc_act()
        return g.planner

    def attach_ig_greedy(self, detect_fov=60.0, detect_range=5.0, radius=0.5, coordinate=False, episodic=False):
        """From now on step() chooses the (v, omega) of every IG robot by the one-step greedy rule of policies/ig_greedy.py
        (find_next_action with the intended update([pose], [targets])): robot poses and detections
        (cagym_ig_robot_inputs), belief update, the team's MI reward into self.team_reward, ONE cagym_ig_greedy_plan launch, the
        robots' rows of the action table (cagym_ig_robot_actions), then the step - attach_ig_mcts's sequence with the greedy
        plan in place of the Dec-MCTS one, and it replaces an attached ig_mcts (attach_ig_mcts replaces this; detach_ig_mcts
        clears either).  One belief per world, shared by its robots; coordinate=True lets a world's robots choose in slot order,
        each without the cells the earlier ones chose (the reference's robots each own a map and cannot collide on cells).
        episodic: as attach_ig_mcts (the policy keeps nothing across steps, so a restart is the belief and the running return).
        Returns the ig.GreedyPlanner, which holds the last plan's choice / mi / claimed."""
        if self._n_ig is not None and self._n_ig > 8:
            raise ValueError("attach_ig_greedy: at most 8 IG robots per world (cagym_ig_greedy_plan), the pool has %d" % self._n_ig)
        return self._attach_ig("ig_greedy", detect_fov, detect_range, 1, episodic,
                               lambda g: GreedyPlanner(g.ig, g.R, radius=radius, coordinate=coordinate))

    def detach_ig_mcts(self):
        self._igm = None
        self.team_reward = None

    def _alloc_act(self):
        if self._act is None:
            self._act = torch.zeros((self.N, self.M, 2), dtype=torch.float32, device=self.device)

    def _drives_ga3c(self):
        return self._ga3c is not None and sc.POLICY_GA3C in self._pool_policies

    def ig_episode_stats(self):
        """Zero-copy device views of the IG team's per-world episode accumulators (an episodic attach_ig_mcts keeps them):
        running [N] f64 team return of the episode in progress, sum [N] f64 over the finished episodes, last [N] f64 return of
        the last finished one, episodes [N] i32 finished episodes."""
        if self._igm is None:
            raise RuntimeError("ig_episode_stats() needs attach_ig_mcts or attach_ig_greedy")
        return dict(self._igm.ig.episode_stats)

    def _internal_actions(self, a, team_reward_out=None, oas=None):
        """The action table the step reads: the caller's `a` (or None) when nothing is attached, else the env's own buffer.
        team_reward_out: where the team reward of this step goes (rollout: slice t of its buffer); oas: the OtherAgentsStates
        table the last step wrote, when that is not self.obs_oas (rollout: slice t - 1)."""
        ga3c = self._drives_ga3c()
        if not ga3c and self._igm is None:
            return a
        table = self._act
        if ga3c:
            self._ga3c.act_merge(a, table)
        elif a is None:
            table.zero_()
        else:
            table.copy_(a)
        if self._igm is not None:
            g = self._igm
            g.ig.robot_inputs(g.R, g.range, self.obs_oas if oas is None else oas, g.poses, g.det, g.n_det)
            observed = g.ig.update_belief(g.poses, g.det, g.n_det)
            self.team_reward = g.ig.mi_reward(observed, g.world, out=team_reward_out)  # before the move, as the reference computes it
            planned, _ = g.planner.plan(g.poses)
            g.ig.robot_actions(g.R, planned, table)
        return table

    def _chained_step(self, a, o, auto_reset, restart, team_reward_out=None, oas=None, term=False):
        """One step with whatever is attached, three parts in stream order: the internal actions (_internal_actions), the step
        launch into the CagymOutputs `o`, and the episodic IG team's end of the step - its running return and the restart of the
        worlds of `restart` (under auto_reset the game_over tensor `o` points at, else None).  term: hand the env's terminal buffers
        to the step (step() does, rollout() does not).  (No torch.cuda.device context
        here or anywhere else around the C ABI: every launching entry makes the handle's device current itself.)"""
        a = self._internal_actions(a, team_reward_out, oas)
        if auto_reset and (self._traj is not None or (term and self._term is not None)):  # same results, three launches (cagym_step_autoreset_keep)
            rc = self._keep_fn(self.h, _lib.ptr(a), C.byref(o), self._term_c if term else None, self._stream())
        else:
            rc = self._step_fn[bool(auto_reset)](self.h, _lib.ptr(a), C.byref(o), self._stream())
        if rc:
            _lib.check(self.L, self.h, rc, "cagym_step")
        g = self._igm
        if g is not None and g.episodic:
            g.ig.episode_boundary(g.planner.P, g.planner.workspace, self.team_reward, restart, EPISODE_FOLD)

    def step(self, actions=None, auto_reset=False):
        """One env.step() of every world.  auto_reset=True: finished worlds restart inside the same launch
        (VecEnv semantics: the returned observation is the first one of the new episode).  With a policy attached
        (attach_ga3c / attach_ig_mcts) its agents' rows of `actions` are ignored and the env computes them; `actions`
        itself is only read."""
        if auto_reset and self._igm is not None and not self._igm.episodic:
            k = self._igm.kind
            raise RuntimeError("step(auto_reset=True) with %s attached: the planner's per-world restart (beliefs, "
                               "communicated plans) is not implemented for this attach; attach_%s(episodic=True), or step "
                               "without auto-reset and reset() yourself" % (k, k))
        self._records_contract(auto_reset, "step")
        self._chained_step(self._actions(actions), self._out, auto_reset, self.game_over if auto_reset else None, term=True)
        self._after_steps(auto_reset, self.flags, self.reward, self.game_over, 1)
        info = {"flags": self.flags}
        if auto_reset and self._term is not None:
            info["terminal"] = dict(self._term, valid=self.game_over)
        return self._obs(), self.reward, self.game_over, info

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

    def _after_steps(self, auto_reset, flags, reward, game_over, T):
        """What follows the step launch(es) of one call on the stream, in this order: the episode log's update (it reads the pool
        slot of the episode that ended, which the refill regenerates next), the stream's refill, the records' update."""
        if self._log is not None:
            rc = self._log_fn(self.h, flags.data_ptr(), reward.data_ptr(), game_over.data_ptr(), int(T), self._stream())
            if rc:
                _lib.check(self.L, self.h, rc, "cagym_episode_log_update")
        if self._streaming and auto_reset:
            self._refill()
        if self._rec is not None:
            self._records_update(flags, reward, game_over, T)

    def _records_contract(self, auto_reset, what):
        if self._traj is not None and not auto_reset:
            raise RuntimeError("%s(auto_reset=False) with a trajectory ring attached: the ring is fed by cagym_step_autoreset_keep "
                               "only, every step exactly once and in order (include/cagym.h); detach_trajectory_ring() first" % what)
        if self._log is not None and not auto_reset:
            raise RuntimeError("%s(auto_reset=False) with an episode log attached: cagym_episode_log_update takes the outputs "
                               "of auto-reset stepping only, every step exactly once and in order (include/cagym.h); "
                               "detach_episode_log() first" % what)
        if self._rec is not None and not auto_reset:
            raise RuntimeError("%s(auto_reset=False) with episode records attached: cagym_episode_records_update takes the outputs "
                               "of auto-reset stepping only, every step exactly once and in order (include/cagym.h); "
                               "detach_episode_records() first" % what)

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
            rp = _lib.CagymEpisodeRecordPtrs()
            _lib.call(self.L, self.h, "cagym_episode_records_get", C.byref(rp))
            dims = {"S": (self.S,), "SM": (self.S, self.M), "N": (self.N,), "NM": (self.N, self.M), "1": (1,)}
            v = {}
            for name, ts, shape in _lib.EPREC_FIELDS:
                t = torch.as_tensor(_DevArray(getattr(rp, name), dims[shape], ts), device=self.device)
                v[name] = t.view(torch.int32) if ts == "u4" else t
            v["n_agents"] = self.scenarios()["n_agents"]
            self._rec_views = v
        if check:
            d = int(self._rec_views["desync"].item())
            if d:
                raise RuntimeError("episode records are out of step with the env in %d world-launches (desync): the recorder was "
                                   "fed a step twice, skipped one, or saw a step without auto-reset; attach_episode_records() "
                                   "again to clear" % d)
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
        self._refuse_without_log("clear_episode_log")
        _lib.call(self.L, self.h, "cagym_episode_log_restart", None, 1, self._stream())

    def _refuse_without_log(self, what):
        if self._log is None:
            raise RuntimeError("%s() without an episode log: attach_episode_log() first" % what)

    def episode_log_views(self):
        """Zero-copy device views of the ring and its words, no synchronisation: key (u32 bits as int32), world, episode, steps,
        outcome, n_agents, n_obst [L] i32, slice [L] i64, ret [L] f64, t / extra_t [L, M] f64, flags [L, M] u8, the running t_run
        [N, M], ret_run, steps_run, atgoal_run, cursor [N], head [1] i64 (rows ever appended; row i lives at index i % L) and
        desync [1]."""
        self._refuse_without_log("episode_log_views")
        if self._log_views is None:
            lp = _lib.CagymEpisodeLogPtrs()
            _lib.call(self.L, self.h, "cagym_episode_log_get", C.byref(lp))
            L = int(lp.capacity)
            dims = {"L": (L,), "LM": (L, self.M), "N": (self.N,), "NM": (self.N, self.M), "1": (1,)}
            v = {}
            for name, ts, shape in _lib.EPLOG_FIELDS:
                ts = {"u4": "i4", "u8": "i8"}.get(ts, ts)  # the bits, in the signed types torch computes with
                v[name] = torch.as_tensor(_DevArray(getattr(lp, name), dims[shape], ts), device=self.device)
            self._log_views = v
        return dict(self._log_views)

    def episode_log(self, last=None, sort=False, check=True):
        """The valid rows in append order, oldest first, as device tensors (copies): the columns of episode_log_views() with key
        as int64 in [0, 2^32), plus count (int32 ones) so that stats.suite_statistics(env.episode_log(last=K)) works on a window.
        One synchronisation, to read head.  last=K: the newest K rows only; sort=True: ordered by (slice, world) instead;
        check: raise RuntimeError when the log saw a skipped, doubled or non-auto-reset step (desync != 0)."""
        v = self.episode_log_views()
        L = self._log
        head, d = torch.cat([v["head"], v["desync"].to(torch.int64)]).tolist()
        if check and d:
            raise RuntimeError("the episode log is out of step with the env in %d world-launches (desync): the recorder was "
                               "fed a step twice, skipped one, or saw a step without auto-reset; attach_episode_log() "
                               "again to clear" % d)
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

    def _refuse_with_ring(self, what):
        if self._traj is not None:
            raise RuntimeError("%s() with a trajectory ring attached: its running values would describe another timeline (the library "
                               "refuses as long as the ring is initialised)" % what)

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

    def _refuse_without_ring(self, what):
        if self._traj is None:
            raise RuntimeError("%s() without a trajectory ring: attach_trajectory_ring() first" % what)

    def trajectory_views(self):
        """Zero-copy device views of the ring, no synchronisation: rows [L, 13, N, M] f64 (column planes, _lib.TRAJ_COLUMNS),
        moved [L, N, M] u8, episode [L, N] i32, last [L, N] u8, head [1] i64 (slices ever written; slice i lives at index i % L),
        desync [1] i32, and the ring's running t_prev [N, M] f64, seen [N, M] i32."""
        self._refuse_without_ring("trajectory_views")
        if self._traj_views is None:
            tp = _lib.CagymTrajectoryPtrs()
            _lib.call(self.L, self.h, "cagym_trajectory_get", C.byref(tp))
            L, N, M = int(tp.n_slices), self.N, self.M
            dims = {"LCNM": (L, len(_lib.TRAJ_COLUMNS), N, M), "LNM": (L, N, M), "LN": (L, N), "NM": (N, M), "1": (1,)}
            v = {}
            for name, ts, shape in _lib.TRAJ_FIELDS:
                ts = {"u8": "i8"}.get(ts, ts)  # the bits, in the signed type torch computes with
                v[name] = torch.as_tensor(_DevArray(getattr(tp, name), dims[shape], ts), device=self.device)
            self._traj_views = v
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
        if check and d:
            raise RuntimeError("the trajectory ring is out of step with the env (desync: %d agent-steps went past it): the env was "
                               "stepped through another entry than step(auto_reset=True) / rollout(auto_reset=True); "
                               "attach_trajectory_ring() again to clear" % d)
        planes = {"rows": v["rows"][:, :, w:w + 1].cpu().numpy(), "moved": v["moved"][:, w:w + 1].cpu().numpy(),
                  "episode": v["episode"][:, w:w + 1].cpu().numpy(), "last": v["last"][:, w:w + 1].cpu().numpy(), "head": head}
        H, mv, complete = dataset.ring_slices(planes, 0, int(episode))
        return {"history": H, "moved": mv, "complete": complete}

    # ---- the split step: env.step() in two launches (include/cagym.h: cagym_step_begin / cagym_step_finish) ------------------
    def step_begin(self, stream=None):
        """First half of step(): the internal RVO policies' half-planes and linear programs on the current state (they do not
        depend on the external actions: env.py:287-340 gathers every agent's action before any agent moves).  `stream`: a
        torch.cuda.Stream to run it on BESIDE the producer of the external actions (default: the current stream); the caller
        orders step_finish behind it (step_overlapped does).  Refused while a policy is attached (see step_finish)."""
        self._refuse_split()
        raw = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.call(self.L, self.h, "cagym_step_begin", raw)

    def _refuse_split(self):
        if self._drives_ga3c() or self._igm is not None:
            raise RuntimeError("the split step (step_begin / step_finish / step_overlapped) takes every action from the caller: "
                               "use step() while a policy is attached (attach_ga3c / attach_ig_mcts)")

    def step_finish(self, actions=None, auto_reset=False):
        """Second half of step(): everything else, with every agent's action in hand.  Same results as step(), bit for bit.
        Takes every action from the caller: refused while attach_ga3c / attach_ig_mcts drive agents inside step()."""
        self._refuse_split()
        self._refuse_split_keep(auto_reset, "step_finish")
        self._records_contract(auto_reset, "step_finish")
        a = self._actions(actions)
        _lib.call(self.L, self.h, "cagym_step_finish", _lib.ptr(a), C.byref(self._out), int(bool(auto_reset)), self._stream())
        self._after_steps(auto_reset, self.flags, self.reward, self.game_over, 1)
        return self._obs(), self.reward, self.game_over, {"flags": self.flags}

    def step_overlapped(self, policy, actions, auto_reset=False):
        """step() with a device policy in the loop: `policy(actions)` fills the external actions on the current stream (e.g.
        GA3CCADRLPolicy.act) WHILE the RVO half of the step runs on a side stream; the rest of the step follows both.
        Worth it when the policy leaves the GPU idle (a host-side or remote policy).  NOT for cagym_ga3c_act on the same GPU:
        measured on MI355X (profiles/r4/cfg4_overlap_trace_*.txt) the two kernels do run side by side, but sharing the CUs halves
        each one's occupancy and both take twice as long - 0.251 ms per cfg4 step against 0.194 ms for the fused launch."""
        self._refuse_split()
        self._refuse_split_keep(auto_reset, "step_overlapped")
        main = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(main)          # the previous step's state
        self.step_begin(stream=self._side)
        policy(actions)
        main.wait_stream(self._side)
        return self.step_finish(actions, auto_reset=auto_reset)

    def alloc_rollout(self, n_steps, obs=True):
        T, N, M, K, dev = int(n_steps), self.N, self.M, self.K, self.device
        buf = {"reward": torch.empty((T, N, M), dtype=torch.float32, device=dev),
               "flags": torch.empty((T, N, M), dtype=torch.uint8, device=dev),
               "game_over": torch.empty((T, N), dtype=torch.uint8, device=dev)}
        if obs:
            buf["other_agents_states"] = torch.empty((T, N, M, K, 10), dtype=torch.float32, device=dev)
            buf["ego"] = torch.empty((T, N, M, _lib.EGO_WIDTH), dtype=torch.float32, device=dev)
            if self.laserscan:
                buf["laserscan"] = torch.empty((T, N, M, 16), dtype=torch.float32, device=dev)
        if self._igm is not None:
            buf["team_reward"] = torch.empty((T, N), dtype=torch.float64, device=dev)
        return buf

    def rollout(self, n_steps, auto_reset=True, out=None):
        """n_steps env steps in one launch (all agents internally driven); returns [T, ...] buffers.  With GA3C attached and
        GA3C agents in the pool: T x (cagym_ga3c_act_merge, step), each step writing slice t of the buffers - no host
        synchronisation, so the chain can be captured in a graph.  With an episodic attach_ig_mcts: T x (robot inputs, belief
        update, team reward into out["team_reward"][t], plan, robot actions, step, episode boundary), no host synchronisation
        either; not under stream capture (the planner's call_base is a kernel argument the host advances per call).
        On a streaming env (stream_reference_scenarios) the ring is refilled ONCE, behind the last step: a world may finish at
        most n_scenarios / n_worlds - 1 episodes per launch.  A world that finishes more starts an episode on a slot that was not
        refilled (it replays an older scenario); nothing faults, and stream_stats()["n_lapped"] counts it - that is how a caller
        finds out, and the remedy is a shorter rollout or a deeper ring.
        With a trajectory ring attached (attach_trajectory_ring) rollout(auto_reset=True) gives up the single launch: the roll-out
        kernel keeps the agents on chip for all T steps and restarts finished worlds in place, so the state after each move never
        reaches memory where the ring's capture kernel could read it.  It runs T x (step, capture, reset) instead - the chain of
        step(auto_reset=True), each step writing slice t of the buffers, with one log update, one refill and one records update
        behind the last step, as the GA3C chain does; no host synchronisation.  The results are the single launch's, bit for bit;
        the cost is three launches per step (tools/terminal_cost.py measures it).  rollout() returns no terminal observations:
        with keep_terminal_observations() alone it stays the single launch."""
        self._records_contract(auto_reset, "rollout")
        T, g = int(n_steps), self._igm
        if g is not None and not g.episodic:
            raise RuntimeError("rollout() with %s attached is not implemented for this attach (the planner needs per-world "
                               "restarts): attach_%s(episodic=True)" % (g.kind, g.kind))
        if g is not None and torch.cuda.is_current_stream_capturing():
            if g.kind == "ig_greedy":
                raise RuntimeError("rollout() with ig_greedy attached cannot be captured in a graph: the chain allocates its "
                                   "observed-set buffers per step and has not been validated under capture")
            raise RuntimeError("rollout() with ig_mcts attached cannot be captured in a graph: the planner's call_base is a "
                               "by-value kernel argument that the host advances with every planning step")
        if out is None:
            out = self.alloc_rollout(T)
        if g is not None and out.get("team_reward") is None:
            out["team_reward"] = torch.empty((T, self.N), dtype=torch.float64, device=self.device)
        caller_out, out = out, self._records_out(out, T)
        if g is None and not self._drives_ga3c() and not (auto_reset and self._traj is not None):
            o = self._outputs(*[out.get(k) for k in _OUT_KEYS])
            rc = self._rollout_fn(self.h, T, int(bool(auto_reset)), C.byref(o), self._stream())
            if rc:
                _lib.check(self.L, self.h, rc, "cagym_rollout")
        else:
            # an IG team's detector reads the OtherAgentsStates table of the step before: slice t - 1, or the env's own table, which
            # every step writes when the caller asked for no observation slices and which ends up holding the last step's rows
            oas = out.get("other_agents_states") if g is not None else None
            restart = team_reward = prev = None  # what only an IG team needs (the GA3C-only chain stays capturable in a graph)
            for t in range(T):
                o = self._outputs(*[None if out.get(k) is None else out[k][t] for k in _OUT_KEYS])
                if g is not None:
                    team_reward, restart = out["team_reward"][t], out["game_over"][t] if auto_reset else None
                    if oas is None:
                        o.obs_oas = self.obs_oas.data_ptr()
                    elif t > 0:
                        prev = oas[t - 1]
                self._chained_step(None, o, auto_reset, restart, team_reward, prev)
            if oas is not None and T > 0:
                self.obs_oas.copy_(oas[T - 1])
        # one log update, one refill and one records update behind the last step, over all T slices, whichever chain ran
        self._after_steps(auto_reset, out.get("flags"), out.get("reward"), out.get("game_over"), T)
        return caller_out

    def kernel_name(self, rollout=True, auto_reset=True):
        """The kernel instantiation the library launches for this handle (as rocprofv3 --kernel-trace names it)."""
        buf = C.create_string_buffer(128)
        _lib.call(self.L, self.h, "cagym_kernel_name", int(bool(rollout)), int(bool(auto_reset)), buf, 128)
        return buf.value.decode()

    def sense_laserscan(self, out=None):
        if out is None:
            out = torch.empty((self.N, self.M, 16), dtype=torch.float32, device=self.device)
        _lib.call(self.L, self.h, "cagym_laserscan", out.data_ptr(), self._stream())
        return out

    # ---- per-world snapshot, restore and fork (include/cagym.h: cagym_snapshot / cagym_restore / cagym_fork) --------------------------
    def _id_list(self, ids, what, check, limit, distinct=True):
        """A world / row list (sequence, numpy array or tensor) as (contiguous i32 device tensor, host int64 array or None).
        Data that arrives on the host is validated there; a device tensor is read back (ONE synchronisation) unless
        check=False - then nothing is known on the host, and the kernel's bounds guard and _row_map's masks take over."""
        if torch.is_tensor(ids) and ids.is_cuda:
            t = ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if not check:
                return t, None
            host = t.cpu().numpy().astype(np.int64)
        else:
            host = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).astype(np.int64).reshape(-1)
            t = torch.as_tensor(host.astype(np.int32), device=self.device)
        if host.size and (host.min() < 0 or host.max() >= limit):
            raise ValueError("%s: ids must lie in [0, %d), got %d..%d" % (what, limit, host.min(), host.max()))
        if distinct and np.unique(host).size != host.size:
            raise ValueError("%s: the ids must be distinct" % what)
        return t, host

    def _outs(self):
        return {k: getattr(self, k) for k in _SNAP_OUT if getattr(self, k) is not None}

    def _row_map(self, dst, valid):
        """For lists the host could not validate (valid: bool [n] device mask of the usable entries, None: validated): world ->
        (row of the list that writes it, whether one does), through an inverse map with one spare slot for the skipped
        entries - no synchronisation, and an id out of range never indexes a tensor."""
        if valid is None or dst.shape[0] == 0:
            return None
        N = self.N
        inv = torch.full((N + 1,), -1, dtype=torch.long, device=self.device)
        inv.index_copy_(0, torch.where(valid, dst, torch.full_like(dst, N)), torch.arange(dst.shape[0], device=self.device))
        return inv[:N].clamp(min=0), inv[:N] >= 0

    @staticmethod
    def _put_rows(t, dst, vals, mapped):
        """t[dst[r]] = vals[r]; mapped: _row_map's pair for an unvalidated dst, else None."""
        if dst.shape[0] == 0:
            return
        if mapped is None:
            t.index_copy_(0, dst, vals)
            return
        row, has = mapped
        t.copy_(torch.where(has.view((-1,) + (1,) * (t.dim() - 1)), vals.index_select(0, row), t))

    def snapshot_layout(self):
        L = _lib.CagymSnapshotLayout()
        _lib.call(self.L, self.h, "cagym_snapshot_layout_of", C.byref(L))
        return L

    def snapshot(self, worlds=None, check=True):
        """The state of the listed worlds (default: all) as an EnvSnapshot: ONE cagym_snapshot launch on the current stream plus
        clones of those worlds' rows of the output tensors.  Everything a world carries from step to step is in it (after
        cagym_ig_init the belief too), except an attached planner's workspace and the scenario pool.  Does not disturb a
        pending step_begin.  worlds: distinct ids; a device tensor is validated with one synchronisation unless check=False."""
        L = self.snapshot_layout()
        if worlds is None:
            blob = torch.empty((self.N, int(L.row_bytes)), dtype=torch.uint8, device=self.device)
            _lib.call(self.L, self.h, "cagym_snapshot", None, self.N, blob.data_ptr(), self._stream())
            return EnvSnapshot(L, blob, torch.arange(self.N, dtype=torch.int32, device=self.device),
                               {k: v.clone() for k, v in self._outs().items()}, True, True)
        ids, host = self._id_list(worlds, "snapshot(worlds)", check, self.N)
        # rows of ids the kernel skips must not look like rows: zeros carry no magic
        blob = (torch.empty if host is not None else torch.zeros)((ids.numel(), int(L.row_bytes)), dtype=torch.uint8, device=self.device)
        _lib.call(self.L, self.h, "cagym_snapshot", ids.data_ptr(), ids.numel(), blob.data_ptr(), self._stream())
        pick = ids.long() if host is not None else ids.long().clamp(0, self.N - 1)
        return EnvSnapshot(L, blob, ids, {k: v.index_select(0, pick) for k, v in self._outs().items()}, False, host is not None)

    def _refuse_streaming(self, what, why):
        if self._streaming:
            raise RuntimeError("%s() on a streaming env: %s; stop_streaming() first" % (what, why))

    def _refuse_with_log(self, what):
        if self._log is not None:
            raise RuntimeError("%s() with an episode log attached: its running rows would describe another timeline (the library "
                               "refuses as long as the log is initialised)" % what)

    def _refuse_with_planner(self, what):
        if self._igm is not None:
            raise RuntimeError("%s() with %s attached: the planner's workspace, its published plans and the host-side call counter are "
                               "not part of a snapshot; detach_ig_mcts() first" % (what, self._igm.kind))

    def restore(self, snap, rows=None, check=True):
        """Put the rows of an EnvSnapshot (default: all; else distinct row indices into it) back, each into its origin world:
        ONE cagym_restore launch, then the same worlds' output rows.  A pending step_begin is void afterwards.  The snapshot
        may come from another handle of the same shape (resume): install the same scenario pool first.  Refused while an
        ig_mcts / ig_greedy planner is attached, while the env streams scenarios, and by the library while episode records are
        initialised."""
        self._refuse_with_planner("restore")
        self._refuse_with_log("restore")
        self._refuse_with_ring("restore")
        self._refuse_streaming("restore", "the ring of scenario slots is not part of a snapshot (a restored episode index would meet "
                               "other scenarios)")
        valid = None
        if rows is None and snap.all_worlds:  # whole tensors, and nothing allocated: the form a graph capture takes
            _lib.call(self.L, self.h, "cagym_restore", C.byref(snap.layout), snap.blob.data_ptr(), None, snap.n, self._stream())
            for k, t in self._outs().items():
                t.copy_(snap.outputs[k])
            return
        if rows is None:
            r, n, dst, vals = None, snap.n, snap.worlds.long(), snap.outputs
        else:
            r, host = self._id_list(rows, "restore(rows)", check, snap.n)
            n = r.numel()
            if host is None:  # nothing known on the host: rows outside the blob become -1, which the kernel skips
                valid = (r >= 0) & (r < snap.n)
                r = torch.where(valid, r, torch.full_like(r, -1))
            pick = r.long().clamp(0, max(snap.n - 1, 0))
            dst = snap.worlds.long().index_select(0, pick) if snap.n else snap.worlds.long()
            vals = {k: v.index_select(0, pick) for k, v in snap.outputs.items()} if snap.n else snap.outputs
        if not snap.trusted:
            in_range = (dst >= 0) & (dst < self.N)
            valid = in_range if valid is None else valid & in_range
        _lib.call(self.L, self.h, "cagym_restore", C.byref(snap.layout), snap.blob.data_ptr(), _lib.ptr(r), n, self._stream())
        mapped = self._row_map(dst, valid)
        for k, t in self._outs().items():
            self._put_rows(t, dst, vals[k], mapped)

    def fork(self, src, dst, check=True):
        """World dst[r] continues as a copy of world src[r]: cagym_fork (state rows except dst's own episode index and stat_*, and
        the pool rows of src's current scenario slot over dst's), then the same copy of the output rows.  dst ids are distinct
        and none is also a src.  Needs n_scenarios % n_worlds == 0; refused while a planner is attached, while the env streams
        scenarios, on handles with information-gain state and while episode records are initialised.  A pending step_begin is void
        afterwards."""
        self._refuse_with_planner("fork")
        self._refuse_with_log("fork")
        self._refuse_with_ring("fork")
        self._refuse_streaming("fork", "the ring of scenario slots is not part of a snapshot, and a refill would overwrite the forked slot")
        s, hs = self._id_list(src, "fork(src)", check, self.N, distinct=False)
        d, hd = self._id_list(dst, "fork(dst)", check, self.N)
        if s.numel() != d.numel():
            raise ValueError("fork: src and dst must have the same length (%d, %d)" % (s.numel(), d.numel()))
        if hs is not None and hd is not None and np.intersect1d(hs, hd).size:
            raise ValueError("fork: a world is both src and dst: %s" % np.intersect1d(hs, hd).tolist())
        _lib.call(self.L, self.h, "cagym_fork", s.data_ptr(), d.data_ptr(), s.numel(), self._stream())
        valid = None
        if hs is None or hd is None:
            valid = (s >= 0) & (s < self.N) & (d >= 0) & (d < self.N)
        pick, to = s.long().clamp(0, self.N - 1), d.long()
        mapped = self._row_map(to, valid)
        for t in self._outs().values():
            self._put_rows(t, to, t.index_select(0, pick), mapped)

    # ---- zero-copy state views --------------------------------------------------------------------
    def state(self):
        if self._state is None:
            sp = _lib.CagymStatePtrs()
            _lib.call(self.L, self.h, "cagym_get_state", C.byref(sp))
            N, M = self.N, self.M
            shapes = {"action": (N, M, 2), "n_agents": (N,), "episode": (N,), "stat_return": (N,),
                      "stat_episodes": (N,), "stat_steps": (N,), "stat_outcomes": (N, 3),
                      "map_bits": (self.S, 300, 10)}
            st = {}
            for name, ts in _lib.STATE_FIELDS:
                ptr = getattr(sp, name)
                if not ptr:
                    continue
                shape = shapes.get(name, (N, M))
                t = torch.as_tensor(_DevArray(ptr, shape, ts), device=self.device)
                st[name] = t.view(torch.int32) if ts == "u4" else t  # uint32 has few torch kernels
            self._state = st
        return self._state

    def episode_stats(self):
        s = self.state()
        return {k: s[k] for k in ("stat_return", "stat_episodes", "stat_steps", "stat_outcomes")}

    def packed_episode_stats(self, out=None):
        """[N, 6] int32 records (stats.py layout) written by ONE kernel on the current stream (cagym_pack_episode_stats)."""
        if out is None:
            out = torch.empty((self.N, 6), dtype=torch.int32, device=self.device)
        _lib.call(self.L, self.h, "cagym_pack_episode_stats", out.data_ptr(), self._stream())
        return out

    # ---- parity-test interface (f/u/i accessors used by tests/golden_util.replay) ----------------------------
    def f(self, name):
        torch.cuda.synchronize(self.device)
        s = self.state()
        g = lambda k: s[k].cpu().numpy()
        if name == "pos":
            return np.stack([g("pos_x"), g("pos_y")], -1)
        if name == "vel":
            return np.stack([g("vel_x"), g("vel_y")], -1)
        if name == "rel_goal":
            return np.stack([g("goal_x") - g("pos_x"), g("goal_y") - g("pos_y")], -1)
        if name == "oas":
            return self.obs_oas.double().cpu().numpy()
        if name == "laserscan":
            return self.obs_laser.double().cpu().numpy()
        if name == "reward":
            return self.reward.double().cpu().numpy()
        if name == "action":
            return g("action").astype(np.float64)
        return g(name)

    def u(self, name):
        torch.cuda.synchronize(self.device)
        if name == "game_over":
            return self.game_over.cpu().numpy()
        st = self.state()["status"].cpu().numpy().astype(np.uint32)
        bit = {"is_at_goal": _lib.FLAG_AT_GOAL, "was_at_goal_already": _lib.FLAG_WAS_AT_GOAL,
               "in_collision": _lib.FLAG_IN_COLLISION, "was_in_collision_already": _lib.FLAG_WAS_IN_COLLISION,
               "ran_out_of_time": _lib.FLAG_RAN_OUT_OF_TIME, "is_done": _lib.FLAG_DONE}[name]
        return ((st & bit) != 0).astype(np.uint8)

    def i(self, name):
        torch.cuda.synchronize(self.device)
        key = {"step_num": "step_num", "num_other_agents_observed": "n_observed"}[name]
        return self.state()[key].cpu().numpy()
