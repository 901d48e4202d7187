"""BatchedCollisionAvoidanceEnv: N worlds x M agents of the reference's CollisionAvoidanceEnv
(gym_collision_avoidance/envs/collision_avoidance_env.py) stepped by hand-written HIP kernels.

Vectorised convention of the reference's DummyVecEnv use (experiments/src/env_utils.py:29-31,
envs/wrappers.py:101-106): step(actions[N, M, 2]) -> (obs, rewards[N, M], game_over[N], info);
observations and outputs are PyTorch-ROCm tensors that the kernels write in place (zero-copy).

Here: construction and plumbing, the gym surface, the attached policies, the state views and the parity accessors; the scenario pool
is in _pool.py, the step consumers and the terminal observations in _consumers.py, snapshot / restore / fork in _snapshot.py,
checkpoint / load_checkpoint in _checkpoint.py.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import scenarios as sc
from ._checkpoint import EnvCheckpoint, _CheckpointMixin  # noqa: F401  (EnvCheckpoint is re-exported)
from ._consumers import _ConsumersMixin
from ._lib import _DevArray  # noqa: F401  (re-exported)
from ._pool import _PoolMixin
from ._snapshot import _SNAP_OUT, EnvSnapshot, _SnapshotMixin  # noqa: F401  (EnvSnapshot and _SNAP_OUT are re-exported)
from .dmcts import DeviceDecMCTSPlanner
from .ga3c import GA3CCADRLPolicy
from .ig import CONTEXT_ONLY_MASKED, EPISODE_FOLD, OBSERVE_ONLY_RESTARTED, GreedyPlanner, InfoGain

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (device index) -> hipStream_t as an int


class _IgState(object):
    """What step() needs of an attached IG policy, whichever it is: the primitives, the planner and the robots' input buffers."""
    __slots__ = ("kind", "ig", "R", "range", "episodic", "poses", "det", "n_det", "world", "planner",
                 "window", "rotate", "team_reward", "gain", "observed", "belief_window",  # (second row: attach_ig_learner's,
                 "context_window", "clear_max")  # third: its context=True)


class _IgGoals(object):
    """attach_ig_goals' state: the parameter block of the three launches and the tensors they keep."""
    __slots__ = ("P", "out", "goal_distance", "goal_reached", "choice",
                 "view", "own", "proposals", "proposals_k",  # (second row: ig_view_gain's / ig_propose_goals' buffers, made on first use)
                 "face_tol", "goal_heading", "goal_facing", "hview", "hprop",  # (third: goal headings, made by the first headings= call)
                 "last_proposal", "assign",  # (fourth: ig_assign_goals' - what the last proposal call was, its buffers made on first use)
                 "route")  # (fifth: ig_route_gains' buffers, made on first use)


class _IgCredit(object):
    """attach_ig_credit's state: the tensors the credit launch writes and the per-robot accumulators it keeps."""
    __slots__ = ("out", "acc")


_OUT_KEYS = ("other_agents_states", "ego", "laserscan", "reward", "flags", "game_over")  # a rollout's buffers in CagymOutputs order
GAME_OVER_MODES = {"agent0": _lib.GO_AGENT0, "all": _lib.GO_ALL, "learning": _lib.GO_LEARNING}


class BatchedCollisionAvoidanceEnv(_PoolMixin, _ConsumersMixin, _SnapshotMixin, _CheckpointMixin):
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
        self._rollout_fn = self.L.cagym_rollout
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
        # policies the env drives itself inside step() (attach_ga3c / attach_ig_mcts)
        self._ga3c = None
        self._igm = None
        self._goals = None        # attach_ig_goals' state, with attach_ig_learner only
        self._credit = None       # attach_ig_credit's state, with attach_ig_learner only
        self._act = None          # [N, M, 2] f32 action table of an internal step (the caller's buffer is only read)
        self.team_reward = None   # [N] f64: the team's MI reward of the last step with ig_mcts attached (policy.team_reward)
        self._init_pool()
        self._init_consumers()

    # ---- plumbing ------------------------------------------------------------------------------
    def _views(self, ptrs, fields, L=0):
        """_lib.views with this handle's sizes; L: the rows of the ring the pointers belong to."""
        return _lib.views(ptrs, fields, self.device, N=self.N, M=self.M, S=self.S, K=self.Kobs, L=L, C=len(_lib.TRAJ_COLUMNS))

    def _get_views(self, fn, ptrs, fields, rows=None):
        """The views of the pointer struct `ptrs` as the *_get call `fn` fills it; rows: its field that holds a ring's row count."""
        _lib.call(self.L, self.h, fn, C.byref(ptrs))
        return self._views(ptrs, fields, int(getattr(ptrs, rows)) if rows else 0)

    def _address_views(self, fn, fields):
        """The views of a call that hands out one device address per row of `fields` through void** parameters."""
        a = [C.c_void_p() for _ in fields]
        _lib.call(self.L, self.h, fn, *[C.byref(x) for x in a])
        return self._views({f[0]: x.value for f, x in zip(fields, a)}, fields)

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

    def sense_occupancy_grid(self, out=None):
        """'local_grid' observation of every agent (OccupancyGridSensor.sense): uint8 [N, M, 60, 60], 1 = occupied.
        Parity unpinned (cv2.warpAffine is restated, OpenCV is not installed): see include/cagym.h."""
        if out is None:
            out = torch.empty((self.N, self.M, 60, 60), dtype=torch.uint8, device=self.device)
        _lib.call(self.L, self.h, "cagym_occupancy_grid", out.data_ptr(), self._stream())
        return out

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
        if g is not None and g.kind == "ig_learner":
            if m is None:  # a new episode everywhere: prior beliefs, no running return, then the first observation of every world
                g.ig.reset_belief(None)
                g.ig.episode_stats["running"].zero_()
                if self._credit is not None:
                    self._credit.acc["running"].zero_()
                self._ig_observe(None, 0)
                if self._goals is not None:  # new maps everywhere: no goal survives
                    self._goals.out["active"].zero_()
            else:  # a manual restart of the masked worlds alone, inside the launch; not a finished episode, so nothing is folded
                self._ig_observe(m, OBSERVE_ONLY_RESTARTED)
            self._ig_goal_status(m)
        elif g is not None and g.episodic and m is not None:
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
        self._igm = self._goals = self._credit = None
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

    def attach_ig_learner(self, detect_fov=60.0, detect_range=5.0, window=24, rotate=True, context=False, clear_max=3.0):
        """From now on the IG robots are the CALLER's to move - their rows of step()'s `actions` are their (v, omega), as for any
        externally driven agent - and the env keeps what a learner needs around them: one belief per world, the team's MI reward,
        the episode accumulators of ig_episode_stats(), and the belief as each robot sees it.  Every step() and reset() is followed,
        on the same stream, by ONE cagym_ig_observe launch on the state it left (the observation follows the move: the learner's
        next action is chosen from it).  It writes, in place, self.team_reward [N] f64 and three more entries of step()'s info:
          "belief_window" [N, R, 3, window, window] f32 - robot k's ego-centred view of the world's belief, rows forward along its
              heading (along +x with rotate=False), columns to its left, 0.5 m cells: P(occupied), cell mutual information, 1
              inside the map (ig.belief_window_spec states the layout);
          "gain" [N] f64 - the MI sum over the cells the team just observed, on the updated belief;
          "observed" [N, 60] i64 - those cells (bit i of word j <=> cell (i, j)).
        team_reward is gain, except for a world that step(auto_reset=True) just restarted: its gain is the first observation of
        the new episode (on a prior belief, from the new start poses), which counts toward the new episode's return and is no
        reward for the action that ended the old one - team_reward is 0 there, and the old episode's return is folded into
        ig_episode_stats() before the new one starts.  reset() restarts every world and makes the first observation of each;
        reset(world_mask=m) does both for the masked worlds alone, without counting an episode, and leaves the other worlds'
        entries of the four tensors as they were.  Call reset() after attaching.  With attach_ga3c the GA3C agents' rows are the
        network's and every other row, the robots' included, the caller's.  Replaces attach_ig_mcts / attach_ig_greedy and is
        replaced by them; detach_ig_mcts() clears it.  rollout() is refused (it takes no external actions), and so is whatever an
        attached planner refuses: snapshot / restore / fork, checkpoint, terminal observations, the trajectory ring, the split step.
        context=True adds a second image in the same frame and on the same sample points, written by one more launch directly
        behind the observe launch (cagym_ig_context_window, with the same mask: a world the observe skips keeps its bytes here too):
          "context_window" [N, R, 3, window, window] f32 - what the built-in planners use and the belief does not show: the
              clearance min(EDF, clear_max) / clear_max of the world's current map (0 outside it), the other moving agents (1.0 a
              teammate's cell, 0.5 any other non-static agent's; the targets stay hidden) and 1 on the cells the team's sensors
              covered in this update, i.e. "observed" in the window's frame (ig.context_window_spec states the three channels).
        With the default context=False nothing is allocated, no launch runs and info has no such key."""
        window = int(window)
        if context and not (float(clear_max) > 0.0 and np.isfinite(float(clear_max))):
            raise ValueError("attach_ig_learner: clear_max must be finite and positive, got %r" % (clear_max,))
        if window < 4 or window > 64 or window % 2:
            raise ValueError("attach_ig_learner: window must be even and within 4..64, got %d" % window)
        if self._n_ig is not None and self._n_ig > 8:
            raise ValueError("attach_ig_learner: at most 8 IG robots per world (cagym_ig_observe), the pool has %d" % self._n_ig)
        self._attach_ig("ig_learner", detect_fov, detect_range, 1, True, lambda g: None)
        g, N, dev = self._igm, self.N, self.device
        g.window, g.rotate = window, bool(rotate)
        g.team_reward = torch.zeros((N,), dtype=torch.float64, device=dev)
        g.gain = torch.zeros((N,), dtype=torch.float64, device=dev)
        g.observed = torch.zeros((N, 60), dtype=torch.int64, device=dev)
        g.belief_window = torch.zeros((N, g.R, 3, window, window), dtype=torch.float32, device=dev)
        g.context_window, g.clear_max = None, float(clear_max)
        if context:
            g.context_window = torch.zeros((N, g.R, 3, window, window), dtype=torch.float32, device=dev)
        self.team_reward = g.team_reward
        return g.ig

    def _ig_observe(self, restart_mask, flags):
        g = self._igm
        g.ig.observe(g.R, g.range, self.obs_oas, g.window, g.rotate, restart_mask, flags, g.team_reward, g.gain, g.observed, g.belief_window)
        if g.context_window is not None:  # the second image, of the worlds the observe launch just wrote and of no other
            g.ig.context_window(g.R, g.context_window, g.window, g.rotate, g.clear_max, g.observed, restart_mask,
                                CONTEXT_ONLY_MASKED if flags & OBSERVE_ONLY_RESTARTED else 0)
        q = self._credit
        if q is not None:  # whose cone earned it: the same mask and flags, on the belief the observe launch just left
            g.ig.robot_credit(g.R, g.range, self.obs_oas, restart_mask, flags, q.out, q.acc)

    def attach_ig_credit(self):
        """Per-robot credit for the team reward (needs attach_ig_learner): from now on every observe launch - behind step() and
        reset() - is followed by ONE cagym_ig_credit launch with the same restart mask and flags (behind the context launch where
        there is one), and step()'s info gains
          "credit" [N, R, 3] f64 - per robot: own, the MI sum over the cells of its own cone; exclusive, over the cells no
              teammate saw as well; difference, the team's gain minus what the gain would have been had this robot not looked
              (its odds factor divided out of the cells it shares, its other cells dropped) - raw, as "gain" is;
          "robot_reward" [N, R, 3] f64 - credit, but 0 for a world the step just restarted, as team_reward is;
          "robot_observed" [N, R, 60] i64 - each robot's visible cells (their union is "observed");
          "loo" [N, R] f64 - the leave-one-out gain itself
        (ig.robot_credit_spec states all of it).  ig_robot_episode_stats() hands out per-robot accumulators kept as
        ig_episode_stats() keeps the team's.  reset(world_mask=m) leaves the other worlds' rows as they were.  Attaching another IG
        policy, or detach_ig_mcts(), drops it.  Without this call nothing is allocated, no launch runs and info has no such key.
        The built-in planners, the exploration episode log, rollout(), snapshot and checkpoint know nothing of it."""
        g = self._igm
        if g is None or g.kind != "ig_learner":
            raise RuntimeError("attach_ig_credit needs attach_ig_learner first: the credit is for the learner's robots")
        N, R, dev = self.N, g.R, self.device
        q = _IgCredit()
        q.out = {"gain": torch.zeros((N,), dtype=torch.float64, device=dev),
                 "robot_observed": torch.zeros((N, R, 60), dtype=torch.int64, device=dev),
                 "credit": torch.zeros((N, R, 3), dtype=torch.float64, device=dev),
                 "loo": torch.zeros((N, R), dtype=torch.float64, device=dev),
                 "reward": torch.zeros((N, R, 3), dtype=torch.float64, device=dev)}
        q.acc = {k: torch.zeros((N, R, 3), dtype=torch.float64, device=dev) for k in ("running", "sum", "last")}
        q.acc["episodes"] = torch.zeros((N,), dtype=torch.int32, device=dev)
        self._credit = q

    def ig_robot_credit(self):
        """The device tensors the last credit launch wrote (attach_ig_credit), by the names of InfoGain.robot_credit: gain [N] f64 -
        the team's gain as that launch recomputed it, observe's bit for bit -, robot_observed [N, R, 60] i64, credit [N, R, 3] f64,
        loo [N, R] f64 and reward [N, R, 3] f64 (info["robot_reward"])."""
        if self._credit is None:
            raise RuntimeError("ig_robot_credit() needs attach_ig_credit")
        return dict(self._credit.out)

    def ig_robot_episode_stats(self):
        """Device views of the per-robot accumulators attach_ig_credit keeps, [N, R, 3] f64 over (own, exclusive, difference):
        running - the return of the episode in progress, sum - over the finished episodes, last - of the last finished one; and
        episodes [N] i32, the finished episodes per world."""
        if self._credit is None:
            raise RuntimeError("ig_robot_episode_stats() needs attach_ig_credit")
        return dict(self._credit.acc)

    def attach_ig_goals(self, radius=0.5, v_max=2.0, w_max=np.pi, align_tol=np.pi / 4, goal_tol=0.25, face_tol=np.pi / 18):
        """Goal actions for the learner's robots (needs attach_ig_learner): from now on a robot may be given a PLACE to go to
        (ig_set_goals) instead of a (v, omega) per step, and while it holds an active goal step() overwrites its row of the action
        table with a controller's that descends the goal's geodesic field - the obstacle-aware shortest-path distance on the
        belief's 60 x 60 grid of 0.5 m cells, a cell free when the distance field at its centre passes the planners' test
        EDF > radius + 0.1 (ig.geodesic_spec; the controller: ig.goal_action_spec).  The controller turns at up to w_max towards
        the next cell's centre, drives at v_max once the heading error left after the step's turn is within align_tol, and stops
        within goal_tol of the goal point.  Robots without an active goal keep the caller's row: a team may mix both.  A world that
        restarts - under auto-reset, reset() or reset(world_mask=) - loses its robots' goals: its map is gone.  step()'s info gains
          "goal_distance" [N, R] f32 - the field at the robot's own cell, metres still to go along the grid (+inf: no active goal,
              outside the map, or the goal cannot be reached), and
          "goal_reached" [N, R] u8 - 1 when an active goal lies within goal_tol of the robot,
        both of the state the step left, written by one launch behind the observe launch (cagym_ig_goal_status); one launch in front
        of the step writes the rows (cagym_ig_goal_actions, on the env's own table: `actions` is only read).  Everything is
        stream-ordered, nothing synchronises.  Attaching another IG policy, or detach_ig_mcts(), drops the goals.
        A goal may carry a heading (ig_set_goals(..., headings=)): from the first such call on, a robot that has arrived turns on
        the spot to its goal's heading (cagym_ig_goal_face_actions behind the controller's launch) and info gains
          "goal_facing" [N, R] u8 - 1 when the robot is within goal_tol of an active goal and either has no goal heading or faces
              it within face_tol radians (cagym_ig_goal_face_status behind the status launch; ig.goal_face_spec states both).
        Until that call nothing of this is allocated or launched and info has no such key."""
        g = self._igm
        if g is None or g.kind != "ig_learner":
            raise RuntimeError("attach_ig_goals needs attach_ig_learner first: the goals drive the learner's robots")
        for name, val in (("radius", radius), ("v_max", v_max), ("w_max", w_max), ("align_tol", align_tol), ("goal_tol", goal_tol),
                          ("face_tol", face_tol)):
            if not (float(val) > 0.0 and np.isfinite(float(val))):
                raise ValueError("attach_ig_goals: %s must be finite and positive, got %r" % (name, val))
        N, R, dev = self.N, g.R, self.device
        q = _IgGoals()
        q.P = g.ig.goal_params(R, g.window, g.rotate, radius, v_max, w_max, align_tol, goal_tol)
        q.out = {"field": torch.full((N, R, 60, 60), float("inf"), dtype=torch.float32, device=dev),
                 "goal_xy": torch.zeros((N, R, 2), dtype=torch.float64, device=dev),
                 "active": torch.zeros((N, R), dtype=torch.uint8, device=dev)}
        q.goal_distance = torch.full((N, R), float("inf"), dtype=torch.float32, device=dev)
        q.goal_reached = torch.zeros((N, R), dtype=torch.uint8, device=dev)
        q.choice = torch.full((N, R), 255, dtype=torch.uint8, device=dev)
        q.view = q.own = q.proposals = q.proposals_k = q.last_proposal = q.assign = q.route = None
        q.face_tol, q.goal_heading, q.goal_facing, q.hview, q.hprop = float(face_tol), None, None, None, None
        self._goals = q
        self._alloc_act()

    def _need_goals(self, what):
        if self._goals is None:
            raise RuntimeError("%s needs attach_ig_goals" % what)
        return self._goals

    def ig_set_goals(self, goals, mask=None, frame="world", headings=None):
        """Give the masked robots (mask [N, R], default: every robot) a goal each, in ONE geodesic launch on the current stream
        followed by the status launch: goals [N, R, 2], with frame="world" points (x, y) in metres, with frame="window" cells (a, b)
        of each robot's belief window as the state has it now (a forward, b left - e.g. the argmax of a channel of
        info["belief_window"]).  A goal that is not finite or lies outside the map leaves its robot without an active goal.  Robots
        outside the mask keep every byte of their field, goal and active flag.
        headings [N, R] f64: the heading in radians each masked robot is to face once it has arrived, NaN for none (e.g.
        ig_propose_goals(headings=8)["heading"][:, :, 0]).  The first call with headings allocates goal_heading [N, R] (NaN) and
        switches on the two face launches and info["goal_facing"] (attach_ig_goals); a later call without headings stores NaN for
        the masked robots."""
        q = self._need_goals("ig_set_goals")
        if frame not in ("world", "window"):
            raise ValueError("ig_set_goals: frame must be 'world' or 'window', got %r" % (frame,))
        ig, N, R, dev = self._igm.ig, self.N, self._igm.R, self.device
        kw = {"points": goals} if frame == "world" else {"cells": goals}
        ig.geodesic(mask=mask, radius=q.P.radius, window=q.P.window, rotate=bool(q.P.rotate), out=q.out, **kw)
        if headings is not None and q.goal_heading is None:
            q.goal_heading = torch.full((N, R), float("nan"), dtype=torch.float64, device=dev)
            q.goal_facing = torch.zeros((N, R), dtype=torch.uint8, device=dev)
        if q.goal_heading is not None:
            new = torch.full((N, R), float("nan"), dtype=torch.float64, device=dev) if headings is None else \
                torch.as_tensor(headings, device=dev).to(torch.float64).reshape(N, R)
            if mask is None:
                q.goal_heading.copy_(new)
            else:
                m = torch.as_tensor(mask, device=dev).reshape(N, R) != 0
                q.goal_heading.copy_(torch.where(m, new, q.goal_heading))
        self._ig_goal_status(None)

    def ig_clear_goals(self, mask=None):
        """Take the goals of the masked robots (mask [N, R], default: every robot) away: their rows are the caller's again."""
        q = self._need_goals("ig_clear_goals")
        if mask is None:
            q.out["active"].zero_()
        else:
            q.out["active"].masked_fill_(torch.as_tensor(mask, device=self.device).reshape(self.N, -1).bool(), 0)
        self._ig_goal_status(None)

    def ig_goals(self):
        """Zero-copy device views of the goal state: field [N, R, 60, 60] f32 (indexed [j, i]), goal_xy [N, R, 2] f64, active
        [N, R] u8, goal_distance [N, R] f32, goal_reached [N, R] u8 and, once a goal has been given a heading, goal_heading
        [N, R] f64 (NaN: none) and goal_facing [N, R] u8."""
        q = self._need_goals("ig_goals")
        d = dict(q.out, goal_distance=q.goal_distance, goal_reached=q.goal_reached)
        if q.goal_heading is not None:
            d.update(goal_heading=q.goal_heading, goal_facing=q.goal_facing)
        return d

    def ig_view_gain(self, points=None, world_mask=None):
        """What a place is worth (needs attach_ig_goals, whose radius it uses; the range is attach_ig_learner's detect_range): ONE
        launch on the current stream (cagym_ig_view_gain, InfoGain.view_gain).  points [N, P, 2] in world metres, or None: the
        3600 cell centres.  Returns new device tensors gain f64, n_visible i32, valid u8, each [N, P], or [N, 60, 60] indexed
        [j, i] for the map; a world whose byte of world_mask [N] is 0 keeps what the (uninitialised) tensors held."""
        q = self._need_goals("ig_view_gain")
        return self._igm.ig.view_gain(points=points, world_mask=world_mask, radius=q.P.radius)

    def ig_view_gain_headings(self, points=None, headings=8, world_mask=None):
        """What a POSE is worth (needs attach_ig_goals, whose radius it uses; fov and range are attach_ig_learner's detect_fov and
        detect_range): ONE launch on the current stream (cagym_ig_view_gain_headings, InfoGain.view_gain_headings).  points
        [N, P, 2] in world metres, or None: the 3600 cell centres; headings: an int H, meaning h * 2 pi / H, or a sequence of
        1..16 radians.  Returns new device tensors gain_h f64 and n_visible_h i32 [N, P, H], best_heading i32, best_gain f64 and
        valid u8 [N, P] ([N, 60, 60, H] and [N, 60, 60] indexed [j, i] for the map), and "headings", the list used; for heading h
        the counted cells are exactly those the reward's sensor model sees from the pose (x, y, headings[h])."""
        q = self._need_goals("ig_view_gain_headings")
        return self._igm.ig.view_gain_headings(points=points, headings=headings, world_mask=world_mask, radius=q.P.radius)

    def ig_propose_goals(self, k=8, min_sep=2.0, d0=1.0, mask=None, headings=None):
        """The best k places of every masked robot (mask [N, R], default: every robot) on the belief and the map as they are now -
        a goal-level policy's discrete action space ("pick one of k").  Three launches on the current stream, nothing synchronises:
        the view-gain map of the worlds that have a masked robot (cagym_ig_view_gain), the geodesic field FROM every masked robot's
        own position, read from the state on the device, into a buffer of its own (cagym_ig_geodesic: the goal fields of ig_goals()
        keep every byte), and the proposals (cagym_ig_propose_goals): cells ranked by gain / (distance + d0), chosen best first,
        each suppressing the cells within min_sep metres of it (ig.propose_goals_spec).  The robots are the first R agent slots of
        every world, as generate_exploration_worlds / stream_exploration_worlds lay them out.  Returns the dict of device tensors
        cells [N, R, k, 2] i32 (i, j), xy [N, R, k, 2] f64, utility, gain [N, R, k] f64, distance [N, R, k] f32 and n_found [N, R]
        i32 (rows past n_found: cells -1, xy NaN, utility = gain = 0, distance +inf), and the view-gain map it ranked as
        view_gain / view_valid [N, 60, 60]; the buffers are allocated on the first call and written again by every later call with
        the same k, and a robot outside the mask keeps its rows.  ig_set_goals(prop["xy"][:, :, 0]) sends every robot to its best
        viewpoint (a robot with n_found = 0 gets a NaN goal: no active goal).
        headings=H or a sequence (ig_view_gain_headings'): the map that is ranked is the heading-resolved one's best_gain - what the
        best single sensor cone at a place sees, not a robot turning once round - and the result gains heading [N, R, k] f64, the
        heading of the chosen cell's best cone, and heading_index [N, R, k] i32, its index in this call's list (rows past n_found:
        NaN and -1), gathered on the device for the masked robots; view_gain is then that best_gain map.  The two are buffers like
        the other keys: a robot outside the mask keeps the rows an earlier headings call gave it - the heading in radians stays
        what it was, heading_index refers to THAT call's list - or NaN and -1 if there was none with this k.  The heading map is
        one buffer too: a call with another list of headings empties it first (valid 0, best_heading -1), so a world without a
        masked robot never shows indices of another list.  ig_set_goals(prop["xy"][:, :, 0], headings=prop["heading"][:, :, 0])
        sends every robot to its best pose."""
        q = self._need_goals("ig_propose_goals")
        g, N, dev = self._igm, self.N, self.device
        ig, R, k = g.ig, g.R, int(k)
        if k < 1 or k > 16:
            raise ValueError("ig_propose_goals: k must be within 1..16, got %d" % k)
        for name, val in (("min_sep", min_sep), ("d0", d0)):
            if not (float(val) > 0.0 and np.isfinite(float(val))):
                raise ValueError("ig_propose_goals: %s must be finite and positive, got %r" % (name, val))
        world_mask = None
        if mask is not None:
            mask = torch.as_tensor(mask, device=dev).to(torch.uint8).reshape(N, R).contiguous()
            world_mask = (mask != 0).any(dim=1).to(torch.uint8)
        if q.view is None:  # (zeroed once: a world that was never asked for has an empty map, not garbage)
            q.view = {"gain": torch.zeros((N, 60, 60), dtype=torch.float64, device=dev),
                      "n_visible": torch.zeros((N, 60, 60), dtype=torch.int32, device=dev),
                      "valid": torch.zeros((N, 60, 60), dtype=torch.uint8, device=dev)}
            q.own = {"field": torch.full((N, R, 60, 60), float("inf"), dtype=torch.float32, device=dev),
                     "goal_xy": torch.zeros((N, R, 2), dtype=torch.float64, device=dev),
                     "active": torch.zeros((N, R), dtype=torch.uint8, device=dev)}
        if q.proposals_k != k:
            q.proposals = {"cells": torch.full((N, R, k, 2), -1, dtype=torch.int32, device=dev),
                           "xy": torch.full((N, R, k, 2), float("nan"), dtype=torch.float64, device=dev),
                           "utility": torch.zeros((N, R, k), dtype=torch.float64, device=dev),
                           "gain": torch.zeros((N, R, k), dtype=torch.float64, device=dev),
                           "distance": torch.full((N, R, k), float("inf"), dtype=torch.float32, device=dev),
                           "n_found": torch.zeros((N, R), dtype=torch.int32, device=dev)}
            q.proposals_k = k
            if q.hprop is not None:  # (the rows of another k are gone: so are their headings)
                q.hprop["heading"] = q.hprop["heading_index"] = None
        if headings is None:
            ig.view_gain(world_mask=world_mask, radius=q.P.radius, out=q.view)
            gain_map, valid_map = q.view["gain"], q.view["valid"]
        else:
            if q.hview is None:  # (zeroed once, as the omni map above)
                q.hview = {"best_heading": torch.full((N, 60, 60), -1, dtype=torch.int32, device=dev),
                           "best_gain": torch.zeros((N, 60, 60), dtype=torch.float64, device=dev),
                           "valid": torch.zeros((N, 60, 60), dtype=torch.uint8, device=dev)}
            hs = tuple(ig.heading_list(headings))
            if q.hprop is None or q.hprop["list"] != hs:  # another list: uploaded once, and the map of the old one is emptied
                if q.hprop is not None:
                    q.hview["best_heading"].fill_(-1)
                    q.hview["best_gain"].zero_()
                    q.hview["valid"].zero_()
                old = q.hprop or {}
                q.hprop = {"list": hs, "table": torch.tensor(hs, dtype=torch.float64, device=dev), "heading": old.get("heading"),
                           "heading_index": old.get("heading_index")}
            if q.hprop["heading"] is None:
                q.hprop["heading"] = torch.full((N, R, k), float("nan"), dtype=torch.float64, device=dev)
                q.hprop["heading_index"] = torch.full((N, R, k), -1, dtype=torch.int32, device=dev)
            hv = ig.view_gain_headings(headings=list(hs), world_mask=world_mask, radius=q.P.radius, out=q.hview, want_rows=False)
            gain_map, valid_map = hv["best_gain"], hv["valid"]
        st = self.state()
        here = torch.stack((st["pos_x"][:, :R], st["pos_y"][:, :R]), dim=-1).contiguous()
        ig.geodesic(points=here, mask=mask, radius=q.P.radius, window=q.P.window, rotate=bool(q.P.rotate), out=q.own)
        ig.propose_goals(gain_map, valid_map, q.own["field"], k, min_sep, d0, mask=mask, out=q.proposals)
        res = dict(q.proposals, view_gain=gain_map, view_valid=valid_map)
        if headings is not None:  # the chosen cells' best cones: a gather on the device, nothing synchronises
            cells = q.proposals["cells"].long()
            found = cells[..., 0] >= 0
            flat = (cells[..., 1] * 60 + cells[..., 0]).clamp_(min=0).reshape(N, R * k)
            idx = torch.gather(hv["best_heading"].reshape(N, 3600), 1, flat).reshape(N, R, k)
            table = q.hprop["table"]
            idx = torch.where(found & (idx >= 0) & (idx < table.numel()), idx, torch.full_like(idx, -1))  # (never past the table)
            new = torch.where(idx >= 0, table[idx.clamp(min=0).long()], torch.full((), float("nan"), dtype=torch.float64, device=dev))
            if mask is None:
                q.hprop["heading_index"].copy_(idx)
                q.hprop["heading"].copy_(new)
            else:  # the masked robots' rows alone
                on = (mask != 0)[:, :, None]
                q.hprop["heading_index"].copy_(torch.where(on, idx, q.hprop["heading_index"]))
                q.hprop["heading"].copy_(torch.where(on, new, q.hprop["heading"]))
            res["heading_index"], res["heading"] = q.hprop["heading_index"], q.hprop["heading"]
        q.last_proposal = (headings is not None, float(d0))  # what ig_assign_goals reads: whether this call's rows carry headings, its d0
        return res

    def ig_assign_goals(self, mode="best", mask=None, claim_active=True, set_goals=True, d0=None):
        """Send the masked robots (mask [N, R], default: every robot) to COMPLEMENTARY viewpoints: ONE launch on the current stream
        (cagym_ig_assign_goals, InfoGain.assign_goals; ig.assign_goals_spec states the rule) on the buffers of the last
        ig_propose_goals call - its xy and distance, its heading rows if that call had headings=, and by default its d0.  Every
        proposal's visible cell set is a 60-word mask (the cone's with a heading, a robot turning on the spot without); the team
        claims masks one robot at a time, and every proposal still open is priced by the mutual information of the cells nobody has
        claimed yet, divided by distance + d0.  mode "best": every round assigns the best (robot, proposal) left; "slot": the
        masked robots choose in slot order.  claim_active: the robots OUTSIDE the mask whose goal is active keep what they are going
        to see from it - goal_xy, and goal_heading where one exists - before anybody chooses; a masked robot's own goal is no seed.
        Returns the dict of device tensors choice, order [N, R] i32 (-1: nothing was left to see), marginal, utility [N, R] f64,
        claimed [N, 60] i64, masks [N, R, k, 60] i64, round_gain [N, R, R, k] f64 indexed [round, robot, proposal] - what each of
        a robot's k options is worth GIVEN what its teammates are already going to see, NaN where it was not priced - and the
        gathered xy [N, R, 2] and heading [N, R] f64 of the chosen proposals, NaN where choice is -1 (and for robots outside the
        mask, whose rows of the other tensors keep what they held).  set_goals: then ig_set_goals(xy, mask=mask, headings=heading
        when the proposals carry headings): a masked robot for which nothing is left to see gets a NaN goal, that is, no active
        goal - its row is the caller's.  The robots are the first R agent slots, as ig_propose_goals assumes.  The buffers are
        allocated on the first call and written again by every later one with the same k; nothing synchronises."""
        q = self._need_goals("ig_assign_goals")
        if q.proposals is None or q.last_proposal is None:
            raise RuntimeError("ig_assign_goals needs an earlier ig_propose_goals call: it assigns that call's proposals")
        g, N, dev = self._igm, self.N, self.device
        ig, R, k = g.ig, g.R, q.proposals_k
        headed, d0_prop = q.last_proposal
        d0 = d0_prop if d0 is None else float(d0)
        if not (d0 > 0.0 and np.isfinite(d0)):
            raise ValueError("ig_assign_goals: d0 must be finite and positive, got %r" % (d0,))
        if mode not in _lib.IG_ASSIGN_MODES:
            raise ValueError("ig_assign_goals: mode must be 'slot' or 'best', got %r" % (mode,))
        if mask is not None:
            mask = torch.as_tensor(mask, device=dev).to(torch.uint8).reshape(N, R).contiguous()
        a = q.assign
        if a is None or a["masks"].shape[2] != k:
            a = q.assign = {"choice": torch.full((N, R), -1, dtype=torch.int32, device=dev),
                            "order": torch.full((N, R), -1, dtype=torch.int32, device=dev),
                            "marginal": torch.zeros((N, R), dtype=torch.float64, device=dev),
                            "utility": torch.zeros((N, R), dtype=torch.float64, device=dev),
                            "claimed": torch.zeros((N, 60), dtype=torch.int64, device=dev),
                            "masks": torch.zeros((N, R, k, 60), dtype=torch.int64, device=dev),
                            "round_gain": torch.full((N, R, R, k), float("nan"), dtype=torch.float64, device=dev)}
        seeds = {}
        if claim_active and mask is not None:  # (with every robot choosing there is nobody under way)
            seeds = dict(claim=q.out["active"], claim_xy=q.out["goal_xy"], claim_heading=q.goal_heading)
        ig.assign_goals(q.proposals["xy"], q.proposals["distance"], cand_heading=q.hprop["heading"] if headed else None, mask=mask,
                        mode=mode, radius=q.P.radius, d0=d0, out=a, **seeds)
        on = a["choice"] >= 0 if mask is None else (a["choice"] >= 0) & (mask != 0)
        idx = a["choice"].clamp(min=0).long()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        xy = torch.where(on[:, :, None], torch.gather(q.proposals["xy"], 2, idx[:, :, None, None].expand(N, R, 1, 2))[:, :, 0], nan)
        heading = torch.where(on, torch.gather(q.hprop["heading"], 2, idx[:, :, None])[:, :, 0], nan) if headed else torch.full_like(a["marginal"], float("nan"))
        if set_goals:
            self.ig_set_goals(xy, mask=mask, headings=heading if headed else None)
        return dict(a, xy=xy, heading=heading)

    def ig_route_gains(self, mask=None, stride=4, d0=None, exclude=None, set_goals=False):
        """Price what the masked robots (mask [N, R], default: every robot) see ON THE WAY to each of their proposals: ONE launch on
        the current stream (cagym_ig_route_gains, InfoGain.route_gains; ig.route_spec and ig.route_gains_spec state the rule) on the
        buffers of the last ig_propose_goals call - its cells, its field from every robot's own position, its heading rows if that
        call had headings=, and by default its d0.  Every proposal's shortest path is walked back on that field by the goal
        controller's neighbour rule; every `stride` cells along it, at most 16 times, the sensor cone is taken looking the way the
        robot drives; the union, and the union with the proposal's own view, are priced by the mutual information of their cells
        outside `exclude` [N, 60] i64 (e.g. ig_assign_goals(...)["claimed"]; default: nothing).  Returns the dict of device tensors
        route_masks, total_masks [N, R, k, 60] i64, route_gain, total_gain, utility [N, R, k] f64 (utility = total_gain / (distance
        + d0)), n_path, n_way [N, R, k] i32 (n_path -1: no route), truncated [N, R, k] u8, best [N, R] i32 (the proposal of largest
        utility that has a route and total_gain > 0; -1: none), and the gathered xy [N, R, 2] and heading [N, R] f64 of `best`, NaN
        where it is -1 (and for robots outside the mask, whose rows of the other tensors keep what they held).  set_goals: then
        ig_set_goals(xy, mask=mask, headings=heading when the proposals carry headings), exactly as ig_assign_goals does.  The
        buffers are allocated on the first call and written again by every later one with the same k; nothing synchronises, and
        step() gains no launch."""
        q = self._need_goals("ig_route_gains")
        if q.proposals is None or q.last_proposal is None:
            raise RuntimeError("ig_route_gains needs an earlier ig_propose_goals call: it prices that call's proposals")
        g, N, dev = self._igm, self.N, self.device
        ig, R, k = g.ig, g.R, q.proposals_k
        headed, d0_prop = q.last_proposal
        d0 = d0_prop if d0 is None else float(d0)
        if not (d0 > 0.0 and np.isfinite(d0)):
            raise ValueError("ig_route_gains: d0 must be finite and positive, got %r" % (d0,))
        if int(stride) < 1:
            raise ValueError("ig_route_gains: stride must be at least 1, got %r" % (stride,))
        if mask is not None:
            mask = torch.as_tensor(mask, device=dev).to(torch.uint8).reshape(N, R).contiguous()
        a = q.route
        if a is None or a["route_masks"].shape[2] != k:
            a = q.route = {"route_masks": torch.zeros((N, R, k, 60), dtype=torch.int64, device=dev),
                           "total_masks": torch.zeros((N, R, k, 60), dtype=torch.int64, device=dev),
                           "route_gain": torch.zeros((N, R, k), dtype=torch.float64, device=dev),
                           "total_gain": torch.zeros((N, R, k), dtype=torch.float64, device=dev),
                           "utility": torch.zeros((N, R, k), dtype=torch.float64, device=dev),
                           "n_path": torch.full((N, R, k), -1, dtype=torch.int32, device=dev),
                           "n_way": torch.zeros((N, R, k), dtype=torch.int32, device=dev),
                           "truncated": torch.zeros((N, R, k), dtype=torch.uint8, device=dev),
                           "best": torch.full((N, R), -1, dtype=torch.int32, device=dev)}
        ig.route_gains(q.own["field"], q.proposals["cells"], cand_heading=q.hprop["heading"] if headed else None, mask=mask,
                       exclude=exclude, stride=int(stride), radius=q.P.radius, d0=d0, out=a)
        on = a["best"] >= 0 if mask is None else (a["best"] >= 0) & (mask != 0)
        idx = a["best"].clamp(min=0).long()
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        xy = torch.where(on[:, :, None], torch.gather(q.proposals["xy"], 2, idx[:, :, None, None].expand(N, R, 1, 2))[:, :, 0], nan)
        heading = torch.where(on, torch.gather(q.hprop["heading"], 2, idx[:, :, None])[:, :, 0], nan) if headed else torch.full_like(xy[:, :, 0], float("nan"))
        if set_goals:
            self.ig_set_goals(xy, mask=mask, headings=heading if headed else None)
        return dict(a, xy=xy, heading=heading)

    def _ig_goal_status(self, restart_mask):
        q = self._goals
        if q is not None:
            self._igm.ig.goal_status(q.P, q.out, q.goal_distance, q.goal_reached, restart_mask)
            if q.goal_heading is not None:
                self._igm.ig.goal_face_status(q.P, q.out, q.goal_heading, q.goal_facing, q.face_tol)

    def detach_ig_mcts(self):
        self._igm = self._goals = self._credit = None
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
            raise RuntimeError("ig_episode_stats() needs attach_ig_mcts, attach_ig_greedy or attach_ig_learner")
        return dict(self._igm.ig.episode_stats)

    def _internal_actions(self, a, team_reward_out=None, oas=None):
        """The action table the step reads: the caller's `a` (or None) when nothing is attached, else the env's own buffer.
        team_reward_out: where the team reward of this step goes (rollout: slice t of its buffer); oas: the OtherAgentsStates
        table the last step wrote, when that is not self.obs_oas (rollout: slice t - 1)."""
        ga3c = self._drives_ga3c()
        plans = self._igm is not None and self._igm.kind != "ig_learner"  # (a learner's robots are driven by the caller's rows)
        goals = self._goals  # ... or, with attach_ig_goals, by the goal controller's, written over a copy of the caller's table
        if not ga3c and not plans and goals is None:
            return a
        table = self._act
        if ga3c:
            self._ga3c.act_merge(a, table)
        elif a is None:
            table.zero_()
        else:
            table.copy_(a)
        if plans:
            g = self._igm
            g.ig.robot_inputs(g.R, g.range, self.obs_oas if oas is None else oas, g.poses, g.det, g.n_det)
            observed = g.ig.update_belief(g.poses, g.det, g.n_det)
            self.team_reward = g.ig.mi_reward(observed, g.world, out=team_reward_out)  # before the move, as the reference computes it
            planned, _ = g.planner.plan(g.poses)
            g.ig.robot_actions(g.R, planned, table)
        if goals is not None:
            self._igm.ig.goal_actions(goals.P, goals.out, table, goals.choice)
            if goals.goal_heading is not None:
                self._igm.ig.goal_face_actions(goals.P, goals.out, goals.goal_heading, table)
        return table

    def _chained_step(self, a, o, auto_reset, restart, team_reward_out=None, oas=None, term=False):
        """One step with whatever is attached, three parts in stream order: the internal actions (_internal_actions), the step
        launch into the CagymOutputs `o`, and the episodic IG team's end of the step - its episode log's update
        (attach_ig_episode_log), then its running return and the restart of the worlds of `restart` (under auto_reset the
        game_over tensor `o` points at, else None).  term: hand the env's terminal buffers
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
        if self._iglog is not None and g is not None and restart is not None:  # rows of the finished worlds, before their beliefs restart
            self._ig_log_update(restart, None if g.kind == "ig_learner" else self.team_reward)
        if g is not None and g.kind == "ig_learner":  # the observation of the state the step left; restarted worlds fold and start anew
            self._ig_observe(restart, EPISODE_FOLD if restart is not None else 0)
            self._ig_goal_status(restart)  # (attach_ig_goals: the restarted worlds lose their goals)
        elif g is not None and g.episodic:
            g.ig.episode_boundary(g.planner.P, g.planner.workspace, self.team_reward, restart, EPISODE_FOLD)

    def step(self, actions=None, auto_reset=False):
        """One env.step() of every world.  auto_reset=True: finished worlds restart inside the same launch
        (VecEnv semantics: the returned observation is the first one of the new episode).  With a policy attached
        (attach_ga3c / attach_ig_mcts) its agents' rows of `actions` are ignored and the env computes them; `actions`
        itself is only read.  With attach_ig_learner the robots' rows are the learner's (v, omega), and info also carries
        "belief_window", "gain" and "observed" of the state the step left, with context=True "context_window", with
        attach_ig_credit "credit", "robot_reward", "robot_observed" and "loo", and with
        attach_ig_goals "goal_distance" and "goal_reached" (and "goal_facing" once a goal has carried a heading)."""
        if auto_reset and self._igm is not None and not self._igm.episodic:
            k = self._igm.kind
            raise RuntimeError("step(auto_reset=True) with %s attached: the planner's per-world restart (beliefs, "
                               "communicated plans) is not implemented for this attach; attach_%s(episodic=True), or step "
                               "without auto-reset and reset() yourself" % (k, k))
        self._records_contract(auto_reset, "step")
        self._chained_step(self._actions(actions), self._out, auto_reset, self.game_over if auto_reset else None, term=True)
        self._after_steps(auto_reset, self.flags, self.reward, self.game_over, 1)
        info = {"flags": self.flags}
        g = self._igm
        if g is not None and g.kind == "ig_learner":
            info.update(belief_window=g.belief_window, gain=g.gain, observed=g.observed)
            if g.context_window is not None:
                info["context_window"] = g.context_window
            if self._credit is not None:
                o = self._credit.out
                info.update(credit=o["credit"], robot_reward=o["reward"], robot_observed=o["robot_observed"], loo=o["loo"])
            if self._goals is not None:
                info.update(goal_distance=self._goals.goal_distance, goal_reached=self._goals.goal_reached)
                if self._goals.goal_heading is not None:
                    info["goal_facing"] = self._goals.goal_facing
        if auto_reset and self._term is not None:
            info["terminal"] = dict(self._term, valid=self.game_over)
        return self._obs(), self.reward, self.game_over, info

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
        if g is not None and g.kind == "ig_learner":
            raise RuntimeError("rollout() with ig_learner attached: the learner's robots need the caller's actions at every step; use step()")
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

    # ---- zero-copy state views --------------------------------------------------------------------
    def state(self):
        if self._state is None:
            self._state = self._get_views("cagym_get_state", _lib.CagymStatePtrs(), _lib.STATE_FIELDS)
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
