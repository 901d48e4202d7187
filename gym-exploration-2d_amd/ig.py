"""Information-gain planner primitives on device (cagym_ig_* of include/cagym.h).

Counterparts of the reference's targetMap / edfMap objects and of the Dec-MCTS roll-out primitives
(information_models/targetMap.py, information_models/edfMap.py, policies/ig_mcts.py:117-253,
policies/pydecmcts/DecMCTS.py:233-271).  Visibility sets are [.., 60] int64 tensors (bit i of word j
<=> belief cell (i, j)); the tree bookkeeping (UCT select / expand / back-propagate) stays with the caller.
"""
import ctypes as C
import heapq
import math

import numpy as np
import torch

from . import _lib

EPISODE_FOLD, EPISODE_PLANS_ONLY = 1, 2  # CAGYM_IG_EPISODE_* (include/cagym.h)
OBSERVE_ONLY_RESTARTED = _lib.IG_OBSERVE_ONLY_RESTARTED  # cagym_ig_observe's second flag, beside EPISODE_FOLD
CONTEXT_ONLY_MASKED = _lib.IG_CONTEXT_ONLY_MASKED  # cagym_ig_context_window's flag
FOV_DEG60 = 60.0 * np.pi / 180  # detect_fov=60.0 -> targetMap.sensFOV (ig_mcts.py:67)
PRIMITIVES = np.array([[v, w] for v in (0.0, 2.0, 4.0) for w in (-0.5 * np.pi, 0.0, 0.5 * np.pi)])  # ig_mcts.py:247-253
GREEDY_V, GREEDY_W = (0.0, 2.0, 4.0), (-np.pi, 0.0, np.pi)  # ig_greedy.py:65-66: candidate c = 3 a + b is (v[a], w[b])


GreedyParams = _lib.GreedyParams  # the struct mirrors live beside the prototypes


class InfoGain(object):
    def __init__(self, benv, fov_rad=FOV_DEG60, sens_range=5.0, xdt=5, dt=0.1):
        self.b = benv
        self.L = benv.L
        self.fov, self.range, self.xdt, self.dt = float(fov_rad), float(sens_range), int(xdt), float(dt)
        _lib.call(self.L, self.b.h, "cagym_ig_init", benv._stream())
        v = benv._address_views("cagym_ig_get", _lib.IG_FIELDS)
        self.edf_d2, self.belief = v["edf_d2"], v["belief"]
        # the team reward's per-world episode accumulators (cagym_ig_episode_boundary); zeroed by cagym_ig_init
        self.episode_stats = benv._address_views("cagym_ig_get_episode_stats", _lib.IG_EPISODE_FIELDS)

    def _t(self, x, dtype, shape=None):
        t = torch.as_tensor(x, device=self.b.device).to(dtype)
        if shape is not None:
            t = t.reshape(shape)
        return t.contiguous()

    def _dev(self, x, dtype, shape=None):
        """x itself (the same memory: callers rely on in-place writes) when it is a contiguous device tensor of that dtype, else _t's copy."""
        as_it_is = torch.is_tensor(x) and x.is_cuda and x.dtype == dtype and x.is_contiguous()
        return x if as_it_is else self._t(x, dtype, shape)

    def _out(self, out, spec):
        """`out` when the caller gave one, else new device tensors of spec = {name: (shape, dtype)}."""
        return out if out is not None else {k: torch.empty(s, dtype=d, device=self.b.device) for k, (s, d) in spec.items()}

    def _viewpoints(self, points, world_mask):
        """view_gain()'s and view_gain_headings()'s places: (points [N,P,2] f64 or None for the map, world_mask [N] u8 or None, the
        shape of a per-point output, n_points of the parameter block)."""
        N = self.b.N
        if points is not None:
            points = self._dev(points, torch.float64).reshape(N, -1, 2)
        shape = (N, 60, 60) if points is None else (N, points.shape[1])
        if world_mask is not None:
            world_mask = self._t(world_mask, torch.uint8, (N,))
        return points, world_mask, shape, 0 if points is None else shape[1]

    def robot_inputs(self, n_robots, detect_range, obs_oas, poses, detections, n_det):
        """cagym_ig_robot_inputs: the R robots' poses [N,R,3] and detections [N,R,M-1,2] / n_det [N,R] (the detector emulation of
        find_targets_in_obs on their rows of obs_oas), written into the given device tensors."""
        _lib.call(self.L, self.b.h, "cagym_ig_robot_inputs", int(n_robots), float(detect_range), obs_oas.data_ptr(), poses.data_ptr(),
                  detections.data_ptr(), n_det.data_ptr(), self.b._stream())

    def robot_actions(self, n_robots, planner_actions, actions):
        """cagym_ig_robot_actions: the planner's (v, omega) [N,R,2] f64 into the robots' rows of actions [N,M,2] f32."""
        _lib.call(self.L, self.b.h, "cagym_ig_robot_actions", int(n_robots), planner_actions.data_ptr(), actions.data_ptr(), self.b._stream())

    def edf(self):
        """[S,300,300] f64 Euclidean distance field in metres (edfMap.map)."""
        return self.edf_d2.double().sqrt() * 0.1

    def reset_belief(self, world_mask=None):
        m = self.b._mask(world_mask)
        _lib.call(self.L, self.b.h, "cagym_ig_reset_belief", _lib.ptr(m), self.b._stream())

    def episode_boundary(self, params, workspace, team_reward=None, restart_mask=None, flags=0):
        """cagym_ig_episode_boundary on the current stream: running += team_reward [N] f64; the worlds of the DEVICE mask
        restart_mask [N] u8 get a prior belief, no communicated plans (params / workspace: the planner's) and running = 0, after
        folding it into sum / last / episodes with EPISODE_FOLD.  EPISODE_PLANS_ONLY: only the plans are forgotten."""
        if restart_mask is not None and (restart_mask.dtype != torch.uint8 or not restart_mask.is_cuda or not restart_mask.is_contiguous()):
            restart_mask = self._t(restart_mask, torch.uint8, (self.b.N,))
        if team_reward is not None and (team_reward.dtype != torch.float64 or not team_reward.is_contiguous()):
            team_reward = self._t(team_reward, torch.float64, (self.b.N,))
        _lib.call(self.L, self.b.h, "cagym_ig_episode_boundary", C.byref(params), _lib.ptr(team_reward), _lib.ptr(restart_mask), int(flags),
                  workspace.data_ptr(), workspace.numel(), self.b._stream())

    def observe(self, n_robots, detect_range, obs_oas, window=24, rotate=True, restart_mask=None, flags=0, team_reward=None, gain=None,
                observed=None, belief_window=None):
        """cagym_ig_observe: ONE launch on the current stream behind the step or reset that wrote obs_oas - the restart of the worlds
        of the DEVICE mask restart_mask [N] u8 (EPISODE_FOLD folds their running return, OBSERVE_ONLY_RESTARTED skips every other
        world), the robots' poses and detections, the belief update, the MI sum over the observed cells and the robots' belief
        windows.  Every output is a contiguous device tensor to write into, or None: team_reward / gain [N] f64, observed [N,60]
        i64, belief_window [N,R,3,G,G] f32."""
        P = _lib.IgObserveParams(int(n_robots), int(window), int(rotate), int(flags), float(detect_range), self.fov, self.range)
        _lib.call(self.L, self.b.h, "cagym_ig_observe", C.byref(P), obs_oas.data_ptr(), _lib.ptr(restart_mask), _lib.ptr(team_reward),
                  _lib.ptr(gain), _lib.ptr(observed), _lib.ptr(belief_window), self.b._stream())

    def context_window(self, n_robots, context_window, window=24, rotate=True, clear_max=3.0, observed=None, world_mask=None, flags=0):
        """cagym_ig_context_window: ONE launch on the current stream, directly behind observe() - the robots' second image
        context_window [N,R,3,G,G] f32 (a contiguous device tensor to write into) on the belief window's sample points: clearance
        min(EDF, clear_max) / clear_max on the world's current scenario slot, the other non-static agents (1.0 a teammate, 0.5
        anything else) and the cells of `observed` [N,60] i64 (the tensor observe() just wrote, or None: nothing seen).
        CONTEXT_ONLY_MASKED in flags skips the worlds whose byte of the DEVICE mask world_mask [N] u8 is 0."""
        P = _lib.IgContextParams(int(n_robots), int(window), int(rotate), int(flags), float(clear_max))
        _lib.call(self.L, self.b.h, "cagym_ig_context_window", C.byref(P), _lib.ptr(observed), _lib.ptr(world_mask),
                  context_window.data_ptr(), self.b._stream())

    def goal_params(self, n_robots, window=24, rotate=True, radius=0.5, v_max=2.0, w_max=np.pi, align_tol=np.pi / 4, goal_tol=0.25):
        """The cagym_ig_goal_params block of geodesic() / goal_actions() / goal_status() (dt is this object's)."""
        return _lib.IgGoalParams(int(n_robots), int(window), int(rotate), 0, float(radius), float(v_max), float(w_max), float(align_tol),
                                 float(goal_tol), self.dt)

    def geodesic(self, points=None, cells=None, mask=None, radius=0.5, window=24, rotate=True, out=None):
        """cagym_ig_geodesic: ONE launch on the current stream, one workgroup per (world, robot) - the obstacle-aware shortest-path
        distance on the 60 x 60 belief grid FROM a source point per robot, on the world's current map: `points` [N,R,2] f64 in world
        metres, or `cells` [N,R,2] i32, a cell (a, b) of each robot's belief window (window, rotate: attach_ig_learner's) on the
        pose the state holds now - exactly one of the two.  mask [N,R] u8 or None (every robot): a robot whose byte is 0 keeps every
        byte of its outputs.  A cell is free when EDF(centre) > radius + 0.1, the planners' test; ig.geodesic_spec states the rest.
        With the robots' own positions as sources it tells which candidate goals each robot can reach before one is chosen.
        Returns the dict of device tensors it wrote: field [N,R,60,60] f32 indexed [j, i] (+inf: blocked or unreachable), goal_xy
        [N,R,2] f64 the point used, active [N,R] u8 (0: the point is not finite or outside the map; its field is all +inf), sweeps
        [N,R] i32 the relaxation sweeps run; `out`: such a dict to write into again (default: new tensors)."""
        if (points is None) == (cells is None):
            raise ValueError("geodesic: exactly one of points and cells must be given")
        N = self.b.N
        src = (self._dev(points, torch.float64) if points is not None else self._dev(cells, torch.int32)).reshape(N, -1, 2)
        R = src.shape[1]
        if mask is not None:
            mask = self._t(mask, torch.uint8, (N, R))
        out = self._out(out, {"field": ((N, R, 60, 60), torch.float32), "goal_xy": ((N, R, 2), torch.float64),
                              "active": ((N, R), torch.uint8), "sweeps": ((N, R), torch.int32)})
        P = self.goal_params(R, window, rotate, radius)
        _lib.call(self.L, self.b.h, "cagym_ig_geodesic", C.byref(P), _lib.ptr(mask), _lib.ptr(src if points is not None else None),
                  _lib.ptr(src if cells is not None else None), out["field"].data_ptr(), out["goal_xy"].data_ptr(),
                  out["active"].data_ptr(), _lib.ptr(out.get("sweeps")), self.b._stream())
        return out

    def goal_actions(self, params, goals, actions, choice=None):
        """cagym_ig_goal_actions: the rows of the robots with an active goal in the action table `actions` [N,M,2] f32 (in place);
        goals: geodesic()'s dict; choice [N,R] u8 or None: what each robot aims at (0..7 neighbour, 8 the goal point, 255 nothing)."""
        _lib.call(self.L, self.b.h, "cagym_ig_goal_actions", C.byref(params), goals["field"].data_ptr(), goals["goal_xy"].data_ptr(),
                  goals["active"].data_ptr(), actions.data_ptr(), _lib.ptr(choice), self.b._stream())

    def goal_status(self, params, goals, goal_distance, goal_reached, restart_mask=None):
        """cagym_ig_goal_status: behind the step and observe() - active = 0 for the worlds of the DEVICE mask restart_mask [N] u8,
        then goal_distance [N,R] f32 (the field at the robot's cell) and goal_reached [N,R] u8."""
        _lib.call(self.L, self.b.h, "cagym_ig_goal_status", C.byref(params), _lib.ptr(restart_mask), goals["field"].data_ptr(),
                  goals["goal_xy"].data_ptr(), goals["active"].data_ptr(), goal_distance.data_ptr(), goal_reached.data_ptr(),
                  self.b._stream())

    def view_params(self, n_points=0, n_robots=1, k=1, radius=0.5, range=None, min_sep=2.0, d0=1.0):
        """The cagym_ig_view_params block of view_gain() / propose_goals() (range: this object's sensing range by default)."""
        return _lib.IgViewParams(int(n_points), int(n_robots), int(k), 0, float(radius), float(self.range if range is None else range),
                                 float(min_sep), float(d0))

    def view_gain(self, points=None, world_mask=None, radius=0.5, range=None, out=None):
        """cagym_ig_view_gain: ONE launch on the current stream - what a place is worth: the mutual information of every belief cell
        a robot standing there could see through the walls of the world's current map, turning on the spot (no field of view, no
        heading; ig.view_gain_spec states the rule).  `points` [N,P,2] f64 in world metres, or None: the 3600 cell centres - "the
        map", whose values are the points call's on the same points bit for bit.  world_mask [N] u8 or None (every world): a world
        whose byte is 0 keeps every byte of its outputs.  range: the sensing range (default: this object's).  Returns the dict of
        device tensors it wrote: gain f64, n_visible i32, valid u8 (0: not finite, outside the map or within radius + 0.1 of an
        obstacle; its gain and n_visible are 0), each [N,P], or [N,60,60] indexed [j, i] for the map; `out`: such a dict to write
        into again (default: new tensors)."""
        points, world_mask, shape, n_points = self._viewpoints(points, world_mask)
        out = self._out(out, {"gain": (shape, torch.float64), "n_visible": (shape, torch.int32), "valid": (shape, torch.uint8)})
        P = self.view_params(n_points=n_points, radius=radius, range=range)
        _lib.call(self.L, self.b.h, "cagym_ig_view_gain", C.byref(P), _lib.ptr(world_mask), _lib.ptr(points), out["gain"].data_ptr(),
                  out["n_visible"].data_ptr(), out["valid"].data_ptr(), self.b._stream())
        return out

    def propose_goals(self, gain, valid, field, k, min_sep, d0, mask=None, out=None):
        """cagym_ig_propose_goals: ONE launch on the current stream, one workgroup per (world, robot) - the best k places of each
        robot: gain, valid [N,60,60] a view-gain map (view_gain()'s), field [N,R,60,60] f32 the geodesic field FROM the robot's own
        place (geodesic(points=robot positions)["field"]).  A cell is eligible when valid, gain > 0 and field finite; its utility
        is gain / (field + d0); k rounds take the best cell left and suppress every cell within min_sep metres of it
        (ig.propose_goals_spec states the rule).  mask [N,R] u8 or None (every robot): a robot whose byte is 0 keeps every byte of
        its outputs.  Returns the dict of device tensors it wrote: cells [N,R,k,2] i32 (i, j), xy [N,R,k,2] f64 their centres,
        utility, gain [N,R,k] f64, distance [N,R,k] f32, n_found [N,R] i32; rows past n_found hold cells -1, xy NaN, utility =
        gain = 0, distance +inf.  `out`: such a dict to write into again (default: new tensors)."""
        N = self.b.N
        field = self._dev(field, torch.float32).reshape(N, -1, 60, 60)
        R, k = field.shape[1], int(k)
        gain = self._dev(gain, torch.float64, (N, 60, 60))
        valid = self._dev(valid, torch.uint8, (N, 60, 60))
        if gain.numel() != N * 3600 or valid.numel() != N * 3600:
            raise ValueError("propose_goals: gain and valid must be [N, 60, 60] maps")
        if mask is not None:
            mask = self._t(mask, torch.uint8, (N, R))
        P = self.view_params(n_robots=R, k=k, min_sep=min_sep, d0=d0)
        kk = max(k, 1)  # (a k the library refuses: nothing is written)
        out = self._out(out, {"cells": ((N, R, kk, 2), torch.int32), "xy": ((N, R, kk, 2), torch.float64), "utility": ((N, R, kk), torch.float64),
                              "gain": ((N, R, kk), torch.float64), "distance": ((N, R, kk), torch.float32), "n_found": ((N, R), torch.int32)})
        _lib.call(self.L, self.b.h, "cagym_ig_propose_goals", C.byref(P), _lib.ptr(mask), gain.data_ptr(), valid.data_ptr(), field.data_ptr(),
                  *[out[n].data_ptr() for n in ("cells", "xy", "utility", "gain", "distance", "n_found")], self.b._stream())
        return out

    def assign_goals(self, cand_xy, cand_distance, cand_heading=None, mask=None, claim=None, claim_xy=None, claim_heading=None, mode="best",
                     radius=0.5, range=None, d0=1.0, out=None, want_rounds=True):
        """cagym_ig_assign_goals: ONE launch on the current stream, one workgroup per world - a TEAM's goals by the sequential-greedy
        allocation of coverage (ig.assign_goals_spec states the rule).  cand_xy [N,R,k,2] f64 and cand_distance [N,R,k] f32: every
        robot's k candidate goals and how far each is (propose_goals()' xy and distance); cand_heading [N,R,k] f64 or None: with a
        finite heading a candidate's cell set is visible_cells() of the pose (this object's fov), without one (NaN, or None for
        all) the cells view_gain() counts at the point.  mask [N,R] u8 or None (every robot): the robots that choose now; a robot
        whose byte is 0 keeps every byte of its rows, and a world without a masked robot is not touched at all.  claim [N,R] u8
        with claim_xy [N,R,2] f64 and claim_heading [N,R] f64 or None: robots OUTSIDE the mask whose claim byte is set keep the
        cells of that pose - teammates under way.  Every candidate is priced by mi_reward() of its cells that nobody has claimed
        yet (bit for bit), and ranked by that marginal gain / (distance + d0).  mode "slot": the masked robots choose in slot
        order; "best": every round assigns the best (robot, candidate) left.  Returns the dict of device tensors it wrote: choice,
        order [N,R] i32 (-1: nothing was left to see), marginal, utility [N,R] f64, claimed [N,60] i64 the final union, masks
        [N,R,k,60] i64 every candidate's cell set before any claim and, with want_rounds, round_gain [N,R,R,k] f64 indexed [round,
        robot, candidate] (NaN: not priced in that round).  `out`: such a dict to write into again (default: new tensors)."""
        N = self.b.N
        if mode not in _lib.IG_ASSIGN_MODES:
            raise ValueError("assign_goals: mode must be 'slot' or 'best', got %r" % (mode,))
        dist = self._dev(cand_distance, torch.float32)
        if dist.dim() != 3 or dist.shape[0] != N:
            raise ValueError("assign_goals: cand_distance must be [N, R, k]")
        R, k = int(dist.shape[1]), int(dist.shape[2])
        xy = self._dev(cand_xy, torch.float64).reshape(N, R, k, 2)
        hd = None if cand_heading is None else self._dev(cand_heading, torch.float64).reshape(N, R, k)
        if mask is not None:
            mask = self._t(mask, torch.uint8, (N, R))
        if claim is not None:
            if claim_xy is None:
                raise ValueError("assign_goals: claim needs claim_xy")
            claim = self._t(claim, torch.uint8, (N, R))
        cxy = None if claim_xy is None else self._dev(claim_xy, torch.float64).reshape(N, R, 2)
        chd = None if claim_heading is None else self._dev(claim_heading, torch.float64).reshape(N, R)
        spec = {"choice": ((N, R), torch.int32), "order": ((N, R), torch.int32), "marginal": ((N, R), torch.float64),
                "utility": ((N, R), torch.float64), "claimed": ((N, 60), torch.int64), "masks": ((N, R, k, 60), torch.int64)}
        if want_rounds:
            spec["round_gain"] = ((N, R, R, k), torch.float64)
        out = self._out(out, spec)
        rounds = out.get("round_gain") if want_rounds else None
        if want_rounds and rounds is None:
            raise ValueError("assign_goals: want_rounds=True needs out['round_gain']")
        P = _lib.IgAssignParams(R, k, _lib.IG_ASSIGN_MODES[mode], 0, float(radius), float(self.range if range is None else range), float(d0),
                                self.fov)
        _lib.call(self.L, self.b.h, "cagym_ig_assign_goals", C.byref(P), _lib.ptr(mask), xy.data_ptr(), _lib.ptr(hd), dist.data_ptr(),
                  _lib.ptr(claim), _lib.ptr(cxy), _lib.ptr(chd), *[out[n].data_ptr() for n in ("choice", "order", "marginal", "utility", "claimed", "masks")],
                  _lib.ptr(rounds), self.b._stream())
        return out if want_rounds else {n: v for n, v in out.items() if n != "round_gain"}

    def route_gains(self, field, cand_cells, cand_heading=None, mask=None, exclude=None, stride=4, radius=0.5, range=None, d0=1.0, out=None,
                    want_waypoints=False):
        """cagym_ig_route_gains: ONE launch on the current stream, one workgroup per world - what a robot sees ON THE WAY to each of
        its candidate goals (ig.route_spec and ig.route_gains_spec state the rule).  field [N,R,60,60] f32: every robot's geodesic
        field with its own position as the source (geodesic(points=robot positions)["field"]); cand_cells [N,R,k,2] i32 (i, j):
        the candidates (propose_goals()' cells; a cell outside 0..59 has no route); cand_heading [N,R,k] f64 or None: with a finite
        heading the candidate's own set is the cone's, without one a robot turning on the spot, as assign_goals() has it.  mask
        [N,R] u8 or None (every robot): a robot whose byte is 0 keeps every byte of its rows, a world without a masked robot is not
        touched.  exclude [N,60] i64 or None: cells already spoken for (assign_goals()["claimed"]).  Every candidate's shortest
        path is walked back on the field by the controller's neighbour rule; every `stride` cells along it - at most 16 times - the
        cone of this object's fov is taken at the cell's centre, looking the way the robot drives; route = their union, total =
        route | the candidate's own set, each priced by mi_reward() of its cells outside `exclude` (bit for bit), utility =
        total_gain / (field[cell] + d0).  Returns the dict of device tensors it wrote: route_masks, total_masks [N,R,k,60] i64,
        route_gain, total_gain, utility [N,R,k] f64, n_path [N,R,k] i32 (the path's moves; -1: no route - gains 0, empty masks),
        n_way [N,R,k] i32, truncated [N,R,k] u8 (way-points beyond the 16th were dropped), best [N,R] i32 (the candidate with a
        route and total_gain > 0 of largest utility, ties to the smaller index; -1: none) and, with want_waypoints, way_cells
        [N,R,k,16,2] i32 and way_dir [N,R,k,16] i8 (the way-points in travel order and the move into each, an index into
        GEO_NEIGHBOURS; rows past n_way -1).  `out`: such a dict to write into again (default: new tensors)."""
        N = self.b.N
        cells = self._dev(cand_cells, torch.int32)
        if cells.dim() != 4 or cells.shape[0] != N or cells.shape[3] != 2:
            raise ValueError("route_gains: cand_cells must be [N, R, k, 2]")
        R, k = int(cells.shape[1]), int(cells.shape[2])
        field = self._dev(field, torch.float32)
        if field.numel() != N * R * 3600:
            raise ValueError("route_gains: field must be [N, R, 60, 60]")
        hd = None if cand_heading is None else self._dev(cand_heading, torch.float64).reshape(N, R, k)
        if mask is not None:
            mask = self._t(mask, torch.uint8, (N, R))
        ex = None if exclude is None else self._dev(exclude, torch.int64).reshape(N, 60)
        W = _lib.IG_ROUTE_MAX_WAYPOINTS
        spec = {"route_masks": ((N, R, k, 60), torch.int64), "total_masks": ((N, R, k, 60), torch.int64),
                "route_gain": ((N, R, k), torch.float64), "total_gain": ((N, R, k), torch.float64), "utility": ((N, R, k), torch.float64),
                "n_path": ((N, R, k), torch.int32), "n_way": ((N, R, k), torch.int32), "truncated": ((N, R, k), torch.uint8),
                "best": ((N, R), torch.int32)}
        if want_waypoints:
            spec.update(way_cells=((N, R, k, W, 2), torch.int32), way_dir=((N, R, k, W), torch.int8))
        out = self._out(out, spec)
        ways = [out.get("way_cells"), out.get("way_dir")] if want_waypoints else [None, None]
        if want_waypoints and (ways[0] is None or ways[1] is None):
            raise ValueError("route_gains: want_waypoints=True needs out['way_cells'] and out['way_dir']")
        P = _lib.IgRouteParams(R, k, int(stride), 0, float(radius), float(self.range if range is None else range), self.fov, float(d0))
        _lib.call(self.L, self.b.h, "cagym_ig_route_gains", C.byref(P), _lib.ptr(mask), field.data_ptr(), cells.data_ptr(), _lib.ptr(hd),
                  _lib.ptr(ex), *[out[n].data_ptr() for n in ("route_masks", "total_masks", "route_gain", "total_gain", "utility", "n_path",
                                                               "n_way", "truncated", "best")], _lib.ptr(ways[0]), _lib.ptr(ways[1]), self.b._stream())
        return out if want_waypoints else {n: v for n, v in out.items() if n not in ("way_cells", "way_dir")}

    def robot_credit(self, n_robots, detect_range, obs_oas, restart_mask=None, flags=0, out=None, accumulators=None, range=None):
        """cagym_ig_credit: ONE launch on the current stream, directly behind observe() (and context_window()) with the same obs_oas,
        restart_mask and flags - whose cone earned the team's gain (ig.robot_credit_spec states the rule).  Returns the dict of device
        tensors it wrote: gain [N] f64 (observe's gain, bit for bit), robot_observed [N,R,60] i64 (each robot's visible cells),
        credit [N,R,3] f64 (own: the MI sum over the robot's cells; exclusive: over the cells it alone saw; difference: gain minus
        what the gain would have been had it not looked), loo [N,R] f64 (that leave-one-out gain) and reward [N,R,3] f64 (credit, but
        0 for a world restarted in this launch, as team_reward is).  `out`: such a dict to write into again (default: new tensors); a
        key it lacks is not written.  accumulators: a dict of running, sum, last [N,R,3] f64 and episodes [N] i32 that the launch
        keeps by observe's statements per robot and kind (EPISODE_FOLD folds a restarted world's running values), or None.  R may
        exceed the worlds' teams: the rows past a team are zero (loo = gain).  OBSERVE_ONLY_RESTARTED skips every other world.  range:
        the cones' sensing range in metres (default: this object's, which is what observe() uses)."""
        N, R = self.b.N, int(n_robots)
        if out is None:
            out = self._out(None, {"gain": ((N,), torch.float64), "robot_observed": ((N, R, 60), torch.int64), "credit": ((N, R, 3), torch.float64),
                                   "loo": ((N, R), torch.float64), "reward": ((N, R, 3), torch.float64)})
        acc = accumulators or {}
        P = _lib.IgCreditParams(R, int(flags), float(detect_range), self.fov, float(self.range if range is None else range))
        _lib.call(self.L, self.b.h, "cagym_ig_credit", C.byref(P), obs_oas.data_ptr(), _lib.ptr(restart_mask),
                  *[_lib.ptr(out.get(n)) for n in ("gain", "robot_observed", "credit", "loo", "reward")],
                  *[_lib.ptr(acc.get(n)) for n in ("running", "sum", "last", "episodes")], self.b._stream())
        return out

    def heading_list(self, headings):
        """The headings a caller means: an int H is h * 2 pi / H for h = 0..H-1, computed in fp64 here; a sequence is taken as
        given (radians).  Returns a list of 1..16 floats."""
        if isinstance(headings, (int, np.integer)) and not isinstance(headings, bool):
            H = int(headings)
            if H < 1 or H > 16:
                raise ValueError("headings: H must be within 1..16, got %d" % H)
            return [h * 2.0 * math.pi / H for h in range(H)]
        hs = [float(v) for v in (headings.tolist() if hasattr(headings, "tolist") else headings)]
        if not 1 <= len(hs) <= 16:
            raise ValueError("headings: 1..16 headings, got %d" % len(hs))
        return hs

    def view_gain_headings(self, points=None, headings=8, world_mask=None, radius=0.5, range=None, out=None, want_rows=True):
        """cagym_ig_view_gain_headings: ONE launch on the current stream - what a POSE is worth: view_gain() for the sensor cone
        (this object's fov) at H headings per point.  For heading h the counted cells are exactly visible_cells() of the pose
        (x, y, headings[h]); every cell is traced once and shared by the H cones (ig.view_gain_headings_spec states the rule).
        points, world_mask, radius, range: as view_gain().  headings: an int H (h * 2 pi / H) or a sequence of 1..16 radians.
        Returns the dict of device tensors it wrote: gain_h f64 and n_visible_h i32 [N,P,H], best_heading i32 (the first index of
        the largest gain_h; -1: invalid), best_gain f64 (that value bit for bit) and valid u8 [N,P] - [N,60,60,H] and [N,60,60]
        indexed [j, i] for the map - and "headings", the list used.  want_rows=False: the two [.., H] tensors are not written
        (NULL) and not returned.  `out`: a dict of such tensors to write into again (default: new tensors; with want_rows=True it
        must hold the two rows), which itself is left as it is: the result is a new dict of the same tensors."""
        hs = self.heading_list(headings)
        H = len(hs)
        points, world_mask, shape, n_points = self._viewpoints(points, world_mask)
        spec = {"best_heading": (shape, torch.int32), "best_gain": (shape, torch.float64), "valid": (shape, torch.uint8)}
        if want_rows:
            spec.update(gain_h=(shape + (H,), torch.float64), n_visible_h=(shape + (H,), torch.int32))
        out = self._out(out, spec)
        rows = [out.get("gain_h"), out.get("n_visible_h")] if want_rows else [None, None]
        if want_rows and (rows[0] is None or rows[1] is None):
            raise ValueError("view_gain_headings: want_rows=True needs out['gain_h'] and out['n_visible_h']")
        for t in rows:
            if t is not None and t.shape[-1] != H:
                raise ValueError("view_gain_headings: out's rows hold %d headings, asked for %d" % (t.shape[-1], H))
        P = _lib.IgHeadingParams(n_points, H, 0, float(radius), float(self.range if range is None else range),
                                 self.fov, (C.c_double * 16)(*hs))
        _lib.call(self.L, self.b.h, "cagym_ig_view_gain_headings", C.byref(P), _lib.ptr(world_mask), _lib.ptr(points), _lib.ptr(rows[0]),
                  _lib.ptr(rows[1]), out["best_heading"].data_ptr(), out["best_gain"].data_ptr(), out["valid"].data_ptr(), self.b._stream())
        return dict(out, headings=hs)  # (a new dict: the caller's `out` gains no key)

    def goal_face_actions(self, params, goals, goal_heading, actions):
        """cagym_ig_goal_face_actions: directly behind goal_actions() - the rows of the robots that stand within goal_tol of an
        active goal with a finite goal_heading [N,R] f64 become (0, clip(wrap(goal_heading - heading) / dt, -w_max, w_max))."""
        _lib.call(self.L, self.b.h, "cagym_ig_goal_face_actions", C.byref(params), goals["goal_xy"].data_ptr(), goals["active"].data_ptr(),
                  goal_heading.data_ptr(), actions.data_ptr(), self.b._stream())

    def goal_face_status(self, params, goals, goal_heading, goal_facing, face_tol):
        """cagym_ig_goal_face_status: directly behind goal_status() - goal_facing [N,R] u8 = 1 for a robot within goal_tol of an
        active goal that has no finite goal heading or faces it within face_tol."""
        _lib.call(self.L, self.b.h, "cagym_ig_goal_face_status", C.byref(params), float(face_tol), goals["goal_xy"].data_ptr(),
                  goals["active"].data_ptr(), goal_heading.data_ptr(), goal_facing.data_ptr(), self.b._stream())

    def visible_cells(self, poses, world):
        poses = self._t(poses, torch.float64, (-1, 3))
        world = self._t(world, torch.int32, (-1,))
        Q = poses.shape[0]
        masks = torch.empty((Q, 60), dtype=torch.int64, device=self.b.device)
        _lib.call(self.L, self.b.h, "cagym_ig_visible_cells", poses.data_ptr(), world.data_ptr(), Q, self.fov, self.range, masks.data_ptr(),
                  self.b._stream())
        return masks

    def update_belief(self, poses, detections, n_det, n_poses=None):
        """poses [N,P,3]; detections [N,P,Dmax,2] (global positions); n_det [N,P]. Returns observed [N,60]."""
        N = self.b.N
        poses = self._t(poses, torch.float64)
        P = poses.shape[1]
        det = self._t(detections, torch.float64)
        Dmax = det.shape[2]
        nd = self._t(n_det, torch.int32, (N, P))
        npz = None if n_poses is None else self._t(n_poses, torch.int32, (N,))
        obs = torch.empty((N, 60), dtype=torch.int64, device=self.b.device)
        _lib.call(self.L, self.b.h, "cagym_ig_update_belief", poses.data_ptr(), _lib.ptr(npz), det.data_ptr(), nd.data_ptr(), P, Dmax, self.fov,
                  self.range, obs.data_ptr(), self.b._stream())
        return obs

    def mi_reward(self, masks, world, out=None):
        """out: a contiguous f64 [Q] device tensor to write into (default: a new one)."""
        masks = self._t(masks, torch.int64, (-1, 60))
        world = self._t(world, torch.int32, (-1,))
        if out is None:
            out = torch.empty((masks.shape[0],), dtype=torch.float64, device=self.b.device)
        _lib.call(self.L, self.b.h, "cagym_ig_mi_reward", masks.data_ptr(), world.data_ptr(), masks.shape[0], out.data_ptr(), self.b._stream())
        return out

    def next_pose(self, poses, actions, world, radius):
        poses = self._t(poses, torch.float64, (-1, 3))
        actions = self._t(actions, torch.float64, (-1, 2))
        world = self._t(world, torch.int32, (-1,))
        radius = self._t(radius, torch.float64, (-1,))
        Q = poses.shape[0]
        nxt = torch.empty((Q, 3), dtype=torch.float64, device=self.b.device)
        ok = torch.empty((Q,), dtype=torch.uint8, device=self.b.device)
        _lib.call(self.L, self.b.h, "cagym_ig_next_pose", poses.data_ptr(), actions.data_ptr(), world.data_ptr(), radius.data_ptr(), Q, self.xdt,
                  self.dt, nxt.data_ptr(), ok.data_ptr(), self.b._stream())
        return nxt, ok

    def greedy_plan(self, poses, coordinate=False, radius=0.5, v=GREEDY_V, w=GREEDY_W, out=None):
        """cagym_ig_greedy_plan: ig_greedy.greedy_action for the R robots of every world, poses [N,R,3] f64 (a contiguous device
        tensor is taken as it is).  One launch on the current stream, no synchronisation.  coordinate=True: a world's robots
        choose in slot order, each without the cells the earlier ones chose.  Returns the dict of device tensors it wrote:
        actions [N,R,2] f64, choice [N,R] u8 (255: no feasible candidate), mi [N,R,9] f64 (-1: infeasible), claimed [N,60] i64;
        `out`: such a dict to write into again (default: new tensors)."""
        N = self.b.N
        poses = self._dev(poses, torch.float64).reshape(N, -1, 3)
        R = poses.shape[1]
        out = self._out(out, {"actions": ((N, R, 2), torch.float64), "choice": ((N, R), torch.uint8), "mi": ((N, R, 9), torch.float64),
                              "claimed": ((N, 60), torch.int64)})
        P = GreedyParams(R, int(bool(coordinate)), self.dt, float(radius), self.fov, self.range,
                         (C.c_double * 3)(*[float(x) for x in v]), (C.c_double * 3)(*[float(x) for x in w]))
        _lib.call(self.L, self.b.h, "cagym_ig_greedy_plan", C.byref(P), poses.data_ptr(),
                  *[_lib.ptr(out.get(k)) for k in ("actions", "choice", "mi", "claimed")], self.b._stream())
        return out

    def rollouts(self, pose0, observed0, exclude, world, n_steps, radius, nsims, seed, max_steps=None,
                 want_observed=False):
        """nsims random roll-outs per query; returns (rewards [Q,nsims], actions [Q,nsims,H], final_pose) and, with
        want_observed, the cells observed along each roll-out [Q,nsims,60]."""
        pose0 = self._t(pose0, torch.float64, (-1, 3))
        Q = pose0.shape[0]
        observed0 = self._t(observed0, torch.int64, (Q, 60))
        exclude = self._t(exclude, torch.int64, (Q, 60))
        world = self._t(world, torch.int32, (Q,))
        n_steps = self._t(n_steps, torch.int32, (Q,))
        radius = self._t(radius, torch.float64, (Q,))
        H = int(max_steps if max_steps is not None else int(n_steps.max().item()) if Q else 0)
        rew = torch.empty((Q, nsims), dtype=torch.float64, device=self.b.device)
        acts = torch.full((Q, nsims, max(H, 1)), 255, dtype=torch.uint8, device=self.b.device)
        fin = torch.empty((Q, nsims, 3), dtype=torch.float64, device=self.b.device)
        obs_out = torch.empty((Q, nsims, 60), dtype=torch.int64, device=self.b.device) if want_observed else None
        _lib.call(self.L, self.b.h, "cagym_ig_rollouts", pose0.data_ptr(), observed0.data_ptr(), exclude.data_ptr(), world.data_ptr(),
                  n_steps.data_ptr(), radius.data_ptr(), Q, int(nsims), max(H, 1), self.xdt, self.dt, self.fov, self.range,
                  int(seed), rew.data_ptr(), acts.data_ptr(), fin.data_ptr(), _lib.ptr(obs_out), self.b._stream())
        return (rew, acts, fin, obs_out) if want_observed else (rew, acts, fin)


class GreedyPlanner(object):
    """The greedy policy of a handle's IG robots (BatchedCollisionAvoidanceEnv.attach_ig_greedy): plan() is one
    cagym_ig_greedy_plan launch; `choice` [N,R] u8, `mi` [N,R,9] f64, `claimed` [N,60] i64 and `actions` [N,R,2] f64 hold the
    last plan.  The policy keeps nothing across steps.  P / workspace: a minimum-size Dec-MCTS parameter block and workspace,
    there solely so that cagym_ig_episode_boundary finds publications to clear when it restarts a world."""

    def __init__(self, ig, n_robots, radius=0.5, coordinate=False):
        self.ig, self.R = ig, int(n_robots)
        self.radius, self.coordinate = float(radius), bool(coordinate)
        self.P = _lib.DmctsParams(self.R, 1, 1, 1, 1, 1, ig.xdt, 1, 0, 0, 1.0, 1.0, self.radius, ig.dt, ig.fov, ig.range, 0)
        self.workspace = torch.zeros(ig.L.cagym_dmcts_workspace_bytes(ig.b.N, C.byref(self.P)), dtype=torch.uint8, device=ig.b.device)
        self._out = None
        self.actions = self.choice = self.mi = self.claimed = None

    def reset(self, world_mask=None):
        """Nothing to forget: every plan starts from the poses and the belief alone."""

    def plan(self, poses):
        """poses [N,R,3].  Returns device tensors (actions [N,R,2], choice [N,R] u8)."""
        self._out = self.ig.greedy_plan(poses, coordinate=self.coordinate, radius=self.radius, out=self._out)
        o = self._out
        self.actions, self.choice, self.mi, self.claimed = o["actions"], o["choice"], o["mi"], o["claimed"]
        return self.actions, self.choice


def belief_window_spec(belief, mi, poses, G, rotate):
    """The belief windows of cagym_ig_observe in plain numpy - the executable statement of their layout.  belief, mi: [60, 60] f64
    odds ratios and cached cell MI of one world, indexed [j, i] (j along y); poses [R, 3] f64 (x, y, heading).  Returns
    (window [R, 3, G, G] f32, i [R, G, G], j [R, G, G] int64 source cells, qx, qy [R, G, G] f64 sample points).  Out cell (a, b):
    a forward, b left; channel 0 = odds / (odds + 1), channel 1 = cell MI, channel 2 = 1 inside the map; outside all three are 0.
    Every product and sum is a separate fp64 operation in the order written (numpy fuses nothing); with rotate the sine and cosine
    are numpy's, which may differ from the library's in the last bit."""
    belief, mi = np.asarray(belief, dtype=np.float64), np.asarray(mi, dtype=np.float64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    G, c = int(G), 0.5
    e = (np.arange(G, dtype=np.float64) - G // 2 + 0.5) * c
    ex, ey = e[None, :, None], e[None, None, :]
    px, py, th = (poses[:, k][:, None, None] for k in range(3))
    s, cs = (np.sin(th), np.cos(th)) if rotate else (np.zeros_like(th), np.ones_like(th))
    qx = px + cs * ex - s * ey
    qy = py + s * ex + cs * ey
    i = np.floor((qx + 15.0) / c).astype(np.int64)
    j = np.floor((qy + 15.0) / c).astype(np.int64)
    inside = (i >= 0) & (i < 60) & (j >= 0) & (j < 60)
    ic, jc = np.clip(i, 0, 59), np.clip(j, 0, 59)
    odds = belief[jc, ic]
    out = np.zeros((poses.shape[0], 3, G, G), dtype=np.float32)
    out[:, 0] = np.where(inside, odds / (odds + 1), 0.0).astype(np.float32)
    out[:, 1] = np.where(inside, mi[jc, ic], 0.0).astype(np.float32)
    out[:, 2] = inside.astype(np.float32)
    return out, i, j, qx, qy


def episode_log_spec(belief, target_xy, odds_found):
    """The belief columns of the IG team's episode log (cagym_ig_episode_log_update) in plain numpy - the executable statement of
    what a row holds.  belief [60, 60] f64 odds ratios of one world, indexed [j, i] (j along y); target_xy [T, 2] f64 target
    positions; odds_found: the threshold p_found / (1 - p_found), the double the library was given.  Returns a dict:
      "entropy": sum over the cells of -(P ln P + (1 - P) ln(1 - P)), P = r / (r + 1), in nats (a side whose P or 1 - P is 0 in
          fp64 contributes its limit, 0);
      "residual_mi": sum over the cells of cell_mi(r);
      "n_touched": cells whose odds differ from the prior 1.0;
      "found" [T] bool: the odds of the cell that holds the target, i = floor((x + 15) / 0.5), j likewise of y, are >= odds_found
          (False for a target outside the map); "cell" [T, 2] int64 those (i, j).
    The two sums agree with the library's up to the last bits of the logarithms and the order of the additions."""
    belief = np.asarray(belief, dtype=np.float64).reshape(60, 60)
    xy = np.asarray(target_xy, dtype=np.float64).reshape(-1, 2)
    p = belief / (belief + 1)
    q = 1 - p
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -(np.where(p > 0, p * np.log(p), 0.0) + np.where(q > 0, q * np.log(q), 0.0))
    cell = np.floor((xy + 15.0) / 0.5).astype(np.int64)
    inside = ((cell >= 0) & (cell < 60)).all(axis=1)
    c = np.clip(cell, 0, 59)
    found = inside & (belief[c[:, 1], c[:, 0]] >= float(odds_found))
    # (math.fsum: the correctly rounded sum, whatever the order)
    return {"entropy": math.fsum(h.ravel()), "residual_mi": math.fsum(cell_mi(belief).ravel()), "n_touched": int((belief != 1.0).sum()),
            "found": found, "cell": cell}


def context_window_spec(edf, observed, poses, agents_xy, agents_value, G, rotate, clear_max):
    """The context windows of cagym_ig_context_window in plain numpy - the executable statement of their three channels, on the
    sample points and source cells of belief_window_spec.  edf: [300, 300] f64 distance field in metres of the world's current
    scenario slot (InfoGain.edf()[slot]), indexed [row = y, column = x]; observed: [60] integer words of the world (bit i of word
    j <=> belief cell (i, j)) or None; poses [R, 3] f64 (x, y, heading); agents_xy: per robot k the [n_k, 2] f64 positions of the
    world's active non-static agents other than robot k itself, agents_value: per robot the matching [n_k] values (1.0 a
    teammate, 0.5 anything else).  Returns (window [R, 3, G, G] f32, a_s, b_s: per robot the int64 window cells of its agents,
    fx, fy: their fp64 offsets in its frame).  Channel 0 = min(edf, clear_max) / clear_max inside the map, 0 outside; channel 1 =
    the largest value among the agents whose cell (a_s, b_s) = floor(f * 2) + G / 2 is the out cell, not masked by the map;
    channel 2 = 1 where the source cell is inside and in observed.  Every product and sum is a separate fp64 operation in the
    order written; with rotate the sine and cosine are numpy's, which may differ from the library's in the last bit."""
    edf = np.asarray(edf, dtype=np.float64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    R, G, cap = poses.shape[0], int(G), float(clear_max)
    _, i, j, qx, qy = belief_window_spec(np.ones((60, 60)), np.zeros((60, 60)), poses, G, rotate)
    inside = (i >= 0) & (i < 60) & (j >= 0) & (j < 60)
    ic, jc = np.clip(i, 0, 59), np.clip(j, 0, 59)
    # edfMap.get_edf_value_from_pose: column floor((x + 15) / 0.1), row floor((y + 15) / 0.1); inside the map both lie in 0..299
    xi = np.clip(np.floor((qx + 15.0) / 0.1), 0, 299).astype(np.int64)
    yi = np.clip(np.floor((qy + 15.0) / 0.1), 0, 299).astype(np.int64)
    out = np.zeros((R, 3, G, G), dtype=np.float32)
    out[:, 0] = np.where(inside, np.minimum(edf[yi, xi], cap) / cap, 0.0).astype(np.float32)
    if observed is not None:
        words = np.asarray(observed).astype(np.int64).view(np.uint64).reshape(60)
        bit = (words[jc] >> ic.astype(np.uint64)) & np.uint64(1)
        out[:, 2] = (inside & (bit == 1)).astype(np.float32)
    a_s, b_s, fxs, fys = [], [], [], []
    for k in range(R):
        xy = np.asarray(agents_xy[k], dtype=np.float64).reshape(-1, 2)
        val = np.asarray(agents_value[k], dtype=np.float32).reshape(-1)
        px, py, th = poses[k]
        s, cs = (np.sin(th), np.cos(th)) if rotate else (0.0, 1.0)
        dx, dy = xy[:, 0] - px, xy[:, 1] - py
        fx = cs * dx + s * dy
        fy = cs * dy - s * dx
        a = np.floor(fx * 2.0).astype(np.int64) + G // 2
        b = np.floor(fy * 2.0).astype(np.int64) + G // 2
        for n in np.flatnonzero((a >= 0) & (a < G) & (b >= 0) & (b < G)):
            out[k, 1, a[n], b[n]] = max(out[k, 1, a[n], b[n]], val[n])
        a_s.append(a), b_s.append(b), fxs.append(fx), fys.append(fy)
    return out, a_s, b_s, fxs, fys


GEO_ORTHO, GEO_DIAG = np.float32(0.5), np.float32(0.5 * np.sqrt(2.0))  # the move costs of the geodesic field
# the controller's candidates in order: E, N, W, S, NE, NW, SW, SE as (di, dj), E = +x, N = +y
GEO_NEIGHBOURS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))


_ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
       9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
       4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)
_PI, _PI_LO = 3.1415926535897931160e+00, 1.2246467991473531772e-16


def _atan_pos(x):
    """fdlibm's atan (s_atan.c, public domain constants) for x >= 0, every product, sum and quotient a separate fp64 operation"""
    if x >= 73786976294838206464.0:  # 2^66
        return _ATANHI[3] + _ATANLO[3]
    if x < 0.4375:
        if x < 1.862645149230957e-09:  # 2^-29
            return x
        k = -1
    elif x < 1.1875:
        if x < 0.6875:
            k, x = 0, (2.0 * x - 1.0) / (2.0 + x)
        else:
            k, x = 1, (x - 1.0) / (x + 1.0)
    elif x < 2.4375:
        k, x = 2, (x - 1.5) / (1.0 + 1.5 * x)
    else:
        k, x = 3, -1.0 / x
    z = x * x
    w = z * z
    s1 = z * (_AT[0] + w * (_AT[2] + w * (_AT[4] + w * (_AT[6] + w * (_AT[8] + w * _AT[10])))))
    s2 = w * (_AT[1] + w * (_AT[3] + w * (_AT[5] + w * (_AT[7] + w * _AT[9]))))
    if k < 0:
        return x - x * (s1 + s2)
    return _ATANHI[k] - ((x * (s1 + s2) - _ATANLO[k]) - x)


def atan2_spec(y, x):
    """The controller's atan2 for finite operands: fdlibm's (e_atan2.c / s_atan.c), restated with nothing but fp64 sums, products
    and quotients in a fixed order, so that cagym_ig_goal_actions (igg_atan2 in csrc/cagym_ig_geodesic.h, compiled without
    contraction) and this function return the same double bit for bit; it is within an ulp of the C library's.  The heading error
    of an aligned robot is a difference of two nearly equal angles: two atan2 that differ in their last bit would give turn rates
    that differ by their whole size there."""
    y, x = float(y), float(x)
    m = (1 if math.copysign(1.0, y) < 0 else 0) + (2 if math.copysign(1.0, x) < 0 else 0)
    if y == 0.0:
        return y if m < 2 else (_PI if m == 2 else -_PI)
    if x == 0.0:
        return -(_ATANHI[3] + _ATANLO[3]) if m & 1 else _ATANHI[3] + _ATANLO[3]
    z = _atan_pos(abs(y / x))
    if m == 0:
        return z
    if m == 1:
        return -z
    if m == 2:
        return _PI - (z - _PI_LO)
    return (z - _PI_LO) - _PI


def geodesic_spec(edf, point, radius):
    """The field of cagym_ig_geodesic in plain numpy with heapq - its bit-exact specification.  edf: [300, 300] f64 distance field
    in metres of the world's current scenario slot (InfoGain.edf()[slot]), indexed [row = y, column = x]; point: (x, y) in world
    metres; radius: the robot's.  Returns (field [60, 60] f32 indexed [j, i], free [60, 60] bool, source_cell (si, sj) or None).
    free[j, i] <=> edf[5 j + 2, 5 i + 2] > radius + 0.1 - the raster cell in the middle of the belief cell - or (i, j) is the
    source cell si = floor((x + 15) / 0.5), sj likewise of y.  A point that is not finite or whose cell lies outside 0..59 has no
    source cell: the field is all +inf.  Otherwise field[sj, si] = 0 and a Dijkstra search relaxes v from u with
    np.float32(field[u] + cost), cost GEO_ORTHO for an orthogonal and GEO_DIAG for a diagonal move, v free, and for a diagonal both
    orthogonal cells it passes between free.  fp32 addition is monotone and the costs are positive, so this is the unique fixed
    point of field[v] = min over allowed u of fl32(field[u] + cost), whatever order a relaxation reaches it in."""
    edf = np.asarray(edf, dtype=np.float64)
    x, y = float(point[0]), float(point[1])
    field = np.full((60, 60), np.inf, dtype=np.float32)
    free = edf[2::5, 2::5] > float(radius) + 0.1
    if not (np.isfinite(x) and np.isfinite(y)):
        return field, free, None
    si, sj = int(math.floor((x + 15.0) / 0.5)), int(math.floor((y + 15.0) / 0.5))
    if not (0 <= si < 60 and 0 <= sj < 60):
        return field, free, None
    free = free.copy()
    free[sj, si] = True
    field[sj, si] = 0.0
    heap = [(0.0, sj, si)]
    while heap:
        d, j, i = heapq.heappop(heap)
        if d > field[j, i]:
            continue
        for k, (di, dj) in enumerate(GEO_NEIGHBOURS):
            ni, nj = i + di, j + dj
            if not (0 <= ni < 60 and 0 <= nj < 60 and free[nj, ni]):
                continue
            if k >= 4 and not (free[j, ni] and free[nj, i]):
                continue
            nd = np.float32(field[j, i] + (GEO_ORTHO if k < 4 else GEO_DIAG))
            if nd < field[nj, ni]:
                field[nj, ni] = nd
                heapq.heappush(heap, (float(nd), nj, ni))
    return field, free, (si, sj)


def goal_action_spec(field, pose, goal_xy, dt, v_max, w_max, align_tol, goal_tol):
    """The controller of cagym_ig_goal_actions for one robot with an active goal, in plain numpy fp64 - its specification.  field
    [60, 60] f32 indexed [j, i] (geodesic_spec's), pose (x, y, heading), goal_xy the goal point.  Returns (v, omega, chosen_cell,
    reached): the fp64 action (the library stores (float)v, (float)omega), the cell (i, j) aimed at - a neighbour, or the own
    cell when the aim is the goal point itself, None when the action is (0, 0) - and dist <= goal_tol.
      own cell (ci, cj) = floor((x + 15) / 0.5), floor((y + 15) / 0.5); outside the map: (0, 0).  dist = sqrt(dx dx + dy dy) to the
      goal; reached: (0, 0).  Own cell == the goal's cell: aim at the goal point.  Else the neighbour with the smallest key
      np.float32(field[n] + cost) among GEO_NEIGHBOURS in order (the first of equal keys), finite field values only, a diagonal
      while the own value is finite only with both orthogonal neighbours finite; none: (0, 0); aim at its centre.
      err = wrap(atan2_spec(ay - y, ax - x) - heading), wrap(a) = (a + pi) % (2 pi) - pi; omega = clip(err / dt, -w_max, w_max);
      rem = err - omega dt; v = 0 when |rem| > align_tol, else v_max, or min(v_max, dist / dt) when the aim is the goal point."""
    field = np.asarray(field, dtype=np.float32).reshape(60, 60)
    x, y, th = (float(v) for v in pose)
    gx, gy = float(goal_xy[0]), float(goal_xy[1])
    ci, cj = int(math.floor((x + 15.0) / 0.5)), int(math.floor((y + 15.0) / 0.5))
    dx, dy = gx - x, gy - y
    dist = math.sqrt(dx * dx + dy * dy)
    reached = dist <= goal_tol
    if not (0 <= ci < 60 and 0 <= cj < 60) or reached:
        return 0.0, 0.0, None, reached
    at = lambda i, j: field[j, i] if (0 <= i < 60 and 0 <= j < 60) else np.float32(np.inf)
    to_goal = (ci, cj) == (int(math.floor((gx + 15.0) / 0.5)), int(math.floor((gy + 15.0) / 0.5)))
    if to_goal:
        ax, ay, cell = gx, gy, (ci, cj)
    else:
        own, best, cell = np.isfinite(field[cj, ci]), np.float32(np.inf), None
        for k, (di, dj) in enumerate(GEO_NEIGHBOURS):
            val = at(ci + di, cj + dj)
            if not np.isfinite(val):
                continue
            if k >= 4 and own and not (np.isfinite(at(ci + di, cj)) and np.isfinite(at(ci, cj + dj))):
                continue
            key = np.float32(val + (GEO_ORTHO if k < 4 else GEO_DIAG))
            if key < best:
                best, cell = key, (ci + di, cj + dj)
        if cell is None:
            return 0.0, 0.0, None, reached
        ax, ay = cell[0] * 0.5 - 15.0 + 0.25, cell[1] * 0.5 - 15.0 + 0.25
    err = (atan2_spec(ay - y, ax - x) - th + np.pi) % (2 * np.pi) - np.pi
    omega = min(max(err / dt, -w_max), w_max)
    rem = err - omega * dt
    v = 0.0
    if not abs(rem) > align_tol:
        v = min(v_max, dist / dt) if to_goal else float(v_max)
    return float(v), float(omega), cell, reached


def edf_at_spec(edf, x, y):
    """edfMap.get_edf_value_from_pose on arrays: edf [300, 300] f64 indexed [row = y, column = x]; the column is the floor of the
    true quotient (x + 15) / 0.1, the row likewise of y; a negative index wraps once, as numpy's does; anything else outside, and
    a coordinate that is not finite, reads 0.0."""
    edf = np.asarray(edf, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor((x + 15.0) / 0.1), np.floor((y + 15.0) / 0.1)
        ok = (np.abs(fx) < 1e6) & (np.abs(fy) < 1e6)  # (False for NaN and for +-inf)
    xi = np.where(ok, fx, -1000.0).astype(np.int64)
    yi = np.where(ok, fy, -1000.0).astype(np.int64)
    xi, yi = np.where(xi < 0, xi + 300, xi), np.where(yi < 0, yi + 300, yi)
    ok = ok & (xi >= 0) & (xi < 300) & (yi >= 0) & (yi < 300)
    return np.where(ok, edf[np.clip(yi, 0, 299), np.clip(xi, 0, 299)], 0.0)


def check_visibility_spec(edf, point, cx, cy):
    """edfMap.checkVisibility(point, (cx[n], cy[n])) for arrays of goals, the statements of ig_check_visibility in csrc/cagym_ig.h:
    dist = sqrt(dx dx + dy dy), u = 0.05 / dist; while u < 1: sample (1 - u) p + u c, fail when edf_at_spec there is < 0.001, else
    u += edf / dist.  A goal at dist = 0 is visible (u is infinite, the loop is skipped).  The goals are lanes that step in lockstep
    under a mask; a lane still inside the loop after 100000 trips fails.  Every product and sum is a separate fp64 operation.
    point: (x, y), two numbers - or two arrays of cx's shape, a viewpoint per goal.  Returns a bool array of cx's shape."""
    cx, cy = np.asarray(cx, dtype=np.float64), np.asarray(cy, dtype=np.float64)
    shape = cx.shape
    cx, cy = cx.ravel(), cy.ravel()
    px = np.broadcast_to(np.asarray(point[0], dtype=np.float64), shape).ravel()
    py = np.broadcast_to(np.asarray(point[1], dtype=np.float64), shape).ravel()
    dx, dy = cx - px, cy - py
    dist = np.sqrt(dx * dx + dy * dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = 0.05 / dist
        live = u < 1
        for _ in range(100000):
            if not live.any():
                break
            n = np.flatnonzero(live)
            un = u[n]
            md = edf_at_spec(edf, (1 - un) * px[n] + un * cx[n], (1 - un) * py[n] + un * cy[n])
            hit = md < 0.001
            u[n] = np.where(hit, np.nan, un + md / dist[n])  # (NaN: failed, and out of the loop)
            live[n] = u[n] < 1
        return (~(u < 1) & ~np.isnan(u)).reshape(shape)


def view_gain_spec(edf, mi, point, radius, range=5.0):
    """The view gain of cagym_ig_view_gain for one point of one world, in numpy - its specification.  edf: [300, 300] f64 distance
    field in metres of the world's current scenario slot (InfoGain.edf()[slot]); mi: [60, 60] f64 cell MI, cell_mi(belief), indexed
    [j, i]; point (x, y) in world metres; radius: the robot's; range: the sensing range.  Returns (gain, n_visible, valid, visible
    [60, 60] bool, in_range [60, 60] bool).
      valid <=> x, y finite, the cell floor((p + 15) / 0.5) in 0..59 on both axes and edf_at_spec(x, y) > radius + 0.1, the planners'
        feasibility test at the point itself; an invalid point has gain 0, n_visible 0 and empty masks.
      candidates: i in max(0, cell(x - range)) .. min(59, cell(x + range)), j likewise; centre c = i * 0.5 - 15 + 0.25;
      in_range <=> dx dx + dy dy < range range, dx = cx - x; visible <=> in_range and check_visibility_spec(point, c): a robot
        turning on the spot, no field of view, no heading.
      gain = math.fsum of mi over the visible cells (the library adds them in a fixed order: equal up to the rounding of ~300 sums)."""
    mi = np.asarray(mi, dtype=np.float64).reshape(60, 60)
    x, y, rng = float(point[0]), float(point[1]), float(range)
    vis, inr = np.zeros((60, 60), dtype=bool), np.zeros((60, 60), dtype=bool)
    if not (math.isfinite(x) and math.isfinite(y)):
        return 0.0, 0, False, vis, inr
    cell = lambda v: int(min(max(math.floor((v + 15.0) / 0.5), -10 ** 6), 10 ** 6))
    if not (0 <= cell(x) < 60 and 0 <= cell(y) < 60) or not float(edf_at_spec(edf, x, y)) > float(radius) + 0.1:
        return 0.0, 0, False, vis, inr
    i = np.arange(max(0, cell(x - rng)), min(59, cell(x + rng)) + 1)
    j = np.arange(max(0, cell(y - rng)), min(59, cell(y + rng)) + 1)
    jj, ii = np.meshgrid(j, i, indexing="ij")
    cx, cy = ii * 0.5 - 15.0 + 0.25, jj * 0.5 - 15.0 + 0.25
    dx, dy = cx - x, cy - y
    near = dx * dx + dy * dy < rng * rng
    inr[jj[near], ii[near]] = True
    seen = check_visibility_spec(edf, (x, y), cx[near], cy[near])
    vis[jj[near][seen], ii[near][seen]] = True
    return math.fsum(mi[vis]), int(vis.sum()), True, vis, inr


def view_gain_headings_spec(edf, mi, point, headings, radius, fov, range):
    """The heading-resolved view gains of cagym_ig_view_gain_headings for one point of one world, in numpy - their specification.
    edf, mi, point, radius: as view_gain_spec; headings: a sequence of H radians; fov: the cone's full opening angle; range: the
    sensing range.  Returns a dict: gain_h [H] f64, n_visible_h [H] i32, best_heading, best_gain, valid and masks [H, 60, 60]
    bool indexed [h, j, i].
      valid: view_gain_spec's rule; an invalid point has zero rows, best_heading -1 and best_gain 0.
      For heading phi the counted cells are targetMap.getVisibleCells of the pose (x, y, phi), written out:
        box: with the four points p, p + range (cos, sin)(phi), p + range (cos, sin)(phi + fov), p + range (cos, sin)(phi - fov),
          each coordinate clamped to +-15, and cell(v) = floor((v + 15) / 0.5): i in max(0, min cell) .. min(60, max cell) - 1, the
          upper bound EXCLUSIVE, j likewise;
        cone: r0 = c dx + s dy, r1 = -s dx + c dy with dx = centre - x; inside <=> sqrt(r0 r0 + r1 r1) < range and
          |atan2(r1 + 0.0, r0 + 0.0)| < fov / 2;
        visible <=> check_visibility_spec(point, centre) - which does not depend on the heading: every cell is traced once.
      gain_h = math.fsum of mi over the heading's cells, n_visible_h their number; best_heading = the first index of the largest
      gain_h.  (Sine and cosine are the C library's here and ig_sincos on the device: a cell exactly on a cone edge or on the range
      circle may be decided differently; headings h 2 pi / 8 or / 16 with range 4.9 or 2.3 keep every cell of a cell-centre
      viewpoint at least 4e-3 rad and 2e-2 m off.)"""
    mi = np.asarray(mi, dtype=np.float64).reshape(60, 60)
    hs = [float(h) for h in headings]
    H = len(hs)
    x, y, rng, fov = float(point[0]), float(point[1]), float(range), float(fov)
    out = {"gain_h": np.zeros(H), "n_visible_h": np.zeros(H, dtype=np.int32), "best_heading": -1, "best_gain": 0.0, "valid": False,
           "masks": np.zeros((H, 60, 60), dtype=bool)}
    if not (math.isfinite(x) and math.isfinite(y)):
        return out
    cell = lambda v: int(min(max(math.floor((v + 15.0) / 0.5), -10 ** 6), 10 ** 6))
    clamp = lambda v: max(min(v, 15.0), -15.0)
    if not (0 <= cell(x) < 60 and 0 <= cell(y) < 60) or not float(edf_at_spec(edf, x, y)) > float(radius) + 0.1:
        return out
    out["valid"] = True
    inside = np.zeros((H, 60, 60), dtype=bool)
    for h, phi in enumerate(hs):
        s, c = math.sin(phi), math.cos(phi)
        sl, cl, sr, cr = math.sin(phi + fov), math.cos(phi + fov), math.sin(phi - fov), math.cos(phi - fov)
        cxs = [cell(x), cell(clamp(x + rng * c)), cell(clamp(x + rng * cl)), cell(clamp(x + rng * cr))]
        cys = [cell(y), cell(clamp(y + rng * s)), cell(clamp(y + rng * sl)), cell(clamp(y + rng * sr))]
        xs, xe, ys, ye = max(min(cxs), 0), min(max(cxs), 60), max(min(cys), 0), min(max(cys), 60)
        if xe <= xs or ye <= ys:
            continue
        jj, ii = np.meshgrid(np.arange(ys, ye), np.arange(xs, xe), indexing="ij")
        dx, dy = (ii * 0.5 - 15.0 + 0.25) - x, (jj * 0.5 - 15.0 + 0.25) - y
        r0, r1 = c * dx + s * dy, -s * dx + c * dy
        ok = (np.sqrt(r0 * r0 + r1 * r1) < rng) & (np.abs(np.arctan2(r1 + 0.0, r0 + 0.0)) < fov / 2)
        inside[h, jj[ok], ii[ok]] = True
    jall, iall = np.nonzero(inside.any(axis=0))
    seen = np.zeros((60, 60), dtype=bool)
    if len(jall):
        seen[jall, iall] = check_visibility_spec(edf, (x, y), iall * 0.5 - 15.0 + 0.25, jall * 0.5 - 15.0 + 0.25)
    out["masks"] = inside & seen[None]
    for h in np.arange(H):
        out["gain_h"][h] = math.fsum(mi[out["masks"][h]])
        out["n_visible_h"][h] = int(out["masks"][h].sum())
    out["best_heading"] = int(np.argmax(out["gain_h"]))  # (the first of equal maxima)
    out["best_gain"] = float(out["gain_h"][out["best_heading"]])
    return out


def goal_face_spec(pose, goal_xy, goal_heading, dt, w_max, goal_tol, face_tol):
    """cagym_ig_goal_face_actions and cagym_ig_goal_face_status for one robot with an ACTIVE goal, in plain fp64 - their bit-exact
    specification.  pose (x, y, heading), goal_xy the goal point, goal_heading in radians or NaN: none.  Returns (row, reached,
    facing): row is None when the robot's row keeps its bytes, else (0.0, omega) in fp64 (the library stores (float)omega).
      reached = sqrt(dx dx + dy dy) <= goal_tol, the test on which goal_action_spec stops the robot;
      err = wrap(goal_heading - heading), wrap(a) = (a + pi) % (2 pi) - pi, goal_action_spec's; the short way across +-pi;
      row = (0, clip(err / dt, -w_max, w_max)) when reached and the goal heading is finite;
      facing = reached and (the goal heading is not finite or |err| <= face_tol)."""
    x, y, th = (float(v) for v in pose)
    dx, dy = float(goal_xy[0]) - x, float(goal_xy[1]) - y
    reached = math.sqrt(dx * dx + dy * dy) <= goal_tol
    gh = float(goal_heading)
    if not math.isfinite(gh):
        return None, reached, reached
    err = (gh - th + np.pi) % (2 * np.pi) - np.pi
    if not reached:
        return None, False, False
    return (0.0, min(max(err / dt, -w_max), w_max)), True, abs(err) <= face_tol


def cells_to_words(cells):
    """bool [.., 60, 60] indexed [j, i] -> the library's visibility words [.., 60] uint64 (bit i of word j <=> cell (i, j))"""
    cells = np.asarray(cells, dtype=bool)
    return (cells.astype(np.uint64) << np.arange(60, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def words_to_cells(words):
    """the library's visibility words [.., 60] (uint64, or the int64 a tensor holds) -> bool [.., 60, 60] indexed [j, i]"""
    words = np.ascontiguousarray(words)
    words = words.view(np.uint64) if words.dtype == np.int64 else words.astype(np.uint64)
    return ((words[..., None] >> np.arange(60, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def assign_goals_spec(masks, claimed0, distance, valid, reward, mode, d0, open_robots):
    """The team assignment of cagym_ig_assign_goals for one world, in numpy - its specification, given the candidates' cell sets.
    masks [R, k, 60, 60] bool indexed [j, i]: every candidate's cell set (view_gain_spec(...)[3] for a candidate without a heading,
    view_gain_headings_spec(...)["masks"][h] for one with; empty for an invalid point); claimed0 [60, 60] bool: the seed, the union of
    the cell sets of the teammates under way; distance [R, k] f32; valid [R, k]: the points that pass view_gain_spec's rule;
    reward(cells [60, 60] bool) -> float: the mutual information of a cell set (InfoGain.mi_reward on the device, oracle.mi_reward
    on a belief); mode "slot" / "best" (or 0 / 1); d0 > 0; open_robots: the robots that choose now, a sequence of slots or a bool [R].
      marginal gain of a candidate = reward(cells & ~claimed); eligible <=> valid, distance finite, marginal > 0;
      utility = marginal / ((double)distance + d0), one fp64 addition and one fp64 division.
      "slot": round t is the turn of the t-th open robot in slot order; it takes its eligible candidate of largest utility, of equal
        utilities the smaller index, and claimed |= cells; none eligible: choice -1, nothing claimed.
      "best": up to len(open_robots) rounds; each takes the eligible (robot, candidate) of largest utility among the open robots not
        yet assigned - ties to the smaller slot, then the smaller index - and claimed |= cells; the rounds stop when nothing is eligible.
    Returns a dict: choice, order [R] int32 (-1: unassigned, and every robot that is not open), marginal, utility [R] f64 (0 likewise),
    claimed [60, 60] bool the final union, round_gain [R, R, k] f64 indexed [round, robot, candidate]: the marginal gain of every
    valid candidate with a finite distance priced in that round ("slot": the robot whose turn it is, "best": every robot still
    open), NaN everywhere else."""
    masks = np.asarray(masks, dtype=bool)
    R, k = masks.shape[:2]
    dist = np.asarray(distance, dtype=np.float32).reshape(R, k)
    ok = np.asarray(valid).reshape(R, k).astype(bool) & np.isfinite(dist)
    mode = {"slot": 0, "best": 1, 0: 0, 1: 1}[mode]
    d0 = float(d0)
    o = np.asarray(open_robots)
    opened = [int(r) for r in (np.flatnonzero(o) if o.dtype == bool else o.ravel())]
    if sorted(set(opened)) != opened or any(r < 0 or r >= R for r in opened):
        raise ValueError("assign_goals_spec: open_robots must be distinct slots in ascending order")
    claimed = np.array(claimed0, dtype=bool).reshape(60, 60).copy()
    out = {"choice": np.full(R, -1, dtype=np.int32), "order": np.full(R, -1, dtype=np.int32), "marginal": np.zeros(R), "utility": np.zeros(R),
           "round_gain": np.full((R, R, k), np.nan)}
    left = list(opened)
    for t in range(len(opened)):
        pricing = [opened[t]] if mode == 0 else list(left)
        best = None  # (utility, robot, candidate, marginal)
        for r in pricing:
            for c in range(k):
                if not ok[r, c]:
                    continue
                m = float(reward(masks[r, c] & ~claimed))
                out["round_gain"][t, r, c] = m
                if not m > 0:
                    continue
                with np.errstate(divide="ignore", over="ignore"):
                    u = float(np.float64(m) / (np.float64(dist[r, c]) + np.float64(d0)))
                if best is None or u > best[0]:  # (in ascending (slot, index): the strict test keeps the first of equal utilities)
                    best = (u, r, c, m)
        if best is None:
            if mode == 1:
                break
            continue
        u, r, c, m = best
        out["choice"][r], out["order"][r], out["marginal"][r], out["utility"][r] = c, t, m, u
        claimed |= masks[r, c]
        left.remove(r)
    out["claimed"] = claimed
    return out


ROUTE_MAX_WAYPOINTS = _lib.IG_ROUTE_MAX_WAYPOINTS
ROUTE_WALK_CAP = 3600  # moves per walk
ROUTE_HEADING_M = (0, 2, 4, -2, 1, 3, -3, -1)  # a move in GEO_NEIGHBOURS order heads ROUTE_HEADING_M[d] * (pi / 4)


def route_heading(d):
    """The heading of a move in direction d of GEO_NEIGHBOURS: the double m * (pi / 4), one fp64 product."""
    return ROUTE_HEADING_M[int(d)] * (math.pi / 4)


def route_path_spec(field, cell):
    """The walk of cagym_ig_route_gains from `cell` (i, j) down `field` [60, 60] f32 indexed [j, i] - a robot's geodesic field with
    its own cell as the source - in plain numpy: the list of (i, j, move) in WALK order, the candidate's cell first, move the index in
    GEO_NEIGHBOURS of the step taken out of the cell (None in the last cell, whose field is 0), or None when there is no route.
      No route: the cell outside 0..59, or its field not finite.  From a cell whose value is not 0 the next cell is the neighbour
      goal_action_spec chooses: GEO_NEIGHBOURS in order, finite values only, a diagonal only with both orthogonal neighbours finite,
      key np.float32(field[n] + cost), the first of equal smallest keys.  No such neighbour, a neighbour whose value is not below the
      cell's own, or more than 3600 moves: no route."""
    field = np.asarray(field, dtype=np.float32).reshape(60, 60)
    ci, cj = int(cell[0]), int(cell[1])
    if not (0 <= ci < 60 and 0 <= cj < 60) or not np.isfinite(field[cj, ci]):
        return None
    at = lambda i, j: field[j, i] if (0 <= i < 60 and 0 <= j < 60) else np.float32(np.inf)
    path = []
    for s in range(ROUTE_WALK_CAP + 1):
        cur = field[cj, ci]
        if cur == 0:
            path.append((ci, cj, None))
            return path
        if s == ROUTE_WALK_CAP:
            break
        best, pick = np.float32(np.inf), None
        for k, (di, dj) in enumerate(GEO_NEIGHBOURS):
            val = at(ci + di, cj + dj)
            if not np.isfinite(val):
                continue
            if k >= 4 and not (np.isfinite(at(ci + di, cj)) and np.isfinite(at(ci, cj + dj))):
                continue
            key = np.float32(val + (GEO_ORTHO if k < 4 else GEO_DIAG))
            if key < best:
                best, pick = key, k
        if pick is None or not at(ci + GEO_NEIGHBOURS[pick][0], cj + GEO_NEIGHBOURS[pick][1]) < cur:
            return None
        path.append((ci, cj, pick))
        ci, cj = ci + GEO_NEIGHBOURS[pick][0], cj + GEO_NEIGHBOURS[pick][1]
    return None


def route_spec(field, cell, stride):
    """The route of cagym_ig_route_gains for one candidate cell (i, j) of one robot, in numpy - its specification.  field [60, 60]
    f32 indexed [j, i]: the robot's geodesic field with its own cell as the source (geodesic_spec's); stride >= 1.  Returns (n_path,
    way_cells [n_way, 2] i32 (i, j), way_dir [n_way] i8, truncated).
      route_path_spec walks q_0 = cell .. q_n, the cell whose field is 0; no route: (-1, no way-points, False).
      Travel order: p_t = q_{n-t}.  The move INTO p_t, p_{t-1} -> p_t, is the opposite of the walk's move out of it: way_dir is its
      index in GEO_NEIGHBOURS (the walk's index ^ 2), its heading route_heading(way_dir).
      Way-points: t = stride, 2 stride, .. with t < n and t <= 16 stride, in travel order; truncated <=> a t < n beyond 16 stride
      was dropped, that is, ceil(n / stride) - 1 > 16."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("route_spec: stride must be at least 1")
    none = (-1, np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int8), False)
    path = route_path_spec(field, cell)
    if path is None:
        return none
    n = len(path) - 1
    cells, dirs, truncated = [], [], False
    for t in range(stride, n, stride):
        if t > ROUTE_MAX_WAYPOINTS * stride:
            truncated = True
            break
        i, j, move = path[n - t]
        cells.append((i, j))
        dirs.append(move ^ 2)
    return n, np.array(cells, dtype=np.int32).reshape(-1, 2), np.array(dirs, dtype=np.int8), truncated


def route_gains_spec(route_masks, terminal_masks, distance, has_route, reward, d0, exclude=None):
    """The prices and the choice of cagym_ig_route_gains for ONE robot, in numpy - their specification, given the cell sets.
    route_masks [k, 60, 60] bool indexed [j, i]: the union of every candidate's way-point sets (visible_cells of the poses
    route_spec names); terminal_masks [k, 60, 60] bool: every candidate's own set by assign_goals_spec's rule (empty for an invalid
    point); distance [k] f32: the robot's field at the candidate's cell; has_route [k]; reward(cells [60, 60] bool) -> float, as
    assign_goals_spec takes it; d0 > 0; exclude [60, 60] bool or None: cells already spoken for.
      A candidate without a route has empty masks, gains 0 and utility 0.  Else total = route | terminal, route_gain = reward(route
      & ~exclude), total_gain = reward(total & ~exclude), utility = total_gain / ((double)distance + d0): one fp64 addition, one fp64
      division.  best: the candidate with a route and total_gain > 0 of largest utility, of equal utilities the smaller index; -1
      when there is none.
    Returns a dict: route_masks, total_masks [k, 60, 60] bool (emptied where there is no route), route_gain, total_gain, utility
    [k] f64 and best."""
    route = np.array(route_masks, dtype=bool).reshape(-1, 60, 60)
    k = route.shape[0]
    term = np.asarray(terminal_masks, dtype=bool).reshape(k, 60, 60)
    dist = np.asarray(distance, dtype=np.float32).reshape(k)
    ok = np.asarray(has_route).reshape(k).astype(bool)
    ex = np.zeros((60, 60), dtype=bool) if exclude is None else np.asarray(exclude, dtype=bool).reshape(60, 60)
    d0 = float(d0)
    route[~ok] = False
    total = route | term
    total[~ok] = False
    out = {"route_masks": route, "total_masks": total, "route_gain": np.zeros(k), "total_gain": np.zeros(k), "utility": np.zeros(k), "best": -1}
    best = None
    for c in range(k):
        if not ok[c]:
            continue
        out["route_gain"][c] = float(reward(route[c] & ~ex))
        out["total_gain"][c] = tg = float(reward(total[c] & ~ex))
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            out["utility"][c] = u = float(np.float64(tg) / (np.float64(dist[c]) + np.float64(d0)))
        if tg > 0 and (best is None or u > best):  # (ascending: the strict test keeps the first of equal utilities)
            best, out["best"] = u, c
    return out


def propose_goals_spec(gain, valid, field, k, min_sep, d0):
    """The proposals of cagym_ig_propose_goals for one (world, robot), in numpy - their bit-exact specification.  gain [60, 60] f64
    and valid [60, 60]: the world's view-gain map at the cell centres, indexed [j, i]; field [60, 60] f32: the robot's geodesic field
    with its own position as the source; k in 1..16, min_sep > 0 and d0 > 0 in metres.
      A cell is eligible iff valid != 0, gain > 0 and field is finite; its utility is gain / ((double)field + d0): one fp64 addition,
      one fp64 division.  Up to k rounds: take the eligible, unsuppressed cell of largest utility, of equal utilities the smallest flat
      index j * 60 + i; then suppress every cell with (double)(di di + dj dj) * 0.25 < min_sep min_sep, the chosen cell included.
      Stop when nothing is left.
    Returns a dict: cells [k, 2] i32 (i, j), xy [k, 2] f64 the cell centres, utility, gain [k] f64, distance [k] f32, n_found; rows
    past n_found hold cells = -1, xy = NaN, utility = gain = 0 and distance = +inf."""
    gain = np.asarray(gain, dtype=np.float64).reshape(60, 60)
    valid = np.asarray(valid).reshape(60, 60)
    field = np.asarray(field, dtype=np.float32).reshape(60, 60)
    k, sep2, d0 = int(k), float(min_sep) * float(min_sep), float(d0)
    if not (1 <= k <= 16 and float(min_sep) > 0 and d0 > 0):
        raise ValueError("propose_goals_spec: k must be 1..16, min_sep and d0 positive")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        eligible = (valid != 0) & (gain > 0) & np.isfinite(field)
        util = np.where(eligible, gain / (field.astype(np.float64) + d0), -1.0)  # (an eligible cell's utility is >= 0)
    out = {"cells": np.full((k, 2), -1, dtype=np.int32), "xy": np.full((k, 2), np.nan), "utility": np.zeros(k), "gain": np.zeros(k),
           "distance": np.full(k, np.inf, dtype=np.float32), "n_found": 0}
    jj, ii = np.meshgrid(np.arange(60), np.arange(60), indexing="ij")
    for n in range(k):
        q = int(np.argmax(util))  # (the first of equal maxima: the smallest flat index)
        j, i = divmod(q, 60)
        if not util[j, i] >= 0:
            break
        out["cells"][n] = (i, j)
        out["xy"][n] = (i * 0.5 - 15.0 + 0.25, j * 0.5 - 15.0 + 0.25)
        out["utility"][n], out["gain"][n], out["distance"][n] = util[j, i], gain[j, i], field[j, i]
        out["n_found"] = n + 1
        util[((ii - i) ** 2 + (jj - j) ** 2).astype(np.float64) * 0.25 < sep2] = -1.0
    return out


def block_sum_spec(values, member):
    """The MI sums of the library in their own order (ig_reward_block of csrc/cagym_ig.h): values, member [60, 60] indexed [j, i];
    thread q % 256 adds the values of its member cells q = 60 j + i in ascending order, then the 256 partial sums go through the
    halving tree.  Sequential fp64 additions: the library's bits, given its values.  An empty set sums to +0.0."""
    v = np.where(np.asarray(member, dtype=bool).ravel(), np.asarray(values, dtype=np.float64).ravel(), 0.0)  # (x + 0.0 is x for x >= +0.0)
    v = np.concatenate([v, np.zeros(15 * 256 - 3600)]).reshape(15, 256)
    acc = np.zeros(256)
    for row in v:
        acc = acc + row
    h = 128
    while h > 0:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def robot_credit_spec(belief, mi, masks, poses, oas_rows, det_range=5.0):
    """The per-robot credit of cagym_ig_credit for ONE world, in numpy - its specification, given the robots' cell sets.  belief, mi
    [60, 60] f64 indexed [j, i]: the world's odds ratios and MI cache as the observe launch left them; masks [R, 60] u64 (or i64),
    robot r's visible cells V_r (bit i of word j <=> cell (i, j); an absent robot: zeros); poses [R, 3] f64 (x, y, heading);
    oas_rows [R, K, 10] f32, the robots' OtherAgentsStates rows (an absent robot: zeros).  Returns a dict:
      "detections": a list of R arrays [n_r, 2] f64 - row + pose for the rows with row[9] == 1 and sqrt(r0^2 + r1^2) <= det_range,
          the test in fp32 as the table is, in row order;
      "factor" [R, 60, 60] f64: f_r = 1.5 where a detection of robot r lies within sqrt(0.5) * 0.5 + 0.01 of the cell's centre,
          both rotated into the robot's frame (the belief update's test), else 0.66 - over the whole grid, not only V_r;
      "gain": the sum of mi over U, the union of the V_r;
      "own" [R]: over V_r; "exclusive" [R]: over V_r & ~U_-r, U_-r the union of V_s over s != r;
      "loo" [R]: over q in U_-r of (q in V_r ? cell_mi(belief[q] / f_r(q)) : mi[q]) - the gain had robot r not looked;
      "difference" [R] = gain - loo.
    Every sum runs in block_sum_spec's order.  own, exclusive and gain are the library's bits given its mi; loo agrees up to the last
    bits of the logarithms and of numpy's sine and cosine (the library's rotation also fuses one product into its sum)."""
    belief, mi = np.asarray(belief, dtype=np.float64).reshape(60, 60), np.asarray(mi, dtype=np.float64).reshape(60, 60)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    R = poses.shape[0]
    words = np.asarray(masks).reshape(R, 60).astype(np.uint64)
    V = ((words[:, :, None] >> np.arange(60, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)  # [R, j, i]
    rows = np.asarray(oas_rows, dtype=np.float32).reshape(R, -1, 10)
    centre = np.arange(60, dtype=np.float64) * 0.5 - 15.0 + 0.25
    cx, cy = centre[None, :], centre[:, None]
    thr = np.sqrt(0.5) * 0.5 + 0.01
    dets, factor = [], np.full((R, 60, 60), 0.66)
    for r in range(R):
        px, py, th = poses[r]
        r0, r1 = rows[r, :, 0], rows[r, :, 1]
        hit = (rows[r, :, 9] == np.float32(1.0)) & (np.sqrt(r0 * r0 + r1 * r1) <= np.float32(det_range))  # fp32 throughout
        d = np.stack([r0[hit].astype(np.float64) + px, r1[hit].astype(np.float64) + py], axis=1)
        dets.append(d)
        c, s = np.cos(th), np.sin(th)
        q0, q1 = c * (cx - px) + s * (cy - py), -s * (cx - px) + c * (cy - py)
        for tx, ty in d:
            t0, t1 = c * (tx - px) + s * (ty - py), -s * (tx - px) + c * (ty - py)
            factor[r][np.sqrt((t0 - q0) ** 2 + (t1 - q1) ** 2) < thr] = 1.5
    U = V.any(axis=0)
    out = {"detections": dets, "factor": factor, "gain": block_sum_spec(mi, U), "own": np.zeros(R), "exclusive": np.zeros(R),
           "loo": np.zeros(R), "difference": np.zeros(R)}
    for r in range(R):
        others = np.delete(V, r, axis=0).any(axis=0) if R > 1 else np.zeros((60, 60), dtype=bool)
        out["own"][r] = block_sum_spec(mi, V[r])
        out["exclusive"][r] = block_sum_spec(mi, V[r] & ~others)
        out["loo"][r] = block_sum_spec(np.where(V[r], cell_mi(belief / factor[r]), mi), others)
        out["difference"][r] = out["gain"] - out["loo"][r]
    return out


def cell_mi(r):
    """ig_cell_mi of csrc/cagym_ig.h (targetMap's per-cell mutual information of an odds ratio r) in numpy: what the library's MI
    cache holds, up to the last bits of the logarithm."""
    r = np.asarray(r, dtype=np.float64)
    rO, rE, fn, fp = 1.5, 0.66, 0.1, 0.05
    p = r / (r + 1)
    f_p = np.log((r + 1) / (r + (1 / rO))) - np.log(rO) / (r * rO + 1)
    f_n = np.log((r + 1) / (r + (1 / rE))) - np.log(rE) / (r * rE + 1)
    return (p * (1 - fn) + (1 - p) * fp) * f_p + (p * fn + (1 - p) * (1 - fp)) * f_n


def find_targets_in_obs(other_agents_states, detect_range=5.0):
    """Detector emulation of ig_mcts.find_targets_in_obs (ig_mcts.py:135-152) on an OAS table [.., K, 10]:
    a target is a row of type 1 (Static) within range; the FOV test of the reference compares radians with
    degrees and is therefore always true.  Returns (mask [.., K], global offsets rows[.., 0:2])."""
    oas = other_agents_states
    r = torch.sqrt(oas[..., 0] ** 2 + oas[..., 1] ** 2)
    return (oas[..., 9] == 1.0) & (r <= detect_range), oas[..., 0:2]


class InfoGainBackend(object):
    """numpy-in / numpy-out adapter of InfoGain for dmcts.DecMCTSPlanner (host tree, device primitives)."""

    def __init__(self, ig):
        self.ig = ig

    def next_pose(self, poses, prim_idx, world, radius):
        acts = PRIMITIVES[np.asarray(prim_idx)]
        nxt, ok = self.ig.next_pose(poses, acts, world, radius)
        torch.cuda.synchronize(self.ig.b.device)
        return nxt.cpu().numpy(), ok.cpu().numpy().astype(bool)

    def visible_cells(self, poses, world):
        if len(poses) == 0:
            return np.zeros((0, 60), dtype=np.uint64)
        m = self.ig.visible_cells(poses, world)
        return m.cpu().numpy().view(np.uint64)

    def rollouts(self, pose0, observed0, exclude, world, n_steps, radius, nsims, seed):
        H = int(max(1, np.max(n_steps)))
        rew, acts, fin, obs = self.ig.rollouts(pose0, np.ascontiguousarray(observed0).view(np.int64),
                                               np.ascontiguousarray(exclude).view(np.int64), world, n_steps, radius,
                                               nsims, seed, max_steps=H, want_observed=True)
        return rew.cpu().numpy(), acts.cpu().numpy(), obs.cpu().numpy().view(np.uint64)
