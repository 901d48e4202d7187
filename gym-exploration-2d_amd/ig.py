"""Information-gain planner primitives on device (cagym_ig_* of include/cagym.h).

Counterparts of the reference's targetMap / edfMap objects and of the Dec-MCTS roll-out primitives
(information_models/targetMap.py, information_models/edfMap.py, policies/ig_mcts.py:117-253,
policies/pydecmcts/DecMCTS.py:233-271).  Visibility sets are [.., 60] int64 tensors (bit i of word j
<=> belief cell (i, j)); the tree bookkeeping (UCT select / expand / back-propagate) stays with the caller.
"""
import ctypes as C
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
        N, dev = self.b.N, self.b.device
        if not (torch.is_tensor(poses) and poses.is_cuda and poses.dtype == torch.float64 and poses.is_contiguous()):
            poses = self._t(poses, torch.float64)
        poses = poses.reshape(N, -1, 3)
        R = poses.shape[1]
        if out is None:
            out = {"actions": torch.empty((N, R, 2), dtype=torch.float64, device=dev),
                  "choice": torch.empty((N, R), dtype=torch.uint8, device=dev),
                  "mi": torch.empty((N, R, 9), dtype=torch.float64, device=dev),
                  "claimed": torch.empty((N, 60), dtype=torch.int64, device=dev)}
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
