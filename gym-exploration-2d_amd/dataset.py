"""Trajectory-dataset export (second half).

The reference's dataset creator (experiments/src/run_trajectory_dataset_creator.py:53-109) walks each agent's
`global_state_history` (agent.py:217-232: rows [t, px, py, gx, gy, radius, pref_speed, vx, vy, speed, heading,
a0, a1]) and writes, per agent, a list of records.  Row k is written by Agent.take_action during the agent's
(k+1)-th step AFTER the move and BEFORE `t += dt` (agent.py:176-186, 198-201): position / velocity / heading after
k+1 moves next to the time stamp k * dt; the initial state is never logged, a done agent logs nothing more, and
main() keeps rows [:step_num] (:164-167).  Pinned by tests/golden/adapters.npz (add_traj run on a reference episode).

    {'time', 'pedestrian_goal_position', 'coop_coef', 'other_agents_pos', 'other_agents_vel',
     'pedestrian_state': {'position', 'velocity'}}

This module records the same history for N worlds at once from the batched env (device tensors, one host copy
at the end) and formats it with the same schema.  Files are written with pickle, like the reference's `.pkl`.
"""
import pickle

import numpy as np
import torch

HISTORY_COLUMNS = ("t", "pos_x", "pos_y", "goal_x", "goal_y", "radius", "pref_speed", "vel_x", "vel_y", "speed", "heading")


def record_episode(env, max_steps=1000, actions=None):
    """Step every world of `env` (freshly reset) until every agent is done (no auto-reset) or max_steps.
    Returns dict of numpy arrays: history [T, N, M, 13] in the reference's row convention (row k = state after step k+1,
    time stamp of before it), step_num [N, M] (the rows of agent i are history[:step_num, w, i]), n_agents [N],
    coop [N, M]."""
    rows = []

    def snap():
        st = env.state()
        cols = [st[k] for k in HISTORY_COLUMNS] + [st["action"][..., 0].double(), st["action"][..., 1].double()]
        return torch.stack([c.double() for c in cols], dim=-1)

    prev = snap()
    for _ in range(max_steps):
        env.step(actions)
        cur = snap()
        row = cur.clone()
        row[..., 0] = prev[..., 0]  # Agent._update_state_history runs before `self.t += dt`
        rows.append(row)
        prev = cur
        st = env.state()
        active = torch.arange(env.M, device=env.device)[None, :] < st["n_agents"][:, None]
        if bool((((st["status"] & 8) != 0) | ~active).all()):  # CAGYM_FLAG_DONE for every agent of every world
            break
    torch.cuda.synchronize(env.device)
    st = env.state()
    sc = env.scenarios()
    S = env.S
    sidx = ((torch.arange(env.N, device=env.device) + st["episode"].long() * env.N) % S).long()
    return {"history": torch.stack(rows).cpu().numpy(), "step_num": st["step_num"].cpu().numpy(),
            "n_agents": st["n_agents"].cpu().numpy(), "coop": sc["coop"][sidx].cpu().numpy()}


def to_reference_records(rec, world, dt=0.1, last_time=0.0):
    """add_traj (run_trajectory_dataset_creator.py:53-109) for one world: list (one per agent) of lists of records.
    Returns (trajectories, last_time for the next episode)."""
    H, steps = rec["history"][:, world], rec["step_num"][world]
    n = int(rec["n_agents"][world])
    trajs = []
    d = None
    for i in range(n):
        traj = []
        max_ts = int(steps[i])  # global_state_history[:step_num]: one row per step the agent took
        for t in range(max_ts):
            opos, ovel = [], []
            for j in range(n):
                if j == i:
                    continue
                lj = int(steps[j])
                if t >= lj:  # the other agent finished earlier: last position, zero velocity (:73-75)
                    opos.append((H[lj - 1, j, 1], H[lj - 1, j, 2]))
                    ovel.append((0, 0))
                else:
                    opos.append((H[t, j, 1], H[t, j, 2]))
                    ovel.append((H[t, j, 7], H[t, j, 8]))
            d = {"time": np.round(last_time + t * 0.1, decimals=1),
                 "pedestrian_goal_position": (H[t, i, 3], H[t, i, 4]),
                 "coop_coef": float(rec["coop"][world, i]),
                 "other_agents_pos": opos, "other_agents_vel": ovel,
                 "pedestrian_state": {"position": (H[t, i, 1], H[t, i, 2]), "velocity": (H[t, i, 7], H[t, i, 8])}}
            traj.append(d)
        trajs.append(traj)
    return trajs, (d["time"] + 1.0 if d is not None else last_time)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def ring_slices(planes, world, episode):
    """The slices of (world, episode) still in a trajectory ring, oldest first (pure array code; numpy arrays or tensors).
    planes: "rows" [L, 13, N, M] (or [L, 13, N * M]), "moved" [L, N, M], "episode" [L, N], "last" [L, N], "head" (slices ever
    written; slice i lives at index i % L) - env.trajectory_views(), or copies of it.
    Returns (history [T, M, 13] in slice order, moved [T, M] bool, complete).  An agent's first row carries t_before == 0.0
    (Agent.t starts at 0), which is how the start of an episode is recognised: `complete` means that row and the slice whose
    `last` byte is set are both present.  Where reset(world_mask) restarted the same episode index, the newest run is returned."""
    episode_plane, last = _host(planes["episode"]), _host(planes["last"])
    L, N = episode_plane.shape
    moved = _host(planes["moved"]).reshape(L, N, -1)
    M = moved.shape[2]
    rows = _host(planes["rows"]).reshape(L, 13, N, M)
    head = int(np.asarray(_host(planes["head"])).reshape(-1)[0])
    n = min(head, L)
    order = np.arange(head - n, head) % L
    sel = order[episode_plane[order, world] == episode]
    H = np.transpose(rows[sel][:, :, world, :], (0, 2, 1))  # [T, M, 13]
    mv = moved[sel, world] != 0
    starts = np.nonzero((mv & (H[:, :, 0] == 0.0)).any(axis=1))[0]
    if starts.size:
        sel, H, mv = sel[starts[-1]:], H[starts[-1]:], mv[starts[-1]:]
    complete = bool(starts.size and sel.size and last[sel[-1], world] != 0)
    return np.ascontiguousarray(H), mv, complete


def ring_episode(planes, world, episode, n_agents, coop):
    """One episode out of a trajectory ring as the `rec` dict to_reference_records takes, for ONE world (pass world=0 there):
    history [T, 1, M, 13] with every agent's rows packed to the front (the rows of agent i are history[:step_num[0, i], 0, i],
    the history[:step_num] rule of record_episode), step_num [1, M] = the rows present, n_agents [1], coop [1, M]; "complete"
    rides along (ring_slices).  n_agents: the episode's agent count, coop: its [M] cooperation coefficients - the pool row of
    slot (world + episode * N) % S on a fixed pool, the episode log's n_agents under streaming."""
    H, mv, complete = ring_slices(planes, world, episode)
    T, M = mv.shape
    hist = np.zeros((T, 1, M, 13), dtype=np.float64)
    steps = mv.sum(axis=0).astype(np.int32)
    for i in range(M):
        hist[:steps[i], 0, i] = H[mv[:, i], i]
    return {"history": hist, "step_num": steps[None, :], "n_agents": np.asarray([int(n_agents)], dtype=np.int32),
            "coop": np.asarray(coop, dtype=np.float64).reshape(1, M), "complete": complete}


def export_ring(env, path, episodes, n_agents=None, coop=None, complete_only=True):
    """Write the reference-schema trajectory pickle of the listed (world, episode) pairs - e.g. the world / episode columns of
    env.episode_log() - out of the env's trajectory ring (attach_trajectory_ring).  One synchronisation and one host copy of
    the ring.  n_agents / coop: per listed episode ([K] / [K, M]); default: the pool rows of slot (world + episode * N) % S,
    which describe the episode only on a pool that is not streamed (a streamed slot is regenerated once its episode ends:
    pass the log's n_agents and the sampler's coefficients there).  complete_only: skip episodes whose first row or last slice
    is no longer in the ring.  Returns the number of agent trajectories written."""
    planes = {k: _host(v) for k, v in env.trajectory_views().items()}
    if int(planes["desync"][0]):
        raise RuntimeError("export_ring: the trajectory ring is out of step with the env (desync %d)" % int(planes["desync"][0]))
    episodes = [(int(w), int(e)) for w, e in episodes]
    if (n_agents is None or coop is None) and getattr(env, "_streaming", False):
        raise ValueError("export_ring on a streaming env needs n_agents and coop: the pool slot of a finished episode has been regenerated")
    sc = {k: _host(v) for k, v in env.scenarios().items()} if (n_agents is None or coop is None) else None
    out, last = [], 0.0
    for k, (w, e) in enumerate(episodes):
        slot = (w + e * env.N) % env.S
        rec = ring_episode(planes, w, e, sc["n_agents"][slot] if n_agents is None else n_agents[k],
                           sc["coop"][slot] if coop is None else coop[k])
        if complete_only and not rec["complete"]:
            continue
        trajs, last = to_reference_records(rec, 0, last_time=last)
        out.extend(trajs)
    with open(path, "wb") as f:
        pickle.dump(out, f)
    return len(out)


def export(env, path, max_steps=1000):
    """Record one episode of every world and write the reference-schema trajectories of all of them to `path`."""
    rec = record_episode(env, max_steps)
    out, last = [], 0.0
    for w in range(env.N):
        trajs, last = to_reference_records(rec, w, last_time=last)
        out.extend(trajs)
    with open(path, "wb") as f:
        pickle.dump(out, f)
    return len(out)
