"""dataset.ring_episode / ring_slices, the array code that reads an episode out of a trajectory ring, on numpy planes (no GPU):
against a straightforward loop on a synthetic timeline with a wrapped ring, episodes cut by the wrap or still running, and
n_agents < M; and, with the planes filled from the reference episode of tests/golden/adapters.npz, through to_reference_records
against the add_traj records pinned there."""
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "adapters.npz")
ds = importlib.import_module("gym-exploration-2d_amd.dataset")


def _timeline(N, M, L, steps, seed):
    """Planes after `steps` slices of a made-up run, and the slices themselves: per world a sequence of episodes of random length;
    in an episode agent i < n_agents moves in its first k_i steps (1 <= k_i <= length, agent 0 all of them)."""
    rng = np.random.default_rng(seed)
    planes = {"rows": np.full((L, 13, N, M), np.nan), "moved": np.zeros((L, N, M), dtype=np.uint8),
              "episode": np.full((L, N), -1, dtype=np.int32), "last": np.zeros((L, N), dtype=np.uint8), "head": np.asarray([steps])}
    slices = []  # per step: (episode [N], last [N], moved [N, M], rows [N, M, 13])
    ep = np.zeros(N, dtype=np.int64)
    k = np.zeros(N, dtype=np.int64)           # steps into the episode
    length = rng.integers(1, 9, N)
    n_agents = {}
    moves = {}

    def start(w):
        n = int(rng.integers(2, M + 1)) if w else 2
        n_agents[(w, int(ep[w]))] = n
        m = np.zeros(M, dtype=np.int64)
        m[:n] = rng.integers(1, length[w] + 1, n)
        m[0] = length[w]
        moves[(w, int(ep[w]))] = m
    for w in range(N):
        start(w)
    for i in range(steps):
        mv = np.zeros((N, M), dtype=bool)
        rows = rng.random((N, M, 13)) + 1.0
        last = np.zeros(N, dtype=np.uint8)
        for w in range(N):
            mv[w] = k[w] < moves[(w, int(ep[w]))]
            rows[w, :, 0] = 0.1 * k[w]  # t_before: 0.0 in an agent's first row
            last[w] = k[w] + 1 == length[w]
        slices.append((ep.copy(), last, mv, rows))
        s = i % L
        planes["episode"][s], planes["last"][s], planes["moved"][s] = ep, last, mv
        planes["rows"][s] = np.where(mv[None], np.transpose(rows, (2, 0, 1)), planes["rows"][s])  # unmoved agents' rows stay stale
        for w in range(N):
            k[w] += 1
            if last[w]:
                ep[w], k[w], length[w] = ep[w] + 1, 0, rng.integers(1, 9)
                start(w)
    return planes, slices, n_agents


def _loop(slices, lo, w, e, M):
    """the rows of every agent of (w, e) among slices[lo:], one by one; whether the first and the last slice are among them"""
    per_agent = [[] for _ in range(M)]
    first = ended = False
    for i in range(lo, len(slices)):
        ep, last, mv, rows = slices[i]
        if ep[w] != e:
            continue
        first |= bool((rows[w, mv[w], 0] == 0.0).any())
        ended |= bool(last[w])
        for a in range(M):
            if mv[w, a]:
                per_agent[a].append(rows[w, a])
    return per_agent, first and ended


def test_ring_episode_equals_a_straightforward_loop():
    N, M, L, steps = 3, 5, 16, 45
    planes, slices, n_agents = _timeline(N, M, L, steps, seed=4)
    lo = steps - L
    seen = {"complete": 0, "cut": 0, "running": 0, "short": 0}
    for (w, e), n in n_agents.items():
        want, complete = _loop(slices, lo, w, e, M)
        rec = ds.ring_episode(planes, w, e, n, np.linspace(0.1, 0.5, M))
        assert rec["complete"] == complete, (w, e)
        assert rec["history"].shape[1:] == (1, M, 13) and rec["step_num"].shape == (1, M) and rec["n_agents"].tolist() == [n]
        assert rec["coop"].shape == (1, M)
        for a in range(M):
            assert rec["step_num"][0, a] == len(want[a]), (w, e, a)
            if want[a]:
                assert np.array_equal(rec["history"][:len(want[a]), 0, a], np.asarray(want[a])), (w, e, a)
        assert not rec["step_num"][0, n:].any()  # slots at or above n_agents never move
        H, mv, c2 = ds.ring_slices(planes, w, e)
        assert c2 == complete and H.shape == (mv.shape[0], M, 13) and np.array_equal(mv.sum(axis=0), rec["step_num"][0])
        rows_in = sum(len(x) for x in want)
        seen["complete"] += complete
        seen["cut"] += (not complete) and rows_in > 0 and any(s[0][w] == e and s[1][w] for s in slices[lo:])
        seen["running"] += (not complete) and rows_in > 0 and not any(s[0][w] == e and s[1][w] for s in slices)
        seen["short"] += n < M and rows_in > 0
    assert all(seen.values()), seen  # whole episodes, ones whose start the wrap took, ones still running, ones with n_agents < M


def test_a_ring_that_never_wrapped_and_an_empty_one():
    planes, slices, n_agents = _timeline(2, 3, 64, 20, seed=1)
    want, complete = _loop(slices, 0, 1, 0, 3)
    rec = ds.ring_episode(planes, 1, 0, n_agents[(1, 0)], np.ones(3))
    assert rec["complete"] == complete and complete
    assert [int(x) for x in rec["step_num"][0]] == [len(x) for x in want]
    none = ds.ring_episode(planes, 0, 999, 2, np.ones(3))
    assert none["history"].shape == (0, 1, 3, 13) and not none["complete"] and not none["step_num"].any()


def test_ring_episode_feeds_the_reference_schema():
    """the fixture's episode (4 agents, 10 slots, 331 steps) written into ring planes slice by slice, read back with ring_episode
    and formatted by to_reference_records: the add_traj records the reference produced"""
    z = np.load(GOLD)
    n, M, L = int(z["n_traj"]), 10, 400
    steps = z["step_num"].astype(np.int64)
    T = int(steps.max())
    planes = {"rows": np.zeros((L, 13, 1, M)), "moved": np.zeros((L, 1, M), dtype=np.uint8), "episode": np.full((L, 1), 7, dtype=np.int32),
              "last": np.zeros((L, 1), dtype=np.uint8), "head": T}
    for i in range(n):
        k = int(steps[i])
        planes["moved"][:k, 0, i] = 1
        planes["rows"][:k, 0, 0, i] = 0.1 * np.arange(k)
        planes["rows"][:k, 1:3, 0, i] = z["traj%d__pos" % i]
        planes["rows"][:k, 3:5, 0, i] = z["traj%d__goal" % i]
        planes["rows"][:k, 7:9, 0, i] = z["traj%d__vel" % i]
    planes["last"][T - 1, 0] = 1
    coop = np.ones(M)
    coop[:n] = z["coop"]
    rec = ds.ring_episode(planes, 0, 7, n, coop)
    assert rec["complete"] and np.array_equal(rec["step_num"][0, :n], steps) and not rec["step_num"][0, n:].any()
    trajs, last = ds.to_reference_records(rec, world=0, last_time=5.0)
    assert len(trajs) == n and abs(last - float(z["last_time"])) < 1e-12
    for i, tr in enumerate(trajs):
        g = lambda k: z["traj%d__%s" % (i, k)]
        assert len(tr) == len(g("time"))
        assert np.array_equal(np.array([d["time"] for d in tr]), g("time"))
        assert np.array_equal(np.array([d["pedestrian_goal_position"] for d in tr]), g("goal"))
        assert np.array_equal(np.array([d["coop_coef"] for d in tr]), g("coop"))
        assert np.array_equal(np.array([d["pedestrian_state"]["position"] for d in tr]), g("pos"))
        assert np.array_equal(np.array([d["pedestrian_state"]["velocity"] for d in tr]), g("vel"))
        assert np.array_equal(np.array([d["other_agents_pos"] for d in tr], dtype=np.float64), g("other_pos"))
        assert np.array_equal(np.array([d["other_agents_vel"] for d in tr], dtype=np.float64), g("other_vel"))
