"""The append-only episode log on the device (csrc/cagym_episode_log.h, include/cagym.h: cagym_episode_log_*) against its numpy twin
(tests/episode_log_twin.py, held to the reference's fixtures by tests/test_episode_log_twin.py) fed the SAME device outputs.  Every
integer, flag and key column, t, ret, head and the running arrays must be equal (doubles compared as their bits), extra_t within
1e-12: the twin's sqrt(dx^2 + dy^2) against the kernels' norm2, the bound tests/test_episode_records.py uses for this column.

Hand-built pools of six kinds of scenario (a Static agent 0 runs into its time limit of 3 (d - 0.75) / pref_speed seconds):
  0  every agent in a lane of its own, agent 0 1.5 m from its goal and the others nearer: all at goal after about 8 steps;
  1  a NonCooperative head-on pair 1.2 m apart (radius 0.5): a collision in the first step;
  2  a Static agent 0 with its goal 1.2 m away: a time-out after 14 steps;
  3, 4, 5  the same with the goal 1.75 / 2.25 / 4.75 m away: 30, 45 and 120 steps.  Episodes of at most 15 steps cannot give a
     launch of 33 slices a world that finishes nothing or exactly one episode, which every multi-slice launch here must contain.
Which slot gets which kind is drawn per (N, S) and checked on the host against the worlds' slot schedule (w + e N) % S with these
nominal lengths (_kinds): every multi-slice launch of SEQUENCE then holds worlds that finish 0, 1 and >= 2 episodes, for S % N != 0
too, where a world wanders over the slots.  The device run asserts it again on what really happened.
"""
import ctypes
import importlib

import numpy as np
import pytest

from episode_log_twin import EpisodeLogTwin
from episode_records_twin import straight_line_time

pytestmark = pytest.mark.gpu
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
DT = 0.1
RING_EXACT = ("key", "world", "episode", "slice", "steps", "outcome", "n_agents", "n_obst", "flags", "t", "ret")
RUNNING = ("t_run", "ret_run", "steps_run", "atgoal_run", "cursor")


def _B():
    return importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


WINDOWS = ((4, 8), (9, 41), (44, 48), (49, 81))  # the multi-slice launches of SEQUENCE, first and last step (1-based)
_KINDS = {}


def _finishes(kinds, N, S, lengths):
    """[window, world] episodes finished, with episode length lengths[kind]"""
    out = np.zeros((len(WINDOWS), N), dtype=np.int64)
    for w in range(N):
        t = e = 0
        while t <= WINDOWS[-1][1]:
            t += lengths[kinds[(w + e * N) % S]]
            e += 1
            for i, (a, b) in enumerate(WINDOWS):
                out[i, w] += a <= t <= b
    return out


def _kinds(N, S):
    """kind per slot: the first draw whose schedule gives every window worlds finishing 0, 1 and >= 2 episodes, whether the
    time-outs take their nominal step count or one more (the goal episodes take 8 steps)"""
    if (N, S) not in _KINDS:
        # (few worlds wandering over few slots need more of the long kinds to leave one of them idle in every window)
        p = [0.15, 0.45, 0.15, 0.1, 0.1, 0.05] if N >= 12 or S % N == 0 else [0.1, 0.4, 0.1, 0.1, 0.1, 0.2]
        for seed in range(2000):
            kinds = np.random.default_rng(seed).choice(6, size=S, p=p)
            ok = len(set(kinds[:N].tolist())) == 6 or N < 12
            for late in (0, 1):
                c = _finishes(kinds, N, S, [8, 1, 14 + late, 30 + late, 45 + late, 120 + late])
                ok = ok and all((c[i] == 0).any() and (c[i] == 1).any() and (c[i] >= 2).any() for i in range(len(WINDOWS)))
            if ok:
                _KINDS[(N, S)] = kinds
                break
        else:
            raise RuntimeError("no kind layout for N %d S %d" % (N, S))
    return _KINDS[(N, S)]


def _pool(S, M, seed, N=None):
    rng = np.random.default_rng(seed)
    kinds = np.arange(S) % 6 if N is None else _kinds(N, S)
    a6 = np.zeros((S, M, 6))
    pol = np.full((S, M), scen.POLICY_NONCOOP, dtype=np.int32)
    n_agents = rng.integers(2, M + 1, S).astype(np.int32)
    n_agents[0], n_agents[S - 1] = M, 2
    for s in range(S):
        kind = int(kinds[s])
        for j in range(M):  # lanes 3 m apart, alternating direction; the others travel 1.0 .. 1.3 m
            d = (1.0 + 0.1 * ((s + j) % 4)) * (1 if j % 2 == 0 else -1)
            a6[s, j] = [0.0, 3.0 * j, d, 3.0 * j, 1.0, 0.5]
        a6[s, 0, 2] = 1.5 + 0.01 * (s % 5)
        if kind == 1:
            a6[s, 0] = [0.0, 0.0, 1.5, 0.0, 1.0, 0.5]
            a6[s, 1] = [1.2, 0.0, -0.3, 0.0, 1.0, 0.5]
        elif kind >= 2:
            a6[s, 0, 2] = {2: 1.2, 3: 1.75, 4: 2.25, 5: 4.75}[kind]
            pol[s, 0] = scen.POLICY_STATIC
    return a6, pol, n_agents


def _env(N, M, S, pool, capacity, mode="agent0"):
    a6, pol, n_agents = pool
    env = _B()(N, M, n_scenarios=S, game_over_mode=mode)
    env.set_scenarios(a6, pol, scen.DYN_UNICYCLE, n_agents=n_agents, coop=np.full((S, M), 0.5))
    env.reset()
    if capacity is not None:
        env.attach_episode_log(capacity)
    return env


def _twin(env, pool, capacity, n_obst=None, episode0=None):
    return EpisodeLogTwin(env.N, env.M, pool[0], pool[2], DT, capacity, n_obst=n_obst, episode0=episode0)


def _launch(env, how, T, out=None):
    """One feeding call: T = 1 through step(), or rollout(T).  Returns its outputs as [T, ...] host arrays."""
    import torch
    if how == "step":
        assert T == 1
        env.step(auto_reset=True)
        F, R, G = env.flags[None], env.reward[None], env.game_over[None]
    else:
        tr = env.rollout(T, auto_reset=True, out=env.alloc_rollout(T, obs=False) if out is None else out)
        F, R, G = tr["flags"], tr["reward"], tr["game_over"]
    torch.cuda.synchronize()
    return F.cpu().numpy(), R.cpu().numpy(), G.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _compare(env, tw, what):
    v = {k: t.cpu().numpy() for k, t in env.episode_log_views().items()}
    assert int(v["desync"][0]) == 0, what
    print(what, "head", int(v["head"][0]), "twin", tw.head)
    assert int(v["head"][0]) == tw.head, what
    ring = dict(tw.ring)
    v["key"] = v["key"].astype(np.int64) & 0xFFFFFFFF
    for k in RING_EXACT:
        assert np.array_equal(_bits(v[k]), _bits(ring[k])), (what, k, v[k], ring[k])
    e = np.abs(v["extra_t"] - ring["extra_t"]).max()
    print(what, "extra_t max |diff| %.3e" % e)
    assert e <= 1e-12, (what, e)
    run = tw.running()
    for k in RUNNING:
        if v[k].dtype == np.float64:
            assert np.array_equal(_bits(v[k]), _bits(run[k])), (what, k)
        else:
            assert np.array_equal(v[k].astype(np.int64), run[k].astype(np.int64)), (what, k)
    dead = np.arange(env.M)[None, :] >= v["n_agents"][:, None]
    for k in ("t", "extra_t", "flags"):
        assert not v[k][dead].any(), (what, k)  # slots at or above n_agents hold zeros


SEQUENCE = (("step", 1), ("step", 1), ("step", 1), ("rollout", 5), ("rollout", 33), ("rollout", 1), ("step", 1), ("rollout", 5),
            ("rollout", 33))  # launches over steps 1, 2, 3, 4-8, 9-41, 42, 43, 44-48, 49-81


# (N, M): 21 / 16 / 6 / 3 worlds per wave, tail lanes in the last wave of every one; S = N, 3 N and 2 N + 5 (S % N != 0: worlds share
# scenarios); L = 8 wraps and meets the n > L rule in the 33-slice launches, L = 4096 never wraps
@pytest.mark.parametrize("L", [8, 4096])
@pytest.mark.parametrize("S_of", ["N", "3N", "2N+5"])
@pytest.mark.parametrize("N,M", [(6, 3), (64, 4), (70, 10), (33, 20)])
def test_device_equals_twin(N, M, S_of, L):
    S = {"N": N, "3N": 3 * N, "2N+5": 2 * N + 5}[S_of]
    pool = _pool(S, M, seed=N + M + S, N=N)
    env = _env(N, M, S, pool, L)
    tw = _twin(env, pool, L)
    over = False
    for i, (how, T) in enumerate(SEQUENCE):
        F, R, G = _launch(env, how, T)
        n = tw.update(F, R, G)
        over |= n > L
        if T > 1:  # worlds that finish nothing, one episode and several in the same launch
            per_world = G.astype(bool).sum(axis=0)
            assert (per_world == 0).any() and (per_world == 1).any() and (per_world >= 2).any(), (how, T, per_world)
        _compare(env, tw, "N%d M%d S%d L%d call %d (%s %d)" % (N, M, S, L, i, how, T))
    if L == 4096:  # (the same run as its L = 8 twin case, with every row kept)
        seen = np.bitwise_or.reduce(tw.rows()["outcome"])
        assert seen & 1 and seen & 2 and seen & 4, tw.rows()["outcome"]  # a collision, an all-at-goal and a neither ending were logged
    assert over == (L == 8)
    # the same rows through the host API: append order, the newest K, sorted
    import torch
    for kw in ({}, {"last": 5}, {"sort": True}, {"last": 7, "sort": True}):
        got, want = env.episode_log(**kw), tw.rows(**kw)
        assert torch.equal(got["count"], torch.ones_like(got["count"])) and got["count"].dtype == torch.int32
        for k in RING_EXACT:
            assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(want[k])), (kw, k)
    env.close()


def test_two_identical_runs_give_bitwise_equal_rings():
    import torch
    N, M, S, L = 70, 10, 145, 8
    pool = _pool(S, M, seed=3, N=N)
    rings = []
    for _ in range(2):
        env = _env(N, M, S, pool, L)
        for how, T in SEQUENCE:
            _launch(env, how, T)
        rings.append({k: t.clone() for k, t in env.episode_log_views().items()})
        env.close()
    for k in rings[0]:
        a, b = rings[0][k], rings[1][k]
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k
    assert int(rings[0]["head"]) > L


def test_beside_the_recorder():
    """Records (keep='last') and log attached together on an S = 3 N pool: every row the log appends in a one-step call equals
    the table row of its slot at that moment, bit for bit; the two share no state."""
    import torch
    N, M = 33, 4
    S = 3 * N
    pool = _pool(S, M, seed=21, N=N)
    env = _env(N, M, S, pool, 4096)
    env.attach_episode_records(keep="last")
    head = 0
    for step in range(40):
        env.step(auto_reset=True)
        rec, log = env.episode_records(), env.episode_log()
        new = int(log["count"].numel()) - head
        assert new == int(env.game_over.sum())
        if new:
            slot = (log["key"][head:] % S).long()
            for k in ("t", "extra_t", "flags", "ret", "steps", "outcome"):
                a, b = log[k][head:], rec[k].index_select(0, slot)
                a, b = (a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else (a, b)
                assert torch.equal(a, b), (step, k)
            assert torch.equal(log["n_agents"][head:], rec["n_agents"].index_select(0, slot))
        head += new
    assert head >= 2 * N
    env.close()


# ---- streaming: the point of the feature ---------------------------------------------------------------------------------------------
def _stream_run(N, M, depth, E, args, K=0, laserscan=False, rollout_T=None, min_episodes=3, max_steps=1600):
    """A streaming handle with the log attached beside a handle holding the plain pool of E * N slots generated with the same
    arguments.  Steps (one-step launches, or rollout(rollout_T)) until every world finished min_episodes; the twin runs on the
    PLAIN pool, whose slot of (w, e) is row key = w + e * N itself."""
    import torch
    B = _B()
    env = B(N, M, n_scenarios=depth * N, max_obstacles=K, game_over_mode="agent0", laserscan=laserscan)
    ref = B(N, M, n_scenarios=E * N, max_obstacles=K, game_over_mode="agent0", laserscan=laserscan)
    assert env.stream_reference_scenarios(**args) == ref.generate_reference_scenarios(**args)
    env.reset()
    env.attach_episode_log(4096)
    plain = {k: t.cpu().numpy() for k, t in dict(ref.scenarios(), **ref.obstacles()).items()}
    tw = EpisodeLogTwin(N, M, plain["agents6"], plain["n_agents"], DT, 4096, n_obst=plain["n_obst"])
    T = rollout_T or 32
    steps = 0
    while steps < max_steps:
        if rollout_T:
            tw.update(*_launch(env, "rollout", T))
        else:  # T one-step launches, their outputs read back together
            F = torch.zeros((T, N, M), dtype=torch.uint8, device=env.device)
            R = torch.zeros((T, N, M), dtype=torch.float32, device=env.device)
            G = torch.zeros((T, N), dtype=torch.uint8, device=env.device)
            for t in range(T):
                env.step(auto_reset=True)
                F[t], R[t], G[t] = env.flags, env.reward, env.game_over
            F, R, G = F.cpu().numpy(), R.cpu().numpy(), G.cpu().numpy()
            for t in range(T):
                tw.update(F[t:t + 1], R[t:t + 1], G[t:t + 1])
        steps += T
        if int(env.episode_stats()["stat_episodes"].min()) >= min_episodes:
            break
    assert int(env.episode_stats()["stat_episodes"].min()) >= min_episodes, steps
    assert int(env.state()["episode"].max()) < E, "the plain pool is too short"
    assert env.stream_stats()["n_lapped"] == 0
    _compare(env, tw, "stream N%d depth %d" % (N, depth))
    rows = {k: t.cpu().numpy() for k, t in env.episode_log().items()}
    key = rows["key"]
    assert len(key) == tw.head and np.array_equal(key, rows["world"] + rows["episode"].astype(np.int64) * N)
    assert key.max() >= (min_episodes - 1) * N  # rows of refilled slots are among them
    # every row describes the scenario its key names in the plain pool
    assert np.array_equal(rows["n_agents"], plain["n_agents"][key])
    assert np.array_equal(rows["n_obst"], plain["n_obst"][key])
    live = np.arange(M)[None, :] < rows["n_agents"][:, None]
    sl = np.zeros_like(rows["t"])
    sl[live] = straight_line_time(plain["agents6"][key])[live]
    e = np.abs(rows["extra_t"] - np.where(live, rows["t"] - sl, 0.0)).max()
    print("stream extra_t against the plain pool's rows: max |diff| %.3e over %d rows" % (e, len(key)))
    assert e <= 1e-12
    env.close()
    ref.close()
    return rows


def _swap_circle_args(seed=11):
    # as tests/test_stream_scenarios.py: the reference's default agent count range, NonCooperative unicycles
    return dict(kinds="train_agents_swap_circle", seed=seed, ego_policy=scen.POLICY_NONCOOP, ego_dynamics=scen.DYN_UNICYCLE,
                other_policies=scen.POLICY_NONCOOP)


def test_streaming_one_step_launches():
    """Ring depth 2: the refill behind a step regenerates the slot of the episode that just ended at once - an update enqueued
    behind the refill would log the NEXT scenario's agent count and straight-line times."""
    rows = _stream_run(16, 4, 2, 32, _swap_circle_args())
    assert len(set(rows["n_agents"].tolist())) > 1  # the agent count varies over the keys: a wrong slot would show


def test_streaming_rectangles_rvo_laserscan():
    # (RVO agents among rectangles: at max_agents 4 the handle takes 4 of them, so stage 2's 2..10 are narrowed to 2..4)
    rows = _stream_run(8, 4, 2, 128, dict(kinds="train_stage_2", seed=12, n_obst=(2, 4), ego_policy=scen.POLICY_NONCOOP,
                                          ego_dynamics=scen.DYN_UNICYCLE), K=4, laserscan=True)
    assert rows["n_obst"].min() >= 2 and len(set(rows["n_obst"].tolist())) > 1


def test_streaming_rollouts():
    _stream_run(16, 4, 4, 32, _swap_circle_args(seed=12), rollout_T=40)


# ---- chains --------------------------------------------------------------------------------------------------------------------------
def test_ga3c_chain_feeds_the_log():
    N, M, S, L = 4, 3, 8, 64
    a6, pol, n_agents = _pool(S, M, seed=5)
    pol[:, 0] = scen.POLICY_GA3C  # one GA3C agent, NonCooperative others
    n_agents[:] = M
    env = _env(N, M, S, (a6, pol, n_agents), L)
    env.attach_ga3c()
    tw = _twin(env, (a6, pol, n_agents), L)
    for T in (12, 1, 30):
        tw.update(*_launch(env, "rollout", T))
        _compare(env, tw, "GA3C chain T %d" % T)
    assert tw.head >= 2
    env.close()


def test_episodic_ig_greedy_chain_feeds_the_log():
    team_env = importlib.import_module("test_ig_greedy")._team_env
    env = team_env(2, episodic_pool=True)  # 2 worlds, 2 robots; time limits of 5 to 9 steps
    env.attach_ig_greedy(episodic=True)
    env.attach_episode_log(64)
    sc = {k: t.cpu().numpy() for k, t in dict(env.scenarios(), **env.obstacles()).items()}
    tw = EpisodeLogTwin(env.N, env.M, sc["agents6"], sc["n_agents"], DT, 64, n_obst=sc["n_obst"])
    for T in (7, 1, 16):
        tw.update(*_launch(env, "rollout", T))
        _compare(env, tw, "IG chain T %d" % T)
    assert tw.head >= 3 and (tw.rows()["n_obst"] == 4).all()
    env.close()


def test_vecenv_feeds_the_log():
    vec = importlib.import_module("gym-exploration-2d_amd.vecenv")
    N, M, S = 6, 3, 18
    pool = _pool(S, M, seed=12)
    env = _env(N, M, S, pool, 64)
    v = vec.CagymVecEnv(env, ["dist_to_goal", "other_agents_states"])
    dones = 0
    for _ in range(20):
        dones += int(v.step([None])[2].sum())
    log = env.episode_log()
    assert dones > 0 and int(log["count"].numel()) == dones == int(env.episode_stats()["stat_episodes"].sum())
    env.close()


def test_graph_replay_equals_eager_calls():
    """The single-launch rollout(8) and its log update captured on one stream and replayed three times: the rows of three eager
    calls (no argument of the update advances on the host)."""
    import torch
    N, M, S, L = 64, 4, 192, 4096
    pool = _pool(S, M, seed=8)
    a, b = _env(N, M, S, pool, L), _env(N, M, S, pool, L)
    for _ in range(3):
        a.rollout(8, auto_reset=True, out=a.alloc_rollout(8, obs=False))
    buf = b.alloc_rollout(8, obs=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.rollout(8, auto_reset=True, out=buf)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    va, vb = a.episode_log_views(), b.episode_log_views()
    assert int(va["head"]) >= N // 4 and int(vb["desync"]) == 0
    for k in va:
        x, y = va[k], vb[k]
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y), k
    a.close()
    b.close()


# ---- lifecycle and refusals -------------------------------------------------------------------------------------------------------------
def test_manual_reset_leaves_no_row():
    import torch
    N, M, S, L = 6, 3, 18, 64
    pool = _pool(S, M, seed=9)
    env = _env(N, M, S, pool, L)
    tw = _twin(env, pool, L)
    for _ in range(3):
        tw.update(*_launch(env, "step", 1))
    assert int(env.state()["episode"][2]) == 0 and int(env.state()["episode"][0]) == 0  # worlds 0 (goal) and 2 (time-out) in mid-episode
    mask = np.zeros(N, dtype=np.uint8)
    mask[0] = mask[2] = 1
    env.reset(world_mask=mask, advance_episode=True)
    torch.cuda.synchronize()
    tw.restart(mask, episode0=env.state()["episode"].cpu().numpy())
    G = []
    for _ in range(20):
        F, R, g = _launch(env, "step", 1)
        tw.update(F, R, g)
        G.append(g[0])
    _compare(env, tw, "manual reset")
    G = np.array(G)
    rows = {k: t.cpu().numpy() for k, t in env.episode_log(sort=True).items()}
    for w in (0, 2):
        mine = rows["world"] == w
        assert 0 not in rows["episode"][mine].tolist()  # the abandoned episode 0 left no row
        first = int(np.argmax(G[:, w]))
        assert G[first, w] and rows["episode"][mine][0] == 1 and rows["steps"][mine][0] == first + 1  # counted from the reset
    env.close()


def test_new_pool_keeps_rows_clear_and_reattach():
    import torch
    N, M, S, L = 6, 3, 18, 32
    pool = _pool(S, M, seed=10)
    env = _env(N, M, S, pool, L)
    tw = _twin(env, pool, L)
    tw.update(*_launch(env, "rollout", 9))
    before = {k: t.clone() for k, t in env.episode_log().items()}
    assert tw.head > 0
    pool2 = _pool(S, M, seed=11)
    env.set_scenarios(pool2[0], pool2[1], scen.DYN_UNICYCLE, n_agents=pool2[2], coop=np.full((S, M), 0.5))
    v = env.episode_log_views()
    for k in RUNNING:
        assert not bool(v[k].any()), k  # the running values are cleared ...
    after = env.episode_log()
    for k in before:
        assert torch.equal(before[k], after[k]), k  # ... the rows stay
    env.reset()
    tw.set_pool(pool2[0], pool2[2])
    tw.update(*_launch(env, "rollout", 9))
    tw.update(*_launch(env, "step", 1))
    _compare(env, tw, "new pool")
    assert int(env.episode_log()["slice"].max()) >= 9  # slice goes on counting
    env.clear_episode_log()
    v = env.episode_log_views()
    assert int(v["head"]) == 0 and int(env.episode_log()["count"].numel()) == 0
    for k in RING_EXACT + ("extra_t",):
        assert not bool(v[k].any()), k
    # another capacity: a fresh, empty ring that works
    env.reset()
    env.attach_episode_log(5)
    v = env.episode_log_views()
    assert v["key"].shape == (5,) and v["t"].shape == (5, M) and int(v["head"]) == 0
    tw = _twin(env, pool2, 5, episode0=env.state()["episode"].cpu().numpy())  # reset() keeps the episode indices
    tw.update(*_launch(env, "rollout", 20))
    _compare(env, tw, "capacity 5")
    assert tw.head > 5
    env.detach_episode_log()
    env.step(auto_reset=False)  # detached: not fed, not refused
    env.close()


def test_desync_is_reported():
    import torch
    N, M, S = 6, 3, 18
    env = _env(N, M, S, _pool(S, M, seed=6), 16)
    env.step(auto_reset=True)
    assert int(env.episode_log_views()["desync"]) == 0
    env.detach_episode_log()
    env.step(auto_reset=True)  # a step the log never sees
    env._log = 16
    env.step(auto_reset=True)
    assert int(env.episode_log_views()["desync"]) >= 1
    with pytest.raises(RuntimeError, match="desync"):
        env.episode_log()
    env.episode_log(check=False)
    env.attach_episode_log(16)  # clears
    assert int(env.episode_log_views()["desync"]) == 0
    env.close()


def test_contract_and_error_codes():
    import torch
    lib = importlib.import_module("gym-exploration-2d_amd._lib")
    N, M, S = 6, 3, 12
    env = _B()(N, M, n_scenarios=S)
    L, h, st = env.L, env.h, env._stream()
    f, r, g = env.flags.data_ptr(), env.reward.data_ptr(), env.game_over.data_ptr()
    ptrs = lib.CagymEpisodeLogPtrs()
    E_INVALID, E_STATE = -1, -5
    # before a pool is installed
    assert L.cagym_episode_log_init(h, 8, st) == E_STATE
    assert L.cagym_episode_log_update(h, f, r, g, 1, st) == E_STATE
    assert L.cagym_episode_log_restart(h, None, 0, st) == E_STATE
    assert L.cagym_episode_log_get(h, ctypes.byref(ptrs)) == E_STATE
    a6, pol, n_agents = _pool(S, M, seed=8)
    env.set_scenarios(a6, pol, scen.DYN_UNICYCLE, n_agents=n_agents)
    env.reset()
    # before init
    assert L.cagym_episode_log_update(h, f, r, g, 1, st) == E_STATE
    assert L.cagym_episode_log_restart(h, None, 0, st) == E_STATE
    assert L.cagym_episode_log_get(h, ctypes.byref(ptrs)) == E_STATE
    assert b"cagym_episode_log_init" in L.cagym_last_error(h)
    assert L.cagym_episode_log_init(h, 0, st) == E_INVALID
    assert L.cagym_episode_log_init(h, -3, st) == E_INVALID
    with pytest.raises(ValueError):
        env.attach_episode_log(0)
    with pytest.raises(RuntimeError, match="attach_episode_log"):
        env.episode_log()
    env.step(auto_reset=False)  # a handle that never called init behaves as before
    snap0 = env.snapshot()
    env.restore(snap0)
    env.reset()
    env.attach_episode_log(8)
    assert L.cagym_episode_log_update(h, None, r, g, 1, st) == E_INVALID
    assert L.cagym_episode_log_update(h, f, None, g, 1, st) == E_INVALID
    assert L.cagym_episode_log_update(h, f, r, None, 1, st) == E_INVALID
    assert L.cagym_episode_log_update(h, f, r, g, 0, st) == E_INVALID
    assert L.cagym_episode_log_get(h, None) == E_INVALID
    assert L.cagym_episode_log_get(h, ctypes.byref(ptrs)) == 0 and ptrs.t and ptrs.head and ptrs.capacity == 8
    # the contract, at the Python surface
    with pytest.raises(RuntimeError, match="auto-reset stepping only"):
        env.step(auto_reset=False)
    with pytest.raises(RuntimeError, match="auto-reset stepping only"):
        env.rollout(4, auto_reset=False)
    with pytest.raises(RuntimeError, match="auto-reset stepping only"):
        env.step_begin()
        env.step_finish(auto_reset=False)
    env.step_finish(auto_reset=True)  # consumes the begin; logged
    env.step_overlapped(lambda a: None, None, auto_reset=True)
    torch.cuda.synchronize()
    assert int(env.episode_log_views()["desync"]) == 0 and int(env.episode_log_views()["steps_run"].max()) == 2
    # restore and fork are refused, by the env while attached and by the library while initialised; snapshot is not
    snap = env.snapshot()
    with pytest.raises(RuntimeError, match="episode log"):
        env.restore(snap)
    with pytest.raises(RuntimeError, match="episode log"):
        env.fork([0], [1])
    ids = torch.zeros(1, dtype=torch.int32, device=env.device)
    assert L.cagym_restore(h, ctypes.byref(snap.layout), snap.blob.data_ptr(), None, snap.n, st) == E_STATE
    assert L.cagym_fork(h, ids.data_ptr(), (ids + 1).data_ptr(), 1, st) == E_STATE
    assert b"episode log" in L.cagym_last_error(h)
    env.close()


def test_records_are_still_refused_on_a_streaming_env_and_the_log_is_not():
    N = 8
    env = _B()(N, 4, n_scenarios=2 * N, game_over_mode="agent0")
    env.stream_reference_scenarios(**_swap_circle_args())
    env.reset()
    with pytest.raises(RuntimeError, match="streaming"):
        env.attach_episode_records()
    assert env.L.cagym_episode_records_init(env.h, 0, env._stream()) == -5
    env.attach_episode_log(64)
    env.set_stream_params(**_swap_circle_args(seed=3))  # not refused with a log
    env.stream_reference_scenarios(**_swap_circle_args(seed=4))  # nor is a restart of the stream
    env.reset()
    env.step(auto_reset=True)
    assert int(env.episode_log_views()["desync"]) == 0
    env.close()


def test_suite_statistics_on_a_window():
    stats = importlib.import_module("gym-exploration-2d_amd.stats")
    N, M, S, L = 33, 10, 71, 4096
    pool = _pool(S, M, seed=14, N=N)
    env = _env(N, M, S, pool, L)
    tw = _twin(env, pool, L)
    for T in (33, 33, 33):
        tw.update(*_launch(env, "rollout", T))
    for K in (64, 7, 100000):
        got = stats.suite_statistics(env.episode_log(last=K))
        rows = tw.rows(last=K)
        n = len(rows["key"])
        coll = (rows["outcome"] & 1) != 0
        goal = (rows["outcome"] & 2) != 0
        clean = ~coll & goal
        mean = np.array([rows["extra_t"][i, :rows["n_agents"][i]].mean() for i in range(n)])
        p = np.percentile(mean[clean], [50, 75, 90]) if clean.any() else np.full(3, np.nan)
        assert got["n_cases"] == n == got["n_run"] == min(K, tw.head)
        assert got["pct_collision"] == 100.0 * coll.sum() / n and got["pct_stuck"] == 100.0 * (~coll & ~goal).sum() / n
        assert (got["clean"].cpu().numpy() == clean).all()
        gp = got["extra_time_pctls"].cpu().numpy()
        print("window", K, "rows", n, "pctls", gp, p)
        assert np.allclose(gp, p, rtol=0, atol=1e-12, equal_nan=True), (gp, p)
    assert tw.head > 64
    env.close()
