"""Replay of failed scenarios in the scenario stream (include/cagym.h: cagym_stream_replay_*): a device buffer of stream keys,
harvested from the episode log or pushed, from which the armed refill draws some of the slots it generates.

The yardsticks: scenarios.replay_choice (the draw in plain Python, itself pinned to tests/sampler_twin.py's generator), a plain
reference pool whose row v is the scenario of key v, a plain stream on a second handle, and the episode log of the handle under
test: with one-step launches the log alone determines the buffer at every refill, so _predict() replays the whole run on the host
and every key the device chose is compared with it.  Every comparison is exact.

Workloads (lengths and outcomes from the C oracle and the sampler twin over keys 0..1023):
  collisions   train_agents_random_positions, seed 11, four NonCooperative unicycles, game over with agent 0: 286 of 1024 keys end
               in an ego collision, 738 at the goal, every block of 64 consecutive keys holds 9..27 collisions, lengths 6..179
               (median 61.5), n_failed 0
  all-collide  test_stream_scenarios' swap circle (seed 11): all 1024 keys end in an ego collision, lengths 16..72
  rectangles   test_stream_scenarios.test_mixture_and_tail_lanes' 96 x 10 mixture with seed 15 (lengths 6..192, n_failed 0)"""
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sampler_twin as tw
from test_stream_scenarios import _bits, _mods, _outs, _pool, _same, _swap_circle_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cagym_stream_replay_init": 4, "cagym_stream_replay_set": 3, "cagym_stream_replay_push": 4, "cagym_stream_replay_harvest": 2,
           "cagym_stream_replay_get": 6}
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -5, -6
SALT = 0x9E3779B97F4A7C15
PUSHED = [3, 700, 64, 999, 3]
ROW_COLUMNS = ("steps", "ret", "outcome", "n_agents", "t", "extra_t", "flags")  # what a replayed key must reproduce


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_prototype_table_carry_the_replay_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cagym.h")).read(), flags=re.S)
    declared = {n: (0 if p.strip() in ("", "void") else p.count(",") + 1)
                for n, p in re.findall(r"\b(cagym_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}
    lib = importlib.import_module("gym-exploration-2d_amd._lib")
    for name, n_params in ENTRIES.items():
        assert declared.get(name) == n_params, (name, declared.get(name))
        assert name in lib._ARGTYPES and len(lib._ARGTYPES[name]) == n_params, name


def _rule(seed, key, p, live):
    """The specification of include/cagym.h evaluated with the sampler twin's generator."""
    rs = (seed ^ SALT) & tw.MASK
    u0, u1 = tw.u01(rs, key, 0), tw.u01(rs, key, 1)
    if not (live > 0 and u0 < p):
        return False, 0
    return True, min(live - 1, int(u1 * live))


def test_replay_choice_is_the_rule():
    sc = importlib.import_module("gym-exploration-2d_amd.scenarios")
    keys = list(range(0, 40)) + [63, 64, 1023, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 64, 2 ** 32 - 2, 2 ** 32 - 1]
    n = picked = 0
    seen = set()
    for seed in (0, 1, 11, 2 ** 63 + 5, 2 ** 64 - 1):
        for p in (0.0, 0.25, 0.5, 1.0):
            for live in (0, 1, 2, 5, 256, 4096):
                for key in keys:
                    got = sc.replay_choice(seed, key, p, live)
                    assert got == _rule(seed, key, p, live), (seed, key, p, live)
                    assert got[0] == (live > 0 and p > 0.0) if p in (0.0, 1.0) else True
                    assert 0 <= got[1] < max(live, 1)
                    n += 1
                    picked += got[0]
                    if got[0] and live == 5:
                        seen.add(got[1])
    assert 0 < picked < n and seen == set(range(5))
    assert sc.replay_choice(3, 2 ** 32 + 7, 0.5, 9) == sc.replay_choice(3, 7, 0.5, 9)  # the key is a u32
    assert sc.generator_u01(5, 6, 7) == tw.u01(5, 6, 7)


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------------
def _collision_args(sc, seed=11):
    return dict(kinds="train_agents_random_positions", seed=seed, number_of_agents=4, fixed_count=True, ego_policy=sc.POLICY_NONCOOP,
                ego_dynamics=sc.DYN_UNICYCLE, other_policies=sc.POLICY_NONCOOP, other_dynamics=sc.DYN_UNICYCLE)


def _stream_env(N, M, depth, args, K=0, log=4096):
    torch, sc, B = _mods()
    env = B(N, M, n_scenarios=depth * N, max_obstacles=K, game_over_mode="agent0")
    assert env.stream_reference_scenarios(**args) == 0
    if log:
        env.attach_episode_log(log)
    env.reset()
    return env


def _rows(env):
    """The log's rows in append order as host arrays (key as int64 in [0, 2^32))."""
    return {k: v.cpu().numpy() for k, v in env.episode_log().items()}


def _u32(t):
    return (t.to(__import__("torch").int64) & 0xFFFFFFFF).cpu().numpy()


def _ring(env):
    """(idx, slot) int64 [N, depth] of the ring: world w's episodes episode[w] .. episode[w] + depth - 1."""
    N, S = env.N, env.S
    ep = env.state()["episode"].cpu().numpy().astype(np.int64)
    idx = np.arange(N)[:, None] + (ep[:, None] + np.arange(S // N)[None, :]) * N
    return idx, idx % S


def _predict(rows, N, depth, seed, p, Q, buf=(), mask=0):
    """Host replay of a run of ONE-STEP launches from its log: behind the step of slice t the harvest appends the keys of that slice's
    rows whose outcome meets `mask` (in row order), then the refill generates, for every world that finished episode e in that
    slice, the slot of episode e + depth - from replay_choice's pick among the newest min(len(buf), Q) entries, or from its own
    key.  Returns ({idx: key} of every slot generated behind a step, the buffer's entries in append order, slots generated while
    the buffer was not empty, how many of those were replayed)."""
    sc = importlib.import_module("gym-exploration-2d_amd.scenarios")
    buf, pred, n, r = list(buf), {}, 0, 0
    order = np.arange(len(rows["slice"]))
    assert (np.diff(rows["slice"]) >= 0).all()  # append order is slice-major
    for t in np.unique(rows["slice"]):
        at = order[rows["slice"] == t]
        buf += [int(rows["key"][i]) for i in at if int(rows["outcome"][i]) & mask]
        live = min(len(buf), Q)
        for i in at:
            idx = int(rows["world"][i]) + (int(rows["episode"][i]) + depth) * N
            rp, j = sc.replay_choice(seed, idx, p, live)
            pred[idx] = buf[len(buf) - live + j] if rp else idx & 0xFFFFFFFF
            n += live > 0
            r += rp
    return pred, buf, n, r


def _assert_keys(env, rows, pred, depth):
    """The log's key of every episode, and slot_key of every slot of the ring, is its own key for the first `depth` episodes of a
    world (the stream's first fill) and the predicted one for every later episode."""
    N = env.N
    want = lambda idx: pred[idx] if idx >= depth * N else idx
    for i in range(len(rows["key"])):
        idx = int(rows["world"][i]) + int(rows["episode"][i]) * N
        assert int(rows["key"][i]) == want(idx), ("log row", i, idx)
    idx, slot = _ring(env)
    sk = _u32(env.stream_keys())
    for a, s in zip(idx.flatten(), slot.flatten()):
        assert int(sk[s]) == want(int(a)), ("slot", int(s), int(a))
    assert (env.replay_views()["slot_gen"] == 1).all()


def _assert_reproduced(rows, sel=None):
    """(c) a row whose key is not its own (world + episode * N: a replayed scenario, or one a lapped world met again) equals, in every
    column the episode computes, the FIRST row of that key.  Returns how many such rows there were."""
    first, n = {}, 0
    for i in range(len(rows["key"])):
        if sel is not None and not sel[i]:
            continue
        k = int(rows["key"][i])
        if k not in first:
            first[k] = i
            continue
        n += 1
        for c in ROW_COLUMNS:
            a, b = rows[c][i], rows[c][first[k]]
            assert a.tobytes() == b.tobytes(), (c, i, first[k], k)
    return n


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_means_off():
    """Armed with nothing in the buffer (p = 0.5), and armed with keys in the buffer and p = 0, the stream is the plain stream bit
    for bit: outputs of every step, the pool, the stream's counters and the log; slot_key names every slot's own key."""
    torch, sc, B = _mods()
    N, depth, T = 64, 2, 224
    args = _swap_circle_args(sc)
    plain, empty, paused = (_stream_env(N, 4, depth, args) for _ in range(3))
    empty.attach_replay(capacity=64, p=0.5, outcomes=None, seed=7)
    paused.attach_replay(capacity=64, p=0.0, outcomes=None, seed=7)
    paused.replay_push(PUSHED)
    eq = torch.ones((T, 2, len(_outs(plain))), dtype=torch.bool, device=plain.device)
    for t in range(T):
        for h in (plain, empty, paused):
            h.step(auto_reset=True)
        for k, h in enumerate((empty, paused)):
            for i, (a, b) in enumerate(zip(_outs(h), _outs(plain))):
                eq[t, k, i] = (_bits(a) == _bits(b)).all()
    assert int(plain.episode_stats()["stat_episodes"].min()) >= 3  # (lengths 16..72: every world ran on refilled slots)
    bad = (~eq).nonzero()
    assert bad.numel() == 0, "first (step, handle, output) that differs from the plain stream: %s" % bad[0].tolist()
    want_pool, want_log, want_stats = _pool(plain), plain.episode_log(), plain.stream_stats()
    assert want_stats["generated"] > plain.S and len(want_log["key"]) >= 3 * N
    for h in (empty, paused):
        for name, t in _pool(h).items():
            assert _same(t, want_pool[name]), name
        assert h.stream_stats() == want_stats
        got = h.episode_log()
        assert sorted(got) == sorted(want_log)
        for name, t in got.items():
            assert _same(t, want_log[name]), name
        idx, slot = _ring(h)
        assert (_u32(h.stream_keys())[slot] == idx).all()
        st = h.replay_stats()
        assert st["replayed"] == 0 and st["harvested"] == 0 and st["n_missed"] == 0 and st["n_stale"] == 0
    assert empty.replay_stats()["count"] == 0 and paused.replay_stats()["count"] == paused.replay_stats()["pushed"] == len(PUSHED)
    assert _u32(paused.replay_views()["buf_key"])[:len(PUSHED)].tolist() == PUSHED
    for h in (plain, empty, paused):
        h.close()


def _run_pushed(N, M, K, args, T=400, seed=5):
    torch, sc, B = _mods()
    depth, Q = 2, 8
    env = _stream_env(N, M, depth, args, K=K)
    ref = B(N, M, n_scenarios=1024, max_obstacles=K, game_over_mode="agent0")
    assert ref.generate_reference_scenarios(**args) == 0
    env.attach_replay(capacity=Q, p=1.0, outcomes=None, seed=seed)
    env.replay_push(PUSHED)
    for _ in range(T):
        env.step(auto_reset=True)
    assert int(env.episode_stats()["stat_episodes"].min()) >= 2, "precondition: every world ran on a slot generated after the push"
    st, ss = env.replay_stats(), env.stream_stats()
    assert ss["n_lapped"] == 0 and ss["n_failed"] == 0
    assert st["count"] == st["pushed"] == st["live"] == len(PUSHED) and st["harvested"] == 0
    assert st["replayed"] == ss["generated"] - env.S and st["replayed"] >= N
    rows = _rows(env)
    pred, _, n, r = _predict(rows, N, depth, seed, 1.0, Q, buf=PUSHED)
    assert n == r == st["replayed"] == len(rows["key"])
    assert {PUSHED[sc.replay_choice(seed, idx, 1.0, 5)[1]] for idx in pred} == set(PUSHED)  # (the picks reach every entry)
    assert all(pred[idx] == PUSHED[sc.replay_choice(seed, idx, 1.0, 5)[1]] for idx in pred)
    _assert_keys(env, rows, pred, depth)
    # the pool rows of every slot are the reference pool's row slot_key, over every array the ABI shows
    sk = env.stream_keys().to(torch.int64) & 0xFFFFFFFF
    assert int(sk.max()) < 1024
    ring, big = _pool(env), _pool(ref)
    assert sorted(ring) == sorted(big) and (K == 0 or ("map_bits" in ring and "obstacles" in ring))
    for name, t in ring.items():
        assert _same(t, big[name].index_select(0, sk)), name
    if K:
        assert int(ring["n_obst"].max()) > 0 and int(ring["map_bits"].ne(0).sum()) > 0
    assert _assert_reproduced(rows) >= 8
    env.close()
    ref.close()


@pytest.mark.gpu
def test_pushed_keys_exact_picks():
    """Collisions workload, p = 1 with five pushed keys: in 400 steps every world finishes >= 2 episodes (lengths <= 179), and
    every slot generated behind a step is the reference pool's row of replay_choice's pick."""
    _, sc, _ = _mods()
    _run_pushed(64, 4, 0, _collision_args(sc))


@pytest.mark.gpu
def test_pushed_keys_rectangles_and_tail_lanes():
    """The same on the 96 x 10 mixture among rectangles (lengths 6..192): the refill's second wave is half full, and the pool check
    covers obstacles, prep-dependent n_obst and the rasters."""
    _, sc, _ = _mods()
    _run_pushed(96, 10, 10, dict(kinds=[0, 1, 2, 3, 4], seed=15, ego_policy=sc.POLICY_NONCOOP))


def _assert_buffer(env, want_keys, Q):
    """(a) the buffer's newest live entries are `want_keys`' newest, in order; count is their number."""
    st = env.replay_stats()
    assert st["count"] == len(want_keys) and st["live"] == min(len(want_keys), Q)
    buf = _u32(env.replay_views()["buf_key"])
    c, live = st["count"], st["live"]
    got = [int(buf[i % Q]) for i in range(c - live, c)]
    assert got == [int(k) for k in want_keys[len(want_keys) - live:]]
    return st


@pytest.mark.gpu
def test_harvest_from_the_log():
    """Collisions workload, N = 64, depth 2, log of 4096 rows, buffer of 256 keys, p = 0.5, outcomes = collision, 400 one-step
    launches.  On the device: 428 rows, 295 of them harvested (a replayed collision collides again), 226 slots replayed, 164
    replayed episodes finished."""
    torch, sc, B = _mods()
    N, depth, Q, seed, p, T = 64, 2, 256, 3, 0.5, 400
    env = _stream_env(N, 4, depth, _collision_args(sc))
    env.attach_replay(capacity=Q, p=p, outcomes=("collision",), seed=seed)
    for _ in range(T):
        env.step(auto_reset=True)
    rows = _rows(env)
    st, ss = env.replay_stats(), env.stream_stats()
    own = rows["world"] + rows["episode"].astype(np.int64) * N
    replayed_rows = rows["key"] != own
    print("harvested %d replayed %d finished replayed %d rows %d" % (st["harvested"], st["replayed"], replayed_rows.sum(), len(own)))
    assert ss["n_lapped"] == 0 and ss["n_failed"] == 0 and len(own) < 4096
    assert st["harvested"] >= 32 and st["replayed"] >= 32 and int(replayed_rows.sum()) >= 8, "preconditions"
    # (a)
    coll = (rows["outcome"] & 1) != 0
    got = _assert_buffer(env, rows["key"][coll], Q)
    assert got["count"] == got["harvested"] and got["pushed"] == 0
    # (b), exactly: every key of the log and of the ring is the one the host replay of the log predicts
    pred, buf, n, r = _predict(rows, N, depth, seed, p, Q, mask=1)
    assert buf == [int(k) for k in rows["key"][coll]]
    _assert_keys(env, rows, pred, depth)
    for i in np.nonzero(replayed_rows)[0]:  # ... which implies: its own key, or the key of an EARLIER collision row
        assert int(rows["key"][i]) in set(int(k) for k in rows["key"][:i][coll[:i]])
    # (c)
    assert _assert_reproduced(rows) >= int(replayed_rows.sum())
    # (d) 6 sigma of the binomial(n, 1/2)
    assert r == st["replayed"] and n >= 32
    assert abs(r - n / 2.0) <= 3.0 * math.sqrt(n), (r, n)
    # (e)
    assert st["n_missed"] == 0 and st["n_stale"] == 0
    env.close()


def _assert_lineage(rows, N, depth, lapped):
    """(b) under roll-outs: a row's key is its own, or the key of an earlier collision row, or - only when the stream counted laps -
    the key of the same world's row `depth` episodes earlier (the slot's content, which a lapped world met again)."""
    seen_coll, by_we = set(), {}
    for i in range(len(rows["key"])):
        w, e, k = int(rows["world"][i]), int(rows["episode"][i]), int(rows["key"][i])
        ok = k == (w + e * N) & 0xFFFFFFFF or k in seen_coll or (lapped and by_we.get((w, e - depth)) == k)
        assert ok, (i, w, e, k)
        by_we[(w, e)] = k
        if int(rows["outcome"][i]) & 1:
            seen_coll.add(k)


@pytest.mark.gpu
def test_rollouts_and_a_small_log():
    """Depth 3, four rollout(64) launches: a harvest sees several rows per world.  Two identical handles agree in everything; a third
    one with a log of 32 rows misses exactly the rows its log dropped.  (The third handle's buffer differs from the first launch's
    harvest on, so its later launches finish other episodes than the big-log handles': the rows of each of ITS updates are read
    from its own head - the log's counter, not the replay's -, and compared with the big-log handles' where the runs still
    coincide, in the first launch.)"""
    torch, sc, B = _mods()
    N, depth, Q, seed, L = 64, 3, 256, 3, 32
    args = _collision_args(sc)
    a, b, c = _stream_env(N, 4, depth, args), _stream_env(N, 4, depth, args), _stream_env(N, 4, depth, args, log=L)
    for h in (a, b, c):
        h.attach_replay(capacity=Q, p=0.5, outcomes=("collision",), seed=seed)
    heads = {h: [0] for h in (a, c)}
    surviving_collisions = 0
    for launch in range(4):
        for h in (a, b, c):
            h.rollout(64, auto_reset=True)
        for h in (a, c):
            heads[h].append(int(h.episode_log_views()["head"].item()))
        n = heads[c][-1] - heads[c][-2]
        kept = c.episode_log(last=min(n, L))
        surviving_collisions += int((kept["outcome"] & 1).ne(0).sum())
    per_update = {h: np.diff(heads[h]) for h in (a, c)}
    assert per_update[a][0] == per_update[c][0]
    dropped = int(np.maximum(per_update[c] - L, 0).sum())
    assert dropped > 0, "precondition: an update outgrows the small log"
    sc_ = c.replay_stats()
    assert sc_["n_missed"] == dropped and sc_["harvested"] == surviving_collisions and sc_["n_stale"] == 0
    # the two identical handles
    va, vb = a.replay_views(), b.replay_views()
    for name in va:
        assert _same(va[name], vb[name]), name
    la, lb = a.episode_log(), b.episode_log()
    for name in la:
        assert _same(la[name], lb[name]), name
    assert a.stream_stats() == b.stream_stats() and a.replay_stats() == b.replay_stats()
    # (a) - (c) on the big log
    rows = _rows(a)
    per_world = np.unique(np.stack([rows["slice"] // 64, rows["world"]]), axis=1, return_counts=True)[1]
    assert int(per_world.max()) >= 2, "precondition: a harvest sees several rows of one world"
    st = _assert_buffer(a, rows["key"][(rows["outcome"] & 1) != 0], Q)
    assert st["count"] == st["harvested"] and st["n_missed"] == 0 and st["n_stale"] == 0 and st["replayed"] >= 32
    _assert_lineage(rows, N, depth, a.stream_stats()["n_lapped"] > 0)
    own = rows["world"] + rows["episode"].astype(np.int64) * N
    assert int((rows["key"] != own).sum()) >= 8
    assert _assert_reproduced(rows) >= 8
    for h in (a, b, c):
        h.close()


@pytest.mark.gpu
def test_parameter_switch_empties_the_buffer():
    """The collisions workload, then set_stream_params to the swap circle, where every key collides (lengths 16..72).  A world meets
    the new set `depth` episodes after the switch, up to 2 x 179 steps later.  On the device, 150 + 1 + 500 one-step launches:
    128 stale rows (every world's two slots of the old set), 511 rows of the new set, 222 of them replayed."""
    torch, sc, B = _mods()
    N, depth, Q, seed = 64, 2, 256, 3
    env = _stream_env(N, 4, depth, _collision_args(sc))
    env.attach_replay(capacity=Q, p=0.5, outcomes=("collision",), seed=seed)
    for _ in range(150):
        env.step(auto_reset=True)
    before = env.replay_stats()
    n_before = len(_rows(env)["key"])
    assert before["live"] >= 8 and before["n_stale"] == 0
    env.set_stream_params(**_swap_circle_args(sc))
    c = env.state()["episode"].cpu().numpy().astype(np.int64)  # slots of episodes >= c + depth come from the new set
    env.step(auto_reset=True)
    st = env.replay_stats()
    new_rows = len(_rows(env)["key"]) - n_before
    assert st["count"] == 0 and st["live"] == 0 and st["n_stale"] == new_rows and st["harvested"] == before["harvested"]
    for _ in range(500):
        env.step(auto_reset=True)
    rows = _rows(env)
    after = np.arange(len(rows["key"])) >= n_before
    new_gen = rows["episode"] >= c[rows["world"]] + depth
    assert not (new_gen & ~after).any()
    own = rows["world"] + rows["episode"].astype(np.int64) * N
    st = env.replay_stats()
    print("stale %d new-generation rows %d of them replayed %d" % (st["n_stale"], new_gen.sum(), (new_gen & (rows["key"] != own)).sum()))
    assert st["n_stale"] == int((after & ~new_gen).sum()) and st["n_stale"] > 0 and st["n_missed"] == 0
    assert (rows["outcome"][new_gen] & 1).all() and int(new_gen.sum()) >= 32  # every key of the swap circle collides
    _assert_buffer(env, rows["key"][new_gen], Q)  # nothing of the old set entered, every row of the new one did
    assert st["harvested"] == before["harvested"] + int(new_gen.sum())
    # the new generation's keys: its own, or one of an earlier row of the NEW generation; a replayed one reproduces its episode
    seen = set()
    for i in np.nonzero(new_gen)[0]:
        assert int(rows["key"][i]) == int(own[i]) or int(rows["key"][i]) in seen, i
        seen.add(int(rows["key"][i]))
    assert int((new_gen & (rows["key"] != own)).sum()) >= 8, "precondition: replayed episodes of the new set finished"
    assert _assert_reproduced(rows, new_gen) >= 8
    idx, slot = _ring(env)
    gen = env.replay_views()["slot_gen"].cpu().numpy()
    e = (idx - np.arange(N)[:, None]) // N
    assert (gen[slot] == np.where(e >= c[:, None] + depth, 2, 1)).all()
    env.close()


@pytest.mark.gpu
def test_refusals_and_lifecycle():
    torch, sc, B = _mods()
    lib = importlib.import_module("gym-exploration-2d_amd._lib")
    N = 8
    args = _swap_circle_args(sc)
    env = B(N, 4, n_scenarios=2 * N, game_over_mode="agent0")
    env.generate_reference_scenarios(**args)
    env.reset()
    L, h, st = env.L, env.h, env._stream
    keys = torch.tensor([1, 2], dtype=torch.int32, device=env.device)
    # not streaming
    assert L.cagym_stream_replay_init(h, 16, 0, st()) == E_STATE
    assert L.cagym_stream_replay_set(h, 0.5, 1) == E_STATE
    assert L.cagym_stream_replay_push(h, keys.data_ptr(), 2, st()) == E_STATE
    assert L.cagym_stream_replay_harvest(h, st()) == E_STATE
    assert L.cagym_stream_replay_get(h, None, None, None, None, None) == E_STATE
    with pytest.raises(RuntimeError, match="not streaming"):
        env.attach_replay()
    for call in (env.set_replay, env.replay_stats, env.stream_keys, lambda: env.replay_push([1])):
        with pytest.raises(RuntimeError, match="attach_replay"):
            call()
    # streaming: outcomes without a log, capacity, p; push and harvest before init
    assert env.stream_reference_scenarios(**args) == 0
    env.reset()
    with pytest.raises(RuntimeError, match=r"attach_episode_log\(\)"):
        env.attach_replay(outcomes=("collision",))
    with pytest.raises(ValueError, match="outcomes"):
        env.attach_replay(outcomes=("crash",))
    assert L.cagym_stream_replay_push(h, keys.data_ptr(), 2, st()) == E_STATE
    assert L.cagym_stream_replay_harvest(h, st()) == E_STATE
    assert L.cagym_stream_replay_init(h, 0, 0, st()) == E_INVALID
    with pytest.raises(RuntimeError, match="capacity"):
        env.attach_replay(capacity=0, outcomes=None)
    assert env._replay is None
    env.attach_replay(capacity=16, p=0.5, outcomes=None)
    assert L.cagym_stream_replay_harvest(h, st()) == E_STATE  # armed, but no log
    for bad in (-0.1, 1.5, float("nan")):
        assert L.cagym_stream_replay_set(h, bad, 0) == E_INVALID
        with pytest.raises(RuntimeError, match="p must lie"):
            env.set_replay(p=bad)
    assert L.cagym_stream_replay_set(h, 0.5, 8) == E_INVALID
    with pytest.raises(RuntimeError, match=r"attach_episode_log\(\)"):
        env.set_replay(outcomes=("collision",))
    assert env.replay_stats()["p"] == 0.5
    env.attach_episode_log(256)
    env.set_replay(outcomes=("collision", "stuck"))
    assert env._replay["mask"] == 5
    assert L.cagym_stream_replay_harvest(h, st()) == 0
    snap = env.snapshot()  # stays allowed
    assert snap.n == N
    # reset(advance_episode=True) refills with replay
    env.set_replay(p=1.0)
    env.replay_push([5, 5, 5])
    env.reset(advance_episode=True)
    stats = env.replay_stats()
    assert stats["replayed"] == N and stats["count"] == 3 and stats["capacity"] == 16
    idx, slot = _ring(env)
    assert (_u32(env.stream_keys())[slot[:, 1]] == 5).all() and (_u32(env.stream_keys())[slot[:, 0]] == idx[:, 0]).all()
    # attaching again clears the buffer and may change the capacity; the key tables stay
    env.attach_replay(capacity=4, p=1.0, outcomes=None)
    stats = env.replay_stats()
    assert stats["count"] == 0 and stats["replayed"] == 0 and stats["capacity"] == 4 and env.replay_views()["buf_key"].numel() == 4
    assert (_u32(env.stream_keys())[slot[:, 1]] == 5).all()
    # an exploration stream
    ex = B(N, 6, n_scenarios=2 * N, max_obstacles=4)
    ex.stream_exploration_worlds("train_stage_1", 21, n_robots=2, n_targets=2, n_obst=(1, 4))
    assert ex.L.cagym_stream_replay_init(ex.h, 16, 0, ex._stream()) == E_UNSUPPORTED
    with pytest.raises(RuntimeError, match="exploration"):
        ex.attach_replay(outcomes=None)
    ex.close()
    # stop_streaming() and a pool setter end replay; a restarted stream is un-armed and bitwise plain
    env.stop_streaming()
    assert env._replay is None and L.cagym_stream_replay_set(h, 0.5, 0) == E_STATE
    assert L.cagym_stream_replay_get(h, None, None, None, None, None) == 0  # the views stay readable
    assert env.stream_reference_scenarios(**args) == 0
    env.attach_replay(capacity=16, p=1.0, outcomes=None)
    env.replay_push([5])
    env.generate_reference_scenarios(**args)
    assert env._replay is None and L.cagym_stream_replay_push(h, keys.data_ptr(), 2, st()) == E_STATE
    plain = B(N, 4, n_scenarios=2 * N, game_over_mode="agent0")
    for e in (env, plain):
        assert e.stream_reference_scenarios(**args) == 0
        e.attach_episode_log(256)
        e.reset()
    assert L.cagym_stream_replay_set(h, 0.5, 0) == E_STATE
    for _ in range(120):
        env.step(auto_reset=True)
        plain.step(auto_reset=True)
    assert int(plain.episode_stats()["stat_episodes"].min()) >= 1
    for a, b in zip(_outs(env), _outs(plain)):
        assert _same(a, b)
    for name, t in _pool(env).items():
        assert _same(t, _pool(plain)[name]), name
    la, lb = env.episode_log(), plain.episode_log()
    for name in la:
        assert _same(la[name], lb[name]), name
    assert env.stream_stats() == plain.stream_stats()
    env.close()
    plain.close()


@pytest.mark.gpu
def test_replay_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "replay_failures.py"), "--worlds", "64", "--steps", "400"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "replay done" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert re.search(r"fresh +\d+ episodes", r.stdout) and re.search(r"replayed +\d+ episodes", r.stdout), r.stdout
