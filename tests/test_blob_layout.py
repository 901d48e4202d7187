"""The byte layout of the snapshot and checkpoint blobs (include/cagym.h: cagym_snapshot / cagym_checkpoint_save), pinned under
CAGYM_SNAP_VERSION 1 / CAGYM_CKPT_VERSION 1.  Every offset is computed here, from the order the header documents: a 16-byte row
header, then each field at the next multiple of 16; a flat section starts at 0.  No table of the library is read.  Where the ABI
has a view of a field, the blob's bytes at the computed offset are compared with the view's.

Shapes, the smallest that reach every copy path:
  N = 3, M = 2         16-byte rows of fp64, 8-byte rows of int32 (the 16-byte and the word path), three rows
  N = 5, M = 4, K = 2  rectangles: sc_obst, sc_obst_prep, and the raster a checkpoint leaves out; the IG tail of a snapshot row
  N = 3, M = 2, depth 2, log capacity 7, replay capacity 5   the flat sections; the log's flags column is 14 bytes (byte tail)"""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_snapshot import KEPT_BY_FORK_DST

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
benv = importlib.import_module("gym-exploration-2d_amd.batched_env")
lib = importlib.import_module("gym-exploration-2d_amd._lib")
pytestmark = pytest.mark.gpu

SNAP_MAGIC, POOL_ROW_MAGIC = 0x43475331, 0x43475031  # CAGYM_SNAP_MAGIC, CAGYM_CKPT_ROW_MAGIC
HOST_BYTES = 8 + 48 + 32 + 8 + 4 + 20 + 8 + 8 + 16 + 8 + 8 + 64  # the checkpoint's host header, member by member: 232
RASTER_BYTES = 300 * 10 * 4
F64_STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "heading_ego", "dist_to_goal", "time_remaining", "t", "goal_x", "goal_y",
             "radius", "pref_speed", "speed", "delta_heading", "aux0", "aux1")


# ---- the documented orders: (view name or None, bytes) ---------------------------------------------------------------------------
def _state_fields(M, ig):
    f = [(k, 8 * M) for k in F64_STATE] + [(None, 8 * M)]  # ... and coop
    f += [("action", 8 * M), ("status", 4 * M), ("step_num", 4 * M), ("n_observed", 4 * M)]
    f += [("n_agents", 4), ("episode", 4), (None, 4), (None, 4)]  # ... the running episode length and return
    f += [("stat_return", 4), ("stat_episodes", 4), ("stat_steps", 4), ("stat_outcomes", 12)]
    if ig:
        f += [("belief", 3600 * 8), (None, 3600 * 8), ("running", 8), ("sum", 8), ("last", 8), ("episodes", 4)]
    return f


def _pool_fields(M, K):
    f = [("agents6", 48 * M), (None, 8 * M), ("coop", 8 * M), ("policy", 4 * M), ("dynamics", 4 * M), ("n_agents", 4),
         ("n_obst" if K else None, 4)]
    return f + ([("obstacles", 32 * K), (None, 64 * K)] if K else [])  # the rectangles and their prepared RVO form; no raster


def _stream_fields(N):
    return [("words", 16), ("next_episode", 4 * N)]  # generated u64, n_failed i32, n_lapped i32: one field


def _log_fields(N, M, L):
    return [("slice", 8 * L), ("ret", 8 * L), ("t", 8 * L * M), ("extra_t", 8 * L * M), ("key", 4 * L), ("world", 4 * L), ("episode", 4 * L),
            ("steps", 4 * L), ("outcome", 4 * L), ("n_agents", 4 * L), ("n_obst", 4 * L), ("flags", L * M),
            ("t_run", 8 * N * M), ("ret_run", 8 * N), ("steps_run", 4 * N), ("atgoal_run", 4 * N), ("cursor", 4 * N), ("desync", 4),
            (None, 8), ("head", 8)]  # ... the slice counter


def _replay_fields(S, Q):
    return [("buf_key", 4 * Q), ("words", 8 * 7), (None, 4), ("slot_key", 4 * S), ("slot_gen", 4 * S)]  # counters + cursor; buf_gen


def _offsets(fields, start):
    """[(name, offset, bytes)] and the end rounded up to 16"""
    out, off = [], start
    for name, nbytes in fields:
        out.append((name, off, nbytes))
        off += (nbytes + 15) & ~15
    return out, off


def _bytes(t):
    """[rows, ...] as [rows, bytes per row]"""
    import torch
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


def _check_rows(blob, fields, views, magic, ids, what):
    """blob [n, row_bytes] u8: row r's header names ids[r], and every viewed field holds the view's row ids[r]"""
    import torch
    table, row_bytes = _offsets(fields, 16)
    assert blob.shape[1] == row_bytes, (what, blob.shape[1], row_bytes)
    header = blob[:, :16].contiguous().view(torch.int32).cpu()
    want = torch.tensor([[w, magic, 0, 0] for w in ids], dtype=torch.int32)
    assert torch.equal(header, want), (what, header.tolist())
    pick = torch.tensor(ids, device=blob.device)
    checked = 0
    for name, off, nbytes in table:
        if name is None:
            continue
        src = _bytes(views[name])[pick]
        assert src.shape[1] == nbytes, (what, name, src.shape[1], nbytes)
        assert torch.equal(blob[:, off:off + nbytes], src), (what, name, off)
        checked += 1
    assert checked == sum(n is not None for n, _ in fields)


def _check_flat(flat, fields, views, what):
    """flat: one section of a checkpoint's blob; every viewed field holds the whole view"""
    import torch
    table, nbytes_all = _offsets(fields, 0)
    assert flat.numel() == nbytes_all, (what, flat.numel(), nbytes_all)
    for name, off, nbytes in table:
        if name is None:
            continue
        src = views[name].contiguous().reshape(-1).view(torch.uint8)
        assert src.numel() == nbytes, (what, name, src.numel(), nbytes)
        assert torch.equal(flat[off:off + nbytes], src), (what, name, off)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _fixed_pool_env(N, M, K):
    env = benv.BatchedCollisionAvoidanceEnv(N, M, n_scenarios=N, max_obstacles=K, game_over_mode="all", laserscan=bool(K))
    if K:
        a6, obst, n_obst, _ = scen.obstacle_worlds(N, M, K, seed=7)
    else:
        a6, obst, n_obst = scen.random_worlds_fast(N, M, seed=7), None, None
    heading0 = np.linspace(-1.0, 1.0, N * M).reshape(N, M)
    env.set_scenarios(a6, scen.POLICY_RVO, scen.DYN_UNICYCLE, heading0=heading0, coop=np.full((N, M), 0.25), obstacles=obst, n_obst=n_obst)
    env.reset()
    for _ in range(5):
        env.step()
    _fill_stats(env)
    return env


def _fill_stats(env):
    """the per-world statistics are plain accumulators, all zeros until an episode ends: give every word its own value"""
    import torch
    s = env.state()
    for j, k in enumerate(("stat_return", "stat_episodes", "stat_steps", "stat_outcomes")):
        s[k].copy_((torch.arange(s[k].numel(), device=env.device) + 10 * j + 1).reshape(s[k].shape).to(s[k].dtype))


def _state_views(env, ig_views=None):
    v = {k: t for k, t in env.state().items() if k != "map_bits"}
    v.update(ig_views or {})
    return v


def _pool_views(env):
    p = dict(env.scenarios())
    if env.Kobs:
        p.update(env.obstacles())
    return p


def _check_snapshot(env, ig_views=None):
    import torch
    fields = _state_fields(env.M, ig_views is not None)
    L = env.snapshot_layout()
    assert L.row_bytes == _offsets(fields, 16)[1] and L.row_bytes % 16 == 0
    assert L.fields == (3 if ig_views is not None else 1)
    ids = list(range(env.N))[::-1][:max(env.N - 1, 1)]  # not the identity, not every world
    snap = env.snapshot(ids)
    torch.cuda.synchronize()
    _check_rows(snap.blob, fields, _state_views(env, ig_views), SNAP_MAGIC, ids, "snapshot")


def _check_checkpoint(env, stream=None, log=None, replay=None):
    """every entry of cagym_checkpoint_sizes and every viewed byte of the blob; returns the sizes"""
    import torch
    N, M, S, K = env.N, env.M, env.S, env.Kobs
    state, pool = _state_fields(M, False), _pool_fields(M, K)
    flat = [_stream_fields(N) if stream else [], _log_fields(N, M, log["capacity"]) if log else [],
            _replay_fields(S, replay["capacity"]) if replay else []]
    want = [HOST_BYTES, N * _offsets(state, 16)[1], S * _offsets(pool, 16)[1]] + [_offsets(f, 0)[1] for f in flat]
    sizes = (C.c_uint64 * 6)()
    lib.call(env.L, env.h, "cagym_checkpoint_sizes", sizes)
    assert [int(s) for s in sizes] == want
    ck = env.checkpoint()
    torch.cuda.synchronize()
    assert ck.sizes == want and ck.header.numel() == HOST_BYTES and ck.blob.numel() == sum(want[1:])
    at = np.cumsum([0] + want[1:])
    sec = [ck.blob[int(at[k]):int(at[k + 1])] for k in range(5)]
    _check_rows(sec[0].reshape(N, -1), state, _state_views(env), SNAP_MAGIC, list(range(N)), "checkpoint state")
    _check_rows(sec[1].reshape(S, -1), pool, _pool_views(env), POOL_ROW_MAGIC, list(range(S)), "checkpoint pool")
    if K:
        assert _offsets(pool, 16)[1] < RASTER_BYTES  # no raster in a row
    for k, views, what in ((0, stream, "stream"), (1, log, "log"), (2, replay, "replay")):
        if views:
            _check_flat(sec[2 + k], flat[k], views, "checkpoint " + what)
    return want


def test_free_space_rows():
    env = _fixed_pool_env(3, 2, 0)
    _check_snapshot(env)
    want = _check_checkpoint(env)
    assert want[3:] == [0, 0, 0]
    env.close()


def test_rectangles_ig_tail_and_fork():
    import torch
    env = _fixed_pool_env(5, 4, 2)
    _check_snapshot(env)
    _check_checkpoint(env)
    # fork: dst keeps its episode index and statistics, every other viewed field is src's
    before = {k: v.clone() for k, v in _state_views(env).items()}
    env.fork([1], [3])
    for k, v in _state_views(env).items():
        assert torch.equal(v[3], before[k][3 if k in KEPT_BY_FORK_DST else 1]), k
        rest = [0, 1, 2, 4]
        assert torch.equal(v[rest], before[k][rest]), k
    # after cagym_ig_init a row also carries the belief, its MI cache and the team accumulators
    lib.call(env.L, env.h, "cagym_ig_init", env._stream())
    ig = {k: v for k, v in env._address_views("cagym_ig_get", lib.IG_FIELDS).items() if k == "belief"}
    ig.update(env._address_views("cagym_ig_get_episode_stats", lib.IG_EPISODE_FIELDS))
    ig["belief"].copy_(torch.rand(ig["belief"].shape, dtype=torch.float64, device=env.device))
    for j, k in enumerate(("running", "sum", "last", "episodes")):
        ig[k].copy_((torch.arange(env.N, device=env.device) + 7 * j + 1).to(ig[k].dtype))
    _check_snapshot(env, ig)
    env.close()


def test_stream_log_and_replay_sections():
    import torch
    N, M, DEPTH, LOG, Q = 3, 2, 2, 7, 5
    env = benv.BatchedCollisionAvoidanceEnv(N, M, n_scenarios=DEPTH * N, game_over_mode="agent0")
    args = dict(kinds="train_agents_swap_circle", seed=11, number_of_agents=2, fixed_count=True, ego_policy=scen.POLICY_NONCOOP,
                ego_dynamics=scen.DYN_UNICYCLE, other_policies=scen.POLICY_NONCOOP)
    assert env.stream_reference_scenarios(**args) == 0
    env.reset()
    env.attach_episode_log(LOG)
    env.attach_replay(capacity=Q, p=0.5, outcomes=("collision", "stuck", "goal"), seed=3)
    for _ in range(6):
        env.rollout(32, auto_reset=True)
    _fill_stats(env)
    env.stream_stats()
    sv = env._stream_views
    words = torch.cat([sv["generated"].view(torch.uint8), sv["n_failed"].view(torch.uint8), sv["n_lapped"].view(torch.uint8)])
    assert sv["n_failed"].data_ptr() == sv["generated"].data_ptr() + 8 and sv["n_lapped"].data_ptr() == sv["generated"].data_ptr() + 12
    log, rep = env.episode_log_views(), env.replay_views()
    # the replay's word view shows the six counters; the seventh word of the field is the harvest cursor
    rep7 = lib.views({"words": rep["words"].data_ptr()}, [("words", "u8", "7")], env.device)
    rep = dict(rep, words=rep7["words"], capacity=Q)
    head = int(log["head"].item())
    assert head > LOG and int(rep["words"][0].item()) > Q, "both rings have wrapped"  # rows logged, keys appended
    _check_checkpoint(env, stream={"words": words, "next_episode": sv["next_episode"]}, log=dict(log, capacity=LOG), replay=rep)
    env.close()
