"""Multi-GPU: worlds are independent, so ranks shard them with no data-path exchange.  The single
collective is an all-gather of the per-world episode statistics (24 B/world) over RCCL
(torch.distributed backend "nccl" on ROCm; "gloo" in the CPU tests).  The reference has no
counterpart (single process); its per-episode statistics are those of
experiments/src/env_utils.py:41-75 (return, steps, outcome flags of the previous episode).

Record per world: {f32 return_sum, i32 episodes, i32 steps, i32 n_goal, i32 n_collision, i32 n_timeout}
carried as six 32-bit words (the return's bit pattern in word 0), so the counters stay exact however long
the run is (fp32 would lose exactness past 2^24).
"""
import torch

RECORD_WORDS = 6


def shard_worlds(total_worlds, rank, world_size):
    """Contiguous block partition of `total_worlds` (first ranks take the remainder)."""
    base, rem = divmod(int(total_worlds), int(world_size))
    count = base + (1 if rank < rem else 0)
    start = rank * base + min(rank, rem)
    return start, count


def pack_episode_stats(stats):
    """[N, 6] int32 records (word 0 = bit pattern of the fp32 return sum)."""
    ret = stats["stat_return"].float().contiguous().view(torch.int32)
    out = stats["stat_outcomes"].to(torch.int32)
    cols = [ret, stats["stat_episodes"].to(torch.int32), stats["stat_steps"].to(torch.int32), out[:, 0], out[:, 1], out[:, 2]]
    return torch.stack(cols, dim=1).contiguous()


def all_gather_episode_stats(local, group=None, total_worlds=None):
    """all-gather [N_local, 6] -> [sum of N_local, 6].  Shards may differ by one world (shard_worlds): every rank pads
    to ceil(total / world_size) rows for the one equal-size collective and the padding is trimmed afterwards.
    total_worlds = None means equal shards."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized():
        return local
    ws = dist.get_world_size(group)
    n_local = int(local.shape[0])
    if total_worlds is None:
        rows, counts = n_local, [n_local] * ws
    else:
        rows = -(-int(total_worlds) // ws)
        counts = [shard_worlds(total_worlds, r, ws)[1] for r in range(ws)]
        if counts[dist.get_rank(group)] != n_local:
            raise ValueError("rank holds %d worlds, shard_worlds(%d, rank, %d) says %d"
                             % (n_local, total_worlds, ws, counts[dist.get_rank(group)]))
    send = local.contiguous()
    if rows != n_local:
        send = torch.zeros((rows,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        send[:n_local] = local
    out = torch.empty((ws * rows,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, send, group=group)
    if all(c == rows for c in counts):
        return out
    return torch.cat([out[r * rows:r * rows + counts[r]] for r in range(ws)], dim=0)


def unpack_episode_stats(packed):
    """[n, 6] int32 records -> dict of exact columns (return as float64)."""
    p = packed.contiguous()
    return {"return_sum": p[:, 0].contiguous().view(torch.float32).double(), "episodes": p[:, 1].long(), "steps": p[:, 2].long(),
            "n_goal": p[:, 3].long(), "n_collision": p[:, 4].long(), "n_timeout": p[:, 5].long()}


def summarize(gathered):
    u = unpack_episode_stats(gathered)
    eps_n = int(u["episodes"].sum())
    eps = max(float(eps_n), 1.0)
    goal, coll, tout = int(u["n_goal"].sum()), int(u["n_collision"].sum()), int(u["n_timeout"].sum())
    agents = max(float(goal + coll + tout), 1.0)
    return {"episodes": float(eps_n), "mean_return": float(u["return_sum"].sum()) / eps,
            "mean_steps": float(int(u["steps"].sum())) / eps, "frac_goal": goal / agents,
            "frac_collision": coll / agents, "frac_timeout": tout / agents}


# ---- the reference's test-suite table from per-scenario episode records (env.episode_records()) ------------------------------------
OUTCOME_COLLISION, OUTCOME_ALL_AT_GOAL, OUTCOME_STUCK = 1, 2, 4  # bits of the records' outcome column (env_utils.py:55-60)


def suite_statistics(records, first=0, count=None, include=None):
    """What experiments/src/process_full_test_suite_pickles.py:90-116 prints for one policy, from the table of
    BatchedCollisionAvoidanceEnv.episode_records() (torch tensors, on the device they live on), over the scenarios
    first .. first + count - 1 (default: to the end of the pool):
      n_cases, n_run (rows with count > 0);
      pct_collision (any agent in collision), pct_stuck (no collision and not all at goal, env_utils.py:72-74), in percent of
        n_cases as the reference counts them;
      clean [n_cases] bool: run, no collision, all at goal - the rows the reference intersects across policies;
      extra_time_pctls: the 50 / 75 / 90th percentiles (np.percentile's default, linear interpolation) of the per-case mean of
        extra_t over the case's active agents (slots < n_agents; every slot when the records carry no n_agents), taken over the
        rows of `include` (a [n_cases] bool mask, e.g. the intersection of several policies' clean rows; default: this
        table's clean rows).  NaN when no row is included.
    A window of the append-only episode log works unchanged: BatchedCollisionAvoidanceEnv.episode_log(last=K) carries count (ones)
    and n_agents per row, so every row is a case that ran (collision rate over the last K episodes)."""
    cnt = records["count"]
    S = int(cnt.shape[0])
    first = int(first)
    last = S if count is None else first + int(count)
    if not (0 <= first < last <= S):
        raise ValueError("suite_statistics: cases %d..%d outside the pool of %d scenarios" % (first, last, S))
    sl = slice(first, last)
    cnt, outcome, extra = cnt[sl], records["outcome"][sl], records["extra_t"][sl]
    n_cases = last - first
    run = cnt > 0
    coll = run & ((outcome & OUTCOME_COLLISION) != 0)
    goal = (outcome & OUTCOME_ALL_AT_GOAL) != 0
    stuck = run & ~coll & ~goal
    clean = run & ~coll & goal
    M = int(extra.shape[1])
    if records.get("n_agents") is not None:
        n = records["n_agents"][sl].to(torch.int64)
    else:
        n = torch.full((n_cases,), M, dtype=torch.int64, device=extra.device)
    live = torch.arange(M, device=extra.device)[None, :] < n[:, None]
    mean_extra = (extra * live).sum(dim=1) / n.clamp(min=1).to(extra.dtype)
    inc = clean if include is None else torch.as_tensor(include, device=extra.device).to(torch.bool).reshape(n_cases)
    vals = mean_extra[inc]
    q = torch.tensor([0.5, 0.75, 0.9], dtype=extra.dtype, device=extra.device)
    pct = torch.quantile(vals, q, interpolation="linear") if vals.numel() else torch.full((3,), float("nan"), dtype=extra.dtype,
                                                                                         device=extra.device)
    return {"n_cases": n_cases, "n_run": int(run.sum()), "pct_collision": 100.0 * float(coll.sum()) / n_cases,
            "pct_stuck": 100.0 * float(stuck.sum()) / n_cases, "clean": clean, "extra_time_pctls": pct}


# ---- a target search's table from the IG team's episode log (env.ig_episode_log()) --------------------------------------------------
BELIEF_CELLS = 3600  # the 60 x 60 belief grid of a world


def exploration_statistics(rows):
    """One policy's summary of BatchedCollisionAvoidanceEnv.ig_episode_log() (torch tensors, on the device they live on; every row
    is a finished team episode):
      episodes; mean_return, median_return of `ret`;
      found_share = sum(n_found) / sum(n_targets) (NaN when the log holds no target);
      all_found_share: the share of episodes that found every one of their targets;
      found_at_pctls: the 50 / 75 / 90th percentiles (linear interpolation) of found_at over the found targets, in steps (NaN
        when nothing was found);
      mean_entropy (nats) and mean_touched = mean of n_touched / 3600, of the beliefs the episodes ended on.
    An empty log gives episodes 0 and NaN everywhere else."""
    ret = torch.as_tensor(rows["ret"]).to(torch.float64)
    n = int(ret.shape[0])
    nan = float("nan")
    dev = ret.device
    fa = torch.as_tensor(rows["found_at"]).to(dev)
    found = fa[fa >= 0].to(torch.float64)
    q = torch.tensor([0.5, 0.75, 0.9], dtype=torch.float64, device=dev)
    pct = torch.quantile(found, q, interpolation="linear") if found.numel() else torch.full((3,), nan, dtype=torch.float64, device=dev)
    if n == 0:
        return {"episodes": 0, "mean_return": nan, "median_return": nan, "found_share": nan, "all_found_share": nan,
                "found_at_pctls": pct, "mean_entropy": nan, "mean_touched": nan}
    n_t, n_f = torch.as_tensor(rows["n_targets"]).to(torch.int64), torch.as_tensor(rows["n_found"]).to(torch.int64)
    targets = int(n_t.sum())
    return {"episodes": n, "mean_return": float(ret.mean()), "median_return": float(torch.quantile(ret, 0.5, interpolation="linear")),
            "found_share": float(n_f.sum()) / targets if targets else nan, "all_found_share": float((n_f == n_t).sum()) / n,
            "found_at_pctls": pct, "mean_entropy": float(torch.as_tensor(rows["entropy"]).to(torch.float64).mean()),
            "mean_touched": float(torch.as_tensor(rows["n_touched"]).to(torch.float64).mean()) / BELIEF_CELLS}


def paired_by_key(a, b):
    """The inner join of two episode logs on `key`: (ia, ib), two int64 index tensors of equal length with a["key"][ia] ==
    b["key"][ib], ordered by key.  Two handles on one stream seed meet the same world under the same key whatever drives them, so
    a["ret"][ia] - b["ret"][ib] is the paired return difference, episode by episode.  A key that a log holds more than once (a ring
    that wrapped past 2^32 episodes) is paired by its first row."""
    ka, kb = torch.as_tensor(a["key"]).to(torch.int64), torch.as_tensor(b["key"]).to(torch.int64).to(torch.as_tensor(a["key"]).device)
    sa, oa = torch.sort(ka, stable=True)
    sb, ob = torch.sort(kb, stable=True)
    first_a = torch.ones_like(sa, dtype=torch.bool)
    first_a[1:] = sa[1:] != sa[:-1]
    sa, oa = sa[first_a], oa[first_a]
    first_b = torch.ones_like(sb, dtype=torch.bool)
    first_b[1:] = sb[1:] != sb[:-1]
    sb, ob = sb[first_b], ob[first_b]
    if sa.numel() == 0 or sb.numel() == 0:
        e = torch.zeros((0,), dtype=torch.int64, device=ka.device)
        return e, e.clone()
    at = torch.searchsorted(sb, sa).clamp(max=sb.numel() - 1)
    hit = sb[at] == sa
    return oa[hit], ob[at[hit]]
