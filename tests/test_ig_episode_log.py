"""GPU: the IG team's episode log (csrc/cagym_ig_episode_log.h, attach_ig_episode_log) - one row per finished team episode with the
belief's entropy, the MI left, the touched cells and the step at which each target was localised.

The rows are held to ig.episode_log_spec on beliefs the test cloned before each step (learner flow), to a found_at the test names
in advance on a hand-made pool, to a second policy's log of the same actions (an episodic ig_greedy handle and a learner fed its
action table hold equal logs, bit for bit), to the same handle stepped through rollout(), and to the ring's and the contract's
edges.  Shapes of tests/test_refusals.py: 4 worlds x 4 agents (2 robots, 2 targets), 8 scenarios, max_obstacles=4 - the smallest
at which two robots share a belief and a world's ring of slots has two entries - on stream_exploration_worlds with
robot_pref_speed=30, so that episodes time out within a few steps."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
igm = importlib.import_module("gym-exploration-2d_amd.ig")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
N, M, S = 4, 4, 8
E_INVALID, E_STATE = -1, -5
ODDS = 0.75 / (1.0 - 0.75)  # what attach_ig_episode_log(p_found=0.75) hands the library
STREAM = dict(kinds="train_stage_1", n_robots=2, n_targets=2, n_obst=(1, 4), robot_pref_speed=30.0)
SEED = 21
# Test 1's stream and action seed and its action ranges, chosen on the device so that its three non-emptiness conditions hold: with
# omega within +-1 rad/s the robots hardly turn in the 12 to 16 steps of an episode, and none of 12 seeds localised a target in 60
# steps; within +-10 rad/s (up to a radian per step: the robots look around) every one of the 12 did, seed 3 in 5 of its 17 episodes
# (one of them both targets), and left a target unfound in 16.
SPEC_SEED, SPEC_V_MAX, SPEC_W_MAX = 3, 4.0, 10.0
COLUMNS = [f[0] for f in _lib.IGLOG_FIELDS if f[2] in ("L", "LM")]
CONTRACT = ("%s(auto_reset=False) with an IG episode log attached: cagym_ig_episode_log_update goes behind the auto-resetting step "
            "only, every step exactly once and in order (include/cagym.h); detach_ig_episode_log() first")
LIBRARY = "%s with an IG episode log initialised: its running values would describe another timeline"


def _B():
    return importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv


def _stream_env(seed=SEED):
    env = _B()(N, M, n_scenarios=S, max_obstacles=4, game_over_mode="agent0")
    assert env.stream_exploration_worlds(seed=seed, **STREAM) == 0
    env.reset()
    return env


def _actions(env, rng, v_max=3.0, w_max=1.0):
    import torch
    a = np.stack([rng.uniform(0.0, v_max, (N, M)), rng.uniform(-w_max, w_max, (N, M))], axis=-1).astype(np.float32)
    return torch.as_tensor(a, device=env.device)


def _equal_logs(a, b):
    import torch
    assert sorted(a) == sorted(b) == sorted(COLUMNS)
    for k in COLUMNS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ---- 1. the learner's log against the numpy specification --------------------------------------------------------------------------
def learner_against_spec(seed, steps=60, v_max=3.0, w_max=1.0):
    """The run of test 1 for one seed (the stream's and the actions'): returns (rows of the log, the rows the host expects, the
    `last` the handle held behind each finishing step).  The host keeps its own steps_run / found_run: before each step it clones
    the beliefs and reads the targets of each world's pool slot, which the refill behind the step may regenerate."""
    import torch
    env = _stream_env(seed)
    ig = env.attach_ig_learner(window=4)
    env.attach_ig_episode_log(capacity=256)
    env.reset()
    rng = np.random.default_rng(seed)
    sc = env.scenarios()
    steps_run, found_run = np.zeros(N, dtype=np.int64), np.full((N, M), -1, dtype=np.int64)
    want, lasts = [], []
    for t in range(steps):
        bel = ig.belief.cpu().numpy()
        ep = env.state()["episode"].cpu().numpy().astype(np.int64)
        slot = (np.arange(N) + ep * N) % S
        a6, pol, na = sc["agents6"].cpu().numpy()[slot], sc["policy"].cpu().numpy()[slot], sc["n_agents"].cpu().numpy()[slot]
        _, _, go, _ = env.step(_actions(env, rng, v_max, w_max), auto_reset=True)
        over = go.cpu().numpy().astype(bool)
        last = env.ig_episode_stats()["last"].cpu().numpy().copy()
        for w in range(N):
            steps_run[w] += 1
            target = (pol[w] == scen.POLICY_STATIC) & (np.arange(M) < na[w])
            spec = igm.episode_log_spec(bel[w], a6[w, :, 0:2], ODDS)
            newly = target & (found_run[w] < 0) & spec["found"]
            found_run[w, newly] = steps_run[w]
            if over[w]:
                want.append({"key": (w + int(ep[w]) * N) & 0xFFFFFFFF, "world": w, "episode": int(ep[w]), "slice": t, "steps": int(steps_run[w]),
                             "n_targets": int(target.sum()), "n_found": int((target & (found_run[w] >= 0)).sum()),
                             "found_at": np.where(target, found_run[w], -2), "n_touched": spec["n_touched"],
                             "entropy": spec["entropy"], "residual_mi": spec["residual_mi"]})
                lasts.append(last[w])
                steps_run[w], found_run[w] = 0, -1
    rows = {k: v.cpu() for k, v in env.ig_episode_log().items()}
    env.close()
    return rows, want, lasts


def test_learner_rows_equal_the_specification():
    """60 auto-resetting steps with seeded random (v, omega) in [0, 4] x [-10, 10].  key, world, episode, slice, steps, n_targets, n_found, found_at and
    n_touched are equal exactly, ret is the handle's `last` bit for bit, entropy and residual_mi agree within relative 1e-11: at
    most 3600 terms, each within a few ulp of numpy's (the logarithms differ in the last bits, the order of the sums differs), so
    the sums differ by at most 3600 * 4 * 2^-53 = 1.6e-12 relative, with a margin of six."""
    import torch
    rows, want, lasts = learner_against_spec(SPEC_SEED, v_max=SPEC_V_MAX, w_max=SPEC_W_MAX)
    n = len(want)
    found_rows = sum(1 for r in want if r["n_found"] > 0)
    unfound_rows = sum(1 for r in want if r["n_found"] < r["n_targets"])
    print("episodes %d, rows with a found target %d, with an unfound target %d" % (n, found_rows, unfound_rows))
    assert n >= 8 and found_rows >= 1 and unfound_rows >= 1  # the test cannot pass emptily
    assert rows["key"].shape == (n,) and rows["found_at"].shape == (n, M)
    for k in ("key", "world", "episode", "slice", "steps", "n_targets", "n_found", "n_touched"):
        assert rows[k].tolist() == [r[k] for r in want], k
    assert np.array_equal(rows["found_at"].numpy(), np.stack([r["found_at"] for r in want]))
    assert torch.equal(rows["ret"], torch.tensor(lasts, dtype=torch.float64))
    for k in ("entropy", "residual_mi"):
        got, ref = rows[k].numpy(), np.array([r[k] for r in want])
        err = np.abs(got - ref) / np.abs(ref)
        print("%s: largest relative difference %.3g" % (k, err.max()))
        assert (err <= 1e-11).all(), k
    assert (rows["n_targets"] == 2).all() and (rows["found_at"][:, :2] == -2).all()  # slots 0 and 1 are the robots


# ---- 2. a found_at named in advance ------------------------------------------------------------------------------------------------
def test_found_at_of_a_target_straight_ahead():
    """A fixed pool of one scenario: robot 0 at the origin facing its goal at (10, 0), robot 1 out of everyone's range, a target on
    the centre of belief cell (34, 30), 2.25 m ahead of robot 0 and inside its cone, another 2.75 m behind it (detected - the
    detector has no cone - but its cell is never visible, so never updated), one rectangle far from everything.  The learner feeds
    zero actions, so robot 0 stays, and its pref_speed of 18.5 gives it 3 (10 - 0.75) / 18.5 = 1.5 s.  Every update multiplies
    the odds of the target's cell by 1.5 (rOcc), and behind step k the log sees k updates: 1.5, 2.25, 3.375 >= 3 -> found_at 3."""
    import torch
    a6 = np.zeros((S, M, 6))
    a6[:, 0] = [0, 0, 10, 0, 18.5, .5]
    a6[:, 1] = [12.25, 12.25, 12.25, 14, 1.0, .5]
    a6[:, 2] = [2.25, 0.25, 0, 0, 1.0, .2]
    a6[:, 3] = [-2.75, 0.25, 0, 0, 1.0, .2]
    pol = np.full((S, M), scen.POLICY_STATIC, dtype=np.int32)
    pol[:, :2] = scen.POLICY_IGMCTS
    h0 = np.zeros((S, M))
    h0[:, 1] = np.pi / 2
    env = _B()(N, M, n_scenarios=S, max_obstacles=4, game_over_mode="agent0")
    env.set_scenarios(a6, pol, scen.DYN_FIRSTORDER, heading0=h0, n_agents=[M] * S, obstacles=np.array([[(-13, -13, -11, -11)]] * S, dtype=np.float64),
                      n_obst=[1] * S)
    env.reset()
    ig = env.attach_ig_learner(window=4)
    env.attach_ig_episode_log(capacity=16, p_found=0.75)
    env.reset()
    zero = torch.zeros((N, M, 2), dtype=torch.float32, device=env.device)
    ended, cell = None, []
    for t in range(1, 25):
        cell.append(float(ig.belief[0, 30, 34].item()))  # what the log sees behind step t
        _, _, go, _ = env.step(zero, auto_reset=True)
        if go.any().item():
            assert go.all().item()
            ended = t
            break
    assert cell[:4] == [1.5, 1.5 ** 2, 1.5 ** 3, 1.5 ** 4]
    assert ended is not None and 10 <= ended <= 20
    rows = env.ig_episode_log()
    assert rows["world"].tolist() == [0, 1, 2, 3] and rows["episode"].tolist() == [0] * N and rows["key"].tolist() == [0, 1, 2, 3]
    assert rows["steps"].tolist() == [ended] * N and rows["slice"].tolist() == [ended - 1] * N
    assert rows["found_at"].tolist() == [[-2, -2, 3, -1]] * N
    assert rows["n_targets"].tolist() == [2] * N and rows["n_found"].tolist() == [1] * N
    assert torch.equal(rows["ret"], env.ig_episode_stats()["last"])
    for k in ("entropy", "residual_mi", "n_touched"):  # four worlds on one belief: equal sums, bit for bit
        assert (rows[k] == rows[k][0]).all(), k
    assert 0 < int(rows["n_touched"][0]) < 3600 and float(rows["entropy"][0]) < 3600 * np.log(2)
    env.close()


# ---- 3. two policies, one log ------------------------------------------------------------------------------------------------------
def test_planner_and_learner_hold_equal_logs():
    """G: attach_ig_greedy(episodic=True).  L: attach_ig_learner fed, each step, the action table G's step read (as
    tests/test_ig_learner.py does).  Behind step k of an episode both beliefs hold the same k updates, and the planners' chain
    hands the log the terminal reward the boundary adds: the two logs are equal row for row and column for column, entropy
    included, and ret is each handle's `last`."""
    import torch
    g, L = _stream_env(), _stream_env()
    g.attach_ig_greedy(episodic=True)
    L.attach_ig_learner(window=4)
    for e in (g, L):
        e.attach_ig_episode_log(capacity=256)
        e.reset()
    lasts = {id(g): [], id(L): []}
    for t in range(40):
        g.step(None, auto_reset=True)
        L.step(g._act.clone(), auto_reset=True)
        assert torch.equal(L.game_over, g.game_over), t
        for e in (g, L):
            lasts[id(e)].append(e.ig_episode_stats()["last"][e.game_over.bool()].clone())
    rg, rl = g.ig_episode_log(), L.ig_episode_log()
    _equal_logs(rg, rl)
    assert rg["key"].numel() >= 8 and (rg["ret"] > 0).all()
    for e, rows in ((g, rg), (L, rl)):
        assert torch.equal(rows["ret"], torch.cat(lasts[id(e)]))
    g.close()
    L.close()


# ---- 4. rollout() feeds it ---------------------------------------------------------------------------------------------------------
def test_rollout_feeds_the_log_like_steps():
    """An episodic ig_greedy handle run by 12 x rollout(2) and its twin by 24 x step(auto_reset=True): equal logs.  Two steps per
    launch, so that no world finishes two episodes inside one (the ring holds two slots per world): n_lapped == 0 is asserted."""
    import torch
    a, b = _stream_env(), _stream_env()
    for e in (a, b):
        e.attach_ig_greedy(episodic=True)
        e.attach_ig_episode_log(capacity=256)
        e.reset()
    for _ in range(12):
        a.rollout(2, auto_reset=True)
        for _ in range(2):
            b.step(None, auto_reset=True)
    assert a.stream_stats()["n_lapped"] == 0 and b.stream_stats()["n_lapped"] == 0
    ra, rb = a.ig_episode_log(), b.ig_episode_log()
    _equal_logs(ra, rb)
    assert ra["key"].numel() >= 4 and int(ra["slice"].max()) < 24
    assert torch.equal(ra["slice"], torch.sort(ra["slice"], stable=True)[0])  # appended in call order
    a.close()
    b.close()


# ---- 5. ring and contract ----------------------------------------------------------------------------------------------------------
def test_ring_of_four_rows_keeps_the_newest():
    import torch
    small, big = _stream_env(), _stream_env()
    for e, cap in ((small, 4), (big, 256)):
        e.attach_ig_learner(window=4)
        e.attach_ig_episode_log(capacity=cap)
        e.reset()
    rng_s, rng_b = np.random.default_rng(3), np.random.default_rng(3)
    for t in range(40):
        small.step(_actions(small, rng_s), auto_reset=True)
        big.step(_actions(big, rng_b), auto_reset=True)
    v = small.ig_episode_log_views()
    head = int(v["head"].item())
    assert head > 4 and v["key"].shape == (4,) and v["found_at"].shape == (4, M) and v["found_run"].shape == (N, M)
    all_rows = big.ig_episode_log()
    assert all_rows["key"].numel() == head
    _equal_logs(small.ig_episode_log(), {k: t_[-4:] for k, t_ in all_rows.items()})
    _equal_logs(small.ig_episode_log(last=2), {k: t_[-2:] for k, t_ in all_rows.items()})
    _equal_logs(big.ig_episode_log(last=3), {k: t_[-3:] for k, t_ in all_rows.items()})
    assert (all_rows["key"] >= 0).all() and all_rows["key"].dtype == torch.int64
    # reset(world_mask=m): the masked worlds' running values start anew, the others' stay
    for _ in range(20):  # until every world is in mid-episode (a step or two)
        if (small.ig_episode_log_views()["steps_run"] > 0).all().item():
            break
        small.step(_actions(small, rng_s), auto_reset=True)
    assert (small.ig_episode_log_views()["steps_run"] > 0).all().item()
    before = {k: small.ig_episode_log_views()[k].clone() for k in ("steps_run", "found_run", "cursor")}
    head = int(small.ig_episode_log_views()["head"].item())
    m = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=small.device)
    small.reset(world_mask=m)
    after = small.ig_episode_log_views()
    keep = ~m.bool()
    assert (after["steps_run"][m.bool()] == 0).all() and (after["found_run"][m.bool()] == -1).all()
    assert torch.equal(after["steps_run"][keep], before["steps_run"][keep]) and torch.equal(after["found_run"][keep], before["found_run"][keep])
    assert torch.equal(after["cursor"], small.state()["episode"]) and int(after["head"].item()) == head  # rows kept
    small.step(_actions(small, rng_s), auto_reset=True)
    small.ig_episode_log()  # in step: no desync
    small.clear_ig_episode_log()
    assert int(small.ig_episode_log_views()["head"].item()) == 0 and small.ig_episode_log()["key"].numel() == 0
    assert (small.ig_episode_log_views()["steps_run"] == 0).all()
    small.close()
    big.close()


def test_attach_needs_a_team_that_restarts_per_world():
    env = _stream_env()
    with pytest.raises(RuntimeError, match="needs an IG attach that restarts per world"):
        env.attach_ig_episode_log()
    with pytest.raises(RuntimeError, match="without an IG episode log: attach_ig_episode_log\\(\\) first"):
        env.ig_episode_log()
    env.attach_ig_greedy()  # episodic=False
    with pytest.raises(RuntimeError, match="needs an IG attach that restarts per world"):
        env.attach_ig_episode_log()
    assert env._iglog is None
    with pytest.raises(ValueError, match="capacity must be >= 1"):
        env.attach_ig_episode_log(capacity=0)
    with pytest.raises(ValueError, match="p_found must lie inside"):
        env.attach_ig_episode_log(p_found=1.0)
    env.attach_ig_greedy(episodic=True)
    env.attach_ig_episode_log(capacity=8)
    env.attach_ig_learner(window=4)  # one IG attach replaces another: the log stays attached
    assert env._iglog == 8
    env.reset()
    for what, call in (("step", lambda: env.step(auto_reset=False)), ("rollout", lambda: env.rollout(2, auto_reset=False))):
        with pytest.raises(RuntimeError) as ei:
            call()
        assert str(ei.value) == CONTRACT % what
    env.step(None, auto_reset=True)
    env.ig_episode_log()
    env.detach_ig_episode_log()
    env.step(None, auto_reset=False)  # nothing refuses any more
    env.close()


def test_the_library_refuses_and_counts_desync():
    """Raw calls: the four entries before cagym_ig_init and before init, init's arguments, a doubled update (desync), and
    cagym_restore / cagym_fork with the log initialised - after each the handle still steps."""
    import torch
    env = _B()(N, M, n_scenarios=S, max_obstacles=4, game_over_mode="agent0")
    assert env.generate_exploration_worlds(seed=SEED, **STREAM) == 0  # a fixed pool: restore and fork get past the stream's refusal
    env.reset()
    Lb, h, st = env.L, env.h, env._stream()
    ptrs = _lib.CagymIgEpisodeLogPtrs()
    go = env.game_over.data_ptr()
    err = lambda: Lb.cagym_last_error(h).decode()
    calls = {"init": lambda: Lb.cagym_ig_episode_log_init(h, 8, ODDS, st), "update": lambda: Lb.cagym_ig_episode_log_update(h, go, None, st),
             "restart": lambda: Lb.cagym_ig_episode_log_restart(h, None, 0, st), "get": lambda: Lb.cagym_ig_episode_log_get(h, C.byref(ptrs))}
    for name, call in calls.items():
        assert call() == E_STATE and err() == "cagym_ig_episode_log_%s before cagym_ig_init" % name
    env.attach_ig_learner(window=4)
    for name in ("update", "restart", "get"):
        assert calls[name]() == E_STATE and err() == "cagym_ig_episode_log_%s before cagym_ig_episode_log_init" % name
    for cap, odds in ((0, ODDS), (-3, ODDS), (8, 0.0), (8, -1.0), (8, float("nan")), (8, float("inf"))):
        assert Lb.cagym_ig_episode_log_init(h, cap, odds, st) == E_INVALID, (cap, odds)
    assert calls["update"]() == E_STATE  # a refused init initialised nothing
    env.attach_ig_episode_log(capacity=8)
    env.reset()
    assert Lb.cagym_ig_episode_log_update(h, None, None, st) == E_INVALID and Lb.cagym_ig_episode_log_get(h, None) == E_INVALID
    # restore and fork: every argument valid, refused for the log alone
    snap = env.snapshot()
    ids = torch.tensor([0, 1], dtype=torch.int32, device=env.device)
    assert Lb.cagym_restore(h, C.byref(snap.layout), snap.blob.data_ptr(), None, snap.n, st) == E_STATE and err() == LIBRARY % "cagym_restore"
    env.step(None, auto_reset=True)
    assert Lb.cagym_fork(h, ids[:1].data_ptr(), ids[1:].data_ptr(), 1, st) == E_STATE and err() == LIBRARY % "cagym_fork"
    # a doubled update of a step that finished a world
    rng = np.random.default_rng(5)
    for t in range(40):
        _, _, over, _ = env.step(_actions(env, rng), auto_reset=True)
        if over.any().item():
            break
    finished = int(over.sum().item())
    assert finished > 0
    rows = env.ig_episode_log()  # in step so far
    assert calls["update"]() == 0
    with pytest.raises(RuntimeError, match="IG episode log is out of step with the env in %d world-launches" % finished):
        env.ig_episode_log()
    again = env.ig_episode_log(check=False)
    _equal_logs(rows, again)  # the doubled update logged nothing
    assert int(env.ig_episode_log_views()["desync"].item()) == finished
    env.step(None, auto_reset=True)
    env.attach_ig_episode_log(capacity=8)  # attaching again clears
    assert int(env.ig_episode_log_views()["desync"].item()) == 0 and env.ig_episode_log()["key"].numel() == 0
    env.close()
