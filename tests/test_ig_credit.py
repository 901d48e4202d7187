"""GPU: cagym_ig_credit (csrc/cagym_ig_credit.h), its binding InfoGain.robot_credit, attach_ig_credit and CagymRobotVecEnv.

Device against device, bit for bit: every robot's mask against cagym_ig_visible_cells of its pose, their union against the observe
launch's, own and exclusive against cagym_ig_mi_reward of the masks, the gain against observe's, difference against gain - loo.
The leave-one-out sum against ig.robot_credit_spec on the belief and the MI cache read back (1e-12 max(1, |x|), the bound
tests/test_hip_ig.py holds rewards to against the oracle).  6 worlds, window 4; placed poses (the worlds of
tests/test_ig_credit_spec.py): one pose twice, back to back, a target both robots detect, a target in both cones that one detector
reaches, no detection, a general pair; the pool of tests/test_ig_learner.py cut to 6 worlds for the episodes."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_ig_learner import OBST, OBST2, _B

pytestmark = pytest.mark.gpu
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
igm = importlib.import_module("gym-exploration-2d_amd.ig")
vec = importlib.import_module("gym-exploration-2d_amd.vecenv")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
N, M, G = 6, 10, 4
E_INVALID, E_STATE = -1, -5
PI = np.pi
# (robot 0, robot 1, the target) of world w; further robots come from FILL
PLACED = [((-5.0, 0.3, 0.2), (-5.0, 0.3, 0.2), (-2.6, 0.9)),      # 0: one pose twice
          ((0.3, -0.4, 0.0), (0.3, -0.4, PI), (2.4, -0.2)),       # 1: back to back
          ((-6.0, 0.0, 0.0), (-5.2, 0.9, -0.3), (-3.1, 0.2)),     # 2: overlapping cones, both detect the target
          ((-8.0, 0.2, 0.0), (-0.4, 0.3, PI), (-5.55, 0.3)),      # 3: the target in both cones, within 5 m of robot 0 only
          ((-6.0, -0.6, 0.1), (-5.0, 0.8, -0.2), (12.5, 12.5)),   # 4: no detection
          ((0.2, 0.1, 0.0), (0.9, -0.3, 0.5), (2.9, 0.4))]        # 5: a general pair
FILL = [(0.8, 6.1, -2.2), (12.2, 0.6, 3.0), (-0.7, 0.9, 1.1), (1.1, -1.3, PI / 2), (5.3, -0.6, -PI), (-12.4, 13.3, -0.3), (0.4, -6.2, 1.9)]


def _placed(R):
    """R robots in slots 0 .. R-1, two static targets behind them, the other slots of the M = 10 empty."""
    a6, h0 = np.zeros((N, M, 6)), np.zeros((N, M))
    pol = np.full((N, M), scen.POLICY_STATIC, dtype=np.int32)
    for w in range(N):
        p0, p1, tg = PLACED[w]
        for r in range(R):
            x, y, th = (p0, p1)[r] if r < 2 else FILL[(w + r) % len(FILL)]
            a6[w, r], h0[w, r] = [x, y, x + 1.0, y, 1.0, .3], th
        a6[w, R], a6[w, R + 1] = [tg[0], tg[1], 0, 0, 1, .2], [-13.0, 13.0, 0, 0, 1, .2]
    pol[:, :R] = scen.POLICY_IGMCTS
    env = _B()(N, M, max_obstacles=4, game_over_mode="all")
    env.set_scenarios(a6, pol, scen.DYN_FIRSTORDER, heading0=h0, n_agents=[R + 2] * N, obstacles=np.array([OBST] * N, dtype=np.float64),
                      n_obst=[4] * N)
    env.reset()
    return env


def _pool():
    """tests/test_ig_learner.py's pool at 6 worlds over 12 scenarios: slots 0 and 3 the robots, 1 and 2 static targets, 4 and 5
    walkers; robot 0's goal lies 1.25 + 0.1 (s % 4) m behind it at pref_speed 3, a time limit of 5 to 9 steps."""
    S, m = 2 * N, 6
    a6 = np.zeros((S, m, 6))
    pol = np.full((S, m), scen.POLICY_STATIC, dtype=np.int32)
    dyn = np.full((S, m), scen.DYN_FIRSTORDER, dtype=np.int32)
    for s in range(S):
        d, far = 1.25 + 0.1 * (s % 4), s >= N
        a6[s, 0] = [-5, 0.5 if far else 0, -5 - d, 0.5 if far else 0, 3.0, .5]
        a6[s, 1] = [-2.8, 1.3 if far else 0.8, 0, 0, 1, .2]
        a6[s, 2] = [6.5, -1.0, 0, 0, 1, .2]
        a6[s, 3] = [5, -0.4 if far else 0, 16, 0, 1, .5]
        a6[s, 4] = [0.5, 12, 0.5, -12, 1, .3]
        a6[s, 5] = [-12, -1.2, 12, -1.2, 1, .3]
    pol[:, [0, 3]] = scen.POLICY_IGMCTS
    pol[:, 4:] = scen.POLICY_NONCOOP
    dyn[:, 4:] = scen.DYN_UNICYCLE
    h0 = np.zeros((S, m))
    h0[:, 4], h0[N:, 3] = -np.pi / 2, 0.4
    env = _B()(N, m, n_scenarios=S, max_obstacles=4, game_over_mode="agent0")
    env.set_scenarios(a6, pol, dyn, heading0=h0, n_agents=[m] * S, obstacles=np.array([OBST] * N + [OBST2] * N, dtype=np.float64),
                      n_obst=[4] * S)
    env.reset()
    return env


def _actions(env, rng):
    import torch
    a = np.stack([rng.uniform(0.0, 3.0, (env.N, env.M)), rng.uniform(-1.0, 1.0, (env.N, env.M))], axis=-1).astype(np.float32)
    return torch.as_tensor(a, device=env.device)


def _has_credit(env):
    try:
        env.ig_robot_credit()
    except RuntimeError:
        return False
    return True


def _sentinel(env, R):
    """The nine output tensors of a raw call, pre-filled so that an unwritten entry shows."""
    import torch
    dev, n = env.device, env.N
    f = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    out = {"gain": f(n), "robot_observed": torch.full((n, R, 60), -1, dtype=torch.int64, device=dev), "credit": f(n, R, 3), "loo": f(n, R),
           "reward": f(n, R, 3)}
    acc = {"running": f(n, R, 3), "sum": f(n, R, 3), "last": f(n, R, 3), "episodes": torch.full((n,), -7, dtype=torch.int32, device=dev)}
    return out, acc


def _untouched(out, acc, rows=None):
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    return all(bool((sel(t) == (-1 if k == "robot_observed" else -7)).all()) for d in (out, acc) for k, t in d.items())


_ONE_HOT = {}


def _cache(ig, n):
    """The MI cache [n, 60, 60] read back bit for bit: cagym_ig_mi_reward of the one-cell masks (0.0 + mi[q] + zeros = mi[q])."""
    import torch
    dev = ig.b.device
    if n not in _ONE_HOT:
        q = torch.arange(3600, device=dev)
        hot = torch.zeros((3600, 60), dtype=torch.int64, device=dev)
        hot[q, q // 60] = torch.ones_like(q) << (q % 60)
        _ONE_HOT[n] = (hot.repeat(n, 1), torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(3600))
    masks, world = _ONE_HOT[n]
    return ig.mi_reward(masks, world).reshape(n, 60, 60)


def _check(env, ig, R, out, observed, gain, fresh, spec_worlds=None):
    """Every assertion that holds for any state: `out` is what a credit launch wrote behind the observe launch that wrote `observed`
    and `gain`; fresh: the belief was the prior before that observe launch.  Returns the host copies."""
    import torch
    n, dev = env.N, env.device
    torch.cuda.synchronize()
    poses = torch.zeros((n, R, 3), dtype=torch.float64, device=dev)
    det = torch.zeros((n, R, env.K, 2), dtype=torch.float64, device=dev)
    n_det = torch.zeros((n, R), dtype=torch.int32, device=dev)
    ig.robot_inputs(R, 5.0, env.obs_oas, poses, det, n_det)  # (the robots in slot order, wherever their slots are)
    world = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(R)
    V = out["robot_observed"]
    assert torch.equal(V, ig.visible_cells(poses.reshape(-1, 3), world).reshape(n, R, 60))
    union = torch.zeros((n, 60), dtype=torch.int64, device=dev)
    for r in range(R):
        union |= V[:, r]
    assert torch.equal(union, observed)
    assert torch.equal(out["gain"], gain)
    credit, loo = out["credit"], out["loo"]
    assert torch.equal(credit[:, :, 0].reshape(-1), ig.mi_reward(V.reshape(-1, 60), world))
    excl = torch.empty_like(V)
    for r in range(R):
        others = torch.zeros((n, 60), dtype=torch.int64, device=dev)
        for s in range(R):
            if s != r:
                others |= V[:, s]
        excl[:, r] = V[:, r] & ~others
    assert torch.equal(credit[:, :, 1].reshape(-1), ig.mi_reward(excl.reshape(-1, 60), world))
    assert torch.equal(credit[:, :, 2], out["gain"][:, None] - loo)
    if R == 1:
        g = out["gain"][:, None]
        assert torch.equal(credit[:, :, 0], g) and torch.equal(credit[:, :, 1], g) and torch.equal(credit[:, :, 2], g)
        assert (loo == 0).all() and not torch.signbit(loo).any()
    # the leave-one-out sum against the specification, on the belief and the cache read back
    bel, mi = ig.belief.cpu().numpy(), _cache(ig, n).cpu().numpy()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    Vh, ph, rows, nd = V.cpu().numpy(), poses.cpu().numpy(), env.obs_oas.cpu().numpy(), n_det.cpu().numpy()
    slots = _robot_slots(env, ph)
    for w in (range(n) if spec_worlds is None else spec_worlds):
        want = igm.robot_credit_spec(bel[w], mi[w], Vh[w], ph[w], rows[w, slots[w]])
        assert [len(d) for d in want["detections"]] == nd[w].tolist(), w
        assert want["gain"] == h["gain"][w] and np.array_equal(want["own"], h["credit"][w, :, 0]), w  # (sums of the cache: the same bits)
        assert np.array_equal(want["exclusive"], h["credit"][w, :, 1]), w
        assert (np.abs(h["loo"][w] - want["loo"]) <= 1e-12 * np.maximum(1.0, np.abs(want["loo"]))).all(), (w, h["loo"][w], want["loo"])
        if fresh:  # the belief is the product, in slot order, of the factors of the robots that saw the cell
            bits = ((Vh[w].view(np.uint64)[:, :, None] >> np.arange(60, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
            expect = np.ones((60, 60))
            for r in range(R):
                expect[bits[r]] = expect[bits[r]] * want["factor"][r][bits[r]]
            assert np.array_equal(bel[w], expect), w
    return h, Vh, nd


def _robot_slots(env, poses):
    """[N][R] the robots' slots: the robot-inputs call names them in slot order, the state says which slot stands at each pose."""
    st = env.state()
    px, py, hd = (st[k].cpu().numpy() for k in ("pos_x", "pos_y", "heading"))
    slots = []
    for w in range(env.N):
        row = []
        for x, y, th in poses[w]:
            row.append([s for s in range(env.M) if s not in row and px[w, s] == x and py[w, s] == y and hd[w, s] == th][0])
        slots.append(row)
    return slots


# ---- 1. placed poses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_credit_on_placed_poses(R):
    import torch
    env = _placed(R)
    ig = env.attach_ig_learner(window=G)
    env.attach_ig_credit()
    env.reset()
    q = env.ig_robot_credit()
    h, V, nd = _check(env, ig, R, q, env._igm.observed, env._igm.gain, fresh=True)
    own, excl, diff = h["credit"][:, :, 0], h["credit"][:, :, 1], h["credit"][:, :, 2]
    assert (own > 0).all() and (h["gain"] > 0).all()
    assert torch.equal(q["reward"], q["credit"])  # nothing restarted: the reward is the raw credit
    if R >= 2:
        assert np.array_equal(V[0, 0], V[0, 1]) and own[0, 0] == own[0, 1] and excl[0, 0] == 0 and excl[0, 1] == 0  # one pose twice
        assert nd[2, 0] == 1 and nd[2, 1] == 1 and nd[3, 0] == 1 and nd[3, 1] == 0 and (nd[4] == 0).all()
        assert (V[2, 0] & V[2, 1]).any() and (V[3, 0] & V[3, 1]).any()
    if R == 2:  # (only here: at R = 3 and 8 the further robots' cones may overlap these two; every R has the generic checks)
        assert not (V[1, 0] & V[1, 1]).any() and np.array_equal(excl[1], own[1])  # back to back: disjoint cones
        assert h["loo"][1, 0] == own[1, 1] and h["loo"][1, 1] == own[1, 0]
        assert diff[0, 0] == diff[0, 1] and h["loo"][0, 0] == h["loo"][0, 1] != h["gain"][0]  # the twin's second look changed what is left
        bel = ig.belief.cpu().numpy()
        assert (bel[2] == 1.5 * 1.5).any() and (bel[3] == 1.5 * 0.66).any()  # both detect it; one detects it, the other sees the cell empty
    # one more observation of the same poses, through step(): a belief that is no prior any more
    _, _, _, info = env.step(None, auto_reset=False)
    assert info["credit"] is q["credit"] and info["robot_reward"] is q["reward"] and info["robot_observed"] is q["robot_observed"]
    assert info["loo"] is q["loo"] and info["credit"].shape == (N, R, 3) and info["robot_observed"].shape == (N, R, 60)
    _check(env, ig, R, q, info["observed"], info["gain"], fresh=False)
    st = env.ig_robot_episode_stats()
    assert st["running"].shape == (N, R, 3) and st["episodes"].shape == (N,) and (st["episodes"] == 0).all()
    env.close()


def test_a_raw_call_with_more_rows_than_the_team_and_twice():
    """R = 4 on teams of 2: the rows past the team are zero with loo = gain, the team's rows are those of the R = 2 call; the same
    call twice writes the same bytes."""
    import torch
    env = _placed(2)
    ig = env.attach_ig_learner(window=G)
    env.reset()
    two = ig.robot_credit(2, 5.0, env.obs_oas)
    four = ig.robot_credit(4, 5.0, env.obs_oas)
    again, _ = _sentinel(env, 4)
    ig.robot_credit(4, 5.0, env.obs_oas, out=again)
    torch.cuda.synchronize()
    for k in four:
        assert torch.equal(four[k], again[k]), k
    assert torch.equal(four["gain"], two["gain"]) and torch.equal(four["gain"], env._igm.gain)
    for k in ("robot_observed", "credit", "loo", "reward"):
        assert torch.equal(four[k][:, :2], two[k]), k
    assert (four["credit"][:, 2:] == 0).all() and (four["robot_observed"][:, 2:] == 0).all() and (four["reward"][:, 2:] == 0).all()
    assert torch.equal(four["loo"][:, 2:], four["gain"][:, None].expand(N, 2))
    env.close()


# ---- 2. episodes ---------------------------------------------------------------------------------------------------------------
def test_restart_semantics_and_the_untouched_twin():
    """L: attach_ig_learner + attach_ig_credit under step(auto_reset=True); T: the same without attach_ig_credit, fed the same
    actions.  In a restart step robot_reward is 0 while credit is not; the accumulators equal sequential fp64 adds on the host;
    every output that existed before is T's, bit for bit; then reset(world_mask=m) on sentinel-filled rows."""
    import torch
    L, T = _pool(), _pool()
    ig = L.attach_ig_learner(window=G)
    L.attach_ig_credit()
    T.attach_ig_learner(window=G)
    L.reset()
    T.reset()
    torch.cuda.synchronize()
    R = 2
    run = L.ig_robot_credit()["credit"].cpu().numpy().copy()
    tot, last, eps = np.zeros((N, R, 3)), np.zeros((N, R, 3)), np.zeros(N, dtype=np.int32)
    assert np.array_equal(L.ig_robot_episode_stats()["running"].cpu().numpy(), run) and (run[:, :, 0] > 0).all()
    rng_l, rng_t = np.random.default_rng(3), np.random.default_rng(3)
    fired = 0
    for t in range(12):
        _, rew, go, info = L.step(_actions(L, rng_l), auto_reset=True)
        _, rew_t, go_t, info_t = T.step(_actions(T, rng_t), auto_reset=True)
        torch.cuda.synchronize()
        assert "credit" not in info_t and "robot_reward" not in info_t and "loo" not in info_t and "robot_observed" not in info_t
        assert torch.equal(L.obs_oas, T.obs_oas) and torch.equal(L.obs_ego, T.obs_ego) and torch.equal(rew, rew_t) and torch.equal(go, go_t), t
        assert torch.equal(L.flags, T.flags) and torch.equal(ig.belief, T._igm.ig.belief) and torch.equal(L.team_reward, T.team_reward), t
        for k in ("belief_window", "gain", "observed"):
            assert torch.equal(info[k], info_t[k]), (k, t)
        for k, v in L.ig_episode_stats().items():
            assert torch.equal(v, T.ig_episode_stats()[k]), (k, t)
        over = go.cpu().numpy().astype(bool)
        c, rr = info["credit"].cpu().numpy(), info["robot_reward"].cpu().numpy()
        assert (rr[over] == 0).all() and (c[over][:, :, 0] > 0).all() and np.array_equal(rr[~over], c[~over]), t
        assert torch.equal(info["credit"][:, :, 2], info["gain"][:, None] - info["loo"]), t
        for w in range(N):
            if over[w]:
                tot[w] += run[w]
                last[w] = run[w]
                eps[w] += 1
                run[w] = 0.0
            run[w] += c[w]
        st = {k: v.cpu().numpy() for k, v in L.ig_robot_episode_stats().items()}
        assert np.array_equal(st["running"], run) and np.array_equal(st["sum"], tot) and np.array_equal(st["last"], last), t
        assert np.array_equal(st["episodes"], eps) and np.array_equal(eps, L.ig_episode_stats()["episodes"].cpu().numpy()), t
        fired += int(over.sum())
    assert fired >= N and (eps >= 1).all()
    _check(L, ig, R, L.ig_robot_credit(), L._igm.observed, L._igm.gain, fresh=False, spec_worlds=[0, 3])
    # a manual restart of worlds 1 and 4 on sentinel-filled outputs: the other worlds' rows keep every byte
    sent, _ = _sentinel(L, R)
    for k, v in L.ig_robot_credit().items():
        v.copy_(sent[k])
    m = np.zeros(N, dtype=np.uint8)
    m[[1, 4]] = 1
    keep = torch.as_tensor(~m.astype(bool), device=L.device)
    L.reset(world_mask=m)
    torch.cuda.synchronize()
    assert _untouched(L.ig_robot_credit(), {}, rows=keep)
    for k, v in L.ig_robot_credit().items():
        assert not (v[~keep] == (-1 if k == "robot_observed" else -7)).any(), k
    assert (L.ig_robot_credit()["reward"][~keep] == 0).all() and (L.ig_robot_credit()["credit"][~keep][:, :, 0] > 0).all()
    st = {k: v.cpu().numpy() for k, v in L.ig_robot_episode_stats().items()}
    kp, c = keep.cpu().numpy(), L.ig_robot_credit()["credit"].cpu().numpy()
    assert np.array_equal(st["running"][kp], run[kp]) and np.array_equal(st["running"][~kp], c[~kp])  # not a finished episode: nothing folded
    assert np.array_equal(st["episodes"], eps) and np.array_equal(st["sum"], tot) and np.array_equal(st["last"], last)
    # reset(): everything anew, no episode counted
    L.reset()
    torch.cuda.synchronize()
    assert torch.equal(L.ig_robot_episode_stats()["running"], L.ig_robot_credit()["credit"])
    assert np.array_equal(L.ig_robot_episode_stats()["episodes"].cpu().numpy(), eps)
    assert torch.equal(L.ig_robot_credit()["reward"], L.ig_robot_credit()["credit"])
    L.close()
    T.close()


def test_on_an_exploration_stream_across_restarts():
    """Streamed worlds, 2 robots and 2 targets on fresh maps: after restarts onto rebuilt fields every robot's mask is still the
    visibility query's on the world's current slot, and the sums are still those of the masks."""
    import torch
    env = _B()(N, 6, n_scenarios=2 * N, max_obstacles=4, game_over_mode="agent0")
    assert env.stream_exploration_worlds(kinds="train_stage_1", seed=21, n_robots=2, n_targets=2, n_obst=(1, 4), target_radius=0.2,
                                         robot_pref_speed=30.0) == 0
    env.reset()
    ig = env.attach_ig_learner(window=G)
    env.attach_ig_credit()
    env.reset()
    rng = np.random.default_rng(4)
    restarts = 0
    for t in range(30):
        a = np.stack([rng.uniform(0.0, 4.0, (N, 6)), rng.uniform(-1.0, 1.0, (N, 6))], axis=-1).astype(np.float32)
        _, _, go, info = env.step(torch.as_tensor(a, device=env.device), auto_reset=True)
        restarts += int(go.sum().item())
        if t % 10 == 9:
            _check(env, ig, 2, env.ig_robot_credit(), info["observed"], info["gain"], fresh=False, spec_worlds=[t // 10])
    assert restarts >= N and int(env.state()["episode"].max().item()) >= 2 and env.exploration_stream_stats()["fields_built"] > 0
    assert torch.equal(env.ig_robot_episode_stats()["episodes"], env.ig_episode_stats()["episodes"])
    env.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def _raw(env, out, acc, env_h="own", params="own", oas="own", **kw):
    p = dict(n_robots=2, flags=0, detect_range=5.0, fov_rad=igm.FOV_DEG60, range=5.0)
    p.update(kw)
    P = _lib.IgCreditParams(p["n_robots"], p["flags"], p["detect_range"], p["fov_rad"], p["range"])
    return env.L.cagym_ig_credit(env.h if env_h == "own" else None, C.byref(P) if params == "own" else None,
                                 env.obs_oas.data_ptr() if oas == "own" else None, None,
                                 *[out[k].data_ptr() for k in ("gain", "robot_observed", "credit", "loo", "reward")],
                                 *[acc[k].data_ptr() for k in ("running", "sum", "last", "episodes")], env._stream())


def test_every_refusal_returns_its_code_and_writes_nothing():
    import torch
    env = _placed(2)
    out, acc = _sentinel(env, 2)
    assert _raw(env, out, acc) == E_STATE and b"cagym_ig_credit before cagym_ig_init" in env.L.cagym_last_error(env.h)
    ig = env.attach_ig_learner(window=G)
    env.reset()
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_robots=0), dict(n_robots=9), dict(n_robots=-1), dict(flags=2), dict(flags=8), dict(fov_rad=0.0), dict(fov_rad=nan),
           dict(fov_rad=inf), dict(fov_rad=-1.0), dict(range=0.0), dict(range=-1.0), dict(range=inf), dict(range=nan),
           dict(detect_range=0.0), dict(detect_range=nan), dict(detect_range=inf), dict(detect_range=-2.0)]
    for kw in bad:
        assert _raw(env, out, acc, **kw) == E_INVALID and b"cagym_ig_credit" in env.L.cagym_last_error(env.h), kw
    assert _raw(env, out, acc, env_h=None) == E_INVALID
    assert _raw(env, out, acc, params=None) == E_INVALID and _raw(env, out, acc, oas=None) == E_INVALID
    belief = ig.belief.clone()
    torch.cuda.synchronize()
    assert _untouched(out, acc)  # nothing was launched
    assert _raw(env, out, acc, flags=igm.EPISODE_FOLD | igm.OBSERVE_ONLY_RESTARTED) == 0  # NULL mask: no world is restarted, all are skipped
    torch.cuda.synchronize()
    assert _untouched(out, acc)
    assert _raw(env, out, acc) == 0
    torch.cuda.synchronize()
    assert not _untouched(out, {}) and torch.equal(out["gain"], env._igm.gain) and torch.equal(ig.belief, belief)  # the handle is only read
    assert torch.equal(acc["running"], out["credit"] - 7.0) and (acc["sum"] == -7).all() and (acc["episodes"] == -7).all()
    env.close()


def test_attach_needs_the_learner_and_leaves_with_it():
    env = _placed(2)
    with pytest.raises(RuntimeError, match="attach_ig_credit needs attach_ig_learner"):
        env.attach_ig_credit()
    with pytest.raises(RuntimeError, match="needs attach_ig_credit"):
        env.ig_robot_episode_stats()
    env.attach_ig_greedy(episodic=True)
    with pytest.raises(RuntimeError, match="attach_ig_credit needs attach_ig_learner"):
        env.attach_ig_credit()
    env.attach_ig_learner(window=G)
    env.attach_ig_credit()
    assert _has_credit(env)
    env.attach_ig_learner(window=G)  # attaching another IG policy drops it, as it drops the goals
    assert not _has_credit(env)
    env.reset()
    assert "credit" not in env.step(None)[3]
    env.attach_ig_credit()
    env.reset()
    assert "credit" in env.step(None)[3]
    env.detach_ig_mcts()
    assert not _has_credit(env) and "credit" not in env.step(None)[3]
    env.close()


# ---- 4. the robots as environments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward", ["difference", "own", "exclusive", "team"])
def test_robot_vecenv(reward):
    import torch
    env = _pool()
    env.attach_ig_learner(window=G, context=(reward == "own"))
    env.attach_ig_goals()
    R, slots = 2, [0, 3]
    v = vec.CagymRobotVecEnv(env, reward=reward)
    assert (_has_credit(env)) == (reward != "team") and v.num_envs == N * R
    obs = v.reset()
    C_ = 6 if reward == "own" else 3
    assert obs.shape == (N * R, C_, G, G)
    goals = torch.zeros((N, R, 2), dtype=torch.float64, device=env.device)
    goals[:, 0, 0], goals[:, 0, 1] = -3.0, 0.0
    mask = torch.zeros((N, R), dtype=torch.uint8, device=env.device)
    mask[:, 0] = 1
    env.ig_set_goals(goals, mask=mask)  # robot 0 of every world holds a goal 2 m ahead; robot 1 is the caller's
    acts = torch.zeros((N * R, 2), dtype=torch.float32, device=env.device)
    acts[:, 0] = 0.25 + 0.125 * torch.arange(N * R, device=env.device)  # a speed of its own per environment, exact in fp32
    obs, rews, dones, infos = v.step(acts)
    torch.cuda.synchronize()
    table = v._table.cpu().numpy()
    want = np.zeros((N, 6, 2), dtype=np.float32)
    want[:, slots, 0] = acts[:, 0].cpu().numpy().reshape(N, R)  # env w * R + r is robot r of world w; the other rows stay zero
    assert np.array_equal(table, want)
    assert obs.shape == (N * R, C_, G, G) and torch.equal(obs[:, :3].reshape(N, R, 3, G, G), env._igm.belief_window)
    if C_ == 6:
        assert torch.equal(obs[:, 3:].reshape(N, R, 3, G, G), env._igm.context_window)
    assert rews.shape == (N * R,) and dones.shape == (N * R,) and dones.dtype == torch.bool
    assert torch.equal(dones.reshape(N, R), env.game_over.bool()[:, None].expand(N, R))
    assert infos["team_reward"] is env.team_reward and "goal_distance" in infos and "goal_reached" in infos
    if reward == "team":
        assert "credit" not in infos and torch.equal(rews.reshape(N, R), env.team_reward[:, None].expand(N, R))
    else:
        col = {"own": 0, "exclusive": 1, "difference": 2}[reward]
        assert infos["credit"] is env.ig_robot_credit()["credit"]
        assert torch.equal(rews.reshape(N, R), env.ig_robot_credit()["reward"][:, :, col]) and (env.ig_robot_credit()["reward"][:, :, 0] > 0).all()
    # the robot that holds a goal followed the controller - the step read the controller's row, not the caller's; every other row,
    # the other robot's included, is the caller's
    read = env._act.cpu().numpy()
    assert np.array_equal(read[:, 3], want[:, 3]) and np.array_equal(read[:, [1, 2, 4, 5]], want[:, [1, 2, 4, 5]])
    assert (read[:, 0] != want[:, 0]).any(axis=1).all()  # (v is 0 or v_max = 2 there, never the 0.25 .. 1.5 the caller asked for)
    assert torch.isfinite(infos["goal_distance"][:, 0]).all() and torch.isinf(infos["goal_distance"][:, 1]).all()
    with pytest.raises(ValueError, match="reward must be one of"):
        vec.CagymRobotVecEnv(env, reward="shared")
    # CagymVecEnv passes the per-robot reward through when the env has it
    flat = vec.CagymVecEnv(env, ["dist_to_goal"])
    infos = flat.step(torch.zeros((N, 6, 2), dtype=torch.float32, device=env.device))[3]
    assert ("robot_reward" in infos) == (reward != "team")
    env.close()
    plain = _pool()
    with pytest.raises(RuntimeError, match="CagymRobotVecEnv needs attach_ig_learner"):
        vec.CagymRobotVecEnv(plain)
    plain.close()
