"""Every generation-3 kernel instantiation against the CPU oracle, driven by the spec table.

The env step runs in one of the (lanes, compile-time M, worlds per workgroup) rows of CAGYM_K3_SPECS (csrc/cagym_launch3.h,
parsed by build.K3_SPECS) times OBST in {0, 1}; spec2() in cagym_api.hip picks the row from max_agents.  Per row and shape:

(a) the one-step launch (k_step3) in lock-step with the fp64 oracle: a ragged last workgroup, ragged n_agents (0, 1 and M
    agents), RVO / NonCoop / Static agents with agent 0 External; OBST: LaserScan, 0, 1 and K rectangles per world, once with
    RVO agents (obstacle lines) and once without (the lines-free layout);
(b) the same at the largest rectangle count the row accepts (CAPACITY), one past it refused;
(c) every other launch form - k_rollout3 with and without auto-reset, k_step3 with auto-reset, the split step - bit for bit
    against step() + a host-side reset, with restarts inside the launches.

(a) holds k_step3 to the oracle and (c) holds every other form to k_step3: together they pin every instantiation.
Tolerances are those of the other oracle tests (test_hip_parity.py, test_cfg4.py)."""
import importlib

import numpy as np
import pytest

from oracle import oracle as orc

build = importlib.import_module("gym-exploration-2d_amd.build")
scen = importlib.import_module("gym-exploration-2d_amd.scenarios")


def shape_for(nt, mt, wp):
    """The shapes that run a row of CAGYM_K3_SPECS: [(max_agents, CAGYM_WPW10 override or None)].  An unknown row raises:
    a new specialisation needs shapes here before it has coverage."""
    if (nt, mt) == (256, 10) and wp in (4, 5):
        return [(10, str(wp))]  # the worlds-per-workgroup choice of M = 10 is a heuristic: pinned by the override
    if (nt, mt, wp) == (256, 4, 0):
        return [(4, None)]
    if (nt, mt, wp) == (256, 20, 2):
        return [(20, None)]
    if (nt, mt, wp) == (256, 0, 0):
        return [(7, None)]
    if (nt, mt, wp) == (512, 0, 0):
        return [(13, None), (32, None)]  # the narrowest and the widest world of the 512-lane row
    raise KeyError("no test shape for the kernel specialisation (%d, %d, %d)" % (nt, mt, wp))


# Largest max_obstacles a handle with RVO agents among rectangles accepts (cagym_set_scenarios): 2 K + M - 1 half-planes in an
# LP group of gw lanes x 4, 2 K <= 32 coverage bits, 13 B per (ego, obstacle candidate) in the LP scratch, the roll-out layout
# within 160 KB of LDS.  Which rule binds: M 4 / 10 / 32 the LP group, M 20 / generic 256 the candidate lists, M 13 the coverage
# bits; M = 32, K = 16 puts the roll-out layout at 161 488 of the 163 840 bytes of LDS.
CAPACITY = {(256, 10, 4, 10): 11, (256, 10, 5, 10): 11, (256, 4, 0, 4): 6, (256, 20, 2, 20): 15, (256, 0, 0, 7): 9,
            (512, 0, 0, 13): 16, (512, 0, 0, 32): 16}
K_PLAIN = 5  # rectangles per world of the (a) and (c) cases


def _cases():
    return [(nt, mt, wp, M, wpw) for nt, mt, wp in build.K3_SPECS for M, wpw in shape_for(nt, mt, wp)]


def _id(nt, mt, wp, M):
    return "%d-%d-%d-M%d" % (nt, mt, wp, M)


CASES = [pytest.param(*c, id=_id(*c[:4])) for c in _cases()]
OBST_VARIANTS = [pytest.param(False, True, id="free"), pytest.param(True, True, id="obst"),
                 pytest.param(True, False, id="obst-nolines")]


def test_every_kernel_specialisation_has_a_test_shape():
    """CPU: every row of CAGYM_K3_SPECS runs in this module, and every shape of an OBST row has a capacity entry."""
    assert len(build.K3_SPECS) >= 6
    for nt, mt, wp in build.K3_SPECS:
        for M, wpw in shape_for(nt, mt, wp):
            assert 2 <= M <= 32
            assert (nt, mt, wp, M) in CAPACITY, (nt, mt, wp, M)
            assert _n_worlds(M, wp) % _wpw(M, wp) != 0
    with pytest.raises(KeyError):
        shape_for(256, 12, 3)


def test_a_ring_of_rectangles_gives_the_ego_one_obstacle_line_each():
    """CPU, the oracle: the capacity worlds below put K small squares around an RVO ego; each gives it an obstacle line (the
    second visible edge of a convex rectangle is always covered by the first one's line, so K lines per ego is the most K
    rectangles can give).  Without this the capacity cases would not reach the edge they are there for."""
    for K in sorted(set(CAPACITY.values())):
        rects = _ring(K, 0.0, 0.0, 0.3)
        pos = np.array([[0.0, 0.0], [9.0, 1.0]])
        r = orc.orca_action_ex(pos, np.zeros((2, 2)), np.array([[0.0, 9.0], [-9.0, 0.0]]), [1.0, 1.0], [0.5, 0.5], 0, 0.3,
                               0.5, rects=rects)
        assert r["n_obst_lines"] == K, (K, r["n_obst_lines"])


# ---- scenario pools ----------------------------------------------------------------------------------------------------------
def _wpw(M, wp):
    return wp if wp else 64 // M  # worlds per workgroup (cagym_api.hip: n_wg2)


def _n_worlds(M, wp):
    """A few workgroups and a last one that holds a single world."""
    w = _wpw(M, wp)
    return w * -(-40 // w) + 1


def _ring(K, cx, cy, rot):
    """K squares of side 0.4 on a circle of radius 1.6 around (cx, cy), none on an axis through the centre."""
    ang = 2 * np.pi * (np.arange(K) + 0.5) / K + rot
    c = np.stack([cx + 1.6 * np.cos(ang), cy + 1.6 * np.sin(ang)], 1)
    return np.concatenate([c - 0.2, c + 0.2], 1)


def _clear_of(p, rects, margin):
    """points p [n, 2] at least `margin` from every rectangle [k, 4] (box distance)"""
    if not len(rects):
        return np.ones(len(p), dtype=bool)
    r = np.asarray(rects)
    dx = np.maximum(np.maximum(r[None, :, 0] - p[:, None, 0], p[:, None, 0] - r[None, :, 2]), 0.0)
    dy = np.maximum(np.maximum(r[None, :, 1] - p[:, None, 1], p[:, None, 1] - r[None, :, 3]), 0.0)
    return (np.hypot(dx, dy) >= margin).all(1)


def _crowd_with_rectangles(S, M, K, rng, side=11.0):
    """obstacle_worlds cannot seat more than about 20 agents: random start / goal pairs in a wider square
    (random_worlds_fast), then 2..K squares and walls of up to 2 m where they keep 1 m from every start and goal."""
    a6 = scen.random_worlds_fast(S, M, seed=int(rng.integers(1 << 30)), side=side)
    obst, n_obst = np.zeros((S, K, 4)), np.zeros(S, dtype=np.int32)
    for w in range(S):
        want, pts = rng.integers(2, K + 1), a6[w, :, 0:4].reshape(-1, 2)
        for _ in range(200):
            if n_obst[w] == want:
                break
            lo = rng.uniform(-side, side - 2.0, 2)
            r = np.concatenate([lo, lo + rng.uniform(0.4, 2.0, 2)])
            if _clear_of(pts, [r], 1.0).all() and _clear_of(np.array([r[0:2], r[2:4], r[[0, 3]], r[[2, 1]]]), obst[w, :n_obst[w]], 0.2).all():
                obst[w, n_obst[w]] = r
                n_obst[w] += 1
    return a6, obst, n_obst


def _ring_world(a6, M, rng):
    """agent 1 at the origin (inside the ring), the others on start / goal pairs through the middle, 4 to 11 m out"""
    a6[1, 0:2] = 0.0
    ang = rng.uniform(0, 2 * np.pi)
    a6[1, 2:4] = 9.0 * np.cos(ang), 9.0 * np.sin(ang)
    seated = [a6[1, 0:2]]
    for i in [0] + list(range(2, M)):
        while True:
            d, ang = rng.uniform(4.0, 11.0), rng.uniform(0, 2 * np.pi)
            s = np.array([d * np.cos(ang), d * np.sin(ang)])
            if all(np.hypot(*(s - q)) >= 1.5 for q in seated):
                break
        a6[i, 0:2], a6[i, 2:4] = s, -s
        seated.append(s)


def _pool(S, M, K, seed, rvo=True, ring=()):
    """S scenarios: agent 0 External, the others RVO / NonCoop / Static (rvo=False: no RVO agent at all); n_agents 0, 1 and M
    among ragged counts; K > 0: 0, 1 and K rectangles among 2..min(K, 6) random ones, and in the worlds of `ring` agent 1 - an
    RVO ego - at the origin inside a ring of K squares (test_a_ring_of_rectangles_...)."""
    rng = np.random.default_rng(seed)
    if K and M <= 20:
        a6, ob, nob, _ = scen.obstacle_worlds(S, M, min(K, 6), seed=seed)
        obst = np.zeros((S, K, 4))
        obst[:, :ob.shape[1]] = ob
        n_obst = nob.copy()
    elif K:
        a6, ob, n_obst = _crowd_with_rectangles(S, M, min(K, 6), rng)
        obst = np.zeros((S, K, 4))
        obst[:, :ob.shape[1]] = ob
    else:
        a6, obst, n_obst = scen.random_worlds_fast(S, M, seed=seed, side=7.5 if M <= 20 else 11.0), None, None
    u = rng.uniform(size=(S, M))
    pol = np.where(u < 0.7, scen.POLICY_RVO, np.where(u < 0.9, scen.POLICY_NONCOOP, scen.POLICY_STATIC)).astype(np.int32)
    pol[:, 0] = scen.POLICY_EXTERNAL
    n_agents = rng.integers(max(2, M - 3), M + 1, S).astype(np.int32)
    n_agents[2], n_agents[3], n_agents[4] = 0, 1, M
    if K:
        n_obst[0], n_obst[1] = 0, 1
        for w in ring:
            obst[w] = _ring(K, 0.0, 0.0, rng.uniform(0, 0.3))
            n_obst[w] = K
            _ring_world(a6[w], M, rng)
            pol[w, 1] = scen.POLICY_RVO
            n_agents[w] = M
        obst[np.arange(K)[None, :] >= n_obst[:, None]] = 0.0
    if not rvo:
        pol[pol == scen.POLICY_RVO] = scen.POLICY_NONCOOP
    return dict(agents6=a6, policy_id=pol, dynamics_id=scen.DYN_UNICYCLE, n_agents=n_agents, coop=np.full((S, M), 0.5),
                obstacles=obst, n_obst=n_obst)


def _kernel(env, nt, mt, wp, obst, rollout, auto_reset):
    name = env.kernel_name(rollout=rollout, auto_reset=auto_reset)
    exp = "%s3<%d, %d, %d, %s, %s>" % ("k_rollout" if rollout else "k_step", nt, mt, wp, "true" if auto_reset else "false",
                                      "true" if obst else "false")
    assert name == exp, (name, exp)
    return name


# ---- (a) / (b): k_step3 in lock-step with the oracle ------------------------------------------------------------------------
def _lockstep(hip, cpu, pool, N, M, laser, T, seed, lines=None):
    """Both backends on `pool`, T steps with agent 0 External (towards its goal with a wobble); every step held to the oracle.
    lines: (world, ego, count) - the oracle's obstacle-line count of that ego in the initial state must be `count`."""
    from test_cfg4 import _laser_close
    from test_hip_parity import _compare_batch
    for e in (hip, cpu):
        e.set_scenario(**pool)
        e.reset()
    if lines is not None:
        w, ego, count = lines
        a6 = pool["agents6"][w]
        n = pool["n_agents"][w]
        r = orc.orca_action_ex(cpu.f("pos")[w, :n], cpu.f("vel")[w, :n], a6[:n, 2:4], a6[:n, 4], a6[:n, 5], ego,
                               float(cpu.f("heading")[w, ego]), 0.5, max_neighbors=M, rects=pool["obstacles"][w, :pool["n_obst"][w]])
        assert r["n_obst_lines"] == count, ("obstacle lines of the capacity ego", w, r["n_obst_lines"], count)
    _compare_batch(hip, cpu, N, M, 0)
    if laser:
        _laser_close(hip, cpu, 0)
    rng = np.random.default_rng(seed)
    for t in range(T):
        ext = np.zeros((N, M, 2), dtype=np.float32)
        ext[:, 0, 0] = rng.uniform(0.6, 1.0, N)
        ext[:, 0, 1] = np.clip(-cpu.f("heading_ego")[:, 0], -0.5, 0.5) + rng.uniform(-0.1, 0.1, N)
        hip.step(ext)
        cpu.step(ext.astype(np.float64))
        assert np.abs(hip.f("action") - cpu.f("action")).max() <= 2e-7, ("action", t)
        _compare_batch(hip, cpu, N, M, t + 1, ftol=1e-7)
        if laser:
            _laser_close(hip, cpu, t + 1)


def _handles(N, M, K, laser, n_scenarios=None):
    from test_hip_parity import _hip
    hip = _hip(N=N, M=M, max_obstacles=K, game_over_mode=1, laserscan=laser, n_scenarios=n_scenarios)
    cpu = orc.OracleEnv(N=N, M=M, max_obstacles=K, game_over_mode=1, laserscan=laser)
    return hip, cpu


@pytest.mark.gpu
@pytest.mark.parametrize("obst,rvo", OBST_VARIANTS)
@pytest.mark.parametrize("nt,mt,wp,M,wpw", CASES)
def test_step_matches_oracle(nt, mt, wp, M, wpw, obst, rvo, monkeypatch):
    if wpw:
        monkeypatch.setenv("CAGYM_WPW10", wpw)
    N, T = _n_worlds(M, wp), 60
    K = K_PLAIN if obst else 0
    pool = _pool(N, M, K, seed=1100 + 7 * M + wp, rvo=rvo, ring=(5, N - 1) if obst else ())
    hip, cpu = _handles(N, M, K, obst)
    print(_kernel(hip.env, nt, mt, wp, obst, False, False), "N=%d K=%d rvo=%d" % (N, K, rvo))
    _lockstep(hip, cpu, pool, N, M, obst, T, seed=M, lines=(N - 1, 1, K) if obst and rvo else None)
    if rvo:
        assert int((pool["policy_id"][:N] == scen.POLICY_RVO).sum()) > 0
    hip.env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt,mt,wp,M,wpw", CASES)
def test_step_matches_oracle_at_rectangle_capacity(nt, mt, wp, M, wpw, monkeypatch):
    """The largest max_obstacles the row accepts with RVO agents, K rectangles around an RVO ego in a full workgroup and in the
    ragged last one; one rectangle more is refused - by the handle's max_obstacles, whatever the pool's n_obst - and leaves the
    handle usable for a pool without RVO agents."""
    if wpw:
        monkeypatch.setenv("CAGYM_WPW10", wpw)
    N, T = _n_worlds(M, wp), 60
    K = CAPACITY[(nt, mt, wp, M)]
    pool = _pool(N, M, K, seed=2000 + 7 * M + wp, ring=(5, N - 1))
    hip, cpu = _handles(N, M, K, True)
    print(_kernel(hip.env, nt, mt, wp, True, False, False), "N=%d K=%d (capacity)" % (N, K))
    _lockstep(hip, cpu, pool, N, M, True, T, seed=M, lines=(N - 1, 1, K))
    hip.env.close()
    # one past the edge
    hip, cpu = _handles(N, M, K + 1, True)
    with pytest.raises(RuntimeError, match="too many rectangles"):
        hip.set_scenario(**pool)  # at most K rectangles per world, but a handle sized for K + 1
    over = _pool(N, M, K + 1, seed=3000 + M, rvo=False, ring=(5, N - 1))
    with pytest.raises(RuntimeError, match="too many rectangles"):
        hip.set_scenario(**dict(over, policy_id=pool["policy_id"]))
    _lockstep(hip, cpu, over, N, M, True, 30, seed=M + 1)
    hip.env.close()


# ---- (c): every launch form against step() + host reset -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("obst,rvo", OBST_VARIANTS)
@pytest.mark.parametrize("nt,mt,wp,M,wpw", CASES)
def test_launch_forms_equal_step_bitwise(nt, mt, wp, M, wpw, obst, rvo, monkeypatch):
    """k_rollout3 (auto-reset on and off), k_step3 with auto-reset and the split step == k_step3 + cagym_reset(advance) of the
    finished worlds, bit for bit, step after step.  OBST with RVO agents: at the rectangle capacity of the row (the roll-out
    kernels' largest layout)."""
    import torch
    from test_hip_parity import _hip
    if wpw:
        monkeypatch.setenv("CAGYM_WPW10", wpw)
    N, T = _n_worlds(M, wp), 250
    S = 3 * N
    K = (CAPACITY[(nt, mt, wp, M)] if rvo else K_PLAIN) if obst else 0
    pool = _pool(S, M, K, seed=4000 + 7 * M + wp, rvo=rvo, ring=(5, N - 1, N + 5) if obst else ())
    pool["policy_id"][:, 0] = scen.POLICY_NONCOOP  # every form runs without external actions (the roll-outs have none)
    envs = {}
    for k in ("ref", "ref_plain", "rollout", "rollout_plain", "step_auto", "split"):
        e = _hip(N=N, M=M, max_obstacles=K, game_over_mode=0, laserscan=obst, n_scenarios=S)
        e.set_scenario(**pool)
        e.reset()
        envs[k] = e.env
    ref, plain = envs["ref"], envs["ref_plain"]
    names = {_kernel(ref, nt, mt, wp, obst, r, a) for r in (False, True) for a in (False, True)}
    print(sorted(names), "N=%d S=%d K=%d rvo=%d" % (N, S, K, rvo))
    tr = envs["rollout"].rollout(T, auto_reset=True)
    tp = envs["rollout_plain"].rollout(T, auto_reset=False)
    keys = ["reward", "flags", "game_over", "other_agents_states", "ego"] + (["laserscan"] if obst else [])
    out = lambda e: {"reward": e.reward, "flags": e.flags, "game_over": e.game_over, "other_agents_states": e.obs_oas,
                     "ego": e.obs_ego, "laserscan": e.obs_laser}
    restarts = 0
    for t in range(T):
        plain.step()
        for k in keys:
            assert torch.equal(tp[k][t], out(plain)[k]), ("rollout auto_reset=False", k, t)
        ref.step()
        go = ref.game_over.clone()
        step_out = {k: out(ref)[k].clone() for k in ("reward", "flags", "game_over")}
        if bool(go.any()):
            restarts += int(go.sum())
            ref.reset(world_mask=go, advance_episode=True)
        exp = dict(out(ref), **step_out)
        envs["step_auto"].step(auto_reset=True)
        envs["split"].step_begin()
        envs["split"].step_finish(auto_reset=True)
        for k in keys:
            assert torch.equal(tr[k][t], exp[k]), ("rollout auto_reset=True", k, t)
            assert torch.equal(out(envs["step_auto"])[k], exp[k]), ("step auto_reset=True", k, t)
            assert torch.equal(out(envs["split"])[k], exp[k]), ("split step", k, t)
    torch.cuda.synchronize()
    for k, e in envs.items():
        if k in ("ref", "ref_plain"):
            continue
        want = plain if k == "rollout_plain" else ref
        for f, v in want.state().items():
            if f != "map_bits":
                assert torch.equal(e.state()[f], v), (k, "state", f)
    assert restarts > 0 and int(ref.episode_stats()["stat_episodes"].sum()) > 0
    for e in envs.values():
        e.close()
