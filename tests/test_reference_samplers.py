"""On-device samplers of the reference's training scenarios (cagym_generate_reference_scenarios):
train_agents_swap_circle / _pairwise_swap / _random_positions and train_stage_1 / _2 (test_cases.py:1192-1463, 2359-2572).
CPU: the twin (tests/sampler_twin.py) obeys every rule and matches the reference's own draws (tests/golden/scenario_samplers.npz)
in distribution; the curriculum restates _init_agents.  GPU: the device equals the twin; a generated pool drives the env exactly
like the same pool uploaded; generated obstacle pools run in lock-step with the fp64 oracle; refusals leave the handle as it was."""
import ctypes as C
import filecmp
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

import sampler_twin as tw

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SWAPS = (scen.GEN_SWAP_CIRCLE, scen.GEN_PAIRWISE_SWAP)
STAGES = (scen.GEN_STAGE_1, scen.GEN_STAGE_2)
NAMES = {v: k for k, v in scen.REFERENCE_SAMPLERS.items()}
# the arguments make_golden_samplers.py passes, and the twin's seeds
FIXTURE_ARGS = {scen.GEN_SWAP_CIRCLE: 8, scen.GEN_PAIRWISE_SWAP: 8, scen.GEN_STAGE_1: 4, scen.GEN_STAGE_2: 10}


def _live_rows(pool, w):
    n = int(pool["n_agents"][w])
    return pool["agents6"][w, :n]


def _pairwise_min(p):
    if len(p) < 2:
        return np.inf
    d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) + np.eye(len(p)) * 1e9
    return d.min()


def _overlap(a, b):
    """not is_shape_valid (test_cases.py:150-170) for two (xl, yl, xu, yu) rectangles"""
    return not (a[0] >= b[2] or b[0] >= a[2] or a[3] <= b[1] or b[3] <= a[1])


def _clear(p, r):
    """is_pose_valid_with_obstacles (test_cases.py:135-148) for one rectangle"""
    return p[0] >= r[2] + 1 or p[1] >= r[3] + 1 or p[0] <= r[0] - 1 or p[1] <= r[1] - 1


# ---- CPU: the twin obeys each rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [scen.GEN_SWAP_CIRCLE, scen.GEN_PAIRWISE_SWAP, scen.GEN_STAGE_1, scen.GEN_STAGE_2])
@pytest.mark.parametrize("ego", [scen.POLICY_RVO, scen.POLICY_GA3C])
def test_twin_obeys_the_rules(kind, ego):
    S, M, K = 300, 10, 10
    p = tw.generate(S, M, K, [kind], seed=5 + kind, ego_policy=ego)
    assert p["n_failed"] == 0
    na = p["n_agents"]
    if kind in SWAPS:
        assert na.min() == 2 and na.max() == M and (na % 2 == 0).all()
        assert set(np.unique(na)) == {2, 4, 6, 8, 10}
    else:
        assert na.min() == 2 and na.max() == M and len(np.unique(na)) == M - 1
        lo, hi = (0, 4) if kind == scen.GEN_STAGE_1 else (2, 10)
        assert p["n_obst"].min() == lo and p["n_obst"].max() == hi
    nc = []
    for w in range(S):
        r = _live_rows(p, w)
        n = len(r)
        assert (r[:, 4] == 1.0).all() and (r[:, 5] == 0.5).all()
        assert (p["agents6"][w, n:, :4] == 0).all() and (p["policy"][w, n:] == scen.POLICY_STATIC).all()
        if kind == scen.GEN_PAIRWISE_SWAP:
            assert (np.abs(r[:, :2]) <= 7.5).all() and _pairwise_min(r[:, :2]) >= 2.0
        else:
            rad = np.hypot(r[:, 0], r[:, 1])
            lo, hi = {scen.GEN_SWAP_CIRCLE: (4, 8), scen.GEN_STAGE_1: (6, 8), scen.GEN_STAGE_2: (8, 10)}[kind]
            assert (rad >= lo - 1e-12).all() and (rad <= hi + 1e-12).all()
            assert np.array_equal(r[:, 2:4], -r[:, 0:2])  # antipodal goal
            # is_pose_valid against every earlier start and goal (a swap pair's goals are its own starts)
            pts = r[:, 0:2] if kind == scen.GEN_SWAP_CIRCLE else np.concatenate([r[:, 0:2], r[:, 2:4]])
            assert _pairwise_min(pts) >= 1.5
        if kind in SWAPS:
            assert np.array_equal(r[0::2, 2:4], r[1::2, 0:2]) and np.array_equal(r[1::2, 2:4], r[0::2, 0:2])  # pairs swap
            assert p["dynamics"][w, 0] == (scen.DYN_MAXACC if ego == scen.POLICY_GA3C else scen.DYN_FIRSTORDER)
            assert set(p["policy"][w, 1:n]) <= {scen.POLICY_RVO, scen.POLICY_NONCOOP}
            assert p["coop"][w, 0] == 1.0 and (p["coop"][w, 1:n] == 0.5).all()
            nc += list(p["policy"][w, 1:n] == scen.POLICY_NONCOOP)
        else:
            no = p["n_obst"][w]
            rects = p["obstacles"][w, :no]
            assert (p["obstacles"][w, no:] == 0).all()
            sx, sy = rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]
            lo_c, hi_c = (-4, 6) if kind == scen.GEN_STAGE_1 else (-8, 10)
            assert ((rects[:, 2:4] >= lo_c) & (rects[:, 2:4] <= hi_c)).all()
            assert ((sx >= 1 - 1e-12) & (sx <= 4 + 1e-12) & (sy >= 1 - 1e-12) & (sy <= 4 + 1e-12)).all()
            for a in range(no):
                for b in range(a):
                    assert not _overlap(rects[a], rects[b])
                for q in np.concatenate([r[:, 0:2], r[:, 2:4]]):
                    assert _clear(q, rects[a])
            assert p["dynamics"][w, 0] == scen.DYN_FIRSTORDER and (p["dynamics"][w, 1:n] == scen.DYN_UNICYCLE).all()
            assert (p["policy"][w, 1:n] == scen.POLICY_RVO).all() and (p["coop"][w, :n] == 1.0).all()
        assert p["policy"][w, 0] == ego
    if nc:
        f, m = np.mean(nc), len(nc)
        assert abs(f - 0.2) < 3 * np.sqrt(0.16 / m), f


def test_rectangle_bounds_narrow_each_stage():
    """n_obst bounds narrow the reference's range of each stage kind: in the curriculum's stage mixture n_obst=(-1, 9) caps
    stage 2 at 9 and leaves stage 1 at randint(0, 4)"""
    p = tw.generate(600, 8, 9, [scen.GEN_PAIRWISE_SWAP, scen.GEN_STAGE_1, scen.GEN_STAGE_2], seed=21, number_of_agents=6, n_obst=(-1, 9))
    s1, s2 = p["n_obst"][p["kind"] == scen.GEN_STAGE_1], p["n_obst"][p["kind"] == scen.GEN_STAGE_2]
    assert set(s1) == {0, 1, 2, 3, 4} and set(s2) == set(range(2, 10))
    assert (p["n_obst"][p["kind"] == scen.GEN_PAIRWISE_SWAP] == 0).all()
    q = tw.generate(300, 8, 10, [scen.GEN_STAGE_1, scen.GEN_STAGE_2], seed=22, n_obst=(3, 20))
    assert set(q["n_obst"][q["kind"] == scen.GEN_STAGE_1]) == {3, 4} and set(q["n_obst"][q["kind"] == scen.GEN_STAGE_2]) == set(range(3, 11))


def test_twin_counts_random_positions_failures_per_scenario():
    """with a tiny max_tries the random-positions rule fails often: the twin's per-scenario count adds up to the oracle's total,
    and in a mixture only the random-positions scenarios contribute"""
    from oracle import oracle as orc
    for mt in (1, 3):
        p = tw.generate(400, 10, 0, [scen.GEN_RANDOM_POSITIONS], seed=4, max_tries=mt)
        nf = orc.generate_scenarios(400, 10, seed=4, n_min=2, n_max=10, ego_policy=scen.POLICY_RVO, ego_dynamics=scen.DYN_FIRSTORDER,
                                    policy_a=scen.POLICY_RVO, policy_b=scen.POLICY_NONCOOP, p_b=0.5, other_dynamics=scen.DYN_UNICYCLE,
                                    max_tries=mt)[5]
        assert p["n_failed"] == nf > 0
    kinds = [scen.GEN_SWAP_CIRCLE, scen.GEN_PAIRWISE_SWAP, scen.GEN_RANDOM_POSITIONS]
    mix = tw.generate(400, 10, 0, kinds, seed=4, max_tries=1)
    assert mix["n_failed"] == mix["failed"].sum()
    for k in kinds:
        w = mix["kind"] == k
        alone = tw.generate(400, 10, 0, [k], seed=4, max_tries=1)
        assert np.array_equal(mix["failed"][w], alone["failed"][w]) and alone["failed"][w].sum() > 0, k


def test_twin_overrides_policies_and_counts():
    p = tw.generate(200, 10, 10, [scen.GEN_STAGE_2], seed=3, ego_policy=scen.POLICY_GA3C, other_policies=(5, 1), p_b=0.2,
                    n_obst=(3, 6), fixed_count=True, number_of_agents=7)
    assert (p["n_agents"] == 7).all() and p["n_obst"].min() == 3 and p["n_obst"].max() == 6
    assert (p["dynamics"][:, 0] == scen.DYN_FIRSTORDER).all()  # the stage samplers keep the given ego dynamics
    others = np.concatenate([p["policy"][w, 1:7] for w in range(200)])
    assert set(others) == {5, 1} and abs((others == 1).mean() - 0.2) < 3 * np.sqrt(0.16 / len(others))
    # a single kind draws no kind; a mixture spreads uniformly and leaves each kind's scenarios as that kind alone makes them
    mix = tw.generate(400, 10, 10, [0, 1, 3, 4], seed=9)
    counts = np.bincount(mix["kind"], minlength=5)
    assert counts[2] == 0 and stats.chisquare(counts[[0, 1, 3, 4]]).pvalue > 1e-3
    alone = tw.generate(400, 10, 10, [scen.GEN_STAGE_2], seed=9)
    w = mix["kind"] == scen.GEN_STAGE_2
    assert np.array_equal(mix["agents6"][w], alone["agents6"][w]) and np.array_equal(mix["obstacles"][w], alone["obstacles"][w])


# ---- CPU: the reference's own draws --------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout is only present in the development container")
def test_fixture_reproduces(tmp_path):
    env = dict(os.environ, CAGYM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_samplers.py")], check=True, env=env, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=300)
    assert filecmp.cmp(str(tmp_path / "scenario_samplers.npz"), os.path.join(GOLD, "scenario_samplers.npz"), shallow=False)


def _features(rows, na):
    f = {"start_r": [], "travel": [], "nn_start": [], "nn_goal": []}
    for w in range(len(na)):
        r = rows[w, :na[w]]
        f["start_r"] += list(np.hypot(r[:, 0], r[:, 1]))
        f["travel"] += list(np.hypot(r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]))
        for c, key in ((0, "nn_start"), (2, "nn_goal")):
            d = np.hypot(r[:, None, c] - r[None, :, c], r[:, None, c + 1] - r[None, :, c + 1]) + np.eye(len(r)) * 1e9
            f[key] += list(d.min(1))
    return {k: np.asarray(v) for k, v in f.items()}


def _chi2(a, b):
    bins = np.union1d(np.unique(a), np.unique(b))
    table = np.array([[np.sum(a == v) for v in bins], [np.sum(b == v) for v in bins]])
    return stats.chi2_contingency(table)[1] if len(bins) > 1 else 1.0


@pytest.mark.parametrize("kind", [scen.GEN_SWAP_CIRCLE, scen.GEN_PAIRWISE_SWAP, scen.GEN_STAGE_1, scen.GEN_STAGE_2])
def test_twin_matches_the_reference_distribution(kind):
    z = np.load(os.path.join(GOLD, "scenario_samplers.npz"))
    g = lambda k: z[NAMES[kind] + "__" + k]
    p = tw.generate(1200, 10, 10, [kind], seed=2024 + kind, number_of_agents=FIXTURE_ARGS[kind])
    assert p["n_failed"] == 0
    fr, fm = _features(g("rows"), g("n_agents")), _features(p["agents6"][..., :4], p["n_agents"])
    for k in fr:
        pv = stats.ks_2samp(fr[k], fm[k]).pvalue
        assert pv > 1e-3, (k, pv)
    assert _chi2(g("n_agents"), p["n_agents"]) > 1e-3
    # policies, dynamics and cooperation coefficients: the same assignment as the reference's
    for w in range(len(g("n_agents"))):
        n = g("n_agents")[w]
        assert g("policy")[w, 0] == scen.POLICY_RVO and g("dynamics")[w, 0] == scen.DYN_FIRSTORDER
        assert (g("dynamics")[w, 1:n] == scen.DYN_UNICYCLE).all()
    lp = [g("policy")[w, 1:g("n_agents")[w]] for w in range(len(g("n_agents")))]
    lc = [g("coop")[w, :g("n_agents")[w]] for w in range(len(g("n_agents")))]
    mp = [p["policy"][w, 1:p["n_agents"][w]] for w in range(1200)]
    mc = [p["coop"][w, :p["n_agents"][w]] for w in range(1200)]
    assert set(np.concatenate(lc)) == set(np.concatenate(mc))
    assert all(c[0] == 1.0 for c in lc) and all(c[0] == 1.0 for c in mc)
    fr_nc, fm_nc = (np.concatenate(lp) == scen.POLICY_NONCOOP), (np.concatenate(mp) == scen.POLICY_NONCOOP)
    if kind in SWAPS:
        for f in (fr_nc, fm_nc):
            assert abs(f.mean() - 0.2) < 3 * np.sqrt(0.16 / len(f)), f.mean()
    else:
        assert not fr_nc.any() and not fm_nc.any()
        assert _chi2(g("n_obst"), p["n_obst"]) > 1e-3
        rr = np.concatenate([g("rects")[w, :g("n_obst")[w]] for w in range(len(g("n_obst")))])
        rm = np.concatenate([p["obstacles"][w, :p["n_obst"][w]] for w in range(1200)])
        for c, name in ((2, "xu"), (3, "yu")):
            assert stats.ks_2samp(rr[:, c], rm[:, c]).pvalue > 1e-3, name
        for a, b, name in ((2, 0, "width"), (3, 1, "height")):
            assert stats.ks_2samp(rr[:, a] - rr[:, b], rm[:, a] - rm[:, b]).pvalue > 1e-3, name


def test_the_distribution_test_tells_samplers_apart():
    """power check: the swap-circle rule (1.5 m between positions on a ring) against the reference's pairwise swaps (2 m in a
    square) is rejected by the same test"""
    z = np.load(os.path.join(GOLD, "scenario_samplers.npz"))
    g = lambda k: z["train_agents_pairwise_swap__" + k]
    p = tw.generate(1200, 10, 0, [scen.GEN_SWAP_CIRCLE], seed=77, number_of_agents=8)
    fr, fm = _features(g("rows"), g("n_agents")), _features(p["agents6"][..., :4], p["n_agents"])
    assert stats.ks_2samp(fr["nn_start"], fm["nn_start"]).pvalue < 1e-6


# ---- CPU: the curriculum of _init_agents, the ABI ---------------------------------------------------------------------------
def test_reference_curriculum():
    S, P, R = scen.GEN_SWAP_CIRCLE, scen.GEN_PAIRWISE_SWAP, scen.GEN_RANDOM_POSITIONS
    assert scen.reference_curriculum(0) == ([S], 2)
    assert scen.reference_curriculum(199999) == ([S], 2)
    assert scen.reference_curriculum(2e5) == ([S], 4)
    assert scen.reference_curriculum(1e6) == ([R], 4)  # config.py:91 lists random positions second
    assert scen.reference_curriculum(3e6) == ([P], 6)
    assert scen.reference_curriculum(5e6) == ([P], 6)  # np.random.randint(2, 3) is always 2
    assert scen.reference_curriculum(7e6) == ([P], 8)
    names = scen.TRAINING_SCENARIOS + ("train_stage_1", "train_stage_2")
    assert scen.reference_curriculum(6e6, names) == ([P, scen.GEN_STAGE_1, scen.GEN_STAGE_2], 6)
    with pytest.raises(ValueError, match="train_stage_2"):
        scen.reference_curriculum(0, ("IG_agent_crossing",))


def test_abi_layout():
    L = importlib.import_module("gym-exploration-2d_amd._lib")
    assert C.sizeof(L.CagymGen2Params) == 64 and L.CagymGen2Params.p_b.offset == 56
    lib = L.load()
    for name in ("cagym_generate_reference_scenarios", "cagym_get_obstacles"):
        assert hasattr(lib, name)
    assert lib.cagym_version() == 112


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _env(N, M, S=None, K=10, **kw):
    B = importlib.import_module("gym-exploration-2d_amd.batched_env").BatchedCollisionAvoidanceEnv
    return B(N, M, n_scenarios=S, max_obstacles=K, **kw)


def _download(env):
    d = {k: v.cpu().numpy().copy() for k, v in env.scenarios().items()}
    d.update({k: v.cpu().numpy().copy() for k, v in env.obstacles().items()})
    return d


def _assert_pool_equal(dev, twin, kinds):
    for k in ("policy", "dynamics", "n_agents", "coop", "n_obst", "obstacles"):
        assert np.array_equal(dev[k], twin[k]), k
    trig = np.isin(twin["kind"], [scen.GEN_SWAP_CIRCLE, scen.GEN_STAGE_1, scen.GEN_STAGE_2])
    a, b = dev["agents6"], twin["agents6"]
    assert np.array_equal(a[~trig], b[~trig])
    # fp64 cos / sin of the device and of libm may differ in the last bit; more is a flipped rejection decision
    assert np.abs(a[trig] - b[trig]).max(initial=0.0) <= 1e-12, np.abs(a[trig] - b[trig]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [4, 10])
@pytest.mark.parametrize("kinds", [[0], [1], [2], [3], [4], [0, 1, 2, 3, 4]])
def test_device_equals_twin(M, kinds):
    S = 1000
    K = 10 if M == 10 else 6  # RVO agents among rectangles: at most 6 at max_agents 4, so the stages' 10 is lowered there
    env = _env(8, M, S=S, K=K)
    kw = dict(number_of_agents=M, ego_policy=scen.POLICY_GA3C if M == 10 else scen.POLICY_RVO, n_obst=None if M == 10 else (-1, 6))
    # ten agents among up to ten rectangles: a world can leave no room for the last agent (the reference would loop for ever);
    # such an agent keeps its last draw and is counted, on the device as in the twin
    n_failed = env.generate_reference_scenarios(kinds, seed=31 + M, **kw)
    dev = _download(env)
    twin = tw.generate(S, M, K, kinds, seed=31 + M, **kw)
    assert twin["n_failed"] == n_failed
    _assert_pool_equal(dev, twin, kinds)
    # caller-given policies and rectangle counts
    kw2 = dict(number_of_agents=M - 1, fixed_count=True, other_policies=(scen.POLICY_RVO, scen.POLICY_NONCOOP), p_b=0.3,
               n_obst=(1, 6), other_dynamics=scen.DYN_MAXTURNRATE)
    assert env.generate_reference_scenarios(kinds, seed=7, **kw2) == 0
    _assert_pool_equal(_download(env), tw.generate(S, M, K, kinds, seed=7, **kw2), kinds)
    env.close()


@pytest.mark.gpu
def test_device_equals_twin_in_the_curriculum_stage_mixture():
    """the pool examples/curriculum_pools.py draws from 5e6 steps on: pairwise swaps, stage 1 and stage 2 at max_agents 8, whose
    RVO agents take at most 9 rectangles - stage 2 capped at 9, stage 1 left at randint(0, 4)"""
    names = scen.TRAINING_SCENARIOS + ("train_stage_1", "train_stage_2")
    kinds, n = scen.reference_curriculum(5e6, names)
    assert kinds == [scen.GEN_PAIRWISE_SWAP, scen.GEN_STAGE_1, scen.GEN_STAGE_2] and n == 6
    S, M, K = 1000, 8, 9
    env = _env(8, M, S=S, K=K)
    n_failed = env.generate_reference_scenarios(kinds, 17, number_of_agents=n, n_obst=(-1, 9))
    dev = _download(env)
    twin = tw.generate(S, M, K, kinds, seed=17, number_of_agents=n, n_obst=(-1, 9))
    assert twin["n_failed"] == n_failed
    _assert_pool_equal(dev, twin, kinds)
    s1, s2 = dev["n_obst"][twin["kind"] == scen.GEN_STAGE_1], dev["n_obst"][twin["kind"] == scen.GEN_STAGE_2]
    assert set(s1) == {0, 1, 2, 3, 4} and set(s2) == set(range(2, 10))
    env.close()


@pytest.mark.gpu
def test_device_counts_failures_as_the_twin():
    """max_tries 2: every kind's rejection loops run out often; the device's count equals the twin's, random positions included"""
    S, M, K = 1000, 10, 10
    env = _env(8, M, S=S, K=K)
    kinds = [0, 1, 2, 3, 4]
    n_failed = env.generate_reference_scenarios(kinds, 5, max_tries=2)
    twin = tw.generate(S, M, K, kinds, seed=5, max_tries=2)
    for k in kinds:
        assert twin["failed"][twin["kind"] == k].sum() > 0, k
    assert twin["n_failed"] == n_failed
    _assert_pool_equal(_download(env), twin, kinds)
    env.close()


@pytest.mark.gpu
def test_random_positions_equals_generate_scenarios():
    M, S = 10, 1000
    a, b = _env(8, M, S=S, K=0), _env(8, M, S=S, K=0)
    for seed, fixed, ego in ((5, False, scen.POLICY_RVO), (6, True, scen.POLICY_GA3C)):
        assert a.generate_reference_scenarios("train_agents_random_positions", seed, number_of_agents=M, fixed_count=fixed,
                                              ego_policy=ego, ego_dynamics=scen.DYN_UNICYCLE) == 0
        assert b.generate_scenarios(seed, n_agents=(M if fixed else 2, M), ego_policy=ego,
                                    ego_dynamics=scen.DYN_MAXACC if ego == scen.POLICY_GA3C else scen.DYN_UNICYCLE,
                                    other_policies=(scen.POLICY_RVO, scen.POLICY_NONCOOP), p_b=0.5, coop=0.5) == 0
        da, db = a.scenarios(), b.scenarios()
        for k in da:
            assert np.array_equal(da[k].cpu().numpy(), db[k].cpu().numpy()), (seed, k)
    a.close(); b.close()


@pytest.mark.gpu
def test_generated_stage2_pool_drives_the_env_like_an_upload():
    """S = 2N (auto-reset changes scenario), GA3C ego, 80/20 RVO / NonCooperative among stage-2 rectangles, LaserScan: the device
    prep rows, rasters and handle flags give what set_scenarios gives for the same pool"""
    import torch
    N, M, K = 64, 10, 10
    gen = _env(N, M, S=2 * N, K=K, laserscan=True)
    assert gen.generate_reference_scenarios("train_stage_2", 4242, ego_policy=scen.POLICY_GA3C,
                                            other_policies=(scen.POLICY_RVO, scen.POLICY_NONCOOP), p_b=0.2) == 0
    pool = _download(gen)
    assert pool["n_obst"].min() >= 2 and (pool["policy"] == scen.POLICY_NONCOOP).any()
    up = _env(N, M, S=2 * N, K=K, laserscan=True)
    up.set_scenarios(pool["agents6"], pool["policy"], pool["dynamics"], n_agents=pool["n_agents"], coop=pool["coop"],
                     obstacles=pool["obstacles"], n_obst=pool["n_obst"])
    assert torch.equal(gen.state()["map_bits"], up.state()["map_bits"])
    outs = []
    for e in (gen, up):
        e.attach_ga3c()
        e.reset()
        tr = e.rollout(64, auto_reset=True)
        obs, rew, go, info = e.step()
        outs.append((tr, {k: v.clone() for k, v in obs.items()}, rew.clone(), go.clone(), info["flags"].clone(),
                     {k: v.clone() for k, v in e.episode_stats().items()}))
    torch.cuda.synchronize()
    (t1, o1, r1, g1, f1, s1), (t2, o2, r2, g2, f2, s2) = outs
    for k in t1:
        assert torch.equal(t1[k], t2[k]), k
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    assert torch.equal(r1, r2) and torch.equal(g1, g2) and torch.equal(f1, f2)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert int(s1["stat_episodes"].sum()) > 0
    gen.close(); up.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["train_stage_1", "train_stage_2"])
def test_generated_obstacle_pool_matches_the_oracle(kind):
    from oracle import oracle as orc
    from test_cfg4 import _laser_close
    from test_hip_parity import _compare_batch, _hip
    N, M, K, T = 64, 10, 10, 60
    hip = _hip(N=N, M=M, max_obstacles=K, game_over_mode=1, laserscan=True)
    assert hip.env.generate_reference_scenarios(kind, 99, ego_policy=scen.POLICY_RVO) == 0
    pool = _download(hip.env)
    assert (pool["n_obst"] > 0).any() and (pool["policy"] == scen.POLICY_RVO).sum() > N
    name = hip.env.kernel_name(rollout=False, auto_reset=False)
    assert name.startswith("k_step3<") and name.endswith(", false, true>"), name  # the OBST specialisation
    cpu = orc.OracleEnv(N=N, M=M, max_obstacles=K, game_over_mode=1, laserscan=True)
    cpu.set_scenario(pool["agents6"], pool["policy"], pool["dynamics"], n_agents=pool["n_agents"], coop=pool["coop"],
                     obstacles=pool["obstacles"], n_obst=pool["n_obst"])
    hip.reset()
    cpu.reset()
    _compare_batch(hip, cpu, N, M, 0)
    _laser_close(hip, cpu, 0)
    for t in range(T):
        hip.step()
        cpu.step()
        assert np.abs(hip.f("action") - cpu.f("action")).max() <= 2e-7, ("action", t)
        _compare_batch(hip, cpu, N, M, t + 1, ftol=1e-7)
        _laser_close(hip, cpu, t + 1)
    hip.env.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    import torch
    L = importlib.import_module("gym-exploration-2d_amd._lib")
    M, K = 4, 7  # max_agents 4 takes at most 6 rectangles among RVO agents
    env, ctl = _env(16, M, S=32, K=K), _env(16, M, S=32, K=K)  # ctl: the same calls without the refused ones
    for e in (env, ctl):
        assert e.generate_reference_scenarios("train_stage_2", 1, n_obst=(2, 7), ego_policy=scen.POLICY_NONCOOP,
                                              other_policies=scen.POLICY_NONCOOP) == 0  # no RVO agent: 7 rectangles are fine
        e.reset()
        e.rollout(8, auto_reset=True)
    before = _download(env)
    flags = (env._pool_policies, env._n_ig)

    def refused(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            env.generate_reference_scenarios(*a, **kw)
        after = _download(env)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        assert (env._pool_policies, env._n_ig) == flags

    refused("train_stage_2 \\(up to 10\\) exceeds the handle's max_obstacles", "train_stage_2", 2)  # the reference's 10 > 7
    refused("train_stage_2 \\(up to 10\\) exceeds", [3, 4], 2)  # stage 1 (up to 4) is within it, stage 2 is not
    refused("n_obst_max exceeds", "train_stage_1", 2, n_obst=(0, K + 1))
    refused("n_obst_min exceeds", "train_stage_2", 2, n_obst=(5, 3))
    refused("leave train_stage_2 no rectangle count", "train_stage_2", 2, n_obst=(0, 1))  # stage 2 draws 2..10
    refused("leave train_stage_1 no rectangle count", [3, 4], 2, n_obst=(5, 7))          # stage 1 draws 0..4
    # RVO agents among 7 rectangles at max_agents 4: the message of set_scenarios
    with pytest.raises(RuntimeError) as up:
        env.set_scenarios(before["agents6"], scen.POLICY_RVO, scen.DYN_UNICYCLE, n_agents=before["n_agents"],
                          obstacles=before["obstacles"], n_obst=before["n_obst"])
    msg = str(up.value).split(": ", 1)[1]
    assert "too many rectangles" in msg
    refused(re.escape(msg), "train_stage_2", 2, n_obst=(2, 6))  # the handle's max_obstacles decides, not n_obst_max
    refused("max_agents", "train_agents_swap_circle", 2, number_of_agents=M + 1)
    refused("policy id", "train_stage_1", 2, ego_policy=9)
    refused("dynamics id", "train_stage_1", 2, other_dynamics=7)
    refused("bad generator", "train_stage_1", 2, max_tries=0)
    with pytest.raises(ValueError, match="no device sampler"):
        env.generate_reference_scenarios("IG_agent_crossing", 2)
    for mask in (0, 1 << 5):  # the raw entry: an empty or unknown kind
        P = L.CagymGen2Params(2, mask, M, 0, 5, 4, 0, 5, 1, 0, -1, -1, 100, 0.0)
        assert env.L.cagym_generate_reference_scenarios(env.h, C.byref(P), None, env._stream()) == -1
    # the handle goes on exactly as the one that saw none of the refused calls
    outs = []
    for e in (env, ctl):
        e.reset()
        outs.append(e.rollout(8, auto_reset=True))
    torch.cuda.synchronize()
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(env.state()["episode"], ctl.state()["episode"])
    assert before["n_obst"].max() <= K and (before["policy"] != scen.POLICY_RVO).all()
    env.close(); ctl.close()


@pytest.mark.gpu
def test_curriculum_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "curriculum_pools.py"), "--worlds", "64", "--pool", "128",
                        "--redraw", "32", "--steps", "64", "--start", "5e6", "--stages"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "curriculum done" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("kinds 1,3,4 ") == 2 and " rejected 0 " in r.stdout, r.stdout  # the stage mixture, RVO among 9 rectangles
