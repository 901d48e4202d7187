"""GPU: the OtherAgentsStates rows of the generation-3 kernels - the dense row index (wpw M (M - 1) rows in chunks of 64, no lane
for a self pair) and the integer rank with its wave-level fallback to the fp64 definition (csrc/cagym_oas_rank.h).

rollout(T) == T x step(auto_reset=True) == the generation-1 kernels (CAGYM_KERNEL=v1: one lane per agent, a serial rank), byte for
byte on every output tensor, and the rows of every step against the CPU oracle (golden_util.oas_mismatch).  T = 12.  Shapes:

  - M = 10: N = 9 with 4 worlds per workgroup (three workgroups, the last with one world; 360 rows = 5 chunks and 40 rows), N = 11
    with 5 (450 rows);
  - M = 4, N = 17: 192 rows, exactly three full chunks, and a last workgroup with one world;
  - M = 20, N = 3: 760 rows, a last workgroup with one world;
  - run-time M = 7 and 13 (odd: a padding key in every key row), N = 5.

Every handle mixes random RVO worlds, a lattice world of lp_worlds.py (exactly tied keys between agents on the lattice), a world
with fewer agents than M (zero rows) and two hand-made static scenes that force the fallback: an ego with other agents of its
radius at (+-2, 0), (0, +-2) - keys tied exactly by the symmetry of the operands - and an ego overlapped by three agents, two of
them mirror images (a tie among negative keys), one deeper.  The keys of those rows are computed here from the positions and the
test asserts what it relies on: a row with a tie of at least 3 keys and a row with at least 2 negative keys in every handle."""
import numpy as np
import pytest

import golden_util as gu
import lp_worlds as lw
from oracle import oracle as orc
from test_hip_parity import _hip
from test_rollout_sync import OUT, _status_clean

scen = lw.scen
pytestmark = pytest.mark.gpu
T = 12
KEYS = [k for k in OUT if k != "laserscan"]
FAR = 12.0  # m from the scenes to the parked agents and the walker


def _parked(M):
    """M Static agents in a row far from everything"""
    a6 = np.zeros((M, 6))
    a6[:, 0] = -FAR + 0.875 * np.arange(M)
    a6[:, 1] = FAR
    a6[:, 2:4] = a6[:, 0:2] - [0.0, 1.0]
    a6[:, 4], a6[:, 5] = 1.0, 0.25
    return a6, np.full(M, scen.POLICY_STATIC, dtype=np.int32)


def _place(a6, at, cx, scene):
    """Static agents of radius 0.5 at cx + the scene's positions, from slot `at` on -> the next free slot"""
    for k, (x, y) in enumerate(scene):
        a6[at + k] = [cx + x, y, cx + x, y - 1.0, 1.0, 0.5]
    return at + len(scene)


def _tie_scene(M):
    # the ego and agents at distance 2 exactly (dx dx + dy dy = 4 whatever the order of the operands): three of them when M = 4
    return [(0.0, 0.0), (2.0, 0.0), (-2.0, 0.0), (0.0, 2.0), (0.0, -2.0)][:min(5, M)]


OVERLAP_SCENE = [(0.0, 0.0), (0.625, 0.3125), (0.625, -0.3125), (-0.25, 0.0)]  # two mirror images and a deeper one


def _hand_world(M, scenes):
    """the scenes side by side (8 m apart) and somebody who is not done, so that the world does not end: a NonCooperative walker far
    away, or, when no slot is left (M = 4), the scene's ego as a NonCooperative agent of preferred speed 0 - it turns on the spot,
    its position is added +-0 per step and stays what it is bit for bit, and as the lowest slot it does not collide with the
    Static agents on top of it -> (a6, policy, agents used)"""
    a6, pol = _parked(M)
    at = 0
    for k, s in enumerate(scenes):
        at = _place(a6, at, 8.0 * k, s)
    if at < M:
        a6[at] = [-FAR, -FAR, FAR, -FAR, 1.0, 0.5]
        pol[at] = scen.POLICY_NONCOOP
        at += 1
    else:
        a6[0, 4] = 0.0
        pol[0] = scen.POLICY_NONCOOP
    return a6, pol, at


def _pool(N, M, seed):
    rng = np.random.default_rng(seed)
    rnd = scen.random_worlds_fast(N, M, seed=seed)
    worlds, n_agents, hand = [], [], []
    rvo, half = np.full(M, scen.POLICY_RVO, dtype=np.int32), np.full(M, 0.5)
    if N >= 5:
        plan = ["tie", "overlap", "lattice", "few"] + ["random"] * (N - 4)
    else:
        plan = ["tie+overlap", "lattice", "random"][:N]
    for w, kind in enumerate(plan):
        if kind in ("tie", "overlap", "tie+overlap"):
            scenes = {"tie": [_tie_scene(M)], "overlap": [OVERLAP_SCENE], "tie+overlap": [_tie_scene(M), OVERLAP_SCENE]}[kind]
            a6, pol, used = _hand_world(M, scenes)
            n = min(M, used + 1) if kind == "tie+overlap" else M  # (the combined world is also the one with fewer agents than M)
            worlds.append((a6, pol, half))
            n_agents.append(n)
            hand.append((w, n))
        elif kind == "lattice":
            a6, pol, coop, _, _ = lw.lattice_world(rng, M, False)
            worlds.append((a6, pol, coop))
            n_agents.append(M)
        else:
            worlds.append((rnd[w], rvo, half))
            n_agents.append(max(2, M - 2) if kind == "few" else M)
    a6, pol, coop = (np.stack([w[k] for w in worlds]) for k in range(3))
    pool = dict(agents6=a6, policy_id=pol, dynamics_id=scen.DYN_UNICYCLE, n_agents=np.array(n_agents, dtype=np.int32), coop=coop)
    return pool, hand


def _host_keys(a6, n):
    """the sort keys of every row of a world of Static agents: (d - r_ego) - r_other, d = sqrt(dx dx + dy dy), fp64"""
    p, r = a6[:n, 0:2], a6[:n, 5]
    d = np.sqrt((p[None, :, 0] - p[:, None, 0]) ** 2 + (p[None, :, 1] - p[:, None, 1]) ** 2)
    k = (d - r[:, None]) - r[None, :]
    k[np.arange(n), np.arange(n)] = -np.inf
    return k


def _assert_forces_the_fallback(pool, hand):
    ties = negatives = 0
    for w, n in hand:
        assert (pool["policy_id"][w][:n] != scen.POLICY_RVO).all()
        for row in _host_keys(pool["agents6"][w], n):  # (Static agents: these are the keys of every step; a walker's own differ)
            live = row[row > -np.inf]
            _, counts = np.unique(live, return_counts=True)
            ties += int(counts.max(initial=0) >= 3)
            negatives += int((live < 0).sum() >= 2)
    assert ties >= 1 and negatives >= 1, (ties, negatives)


def _forms_agree(N, M, wpw10, kernel, monkeypatch):
    import torch
    pool, hand = _pool(N, M, seed=4100 + 16 * M + N)
    _assert_forces_the_fallback(pool, hand)
    assert (pool["n_agents"] < M).any()
    if wpw10:
        monkeypatch.setenv("CAGYM_WPW10", wpw10)
    envs = {}
    for k in ("roll", "ref", "v1"):
        if k == "v1":
            monkeypatch.setenv("CAGYM_KERNEL", "v1")
        e = _hip(N=N, M=M, game_over_mode=1)
        e.set_scenario(**pool)
        e.reset()
        envs[k] = e.env
    monkeypatch.delenv("CAGYM_KERNEL", raising=False)
    cpu = orc.OracleEnv(N=N, M=M, game_over_mode=1)
    cpu.set_scenario(**pool)
    cpu.reset()
    roll, ref, v1 = envs["roll"], envs["ref"], envs["v1"]
    if kernel:
        assert roll.kernel_name(rollout=True, auto_reset=True) == kernel
    tr = roll.rollout(T, auto_reset=True)
    tr1 = v1.rollout(T, auto_reset=True)
    worst = 0.0
    for t in range(T):
        ref.step(auto_reset=True)
        cpu.step()
        assert not cpu.u("game_over").any(), ("a world of the pool ends inside the test: the oracle does not restart it", t)
        for k in KEYS:
            assert torch.equal(tr[k][t], getattr(ref, OUT[k])), ("rollout against step()", k, t)
            assert torch.equal(tr1[k][t], tr[k][t]), ("generation 1 against the rollout", k, t)
        a, b, nobs = tr["other_agents_states"][t].cpu().numpy(), cpu.f("oas"), cpu.i("num_other_agents_observed")
        for w in range(N):
            worst = max(worst, gu.oas_mismatch(a[w], b[w], nobs[w], tol=1e-5, key_tie=1e-5)[0])
    print("largest difference of an OtherAgentsStates entry from the oracle's: %.2e" % worst)
    assert worst <= 1e-5
    torch.cuda.synchronize()
    for name, e in envs.items():
        for f, v in ref.state().items():
            if name != "ref" and f != "map_bits":
                assert torch.equal(e.state()[f], v), (name, "state", f)
    _status_clean(roll, ref)
    v1.rollout(1)
    torch.cuda.synchronize()
    v1.close()


@pytest.mark.parametrize("N,M,wpw10,kernel", [
    (9, 10, "4", "k_rollout3<256, 10, 4, true, false>"),
    (11, 10, "5", "k_rollout3<256, 10, 5, true, false>"),
    (17, 4, None, "k_rollout3<256, 4, 0, true, false>"),
    (3, 20, None, "k_rollout3<256, 20, 2, true, false>"),
    (5, 7, None, "k_rollout3<256, 0, 0, true, false>"),
    (5, 13, None, "k_rollout3<512, 0, 0, true, false>")])
def test_rows_of_every_form_agree(N, M, wpw10, kernel, monkeypatch):
    _forms_agree(N, M, wpw10, kernel, monkeypatch)
