"""The roll-out kernel's fused pair phase (csrc/cagym_kernels3.h: pair_phase3) against the one-step launch, which keeps the two
barrier-separated phases: rollout(T) == T x step(auto_reset=True), byte for byte, on every output and on the state.  In the
fused phase the pair lanes of waves 1.. store distances and ranking keys, build their half-planes and rank them behind two LDS
arrival counters instead of a barrier, while wave 0 prepares the LP inputs, updates the ego frames and runs S2 behind the pair
waves' counter: a key, a collision bit, an LP start or a restart taken too early shows as a differing byte.  The cases are the
smallest that reach every path of the phase - a second workgroup with one world, worlds with inactive slots, a handle without
RVO agents (the pair lanes arrive and build nothing), mixed policies, more busy egos than one LP wave holds - and the shapes
that stay on the two-phase code (5 worlds per workgroup, M = 7, M = 20).  Worlds restart inside the launches, and every case has
steps in which no world of the first workgroup restarts: only those consume the half-planes the fused phase built.  Every case ends with one more launch per handle: a bounded wait that gave up (CagymDev::dev_status) would make it raise."""
import importlib

import numpy as np
import pytest

from test_rollout_sync import _handles, _rollout_equals_steps, _status_clean

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
pytestmark = pytest.mark.gpu

SCHEDULE = (1, 2, 3, 33, 1, 2, 3, 33)  # launches of one pair of handles, each from where the last one ended


def _trip_pool(S, M, seed, side, trip):
    """A crowd in a small square whose agent 0 has trip[0] .. trip[1] m to go (the goal counts as reached within 0.75 m, a step is
    0.1 m at most): with game over = "agent 0 done" a world restarts every 1 .. 10 steps when trip = (0.8, 1.7), so restarts fall inside the launches AND a
    workgroup has steps without one - only those consume the half-planes of the fused phase (a restart rebuilds them)."""
    a6 = scen.random_worlds_fast(S, M, seed=seed, side=side, min_travel=2.0, min_sep=1.2)
    rng = np.random.default_rng(seed)
    d = a6[:, 0, 2:4] - a6[:, 0, 0:2]
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    a6[:, 0, 2:4] = a6[:, 0, 0:2] + d * rng.uniform(trip[0], trip[1], S)[:, None]
    return a6


def _run(N, M, kernel, wpw10, monkeypatch, seed, side=3.0, each_step=None, wg=4, trip=(0.8, 1.7), **pool):
    if wpw10:
        monkeypatch.setenv("CAGYM_WPW10", wpw10)
    S = 8 * N
    pool.setdefault("agents6", _trip_pool(S, M, seed=seed, side=side, trip=trip))
    pool.setdefault("policy_id", scen.POLICY_RVO)
    roll, ref = _handles(N, M, S, 0, False, dynamics_id=scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5), **pool)
    assert roll.kernel_name(rollout=True, auto_reset=True) == kernel
    first = []  # restarts per step among the wg worlds of the first workgroup

    def count(env):
        first.append(int(env.game_over[:wg].sum()))
        if each_step is not None:
            each_step(env)
    restarts = _rollout_equals_steps(roll, ref, SCHEDULE, each_step=count)
    print(kernel, "restarts by launch length", restarts, "steps of the first workgroup without / with a restart",
          first.count(0), len(first) - first.count(0))
    assert restarts[33] > 0, restarts
    assert 0 < first.count(0) < len(first), first  # steps whose half-planes come from the phase under test, and steps rebuilt
    _status_clean(roll, ref)


def test_two_workgroups_second_with_one_world(monkeypatch):
    _run(5, 10, "k_rollout3<256, 10, 4, true, false>", "4", monkeypatch, seed=810)


def test_worlds_with_inactive_slots(monkeypatch):
    """2 .. 10 agents per world: pair lanes whose higher slot is inactive store 'no neighbour' keys and build no half-plane"""
    N, M = 5, 10
    S = 8 * N
    n_agents = np.resize(np.arange(2, M + 1), S)
    np.random.default_rng(3).shuffle(n_agents)
    _run(N, M, "k_rollout3<256, 10, 4, true, false>", "4", monkeypatch, seed=811, n_agents=n_agents)


def test_no_rvo_agent_pair_lanes_arrive_without_half_planes(monkeypatch):
    _run(5, 10, "k_rollout3<256, 10, 4, true, false>", "4", monkeypatch, seed=812, policy_id=scen.POLICY_NONCOOP)


def test_mixed_policies(monkeypatch):
    """RVO, static and non-cooperative agents side by side (agent 0, whose arrival ends the episode, is an RVO agent)"""
    N, M = 5, 10
    S = 8 * N
    pol = np.random.default_rng(4).choice([scen.POLICY_RVO, scen.POLICY_STATIC, scen.POLICY_NONCOOP], size=(S, M)).astype(np.int32)
    pol[:, 0] = scen.POLICY_RVO
    _run(N, M, "k_rollout3<256, 10, 4, true, false>", "4", monkeypatch, seed=813, policy_id=pol)


def test_crowd_with_more_busy_egos_than_one_lp_wave(monkeypatch):
    """A dense crowd in a small square: an ego whose commanded speed is below its preferred speed had its linear program change
    the preferred velocity, so it was busy (a proxy read from the state, as in test_rollout_sync.py): more than 8 of them in
    the first workgroup (worlds 0 .. 3) need a second LP wave, so wave 0 and the pair lanes meet LP waves of different length."""
    slowed = []

    def count(env):
        s = env.state()
        slow = (s["action"][:4, :, 0].double() < s["pref_speed"][:4] - 1e-4) & (s["status"][:4] & 8 == 0)
        slowed.append(int(slow.sum()))
    _run(5, 10, "k_rollout3<256, 10, 4, true, false>", "4", monkeypatch, seed=814, side=2.4, each_step=count)
    print("slowed egos of workgroup 0 per step", slowed)
    assert max(slowed) > 8, slowed


@pytest.mark.parametrize("N,M,kernel,wpw10,wg", [(6, 10, "k_rollout3<256, 10, 5, true, false>", "5", 5),
                                                 (17, 4, "k_rollout3<256, 4, 0, true, false>", None, 16),
                                                 (10, 7, "k_rollout3<256, 0, 0, true, false>", None, 9),
                                                 (3, 20, "k_rollout3<256, 20, 2, true, false>", None, 2)])
def test_other_shapes_agree(N, M, kernel, wpw10, wg, monkeypatch):
    """M = 4 (16 worlds per workgroup: 96 pairs on waves 1 and 2, wave 3 arrives without a pair) takes the fused phase as well; 5
    worlds of 10 agents per workgroup (225 pairs: a second pass), the run-time-M kernel and M = 20 keep the two phases"""
    _run(N, M, kernel, wpw10, monkeypatch, seed=820 + M, side=3.0 if M <= 10 else 4.5, wg=wg, trip=(0.8, 3.0) if M == 4 else (0.8, 1.7))
