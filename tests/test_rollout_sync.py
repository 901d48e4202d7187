"""The roll-out kernel's step boundary (csrc/cagym_kernels3.h: run_steps3) against the one-step launch: rollout(T) ==
T x step(auto_reset=True), byte for byte, on every output and on the state, at the smallest shapes where the synchronisation
between the waves of a workgroup can go wrong - two workgroups (the second with one world), launches of 1, 2 and 3 steps (first
step without rows, first step with rows, one full period) and one long enough for many restarts, every kernel specialisation,
a handle without LP waves, a workgroup with more busy egos than one LP wave (and than one round of LP groups) holds, and the
rectangle kernels with the LaserScan's claim counters.  The output slices of a step are computed where they are consumed (row
workers: step t - 1, S2: step t) and the restart / lagging flags travel in one read at the step's end: a slice or a flag taken
from the wrong step shows here.  Every case ends with one more launch per handle: a bounded wait that gave up
(CagymDev::dev_status) would make it raise."""
import importlib

import numpy as np
import pytest

from test_hip_parity import _hip

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")
pytestmark = pytest.mark.gpu

OUT = {"reward": "reward", "flags": "flags", "game_over": "game_over", "other_agents_states": "obs_oas", "ego": "obs_ego",
       "laserscan": "obs_laser"}
SCHEDULE = (1, 2, 3, 40, 1, 1, 1, 1, 1, 1, 2, 3)  # launches of one pair of handles, each from where the last one ended


def _short_trip_pool(S, M, seed, side):
    """A crowd in a small square (RVO egos with violated half-planes from the first step on) whose agent 0 has 0.12 .. 0.6 m to
    go: with game over = "agent 0 done" every world restarts every few steps, so restarts fall inside every launch."""
    a6 = scen.random_worlds_fast(S, M, seed=seed, side=side, min_travel=2.0, min_sep=1.2)
    rng = np.random.default_rng(seed)
    d = a6[:, 0, 2:4] - a6[:, 0, 0:2]
    d /= np.hypot(d[:, 0], d[:, 1])[:, None]
    a6[:, 0, 2:4] = a6[:, 0, 0:2] + d * rng.uniform(0.12, 0.6, S)[:, None]
    return a6


def _handles(N, M, S, K, laser, **pool):
    envs = []
    for _ in range(2):
        e = _hip(N=N, M=M, max_obstacles=K, game_over_mode=0, laserscan=laser, n_scenarios=S)
        e.set_scenario(**pool)
        e.reset()
        envs.append(e.env)
    return envs


def _rollout_equals_steps(roll, ref, schedule, laser=False, each_step=None):
    """rollout(T) on `roll` against T x step(auto_reset=True) on `ref`, launch after launch; returns the restarts seen per T"""
    import torch
    keys = [k for k in OUT if k != "laserscan" or laser]
    restarts = {}
    for n, T in enumerate(schedule):
        tr = roll.rollout(T, auto_reset=True)
        for t in range(T):
            ref.step(auto_reset=True)
            for k in keys:
                assert torch.equal(tr[k][t], getattr(ref, OUT[k])), (k, "launch %d of %d steps" % (n, T), t)
            restarts[T] = restarts.get(T, 0) + int(ref.game_over.sum())
            if each_step is not None:
                each_step(ref)
        torch.cuda.synchronize()
        sr, se = roll.state(), ref.state()
        for f in se:
            if f != "map_bits":
                assert torch.equal(sr[f], se[f]), ("state", f, "launch %d of %d steps" % (n, T))
    return restarts


def _status_clean(*envs):
    """dev_status is sticky and every launching entry point refuses to go on once it is set"""
    import torch
    torch.cuda.synchronize()
    for e in envs:
        e.rollout(1)
        e.step()
    torch.cuda.synchronize()
    for e in envs:
        e.close()


@pytest.mark.parametrize("N,M,kernel", [(5, 10, "k_rollout3<256, 10, 4, true, false>"), (3, 20, "k_rollout3<256, 20, 2, true, false>"),
                                        (9, 4, "k_rollout3<256, 4, 0, true, false>"), (3, 7, "k_rollout3<256, 0, 0, true, false>")])
def test_rollout_equals_steps_with_restarts_in_every_launch(N, M, kernel, monkeypatch):
    if M == 10:
        monkeypatch.setenv("CAGYM_WPW10", "4")  # two workgroups, the second with one world
    S = 8 * N
    a6 = _short_trip_pool(S, M, seed=700 + M, side=3.0 if M <= 10 else 4.5)
    roll, ref = _handles(N, M, S, 0, False, agents6=a6, policy_id=scen.POLICY_RVO, dynamics_id=scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5))
    assert roll.kernel_name(rollout=True, auto_reset=True) == kernel
    restarts = _rollout_equals_steps(roll, ref, SCHEDULE)
    print(kernel, "restarts by launch length", restarts)
    assert all(restarts[T] > 0 for T in (1, 2, 3, 40)), restarts
    _status_clean(roll, ref)


def test_rollout_without_any_rvo_agent(monkeypatch):
    """no LP wave at all (lp_waves == 0): S1 follows the step's top directly"""
    monkeypatch.setenv("CAGYM_WPW10", "4")
    N, M, S = 5, 10, 40
    a6 = _short_trip_pool(S, M, seed=11, side=3.0)
    roll, ref = _handles(N, M, S, 0, False, agents6=a6, policy_id=scen.POLICY_NONCOOP, dynamics_id=scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5))
    restarts = _rollout_equals_steps(roll, ref, (8,))
    assert restarts[8] > 0, restarts
    _status_clean(roll, ref)


def test_rollout_with_more_busy_egos_than_one_lp_wave(monkeypatch):
    """Antipodal swaps on small circles: every ego of a world is in the crowd at once.  An ego whose commanded speed is below its
    preferred speed had its linear program change the preferred velocity, so it was busy (a proxy read from the state: the kernel
    does not export its busy count): more than 8 of them in the first workgroup (worlds 0 .. 3) need the second LP wave, more than
    32 a second round of LP groups.  Both are asserted."""
    monkeypatch.setenv("CAGYM_WPW10", "4")
    N, M, S = 5, 10, 15
    rng = np.random.default_rng(5)
    a6 = np.stack([scen.circle_world(M, r) for r in rng.uniform(2.0, 3.0, S)])
    a6[:, :, 0:4] += rng.uniform(-0.02, 0.02, (S, M, 4))  # no exact symmetry
    roll, ref = _handles(N, M, S, 0, False, agents6=a6, policy_id=scen.POLICY_RVO, dynamics_id=scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5))
    assert roll.kernel_name(rollout=True, auto_reset=True) == "k_rollout3<256, 10, 4, true, false>"
    slowed = []

    def count(env):
        s = env.state()
        slow = (s["action"][:4, :, 0].double() < s["pref_speed"][:4] - 1e-4) & (s["status"][:4] & 8 == 0)
        slowed.append(int(slow.sum()))
    _rollout_equals_steps(roll, ref, (40,), each_step=count)
    print("slowed egos of workgroup 0 per step", slowed)
    assert max(slowed) > 32, slowed  # (> 8: the second LP wave; > 32: a second round of the 32 LP groups)
    _status_clean(roll, ref)


def test_rollout_among_rectangles_with_laserscan(monkeypatch):
    """OBST: the LaserScan's claim counters and the row-claim counter start again between the two barriers of every step; the
    one-step launch and the roll-out pin each other"""
    monkeypatch.setenv("CAGYM_WPW10", "4")
    N, M, K, S = 5, 10, 2, 15
    a6, obst, n_obst, _ = scen.obstacle_worlds(S, M, K, seed=77)
    assert (n_obst == K).all()
    roll, ref = _handles(N, M, S, K, True, agents6=a6, policy_id=scen.POLICY_RVO, dynamics_id=scen.DYN_UNICYCLE, coop=np.full((S, M), 0.5),
                         obstacles=obst, n_obst=n_obst)
    assert roll.kernel_name(rollout=True, auto_reset=True) == "k_rollout3<256, 10, 4, true, true>"
    _rollout_equals_steps(roll, ref, (6,), laser=True)
    _status_clean(roll, ref)
