"""GPU: the linearProgram1 round of the LP groups (csrc/cagym_orca.h: orca_lp1_group - the chord through the lane reductions, the next
violated line as a group minimum, the paired DPP reductions, the clamp by max and min; orca_lp_group - the stored LP start and the
one read of lane 0's second line) on the headline specialisation and its neighbours.

rollout(T) == T x step(auto_reset=True) == the generation-1 kernels (CAGYM_KERNEL=v1: one lane per agent, serial linearProgram1 / 2 /
3, no lane reduction at all), byte for byte: the trajectories' rewards, flags, game-over bits and observations step by step, the
state and its episode statistics at the end.  Every case ends with one more launch per handle: a bounded wait that gave up
(CagymDev::dev_status) would make it raise.

  - the M = 10 LP pool of lp_worlds.py (its first 9 worlds: every hand-made scene and a lattice world) on 9 worlds x 10 agents: two
    full workgroups and a third with one world;
  - pools with exactly 1, 9 and 17 busy egos per full workgroup in every step: one partly filled LP wave, a full one and one group,
    two full ones and one group.  The DPP reads of a group count on the whole group being there and on nothing else: the other
    groups of the wave are switched off.  The scenes are built here - walkers with a Static agent in their way, everybody else
    Static - and the oracle counts the busy egos (an ego with a half-plane that its start velocity violates) step by step;
  - M = 4 (groups of 4 lanes, no second slot) and M = 20 (groups of 16 lanes, two slots per lane), each at the smallest N with
    two workgroups, on worlds of their LP pools."""
import numpy as np
import pytest

import lp_worlds as lw
from oracle import oracle as orc
from test_hip_parity import _hip
from test_kernel_matrix import _n_worlds
from test_rollout_sync import OUT, _status_clean

scen = lw.scen
pytestmark = pytest.mark.gpu
f32 = np.float32
T = lw.T_STEPS
KEYS = [k for k in OUT if k != "laserscan"]
HEADLINE = "k_rollout3<256, 10, 4, true, false>"


def _worlds(pool, idx):
    """the worlds `idx` (a count: the first ones) of a pool"""
    idx = np.arange(idx) if np.isscalar(idx) else np.asarray(idx)
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in pool.items()}


def _forms_agree(pool, N, M, kernel, monkeypatch, steps=T):
    import torch
    if M == 10:
        monkeypatch.setenv("CAGYM_WPW10", "4")
    envs = {}
    for k in ("roll", "ref", "v1"):
        if k == "v1":
            monkeypatch.setenv("CAGYM_KERNEL", "v1")
        e = _hip(N=N, M=M, game_over_mode=1)
        e.set_scenario(**pool)
        e.reset()
        envs[k] = e.env
    monkeypatch.delenv("CAGYM_KERNEL", raising=False)
    roll, ref, v1 = envs["roll"], envs["ref"], envs["v1"]
    assert roll.kernel_name(rollout=True, auto_reset=True) == kernel
    tr = roll.rollout(steps, auto_reset=True)
    tr1 = v1.rollout(steps, auto_reset=True)  # (generation 1 restarts worlds in its roll-out only)
    for t in range(steps):
        ref.step(auto_reset=True)
        for k in KEYS:
            assert torch.equal(tr[k][t], getattr(ref, OUT[k])), ("rollout against step()", k, t)
            assert torch.equal(tr1[k][t], tr[k][t]), ("generation 1 against the rollout", k, t)
    torch.cuda.synchronize()
    for name, e in envs.items():
        for f, v in ref.state().items():
            if name != "ref" and f != "map_bits":
                assert torch.equal(e.state()[f], v), (name, "state", f)
    _status_clean(roll, ref)
    v1.rollout(1)
    torch.cuda.synchronize()
    v1.close()


def test_headline_kernel_on_the_lp_pool(monkeypatch):
    N, M = 9, 10
    pool, info = lw.build_pool(M, _n_worlds(M, 4), False)
    assert info["n_scenes"] < N  # every scene of the pool and a lattice world
    _forms_agree(_worlds(pool, N), N, M, HEADLINE, monkeypatch)


# ---- pools with a chosen number of busy egos per workgroup -------------------------------------------------------------------
PITCH = 8.0  # m between the walkers of one world: at 1 m/s and a time horizon of 5 s nobody meets another pair


def _walker_world(pairs, M, seed):
    """`pairs` RVO walkers, each with a Static agent 1.3 .. 1.75 m ahead and 0.1 .. 0.4 m off its path to a goal 8 m away, every
    other slot a Static agent in a row far off"""
    rng = np.random.default_rng(seed)
    a6 = np.zeros((M, 6))
    a6[:, 0] = -40.0 + 2.0 * np.arange(M)
    a6[:, 1] = 40.0
    a6[:, 2:4] = a6[:, 0:2] - [0.0, 1.0]
    a6[:, 4], a6[:, 5] = 1.0, 0.25
    pol = np.full(M, scen.POLICY_STATIC, dtype=np.int32)
    for p in range(pairs):
        y = PITCH * p
        ahead, off = 1.3 + 0.0625 * rng.integers(0, 8), (0.1 + 0.0625 * rng.integers(0, 5)) * rng.choice([-1.0, 1.0])
        a6[2 * p] = [0.0, y, 8.0, y, 1.0, 0.4375]
        a6[2 * p + 1] = [ahead, y + off, ahead, y + off - 1.0, 1.0, 0.4375]
        pol[2 * p] = scen.POLICY_RVO
    return a6, pol, np.full(M, 0.5), np.zeros((lw.K_RECT, 4)), 0


def _busy_pool(busy, N, M, wpw):
    """N worlds in workgroups of wpw: `busy` walkers in every full workgroup (as many per world as fit, first worlds first), one in
    the last, ragged one"""
    worlds = []
    for w in range(N):
        full = w // wpw < N // wpw
        left = busy - (w % wpw) * (M // 2) if full else 1
        worlds.append(_walker_world(int(np.clip(left, 0, M // 2)), M, seed=100 * busy + w))
    return lw.as_pool(worlds, False)


def _busy_counts(pool, N, M, wpw, steps):
    """the oracle on the pool: per step, per workgroup, the egos whose start velocity (the preferred velocity cut to the preferred
    speed, fp32) violates one of their half-planes - the egos the kernel hands to an LP group"""
    env = orc.OracleEnv(N=N, M=M, max_obstacles=0, game_over_mode=1)
    env.set_scenario(**pool)
    env.reset()
    a6, pol, coop = pool["agents6"], pool["policy_id"], pool["coop"]
    out = np.zeros((steps, -(-N // wpw)), dtype=np.int64)
    for t in range(steps):
        pos, vel, hd, done = env.f("pos").copy(), env.f("vel").copy(), env.f("heading").copy(), env.u("is_done").copy()
        for w in range(N):
            for i in np.nonzero((pol[w] == scen.POLICY_RVO) & (done[w] == 0))[0]:
                r = orc.orca_action_ex(pos[w], vel[w], a6[w, :, 2:4], a6[w, :, 4], a6[w, :, 5], int(i), float(hd[w, i]),
                                       float(coop[w, i]), max_neighbors=M, rects=None)
                L = np.ascontiguousarray(r["lines"], dtype=f32).reshape(-1, 4)
                g = a6[w, i, 2:4] - pos[w, i]
                sc = a6[w, i, 4] / np.hypot(*g)
                ox, oy, rad = f32(sc * g[0]), f32(sc * g[1]), f32(a6[w, i, 4])
                if ox * ox + oy * oy > rad * rad:
                    inv = f32(1.0) / np.sqrt(ox * ox + oy * oy)
                    ox, oy = ox * inv * rad, oy * inv * rad
                out[t, w // wpw] += int((L[:, 2] * (L[:, 1] - oy) - L[:, 3] * (L[:, 0] - ox) > 0).any())
        env.step()
    return out


@pytest.mark.parametrize("busy", [1, 9, 17])
def test_partly_filled_lp_waves(busy, monkeypatch):
    N, M, wpw = 9, 10, 4
    pool = _busy_pool(busy, N, M, wpw)
    counts = _busy_counts(pool, N, M, wpw, T)
    print("busy egos per step and workgroup", counts.tolist())
    assert (counts[:, :N // wpw] == busy).all() and (counts[:, N // wpw:] == 1).all(), counts
    _forms_agree(pool, N, M, HEADLINE, monkeypatch)


@pytest.mark.parametrize("M,wp,N,kernel", [(4, 0, 17, "k_rollout3<256, 4, 0, true, false>"),
                                           (20, 2, 3, "k_rollout3<256, 20, 2, true, false>")])
def test_other_group_widths(M, wp, N, kernel, monkeypatch):
    pool, info = lw.build_pool(M, _n_worlds(M, wp), False)
    # M = 20: the ring (outer rounds of linearProgram3 on the lanes' second slot), the box and a lattice world
    names = lw.scene_names(M, False)
    idx = [names.index("ring"), names.index("box"), info["n_scenes"]] if M == 20 else N
    _forms_agree(_worlds(pool, idx), N, M, kernel, monkeypatch)
