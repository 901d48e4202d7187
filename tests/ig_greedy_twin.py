"""CPU twin of cagym_ig_greedy_plan (csrc/cagym_ig_greedy.h) for one world: the specification of both modes, composed from the
C oracle's information-gain entries (oracle.visible_cells / oracle.mi_reward) and the next-pose arithmetic of
policies/ig_greedy.py:80-94 in numpy.  Rewards are the oracle's sequential sums: they agree with the device's block reduction to
rounding, not bit for bit (tests/test_ig_greedy.py composes the bit-exact counterpart from the device's own entries).
Used by tests/test_ig_greedy_twin.py and tests/test_ig_greedy.py."""
import numpy as np

from oracle import oracle as orc

GREEDY_V, GREEDY_W = (0.0, 2.0, 4.0), (-np.pi, 0.0, np.pi)  # ig_greedy.py:65-66: candidate c = 3 a + b is (v[a], w[b])
NONE = 255  # choice of a robot without a feasible candidate (deviation D6)


def candidates(v=GREEDY_V, w=GREEDY_W):
    return np.array([[a, b] for a in v for b in w], dtype=np.float64)


def next_poses(pose, v=GREEDY_V, w=GREEDY_W, dt=0.1):
    """[9,3]: pose + (v cos(heading), v sin(heading), w) dt per candidate, the products of np.dot(R, [v, 0])"""
    pose = np.asarray(pose, dtype=np.float64)
    c, s = np.cos(pose[2]), np.sin(pose[2])
    out = np.zeros((9, 3))
    for k, (vv, ww) in enumerate(candidates(v, w)):
        vx, vy = c * vv + (-s) * 0.0, s * vv + c * 0.0
        out[k] = pose + np.array([vx, vy, ww]) * dt
    return out


def cell_outside(nxt):
    """[..] bool: the raster cell floor((x + 15) / 0.1), floor((y + 15) / 0.1) is outside [0, 300)^2 (deviation D5)"""
    idx = np.floor((np.asarray(nxt)[..., 0:2] + 15.0) / 0.1)
    return ~(np.isfinite(idx).all(axis=-1) & (idx >= 0).all(axis=-1) & (idx < 300).all(axis=-1))


def feasibility(edf, nxt, radius=0.5):
    """([9] feasible, [9] outside): inside the raster and EDF(next) > radius + 0.1, tested for v = 0 as well"""
    outside = cell_outside(nxt)
    feas = np.zeros(len(nxt), dtype=bool)
    for k in np.nonzero(~outside)[0]:
        xi, yi = int(np.floor((nxt[k, 0] + 15.0) / 0.1)), int(np.floor((nxt[k, 1] + 15.0) / 0.1))
        feas[k] = edf[yi, xi] > radius + 0.1
    return feas, outside


def choose(mi):
    """the first candidate with strictly the largest reward, the running maximum starting at -1 (infeasible ones hold -1)"""
    best, best_mi = NONE, -1.0
    for c, m in enumerate(mi):
        if m > best_mi:
            best, best_mi = c, m
    return best


def greedy_plan(belief, edf, poses, coordinate=False, radius=0.5, dt=0.1, fov=orc.FOV60, rng=5.0, v=GREEDY_V, w=GREEDY_W,
                reward=None, visible=None):
    """The robots of one world, poses [R,3].  Returns dict(actions [R,2], choice [R] u8, mi [R,9], claimed [60] u64, feasible [R,9],
    outside [R,9], masks [R,9,60] u64: each candidate's visible cells less the claimed ones, zero where infeasible).
    reward(mask) / visible(pose): replacements of the oracle's entries (the GPU test passes the device's)."""
    reward = reward or (lambda mask: orc.mi_reward(belief, mask))
    visible = visible or (lambda pose: orc.visible_cells(edf, pose, fov, rng))
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    R = len(poses)
    cand = candidates(v, w)
    out = dict(actions=np.zeros((R, 2)), choice=np.full(R, NONE, dtype=np.uint8), mi=np.full((R, 9), -1.0),
               claimed=np.zeros(60, dtype=np.uint64), feasible=np.zeros((R, 9), dtype=bool), outside=np.zeros((R, 9), dtype=bool),
               masks=np.zeros((R, 9, 60), dtype=np.uint64))
    claimed = np.zeros(60, dtype=np.uint64)
    for r in range(R):
        nxt = next_poses(poses[r], v, w, dt)
        feas, outside = feasibility(edf, nxt, radius)
        out["feasible"][r], out["outside"][r] = feas, outside
        for c in np.nonzero(feas)[0]:
            out["masks"][r, c] = visible(nxt[c]) & ~claimed
            out["mi"][r, c] = reward(out["masks"][r, c])
        b = choose(out["mi"][r])
        out["choice"][r] = b
        if b != NONE:
            out["actions"][r] = cand[b]
            if coordinate:
                claimed = claimed | out["masks"][r, b]
    out["claimed"] = claimed
    return out
