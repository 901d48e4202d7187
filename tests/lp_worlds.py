"""Seeded worlds that reach the rare branches of the ORCA linear programs (tests/orca_lp_twin.py names them), for any M in 2..32.

Random start / goal pairs (scenarios.random_worlds_fast) never give exactly parallel half-planes, a half-plane that misses the
speed disc or tied neighbour distances.  These do:

lattice worlds   agents on a square lattice of pitch 1.125 m (exactly representable coordinates), cells drawn from a block of
                 ceil(sqrt(1.6 M)) + 1 cells per side, made even (no cell on an axis through the centre: an agent walking along
                 such an axis straight at a Static one is ORCA's unstable head-on, see noisy_twins_part()), radii <= 0.5 (no pair collides at reset, pairs of radius 0.5 overlap in the
                 inflated RVO radius: 1.15 > 1.125), goals through the centre, pref_speed from {0.125, 0.5, 1, 1.5} (the slow
                 ones give disc < 0), coop from {0.5, 1}, about 70 % RVO and the rest Static, agent 0 RVO.  Velocities are zero at
                 reset: exactly parallel and anti-parallel half-planes and exactly tied distances at step 0, and between Static
                 agents later.  An agent of pref_speed 0.125 gets coop 1: with coop 0.5 a touching pair of radius 0.5 puts its
                 half-plane at 0.5 (11.5 - 11.25) = 0.125 from the origin, tangent to its own speed disc - disc == 0 exactly.
                 With rectangles: in 40 % of the worlds a wall 0.53 m beside the upper half of the block's last column (inside the
                 inflated radius 0.575, outside the radius).
scenes           hand-made, in the first worlds of every pool and in its last world (the ragged last workgroup): SCENES below.

Tie rejection.  The device's and glibc's sincos / atan2 differ in the last ulp, which moves a half-plane's point by up to about
1e-6 after a few steps; a comparison of a linear program closer to its threshold than that may legitimately go the other way
on the device.  build_pool() therefore runs the oracle for the T steps of the test, classifies every RVO solve with the twin and
replaces a candidate world in which some solve's decision margin is below orca_lp_twin.TIE_MARGIN (1e-4, 100 times the 1e-6) by
the next candidate of the seeded stream; a rejected scene is perturbed by a lattice-exact amount (neighbour k moves outwards by
a * k / 512 m, beside a wall sideways by a / 8 m, a = 1, 2, ..) until it is accepted and still reaches its branches - never
dropped.  (The unperturbed wall and corner scenes put the neighbour's half-plane exactly parallel to the wall's: linearProgram3
then picks an end of the wall's line by the sign of an exact 0.)  "Margin" is the twin's: the smallest distance from its
threshold of a comparison that DECIDES something, see orca_lp_twin.py.  The twin sees the linear programs only; what is decided
before them (the construction of the half-planes) and behind them (the turn towards the new velocity) is put to a direct test:
a world also goes when the oracle, run again with noise of 2e-16 on the state of the agents that have moved, leaves its own
trajectory by more than the device tests allow - see noisy_twins_part(), and displacement() for the turn.  The share of rejected
candidates is reported and bounded (test_orca_lp_twin.py: at most 25 %), so that rejection cannot hide a failing kernel.
The GPU tests then assert every world of the pool."""
import functools
import importlib

import numpy as np

import orca_lp_twin as twin
from oracle import oracle as orc

scen = importlib.import_module("gym-exploration-2d_amd.scenarios")

PITCH = 1.125
T_STEPS = 12
SEED = 7200
MAX_REJECTED = 0.25
K_RECT = 2
# the state is fp64 and the libms differ in the last ulp (1.1e-16) of sincos / atan2: a step adds v dt cos(heading) to a position,
# 12 steps of v <= 1.5 and dt = 0.1 at most 12 * 0.15 * 1.1e-16 = 2e-16 m of difference, and as much on a velocity or a heading.
# ACTION_TOL and STATE_TOL are the tolerances of the device tests on an action and on the state
STATE_NOISE, N_NOISY, ACTION_TOL, STATE_TOL = 2e-16, 4, 2e-7, 1e-7
ANGLE_NOISE = 2e-15  # rad: a few ulps of an angle near pi (4.4e-16): atan2, and the 2 pi that wrap() adds or takes away
# an agent that turns on the spot by (float)(pi / 6) per step comes to within 3e-8 rad of pi / 6 - the rounding of the fp32 action,
# the same on both sides; what the libms add is ANGLE_NOISE
TURN_TIE = 1e-9
RESIDUE = 1e-12  # m: no step the linear programs ask for is that short
WALL = [0.53, -3.0, 1.5, 3.0]  # on the ego's right, inside its inflated radius 0.575 and outside its radius 0.5
FLOOR = [-3.0, -1.5, 0.4, -0.54]

# name: (positions ego first, radii, ego goal, ego pref_speed, ego coop, rectangles, counters the ego's solves must reach,
#        the perturbation step of a neighbour: None = outwards by k / 512 m, else that vector)
SCENES = {
    "squeeze": ([(0, 0), (1.1, 0), (-1.1, 0)], [0.5] * 3, (6, 0), 1.0, 0.5, [], ["lp3_solves", "lp3_parallel_opposite"], None),
    "file": ([(0, 0), (-1.1, 0), (1.5, 0), (3.0, 0)], [0.5, 0.5, 0.5, 2.0], (6, 0), 1.0, 0.5, [],
             ["lp3_parallel_same", "lp3_parallel_opposite", "lp1_parallel_outside"], None),
    # the fat neighbour 2^-20 m off the axis: its half-plane and the near one's have the same direction to 3e-7, not bit for
    # bit.  Kept by mistake, the projected line of such a pair is a real (wrong) constraint; of an identical pair it is all NaN
    # and constrains nothing - only this scene tells a linearProgram3 that forgets the same-direction hole from one that has it
    "file_skew": ([(0, 0), (-1.1, 0), (1.5, 0), (3.0, 2.0 ** -20)], [0.5, 0.5, 0.5, 2.0], (6, 0), 1.0, 0.5, [],
                  ["lp3_parallel_same", "lp3_parallel_opposite"], None),
    "row": ([(0, 0), (-1.4, 0), (1.5, 0)], [0.5] * 3, (6, 0), 1.0, 0.5, [], ["lp1_parallel_inside"], None),
    "box": ([(0, 0), (1.1, 0), (-1.1, 0), (0, 1.1), (0, -1.1)], [0.5] * 5, (6, 0), 1.0, 0.5, [], ["lp3_solves", "lp3_outer_2inner"], None),
    "wall": ([(0, 0), (-1.1, 0)], [0.5] * 2, (-6, 0), 0.25, 1.0, [WALL], ["lp3_with_obstacle_lines", "lp1_disc_negative_original"],
             (0, 0.125)),
    # found by a seeded search (test_orca_lp_twin.py (4)): the inner program of linearProgram3 FAILS by rounding and the result
    # is restored; no comparison of these solves is anywhere near its threshold
    "trap_a": ([(0, 0), (0.8701171875, 0.7314453125), (-0.71875, 0.8388671875), (0.6591796875, -0.7705078125)], [0.5] * 4,
               (-5.0, -3.25), 0.5, 1.0, [], ["lp3_inner_failed"], None),
    "trap_b": ([(0, 0), (1.0595703125, 0.3974609375), (-0.7724609375, 0.7841796875), (0.728515625, -0.7412109375)], [0.5] * 4,
               (3.75, -4.75), 0.5, 1.0, [], ["lp3_inner_failed"], None),
    "trap_c": ([(0, 0), (0.61328125, 0.849609375), (-0.6240234375, -0.87109375), (1.0107421875, -0.423828125)], [0.5] * 4,
               (-5.5, -2.25), 0.125, 1.0, [], ["lp3_inner_failed"], None),
    # 19 small neighbours all around, none touching the ego and every one inside its inflated band, the farther ones a little
    # larger so that they overlap a little MORE (1.15 dr > dd > dr): the penetration linearProgram3 minimises keeps growing -
    # outer rounds up to the last lines, on the second slot of an LP lane (i >= 17), whatever the lattice worlds happen to reach
    "ring": ([(0, 0)] + [(round(4096 * (0.56 + 0.00215 * k) * np.cos(2 * np.pi * k * 7 / 19)) / 4096,
                          round(4096 * (0.56 + 0.00215 * k) * np.sin(2 * np.pi * k * 7 / 19)) / 4096) for k in range(19)],
             [0.5] + [0.05 + 0.002 * k for k in range(19)], (6, 1), 1.0, 0.5, [], ["lp3_solves", "lp3_outer_2inner"], None),
    "corner": ([(0, 0), (-1.1, 0)], [0.5] * 2, (-6, 3), 0.25, 1.0, [WALL, FLOOR], ["lp3_with_obstacle_lines"], (0, 0.125)),
}


def scene_names(M, rects):
    """the scenes that fit M agent slots (box needs 5), in pool order"""
    names = [k for k in ("squeeze", "file", "file_skew", "row", "box", "trap_a", "trap_b", "trap_c", "ring") if len(SCENES[k][0]) <= M]
    return names + (["wall", "corner"] if rects else [])


def scene_world(name, M, a=0):
    """-> (agents6 [M, 6], policy [M], coop [M], obstacles [K_RECT, 4], n_obst); the ego is agent 0 (RVO), its neighbours
    Static, far-away Static agents up to M.  a: the perturbation step."""
    pos, rad, goal, pref, coop, rects, _, nudge = SCENES[name]
    pos = np.array(pos, dtype=np.float64)
    n = len(pos)
    for k in range(1, n):
        pos[k] += np.sign(pos[k] - pos[0]) * (a * k / 512.0) if nudge is None else a * np.array(nudge)
    a6 = np.zeros((M, 6))
    a6[:, 0] = -13.5 + 0.875 * np.arange(M)  # a row along the map's edge, 10 m and more from the scene
    a6[:, 1] = 13.5
    a6[:, 2:4] = a6[:, 0:2] - [0.0, 1.0]
    a6[:, 4], a6[:, 5] = 1.0, 0.25
    a6[:n, 0:2], a6[:n, 5] = pos, rad
    a6[:n, 2:4], a6[:n, 4] = goal, pref
    pol = np.full(M, scen.POLICY_STATIC, dtype=np.int32)
    pol[0] = scen.POLICY_RVO
    obst = np.zeros((K_RECT, 4))
    if rects:
        obst[:len(rects)] = rects
    return a6, pol, np.full(M, float(coop)), obst, len(rects)


def lattice_world(rng, M, rects):
    side = int(np.ceil(np.sqrt(1.6 * M))) + 1
    side += side % 2  # even: no cell on an axis through the centre, see the module docstring
    cells = rng.permutation(side * side)[:M]
    xy = (np.stack([cells % side, cells // side], 1).astype(np.float64) - (side - 1) / 2) * PITCH
    a6 = np.zeros((M, 6))
    a6[:, 0:2] = xy
    a6[:, 2:4] = -xy + np.where(np.abs(xy).sum(1, keepdims=True) == 0, 3.0, 0.0)
    a6[:, 4] = rng.choice([0.125, 0.5, 1.0, 1.5], M)
    a6[:, 5] = rng.choice([0.375, 0.4375, 0.5, 0.5], M)
    pol = np.where(rng.uniform(size=M) < 0.7, scen.POLICY_RVO, scen.POLICY_STATIC).astype(np.int32)
    pol[0] = scen.POLICY_RVO
    coop = rng.choice([0.5, 1.0], M)
    coop[a6[:, 4] == 0.125] = 1.0  # see the module docstring: 0.125 with coop 0.5 is tangent to its own disc
    obst, n_obst = np.zeros((K_RECT, 4)), 0
    if rects and rng.uniform() < 0.4:
        h = (side - 1) / 2 * PITCH
        obst[0] = h + 0.53, -0.25, h + 1.5, h + 1.0
        n_obst = 1
    return a6, pol, coop, obst, n_obst


def as_pool(worlds, rects):
    a6, pol, coop, obst, n_obst = (np.stack([w[k] for w in worlds]) for k in range(5))
    M = a6.shape[1]
    return dict(agents6=a6, policy_id=pol, dynamics_id=scen.DYN_UNICYCLE, n_agents=np.full(len(worlds), M, dtype=np.int32),
                coop=coop, obstacles=obst if rects else None, n_obst=n_obst.astype(np.int32) if rects else None)


def trace(pool, M, rects, T=T_STEPS, rvo_max_neighbors=0, oracle=orc):
    """The oracle on `pool` for T steps, every RVO solve re-solved by the twin.
    -> per world: [smallest decision margin, counters, solves, solves whose twin result differs from the oracle's new_vel,
    (step, ego, comparison) of the smallest margin]"""
    N = len(pool["agents6"])
    K = K_RECT if rects else 0
    env = oracle.OracleEnv(N=N, M=M, max_obstacles=K, game_over_mode=1, rvo_max_neighbors=rvo_max_neighbors)
    env.set_scenario(**pool)
    env.reset()
    a6, pol, coop = pool["agents6"], pool["policy_id"], pool["coop"]
    maxnb = rvo_max_neighbors if rvo_max_neighbors > 0 else M
    out = [[twin.INF, {}, 0, 0, None] for _ in range(N)]
    for t in range(T):
        pos, vel, hd, done = env.f("pos").copy(), env.f("vel").copy(), env.f("heading").copy(), env.u("is_done").copy()
        for w in range(N):
            rc = pool["obstacles"][w, :pool["n_obst"][w]] if rects else None
            for i in np.nonzero((pol[w] == scen.POLICY_RVO) & (done[w] == 0))[0]:
                r = oracle.orca_action_ex(pos[w], vel[w], a6[w, :, 2:4], a6[w, :, 4], a6[w, :, 5], int(i), float(hd[w, i]),
                                          float(coop[w, i]), max_neighbors=maxnb, rects=rc)
                g = a6[w, i, 2:4] - pos[w, i]
                pv = a6[w, i, 4] / np.hypot(*g) * g
                got, c, margin = twin.classify(r["lines"], r["n_obst_lines"], a6[w, i, 4], pv, pos=pos[w], ego=int(i),
                                               max_neighbors=maxnb)
                o = out[w]
                if margin < o[0]:
                    o[0], o[4] = margin, (t, int(i), c.what)
                step, turn = displacement(pos[w, i], float(hd[w, i]), got)
                if 0.0 < step < RESIDUE:
                    o[0], o[4] = 0.0, (t, int(i), "the new velocity moves the ego by %.1e m: the direction of a rounding residue" % step)
                if turn < TURN_TIE:
                    o[0], o[4] = 0.0, (t, int(i), "the turn is %.1e rad from pi / 6 or from the seam at pi" % turn)
                twin.merge(o[1], c)
                o[2] += 1
                o[3] += int(got.tobytes() != r["new_vel"].tobytes())
        env.step()
    for w, t in enumerate(noisy_twins_part(pool, M, rects, T, rvo_max_neighbors, oracle)):
        if t is not None and out[w][0] > 0.0:
            out[w][0], out[w][4] = 0.0, (t, -1, "state noise of %.0e parts the trajectories" % STATE_NOISE)
    return out


def displacement(pos, heading, new_vel, dt=0.1):
    """-> (|new position - position|, how far the turn towards it is from a decision), as RVOPolicy sees them: the fp32 position
    plus the fp32 step, minus the fp64 position.  The action's heading is the direction of that vector.  Where the step is too small to move an fp32 position (a new velocity of
    1e-18 m/s: two residues cancelling) the vector is the low bits of the fp64 position - 1e-19 m of cos(pi / 2) - and its
    direction anybody's guess; an exact 0 (atan2(0, 0) = 0 in any libm) is not.
    The turn, wrap(atan2(d) - heading) in fp64, is cut to +-pi / 6 at speed 0 beyond pi / 6, and an about-turn goes left or right
    at the seam of wrap(): the smaller distance of |turn| from pi / 6 and from pi.  An about-turn along a coordinate axis whose
    difference is +-pi bit for bit is exempt - atan2 of an axis is exact in any libm, so this pins how the device wraps AT the
    seam; one along a diagonal is not: atan2(-a, -a) is -3 pi / 4 to the last ulp, or not."""
    p32 = np.asarray(pos, dtype=np.float64).astype(np.float32)
    d = (p32 + np.asarray(new_vel, dtype=np.float32) * np.float32(dt)).astype(np.float64) - np.asarray(pos, dtype=np.float64)
    nh = float(np.arctan2(d[1], d[0]))
    raw = (nh + 2 * np.pi if nh < 0 else nh) - heading
    dh = abs((raw + np.pi) % (2 * np.pi) - np.pi)
    seam = np.pi - dh
    if (d[0] == 0.0 or d[1] == 0.0) and abs(raw) == np.pi:  # along an axis: atan2 is exact by definition (0, +-pi / 2, pi)
        seam = float("inf")
    return float(np.hypot(d[0], d[1])), min(abs(dh - np.pi / 6), seam)


def noisy_twins_part(pool, M, rects, T, rvo_max_neighbors, oracle):
    """Does noise of the size two libms differ by send a world somewhere else?  The oracle runs the pool N_NOISY more times; behind
    every step each coordinate of a position that has changed since reset, each non-zero velocity component and each heading that
    has turned is moved by STATE_NOISE (ANGLE_NOISE) - all up, all down, then at random: the fragile thing is nearly always the
    SIGN of one residue.  What never changed is exact on both sides and stays.  That leaves nearly every fp32 operand as it
    was, but not an x = 6e-18 m that cos(pi / 2) v dt left where another libm leaves 0.  Such a residue decides things the twin
    does not see - the leg of a velocity obstacle between two agents exactly head-on on a lattice axis (det(rp, w) > 0 in the
    half-plane's construction: the side the ego passes on) - and it GROWS where ORCA is unstable: an agent walking straight at a
    Static one on a lattice axis multiplies its sideways velocity by 8.7 per step, 1.6e-19 m/s after the first step, 2.4e-8
    after the twelfth, 5e-7 rad of heading.
    -> per world: None, or the first step at which a noisy run leaves the plain one by more than the device tests allow."""
    N = len(pool["agents6"])
    K = K_RECT if rects else 0
    rng = np.random.default_rng(20)
    envs = []
    for _ in range(N_NOISY + 1):
        e = oracle.OracleEnv(N=N, M=M, max_obstacles=K, game_over_mode=1, rvo_max_neighbors=rvo_max_neighbors)
        e.set_scenario(**pool)
        e.reset()
        envs.append(e)
    plain, p0, h0 = envs[0], envs[0].f("pos").copy(), envs[0].f("heading").copy()
    parted = [None] * N
    for t in range(T):
        for e in envs:
            e.step()
        for k, e in enumerate(envs[1:]):
            bad = np.abs(e.f("action") - plain.f("action")).max(axis=(1, 2)) > ACTION_TOL
            for key in ("pos", "vel"):
                bad |= np.abs(e.f(key) - plain.f(key)).max(axis=(1, 2)) > STATE_TOL
            bad |= np.abs((e.f("heading") - plain.f("heading") + np.pi) % (2 * np.pi) - np.pi).max(axis=1) > STATE_TOL
            bad |= (e.u("is_done") != plain.u("is_done")).any(axis=1)
            for w in np.nonzero(bad)[0]:
                if parted[w] is None:
                    parted[w] = t
            sign = (lambda shape: np.full(shape, 1.0 - 2.0 * k)) if k < 2 else (lambda shape: rng.choice([-1.0, 1.0], shape))
            pos, vel, hd = e.f("pos"), e.f("vel"), e.f("heading")  # views of the oracle's own state
            pos += (pos != p0) * sign(pos.shape) * STATE_NOISE
            vel += (vel != 0) * sign(vel.shape) * STATE_NOISE
            hd += (hd != h0) * sign(hd.shape) * ANGLE_NOISE
    return parted


def _total(traces):
    tot = {}
    for _, c, _, _, _ in traces:
        twin.merge(tot, c)
    return tot


def _accepted_scene(name, M, rects, rvo_max_neighbors, T, info):
    want = SCENES[name][6]
    for a in range(16):
        w = scene_world(name, M, a)
        tr = trace(as_pool([w], rects), M, rects, T, rvo_max_neighbors)[0]
        info["candidates"] += 1
        reaches = rvo_max_neighbors > 0 or all(tr[1].get(k, 0) > 0 for k in want)
        if tr[0] >= twin.TIE_MARGIN and reaches:
            info["scene_steps"][name] = a
            return w, tr
        info["rejected"] += 1
    raise AssertionError("no accepted perturbation of the scene %r for M = %d" % (name, M))


@functools.lru_cache(maxsize=None)
def build_pool(M, N, rects=False, rvo_max_neighbors=0, T=T_STEPS, scenes=True):
    """-> (pool for set_scenario, info): the scenes of scene_names() in worlds 0.., accepted lattice worlds, and in the last world
    (the ragged last workgroup of the kernel tests) one more scene.  info: candidates, rejected, rate, scene_steps (the
    perturbation step each scene needed), counters (summed over the pool's solves), solves, mismatches, traces (per world).
    Cached: the CPU and the GPU tests share the pools and leave them unchanged."""
    info = dict(candidates=0, rejected=0, scene_steps={}, rejected_why=[])
    names = scene_names(M, rects) if scenes else []
    head = [_accepted_scene(k, M, rects, rvo_max_neighbors, T, info) for k in names]
    tail = [head[(M + int(rects)) % len(head)]] if head else []
    rng = np.random.default_rng(SEED + 16 * M + 7 * rvo_max_neighbors + int(rects))
    want, lat = N - len(head) - len(tail), []
    while len(lat) < want:
        batch = [lattice_world(rng, M, rects) for _ in range(max(4, (want - len(lat)) * 5 // 4))]
        for w, tr in zip(batch, trace(as_pool(batch, rects), M, rects, T, rvo_max_neighbors)):
            if len(lat) == want:
                break
            info["candidates"] += 1
            if tr[0] >= twin.TIE_MARGIN:
                lat.append((w, tr))
            else:
                info["rejected"] += 1
                info["rejected_why"].append(tr[4])
        assert info["candidates"] < 20 * N, "the tie rejection starves the pool"
    worlds = head + lat + tail
    info["traces"] = [tr for _, tr in worlds]
    info["counters"] = _total(info["traces"])
    info["solves"] = sum(tr[2] for tr in info["traces"])
    info["mismatches"] = sum(tr[3] for tr in info["traces"])
    info["rate"] = info["rejected"] / info["candidates"]
    info["n_scenes"] = len(head)
    return as_pool([w for w, _ in worlds], rects), info
