#!/usr/bin/env python3
"""Fixture of the reference's greedy information-gain policy (development container only; needs the reference checkout).

Run:  python tests/golden/make_golden_ig_greedy.py        (about a minute)
Output: tests/golden/ig_greedy.npz -- data only.  policies/ig_greedy.py is executed unmodified through ref_harness.py on the two
obstacle sets of make_golden.ig_primitives ("corridor", "rects"), parameters of its init_maps call in experiments (60 deg, 5 m,
dt 0.1, ego radius 0.5).  Per world <w>:
  <w>__obstacles [4,4]          xl, yl, xu, yu
  <w>__upd_poses [8,24,3], <w>__upd_dets [8,24,1,2], <w>__upd_ndet [8,24]   the inputs of eight targetMap.update(poses, dets)
                                calls (the list API) that make the belief non-uniform: 24 free-space poses, heading += 0.8 per
                                round, one detection 2 m ahead of every third pose
  <w>__belief [60,60]           targetMap.map after them
  <w>__poses [Q,3]              query poses (EDF > 0.05; the last four sit 0.3 m inside a map edge, heading outwards)
  per query pose and candidate c = 3 a + b = (v[a], w[b]) of greedy_action's action_list:
  <w>__outside [Q,9] bool       the next pose's raster cell lies outside [0, 300)^2 (get_next_pose raises IndexError beyond 299
                                and wraps a negative index; both are recorded here and nowhere else)
  <w>__feasible [Q,9] bool      get_next_pose returned a pose, and not outside
  <w>__next [Q,9,3]             that pose (NaN where not feasible)
  <w>__mi [Q,9]                 targetMap.get_reward_from_pose(next) (NaN where not feasible)
  <w>__action [Q,2]             greedy_action(pose): the chosen (v, w); (-1, -1) for its scalar -1 (nothing feasible); NaN when it
                                raised IndexError
The generator asserts what tests/test_ig_greedy_twin.py re-asserts from the file: near ties (relative top-2 gap <= 1e-9) on at
most 10 % of the poses with a feasible candidate, >= 1 pose without a feasible candidate, >= 1 with 3 or 6, >= 1 outside candidate.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

OUT = os.environ.get("CAGYM_GOLDEN_OUT") or HERE
WORLDS = {
    "corridor": [(2, 2, 10, 10), (-10, 2, -2, 10), (2, -10, 10, -2), (-10, -10, -2, -2)],
    "rects": [(-6.3, 1.2, -3.1, 4.4), (1.7, -8.2, 4.9, -5.5), (5.2, 3.3, 6.1, 9.7), (-1.4, -2.6, 0.8, -1.9)],
}
NEAR_TIE = 1e-9
N_UPD, N_ROUNDS, N_QUERY = 24, 8, 60


def near_tie(mi_row, feasible_row):
    """relative gap of the two largest feasible rewards <= NEAR_TIE (False with fewer than two)"""
    m = np.sort(mi_row[feasible_row])[::-1]
    return len(m) >= 2 and (m[0] - m[1]) <= NEAR_TIE * max(abs(m[0]), 1e-300)


def check(arrays):
    """the conditions the fixture has to meet, per world; returns the counts"""
    counts = {}
    for w in WORLDS:
        feas, mi, outside = arrays[w + "__feasible"], arrays[w + "__mi"], arrays[w + "__outside"]
        nf = feas.sum(axis=1)
        some = nf > 0
        ties = sum(bool(near_tie(mi[q], feas[q])) for q in range(len(feas)) if some[q])
        assert ties <= 0.10 * some.sum(), (w, ties, int(some.sum()))
        assert (nf == 0).sum() >= 1, w
        assert ((nf == 3) | (nf == 6)).sum() >= 1, w
        assert outside.sum() >= 1 and not (outside & feas).any(), w
        counts[w] = dict(poses=len(feas), with_feasible=int(some.sum()), near_ties=int(ties), none_feasible=int((nf == 0).sum()),
                         partial=int(((nf == 3) | (nf == 6)).sum()), outside=int(outside.sum()))
    return counts


def main():
    rh.install_standins()
    with rh.quiet():
        from gym_collision_avoidance.envs.Map import Map
        from gym_collision_avoidance.envs.policies.ig_greedy import ig_greedy

    class Ego(object):
        radius = 0.5

    rng = np.random.default_rng(20260)
    arrays = {}
    for w, obst in WORLDS.items():
        with rh.quiet():
            m = Map(30, 30, 0.1, [[(xu, yu), (xl, yu), (xl, yl), (xu, yl)] for (xl, yl, xu, yu) in obst])  # test_cases.py:2496
            pol = ig_greedy()
            pol.init_maps(Ego(), m, (30, 30), 0.1, 60.0, 5.0)
        tm, edf = pol.targetMap, pol.edfMap
        arrays[w + "__obstacles"] = np.asarray(obst, dtype=np.float64)

        def free_pose(min_edf):
            while True:
                p = np.append(rng.uniform(-13.5, 13.5, 2), rng.uniform(-np.pi, np.pi))
                if edf.get_edf_value_from_pose(p) > min_edf:
                    return p

        # a dense belief update through the list API
        cur = np.array([free_pose(0.3) for _ in range(N_UPD)])
        up, ud, un = [], [], []
        for _ in range(N_ROUNDS):
            dets, dd, nd = [], np.zeros((N_UPD, 1, 2)), np.zeros(N_UPD, dtype=np.int32)
            for k, p in enumerate(cur):
                d = [p[0:2] + 2.0 * np.array([np.cos(p[2]), np.sin(p[2])])] if k % 3 == 0 else []
                dets.append(d)
                nd[k] = len(d)
                if d:
                    dd[k, 0] = d[0]
            tm.update([p.copy() for p in cur], [list(d) for d in dets], frame='global')
            up.append(cur.copy())
            ud.append(dd)
            un.append(nd)
            cur = cur + np.array([0.0, 0.0, 0.8])
        arrays[w + "__upd_poses"], arrays[w + "__upd_dets"], arrays[w + "__upd_ndet"] = np.array(up), np.array(ud), np.array(un)
        arrays[w + "__belief"] = tm.map.copy()

        # query poses; the last four look out of the map from 0.3 m inside an edge (v = 4 leaves it)
        poses = [free_pose(0.05) for _ in range(N_QUERY - 4)]
        t = rng.uniform(-1.0, 1.0, 4)
        poses += [np.array([14.7, t[0], 0.0]), np.array([-14.7, t[1], np.pi]), np.array([t[2], 14.7, 0.5 * np.pi]),
                  np.array([t[3], -14.7, -0.5 * np.pi])]
        poses = np.array(poses)
        acts = [np.array([v, dphi]) for v in [0.0, 2.0, 4.0] for dphi in [-np.pi, 0, np.pi]]  # ig_greedy.py:65-68
        Q = len(poses)
        outside = np.zeros((Q, 9), dtype=bool)
        feas = np.zeros((Q, 9), dtype=bool)
        nxt = np.full((Q, 9, 3), np.nan)
        mi = np.full((Q, 9), np.nan)
        action = np.full((Q, 2), np.nan)
        for q, p in enumerate(poses):
            for c, a in enumerate(acts):
                try:
                    r = pol.get_next_pose(p.copy(), a)
                    raised = False
                except IndexError:
                    r, raised = None, True
                # the cell of the next pose, from the pose get_next_pose would return (its own expressions, ig_greedy.py:84-89)
                cs, sn = np.cos(p[2]), np.sin(p[2])
                cand = p + np.append(np.dot(np.array(((cs, -sn), (sn, cs))), np.array([a[0], 0.0])), a[1]) * 0.1
                idx = [np.floor((cand[k] + 30 / 2) / 0.1) for k in (0, 1)]
                outside[q, c] = any(i < 0 or i >= 300 for i in idx)
                assert not raised or outside[q, c]
                if r is not None and not outside[q, c]:
                    assert np.array_equal(r, cand)
                    feas[q, c] = True
                    nxt[q, c] = r
                    mi[q, c] = tm.get_reward_from_pose(r)
            try:
                best = pol.greedy_action(p.copy())
                action[q] = best if np.ndim(best) else (-1.0, -1.0)
            except IndexError:
                pass
        arrays[w + "__poses"], arrays[w + "__outside"], arrays[w + "__feasible"] = poses, outside, feas
        arrays[w + "__next"], arrays[w + "__mi"], arrays[w + "__action"] = nxt, mi, action
    for w, c in check(arrays).items():
        print(w, c)
    path = os.path.join(OUT, "ig_greedy.npz")
    np.savez_compressed(path, **arrays)
    print("%-28s          %8.1f KB" % ("ig_greedy", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
