#!/usr/bin/env python3
"""Fixture of the information-gain primitives at their edges (development container only; needs the reference checkout).

Run:  python tests/golden/make_golden_ig_edges.py        (a few seconds)
Output: tests/golden/ig_edges.npz -- data only.  The reference's own Map / edfMap / targetMap / ig_mcts objects, set up as in
make_golden.ig_primitives (60 deg, 5 m, dt 0.1, xdt 5, ego radius 0.5), on the "rects" world and on "corner", one rectangle that
touches the map corner.  tests/golden/ig_primitives.npz holds the same calls at 40 poses per world of which 37 are random, away
from the border, off every grid line and with |heading| < 2.8; this file holds the poses that one does not.  Per world <w>:
  <w>__obstacles [K,4]          xl, yl, xu, yu
  <w>__raster [300,38] u8       Map.static_map, np.packbits along the columns
  <w>__edf_d2_rows [20,300] u32 every 15th row of edfMap.map as squared cell distances d2: sqrt(d2) * 0.1 == edfMap.map bit for bit
                                (asserted here for the whole field)
  <w>__edf_d2_rowsum, <w>__edf_d2_colsum [300] u64   the sums of d2 over every row and every column
  <w>__vis_poses [Q,3]          x, y, heading: belief-cell centres (x = -14.75 + 0.5 k, same in y) at the twelve headings k * 30 deg
                                and in the four corner cells, belief-cell corners, poses on 0.1 m raster lines (written k * 0.1 - 15 and
                                (k - 150) / 10), poses within 0.3 m of each border and of each map corner looking out and in, and
                                headings +-100, +-12345.678 and 99999.9
  <w>__vis_masks [Q,60] u64     targetMap.getVisibleCells: bit i of word j <=> cell (i, j)
  <w>__np_feasible [Q,9] bool   ig_mcts.get_next_pose(pose, primitive) returned a pose; primitive 3 a + b = ({0, 2, 4}[a], {-pi/2, 0, pi/2}[b])
  <w>__np_next [Q,9,3]          that pose (NaN where it returned None)
  <w>__cv_a, <w>__cv_b [P,2]    point pairs of edfMap.checkVisibility(a, b): a lies on a 0.1 m raster line, or outside the map by less
                                than 30 m on the low side of an axis, where the reference's negative raster indices wrap (numpy); pairs on
                                which the reference raises (a beyond the high side, or 30 m and more outside) are dropped
  <w>__cv_visible [P] bool
The generator asserts what tests/test_oracle_ig_edges.py re-asserts from the file: the own cell of a centre pose is set at some
headings and not at others, both outcomes of checkVisibility occur among the pairs that start outside the map, and every primitive
is feasible somewhere and infeasible somewhere.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

OUT = os.environ.get("CAGYM_GOLDEN_OUT") or HERE
WORLDS = {
    "rects": [(-6.3, 1.2, -3.1, 4.4), (1.7, -8.2, 4.9, -5.5), (5.2, 3.3, 6.1, 9.7), (-1.4, -2.6, 0.8, -1.9)],
    # raster rows 0..30 (Map flips y; the distance field reads the rows unflipped, SURVEY Q12: to the planner this is y <= -11.9),
    # columns 260..299: the corner cell included.  (A rectangle on the low-y or the high-x border raises in Map.get_occupancy_grid.)
    "corner": [(11.0, 12.0, 14.95, 15.0)],
}
CENTRE = (9.25, -0.25)  # belief cell (48, 29); free in both worlds
N_CENTRE = 12
EDF_ROW_STEP = 15


def line(k, form):
    """the raster line -15 + 0.1 k, written the two ways callers write it"""
    return k * 0.1 - 15 if form == 0 else (k - 150) / 10


def vis_poses():
    d = np.deg2rad
    p = [(CENTRE[0], CENTRE[1], d(30.0 * k)) for k in range(N_CENTRE)]                                 # cell centres, k * 30 deg
    p += [(-14.75, -14.75, d(45.0)), (14.75, 14.75, d(225.0)), (14.75, -14.75, d(100.0)), (-14.75, 14.75, d(-10.0)),
          (0.25, 0.25, d(10.0)), (-9.75, 6.25, d(75.0))]                                                 # centres, corner cells
    p += [(9.0, -0.5, h) for h in (0.0, d(45.0), d(90.0), d(180.0), d(270.0), d(200.0))]                 # cell corners
    p += [(-5.0, 3.0, d(30.0)), (0.0, 0.0, d(120.0)), (12.5, 12.5, d(-135.0))]
    p += [(line(183, 0), -7.13, 0.3), (line(183, 1), -7.13, 0.3), (2.71, line(41, 0), d(60.0)), (2.71, line(41, 1), d(60.0)),
          (line(7, 0), line(292, 1), d(-30.0)), (line(250, 1), line(150, 0), d(150.0)), (line(99, 0), line(99, 0), d(240.0)),
          (line(201, 1), 4.44, -2.2)]                                                                    # 0.1 m lines
    p += [(14.8, 2.13, 0.0), (14.8, 2.13, np.pi), (14.95, -3.3, 1.0), (-14.8, 5.5, np.pi), (-14.8, 5.5, 0.0), (-14.9, -8.4, 2.0),
          (1.3, 14.85, 0.5 * np.pi), (1.3, 14.85, -0.5 * np.pi), (-6.6, -14.77, -0.5 * np.pi), (-6.6, -14.77, 0.5 * np.pi),
          (14.8, 14.8, d(45.0)), (14.8, 14.8, d(-135.0)), (-14.9, -14.9, -2.3), (-14.9, -14.9, 0.8), (14.9, -14.8, -0.8),
          (10.5, -11.8, -0.8), (-14.8, 14.9, 2.4), (-14.8, 14.9, -0.7)]                                  # borders and corners
    for x, y in ((CENTRE[0], CENTRE[1]), (-8.31, -3.77)):
        p += [(x, y, h) for h in (100.0, -100.0, 12345.678, -12345.678, 99999.9)]                        # large headings
    return np.array(p, dtype=np.float64)


def cv_pairs(rng):
    a = []
    for k in range(40):  # on a raster line in x, in y or in both; the three writings
        kk = int(rng.integers(5, 295))
        v = line(kk, k % 2)
        o = rng.uniform(-14, 14)
        a.append((v, o) if k % 3 == 0 else (o, v) if k % 3 == 1 else (v, line(int(rng.integers(5, 295)), (k + 1) % 2)))
    for k in range(60):  # outside on the low side of x, of y or of both, by less than 30 m
        out = -15.0 - rng.uniform(0.0, 30.0, 2)
        ins = rng.uniform(-14, 14, 2)
        a.append((out[0], ins[1]) if k % 3 == 0 else (ins[0], out[1]) if k % 3 == 1 else (out[0], out[1]))
    a += [(-15.0, 3.0), (2.0, -15.0), (-45.0 + 1e-9, 0.0), (-25.0, -44.0)]
    a += [(-17.0, -13.5), (-15.7, -14.2), (-18.3, -12.4)]  # wrap into the rectangle of "corner"
    a += [(15.0 + 1e-9, 0.0), (0.0, 16.0), (-45.5, 0.0), (0.0, -50.0), (15.0, 15.0), (40.0, -20.0)]  # the reference raises on these
    a = np.array(a, dtype=np.float64)
    b = rng.uniform(-14, 14, a.shape)
    b[0:40:5] = rng.uniform((11.5, -14.5), (14.5, -12.5), (8, 2))  # goals inside the rectangle of "corner"
    return a, b


def pin_arctan2():
    """targetMap.py:77-79 compares np.arctan2 with sensFOV / 2, and for a pose on a cell centre at a heading of k * 30 deg cells lie
    on the cone's edge to the last bit.  numpy's AVX-512 arctan2 is not correctly rounded (it differs from the C library's on 8 %
    of random arguments, by one ulp), so what the reference returns for those cells depends on the CPU it runs on.  Where
    np.arctan2 is not the C library's atan2 (which the oracle calls), the generator runs again in a child process with numpy's
    AVX-512 kernels disabled; np.arctan2 is the C library's then, on every CPU."""
    import math
    import subprocess
    x = np.random.default_rng(1).uniform(-5, 5, (4000, 2))
    if all(float(np.arctan2(a, b)) == math.atan2(a, b) for a, b in x):
        return
    assert not os.environ.get("CAGYM_GOLDEN_PINNED"), "np.arctan2 differs from the C library's atan2 without numpy's AVX-512 kernels"
    um = getattr(np, "_core", None) or np.core
    um = um._multiarray_umath
    off = [f for f in um.__cpu_dispatch__ if f.startswith("AVX512") and um.__cpu_features__.get(f)]
    env = dict(os.environ, NPY_DISABLE_CPU_FEATURES=" ".join(off), CAGYM_GOLDEN_PINNED="1")
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))


def main():
    pin_arctan2()
    rh.install_standins()
    with rh.quiet():
        from gym_collision_avoidance.envs.Map import Map
        from gym_collision_avoidance.envs.policies.ig_mcts import ig_mcts

    class Ego(object):
        radius = 0.5

    poses = vis_poses()
    acts = [np.array([v, w]) for v in (0.0, 2.0, 4.0) for w in (-0.5 * np.pi, 0, 0.5 * np.pi)]  # ig_mcts.py:247-253
    arrays = {}
    for w, obst in WORLDS.items():
        with rh.quiet():
            m = Map(30, 30, 0.1, [[(xu, yu), (xl, yu), (xl, yl), (xu, yl)] for (xl, yl, xu, yu) in obst])  # test_cases.py:2496
            pol = ig_mcts()
            pol.set_param(ego_agent=Ego(), occ_map=m, map_size=(30, 30), detect_fov=60.0, map_res=0.1, detect_range=5.0, Ntree=5,
                          Nsims=3, parallelize_sims=False, mcts_cp=1., mcts_horizon=4, parallelize_agents=False, dt=0.1, xdt=5,
                          mcts_gamma=0.95, Ncycles=2)
        tm, edf = pol.targetMap, pol.edfMap
        arrays[w + "__obstacles"] = np.asarray(obst, dtype=np.float64)
        d2 = np.rint((np.asarray(edf.map, dtype=np.float64) / 0.1) ** 2).astype(np.uint32)
        assert np.array_equal(np.sqrt(d2.astype(np.float64)) * 0.1, edf.map), w
        arrays[w + "__raster"] = np.packbits(np.asarray(m.static_map, dtype=bool), axis=1)
        arrays[w + "__edf_d2_rows"] = d2[::EDF_ROW_STEP]
        arrays[w + "__edf_d2_rowsum"], arrays[w + "__edf_d2_colsum"] = d2.sum(axis=1, dtype=np.uint64), d2.sum(axis=0, dtype=np.uint64)

        masks = np.zeros((len(poses), 60), dtype=np.uint64)
        with np.errstate(divide="ignore"):  # the own cell of a centre pose: checkVisibility divides by a zero distance
            for q, p in enumerate(poses):
                for (i, j) in tm.getVisibleCells(p.copy()):
                    assert 0 <= i < 60 and 0 <= j < 60
                    masks[q, j] |= np.uint64(1) << np.uint64(i)
        arrays[w + "__vis_poses"], arrays[w + "__vis_masks"] = poses, masks
        own = [(int(masks[q, 29]) >> 48) & 1 for q in range(N_CENTRE)]
        assert 0 < sum(own) < N_CENTRE, (w, own)

        nxt = np.full((len(poses), 9, 3), np.nan)
        feas = np.zeros((len(poses), 9), dtype=bool)
        for q, p in enumerate(poses):
            for k, a in enumerate(acts):
                r = pol.get_next_pose(p.copy(), a)
                if r is not None:
                    nxt[q, k] = r
                    feas[q, k] = True
        assert feas.any(axis=0).all() and (~feas)[:, 3:].any(axis=0).all(), w
        arrays[w + "__np_next"], arrays[w + "__np_feasible"] = nxt, feas

        a, b = cv_pairs(np.random.default_rng(777))
        keep, vis = [], []
        for x, y in zip(a, b):
            try:
                vis.append(bool(edf.checkVisibility(x, y)))
                keep.append(True)
            except IndexError:
                keep.append(False)
        keep, vis = np.array(keep), np.array(vis)
        a, b = a[keep], b[keep]
        outside = (a < -15.0).any(axis=1)
        assert (~keep).sum() >= 4 and outside.sum() >= 40, (w, int((~keep).sum()), int(outside.sum()))
        assert vis[outside].any() and (~vis[outside]).any() and vis[~outside].any() and (~vis[~outside]).any(), w
        arrays[w + "__cv_a"], arrays[w + "__cv_b"], arrays[w + "__cv_visible"] = a, b, vis
        print(w, dict(poses=len(poses), own_cell_set=own, visible_cells=int(sum(bin(int(x)).count("1") for x in masks.ravel())),
                      feasible=int(feas.sum()), pairs=len(a), pairs_outside=int(outside.sum()), pairs_visible=int(vis.sum()),
                      dropped=int((~keep).sum())))
    path = os.path.join(OUT, "ig_edges.npz")
    np.savez_compressed(path, **arrays)
    print("%-28s          %8.1f KB" % ("ig_edges", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
