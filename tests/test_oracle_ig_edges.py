"""Pin the oracle's information-gain primitives at their edges against vectors produced by the reference's own Map / edfMap /
targetMap / ig_mcts objects (tests/golden/ig_edges.npz, written by tests/golden/make_golden_ig_edges.py): belief-cell centres
and corners, poses on 0.1 m raster lines, next to the map border, with large headings, and sphere traces that start on a raster
line or outside the map, where the reference's negative indices wrap.  The bounds are those of tests/test_oracle_ig.py."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = os.path.join(GOLD_DIR, "ig_edges.npz")
WORLDS = ["rects", "corner"]
N_CENTRE, OWN_I, OWN_J = 12, 48, 29  # the first twelve poses: (9.25, -0.25) = centre of cell (48, 29), heading k * 30 deg


@pytest.fixture(scope="module")
def z():
    orc.build()
    return np.load(GOLD)


@pytest.fixture(scope="module")
def edf(z):
    out = {}
    for w in WORLDS:
        e, d2 = orc.edt(orc.rasterize(z[w + "__obstacles"]))
        out[w] = (np.ascontiguousarray(e), d2)
    return out


@pytest.mark.parametrize("w", WORLDS)
def test_edt_exact(z, edf, w):
    e, d2 = edf[w]
    assert np.array_equal(np.packbits(orc.rasterize(z[w + "__obstacles"]).astype(bool), axis=1), z[w + "__raster"])
    rows = z[w + "__edf_d2_rows"]
    step = 300 // len(rows)
    assert np.array_equal(d2[::step], rows)
    assert np.array_equal(e[::step], np.sqrt(rows.astype(np.float64)) * 0.1)  # == edfMap.map there, asserted by the generator
    assert np.array_equal(d2.sum(axis=1, dtype=np.uint64), z[w + "__edf_d2_rowsum"])
    assert np.array_equal(d2.sum(axis=0, dtype=np.uint64), z[w + "__edf_d2_colsum"])
    if w == "corner":
        assert d2[0, 299] == 0 and d2[30, 260] == 0 and d2[31, 260] == 1 and d2[0, 259] == 1


@pytest.mark.parametrize("w", WORLDS)
def test_visible_cells_bit_exact(z, edf, w):
    e = edf[w][0]
    for p, m in zip(z[w + "__vis_poses"], z[w + "__vis_masks"]):
        assert np.array_equal(orc.visible_cells(e, p), m), p
    assert not (z[w + "__vis_masks"] >> np.uint64(60)).any()


@pytest.mark.parametrize("w", WORLDS)
def test_own_cell_of_a_centre_pose(z, edf, w):
    """A robot on a belief-cell centre sees its own cell when atan2 of the two zeros of its ego-frame offset is +-0 and the
    cell is not in the window's excluded last row / column (targetMap.py:73-79): set at some of the twelve headings, not at
    others; the signs of the zeros and the window decide, nothing else."""
    poses, masks = z[w + "__vis_poses"][:N_CENTRE], z[w + "__vis_masks"][:N_CENTRE]
    assert np.allclose(poses[:, :2], (OWN_I * 0.5 - 14.75, OWN_J * 0.5 - 14.75), rtol=0, atol=0)
    own = (masks[:, OWN_J] >> np.uint64(OWN_I)) & np.uint64(1)
    assert 0 < own.sum() < N_CENTRE
    got = np.array([(orc.visible_cells(edf[w][0], p)[OWN_J] >> np.uint64(OWN_I)) & np.uint64(1) for p in poses])
    assert np.array_equal(got, own)
    # sine and cosine both negative: fma(c, 0, s * 0) is -0 and atan2(+0, -0) = pi, but np.dot returns +0 and the reference sees the cell
    p = z[w + "__vis_poses"][N_CENTRE + 1]
    assert tuple(p[:2]) == (14.75, 14.75) and np.cos(p[2]) < 0 and np.sin(p[2]) < 0
    assert (z[w + "__vis_masks"][N_CENTRE + 1][59] >> np.uint64(59)) & np.uint64(1) == 1
    assert (orc.visible_cells(edf[w][0], p)[59] >> np.uint64(59)) & np.uint64(1) == 1


@pytest.mark.parametrize("w", WORLDS)
def test_check_visibility(z, edf, w):
    e = edf[w][0]
    a, b, want = z[w + "__cv_a"], z[w + "__cv_b"], z[w + "__cv_visible"]
    got = np.array([orc.check_visibility(e, x, y) for x, y in zip(a, b)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    outside = (a < -15.0).any(axis=1)  # negative raster indices: numpy wraps them
    assert outside.sum() >= 40 and got[outside].any() and (~got[outside]).any() and got[~outside].any() and (~got[~outside]).any()


@pytest.mark.parametrize("w", WORLDS)
def test_next_pose(z, edf, w):
    e = edf[w][0]
    acts = [np.array([v, ww]) for v in (0.0, 2.0, 4.0) for ww in (-0.5 * np.pi, 0, 0.5 * np.pi)]
    nxt, feas = z[w + "__np_next"], z[w + "__np_feasible"]
    for q, p in enumerate(z[w + "__vis_poses"]):
        for k, a in enumerate(acts):
            r = orc.next_pose(e, p, a)
            assert (r is not None) == bool(feas[q, k]), (q, k)
            if r is not None:
                assert np.abs(r - nxt[q, k]).max() <= 1e-12
    assert feas.any(axis=0).all() and (~feas)[:, 3:].any(axis=0).all()


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference checkout is only present in the development container")
def test_generator_reproduces_committed_fixture(tmp_path):
    env = dict(os.environ, CAGYM_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD_DIR, "make_golden_ig_edges.py")], check=True, env=env, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=300)
    assert filecmp.cmp(str(tmp_path / "ig_edges.npz"), GOLD, shallow=False), "ig_edges.npz differs from the committed fixture"
