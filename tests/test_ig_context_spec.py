"""CPU: ig.context_window_spec, the numpy statement of cagym_ig_context_window's three channels that tests/test_ig_context.py holds
the kernel to, the layout of the call's parameter block and its prototype row.  A distance field with a different value in every
raster cell makes every misplaced, transposed or mirrored cell visible."""
import ctypes
import importlib
import os
import subprocess

import numpy as np

from test_abi import ROOT, _c_compiler

igm = importlib.import_module("gym-exploration-2d_amd.ig")
_lib = importlib.import_module("gym-exploration-2d_amd._lib")
NONE = ([np.zeros((0, 2))], [np.zeros(0)])  # no agents round one robot


def _edf():
    return np.random.default_rng(7).uniform(0.0, 4.0, size=(300, 300))  # [row = y, column = x], metres, all distinct


def _observed():
    return np.random.default_rng(8).integers(0, 1 << 60, size=60, dtype=np.int64)


def test_heading_zero_on_a_cell_corner_is_a_slice_of_the_capped_field():
    """A robot at the origin, heading 0: out cell (a, b) samples (0.25 + 0.5 (a - G/2), 0.25 + 0.5 (b - G/2)), the raster cell
    (column, row) = (152 + 5 (a - G/2), 152 + 5 (b - G/2)): channel 0 is every fifth cell of min(edf, cap) / cap, a along x."""
    edf = _edf()
    for G, cap in ((4, 3.0), (24, 3.0), (24, 0.7)):
        win, a_s, b_s, fx, fy = igm.context_window_spec(edf, None, [[0.0, 0.0, 0.0]], *NONE, G, True, cap)
        assert win.shape == (1, 3, G, G) and win.dtype == np.float32
        lo = 152 - 5 * (G // 2)
        block = edf[lo:lo + 5 * G:5, lo:lo + 5 * G:5]  # [row, column]
        assert np.array_equal(win[0, 0], (np.minimum(block, cap) / cap).T.astype(np.float32))
        assert win[0, 0].max() == 1.0 and (win[0, 0] < 1.0).any()  # the cap bites, and not everywhere
        assert (win[0, 1] == 0).all() and (win[0, 2] == 0).all()  # no agents; observed None: nothing seen
        assert len(a_s) == 1 and a_s[0].shape == (0,)


def test_outside_the_map_everything_is_zero_but_the_agents():
    """A robot 1 m inside the map's corner: clearance and seen-now are 0 beyond x = 15 or y = 15; a walker standing out there
    still shows (channel 1 is not masked by the map)."""
    edf, obs = _edf() + 0.1, np.full(60, -1, dtype=np.int64)  # every cell observed, no clearance of 0 inside
    poses = [[14.0, 14.0, 0.0], [-14.0, 14.0, 0.0]]
    xy, val = [np.array([[15.6, 14.1]]), np.zeros((0, 2))], [np.array([0.5]), np.zeros(0)]
    win, a_s, b_s, fx, fy = igm.context_window_spec(edf, obs, poses, xy, val, 24, False, 3.0)
    _, i, j, qx, qy = igm.belief_window_spec(np.ones((60, 60)), np.zeros((60, 60)), poses, 24, False)
    inside = (qx >= -15) & (qx < 15) & (qy >= -15) & (qy < 15)
    assert 0 < inside[0].sum() < 24 * 24 and 0 < inside[1].sum() < 24 * 24
    assert np.array_equal(win[:, 2], inside.astype(np.float32))
    assert (win[:, 0][~inside] == 0).all() and (win[:, 0][inside] > 0).all()
    assert (a_s[0][0], b_s[0][0]) == (15, 12) and not inside[0, 15, 12]
    assert win[0, 1, 15, 12] == 0.5 and win[:, 1].sum() == 0.5


def test_a_rotation_by_pi_reverses_both_axes_of_every_channel():
    """Away from raster, belief-cell and window-cell borders (the sine of numpy's pi is 1.2e-16, not 0) the image at heading pi is
    the image at heading 0 reversed along both axes: window cell c of an offset f becomes cell G - 1 - c of the offset -f."""
    edf, obs = _edf(), _observed()
    p = [1.3, -2.2]
    xy = [np.array([[1.9, -1.85], [-0.55, -4.1], [1.45, -2.05], [9.0, 9.0]])]  # offsets (0.6, 0.35), (-1.85, -1.9), (0.15, 0.15), far away
    val = [np.array([1.0, 0.5, 0.5, 1.0])]
    w0, a0, b0, _, _ = igm.context_window_spec(edf, obs, [p + [0.0]], xy, val, 24, True, 3.0)
    assert (w0[0, 1] > 0).sum() == 3 and 0 < w0[0, 2].sum() < 24 * 24 and len(np.unique(w0[0, 0])) > 100
    for th in (np.pi, -np.pi):
        wp, ap, bp, _, _ = igm.context_window_spec(edf, obs, [p + [th]], xy, val, 24, True, 3.0)
        assert np.array_equal(wp, w0[:, :, ::-1, ::-1])
        assert np.array_equal(ap[0], 23 - a0[0]) and np.array_equal(bp[0], 23 - b0[0])
    wr = igm.context_window_spec(edf, obs, [p + [np.pi]], xy, val, 24, False, 3.0)[0]
    assert np.array_equal(wr, w0)  # rotate=False ignores the heading


def test_agent_values():
    """A teammate gives 1.0, a walker 0.5, a static target nothing (the caller's lists leave it out); a teammate and a walker in one
    cell give 1.0 in either order; an agent at a_s == G (or b_s == -1) is dropped.  Heading pi / 2: forward is +y, left is -x."""
    G = 8  # the window spans 2 m to every side: window cell = floor(2 f) + 4
    pose = [[2.0, 3.0, 0.0]]
    xy = np.array([[2.6, 3.2],    # teammate:            f = (0.6, 0.2)   -> (5, 4)
                   [1.1, 2.4],    # walker:              f = (-0.9, -0.6) -> (2, 2)
                   [3.3, 1.6],    # walker ...           f = (1.3, -1.4)  -> (6, 1)
                   [3.4, 1.9],    # ... and a teammate in the same cell
                   [0.2, 4.7],    # teammate ...         f = (-1.8, 1.7)  -> (0, 7)
                   [0.4, 4.6],    # ... and a walker in the same cell, in the other order
                   [4.0, 3.0],    # teammate at f_x = 2.0 exactly: a_s = 8 == G, dropped
                   [2.0, 0.9]])   # walker at f_y = -2.1: b_s = -1, dropped
    val = np.array([1.0, 0.5, 0.5, 1.0, 1.0, 0.5, 1.0, 0.5])
    win, a_s, b_s, fx, fy = igm.context_window_spec(np.ones((300, 300)), None, pose, [xy], [val], G, True, 3.0)
    assert list(zip(a_s[0], b_s[0])) == [(5, 4), (2, 2), (6, 1), (6, 1), (0, 7), (0, 7), (8, 4), (4, -1)]
    want = np.zeros((G, G), dtype=np.float32)
    want[5, 4], want[2, 2], want[6, 1], want[0, 7] = 1.0, 0.5, 1.0, 1.0
    assert np.array_equal(win[0, 1], want)
    assert np.array_equal(fx[0][:2], xy[:2, 0] - 2.0) and np.array_equal(fy[0][:2], xy[:2, 1] - 3.0)
    # no agents at all: the static targets of a world never reach the lists
    assert (igm.context_window_spec(np.ones((300, 300)), None, pose, *NONE, G, True, 3.0)[0][0, 1] == 0).all()
    # a quarter turn: the teammate 0.6 m along +x lies to the robot's RIGHT (b below G/2), the one 0.7 m along +y ahead of it
    q = igm.context_window_spec(np.ones((300, 300)), None, [[2.0, 3.0, np.pi / 2]], [np.array([[2.6, 3.2], [2.2, 3.7]])],
                                [np.array([1.0, 1.0])], G, True, 3.0)
    assert list(zip(q[1][0], q[2][0])) == [(4, 2), (5, 3)]
    # two robots: each has its own list, and what one robot's list holds leaves the other's image alone
    two = igm.context_window_spec(np.ones((300, 300)), None, [[2.0, 3.0, 0.0], [2.6, 3.2, 0.0]],
                                  [np.array([[2.6, 3.2]]), np.array([[2.0, 3.0]])], [np.array([1.0]), np.array([1.0])], G, False, 3.0)[0]
    assert two[0, 1, 5, 4] == 1.0 and two[0, 1].sum() == 1.0 and two[1, 1, 2, 3] == 1.0 and two[1, 1].sum() == 1.0


def test_bit_i_of_word_j_lands_on_cell_i_j():
    """Robot at the origin, heading 0, G = 24: out cell (a, b) reads belief cell (i, j) = (18 + a, 18 + b)."""
    obs = np.zeros(60, dtype=np.int64)
    obs[28] = 1 << 31
    obs[20] = (1 << 19) | (1 << 59)  # (bit 59: cell (59, 20), outside this window)
    obs[5] = -1                      # (row 5 lies outside it too)
    win = igm.context_window_spec(np.ones((300, 300)), obs, [[0.0, 0.0, 0.0]], *NONE, 24, True, 3.0)[0]
    want = np.zeros((24, 24), dtype=np.float32)
    want[31 - 18, 28 - 18] = want[19 - 18, 20 - 18] = 1.0
    assert np.array_equal(win[0, 2], want)
    # the sign bit of an int64 word is bit 63 and no cell; an all-ones word shows its whole row, as uint64 too
    obs = np.zeros(60, dtype=np.int64)
    obs[30] = -1
    for words in (obs, obs.view(np.uint64)):
        win = igm.context_window_spec(np.ones((300, 300)), words, [[0.0, 0.0, 0.0]], *NONE, 24, True, 3.0)[0]
        assert (win[0, 2][:, 12] == 1).all() and win[0, 2].sum() == 24


def test_parameter_block_mirror_matches_the_header(tmp_path):
    """sizeof and offsetof of cagym_ig_context_params (include/cagym_ig_context.h), as the host C compiler lays it out, against the
    ctypes mirror; the flag's value; the prototype row takes the six arguments the header declares."""
    S = _lib.IgContextParams
    fields = [f[0] for f in S._fields_]
    assert fields == ["n_robots", "window", "rotate", "flags", "clear_max"]
    lines = ['printf("size %d\\n", (int)sizeof(struct cagym_ig_context_params));']
    lines += ['printf("%s %%d\\n", (int)offsetof(struct cagym_ig_context_params, %s));' % (f, f) for f in fields]
    lines += ['printf("flag %d\\n", (int)CAGYM_IG_CONTEXT_ONLY_MASKED);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cagym_ig_context.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([_c_compiler(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert ctypes.sizeof(S) == int(got["size"]) == 24
    for f in fields:
        assert getattr(S, f).offset == int(got[f]), f
    assert int(got["flag"]) == _lib.IG_CONTEXT_ONLY_MASKED == igm.CONTEXT_ONLY_MASKED == 1


def test_prototype_row():
    row = _lib._ARGTYPES["cagym_ig_context_window"]
    assert len(row) == 6 and row[1] is ctypes.POINTER(_lib.IgContextParams)
    header = open(os.path.join(ROOT, "include", "cagym.h")).read()
    assert "typedef struct cagym_ig_context_params cagym_ig_context_params;" in header
    assert "struct cagym_ig_context_params {" not in header  # (defined in a header of its own)
