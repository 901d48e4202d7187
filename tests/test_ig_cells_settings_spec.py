"""CPU: the inputs of tests/test_ig_cells_settings.py and a numpy twin of iga_cells' packed ballot (csrc/cagym_ig_assign.h).

iga_cells builds every cell set of k_ig_assign_goals and k_ig_route_gains: the rows of a pose's box are dealt 64 / wd at a time into
ONE ballot per trip and lane j cuts row j out of it, ((b >> (ms wd)) & wmask) << xs.  At the default 60 degrees and a range of at
most 5 m a box is 10 to 21 cells wide, so 64 / wd is never below 3 and the shift, the mask and the per-lane guards never leave that
regime.  The settings below - any fov and range InfoGain takes - reach 64 / wd = 1 and 2, wd = 32 (two rows fill the ballot), wd = 60
(the whole map), wd = 1 and the empty cone box; what they reach is asserted here, on the boxes restated in numpy, before the gpu
test compares anything.  The twin reproduces a predicate image on every one of those boxes, and each slip of SLIPS is run on them
and at range 5.0: which slips the range-5 inputs would have let through is printed and asserted.

Also the heading kernel's fp32 quotient (int)((q + 0.5f) * (1.0f / wd)), exhaustively: every wd in 1..60, every q < 3600."""
import importlib
import math

import numpy as np
import pytest

igm = importlib.import_module("gym-exploration-2d_amd.ig")
FOV60 = igm.FOV_DEG60
# (fov, range): (2 range)^2 is no integer, so no cell centre lies on the range circle of a cell-centre viewpoint
SETTINGS = ((FOV60, 0.3), (FOV60, 7.9), (2.9, 10.4), (FOV60, 16.1), (math.pi, 16.1), (2.9, 50.0))
SPEC_SETTINGS = tuple(s for s in SETTINGS if s[0] != math.pi)  # at fov pi the cone edges run through cell centres
N, R_ALL, K_ALL = 6, 8, 16
ROWS = (0, 7, 29, 30, 59)
COLS = (0, 1, 3, 5, 8, 11, 13, 15, 16, 18, 21, 24, 27, 29, 30, 32, 35, 38, 41, 43, 44, 46, 50, 54, 58, 59)
# the poses held to the numpy specifications, (i, j, h) with h the heading h 2 pi / 8 or None - a robot turning on the spot: an
# interior cell, the two border-clipped rectangles of width 32 at range 7.9 (the second with xs > 0 and its right edge in column
# 59), the one of width 22, a corner, an edge; then cones in the open, on every edge (column 0 looking west: the empty box) and in a corner
KEYS = ((30, 30, None), (15, 29, None), (44, 7, None), (5, 59, None), (0, 0, None), (59, 30, None),
        (30, 29, 0), (0, 30, 4), (59, 59, 5), (29, 0, 2), (13, 7, 1), (46, 30, 7))


def centre(c):
    return c * 0.5 - 15.0 + 0.25


def lattice():
    """the 128 cell-centre poses of every world: cells [128, 2] (i, j) and the heading index h [128] each is given as a candidate
    with a heading - the KEYS first, then ROWS x COLS"""
    cells = [(i, j) for i, j, _ in KEYS]
    hs = [0 if h is None else h for _, _, h in KEYS]
    for j in ROWS:
        for i in COLS:
            if (i, j) not in cells and len(cells) < R_ALL * K_ALL:
                cells.append((i, j))
                hs.append((3 * i + 5 * j) % 8)
    assert len(cells) == R_ALL * K_ALL
    return np.array(cells, dtype=np.int64), np.array(hs, dtype=np.int64)


def off_lattice():
    """comparison 1's poses: [N, 8, 16, 3] (x, y, heading) anywhere in the map, any heading (and the same places without one)"""
    rng = np.random.default_rng(41)
    poses = np.concatenate([rng.uniform(-14.95, 14.95, (N, R_ALL, K_ALL, 2)), rng.uniform(-math.pi, math.pi, (N, R_ALL, K_ALL, 1))], axis=-1)
    # three places within 0.2 m of the map's border: at range 0.3 the rectangle is clipped to one column, one row, one cell
    poses[:, 0, 0, 0], poses[:, 0, 1, 1], poses[:, 0, 2, :2] = 14.9, -14.93, (14.85, 14.9)
    return poses


def _cell(v):
    return int(min(max(math.floor((v + 15.0) / 0.5), -10 ** 6), 10 ** 6))


def rect_box(x, y, rng):
    """igv_rect: (xs, ys, wd, ht) of the unheaded rectangle cell(p - range) .. cell(p + range) inside the map"""
    xs, ys = max(0, _cell(x - rng)), max(0, _cell(y - rng))
    xe, ye = min(59, _cell(x + rng)), min(59, _cell(y + rng))
    return xs, ys, xe - xs + 1, ye - ys + 1


def cone_box(x, y, phi, fov, rng):
    """ig_visible_box: (xs, ys, wd, ht) of the cone's box, its upper bounds exclusive as the reference's ranges are"""
    clamp = lambda v: max(min(v, 15.0), -15.0)
    cxs = [_cell(x)] + [_cell(clamp(x + rng * math.cos(a))) for a in (phi, phi + fov, phi - fov)]
    cys = [_cell(y)] + [_cell(clamp(y + rng * math.sin(a))) for a in (phi, phi + fov, phi - fov)]
    xs, xe, ys, ye = max(min(cxs), 0), min(max(cxs), 60), max(min(cys), 0), min(max(cys), 60)
    return xs, ys, xe - xs, ye - ys


def predicate(x, y, phi, fov, rng, seed=0):
    """A stand-in for `wanted and visible` of every cell of the map, [60, 60] bool indexed [j, i]: the cone (or, phi None, the
    range) test of the specifications in numpy, and a fixed pattern that hides one cell in seven in place of the sphere trace."""
    jj, ii = np.meshgrid(np.arange(60), np.arange(60), indexing="ij")
    dx, dy = centre(ii) - x, centre(jj) - y
    if phi is None:
        want = dx * dx + dy * dy < rng * rng
    else:
        s, c = math.sin(phi), math.cos(phi)
        r0, r1 = c * dx + s * dy, -s * dx + c * dy
        want = (np.sqrt(r0 * r0 + r1 * r1) < rng) & (np.abs(np.arctan2(r1 + 0.0, r0 + 0.0)) < fov / 2)
    return want & ((3 * ii + 5 * jj + seed) % 7 != 0)


SLIPS = ("no_sub_guard", "shift_by_rpt", "no_wmask", "no_row_guard", "no_xs_shift")
U64 = (1 << 64) - 1


def ballot_twin(image, box, slip=None):
    """iga_cells' trip loop for one pose, lane by lane: image [60, 60] bool is `wanted and visible` of every cell of the map (a cell
    outside it: False), box = (xs, ys, wd, ht).  Returns (words [60] uint64, the number of cells tested outside the box).  slip:
      no_sub_guard   `sub < rpt` dropped: the lanes behind the trip's last whole row test the next rows' first cells
      shift_by_rpt   the lane's row is cut out at bit ms rpt instead of ms wd
      no_wmask       the row word keeps the ballot's bits above its own wd
      no_row_guard   `jj < ht` dropped: the last trip tests the rows above the box
      no_xs_shift    the row word stays at bit 0"""
    xs, ys, wd, ht = box
    words = [0] * 64
    if wd <= 0 or ht <= 0:
        return np.zeros(60, dtype=np.uint64), 0
    lane = np.arange(64)
    rpt = 64 // wd
    sub = lane // wd
    col = lane - sub * wd
    wmask = (1 << wd) - 1
    beyond = 0
    for t0 in range(0, ht, rpt):
        jj = t0 + sub
        on = np.ones(64, dtype=bool)
        if slip != "no_sub_guard":
            on &= sub < rpt
        if slip != "no_row_guard":
            on &= jj < ht
        i, j = xs + col, ys + jj
        beyond += int((on & ((jj >= ht) | (sub >= rpt))).sum())
        inside = on & (i < 60) & (j < 60)
        vis = np.zeros(64, dtype=bool)
        vis[inside] = image[j[inside], i[inside]]
        b = sum(1 << int(n) for n in np.flatnonzero(vis))
        for ms in range(rpt):
            row = ys + t0 + ms  # the lane whose row this is
            if row >= 64:
                continue
            w = b >> (ms * (rpt if slip == "shift_by_rpt" else wd))
            if slip != "no_wmask":
                w &= wmask
            if slip != "no_xs_shift":
                w <<= xs
            words[row] = w & U64
    return np.array(words[:60], dtype=np.uint64), beyond


def in_box(image, box):
    """the cell set iga_cells must return: the image inside the box"""
    xs, ys, wd, ht = box
    out = np.zeros((60, 60), dtype=bool)
    if wd > 0 and ht > 0:
        out[ys:ys + ht, xs:xs + wd] = image[ys:ys + ht, xs:xs + wd]
    return out


def boxes_of(fov, rng):
    """every box of the gpu test at one setting: (headed, x, y, phi or None, box) - the lattice poses without a heading and with
    each of the eight, and the off-lattice poses with and without theirs"""
    cells, _ = lattice()
    out = []
    for i, j in cells:
        x, y = centre(int(i)), centre(int(j))
        out.append((False, x, y, None, rect_box(x, y, rng)))
        for h in range(8):
            phi = h * 2.0 * math.pi / 8
            out.append((True, x, y, phi, cone_box(x, y, phi, fov, rng)))
    for x, y, phi in off_lattice().reshape(-1, 3):
        out.append((True, float(x), float(y), float(phi), cone_box(float(x), float(y), float(phi), fov, rng)))
        out.append((False, float(x), float(y), None, rect_box(float(x), float(y), rng)))
    return out


# ---- 1. what the settings and the poses were picked for ---------------------------------------------------------------------------
def missing_regimes(boxes, verbose=False):
    """boxes: {(fov, range): [(headed, x, y, phi, box)]}.  The regimes of the packed ballot that NO box reaches, by name."""
    rpts = {False: set(), True: set()}
    widths = {False: set(), True: set()}
    whole_map = right_edge = empty = 0
    clipped_32 = set()
    for (fov, rng), rows in boxes.items():
        for headed, x, y, phi, (xs, ys, wd, ht) in rows:
            if wd <= 0 or ht <= 0:
                empty += int(headed and wd == 0)
                continue
            rpts[headed].add(64 // wd)
            widths[headed].add(wd)
            whole_map += int(wd == 60 and ht == 60)
            right_edge += int(not headed and xs > 0 and xs + wd == 60)
            if not headed and rng == 7.9 and wd == 32 and (xs == 0 or xs + wd == 60):
                clipped_32.add(xs)
    if verbose:
        print("rows per trip reached: unheaded %s, headed %s; widths unheaded %d .. %d, headed %d .. %d; %d whole-map boxes, %d empty cone boxes"
              % (sorted(rpts[False]), sorted(rpts[True]), min(widths[False]), max(widths[False]), min(widths[True]), max(widths[True]), whole_map, empty))
    missing = []
    for headed in (False, True):
        name = "headed" if headed else "unheaded"
        missing += ["%s 64 // wd == %d" % (name, v) for v in (1, 2) if v not in rpts[headed]]
        if not any(v >= 7 for v in rpts[headed]):
            missing.append("%s 64 // wd >= 7" % name)
        missing += ["%s wd == 1" % name] if 1 not in widths[headed] else []
    missing += ["a border-clipped rectangle of width 32 at range 7.9, at either border"] if clipped_32 != {0, 28} else []
    missing += ["wd == 60 with ht == 60"] if not whole_map else []
    missing += ["an empty headed box"] if not empty else []
    missing += ["a rectangle with xs > 0 whose right edge is column 59"] if not right_edge else []
    return missing


def test_the_settings_reach_every_regime_of_the_packed_ballot():
    missing = missing_regimes({s: boxes_of(*s) for s in SETTINGS}, verbose=True)
    assert not missing, missing
    # ... none of which the default setting reaches at a range of 5.0, 4.9 or 2.3
    for rng in (5.0, 4.9, 2.3):
        r5 = {64 // b[4][2] for b in boxes_of(FOV60, rng) if b[4][2] > 0 and b[4][3] > 0}
        assert min(r5) >= 3, (rng, sorted(r5))
    # the KEYS sit in the rows whose margins were measured, and hold the boxes they are named for at range 7.9
    assert all(j in ROWS for _, j, _ in KEYS)
    named = [rect_box(centre(i), centre(j), 7.9) for i, j, _ in KEYS[:4]]
    assert [b[2] for b in named] == [33, 32, 32, 22] and named[1][0] == 0 and named[2][0] == 28 and named[2][0] + named[2][2] == 60
    assert cone_box(centre(0), centre(30), 4 * 2.0 * math.pi / 8, FOV60, 7.9)[2] == 0


def test_the_lattice_poses_keep_their_margins():
    """Every lattice pose the gpu test holds to the numpy specifications - the KEYS - is farther than 1e-6 from a cone edge and from
    the range circle at the five settings whose fov is not pi (the gpu test asserts the same on the poses it compares); at fov pi
    and headings h 2 pi / 8 a cone edge runs through cell centres, which is why that setting is compared device against device only."""
    from test_ig_headings_spec import margins
    smallest = [math.inf, math.inf]
    for fov, rng in SPEC_SETTINGS:
        for i, j, h in KEYS:
            a, rad = margins(centre(i), centre(j), [] if h is None else [h * 2.0 * math.pi / 8], fov, rng)
            smallest = [min(smallest[0], a), min(smallest[1], rad)]
            assert a > 1e-6 and rad > 1e-6, (fov, rng, i, j, h, a, rad)
    print("smallest margins over the KEYS: %.3g rad, %.3g m" % tuple(smallest))
    assert margins(centre(30), centre(29), [0.0], math.pi, 16.1)[0] < 1e-9


# ---- 2. the heading kernel's quotient -----------------------------------------------------------------------------------------------
def test_the_fp32_quotient_of_the_heading_kernel_is_exact():
    """k_ig_view_gain_headings finds a candidate's row as (int)(((float)q + 0.5f) * (1.0f / (float)wd)): the quotient q / wd for
    every q < 3600 and wd <= 60 - at range 50 it is evaluated for 57 trips of 64 candidates, at range 5 for 7."""
    q = np.arange(3600)
    for wd in range(1, 61):
        rwd = np.float32(1.0) / np.float32(wd)
        prod = (q.astype(np.float32) + np.float32(0.5)) * rwd
        assert prod.dtype == np.float32
        assert np.array_equal(prod.astype(np.int64), q // wd), wd
    assert (3600 + 63) // 64 == 57 and (21 * 21 + 63) // 64 == 7


# ---- 3. the twin, and what each slip changes -------------------------------------------------------------------------------------------
def _words(cells):
    return igm.cells_to_words(cells)


def test_the_twin_reproduces_the_image_on_every_box_of_the_gpu_test():
    n = 0
    for fov, rng in SETTINGS:
        for q, (headed, x, y, phi, box) in enumerate(boxes_of(fov, rng)):
            image = predicate(x, y, phi, fov, rng, seed=q)
            words, beyond = ballot_twin(image, box)
            assert beyond == 0 and np.array_equal(words, _words(in_box(image, box))), (fov, rng, x, y, phi, box)
            n += 1
    print("%d boxes" % n)
    assert n == 6 * (128 * 9 + 768 * 2)


def _slip_changes(fov, rng, poses):
    """per slip, how many of the poses' masks it changes and how many cells outside the box it tests"""
    changed = {s: 0 for s in SLIPS}
    beyond = {s: 0 for s in SLIPS}
    for q, (i, j, h) in enumerate(poses):
        x, y = centre(i), centre(j)
        phi = None if h is None else h * 2.0 * math.pi / 8
        box = rect_box(x, y, rng) if h is None else cone_box(x, y, phi, fov, rng)
        image = predicate(x, y, phi, fov, rng, seed=q)
        want = _words(in_box(image, box))
        for s in SLIPS:
            words, b = ballot_twin(image, box, s)
            changed[s] += int(not np.array_equal(words, want))
            beyond[s] += b
    return changed, beyond


def test_every_slip_of_the_ballot_shows_and_what_range_five_would_have_missed():
    """The KEYS and the same cells with the other headings, at the six settings and at the suite's own (60 degrees, 5.0).
    shift_by_rpt, no_wmask, no_row_guard and no_xs_shift each change a mask at the new settings.  no_sub_guard changes no mask at any
    setting, and cannot: lane sub >= rpt writes ballot bit rpt wd or above, and a row is cut out of the bits ms wd .. ms wd + wd - 1
    with ms < rpt.  The guard saves the traces of cells the mask then drops - among them cells of rows beyond the map - and that
    work is what the twin counts for it."""
    poses = list(KEYS) + [(i, j, (h0 or 0) + 3) for i, j, h0 in KEYS] + [(i, j, None) for i, j, h in KEYS if h is not None]
    new = {s: 0 for s in SLIPS}
    work = {s: 0 for s in SLIPS}
    for fov, rng in SETTINGS:
        c, b = _slip_changes(fov, rng, poses)
        for s in SLIPS:
            new[s] += c[s]
            work[s] += b[s]
    old, _ = _slip_changes(FOV60, 5.0, poses)
    hidden = [s for s in SLIPS if old[s] == 0]
    print("masks changed at the new settings: %s; at (60 degrees, 5.0): %s; slips range 5 lets through: %s" % (new, old, hidden))
    for s in ("shift_by_rpt", "no_wmask", "no_row_guard", "no_xs_shift"):
        assert new[s] > 0, s
    assert new["no_sub_guard"] == 0 and old["no_sub_guard"] == 0 and work["no_sub_guard"] > 0
    assert work["shift_by_rpt"] == 0 and work["no_wmask"] == 0 and work["no_xs_shift"] == 0
    assert hidden == HIDDEN_AT_RANGE_5


HIDDEN_AT_RANGE_5 = ["no_sub_guard", "no_row_guard"]  # the record: what the line printed above says, asserted
