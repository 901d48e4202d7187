"""Hand-made worlds for the geodesic field kernel k_ig_geodesic (csrc/cagym_ig_geodesic.h), plain numpy: rectangles [n, 4] =
(xl, yl, xu, yu) for set_scenarios(obstacles=...), and what tests/test_ig_goals_edges.py asserts about them on the CPU before any
device comparison.

The grid.  The raster has 300 x 300 cells of 0.1 m; a rectangle fills the raster rows floor(150 - yu / 0.1) .. floor(150 - yl / 0.1)
and the columns floor(150 + xl / 0.1) .. floor(150 + xu / 0.1), both ends included (oracle.rasterize).  The distance field reads the
raster WITHOUT that y-flip: belief cell (i, j) - i along x, j along y, 0.5 m - is free iff d2 > 36 at raster cell (row 5 j + 2,
column 5 i + 2), d2 the squared distance in raster cells to the nearest occupied one (radius 0.5: EDF > 0.6 m).  So the worlds here
are laid out in raster rows and columns, box() turns a block of raster cells into the rectangle that fills exactly that block (its
corners are raster-cell centres: no floor() of a value on a cell border), and a field's row j is a raster row, not a world y.

The kernel's structure the worlds aim at: thread t < 240 owns column t % 60, rows 15 (t / 60) .. + 14 of the field.  A strip's first
and last cell read their vertical neighbour from LDS, every other cell from a register: the seams are the row pairs 14/15, 29/30,
44/45.  Rows and columns 0 and 59 lie next to the tile's infinite halo.

serpentine      19 walls two raster cells thick between one-cell-wide corridors at a pitch of 3 belief cells, each wall 0.7 m
                beyond a corridor's centre line, with 2-cell gaps alternating between the two ends: one chain through 20 corridors,
                about 600 m long.  Corridors along the field's rows axis (every corridor crosses the three seams), or transposed:
                along its columns axis, where every advance crosses a column - a thread boundary - and costs a sweep.  The two
                columns (rows) beyond the last corridor stay open.
staircase       a diagonal chain of small squares at a pitch of 3 belief cells.  Every square blocks a blob of belief cells; where
                two blobs touch at a corner two free cells face each other across two blocked ones, and along a blob's flank a free
                pair has one blocked orthogonal cell: diagonals the field must refuse.  `origin` shifts the chain against the strip
                seams, `mirrored` runs it NW-SE (the kernel's four diagonal bits are separate code), `missing` leaves squares out.
sealed_pocket   a ring of four walls round a pocket of free cells, and two one-cell dots that block the four orthogonal neighbours
                of a free cell and leave two of its diagonal neighbours free.
open_map        no rectangle at all: the field is the octile distance."""
import numpy as np

from oracle import oracle as orc

MAPD, BEL = 300, 60
SEAMS = (15, 30, 45)  # the first row of the kernel's strips 1, 2 and 3: a seam is the row pair (s - 1, s)
D2_FREE = 36          # free <=> d2 > 36 (radius 0.5 m: EDF > 0.6 m)


def box(r0, r1, c0, c1):
    """the rectangle (xl, yl, xu, yu) that fills raster rows r0 .. r1 and columns c0 .. c1 (both included), clipped to the raster"""
    r0, r1, c0, c1 = max(r0, 0), min(r1, MAPD - 1), max(c0, 0), min(c1, MAPD - 1)
    return [(c0 - 149.5) * 0.1, (149.5 - r1) * 0.1, (c1 - 149.5) * 0.1, (149.5 - r0) * 0.1]


def raster_of(rects):
    return orc.rasterize(np.asarray(rects, dtype=np.float64).reshape(-1, 4))


def edf_of(rects):
    """the distance field [300, 300] f64 in metres, as InfoGain.edf() returns it for a slot that holds these rectangles"""
    return orc.edt(raster_of(rects))[0]


def free_mask(rects):
    """free[j, i] of geodesic_spec for radius 0.5, before the source cell is added, from the integer d2"""
    return orc.edt(raster_of(rects))[1][2::5, 2::5] > D2_FREE


def centre(i, j):
    """the centre of belief cell (i, j) in the field's frame"""
    return (i * 0.5 - 15.0 + 0.25, j * 0.5 - 15.0 + 0.25)


def serpentine(transposed=False, phase=9):
    """Corridor k = 0 .. 19 is column 3 k of the field (raster column 15 k + 2 is its centre line); wall k = 0 .. 18 fills the raster
    columns 15 k + 9 and 15 k + 10, 0.7 m beyond that line and 0.7 m before the next one.  An even wall leaves the rows 58 and 59
    free (it ends at raster row 286: row 58's centre, raster row 292, is 6 raster cells away and 2 to the side - d2 = 40), an odd one
    the rows 0 and 1.  transposed: rows and columns change places.
    phase: the first wall's first raster column.  With 14 the corridors are the columns 3 k + 1, column 0 is open beside the first
    and column 59 beside the last, and the walls map onto themselves under c -> 299 - c (wall k onto wall 18 - k, which leaves the
    same end free): transposed, that is a world whose raster is its own y-flip - the env's wall-collision test, which reads the
    raster flipped, and the distance field, which does not, then see the same walls."""
    rects = []
    for k in range(19):
        r0, r1 = (0, 286) if k % 2 == 0 else (13, 299)
        c0, c1 = 15 * k + phase, 15 * k + phase + 1
        rects.append(box(c0, c1, r0, r1) if transposed else box(r0, r1, c0, c1))
    return np.array(rects)


def staircase(step=1.5, side=0.3, missing=(), mirrored=False, origin=(21, 11), count=19, foot=True):
    """Squares of `side` metres every `step` metres along a diagonal: square n = 0 .. count - 1, those in `missing` left out, has its
    first raster cell at row origin[0] + n step / 0.1 and column origin[1] + n step / 0.1 - mirrored: the column counted back from
    299 - and is dropped where it leaves the raster.  A square of 3 raster cells blocks 3 x 3 belief cells when it starts 4 raster
    cells into a belief cell (the centre lines 6, 1, 4 cells before and 6 behind it: d2 <= 36), and at a pitch of 3 belief cells
    these blobs touch at their corners.  With the defaults they touch between the rows 5/6, 8/9, .. - 14/15, 29/30 and 44/45 among
    them - and the columns 3/4, 6/7, ...  foot: one more block, one raster cell wide, on the raster's first column a step below
    square 0; its blob is the single column 0 (column 1's centre line is 7 cells away), rows 0 .. 2, and touches square 0's blob
    at the corner between columns 0 and 1: refused diagonals of both kinds on the map's border."""
    p, s = int(round(step * 10)), int(round(side * 10))
    at = lambda r, c, w: box(r, r + s - 1, MAPD - c - w, MAPD - 1 - c) if mirrored else box(r, r + s - 1, c, c + w - 1)
    rects = [at(origin[0] - p, 0, 1)] if foot else []
    for n in range(count):
        if n in missing:
            continue
        r, c = origin[0] + n * p, origin[1] + n * p
        if r + s > MAPD or c + s > MAPD or r < 0 or c < 0:
            continue
        rects.append(at(r, c, s))
    return np.array(rects)


POCKET = (20, 24)  # the pocket's free cells: columns and rows 20 .. 23
LONELY = (40, 12)  # the free cell (i, j) whose four orthogonal neighbours the two dots block


def sealed_pocket():
    """Four walls two raster cells thick round the belief cells 20 .. 23 squared: the walls' inner faces are 7 raster cells from the
    first and last centre line of the pocket (free), their blocked bands overlap at the corners.  Two dots, one raster cell each, on
    the centres of the cells NE and SW of LONELY: a one-cell dot blocks its own cell and the four next to it (d2 = 0 and 25) and no
    diagonal neighbour (d2 = 50), so LONELY, its NW and its SE neighbour are free and E, N, W, S of it are blocked."""
    lo, hi = 5 * POCKET[0] + 2 - 7, 5 * (POCKET[1] - 1) + 2 + 7  # the inner faces: raster 95 and 124
    rects = [box(lo - 1, lo, lo - 1, hi + 1), box(hi, hi + 1, lo - 1, hi + 1), box(lo - 1, hi + 1, lo - 1, lo), box(lo - 1, hi + 1, hi, hi + 1)]
    i, j = LONELY
    for di, dj in ((1, 1), (-1, -1)):
        rects.append(box(5 * (j + dj) + 2, 5 * (j + dj) + 2, 5 * (i + di) + 2, 5 * (i + di) + 2))
    return np.array(rects)


def open_map():
    return np.zeros((0, 4))


DIAGONALS = ((1, 1), (-1, 1), (-1, -1), (1, -1))  # NE, NW, SW, SE as (di, dj): the order of the kernel's four bits


def refused_diagonals(free):
    """Every diagonal step between two free cells that the rule refuses, once per direction: rows (i, j, di, dj, n) - from cell (i, j)
    to (i + di, j + dj), n = 1 or 2 of the two orthogonal cells (i + di, j) and (i, j + dj) blocked."""
    out = []
    for j in range(BEL):
        for i in range(BEL):
            if not free[j, i]:
                continue
            for di, dj in DIAGONALS:
                ni, nj = i + di, j + dj
                if 0 <= ni < BEL and 0 <= nj < BEL and free[nj, ni]:
                    n = int(not free[j, ni]) + int(not free[nj, i])
                    if n:
                        out.append((i, j, di, dj, n))
    return np.array(out, dtype=np.int64).reshape(-1, 5)


def on_seam(rows, seam):
    """which rows of refused_diagonals() have their two cells in the rows seam - 1 and seam"""
    j, nj = rows[:, 1], rows[:, 1] + rows[:, 3]
    return np.minimum(j, nj) == seam - 1


def on_border(rows):
    """which rows of refused_diagonals() have a cell in row or column 0 or 59"""
    cells = np.stack([rows[:, 0], rows[:, 1], rows[:, 0] + rows[:, 2], rows[:, 1] + rows[:, 3]], axis=1)
    return ((cells == 0) | (cells == BEL - 1)).any(axis=1)


def octile(si, sj):
    """the obstacle-free distance from cell (si, sj) in exact arithmetic, [60, 60] f64: min(a, b) diagonal and |a - b| straight moves"""
    a, b = np.abs(np.arange(BEL)[None, :] - si), np.abs(np.arange(BEL)[:, None] - sj)
    return np.minimum(a, b) * (0.5 * np.sqrt(2.0)) + np.abs(a - b) * 0.5
