"""CPU: the hand-made fields of tests/test_ig_route_edges.py, and what each was built for, on ig.route_path_spec / ig.route_spec alone.

igr_next (csrc/cagym_ig_route.h) restates k_ig_goal_actions' neighbour choice, and cagym_ig_route_gains takes any field tensor.  On a
real geodesic field an exact tie of two keys is luck, and a move that does not descend, a NaN, a -inf or a value below zero cannot
occur at all; here every one of them is built: a field is +inf everywhere but for small gadgets, and since a walk ends at ANY cell
that equals 0 one field holds sixteen independent gadgets, each with zeros of its own.

A decision gadget is a 5 x 5 block: the candidate in the middle, the eight values under test round it, and sixteen zeros round
those - whichever neighbour the rule takes, the walk ends one orthogonal move later, n = 2, and at stride 1 the single way-point IS
the neighbour taken.  A chain gadget is a row of given values with the candidate at its east end.  build() returns eight fields (the
eight robots of every world) of up to sixteen candidates each, and per candidate what it is there for.

Last, the two copies of the neighbour rule against each other: on every finite non-zero cell of every field here, and on sampled
cells of the hand-made worlds' specification fields, route_path_spec's first move is the cell goal_action_spec drives to."""
import importlib
import math

import numpy as np
import pytest

import geodesic_worlds as gw
from test_ig_goals_edges import _equal_key_diagonal, _field_of, _nb, _rounded_ties

igm = importlib.import_module("gym-exploration-2d_amd.ig")
INF, NAN = np.float32(np.inf), np.float32(np.nan)
ORTHO, DIAG = igm.GEO_ORTHO, igm.GEO_DIAG
NB = igm.GEO_NEIGHBOURS
R, K = 8, 16
STRIDES = (1, 2, 3, 51, 52, 53, 3601, 2 ** 31 - 1)  # 51 .. 53: n - 1, n, n + 1 of the corridor of 52 moves
CORRIDORS = sorted({n for s in (1, 2, 3) for n in (1, s - 1, s, s + 1, 16 * s, 16 * s + 1, 17 * s, 17 * s + 1)})
B_RULE, B_NONE, B_TOP, B_BOTTOM, B_SIDES, B_COUNT, B_TURNS, B_MIRROR = range(R)  # the fields build() returns


def _f32(v):
    return np.float32(v)


def _ring2():
    return [(a, b) for a in range(-2, 3) for b in range(-2, 3) if max(abs(a), abs(b)) == 2]


class _Bank(object):
    def __init__(self):
        self.cells = [dict() for _ in range(R)]   # (i, j) -> value
        self.cands = [[] for _ in range(R)]       # (i, j)
        self.gadgets = []                         # dict(name, kind, r, c, cell, n, first)

    def _slot(self, r):
        s = len(self.cands[r])
        assert s < K
        return 2 + 14 * (s % 4), 4 + 7 * (s // 4)  # the origin of a block 13 wide and 6 high; rows and columns 0, 1, 58, 59 stay free

    def _add(self, r, cells, cand, name, kind, n, first=None):
        for q, v in cells.items():
            assert q not in self.cells[r], (name, q)
            self.cells[r][q] = _f32(v)
        self.gadgets.append(dict(name=name, kind=kind, r=r, c=len(self.cands[r]), cell=cand, n=n, first=first))
        self.cands[r].append(cand)

    def decision(self, r, name, kind, own, ring, n, first=None):
        """ring: {k: value} of the neighbours in GEO_NEIGHBOURS order (missing: +inf); first: the neighbour index the rule takes"""
        ox, oy = self._slot(r)
        home = (ox + 2, oy + 2)
        cells = {home: own}
        for k, v in ring.items():
            cells[_nb(k, home)] = v
        for a, b in _ring2():
            cells[(home[0] + a, home[1] + b)] = 0.0
        self._add(r, cells, home, name, kind, n, None if first is None else _nb(first, home))

    def chain(self, r, name, kind, values, n, extra=None):
        """values from the candidate's own westwards; extra: {(dx, dy): value} relative to the candidate"""
        ox, oy = self._slot(r)
        assert len(values) <= 12
        cand = (ox + 12, oy + 2)
        cells = {(cand[0] - t, cand[1]): v for t, v in enumerate(values)}
        for (a, b), v in (extra or {}).items():
            cells[(cand[0] + a, cand[1] + b)] = v
        self._add(r, cells, cand, name, kind, n)

    def place(self, r, name, kind, cells, cand, n):
        self._add(r, cells, cand, name, kind, n)

    def again(self, r, name, kind, c):
        """the candidate c of this field once more"""
        g = [g for g in self.gadgets if g["r"] == r and g["c"] == c][0]
        self.gadgets.append(dict(g, name=name, kind=kind, c=len(self.cands[r])))
        self.cands[r].append(g["cell"])

    def fields(self):
        return np.stack([_field_of(c) for c in self.cells])


def _turns_path():
    """a path of 16 moves whose first 15 - the way-points of stride 1 - run through all eight directions, E, NE, N, NW, W, SW, S,
    SE and E again: an open octagon; the cells in travel order, the source first, and the moves"""
    moves = [0] * 3 + [4] * 2 + [1] * 2 + [5] * 2 + [2] * 2 + [6] * 2 + [3] + [7] + [0]
    cells = [(30, 34)]
    for m in moves:
        cells.append((cells[-1][0] + NB[m][0], cells[-1][1] + NB[m][1]))
    return cells, moves


def build():
    B = _Bank()
    d_eq = _equal_key_diagonal()
    worse = _f32(1.25)
    # ---- field B_RULE: the neighbour choice, and candidates whose own value is no start of a walk
    for k in range(8):  # the neighbours k .. 7 share the smallest key 1.5; those before k are finite and worse (the diagonals' gates stay open)
        ring = {n: (_f32(1.0) if n < 4 else d_eq) for n in range(k, 8)}
        ring.update({n: (worse if n < 4 else _f32(1.0)) for n in range(k)})
        B.decision(B_RULE, "equal keys from %d" % k, "equal", 2.0, ring, 2, k)
    for n, (d, o) in enumerate(_rounded_ties()):  # S (3) against NE (4): equal in fp32, unequal exactly; E and N open the diagonal
        B.decision(B_RULE, "rounded tie %d" % n, "tie", _f32(o + _f32(2.0)), {3: o, 4: d, 0: _f32(o + _f32(1.0)), 1: _f32(o + _f32(1.0))}, 2, 3)
    gate = {4: 1.0, 0: 3.0, 2: 4.0}  # NE smallest, N infinite: refused, E is taken; with N finite and worse: open
    B.decision(B_RULE, "diagonal refused", "gate", 5.0, gate, 2, 0)
    B.decision(B_RULE, "diagonal open", "gate", 5.0, {**gate, 1: 3.5}, 2, 4)
    B.decision(B_RULE, "own cell", "own", 0.0, {0: 1.0}, 0)
    for name, v in (("NaN", NAN), ("-inf", -INF), ("+inf", INF)):
        B.decision(B_RULE, "candidate %s" % name, "bad candidate", v, {0: 1.0, 1: 1.0}, -1)
    # ---- field B_NONE: no route, at the first move and after four; values a real field never holds
    B.decision(B_NONE, "isolated", "no route", 2.0, {}, -1)
    B.decision(B_NONE, "best neighbour equal", "no route", 2.0, {0: 2.0}, -1)
    B.decision(B_NONE, "best neighbour above", "no route", 2.0, {0: 3.0, 5: 1.9}, -1)  # (NW 1.9 is lower, and closed)
    B.chain(B_NONE, "dead end after four moves", "no route later", [5.0, 4.5, 4.0, 3.5, 3.0], -1)
    B.chain(B_NONE, "equal after four moves", "no route later", [5.0, 4.5, 4.0, 3.5, 3.0, 3.0, 0.0], -1)
    B.chain(B_NONE, "NaN after four moves", "no route later", [5.0, 4.5, 4.0, 3.5, 3.0, NAN, 0.0], -1)
    # E is NaN (-inf): refused though no key is smaller, and NE and SE beside it are closed - N, finite and worse than both, is taken
    for name, v in (("NaN", NAN), ("-inf", -INF)):
        B.decision(B_NONE, "%s neighbour" % name, "bad neighbour", 5.0, {0: v, 4: 0.5, 7: 0.5, 1: 3.0, 3: 3.5, 2: 4.0}, 2, 1)
    B.chain(B_NONE, "below zero without a 0", "below zero", [1.0, 0.5, -0.25, -1.0], -1)
    B.chain(B_NONE, "ends on -0.0", "minus zero", [1.0, 0.5, -0.0], 2)
    B.chain(B_NONE, "a negative candidate", "below zero", [-0.5, -1.0, -1.5], -1)
    B.decision(B_NONE, "every neighbour -inf", "bad neighbour", 5.0, {k: -INF for k in range(8)}, -1)
    B.decision(B_NONE, "+inf beside a lower diagonal", "gate", 5.0, {0: INF, 4: 0.5, 1: 3.0, 3: 2.0}, 2, 3)
    B.again(B_NONE, "ends on -0.0, again", "minus zero", 9)
    assert B.gadgets[-1]["name"].startswith("ends on -0.0") and B.gadgets[-1]["n"] == 2
    # ---- the borders: a corridor along each, the four corners as candidates and as sources.  A neighbour index that is not
    # checked wraps: east of (59, j) lies (0, j + 1), south of row 0 the field before's row 59 - the other corridors wait there
    top = {(i, 59): 0.5 * (59 - i) for i in range(60)}
    B.place(B_TOP, "top border, corner to corner", "border", top, (0, 59), 59)
    bottom = {(i, 0): 0.5 * i for i in range(60)}
    B.place(B_BOTTOM, "bottom border, corner to corner", "border", bottom, (59, 0), 59)
    sides = {(0, j): 0.5 * (59 - j) for j in range(60)}
    sides.update({(59, j): 0.5 * j for j in range(60)})
    B.place(B_SIDES, "left border, corner to corner", "border", sides, (0, 0), 59)
    for r, cands in ((B_TOP, ((59, 59), (31, 59), (58, 59))), (B_BOTTOM, ((0, 0), (17, 0), (1, 0))), (B_SIDES, ((59, 59), (0, 59), (59, 0), (0, 30), (59, 29)))):
        for cand in cands:
            n = int(round(2 * B.cells[r][cand]))
            B.place(r, "border cell %s" % (cand,), "border", {}, cand, n)
    # ---- field B_COUNT: straight corridors of exact length n, the source in column 3
    for q, n in enumerate(CORRIDORS):
        j = 2 + 3 * q
        B.place(B_COUNT, "corridor of %d" % n, "count", {(3 + t, j): 0.5 * t for t in range(n + 1)}, (3 + n, j), n)
    # ---- field B_TURNS: all eight directions on one path; a diagonal move needs its two orthogonal cells finite - they are, and
    # so high that no walk enters them
    cells, moves = _turns_path()
    value, acc = {cells[0]: _f32(0.0)}, _f32(0.0)
    for cell, m in zip(cells[1:], moves):
        acc = _f32(acc + (ORTHO if m < 4 else DIAG))
        value[cell] = acc
    for (a, b), m in zip(cells[:-1], moves):
        if m >= 4:
            for q in ((a + NB[m][0], b), (a, b + NB[m][1])):
                value.setdefault(q, _f32(1000.0))
    B.place(B_TURNS, "all eight directions", "turns", value, cells[-1], len(moves))
    B.again(B_TURNS, "all eight directions, again", "turns", 0)
    for t in (1, 4, 7, 12, 15):
        B.place(B_TURNS, "the path's cell %d" % t, "turns", {}, cells[t], t)
    B.place(B_TURNS, "the gate cell east of the path's cell 3", "turns", {}, (34, 34), 4)  # (from 1000 down onto the path)
    # ---- field B_MIRROR: B_RULE's gadgets in the same places, its candidates in reverse order
    B.cells[B_MIRROR] = dict(B.cells[B_RULE])
    for g in [g for g in B.gadgets if g["r"] == B_RULE][::-1]:
        B.gadgets.append(dict(g, r=B_MIRROR, c=len(B.cands[B_MIRROR])))
        B.cands[B_MIRROR].append(g["cell"])
    return B


def candidates(B):
    """[R, K, 2] i32: the fields' candidates, a list that is not full filled up with cells outside the map"""
    out = np.zeros((R, K, 2), dtype=np.int32)
    for r in range(R):
        for c in range(K):
            out[r, c] = B.cands[r][c] if c < len(B.cands[r]) else (60 + c, -1 - r)
    return out


@pytest.fixture(scope="module")
def bank():
    return build()


# ---- what every gadget was built for ----------------------------------------------------------------------------------------------
def test_every_gadget_is_what_it_was_built_for(bank):
    fields = bank.fields()
    assert fields.shape == (R, 60, 60) and fields.dtype == np.float32
    kinds = {}
    for g in bank.gadgets:
        f = fields[g["r"]]
        path = igm.route_path_spec(f, g["cell"])
        n, way_cells, way_dir, trunc = igm.route_spec(f, g["cell"], 1)
        assert n == g["n"] and (path is None) == (n < 0), (g["name"], n)
        if g["first"] is not None:  # the neighbour taken is the single way-point, and the cell after the candidate's on the walk
            assert path[1][:2] == g["first"] and len(way_cells) == 1 and tuple(way_cells[0]) == g["first"], (g["name"], path)
        if n < 0:
            assert len(way_cells) == 0 and trunc is False
        kinds[g["kind"]] = kinds.get(g["kind"], 0) + 1
    print("walk gadgets by kind: %s (%d candidates)" % (kinds, len(bank.gadgets)))
    assert set(kinds) == {"equal", "tie", "gate", "own", "bad candidate", "no route", "no route later", "bad neighbour", "below zero",
                          "minus zero", "border", "count", "turns"}
    assert all(len(c) <= K for c in bank.cands) and len(bank.cands[B_RULE]) == K and len(bank.cands[B_COUNT]) == K == len(CORRIDORS)
    # the ties are ties: equal fp32 keys, unequal exact sums, in either order
    (d0, o0), (d1, o1) = _rounded_ties()
    assert _f32(d0 + DIAG) == _f32(o0 + ORTHO) and float(d0) + float(DIAG) < float(o0) + float(ORTHO)
    assert _f32(d1 + DIAG) == _f32(o1 + ORTHO) and float(d1) + float(DIAG) > float(o1) + float(ORTHO)
    assert _f32(_equal_key_diagonal() + DIAG) == _f32(_f32(1.0) + ORTHO)
    by = {g["name"]: g for g in bank.gadgets if g["r"] != B_MIRROR}
    f = fields[B_NONE]
    # "after four moves": four descending moves, then the end - at stride 1, 2 and 3 a way-point would have been due
    for name in ("dead end after four moves", "equal after four moves", "NaN after four moves"):
        i, j = by[name]["cell"]
        assert all(f[j, i - t - 1] < f[j, i - t] for t in range(4)) and not f[j, i - 5] < f[j, i - 4]
    i, j = by["ends on -0.0"]["cell"]
    assert f[j, i - 2] == 0 and np.signbit(f[j, i - 2])
    i, j = by["below zero without a 0"]["cell"]
    assert f[j, i - 1] > 0 > f[j, i - 2] and not (f == 0)[j, i - 3:i + 1].any()
    # the refused NaN / -inf neighbour would have been E, and the diagonals beside it hold the smallest keys
    for name in ("NaN neighbour", "-inf neighbour"):
        home = by[name]["cell"]
        e, ne, nn = (f[_nb(k, home)[1], _nb(k, home)[0]] for k in (0, 4, 1))
        assert not np.isfinite(e) and ne + DIAG < nn + ORTHO and by[name]["first"] == _nb(1, home)


def test_the_turns_path_is_walked_whole_and_shows_all_eight_directions(bank):
    f = bank.fields()[B_TURNS]
    cells, moves = _turns_path()
    assert sorted(set(moves)) == list(range(8))
    n, way_cells, way_dir, trunc = igm.route_spec(f, cells[-1], 1)
    assert n == len(moves) == 16 and not trunc and len(way_dir) == 15
    path = igm.route_path_spec(f, cells[-1])
    assert [p[:2] for p in path] == cells[::-1] and [p[2] ^ 2 for p in path[:-1]] == moves[::-1]
    assert sorted(set(way_dir.tolist())) == list(range(8))
    assert [tuple(c) for c in way_cells] == cells[1:16] and way_dir.tolist() == moves[:15]
    for d in range(8):  # the headings of the eight moves: the angle of the move itself
        assert abs(igm.route_heading(d) - math.atan2(NB[d][1], NB[d][0])) < 1e-15


def test_the_count_boundaries_flip_where_the_rule_says(bank):
    f = bank.fields()[B_COUNT]
    cand = {n: (3 + n, 2 + 3 * q) for q, n in enumerate(CORRIDORS)}
    assert max(CORRIDORS) == 52 and 0 in CORRIDORS
    spec = lambda n, s: igm.route_spec(f, cand[n], s)
    for s in (1, 2, 3):
        assert spec(17 * s, s)[3] is False and spec(17 * s + 1, s)[3] is True and len(spec(17 * s, s)[1]) == 16 == len(spec(17 * s + 1, s)[1])
        for k in (1, 16):  # n_way between k s and k s + 1
            assert len(spec(k * s, s)[1]) == k - 1 and len(spec(k * s + 1, s)[1]) == k, (s, k)
        if s > 1:
            assert spec(s - 1, s)[0] == s - 1 and len(spec(s - 1, s)[1]) == 0
    for s, n_way in ((51, 1), (52, 0), (53, 0), (3601, 0), (2 ** 31 - 1, 0)):
        got = spec(52, s)
        assert got[0] == 52 and len(got[1]) == n_way and got[3] is False
    assert tuple(spec(52, 51)[1][0]) == (3 + 51, cand[52][1]) and spec(52, 51)[2][0] == 0  # one move before the goal, driving east
    for n in CORRIDORS:  # every corridor at every stride: the way-points are the cells stride, 2 stride, .. from the source
        for s in STRIDES:
            got = spec(n, s)
            want = [t for t in range(s, n, s) if t <= 16 * s]
            assert got[0] == n and [int(c[0]) - 3 for c in got[1]] == want and got[3] == ((n - 1) // s > 16 if n else False)


# ---- the two copies of the neighbour rule --------------------------------------------------------------------------------------------
CTL = dict(dt=0.1, v_max=2.0, w_max=20.0, align_tol=np.pi / 4, goal_tol=0.01)


def _controller_cell(field, cell):
    """the cell goal_action_spec drives to from the centre of `cell`, its goal far away: a neighbour, None, or "goal" when it aims
    at the goal point itself"""
    goal = gw.centre(5, 5) if cell != (5, 5) else gw.centre(50, 50)
    _, _, aim, _ = igm.goal_action_spec(field, (*gw.centre(*cell), 0.3), goal, **CTL)
    return "goal" if aim == tuple(cell) else aim


def _compare(field, cells, routes):
    """On each cell: a route => its first move is the controller's cell; no route => the controller stands still, or its cell does
    not lie lower, or has no route itself.  Returns (compared, skipped)."""
    compared = skipped = 0
    for cell in cells:
        aim = _controller_cell(field, cell)
        if aim == "goal":
            skipped += 1
            continue
        path = routes(cell)
        own = field[cell[1], cell[0]]
        if path is not None:
            assert path[1][:2] == aim, (cell, path[:2], aim)
        else:
            assert aim is None or not field[aim[1], aim[0]] < own or routes(aim) is None, (cell, aim)
        compared += 1
    return compared, skipped


def test_the_walk_and_the_controller_choose_the_same_neighbour(bank):
    compared = skipped = 0
    for f in bank.fields():
        cells = [(int(i), int(j)) for j, i in np.argwhere(np.isfinite(f) & (f != 0))]
        memo = {}
        routes = lambda c, f=f, memo=memo: memo.setdefault(c, igm.route_path_spec(f, c))
        a, b = _compare(f, cells, routes)
        compared, skipped = compared + a, skipped + b
    on_gadgets = compared
    # the hand-made worlds: every third finite cell within 60 moves' worth of the source (a serpentine's far end is 1200 moves away)
    for rects, src in ((gw.serpentine(False), (0, 0)), (gw.staircase(missing=(7,)), (31, 30)), (gw.staircase(mirrored=True), (46, 14)),
                       (gw.sealed_pocket(), (21, 22)), (gw.open_map(), (59, 0))):
        f = igm.geodesic_spec(gw.edf_of(rects), gw.centre(*src), 0.5)[0]
        cells = [(int(i), int(j)) for j, i in np.argwhere(np.isfinite(f) & (f != 0) & (f < 30.0))][::3]
        memo = {}
        routes = lambda c, f=f, memo=memo: memo.setdefault(c, igm.route_path_spec(f, c))
        a, b = _compare(f, cells, routes)
        assert a >= 5  # (the pocket holds 16 cells)
        compared, skipped = compared + a, skipped + b
    print("neighbour rule: %d cells compared (%d on the gadget fields), %d skipped" % (compared, on_gadgets, skipped))
    assert on_gadgets > 800 and compared > 1500 and 10 * skipped < compared + skipped
