"""An fp32 numpy restatement of RVO2's linearProgram1 / 2 / 3 (the algorithm oracle/cagym_oracle.c states as lp1 / lp2 / lp3)
that also says WHICH branches a solve took and how close any of its decisions came to going the other way.

The restatement rounds every intermediate to fp32 in the oracle's operation order (numpy float32 elementwise arithmetic is
IEEE, one rounding per operation, never fused), so its result equals the oracle's new_vel bit for bit
(tests/test_orca_lp_twin.py).  It works on the half-planes orca_action_ex returns (`lines`, `n_obst_lines`): the construction of
the lines is not restated.

classify(lines, n_obst, radius, pref_vel) -> (new_vel, counters, margin)

counters (collections.Counter):
  lp2_rounds                 lines linearProgram2 projected onto (the solve's outer program only)
  lp3_solves                 1 if linearProgram2 failed
  lp3_outer / lp3_inner      rounds of linearProgram3 / lines its inner programs projected onto
  lp3_outer_2inner           outer rounds whose inner program projected onto at least two lines
  lp1_parallel_inside        |den| <= RVO_EPS and num >= 0: the line is skipped
  lp1_parallel_outside       |den| <= RVO_EPS and num <  0: infeasible
  lp1_disc_negative_original / lp1_disc_negative_projected     the line misses the disc
  lp3_parallel_opposite      |d| <= RVO_EPS, opposite directions: the projected line passes through the midpoint
  lp3_parallel_same          |d| <= RVO_EPS, same direction: no projected line
  lp3_inner_failed           the inner program failed and the result was restored
  lp3_with_obstacle_lines    linearProgram3 ran with protected obstacle lines in front
  neighbour_distance_ties    equal fp32 squared distances among the ego's kept neighbours (and the first one cut off),
                             counted from the positions when the caller passes them
  max_lp2_line / max_lp3_outer_line / max_lp3_inner_line       largest LINE INDEX (in `lines`) of a linearProgram2 round, an
                             outer round, an inner round (-1: none): whether the second slot of an LP lane (i >= GW) and the line
                             beyond the lanes (i == GW) were reached
  lp2_line:<i> / lp3_outer_line:<i>                            the same rounds counted per line index
  and, as attributes of the returned Counter: raw_margin / raw_what (below), what (the decision that set the margin).

The comparisons of a solve, each with its distance from the threshold in its own unit:
  det > 0 (linearProgram2) and det > distance (linearProgram3); disc < 0; tl > tr after every clip; num < 0 of a parallel line;
  the sign of den (|den| of a non-parallel line); dot > 0 of the direction-optimising program (*); dot > 0 between parallel lines;
  the parallel test itself: safe when |den| <= 1e-6 (exactly parallel in practice) or |den| >= 2e-5, distance 0 in between.
  min(tr, t), max(tl, t), the clamp of t to [tl, tr] and the clamp of the preferred velocity to the disc give the same value on
  either side of the threshold: they select no branch and are left out.
  (*) except on a projected line of the midpoint branch.  linearProgram3 optimises along (-d_i.y, d_i.x) and that line runs along
  normalize(d_j - d_i): their dot product is det(d_i, d_j) / |d_j - d_i|, the very determinant the parallel test found to be zero
  in practice.  RVO2 picks an end of that line by the sign of a rounding residue (often an exact 0: the left end); there is no
  distance to measure, and "safe" means what it means for the parallel test: the same fp32 operations on the same operands.
  Such a solve pins exactly that - the device must form the residue as the oracle does.

raw_margin is the smallest of these distances.  margin - what lp_worlds rejects on - is the smallest among the comparisons that
DECIDE something.  Most do not: the optimum of a feasible linear program, and the least-penetration point of an infeasible one,
move continuously with the half-planes, and the incremental algorithm reaches that optimum whichever way a comparison at its
threshold goes (a line violated by 1e-5 is projected onto and moves the result by about 1e-5; a chord with tl - tr = 1e-6 sends
the solve to linearProgram3, which returns a point 1e-6 away).  In a crowd such harmless near-misses are the rule - one solve of
20 agents makes some 50 comparisons, a 12-step world of them 10 000 - while a comparison that picks between two distant answers
(an end of a line the objective is constant along, parallel or not, kept or restored) is rare.  So every comparison nearer than
TIE_MARGIN is put to the test: the solve is repeated with that one comparison forced the other way, and it counts as a decision
when the result moves by more than max(FLIP_FLOOR, FLIP_GAIN * distance) - more than a continuous dependence with a gain of 100
explains, FLIP_FLOOR = 2e-7 being the tolerance of the device tests on an action.  A solve with more than MAX_FLIPS such
comparisons is not examined further: margin 0.
A solve whose margin is below TIE_MARGIN may legitimately go the other way on another libm: see tests/lp_worlds.py."""
from collections import Counter

import numpy as np

f32 = np.float32
RVO_EPS = f32(0.00001)
TIE_MARGIN = 1e-4
PARALLEL_SAFE_BELOW, PARALLEL_SAFE_ABOVE = 1e-6, 2e-5
FLIP_FLOOR, FLIP_GAIN, MAX_FLIPS = 2e-7, 100.0, 16
INF = float("inf")


class _Trace(object):
    def __init__(self, flip_at=None):
        self.c = Counter()
        self.raw, self.raw_what = INF, None
        self.hard, self.hard_what = INF, None  # comparisons that are never put to the flip test (the parallel test)
        self.near, self.n_near, self.flip_at = [], 0, flip_at
        self.max = {"max_lp2_line": -1, "max_lp3_outer_line": -1, "max_lp3_inner_line": -1}

    def far(self, x, what):
        """comparisons known to be at least TIE_MARGIN from their threshold, or the smallest of a batch of them"""
        x = float(x)
        if x < self.raw:
            self.raw, self.raw_what = x, what

    def cmp(self, cond, x, what):
        """the outcome of a comparison at distance x from its threshold; the flip_at-th near one is forced the other way"""
        x = float(x)
        self.far(x, what)
        if x < TIE_MARGIN:
            k = self.n_near
            self.n_near += 1
            if self.flip_at is None:
                self.near.append((k, x, what))
            elif k == self.flip_at:
                return not cond
        return bool(cond)

    def parallel_test(self, a):
        if PARALLEL_SAFE_BELOW < float(a) < PARALLEL_SAFE_ABOVE:
            self.raw, self.raw_what = 0.0, "parallel test"
            self.hard, self.hard_what = 0.0, "parallel test"

    def top(self, key, i):
        if i > self.max[key]:
            self.max[key] = int(i)


def _lp1(L, no, radius, ox, oy, dir_opt, tr, projected, midpoint=False):
    px, py, dx, dy = L[no]
    dot = px * dx + py * dy
    disc = dot * dot + radius * radius - (px * px + py * py)
    if tr.cmp(disc < 0, abs(disc), "disc < 0"):
        tr.c["lp1_disc_negative_projected" if projected else "lp1_disc_negative_original"] += 1
        return None
    with np.errstate(all="ignore"):
        sq = np.sqrt(disc) if disc >= 0 else f32(0.0)  # disc < 0 only when the comparison above was forced
    tl, tr_ = -dot - sq, -dot + sq
    if no:
        P = L[:no]
        den = dx * P[:, 3] - dy * P[:, 2]
        num = P[:, 2] * (py - P[:, 1]) - P[:, 3] * (px - P[:, 0])
        with np.errstate(all="ignore"):
            t = num / den
        aden = np.abs(den)
        for i in range(no):
            tr.parallel_test(aden[i])
            if aden[i] <= RVO_EPS:
                if tr.cmp(num[i] < 0, abs(num[i]), "num < 0 of a parallel line"):
                    tr.c["lp1_parallel_outside"] += 1
                    return None
                tr.c["lp1_parallel_inside"] += 1
                continue
            if tr.cmp(den[i] >= 0, aden[i], "sign of den"):
                tr_ = tr_ if tr_ < t[i] else t[i]
            else:
                tl = tl if tl > t[i] else t[i]
            if tr.cmp(tl > tr_, abs(float(tl) - float(tr_)), "tl > tr"):
                return None
    if dir_opt:
        d = ox * dx + oy * dy
        t = tr_ if (d > 0 if midpoint else tr.cmp(d > 0, abs(d), "dot > 0 (dir_opt)")) else tl
    else:
        t = dx * (ox - px) + dy * (oy - py)
        if t < tl:
            t = tl
        elif t > tr_:
            t = tr_
    return px + t * dx, py + t * dy


def _lp2(L, radius, ox, oy, dir_opt, tr, index=None, mid=None):
    """index None: the solve's own program; else the inner program of linearProgram3, index[k] = the line of `lines` that
    row k of L was projected from (-1: an obstacle line), mid[k]: row k came from the midpoint branch"""
    n = len(L)
    if dir_opt:
        rx, ry = ox * radius, oy * radius
    elif ox * ox + oy * oy > radius * radius:
        inv = f32(1.0) / np.sqrt(ox * ox + oy * oy)
        rx, ry = ox * inv * radius, oy * inv * radius
    else:
        rx, ry = ox, oy
    i = rounds = 0
    while i < n:
        R = L[i:]
        det = R[:, 2] * (R[:, 1] - ry) - R[:, 3] * (R[:, 0] - rx)
        viol, adet = det > 0, np.abs(det)
        for e in np.nonzero(adet < TIE_MARGIN)[0]:  # the scan stops at the first violated line: only those before it compare
            if viol[:e].any():
                break
            viol[e] = tr.cmp(viol[e], adet[e], "det > 0")
        hit = np.nonzero(viol)[0]
        k = int(hit[0]) if len(hit) else len(R) - 1
        tr.far(adet[:k + 1][adet[:k + 1] >= TIE_MARGIN].min(initial=INF), "det > 0")
        if not len(hit):
            break
        j = i + k
        rounds += 1
        if index is None:
            tr.c["lp2_rounds"] += 1
            tr.top("max_lp2_line", j)
            tr.c["lp2_line:%d" % j] += 1
        else:
            tr.c["lp3_inner"] += 1
            tr.top("max_lp3_inner_line", index[j])
        r = _lp1(L, j, radius, ox, oy, dir_opt, tr, index is not None, mid is not None and bool(mid[j]))
        if r is None:
            return j, (rx, ry), rounds
        rx, ry = r
        i = j + 1
    return n, (rx, ry), rounds


def _lp3(L, nob, begin, radius, r, tr):
    rx, ry = r
    dist = f32(0.0)
    n = len(L)
    for i in range(begin, n):
        px, py, dx, dy = L[i]
        det = dx * (py - ry) - dy * (px - rx)
        if not tr.cmp(det > dist, abs(float(det) - float(dist)), "det > distance"):
            continue
        tr.c["lp3_outer"] += 1
        tr.top("max_lp3_outer_line", i)
        tr.c["lp3_outer_line:%d" % i] += 1
        J = L[nob:i]
        with np.errstate(all="ignore"):
            d = dx * J[:, 3] - dy * J[:, 2]
            par = np.abs(d) <= RVO_EPS
            same = par & (dx * J[:, 2] + dy * J[:, 3] > 0)
            s = (J[:, 2] * (py - J[:, 1]) - J[:, 3] * (px - J[:, 0])) / d
            qx = np.where(par, f32(0.5) * (px + J[:, 0]), px + s * dx)
            qy = np.where(par, f32(0.5) * (py + J[:, 1]), py + s * dy)
            ddx, ddy = J[:, 2] - dx, J[:, 3] - dy
            inv = f32(1.0) / np.sqrt(ddx * ddx + ddy * ddy)
            proj = np.stack([qx, qy, ddx * inv, ddy * inv], 1)
        for a in np.abs(d):
            tr.parallel_test(a)
        if par.any():  # unit directions: +-1
            tr.far(np.abs(dx * J[par, 2] + dy * J[par, 3]).min(), "dot > 0 of parallel lines")
        tr.c["lp3_parallel_same"] += int(same.sum())
        tr.c["lp3_parallel_opposite"] += int((par & ~same).sum())
        P = np.concatenate([L[:nob], proj[~same]]).astype(f32)
        index = np.concatenate([np.full(nob, -1), nob + np.nonzero(~same)[0]])
        mid = np.concatenate([np.zeros(nob, dtype=bool), par[~same]])
        k, q, rounds = _lp2(P, radius, -dy, dx, True, tr, index, mid)
        if rounds >= 2:
            tr.c["lp3_outer_2inner"] += 1
        if k < len(P):
            tr.c["lp3_inner_failed"] += 1
        else:
            rx, ry = q
        dist = dx * (py - ry) - dy * (px - rx)
    return rx, ry


def _solve(L, n_obst, radius, pvx, pvy, tr):
    fail, r, _ = _lp2(L, radius, pvx, pvy, False, tr)
    if fail < len(L):
        tr.c["lp3_solves"] += 1
        if n_obst:
            tr.c["lp3_with_obstacle_lines"] += 1
        r = _lp3(L, n_obst, fail, radius, r, tr)
    return np.array(r, dtype=f32)


def kept_neighbours(pos, ego, max_neighbors):
    """RVO2's insertAgentNeighbor on fp32 positions: (indices nearest first, their fp32 squared distances, the squared distance of
    the nearest neighbour that was cut off or None).  Strict < on insertion = a stable sort by distance."""
    p = np.asarray(pos, dtype=np.float64).astype(f32)
    others = np.array([a for a in range(len(p)) if a != ego], dtype=np.int64)
    if not len(others):
        return others, np.zeros(0, dtype=f32), None
    dx, dy = p[ego, 0] - p[others, 0], p[ego, 1] - p[others, 1]
    dsq = dx * dx + dy * dy
    order = np.argsort(dsq, kind="stable")
    keep = order[:max_neighbors]
    cut = dsq[order[max_neighbors]] if len(order) > max_neighbors else None
    return others[keep], dsq[keep], cut


def classify(lines, n_obst, radius, pref_vel, pos=None, ego=None, max_neighbors=None):
    """-> (new_vel float32[2], counters, margin); pos [n, 2], ego, max_neighbors: count neighbour_distance_ties too."""
    L = np.ascontiguousarray(lines, dtype=f32).reshape(-1, 4)
    radius, pvx, pvy, n_obst = f32(radius), f32(pref_vel[0]), f32(pref_vel[1]), int(n_obst)
    tr = _Trace()
    res = _solve(L, n_obst, radius, pvx, pvy, tr)
    margin, what = tr.hard, tr.hard_what
    if len(tr.near) > MAX_FLIPS:
        margin, what = 0.0, "more than %d comparisons near their thresholds" % MAX_FLIPS
    else:
        for k, x, w in tr.near:
            if x >= margin:
                continue
            other = _solve(L, n_obst, radius, pvx, pvy, _Trace(flip_at=k))
            move = np.abs(other.astype(np.float64) - res.astype(np.float64)).max()
            if not move <= max(FLIP_FLOOR, FLIP_GAIN * x):
                margin, what = x, w
    if pos is not None:
        _, dsq, cut = kept_neighbours(pos, ego, len(pos) if max_neighbors is None else max_neighbors)
        seq = list(dsq) + ([cut] if cut is not None else [])
        tr.c["neighbour_distance_ties"] += sum(1 for a, b in zip(seq, seq[1:]) if a == b)
    tr.c.update(tr.max)  # a Counter: absent keys read 0; merge() below takes the max of the max_* keys
    tr.c.what, tr.c.raw_margin, tr.c.raw_what = what, tr.raw, tr.raw_what
    return res, tr.c, margin


def merge(total, c):
    """add the counters of one solve to a running total (sums; the largest of the max_* line indices)"""
    for k, v in c.items():
        total[k] = max(total.get(k, -1), v) if k.startswith("max_") else total.get(k, 0) + v
    return total
