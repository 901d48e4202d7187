"""CPU: the identities behind the lane reductions of one linearProgram1 round (csrc/cagym_orca.h: orca_lp1_group, orca_lp_group).

A round projects the result onto line i: every lane clips the line against its own earlier half-planes, a DPP tree takes the
group's maximum of the left bounds and minimum of the right bounds, and the parameter t is clamped into [tl, tr].  Restated here in
numpy float32 (one rounding per operation, never fused, the device's operation order), lane by lane:

  two-stage   clip per lane, reduce, THEN combine with the chord of line i, and clamp t with two compares
              (t < tl ? tl : (t > tr ? tr : t)) - the round as it was;
  folded      the lane that owns line i feeds the chord into the reduction, t is clamped by min(max(t, tl), tr) - the round as it is;
  line index  the next violated line as the group's minimum of (v0 ? j : (v1 ? j + GW : BIG)) against find-first-set of the
              group's ballot mask.

Every round of every solve the oracle makes on the M = 10 and M = 20 pools of lp_worlds.build_pool is walked both ways (the
solves are re-walked through orca_lp_twin, whose result is the oracle's bit for bit), and the folded walk must give the twin's
failing line and the twin's result bits.

Signed zeros.  max and min of the values of a round are a total order but for +0 against -0.  The ISA reference of the vector
unit orders them (V_MAX_F32 / V_MIN_F32 name the +0 / -0 pair: the maximum is +0, the minimum -0), which makes the reductions
associative and commutative outright: whichever lane offers a bound, the group's bound is the same bits.  The clamp is another
matter - t = -0 against tl = +0 stays -0 with the two compares and becomes +0 with a maximum - and what the result's bits make of a
zero's sign hangs on the line's point (x + +0 == x + -0 bit for bit unless x is -0).  So every walk runs under three tie rules -
ORDERED (-0 < +0, the hardware's), FIRST and SECOND (equal operands: the first / the second one is returned) - and under every one
of them every round of the pools gives the same (rx, ry) bits both ways.  The pools do tie: a slow agent's half-plane tangent to
its own speed disc through the origin has the chord (-0, +0), and lattice worlds at rest have points at -0 (the count is printed;
3 rounds of the M = 20 pool).  Hand-made ties follow, held to the same."""
import functools
import math

import numpy as np
import pytest

import lp_worlds as lw
import orca_lp_twin as twin
from oracle import oracle as orc
from test_kernel_matrix import _n_worlds

scen = lw.scen
f32 = np.float32
NINF, PINF, ZERO = f32(-np.inf), f32(np.inf), f32(0.0)
EPS = f32(0.00001)
BIG = 1 << 20
RULES = ("ordered", "first", "second")
SHAPES = [(10, 8), (20, 16)]  # (M, lanes of an LP group): 9 lines on 8 lanes + the line beyond them; 19 lines on 16 lanes x 2 slots


def _bits(*v):
    return np.array(v, dtype=f32).view(np.uint32).tolist()


def _neg(a):
    return math.copysign(1.0, a) < 0


def _zero_tie(a, b):
    return a == b and a == 0 and _neg(a) != _neg(b)


def vmax(a, b, rule, ties=None):
    if a == b:
        if ties is not None and _zero_tie(a, b):
            ties.append(("max", float(a), float(b)))
        if rule == "ordered":
            return b if _neg(a) else a
        return a if rule == "first" else b
    return a if a > b else b


def vmin(a, b, rule, ties=None):
    if a == b:
        if ties is not None and _zero_tie(a, b):
            ties.append(("min", float(a), float(b)))
        if rule == "ordered":
            return a if _neg(a) else b
        return a if rule == "first" else b
    return a if a < b else b


@functools.lru_cache(maxsize=None)
def _perms(GW):
    j = np.arange(GW)
    p = []
    if GW >= 16:
        p.append(15 - j)                  # row_mirror
    if GW >= 8:
        p.append((j & 8) | (7 - (j & 7)))  # row_half_mirror
    p.append(j ^ 2)                       # quad_perm:[2,3,0,1]
    p.append(j ^ 1)                       # quad_perm:[1,0,3,2]
    return [q.tolist() for q in p]


def grp_reduce(v, op, GW, rule, ties=None):
    """the DPP tree: every level is one  v = op(v[partner], v)  on all lanes; -> the lanes' values (all the same but for a zero's sign)"""
    v = [float(x) for x in v]  # max and min only select: python floats compare faster, and every fp32 value (and its zero's sign) survives
    for p in _perms(GW):
        v = [op(v[p[j]], v[j], rule, ties) for j in range(GW)]
    return [f32(x) for x in v]


def chord(ln, radius):
    dot = ln[0] * ln[2] + ln[1] * ln[3]
    disc = dot * dot + radius * radius - (ln[0] * ln[0] + ln[1] * ln[1])
    if disc < 0:
        return PINF, NINF
    sq = np.sqrt(disc)
    return -dot - sq, -dot + sq


def clip_by(ln, m, ltl, ltr, rule, ties=None):
    den = ln[2] * m[3] - ln[3] * m[2]
    num = m[2] * (ln[1] - m[1]) - m[3] * (ln[0] - m[0])
    if abs(den) <= EPS:
        if num < 0:
            ltl = PINF
    else:
        t = num / den
        if den >= 0:
            ltr = vmin(ltr, t, rule, ties)
        else:
            ltl = vmax(ltl, t, rule, ties)
    return ltl, ltr


def _lane_clips(L, i, GW, rule, ties=None):
    """per lane: the bounds from its own lines before i (slot 0: line j, slot 1: line j + GW)"""
    out = []
    for j in range(GW):
        ltl, ltr = NINF, PINF
        for k in (j, j + GW):
            if k < i:
                ltl, ltr = clip_by(L[i], L[k], ltl, ltr, rule, ties)
        out.append((ltl, ltr))
    return out


def _finish(ln, tl, tr, ox, oy, dir_opt, clamp, rule, ties):
    if tl > tr:
        return None
    if dir_opt:
        t = tr if ox * ln[2] + oy * ln[3] > 0 else tl
    else:
        t = ln[2] * (ox - ln[0]) + ln[3] * (oy - ln[1])
        if clamp == "branches":
            if ties is not None and (_zero_tie(t, tl) or _zero_tie(t, tr)):
                ties.append(("clamp", float(t), float(tl), float(tr)))
            t = tl if t < tl else (tr if t > tr else t)
        else:
            t = vmin(vmax(t, tl, rule, ties), tr, rule, ties)
    return ln[0] + t * ln[2], ln[1] + t * ln[3]


def round_two_stage(L, i, radius, ox, oy, dir_opt, GW, rule, ties=None, lanes=None):
    c = chord(L[i], radius)
    lanes = _lane_clips(L, i, GW, rule, ties) if lanes is None else lanes
    tl = vmax(c[0], grp_reduce([a for a, _ in lanes], vmax, GW, rule, ties)[0], rule, ties)
    tr = vmin(c[1], grp_reduce([b for _, b in lanes], vmin, GW, rule, ties)[0], rule, ties)
    return _finish(L[i], tl, tr, ox, oy, dir_opt, "branches", rule, ties), (tl, tr, c, lanes)


def round_folded(L, i, radius, ox, oy, dir_opt, GW, rule, ties=None, lanes=None):
    """the owner lane of line i (lane i mod GW) offers the chord; the line beyond the lanes of a one-slot group (i == GW) computes
    its chord in the round and every lane offers it"""
    c = chord(L[i], radius)
    two = len(L) > GW + 1
    lanes = list(_lane_clips(L, i, GW, rule, ties) if lanes is None else lanes)
    for j in range(GW):
        if j == i % GW or (not two and i >= GW):
            lanes[j] = (vmax(lanes[j][0], c[0], rule, ties), vmin(lanes[j][1], c[1], rule, ties))
    tls = grp_reduce([a for a, _ in lanes], vmax, GW, rule, ties)
    trs = grp_reduce([b for _, b in lanes], vmin, GW, rule, ties)
    if rule == "ordered":  # group-uniform to the bit: the lanes of a group branch on these
        assert len({_bits(a)[0] for a in tls}) == 1 and len({_bits(b)[0] for b in trs}) == 1
    return _finish(L[i], tls[0], trs[0], ox, oy, dir_opt, "max-min", rule, ties)


def next_line(A, n, cur, rx, ry, GW):
    """A: the lines as an [n, 4] fp32 array -> (find-first-set of the group's mask, the group's minimum of the lanes' keys); n when
    no line is violated"""
    viol = A[:, 2] * (A[:, 1] - ry) - A[:, 3] * (A[:, 0] - rx) > 0
    viol[:cur] = False
    v = np.zeros(2 * GW, dtype=bool)
    v[:n] = viol
    mask = sum(1 << int(k) for k in np.nonzero(v)[0])
    keys = [j if v[j] else (j + GW if v[j + GW] else BIG) for j in range(GW)]
    ffs = (mask & -mask).bit_length() - 1 if mask else n
    for p in _perms(GW):  # v_min_u32 with a DPP source, level by level
        keys = [min(keys[p[j]], keys[j]) for j in range(GW)]
    assert len(set(keys)) == 1
    return ffs, (keys[0] if keys[0] != BIG else n)


class Counts(dict):
    def hit(self, k, n=1):
        self[k] = self.get(k, 0) + n


def walk_lp2(L, radius, ox, oy, dir_opt, GW, rule, counts, inner):
    """linearProgram2 by scan-and-jump with the folded round and the group-minimum line index -> (failing line or n, rx, ry)"""
    n = len(L)
    A = np.array(L, dtype=f32).reshape(n, 4)
    if dir_opt:
        rx, ry = ox * radius, oy * radius
    elif ox * ox + oy * oy > radius * radius:
        inv = f32(1.0) / np.sqrt(ox * ox + oy * oy)
        rx, ry = ox * inv * radius, oy * inv * radius
    else:
        rx, ry = ox, oy
    cur = 0
    while cur < n:
        ffs, i = next_line(A, n, cur, rx, ry, GW)
        assert ffs == i, ("line index", ffs, i)
        counts.hit("scans")
        if i == n:
            break
        ties = []
        clips = _lane_clips(L, i, GW, rule, ties)  # the same on both sides: each lane's own lines, in the lane's own order
        old, (tl, tr, c, lanes) = round_two_stage(L, i, radius, ox, oy, dir_opt, GW, rule, ties, clips)
        new = round_folded(L, i, radius, ox, oy, dir_opt, GW, rule, ties, clips)
        assert (old is None) == (new is None), ("feasibility", i)
        if old is not None:
            assert _bits(*old) == _bits(*new), ("round result", rule, i, old, new)
        counts.hit("zero_ties", len(ties))
        if rule == "ordered":
            counts.hit("rounds")
            counts.hit("inner_rounds", int(inner))
            counts.hit("ninth_line", int(n <= GW + 1 and i == GW))
            counts.hit("second_slot", int(n > GW + 1 and i >= GW))
            counts.hit("misses_disc", int(c[0] > c[1]))
            counts.hit("infeasible", int(old is None))
            if old is not None and i > 0:  # the chord's end is the bound although other lines clip on that side
                ctl, ctr = max(a for a, _ in lanes), min(b for _, b in lanes)
                counts.hit("chord_left_binds", int(ctl > NINF and c[0] >= ctl))
                counts.hit("chord_right_binds", int(ctr < PINF and c[1] <= ctr))
        if new is None:
            return i, rx, ry
        rx, ry = new
        cur = i + 1
    return n, rx, ry


def _spy(fn, log):
    def inner(L, radius, ox, oy, dir_opt, tr, index=None, mid=None):
        r = fn(L, radius, ox, oy, dir_opt, tr, index, mid)
        log.append((np.array(L, dtype=f32, copy=True), f32(radius), f32(ox), f32(oy), bool(dir_opt), index is not None, r))
        return r
    return inner


def _programs(M, N, monkeypatch):
    """every linearProgram2 call (outer programs and linearProgram3's inner ones) the twin makes on the pool's solves, with its
    result: the oracle runs the pool as lp_worlds.trace does"""
    pool, _ = lw.build_pool(M, N, False)
    log = []
    monkeypatch.setattr(twin, "_lp2", _spy(twin._lp2, log))
    env = orc.OracleEnv(N=N, M=M, max_obstacles=0, game_over_mode=1, rvo_max_neighbors=0)
    env.set_scenario(**pool)
    env.reset()
    a6, pol, coop = pool["agents6"], pool["policy_id"], pool["coop"]
    solves = 0
    for t in range(lw.T_STEPS):
        pos, vel, hd, done = env.f("pos").copy(), env.f("vel").copy(), env.f("heading").copy(), env.u("is_done").copy()
        for w in range(N):
            for i in np.nonzero((pol[w] == scen.POLICY_RVO) & (done[w] == 0))[0]:
                r = orc.orca_action_ex(pos[w], vel[w], a6[w, :, 2:4], a6[w, :, 4], a6[w, :, 5], int(i), float(hd[w, i]),
                                       float(coop[w, i]), max_neighbors=M, rects=None)
                g = a6[w, i, 2:4] - pos[w, i]
                pv = a6[w, i, 4] / np.hypot(*g) * g
                L = np.ascontiguousarray(r["lines"], dtype=f32).reshape(-1, 4)
                got = twin._solve(L, 0, f32(a6[w, i, 4]), f32(pv[0]), f32(pv[1]), twin._Trace())
                assert got.tobytes() == r["new_vel"].tobytes()
                solves += 1
        env.step()
    return log, solves


@pytest.mark.parametrize("M,GW", SHAPES)
def test_folded_round_and_line_index_equal_the_reference_on_the_lp_pools(M, GW, monkeypatch):
    N = _n_worlds(M, 4 if M == 10 else 2)
    log, solves = _programs(M, N, monkeypatch)
    total, tied = Counts(), 0
    for L, radius, ox, oy, dir_opt, inner, (fail, (rx, ry), _) in log:
        if not len(L):
            continue
        lines = [tuple(r) for r in L]
        for rule in RULES:
            counts = total if rule == "ordered" else Counts()
            before = counts.get("zero_ties", 0)
            with np.errstate(all="ignore"):
                k, qx, qy = walk_lp2(lines, radius, ox, oy, dir_opt, GW, rule, counts, inner)
            assert k == fail, (rule, "failing line", k, fail)
            assert _bits(qx, qy) == _bits(rx, ry), (rule, "result", (qx, qy), (rx, ry))
            # a walk that met no +0 / -0 pair never asked the tie rule anything: the other rules would repeat it operation for operation
            if rule == "ordered" and counts.get("zero_ties", 0) == before:
                break
            tied += int(rule == "ordered")
    print("programs walked under every tie rule (they meet a +0 / -0 pair):", tied)
    print("M = %d, groups of %d lanes: %d solves, %d programs; %s" % (M, GW, solves, len(log), dict(total)))
    need = ["rounds", "chord_left_binds", "chord_right_binds", "infeasible", "misses_disc", "inner_rounds"]
    need += ["ninth_line"] if M == 10 else ["second_slot"]
    for k in need:
        assert total.get(k, 0) > 0, (k, total)


def _tie_rounds():
    """hand-made rounds with a +0 / -0 tie at the deciding bound: line i through the origin along +x or -x, preferred velocity on
    the line's normal (t = +-0), an earlier line that cuts it exactly at the origin (clip t = +-0), radius 1 (chord -1 .. 1)"""
    out = []
    for sx in (1.0, -1.0):
        for oy in (0.5, -0.5):
            for cut in ((0.0, 1.0), (0.0, -1.0), (1.0, 1.0), (-1.0, 1.0)):
                for px in (0.0, 0.25):
                    n = np.hypot(*cut)
                    L = [(0.0, 0.0, cut[0] / n, cut[1] / n), (px, 0.0, sx, 0.0)]
                    out.append(([tuple(f32(v) for v in r) for r in L], f32(-px if sx > 0 else px) * f32(1.0), f32(oy)))
    return out


def test_signed_zero_ties_give_the_same_result_under_every_tie_rule():
    seen = 0
    for L, ox, oy in _tie_rounds():
        got = set()
        for rule in RULES:
            ties = []
            with np.errstate(all="ignore"):
                old, _ = round_two_stage(L, 1, f32(1.0), ox, oy, False, 8, rule, ties)
                new = round_folded(L, 1, f32(1.0), ox, oy, False, 8, rule, ties)
            seen += len(ties)
            assert (old is None) == (new is None)
            if old is not None:
                got.add(tuple(_bits(*old)))
                got.add(tuple(_bits(*new)))
        assert len(got) <= 1, (L, ox, oy, got)
    assert seen > 0  # the scenes do tie


def test_max_then_min_is_the_two_compare_clamp():
    """t < tl ? tl : (t > tr ? tr : t) == min(max(t, tl), tr) for tl <= tr, bit for bit, wherever t does not meet a bound that is
    the zero of the other sign"""
    rng = np.random.default_rng(9)
    vals = np.concatenate([rng.normal(size=64).astype(f32), [f32(0.0), f32(-0.0), f32(1.0), f32(-1.0), PINF, NINF]])
    n = 0
    for t in vals:
        for tl in vals[::3]:
            for tr in vals[::5]:
                if tl > tr or tl == PINF or tr == NINF or _zero_tie(t, tl) or _zero_tie(t, tr):
                    continue
                want = tl if t < tl else (tr if t > tr else t)
                for rule in RULES:
                    assert _bits(vmin(vmax(t, tl, rule), tr, rule)) == _bits(want), (t, tl, tr, rule)
                n += 1
    assert n > 1000
