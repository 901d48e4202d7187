// cagym_ig_geodesic.h -- goal actions for the learner's robots (include/cagym.h: cagym_ig_geodesic, cagym_ig_goal_actions,
// cagym_ig_goal_status): a policy that chooses a PLACE - a world point, or a cell of the belief window it is handed - instead of a
// (v, omega) per step, and underneath it the obstacle-aware shortest-path distance to that place on the belief grid and a controller
// that descends it.
//
// k_ig_geodesic: one workgroup of 256 threads per (world, robot); a workgroup whose mask byte is 0 leaves before its first barrier
// and touches nothing.  The field is the fixed point of the min-plus relaxation on the 60 x 60 grid of 0.5 m cells
//   field[source] = 0,  field[c] = min over allowed neighbours u of fl32(field[u] + cost),  blocked and unreached cells +inf
// with cost 0.5f for an orthogonal move and (float)(0.5 sqrt 2) for a diagonal one, a cell free when the distance field at its
// centre passes the planners' test EDF > radius + 0.1 (the source cell always), and a diagonal move allowed only between two free
// orthogonal cells.  fp32 addition is monotone and every cost is positive, so the fixed point is unique and the order of relaxation
// does not matter: it equals a Dijkstra run with the same additions bit for bit (ig.geodesic_spec).
//
// State lives in LDS: a 62 x 62 f32 tile with an infinite halo (15376 B) and the free mask as 62 words (bit i + 1 of word j + 1 <=>
// cell (i, j) free: the halo's bits are 0).  Thread t < 240 owns a strip: column t % 60, rows 15 (t / 60) .. + 14.  The strip's values,
// which of its cells are free and which of their diagonals are allowed stay in registers for all sweeps; a sweep reads the two
// neighbour columns and the two cells beyond the strip's ends from LDS (36 reads for 15 cells) and stores only what changed.  A sweep
// relaxes every cell IN PLACE: a neighbour's value is the one of this sweep or of the last, either is the length of a real path, and
// values only fall.  A sweep in which no thread stored anything read nothing but final values - that is the fixed point, found by a
// workgroup-wide OR (__syncthreads_or, which is also the barrier between two sweeps).  The loop is capped at 3600 trips (no chain is
// longer than the number of cells).  No global atomics, no waits: barriers only.
//
// k_ig_goal_actions / k_ig_goal_status: one wave per world, lane = agent slot, one lane per robot (ig_robot_rank gives its rank).
#pragma once
#include "cagym_ig.h"

#define IGG_TW 62                 // tile width: 60 cells and a halo of one on either side
#define IGG_SWEEP_CAP 3600
#define IGG_ORTHO 0.5f
#define IGG_DIAG ((float)(0.5 * 1.4142135623730951))  // (float)(0.5 * sqrt(2.0)), the double product rounded once

struct IgGoalParams {
    int R, G, rotate;
    double radius, v_max, w_max, align_tol, goal_tol, dt;
};

__global__ void __launch_bounds__(256) k_ig_geodesic(CagymDev D, IgDev G, IgGoalParams P, const uint8_t* __restrict__ mask,
                                                     const double* __restrict__ goals_xy, const int32_t* __restrict__ goals_ab,
                                                     float* field, double* goal_xy, uint8_t* active, int32_t* sweeps) {
    __shared__ float tile[IGG_TW * IGG_TW];
    __shared__ unsigned long long fm[IGG_TW];
    __shared__ int s_src[3];  // source cell (i, j), and whether there is one
    const int wr = blockIdx.x, w = wr / P.R, r = wr - w * P.R, tid = threadIdx.x;
    if (mask && !mask[wr]) return;  // not flagged: nothing of this robot is read or written

    // 1. the source point (wave 0; every lane the same values, lane = slot only for the ballot that finds the robots)
    if (tid < 64) {
        double x, y;
        if (goals_xy) {
            x = goals_xy[2 * (size_t)wr];
            y = goals_xy[2 * (size_t)wr + 1];
        } else {  // a cell (a, b) of the robot's belief window: ig_window_point on the pose as it is now
            unsigned long long robots;
            ig_robot_slot(D, w, tid, robots);
            const int slot = ig_nth_robot(robots, r);  // wave-uniform
            x = y = ig_nan_d();                        // (a world without that robot: no source)
            if (slot >= 0) {
                const size_t a = (size_t)w * D.M + slot;
                double sn, cs;
                ig_window_sincos(P.rotate, D.heading[a], sn, cs);
                ig_window_point(D.px[a], D.py[a], sn, cs, (double)(P.G / 2), goals_ab[2 * (size_t)wr], goals_ab[2 * (size_t)wr + 1], x, y);
            }
        }
        if (tid == 0) {
            const int si = ig_bel_cell(x), sj = ig_bel_cell(y);
            const bool ok = isfinite(x) && isfinite(y) && si >= 0 && si < IG_BEL && sj >= 0 && sj < IG_BEL;
            s_src[0] = si;
            s_src[1] = sj;
            s_src[2] = ok ? 1 : 0;
            goal_xy[2 * (size_t)wr] = x;
            goal_xy[2 * (size_t)wr + 1] = y;
            active[wr] = ok ? 1 : 0;
        }
    }
    const float inf = ig_inf_f();
    for (int q = tid; q < IGG_TW * IGG_TW; q += blockDim.x) tile[q] = inf;
    for (int q = tid; q < IGG_TW; q += blockDim.x) fm[q] = 0ull;
    __syncthreads();
    const int si = s_src[0], sj = s_src[1];
    float* out = field + (size_t)wr * IG_BEL * IG_BEL;
    if (!s_src[2]) {  // uniform: no source cell, nothing is reachable
        for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) out[q] = inf;
        if (sweeps && tid == 0) sweeps[wr] = 0;
        return;
    }

    // 2. the free mask: the raster cell in the middle of every belief cell (the value edf_at returns for the cell centre)
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double need = P.radius + 0.1;
    for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {
        const int j = q / IG_BEL, i = q - j * IG_BEL;
        const double edf = sqrt((double)d2[(5 * j + 2) * CAGYM_MAPD + 5 * i + 2]) * IG_EDF_CELL;
        if (edf > need || (i == si && j == sj)) atomicOr(&fm[j + 1], 1ull << (i + 1));  // (an LDS atomic)
    }
    if (tid == 0) tile[(sj + 1) * IGG_TW + si + 1] = 0.f;
    __syncthreads();

    // 3. this thread's cells: rows j0 .. j0 + 14 of column i; bit k of `fr`: cell k is free and not the source, bits 4 k .. 4 k + 3 of
    //    `dg`: its NE, NW, SW, SE diagonals pass between two free cells.  Their values stay in registers for all sweeps.
    const bool worker = tid < 240;
    const int i = tid % IG_BEL, j0 = 15 * (tid / IG_BEL);
    const int c0 = (j0 + 1) * IGG_TW + i + 1;
    unsigned int fr = 0u;
    unsigned long long dg = 0ull;
    float v[15];
    if (worker) {
#pragma unroll
        for (int k = 0; k < 15; k++) {
            const int j = j0 + k;
            const unsigned long long dn = fm[j] >> i, md = fm[j + 1] >> i, up = fm[j + 2] >> i;  // bit 0: column i - 1, 1: i, 2: i + 1
            const bool e = (md >> 2) & 1ull, wv = md & 1ull, n = (up >> 1) & 1ull, s = (dn >> 1) & 1ull;
            if (((md >> 1) & 1ull) && !(i == si && j == sj)) fr |= 1u << k;
            const unsigned long long four = (e && n ? 1ull : 0ull) | (wv && n ? 2ull : 0ull) | (wv && s ? 4ull : 0ull) | (e && s ? 8ull : 0ull);
            dg |= four << (4 * k);
            v[k] = tile[c0 + IGG_TW * k];  // +inf, or 0 in the source cell
        }
    }

    // 4. sweeps to the fixed point: the two neighbour columns and the two cells beyond the strip's ends come from LDS once per
    //    sweep (36 reads for 15 cells), the strip is relaxed upwards in registers, each cell on the new value of the one below
    int trips = 0;
    for (; trips < IGG_SWEEP_CAP; trips++) {
        int changed = 0;
        if (worker) {
            float ce[17], cw[17];  // rows j0 - 1 .. j0 + 15 of columns i + 1 and i - 1
#pragma unroll
            for (int k = 0; k < 17; k++) {
                ce[k] = tile[c0 + IGG_TW * (k - 1) + 1];
                cw[k] = tile[c0 + IGG_TW * (k - 1) - 1];
            }
            const float below = tile[c0 - IGG_TW], above = tile[c0 + IGG_TW * 15];
#pragma unroll
            for (int k = 0; k < 15; k++) {
                // (straight-line: a blocked cell's result is dropped by the test below)
                const float s = k == 0 ? below : v[k - 1], n = k == 14 ? above : v[k + 1];
                const float o = fminf(fminf(ce[k + 1], cw[k + 1]), fminf(n, s)) + IGG_ORTHO;
                const unsigned int four = (unsigned int)(dg >> (4 * k)) & 15u;
                const float d = fminf(fminf((four & 1u) ? ce[k + 2] : inf, (four & 2u) ? cw[k + 2] : inf),
                                      fminf((four & 4u) ? cw[k] : inf, (four & 8u) ? ce[k] : inf));
                const float nv = fminf(o, d + IGG_DIAG);
                if (((fr >> k) & 1u) && nv < v[k]) {
                    v[k] = nv;
                    tile[c0 + IGG_TW * k] = nv;
                    changed = 1;
                }
            }
        }
        if (!__syncthreads_or(changed)) break;  // (the barrier between two sweeps; after the last one every value is in place)
    }
    if (sweeps && tid == 0) sweeps[wr] = trips + 1;  // sweeps run, the confirming one included

    // 5. the field row, [j, i]
    for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {
        const int j = q / IG_BEL, ii = q - j * IG_BEL;
        out[q] = tile[(j + 1) * IGG_TW + ii + 1];
    }
}

// The controller's atan2 for finite operands: fdlibm's (e_atan2.c / s_atan.c, public domain constants) written out as separate fp64
// sums, products and quotients in a fixed order - this file is compiled without contraction - so that ig.atan2_spec, the same
// statements in Python, returns the same double bit for bit.  The heading error of an aligned robot is a difference of two nearly
// equal angles: against a specification whose atan2 differs in the last bit the turn rate would be off by its whole size there.
__device__ __forceinline__ double igg_atan_pos(double x) {
    const double hi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double lo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    if (x >= 73786976294838206464.0) return hi[3] + lo[3];  // 2^66
    double h = 0.0, l = 0.0;
    bool small = false;
    if (x < 0.4375) {
        if (x < 1.862645149230957e-09) return x;  // 2^-29
        small = true;
    } else if (x < 1.1875) {
        if (x < 0.6875) { h = hi[0]; l = lo[0]; x = (2.0 * x - 1.0) / (2.0 + x); }
        else { h = hi[1]; l = lo[1]; x = (x - 1.0) / (x + 1.0); }
    } else if (x < 2.4375) { h = hi[2]; l = lo[2]; x = (x - 1.5) / (1.0 + 1.5 * x); }
    else { h = hi[3]; l = lo[3]; x = -1.0 / x; }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 +
                      w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 +
                      w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (small) return x - x * (s1 + s2);
    return h - ((x * (s1 + s2) - l) - x);
}

__device__ __forceinline__ double igg_atan2(double y, double x) {
    const double pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16, pio2 = 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
    const int m = (signbit(y) ? 1 : 0) + (signbit(x) ? 2 : 0);
    if (y == 0.0) return m < 2 ? y : (m == 2 ? pi : -pi);
    if (x == 0.0) return (m & 1) ? -pio2 : pio2;
    const double z = igg_atan_pos(fabs(y / x));
    return m == 0 ? z : m == 1 ? -z : m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi;
}

// (a + pi) mod 2 pi - pi with a non-negative modulo: the reference's wrap, as Python's % computes it
__device__ __forceinline__ double igg_wrap(double a) {
    double m = fmod(a + kPi, 2 * kPi);
    if (m < 0.0) m += 2 * kPi;
    return m - kPi;
}

__device__ __forceinline__ float igg_at(const float* f, int i, int j) {
    return (i >= 0 && i < IG_BEL && j >= 0 && j < IG_BEL) ? f[j * IG_BEL + i] : ig_inf_f();
}

// The controller (ig.goal_action_spec): for every robot with an active goal its row of the action table [N*M, 2] f32; every other
// row stays the caller's.  All pose arithmetic in fp64, separate products and sums in the order written.
__global__ void __launch_bounds__(64) k_ig_goal_actions(CagymDev D, IgGoalParams P, const float* __restrict__ field,
                                                        const double* __restrict__ goal_xy, const uint8_t* __restrict__ active,
                                                        float* actions, uint8_t* choice) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int rank = ig_robot_rank(D, w, lane, P.R);
    if (rank < 0) return;
    const size_t wr = (size_t)w * P.R + rank, a = (size_t)w * D.M + lane;
    if (!active[wr]) {
        if (choice) choice[wr] = 255;
        return;
    }
    const float* f = field + wr * IG_BEL * IG_BEL;
    const double x = D.px[a], y = D.py[a], th = D.heading[a];
    const double gx = goal_xy[2 * wr], gy = goal_xy[2 * wr + 1];
    const int ci = ig_bel_cell(x), cj = ig_bel_cell(y);
    const double dx = gx - x, dy = gy - y;
    const double dist = sqrt(dx * dx + dy * dy);
    double v = 0.0, om = 0.0;
    bool go = ci >= 0 && ci < IG_BEL && cj >= 0 && cj < IG_BEL && !(dist <= P.goal_tol);
    double ax = gx, ay = gy;
    int pick = go ? 8 : 255;  // what the robot aims at: 0..7 the neighbour in candidate order, 8 the goal point, 255 nothing
    const bool to_goal = ci == ig_bel_cell(gx) && cj == ig_bel_cell(gy);
    if (go && !to_goal) {
        const float inf = ig_inf_f();
        const bool own = f[cj * IG_BEL + ci] < inf;
        const float e = igg_at(f, ci + 1, cj), n = igg_at(f, ci, cj + 1), wv = igg_at(f, ci - 1, cj), s = igg_at(f, ci, cj - 1);
        // E, N, W, S, NE, NW, SW, SE: the first of the smallest keys wins (the loop unrolls: every index below is a constant)
        const int di[8] = {1, 0, -1, 0, 1, -1, -1, 1}, dj[8] = {0, 1, 0, -1, 1, 1, -1, -1};
        const float val[8] = {e, n, wv, s, igg_at(f, ci + 1, cj + 1), igg_at(f, ci - 1, cj + 1), igg_at(f, ci - 1, cj - 1),
                              igg_at(f, ci + 1, cj - 1)};
        const bool open[8] = {true, true, true, true, !own || (e < inf && n < inf), !own || (wv < inf && n < inf),
                              !own || (wv < inf && s < inf), !own || (e < inf && s < inf)};
        float best = inf;
        int ni = 0, nj = 0;
        go = false;
        pick = 255;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float key = val[k] + (k < 4 ? IGG_ORTHO : IGG_DIAG);
            if (open[k] && val[k] < inf && key < best) {
                best = key;
                ni = ci + di[k];
                nj = cj + dj[k];
                go = true;
                pick = k;
            }
        }
        ax = ig_cell_centre(ni);
        ay = ig_cell_centre(nj);
    }
    if (go) {
        const double err = igg_wrap(igg_atan2(ay - y, ax - x) - th);
        om = clipd(err / P.dt, -P.w_max, P.w_max);
        const double rem = err - om * P.dt;
        if (!(fabs(rem) > P.align_tol)) v = to_goal ? fmin(P.v_max, dist / P.dt) : P.v_max;
    }
    reinterpret_cast<float2*>(actions)[a] = make_float2((float)v, (float)om);
    if (choice) choice[wr] = (uint8_t)pick;
}

// Behind the step and the observe launch: the worlds the restart mask names lose their goals (their map is gone); every robot's
// distance to go - the field at its own cell - and whether it stands within goal_tol of its goal.
__global__ void __launch_bounds__(64) k_ig_goal_status(CagymDev D, IgGoalParams P, const uint8_t* __restrict__ restart_mask,
                                                       const float* __restrict__ field, const double* __restrict__ goal_xy,
                                                       uint8_t* active, float* goal_distance, uint8_t* goal_reached) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int rank = ig_robot_rank(D, w, lane, P.R);
    if (rank < 0) return;
    const size_t wr = (size_t)w * P.R + rank, a = (size_t)w * D.M + lane;
    bool act = active[wr] != 0;
    if (restart_mask && restart_mask[w]) {
        act = false;
        active[wr] = 0;
    }
    float dist = ig_inf_f();
    bool reached = false;
    if (act) {
        const double x = D.px[a], y = D.py[a];
        dist = igg_at(field + wr * IG_BEL * IG_BEL, ig_bel_cell(x), ig_bel_cell(y));
        const double dx = goal_xy[2 * wr] - x, dy = goal_xy[2 * wr + 1] - y;
        reached = sqrt(dx * dx + dy * dy) <= P.goal_tol;
    }
    goal_distance[wr] = dist;
    goal_reached[wr] = reached ? 1 : 0;
}
