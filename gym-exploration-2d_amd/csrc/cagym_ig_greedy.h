// cagym_ig_greedy.h -- the one-step greedy information-gain policy (gfx950): policies/ig_greedy.py:64-94 for every IG robot of
// every world in one launch, on the primitives of cagym_ig.h (distance field, sphere-traced visibility, the belief's MI cache).
//
// Per robot: nine candidates c = 3 a + b = (v[a], w[b]); next pose by one Euler step, feasible <=> EDF(next) > radius + 0.1 (tested
// for v = 0 too, unlike ig_mcts.get_next_pose), reward = sum of cell MI over getVisibleCells(next); the first candidate with
// strictly the largest reward wins, the running maximum starting at -1.  Deviations from the reference: a next
// cell outside the 300 x 300 raster is infeasible; no feasible candidate gives choice 255 and the action (0, 0).
//
// Launch: 128 lanes per workgroup, the width k_ig_visible runs ig_visible_block at (a query's window holds ~200 cells of which
// ~50 are traced: wider groups add idle waves, not speed).  Independent mode: one workgroup per (world, robot).  Coordinated
// mode: one per world, its robots in slot order with the cells the earlier ones chose taken out of the later ones' rewards.
// Every mi[c] is the double cagym_ig_mi_reward returns for the same mask: ig_reward_256 below.
#pragma once
#include "cagym_ig.h"

#define IGG_THREADS 128

struct IgGreedyParams {
    int R, coordinate;
    double dt, radius, fov, range;
    double v0, v1, v2, w0, w1, w2;  // (scalars: an indexed by-value array would live in scratch)
};

// floor((t + 15) / 0.1) as edf_at takes it, without its numpy-style wrap of a negative index: -1 when the cell is outside
// [0, 300) (or t is huge / NaN)
__device__ __forceinline__ int igg_edf_index(double t) {
    const double tt = t + IG_HALF;
    double q = tt * 10.0;
    if (!(fabs(q - rint(q)) > 1e-7 && fabs(q) < 1e6)) q = tt / IG_EDF_CELL;
    const double f = floor(q);
    if (!(f >= 0.0 && f < (double)CAGYM_MAPD)) return -1;
    return (int)f;
}

// ig_reward_block's result AT 256 THREADS, computed by 128: lane t carries the partial sums of that block's threads t and t + 128
// (cells q = T, T + 256, ... in ascending order each); their sum is the first step of its tree, the remaining steps are the same.
__device__ inline double ig_reward_256(const double* mi, const unsigned long long* mask, double* red, int tid) {
    double lo = 0.0, hi = 0.0;
    for (int q = tid; q < IG_BEL * IG_BEL; q += 256) {
        const int j = q / IG_BEL, i = q - j * IG_BEL;
        if ((mask[j] >> i) & 1ull) lo += mi[q];
        const int q2 = q + 128;
        if (q2 < IG_BEL * IG_BEL) {
            const int j2 = q2 / IG_BEL, i2 = q2 - j2 * IG_BEL;
            if ((mask[j2] >> i2) & 1ull) hi += mi[q2];
        }
    }
    red[tid] = lo + hi;
    __syncthreads();
    for (int s = IGG_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(IGG_THREADS) k_ig_greedy(IgDev G, IgGreedyParams P, const double* __restrict__ poses,
                                                           double* __restrict__ actions, uint8_t* __restrict__ choice,
                                                           double* __restrict__ mi_out, unsigned long long* __restrict__ claimed_out) {
    __shared__ unsigned long long vis[IG_BEL];      // the candidate's visible cells (less the claimed ones)
    __shared__ unsigned long long best[IG_BEL];     // ... of the best candidate so far
    __shared__ unsigned long long claimed[IG_BEL];  // cells the world's earlier robots chose (coordinated mode; else empty)
    __shared__ double red[IGG_THREADS];
    const int tid = threadIdx.x;
    const int w = P.coordinate ? (int)blockIdx.x : (int)blockIdx.x / P.R;
    const int r_begin = P.coordinate ? 0 : (int)blockIdx.x % P.R, r_end = P.coordinate ? P.R : r_begin + 1;
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double* mi = G.mi + (size_t)w * IG_BEL * IG_BEL;
    const IgCone cone = ig_cone(P.fov);
    // lane j < 60 owns word j of the three masks from here on (IGG_THREADS > IG_BEL): no barrier is needed between its own accesses
    if (tid < IG_BEL) claimed[tid] = 0ull;
    for (int r = r_begin; r < r_end; r++) {
        const double* pose = poses + ((size_t)w * P.R + r) * 3;
        const double x = pose[0], y = pose[1], th = pose[2];
        double sn, cs;
        ig_sincos(th, &sn, &cs);
        double best_mi = -1.0, best_v = 0.0, best_w = 0.0;  // max_mi = -1 (ig_greedy.py:69)
        int best_c = 255;
        for (int c = 0; c < 9; c++) {  // everything below is uniform across the workgroup
            const int a = c / 3, b = c - 3 * a;
            const double v = a == 0 ? P.v0 : a == 1 ? P.v1 : P.v2, om = b == 0 ? P.w0 : b == 1 ? P.w1 : P.w2;
            const double vx = fma(cs, v, -sn * 0.0), vy = fma(sn, v, cs * 0.0);  // ig_next_pose's sub-step: np.dot(R, [v, 0])
            const double nx = x + vx * P.dt, ny = y + vy * P.dt, nt = th + om * P.dt;
            const bool feasible = igg_edf_index(nx) >= 0 && igg_edf_index(ny) >= 0 && edf_at(d2, nx, ny) > P.radius + 0.1;
            double m = -1.0;
            if (feasible) {
                ig_visible_block(d2, nx, ny, nt, P.fov, P.range, vis, tid, IGG_THREADS, &cone);
                if (tid < IG_BEL) vis[tid] &= ~claimed[tid];
                __syncthreads();
                m = ig_reward_256(mi, vis, red, tid);
                if (m > best_mi) {
                    best_mi = m; best_c = c; best_v = v; best_w = om;
                    if (tid < IG_BEL) best[tid] = vis[tid];
                }
            }
            if (tid == 0 && mi_out) mi_out[((size_t)w * P.R + r) * 9 + c] = m;
        }
        if (tid == 0) {
            actions[((size_t)w * P.R + r) * 2] = best_v;
            actions[((size_t)w * P.R + r) * 2 + 1] = best_w;
            choice[(size_t)w * P.R + r] = (uint8_t)best_c;
        }
        if (P.coordinate && best_c != 255 && tid < IG_BEL) claimed[tid] |= best[tid];  // (best is already less the claimed cells)
    }
    if (claimed_out && r_begin == 0 && tid < IG_BEL) claimed_out[(size_t)w * IG_BEL + tid] = claimed[tid];
}
