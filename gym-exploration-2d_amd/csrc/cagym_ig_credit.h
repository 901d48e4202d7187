// cagym_ig_credit.h -- whose cone earned the team's reward (include/cagym.h: cagym_ig_credit): per robot of a learner's team, the MI
// sum over its own visible cells, over the cells it alone saw, and the difference reward - the team's gain minus what the gain would
// have been had this robot not looked.  The counterfactual needs each robot's odds factor per cell, which never leaves the observe
// kernel; this launch, directly behind it, recomputes the factor from the same poses and detections (ig_robot_inputs_lds and
// ig_odds_factor of cagym_ig_observe.h: one statement of each, both kernels call it) and divides it out of the belief observe left.
//
// One workgroup of 256 threads per world:
//   1. poses and detections of the R robots into LDS on wave 0 (observe's phase 2); a slot past the world's team has no rows;
//   2. R passes of ig_visible_block into R LDS masks V_r (an absent robot: the empty mask); their union U, and per cell a byte with
//      bit r set where the cell is in V_r (U_-r is then "any other bit");
//   3. gain = ig_reward_block(mi, U) - observe's gain[w] bit for bit, same cache, same mask, same order - and per robot three block
//      sums in ig_reward_block's order (thread q % 256 accumulates its cells strided, then the halving tree), run through ONE tree:
//        own       over V_r                     of mi[q]
//        exclusive over V_r & ~U_-r             of mi[q]
//        loo       over U_-r                    of (q in V_r ? ig_cell_mi(belief[q] / f_r(q)) : mi[q])
//      difference = gain - loo.  An empty set sums to +0.0; an absent robot's row is (0, 0, 0) with loo = gain.
//   4. threads 0 .. 3R-1, one per (robot, kind): credit, reward (0 for a world restarted in this launch, as team_reward is) and the
//      caller's accumulators by k_ig_observe's statements; thread 0 counts the episode.
// The R traces repeat what observe already traced: the price of leaving observe's outputs and launch untouched.  Nothing of the
// handle is written.  No atomics on global memory, no waits: barriers only, one uniform early exit before the first barrier.
#pragma once
#include "cagym_ig_observe.h"

struct IgCreditParams {
    int R;
    unsigned int flags;  // CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED
    float det_range;     // fp32, as k_ig_observe takes it
    double fov, range;
};

struct IgCreditOut {                       // caller-owned, each may be null
    double* gain;                          // [N]
    unsigned long long* robot_observed;    // [N,R,60]
    double* credit;                        // [N,R,3] own, exclusive, difference
    double* loo;                           // [N,R]
    double* reward;                        // [N,R,3]
    double *running, *sum, *last;          // [N,R,3]
    int32_t* episodes;                     // [N]
};

__global__ void __launch_bounds__(256) k_ig_credit(CagymDev D, IgDev G, IgCreditParams P, const float* __restrict__ oas,
                                                   const uint8_t* __restrict__ restart_mask, IgCreditOut O) {
    __shared__ unsigned long long vis[IG_MAXR][IG_BEL];
    __shared__ unsigned long long uni[IG_BEL];
    __shared__ unsigned char cover[IG_BEL * IG_BEL];  // bit r: the cell is in V_r
    __shared__ double red[3][256];
    __shared__ double s_pose[IG_MAXR][3];
    __shared__ double s_det[IG_MAXR][IG_MAXK][2];
    __shared__ int s_nd[IG_MAXR];
    __shared__ int s_has[IG_MAXR];
    __shared__ double s_credit[IG_MAXR][4];  // own, exclusive, difference, loo
    const int w = blockIdx.x, tid = threadIdx.x, R = P.R;
    const bool restarted = restart_mask && restart_mask[w];  // uniform
    if ((P.flags & 4u) && !restarted) return;                // CAGYM_IG_OBSERVE_ONLY_RESTARTED: nothing of this world is read or written

    // 1. poses and detections, as observe took them
    if (tid < 64) ig_robot_inputs_lds(D, w, tid, R, P.det_range, oas, s_pose, s_det, s_nd, [&](int r, int slot, double) { s_has[r] = slot >= 0; });
    __syncthreads();

    // 2. every robot's visible cells, their union, the cover bytes
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double* bel = G.belief + (size_t)w * IG_BEL * IG_BEL;
    const double* mi = G.mi + (size_t)w * IG_BEL * IG_BEL;
    for (int r = 0; r < R; r++) {
        if (s_has[r]) {  // uniform
            ig_visible_block(d2, s_pose[r][0], s_pose[r][1], s_pose[r][2], P.fov, P.range, vis[r], tid, blockDim.x);
        } else {
            for (int j = tid; j < IG_BEL; j += blockDim.x) vis[r][j] = 0ull;
            __syncthreads();
        }
    }
    for (int j = tid; j < IG_BEL; j += blockDim.x) {
        unsigned long long u = 0ull;
        for (int r = 0; r < R; r++) {
            u |= vis[r][j];
            if (O.robot_observed) O.robot_observed[((size_t)w * R + r) * IG_BEL + j] = vis[r][j];
        }
        uni[j] = u;
    }
    for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {
        const int j = q / IG_BEL, i = q - j * IG_BEL;
        unsigned int cv = 0u;
        for (int r = 0; r < R; r++) cv |= (unsigned int)((vis[r][j] >> i) & 1ull) << r;
        cover[q] = (unsigned char)cv;
    }
    __syncthreads();

    // 3. the team's gain, then own / exclusive / leave-one-out per robot
    const double gain = ig_reward_block(mi, uni, red[0], tid, blockDim.x);  // ends with a barrier
    const double thr = sqrt(0.5) * IG_BEL_CELL + 0.01;
    for (int r = 0; r < R; r++) {
        const double px = s_pose[r][0], py = s_pose[r][1];
        double s, c;
        ig_sincos(s_pose[r][2], &s, &c);
        const int nd = s_nd[r];
        const unsigned int bit = 1u << r;
        double own = 0.0, excl = 0.0, loo = 0.0;
        for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {
            const unsigned int cv = cover[q];
            const bool mine = cv & bit, others = cv & ~bit;
            if (!mine && !others) continue;
            const double m = mi[q];
            if (mine) {
                own += m;
                if (!others) excl += m;
            }
            if (others) {
                double term = m;
                if (mine) {  // the cell as the others alone would have left it: this robot's factor divided out
                    const int j = q / IG_BEL, i = q - j * IG_BEL;
                    term = ig_cell_mi(bel[q] / ig_odds_factor(i, j, px, py, c, s, s_det[r], nd, thr));
                }
                loo += term;
            }
        }
        red[0][tid] = own;
        red[1][tid] = excl;
        red[2][tid] = loo;
        __syncthreads();
        for (int h = blockDim.x / 2; h > 0; h >>= 1) {
            if (tid < h) {
                red[0][tid] += red[0][tid + h];
                red[1][tid] += red[1][tid + h];
                red[2][tid] += red[2][tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) {
            s_credit[r][0] = red[0][0];
            s_credit[r][1] = red[1][0];
            s_credit[r][2] = gain - red[2][0];
            s_credit[r][3] = red[2][0];
        }
        __syncthreads();
    }

    // 4. outputs and the caller's accumulators (k_ig_observe's statements, per robot and kind)
    if (tid < 3 * R) {
        const int r = tid / 3, k = tid - 3 * r;
        const size_t idx = ((size_t)w * R + r) * 3 + k;
        const double cr = s_credit[r][k];
        if (O.credit) O.credit[idx] = cr;
        if (O.reward) O.reward[idx] = restarted ? 0.0 : cr;  // the first observation of a new episode is no reward for the old one's last action
        if (O.running) {
            double run = O.running[idx];
            if (restarted) {
                if (P.flags & 1u) {
                    if (O.sum) O.sum[idx] += run;
                    if (O.last) O.last[idx] = run;
                }
                run = 0.0;
            }
            O.running[idx] = run + cr;  // ... and counts toward the new episode's return
        }
    }
    if (tid < R && O.loo) O.loo[(size_t)w * R + tid] = s_credit[tid][3];
    if (tid == 0) {
        if (O.gain) O.gain[w] = gain;
        if (O.episodes && restarted && (P.flags & 1u)) O.episodes[w] += 1;
    }
}
