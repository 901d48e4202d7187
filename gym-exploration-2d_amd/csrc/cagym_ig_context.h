// cagym_ig_context.h -- the second image of a learner's view (include/cagym.h: cagym_ig_context_window): beside each robot's window of the
// TARGET belief (k_ig_observe's phase 5) a window of what the built-in planners use and the belief does not show - the walls, the other
// moving agents and the cells the team's sensors covered in this update.  Same frame, same G x G sample points, three channels:
//   0  clearance: min(EDF(sample), clear_max) / clear_max on the world's current scenario slot (edf_at, the planners' feasibility test)
//   1  agents:    1.0 in the window cell of a teammate (CAGYM_POL_IGMCTS), 0.5 in that of any other non-static agent; targets stay hidden
//   2  seen now:  1 where the sample's belief cell is in `observed`, the union k_ig_observe just wrote
//
// One workgroup of 256 threads per world.  Wave 0 (lane j = slot j, M <= 32) finds the robots with ig_robot_slot and leaves poses and
// (sin, cos) in LDS - ig_window_sincos, and ig_window_walk over them, as k_ig_observe: both windows agree on every sample point - and compacts,
// per robot, the agents whose window cell lies inside its window into a short LDS list (ballot + popcount, at most M - 1 entries of
// cell index | teammate bit).  Then lanes stride over the R * G * G out cells, b fastest: one gather from the distance field, one LDS
// word of the observed set, a walk over the robot's list (a handful of entries, not M slots), three stores contiguous in b.
// No atomics, no waits: one barrier, one early exit per workgroup in front of it.
#pragma once
#include "cagym_ig.h"

struct IgContextParams {
    int R, G, rotate;
    unsigned int flags;  // CAGYM_IG_CONTEXT_ONLY_MASKED
    double clear_max;
};

__global__ void __launch_bounds__(256) k_ig_context_window(CagymDev D, IgDev G, IgContextParams P, const unsigned long long* __restrict__ observed,
                                                           const uint8_t* __restrict__ world_mask, float* window) {
    __shared__ unsigned long long s_obs[IG_BEL];
    __shared__ double s_pose[IG_MAXR][2];
    __shared__ double s_sc[IG_MAXR][2];
    __shared__ int s_agent[IG_MAXR][IG_MAXK + 1];  // a_s * G + b_s, bit 16: a teammate
    __shared__ int s_na[IG_MAXR];
    const int w = blockIdx.x, tid = threadIdx.x, M = D.M, R = P.R, Gw = P.G;
    if ((P.flags & 1u) && !(world_mask && world_mask[w])) return;  // CAGYM_IG_CONTEXT_ONLY_MASKED: nothing of this world is read or written

    // 1. robots, their frames and their agent lists (wave 0)
    if (tid < 64) {
        const int lane = tid;
        unsigned long long robots;
        ig_robot_slot(D, w, lane, robots);
        const uint32_t st = lane < M ? D.status[(size_t)w * M + lane] : 0u;
        const bool shown = (st & CAGYM_FLAG_ACTIVE) && ST_POLICY(st) != CAGYM_POL_STATIC;
        const bool mate = ST_POLICY(st) == CAGYM_POL_IGMCTS;
        double ax = 0.0, ay = 0.0;
        if (shown) {
            ax = D.px[(size_t)w * M + lane];
            ay = D.py[(size_t)w * M + lane];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const double half = (double)(Gw / 2);
        for (int r = 0; r < R; r++) {
            const int slot = ig_next_robot(robots);
            double px = 0.0, py = 0.0, th = 0.0;
            if (slot >= 0) {
                const size_t a = (size_t)w * M + slot;
                px = D.px[a]; py = D.py[a]; th = D.heading[a];
            }
            double sn, cs;
            ig_window_sincos(P.rotate, th, sn, cs);
            // this lane's agent in robot r's frame: window cell (a_s, b_s) = floor(f / 0.5) + G / 2
            const double dx = ax - px, dy = ay - py;
            const double fx = cs * dx + sn * dy, fy = cs * dy - sn * dx;
            const double ca = floor(fx * 2.0) + half, cb = floor(fy * 2.0) + half;  // (exact in fp64 wherever the test below holds)
            const bool in = shown && slot >= 0 && lane != slot && ca >= 0.0 && ca < (double)Gw && cb >= 0.0 && cb < (double)Gw;  // (NaN: false)
            const unsigned long long im = __ballot(in);
            if (in) s_agent[r][__popcll(im & below)] = ((int)ca * Gw + (int)cb) | (mate ? 0x10000 : 0);
            if (lane == 0) {
                s_pose[r][0] = px;
                s_pose[r][1] = py;
                s_sc[r][0] = sn;
                s_sc[r][1] = cs;
                s_na[r] = __popcll(im);
            }
        }
    }
    for (int j = tid; j < IG_BEL; j += blockDim.x) s_obs[j] = observed ? observed[(size_t)w * IG_BEL + j] : 0ull;
    __syncthreads();

    // 2. the cells (ig_window_walk: k_ig_observe's sample points and source cells)
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    ig_window_walk(s_pose, s_sc, R, Gw, window, w, tid,
                   [&](int rb, int ab, double qx, double qy, int i, int j, bool inside, float* ch) {
                       if (inside) {
                           ch[0] = (float)(fmin(edf_at(d2, qx, qy), P.clear_max) / P.clear_max);  // clearance
                           ch[2] = ((s_obs[j] >> i) & 1ull) ? 1.f : 0.f;                          // seen now
                       }
                       const int na = s_na[rb];
                       for (int n = 0; n < na; n++) {  // agents
                           const int e = s_agent[rb][n];
                           if ((e & 0xffff) == ab) ch[1] = fmaxf(ch[1], (e & 0x10000) ? 1.0f : 0.5f);
                       }
                   });
}
