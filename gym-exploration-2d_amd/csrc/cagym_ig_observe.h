// cagym_ig_observe.h -- the learner's end of a step (include/cagym.h: cagym_ig_observe): what an exploration policy that is NOT one
// of the built-in planners needs behind every step or reset, in ONE launch - the per-world restart, the robots' poses and detections,
// the belief update, the team's MI reward with its episode accumulators, and the belief as each robot sees it (an ego-centred,
// optionally heading-aligned window of G x G cells with three channels: P(occupied), cached cell MI, inside-the-map).
//
// One workgroup of 256 threads per world, the phases of the four-launch chain in its order:
//   k_ig_fill_belief (restart)  ->  k_ig_robot_inputs  ->  k_ig_update  ->  k_ig_reward  ->  k_ig_episode_boundary's accumulators
// with the same device functions (ig_fill_world_prior, ig_robot_slot, ig_visible_block, mat2vec, ig_cell_mi, ig_reward_block) and,
// where the chain's arithmetic lives in a kernel body (the detector's fp32 test, detection = row + pose, the odds factor), the same
// expressions on the same operands: belief, observed and reward are the chain's bit for bit (tests/test_ig_learner.py).  Poses,
// detections and their counts never reach global memory: wave 0 leaves them in LDS (K <= 31 rows per robot, 4 KB).
//
// Who writes what: cell q of the world's belief and MI cache belongs to thread q % 256 in every phase (fill, update, cache refresh,
// reward sum), the accumulators to thread 0.  The window phase reads cells other threads wrote, behind the barrier that ends
// ig_reward_block.  No atomics on global memory, no waits: barriers only, one early exit per workgroup (before the first barrier).
#pragma once
#include "cagym_ig.h"
#include "cagym_ig_episode.h"

struct IgObserveParams {
    int R, G, rotate;
    unsigned int flags;  // CAGYM_IG_EPISODE_FOLD | CAGYM_IG_OBSERVE_ONLY_RESTARTED
    float det_range;     // fp32, as k_ig_robot_inputs takes it
    double fov, range;
};

// Phase 2 below, poses and detections of world w's R robots into LDS (k_ig_robot_inputs on wave 0, lane j = slot j): the ONE statement
// of it, for this kernel and for k_ig_credit (cagym_ig_credit.h), which must see the robots exactly as this launch did.  A slot past the
// world's team gets a zero pose and no rows.  each(r, slot, heading) runs on lane 0 per robot (slot < 0: no such robot).
template <typename F>
__device__ __forceinline__ void ig_robot_inputs_lds(const CagymDev& D, int w, int lane, int R, float det_range, const float* __restrict__ oas,
                                                    double (*s_pose)[3], double (*s_det)[IG_MAXK][2], int* s_nd, F each) {
    const int M = D.M, K = M - 1;
    unsigned long long robots;
    ig_robot_slot(D, w, lane, robots);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < R; r++) {
        const int slot = ig_next_robot(robots);
        double px = 0.0, py = 0.0, th = 0.0;
        int cnt = 0;
        if (slot >= 0) {
            const size_t a = (size_t)w * M + slot;
            px = D.px[a]; py = D.py[a]; th = D.heading[a];
            bool tgt = false;
            float r0 = 0.f, r1 = 0.f;
            if (lane < K) {
                const float* row = oas + (a * K + lane) * 10;
                r0 = row[0];
                r1 = row[1];
                tgt = row[9] == 1.0f && sqrtf(r0 * r0 + r1 * r1) <= det_range;
            }
            const unsigned long long tm = __ballot(tgt);
            if (tgt) {
                double* d = s_det[r][__popcll(tm & below)];
                d[0] = (double)r0 + px;
                d[1] = (double)r1 + py;
            }
            cnt = __popcll(tm);
        }
        if (lane < 3) s_pose[r][lane] = lane == 0 ? px : lane == 1 ? py : th;
        if (lane == 0) {
            s_nd[r] = cnt;
            each(r, slot, th);
        }
    }
}

// The odds factor of belief cell (i, j) under a robot at (px, py) with (c, s) = (cos, sin) of its heading and nd detections det:
// 1.5 when a detection lies within thr of the cell's centre (both points rotated by mat2vec, k_ig_update's expression), else 0.66.
__device__ __forceinline__ double ig_odds_factor(int i, int j, double px, double py, double c, double s, const double (*det)[2], int nd,
                                                 double thr) {
    double rs = 0.66;
    if (nd > 0) {
        double cx = ig_cell_centre(i), cy = ig_cell_centre(j);
        double r0, r1;
        mat2vec(c, s, cx - px, cy - py, r0, r1);
        for (int d = 0; d < nd; d++) {
            const double* tg = det[d];
            double t0, t1;
            mat2vec(c, s, tg[0] - px, tg[1] - py, t0, t1);
            double e0 = t0 - r0, e1 = t1 - r1;
            if (sqrt(e0 * e0 + e1 * e1) < thr) { rs = 1.5; break; }
        }
    }
    return rs;
}

__global__ void __launch_bounds__(256) k_ig_observe(CagymDev D, IgDev G, IgEpisode A, IgObserveParams P, const float* __restrict__ oas,
                                                    const uint8_t* __restrict__ restart_mask, double* team_reward, double* gain,
                                                    unsigned long long* observed, float* window) {
    __shared__ unsigned long long vis[IG_BEL];
    __shared__ unsigned long long uni[IG_BEL];
    __shared__ double red[256];
    __shared__ double s_pose[IG_MAXR][3];
    __shared__ double s_sc[IG_MAXR][2];  // the window's (sin, cos) of each robot
    __shared__ double s_det[IG_MAXR][IG_MAXK][2];
    __shared__ int s_nd[IG_MAXR];
    const int w = blockIdx.x, tid = threadIdx.x, R = P.R;
    const bool restarted = restart_mask && restart_mask[w];  // uniform
    if ((P.flags & 4u) && !restarted) return;                // CAGYM_IG_OBSERVE_ONLY_RESTARTED: nothing of this world is read or written

    // 1. the restart: fold and zero the running return (k_ig_episode_boundary's statements), belief and MI cache at the prior
    double run = 0.0;
    if (tid == 0) {
        run = A.running[w];
        if (restarted) {
            if (P.flags & 1u) {
                A.sum[w] += run;
                A.last[w] = run;
                A.episodes[w] += 1;
            }
            run = 0.0;
        }
    }
    if (restarted) ig_fill_world_prior(G, w, tid, blockDim.x);

    // 2. poses and detections (k_ig_robot_inputs on wave 0, lane j = slot j), into LDS
    if (tid < 64)
        ig_robot_inputs_lds(D, w, tid, R, P.det_range, oas, s_pose, s_det, s_nd, [&](int r, int, double th) {
            double s, c;
            ig_window_sincos(P.rotate, th, s, c);
            s_sc[r][0] = s;
            s_sc[r][1] = c;
        });
    for (int j = tid; j < IG_BEL; j += blockDim.x) uni[j] = 0ull;
    __syncthreads();  // (also: the prior of a restarted world is in place)

    // 3. the belief update of k_ig_update, robots in slot order, poses and detections from LDS
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    double* bel = G.belief + (size_t)w * IG_BEL * IG_BEL;
    double* mi = G.mi + (size_t)w * IG_BEL * IG_BEL;
    const double thr = sqrt(0.5) * IG_BEL_CELL + 0.01;
    for (int p = 0; p < R; p++) {
        const double px = s_pose[p][0], py = s_pose[p][1], phi = s_pose[p][2];
        ig_visible_block(d2, px, py, phi, P.fov, P.range, vis, tid, blockDim.x);
        double s, c;
        ig_sincos(phi, &s, &c);
        const int nd = s_nd[p];
        for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {
            int j = q / IG_BEL, i = q - j * IG_BEL;
            if (!((vis[j] >> i) & 1ull)) continue;
            bel[q] *= ig_odds_factor(i, j, px, py, c, s, s_det[p], nd, thr);
        }
        for (int j = tid; j < IG_BEL; j += blockDim.x) uni[j] |= vis[j];
        __syncthreads();
    }
    if (observed)
        for (int j = tid; j < IG_BEL; j += blockDim.x) observed[(size_t)w * IG_BEL + j] = uni[j];
    for (int q = tid; q < IG_BEL * IG_BEL; q += blockDim.x) {  // the MI cache follows the belief (only cells seen in this update changed)
        int j = q / IG_BEL, i = q - j * IG_BEL;
        if ((uni[j] >> i) & 1ull) mi[q] = ig_cell_mi(bel[q]);
    }

    // 4. the team reward (k_ig_reward's sum: every thread sums cells it refreshed itself) and the accumulators
    const double r = ig_reward_block(mi, uni, red, tid, blockDim.x);  // ends with a barrier: the whole belief and cache are in place
    if (tid == 0) {
        A.running[w] = run + r;  // the first observation of a new episode counts toward that episode's return ...
        if (gain) gain[w] = r;
        if (team_reward) team_reward[w] = restarted ? 0.0 : r;  // ... and is no reward for the action that ended the old one
    }

    // 5. each robot's window (ig_window_walk: the sample point and the source cell are the same for all three channels)
    if (!window) return;
    ig_window_walk(s_pose, s_sc, R, P.G, window, w, tid,
                   [&](int, int, double, double, int i, int j, bool inside, float* ch) {
                       if (!inside) return;
                       const int q = j * IG_BEL + i;
                       const double odds = bel[q];
                       ch[0] = (float)(odds / (odds + 1));  // P(occupied)
                       ch[1] = (float)mi[q];                // cached cell MI
                       ch[2] = 1.f;                         // inside the map
                   });
}
