// cagym_ga3c_state.h -- the GA3C-CADRL state vector (ga3c_state_row, k_ga3c_state) and the on-device list of GA3C agents
// (k_ga3c_select).  Included by cagym_ga3c.h; cagym_ga3c16.h builds its rows in LDS with the same ga3c_state_row.
#pragma once
#include "cagym_device.h"

// GA3CCADRLPolicy.agents_to_ga3c_cadrl_state (policies/GA3CCADRLPolicy.py:45-106): LPA lanes per agent (lane j <-> other agent
// j: its distance, sort key and feature row; the rank is a count over the keys the agent's lanes left in LDS),
// out[N,M,76] f32 = [id, n_others, dist_to_goal, heading_ego, pref_speed, radius, 10 x 7 other-agent features], rows indexed by
// flat agent (world * M + slot) - by place in the list for cagym_ga3c_act -; others ordered by (-round(d,2), p_orth), stable, last `max_observed` kept.  Zero rows for
// inactive slots.  agent_idx == null: every agent slot of the handle; else the B (or *B_dev) listed agents only - the
// reference builds the vector for the GA3C agent alone (find_next_action is per agent).
// the state row of one agent on the LPA lanes of group `al` (every thread of the block calls it: one barrier inside)
template <int LPA>
__device__ __forceinline__ void ga3c_state_row(const CagymDev& D, int max_observed, bool have, size_t a, size_t orow, int al, int j,
                                               double (*sk1)[LPA], double (*sk2)[LPA], float* out) {
    const int world = (int)(a / D.M), i = (int)(a - (size_t)world * D.M);
    float* o = out + orow * 76;
    if (have)
        for (int c = j; c < 76; c += LPA) o[c] = 0.f;
    // every load the lane may need is requested before the first is looked at (slot indices clamped into the world: in bounds whatever
    // the world's agent count is) - the agent count, the ego's and the other agent's records come back in ONE round trip instead of three
    const size_t base = (size_t)world * D.M;
    const size_t oj = base + (size_t)(j < D.M ? j : D.M - 1);
    int n = 0;
    double px = 0, py = 0, ri = 0, gxa = 0, gya = 0, pxj = 0, pyj = 0, rj = 0, vxj = 0, vyj = 0;
    if (have) {
        n = D.n_agents[world];
        px = D.px[a]; py = D.py[a]; ri = D.radius[a]; gxa = D.gx[a]; gya = D.gy[a];
        pxj = D.px[oj]; pyj = D.py[oj]; rj = D.radius[oj]; vxj = D.vx[oj]; vyj = D.vy[oj];
    }
    const bool ego_live = have && i < n;
    double prx = 0, pry = 0, orx = 0, ory = 0;
    double dx = 0, dy = 0, ed = 0, k1 = 0, k2 = 0;
    const bool mine = ego_live && j < n && j != i;
    if (ego_live) {
        const double gx = gxa - px, gy = gya - py;
        const double dist = sqrt(gx * gx + gy * gy);
        prx = gx; pry = gy;
        if (dist > 1e-8) { prx = gx / dist; pry = gy / dist; }
        orx = -pry; ory = prx;
    }
    if (mine) {
        dx = pxj - px; dy = pyj - py;
        ed = norm2(dx, dy) - ri - rj;
        k1 = -(rint(ed * 100.0) / 100.0);
        k2 = dot2(dx, dy, orx, ory);
        sk1[al][j] = k1;
        sk2[al][j] = k2;
    }
    __syncthreads();  // keys of the agent's lanes; also orders the zero fill before the row stores below
    const int cnt = n - 1;
    const int drop = cnt > max_observed ? cnt - max_observed : 0;
    if (mine) {
        int before = 0;  // others sorted strictly before j: smaller (k1, k2), ties by lower index (stable)
        for (int l = 0; l < n; l++) {
            if (l == i || l == j) continue;
            const double l1 = sk1[al][l], l2 = sk2[al][l];
            before += (l1 < k1) || (l1 == k1 && (l2 < k2 || (l2 == k2 && l < j)));
        }
        const int row = before - drop;
        if (row >= 0) {
            const double vx = vxj, vy = vyj;
            float* r = o + 6 + 7 * row;
            r[0] = (float)dot2(dx, dy, prx, pry);
            r[1] = (float)k2;
            r[2] = (float)dot2(vx, vy, prx, pry);
            r[3] = (float)dot2(vx, vy, orx, ory);
            r[4] = (float)rj;
            r[5] = (float)(ri + rj);
            r[6] = (float)ed;
        }
    }
    if (ego_live && j == i) {
        o[0] = (float)i;
        o[1] = (float)(cnt - drop);  // rows kept: the ranks are a permutation of 0 .. cnt - 1
        o[2] = (float)D.dist_goal[a];
        o[3] = (float)D.heading_ego[a];
        o[4] = (float)D.pref[a];
        o[5] = (float)ri;
    }
}

template <int LPA>
__global__ void __launch_bounds__(256) k_ga3c_state(CagymDev D, int max_observed, const int32_t* __restrict__ agent_idx, int B,
                                                    uint32_t* ctr, float* out) {
    constexpr int APB = 256 / LPA;
    __shared__ double sk1[APB][LPA], sk2[APB][LPA];
    const int al = threadIdx.x / LPA, j = threadIdx.x % LPA;
    // ctr (cagym_ga3c_act): the list k_ga3c_select just built holds ctr[0] - ctr[1] agents; word 2 passes that on to the forward kernel
    const uint32_t listed = ctr ? ctr[0] - ctr[1] : 0u;
    if (ctr && blockIdx.x == 0 && threadIdx.x == 0) ctr[2] = listed;
    const long long total = agent_idx ? (long long)(ctr ? (int)listed : B) : (long long)D.N * D.M;
    if ((long long)blockIdx.x * APB >= total) return;  // uniform: the whole block is beyond the list
    const long long q = (long long)blockIdx.x * APB + al;
    const bool have = q < total;
    const size_t a = have ? (agent_idx ? (size_t)agent_idx[q] : (size_t)q) : 0;
    // cagym_ga3c_act's rows are stored by PLACE IN THE LIST (the forward kernel's tile of 32 agents is one contiguous 9.7 KB
    // block and needs no index look-up in front of its loads); every other caller gets rows indexed by flat agent
    ga3c_state_row<LPA>(D, max_observed, have, a, (ctr && have) ? (size_t)q : a, al, j, sk1, sk2, out);
}


// indices (world * M + slot) of the active agents whose policy id is CAGYM_POL_GA3C, compacted on the device (order within
// the list is not fixed: every consumer treats the listed agents independently).  The list needs no reset from the host
// (round 3; a memset in front of every call was 4.9 us of cfg4's step): ctr[0] is a ticket counter that only ever grows
// (unsigned, wraps), ctr[1] its value when this list began; a place in the list is ticket - ctr[1].  k_ga3c_state turns the
// difference into the list length (ctr[2]) and the forward kernel - the last reader - starts the next list (ctr[1] = ctr[0]).
// The words are the handle's, zero at creation; the chain replays from a captured graph as it is.  One call per handle in flight
// (include/cagym.h): a chain that was cut short (a failed launch) leaves the list open - cagym_ga3c_act re-zeroes the words then -
// and a place beyond the table (possible only then) is never stored.
__global__ void __launch_bounds__(1024) k_ga3c_select(CagymDev D, int32_t* idx, uint32_t* ctr) {
    // one returning atomic per 1024-thread block (all of them hit one L2 address: per-wave atomics took 16 us for 81 920 slots)
    __shared__ int wave_cnt[16], wave_base[16];
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)D.N * D.M;
    bool take = false;
    if (a < total) {
        const uint32_t st = D.status[a];
        take = (st & CAGYM_FLAG_ACTIVE) && ST_POLICY(st) == CAGYM_POL_GA3C;
    }
    const unsigned long long m = __ballot(take);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < 16; w++) { wave_base[w] = tot; tot += wave_cnt[w]; }
        const int base = tot ? (int)(atomicAdd(&ctr[0], (uint32_t)tot) - ctr[1]) : 0;
        for (int w = 0; w < 16; w++) wave_base[w] += base;
    }
    __syncthreads();
    if (take) {
        const size_t place = (size_t)(unsigned)(wave_base[wave] + __popcll(m & ((1ull << lane) - 1ull)));
        if (place < total) idx[place] = (int32_t)a;
    }
}
