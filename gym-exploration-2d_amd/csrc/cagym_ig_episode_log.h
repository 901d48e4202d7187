// cagym_ig_episode_log.h -- append-only episode log of the information-gathering team (include/cagym.h: cagym_ig_episode_log_*).
// The collision-avoidance log (cagym_episode_log.h) rebuilds its rows from the step's outputs; what a target search is judged by -
// which targets the belief localised and when, how uncertain it was at the end - lives in the belief, which the chain puts back to
// the prior in the launch that folds the episode's return (k_ig_observe phase 1, k_ig_episode_boundary).  So this log sits between
// the step launch and that launch and reads the belief, the MI cache and the running return as the finished episode left them:
// one row per finished team episode in a device ring of `capacity` rows, keyed by the stream key (uint32_t)(w + e * N).
//
// One update per env step, two launches chained by stream order:
//   k_ig_episode_log_scan    ONE workgroup: per world, does the log's cursor agree with D.episode (a finished world's has advanced by
//                            one)?  pos[w] = the row number of a finished world - head + the finished worlds before it, so the rows of
//                            an update are appended in world order -, IGLOG_IDLE for a world in mid-episode, IGLOG_DESYNC for one
//                            that disagrees.  The single writer of head (+= finished), seq (+= 1) and desync (+= disagreeing).
//   k_ig_episode_log_update  one workgroup of 256 per world.  Wave 0: steps_run += 1 and the threshold test of the episode's targets
//                            (the STATIC agents of its pool slot; lane i = slot i, one gather of the belief cell each).  A world that
//                            did not finish leaves there.  A finished one writes its row - the return with the boundary's own fp64 add,
//                            found_at, and three sums over the 3600 cells - and starts its running values anew.
// The sums are reproducible: thread t adds the cells t, t + 256, ... in that order, the 64 partials of a wave meet in a butterfly of
// __shfl_xor (both partners add the same two doubles, so every lane ends on the same bits), the four waves' sums meet in LDS and
// thread 0 adds them in wave order.  No atomics, no waits: one barrier, one early exit per workgroup in front of it, plain vector
// stores.  pos is read-only in the update launch, cursor is read by the scan alone and steps_run / found_run by wave 0 alone, so no
// thread reads a word that a thread of another wave of the same launch writes.
// (Measured and dropped: one WAVE per world.  A quarter of the waves to dispatch, but a finished world's wave then walks 57 cells
// alone and the launch waits for it: 23.8 us instead of 15.0 us added per step at 2048 worlds, 12.0 instead of 8.4 at 256.)
#pragma once
#include "cagym_ig.h"
#include "cagym_ig_episode.h"

struct IgEpLog {
    // ring [capacity, ...]
    long long* slice;
    double *ret, *entropy, *residual_mi;
    uint32_t* key;
    int32_t *world, *episode, *steps, *n_targets, *n_found, *n_touched;
    int32_t* found_at;  // [capacity, M] -2: no target, -1: a target never found, else the 1-based step of the episode
    // the episode in progress of every world
    int32_t* steps_run;  // [N]
    int32_t* found_run;  // [N, M] -1 or the step at which the log first saw the target's cell at or above the threshold
    int32_t* cursor;     // [N] the episode the running values belong to
    unsigned long long* head;  // rows ever appended since the last clear
    unsigned long long* seq;   // update calls since the last clear
    int32_t* desync;
    unsigned long long* pos;  // [N] between the two launches of one update
    int capacity;
    double odds_found;  // p_found / (1 - p_found), divided on the host
};

#define IGLOG_NT_SCAN 1024 /* lanes of the single scan workgroup */
#define IGLOG_IDLE (~0ull)
#define IGLOG_DESYNC (~0ull - 1ull)

// grid = 1, IGLOG_NT_SCAN lanes
__global__ void __launch_bounds__(IGLOG_NT_SCAN) k_ig_episode_log_scan(IgEpLog E, int N, const int32_t* __restrict__ episode,
                                                                      const uint8_t* __restrict__ game_over) {
    __shared__ unsigned wsum[IGLOG_NT_SCAN / CAGYM_WAVE], wbad[IGLOG_NT_SCAN / CAGYM_WAVE];
    const int lane = threadIdx.x & (CAGYM_WAVE - 1), wave = threadIdx.x >> 6;
    const unsigned long long head0 = *E.head;  // written by thread 0 behind the last barrier only
    unsigned long long carry = 0;              // the same in every lane
    unsigned bad_total = 0;
    for (int base = 0; base < N; base += IGLOG_NT_SCAN) {
        const int w = base + (int)threadIdx.x;
        unsigned c = 0;
        bool bad = false;
        if (w < N) {
            const bool go = game_over[w] != 0;
            bad = episode[w] != E.cursor[w] + (go ? 1 : 0);
            c = go && !bad;
        }
        unsigned x = c;  // inclusive scan inside the wave
        for (int d = 1; d < CAGYM_WAVE; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const unsigned long long bm = __ballot(bad);
        if (lane == CAGYM_WAVE - 1) wsum[wave] = x;
        if (lane == 0) wbad[wave] = (unsigned)__popcll(bm);
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int k = 0; k < IGLOG_NT_SCAN / CAGYM_WAVE; k++) {
            const unsigned s = wsum[k];
            before += k < wave ? s : 0u;
            total += s;
            bad_total += wbad[k];
        }
        if (w < N) E.pos[w] = bad ? IGLOG_DESYNC : c ? head0 + carry + before + (x - c) : IGLOG_IDLE;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *E.head = head0 + carry;
        *E.seq += 1ull;
        *E.desync += (int32_t)bad_total;
    }
}

// one cell's share of the belief's entropy in nats, -(P ln P + (1 - P) ln(1 - P)) with P = r / (r + 1); a cell whose P has reached
// 0 or 1 in fp64 contributes the limit 0 of that side (ig.episode_log_spec states the same)
__device__ __forceinline__ double ig_cell_entropy(double r) {
    const double p = r / (r + 1), q = 1 - p;
    double t = 0.0;
    if (p > 0.0) t = p * log(p);
    if (q > 0.0) t = t + q * log(q);
    return -t;
}

#define IGLOG_NT 256                                                  /* lanes of a world's workgroup */
#define IGLOG_CELLS ((IG_BEL * IG_BEL + IGLOG_NT - 1) / IGLOG_NT) /* cells per lane of a finished world: 15 */

// grid = N, IGLOG_NT lanes.  team_reward: the pointer the chain's boundary launch gets (NULL behind a learner's step)
__global__ void __launch_bounds__(IGLOG_NT) k_ig_episode_log_update(CagymDev D, IgDev G, IgEpisode A, IgEpLog E, const double* __restrict__ team_reward) {
    __shared__ double s_h[IGLOG_NT / CAGYM_WAVE], s_m[IGLOG_NT / CAGYM_WAVE];
    __shared__ int s_n[IGLOG_NT / CAGYM_WAVE];
    const int w = blockIdx.x, tid = threadIdx.x, M = D.M;
    const unsigned long long pos = E.pos[w], head = *E.head, cap = (unsigned long long)E.capacity;
    const bool sync = pos != IGLOG_DESYNC, finish = sync && pos != IGLOG_IDLE;  // uniform
    const bool write = finish && head - pos <= cap;  // among the last `capacity` rows ever appended (pos < head): else skipped, not raced
    const size_t r = write ? (size_t)(pos % cap) : 0;
    const double* bel = G.belief + (size_t)w * IG_BEL * IG_BEL;
    if (tid < CAGYM_WAVE) {  // wave 0, lane i = slot i: the running values and the threshold test
        const int ep = D.episode[w];
        const int steps = sync ? E.steps_run[w] + 1 : 0;
        bool target = false;
        int f = -1;
        if (sync && tid < M) {
            // the pool slot of the episode in progress; of a finished world that is the episode that ended (D.episode has advanced)
            long long s = ((long long)w + (long long)(ep - (finish ? 1 : 0)) * D.N) % D.S;
            if (s < 0) s += D.S;
            target = tid < D.sc_nagents[s] && D.sc_policy[(size_t)s * M + tid] == CAGYM_POL_STATIC;
            f = E.found_run[(size_t)w * M + tid];
            if (target && f < 0) {
                const double* s6 = D.sc_agents6 + ((size_t)s * M + tid) * 6;
                const int i = ig_bel_cell(s6[0]), j = ig_bel_cell(s6[1]);
                if (i >= 0 && i < IG_BEL && j >= 0 && j < IG_BEL && bel[j * IG_BEL + i] >= E.odds_found) f = steps;
            }
        }
        const unsigned long long tm = __ballot(target), fm = __ballot(target && f >= 0);
        if (tid < M) {
            if (write) E.found_at[r * M + tid] = target ? f : -2;
            E.found_run[(size_t)w * M + tid] = finish || !sync ? -1 : f;
        }
        if (tid == 0) {
            E.steps_run[w] = finish ? 0 : steps;
            E.cursor[w] = ep;
            if (write) {
                double run = A.running[w];
                if (team_reward) run += team_reward[w];  // k_ig_episode_boundary's add: the terminal step's reward belongs to the episode
                E.key[r] = (uint32_t)w + (uint32_t)(ep - 1) * (uint32_t)D.N;
                E.world[r] = w;
                E.episode[r] = ep - 1;
                E.slice[r] = (long long)(*E.seq - 1ull);
                E.steps[r] = steps;
                E.ret[r] = run;
                E.n_targets[r] = __popcll(tm);
                E.n_found[r] = __popcll(fm);
            }
        }
    }
    if (!write) return;

    // The three sums.  A finished world's workgroup is the launch's critical path, so its loads are issued together (15 cells per lane,
    // one round trip) and a cell at the prior - nine in ten after a short episode, and whole waves of them: a wave's 64 cells are
    // neighbours in a row - takes the entropy evaluated once per lane instead of its two logarithms (the same double: the same call).
    const double* mi = G.mi + (size_t)w * IG_BEL * IG_BEL;
    double odds[IGLOG_CELLS], cm[IGLOG_CELLS];
#pragma unroll
    for (int k = 0; k < IGLOG_CELLS; k++) {
        const int q = tid + k * IGLOG_NT;
        const bool in = q < IG_BEL * IG_BEL;
        odds[k] = in ? bel[q] : 1.0;
        cm[k] = in ? mi[q] : 0.0;
    }
    const double h_prior = ig_cell_entropy(1.0);
    double h = 0.0, m = 0.0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < IGLOG_CELLS; k++) {
        if (tid + k * IGLOG_NT < IG_BEL * IG_BEL) {
            h += odds[k] == 1.0 ? h_prior : ig_cell_entropy(odds[k]);
            m += cm[k];
            n += odds[k] != 1.0;
        }
    }
    for (int d = CAGYM_WAVE / 2; d > 0; d >>= 1) {
        h += __shfl_xor(h, d);
        m += __shfl_xor(m, d);
        n += __shfl_xor(n, d);
    }
    if ((tid & (CAGYM_WAVE - 1)) == 0) {
        s_h[tid >> 6] = h;
        s_m[tid >> 6] = m;
        s_n[tid >> 6] = n;
    }
    __syncthreads();
    if (tid == 0) {
        E.entropy[r] = ((s_h[0] + s_h[1]) + s_h[2]) + s_h[3];
        E.residual_mi[r] = ((s_m[0] + s_m[1]) + s_m[2]) + s_m[3];
        E.n_touched[r] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}

// The masked worlds (NULL = all) forget the episode in progress and take the handle's episode index; clear_rows: every row of the
// ring, head, the call counter and desync as cagym_ig_episode_log_init leaves them.  Grid-stride over max(N, capacity) * M.
__global__ void __launch_bounds__(256) k_ig_episode_log_restart(CagymDev D, IgEpLog E, const uint8_t* __restrict__ world_mask, int clear_rows) {
    const size_t NM = (size_t)D.N * D.M, LM = (size_t)E.capacity * D.M, stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = i0; i < NM; i += stride) {
        const size_t w = i / D.M;
        if (world_mask && !world_mask[w]) continue;
        E.found_run[i] = -1;
        if (i - w * D.M == 0) {
            E.steps_run[w] = 0;
            E.cursor[w] = D.episode[w];
        }
    }
    if (!clear_rows) return;
    for (size_t i = i0; i < LM; i += stride) {
        E.found_at[i] = 0;
        if (i < (size_t)E.capacity) {
            E.key[i] = 0u;
            E.world[i] = 0;
            E.episode[i] = 0;
            E.slice[i] = 0;
            E.steps[i] = 0;
            E.ret[i] = 0.0;
            E.n_targets[i] = 0;
            E.n_found[i] = 0;
            E.entropy[i] = 0.0;
            E.residual_mi[i] = 0.0;
            E.n_touched[i] = 0;
        }
    }
    if (i0 == 0) {
        *E.desync = 0;
        *E.seq = 0ull;
        *E.head = 0ull;
    }
}
