// cagym_episode_log.h -- append-only episode log rebuilt from the step outputs (include/cagym.h: cagym_episode_log_*).
// The per-scenario records (cagym_episode_records.h) keep one row per pool slot, which a streamed pool reuses; this log keeps one
// row per FINISHED EPISODE in a device ring of `capacity` rows instead, so it works on any pool, streamed ones included.  It consumes
// the same inputs under the same contract - flags [T,N,M], reward [T,N,M], game_over [T,N] of auto-reset stepping, every step once
// and in order - and computes t, ret, steps, outcome, extra_t and the masking with the recorder's own device functions
// (eprec_lane / eprec_advance / eprec_row / eprec_next / eprec_check): log and table hold the same doubles by construction.
//
// A row names its episode by the stream key (uint32_t)(w + e * N); its pool columns (n_agents, n_obst, the straight-line time inside
// extra_t) are read from slot (w + e * N) % S.  Under streaming the next cagym_stream_refill regenerates exactly that slot (it is
// the slot of episode e + k), so the update goes BEHIND the step(s) and BEFORE the refill.
//
// Order (deterministic): the rows of one update are appended world-major - ascending world, inside a world ascending slice -,
// updates append in call order, row number i since the last clear lives at ring index i % capacity.  An update that finishes
// n > capacity episodes writes its last `capacity` rows only (the others are skipped, not raced); head still grows by n.
//   k_episode_log_count  finished episodes per world over the T slices (skipped when T == 1: the scan reads game_over)
//   k_episode_log_scan   ONE workgroup: exclusive scan of the N counts on top of head -> pos[w], the row number of world w's first
//                        row of this update; the single writer of head (+= n) and seq (+= T)
//   k_episode_log_write  the recorder's one-writer kernel with another store: lane per (world, slot), running values in registers
//                        over the T slices, row pos[w] + (episodes of w finished so far) written iff it is among the last `capacity`
// chained by stream order only: no workgroup waits on another, no atomics on row positions (desync is counted as the recorder's is).
#pragma once
#include "cagym_episode_records.h"

struct EpLog {
    // ring [capacity, ...]
    uint32_t* key;
    int32_t *world, *episode;
    long long* slice;
    int32_t* steps;
    double* ret;
    int32_t *outcome, *n_agents, *n_obst;
    double *t, *extra_t;
    uint8_t* flags;
    EpRunning run;             // the log's own
    unsigned long long* seq;   // slices fed since the last clear
    unsigned long long* head;  // rows ever appended since the last clear
    // between the launches of one update
    int32_t* cnt;             // [N] episodes world w finishes in this update
    unsigned long long* pos;  // [N] row number of its first one
    int capacity;
    const uint32_t* slot_key;  // [S] the key each pool slot was generated from while replay is armed (cagym_replay.h), else NULL
};

#define EPLOG_NT_SCAN 1024 /* lanes of the single scan workgroup */
#define EPLOG_CNT_WAVES 16 /* waves per workgroup of the count pass, each on its own slices */

// grid = ceil(N / 64), 64 x EPLOG_CNT_WAVES lanes: wave y sums the slices y, y + EPLOG_CNT_WAVES, ... of 64 worlds (one lane per
// world: a slice's 64 bytes are contiguous), the waves' sums meet in LDS and wave 0 adds them up
__global__ void __launch_bounds__(CAGYM_WAVE * EPLOG_CNT_WAVES) k_episode_log_count(EpLog G, int N, const uint8_t* __restrict__ game_over, int T) {
    __shared__ int part[EPLOG_CNT_WAVES][CAGYM_WAVE];
    const int lane = threadIdx.x & (CAGYM_WAVE - 1), y = threadIdx.x >> 6, w = blockIdx.x * CAGYM_WAVE + lane;
    int c = 0;
    if (w < N)
        for (int t = y; t < T; t += EPLOG_CNT_WAVES) c += game_over[(size_t)t * N + w] != 0;
    part[y][lane] = c;
    __syncthreads();
    if (y != 0 || w >= N) return;
    int sum = 0;
    for (int k = 0; k < EPLOG_CNT_WAVES; k++) sum += part[k][lane];
    G.cnt[w] = sum;
}

// grid = 1, EPLOG_NT_SCAN lanes.  go1: the game_over of a one-slice update (the counts are its bytes), else null (G.cnt).
__global__ void __launch_bounds__(EPLOG_NT_SCAN) k_episode_log_scan(EpLog G, int N, int T, const uint8_t* __restrict__ go1) {
    __shared__ unsigned wsum[EPLOG_NT_SCAN / CAGYM_WAVE];
    const int lane = threadIdx.x & (CAGYM_WAVE - 1), wave = threadIdx.x >> 6;
    const unsigned long long head0 = *G.head;  // written by thread 0 behind the last barrier only
    unsigned long long carry = 0;              // the same in every lane
    for (int base = 0; base < N; base += EPLOG_NT_SCAN) {
        const int w = base + (int)threadIdx.x;
        unsigned c = 0;
        if (w < N) c = go1 ? (unsigned)(go1[w] != 0) : (unsigned)G.cnt[w];
        unsigned x = c;  // inclusive scan inside the wave
        for (int d = 1; d < CAGYM_WAVE; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == CAGYM_WAVE - 1) wsum[wave] = x;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int k = 0; k < EPLOG_NT_SCAN / CAGYM_WAVE; k++) {
            const unsigned s = wsum[k];
            before += k < wave ? s : 0u;
            total += s;
        }
        if (w < N) G.pos[w] = head0 + carry + before + (x - c);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *G.head = head0 + carry;
        *G.seq += (unsigned long long)T;
    }
}

// grid = ceil(ceil(N / (64 / M)) / 4), EPREC_NT lanes (the recorder's one-writer geometry)
__global__ void __launch_bounds__(EPREC_NT) k_episode_log_write(CagymDev D, EpLog G, const uint8_t* __restrict__ flags,
                                                                const float* __restrict__ reward, const uint8_t* __restrict__ game_over,
                                                                int T) {
    const int M = D.M;
    const EpLane L = eprec_lane(D.N, M, blockIdx.x * (EPREC_NT / CAGYM_WAVE) + (threadIdx.x >> 6));
    const unsigned long long head = *G.head, seq0 = *G.seq - (unsigned long long)T, cap = (unsigned long long)G.capacity;
    EpRun R{};
    unsigned long long pos = 0;
    if (L.valid) {
        R = eprec_load(G.run, L, M);
        pos = G.pos[L.world];
    }
    for (int t = 0; t < T; t++) {
        uint32_t f = 0;
        bool go = false;
        if (L.valid) {
            f = eprec_advance(D, L, R, flags, reward, (size_t)t);
            go = game_over[(size_t)t * D.N + L.world] != 0;
        }
        if (__ballot(go) == 0ull) continue;  // wave-uniform
        const bool write = go && head - pos <= cap;  // among the last `capacity` rows ever appended (pos < head)
        const EpRow W = eprec_row(D, L, R, go, write, f);
        if (write) {
            const size_t r = (size_t)(pos % cap), k = r * M + L.slot;
            G.t[k] = W.t;
            G.extra_t[k] = W.extra;
            G.flags[k] = W.fb;
            if (L.slot == 0) {
                G.key[r] = G.slot_key ? G.slot_key[W.s] : (uint32_t)L.world + (uint32_t)R.cursor * (uint32_t)D.N;
                G.world[r] = L.world;
                G.episode[r] = R.cursor;
                G.slice[r] = (long long)(seq0 + (unsigned long long)t);
                G.steps[r] = R.steps;
                G.ret[r] = R.ret;
                G.outcome[r] = W.outcome;
                G.n_agents[r] = W.n;
                G.n_obst[r] = D.sc_nobst[W.s];
            }
        }
        if (go) {
            pos += 1;
            eprec_next(R);
        }
    }
    eprec_check(D, G.run, L, R);
    eprec_store(G.run, L, M, R);
}

// eprec_forget; clear_rows: every row of the ring, head, the slice counter and desync as cagym_episode_log_init leaves them.
// Grid-stride over max(N, capacity) * M.
__global__ void __launch_bounds__(256) k_episode_log_restart(CagymDev D, EpLog G, const uint8_t* __restrict__ world_mask, int clear_rows) {
    const size_t LM = (size_t)G.capacity * D.M, stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    eprec_forget(D, G.run, world_mask, i0, stride);
    if (!clear_rows) return;
    for (size_t i = i0; i < LM; i += stride) {
        G.t[i] = 0.0;
        G.extra_t[i] = 0.0;
        G.flags[i] = 0;
        if (i < (size_t)G.capacity) {
            G.key[i] = 0u;
            G.world[i] = 0;
            G.episode[i] = 0;
            G.slice[i] = 0;
            G.steps[i] = 0;
            G.ret[i] = 0.0;
            G.outcome[i] = 0;
            G.n_agents[i] = 0;
            G.n_obst[i] = 0;
        }
    }
    if (i0 == 0) {
        *G.run.desync = 0;
        *G.seq = 0ull;
        *G.head = 0ull;
    }
}
