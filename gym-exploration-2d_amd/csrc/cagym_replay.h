// cagym_replay.h -- replay of logged scenarios inside the scenario stream (include/cagym.h: cagym_stream_replay_*).
// A device ring of stream keys (the replay buffer) is filled from the episode log (k_replay_harvest: the rows whose outcome matches a
// mask) or by the caller (k_replay_push); the armed refill (k_stream_refill_replay) decides per slot it generates, by a counter-based
// draw, between the fresh key w + e * N and a key sampled from the buffer with replacement, and records in slot_key / slot_gen [S]
// which key and which parameter generation every slot was really generated from.  Nothing is consumed, so no workgroup waits on
// another; atomics on counters only; everything is ordered by the stream.  k_stream_refill itself (cagym_stream.h) is not touched:
// a handle that never arms replay launches the same kernel as before.  Included by cagym_api.hip only.
#pragma once
#include "cagym_episode_log.h"
#include "cagym_stream.h"

struct ReplayDev {
    uint32_t* buf_key;          // [Q] entry number i since the last clear lives at i % Q
    unsigned long long* words;  // RPW_*: count, harvested, pushed, replayed, n_missed, n_stale, cursor
    uint32_t* buf_gen;          // the parameter generation the buffer belongs to
    uint32_t* slot_key;         // [S] key each slot was generated from
    uint32_t* slot_gen;         // [S] generation each slot was generated under (0: unknown)
    int Q;
};
enum { RPW_COUNT = 0, RPW_HARVESTED, RPW_PUSHED, RPW_REPLAYED, RPW_MISSED, RPW_STALE, RPW_CURSOR, RPW_WORDS };

#define REPLAY_SEED_SALT 0x9E3779B97F4A7C15ull
#define REPLAY_NT 1024 /* lanes of the single harvest / push workgroup */

// One lane per world.  tables: write slot_key / slot_gen of the ring as the plain stream generated it (known: 0 when a parameter
// switch preceded arming - the ring may hold slots of an older set, every slot is unknown); else only the buffer is cleared.
// head: the log's row counter or NULL - rows logged before this launch are never harvested (their slots may have been regenerated).
__global__ void __launch_bounds__(64) k_replay_arm(ReplayDev R, StreamDev T, int S, uint32_t gen, int tables, int known,
                                                   const unsigned long long* __restrict__ head) {
    const int w = blockIdx.x * CAGYM_WAVE + threadIdx.x;
    if (w == 0) {
        for (int i = 0; i < RPW_CURSOR; i++) R.words[i] = 0ull;
        R.words[RPW_CURSOR] = head ? *head : 0ull;
        *R.buf_gen = gen;
    }
    if (w >= T.N || !tables) return;
    const int ep = T.episode[w], nx = T.next_episode[w];
    for (int j = 0; j < T.depth; j++) {
        const int e = ep + j;
        const long long idx = (long long)w + (long long)e * T.N;
        const int slot = (int)(idx % S);
        const bool made = e < nx;  // else not generated (a lapped world's): unknown
        R.slot_key[slot] = made ? (uint32_t)idx : 0u;
        R.slot_gen[slot] = made && known ? gen : 0u;
    }
}

// k_stream_refill with the replay draw: windows, early exit, rasterisation and counters as there.
__global__ void __launch_bounds__(64) k_stream_refill_replay(Gen2Dev D, cagym_gen2_params P, StreamDev T, ReplayDev R, double p, uint64_t seed,
                                                             uint32_t gen) {
    const int w = blockIdx.x * CAGYM_WAVE + threadIdx.x;
    const bool valid = w < T.N;
    const int ep = valid ? T.episode[w] : 0;
    const int nx = valid ? T.next_episode[w] : T.depth;
    const int last = ep + T.depth - 1;
    const bool lapped = valid && nx <= ep;
    const int first = nx > ep + 1 ? nx : ep + 1;
    const bool work = valid && first <= last;
    if (__ballot(work) == 0ull) return;  // wave-uniform
    int failed = 0, made = 0, drawn = 0;
    if (work) {
        const unsigned long long count = R.words[RPW_COUNT], Q = (unsigned long long)R.Q;
        const unsigned long long live = *R.buf_gen == gen ? (count < Q ? count : Q) : 0ull;  // a buffer of another generation is empty
        const uint64_t rs = seed ^ REPLAY_SEED_SALT;
        for (int e = first; e <= last; e++) {
            const long long idx = (long long)w + (long long)e * T.N;
            const uint32_t key32 = (uint32_t)idx, slot = (uint32_t)(idx % D.G.S);
            uint32_t key = key32;
            if (live > 0 && gen_u01(rs, key32, 0) < p) {
                long long j = (long long)(gen_u01(rs, key32, 1) * (double)live);
                j = j > (long long)live - 1 ? (long long)live - 1 : j;
                key = R.buf_key[(count - live + (unsigned long long)j) % Q];
                drawn++;
            }
            failed += gen2_scenario(D, P, key, slot);
            R.slot_key[slot] = key;
            R.slot_gen[slot] = gen;
            made++;
        }
        T.next_episode[w] = ep + T.depth;
    }
    __syncthreads();
    if (T.map_bits) {
        uint64_t todo = __ballot(work);
        while (todo) {
            const int l = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int e0 = __builtin_amdgcn_readlane(first, l), e1 = __builtin_amdgcn_readlane(last, l);
            const long long wl = (long long)blockIdx.x * CAGYM_WAVE + l;
            for (int e = e0; e <= e1; e++)
                rasterize_scenario(D.obst, D.G.nobst, D.K, T.map_bits, (int)((wl + (long long)e * T.N) % D.G.S));
        }
    }
    const int f = stream_wave_sum(failed), m = stream_wave_sum(made), r = stream_wave_sum(drawn), lp = __popcll(__ballot(lapped));
    if (threadIdx.x == 0) {
        atomicAdd(T.generated, (unsigned long long)m);
        if (f) atomicAdd(T.n_failed, f);
        if (lp) atomicAdd(T.n_lapped, lp);
        if (r) atomicAdd(R.words + RPW_REPLAYED, (unsigned long long)r);
    }
}

// grid = 1, REPLAY_NT lanes (k_episode_log_scan's pattern).  Log rows [max(cursor, head - L), head) in ascending row number, chunks
// of REPLAY_NT; accepted rows append slot_key[slot] in row order: a ballot, the prefix inside the wave, an LDS scan across waves.
// A chunk that accepts more than Q rows writes its last Q only (no two lanes on one entry); count still grows by all of them.
__global__ void __launch_bounds__(REPLAY_NT) k_replay_harvest(EpLog G, ReplayDev R, int N, int S, uint32_t mask, uint32_t gen) {
    __shared__ unsigned wacc[REPLAY_NT / CAGYM_WAVE], wstale[REPLAY_NT / CAGYM_WAVE];
    const int lane = threadIdx.x & (CAGYM_WAVE - 1), wave = threadIdx.x >> 6;
    // the words thread 0 writes behind the last barrier
    const unsigned long long head = *G.head, cursor = R.words[RPW_CURSOR], L = (unsigned long long)G.capacity, Q = (unsigned long long)R.Q;
    const unsigned long long count0 = *R.buf_gen == gen ? R.words[RPW_COUNT] : 0ull;  // a buffer of another generation is cleared
    const unsigned long long oldest = head > L ? head - L : 0ull, lo = cursor > oldest ? cursor : oldest;
    unsigned long long carry = 0, stale = 0;  // the same in every lane
    for (unsigned long long base = lo; base < head; base += REPLAY_NT) {
        const unsigned long long row = base + threadIdx.x;
        bool acc = false, old = false;
        uint32_t key = 0;
        if (row < head) {
            const size_t r = (size_t)(row % L);
            const int slot = (int)(((long long)G.world[r] + (long long)G.episode[r] * N) % S);
            const uint32_t sg = R.slot_gen[slot];
            acc = ((uint32_t)G.outcome[r] & mask) != 0u && sg == gen;
            old = sg != 0u && sg != gen;
            key = R.slot_key[slot];
        }
        const uint64_t ba = __ballot(acc), bo = __ballot(old);
        const unsigned pre = (unsigned)__popcll(ba & ((1ull << lane) - 1ull));
        if (lane == 0) {
            wacc[wave] = (unsigned)__popcll(ba);
            wstale[wave] = (unsigned)__popcll(bo);
        }
        __syncthreads();
        unsigned before = 0, total = 0, st = 0;
        for (int k = 0; k < REPLAY_NT / CAGYM_WAVE; k++) {
            const unsigned s = wacc[k];
            before += k < wave ? s : 0u;
            total += s;
            st += wstale[k];
        }
        const unsigned at = before + pre;  // this row's number among the chunk's accepted rows
        if (acc && (unsigned long long)(total - 1u - at) < Q) R.buf_key[(count0 + carry + at) % Q] = key;
        carry += total;
        stale += st;
        __syncthreads();
    }
    __syncthreads();  // (an empty range: every lane has read the words)
    if (threadIdx.x == 0) {
        R.words[RPW_COUNT] = count0 + carry;
        R.words[RPW_HARVESTED] += carry;
        R.words[RPW_MISSED] += lo - cursor;
        R.words[RPW_STALE] += stale;
        R.words[RPW_CURSOR] = head;
        *R.buf_gen = gen;
    }
}

// grid = 1, REPLAY_NT lanes: keys [n] (DEVICE) appended in order; of more than Q keys the last Q are written.
__global__ void __launch_bounds__(REPLAY_NT) k_replay_push(ReplayDev R, const uint32_t* __restrict__ keys, int n, uint32_t gen) {
    const unsigned long long Q = (unsigned long long)R.Q;
    const unsigned long long count0 = *R.buf_gen == gen ? R.words[RPW_COUNT] : 0ull;
    const int i0 = (unsigned long long)n > Q ? n - R.Q : 0;
    for (int i = i0 + (int)threadIdx.x; i < n; i += REPLAY_NT) R.buf_key[(count0 + (unsigned long long)i) % Q] = keys[i];
    __syncthreads();  // every lane has read count and buf_gen
    if (threadIdx.x == 0) {
        R.words[RPW_COUNT] = count0 + (unsigned long long)n;
        R.words[RPW_PUSHED] += (unsigned long long)n;
        *R.buf_gen = gen;
    }
}
