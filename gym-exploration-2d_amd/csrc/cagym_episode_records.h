// cagym_episode_records.h -- per-scenario episode records rebuilt from the step outputs (include/cagym.h:
// cagym_episode_records_*).  The reference reads them from env.prev_episode_agents at the end of an episode
// (experiments/src/env_utils.py:41-62); under auto-reset the step kernels re-initialise a finished world inside the launch that
// finished it, so this recorder sits BESIDE them and consumes what they wrote: flags [T,N,M], reward [T,N,M], game_over [T,N].
//
// Those outputs and the scenario pool determine every recorded quantity:
//   Agent.t (agent.py:147-159, 184-186): t = 0 at the start of an episode; every step t += dt, unless the agent's AT_GOAL bit was
//     set in the flags of the previous step of the same episode (a done agent that is not at its goal keeps counting);
//   extra_t = t - (|start - goal| - 0.75) / pref_speed (agent.py:59, env_utils.py:54), from the pool's row like init_agent;
//   the terminal flags byte, the return (score += rew[0], fp64), the step count and the outcome bits (env_utils.py:55-60).
// Slots at or above the pool's n_agents[s] are masked with the pool's count: the flags buffer is never trusted for them.
//
// One lane per (world, slot), 64 / M worlds per wave (a world never straddles a wave, as in the step kernels), per-world
// reductions by 64-bit ballots.  Lane l of wave g owns flat agent g * (64 / M) * M + l: the loads of one slice are contiguous
// across the lanes of a wave and across the waves of a workgroup.
//
// Two worlds may finish the same scenario only when S is not a multiple of N (s = (w + e N) % S, so s % N == w otherwise):
//   k_episode_records_update         S % N == 0: every row has one writer; the running values stay in registers over the T slices;
//   k_episode_records_update_shared  any S: ONE workgroup walks the slices in order with two barriers per slice.  Every finishing
//     episode posts the key (slice number since the last clear) * N + world + 1 on its row with a 64-bit atomic min (keep first)
//     or max (keep last); behind the barrier the episode whose key the row holds writes all columns, every finisher counts.
//     The winner is therefore the first (last) episode in (slice, world) order however the slices are cut into launches.
// No waits, no locks: the only cross-lane dependencies are ballots, shuffles and __syncthreads reached by every wave.
#pragma once
#include "cagym_device.h"

// the episode in progress of every world, [N, ...] (t_run [N, M]), and the desync word: the recorder and the log each keep their own
struct EpRunning {
    double *t_run, *ret_run;
    int32_t* steps_run;
    uint32_t* atgoal_run;
    int32_t* cursor;
    int32_t* desync;
};

struct EpRec {
    // table [S, ...]
    double *t, *extra_t;
    uint8_t* flags;
    double* ret;
    int32_t *steps, *outcome, *count;
    unsigned long long* claim;  // [S] key of the episode that owns the row (shared kernel only)
    EpRunning run;
    unsigned long long* seq;  // slices fed since the last clear (shared kernel only)
    int keep;                 // CAGYM_EPREC_KEEP_*
};

#define EPREC_NT 256          /* lanes per workgroup of the one-writer kernel */
#define EPREC_NT_SHARED 1024  /* ... of the ordered single-workgroup kernel */

struct EpLane {
    int world, slot, base;
    bool valid;
    uint64_t wm;  // the world's lanes
};
__device__ __forceinline__ EpLane eprec_lane(int N, int M, int group) {
    const int lane = threadIdx.x & (CAGYM_WAVE - 1), wpw = CAGYM_WAVE / M, wl = lane / M;
    EpLane L;
    L.slot = lane - wl * M;
    L.world = group * wpw + wl;
    L.base = wl * M;
    L.valid = wl < wpw && L.world < N;
    L.wm = L.valid ? ((1ull << M) - 1ull) << L.base : 0ull;  // M <= 32
    return L;
}

// a lane's running values (ret: slot 0 only)
struct EpRun {
    double t, ret;
    int steps, cursor;
    bool atgoal;
};
__device__ __forceinline__ EpRun eprec_load(const EpRunning& E, const EpLane& L, int M) {
    EpRun R;
    R.t = E.t_run[(size_t)L.world * M + L.slot];
    R.ret = E.ret_run[L.world];
    R.steps = E.steps_run[L.world];
    R.cursor = E.cursor[L.world];
    R.atgoal = (E.atgoal_run[L.world] >> L.slot) & 1u;
    return R;
}
// every lane of the wave calls this (ballot); invalid lanes store nothing
__device__ __forceinline__ void eprec_store(const EpRunning& E, const EpLane& L, int M, const EpRun& R) {
    const uint64_t b = __ballot(L.valid && R.atgoal);
    if (!L.valid) return;
    E.t_run[(size_t)L.world * M + L.slot] = R.t;
    if (L.slot == 0) {
        E.ret_run[L.world] = R.ret;
        E.steps_run[L.world] = R.steps;
        E.cursor[L.world] = R.cursor;
        E.atgoal_run[L.world] = (uint32_t)((b & L.wm) >> L.base);
    }
}

// one slice of a valid lane; returns its flags byte
__device__ __forceinline__ uint32_t eprec_advance(const CagymDev& D, const EpLane& L, EpRun& R, const uint8_t* __restrict__ flags,
                                                  const float* __restrict__ reward, size_t slice) {
    const size_t idx = (slice * (size_t)D.N + L.world) * D.M + L.slot;
    const uint32_t f = flags[idx];
    if (!R.atgoal) R.t += D.dt;
    R.atgoal = (f & CAGYM_FLAG_AT_GOAL) != 0;
    R.steps += 1;
    if (L.slot == 0) R.ret += (double)reward[idx];
    return f;
}

__device__ __forceinline__ int eprec_scenario(const CagymDev& D, int world, int cursor) {
    return (int)(((long long)world + (long long)cursor * D.N) % D.S);
}

// A finished episode's row as the lanes of its world hold it: the pool slot and its agent count, the outcome bits (every lane of
// the world), and this lane's t / extra_t / flags byte (zeros at or above n).  Computing it and storing it are separate so that the
// per-slot table here and the append-only log (cagym_episode_log.h) hold the same doubles.
struct EpRow {
    int s, n, outcome;
    double t, extra;
    uint8_t fb;
};
// Called by EVERY lane of a wave in which some world's game_over fired (go: this lane's world did).  full: this lane's t / extra_t
// are wanted (the row will be stored); otherwise only s, n and the outcome bits are computed.
__device__ __forceinline__ EpRow eprec_row(const CagymDev& D, const EpLane& L, const EpRun& R, bool go, bool full, uint32_t f) {
    EpRow W{};
    if (go) {
        W.s = eprec_scenario(D, L.world, R.cursor);
        W.n = D.sc_nagents[W.s];
    }
    const bool active = go && L.slot < W.n;
    const bool coll = (f & CAGYM_FLAG_IN_COLLISION) != 0, goal = (f & CAGYM_FLAG_AT_GOAL) != 0;
    const uint64_t b_coll = __ballot(active && coll) & L.wm;
    const uint64_t b_notgoal = __ballot(active && !goal) & L.wm;
    const uint64_t b_neither = __ballot(active && !coll && !goal) & L.wm;
    W.outcome = (b_coll ? 1 : 0) | (b_notgoal ? 0 : 2) | (b_neither ? 4 : 0);
    if (active && full) {
        const double* s6 = D.sc_agents6 + ((size_t)W.s * D.M + L.slot) * 6;
        W.t = R.t;
        W.extra = W.t - (norm2(s6[0] - s6[2], s6[1] - s6[3]) - 0.75) / s6[4];  // agent.py:59, as init_agent states it
        W.fb = (uint8_t)f;
    }
    return W;
}
// the running values of a world whose episode ended: zeroes, cursor += 1
__device__ __forceinline__ void eprec_next(EpRun& R) {
    R.t = 0.0;
    R.ret = 0.0;
    R.steps = 0;
    R.atgoal = false;
    R.cursor += 1;
}

// The end of an episode, called by EVERY lane of a wave in which some world's game_over fired (go: this lane's world did).
// write: this episode owns the row (decided by the caller for the lanes with go).  Zeroes the running values, cursor += 1.
__device__ __forceinline__ void eprec_finish(const CagymDev& D, const EpRec& E, const EpLane& L, EpRun& R, bool go, bool write, uint32_t f) {
    const EpRow W = eprec_row(D, L, R, go, write, f);
    if (!go) return;
    if (write) {
        const size_t k = (size_t)W.s * D.M + L.slot;
        E.t[k] = W.t;
        E.extra_t[k] = W.extra;
        E.flags[k] = W.fb;
        if (L.slot == 0) {
            E.ret[W.s] = R.ret;
            E.steps[W.s] = R.steps;
            E.outcome[W.s] = W.outcome;
        }
    }
    eprec_next(R);
}

// After the last slice: the recorder's episode index and step count against the ones the step kernels keep.  A skipped, doubled
// or non-auto-reset step shows here: count it, take the handle's values and drop the world's running values.
__device__ __forceinline__ void eprec_check(const CagymDev& D, const EpRunning& E, const EpLane& L, EpRun& R) {
    if (!L.valid) return;
    const int ep = D.episode[L.world], len = D.ep_len[L.world];
    if (R.cursor == ep && R.steps == len) return;
    if (L.slot == 0) atomicAdd(E.desync, 1);
    R.cursor = ep;
    R.steps = len;
    R.t = 0.0;
    R.ret = 0.0;
    R.atgoal = false;
}

// S % N == 0: one writer per row.  grid = ceil(ceil(N / (64 / M)) / 4), EPREC_NT lanes.
__global__ void __launch_bounds__(EPREC_NT) k_episode_records_update(CagymDev D, EpRec E, const uint8_t* __restrict__ flags,
                                                                     const float* __restrict__ reward,
                                                                     const uint8_t* __restrict__ game_over, int T) {
    const int M = D.M;
    const EpLane L = eprec_lane(D.N, M, blockIdx.x * (EPREC_NT / CAGYM_WAVE) + (threadIdx.x >> 6));
    EpRun R{};
    if (L.valid) R = eprec_load(E.run, L, M);
    for (int t = 0; t < T; t++) {
        uint32_t f = 0;
        bool go = false;
        if (L.valid) {
            f = eprec_advance(D, L, R, flags, reward, (size_t)t);
            go = game_over[(size_t)t * D.N + L.world] != 0;
        }
        if (__ballot(go) == 0ull) continue;  // wave-uniform
        // the row's finished episodes so far: read and bumped by slot 0, told to the world's lanes
        int cnt = 0;
        if (go && L.slot == 0) {
            const int s = eprec_scenario(D, L.world, R.cursor);
            cnt = E.count[s];
            E.count[s] = cnt + 1;
        }
        cnt = __shfl(cnt, L.base);
        eprec_finish(D, E, L, R, go, E.keep == CAGYM_EPREC_KEEP_LAST || cnt == 0, f);
    }
    eprec_check(D, E.run, L, R);
    eprec_store(E.run, L, M, R);
}

// any S: one workgroup, slices in order, rows owned by key (see the head of this file).  grid = 1, EPREC_NT_SHARED lanes.
__global__ void __launch_bounds__(EPREC_NT_SHARED) k_episode_records_update_shared(CagymDev D, EpRec E, const uint8_t* __restrict__ flags,
                                                                                   const float* __restrict__ reward,
                                                                                   const uint8_t* __restrict__ game_over, int T) {
    const int M = D.M, wpw = CAGYM_WAVE / M, ngroups = (D.N + wpw - 1) / wpw;
    const int wave = threadIdx.x >> 6, nwaves = EPREC_NT_SHARED / CAGYM_WAVE;
    const unsigned long long seq0 = *E.seq;  // written by thread 0 behind the last barrier only
    const bool last = E.keep == CAGYM_EPREC_KEEP_LAST;
    for (int t = 0; t < T; t++) {
        // phase 1: the slice into the running values; finishing episodes post their keys
        for (int g = wave; g < ngroups; g += nwaves) {
            const EpLane L = eprec_lane(D.N, M, g);
            EpRun R{};
            if (L.valid) {
                R = eprec_load(E.run, L, M);
                eprec_advance(D, L, R, flags, reward, (size_t)t);
                if (L.slot == 0 && game_over[(size_t)t * D.N + L.world]) {
                    const int s = eprec_scenario(D, L.world, R.cursor);
                    const unsigned long long key = (seq0 + (unsigned long long)t) * (unsigned long long)D.N + (unsigned long long)L.world + 1ull;
                    if (last) atomicMax(&E.claim[s], key);
                    else atomicMin(&E.claim[s], key);
                }
            }
            eprec_store(E.run, L, M, R);
        }
        __syncthreads();
        // phase 2: the owner of a row writes it, every finisher counts
        for (int g = wave; g < ngroups; g += nwaves) {
            const EpLane L = eprec_lane(D.N, M, g);
            const bool go = L.valid && game_over[(size_t)t * D.N + L.world] != 0;
            if (__ballot(go) == 0ull) continue;  // wave-uniform
            EpRun R{};
            uint32_t f = 0;
            bool write = false;
            if (go) {
                R = eprec_load(E.run, L, M);
                f = flags[((size_t)t * D.N + L.world) * M + L.slot];
                const int s = eprec_scenario(D, L.world, R.cursor);
                const unsigned long long key = (seq0 + (unsigned long long)t) * (unsigned long long)D.N + (unsigned long long)L.world + 1ull;
                // (device-scope load: the keys were posted by atomics, which are performed in L2, past this CU's vector cache)
                write = __hip_atomic_load(&E.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key;
                if (L.slot == 0) atomicAdd(&E.count[s], 1);
            }
            eprec_finish(D, E, L, R, go, write, f);
            EpLane Ls = L;  // only the worlds that finished changed
            Ls.valid = go;
            eprec_store(E.run, Ls, M, R);
        }
        __syncthreads();
    }
    for (int g = wave; g < ngroups; g += nwaves) {
        const EpLane L = eprec_lane(D.N, M, g);
        EpRun R{};
        if (L.valid) R = eprec_load(E.run, L, M);
        eprec_check(D, E.run, L, R);
        eprec_store(E.run, L, M, R);
    }
    if (threadIdx.x == 0) *E.seq = seq0 + (unsigned long long)T;
}

// The masked worlds (null = all) forget the episode in progress and take the handle's episode index: the first loop of both restart
// kernels, grid-stride over N * M from i0.
__device__ __forceinline__ void eprec_forget(const CagymDev& D, const EpRunning& E, const uint8_t* __restrict__ world_mask, size_t i0, size_t stride) {
    const size_t NM = (size_t)D.N * D.M;
    for (size_t i = i0; i < NM; i += stride) {
        const size_t w = i / D.M;
        if (world_mask && !world_mask[w]) continue;
        E.t_run[i] = 0.0;
        if (i - w * D.M == 0) {
            E.ret_run[w] = 0.0;
            E.steps_run[w] = 0;
            E.atgoal_run[w] = 0u;
            E.cursor[w] = D.episode[w];
        }
    }
}

// eprec_forget; clear_table: every row, the keys, the slice counter and desync as cagym_episode_records_init leaves them.
// Grid-stride over max(N, S) * M.
__global__ void __launch_bounds__(256) k_episode_records_restart(CagymDev D, EpRec E, const uint8_t* __restrict__ world_mask, int clear_table) {
    const size_t SM = (size_t)D.S * D.M, stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    eprec_forget(D, E.run, world_mask, i0, stride);
    if (!clear_table) return;
    for (size_t i = i0; i < SM; i += stride) {
        E.t[i] = 0.0;
        E.extra_t[i] = 0.0;
        E.flags[i] = 0;
        if (i < (size_t)D.S) {
            E.ret[i] = 0.0;
            E.steps[i] = 0;
            E.outcome[i] = 0;
            E.count[i] = 0;
            E.claim[i] = E.keep == CAGYM_EPREC_KEEP_LAST ? 0ull : ~0ull;
        }
    }
    if (i0 == 0) {
        *E.run.desync = 0;
        *E.seq = 0ull;
    }
}
