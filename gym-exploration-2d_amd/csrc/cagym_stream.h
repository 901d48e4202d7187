// cagym_stream.h -- fresh scenarios streamed into the pool behind auto-resetting steps (include/cagym.h: cagym_stream_*).
// The pool of S = k * N slots is a ring of depth k per world: world w owns slots w, w + N, ..., w + (k - 1) N, and slot
// (w + e * N) % S holds the scenario of its episode e, drawn by cagym_gen2.h's samplers from stream key (uint32)(w + e * N).
// k_stream_refill runs behind the step launches and writes the slots of the episodes a world has not reached yet; the step, reset
// and roll-out kernels do not know of it (they keep deriving the slot from episode[w]).  S % N == 0 gives every slot one writer,
// slot r belongs to world r % N, and the slot of a world's current episode is never written.  Included by cagym_api.hip only.
#pragma once
#include "cagym_gen2.h"
#include "cagym_sensors.h"

struct StreamDev {
    int32_t* next_episode;              // [N] first episode of world w whose slot has not been generated
    unsigned long long* generated;      // slots generated since the stream started (the first fill included)
    int32_t* n_failed;                  // agents and rectangles whose rejection loop hit max_tries, since the stream started
    int32_t* n_lapped;                  // times a world started an episode on a slot that had not been refilled
    const int32_t* episode;             // [N] CagymDev::episode
    uint32_t* map_bits;                 // [S, 300, 10] or NULL (max_obstacles == 0)
    int N, depth;
};

__device__ __forceinline__ int stream_wave_sum(int x) {  // every lane of the wave makes the call
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// One lane per world, one wave per workgroup.  A wave none of whose worlds finished an episode since the last refill - the common
// case behind a one-step launch - leaves after its two loads.  Otherwise the lanes with work run the samplers for their episodes
// max(next_episode, episode + 1) .. episode + depth - 1; after a workgroup barrier (the rows the samplers wrote are visible to the
// whole wave) the wave rasterises those slots together, all 64 lanes on each slot's 300 x 10 words.  One atomic per wave and counter.
__global__ void __launch_bounds__(64) k_stream_refill(Gen2Dev D, cagym_gen2_params P, StreamDev T) {
    const int w = blockIdx.x * CAGYM_WAVE + threadIdx.x;
    const bool valid = w < T.N;  // (the tail lanes of the last wave stay: they take part in the barriers and the rasteriser)
    const int ep = valid ? T.episode[w] : 0;
    const int nx = valid ? T.next_episode[w] : T.depth;
    const int last = ep + T.depth - 1;
    const bool lapped = valid && nx <= ep;  // its current episode runs on a slot that was never refilled: counted, the slot left alone
    const int first = nx > ep + 1 ? nx : ep + 1;
    const bool work = valid && first <= last;
    if (__ballot(work) == 0ull) return;  // wave-uniform (lapped implies work)
    int failed = 0, made = 0;
    if (work) {
        for (int e = first; e <= last; e++) {
            const long long idx = (long long)w + (long long)e * T.N;
            failed += gen2_scenario(D, P, (uint32_t)idx, (uint32_t)(idx % D.G.S));  // the key wraps at 2^32, the slot is the step kernels'
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
    const int f = stream_wave_sum(failed), m = stream_wave_sum(made), lp = __popcll(__ballot(lapped));
    if (threadIdx.x == 0) {
        atomicAdd(T.generated, (unsigned long long)m);
        if (f) atomicAdd(T.n_failed, f);
        if (lp) atomicAdd(T.n_lapped, lp);
    }
}
