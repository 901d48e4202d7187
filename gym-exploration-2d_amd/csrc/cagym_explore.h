// cagym_explore.h -- exploration worlds on the device (include/cagym.h: cagym_generate_exploration_scenarios, cagym_stream_exploration_*):
// a team of R IG robots and T static targets among the stage samplers' rectangles, the stream of such worlds, and the distance
// fields of the refilled slots rebuilt behind the refill.
// A world is cagym_gen2.h's stage scenario for an internal parameter set (explore_validate, cagym_api.hip) followed by the team
// edit below; nothing new is drawn.  The stream is cagym_stream.h's ring with the edit applied to every regenerated row.
// The field refresh is three launches chained by the stream, and no workgroup reads what another wrote inside one launch:
//   k_explore_field_list   per world, the slots that were regenerated and not rebuilt -> a compact list (one atomic per wave)
//   k_explore_field_cols   EDT pass 1 of the listed slots, one slot per workgroup turn
//   k_explore_field_rows   EDT pass 2, one row of a listed slot per workgroup turn
// The list's length is zeroed by k_explore_refill, the launch in front of them.  Included by cagym_api.hip only.
#pragma once
#include "cagym_gen2.h"
#include "cagym_ig.h"
#include "cagym_sensors.h"
#include "cagym_stream.h"

struct ExploreTeam {
    int R, T;  // robots in slots 0..R-1, targets in slots R..R+T-1
    double target_radius, robot_pref_speed;
};

struct ExploreDev {
    int32_t* field_next;               // [N] first episode of world w whose slot has been regenerated but whose field has not been rebuilt
    unsigned long long* fields_built;  // slots rebuilt since the stream started
    int32_t* n_list;                   // length of `list` (zeroed by k_explore_refill, appended to by k_explore_field_list)
    int32_t* list;                     // [S - N] pool slots to rebuild
    int cap;                           // S - N: a world's window holds at most depth - 1 slots
};

// the team edit of pool row s: robots first (the reference's ig_mcts indexes the team by slot), then the targets
__device__ __forceinline__ void explore_team_edit(const Gen2Dev& D, const ExploreTeam& Tm, uint32_t s) {
    const int M = D.G.M;
    for (int i = 0; i < Tm.R + Tm.T && i < M; i++) {
        const size_t a = (size_t)s * M + i;
        if (i < Tm.R) {
            D.G.policy[a] = CAGYM_POL_IGMCTS;
            D.G.dyn[a] = CAGYM_DYN_FIRSTORDER;
            D.G.agents6[a * 6 + 4] = Tm.robot_pref_speed;
        } else {
            D.G.policy[a] = CAGYM_POL_STATIC;
            D.G.agents6[a * 6 + 5] = Tm.target_radius;
        }
    }
}

__device__ __forceinline__ int explore_scenario(const Gen2Dev& D, const cagym_gen2_params& P, const ExploreTeam& Tm, uint32_t v, uint32_t s) {
    const int failed = gen2_scenario(D, P, v, s);
    explore_team_edit(D, Tm, s);
    return failed;
}

__global__ void __launch_bounds__(64) k_generate_exploration_scenarios(Gen2Dev D, cagym_gen2_params P, ExploreTeam Tm, int32_t* n_failed) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= D.G.S) return;
    const int failed = explore_scenario(D, P, Tm, (uint32_t)s, (uint32_t)s);
    if (failed) atomicAdd(n_failed, failed);
}

// k_stream_refill (cagym_stream.h: same windows, same counters, same idle exit) with the team edit behind every sampled row.  Its
// first lane also empties the field refresh's work list: no other workgroup of this launch touches that word.
__global__ void __launch_bounds__(64) k_explore_refill(Gen2Dev D, cagym_gen2_params P, ExploreTeam Tm, StreamDev T, int32_t* n_list) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_list = 0;
    const int w = blockIdx.x * CAGYM_WAVE + threadIdx.x;
    const bool valid = w < T.N;
    const int ep = valid ? T.episode[w] : 0;
    const int nx = valid ? T.next_episode[w] : T.depth;
    const int last = ep + T.depth - 1;
    const bool lapped = valid && nx <= ep;
    const int first = nx > ep + 1 ? nx : ep + 1;
    const bool work = valid && first <= last;
    if (__ballot(work) == 0ull) return;
    int failed = 0, made = 0;
    if (work) {
        for (int e = first; e <= last; e++) {
            const long long idx = (long long)w + (long long)e * T.N;
            failed += explore_scenario(D, P, Tm, (uint32_t)idx, (uint32_t)(idx % D.G.S));
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

// ---- the field refresh ------------------------------------------------------------------------------------------------------------
// One lane per world, one wave per workgroup.  World w's window is episodes max(field_next, episode + 1) .. next_episode - 1 (the
// slot of its current episode is never listed, as the refill never writes it); then field_next = next_episode.  A wave without work
// leaves after its three loads.  The window's episodes are fewer than depth and consecutive, so its slots are distinct, and slot r
// belongs to world r % N: every listed slot is listed once.
__global__ void __launch_bounds__(64) k_explore_field_list(StreamDev T, ExploreDev X, int S) {
    const int w = blockIdx.x * CAGYM_WAVE + threadIdx.x;
    const bool valid = w < T.N;
    const int ep = valid ? T.episode[w] : 0;
    const int nx = valid ? T.next_episode[w] : 0;
    const int fn = valid ? X.field_next[w] : 0;
    int lo = fn > ep + 1 ? fn : ep + 1;
    const int hi = nx - 1;
    if (lo < hi - (T.depth - 2)) lo = hi - (T.depth - 2);  // at most depth - 1 slots (it is what the refill's window leaves anyway)
    const int n = (valid && lo <= hi) ? hi - lo + 1 : 0;
    if (__ballot(n > 0) == 0ull) return;
    // exclusive prefix sum of n over the wave, then one atomic for the wave's room in the list
    int incl = n;
#pragma unroll
    for (int d = 1; d < CAGYM_WAVE; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if ((int)threadIdx.x >= d) incl += up;
    }
    const int total = __builtin_amdgcn_readlane(incl, CAGYM_WAVE - 1);
    int base = 0;
    if (threadIdx.x == 0) {
        base = atomicAdd(X.n_list, total);
        atomicAdd(X.fields_built, (unsigned long long)total);
    }
    base = __builtin_amdgcn_readfirstlane(base) + incl - n;
    for (int j = 0; j < n; j++)
        if (base + j < X.cap) X.list[base + j] = (int)(((long long)w + (long long)(lo + j) * T.N) % S);
    if (valid && nx > fn) X.field_next[w] = nx;
}

// EDT pass 1 of the listed slots: a fixed grid strides over the list, one slot per turn.  ig_any[s] is rewritten whole (a plain
// store of the workgroup's OR), which is the zeroing the whole-pool kernel leaves to a memset.
__global__ void __launch_bounds__(320) k_explore_field_cols(IgDev G, ExploreDev X, uint32_t* any_flag) {
    __shared__ uint32_t lm[CAGYM_MAPD * CAGYM_MAPW];
    int n = *X.n_list;
    n = n < X.cap ? n : X.cap;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int s = X.list[i];
        const bool any = ig_edt_cols_slot(G, s, threadIdx.x, lm);
        const int wg_any = __syncthreads_or(any);  // (also: every thread is done with lm before the next turn overwrites it)
        if (threadIdx.x == 0) any_flag[s] = wg_any ? 1u : 0u;
    }
}

// EDT pass 2: the 300 rows of every listed slot are the work items, one row per workgroup turn, so a slot's rows spread over the grid.
__global__ void __launch_bounds__(320) k_explore_field_rows(IgDev G, ExploreDev X, const uint32_t* any_flag) {
    __shared__ uint32_t g2[CAGYM_MAPD];
    int n = *X.n_list;
    n = n < X.cap ? n : X.cap;
    const long long items = (long long)n * CAGYM_MAPD;
    for (long long i = blockIdx.x; i < items; i += gridDim.x) {
        const int s = X.list[i / CAGYM_MAPD], y = (int)(i % CAGYM_MAPD);
        ig_edt_row(G, s, y, threadIdx.x, any_flag[s] != 0, g2);
    }
}
