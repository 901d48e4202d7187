// cagym_terminal.h -- terminal observations and the trajectory ring under auto-reset (include/cagym.h: cagym_step_autoreset_keep,
// cagym_trajectory_*).
// An auto-resetting step overwrites, inside the launch that ended an episode, the observation the agents ended on and the state they
// ended in.  cagym_step_autoreset_keep runs the same step as THREE launches chained by stream order - the plain step, the capture
// kernel below, k_reset(mask = game_over, advance) - which is bit for bit the auto-resetting launch (tests/test_hip_parity.py,
// tests/test_cfg4.py hold that identity).  Between the first and the third launch the terminal observation sits in the caller's
// output buffers and the terminal state in the SoA: k_terminal_capture reads both.  No step, roll-out or reset kernel knows of it.
//
// k_terminal_capture is ONE launch with two kinds of workgroup (the first n_row_wg copy rows, the others write the slice):
//   terminal rows     a wave per world, TCAP_WORLDS worlds in turn: where the world's game_over byte is set its rows of the step's
//                     OtherAgentsStates / ego / laser tables are copied to the same world index of the caller's terminal buffers, as
//                     16-byte accesses where the row size and both bases allow, else as 4-byte words (k_snapshot_copy's rule).  Rows
//                     of worlds that did not finish are not touched.
//   trajectory slice  a lane per agent slot i = w * M + k, so every load of the SoA state and every store to a column plane
//                     rows[slot][c][N*M] is contiguous across the wave.  The row is the reference's global_state_history row
//                     (agent.py:198-201, written after the move and before t += dt): [t_before, px, py, gx, gy, radius, pref_speed,
//                     vx, vy, speed, heading, a0, a1], t_before from the ring's own t_prev, never from t - dt.  The agent moved iff
//                     its step_num differs from the ring's own `seen` (step_num advances on a real move only, agent.py:186): done
//                     agents write nothing, which is dataset.py's history[:step_num] rule.  Then t_prev <- t and seen <- step_num,
//                     or 0 for both where game_over is set (the reset launch that follows zeroes them).  A moved agent whose
//                     step_num is not seen + 1 was stepped past the ring: desync += 1 (a counter nobody reads in the launch), and
//                     the assignment above resynchronises.
// No workgroup waits on another and none reads what another wrote in the launch: the slice counter every slice workgroup needs is
// kept once PER WORKGROUP (head_wg[b], read and advanced by workgroup b alone; they move in lockstep because every launch runs
// them all), and workgroup 0 publishes the public `head` word.
#pragma once
#include "cagym_device.h"

#define TRAJ_COLS 13
#define TCAP_NT 256
#define TCAP_WORLDS 4 /* worlds a wave of the row workgroups walks */

struct TermOut {
    float *obs_oas, *obs_ego, *laserscan;
};

struct TrajRing {
    // ring, L slices
    double* rows;      // [L][13][N*M]
    uint8_t* moved;    // [L][N*M]
    int32_t* episode;  // [L][N]
    uint8_t* last;     // [L][N]
    // words and the ring's own running values
    unsigned long long* head;     // slices ever written; slice i lives at i % L
    int32_t* desync;
    unsigned long long* head_wg;  // [ceil(N*M / TCAP_NT)] the slice workgroups' own copies of head
    double* t_prev;               // [N*M]
    int32_t* seen;                // [N*M]
    int L;
};

inline unsigned tcap_slice_wgs(int N, int M) { return (unsigned)(((size_t)N * M + TCAP_NT - 1) / TCAP_NT); }
inline unsigned tcap_row_wgs(int N) { return (unsigned)((N + (TCAP_NT / CAGYM_WAVE) * TCAP_WORLDS - 1) / ((TCAP_NT / CAGYM_WAVE) * TCAP_WORLDS)); }

// row `w` of a [N, row_words] table of 4-byte words, one wave
__device__ __forceinline__ void tcap_copy_row(const float* __restrict__ src, float* __restrict__ dst, size_t row_words, size_t w, int lane) {
    if (!src || !dst) return;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src) + w * row_words;
    uint32_t* d = reinterpret_cast<uint32_t*>(dst) + w * row_words;
    if ((((row_words * 4) | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        for (size_t c = lane; c < row_words / 4; c += CAGYM_WAVE) reinterpret_cast<uint4*>(d)[c] = reinterpret_cast<const uint4*>(s)[c];
    } else {
        for (size_t c = lane; c < row_words; c += CAGYM_WAVE) d[c] = s[c];
    }
}

// grid = n_row_wg + n_slice_wg (either may be 0), TCAP_NT lanes.  game_over: the step's [N] bytes (never null).
__global__ void __launch_bounds__(TCAP_NT) k_terminal_capture(CagymDev D, CagymOut out, TermOut term, TrajRing R, unsigned n_row_wg) {
    const int N = D.N, M = D.M;
    if (blockIdx.x < n_row_wg) {
        const int lane = threadIdx.x & (CAGYM_WAVE - 1);
        const int w0 = ((int)blockIdx.x * (TCAP_NT / CAGYM_WAVE) + (int)(threadIdx.x >> 6)) * TCAP_WORLDS;
        for (int k = 0; k < TCAP_WORLDS; k++) {
            const int w = w0 + k;
            if (w >= N) return;
            if (!out.game_over[w]) continue;  // wave-uniform
            tcap_copy_row(out.obs_oas, term.obs_oas, (size_t)M * (M - 1) * 10, (size_t)w, lane);
            tcap_copy_row(out.obs_ego, term.obs_ego, (size_t)M * CAGYM_EGO_WIDTH, (size_t)w, lane);
            tcap_copy_row(out.laserscan, term.laserscan, (size_t)M * 16, (size_t)w, lane);
        }
        return;
    }
    __shared__ unsigned long long s_head;
    const unsigned b = blockIdx.x - n_row_wg;
    if (threadIdx.x == 0) s_head = R.head_wg[b];
    __syncthreads();
    const unsigned long long head = s_head;
    const size_t NM = (size_t)N * M, slot = (size_t)(head % (unsigned long long)R.L), i = (size_t)b * TCAP_NT + threadIdx.x;
    if (i < NM) {
        const int w = (int)(i / (size_t)M), k = (int)(i - (size_t)w * M);
        const bool go = out.game_over[w] != 0;
        const int sn = D.step_num[i], se = R.seen[i];
        const bool moved = k < D.n_agents[w] && sn != se;
        R.moved[slot * NM + i] = moved ? 1 : 0;
        if (moved) {
            double* r = R.rows + slot * TRAJ_COLS * NM + i;
            const float2 a = reinterpret_cast<const float2*>(D.action)[i];
            r[0] = R.t_prev[i];
            r[NM] = D.px[i];
            r[2 * NM] = D.py[i];
            r[3 * NM] = D.gx[i];
            r[4 * NM] = D.gy[i];
            r[5 * NM] = D.radius[i];
            r[6 * NM] = D.pref[i];
            r[7 * NM] = D.vx[i];
            r[8 * NM] = D.vy[i];
            r[9 * NM] = D.speed[i];
            r[10 * NM] = D.heading[i];
            r[11 * NM] = (double)a.x;
            r[12 * NM] = (double)a.y;
            if (sn != se + 1) atomicAdd(R.desync, 1);
        }
        R.t_prev[i] = go ? 0.0 : D.t[i];
        R.seen[i] = go ? 0 : sn;
        if (k == 0) {
            R.episode[slot * (size_t)N + w] = D.episode[w];
            R.last[slot * (size_t)N + w] = go ? 1 : 0;
        }
    }
    if (threadIdx.x == 0) {  // behind the barrier above: this workgroup's lanes have the old value
        R.head_wg[b] = head + 1ull;
        if (b == 0) *R.head = head + 1ull;
    }
}

// The masked worlds (null = all) take the current state as the ring's starting point: t_prev <- t, seen <- step_num.
__global__ void __launch_bounds__(256) k_trajectory_restart(CagymDev D, TrajRing R, const uint8_t* __restrict__ world_mask) {
    const size_t NM = (size_t)D.N * D.M, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < NM; i += stride) {
        if (world_mask && !world_mask[i / (size_t)D.M]) continue;
        R.t_prev[i] = D.t[i];
        R.seen[i] = D.step_num[i];
    }
}
