// cagym_ig_episode.h -- the episode boundary of the information-gathering team (include/cagym.h: cagym_ig_episode_boundary).
//
// What an IG world carries from one env step to the next, and therefore what a per-world restart has to put back:
//   - the belief grid and its MI cache (IgDev::belief / ::mi): back to the prior, with the doubles of k_ig_fill_belief
//     (ig_fill_world_prior is the one statement of them);
//   - the plans its robots communicated (DmPublished, kept across planning steps like policy.best_paths): the next planning
//     step's cycle 0 must hear nothing (the reference's DummyVecEnv reset() builds new ig_mcts objects: a new targetMap, no
//     best_paths);
//   - the team reward's episode bookkeeping (running / sum / last / episodes below).
// Nothing else of the planner survives a planning step.  Checked against cagym_dmcts.h: k_dmcts_plan runs dm_init_tree for every
// robot before its first cycle, and k_dmcts_plan_cycle runs it in the launch of cycle 0 - that rewrites the root, the node and
// mask counters (nn) and the LDS distribution row; every node, mask-pool entry and MU value that is read afterwards was written by
// dm_expand / dm_materialise / dm_grow behind it (the counters bound every read).  DmDist is written at the end of every launch
// but the last and read only by launches of cycle > 0, i.e. always behind a write of the same planning step.  The distance fields
// are per scenario and follow IgDev::episode, which cagym_step_autoreset advances inside its launch.  The generator keys run on
// the handle-wide call_base, as the host planner's self.calls does: a restart does not rewind them.
//
// The two publication buffers: both modes leave a planning step's publications in the first buffer (`pub`) and read them there at
// the next call - the agent-parallel mode's second buffer is a copy of the first (odd Ncycles) or fully rewritten by cycle 0 before
// anything reads it (even Ncycles).  Clearing a world's R entries in `pub` is therefore what makes it hear nothing, in either mode
// and across a mode switch; the second buffer's entries are cleared as well where the workspace holds one, so that a restarted
// world's part of the workspace is byte for byte what reset_comms leaves.
//
// One workgroup per world, one writer per accumulator: the fp64 sums run in step order without atomics.  Plain vector stores,
// one early exit per workgroup, no waits, no LDS.
#pragma once
#include "cagym_dmcts.h"

// the handle's per-world accumulators of the team reward (cagym_ig_get_episode_stats)
struct IgEpisode {
    double* running;    // [N] sum of team_reward over the steps of the episode in progress
    double* sum;        // [N] sum of the finished episodes' returns
    double* last;       // [N] return of the last finished episode
    int32_t* episodes;  // [N] finished episodes
};

static_assert(sizeof(DmPublished) % sizeof(unsigned long long) == 0, "DmPublished is cleared in 8-byte words");

// flags: CAGYM_IG_EPISODE_* of include/cagym.h
__global__ void __launch_bounds__(256) k_ig_episode_boundary(IgDev G, IgEpisode A, int R, unsigned int flags, const double* __restrict__ team_reward,
                                                             const uint8_t* __restrict__ restart_mask, DmPublished* pub, DmPublished* pub2) {
    const int w = blockIdx.x, tid = threadIdx.x;
    const bool restart = restart_mask && restart_mask[w];  // uniform
    const bool plans_only = flags & 2u;
    if (tid == 0 && !plans_only) {
        double run = A.running[w];
        if (team_reward) run += team_reward[w];  // the terminal step's reward belongs to the episode that ends
        if (restart) {
            if (flags & 1u) {
                A.sum[w] += run;
                A.last[w] = run;
                A.episodes[w] += 1;
            }
            run = 0.0;
        }
        if (team_reward || restart) A.running[w] = run;
    }
    if (!restart) return;
    if (!plans_only) ig_fill_world_prior(G, w, tid, blockDim.x);
    constexpr int WORDS = (int)(sizeof(DmPublished) / sizeof(unsigned long long));
    unsigned long long* p = reinterpret_cast<unsigned long long*>(pub + (size_t)w * R);
    for (int q = tid; q < R * WORDS; q += blockDim.x) p[q] = 0ull;
    if (pub2) {
        unsigned long long* p2 = reinterpret_cast<unsigned long long*>(pub2 + (size_t)w * R);
        for (int q = tid; q < R * WORDS; q += blockDim.x) p2[q] = 0ull;
    }
}
