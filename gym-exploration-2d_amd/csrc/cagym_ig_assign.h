// cagym_ig_assign.h -- a TEAM's goals (include/cagym.h: cagym_ig_assign_goals): the sequential-greedy allocation of submodular
// coverage over the robots' candidate goals.  cagym_ig_view_gain / cagym_ig_view_gain_headings / cagym_ig_propose_goals score a robot
// alone; two robots side by side get the same proposals and would look at the same cells, which the team reward counts once.  Here
// every candidate's visible cell set is a 60 x u64 mask, the team claims masks one robot at a time, and every candidate still open is
// re-priced by the mutual information of the cells nobody has claimed yet - the rule ig_greedy(coordinate=True) and Dec-MCTS
// already follow, at the goal layer.
//
// THE RULE (ig.assign_goals_spec is its executable form).  Per world R robots (1..8) with k candidates each (1..16).
//   cell set of a pose: with a finite heading exactly the mask cagym_ig_visible_cells returns for (x, y, heading) at the call's fov
//     and range (ig_visible_box, ig_in_cone, ig_check_visibility); without one (the heading is not finite, or cand_heading is NULL)
//     exactly the cells cagym_ig_view_gain counts at the point: the rectangle cell(p - range) .. cell(p + range), dx dx + dy dy <
//     range range in separate fp64 operations, and the trace.  A point that fails cagym_ig_view_gain's `valid` rule (igv_point:
//     finite, inside the map, edf_at(p) > radius + 0.1) has the empty set.
//   seeding: claimed starts as the union of the cell sets of every robot with claim != 0 and mask == 0 (teammates under way keep
//     what they are going to see); a masked robot's claim byte is ignored.
//   marginal gain of a candidate: the double cagym_ig_mi_reward returns for cells & ~claimed (IgDev::mi summed in ig_reward_block's
//     order at 256 threads, bit for bit).
//   eligible: the point is valid, cand_distance is finite, the marginal gain is > 0.
//   utility: marginal / ((double)distance + d0), one fp64 addition and one fp64 division.
//   mode SLOT (0): the masked robots take turns in slot order; a robot takes its eligible candidate of largest utility, of equal
//     utilities the smaller candidate index, and claimed |= cells; a robot with no eligible candidate gets choice -1 and claims nothing.
//   mode BEST (1): up to R rounds, each taking the eligible (robot, candidate) of largest utility among the masked robots not yet
//     assigned - ties to the smaller slot, then the smaller candidate index; the rounds stop when nothing is eligible.
//   round t is PLAYED when t < the number of masked robots and (BEST) every earlier round assigned a robot; round_gain [round, robot,
//     candidate] holds the marginal gain of every candidate priced in a played round - SLOT: the t-th masked robot's, BEST: every open
//     robot's - and NaN everywhere else (robots assigned or outside the mask, invalid points, non-finite distances, rounds not played).
//   Rows of robots outside the mask keep every byte; a world without a masked robot is neither read nor written, claimed included.
//
// k_ig_assign_goals: one workgroup of 256 threads per world; a world without a masked robot leaves before the first barrier.  The
// world's MI cache goes to LDS once (igv_stage_mi, 28.8 KB).
// Phase 1, the up to R k + R cell sets, one wave per pose round robin.  A set is a set: the order in which its cells are tested does
// not matter, so the rectangle's (the cone's box's) rows are dealt 64 / width at a time - 3 rows of 21 cells at range 5 - and ONE
// ballot per trip holds whole row words, which lane j keeps for row j: no LDS, no atomics, 63 of 64 lanes busy.  Candidates go to
// `masks` (480 B each, read back from L2 by the pricings), claim seeds by LDS atomicOr into claimed[60].
// Phase 2, the rounds.  One wave prices one candidate: it writes cells & ~claimed into its own 60 LDS words, and lane l carries the
// four partial sums of ig_reward_block's threads l, l + 64, l + 128, l + 192 (cells q = T, T + 256, .. ascending each), adds them
// as the tree's steps 128 and 64 do, then steps 32 .. 1 by shuffles (ig_reward_256 in cagym_ig_greedy.h plays the same trick at
// 128 threads).  Rows whose word is empty are skipped - adding nothing is exact.  Four candidates are priced at once, no barrier
// inside a pricing.  In BEST mode a candidate that shares no cell with the mask claimed last keeps its marginal gain - cells &
// ~claimed is the same set - and is not priced again.  The workgroup-wide arg-max on (utility, slot, candidate) goes through LDS as
// k_ig_propose_goals' does.  No global atomics, no unbounded loop (the trace keeps its guard), no host synchronisation; two launches
// give the same bytes.
#pragma once
#include "cagym_ig_viewpoints.h"

#define IGA_MAXC (IG_MAXR * IGV_MAXK)  // 128 candidates per world
#define IGA_WAVES (IGV_THREADS / 64)
#define IGA_NONE 0x7fffffff

struct IgAssignParams {
    int R, k, mode;  // robots, candidates per robot, 0 SLOT / 1 BEST
    double radius, range, fov, d0;
};

struct IgAssignOut {
    int32_t *choice, *order;
    double *marginal, *utility, *round_gain;
    unsigned long long* claimed;
};

// The cell set of the pose (px, py, heading) as row words, lane j < 60 returning word j (a lane >= 60: 0); every lane of the wave
// makes the call with the same arguments.
__device__ __forceinline__ unsigned long long iga_cells(const uint32_t* d2, const IgAssignParams& P, const IgCone& cn, double px, double py,
                                                        double heading, int lane) {
    const bool headed = isfinite(heading);
    int xs, ys, wd, ht;
    double s = 0.0, c = 1.0;
    if (headed) {
        int xe, ye;
        ig_visible_box(px, py, heading, P.fov, P.range, s, c, xs, ys, xe, ye);  // (exclusive upper bounds)
        wd = xe - xs;
        ht = ye - ys;
    } else {
        const int total = igv_rect(px, py, P.range, xs, ys, wd);
        ht = total > 0 ? total / wd : 0;
    }
    if (wd <= 0 || ht <= 0) return 0ull;
    const double r2 = P.range * P.range, r2_in = r2 * (1.0 - 1e-12), r2_out = r2 * (1.0 + 1e-12);  // ig_visible_block's
    const int rpt = 64 / wd;  // rows per trip: wd <= 60
    const int sub = lane / wd, col = lane - sub * wd;
    const unsigned long long wmask = (1ull << wd) - 1ull;
    const int myrow = lane - ys;
    unsigned long long word = 0ull;
    for (int t0 = 0; t0 < ht; t0 += rpt) {  // <= 60 trips
        const int jj = t0 + sub;
        bool vis = false;
        if (sub < rpt && jj < ht) {
            const int i = xs + col, j = ys + jj;  // both within 0..59
            const double cx = ig_cell_centre(i), cy = ig_cell_centre(j);
            const double dx = cx - px, dy = cy - py;
            bool want;
            if (headed) {
                double r0, r1;
                mat2vec(c, s, dx, dy, r0, r1);
                want = ig_in_cone(r0, r1, cn, r2_in, r2_out, P.fov, P.range);
            } else {
                want = dx * dx + dy * dy < r2;
            }
            if (want) vis = ig_check_visibility(d2, px, py, cx, cy);
        }
        const unsigned long long b = __ballot(vis);
        const int ms = myrow - t0;  // my row's place in this trip
        if (ms >= 0 && ms < rpt) word = ((b >> (ms * wd)) & wmask) << xs;
    }
    return lane < IG_BEL ? word : 0ull;
}

// cagym_ig_mi_reward's double for the mask whose word j lane j holds (a lane >= 60: 0), by ONE wave: ig_reward_block's sum at 256
// threads.  s_w: the wave's own 60 LDS words.  Every lane returns the sum.
__device__ __forceinline__ double iga_price(const double* s_mi, unsigned long long* s_w, unsigned long long word, int lane) {
    if (lane < IG_BEL) s_w[lane] = word;
    const unsigned long long rows = __ballot(word != 0ull);
    // the words are read by other lanes of this wave alone: its LDS operations execute in order, the fence keeps the compiler's
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {  // thread T = lane + 64 u of the 256
        double acc = 0.0;
        for (int q = lane + 64 * u; q < IGV_CELLS; q += 256) {
            const int j = q / IG_BEL;
            if ((rows >> j) & 1ull) {
                const int i = q - j * IG_BEL;
                if ((s_w[j] >> i) & 1ull) acc += s_mi[q];
            }
        }
        a[u] = acc;
    }
    double v = (a[0] + a[2]) + (a[1] + a[3]);  // the tree's steps 128 and 64
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);  // steps 32 .. 1 (fp64 addition commutes: every lane ends with red[0])
    __builtin_amdgcn_wave_barrier();  // (every lane has read s_w before the wave's next pricing writes it)
    return v;
}

__global__ void __launch_bounds__(IGV_THREADS) k_ig_assign_goals(IgDev G, IgAssignParams P, const uint8_t* __restrict__ mask,
                                                                 const double* __restrict__ cand_xy, const double* __restrict__ cand_heading,
                                                                 const float* __restrict__ cand_distance, const uint8_t* __restrict__ claim,
                                                                 const double* __restrict__ claim_xy, const double* __restrict__ claim_heading,
                                                                 int32_t* choice, int32_t* order, double* marginal, double* utility,
                                                                 unsigned long long* claimed_out, unsigned long long* masks, double* round_gain) {
    __shared__ double s_mi[IGV_CELLS];
    __shared__ unsigned long long s_claimed[IG_BEL], s_last[IG_BEL], s_w[IGA_WAVES][IG_BEL];
    __shared__ double s_marg[IGA_MAXC], s_dd[IGA_MAXC], s_bu[IGA_WAVES];
    __shared__ int s_bi[IGA_WAVES];
    __shared__ uint8_t s_ok[IGA_MAXC];
    __shared__ IgAssignOut s_out;  // the outputs of phase 2 wait here: phase 1, the traces, needs the scalar registers they would hold
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = P.R, k = P.k, RK = R * k;
    unsigned masked = 0u;
    for (int r = 0; r < R; r++)
        if (!mask || mask[(size_t)w * R + r]) masked |= 1u << r;
    if (!masked) return;  // no robot chooses here: nothing of this world is read or written
    if (tid < IG_BEL) s_claimed[tid] = 0ull;
    if (tid == 0) {
        s_out.choice = choice;
        s_out.order = order;
        s_out.marginal = marginal;
        s_out.utility = utility;
        s_out.claimed = claimed_out;
        s_out.round_gain = round_gain;
    }
    if (round_gain) {
        double* rg = round_gain + (size_t)w * R * RK;
        for (int q = tid; q < R * RK; q += IGV_THREADS) rg[q] = ig_nan_d();
    }
    igv_stage_mi(G, w, tid, s_mi);  // (ends with a barrier)
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double need = P.radius + 0.1;
    const IgCone cn = ig_cone(P.fov);  // one per launch, as k_ig_visible's ig_visible_block evaluates it
    const size_t wRK = (size_t)w * RK;

    // ---- phase 1: the cell sets (every value below but the lane's own cells is wave-uniform)
    for (int p = wave; p < RK + R; p += IGA_WAVES) {
        const bool seed = p >= RK;
        const int r = seed ? p - RK : p / k;
        const size_t wr = (size_t)w * R + r;
        const bool on = (masked >> r) & 1u;
        if (seed ? (on || !claim || !claim[wr]) : !on) continue;
        const size_t o = seed ? wr : wRK + p;
        const double* hd = seed ? claim_heading : cand_heading;
        const double heading = hd ? hd[o] : ig_nan_d();
        double px, py;
        const bool ok = igv_point(d2, seed ? claim_xy : cand_xy, o, 0, need, px, py);
        const unsigned long long word = ok ? iga_cells(d2, P, cn, px, py, heading, lane) : 0ull;
        if (seed) {
            if (lane < IG_BEL && word) atomicOr(&s_claimed[lane], word);
        } else {
            if (lane < IG_BEL) masks[o * IG_BEL + lane] = word;
            if (lane == 0) {
                const float dist = cand_distance[o];
                s_ok[p] = ok && isfinite(dist) ? 1 : 0;
                s_dd[p] = (double)dist + P.d0;
            }
        }
    }
    __syncthreads();  // (the workgroup's own stores to `masks` are visible to it from here on)

    // ---- phase 2: the rounds
    const IgAssignOut O = s_out;
    const int n_rounds = __popc(masked);
    unsigned open = masked, turns = masked;
    for (int t = 0; t < n_rounds; t++) {
        unsigned pricing = open;
        if (P.mode == 0) {  // SLOT: the t-th masked robot's turn
            pricing = turns & (0u - turns);
            turns &= turns - 1u;
        }
        for (int p = wave; p < RK; p += IGA_WAVES) {
            const int r = p / k;
            if (!((pricing >> r) & 1u) || !s_ok[p]) continue;
            const unsigned long long word = lane < IG_BEL ? masks[(wRK + p) * IG_BEL + lane] : 0ull;
            double m;
            if (P.mode != 0 && t > 0 && !__ballot(lane < IG_BEL && (word & s_last[lane < IG_BEL ? lane : 0]) != 0ull)) {
                m = s_marg[p];  // no cell in common with what was claimed last: the same set, the same sum
            } else {
                m = iga_price(s_mi, s_w[wave], lane < IG_BEL ? word & ~s_claimed[lane] : 0ull, lane);
                if (lane == 0) s_marg[p] = m;
            }
            if (lane == 0 && O.round_gain) O.round_gain[((size_t)w * R + t) * RK + p] = m;
        }
        __syncthreads();
        // the arg-max on (utility, slot, candidate): candidate p = slot * k + candidate carries both
        double bu = 0.0;
        int bi = IGA_NONE;
        if (tid < RK && ((pricing >> (tid / k)) & 1u) && s_ok[tid] && s_marg[tid] > 0.0) {
            bu = s_marg[tid] / s_dd[tid];
            bi = tid;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ou = __shfl_xor(bu, off);
            const int oi = __shfl_xor(bi, off);
            if (oi != IGA_NONE && (bi == IGA_NONE || ou > bu || (ou == bu && oi < bi))) {
                bu = ou;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_bu[wave] = bu;
            s_bi[wave] = bi;
        }
        __syncthreads();
        bu = s_bu[0];
        bi = s_bi[0];
#pragma unroll
        for (int v = 1; v < IGA_WAVES; v++) {
            const double ou = s_bu[v];
            const int oi = s_bi[v];
            if (oi != IGA_NONE && (bi == IGA_NONE || ou > bu || (ou == bu && oi < bi))) {
                bu = ou;
                bi = oi;
            }
        }
        if (bi == IGA_NONE) {  // uniform: nothing is eligible
            if (P.mode != 0) break;
            continue;  // (the next round's pricing barrier stands between these reads of s_bu / s_bi and its writes)
        }
        const int r = bi / k;
        open &= ~(1u << r);
        if (tid == 0) {
            const size_t wr = (size_t)w * R + r;
            O.choice[wr] = bi - r * k;
            O.order[wr] = t;
            O.marginal[wr] = s_marg[bi];
            O.utility[wr] = bu;
        }
        if (tid < IG_BEL) {
            const unsigned long long won = masks[(wRK + bi) * IG_BEL + tid];
            s_last[tid] = won;
            s_claimed[tid] |= won;
        }
        __syncthreads();
    }
    if (tid < R && ((open >> tid) & 1u)) {  // the masked robots nothing was left for
        const size_t wr = (size_t)w * R + tid;
        O.choice[wr] = -1;
        O.order[wr] = -1;
        O.marginal[wr] = 0.0;
        O.utility[wr] = 0.0;
    }
    if (tid < IG_BEL) O.claimed[(size_t)w * IG_BEL + tid] = s_claimed[tid];
}
