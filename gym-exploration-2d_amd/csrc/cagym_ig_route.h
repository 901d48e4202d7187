// cagym_ig_route.h -- what a robot sees ON THE WAY to a candidate goal (include/cagym.h: cagym_ig_route_gains).  cagym_ig_view_gain,
// cagym_ig_propose_goals and cagym_ig_assign_goals price a candidate as if the robot were teleported to it; the drive there is often
// several metres, and the sensor cone sweeps fresh cells all along it.  Here every candidate's shortest path is walked back on the
// robot's own geodesic field by the controller's neighbour rule, the cone is taken at way-points along it, and the union is priced by
// the mutual information of its cells - so a cone across unexplored ground can beat a better-looking one next door.
//
// THE RULE (ig.route_spec and ig.route_gains_spec are its executable form).  Per world R robots (1..8) with k candidate cells each
// (1..16); field: each robot's geodesic field with its own cell as the source (cagym_ig_geodesic).  For a masked robot and a
// candidate cell q_0 inside 0..59 whose field value is finite:
//   walk: from q_s to the neighbour k_ig_goal_actions would drive to - GEO_NEIGHBOURS in the order E, N, W, S, NE, NW, SW, SE, key
//     fl32(field[n] + cost) over finite values only, a diagonal only with both orthogonal neighbours finite, the first of equal
//     smallest keys - until the cell whose field is 0, q_n.  A cell without such a neighbour, a move that does not lower the field
//     value, or more than 3600 moves end the walk: the candidate has NO ROUTE (n_path -1, gains and utility 0, empty masks).
//   travel order: p_t = q_{n-t}; the heading into p_t is that of the move p_{t-1} -> p_t, the double m * (M_PI / 4) with m = 0, 2, 4,
//     -2, 1, 3, -3, -1 for E .. SE - one fp64 product.
//   way-points: t = stride, 2 stride, .. with t < n and t <= 16 stride; truncated = 1 when a t < n beyond 16 stride was dropped.  A
//     way-point's pose is its cell's centre with the heading into it, its cell set exactly cagym_ig_visible_cells' for that pose at
//     the call's fov and range (iga_cells' headed branch).
//   route = the union of the way-point sets; terminal = the candidate's own set by cagym_ig_assign_goals' rule at the cell's centre
//     (a finite cand_heading: the cone; none: a robot turning on the spot; igv_point fails: empty); total = route | terminal.
//   route_gain = mi_reward(route & ~exclude), total_gain = mi_reward(total & ~exclude), each cagym_ig_mi_reward's double bit for bit
//     (iga_price); utility = total_gain / ((double)field[q_0] + d0), one fp64 addition and one fp64 division.
//   best: the candidate with a route and total_gain > 0 of largest utility, of equal utilities the smaller index; none: -1.
//   Rows of robots outside the mask keep every byte; a world without a masked robot is neither read nor written.
//
// k_ig_route_gains: one workgroup of 256 threads per world; a world without a masked robot leaves before the first barrier.  The
// world's MI cache goes to LDS once (igv_stage_mi, 28.8 KB).
// Phase 1, the walks: one lane per candidate (<= 128, dealt over the four waves) walks its field row twice - once for n, once to
// record its <= 16 way-points as (cell, direction of travel) words in LDS (8 KB).  Both loops are capped at 3600 moves.
// Phase 2, one wave per candidate, round robin: the way-point sets are ORed in the lanes' registers - lane j holds row word j, as
// iga_cells returns it: no LDS, no atomics - the terminal set is added, and both unions are priced by iga_price.
// Phase 3, a robot's arg-max by one thread in ascending candidate order.  No global atomics, no unbounded loop (the trace keeps its
// guard), no host synchronisation; two launches give the same bytes.
#pragma once
#include "cagym_ig_assign.h"
#include "cagym_ig_geodesic.h"

#define IGR_MAXW 16        // way-points per candidate
#define IGR_WALK_CAP 3600  // moves per walk: no descending chain is longer than the number of cells

struct IgRouteParams {
    int R, k, stride;  // robots, candidates per robot, cells between two way-points (the entry clamps it to IGR_WALK_CAP + 1)
    double radius, range, fov, d0;
};

struct IgRouteOut {
    unsigned long long *route_masks, *total_masks;
    double *route_gain, *total_gain, *utility;
    int32_t *n_path, *n_way;
    uint8_t* truncated;
    int32_t* best;
    int32_t* way_cells;  // or NULL
    int8_t* way_dir;     // or NULL
};

__device__ __forceinline__ bool igr_finite(float v) { return v < ig_inf_f() && v > -ig_inf_f(); }  // (the comparisons refuse NaN)

// k_ig_goal_actions' neighbour choice at a cell whose own value is finite, restated (that kernel's code stays as it is): the index
// 0..7 of the neighbour in GEO_NEIGHBOURS order and its field value, or -1 when no neighbour is finite.
__device__ __forceinline__ int igr_next(const float* f, int ci, int cj, float& nv) {
    const float e = igg_at(f, ci + 1, cj), n = igg_at(f, ci, cj + 1), wv = igg_at(f, ci - 1, cj), s = igg_at(f, ci, cj - 1);
    const bool fe = igr_finite(e), fn = igr_finite(n), fw = igr_finite(wv), fs = igr_finite(s);
    const float val[8] = {e, n, wv, s, igg_at(f, ci + 1, cj + 1), igg_at(f, ci - 1, cj + 1), igg_at(f, ci - 1, cj - 1), igg_at(f, ci + 1, cj - 1)};
    const bool open[8] = {true, true, true, true, fe && fn, fw && fn, fw && fs, fe && fs};
    float best = ig_inf_f();
    int pick = -1;
    nv = ig_inf_f();
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float key = val[k] + (k < 4 ? IGG_ORTHO : IGG_DIAG);
        if (open[k] && igr_finite(val[k]) && key < best) {
            best = key;
            pick = k;
            nv = val[k];
        }
    }
    return pick;
}

// The walk from the candidate's cell (i0, j0) down the field row f to the cell whose value is 0: the number of moves n, or -1 (no
// route).  With `way` (the second walk, n known): the way-points t = stride m, m = 1 .. 16, t < n, as words i | j << 8 | d << 16 in
// way[m - 1], d the direction of TRAVEL into the cell - the opposite of the walk's move out of it, index ^ 2 in GEO_NEIGHBOURS.
__device__ __forceinline__ int igr_walk(const float* f, int i0, int j0, int n, int stride, uint32_t* way) {
    if (i0 < 0 || i0 >= IG_BEL || j0 < 0 || j0 >= IG_BEL) return -1;
    int ci = i0, cj = j0;
    float cur = f[cj * IG_BEL + ci];
    if (!igr_finite(cur)) return -1;
    for (int s = 0; s <= IGR_WALK_CAP; s++) {
        if (cur == 0.f) return s;
        if (s == IGR_WALK_CAP) break;
        float nv;
        const int k = igr_next(f, ci, cj, nv);
        if (k < 0 || !(nv < cur)) return -1;
        if (way && s >= 1) {
            const int t = n - s, m = t / stride;
            if (m * stride == t && m <= IGR_MAXW) way[m - 1] = (uint32_t)ci | ((uint32_t)cj << 8) | ((uint32_t)(k ^ 2) << 16);
        }
        // GEO_NEIGHBOURS' (di, dj) + 1 in two bits per direction: a table indexed by a lane's own k would live in scratch
        const unsigned di1 = 2u | 1u << 2 | 0u << 4 | 1u << 6 | 2u << 8 | 0u << 10 | 0u << 12 | 2u << 14;
        const unsigned dj1 = 1u | 2u << 2 | 1u << 4 | 0u << 6 | 2u << 8 | 2u << 10 | 0u << 12 | 0u << 14;
        ci += (int)((di1 >> (2 * k)) & 3u) - 1;
        cj += (int)((dj1 >> (2 * k)) & 3u) - 1;
        cur = nv;
    }
    return -1;
}

// the heading of a move in GEO_NEIGHBOURS order: m * (M_PI / 4), one fp64 product
__device__ __forceinline__ double igr_heading(int d) {
    const unsigned m3 = 3u | 5u << 3 | 7u << 6 | 1u << 9 | 4u << 12 | 6u << 15 | 0u << 18 | 2u << 21;  // m + 3 in three bits each
    return (double)((int)((m3 >> (3 * d)) & 7u) - 3) * (kPi / 4);
}

__global__ void __launch_bounds__(IGV_THREADS) k_ig_route_gains(IgDev G, IgRouteParams P, const uint8_t* __restrict__ mask,
                                                                const float* __restrict__ field, const int32_t* __restrict__ cand_cells,
                                                                const double* __restrict__ cand_heading,
                                                                const unsigned long long* __restrict__ exclude, IgRouteOut out) {
    __shared__ double s_mi[IGV_CELLS];
    __shared__ unsigned long long s_w[IGA_WAVES][IG_BEL];
    __shared__ uint32_t s_way[IGA_MAXC][IGR_MAXW];
    __shared__ int s_n[IGA_MAXC], s_nw[IGA_MAXC];
    __shared__ double s_u[IGA_MAXC];
    __shared__ uint8_t s_el[IGA_MAXC];
    __shared__ IgRouteOut s_out;  // the outputs wait here while the walks and the traces run, as k_ig_assign_goals' do
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = P.R, k = P.k, RK = R * k;
    unsigned masked = 0u;
    for (int r = 0; r < R; r++)
        if (!mask || mask[(size_t)w * R + r]) masked |= 1u << r;
    if (!masked) return;  // no robot asks here: nothing of this world is read or written
    if (tid == 0) s_out = out;
    igv_stage_mi(G, w, tid, s_mi);  // (ends with a barrier)
    const size_t wRK = (size_t)w * RK;

    // ---- phase 1: the walks, candidate p on thread 64 (p % 4) + p / 4
    {
        const int p = (tid & 63) * IGA_WAVES + wave;
        if (lane < IGA_MAXC / IGA_WAVES && p < RK && ((masked >> (p / k)) & 1u)) {
            const int r = p / k;
            const float* f = field + ((size_t)w * R + r) * IGV_CELLS;
            const int i0 = cand_cells[2 * (wRK + p)], j0 = cand_cells[2 * (wRK + p) + 1];
            const int n = igr_walk(f, i0, j0, 0, 1, nullptr);
            int nw = 0;
            if (n > 0) {
                nw = min(IGR_MAXW, (n - 1) / P.stride);  // ceil(n / stride) - 1 way-points with t < n
                if (nw > 0) igr_walk(f, i0, j0, n, P.stride, s_way[p]);
            }
            s_n[p] = n;
            s_nw[p] = nw;
        }
    }
    __syncthreads();

    // ---- phase 2: the sets and their prices (every value below but the lane's own words is wave-uniform)
    const IgRouteOut O = s_out;
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    IgAssignParams A;  // what iga_cells reads: range and fov
    A.R = R; A.k = k; A.mode = 0;
    A.radius = P.radius; A.range = P.range; A.fov = P.fov; A.d0 = P.d0;
    const double need = P.radius + 0.1;
    const IgCone cn = ig_cone(P.fov);
    const unsigned long long ex = (exclude && lane < IG_BEL) ? exclude[(size_t)w * IG_BEL + lane] : 0ull;
    for (int p = wave; p < RK; p += IGA_WAVES) {
        const int r = p / k;
        if (!((masked >> r) & 1u)) continue;
        const size_t o = wRK + p;
        const int n = __builtin_amdgcn_readfirstlane(s_n[p]), nw = __builtin_amdgcn_readfirstlane(s_nw[p]);
        unsigned long long route = 0ull, total = 0ull;
        double rg = 0.0, tg = 0.0, u = 0.0;
        if (n >= 0) {
            for (int m = 0; m < nw; m++) {  // <= 16
                const uint32_t wp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_way[p][m]);
                route |= iga_cells(d2, A, cn, ig_cell_centre((int)(wp & 255u)), ig_cell_centre((int)((wp >> 8) & 255u)),
                                   igr_heading((int)(wp >> 16)), lane);
            }
            const int i0 = cand_cells[2 * o], j0 = cand_cells[2 * o + 1];  // both within 0..59: the walk began there
            double px, py;
            total = route;
            if (igv_point(d2, nullptr, 0, j0 * IG_BEL + i0, need, px, py))
                total |= iga_cells(d2, A, cn, px, py, cand_heading ? cand_heading[o] : ig_nan_d(), lane);
            rg = iga_price(s_mi, s_w[wave], route & ~ex, lane);
            tg = iga_price(s_mi, s_w[wave], total & ~ex, lane);
            u = tg / ((double)field[((size_t)w * R + r) * IGV_CELLS + j0 * IG_BEL + i0] + P.d0);
        }
        if (lane < IG_BEL) {
            O.route_masks[o * IG_BEL + lane] = route;
            O.total_masks[o * IG_BEL + lane] = total;
        }
        if (lane < IGR_MAXW) {
            const uint32_t wp = lane < nw ? s_way[p][lane] : 0u;
            if (O.way_cells) {
                O.way_cells[(o * IGR_MAXW + lane) * 2] = lane < nw ? (int)(wp & 255u) : -1;
                O.way_cells[(o * IGR_MAXW + lane) * 2 + 1] = lane < nw ? (int)((wp >> 8) & 255u) : -1;
            }
            if (O.way_dir) O.way_dir[o * IGR_MAXW + lane] = lane < nw ? (int8_t)(wp >> 16) : (int8_t)-1;
        }
        if (lane == 0) {
            O.route_gain[o] = rg;
            O.total_gain[o] = tg;
            O.utility[o] = u;
            O.n_path[o] = n;
            O.n_way[o] = nw;
            O.truncated[o] = (n > 0 && (n - 1) / P.stride > IGR_MAXW) ? 1 : 0;
            s_u[p] = u;
            s_el[p] = (n >= 0 && tg > 0.0) ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- phase 3: every masked robot's best candidate (ascending: the strict test keeps the smaller index of equal utilities)
    if (tid < R && ((masked >> tid) & 1u)) {
        double bu = 0.0;
        int bi = -1;
        for (int c = 0; c < k; c++) {
            const int p = tid * k + c;
            if (s_el[p] && (bi < 0 || s_u[p] > bu)) {
                bu = s_u[p];
                bi = c;
            }
        }
        O.best[(size_t)w * R + tid] = bi;
    }
}
