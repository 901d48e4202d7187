// cagym_ig_viewpoints.h -- what a PLACE is worth to an IG robot (include/cagym.h: cagym_ig_view_gain, cagym_ig_propose_goals): the
// mutual information of every belief cell a robot standing at a point could see through the world's walls, turning on the spot, and
// the best k such places per robot, well separated, ranked by that gain against the geodesic distance to them.
//
// k_ig_view_gain: one workgroup of 256 threads per world and IGV_PER_WG = 60 consecutive viewpoints - in map mode (points_xy NULL) the
// 60 cell centres of ONE belief row, generated here, so a workgroup's traces start side by side and walk the same lines of the
// world's distance field in L1 / L2; in points mode the caller's [N,P,2] in order.  Map mode runs the very statements of points mode
// on the same doubles (the centres are exact in fp64): its values are the points mode's bit for bit.  The world's MI cache
// (IgDev::mi, 28.8 KB) is staged in LDS once.  Each of the four waves takes every fourth viewpoint; its candidate cells - the
// rectangle cell(p - range) .. cell(p + range), at most 21 x 21 at range 5 - are dealt to the 64 lanes round robin in row-major
// order, every lane tests the range in fp64 (separate products and sums: this file is compiled without contraction), sphere-traces
// with the pinned ig_check_visibility / edf_at, unchanged, and adds its visible cells' MI in candidate order; the 64 partial sums
// are combined in a fixed butterfly (xor 32, 16, .. 1), so two launches give the same bits.  There is no shortcut for viewpoints in
// the open: edf_at returns the field of the raster cell a sample falls into, which is not 1-Lipschitz in the sample point, so "the
// clearance exceeds the range" does not imply the trace's own tests.  No global atomics, no unbounded loop (the trace keeps its
// guard), one barrier; a world whose mask byte is 0 leaves before it and touches nothing.
//
// k_ig_propose_goals: one workgroup of 256 threads per (world, robot); a robot whose mask byte is 0 leaves before the first barrier.
// The 3600 utilities gain / ((double)field + d0) live in LDS (-1: not eligible or suppressed; an eligible cell's is >= 0); k rounds
// of a workgroup-wide arg-max on the key (utility, smaller flat index j 60 + i) - per thread in ascending index, a butterfly inside
// the wave, the four waves' winners through LDS - and the suppression of every cell within min_sep of the winner.
#pragma once
#include "cagym_ig.h"

#define IGV_MAXK 16
#define IGV_PER_WG 60
#define IGV_THREADS 256
#define IGV_CELLS (IG_BEL * IG_BEL)

struct IgViewParams {
    int P, R, k;  // viewpoints per world (3600 in map mode), robots, proposals per robot
    double radius, range, min_sep, d0;
};

// ---- what k_ig_view_gain and k_ig_view_gain_headings (cagym_ig_headings.h) do alike.  The workgroup's world w and its viewpoints
// p0 <= p < p1 of the n_points per world (n_points >= 1: the entries launch nothing for 0; no sum that could pass INT_MAX) ...
__device__ __forceinline__ void igv_span(int n_points, int& w, int& p0, int& p1) {
    const int chunks = (n_points - 1) / IGV_PER_WG + 1;
    w = blockIdx.x / chunks;
    p0 = (blockIdx.x - w * chunks) * IGV_PER_WG;
    p1 = n_points - p0 < IGV_PER_WG ? n_points : p0 + IGV_PER_WG;
}
// ... the world's MI cache into s_mi[IGV_CELLS] by every thread of the workgroup, ending with the kernel's one barrier ...
__device__ __forceinline__ void igv_stage_mi(const IgDev& G, int w, int tid, double* s_mi) {
    const double* mi = G.mi + (size_t)w * IGV_CELLS;
    for (int q = tid; q < IGV_CELLS; q += IGV_THREADS) s_mi[q] = mi[q];
    __syncthreads();
}
// ... viewpoint o = w * n_points + p: the caller's point, or in map mode (points_xy NULL) the centre of belief cell p, and whether a robot
// can stand there - finite, inside the map and clear by the planners' feasibility test EDF > need = radius + 0.1.
__device__ __forceinline__ bool igv_point(const uint32_t* d2, const double* __restrict__ points_xy, size_t o, int p, double need, double& px, double& py) {
    if (points_xy) {
        px = points_xy[2 * o];
        py = points_xy[2 * o + 1];
    } else {
        px = ig_cell_centre(p % IG_BEL);
        py = ig_cell_centre(p / IG_BEL);
    }
    const int ci = ig_bel_cell(px), cj = ig_bel_cell(py);
    bool ok = isfinite(px) && isfinite(py) && ci >= 0 && ci < IG_BEL && cj >= 0 && cj < IG_BEL;
    if (ok) ok = edf_at(d2, px, py) > need;
    return ok;
}
// ... and its candidate cells: the rectangle cell(p - range) .. cell(p + range) inside the map, wd wide from (xs, ys); returns their number
__device__ __forceinline__ int igv_rect(double px, double py, double range, int& xs, int& ys, int& wd) {
    xs = max(0, ig_bel_cell(px - range));
    ys = max(0, ig_bel_cell(py - range));
    const int xe = min(IG_BEL - 1, ig_bel_cell(px + range)), ye = min(IG_BEL - 1, ig_bel_cell(py + range));
    wd = xe - xs + 1;
    const int ht = ye - ys + 1;
    return (wd > 0 && ht > 0) ? wd * ht : 0;
}

__global__ void __launch_bounds__(IGV_THREADS) k_ig_view_gain(IgDev G, IgViewParams P, const uint8_t* __restrict__ world_mask,
                                                              const double* __restrict__ points_xy, double* gain, int32_t* n_visible,
                                                              uint8_t* valid) {
    __shared__ double s_mi[IGV_CELLS];
    int w, p0, p1;
    igv_span(P.P, w, p0, p1);
    if (world_mask && !world_mask[w]) return;  // not flagged: nothing of this world is read or written
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    igv_stage_mi(G, w, tid, s_mi);
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double need = P.radius + 0.1, r2 = P.range * P.range;
    for (int p = p0 + wave; p < p1; p += IGV_THREADS / 64) {  // (every value below but the lane's own cells is wave-uniform)
        const size_t o = (size_t)w * P.P + p;
        double px, py;
        const bool ok = igv_point(d2, points_xy, o, p, need, px, py);
        double acc = 0.0;
        int cnt = 0;
        if (ok) {
            int xs, ys, wd;
            const int total = igv_rect(px, py, P.range, xs, ys, wd);
            for (int q = lane; q < total; q += 64) {
                const int jj = q / wd;
                const int i = xs + (q - jj * wd), j = ys + jj;  // both within 0..59
                const double cx = ig_cell_centre(i), cy = ig_cell_centre(j);
                const double dx = cx - px, dy = cy - py;
                if (dx * dx + dy * dy < r2 && ig_check_visibility(d2, px, py, cx, cy)) {
                    acc += s_mi[j * IG_BEL + i];
                    cnt++;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {  // a fixed tree: fp64 addition commutes, every lane ends with the same sum
            acc += __shfl_xor(acc, off);
            cnt += __shfl_xor(cnt, off);
        }
        if (lane == 0) {
            gain[o] = acc;
            n_visible[o] = cnt;
            valid[o] = ok ? 1 : 0;
        }
    }
}

// (utility, flat index): the larger utility wins, of equal utilities the smaller index
__device__ __forceinline__ void igv_better(double& bu, int& bi, double ou, int oi) {
    if (ou > bu || (ou == bu && oi < bi)) {
        bu = ou;
        bi = oi;
    }
}

__global__ void __launch_bounds__(IGV_THREADS) k_ig_propose_goals(IgViewParams P, const uint8_t* __restrict__ mask,
                                                                  const double* __restrict__ gain_map,
                                                                  const uint8_t* __restrict__ valid_map, const float* __restrict__ field,
                                                                  int32_t* cells, double* xy, double* utility, double* gain,
                                                                  float* distance, int32_t* n_found) {
    __shared__ double s_u[IGV_CELLS];
    __shared__ double s_bu[IGV_THREADS / 64];
    __shared__ int s_bi[IGV_THREADS / 64];
    const int wr = blockIdx.x, w = wr / P.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (mask && !mask[wr]) return;  // not flagged: nothing of this robot is read or written
    const double* g = gain_map + (size_t)w * IGV_CELLS;
    const uint8_t* v = valid_map + (size_t)w * IGV_CELLS;
    const float* f = field + (size_t)wr * IGV_CELLS;
    const float inf = ig_inf_f();
    for (int q = tid; q < IGV_CELLS; q += IGV_THREADS) {
        const double gv = g[q];
        const float fv = f[q];
        const bool eligible = v[q] != 0 && gv > 0.0 && fv < inf && fv > -inf;  // (the comparisons refuse NaN)
        s_u[q] = eligible ? gv / ((double)fv + P.d0) : -1.0;
    }
    __syncthreads();
    const double sep2 = P.min_sep * P.min_sep;
    const size_t row = (size_t)wr * P.k;
    int found = 0;
    for (; found < P.k; found++) {
        double bu = -1.0;
        int bi = IGV_CELLS;
        for (int q = tid; q < IGV_CELLS; q += IGV_THREADS) {  // ascending: the strict test keeps the smallest index
            const double u = s_u[q];
            if (u > bu) {
                bu = u;
                bi = q;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ou = __shfl_xor(bu, off);
            const int oi = __shfl_xor(bi, off);
            igv_better(bu, bi, ou, oi);
        }
        if (lane == 0) {
            s_bu[wave] = bu;
            s_bi[wave] = bi;
        }
        __syncthreads();
        bu = s_bu[0];
        bi = s_bi[0];
#pragma unroll
        for (int k = 1; k < IGV_THREADS / 64; k++) igv_better(bu, bi, s_bu[k], s_bi[k]);
        if (bi >= IGV_CELLS) break;  // uniform: nothing is left
        const int cj = bi / IG_BEL, ci = bi - cj * IG_BEL;
        if (tid == 0) {
            const size_t o = row + found;
            cells[2 * o] = ci;
            cells[2 * o + 1] = cj;
            xy[2 * o] = ig_cell_centre(ci);
            xy[2 * o + 1] = ig_cell_centre(cj);
            utility[o] = bu;
            gain[o] = g[bi];
            distance[o] = f[bi];
        }
        for (int q = tid; q < IGV_CELLS; q += IGV_THREADS) {
            const int j = q / IG_BEL, i = q - j * IG_BEL;
            const int di = i - ci, dj = j - cj;
            if ((double)(di * di + dj * dj) * 0.25 < sep2) s_u[q] = -1.0;  // (the chosen cell included: min_sep > 0)
        }
        __syncthreads();  // (also: every thread has read s_bu / s_bi before the next round writes them)
    }
    if (tid >= found && tid < P.k) {  // rows past n_found
        const size_t o = row + tid;
        cells[2 * o] = cells[2 * o + 1] = -1;
        xy[2 * o] = xy[2 * o + 1] = ig_nan_d();
        utility[o] = 0.0;
        gain[o] = 0.0;
        distance[o] = inf;
    }
    if (tid == 0) n_found[wr] = found;
}
