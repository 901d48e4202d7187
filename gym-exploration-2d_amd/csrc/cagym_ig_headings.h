// cagym_ig_headings.h -- what a POSE is worth to an IG robot, and goals that carry a heading (include/cagym.h:
// cagym_ig_view_gain_headings, cagym_ig_goal_face_actions, cagym_ig_goal_face_status).  cagym_ig_view_gain scores a robot turning on
// the spot; the sensor is a cone, the planners and the reward score a pose (x, y, theta).  Here every viewpoint is scored at H
// caller-chosen headings: for heading h exactly the cells cagym_ig_visible_cells returns for the pose (x, y, headings[h]).
//
// k_ig_view_gain_headings keeps k_ig_view_gain's layout and shares its opening (igv_span, igv_stage_mi, igv_point, igv_rect): 256 threads,
// IGV_PER_WG = 60 consecutive viewpoints per workgroup (in map mode the 60 cell centres of one belief row: the same bits), the
// world's MI cache staged in LDS once, one wave per viewpoint round robin, the candidate cells - the rectangle cell(p - range) ..
// cell(p + range) - dealt to the 64 lanes round robin in row-major order.  The sphere trace does not depend on the heading, so a
// candidate is traced ONCE and the answer kept as bit t of a per-lane register (candidate lane + 64 t: at most 7 at range 5, at
// most 57 for the whole 60 x 60 grid).  Then H passes over the lane's own candidates: the box of ig_visible_block
// (ig_visible_box_sc, exclusive upper bound and all, on sines and cosines that the lanes of each wave evaluate once per launch with
// ig_sincos), mat2vec, ig_in_cone with one IgCone per launch, and the add - the very device functions k_ig_visible runs.  Only
// candidates that pass a pre-filter are traced: dx dx + dy dy <= range^2 (1 + 1e-9), a superset of every cone's cells
// (ig_in_cone accepts nothing beyond rn^2 = range^2 (1 + 1e-12) on the rotated vector, whose squared norm differs from dx dx + dy dy
// by a few ulp; the range test itself stays ig_in_cone's `rn < range`).  The rectangle is a superset of every heading's box: fp64
// products and sums are monotone, so px + range cos <= px + range.
// Each heading's 64 partial sums are added per lane in candidate order and combined in the fixed butterfly xor 32 .. 1: two launches
// give the same bits.  No global atomics, no unbounded loop, one barrier; a world whose mask byte is 0 leaves before it.
//
// k_ig_goal_face_actions / k_ig_goal_face_status: one wave per world like k_ig_goal_actions / k_ig_goal_status and launched directly
// behind them - a robot that has arrived turns to its goal's heading, and "there, and facing it" is a status of its own.
#pragma once
#include "cagym_ig_geodesic.h"
#include "cagym_ig_viewpoints.h"

#define IGH_MAXH 16

struct IgHeadingParams {
    int P, H;  // viewpoints per world (3600 in map mode), headings
    double radius, range, fov;
    double headings[IGH_MAXH];
};

__global__ void __launch_bounds__(IGV_THREADS) k_ig_view_gain_headings(IgDev G, IgHeadingParams P, const uint8_t* __restrict__ world_mask,
                                                                       const double* __restrict__ points_xy, double* gain_h,
                                                                       int32_t* n_visible_h, int32_t* best_heading, double* best_gain,
                                                                       uint8_t* valid) {
    __shared__ double s_mi[IGV_CELLS];
    int w, p0, p1;
    igv_span(P.P, w, p0, p1);
    if (world_mask && !world_mask[w]) return;  // not flagged: nothing of this world is read or written
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    igv_stage_mi(G, w, tid, s_mi);
    const uint32_t* d2 = G.d2 + (size_t)ig_scenario(G, w) * CAGYM_MAPD * CAGYM_MAPD;
    const double need = P.radius + 0.1, r2_pre = P.range * P.range * (1.0 + 1e-9);
    const IgCone cn = ig_cone(P.fov);  // one per launch, as k_ig_visible's ig_visible_block evaluates it
    const double r2_in = P.range * P.range * (1.0 - 1e-12), r2_out = P.range * P.range * (1.0 + 1e-12);  // ig_visible_block's
    // the sines and cosines of the box and the rotation depend on the heading alone: lane 3 h + k of every wave holds those of
    // headings[h] (k = 0), headings[h] + fov (1) and headings[h] - fov (2), the operands ig_visible_block hands ig_sincos
    double my_s = 0.0, my_c = 1.0;
    for (int h = 0; h < P.H; h++) {
        const double phi = P.headings[h];
        const int k = lane - 3 * h;
        if (k >= 0 && k < 3) ig_sincos(k == 0 ? phi : (k == 1 ? phi + P.fov : phi - P.fov), &my_s, &my_c);
    }
    for (int p = p0 + wave; p < p1; p += IGV_THREADS / 64) {  // (every value below but the lane's own cells is wave-uniform)
        const size_t o = (size_t)w * P.P + p;
        double px, py;
        if (!igv_point(d2, points_xy, o, p, need, px, py)) {
            if (lane < P.H) {
                if (gain_h) gain_h[o * P.H + lane] = 0.0;
                if (n_visible_h) n_visible_h[o * P.H + lane] = 0;
            }
            if (lane == 0) {
                best_heading[o] = -1;
                best_gain[o] = 0.0;
                valid[o] = 0;
            }
            continue;
        }
        // 1. the traces, once per candidate: bit t of `seen` <=> candidate lane + 64 t is near enough and visible
        int xs, ys, wd;
        const int total = igv_rect(px, py, P.range, xs, ys, wd);  // <= 3600
        const int trips = (total + 63) >> 6;                      // <= 57: a bit each
        // q / wd without the integer division: (q + 0.5) / wd lies at least 0.5 / wd from an integer and the fp32 product is off
        // by at most (3600 / wd) 2^-23, so the truncation is the quotient for every q < 3600, wd <= 60
        const float rwd = 1.0f / (float)max(wd, 1);
        unsigned long long seen = 0ull;
        for (int t = 0; t < trips; t++) {
            const int q = lane + 64 * t;
            if (q < total) {
                const int jj = (int)(((float)q + 0.5f) * rwd);
                const int i = xs + (q - jj * wd), j = ys + jj;  // both within 0..59
                const double cx = ig_cell_centre(i), cy = ig_cell_centre(j);
                const double dx = cx - px, dy = cy - py;
                if (dx * dx + dy * dy <= r2_pre && ig_check_visibility(d2, px, py, cx, cy)) seen |= 1ull << t;
            }
        }
        // 2. H passes of box test, cone test and add over the lane's own candidates
        double bg = 0.0;
        int bh = 0;
        for (int h = 0; h < P.H; h++) {
            const double s = __shfl(my_s, 3 * h), c = __shfl(my_c, 3 * h);
            int bxs, bys, bxe, bye;
            ig_visible_box_sc(px, py, P.range, s, c, __shfl(my_s, 3 * h + 1), __shfl(my_c, 3 * h + 1), __shfl(my_s, 3 * h + 2),
                              __shfl(my_c, 3 * h + 2), bxs, bys, bxe, bye);
            double acc = 0.0;
            int cnt = 0;
            for (int t = 0; t < trips; t++) {
                if ((seen >> t) & 1ull) {
                    const int q = lane + 64 * t;
                    const int jj = (int)(((float)q + 0.5f) * rwd);
                    const int i = xs + (q - jj * wd), j = ys + jj;
                    if (i >= bxs && i < bxe && j >= bys && j < bye) {
                        const double cxp = ig_cell_centre(i), cyp = ig_cell_centre(j);
                        double r0, r1;
                        mat2vec(c, s, cxp - px, cyp - py, r0, r1);
                        if (ig_in_cone(r0, r1, cn, r2_in, r2_out, P.fov, P.range)) {
                            acc += s_mi[j * IG_BEL + i];
                            cnt++;
                        }
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {  // a fixed tree: fp64 addition commutes, every lane ends with the same sum
                acc += __shfl_xor(acc, off);
                cnt += __shfl_xor(cnt, off);
            }
            if (h == 0 || acc > bg) {  // the first of equal maxima
                bg = acc;
                bh = h;
            }
            if (lane == 0) {
                if (gain_h) gain_h[o * P.H + h] = acc;
                if (n_visible_h) n_visible_h[o * P.H + h] = cnt;
            }
        }
        if (lane == 0) {
            best_heading[o] = bh;
            best_gain[o] = bg;
            valid[o] = 1;
        }
    }
}

// Directly behind k_ig_goal_actions: a robot with an active goal and a finite goal heading that stands within goal_tol of the goal
// point - the predicate, in the statements, on which k_ig_goal_actions stops it - turns on the spot towards that heading; every
// other row keeps its bytes.
__global__ void __launch_bounds__(64) k_ig_goal_face_actions(CagymDev D, IgGoalParams P, const double* __restrict__ goal_xy,
                                                             const uint8_t* __restrict__ active,
                                                             const double* __restrict__ goal_heading, float* actions) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int rank = ig_robot_rank(D, w, lane, P.R);
    if (rank < 0) return;
    const size_t wr = (size_t)w * P.R + rank, a = (size_t)w * D.M + lane;
    if (!active[wr]) return;
    const double gh = goal_heading[wr];
    if (!isfinite(gh)) return;
    const double x = D.px[a], y = D.py[a], th = D.heading[a];
    const double gx = goal_xy[2 * wr], gy = goal_xy[2 * wr + 1];
    const double dx = gx - x, dy = gy - y;
    const double dist = sqrt(dx * dx + dy * dy);
    if (!(dist <= P.goal_tol)) return;
    const double om = clipd(igg_wrap(gh - th) / P.dt, -P.w_max, P.w_max);
    reinterpret_cast<float2*>(actions)[a] = make_float2(0.f, (float)om);
}

// Directly behind k_ig_goal_status, on the `active` it left: 1 when the robot is within goal_tol of an active goal and either has
// no finite goal heading or faces it within face_tol.
__global__ void __launch_bounds__(64) k_ig_goal_face_status(CagymDev D, IgGoalParams P, double face_tol,
                                                            const double* __restrict__ goal_xy, const uint8_t* __restrict__ active,
                                                            const double* __restrict__ goal_heading, uint8_t* goal_facing) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const int rank = ig_robot_rank(D, w, lane, P.R);
    if (rank < 0) return;
    const size_t wr = (size_t)w * P.R + rank, a = (size_t)w * D.M + lane;
    bool facing = false;
    if (active[wr]) {
        const double x = D.px[a], y = D.py[a], th = D.heading[a];
        const double dx = goal_xy[2 * wr] - x, dy = goal_xy[2 * wr + 1] - y;
        if (sqrt(dx * dx + dy * dy) <= P.goal_tol) {
            const double gh = goal_heading[wr];
            facing = !isfinite(gh) || fabs(igg_wrap(gh - th)) <= face_tol;
        }
    }
    goal_facing[wr] = facing ? 1 : 0;
}
