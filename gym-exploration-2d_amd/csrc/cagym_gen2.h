// cagym_gen2.h -- on-device samplers of the reference's training scenarios (include/cagym.h: cagym_generate_reference_scenarios).
// Restates train_agents_swap_circle / _pairwise_swap / _random_positions (test_cases.py:1192-1463) and train_stage_1 / _2
// (:2359-2572) with is_pose_valid (:129-133), is_pose_valid_with_obstacles (:135-148) and is_shape_valid (:150-170).  One lane per
// scenario, bounded rejection sampling on cagym_gen.h's counter-based generator; the draw order of every kind is documented in
// include/cagym.h.  The CPU twin is tests/sampler_twin.py.  The scenario's rows in HBM double as the sampler's memory of what it
// placed (earlier starts / goals / rectangles are read back from there).
#pragma once
#include "cagym_gen.h"

struct Gen2Dev {
    GenDev G;
    double* obst;   // [S, K, 4] xl, yl, xu, yu (NULL when K == 0)
    float* prep;    // [S, K, 16] RVO prep rows (cagym_set_scenarios' layout)
    int K;
};

// per-kind constants of the reference's samplers
struct Gen2Kind {
    double sq_lo, sq_hi, c_lo, c_hi, d_lo, d_hi;
    int nob_min, nob_max;
};

__device__ __forceinline__ double gen2_uniform(uint64_t seed, uint32_t s, uint32_t& k, double lo, double hi) {
    return lo + (hi - lo) * gen_u01(seed, s, k++);  // np.random.uniform(low, high)
}
// c(lo, hi) of include/cagym.h: random.randint(lo, hi)
__device__ __forceinline__ int gen2_count(uint64_t seed, uint32_t s, uint32_t& k, int lo, int hi) {
    int n = lo + (int)(gen_u01(seed, s, k++) * (double)(hi - lo + 1));
    return n < lo ? lo : (n > hi ? hi : n);
}
// np.linalg.norm(a - b) < dist in plain fp64 (no contraction: the twin computes the same bits)
__device__ __forceinline__ bool gen2_near(double ax, double ay, double bx, double by, double dist) {
    const double dx = ax - bx, dy = ay - by;
    return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))) < dist;
}
// is_pose_valid_with_obstacles (test_cases.py:135-148): 1 m clear of every rectangle, the reference's comparisons
__device__ __forceinline__ bool gen2_clear(const double* ob, int n, double x, double y) {
    for (int j = 0; j < n; j++) {
        const double* r = ob + 4 * j;
        if (!(x >= r[2] + 1.0 || y >= r[3] + 1.0 || x <= r[0] - 1.0 || y <= r[1] - 1.0)) return false;
    }
    return true;
}

__device__ __forceinline__ void gen2_row(double* a, double sx, double sy, double gx, double gy) {
    a[0] = sx; a[1] = sy; a[2] = gx; a[3] = gy; a[4] = 1.0; a[5] = 0.5;  // pref_speed 1.0, radius 0.5 (every sampler)
}

// policies of slots 1..n-1 (slot order), dynamics, coop; slot 0 = the ego; empty slots as cagym_generate_scenarios leaves them
__device__ __forceinline__ void gen2_assign(const Gen2Dev& D, const cagym_gen2_params& P, uint32_t v, uint32_t s, uint32_t& k, int n,
                                            int pol_a, int pol_b, double p_b, int ego_dyn, double coop_ego, double coop_other) {
    const int M = D.G.M;
    for (int i = 0; i < M; i++) {
        int32_t pol = CAGYM_POL_STATIC, dyn = CAGYM_DYN_UNICYCLE;
        double coop = coop_other;
        if (i == 0 && n > 0) {
            pol = P.ego_policy;
            dyn = ego_dyn;
            coop = coop_ego;
        } else if (i < n) {
            pol = gen_u01(P.seed, v, k++) < p_b ? pol_b : pol_a;
            dyn = P.other_dynamics;
        } else {
            gen2_row(D.G.agents6 + ((size_t)s * M + i) * 6, 0.0, 0.0, 0.0, 0.0);
        }
        D.G.policy[(size_t)s * M + i] = pol;
        D.G.dyn[(size_t)s * M + i] = dyn;
        D.G.coop[(size_t)s * M + i] = coop;
    }
    D.G.nagents[s] = n;
}

// train_agents_swap_circle (tc.py:1192-1282)
__device__ int gen2_swap_circle(const Gen2Dev& D, const cagym_gen2_params& P, uint32_t v, uint32_t s, int nmax, int pa, int pb, double p_b,
                                int ego_dyn) {
    double* A = D.G.agents6 + (size_t)s * D.G.M * 6;
    uint32_t k = 0;
    const int c = gen2_count(P.seed, v, k, 2, nmax);
    const int n = P.fixed_count ? nmax : c;
    const int na = 2 * (n / 2);
    int failed = 0;
    for (int p = 0; p < na / 2; p++) {
        double x = 0, y = 0;
        bool ok = false;
        for (int tries = 0; tries < P.max_tries && !ok; tries++) {
            const double d = gen2_uniform(P.seed, v, k, 4.0, 8.0);
            const double ang = gen2_uniform(P.seed, v, k, -M_PI, M_PI);
            x = d * cos(ang);
            y = d * sin(ang);
            ok = true;
            for (int j = 0; j < 2 * p && ok; j++) {  // the earlier starts are positions_list (every earlier goal is one of them)
                const double* b = A + 6 * j;
                if (gen2_near(-x, -y, b[0], b[1], 1.5) || gen2_near(x, y, b[0], b[1], 1.5)) ok = false;
            }
        }
        if (!ok) failed += 2;
        gen2_row(A + 6 * (2 * p), -x, -y, x, y);
        gen2_row(A + 6 * (2 * p + 1), x, y, -x, -y);
    }
    gen2_assign(D, P, v, s, k, na, pa, pb, p_b, ego_dyn, 1.0, 0.5);
    return failed;
}

// train_agents_pairwise_swap (tc.py:1283-1364); the drawn positions wait in the start columns of slots 0..n-1
__device__ int gen2_pairwise_swap(const Gen2Dev& D, const cagym_gen2_params& P, uint32_t v, uint32_t s, int nmax, int pa, int pb, double p_b,
                                  int ego_dyn) {
    double* A = D.G.agents6 + (size_t)s * D.G.M * 6;
    uint32_t k = 0;
    const int c = gen2_count(P.seed, v, k, 2, nmax);
    const int n = P.fixed_count ? nmax : c;
    int failed = 0;
    for (int i = 0; i < n; i++) {
        double x = 0, y = 0;
        bool ok = false;
        for (int tries = 0; tries < P.max_tries && !ok; tries++) {
            x = gen2_uniform(P.seed, v, k, -7.5, 7.5);
            y = gen2_uniform(P.seed, v, k, -7.5, 7.5);
            ok = true;
            for (int j = 0; j < i && ok; j++)
                if (gen2_near(x, y, A[6 * j], A[6 * j + 1], 2.0)) ok = false;
        }
        if (!ok) failed++;
        A[6 * i] = x;
        A[6 * i + 1] = y;
    }
    for (int i = n - 1; i >= 1; i--) {  // random.shuffle
        int j = (int)(gen_u01(P.seed, v, k++) * (double)(i + 1));
        j = j > i ? i : j;
        const double tx = A[6 * i], ty = A[6 * i + 1];
        A[6 * i] = A[6 * j];
        A[6 * i + 1] = A[6 * j + 1];
        A[6 * j] = tx;
        A[6 * j + 1] = ty;
    }
    const int na = 2 * (n / 2);
    for (int p = 0; p < na / 2; p++) {
        const double x0 = A[12 * p], y0 = A[12 * p + 1], x1 = A[12 * p + 6], y1 = A[12 * p + 7];
        gen2_row(A + 6 * (2 * p), x0, y0, x1, y1);
        gen2_row(A + 6 * (2 * p + 1), x1, y1, x0, y0);
    }
    gen2_assign(D, P, v, s, k, na, pa, pb, p_b, ego_dyn, 1.0, 0.5);
    return failed;
}

// train_stage_1 / train_stage_2 (tc.py:2359-2572)
__device__ int gen2_stage(const Gen2Dev& D, const cagym_gen2_params& P, uint32_t v, uint32_t s, const Gen2Kind& C, int nmax, int pa, int pb,
                          double p_b) {
    double* A = D.G.agents6 + (size_t)s * D.G.M * 6;
    double* ob = D.obst + (size_t)s * D.K * 4;
    uint32_t k = 0;
    // the reference's range narrowed by the caller's bounds (< 0: none); cagym_generate_reference_scenarios refuses an empty one
    const int nob_min = P.n_obst_min < 0 ? C.nob_min : max(C.nob_min, P.n_obst_min);
    const int nob_max = P.n_obst_max < 0 ? C.nob_max : min(C.nob_max, P.n_obst_max);
    const int nob = gen2_count(P.seed, v, k, nob_min, nob_max);
    int failed = 0;
    for (int r = 0; r < nob; r++) {
        double sx, sy;
        if (gen_u01(P.seed, v, k++) < 0.5) {  // np.random.choice(['square', 'rectangle'])
            sx = sy = gen2_uniform(P.seed, v, k, C.sq_lo, C.sq_hi);
        } else {
            sx = gen2_uniform(P.seed, v, k, 1.0, 4.0);
            sy = sx > 2.0 ? gen2_uniform(P.seed, v, k, 1.0, 2.0) : gen2_uniform(P.seed, v, k, 3.0, 4.0);
        }
        double xl = 0, yl = 0, xu = 0, yu = 0;
        bool ok = false;
        for (int tries = 0; tries < P.max_tries && !ok; tries++) {
            xu = gen2_uniform(P.seed, v, k, C.c_lo, C.c_hi);
            yu = gen2_uniform(P.seed, v, k, C.c_lo, C.c_hi);
            xl = xu - sx;
            yl = yu - sy;
            ok = true;
            for (int j = 0; j < r && ok; j++) {
                const double* q = ob + 4 * j;
                if (!(q[0] >= xu || xl >= q[2] || q[3] <= yl || yu <= q[1])) ok = false;
            }
        }
        if (!ok) failed++;
        ob[4 * r] = xl; ob[4 * r + 1] = yl; ob[4 * r + 2] = xu; ob[4 * r + 3] = yu;
    }
    for (int r = nob; r < D.K; r++) ob[4 * r] = ob[4 * r + 1] = ob[4 * r + 2] = ob[4 * r + 3] = 0.0;
    D.G.nobst[s] = nob;
    int n = 1;
    for (int i = 0; i < nmax; i++) {
        if (i == 1) {  // others = random.randint(1, max(number_of_agents - 1, 1)), drawn after the ego is placed
            const int hi = nmax - 1;
            const int c = gen2_count(P.seed, v, k, 1, hi);
            n = 1 + (P.fixed_count ? hi : c);
        }
        if (i >= n) break;
        double x = 0, y = 0;
        bool ok = false;
        for (int tries = 0; tries < P.max_tries && !ok; tries++) {
            const double d = gen2_uniform(P.seed, v, k, C.d_lo, C.d_hi);
            const double ang = gen2_uniform(P.seed, v, k, -M_PI, M_PI);
            x = d * cos(ang);
            y = d * sin(ang);
            ok = gen2_clear(ob, nob, x, y) && gen2_clear(ob, nob, -x, -y);
            for (int j = 0; j < i && ok; j++) {
                const double* b = A + 6 * j;
                if (gen2_near(-x, -y, b[0], b[1], 1.5) || gen2_near(-x, -y, b[2], b[3], 1.5) || gen2_near(x, y, b[0], b[1], 1.5) ||
                    gen2_near(x, y, b[2], b[3], 1.5))
                    ok = false;
            }
        }
        if (!ok) failed++;
        gen2_row(A + 6 * i, x, y, -x, -y);
    }
    gen2_assign(D, P, v, s, k, n, pa, pb, p_b, P.ego_dynamics, 1.0, 1.0);
    return failed;
}

// RVOSimulator::addObstacle prep rows of scenario s, bit for bit the host loop of cagym_set_scenarios (plain IEEE fp32, rounded
// to nearest at every operation; rows beyond n_obst are computed too, as there, and never read)
__device__ void gen2_prep(const Gen2Dev& D, uint32_t s) {
    for (int r = 0; r < D.K; r++) {
        const double* o = D.obst + ((size_t)s * D.K + r) * 4;
        float* q = D.prep + ((size_t)s * D.K + r) * 16;
        const float xl = (float)o[0], yl = (float)o[1], xu = (float)o[2], yu = (float)o[3];
        const float X[4] = {xu, xl, xl, xu}, Y[4] = {yu, yu, yl, yl};
        q[0] = xl; q[1] = yl; q[2] = xu; q[3] = yu;
        uint32_t convex = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int nx = (e + 1) & 3, pv = (e + 3) & 3;
            const float ex = __fsub_rn(X[nx], X[e]), ey = __fsub_rn(Y[nx], Y[e]);
            const float len2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
            // sqrtf and 1.0f / x correctly rounded, as on the host: through fp64, whose sqrt and division are (rounding an exact fp32
            // result's fp64 rounding to fp32 again is innocuous for these operations); the fp32 intrinsics differed in the last bit
            const float root = (float)__dsqrt_rn((double)len2);
            const float inv = (float)(1.0 / (double)root);
            q[4 + 2 * e] = __fmul_rn(ex, inv);
            q[5 + 2 * e] = __fmul_rn(ey, inv);
            const float a0 = __fsub_rn(X[pv], X[nx]), a1 = __fsub_rn(Y[pv], Y[nx]), b0 = __fsub_rn(X[e], X[pv]), b1 = __fsub_rn(Y[e], Y[pv]);
            if (__fsub_rn(__fmul_rn(a0, b1), __fmul_rn(a1, b0)) >= 0.0f) convex |= 1u << e;
        }
        q[12] = __uint_as_float(convex);
        q[13] = (xl > -14.7f && yl > -14.7f && xu < 14.7f && yu < 14.7f) ? 1.0f : 0.0f;
        q[14] = 0.0f;
        q[15] = 0.0f;
    }
}

// One scenario of the mixture P, drawn from stream key v and stored in pool row s: the kind pick, the kind's sampler, empty rectangle
// rows for a free-space kind and the RVO prep rows.  Returns the agents and rectangles whose rejection loop hit max_tries.  Every
// draw is keyed by v alone, so a row's bits depend on (P, v) and not on where it is stored (k_generate_reference_scenarios passes
// v == s; k_stream_refill, csrc/cagym_stream.h, keys a ring slot by its world's episode).
__device__ int gen2_scenario(const Gen2Dev& D, const cagym_gen2_params& P, uint32_t v, uint32_t s) {
    int kind = 0;
    {
        const int nk = __popc(P.kinds_mask);
        int pick = 0;
        if (nk > 1) {  // _init_agents' np.random.randint over the kinds, from the scenario's second stream
            pick = (int)(gen_u01(P.seed ^ 0xD1B54A32D192ED03ull, v, 0) * (double)nk);
            pick = pick >= nk ? nk - 1 : pick;
        }
        for (int b = 0, seen = 0; b < CAGYM_GEN_NKINDS; b++)
            if ((P.kinds_mask >> b) & 1u) {
                if (seen == pick) kind = b;
                seen++;
            }
    }
    const int nmax = P.number_of_agents > 2 ? P.number_of_agents : 2;
    const int ego_dyn = P.ego_policy == CAGYM_POL_GA3C ? CAGYM_DYN_MAXACC : P.ego_dynamics;  // tc.py:1256-1261, 1338-1343, 1432-1437
    const bool own = P.override_policies != 0;
    int failed = 0;
    if (kind == CAGYM_GEN_SWAP_CIRCLE || kind == CAGYM_GEN_PAIRWISE_SWAP) {
        const int pa = own ? P.policy_a : CAGYM_POL_RVO, pb = own ? P.policy_b : CAGYM_POL_NONCOOP;
        const double p_b = own ? P.p_b : 0.2;
        failed = kind == CAGYM_GEN_SWAP_CIRCLE ? gen2_swap_circle(D, P, v, s, nmax, pa, pb, p_b, ego_dyn)
                                               : gen2_pairwise_swap(D, P, v, s, nmax, pa, pb, p_b, ego_dyn);
    } else if (kind == CAGYM_GEN_RANDOM_POSITIONS) {
        cagym_gen_params Q;
        Q.seed = P.seed;
        Q.n_min = P.fixed_count ? nmax : 2;
        Q.n_max = nmax;
        Q.ego_policy = P.ego_policy;
        Q.ego_dynamics = ego_dyn;
        Q.policy_a = own ? P.policy_a : CAGYM_POL_RVO;
        Q.policy_b = own ? P.policy_b : CAGYM_POL_NONCOOP;
        Q.other_dynamics = P.other_dynamics;
        Q.max_tries = P.max_tries;
        Q.p_b = own ? P.p_b : 0.5;
        Q.side = 7.5; Q.min_travel = 4.0; Q.min_sep = 1.5; Q.radius = 0.5; Q.pref_speed = 1.0; Q.coop = 0.5;
        failed = gen_random_positions(D.G, Q, v, (int)s);
    } else {
        const Gen2Kind C = kind == CAGYM_GEN_STAGE_1 ? Gen2Kind{1.0, 3.0, -4.0, 6.0, 6.0, 8.0, 0, 4}
                                                     : Gen2Kind{1.0, 2.0, -8.0, 10.0, 8.0, 10.0, 2, 10};
        failed = gen2_stage(D, P, v, s, C, nmax, own ? P.policy_a : CAGYM_POL_RVO, own ? P.policy_b : CAGYM_POL_RVO, own ? P.p_b : 0.0);
    }
    if (kind != CAGYM_GEN_STAGE_1 && kind != CAGYM_GEN_STAGE_2) {  // free space
        D.G.nobst[s] = 0;
        for (int r = 0; r < D.K; r++) {
            double* o = D.obst + ((size_t)s * D.K + r) * 4;
            o[0] = o[1] = o[2] = o[3] = 0.0;
        }
    }
    if (D.K > 0) gen2_prep(D, s);
    return failed;
}

__global__ void __launch_bounds__(64) k_generate_reference_scenarios(Gen2Dev D, cagym_gen2_params P, int32_t* n_failed) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= D.G.S) return;
    const int failed = gen2_scenario(D, P, (uint32_t)s, (uint32_t)s);
    if (failed) atomicAdd(n_failed, failed);
}
