// cagym_sensors.h -- the stand-alone sensor kernels, on the state in HBM: LaserScan, OccupancyGrid and the obstacle rasteriser.
// Included by cagym_api.hip only.
#pragma once
#include "cagym_device.h"

// LaserScanSensor.sense (sensors/LaserScanSensor.py:9-22,27-58), beam b of an agent at (px, py, heading h) with
// `radius`: 16 samples at 2 pi / 16 m into the bit-packed raster `map` (null = empty map), the agent's own disk masked,
// the LAST sample whose running hit count is 1 gives the range.
__device__ __forceinline__ float laserscan_beam(const uint32_t* map, double px, double py, double h, double radius, int b) {
    int egx, egy;
    const bool ego_in = world_to_cell(px, py, egx, egy);
    const double rr = radius / 0.1, r2 = rr * rr;
    const double astep = (kPi - (-kPi)) / 15.0, rstep = 2 * kPi / 16;
    const double ang0 = b == 15 ? kPi : (double)b * astep + (-kPi);
    double sa, ca;
    sincos(ang0 + h, &sa, &ca);
    // all 16 raster words of the beam are requested before the first one is looked at (16 gathers in flight instead of
    // one after the other: the raster is L2-resident, the latency is what costs)
    uint32_t word[16];
    int bit[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        double rg = 0.0 + (double)k * rstep;
        double x = px + rg * ca, y = py + rg * sa;
        int gx, gy;
        bool in = map && world_to_cell(x, y, gx, gy);
        bool masked = false;
        if (in && ego_in) {
            double dx = (double)(gy - egy), dy = (double)(gx - egx);
            masked = dx * dx + dy * dy < r2;
        }
        in = in && !masked;
        bit[k] = in ? (gy & 31) : -1;
        word[k] = in ? map[gx * CAGYM_MAPW + (gy >> 5)] : 0u;
    }
    int count = 0, last = -1;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const bool hit = bit[k] >= 0 && ((word[k] >> (bit[k] & 31)) & 1u);
        count += hit ? 1 : 0;
        if (count == 1) last = k;
    }
    double range = last >= 0 ? 0.0 + (double)last * rstep : 6.0;
    return (float)(1 - range / 6);
}

// one lane per (agent, beam) of the state in HBM (cagym_laserscan, cagym_reset)
__global__ void __launch_bounds__(256) k_laserscan(CagymDev D, float* out) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)D.N * D.M * 16;
    if (gid >= total) return;
    const size_t a = gid >> 4;
    const int b = (int)(gid & 15);
    const int world = (int)(a / D.M), slot = (int)(a - (size_t)world * D.M);
    if (slot >= D.n_agents[world]) { out[gid] = 0.f; return; }
    const int sidx = (int)(((long long)world + (long long)D.episode[world] * D.N) % D.S);
    const uint32_t* map = (D.map_bits && D.sc_nobst[sidx] > 0) ? D.map_bits + (size_t)sidx * CAGYM_MAPD * CAGYM_MAPW : nullptr;
    out[gid] = laserscan_beam(map, D.px[a], D.py[a], D.heading[a], D.radius[a], b);
}

// OccupancyGridSensor.sense (sensors/OccupancyGridSensor.py:70-98, 131-143; Map.getSubmapByIndices Map.py:81-105):
// the occupancy raster rotated about the agent's cell by -heading (cv2.getRotationMatrix2D + cv2.warpAffine,
// bilinear, constant-0 border), 60x60 window around the agent, astype(bool).  One workgroup per agent, 3600 cells.
// warpAffine restated from OpenCV 4.x imgproc (fixed point: AB_BITS 10, INTER_BITS 5, round_delta 16, cvRound =
// round half to even); cv2 is absent here, so this sensor is "parity unpinned" (oracle twin: cagym_oracle_grid.c).
__device__ __forceinline__ int og_src(const uint32_t* map, int x, int y) {  // x = column, y = row; border 0
    if (x < 0 || y < 0 || x >= CAGYM_MAPD || y >= CAGYM_MAPD) return 0;
    return map_bit(map, y, x) ? 1 : 0;
}
__device__ __forceinline__ int og_submap_start(int c) {
    long long si = (long long)((double)c - floor(60 / 2.0));  // int(): truncation toward zero
    if (si < 0) si = 0;
    if (si + 60 > CAGYM_MAPD - 1) si = CAGYM_MAPD - 1 - 60;
    return (int)si;
}
__global__ void __launch_bounds__(256) k_occupancy_grid(CagymDev D, uint8_t* out) {
    const size_t a = blockIdx.x;
    const int world = (int)(a / D.M), slot = (int)(a - (size_t)world * D.M);
    uint8_t* o = out + a * 3600;
    const int sidx = (int)(((long long)world + (long long)D.episode[world] * D.N) % D.S);
    const bool live = slot < D.n_agents[world] && D.map_bits && D.sc_nobst[sidx] > 0;
    if (!live) {  // inactive slot or empty map: all free
        for (int q = threadIdx.x; q < 3600; q += blockDim.x) o[q] = 0;
        return;
    }
    const uint32_t* map = D.map_bits + (size_t)sidx * CAGYM_MAPD * CAGYM_MAPW;
    int gx, gy;
    world_to_cell(D.px[a], D.py[a], gx, gy);
    const int sx0 = og_submap_start(gx), sy0 = og_submap_start(gy);
    double angle = -D.heading[a] * 180 / kPi;
    angle *= kPi / 180;
    double beta, alpha;
    sincos(angle, &beta, &alpha);
    const double cx = (double)gy, cy = (double)gx;
    double M0 = alpha, M1 = beta, M2 = (1 - alpha) * cx - beta * cy, M3 = -beta, M4 = alpha, M5 = beta * cx + (1 - alpha) * cy;
    double Dt = M0 * M4 - M1 * M3;
    Dt = Dt != 0 ? 1. / Dt : 0;
    const double A11 = M4 * Dt, A22 = M0 * Dt;
    M0 = A11; M1 *= -Dt;
    M3 *= -Dt; M4 = A22;
    const double b1 = -M0 * M2 - M1 * M5;
    const double b2 = -M3 * M2 - M4 * M5;
    M2 = b1; M5 = b2;
    for (int q = threadIdx.x; q < 3600; q += blockDim.x) {
        const int r = q / 60, c = q - r * 60;
        const int y = sx0 + r, x = sy0 + c;
        const int X0 = __double2int_rn((M1 * y + M2) * 1024) + 16;
        const int Y0 = __double2int_rn((M4 * y + M5) * 1024) + 16;
        const int X = (X0 + __double2int_rn(M0 * x * 1024)) >> 5;
        const int Y = (Y0 + __double2int_rn(M3 * x * 1024)) >> 5;
        const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
        int v = og_src(map, sx, sy);
        if (fx) v |= og_src(map, sx + 1, sy);
        if (fy) v |= og_src(map, sx, sy + 1);
        if (fx && fy) v |= og_src(map, sx + 1, sy + 1);
        o[q] = (uint8_t)v;
    }
}

// Map.get_occupancy_grid (Map.py:107-123) of pool row s, bit-packed output, by the whole workgroup: every lane of it makes the call
// (it holds workgroup barriers).  The rectangle rows must be visible to the workgroup on entry.
__device__ __forceinline__ void rasterize_scenario(const double* obst, const int32_t* nobst, int Kobs, uint32_t* map_bits, int s) {
    uint32_t* map = map_bits + (size_t)s * CAGYM_MAPD * CAGYM_MAPW;
    for (int q = threadIdx.x; q < CAGYM_MAPD * CAGYM_MAPW; q += blockDim.x) map[q] = 0u;
    __syncthreads();
    const int n = nobst[s];
    for (int o = 0; o < n; o++) {
        const double* ob = obst + ((size_t)s * Kobs + o) * 4;
        int s0, s1, e0, e1;
        world_to_cell(ob[0], ob[3], s0, s1);  // corner[1] = (xl, yu)
        world_to_cell(ob[2], ob[1], e0, e1);  // corner[3] = (xu, yl)
        if (s0 < -CAGYM_MAPD) s0 = -CAGYM_MAPD;
        if (s1 < -CAGYM_MAPD) s1 = -CAGYM_MAPD;
        if (e0 > CAGYM_MAPD - 1) e0 = CAGYM_MAPD - 1;
        if (e1 > CAGYM_MAPD - 1) e1 = CAGYM_MAPD - 1;
        const int h = e0 - s0 + 1, w = e1 - s1 + 1;
        if (h <= 0 || w <= 0) continue;
        for (int q = threadIdx.x; q < h * w; q += blockDim.x) {
            int ii = s0 + q / w, jj = s1 + q % w;
            int a = ii < 0 ? ii + CAGYM_MAPD : ii, b = jj < 0 ? jj + CAGYM_MAPD : jj;  // Python negative-index wrap
            if (a < 0 || b < 0 || a >= CAGYM_MAPD || b >= CAGYM_MAPD) continue;
            atomicOr(&map[a * CAGYM_MAPW + (b >> 5)], 1u << (b & 31));
        }
        __syncthreads();
    }
}

// one workgroup per scenario of the pool (k_stream_refill, csrc/cagym_stream.h, rasterises the slots it refills itself)
__global__ void __launch_bounds__(256) k_rasterize(const double* obst, const int32_t* nobst, int Kobs, uint32_t* map_bits) {
    rasterize_scenario(obst, nobst, Kobs, map_bits, blockIdx.x);
}
