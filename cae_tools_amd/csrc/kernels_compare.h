// kernels_compare.h - models compared on the same pixels, and the bootstrap of a per-case table of sums (include/cae_hip.h,
// cae_case_compare and cae_bootstrap_sums).
//
// k_case_compare: the target and up to CP_MAX predictions of a pixel are read once.  A pixel is a pair when the target and
// every prediction are finite; e_m = P_m - a and q_m = e_m * e_m are rounded on their own, nothing is contracted.  The
// mapping is k_case_importance's without the map: the plane is cut into tiles of CP_TILE = 64 consecutive pixels, lane l of a
// wave owns pixel tile * 64 + l, the wave sums each addend of its tile in the fixed DPP tree (wave_sum_lane63; the counts are
// the population of a ballot, exact) and lane 63 stores them to part[case][tile][2 + 4 M]; k_compare_fold adds a case's
// tiles: lane j of a wave takes tiles j, j + 64, ... in ascending order, then the same tree.  Tile size, both trees and the
// lane order depend on the plane alone, so a case's sums do not depend on the other cases of the call, on n_case or on the
// alignment of the operands.  One wave per (tile, run of CP_RUN cases).  No LDS, no atomics.  MM is the number of predictions
// the loops are unrolled for (2, 4 or 8); the predictions beyond n_pred are skipped by wave-uniform tests, so every array is
// indexed by constants and lives in registers.
//
// k_bootstrap_sums: T[r][c] = S[j(r, 0)][c] + S[j(r, 1)][c] + ... in that order with plain rounded adds from +0.0, the unit
// j(r, i) a counter-based draw (bs_unit: splitmix64 at position (r << 32 | i) + 1, the high 32 bits scaled to n_unit), so
// the bits depend on (S, seed, r) alone.  A lane owns a resample and CG consecutive columns; every lane of a resample forms
// the same units.  LDS: the table is copied to LDS by every workgroup first and the draws read it there; else they read it
// through L2.
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int CP_TILE = 64;             // pixels per tile: one per lane
constexpr int CP_MAX = 8;               // predictions a call
constexpr int CP_RUN = 8;               // cases per work item
constexpr int CP_WAVES = 4;             // waves per 256-thread workgroup

struct CpArgs {
    const unsigned char* p[CP_MAX];
    long long p_stride[CP_MAX];                         // elements from one case to the next
    const unsigned char* a;
    long long a_stride;
    long long n_case, plane, n_tile, items;
    int n_pred, width;                                  // width = 2 + 4 * n_pred
    double* part;                                       // [n_case][n_tile][width]
};

__device__ __forceinline__ bool cp_finite(double v) { return (v - v) == 0.0; }

__device__ __forceinline__ double cp_count(bool yes) { return (double)__popcll(__ballot(yes)); }

template <int KP, int KA, int MM>
__global__ void __launch_bounds__(64 * CP_WAVES) k_case_compare(const CpArgs s) {
#pragma clang fp contract(off)
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    const int lane = threadIdx.x & 63;
    for (long long item = (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6); item < s.items;
         item += (long long)gridDim.x * CP_WAVES) {
        const long long run = item / s.n_tile, tile = item - run * s.n_tile;
        const long long c0 = run * CP_RUN, c1 = c0 + CP_RUN < s.n_case ? c0 + CP_RUN : s.n_case;
        const long long px = tile * CP_TILE + lane;
        const bool inside = px < s.plane;
        const long long pl = inside ? px : s.plane - 1;     // a clamped pixel: every load has a valid address, no predicate
        for (long long cs = c0; cs < c1; cs++) {
            const double av = cm_load1<KA>(s.a + cs * s.a_stride * EA, pl);
            double pv[MM];
#pragma unroll
            for (int m = 0; m < MM; m++) pv[m] = m < s.n_pred ? cm_load1<KP>(s.p[m] + cs * s.p_stride[m] * EP, pl) : 0.0;
            bool pair = inside && cp_finite(av);
#pragma unroll
            for (int m = 0; m < MM; m++) pair = pair && cp_finite(pv[m]);
            double e[MM], q[MM];
#pragma unroll
            for (int m = 0; m < MM; m++) {
                e[m] = pair ? pv[m] - av : 0.0;
                q[m] = e[m] * e[m];
            }
            double qmin = q[0];
#pragma unroll
            for (int m = 1; m < MM; m++) qmin = (m < s.n_pred && q[m] < qmin) ? q[m] : qmin;
            int hits = 0;
#pragma unroll
            for (int m = 0; m < MM; m++) hits += (m < s.n_pred && q[m] == qmin) ? 1 : 0;
            double* out = s.part + (cs * s.n_tile + tile) * s.width;
            const double n = cp_count(pair), tied = cp_count(pair && hits > 1);
            if (lane == 63) *reinterpret_cast<double2*>(out) = make_double2(n, tied);
#pragma unroll
            for (int m = 0; m < MM; m++) {
                if (m < s.n_pred) {         // wave-uniform
                    const double se = wave_sum_lane63(e[m]);
                    const double sa = wave_sum_lane63(fabs(e[m]));
                    const double sq = wave_sum_lane63(q[m]);
                    const double wins = cp_count(pair && hits == 1 && q[m] == qmin);
                    if (lane == 63) {
                        double2* o = reinterpret_cast<double2*>(out + 2 + 4 * m);
                        o[0] = make_double2(se, sa);
                        o[1] = make_double2(sq, wins);
                    }
                }
            }
        }
    }
}

// sums[case][k] = the case's tiles added: lane j takes tiles j, j + 64, ... in ascending order, then the DPP tree.  One wave
// per case.
template <int MM>
__global__ void __launch_bounds__(64 * CP_WAVES) k_compare_fold(const double* __restrict__ part, long long n_case, long long n_tile,
                                                                int width, double* __restrict__ sums) {
    constexpr int HALF = 1 + 2 * MM;        // double2s of the widest row
    const int lane = threadIdx.x & 63;
    for (long long cs = (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6); cs < n_case; cs += (long long)gridDim.x * CP_WAVES) {
        double acc[2 * HALF];
#pragma unroll
        for (int k = 0; k < 2 * HALF; k++) acc[k] = 0.0;
        const double* src = part + cs * n_tile * width;
        for (long long t = lane; t < n_tile; t += 64) {
            const double2* row = reinterpret_cast<const double2*>(src + t * width);
#pragma unroll
            for (int k = 0; k < HALF; k++) {
                if (2 * k < width) {
                    const double2 v = row[k];
                    acc[2 * k] = acc[2 * k] + v.x;
                    acc[2 * k + 1] = acc[2 * k + 1] + v.y;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2 * HALF; k++) {
            if (k < width) {
                const double v = wave_sum_lane63(acc[k]);
                if (lane == 63) sums[cs * width + k] = v;
            }
        }
    }
}

// ---- the bootstrap -------------------------------------------------------------------------------------------------------

constexpr int BS_THREADS = 256;
constexpr int BS_MAX_COL = 32;
constexpr int BS_MAX_UNIT = 1 << 20;
constexpr int BS_LDS_BYTES = 160 * 1024;        // a table up to all of a CU's LDS is staged there
constexpr long long BS_WIDE_ITEMS = 1 << 17;    // from so many (resample, 4 columns) lanes on a lane takes 4 columns, else 1

struct BsArgs {
    const double* table;        // [n_unit][n_col]
    double* out;                // [n_resample][n_col]
    unsigned long long seed;
    long long first, n_resample, items;
    int n_unit, n_col, n_group;
};

__device__ __forceinline__ unsigned long long bs_mix64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the unit of draw i of resample r: below n_unit, because the high word of u * n_unit with u < 2^32 is
__device__ __forceinline__ unsigned bs_unit(unsigned long long seed, unsigned r, unsigned i, unsigned n_unit) {
    const unsigned long long x = ((unsigned long long)r << 32) | i;
    const unsigned long long z = bs_mix64(seed + (x + 1ull) * 0x9E3779B97F4A7C15ull);
    return (unsigned)(((z >> 32) * (unsigned long long)n_unit) >> 32);
}

template <int CG, bool LDS>
__global__ void __launch_bounds__(BS_THREADS) k_bootstrap_sums(const BsArgs s) {
#pragma clang fp contract(off)
    extern __shared__ double bs_table[];
    if (LDS) {
        const int total = s.n_unit * s.n_col;
        for (int i = threadIdx.x; i < total; i += BS_THREADS) bs_table[i] = s.table[i];
        __syncthreads();
    }
    const double* table = LDS ? bs_table : s.table;
    for (long long item = (long long)blockIdx.x * BS_THREADS + threadIdx.x; item < s.items; item += (long long)gridDim.x * BS_THREADS) {
        const long long k = item / s.n_group;
        const int c0 = (int)(item - k * s.n_group) * CG;
        const unsigned r = (unsigned)(s.first + k);
        int col[CG];            // clamped: a lane beyond the last column reads the last one and stores nothing
        double t[CG];
#pragma unroll
        for (int u = 0; u < CG; u++) {
            col[u] = c0 + u < s.n_col ? c0 + u : s.n_col - 1;
            t[u] = 0.0;
        }
#pragma unroll 4
        for (unsigned i = 0; i < (unsigned)s.n_unit; i++) {
            const double* row = table + (long long)bs_unit(s.seed, r, i, (unsigned)s.n_unit) * s.n_col;
#pragma unroll
            for (int u = 0; u < CG; u++) t[u] = t[u] + row[col[u]];
        }
#pragma unroll
        for (int u = 0; u < CG; u++)
            if (c0 + u < s.n_col) s.out[k * s.n_col + c0 + u] = t[u];
    }
}

}  // namespace cae
