// kernels_blend.h - the error moments a weighted blend of models is fitted from, and the blended field (include/cae_hip.h,
// cae_case_error_moments and cae_blend_predictions; DESIGN.md section 9, "Model blending").
//
// k_case_error_moments: k_case_compare's pass with the cross terms.  The target and up to CP_MAX predictions of a pixel are
// read once; a pixel is a pair when the target and every prediction are finite; e_m = P_m - a and every product e_i * e_j
// (i <= j) are rounded on their own, nothing is contracted.  The mapping is k_case_compare's: tiles of CP_TILE = 64
// consecutive pixels, lane l owns pixel tile * 64 + l, the wave sums each addend of its tile in the fixed DPP tree
// (wave_sum_lane63; the count is the population of a ballot) and lane 63 stores them to part[case][tile][pitch], the row
// {n, S e_m (M of them), S e_i e_j for i <= j in row-major order} padded to an even pitch; k_moments_fold adds a case's tiles
// as k_compare_fold does: lane j takes tiles j, j + 64, ... in ascending order, then the same tree.  So n, S e_m and S e_m^2
// carry the bits of cae_case_compare's columns, and a case's row depends on its own plane alone.  One wave per (tile, run of
// CP_RUN cases).  No LDS, no atomics.  MM is the number of predictions the loops are unrolled for (2, 4 or 8); the
// predictions beyond n_pred are skipped by wave-uniform tests, so every register array is indexed by constants.
//
// k_blend_predictions: y = c, then y = y + w_m * P_m for the candidates the host kept (weight not 0) in ascending order, the
// product and the sum rounded separately; NaN where a kept candidate is not finite.  Pure streaming: a lane owns four
// consecutive elements of a case, read and written with 16-byte accesses where the host found every operand aligned for
// them; the ragged last four of a case take clamped scalar loads and guarded stores.
#pragma once
#include "kernels_compare.h"

namespace cae {

constexpr int BD_THREADS = 256;         // of k_blend_predictions; a lane takes BD_VEC elements at a time
constexpr int BD_VEC = 4;

struct BdMoments {
    const unsigned char* p[CP_MAX];
    long long p_stride[CP_MAX];                         // elements from one case to the next
    const unsigned char* a;
    long long a_stride;
    long long n_case, plane, n_tile, items;
    int n_pred, width, pitch;                           // width = 1 + M + M (M + 1) / 2, pitch = width rounded up to even
    double* part;                                       // [n_case][n_tile][pitch]
};

template <int KP, int KA, int MM>
__global__ void __launch_bounds__(64 * CP_WAVES) k_case_error_moments(const BdMoments s) {
#pragma clang fp contract(off)
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    const int lane = threadIdx.x & 63;
    const int M = s.n_pred;
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
            for (int m = 0; m < MM; m++) pv[m] = m < M ? cm_load1<KP>(s.p[m] + cs * s.p_stride[m] * EP, pl) : 0.0;
            bool pair = inside && cp_finite(av);
#pragma unroll
            for (int m = 0; m < MM; m++) pair = pair && cp_finite(pv[m]);
            double e[MM];
#pragma unroll
            for (int m = 0; m < MM; m++) e[m] = pair ? pv[m] - av : 0.0;
            double* out = s.part + (cs * s.n_tile + tile) * s.pitch;
            const double n = cp_count(pair);
            if (lane == 63) {
                out[0] = n;
                if (s.pitch != s.width) out[s.width] = 0.0;
            }
#pragma unroll
            for (int m = 0; m < MM; m++) {
                if (m < M) {                // wave-uniform
                    const double se = wave_sum_lane63(e[m]);
                    if (lane == 63) out[1 + m] = se;
                }
            }
#pragma unroll
            for (int i = 0; i < MM; i++) {
#pragma unroll
                for (int j = i; j < MM; j++) {
                    if (j < M) {            // wave-uniform; row i of the upper triangle starts at i M - i (i - 1) / 2
                        const double prod = e[i] * e[j];
                        const double sp = wave_sum_lane63(prod);
                        if (lane == 63) out[1 + M + i * M - (i * (i - 1)) / 2 + (j - i)] = sp;
                    }
                }
            }
        }
    }
}

// sums[case][k] = the case's tiles added: lane j takes tiles j, j + 64, ... in ascending order, then the DPP tree.  One wave
// per case.
template <int MM>
__global__ void __launch_bounds__(64 * CP_WAVES) k_moments_fold(const double* __restrict__ part, long long n_case, long long n_tile,
                                                                int width, int pitch, double* __restrict__ sums) {
#pragma clang fp contract(off)
    constexpr int WMAX = 1 + MM + MM * (MM + 1) / 2;
    constexpr int HALF = (WMAX + 1) / 2;    // double2s of the widest row
    const int lane = threadIdx.x & 63;
    for (long long cs = (long long)blockIdx.x * CP_WAVES + (threadIdx.x >> 6); cs < n_case; cs += (long long)gridDim.x * CP_WAVES) {
        double acc[2 * HALF];
#pragma unroll
        for (int k = 0; k < 2 * HALF; k++) acc[k] = 0.0;
        const double* src = part + cs * n_tile * pitch;
        for (long long t = lane; t < n_tile; t += 64) {
            const double2* row = reinterpret_cast<const double2*>(src + t * pitch);
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

// ---- the blended field ---------------------------------------------------------------------------------------------------

struct BdField {
    const unsigned char* p[CP_MAX];                     // the kept candidates, ascending
    long long p_stride[CP_MAX];
    double w[CP_MAX];
    double c;
    long long per, n_quad, items, out_stride;           // elements of a case, quads of a case, n_case * n_quad
    double* out;
    int n_kept, vec;                                    // vec: 16-byte accesses are aligned for every operand and the output
};

template <int KP, int MM>
__global__ void __launch_bounds__(BD_THREADS) k_blend_predictions(const BdField s) {
#pragma clang fp contract(off)
    constexpr int EP = CmElem<KP>::bytes;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (long long item = (long long)blockIdx.x * BD_THREADS + threadIdx.x; item < s.items; item += (long long)gridDim.x * BD_THREADS) {
        const long long cs = item / s.n_quad, e0 = (item - cs * s.n_quad) * BD_VEC;
        const bool full = e0 + BD_VEC <= s.per;
        double y[BD_VEC];
        bool ok[BD_VEC];
#pragma unroll
        for (int j = 0; j < BD_VEC; j++) y[j] = s.c, ok[j] = true;
#pragma unroll
        for (int m = 0; m < MM; m++) {
            if (m < s.n_kept) {             // uniform
                const unsigned char* base = s.p[m] + cs * s.p_stride[m] * EP;
                double v[BD_VEC];
                if (full) {
                    cm_load4<KP>(base, e0, s.vec != 0, v);
                } else {                    // the ragged end of a case: clamped loads, the stores below are guarded
#pragma unroll
                    for (int j = 0; j < BD_VEC; j++) v[j] = cm_load1<KP>(base, e0 + j < s.per ? e0 + j : s.per - 1);
                }
#pragma unroll
                for (int j = 0; j < BD_VEC; j++) {
                    const double prod = s.w[m] * v[j];
                    y[j] = y[j] + prod;
                    ok[j] = ok[j] && cp_finite(v[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BD_VEC; j++) y[j] = ok[j] ? y[j] : nan;
        double* o = s.out + cs * s.out_stride + e0;
        if (full && s.vec) {
            reinterpret_cast<double2*>(o)[0] = make_double2(y[0], y[1]);
            reinterpret_cast<double2*>(o)[1] = make_double2(y[2], y[3]);
        } else {
#pragma unroll
            for (int j = 0; j < BD_VEC; j++)
                if (e0 + j < s.per) o[j] = y[j];
        }
    }
}

}  // namespace cae
