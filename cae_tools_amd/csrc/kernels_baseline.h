// kernels_baseline.h - device only: per-case error sums of the interpolated low-resolution input, and of the prediction on
// the same pixels, against the target (include/cae_hip.h, cae_case_baseline).  The interpolated field
// never touches memory unless the caller asks for it.  Two kinds of launch:
//   k_case_baseline<MODE, EA, EP>  (mode; bytes of an element of a and of p)
//                          a wave owns BL_COLS output columns and a band of BL_ROWS output rows.  A lane computes its
//                          column's horizontal tap indices and weights once and walks down the rows with a ring of
//                          horizontally interpolated low-resolution rows (1, 2 or 4 registers by mode); a ring slot is
//                          refreshed only when floor(src_y) advances - at ratio 16 once in 16 output rows.  The
//                          vertical taps are the same in every lane: lane l computes those of the band's row l once,
//                          and every row reads its own from that lane (v_readlane).  The low-resolution plane is read through the
//                          caches (a few kilobytes per case, shared by the case's waves); a and p stream past, four rows
//                          requested before the first is used.  {n, S|b-a|, S(b-a)^2, S|p-a|, S(p-a)^2, n_won} of the
//                          wave are stored plainly as the partial of its (case, band, strip)
//   k_baseline_fold        the partials of a case added in (band, strip) order by one lane per (case, sum)
// The walk itself - taps, ring, vertical pass - is BlWalk<MODE>, which the residual kernels (kernels_residual.h) share.
// No floating-point atomics; the cut into bands and strips depends on (h_out, w_out) alone.  Nothing is contracted into a
// fused multiply-add: the coordinates src, i and t are the host restatement's bits (tests/baseline_ref.py).
// Uses the element conversions of case_elem.h (cm_word) and the helpers of kernels_ssim.h (ss_raw, ss_value,
// ss_finite, ss_wave_sum), so it is included after that.
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int BL_COLS = 64;                 // output columns of a wave
constexpr int BL_ROWS = 64;                 // output rows of a band: at most 64, a lane holds a row's vertical taps
constexpr int BL_AHEAD = 4;                 // rows of a and p requested together
constexpr int BL_SUMS = 6;
constexpr long long BL_MAX_SIDE = 1ll << 30;

struct BlArgs {
    const unsigned char* low;               // [n_case] planes of h_in x w_in
    const unsigned char* p;                 // [n_case] planes of h_out x w_out, or NULL
    const unsigned char* a;
    long long low_stride, p_stride, a_stride;       // elements between cases
    int lk, pk, ak;                         // CAE_ELEM_* kind
    int h_in, w_in, h_out, w_out;
    double sy, sx;                          // (double)n_in / (double)n_out, divided on the host
    int n_band, n_strip;
    long long items;                        // n_case * n_band * n_strip
    double* part;                           // [items][6]
    double* field;                          // NULL or [n_case][h_out][w_out]
};

template <int MODE> struct BlMode { static constexpr int taps = MODE == 0 ? 1 : (MODE == 1 ? 2 : 4); };

// the taps of output index o on an axis of n_in samples: clamped indices, weights, and the index the ring is keyed by
// (floor(src), which every tap index follows).  The weights are the definition's cubics in factored form, so that each
// is a product of values with relative error: c1(t) = (1 - t)(1 + t - 1.25 t^2), c2(t + 1) = -0.75 t (1 - t)^2.
template <int MODE>
__device__ __forceinline__ long long bl_axis(int o, double s, int n_in, int* idx, double* w) {
#pragma clang fp contract(off)
    const double c = (double)o + 0.5;
    const long long last = n_in - 1;
    if constexpr (MODE == 0) {
        const long long f = (long long)floor(c * s);
        const long long i = f < last ? f : last;
        idx[0] = (int)i, w[0] = 1.0;
        return i;
    } else if constexpr (MODE == 1) {
        double src = c * s - 0.5;
        src = src > 0.0 ? src : 0.0;
        const long long f = (long long)floor(src);
        const long long i0 = f < last ? f : last;
        const double t = src - (double)i0;
        idx[0] = (int)i0, idx[1] = (int)(i0 + 1 < last ? i0 + 1 : last);
        w[0] = 1.0 - t, w[1] = t;
        return i0;
    } else {
        const double src = c * s - 0.5;
        const double f = floor(src);
        const long long i = (long long)f;
        const double t = src - f, u = 1.0 - t;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long q = i - 1 + k;
            idx[k] = (int)(q < 0 ? 0 : (q > last ? last : q));
        }
        w[0] = -0.75 * t * u * u;
        w[1] = u * ((1.0 + t) - 1.25 * t * t);
        w[2] = t * ((1.0 + u) - 1.25 * u * u);
        w[3] = -0.75 * u * t * t;
        return i;
    }
}

// lane r's value in every lane; r is the same in every lane
__device__ __forceinline__ int bl_lane(int v, int r) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(r)); }
__device__ __forceinline__ double bl_lane(double v, int r) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)bl_lane((int)(unsigned)b, r), hi = (unsigned)bl_lane((int)(unsigned)((unsigned long long)b >> 32), r);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// a and p in the row walk: the element size is a template argument and the byte order a select, so that no load sits in a
// branch of its own (a load behind a run-time kind switch waits for the ones before it: the walk then pays every
// memory latency in turn)
template <int E>
__device__ __forceinline__ unsigned long long bl_raw(const unsigned char* c, long long e) {
    if constexpr (E == 4) return (unsigned long long)reinterpret_cast<const unsigned*>(c)[e];
    else return reinterpret_cast<const unsigned long long*>(c)[e];
}
template <int E>
__device__ __forceinline__ double bl_value(unsigned long long raw, bool big_endian) {
    if constexpr (E == 4) {
        const unsigned w = (unsigned)raw, x = __builtin_bswap32(w);
        return (double)__uint_as_float(big_endian ? x : w);
    } else {
        const unsigned long long x = __builtin_bswap64(raw);
        return __longlong_as_double((long long)(big_endian ? x : raw));
    }
}

// r(x) of input row `row` for the lane's column: S_k wx_k v_k in ascending tap order, each product and sum rounded;
// bad: a tap that is not finite, whatever its weight
template <int T>
__device__ __forceinline__ double bl_row(const unsigned char* lc, int lk, long long row, int w_in, const int* ix, const double* wx,
                                         bool& bad) {
#pragma clang fp contract(off)
    double r = 0.0;
    bad = false;
#pragma unroll
    for (int k = 0; k < T; k++) {
        const double v = ss_value(ss_raw(lc, row * w_in + ix[k], lk), lk);
        bad = bad || !ss_finite(v);
        const double q = wx[k] * v;
        r = k == 0 ? q : r + q;
    }
    return r;
}

// The ring walk of a lane's column down a band of at most BL_ROWS output rows: the column's horizontal taps, the vertical
// taps of the band's row l in lane l, and the ring of horizontally interpolated low-resolution rows.  k_case_baseline and
// the residual kernels (kernels_residual.h) walk with it, so that both form the same bits of b.
template <int MODE>
struct BlWalk {
    static constexpr int T = BlMode<MODE>::taps;
    const unsigned char* lc;                // the case's low-resolution plane
    int lk, w_in;
    int ix[T], iyl[T];
    double wx[T], wyl[T];
    int basel, cur;                         // floor(src_y) of the lane's row; the one the ring holds
    double ring[T];                         // slot j: r(x) of the j-th vertical tap's row
    bool ring_bad[T];

    // column oxc; lane l takes the vertical taps of output row min(y0 + l, h_out - 1); the ring is filled for row y0
    __device__ __forceinline__ void start(const unsigned char* plane, int kind, int oxc, int y0, int lane, int h_in, int w_in_,
                                          int h_out, double sy, double sx) {
        lc = plane, lk = kind, w_in = w_in_;
        bl_axis<MODE>(oxc, sx, w_in, ix, wx);
        basel = (int)bl_axis<MODE>(min(y0 + lane, h_out - 1), sy, h_in, iyl, wyl);
        cur = bl_lane(basel, 0);
#pragma unroll
        for (int j = 0; j < T; j++) ring[j] = bl_row<T>(lc, lk, bl_lane(iyl[j], 0), w_in, ix, wx, ring_bad[j]);
    }

    // b of the band's row r (the same in every lane; the rows are asked for in ascending order): S_j wy_j r_j, every product
    // and sum rounded; bad: a tap that is not finite, whatever its weight
    __device__ __forceinline__ double row(int r, bool& bad) {
#pragma clang fp contract(off)
        const int base = bl_lane(basel, r);
        if (base != cur) {
            if (T > 1 && base == cur + 1) {             // one row on: slot j + 1's row is slot j's now
#pragma unroll
                for (int j = 0; j + 1 < T; j++) ring[j] = ring[j + 1], ring_bad[j] = ring_bad[j + 1];
                ring[T - 1] = bl_row<T>(lc, lk, bl_lane(iyl[T - 1], r), w_in, ix, wx, ring_bad[T - 1]);
            } else {
#pragma unroll
                for (int j = 0; j < T; j++) ring[j] = bl_row<T>(lc, lk, bl_lane(iyl[j], r), w_in, ix, wx, ring_bad[j]);
            }
            cur = base;
        }
        double b = 0.0;
        bad = false;
#pragma unroll
        for (int j = 0; j < T; j++) {
            const double q = bl_lane(wyl[j], r) * ring[j];
            b = j == 0 ? q : b + q;
            bad = bad || ring_bad[j];
        }
        return b;
    }
};

// One wave per item = (case, band, strip); four items per workgroup, no barrier, no LDS.  EA, EP: bytes of an element of a
// and of p (without a prediction p is a again, read and not used).
template <int MODE, int EA, int EP>
__global__ void __launch_bounds__(256) k_case_baseline(const BlArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.items) return;
    const int per_case = a.n_band * a.n_strip;
    const long long c = item / per_case;
    const int rem = (int)(item - c * per_case);
    const int band = rem / a.n_strip, strip = rem - band * a.n_strip;
    const int W = a.w_out, lk = a.lk;
    const bool a_be = (a.ak & 1) != 0, p_be = (a.pk & 1) != 0;
    const int ox = strip * BL_COLS + lane;
    const bool col_ok = ox < W;
    const int oxc = col_ok ? ox : W - 1;
    const int y0 = band * BL_ROWS, y1 = min(y0 + BL_ROWS, a.h_out);
    const unsigned char* lc = a.low + c * a.low_stride * (lk < 2 ? 4 : 8);
    const unsigned char* ac = a.a + c * a.a_stride * EA;
    const bool has_p = a.p != nullptr;
    const unsigned char* pc = has_p ? a.p + c * a.p_stride * EP : ac;
    double* fc = a.field ? a.field + c * ((long long)a.h_out * W) : nullptr;

    // the vertical taps of the band's rows, row y0 + l in lane l: computed once, handed to the wave row by row
    BlWalk<MODE> walk;
    walk.start(lc, lk, oxc, y0, lane, a.h_in, a.w_in, a.h_out, a.sy, a.sx);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    int cnt = 0, won = 0;

    for (int yb = y0; yb < y1; yb += BL_AHEAD) {
        unsigned long long aq[BL_AHEAD], pq[BL_AHEAD];
#pragma unroll
        for (int d = 0; d < BL_AHEAD; d++) {
            const long long e = (long long)min(yb + d, y1 - 1) * W + oxc;   // always inside the band: no predicate on a load
            aq[d] = bl_raw<EA>(ac, e);
            pq[d] = bl_raw<EP>(pc, e);
        }
#pragma unroll
        for (int d = 0; d < BL_AHEAD; d++) {
            const int oy = yb + d;
            if (oy < y1) {                  // the same in every lane
                bool bad;
                const double b = walk.row(oy - y0, bad);
                const double av = bl_value<EA>(aq[d], a_be);
                const double pv = has_p ? bl_value<EP>(pq[d], p_be) : 0.0;
                if (col_ok) {
                    if (fc) fc[(long long)oy * W + ox] = bad ? __longlong_as_double(0x7ff8000000000000ll) : b;
                    if (!bad && ss_finite(av) && ss_finite(pv)) {
                        const double db = b - av, ab = fabs(db);
                        cnt += 1;
                        s1 += ab;
                        s2 += db * db;
                        if (has_p) {
                            const double dp = pv - av, ap = fabs(dp);
                            s3 += ap;
                            s4 += dp * dp;
                            won += ap < ab ? 1 : 0;
                        }
                    }
                }
            }
        }
    }
    const double t0 = ss_wave_sum((double)cnt), t1 = ss_wave_sum(s1), t2 = ss_wave_sum(s2), t3 = ss_wave_sum(s3),
                 t4 = ss_wave_sum(s4), t5 = ss_wave_sum((double)won);
    if (lane == 0) {
        double* o = a.part + BL_SUMS * item;
        o[0] = t0, o[1] = t1, o[2] = t2, o[3] = t3, o[4] = t4, o[5] = t5;
    }
}

// sums[c][0..5]: the partials of the case added in item order (band, then strip); one lane per (case, k)
__global__ void __launch_bounds__(256) k_baseline_fold(const double* __restrict__ part, long long n_case, int per_case,
                                                       double* __restrict__ sums) {
    const long long total = n_case * BL_SUMS;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long c = i / BL_SUMS;
        const int k = (int)(i - c * BL_SUMS);
        const double* p = part + BL_SUMS * (c * per_case) + k;
        double v = 0.0;
        for (int q = 0; q < per_case; q++) v += p[BL_SUMS * (long long)q];
        sums[i] = v;
    }
}

}  // namespace cae
