// kernels_quantile.h - exact order statistics of the absolute residual for split-conformal prediction intervals
// (include/cae_hip.h, cae_score_quantiles, cae_score_counts and cae_interval_bounds).
//
// The score e = |p - a| (or |p - a| / s) is never negative and never NaN, so its bits order as an unsigned integer: the
// k-th smallest score is found by a radix select on the key, most significant digit first, and everything after the score
// is formed is integer work.  Nothing is sorted, nothing is interpolated, the result is an element of the group.
//
// k_quantile_pixel: one group per pixel.  A workgroup of QT_WAVES waves owns a tile of 64 consecutive pixels for the whole
//   call, lane l of every wave pixel tile * 64 + l; the waves split the cases in runs of QT_AHEAD.  A pass counts digit
//   (key >> shift) & 31 of the keys that share the level's prefix into table[level][digit][lane] in LDS (ds_add_u32; the
//   bank is the lane, so no add waits for another), then every lane walks its 32 counters, finds the digit that holds rank
//   k, and narrows prefix and k.  Pass 0 (shift 60) is shared by the levels and gives n and the ranks; passes 1 .. 12
//   (shift 55 .. 0) follow each level's own prefix.  13 passes over the operands, QT_MAX_LEVELS * 8 KiB of LDS at most.
// k_quantile_pool_count / k_quantile_pool_scan: one group of all scores.  A pass (8-bit digits, shift 56 .. 0) counts into
//   a workgroup's LDS table with integer adds - lanes of a wave that agree on the digit are counted by one add - and merges
//   it into the 64-bit table of the call with integer atomics; the scan, a launch of its own, picks each level's digit.
// k_score_counts_pixel / k_score_counts_pool: the inner comparison on its own, the valid scores <= q per level and group.
// k_interval_bounds: p -+ q * s, the product and the sum rounded separately.
// Integer atomics only, no scratch; the same arguments give the same bits.
#pragma once
#include "kernels_importance.h"     // im_wave_sum_lane63

namespace cae {

constexpr int QT_MAX_LEVELS = 8;
constexpr int QT_DIG = 5;               // pixel mode: bits per digit
constexpr int QT_BINS = 1 << QT_DIG;
constexpr int QT_PASSES = 13;           // shifts 60, 55, .. 0: 65 bits, the top digit is at most 7
constexpr int QT_WAVES = 8;             // waves per workgroup, which share one tile's tables
constexpr int QT_AHEAD = 4;             // cases whose loads are in flight per lane
constexpr int QT_POOL_BINS = 256;       // pooled mode: 8-bit digits, 8 passes
constexpr int QT_POOL_PASSES = 8;
constexpr int QT_POOL_STATE = 32;       // 64-bit words ahead of the tables: prefix[8], k[8], n, unused
constexpr unsigned long long QT_INF = 0x7ff0000000000000ull;
constexpr unsigned long long QT_NONE = ~0ull;       // the prefix of a level whose rank is beyond n: no key has it

struct QtArgs {
    const unsigned char* p;
    const unsigned char* a;
    const unsigned char* s;                 // WS == 0: not read
    long long p_stride, a_stride, s_stride; // elements from one case to the next
    int p_be, a_be, s_be;                   // the operand is stored big-endian
    int n_level, pass;
    long long n_case, plane, n_tile, total; // total = n_case * plane (pooled)
    long long num[QT_MAX_LEVELS], den[QT_MAX_LEVELS];
    const double* q_in;                     // counts: [n_level][G]
    double* q;                              // [n_level][G]
    long long* n;                           // [G]
    unsigned long long* count;              // counts: [n_level][G]
    unsigned long long* pool;               // pooled: QT_POOL_STATE words, then [QT_MAX_LEVELS][QT_POOL_BINS]
};

template <int W> struct QtRaw { typedef unsigned long long type; };
template <> struct QtRaw<4> { typedef unsigned type; };
template <> struct QtRaw<0> { typedef unsigned type; };

template <int W>
__device__ __forceinline__ typename QtRaw<W>::type qt_load(const unsigned char* c, long long e) {
    if constexpr (W == 0) return 0u;
    else return reinterpret_cast<const typename QtRaw<W>::type*>(c)[e];
}

template <int W>
__device__ __forceinline__ double qt_value(typename QtRaw<W>::type raw, int be) {
    if constexpr (W == 4) return (double)__uint_as_float(be ? __builtin_bswap32(raw) : raw);
    else if constexpr (W == 8) return __longlong_as_double((long long)(be ? __builtin_bswap64(raw) : raw));
    else return 1.0;
}

__device__ __forceinline__ bool qt_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// the score of one pixel of one case; false: the pixel is no pair and e means nothing
template <int WP, int WA, int WS>
__device__ __forceinline__ bool qt_score(const QtArgs& g, typename QtRaw<WP>::type rp, typename QtRaw<WA>::type ra,
                                         typename QtRaw<WS>::type rs, double& e) {
#pragma clang fp contract(off)
    const double p = qt_value<WP>(rp, g.p_be), a = qt_value<WA>(ra, g.a_be);
    bool ok = qt_finite(p) && qt_finite(a);
    e = fabs(__dsub_rn(p, a));
    if constexpr (WS != 0) {
        const double s = qt_value<WS>(rs, g.s_be);
        ok = ok && qt_finite(s) && s > 0.0;
        e = __ddiv_rn(e, s);
    }
    return ok;
}

// the raw words of QT_AHEAD consecutive cases of one pixel.  Every address is formed from a clamped case, so all of them
// are valid and the loads need no predicate.
template <int WP, int WA, int WS>
struct QtBatch {
    typename QtRaw<WP>::type rp[QT_AHEAD];
    typename QtRaw<WA>::type ra[QT_AHEAD];
    typename QtRaw<WS>::type rs[QT_AHEAD];
};

template <int WP, int WA, int WS>
__device__ __forceinline__ void qt_load_cases(const QtArgs& g, long long c0, long long pl, QtBatch<WP, WA, WS>& b) {
#pragma unroll
    for (int u = 0; u < QT_AHEAD; u++) {
        const long long cc = c0 + u < g.n_case ? c0 + u : g.n_case - 1;
        b.rp[u] = qt_load<WP>(g.p + cc * g.p_stride * WP, pl);
        b.ra[u] = qt_load<WA>(g.a + cc * g.a_stride * WA, pl);
        b.rs[u] = qt_load<WS>(g.s + cc * g.s_stride * WS, pl);
    }
}

__device__ __forceinline__ void qt_lds_add(unsigned* at, unsigned v) {
    __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the split-conformal rank ceil((n + 1) num / den); n < 2^40 and den <= 10^6, so the product stays below 2^63
__device__ __forceinline__ long long qt_rank(long long n, long long num, long long den) { return ((n + 1) * num + den - 1) / den; }

// ---- pixel mode -----------------------------------------------------------------------------------------------------

template <int WP, int WA, int WS>
__global__ void __launch_bounds__(64 * QT_WAVES) k_quantile_pixel(const QtArgs g) {
    extern __shared__ unsigned qt_table[];          // [level][QT_BINS][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = g.n_level;
    for (long long tile = blockIdx.x; tile < g.n_tile; tile += gridDim.x) {
        const long long px = tile * 64 + lane;
        const bool inside = px < g.plane;
        const long long pl = inside ? px : g.plane - 1;
        unsigned long long prefix[QT_MAX_LEVELS];
        unsigned k[QT_MAX_LEVELS];
        unsigned n = 0;
#pragma unroll
        for (int l = 0; l < QT_MAX_LEVELS; l++) prefix[l] = 0ull, k[l] = 0u;
        for (int pass = 0; pass < QT_PASSES; pass++) {
            const int shift = 60 - QT_DIG * pass;
            const int tables = pass == 0 ? 1 : L;
            for (int i = threadIdx.x; i < tables * QT_BINS * 64; i += 64 * QT_WAVES) qt_table[i] = 0u;
            __syncthreads();
#pragma unroll 1
            for (long long c0 = (long long)wave * QT_AHEAD; c0 < g.n_case; c0 += QT_WAVES * QT_AHEAD) {
                QtBatch<WP, WA, WS> b;
                qt_load_cases<WP, WA, WS>(g, c0, pl, b);
#pragma unroll
                for (int u = 0; u < QT_AHEAD; u++) {
                    double e;
                    const bool ok = qt_score<WP, WA, WS>(g, b.rp[u], b.ra[u], b.rs[u], e) && inside && c0 + u < g.n_case;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(e);
                    const unsigned digit = (unsigned)(key >> shift) & (QT_BINS - 1);
                    if (pass == 0) {
                        if (ok) qt_lds_add(&qt_table[digit * 64 + lane], 1u);
                    } else {
                        const unsigned long long head = key >> (shift + QT_DIG);
#pragma unroll
                        for (int l = 0; l < QT_MAX_LEVELS; l++)
                            if (l < L && ok && head == prefix[l]) qt_lds_add(&qt_table[(l * QT_BINS + digit) * 64 + lane], 1u);
                    }
                }
            }
            __syncthreads();
            // every wave narrows for itself: the same counters, the same result in each
            if (pass == 0) {
                unsigned total = 0;
                for (int d = 0; d < QT_BINS; d++) total += qt_table[d * 64 + lane];
                n = total;
#pragma unroll
                for (int l = 0; l < QT_MAX_LEVELS; l++) {
                    if (l < L) {
                        const long long r = qt_rank((long long)n, g.num[l], g.den[l]);
                        if (r > (long long)n) prefix[l] = QT_NONE;
                        else k[l] = (unsigned)r;
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < QT_MAX_LEVELS; l++) {
                if (l < L && prefix[l] != QT_NONE) {
                    const unsigned* t = qt_table + (pass == 0 ? 0 : l) * QT_BINS * 64 + lane;
                    unsigned below = 0, digit = 0, before = 0;
                    bool found = false;
                    for (int d = 0; d < QT_BINS; d++) {
                        const unsigned c = t[d * 64];
                        if (!found && below + c >= k[l]) found = true, digit = (unsigned)d, before = below;
                        below += c;
                    }
                    k[l] -= before;
                    prefix[l] = (prefix[l] << QT_DIG) | digit;
                }
            }
            __syncthreads();
        }
        if (wave == 0 && inside) {
#pragma unroll
            for (int l = 0; l < QT_MAX_LEVELS; l++)
                if (l < L) g.q[l * g.plane + px] = __longlong_as_double((long long)(prefix[l] == QT_NONE ? QT_INF : prefix[l]));
            g.n[px] = (long long)n;
        }
    }
}

template <int WP, int WA, int WS>
__global__ void __launch_bounds__(64 * QT_WAVES) k_score_counts_pixel(const QtArgs g) {
    __shared__ unsigned sums[(QT_MAX_LEVELS + 1) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = g.n_level;
    for (long long tile = blockIdx.x; tile < g.n_tile; tile += gridDim.x) {
        const long long px = tile * 64 + lane;
        const bool inside = px < g.plane;
        const long long pl = inside ? px : g.plane - 1;
        double q[QT_MAX_LEVELS];
        unsigned cnt[QT_MAX_LEVELS];
        unsigned n = 0;
#pragma unroll
        for (int l = 0; l < QT_MAX_LEVELS; l++) {
            q[l] = l < L ? g.q_in[l * g.plane + pl] : 0.0;
            cnt[l] = 0u;
        }
        for (int i = threadIdx.x; i < (QT_MAX_LEVELS + 1) * 64; i += 64 * QT_WAVES) sums[i] = 0u;
        __syncthreads();
#pragma unroll 1
        for (long long c0 = (long long)wave * QT_AHEAD; c0 < g.n_case; c0 += QT_WAVES * QT_AHEAD) {
            QtBatch<WP, WA, WS> b;
            qt_load_cases<WP, WA, WS>(g, c0, pl, b);
#pragma unroll
            for (int u = 0; u < QT_AHEAD; u++) {
                double e;
                const bool ok = qt_score<WP, WA, WS>(g, b.rp[u], b.ra[u], b.rs[u], e) && inside && c0 + u < g.n_case;
                n += ok ? 1u : 0u;
#pragma unroll
                for (int l = 0; l < QT_MAX_LEVELS; l++) cnt[l] += (l < L && ok && e <= q[l]) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int l = 0; l < QT_MAX_LEVELS; l++)
            if (l < L) qt_lds_add(&sums[l * 64 + lane], cnt[l]);
        qt_lds_add(&sums[QT_MAX_LEVELS * 64 + lane], n);
        __syncthreads();
        if (wave == 0 && inside) {
#pragma unroll
            for (int l = 0; l < QT_MAX_LEVELS; l++)
                if (l < L) g.count[l * g.plane + px] = sums[l * 64 + lane];
            g.n[px] = (long long)sums[QT_MAX_LEVELS * 64 + lane];
        }
        __syncthreads();
    }
}

// ---- pooled mode ----------------------------------------------------------------------------------------------------

// the raw words of score `idx` of the call (case idx / plane, pixel idx % plane); idx is a score that exists
template <int WP, int WA, int WS>
__device__ __forceinline__ void qt_load_flat(const QtArgs& g, long long idx, typename QtRaw<WP>::type& rp,
                                             typename QtRaw<WA>::type& ra, typename QtRaw<WS>::type& rs) {
    long long c, e;
    if (g.total <= 0xffffffffll) {      // the common call: one 32-bit division
        const unsigned cu = (unsigned)idx / (unsigned)g.plane;
        c = cu, e = (long long)((unsigned)idx - cu * (unsigned)g.plane);
    } else {
        c = idx / g.plane, e = idx - c * g.plane;
    }
    rp = qt_load<WP>(g.p + c * g.p_stride * WP, e);
    ra = qt_load<WA>(g.a + c * g.a_stride * WA, e);
    rs = qt_load<WS>(g.s + c * g.s_stride * WS, e);
}

// One add to table[digit] for every lane with `m`.  The lanes that agree with the first such lane on the digit are counted
// by that lane alone, twice over; what is left adds for itself.  A constant field, or the exponent digits of any field,
// would otherwise queue 64 adds on one counter.
__device__ __forceinline__ void qt_pool_add(unsigned* table, bool m, unsigned digit, int lane) {
#pragma unroll
    for (int round = 0; round < 2; round++) {
        const unsigned long long mask = __ballot(m);
        if (mask == 0ull) return;
        const int src = __ffsll((long long)mask) - 1;
        const unsigned ref = (unsigned)__shfl((int)digit, src, 64);
        const unsigned long long same = __ballot(m && digit == ref);
        if (lane == src) qt_lds_add(&table[ref], (unsigned)__popcll(same));
        m = m && digit != ref;
    }
    if (m) qt_lds_add(&table[digit], 1u);
}

template <int WP, int WA, int WS>
__global__ void __launch_bounds__(256) k_quantile_pool_count(const QtArgs g) {
    __shared__ unsigned table[QT_MAX_LEVELS * QT_POOL_BINS];
    const int lane = threadIdx.x & 63;
    const int L = g.n_level, pass = g.pass;
    const int tables = pass == 0 ? 1 : L;
    const int shift = 56 - 8 * pass;
    for (int i = threadIdx.x; i < tables * QT_POOL_BINS; i += 256) table[i] = 0u;
    unsigned long long prefix[QT_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < QT_MAX_LEVELS; l++) prefix[l] = (pass > 0 && l < L) ? g.pool[l] : QT_NONE;
    __syncthreads();
    const long long chunks = (g.total + 63) >> 6;
    const long long waves = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long j0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j0 < chunks; j0 += waves * QT_AHEAD) {
        typename QtRaw<WP>::type rp[QT_AHEAD];
        typename QtRaw<WA>::type ra[QT_AHEAD];
        typename QtRaw<WS>::type rs[QT_AHEAD];
        bool in[QT_AHEAD];
#pragma unroll
        for (int u = 0; u < QT_AHEAD; u++) {
            const long long idx = ((j0 + u * waves) << 6) + lane;
            in[u] = idx < g.total;
            qt_load_flat<WP, WA, WS>(g, in[u] ? idx : g.total - 1, rp[u], ra[u], rs[u]);
        }
#pragma unroll
        for (int u = 0; u < QT_AHEAD; u++) {
            double e;
            const bool ok = qt_score<WP, WA, WS>(g, rp[u], ra[u], rs[u], e) && in[u];
            const unsigned long long key = (unsigned long long)__double_as_longlong(e);
            const unsigned digit = (unsigned)(key >> shift) & (QT_POOL_BINS - 1);
            if (pass == 0) {
                qt_pool_add(table, ok, digit, lane);
            } else {
                const unsigned long long head = key >> (shift + 8);
#pragma unroll
                for (int l = 0; l < QT_MAX_LEVELS; l++)
                    if (l < L) qt_pool_add(table + l * QT_POOL_BINS, ok && head == prefix[l], digit, lane);
            }
        }
    }
    __syncthreads();
    unsigned long long* hist = g.pool + QT_POOL_STATE;
    for (int i = threadIdx.x; i < tables * QT_POOL_BINS; i += 256) {
        const unsigned c = table[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
}

// one workgroup: thread l narrows level l from the merged table of the pass, which is then cleared for the next
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_quantile_pool_scan(const QtArgs g) {
    __shared__ unsigned long long table[QT_MAX_LEVELS * QT_POOL_BINS];
    const int L = g.n_level, pass = g.pass;
    const int tables = pass == 0 ? 1 : L;
    unsigned long long* hist = g.pool + QT_POOL_STATE;
    for (int i = threadIdx.x; i < tables * QT_POOL_BINS; i += BLOCK) {
        table[i] = hist[i];
        hist[i] = 0ull;
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (l >= L) return;
    unsigned long long prefix = 0ull;
    long long k;
    if (pass == 0) {
        long long n = 0;
        for (int d = 0; d < QT_POOL_BINS; d++) n += (long long)table[d];
        if (l == 0) g.n[0] = n;
        k = qt_rank(n, g.num[l], g.den[l]);
        if (k > n) prefix = QT_NONE;
    } else {
        prefix = g.pool[l];
        k = (long long)g.pool[QT_MAX_LEVELS + l];
    }
    if (prefix != QT_NONE) {
        const unsigned long long* t = table + (pass == 0 ? 0 : l) * QT_POOL_BINS;
        long long below = 0, before = 0;
        unsigned digit = 0;
        bool found = false;
        for (int d = 0; d < QT_POOL_BINS; d++) {
            const long long c = (long long)t[d];
            if (!found && below + c >= k) found = true, digit = (unsigned)d, before = below;
            below += c;
        }
        k -= before;
        prefix = (prefix << 8) | digit;
    }
    g.pool[l] = prefix;
    g.pool[QT_MAX_LEVELS + l] = (unsigned long long)k;
    if (pass == QT_POOL_PASSES - 1) g.q[l] = __longlong_as_double((long long)(prefix == QT_NONE ? QT_INF : prefix));
}

template <int WP, int WA, int WS>
__global__ void __launch_bounds__(256) k_score_counts_pool(const QtArgs g) {
    __shared__ unsigned sums[QT_MAX_LEVELS + 1];
    const int lane = threadIdx.x & 63;
    const int L = g.n_level;
    if (threadIdx.x <= QT_MAX_LEVELS) sums[threadIdx.x] = 0u;
    double q[QT_MAX_LEVELS];
    unsigned cnt[QT_MAX_LEVELS];
    unsigned n = 0;
#pragma unroll
    for (int l = 0; l < QT_MAX_LEVELS; l++) {
        q[l] = l < L ? g.q_in[l] : 0.0;
        cnt[l] = 0u;
    }
    __syncthreads();
    const long long chunks = (g.total + 63) >> 6;
    const long long waves = (long long)gridDim.x * 4;
#pragma unroll 1
    for (long long j0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j0 < chunks; j0 += waves * QT_AHEAD) {
        typename QtRaw<WP>::type rp[QT_AHEAD];
        typename QtRaw<WA>::type ra[QT_AHEAD];
        typename QtRaw<WS>::type rs[QT_AHEAD];
        bool in[QT_AHEAD];
#pragma unroll
        for (int u = 0; u < QT_AHEAD; u++) {
            const long long idx = ((j0 + u * waves) << 6) + lane;
            in[u] = idx < g.total;
            qt_load_flat<WP, WA, WS>(g, in[u] ? idx : g.total - 1, rp[u], ra[u], rs[u]);
        }
#pragma unroll
        for (int u = 0; u < QT_AHEAD; u++) {
            double e;
            const bool ok = qt_score<WP, WA, WS>(g, rp[u], ra[u], rs[u], e) && in[u];
            n += ok ? 1u : 0u;
#pragma unroll
            for (int l = 0; l < QT_MAX_LEVELS; l++) cnt[l] += (l < L && ok && e <= q[l]) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int l = 0; l < QT_MAX_LEVELS; l++) {
        const unsigned w = (unsigned)im_wave_sum_lane63((int)cnt[l]);
        if (l < L && lane == 63) qt_lds_add(&sums[l], w);
    }
    {
        const unsigned w = (unsigned)im_wave_sum_lane63((int)n);
        if (lane == 63) qt_lds_add(&sums[QT_MAX_LEVELS], w);
    }
    __syncthreads();
    if ((int)threadIdx.x < L && sums[threadIdx.x]) atomicAdd(&g.count[threadIdx.x], (unsigned long long)sums[threadIdx.x]);
    if (threadIdx.x == QT_MAX_LEVELS && sums[QT_MAX_LEVELS])
        atomicAdd(reinterpret_cast<unsigned long long*>(g.n), (unsigned long long)sums[QT_MAX_LEVELS]);
}

// ---- the outputs of an empty call, and the bounds ---------------------------------------------------------------------

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_quantile_fill(double* __restrict__ q, long long count, double v) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < count; i += (long long)gridDim.x * BLOCK) q[i] = v;
}

struct QbArgs {
    const unsigned char* p;
    const unsigned char* s;
    long long p_stride, s_stride, n_case, plane, total;
    int p_be, s_be, pooled;
    const double* q;
    double* lower;
    double* upper;
};

template <int WP, int WS>
__global__ void __launch_bounds__(256) k_interval_bounds(const QbArgs g) {
#pragma clang fp contract(off)
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < g.total; idx += (long long)gridDim.x * 256) {
        long long c, e;
        if (g.total <= 0xffffffffll) {
            const unsigned cu = (unsigned)idx / (unsigned)g.plane;
            c = cu, e = (long long)((unsigned)idx - cu * (unsigned)g.plane);
        } else {
            c = idx / g.plane, e = idx - c * g.plane;
        }
        const double p = qt_value<WP>(qt_load<WP>(g.p + c * g.p_stride * WP, e), g.p_be);
        double half = g.q[g.pooled ? 0 : e];
        bool ok = qt_finite(p);
        if constexpr (WS != 0) {
            const double s = qt_value<WS>(qt_load<WS>(g.s + c * g.s_stride * WS, e), g.s_be);
            ok = ok && qt_finite(s) && s > 0.0;
            half = half * s;        // plain operators: the pragma above governs them, not the bodies of __dmul_rn and its kin
        }
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        g.lower[idx] = ok ? p - half : nan;
        g.upper[idx] = ok ? p + half : nan;
    }
}

}  // namespace cae
