// kernels_stateless.h — the kernels behind the stateless entry points of include/cae_hip.h (stateless_host.h): the loader
// (scan, normalise + pack, permutation inverse, denormalise, metric sums, byte swap), the evaluator's per-case measures, the
// ensemble moments, the ensemble verification, the case pages and the per-pixel skill sums.  None of them touches an engine.
#pragma once
#include "case_elem.h"
#include "device_common.h"

namespace cae {

// ---------------------------------------------------------------------------------------------
// loader kernels (ds_dataset.py)
// ---------------------------------------------------------------------------------------------

// per-block partial {nan count, min, max}; out [gridDim.x][3] doubles
__global__ void __launch_bounds__(256) k_scan(const float* __restrict__ x, long long n, double* __restrict__ out) {
    __shared__ double red[3][4];
    double cnt = 0;
    float lo = INFINITY, hi = -INFINITY;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        if (v != v) {
            cnt += 1;
        } else {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wv] = cnt;
        red[1][wv] = lo;
        red[2][wv] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0, l = INFINITY, h = -INFINITY;
        for (int i = 0; i < 4; i++) {
            c += red[0][i];
            l = fmin(l, red[1][i]);
            h = fmax(h, red[2][i]);
        }
        out[3 * blockIdx.x + 0] = c;
        out[3 * blockIdx.x + 1] = l;
        out[3 * blockIdx.x + 2] = h;
    }
}

// dst[row(i)][c_off + c][:] = (src[i][c][:] - vmin) / range   (two correctly rounded fp32 ops, as numpy)
// row(i) = dst_row[i] when a table is given (the frozen shuffle's inverse: normalisation writes the samples in batch order
// in the pass it makes anyway - the reference's DataLoader + collate stacking, conv_ae_model.py:291-292,315-325), else i.
__global__ void __launch_bounds__(256) k_normalise_pack(const float* __restrict__ src, long long total, int c_src,
                                                         long long hw, float* __restrict__ dst, int c_dst, int c_off,
                                                         float vmin, float range, int enable,
                                                         const int* __restrict__ dst_row) {
    const long long per = (long long)c_src * hw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long s = i / per, r = i - s * per;
        float v = src[i];
        if (enable) v = (range == 0.f) ? 0.f : __fdiv_rn(__fsub_rn(v, vmin), range);
        const long long d = dst_row ? (long long)dst_row[s] : s;
        dst[(d * c_dst + c_off) * hw + r] = v;
    }
}

// inv[perm[i]] = i: the destination-row table of k_normalise_pack from a frozen sample order
__global__ void __launch_bounds__(256) k_invert_perm(const int* __restrict__ perm, long long n, int* __restrict__ inv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int p = perm[i];
        if (p >= 0 && p < n) inv[p] = (int)i;
    }
}

__global__ void __launch_bounds__(256) k_denorm_f64(const float* __restrict__ y, long long n, double vmin, double range,
                                                     double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = cm_denorm(vmin, (double)y[i], range);
}

// model_metric.py:47-71 per instance: sums[inst][8] += {n, Σa', Σe', Σa'², Σe'², Σa'e', Σ|a-e|, Σ(a-e)²} over the
// pixels whose mask is non-zero, with e = vmin + (double)y*range (the denormalised score of base_model.py:90) and
// a' = a - vmin, e' = e - vmin (shifted so the second moments do not cancel).  grid (chunks, n_inst), block 256.
__global__ void __launch_bounds__(256) k_metric_sums(const float* __restrict__ y, const float* __restrict__ a,
                                                      const float* __restrict__ mask, long long elems, double vmin,
                                                      double range, double* __restrict__ sums) {
    __shared__ double red[4];
    const long long base = (long long)blockIdx.y * elems;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < elems; i += (long long)gridDim.x * 256) {
        if (mask && mask[base + i] == 0.f) continue;
        const double e = cm_denorm(vmin, (double)y[base + i], range);
        const double av = (double)a[base + i];
        const double d = av - e, as = av - vmin, es = e - vmin;
        acc[0] += 1.0;
        acc[1] += as;
        acc[2] += es;
        acc[3] += as * as;
        acc[4] += es * es;
        acc[5] += as * es;
        acc[6] += fabs(d);
        acc[7] += d * d;
    }
    for (int k = 0; k < 8; k++) {
        const double t = block_sum(acc[k], red);
        if (threadIdx.x == 0 && t != 0.0) atomicAdd(&sums[(size_t)blockIdx.y * 8 + k], t);
    }
}

// NetCDF-3 stores big-endian words: swap n 32-bit words in place (16 bytes per lane per trip)
__global__ void __launch_bounds__(256) k_bswap32(unsigned* __restrict__ x, long long n) {
    const long long n4 = n >> 2;
    uint4* x4 = reinterpret_cast<uint4*>(x);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        uint4 v = x4[i];
        v.x = __builtin_bswap32(v.x);
        v.y = __builtin_bswap32(v.y);
        v.z = __builtin_bswap32(v.z);
        v.w = __builtin_bswap32(v.w);
        x4[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) x[(n4 << 2) + threadIdx.x] = __builtin_bswap32(x[(n4 << 2) + threadIdx.x]);
}

// ---- per-case error sums (model_evaluator.py:87-95): S|p - a| and S(p - a)^2 in fp64 over a case's first `plane` elements,
// read with the element loads of case_elem.h.
__device__ __forceinline__ void cm_acc(double p, double a, double& s1, double& s2) {
    const double d = p - a;     // fp64: numpy's promotion of the float64 prediction against the target
    s1 += fabs(d);
    s2 += d * d;
}

// One wave per (case, chunk) item.  A case is cut at its first element h where both p and a are 16 bytes aligned: the
// head [0, h) and the tail after the last whole 4-element group are summed element by element by the lanes of chunk 0;
// the groups in between are split into chunks of CM_GROUPS groups, one lane taking every 64th group in order.  A lane's
// sums, the fixed shuffle tree over the wave and the chunk-ordered fold (k_case_fold) depend on the launch shape and the
// case's alignment only, so the result is the same bits from run to run.  No atomics: each item's two sums are plain
// stores into out[item] - the partials (nch > 1) or the case's result (nch == 1).  NaN and Inf pass through untouched.
constexpr int CM_GROUPS = 1024;          // 4096 elements per chunk
constexpr int CM_WAVES = 4;              // waves per 256-thread workgroup

template <int KP, int KA>
__global__ void __launch_bounds__(256) k_case_measures(const unsigned char* __restrict__ p, long long p_stride,
                                                       const unsigned char* __restrict__ a, long long a_stride,
                                                       long long plane, int nch, long long items,
                                                       double* __restrict__ out) {
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    const int lane = threadIdx.x & 63;
    for (long long item = (long long)blockIdx.x * CM_WAVES + (threadIdx.x >> 6); item < items;
         item += (long long)gridDim.x * CM_WAVES) {
        const long long cs = item / nch;
        const int ch = (int)(item - cs * nch);
        const unsigned char* pc = p + cs * p_stride * EP;
        const unsigned char* ac = a + cs * a_stride * EA;
        int h = -1;
        for (int t = 3; t >= 0; t--)
            if ((((uintptr_t)(pc + t * EP) | (uintptr_t)(ac + t * EA)) & 15) == 0) h = t;
        const bool vec = h >= 0;
        const long long head = vec ? (h < plane ? h : plane) : 0;
        const long long groups = (plane - head) >> 2;
        const long long tail0 = head + (groups << 2);
        double s1 = 0.0, s2 = 0.0;
        if (ch == 0) {
            if (lane < head) cm_acc(cm_load1<KP>(pc, lane), cm_load1<KA>(ac, lane), s1, s2);
            else if (lane >= 4 && lane - 4 < plane - tail0)
                cm_acc(cm_load1<KP>(pc, tail0 + lane - 4), cm_load1<KA>(ac, tail0 + lane - 4), s1, s2);
        }
        const long long g0 = (long long)ch * CM_GROUPS;
        const long long g1 = g0 + CM_GROUPS < groups ? g0 + CM_GROUPS : groups;
        long long g = g0 + lane;
        for (; g + 3 * 64 < g1; g += 4 * 64) {      // four groups in flight per lane, summed in group order
            double vp[4][4], va[4][4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                cm_load4<KP>(pc, head + ((g + u * 64) << 2), vec, vp[u]);
                cm_load4<KA>(ac, head + ((g + u * 64) << 2), vec, va[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) cm_acc(vp[u][j], va[u][j], s1, s2);
        }
        for (; g < g1; g += 64) {
            double vp[4], va[4];
            cm_load4<KP>(pc, head + (g << 2), vec, vp);
            cm_load4<KA>(ac, head + (g << 2), vec, va);
#pragma unroll
            for (int j = 0; j < 4; j++) cm_acc(vp[j], va[j], s1, s2);
        }
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_down(s1, off, 64);
            s2 += __shfl_down(s2, off, 64);
        }
        if (lane == 0) {
            out[2 * item] = s1;
            out[2 * item + 1] = s2;
        }
    }
}

// out[i] = sum over chunks k = 0 .. nch-1, in that order, of part[i * nch + k]
__global__ void __launch_bounds__(256) k_case_fold(const double* __restrict__ part, long long n_case, int nch,
                                                   double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_case; i += (long long)gridDim.x * 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nch; k++) {
            s1 += part[2 * (i * nch + k)];
            s2 += part[2 * (i * nch + k) + 1];
        }
        out[2 * i] = s1;
        out[2 * i + 1] = s2;
    }
}

// ---- ensemble moments (VarAEModel.apply(ensemble_size=K), include/cae_hip.h): per pixel the mean and the sample standard
// deviation of K fp32 draws, denormalised, in fp64.  Nothing crosses a lane: a pixel's draws are summed by one lane in draw
// order (d_k = y_k - y_0, s1 = S d_k, s2 = S d_k^2), so there is no fold, no atomic and no order to fix beyond that one.
// Items and loads are k_case_measures': one wave per (case, chunk of `chunk` 4-pixel groups), a lane takes every 64th group
// and reads it from each draw with one 16-byte load (four draws in flight), the head before the case's first 16-byte phase
// and the tail after its last whole group go element by element to the lanes of chunk 0.  With nothing to fold the chunk
// length is the host's to choose (64 .. CM_GROUPS groups): short chunks when a call brings few cases, so that the waves
// still cover the device.  The draws of a case share that phase
// when draw_stride is a multiple of 4 (or one draw arrives); otherwise every load is scalar.
// FIRST: this call brings draw 0 (y_0 is read from it); otherwise {y_0, s1, s2} come from the workspace planes w0, w1, w2.
// LAST: this call brings draw K-1 and writes mean / sd (16-byte stores where the case's plane starts on one); otherwise the
// three values go back to the workspace.  <true, true> touches no workspace: K * 4 bytes read and 16 written per pixel.
template <int N>
__device__ __forceinline__ void em_load(const float* c, long long e, bool vec, float v[N]) {
    if constexpr (N == 4) {
        if (vec) {
            const float4 w = *reinterpret_cast<const float4*>(c + e);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = c[e + j];
}

template <int N>
__device__ __forceinline__ void em_store(double* dst, long long o, bool vec2, const double v[N]) {
    if constexpr (N == 4) {
        if (vec2) {
            reinterpret_cast<double2*>(dst + o)[0] = make_double2(v[0], v[1]);
            reinterpret_cast<double2*>(dst + o)[1] = make_double2(v[2], v[3]);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) dst[o + j] = v[j];
}

struct EmArgs {
    const float* y;             // draw j of case c of this call: y + c * case_stride + j * draw_stride, `plane` floats
    long long case_stride, draw_stride, plane;
    int kc, K;                  // draws in this call, draws in all
    int nch, chunk;             // chunks per case, 4-pixel groups per chunk
    long long items;
    double vmin, range;
    double* mean;               // (n_case, plane) each; sd may be null
    double* sd;
    float* w0;                  // workspace planes (n_case, plane): y_0, s1, s2
    double* w1;
    double* w2;
};

// N pixels from element e of the case that starts at yc; o = the pixels' index in the (n_case, plane) output planes
template <bool FIRST, bool LAST, int N>
__device__ __forceinline__ void em_pixels(const EmArgs& a, const float* yc, long long e, long long o, bool vec, bool vec2) {
    double y0[N], s1[N], s2[N];
    int k = 0;
    if constexpr (FIRST) {
        float v[N];
        em_load<N>(yc, e, vec, v);
#pragma unroll
        for (int j = 0; j < N; j++) y0[j] = (double)v[j], s1[j] = 0.0, s2[j] = 0.0;    // (d_0 = 0 adds nothing)
        k = 1;
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) y0[j] = (double)a.w0[o + j], s1[j] = a.w1[o + j], s2[j] = a.w2[o + j];
    }
    for (; k + 3 < a.kc; k += 4) {      // four draws in flight per lane, summed in draw order
        float v[4][N];
#pragma unroll
        for (int u = 0; u < 4; u++) em_load<N>(yc + (k + u) * a.draw_stride, e, vec, v[u]);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int j = 0; j < N; j++) {
                const double d = (double)v[u][j] - y0[j];
                s1[j] += d;
                s2[j] += d * d;
            }
    }
    for (; k < a.kc; k++) {
        float v[N];
        em_load<N>(yc + k * a.draw_stride, e, vec, v);
#pragma unroll
        for (int j = 0; j < N; j++) {
            const double d = (double)v[j] - y0[j];
            s1[j] += d;
            s2[j] += d * d;
        }
    }
    if constexpr (LAST) {
        const double K = (double)a.K, ar = fabs(a.range);
        double m[N], s[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            m[j] = a.vmin + (y0[j] + s1[j] / K) * a.range;
            const double var = (s2[j] - s1[j] * s1[j] / K) / (K - 1.0);
            s[j] = sqrt(var < 0.0 ? 0.0 : var) * ar;      // (a NaN stays a NaN)
        }
        em_store<N>(a.mean, o, vec2, m);
        if (a.sd) em_store<N>(a.sd, o, vec2, s);
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) a.w0[o + j] = (float)y0[j], a.w1[o + j] = s1[j], a.w2[o + j] = s2[j];
    }
}

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) k_ensemble_moments(const EmArgs a) {
    const int lane = threadIdx.x & 63;
    const bool same_phase = (a.draw_stride & 3) == 0 || a.kc == 1;
    for (long long item = (long long)blockIdx.x * CM_WAVES + (threadIdx.x >> 6); item < a.items;
         item += (long long)gridDim.x * CM_WAVES) {
        const long long cs = item / a.nch;
        const int ch = (int)(item - cs * a.nch);
        const float* yc = a.y + cs * a.case_stride;
        const long long o0 = cs * a.plane;
        int h = 0;
        if (same_phase)
            for (int t = 3; t >= 0; t--)
                if (((uintptr_t)(yc + t) & 15) == 0) h = t;
        const long long head = h < a.plane ? h : a.plane;
        const long long groups = (a.plane - head) >> 2;
        const long long tail0 = head + (groups << 2);
        // 16-byte stores: the first group of the case lands on a 16-byte boundary of both output planes
        const bool vec2 = (((uintptr_t)(a.mean + o0 + head) | (a.sd ? (uintptr_t)(a.sd + o0 + head) : 0)) & 15) == 0;
        if (ch == 0) {
            if (lane < head) em_pixels<FIRST, LAST, 1>(a, yc, lane, o0 + lane, false, false);
            else if (lane >= 4 && lane - 4 < a.plane - tail0)
                em_pixels<FIRST, LAST, 1>(a, yc, tail0 + lane - 4, o0 + tail0 + lane - 4, false, false);
        }
        const long long g0 = (long long)ch * a.chunk;
        const long long g1 = g0 + a.chunk < groups ? g0 + a.chunk : groups;
        for (long long g = g0 + lane; g < g1; g += 64)
            em_pixels<FIRST, LAST, 4>(a, yc, head + (g << 2), o0 + head + (g << 2), same_phase, vec2);
    }
}

// ---- ensemble verification (include/cae_hip.h, cae_ensemble_verify): the K draws of a pixel against its target.  Per counted
// pixel (the target and all K draws finite) A = S_k |m_k - a| / K, B = S_{i<j} |m_i - m_j| / K^2, (mbar - a)^2 and s^2 with
// m_k = vmin + (double)y_k * range (two roundings), mbar and s^2 formed as k_ensemble_moments forms them; per case the five
// sums {n, S A, S B, S (mbar - a)^2, S s^2}; per call the histogram of below = #{k: m_k < a} and the number of ties.
// One wave (a workgroup of its own) per (case, chunk of `chunk` 4-pixel groups) item, items and loads as
// k_ensemble_moments' (the host picks the chunk, 64 .. CM_GROUPS groups, from the size of the call alone, so that a call
// with few cases still covers the device): the wave walks the chunk in blocks of EV_PIX = 256 pixels.  A lane loads its 4-pixel group of every
// draw (one 16-byte load per draw where the draws share a phase, else four element loads a wave reads along a line) into
// the [K][EV_PIX] fp32 tile in LDS - the members are never a register array - and then takes the pixels lane, lane + 64,
// lane + 128, lane + 192 of the block, each alone: one walk down its column in ascending draw order, eight members at a time
// in registers (then four, then one), gathers {finite?, S|m - a|, below, tied, s1, s2} and pairs each block with itself and
// with every member j below it: all K (K - 1) / 2 pairs, no sort.  The members are converted again at every read
// (cvt, mul, add in fp64): fp64 columns would double the tile, which at K = 64 is already 64 KiB.  The head before the
// case's first 16-byte phase and the tail after its last whole group go to lanes of chunk 0, one pixel each.
// Fixed order, no atomics of any kind: a lane adds its pixels in block order, the wave's lanes meet in a fixed shuffle tree,
// item sums are plain stores (the partials, or the case's result when it has one chunk) and k_verify_fold adds a case's
// chunks in chunk order: the same bits from run to run.  The ranks are integers: per pixel row one ballot per bin, lane b
// keeps bin b of the workgroup (bin 64 and the ties sit in wave-uniform counters), plain stores of the workgroup's K + 2
// counts to the workspace, and the fold adds the workgroups' counts into rank_counts with a load, an add and a store per bin.
constexpr int EV_SUMS = 5;
constexpr int EV_PIX = 256;

struct EvArgs {
    const float* y;             // draw k of case c: y + c * case_stride + k * draw_stride, `plane` floats
    long long case_stride, draw_stride;
    const unsigned char* a;     // target of case c: element c * a_stride
    long long a_stride, plane;
    int K, nch, chunk;          // draws, chunks per case, 4-pixel groups per chunk (a multiple of 64)
    long long items;
    double vmin, range;
    double* sums;               // (items, EV_SUMS)
    long long* ranks;           // (gridDim.x, K + 2)
};

struct EvAcc {
    unsigned n;
    double sa, sb, e, v;        // S_x S_k |m_k - a|, S_x S_{i<j} |m_i - m_j|, S (mbar - a)^2, S s^2
};

// member k of the pixel whose draws are col[k * EV_PIX]
__device__ __forceinline__ double ev_member(const EvArgs& s, const float* col, int k) {
#pragma clang fp contract(off)
    const double t = (double)col[k * EV_PIX] * s.range;
    return s.vmin + t;
}

// what one walk over a pixel's members in ascending draw order gathers
struct EvWalk {
    double av, y0, s1, s2, sa;
    int below;
    bool ok, tie;
};

// member k, and its share of the walk
__device__ __forceinline__ double ev_visit(const EvArgs& s, const float* col, int k, EvWalk& w) {
#pragma clang fp contract(off)
    const float yf = col[k * EV_PIX];
    w.ok = w.ok && fabsf(yf) < __builtin_huge_valf();
    const double y = (double)yf;
    const double t = y * s.range;
    const double m = s.vmin + t;
    const double d = y - w.y0;
    w.s1 += d;
    w.s2 += d * d;
    w.sa += fabs(m - w.av);
    w.below += m < w.av ? 1 : 0;
    w.tie = w.tie || m == w.av;
    return m;
}

// R members i0 .. i0 + R - 1 in registers (visited as they are read): their pairs among themselves and with every j < i0
template <int R>
__device__ __forceinline__ void ev_block(const EvArgs& s, const float* col, int i0, EvWalk& w, double b[4]) {
    double r[R];
#pragma unroll
    for (int u = 0; u < R; u++) r[u] = ev_visit(s, col, i0 + u, w);
#pragma unroll
    for (int u = 1; u < R; u++)
#pragma unroll
        for (int v = 0; v < u; v++) b[(u + v) & 3] += fabs(r[u] - r[v]);
#pragma unroll 2
    for (int j = 0; j < i0; j++) {
        const double mj = ev_member(s, col, j);
#pragma unroll
        for (int u = 0; u < R; u++) b[u & 3] += fabs(r[u] - mj);
    }
}

// the pixel whose draws are col[k * EV_PIX] and whose target is element e of the case at ac: its sums into acc;
// returns `below`, or -1 when the pixel is not counted.  One walk in ascending draw order, in blocks of 8, 4 and 1 members
template <int KA>
__device__ __forceinline__ int ev_pixel(const EvArgs& s, const float* col, const unsigned char* ac, long long e, EvAcc& acc,
                                        bool& tied) {
#pragma clang fp contract(off)
    const int K = s.K;
    EvWalk w;
    w.av = cm_load1<KA>(ac, e);
    w.ok = fabs(w.av) < __builtin_huge_val();
    w.y0 = (double)col[0];
    w.s1 = 0.0, w.s2 = 0.0, w.sa = 0.0, w.below = 0, w.tie = false;
    double b[4] = {0.0, 0.0, 0.0, 0.0};
    int i = 0;
    for (; i + 8 <= K; i += 8) ev_block<8>(s, col, i, w, b);
    if (i + 4 <= K) {
        ev_block<4>(s, col, i, w, b);
        i += 4;
    }
    for (; i < K; i++) ev_block<1>(s, col, i, w, b);
    if (!w.ok) return -1;
    const double Kd = (double)K;
    const double mbar = s.vmin + (w.y0 + w.s1 / Kd) * s.range;
    const double var = (w.s2 - w.s1 * w.s1 / Kd) / (Kd - 1.0);
    const double dm = mbar - w.av;
    acc.n += 1u;
    acc.sa += w.sa;
    acc.sb += (b[0] + b[1]) + (b[2] + b[3]);
    acc.e += dm * dm;
    acc.v += (var < 0.0 ? 0.0 : var) * s.range * s.range;
    tied = w.tie;
    return w.below;
}

// one pixel row of the wave into the rank counters: lane b keeps bin b, c64 and ctied are wave-uniform.  Every lane of the
// wave calls it (below = -1: no counted pixel in this lane)
__device__ __forceinline__ void ev_count(int K, int lane, int below, bool tied, unsigned long long& mine,
                                         unsigned long long& c64, unsigned long long& ctied) {
    for (int b = 0; b <= K; b++) {
        const unsigned long long c = (unsigned long long)__popcll(__ballot(below == b));
        if (b < 64) mine += lane == b ? c : 0ull;
        else c64 += c;
    }
    ctied += (unsigned long long)__popcll(__ballot(below >= 0 && tied));
}

template <int KA>
__global__ void __launch_bounds__(64) k_ensemble_verify(const EvArgs s) {
    extern __shared__ __align__(16) float ev_tile[];          // [K][EV_PIX]
    constexpr int EA = CmElem<KA>::bytes;
    const int lane = threadIdx.x;
    const int K = s.K;
    const bool same_phase = (s.draw_stride & 3) == 0;
    unsigned long long mine = 0ull, c64 = 0ull, ctied = 0ull;
    for (long long item = blockIdx.x; item < s.items; item += gridDim.x) {
        const long long cs = item / s.nch;
        const int ch = (int)(item - cs * s.nch);
        const float* yc = s.y + cs * s.case_stride;
        const unsigned char* ac = s.a + cs * s.a_stride * EA;
        int h = 0;
        if (same_phase)
            for (int t = 3; t >= 0; t--)
                if (((uintptr_t)(yc + t) & 15) == 0) h = t;
        const long long head = h < s.plane ? h : s.plane;
        const long long groups = (s.plane - head) >> 2;
        const long long tail0 = head + (groups << 2);
        EvAcc acc = {0u, 0.0, 0.0, 0.0, 0.0};
        if (ch == 0 && (head > 0 || tail0 < s.plane)) {
            long long e = -1;
            if (lane < head) e = lane;
            else if (lane >= 4 && lane - 4 < s.plane - tail0) e = tail0 + lane - 4;
            int below = -1;
            bool tied = false;
            if (e >= 0) {
                for (int k = 0; k < K; k++) ev_tile[k * EV_PIX + lane] = yc[k * s.draw_stride + e];
                below = ev_pixel<KA>(s, ev_tile + lane, ac, e, acc, tied);
            }
            ev_count(K, lane, below, tied, mine, c64, ctied);
            __syncthreads();
        }
        const long long g0 = (long long)ch * s.chunk;
        const long long g1 = g0 + s.chunk < groups ? g0 + s.chunk : groups;
        for (long long gb = g0; gb < g1; gb += 64) {
            const long long e0 = head + (gb << 2);
            const int npix = (int)(g1 - gb < 64 ? g1 - gb : 64) << 2;
            if (same_phase) {
                if (gb + lane < g1) {
                    const float* src = yc + e0 + 4 * lane;
#pragma unroll 4
                    for (int k = 0; k < K; k++)
                        *reinterpret_cast<float4*>(ev_tile + k * EV_PIX + 4 * lane) =
                            *reinterpret_cast<const float4*>(src + k * s.draw_stride);
                }
            } else {
                for (int c = lane; c < npix; c += 64) {
                    const float* src = yc + e0 + c;
#pragma unroll 4
                    for (int k = 0; k < K; k++) ev_tile[k * EV_PIX + c] = src[k * s.draw_stride];
                }
            }
            __syncthreads();
            for (int c0 = 0; c0 < npix; c0 += 64) {
                const int c = c0 + lane;
                int below = -1;
                bool tied = false;
                if (c < npix) below = ev_pixel<KA>(s, ev_tile + c, ac, e0 + c, acc, tied);
                ev_count(K, lane, below, tied, mine, c64, ctied);
            }
            __syncthreads();
        }
        const double Kd = (double)K;
        double v0 = acc.sa / Kd, v1 = acc.sb / (Kd * Kd), v2 = acc.e, v3 = acc.v;
        unsigned n = acc.n;
        for (int off = 32; off > 0; off >>= 1) {
            n += __shfl_down(n, off, 64);
            v0 += __shfl_down(v0, off, 64);
            v1 += __shfl_down(v1, off, 64);
            v2 += __shfl_down(v2, off, 64);
            v3 += __shfl_down(v3, off, 64);
        }
        if (lane == 0) {
            double* o = s.sums + item * EV_SUMS;
            o[0] = (double)n;
            o[1] = v0;
            o[2] = v1;
            o[3] = v2;
            o[4] = v3;
        }
    }
    long long* rp = s.ranks + (long long)blockIdx.x * (K + 2);
    if (lane <= K) rp[lane] = (long long)mine;      // (lane <= 63: bin 64 of K = 64 follows)
    if (lane == 0) {
        if (K == 64) rp[64] = (long long)c64;
        rp[K + 1] = (long long)ctied;
    }
}

// Workgroup b < n_bin: ranks[b] += the sum over the n_block workgroups' counts of bin b (integers: exact in any order; one
// load, add and store of ranks[b]).  The workgroups after them, when a case has nch > 1 chunks: out[i][q] = the sum over
// chunks k = 0 .. nch-1, in that order, of part[(i * nch + k)][q]
__global__ void __launch_bounds__(256) k_verify_fold(const double* __restrict__ part, long long n_case, int nch,
                                                     double* __restrict__ out, const long long* __restrict__ rpart,
                                                     int n_block, int n_bin, long long* __restrict__ ranks) {
    __shared__ long long red[CM_WAVES];
    if ((int)blockIdx.x < n_bin) {
        const int b = blockIdx.x;
        long long t = 0;
        for (int i = threadIdx.x; i < n_block; i += 256) t += rpart[(long long)i * n_bin + b];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < CM_WAVES; w++) t += red[w];
            ranks[b] = ranks[b] + t;
        }
        return;
    }
    // one thread per (case, sum): its chunks' partials in chunk order, sixteen loads in flight
    const long long nb = (long long)gridDim.x - n_bin;
    for (long long j = ((long long)blockIdx.x - n_bin) * 256 + threadIdx.x; j < n_case * EV_SUMS; j += nb * 256) {
        const long long i = j / EV_SUMS;
        const double* col = part + i * nch * EV_SUMS + (j - i * EV_SUMS);
        double sum = 0.0;
        int k = 0;
        for (; k + 15 < nch; k += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = col[(long long)(k + u) * EV_SUMS];
#pragma unroll
            for (int u = 0; u < 16; u++) sum += v[u];
        }
        for (; k < nch; k++) sum += col[(long long)k * EV_SUMS];
        out[j] = sum;
    }
}

// ---- case pages (evaluate_cae's per-case images): the value range of channel 0 and its palette indices.
// KS is the source's element kind, KB the kind of the optional operand subtracted from it in fp64 (-1: none).
template <int K> struct CpBytes { static constexpr int bytes = CmElem<K>::bytes; };
template <> struct CpBytes<-1> { static constexpr int bytes = 4; };

template <int KS, int KB>
__device__ __forceinline__ double cp_value1(const unsigned char* sc, const unsigned char* bc, long long e) {
    const double v = cm_load1<KS>(sc, e);
    if constexpr (KB >= 0) return v - cm_load1<KB>(bc, e);
    else return v;
}

template <int KS, int KB>
__device__ __forceinline__ void cp_value4(const unsigned char* sc, const unsigned char* bc, long long e, bool vec,
                                          double v[4]) {
    cm_load4<KS>(sc, e, vec, v);
    if constexpr (KB >= 0) {
        double b[4];
        cm_load4<KB>(bc, e, vec, b);
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] -= b[j];
    }
}

// NaN and +-Inf are left out; min / max compare by value
__device__ __forceinline__ void cp_range_acc(double v, double& mn, double& mx, long long& n) {
    if (fabs(v) < __builtin_huge_val()) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        n++;
    }
}

// k_case_measures' items and loads: one wave per (case, 4096-element chunk), 16-byte loads from the case's first common
// 16-byte phase on.  A wave keeps min / max / count over all its items, the workgroup's four waves meet in LDS and
// part[blockIdx.x] = {min, max, count} is one plain store: no atomics.  min and max do not depend on the order and the
// count is an integer, so the result is the same from run to run.
template <int KS, int KB>
__global__ void __launch_bounds__(256) k_case_range(const unsigned char* __restrict__ s, long long s_stride,
                                                    const unsigned char* __restrict__ b, long long b_stride,
                                                    long long plane, int nch, long long items,
                                                    double* __restrict__ part) {
    constexpr int ES = CpBytes<KS>::bytes, EB = CpBytes<KB>::bytes;
    __shared__ double red[CM_WAVES][3];
    const int lane = threadIdx.x & 63;
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    long long cnt = 0;
    for (long long item = (long long)blockIdx.x * CM_WAVES + (threadIdx.x >> 6); item < items;
         item += (long long)gridDim.x * CM_WAVES) {
        const long long cs = item / nch;
        const int ch = (int)(item - cs * nch);
        const unsigned char* sc = s + cs * s_stride * ES;
        const unsigned char* bc = KB >= 0 ? b + cs * b_stride * EB : nullptr;
        int h = -1;
        for (int t = 3; t >= 0; t--)
            if ((((uintptr_t)(sc + t * ES) | (KB >= 0 ? (uintptr_t)(bc + t * EB) : 0)) & 15) == 0) h = t;
        const bool vec = h >= 0;
        const long long head = vec ? (h < plane ? h : plane) : 0;
        const long long groups = (plane - head) >> 2;
        const long long tail0 = head + (groups << 2);
        if (ch == 0) {
            if (lane < head) cp_range_acc(cp_value1<KS, KB>(sc, bc, lane), mn, mx, cnt);
            else if (lane >= 4 && lane - 4 < plane - tail0)
                cp_range_acc(cp_value1<KS, KB>(sc, bc, tail0 + lane - 4), mn, mx, cnt);
        }
        const long long g0 = (long long)ch * CM_GROUPS;
        const long long g1 = g0 + CM_GROUPS < groups ? g0 + CM_GROUPS : groups;
        long long g = g0 + lane;
        for (; g + 3 * 64 < g1; g += 4 * 64) {      // four groups in flight per lane
            double v[4][4];
#pragma unroll
            for (int u = 0; u < 4; u++) cp_value4<KS, KB>(sc, bc, head + ((g + u * 64) << 2), vec, v[u]);
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) cp_range_acc(v[u][j], mn, mx, cnt);
        }
        for (; g < g1; g += 64) {
            double v[4];
            cp_value4<KS, KB>(sc, bc, head + (g << 2), vec, v);
#pragma unroll
            for (int j = 0; j < 4; j++) cp_range_acc(v[j], mn, mx, cnt);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double omn = __shfl_down(mn, off, 64), omx = __shfl_down(mx, off, 64);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        cnt += __shfl_down(cnt, off, 64);
    }
    if (lane == 0) {
        red[threadIdx.x >> 6][0] = mn;
        red[threadIdx.x >> 6][1] = mx;
        red[threadIdx.x >> 6][2] = (double)cnt;      // exact: far below 2^53
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CM_WAVES; w++) {
            mn = red[w][0] < mn ? red[w][0] : mn;
            mx = red[w][1] > mx ? red[w][1] : mx;
            red[0][2] += red[w][2];
        }
        part[3 * (size_t)blockIdx.x] = mn;
        part[3 * (size_t)blockIdx.x + 1] = mx;
        part[3 * (size_t)blockIdx.x + 2] = red[0][2];
    }
}

// out = the fold of n_part workgroup partials {min, max, count}; one workgroup
__global__ void __launch_bounds__(256) k_range_fold(const double* __restrict__ part, int n_part, double* __restrict__ out) {
    __shared__ double red[CM_WAVES][3];
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val(), cnt = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) {
        mn = part[3 * i] < mn ? part[3 * i] : mn;
        mx = part[3 * i + 1] > mx ? part[3 * i + 1] : mx;
        cnt += part[3 * i + 2];                       // integers below 2^53: exact in any order
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double omn = __shfl_down(mn, off, 64), omx = __shfl_down(mx, off, 64);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        cnt += __shfl_down(cnt, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = mn;
        red[threadIdx.x >> 6][1] = mx;
        red[threadIdx.x >> 6][2] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CM_WAVES; w++) {
            mn = red[w][0] < mn ? red[w][0] : mn;
            mx = red[w][1] > mx ? red[w][1] : mx;
            cnt += red[w][2];
        }
        out[0] = mn;
        out[1] = mx;
        out[2] = cnt;
    }
}

// The palette index of one value: 0 for NaN, else 1 + the nearest of 255 levels over [lo, hi] (all of them the middle
// level when hi <= lo).  fp64, every operation rounded on its own - a numpy restatement gives the same bytes only if
// the multiply and the add are not fused.
__device__ __forceinline__ unsigned cp_index(double v, double lo, double hi) {
#pragma clang fp contract(off)
    if (v != v) return 0u;
    double t = 0.5;
    if (hi > lo) {
        t = (v - lo) / (hi - lo);
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double scaled = t * 254.0;
    return 1u + (unsigned)(int)(scaled + 0.5);
}

// A selected case's output is one flat stream of height * (width + 1) bytes: PNG scanlines, each a filter byte 0 and
// `width` palette indices.  The stream is cut at its first 4-byte aligned address: a lane assembles one aligned dword of
// four output bytes (the row and column of its first byte by one 32-bit division, the other three by stepping) and
// stores it; consecutive lanes store consecutive dwords.  The up to 3 bytes before and after the dwords are byte stores
// by lanes of chunk 0.  The four source elements of a dword are consecutive in the plane (a filter byte in between costs
// nothing) but at any element phase, so they are element loads: four loads per lane, the wave's four covering the same
// lines.  One wave per (selected case, RC_DWORDS dwords) item.  A case index outside [0, n_case) draws index 0.
constexpr int RC_DWORDS = 1024;          // 4096 output bytes per chunk

template <int KS, int KB>
__device__ __forceinline__ unsigned cp_pixel(const unsigned char* sc, const unsigned char* bc, unsigned y, unsigned c,
                                             unsigned height, unsigned width, bool flip, bool valid, double lo,
                                             double hi) {
    const unsigned sy = flip ? height - 1u - y : y;
    const long long e = (long long)sy * width + (c ? c - 1u : 0u);       // always inside the plane
    const unsigned idx = valid ? cp_index(cp_value1<KS, KB>(sc, bc, e), lo, hi) : 0u;
    return c ? idx : 0u;
}

template <int KS, int KB>
__global__ void __launch_bounds__(256) k_render_cases(const unsigned char* __restrict__ s, long long s_stride,
                                                      const unsigned char* __restrict__ b, long long b_stride,
                                                      const int* __restrict__ cases, long long n_case, unsigned height,
                                                      unsigned width, double lo, double hi, int flip_y, int nch,
                                                      long long items, unsigned char* __restrict__ out) {
    constexpr int ES = CpBytes<KS>::bytes, EB = CpBytes<KB>::bytes;
    const unsigned lane = threadIdx.x & 63;
    const unsigned pitch = width + 1u;
    const unsigned len = height * pitch;            // the host keeps it below 2^31
    const bool flip = flip_y != 0;
    for (long long item = (long long)blockIdx.x * CM_WAVES + (threadIdx.x >> 6); item < items;
         item += (long long)gridDim.x * CM_WAVES) {
        const long long k = item / nch;
        const unsigned ch = (unsigned)(item - k * nch);
        long long cs = cases ? (long long)cases[k] : k;
        const bool valid = cs >= 0 && cs < n_case;
        if (!valid) cs = 0;
        const unsigned char* sc = s + cs * s_stride * ES;
        const unsigned char* bc = KB >= 0 ? b + cs * b_stride * EB : nullptr;
        unsigned char* ob = out + k * (long long)len;
        unsigned head = (4u - (unsigned)((uintptr_t)ob & 3)) & 3u;
        if (head > len) head = len;
        const unsigned ndw = (len - head) >> 2;
        const unsigned tail0 = head + (ndw << 2);
        if (ch == 0) {
            unsigned q = len;
            if (lane < head) q = lane;
            else if (lane >= 4 && lane - 4 < len - tail0) q = tail0 + lane - 4;
            if (q < len) {
                const unsigned y = q / pitch;
                ob[q] = (unsigned char)cp_pixel<KS, KB>(sc, bc, y, q - y * pitch, height, width, flip, valid, lo, hi);
            }
        }
        const unsigned d0 = ch * RC_DWORDS;
        const unsigned d1 = d0 + RC_DWORDS < ndw ? d0 + RC_DWORDS : ndw;
        for (unsigned d = d0 + lane; d < d1; d += 64) {
            const unsigned q = head + (d << 2);
            unsigned y = q / pitch;
            unsigned c = q - y * pitch;
            unsigned w = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                w |= cp_pixel<KS, KB>(sc, bc, y, c, height, width, flip, valid, lo, hi) << (8 * j);
                if (++c == pitch) {
                    c = 0;
                    y++;
                }
            }
            *reinterpret_cast<unsigned*>(ob + q) = w;
        }
    }
}

// ---- per-pixel skill sums (include/cae_hip.h, cae_pixel_sums): the reduction along the case axis.  For pixel x, over the
// cases whose prediction p and target a at x are both finite, in fp64: {n, S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2,
// S a'p'} with d = p - a, a' = a - shift, p' = p - shift; ABOUT (cae_pixel_sums_about): a shift of its own per pixel, one
// plane for a and one for p, read once per lane and chunk.
// One wave (a workgroup of its own) per (tile of 256 consecutive pixels, chunk of `chunk` consecutive cases).  A lane
// owns one 4-pixel group of the tile and walks the chunk's cases in case order with PsFlight cases' loads in flight
// (128 bytes per lane, or 96), the 36 accumulators in registers (the four counts as integers).  A case that is no pair at a pixel adds exact zeros
// there (both values are replaced by `shift`), so it leaves that pixel's sums as skipping it would and touches no other
// pixel.  Nothing crosses a lane: the item's nine values per pixel are plain stores into plane k of out[chunk] - the
// partials, or the result itself when there is one chunk - and k_pixel_fold adds the chunks' partials in chunk order.  No
// atomics; the sums depend on the arguments alone.  16-byte loads need every case's group on one 16-byte phase: the host
// finds case 0's first element `head` where both operands are 16 bytes aligned and sets `vec` when both case strides keep
// that phase; the `head` pixels before it and the up to 3 after the last whole group go element by element to lanes of
// tile 0.  Otherwise head = 0 and every load is an element load.
// Registers: the loaded words wait unconverted (cm_word turns one pixel's pair into doubles when it is summed) and a
// scheduling barrier after every pixel keeps the compiler from converting a whole round of loads ahead of the sums, which
// costs 100 registers more.  A case's byte offset is wave-uniform (ps_uniform), the lane adds a 32-bit offset of its own.
constexpr int PS_SUMS = 9;
constexpr int PS_TILE = 64;             // 4-pixel groups per tile: one per lane

struct PsArgs {
    const unsigned char* p;     // case c: elements c * stride .. + plane
    const unsigned char* a;
    long long p_stride, a_stride, n_case, plane;
    long long chunk, n_chunk;   // cases per chunk, chunks
    int head, vec;
    double shift;
    const double* shifts;       // ABOUT: a' = a - shifts[x], p' = p - shifts[plane + x] in place of `shift`
    double* out;                // (chunks, PS_SUMS, plane)
};

template <int K> struct PsWord { typedef unsigned long long type; };
template <> struct PsWord<0> { typedef unsigned type; };
template <> struct PsWord<1> { typedef unsigned type; };

// cases in flight per lane: four of two 4-byte operands, else two (the per-pixel shifts of ABOUT take 16 registers more)
template <int KP, int KA, bool ABOUT> struct PsFlight {
    static constexpr int cases = !ABOUT && CmElem<KP>::bytes + CmElem<KA>::bytes == 8 ? 4 : 2;
};

// a wave-uniform byte offset, said so to the compiler: it then stays in scalar registers
__device__ __forceinline__ long long ps_uniform(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the stored words of N elements from byte b of the case at c (c wave-uniform, b the lane's: a scalar base and a 32-bit
// offset for the load): 16-byte loads when `vec`, else element loads
template <int K, int N>
__device__ __forceinline__ void ps_load(const unsigned char* c, unsigned b, bool vec, typename PsWord<K>::type w[N]) {
    typedef typename PsWord<K>::type W;
    if constexpr (N == 4) {
        if (vec) {
            if constexpr (CmElem<K>::bytes == 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(c + b);
                w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
            } else {
                const ulonglong2 q0 = *reinterpret_cast<const ulonglong2*>(c + b);
                const ulonglong2 q1 = *reinterpret_cast<const ulonglong2*>(c + (b + 16u));
                w[0] = q0.x, w[1] = q0.y, w[2] = q1.x, w[3] = q1.y;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) w[j] = *reinterpret_cast<const W*>(c + (b + (unsigned)(j * CmElem<K>::bytes)));
}

// acc: S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2, S a'p' with a' = a - sa, p' = p - sp.  DIFF: sa and sp may differ, so
// the d of a case that is no pair is set to zero on its own
template <bool DIFF>
__device__ __forceinline__ void ps_acc(double p, double a, double sa, double sp, unsigned& n, double acc[8]) {
    const bool pair = fabs(p) < __builtin_huge_val() && fabs(a) < __builtin_huge_val();
    p = pair ? p : sp;
    a = pair ? a : sa;
    n += pair ? 1u : 0u;
    double d = p - a;
    if constexpr (DIFF) d = pair ? d : 0.0;
    const double as = a - sa, ps = p - sp;
    acc[0] += d;
    acc[1] += fabs(d);
    acc[2] += d * d;
    acc[3] += as;
    acc[4] += ps;
    acc[5] += as * as;
    acc[6] += ps * ps;
    acc[7] += as * ps;
}

// pixels e0 + e .. + N-1 (e0 wave-uniform, e the lane's) over the cases [c0, c1), stored to the nine planes at dst
template <int KP, int KA, bool ABOUT, int N>
__device__ __forceinline__ void ps_walk(const PsArgs& s, long long c0, long long c1, long long e0, unsigned e, bool vec,
                                        double* __restrict__ dst) {
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes, U = PsFlight<KP, KA, ABOUT>::cases;
    typedef typename PsWord<KP>::type WP;
    typedef typename PsWord<KA>::type WA;
    double acc[N][8];
    unsigned n[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        n[j] = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) acc[j][k] = 0.0;
    }
    double sa[ABOUT ? N : 1], sp[ABOUT ? N : 1];        // the shifts: per pixel (ABOUT) or the one of the call
#pragma unroll
    for (int j = 0; j < (ABOUT ? N : 1); j++) {
        sa[j] = ABOUT ? s.shifts[e0 + e + j] : s.shift;
        sp[j] = ABOUT ? s.shifts[s.plane + e0 + e + j] : s.shift;
    }
    const long long pstep = s.p_stride * EP, astep = s.a_stride * EA;
    long long pc = c0 * pstep + e0 * EP, ac = c0 * astep + e0 * EA;      // byte offsets of the case in flight
    long long c = c0;
    for (; c + U - 1 < c1; c += U) {        // U cases in flight per lane, summed in case order
        WP wp[U][N];
        WA wa[U][N];
#pragma unroll
        for (int u = 0; u < U; u++) {
            ps_load<KP, N>(s.p + ps_uniform(pc + u * pstep), e * EP, vec, wp[u]);
            ps_load<KA, N>(s.a + ps_uniform(ac + u * astep), e * EA, vec, wa[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int j = 0; j < N; j++) {
                ps_acc<ABOUT>(cm_word<KP>(wp[u][j]), cm_word<KA>(wa[u][j]), sa[ABOUT ? j : 0], sp[ABOUT ? j : 0], n[j], acc[j]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        pc += U * pstep;
        ac += U * astep;
    }
    for (; c < c1; c++) {
        WP wp[N];
        WA wa[N];
        ps_load<KP, N>(s.p + ps_uniform(pc), e * EP, vec, wp);
        ps_load<KA, N>(s.a + ps_uniform(ac), e * EA, vec, wa);
#pragma unroll
        for (int j = 0; j < N; j++)
            ps_acc<ABOUT>(cm_word<KP>(wp[j]), cm_word<KA>(wa[j]), sa[ABOUT ? j : 0], sp[ABOUT ? j : 0], n[j], acc[j]);
        pc += pstep;
        ac += astep;
    }
    dst += e0 + e;
#pragma unroll
    for (int j = 0; j < N; j++) {
        dst[j] = (double)n[j];
#pragma unroll
        for (int k = 0; k < 8; k++) dst[(k + 1) * s.plane + j] = acc[j][k];
    }
}

// grid (tiles, chunks walked with stride gridDim.y), one wave per workgroup
template <int KP, int KA, bool ABOUT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8))) k_pixel_sums(const PsArgs s) {
    const unsigned lane = threadIdx.x;
    const bool vec = s.vec != 0;
    const long long head = s.head;
    const long long groups = (s.plane - head) >> 2;
    const long long tail0 = head + (groups << 2);
    const long long g0 = (long long)blockIdx.x * PS_TILE;
    for (long long ch = blockIdx.y; ch < s.n_chunk; ch += gridDim.y) {
        const long long c0 = ch * s.chunk;
        const long long c1 = c0 + s.chunk < s.n_case ? c0 + s.chunk : s.n_case;
        double* dst = s.out + ch * PS_SUMS * s.plane;
        if (g0 + lane < groups) ps_walk<KP, KA, ABOUT, 4>(s, c0, c1, head + (g0 << 2), lane << 2, vec, dst);
        if (blockIdx.x == 0) {
            if (lane < head) ps_walk<KP, KA, ABOUT, 1>(s, c0, c1, 0, lane, false, dst);
            else if (lane >= 4 && lane - 4 < s.plane - tail0) ps_walk<KP, KA, ABOUT, 1>(s, c0, c1, tail0, lane - 4, false, dst);
        }
    }
}

// out[j] = sum over chunks k = 0 .. n_chunk-1, in that order, of part[k * n + j]  (n = PS_SUMS * plane); eight partials
// in flight per lane
__global__ void __launch_bounds__(256) k_pixel_fold(const double* __restrict__ part, long long n_chunk, long long n,
                                                    double* __restrict__ out) {
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        const double* col = part + j;
        double sum = 0.0;
        long long k = 0;
        for (; k + 7 < n_chunk; k += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = col[(k + u) * n];
#pragma unroll
            for (int u = 0; u < 8; u++) sum += v[u];
        }
        for (; k < n_chunk; k++) sum += col[k * n];
        out[j] = sum;
    }
}

}  // namespace cae
