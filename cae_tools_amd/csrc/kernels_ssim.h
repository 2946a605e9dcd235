// kernels_ssim.h - device only: per-case SSIM / MS-SSIM sums of prediction against target (include/cae_hip.h, cae_case_ssim;
// DESIGN.md section 9).  The definition is the VAE loss's (oracle/vae_oracle.py, kernels_vae.h) in fp64, with a rule for
// values that are not finite and a number per case and scale in place of one batch mean.  Three kinds of launch:
//   k_ssim_pool   the normalised fp64 planes of scale s + 1 from scale s (scale 0: the operands as stored), one per level
//   k_case_ssim   the row walk of kernels_vae.h (k_ssim_fwd_rows) over every scale at once: a wave owns 64 input columns
//                 (54 outputs) and a band of rows, a lane loads its column's pixel of a row, the horizontal taps come from
//                 the neighbour lanes (DPP wave shift, a double as two dwords), the vertical filter reads the last eleven
//                 rows' horizontal results from a register ring with compile-time indices.  {n, S ssim, S cs} of the wave
//                 are stored plainly as the partial of its (case, scale, band, strip)
//   k_ssim_fold   the partials of a (case, scale) added in (band, strip) order by one lane
// No floating-point atomics; the cut into bands and strips depends on the scale's shape alone.  Filter order: along the
// row (w) first, then along the column (h); taps in ascending order, each an fma onto a sum that starts at 0; the second
// moments filter the rounded products x x, y y, x y.  Everything else is rounded operation by operation (no contraction):
// with p bit-identical to a the three second moments are then the same bits, cs and ssim are exactly 1.
// Uses the element conversions of case_elem.h (cm_word).
#pragma once
#include "case_elem.h"

#include <utility>

namespace cae {

constexpr int SS_WIN = 11, SS_HALO = SS_WIN - 1;
constexpr int SS_COLS = 64 - SS_HALO;       // output columns of a wave
constexpr int SS_SCALES = 5;
constexpr int SS_AHEAD = 4;                 // rows requested ahead of the one being filtered (5 spills: DESIGN.md section 9)
constexpr int SS_MAX_SIDE = 16384;

struct SsWindow {
    double g[SS_WIN];
};

// output rows of a wave by the scale's height: a band of R rows filters R + 10, and the walk is unrolled by eleven rows
// without a guard (a guarded row keeps both states of the ring alive: 300 registers), so R + 10 is a multiple of eleven
// and only a plane's last band filters rows it has no use for
inline int ss_band_rows(int rows) { return rows >= 400 ? 34 : (rows >= 200 ? 23 : 12); }

struct SsScale {
    const unsigned char* x;                 // prediction / target planes of the scale: the operands (scale 0) or the workspace
    const unsigned char* y;
    long long x_stride, y_stride;           // elements between cases
    int xk, yk;                             // CAE_ELEM_* kind
    int h, w;
    int rb, n_band, n_strip;                // 0 bands: a side below 11, no window
    long long first;                        // the scale's first item; a case has n_band * n_strip items
};

struct SsArgs {
    SsScale s[SS_SCALES];
    int n_scale;
    long long n_case, items;
    double shift, scale;                    // scale 0 only; the pooled planes are stored normalised
    SsWindow win;
    double* part;                           // [items][3]
};

__device__ __forceinline__ unsigned long long ss_raw(const unsigned char* c, long long e, int kind) {
    return kind < 2 ? (unsigned long long)reinterpret_cast<const unsigned*>(c)[e] : reinterpret_cast<const unsigned long long*>(c)[e];
}

__device__ __forceinline__ double ss_value(unsigned long long raw, int kind) {
    switch (kind) {
    case 0: return cm_word<0>(raw);
    case 1: return cm_word<1>(raw);
    case 2: return cm_word<2>(raw);
    default: return cm_word<3>(raw);
    }
}

// (v - shift) * scale, the subtraction and the product each rounded on its own
__device__ __forceinline__ double ss_norm(double v, double shift, double scale) { return __dmul_rn(__dsub_rn(v, shift), scale); }

__device__ __forceinline__ bool ss_finite(double v) { return v - v == 0.0; }

// lane i <- lane i + 1 (lane 63: 0), a double as its two dwords
__device__ __forceinline__ double ss_from_right(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x130, 0xF, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)b >> 32), 0x130, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double ss_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <class F, int... I>
__device__ __forceinline__ void ss_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void ss_static_for(F&& f) {
    ss_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// dst[c][0 | 1][ho][wo]: the 2 x 2 average of the normalised source planes, ((x00 + x01) + (x10 + x11)) * 0.25 with zeros
// for the padding (pad = size mod 2 on both sides of an axis).  The source is the operands (kind, shift, scale) or the level
// above (fp64, shift 0, scale 1: the normalisation is then exact).  NaN and Inf go into the pooled pixel as IEEE carries them.
__global__ void __launch_bounds__(256) k_ssim_pool(const unsigned char* __restrict__ x, int xk, long long x_stride,
                                                   const unsigned char* __restrict__ y, int yk, long long y_stride, long long n_case,
                                                   int h, int w, double shift, double scale, double* __restrict__ dst) {
    const int ph = h & 1, pw = w & 1;
    const int ho = (h + 2 * ph) / 2, wo = (w + 2 * pw) / 2;
    const long long per = (long long)ho * wo, total = n_case * per;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long c = o / per, r = o - c * per;
        const int i = (int)(r / wo), j = (int)(r - (long long)i * wo);
        const unsigned char* xc = x + c * x_stride * (xk < 2 ? 4 : 8);
        const unsigned char* yc = y + c * y_stride * (yk < 2 ? 4 : 8);
        double vx[4], vy[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = 2 * i - ph + (q >> 1), col = 2 * j - pw + (q & 1);
            const bool in = row >= 0 && row < h && col >= 0 && col < w;
            const long long e = (long long)row * w + col;
            vx[q] = in ? ss_norm(ss_value(ss_raw(xc, e, xk), xk), shift, scale) : 0.0;
            vy[q] = in ? ss_norm(ss_value(ss_raw(yc, e, yk), yk), shift, scale) : 0.0;
        }
        dst[(2 * c) * per + r] = ((vx[0] + vx[1]) + (vx[2] + vx[3])) * 0.25;
        dst[(2 * c + 1) * per + r] = ((vy[0] + vy[1]) + (vy[2] + vy[3])) * 0.25;
    }
}

// One wave per item = (scale, case, band, strip); four items per workgroup, no barrier, no LDS.
__global__ void __launch_bounds__(256, 2) k_case_ssim(const SsArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.items) return;
    int si = 0;
#pragma unroll
    for (int k = 1; k < SS_SCALES; k++)
        if (k < a.n_scale && a.s[k].n_band > 0 && item >= a.s[k].first) si = k;
    const SsScale& sc = a.s[si];
    const long long local = item - sc.first;
    const int per_case = sc.n_band * sc.n_strip;
    const long long c = local / per_case;
    const int rem = (int)(local - c * per_case);
    const int band = rem / sc.n_strip, strip = rem - band * sc.n_strip;
    const int H = sc.h, W = sc.w, xk = sc.xk, yk = sc.yk;
    const int Hv = H - SS_HALO, Wv = W - SS_HALO;
    const int x0 = strip * SS_COLS, y0 = band * sc.rb;
    const int n_out = min(sc.rb, Hv - y0), n_in = n_out + SS_HALO;
    const bool in_ok = x0 + lane < W;
    const bool out_ok = lane < SS_COLS && x0 + lane < Wv;
    const double shift = si == 0 ? a.shift : 0.0, scale = si == 0 ? a.scale : 1.0;
    const unsigned char* xc = sc.x + c * sc.x_stride * (xk < 2 ? 4 : 8);
    const unsigned char* yc = sc.y + c * sc.y_stride * (yk < 2 ? 4 : 8);
    const long long e0 = (long long)y0 * W + (in_ok ? x0 + lane : 0);
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;

    double ring[SS_WIN][5];
    unsigned bad_rows = 0;                  // bit k: row r - k has a bad pixel under the lane's eleven columns
    unsigned long long xq[SS_WIN], yq[SS_WIN];      // rows in flight as loaded: row r lives in slot r % 11
    double acc_ssim = 0.0, acc_cs = 0.0;
    int acc_n = 0;
#pragma unroll
    for (int d = 0; d < SS_AHEAD; d++) {
        const bool ok = in_ok && d < n_in;
        xq[d] = ok ? ss_raw(xc, e0 + (long long)d * W, xk) : 0ull;
        yq[d] = ok ? ss_raw(yc, e0 + (long long)d * W, yk) : 0ull;
    }
    for (int base = 0; base < n_in; base += SS_WIN) {
        ss_static_for<SS_WIN>([&](auto S) {
#pragma clang fp contract(off)
            constexpr int s = decltype(S)::value;
            const int r = base + s;             // input row y0 + r; r % 11 == s.  Rows from n_in on are zeros and give no output
            {
                double xs = in_ok ? ss_norm(ss_value(xq[s], xk), shift, scale) : 0.0;
                double ys = in_ok ? ss_norm(ss_value(yq[s], yk), shift, scale) : 0.0;
                {
                    const bool ok = in_ok && r + SS_AHEAD < n_in;
                    xq[(s + SS_AHEAD) % SS_WIN] = ok ? ss_raw(xc, e0 + (long long)(r + SS_AHEAD) * W, xk) : 0ull;
                    yq[(s + SS_AHEAD) % SS_WIN] = ok ? ss_raw(yc, e0 + (long long)(r + SS_AHEAD) * W, yk) : 0ull;
                }
                // a value that is not finite enters the filters as 0 and marks every window over it
                const bool bad = !(ss_finite(xs) && ss_finite(ys));
                if (bad) xs = 0.0, ys = 0.0;
                const unsigned long long mask = __ballot(bad);
                bad_rows = (bad_rows << 1) | (((mask >> lane) & 0x7FFull) != 0ull ? 1u : 0u);
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
                for (int t = 0; t < SS_WIN; t++) {
                    const double g = a.win.g[t];
                    a0 = fma(g, xs, a0);
                    a1 = fma(g, ys, a1);
                    a2 = fma(g, xs * xs, a2);
                    a3 = fma(g, ys * ys, a3);
                    a4 = fma(g, xs * ys, a4);
                    if (t + 1 < SS_WIN) {
                        xs = ss_from_right(xs);
                        ys = ss_from_right(ys);
                    }
                }
                ring[s][0] = a0, ring[s][1] = a1, ring[s][2] = a2, ring[s][3] = a3, ring[s][4] = a4;
                if (r >= SS_HALO) {             // output row y0 + r - 10: input rows r - 10 .. r = ring[(s + 1 + t) % 11]
                    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int t = 0; t < SS_WIN; t++) {
                        const double g = a.win.g[t];
#pragma unroll
                        for (int k = 0; k < 5; k++) m[k] = fma(g, ring[(s + 1 + t) % SS_WIN][k], m[k]);
                    }
                    if (out_ok && r < n_in && (bad_rows & 0x7FFu) == 0u) {
                        const double mu1 = m[0], mu2 = m[1];
                        const double s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
                        const double cs = (2.0 * s12 + C2) / (s11 + s22 + C2);
                        const double ssim = ((2.0 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs;
                        acc_ssim += ssim;
                        acc_cs += cs;
                        acc_n += 1;
                    }
                }
            }
        });
    }
    const double t0 = ss_wave_sum((double)acc_n), t1 = ss_wave_sum(acc_ssim), t2 = ss_wave_sum(acc_cs);
    if (lane == 0) {
        double* o = a.part + 3 * item;
        o[0] = t0, o[1] = t1, o[2] = t2;
    }
}

// sums[c][s][0..2]: the partials of the (case, scale) added in item order (band, then strip), or three zeros where the
// scale has no window; one lane per (case, scale, k)
__global__ void __launch_bounds__(256) k_ssim_fold(const SsArgs a, double* __restrict__ sums) {
    const long long total = a.n_case * a.n_scale * 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long cs = i / 3;
        const int k = (int)(i - cs * 3);
        const long long c = cs / a.n_scale;
        const int si = (int)(cs - c * a.n_scale);
        const SsScale& sc = a.s[si];
        const int per_case = sc.n_band * sc.n_strip;
        const double* p = a.part + 3 * (sc.first + c * per_case) + k;
        double v = 0.0;
        for (int q = 0; q < per_case; q++) v += p[3 * (long long)q];
        sums[i] = v;
    }
}

}  // namespace cae
