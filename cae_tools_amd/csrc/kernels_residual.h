// kernels_residual.h - device only: the residual target over the interpolated input (include/cae_hip.h, cae_residual_scan,
// cae_residual_pack_rows, cae_residual_restore_f64; DESIGN.md section 9, "Residual target").  With b the field
// cae_case_baseline interpolates from channel 0 of a low-resolution variable (NaN where a tap is not finite):
//   k_residual<MODE, RS_SCAN>     r = (double)t - b per pixel; {k, min r, max r} of the wave stored plainly as the partial of
//                                 its (case, band, strip): k counts the r that are not finite, min and max run over the others
//   k_residual<MODE, RS_PACK>     y = (float)((r - rmin) / span) into row dst_rows[case] (0 at span 0; (float)r when not
//                                 enabled; NaN where r is not finite)
//   k_residual<MODE, RS_RESTORE>  p = b + (rmin + (double)y * span)  (b + (double)y when not enabled; NaN where b or y is)
//   k_residual_fold               the partials of a scan folded by one workgroup: integers added, min and max compared
// The mapping is k_case_baseline's and the walk is its BlWalk (kernels_baseline.h): a wave owns BL_COLS output columns of a
// band of BL_ROWS rows, the fp32 rows of t or y stream past, BL_AHEAD requested before the first is used, and b is formed in a
// register and never stored.  Nothing is contracted into a fused multiply-add; no atomics, no LDS in the walk, no scratch.
// Included after kernels_baseline.h.
#pragma once
#include "kernels_baseline.h"

namespace cae {

constexpr int RS_SCAN = 0, RS_PACK = 1, RS_RESTORE = 2;

struct RsArgs {
    const unsigned char* low;               // [n_case] planes of h_in x w_in
    long long low_stride;                   // elements between cases
    int lk;                                 // CAE_ELEM_* kind
    int h_in, w_in, h_out, w_out;
    double sy, sx;                          // (double)n_in / (double)n_out, divided on the host
    int n_band, n_strip;
    long long items;                        // n_case * n_band * n_strip
    const float* in;                        // [n_case][h_out][w_out]: the target (scan, pack) or the scores (restore)
    double rmin, span;
    int enable;
    const int* dst_rows;                    // pack: NULL or [n_case]
    float* y;                               // pack: [n_case][h_out][w_out]
    double* p;                              // restore: [n_case][h_out][w_out]
    double* part;                           // scan: [items][3]
};

__device__ __forceinline__ double rs_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ double rs_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// One wave per item = (case, band, strip); four items per workgroup, no barrier, no LDS
template <int MODE, int OP>
__global__ void __launch_bounds__(256) k_residual(const RsArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.items) return;
    const int per_case = a.n_band * a.n_strip;
    const long long c = item / per_case;
    const int rem = (int)(item - c * per_case);
    const int band = rem / a.n_strip, strip = rem - band * a.n_strip;
    const int W = a.w_out;
    const long long plane = (long long)a.h_out * W;
    const int ox = strip * BL_COLS + lane;
    const bool col_ok = ox < W;
    const int oxc = col_ok ? ox : W - 1;
    const int y0 = band * BL_ROWS, y1 = min(y0 + BL_ROWS, a.h_out);
    const float* ic = a.in + c * plane;
    const long long row_out = OP == RS_PACK && a.dst_rows ? (long long)a.dst_rows[c] : c;
    const bool enable = a.enable != 0;
    const double rmin = a.rmin, span = a.span;

    BlWalk<MODE> walk;
    walk.start(a.low + c * a.low_stride * (a.lk < 2 ? 4 : 8), a.lk, oxc, y0, lane, a.h_in, a.w_in, a.h_out, a.sy, a.sx);
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    int k = 0;

    for (int yb = y0; yb < y1; yb += BL_AHEAD) {
        float q[BL_AHEAD];
#pragma unroll
        for (int d = 0; d < BL_AHEAD; d++) q[d] = ic[(long long)min(yb + d, y1 - 1) * W + oxc];     // always inside the band
#pragma unroll
        for (int d = 0; d < BL_AHEAD; d++) {
            const int oy = yb + d;
            if (oy < y1) {                  // the same in every lane
                bool bad;
                const double b = walk.row(oy - y0, bad);
                const double v = (double)q[d];
                const long long e = (long long)oy * W + ox;
                if constexpr (OP == RS_RESTORE) {
                    double p;
                    if (enable) {
                        const double u = v * span;
                        const double w = rmin + u;
                        p = b + w;
                    } else {
                        p = b + v;
                    }
                    if (col_ok) a.p[row_out * plane + e] = bad || v != v ? __longlong_as_double(0x7ff8000000000000ll) : p;
                } else {
                    const double r = v - b;
                    const bool ok = !bad && ss_finite(r);
                    if constexpr (OP == RS_SCAN) {
                        if (col_ok) {
                            if (ok) {
                                mn = r < mn ? r : mn;
                                mx = r > mx ? r : mx;
                            } else {
                                k += 1;
                            }
                        }
                    } else {
                        float y;
                        if (enable) {
                            const double u = r - rmin;
                            y = span == 0.0 ? 0.f : (float)(u / span);
                        } else {
                            y = (float)r;
                        }
                        if (col_ok) a.y[row_out * plane + e] = ok ? y : __uint_as_float(0x7fc00000u);
                    }
                }
            }
        }
    }
    if constexpr (OP == RS_SCAN) {
        const double t0 = ss_wave_sum((double)k), t1 = rs_wave_min(mn), t2 = rs_wave_max(mx);   // (k <= 4096: exact)
        if (lane == 0) {
            double* o = a.part + 3 * item;
            o[0] = t0, o[1] = t1, o[2] = t2;
        }
    }
}

// out[0..2] = {S k, min, max} over the n_part partials; one workgroup.  The counts are integers far below 2^53 and min and
// max do not depend on the order, so neither does the result.
__global__ void __launch_bounds__(256) k_residual_fold(const double* __restrict__ part, long long n_part, double* __restrict__ out) {
    __shared__ double red[4][3];
    double k = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    for (long long i = threadIdx.x; i < n_part; i += 256) {
        k += part[3 * i];
        mn = part[3 * i + 1] < mn ? part[3 * i + 1] : mn;
        mx = part[3 * i + 2] > mx ? part[3 * i + 2] : mx;
    }
    k = ss_wave_sum(k), mn = rs_wave_min(mn), mx = rs_wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = k, red[threadIdx.x >> 6][1] = mn, red[threadIdx.x >> 6][2] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            k += red[w][0];
            mn = red[w][1] < mn ? red[w][1] : mn;
            mx = red[w][2] > mx ? red[w][2] : mx;
        }
        out[0] = k, out[1] = mn, out[2] = mx;
    }
}

}  // namespace cae
