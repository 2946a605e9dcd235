// kernels_scene.h — the kernels behind cae_scene_gather and cae_scene_blend (include/cae_hip.h): a trained box model applied
// to a whole scene.  The scene (n_t, c, Y, X) is cut into overlapping h x w boxes whose origins along an axis are
// min(k * stride, extent - box): every tile is a full box and the last one is shifted inward.  k_scene_gather cuts and
// normalises the boxes of one variable into the packed batch the model scores; k_scene_blend folds the scored boxes back
// into the float64 scene.  Both are pure traffic and neither touches an engine.  Uses the element loads of
// case_elem.h.
#pragma once
#include "case_elem.h"
#include "device_common.h"

namespace cae {

// ---- gather -------------------------------------------------------------------------------------------------------------
// One thread per element of the variable's part of the batch, in the batch's own order (tile, channel, row, column), so the
// stores of a wave are consecutive; its loads are runs of w consecutive source elements at any alignment (element loads).
// The arithmetic is k_normalise_pack's: the stored value rounded to fp32 first, then (v - vmin) / range in two rounded fp32
// operations, 0 when range == 0, the value itself when `enable` is off.  A value that is not finite as fp32 marks its tile:
// an integer OR into invalid[tile], the same result in any order.
struct SgArgs {
    const unsigned char* src;       // (n_t, c_src, Y, X) as stored
    long long Y, X;
    int c_src, h, w;
    int stride_y, stride_x;         // h - oy, w - ox
    long long n_x;                  // tiles per tile row
    long long t0, ky0, n_ky;        // first time step, first tile row and tile rows of the call
    long long total;                // n_t_call * n_ky * n_x * c_src * h * w
    float* dst;                     // (n_tile, c_dst, h, w)
    int c_dst, c_off;
    float vmin, range;
    int enable;
    int* invalid;                   // (n_tile)
};

template <int K>
__global__ void __launch_bounds__(256) k_scene_gather(const SgArgs a) {
    const unsigned hw = (unsigned)a.h * (unsigned)a.w;
    const unsigned per = (unsigned)a.c_src * hw;            // the host keeps it below 2^31
    const long long plane = a.Y * a.X;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
        const long long tile = i / per;
        const unsigned r = (unsigned)(i - tile * per);
        const unsigned c = r / hw, q = r - c * hw;
        const unsigned by = q / (unsigned)a.w, bx = q - by * (unsigned)a.w;
        const long long trow = tile / a.n_x, kx = tile - trow * a.n_x;
        const long long tt = trow / a.n_ky, ky = a.ky0 + (trow - tt * a.n_ky);
        long long y0 = ky * a.stride_y, x0 = kx * a.stride_x;
        y0 = y0 < a.Y - a.h ? y0 : a.Y - a.h;
        x0 = x0 < a.X - a.w ? x0 : a.X - a.w;
        const long long e = ((a.t0 + tt) * a.c_src + c) * plane + (y0 + by) * a.X + (x0 + bx);
        float v = (float)cm_load1<K>(a.src, e);
        if (!(fabsf(v) < __builtin_huge_valf())) atomicOr(&a.invalid[tile], 1);
        if (a.enable) v = (a.range == 0.f) ? 0.f : __fdiv_rn(__fsub_rn(v, a.vmin), a.range);
        a.dst[(tile * a.c_dst + a.c_off) * (long long)hw + r] = v;
    }
}

// ---- blend --------------------------------------------------------------------------------------------------------------
// A gather per output pixel: every output element is written once and every prediction element is read once.  A thread owns
// one output column and a band of consecutive output rows; what depends on the column alone (the covering tile columns) is
// found once, and the covering tile rows move on with the row, so that no division is left in the row loop.  Where SB_ROWS
// rows in a row lie under the same tile rows the thread blends them together, their loads in flight at once: one dependent
// load per row left the kernel waiting on memory latency.  For a pixel the
// covering tiles are an index range per axis (the inward shift of the last tile makes three and more), visited in ascending
// tile number; the weight w = wy * wx is an integer below 2^29, so w * (double)p is exact and the numerator is a chain of
// plain fp64 adds in that order.  v = num / den, out = vmin + v * range (k_denorm_f64's two rounded operations); no valid
// covering tile: NaN.  A tile's flag and its prediction are loaded side by side (an invalid tile has a prediction too; it is
// dropped, never added).  Element loads only: a tile's origin puts its rows at any 4-byte phase.
// The tile rows come in two runs, [ka0, ka0 + n_ka) carried from the call before and [kb0, kb0 + n_kb) new, so that a scene
// can be blended in pieces of whole tile rows without copying a prediction; a pixel's sum does not see the cut.
struct SbArgs {
    const float* pred_a;            // (n_t, n_ka, n_x, c_out, H, W); may be null with n_ka == 0
    const int* invalid_a;           // (n_t, n_ka, n_x)
    const float* pred_b;            // (n_t, n_kb, n_x, c_out, H, W)
    const int* invalid_b;
    int ka0, n_ka, kb0, n_kb;
    int n_y, n_x;                   // tile rows and columns of the scene
    int n_t, c_out, H, W;
    int SY, SX;                     // tile stride on the output grid
    int LY, LX;                     // last origin on the output grid: (Y - h) * sy, (X - w) * sx
    int RY2, RX2;                   // 2 * oy * sy, 2 * ox * sx: the weight's cap (0: weight 1)
    int Xs;                         // output columns (the host keeps both output sides within 2^30)
    int row0, row1, band;           // output rows of the call, rows per workgroup
    long long out_c_stride, out_t_stride;       // elements between channels and time steps of out
    double vmin, range;
    double* out;                    // element (tt, c, row, x) at tt * out_t_stride + c * out_c_stride + row * Xs + x
    unsigned long long* nan_pixels; // (n_t): += the pixels of channel 0 without a valid covering tile
};

__device__ __forceinline__ int sb_origin(int k, int S, int L) { return k * S < L ? k * S : L; }

// the tiles k of an axis (n tiles, stride S, last origin L, box side B) that cover coordinate r are lo .. hi.  On entry lo and
// hi are at or below their values (those of a smaller r, or sb_first's)
__device__ __forceinline__ void sb_advance(int r, int S, int L, int B, int n, int& lo, int& hi) {
    while (lo < n - 1 && sb_origin(lo, S, L) + B <= r) lo++;
    while (hi < n - 1 && sb_origin(hi + 1, S, L) <= r) hi++;
}

// bounds from below for sb_advance at coordinate r, by division
__device__ __forceinline__ void sb_first(int r, int S, int L, int B, int n, int& lo, int& hi) {
    lo = r >= B ? (r - B) / S + 1 : 0;
    lo = lo < n - 1 ? lo : n - 1;
    hi = r >= L ? n - 1 : r / S;
}

__device__ __forceinline__ int sb_weight(int q, int B, int R2) {
    if (R2 == 0) return 1;
    const int m = q < B - 1 - q ? q : B - 1 - q;
    return 2 * m + 1 < R2 ? 2 * m + 1 : R2;
}

// The tiles of one run of tile rows (k_first .. k_first + n_k - 1 at pred / inv) among the tile rows ky0 .. ky1, added to the
// sums of R consecutive output rows from `row` on of column x.  The R rows' loads of a tile are independent and in flight
// together; each pixel's sum is still its own chain in ascending tile number
template <int R>
__device__ __forceinline__ void sb_run(const SbArgs& a, const float* __restrict__ pred, const int* __restrict__ inv, int k_first,
                                       int n_k, int tt, int c, int x, int row, int ky0, int ky1, int kx0, int kx1, double num[R],
                                       long long den[R]) {
    const long long hw = (long long)a.H * a.W;
    ky0 = ky0 > k_first ? ky0 : k_first;
    ky1 = ky1 < k_first + n_k - 1 ? ky1 : k_first + n_k - 1;
    for (int ky = ky0; ky <= ky1; ky++) {
        const long long trow = (long long)tt * n_k + (ky - k_first);
        const int qy = row - sb_origin(ky, a.SY, a.LY);
        for (int kx = kx0; kx <= kx1; kx++) {
            const int qx = x - sb_origin(kx, a.SX, a.LX);
            const long long tile = trow * a.n_x + kx;
            const int bad = inv[tile];
            const float* src = pred + (tile * a.c_out + c) * hw + (long long)qy * a.W + qx;
            float p[R];
#pragma unroll
            for (int j = 0; j < R; j++) p[j] = src[j * a.W];
            if (bad != 0) continue;
            const int wx = sb_weight(qx, a.W, a.RX2);
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int wgt = sb_weight(qy + j, a.H, a.RY2) * wx;
                num[j] = __dadd_rn(num[j], __dmul_rn((double)wgt, (double)p[j]));
                den[j] += wgt;
            }
        }
    }
}

// R consecutive output rows of column x, all under the tile rows ky0 .. ky1: the carried run, then the new one (the host
// keeps them in that order); returns the pixels without a valid tile
template <int R>
__device__ __forceinline__ unsigned sb_rows(const SbArgs& a, int tt, int c, int x, int row, int ky0, int ky1, int kx0, int kx1,
                                            double* __restrict__ o) {
    double num[R];
    long long den[R];
#pragma unroll
    for (int j = 0; j < R; j++) num[j] = 0.0, den[j] = 0;
    sb_run<R>(a, a.pred_a, a.invalid_a, a.ka0, a.n_ka, tt, c, x, row, ky0, ky1, kx0, kx1, num, den);
    sb_run<R>(a, a.pred_b, a.invalid_b, a.kb0, a.n_kb, tt, c, x, row, ky0, ky1, kx0, kx1, num, den);
    unsigned holes = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const bool hole = den[j] == 0;
        const double v = cm_denorm(a.vmin, __ddiv_rn(num[j], (double)(hole ? 1 : den[j])), a.range);
        holes += hole ? 1u : 0u;
        o[(long long)j * a.Xs] = hole ? __longlong_as_double(0x7ff8000000000000LL) : v;
    }
    return holes;
}

constexpr int SB_ROWS = 4;      // rows a thread blends at a time where they share their tile rows (the host's choice of ROWS)

// grid (column blocks, row bands, n_t * c_out).  A template like k_scene_gather: instantiated kernels are placed after the
// others in the code object, so that adding these moves no kernel of the training step against another
template <int ROWS>
__global__ void __launch_bounds__(256) k_scene_blend(const SbArgs a) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int tt = blockIdx.z / a.c_out, c = blockIdx.z - tt * a.c_out;
    const int r0 = a.row0 + (int)blockIdx.y * a.band;
    const int r1 = r0 + a.band < a.row1 ? r0 + a.band : a.row1;
    unsigned long long holes = 0;       // of channel 0
    if (x < a.Xs) {
        int kx0, kx1, ky0, ky1;
        sb_first(x, a.SX, a.LX, a.W, a.n_x, kx0, kx1);
        sb_advance(x, a.SX, a.LX, a.W, a.n_x, kx0, kx1);
        sb_first(r0, a.SY, a.LY, a.H, a.n_y, ky0, ky1);
        double* o = a.out + tt * a.out_t_stride + c * a.out_c_stride + x;
        int row = r0;
        while (row < r1) {      // (everything that steers this loop is the same in every lane)
            sb_advance(row, a.SY, a.LY, a.H, a.n_y, ky0, ky1);
            int lo = ky0, hi = ky1;
            if (row + ROWS <= r1) sb_advance(row + ROWS - 1, a.SY, a.LY, a.H, a.n_y, lo, hi);
            if (row + ROWS <= r1 && lo == ky0 && hi == ky1) {
                const unsigned n = sb_rows<ROWS>(a, tt, c, x, row, ky0, ky1, kx0, kx1, o + (long long)row * a.Xs);
                holes += c == 0 ? n : 0u;
                row += ROWS;
            } else {
                const unsigned n = sb_rows<1>(a, tt, c, x, row, ky0, ky1, kx0, kx1, o + (long long)row * a.Xs);
                holes += c == 0 ? n : 0u;
                row += 1;
            }
        }
    }
    if (c == 0) {       // (wave-uniform) integers: exact in any order
        for (int off = 32; off > 0; off >>= 1) holes += __shfl_down(holes, off, 64);
        if ((threadIdx.x & 63) == 0 && holes) atomicAdd(&a.nan_pixels[tt], holes);
    }
}

}  // namespace cae
