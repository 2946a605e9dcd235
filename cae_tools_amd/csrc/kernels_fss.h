// kernels_fss.h - device only: the neighbourhood sums of the Fractions Skill Score of prediction against target
// (include/cae_hip.h, cae_case_fss).  Two launches:
//   k_fss_bits<KP, KA>  (element kinds of p and of a) one streaming pass over the operands for all thresholds.  A wave
//                       takes consecutive words of 64 pixels of a row, FS_AHEAD of them requested before the first is used,
//                       and carries (case, row, word) along the walk: a division per wave, none per word.  It forms `bad`
//                       (the pixel is no pair) and per threshold the event of p and of a among the pairs - fp64 compares,
//                       the last floating-point operation of the call - and lane 0 stores each __ballot word plainly into
//                       planes[case][1 + 2 T][h][ceil(w / 64)]: bit x & 63 of word x >> 6 is pixel x, bits at or beyond w
//                       are zero.  Plane 0 is bad, plane 1 + 2 t the events of p, plane 2 + 2 t those of a.  Every word of
//                       the planes is written, so the workspace needs no clearing.
//   k_fss_windows       a wave takes items = (case, threshold, block of 64 consecutive x0, segment of seg_len window rows)
//                       and loops over the widths outside the walk.  A lane owns x0 = 64 * block + lane and walks y0 down
//                       the segment.  A row's words from the block's first on are the same for the whole wave (uniform
//                       addresses: scalar loads) - two up to n = 63, three up to n = 129, since the block starts on a
//                       word.  The lane shifts its n bits down dword by dword with the 32-bit funnel shift, masks the
//                       last dword and takes __popc: the row counts of eP, eA and bad.  The window counts are running
//                       sums: the first n rows of the segment are added, then each step adds the row that enters and
//                       subtracts the row that leaves (counted again from its words, which lie in the caches: no row
//                       count is kept).  Six 64-bit integer accumulators per lane, folded over the wave with integer adds
//                       and added to the zeroed output with 64-bit integer atomics: exact in any order, so the cut into
//                       items never shows.
// No floating-point arithmetic after the compares of k_fss_bits, no LDS.
// Uses cm_load1 of case_elem.h and ss_finite of kernels_ssim.h, so it is included after that.
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int FS_WAVES = 4;                 // waves of a workgroup
constexpr int FS_AHEAD = 4;                 // words of 64 pixels requested together
constexpr int FS_MAX_THR = 8;
constexpr int FS_MAX_WIDTH = 8;
constexpr int FS_MAX_N = 129;               // the widest neighbourhood: 63 + 129 bits from a word's start are three words
// steps of the walk unrolled: left to itself the compiler unrolls until the scalar loads of many steps fill 256 VGPRs with
// spilled SGPRs (one wave per SIMD); 2 measured 2.5 % faster than 1
#ifndef FS_UNROLL
#define FS_UNROLL 2
#endif
constexpr int FS_SUMS = 6;                  // {windows, S cM, S cO, S cM^2, S cO^2, S cM cO}
constexpr long long FS_MAX_SIDE = 16384;
constexpr long long FS_MAX_CASES = 1ll << 40;   // of a call: every index stays far inside 64 bits
constexpr int FS_BITS_GROUPS = 4096;        // workgroups of k_fss_bits at most
constexpr int FS_WIN_GROUPS = 1 << 20;      // of k_fss_windows

struct FsBitsArgs {
    const unsigned char* p;
    const unsigned char* a;
    long long p_stride, a_stride;           // elements between cases
    int h, w, wpr;                          // wpr: words of a row, ceil(w / 64)
    int n_thr;
    long long words;                        // n_case * h * wpr
    unsigned long long* planes;             // [n_case][1 + 2 n_thr][h][wpr]
    double thr[FS_MAX_THR];
    int below[FS_MAX_THR];                  // 0: the event is v >= thr; 1: v < thr
};

struct FsWinArgs {                          // the planes and the zeroed sums [n_case][n_thr][n_width][6] are arguments of their own
    int h, w, wpr;
    int n_thr, n_width;
    int gap_rule;                           // 0: a window is counted iff it holds no bad pixel; 1: iff it holds a pair
    int seg_len, n_seg;                     // window rows of a segment; segments of a plane, ceil(h / seg_len)
    long long items;                        // n_case * n_thr * n_seg * wpr
    int width[FS_MAX_WIDTH];
};

template <int KP, int KA>
__global__ void __launch_bounds__(64 * FS_WAVES) k_fss_bits(const FsBitsArgs g) {
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // a wave takes `per` consecutive words
    const long long n_wave = (long long)gridDim.x * FS_WAVES, per = (g.words + n_wave - 1) / n_wave;
    const long long i0 = ((long long)blockIdx.x * FS_WAVES + wave) * per;
    const long long i1 = i0 + per < g.words ? i0 + per : g.words;
    if (i0 >= i1) return;
    const long long row0 = i0 / g.wpr;
    long long cs = row0 / g.h;
    int y = (int)(row0 - cs * g.h), xw = (int)(i0 - row0 * g.wpr);
    const int n_plane = 1 + 2 * g.n_thr;
    const long long hw = (long long)g.h * g.wpr;
    for (long long ib = i0; ib < i1; ib += FS_AHEAD) {
        double vp[FS_AHEAD], va[FS_AHEAD];
        bool in[FS_AHEAD];
        long long dst[FS_AHEAD];
#pragma unroll
        for (int u = 0; u < FS_AHEAD; u++) {
            vp[u] = va[u] = 0.0, in[u] = false, dst[u] = 0;
            if (ib + u < i1) {                  // the same in every lane
                const int x = xw * 64 + lane;
                in[u] = x < g.w;
                const long long e = (long long)y * g.w + (in[u] ? x : g.w - 1);   // always a pixel of the row: no predicate on a load
                vp[u] = cm_load1<KP>(g.p + cs * g.p_stride * EP, e);
                va[u] = cm_load1<KA>(g.a + cs * g.a_stride * EA, e);
                dst[u] = (cs * n_plane * g.h + y) * g.wpr + xw;
                if (++xw == g.wpr) {
                    xw = 0;
                    if (++y == g.h) y = 0, cs++;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FS_AHEAD; u++) {
            if (ib + u >= i1) break;            // the same in every lane
            const bool pair = in[u] && ss_finite(vp[u]) && ss_finite(va[u]);
            unsigned long long* out = g.planes + dst[u];
            const unsigned long long bad = __ballot(in[u] && !pair);
            if (lane == 0) out[0] = bad;
            for (int t = 0; t < g.n_thr; t++) {
                const double thr = g.thr[t];    // -0.0 compares as 0.0
                const bool below = g.below[t] != 0;
                const unsigned long long wp = __ballot(pair && (below ? vp[u] < thr : vp[u] >= thr));
                const unsigned long long wa = __ballot(pair && (below ? va[u] < thr : va[u] >= thr));
                if (lane == 0) out[(1 + 2 * t) * hw] = wp, out[(2 + 2 * t) * hw] = wa;
            }
        }
    }
}

// the set bits among bits s .. s + n - 1 of the row whose 64-bit words start at r, bit 0 of r[0] lowest, with s = 32 * up + sh
// the lane's first bit (0 .. 63).  NR = ceil(n / 32) result dwords: dword j of the lane's bits is the 32-bit funnel shift
// (v_alignbit_b32) of source dwords j + up and j + up + 1 by sh, the last one masked to the n - 32 (NR - 1) bits of `ml`.
// The source dwords come from two words (63 + 63 bits at most for NR <= 2) or three; a dword beyond them is zero - it only
// reaches bits that the mask drops.  `last`: the index of the row's last word from r on; a word beyond it is never looked at
// by a lane with a window, so the last one stands in for it.  r and last are the same in every lane: scalar loads
template <int NR>
__device__ __forceinline__ int fs_count(const unsigned long long* __restrict__ r, int last, unsigned sh, bool up, unsigned ml) {
    constexpr int NS = NR <= 2 ? 2 : 3;
    unsigned D[2 * NS + 1];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const unsigned long long W = r[k < last ? k : last];
        D[2 * k] = (unsigned)W, D[2 * k + 1] = (unsigned)(W >> 32);
    }
    D[2 * NS] = 0u;
    unsigned sel[NR + 1];
#pragma unroll
    for (int j = 0; j <= NR; j++) sel[j] = up ? D[j + 1] : D[j];
    int c = 0;
#pragma unroll
    for (int j = 0; j < NR; j++) {
        unsigned v = __builtin_amdgcn_alignbit(sel[j + 1], sel[j], sh);
        if (j == NR - 1) v &= ml;
        c += __popc(v);
    }
    return c;
}

// one window into the lane's sums; a window that is not counted adds nothing
__device__ __forceinline__ void fs_add(bool counted, int cm, int co, unsigned long long (&acc)[FS_SUMS]) {
    const unsigned um = counted ? (unsigned)cm : 0u, uo = counted ? (unsigned)co : 0u;
    acc[0] += counted ? 1ull : 0ull;
    acc[1] += um;
    acc[2] += uo;
    acc[3] += (unsigned long long)um * um;
    acc[4] += (unsigned long long)uo * uo;
    acc[5] += (unsigned long long)um * uo;
}

// one width over one item: the lane's windows x0 = 64 * block + lane, y0 = y_begin .. y_end - 1, added to acc.  pb, pp, pa:
// row 0 of the planes bad, eP and eA at the block's first word; cap: a window is counted iff its bad pixels are fewer
template <int NR>
__device__ __forceinline__ void fs_walk(const unsigned long long* __restrict__ pb, const unsigned long long* __restrict__ pp,
                                        const unsigned long long* __restrict__ pa, int wpr, int last, int lane, int n, int y_begin,
                                        int y_end, bool active, int cap, unsigned long long (&acc)[FS_SUMS]) {
    const unsigned ml = (1u << (n - 32 * (NR - 1))) - 1u, sh = (unsigned)lane & 31u;
    const bool up = lane >= 32;
    int cm = 0, co = 0, cb = 0;
#pragma unroll 1
    for (int r = 0; r < n; r++) {
        const long long o = (long long)(y_begin + r) * wpr;
        cb += fs_count<NR>(pb + o, last, sh, up, ml);
        cm += fs_count<NR>(pp + o, last, sh, up, ml);
        co += fs_count<NR>(pa + o, last, sh, up, ml);
    }
    fs_add(active && cb < cap, cm, co, acc);
#pragma unroll FS_UNROLL
    for (int y0 = y_begin + 1; y0 < y_end; y0++) {
        const long long o0 = (long long)(y0 - 1) * wpr, o1 = (long long)(y0 + n - 1) * wpr;    // leaves, enters
        cb += fs_count<NR>(pb + o1, last, sh, up, ml) - fs_count<NR>(pb + o0, last, sh, up, ml);
        cm += fs_count<NR>(pp + o1, last, sh, up, ml) - fs_count<NR>(pp + o0, last, sh, up, ml);
        co += fs_count<NR>(pa + o1, last, sh, up, ml) - fs_count<NR>(pa + o0, last, sh, up, ml);
        fs_add(active && cb < cap, cm, co, acc);
    }
}

// W: the waves of a workgroup (a template, so that the kernel is emitted with k_fss_bits at the end of the code object).
// planes and sums are arguments of their own, restrict-qualified: the atomics on sums then clobber no load of the planes,
// and the uniform loads of the walk stay scalar
template <int W>
__global__ void __launch_bounds__(64 * W) k_fss_windows(const unsigned long long* __restrict__ planes,
                                                        unsigned long long* __restrict__ sums, const FsWinArgs g) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long hw = (long long)g.h * g.wpr;
    const int n_plane = 1 + 2 * g.n_thr;
    for (long long item = (long long)blockIdx.x * W + wave; item < g.items; item += (long long)gridDim.x * W) {
        // the block of x0 runs fastest, then the threshold, the segment, the case
        long long q = item / g.wpr;
        const int b = (int)(item - q * g.wpr);
        const int t = (int)(q % g.n_thr);
        q /= g.n_thr;
        const int seg = (int)(q % g.n_seg);
        const long long cs = q / g.n_seg;
        const unsigned long long* pb = planes + cs * n_plane * hw + b;
        const unsigned long long* pp = pb + (1 + 2 * t) * hw;
        const unsigned long long* pa = pb + (2 + 2 * t) * hw;
        const int last = g.wpr - 1 - b, x0 = 64 * b + lane, y_begin = seg * g.seg_len;
        for (int s = 0; s < g.n_width; s++) {
            const int n = g.width[s];
            // windows of this width in the item: every condition is the same in every lane
            if (n > g.h || n > g.w || y_begin > g.h - n || 64 * b > g.w - n) continue;
            const int y_end = y_begin + g.seg_len < g.h - n + 1 ? y_begin + g.seg_len : g.h - n + 1;
            const bool active = x0 <= g.w - n;
            const int cap = g.gap_rule ? n * n : 1;
            unsigned long long acc[FS_SUMS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
            switch ((n + 31) / 32) {        // the result dwords of a lane
            case 1: fs_walk<1>(pb, pp, pa, g.wpr, last, lane, n, y_begin, y_end, active, cap, acc); break;
            case 2: fs_walk<2>(pb, pp, pa, g.wpr, last, lane, n, y_begin, y_end, active, cap, acc); break;
            case 3: fs_walk<3>(pb, pp, pa, g.wpr, last, lane, n, y_begin, y_end, active, cap, acc); break;
            case 4: fs_walk<4>(pb, pp, pa, g.wpr, last, lane, n, y_begin, y_end, active, cap, acc); break;
            default: fs_walk<5>(pb, pp, pa, g.wpr, last, lane, n, y_begin, y_end, active, cap, acc); break;
            }
            unsigned long long* dst = sums + ((cs * g.n_thr + t) * g.n_width + s) * FS_SUMS;
#pragma unroll
            for (int k = 0; k < FS_SUMS; k++) {
                unsigned long long v = acc[k];
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0 && v) atomicAdd(&dst[k], v);
            }
        }
    }
}

}  // namespace cae
