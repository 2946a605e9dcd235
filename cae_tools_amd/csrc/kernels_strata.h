// kernels_strata.h - device only: the error sums of prediction against target conditioned on a third field, the
// stratifier (include/cae_hip.h, cae_strata_sums).  Two kinds of launch:
//   k_strata_sums<KP, KA>  (element kinds of p and of a; the stratifier's kind is a run-time argument: it is small and
//                          read through the caches)
//                          a wave takes items = (case, chunk of ST_CHUNK consecutive target pixels) and walks a chunk 64
//                          pixels at a time, ST_AHEAD steps requested before the first is used.  A lane carries (y, x) of its
//                          pixel along the flat walk - 64 pixels on are (64 / w) rows and (64 mod w) columns, one
//                          conditional row more: a division per lane and chunk, none per pixel - and forms the source row
//                          and column of the stratifier by the CAE_INTERP_NEAREST rule of kernels_baseline.h (bl_axis<0>).
//                          The stratum of a finite value is the number of edges at or below it, counted in fp64 against
//                          the edges in the kernel arguments (a uniform loop: scalar loads).  The wave then loops over the
//                          distinct strata among its lanes, as k_joint_hist does over bin pairs: the first live lane's
//                          stratum is read (v_readlane), the lanes that hold it are balloted, their eight addends are
//                          summed over the whole wave in the fixed DPP tree of device_common.h with zeros in the other
//                          lanes, and lane 63, where the tree ends, adds the sums and the two counts plainly into the
//                          wave's own LDS tables [n_strata][8] fp64 and [n_strata][2] 64-bit integers (one lane, its own
//                          table: no bank conflict, no atomic).  A coherent field costs one or two rounds per 64 pixels,
//                          per-pixel noise over 64 strata up to 64.  At the end the workgroup adds its waves' counts to the
//                          outputs (64-bit integer atomics: exact in any order) and stores its waves' sums, added in wave
//                          order, plainly as the partial of the workgroup
//   k_strata_fold          the partials added in workgroup order by one lane per (stratum, sum)
// No floating-point atomics.  The cut into workgroups and waves depends on (n_case, h, w) alone and the order of a wave's
// rounds on the data alone, so the same arguments give the same bits from run to run.  Nothing is contracted into a fused
// multiply-add: every addend is the host restatement's (tests/strata_ref.py).
// Uses cm_load1 of case_elem.h, ss_raw, ss_value and ss_finite of kernels_ssim.h, bl_axis of kernels_baseline.h and
// wave_sum_lane63 of device_common.h, so it is included after them.
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int ST_WAVES = 4;                 // waves of a workgroup: tables of their own each
constexpr int ST_MAX_EDGE = 63;
constexpr int ST_MAX_STRATA = ST_MAX_EDGE + 1;
constexpr int ST_SUMS = 8;                  // {S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2, S a'p'}
constexpr int ST_CHUNK = 4096;              // target pixels of an item
constexpr int ST_AHEAD = 4;                 // steps of 64 pixels requested together
constexpr int ST_MAX_GROUPS = 1024;         // workgroups of a call
constexpr long long ST_MAX_SIDE = 1ll << 30;

struct StArgs {
    const unsigned char* p;
    const unsigned char* a;
    const unsigned char* s;
    long long p_stride, a_stride, s_stride; // elements between cases
    int sk;                                 // CAE_ELEM_* kind of the stratifier
    int h, w, sh, sw;
    int q64, r64;                           // 64 / w and 64 mod w: 64 pixels on along the flat walk
    int n_edge;
    double sy, sx;                          // (double)sh / (double)h and (double)sw / (double)w, divided on the host
    long long plane, nch, items;            // h * w; chunks of a case; n_case * nch
    unsigned long long* counts;             // [n_strata] members, [n_strata] pairs, unclassified: zeroed before the launch
    double* part;                           // [workgroups][n_strata][8]
    double edges[ST_MAX_EDGE];
    double shift_a[ST_MAX_STRATA], shift_p[ST_MAX_STRATA];
};

// 64 pixels, one per lane (`in`: the lane has one); every lane of the wave calls it.  cw: the wave's sums [n_strata][8];
// nw: its counts [n_strata][2] {members, pairs}; unc: the lane's pixels without a stratum
__device__ __forceinline__ void st_pixels(const StArgs& g, int lane, bool in, double sv, double pv, double av, double* cw,
                                          unsigned long long* nw, unsigned long long& unc) {
#pragma clang fp contract(off)
    const bool cls = in && ss_finite(sv);
    unc += in && !cls ? 1ull : 0ull;
    unsigned long long live = __ballot(cls);
    if (live == 0) return;                  // the same in every lane
    const bool pair = cls && ss_finite(pv) && ss_finite(av);
    int k = 0;                              // the edges at or below the value; -0.0 compares as 0.0
    for (int j = 0; j < g.n_edge; j++) k += g.edges[j] <= sv ? 1 : 0;
    if (!pair) pv = av = 0.0;
    const double d = pv - av, ad = fabs(d), dd = __dmul_rn(d, d);
    while (live) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
        const int k0 = __builtin_amdgcn_readlane(k, first);
        const bool m = cls && k == k0;      // a lane cleared earlier held another stratum
        const unsigned long long mm = __ballot(m);
        const bool pm = m && pair;
        const unsigned long long pp = __ballot(pm);
        if (pp) {                           // the same in every lane
            const double a1 = av - g.shift_a[k0], p1 = pv - g.shift_p[k0];
            const double x5 = __dmul_rn(a1, a1), x6 = __dmul_rn(p1, p1), x7 = __dmul_rn(a1, p1);
            // lane 63 asks for the row of the wave's table before the sums are formed: the tree hides the LDS latency
            double* row = cw + ST_SUMS * k0;
            double o[ST_SUMS];
            if (lane == 63) {
#pragma unroll
                for (int q = 0; q < ST_SUMS; q++) o[q] = row[q];
            }
            // the sums land in lane 63 (device_common.h: the tree travels by DPP, not through the LDS crossbar)
            const double s0 = wave_sum_lane63(pm ? d : 0.0), s1 = wave_sum_lane63(pm ? ad : 0.0), s2 = wave_sum_lane63(pm ? dd : 0.0),
                         s3 = wave_sum_lane63(pm ? a1 : 0.0), s4 = wave_sum_lane63(pm ? p1 : 0.0), s5 = wave_sum_lane63(pm ? x5 : 0.0),
                         s6 = wave_sum_lane63(pm ? x6 : 0.0), s7 = wave_sum_lane63(pm ? x7 : 0.0);
            if (lane == 63) {
                row[0] = o[0] + s0, row[1] = o[1] + s1, row[2] = o[2] + s2, row[3] = o[3] + s3;
                row[4] = o[4] + s4, row[5] = o[5] + s5, row[6] = o[6] + s6, row[7] = o[7] + s7;
            }
        }
        if (lane == 63) {
            nw[2 * k0] += (unsigned long long)__popcll(mm);
            nw[2 * k0 + 1] += (unsigned long long)__popcll(pp);
        }
        // the next round's lane-63 loads follow these stores in program order (the LDS serves a wave in order): the
        // compiler must neither keep a row in registers across rounds nor move an access across this point
        asm volatile("" ::: "memory");
        live &= ~mm;
    }
}

// LDS: [ST_WAVES][64][8] doubles and [ST_WAVES][64][2] 64-bit counts - 20 KiB
template <int KP, int KA>
__global__ void __launch_bounds__(64 * ST_WAVES) k_strata_sums(const StArgs g) {
#pragma clang fp contract(off)
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    __shared__ double st_sums[ST_WAVES][ST_MAX_STRATA * ST_SUMS];
    __shared__ unsigned long long st_cnt[ST_WAVES][ST_MAX_STRATA * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_strata = g.n_edge + 1;
    for (int e = lane; e < n_strata * ST_SUMS; e += 64) st_sums[wave][e] = 0.0;
    for (int e = lane; e < n_strata * 2; e += 64) st_cnt[wave][e] = 0ull;
    __syncthreads();
    double* cw = st_sums[wave];
    unsigned long long* nw = st_cnt[wave];
    unsigned long long unc = 0ull;
    const int es = g.sk < 2 ? 4 : 8;
    // a wave takes `per` consecutive items: whole cases where it can
    const long long n_wave = (long long)gridDim.x * ST_WAVES, per = (g.items + n_wave - 1) / n_wave;
    const long long item0 = ((long long)blockIdx.x * ST_WAVES + wave) * per;
    const long long item1 = item0 + per < g.items ? item0 + per : g.items;
    for (long long item = item0; item < item1; item++) {
        const long long cs = item / g.nch, ch = item - cs * g.nch;
        const unsigned char* pc = g.p + cs * g.p_stride * EP;
        const unsigned char* ac = g.a + cs * g.a_stride * EA;
        const unsigned char* sc = g.s + cs * g.s_stride * es;
        const long long e0 = ch * ST_CHUNK, e1 = e0 + ST_CHUNK < g.plane ? e0 + ST_CHUNK : g.plane;
        // (y, x) of the lane's pixel, carried along the walk; past the plane's end y passes h and is clamped where it is used
        const long long yy = (e0 + lane) / g.w;
        int y = (int)yy, x = (int)(e0 + lane - yy * g.w);
        for (long long eb = e0; eb < e1; eb += 64 * ST_AHEAD) {
            unsigned long long sq[ST_AHEAD];
            double vp[ST_AHEAD], va[ST_AHEAD];
            bool in[ST_AHEAD];
#pragma unroll
            for (int u = 0; u < ST_AHEAD; u++) {
                const long long e = eb + u * 64 + lane;
                in[u] = e < e1;
                const long long ec = in[u] ? e : e1 - 1;        // always a pixel of the chunk: no predicate on a load
                int iy, ix;
                double one;
                bl_axis<0>(y < g.h ? y : g.h - 1, g.sy, g.sh, &iy, &one);
                bl_axis<0>(x, g.sx, g.sw, &ix, &one);
                sq[u] = ss_raw(sc, (long long)iy * g.sw + ix, g.sk);
                vp[u] = cm_load1<KP>(pc, ec);
                va[u] = cm_load1<KA>(ac, ec);
                x += g.r64, y += g.q64;
                if (x >= g.w) x -= g.w, y += 1;
            }
#pragma unroll
            for (int u = 0; u < ST_AHEAD; u++)
                if (eb + u * 64 < e1)           // the same in every lane
                    st_pixels(g, lane, in[u], ss_value(sq[u], g.sk), vp[u], va[u], cw, nw, unc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) unc += __shfl_xor(unc, o, 64);
    if (lane == 0 && unc) atomicAdd(&g.counts[2 * n_strata], unc);
    __syncthreads();
    for (int e = tid; e < n_strata * 2; e += 64 * ST_WAVES) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int w = 0; w < ST_WAVES; w++) v += st_cnt[w][e];
        if (v) atomicAdd(&g.counts[(e & 1) * n_strata + (e >> 1)], v);
    }
    double* dst = g.part + (long long)blockIdx.x * (n_strata * ST_SUMS);
    for (int e = tid; e < n_strata * ST_SUMS; e += 64 * ST_WAVES) {
        double s = st_sums[0][e];
#pragma unroll
        for (int w = 1; w < ST_WAVES; w++) s += st_sums[w][e];
        dst[e] = s;
    }
}

// sums[e] = the partials of the workgroups added in workgroup order; one lane per e = (stratum, sum).  W: the waves whose
// sums a partial holds (a template, so that the kernel is emitted with k_strata_sums at the end of the code object)
template <int W>
__global__ void __launch_bounds__(256) k_strata_fold(const double* __restrict__ part, int n_group, int per, double* __restrict__ sums) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double s = 0.0;
    for (int b = 0; b < n_group; b++) s += part[(long long)b * per + e];
    sums[e] = s;
}

}  // namespace cae
