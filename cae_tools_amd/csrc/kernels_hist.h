// kernels_hist.h - device only: the joint histogram of prediction against target over value, its two fine marginal
// histograms and the per-bin error sums (include/cae_hip.h, cae_joint_hist).  Two kinds of launch:
//   k_joint_hist<KP, KA>   (element kinds of p and of a)
//                          a workgroup of JH_WAVES waves keeps in LDS one joint table [n_bin][n_bin] and the two fine
//                          marginal tables [2][n_bin * sub] of 32-bit counts, shared by its waves, and per wave a table
//                          [2][n_bin][4] of fp64 sums.  A wave takes k_case_measures' items - (case, 4096-element chunk),
//                          16-byte loads from the case's first common 16-byte phase, head and tail element by element in
//                          chunk 0 - and bins 64 pixels at a time.  Real data sits on the diagonal: the 64 pixels fall
//                          into a handful of bins, so the wave does not add lane by lane.  It loops over the distinct
//                          coarse pairs (ia, ip) present: the first live lane's pair is read (v_readlane), the lanes that
//                          hold it are balloted, their number goes to the joint table with one integer LDS add, their five
//                          addends {d, |d|, d*d, a - lo, p - lo} are summed over the whole wave in the fixed DPP tree of
//                          device_common.h with zeros in the other lanes, and lane 63, where the tree ends, adds the sums
//                          plainly into the wave's own table under ia and under ip (it asks for the two rows before the
//                          tree, which hides the LDS latency); those lanes are then cleared.  A constant field costs one round
//                          per 64 pixels, noise up to 64.  The fine marginals take one add of the round's count where the
//                          round's lanes share the fine bin, else one integer LDS add per lane.
//                          At the end the workgroup adds its counts that are not zero to the outputs (64-bit integer
//                          atomics: exact in any order) and stores its waves' sums, added in wave order, plainly as the
//                          partial of the workgroup
//   k_joint_hist_fold<W>   the partials added in workgroup order by one lane per (key, bin, sum)
// No floating-point atomics.  The cut into workgroups and waves depends on (n_case, plane) alone and the order of a wave's
// rounds on the data alone, so the same arguments give the same bits from run to run.  Nothing is contracted into a fused
// multiply-add: the bin of a value is the host restatement's (tests/distribution_ref.py).
// Uses the element loads of case_elem.h (cm_load1, cm_load4), ss_finite of kernels_ssim.h and wave_sum_lane63 of
// device_common.h, so it is included after them.
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int JH_WAVES = 4;                 // waves of a workgroup: a table of sums each
constexpr int JH_MAX_BIN = 128;
constexpr int JH_MAX_SUB = 32;
constexpr int JH_MAX_GROUPS = 1024;         // workgroups of a call: n_case * plane < 2^40 keeps a workgroup's share below 2^31
constexpr int JH_SHIFT = 20;                // f / sub = (f * magic) >> 20 for f < 4096, magic = ceil(2^20 / sub), sub <= 32

struct JhArgs {
    const unsigned char* p;
    const unsigned char* a;
    long long p_stride, a_stride, plane;    // elements
    int nch;                                // chunks of a case
    long long items;                        // n_case * nch
    double lo, hi, scale;                   // scale = (double)n_fine / (hi - lo), divided on the host
    int n_bin, sub, n_fine;
    unsigned magic;
    unsigned long long* joint;              // [n_bin][n_bin], zeroed before the launch
    unsigned long long* marg;               // [2][n_fine], likewise
    unsigned long long* outside;            // [4], likewise
    double* part;                           // [workgroups][2][n_bin][4]
};

// the fine bin of a finite value: the comparison in fp64 before the conversion
__device__ __forceinline__ int jh_fine(double v, double lo, double scale, int n_fine) {
#pragma clang fp contract(off)
    const double t = __dmul_rn(__dsub_rn(v, lo), scale);
    return t < 0.0 ? 0 : (t >= (double)n_fine ? n_fine - 1 : (int)t);
}

// 64 pixels, one per lane (`in`: the lane has one); every lane of the wave calls it
__device__ __forceinline__ void jh_pixels(const JhArgs& g, int lane, bool in, double pv, double av, unsigned* joint, unsigned* marg,
                                          double* cw, unsigned (&out)[4]) {
#pragma clang fp contract(off)
    const bool pair = in && ss_finite(pv) && ss_finite(av);
    unsigned long long live = __ballot(pair);
    if (live == 0) return;                  // the same in every lane
    if (!pair) pv = av = g.lo;
    const int fa = jh_fine(av, g.lo, g.scale, g.n_fine), fp = jh_fine(pv, g.lo, g.scale, g.n_fine);
    const int ia = (int)(((unsigned)fa * g.magic) >> JH_SHIFT), ip = (int)(((unsigned)fp * g.magic) >> JH_SHIFT);
    const int key = ia * g.n_bin + ip;
    out[0] += pair && av < g.lo ? 1u : 0u;
    out[1] += pair && av > g.hi ? 1u : 0u;
    out[2] += pair && pv < g.lo ? 1u : 0u;
    out[3] += pair && pv > g.hi ? 1u : 0u;
    const double d = pv - av, ad = fabs(d), dd = __dmul_rn(d, d), xa = av - g.lo, xp = pv - g.lo;
    while (live) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
        const int k = __builtin_amdgcn_readlane(key, first);
        const bool m = pair && key == k;    // a lane cleared earlier held another pair
        const unsigned long long mm = __ballot(m);
        const unsigned cnt = (unsigned)__popcll(mm);
        const int ka = __builtin_amdgcn_readlane(ia, first), kp = __builtin_amdgcn_readlane(ip, first);
        const int fa0 = __builtin_amdgcn_readlane(fa, first), fp0 = __builtin_amdgcn_readlane(fp, first);
        // lane 63 asks for the two rows of the wave's table before the sums are formed: the tree hides the LDS latency
        double* ca = cw + 4 * ka;
        double* cp = cw + 4 * (g.n_bin + kp);
        double o[8];
        if (lane == 63) {
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = ca[q], o[4 + q] = cp[q];
        }
        // the sums land in lane 63 (device_common.h: the tree travels by DPP, not through the LDS crossbar)
        const double s0 = wave_sum_lane63(m ? d : 0.0), s1 = wave_sum_lane63(m ? ad : 0.0), s2 = wave_sum_lane63(m ? dd : 0.0),
                     s3 = wave_sum_lane63(m ? xa : 0.0), s4 = wave_sum_lane63(m ? xp : 0.0);
        // the fine marginals: one add of the round's count where its lanes share the fine bin, else an integer add per lane
        // (one add per distinct fine bin, found as the rounds are, was measured slower: 57.6 against 44.8 ms on smooth data)
        const bool one_a = __ballot(m && fa == fa0) == mm, one_p = __ballot(m && fp == fp0) == mm;
        if (!one_a && m) atomicAdd(&marg[fa], 1u);
        if (!one_p && m) atomicAdd(&marg[g.n_fine + fp], 1u);
        if (lane == 63) {
            atomicAdd(&joint[k], cnt);
            if (one_a) atomicAdd(&marg[fa0], cnt);
            if (one_p) atomicAdd(&marg[g.n_fine + fp0], cnt);
            ca[0] = o[0] + s0, ca[1] = o[1] + s1, ca[2] = o[2] + s2, ca[3] = o[3] + s3;
            cp[0] = o[4] + s0, cp[1] = o[5] + s1, cp[2] = o[6] + s2, cp[3] = o[7] + s4;
        }
        // the next round's lane-63 loads follow these stores in program order (the LDS serves a wave in order): the
        // compiler must neither keep a row in registers across rounds nor move an access across this point
        asm volatile("" ::: "memory");
        live &= ~mm;
    }
}

// LDS: [JH_WAVES][2][n_bin][4] doubles, [n_bin][n_bin] and [2][n_fine] 32-bit counts - 128 KiB at 128 bins of 32
template <int KP, int KA>
__global__ void __launch_bounds__(64 * JH_WAVES) k_joint_hist(const JhArgs g) {
    constexpr int EP = CmElem<KP>::bytes, EA = CmElem<KA>::bytes;
    extern __shared__ __attribute__((aligned(16))) unsigned char jh_lds[];
    const int per_wave = 2 * g.n_bin * 4;
    double* cond = reinterpret_cast<double*>(jh_lds);
    unsigned* joint = reinterpret_cast<unsigned*>(cond + JH_WAVES * per_wave);
    unsigned* marg = joint + g.n_bin * g.n_bin;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_count = g.n_bin * g.n_bin + 2 * g.n_fine;
    for (int e = tid; e < JH_WAVES * per_wave; e += 64 * JH_WAVES) cond[e] = 0.0;
    for (int e = tid; e < n_count; e += 64 * JH_WAVES) joint[e] = 0u;       // the marginals follow the joint table
    __syncthreads();
    double* cw = cond + wave * per_wave;
    unsigned out[4] = {0u, 0u, 0u, 0u};
    // a wave takes `per` consecutive items: whole cases where it can.  (Dealt with the stride of the grid, a multiple of the
    // chunks of a case at the benchmark size, a wave met the same rows of every case, and the waves that got the rows with
    // the most bins set the time.)
    const long long n_wave = (long long)gridDim.x * JH_WAVES, per = (g.items + n_wave - 1) / n_wave;
    const long long item0 = ((long long)blockIdx.x * JH_WAVES + wave) * per;
    const long long item1 = item0 + per < g.items ? item0 + per : g.items;
    for (long long item = item0; item < item1; item++) {
        const long long cs = item / g.nch;
        const int ch = (int)(item - cs * g.nch);
        const unsigned char* pc = g.p + cs * g.p_stride * EP;
        const unsigned char* ac = g.a + cs * g.a_stride * EA;
        int h = -1;
        for (int t = 3; t >= 0; t--)
            if ((((uintptr_t)(pc + t * EP) | (uintptr_t)(ac + t * EA)) & 15) == 0) h = t;
        const bool vec = h >= 0;
        const long long head = vec ? (h < g.plane ? h : g.plane) : 0;
        const long long groups = (g.plane - head) >> 2;
        const long long tail0 = head + (groups << 2);
        if (ch == 0 && (head > 0 || tail0 < g.plane)) {     // head in lanes 0 .. 2, tail in lanes 4 .. 6
            const bool in = lane < head || (lane >= 4 && lane - 4 < g.plane - tail0);
            const long long e = lane < head ? lane : tail0 + lane - 4;
            const double pv = in ? cm_load1<KP>(pc, e) : 0.0, av = in ? cm_load1<KA>(ac, e) : 0.0;
            jh_pixels(g, lane, in, pv, av, joint, marg, cw, out);
        }
        const long long g0 = (long long)ch * CM_GROUPS;
        const long long g1 = g0 + CM_GROUPS < groups ? g0 + CM_GROUPS : groups;
        for (long long gb = g0; gb < g1; gb += 2 * 64) {    // two groups in flight per lane
            double vp[2][4], va[2][4];
            bool in[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const long long gi = gb + u * 64 + lane;
                in[u] = gi < g1;
                const long long gc = in[u] ? gi : g1 - 1;   // always a group of the chunk: no predicate on a load
                cm_load4<KP>(pc, head + (gc << 2), vec, vp[u]);
                cm_load4<KA>(ac, head + (gc << 2), vec, va[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) jh_pixels(g, lane, in[u], vp[u][j], va[u][j], joint, marg, cw, out);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        unsigned v = out[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && v) atomicAdd(&g.outside[k], (unsigned long long)v);
    }
    __syncthreads();
    for (int e = tid; e < n_count; e += 64 * JH_WAVES) {
        const unsigned v = joint[e];
        if (v) atomicAdd(e < g.n_bin * g.n_bin ? &g.joint[e] : &g.marg[e - g.n_bin * g.n_bin], (unsigned long long)v);
    }
    double* dst = g.part + (long long)blockIdx.x * per_wave;
    for (int e = tid; e < per_wave; e += 64 * JH_WAVES) {
        double s = cond[e];
#pragma unroll
        for (int w = 1; w < JH_WAVES; w++) s += cond[w * per_wave + e];
        dst[e] = s;
    }
}

// cond[e] = the partials of the workgroups added in workgroup order; one lane per e = (key, bin, sum).  W: the waves whose
// sums a partial holds (a template, so that the kernel is emitted with k_joint_hist at the end of the code object)
template <int W>
__global__ void __launch_bounds__(256) k_joint_hist_fold(const double* __restrict__ part, int n_group, int per, double* __restrict__ cond) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double s = 0.0;
    for (int b = 0; b < n_group; b++) s += part[(long long)b * per + e];
    cond[e] = s;
}

}  // namespace cae
