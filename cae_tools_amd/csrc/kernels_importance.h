// kernels_importance.h - permutation importance of the model's input variables (include/cae_hip.h, cae_normalise_pack_gather
// and cae_case_importance).
//
// k_normalise_pack_gather: k_normalise_pack with the source row read from a table, dst[i] = norm(src[row[i]]); a row index
// outside 0 .. n_src - 1 is never turned into an address, the destination row gets quiet NaNs instead.
//
// k_case_importance: the unperturbed scores, the perturbed scores and the target of a pixel are read once and feed both
// reductions.  The plane is cut into tiles of IM_TILE = 64 consecutive pixels, lane l of a wave owns pixel tile * 64 + l.
//   per case:  the wave sums each of the eight addends of its tile in the fixed DPP tree (wave_sum_lane63; the three counts
//              travel as one integer, 7 bits each) and lane 63 stores them to part[case][tile][8]; k_importance_fold adds
//              a case's tiles: lane j of a wave takes tiles j, j + 64, ... in ascending order, then the same tree.  Tile
//              size, both trees and the lane order depend on the plane alone, so a case's sums do not depend on the other
//              cases of the call, on n_case, on the alignment of the operands or on MAP.
//   per pixel: (MAP) the wave owns its tile for the whole call: a lane loads its pixel's three running sums from map_dev,
//              adds the cases 0 .. n_case - 1 in that order with plain adds and stores them back.  Cases cut into
//              consecutive calls therefore give the bits of one call.
// Work items: MAP: one wave per tile, walking all cases in batches of IM_AHEAD, the loads of the next batch in flight while
// one is used; otherwise one wave per (tile, run of
// IM_RUN cases), so that a call without a map covers the device however few pixels a case has.  No LDS, no atomics; every
// subtraction, product and sum is rounded on its own, nothing is contracted into a fused multiply-add.
#pragma once
#include "case_elem.h"

namespace cae {

// (A template, as k_importance_fold is, so that it is emitted where stateless_host.h instantiates it, at the end of the code
// object: the kernels of the training step keep their places.)
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_normalise_pack_gather(const float* __restrict__ src, long long n_src, long long total,
                                                                int c_src, long long hw, float* __restrict__ dst, int c_dst,
                                                                int c_off, float vmin, float range, int enable,
                                                                const int* __restrict__ row) {
    const long long per = (long long)c_src * hw;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * BLOCK) {
        const long long d = i / per, r = i - d * per;
        const long long s = (long long)row[d];
        float v = __uint_as_float(0x7fc00000u);
        if (s >= 0 && s < n_src) {
            v = src[s * per + r];
            if (enable) v = (range == 0.f) ? 0.f : __fdiv_rn(__fsub_rn(v, vmin), range);
        }
        dst[(d * c_dst + c_off) * hw + r] = v;
    }
}

constexpr int IM_TILE = 64;             // pixels per tile: one per lane
constexpr int IM_SUMS = 8;
constexpr int IM_AHEAD = 16;            // with a map: cases per batch of loads, the next batch in flight while one is used
constexpr int IM_RUN = 8;               // cases per work item without a map
constexpr int IM_WAVES = 4;             // waves per 256-thread workgroup

struct ImArgs {
    const float* base;
    const float* pert;
    const unsigned char* a;
    long long base_stride, pert_stride, a_stride;       // elements from one case to the next
    long long n_case, plane, n_tile, items;
    double vmin, range;
    double* part;                                       // [n_case][n_tile][IM_SUMS]
    double* map;                                        // [3][plane], MAP only
};

__device__ __forceinline__ int im_wave_sum_lane63(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);
    return v;
}

__device__ __forceinline__ bool im_finite(double v) { return (v - v) == 0.0; }

// One pixel of one case: the eight addends into the tile's tree, and (MAP) the lane's running sums.  inside: the lane has a
// pixel of a case that exists; live: the case exists (wave-uniform).
template <bool MAP>
__device__ __forceinline__ void im_case(const ImArgs& s, bool inside, bool live, float yb, float yp, double av, long long cs,
                                        long long tile, int lane, double m[3]) {
#pragma clang fp contract(off)
    const double p0 = cm_denorm(s.vmin, (double)yb, s.range);
    const double p1 = cm_denorm(s.vmin, (double)yp, s.range);
    const bool pair = inside && im_finite(av) && im_finite(p0) && im_finite(p1);
    double q1 = 0.0, q0 = 0.0, a1 = 0.0, a0 = 0.0, dd = 0.0;
    int cnt = 0;
    if (pair) {
        const double e0 = __dsub_rn(p0, av), e1 = __dsub_rn(p1, av), d = __dsub_rn(p1, p0);
        q0 = __dmul_rn(e0, e0);
        q1 = __dmul_rn(e1, e1);
        a0 = fabs(e0);
        a1 = fabs(e1);
        dd = __dmul_rn(d, d);
        cnt = 1 | (q1 > q0 ? 1 << 7 : 0) | (q1 < q0 ? 1 << 14 : 0);
        if (MAP) {
            m[0] = __dadd_rn(m[0], 1.0);
            m[1] = __dadd_rn(m[1], q1);
            m[2] = __dadd_rn(m[2], q0);
        }
    }
    q1 = wave_sum_lane63(q1);
    q0 = wave_sum_lane63(q0);
    a1 = wave_sum_lane63(a1);
    a0 = wave_sum_lane63(a0);
    dd = wave_sum_lane63(dd);
    cnt = im_wave_sum_lane63(cnt);
    if (lane == 63 && live) {
        double2* out = reinterpret_cast<double2*>(s.part + (cs * s.n_tile + tile) * IM_SUMS);
        out[0] = make_double2((double)(cnt & 127), q1);
        out[1] = make_double2(q0, a1);
        out[2] = make_double2(a0, dd);
        out[3] = make_double2((double)((cnt >> 7) & 127), (double)(cnt >> 14));
    }
}

// the loads of A consecutive cases of one pixel.  Every address is formed from a clamped case and a clamped pixel, so all of
// them are valid and the loads need no predicate: what a lane beyond the plane or a slot beyond the last case reads is
// never used.
template <int A>
struct ImBatch {
    float yb[A], yp[A];
    double av[A];
};

template <int KA, int A>
__device__ __forceinline__ void im_load(const ImArgs& s, long long cs, long long c1, long long pl, ImBatch<A>& b) {
    constexpr int EA = CmElem<KA>::bytes;
#pragma unroll
    for (int u = 0; u < A; u++) {
        const long long cc = cs + u < c1 ? cs + u : c1 - 1;
        b.yb[u] = s.base[cc * s.base_stride + pl];
        b.yp[u] = s.pert[cc * s.pert_stride + pl];
        b.av[u] = cm_load1<KA>(s.a + cc * s.a_stride * EA, pl);
    }
}

template <int KA, bool MAP>
__global__ void __launch_bounds__(256) k_case_importance(const ImArgs s) {
    constexpr int A = MAP ? IM_AHEAD : IM_RUN;
    const int lane = threadIdx.x & 63;
    for (long long item = (long long)blockIdx.x * IM_WAVES + (threadIdx.x >> 6); item < s.items;
         item += (long long)gridDim.x * IM_WAVES) {
        long long tile, c0, c1;
        if (MAP) {
            tile = item, c0 = 0, c1 = s.n_case;
        } else {
            const long long run = item / s.n_tile;
            tile = item - run * s.n_tile;
            c0 = run * IM_RUN;
            c1 = c0 + IM_RUN < s.n_case ? c0 + IM_RUN : s.n_case;
        }
        const long long px = tile * IM_TILE + lane;
        const bool inside = px < s.plane;
        const long long pl = inside ? px : s.plane - 1;
        double m[3] = {0.0, 0.0, 0.0};
        if (MAP && inside) {
            m[0] = s.map[px];
            m[1] = s.map[s.plane + px];
            m[2] = s.map[2 * s.plane + px];
        }
        ImBatch<A> cur, nxt;
        im_load<KA, A>(s, c0, c1, pl, cur);
        for (long long cs = c0; cs < c1; cs += A) {
            if (MAP) im_load<KA, A>(s, cs + A, c1, pl, nxt);        // the next batch is asked for before this one is used
#pragma unroll
            for (int u = 0; u < A; u++)
                im_case<MAP>(s, inside && cs + u < c1, cs + u < c1, cur.yb[u], cur.yp[u], cur.av[u], cs + u, tile, lane, m);
            if (MAP) cur = nxt;
        }
        if (MAP && inside) {
            s.map[px] = m[0];
            s.map[s.plane + px] = m[1];
            s.map[2 * s.plane + px] = m[2];
        }
    }
}

// sums[case][k] = the case's tiles added: lane j takes tiles j, j + 64, ... in ascending order, then the DPP tree.  One wave
// per case.
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_importance_fold(const double* __restrict__ part, long long n_case, long long n_tile,
                                                         double* __restrict__ sums) {
    const int lane = threadIdx.x & 63;
    for (long long cs = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); cs < n_case; cs += (long long)gridDim.x * WAVES) {
        double acc[IM_SUMS];
#pragma unroll
        for (int k = 0; k < IM_SUMS; k++) acc[k] = 0.0;
        const double2* src = reinterpret_cast<const double2*>(part + cs * n_tile * IM_SUMS);
        for (long long t = lane; t < n_tile; t += 64) {
#pragma unroll
            for (int k = 0; k < IM_SUMS / 2; k++) {
                const double2 v = src[t * (IM_SUMS / 2) + k];
                acc[2 * k] = __dadd_rn(acc[2 * k], v.x);
                acc[2 * k + 1] = __dadd_rn(acc[2 * k + 1], v.y);
            }
        }
#pragma unroll
        for (int k = 0; k < IM_SUMS; k++) acc[k] = wave_sum_lane63(acc[k]);
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < IM_SUMS; k++) sums[cs * IM_SUMS + k] = acc[k];
        }
    }
}

}  // namespace cae
