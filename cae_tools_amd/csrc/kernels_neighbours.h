// kernels_neighbours.h - brute-force K nearest neighbours between two sets of fp32 rows, exact in fp64
// (include/cae_hip.h, cae_case_neighbours).
//
// d2(i, j) = S_d ((double)q[i][d] - (double)r[j][d])^2 in the DIFFERENCE form: the conversions are exact, the subtraction is
// one correctly rounded fp64 operation, square and sum are one fma per d, and every accumulator walks d = 0 .. D - 1 in
// ascending order.  So the bits of d2 depend on the two rows and D alone, identical rows give exactly +0.0, and channels
// that two rows share bit for bit cancel exactly (the expansion |q|^2 + |r|^2 - 2 q.r, the only form fp64 MFMA could serve,
// loses that).  Candidates are ordered by (bits of d2, global reference index): a total order, so the K smallest are unique
// whatever the tiling.
//
// k_nb_valid: a row's validity (all D values finite), one wave per row, once per row and call.
// k_nb_tile: a workgroup of 256 lanes owns NB_T queries and walks a run of reference tiles of NB_T rows.  Slices of NB_DK
//   features of both sides are staged in LDS as fp32, rows NB_PITCH dwords apart; lane (ty, tx) owns the 4 x 4 pairs
//   (ty + 16 i, tx + 16 j) and holds their fp64 accumulators in registers: per 4 features 8 ds_read_b128 (the 16 tx of a
//   wave hit 16 distinct 16-byte slots, the 4 ty broadcast), 32 conversions and 64 subtract + fma pairs.  The next slice's
//   global loads are in flight while the current one is consumed.  A ragged tail of D and rows beyond the sets are staged as
//   zeros on both sides: a zero difference adds exactly nothing.  The finished tile goes to LDS (over the staging area), a
//   pair that is no candidate - reference invalid or beyond the set, or the query's own row - as +inf; then one lane per
//   query filters its NB_T candidates against its current K-th best and inserts the few that pass into its sorted list in
//   LDS ([k][query], the bank is the query).  After the run the lists go to the workspace as the partial lists of this split.
// k_nb_merge: one lane per query folds the splits' partial lists, and under merge the lists the outputs already hold, with
//   the same insertion, and writes dist2, index and count.
// No atomics, no scratch; the same arguments give the same bits.  The three kernels are templates over their block size, as
// k_quantile_fill is, so that they are emitted where stateless_host.h instantiates them, at the end of the code object, and no
// kernel of the training step moves.
#pragma once
#include "device_common.h"

namespace cae {

constexpr int NB_T = 64;            // queries and references per tile
constexpr int NB_DK = 32;           // features per staged slice
constexpr int NB_PITCH = NB_DK + 4; // dwords from one staged row to the next: 16-byte aligned, and 36 * tx mod 64 names 16 distinct slots
constexpr int NB_TP = NB_T + 1;     // doubles from one query's finished pairs to the next
constexpr int NB_MAX_K = 32;
constexpr int NB_ROWS = NB_T / 8;   // staged rows per lane and side: 256 lanes cover 8 rows of NB_DK features at a time
constexpr unsigned long long NB_INF = 0x7ff0000000000000ull;
constexpr int NB_TILE_BYTES = NB_T * NB_TP * 8;         // the finished tile, which also covers the 2 * NB_T * NB_PITCH * 4 of staging

struct NbArgs {
    const float* q;
    const float* r;
    long long n_q, q_stride, n_r, r_stride, dim;
    long long ref_base, self_offset;            // self_offset < 0: no exclusion
    int k, merge, n_split, tiles_per_split;
    const int* q_ok;                            // [n_q], [n_r]: 1 where all dim values are finite
    const int* r_ok;
    unsigned long long* part_d;                 // [n_split][n_q][k]
    int* part_i;
    double* dist2;                              // [n_q][k]
    int* index;
    int* count;                                 // [n_q]
};

// ---- validity ---------------------------------------------------------------------------------------------------------

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_nb_valid(const float* x, long long n, long long stride, long long dim, int* ok) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (BLOCK / 64);
    for (long long row = (long long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); row < n; row += waves) {
        const float* p = x + row * stride;
        bool bad = false;
        for (long long d = lane; d < dim; d += 64) bad |= !(fabsf(p[d]) < __builtin_huge_valf());
        const bool any = __any(bad);
        if (lane == 0) ok[row] = any ? 0 : 1;
    }
}

// ---- the sorted list of one query in LDS: entries [k][NB_T], lane `col` owns column col ----------------------------------

// (d, i) before (e, j) in the order of the candidates; the index compares unsigned, so the -1 of an unused slot is last
__device__ __forceinline__ bool nb_before(unsigned long long d, int i, unsigned long long e, int j) {
    return d < e || (d == e && (unsigned)i < (unsigned)j);
}

// insert (d, i), which is before the list's last entry, and return through (td, ti) the new last entry
__device__ __forceinline__ void nb_insert(unsigned long long* ld, int* li, int col, int k, unsigned long long d, int i,
                                          unsigned long long& td, int& ti) {
    int at = k - 1;
    while (at > 0) {
        const unsigned long long e = ld[(at - 1) * NB_T + col];
        const int j = li[(at - 1) * NB_T + col];
        if (!nb_before(d, i, e, j)) break;
        ld[at * NB_T + col] = e;
        li[at * NB_T + col] = j;
        at--;
    }
    ld[at * NB_T + col] = d;
    li[at * NB_T + col] = i;
    td = ld[(k - 1) * NB_T + col];
    ti = li[(k - 1) * NB_T + col];
}

// ---- distances and the partial lists -------------------------------------------------------------------------------------

struct NbStage {
    float q[NB_ROWS], r[NB_ROWS];
};

// the slice of features d0 .. d0 + NB_DK - 1 of the tile's rows into registers: lane t brings feature d0 + (t & 31) of rows
// (t >> 5) + 8 u; what lies beyond the set or beyond dim is zero and is not read
__device__ __forceinline__ void nb_fetch(const NbArgs& a, long long q0, long long r0, long long d0, int t, NbStage& s) {
    const long long d = d0 + (t & 31);
    const int row = t >> 5;
#pragma unroll
    for (int u = 0; u < NB_ROWS; u++) {
        const long long qi = q0 + row + 8 * u, ri = r0 + row + 8 * u;
        s.q[u] = d < a.dim && qi < a.n_q ? a.q[qi * a.q_stride + d] : 0.0f;
        s.r[u] = d < a.dim && ri < a.n_r ? a.r[ri * a.r_stride + d] : 0.0f;
    }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_nb_tile(const NbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nb_lds[];
    float* sq = reinterpret_cast<float*>(nb_lds);                   // [NB_T][NB_PITCH]
    float* sr = sq + NB_T * NB_PITCH;
    unsigned long long* tile = reinterpret_cast<unsigned long long*>(nb_lds);       // [NB_T queries][NB_TP], over sq and sr
    unsigned long long* ld = reinterpret_cast<unsigned long long*>(nb_lds + NB_TILE_BYTES);     // [k][NB_T]
    int* li = reinterpret_cast<int*>(ld + a.k * NB_T);

    static_assert(BLOCK == 256, "16 x 16 lanes of 4 x 4 pairs cover the tile");
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long long q0 = (long long)blockIdx.x * NB_T;
    const int split = blockIdx.y;
    const long long n_tile = (a.n_r + NB_T - 1) / NB_T;
    const long long tile0 = (long long)split * a.tiles_per_split;
    const long long tile1 = tile0 + a.tiles_per_split < n_tile ? tile0 + a.tiles_per_split : n_tile;

    // the list of lane t < NB_T's query, empty; its last entry in registers
    unsigned long long td = NB_INF;
    int ti = -1;
    const bool owner = t < NB_T && q0 + t < a.n_q && a.q_ok[q0 + t] != 0;
    if (t < NB_T)
        for (int e = 0; e < a.k; e++) ld[e * NB_T + t] = NB_INF, li[e * NB_T + t] = -1;

    const long long n_slice = (a.dim + NB_DK - 1) / NB_DK;
    for (long long rt = tile0; rt < tile1; rt++) {
        const long long r0 = rt * NB_T;
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = 0.0;

        NbStage st;
        nb_fetch(a, q0, r0, 0, t, st);
        for (long long sl = 0; sl < n_slice; sl++) {
            __syncthreads();        // the slice before, or the tile before, has been read
#pragma unroll
            for (int u = 0; u < NB_ROWS; u++) {
                sq[((t >> 5) + 8 * u) * NB_PITCH + (t & 31)] = st.q[u];
                sr[((t >> 5) + 8 * u) * NB_PITCH + (t & 31)] = st.r[u];
            }
            __syncthreads();
            if (sl + 1 < n_slice) nb_fetch(a, q0, r0, (sl + 1) * NB_DK, t, st);
#pragma unroll 1
            for (int d4 = 0; d4 < NB_DK; d4 += 4) {
                float4 qv[4], rv[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    qv[i] = *reinterpret_cast<const float4*>(sq + (ty + 16 * i) * NB_PITCH + d4);
                    rv[i] = *reinterpret_cast<const float4*>(sr + (tx + 16 * i) * NB_PITCH + d4);
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    double qd[4], rd[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        qd[i] = (double)(c == 0 ? qv[i].x : c == 1 ? qv[i].y : c == 2 ? qv[i].z : qv[i].w);
                        rd[i] = (double)(c == 0 ? rv[i].x : c == 1 ? rv[i].y : c == 2 ? rv[i].z : rv[i].w);
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const double df = __dsub_rn(qd[i], rd[j]);
                            acc[i][j] = __fma_rn(df, df, acc[i][j]);
                        }
                }
            }
        }
        __syncthreads();            // the last slice has been read: the tile goes over the staging area
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long rj = r0 + tx + 16 * j;
            const bool r_in = rj < a.n_r && a.r_ok[rj < a.n_r ? rj : 0] != 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const long long qi = q0 + ty + 16 * i;
                const bool self = a.self_offset >= 0 && a.ref_base + rj == a.self_offset + qi;
                tile[(ty + 16 * i) * NB_TP + tx + 16 * j] =
                    r_in && !self ? (unsigned long long)__double_as_longlong(acc[i][j]) : NB_INF;
            }
        }
        __syncthreads();
        if (owner) {
            const long long n_here = a.n_r - r0 < NB_T ? a.n_r - r0 : NB_T;
            for (int j = 0; j < (int)n_here; j++) {
                const unsigned long long d = tile[t * NB_TP + j];
                const int gi = (int)(a.ref_base + r0 + j);
                if (d < NB_INF && nb_before(d, gi, td, ti)) nb_insert(ld, li, t, a.k, d, gi, td, ti);
            }
        }
    }
    __syncthreads();
    if (t < NB_T && q0 + t < a.n_q) {
        const long long base = ((long long)split * a.n_q + q0 + t) * a.k;
        for (int e = 0; e < a.k; e++) a.part_d[base + e] = ld[e * NB_T + t], a.part_i[base + e] = li[e * NB_T + t];
    }
}

// ---- the fold of the splits, and of what the outputs hold already --------------------------------------------------------------

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_nb_merge(const NbArgs a) {
    __shared__ unsigned long long ld[NB_MAX_K * NB_T];
    __shared__ int li[NB_MAX_K * NB_T];
    static_assert(BLOCK == NB_T, "one lane per query of the tile");
    const int t = threadIdx.x;
    const long long qi = (long long)blockIdx.x * NB_T + t;
    if (qi >= a.n_q) return;            // no barrier below: every lane works on its own column
    unsigned long long* od = reinterpret_cast<unsigned long long*>(a.dist2) + qi * a.k;
    int* oi = a.index + qi * a.k;
    if (a.q_ok[qi] == 0) {
        for (int e = 0; e < a.k; e++) od[e] = NB_INF, oi[e] = -1;
        a.count[qi] = -1;
        return;
    }
    for (int e = 0; e < a.k; e++) ld[e * NB_T + t] = NB_INF, li[e * NB_T + t] = -1;
    unsigned long long td = NB_INF;
    int ti = -1;
    if (a.merge) {
        for (int e = 0; e < a.k; e++) {
            const unsigned long long d = od[e];
            const int gi = oi[e];
            if (gi >= 0 && d < NB_INF && nb_before(d, gi, td, ti)) nb_insert(ld, li, t, a.k, d, gi, td, ti);
        }
    }
    for (int s = 0; s < a.n_split; s++) {
        const long long base = ((long long)s * a.n_q + qi) * a.k;
        for (int e = 0; e < a.k; e++) {
            const unsigned long long d = a.part_d[base + e];
            const int gi = a.part_i[base + e];
            if (gi < 0 || !nb_before(d, gi, td, ti)) break;     // a partial list ascends: nothing after this entry passes
            nb_insert(ld, li, t, a.k, d, gi, td, ti);
        }
    }
    int n = 0;
    for (int e = 0; e < a.k; e++) {
        const int gi = li[e * NB_T + t];
        od[e] = ld[e * NB_T + t];
        oi[e] = gi;
        n += gi >= 0 ? 1 : 0;
    }
    a.count[qi] = n;
}

}  // namespace cae
