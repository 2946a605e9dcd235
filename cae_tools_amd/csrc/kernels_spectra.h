// kernels_spectra.h - device only: the power spectra of prediction against target (include/cae_hip.h, cae_case_spectra;
// DESIGN.md section 9).  Per case the windowed, mean-free planes p', a' and d' = (p - a)' of channel 0 are transformed by
// a direct two-dimensional DFT in fp64 - two small matrix products per band of kx columns, plain fp64 FMAs - and the four
// products w|P|^2, w|A|^2, w Re(P conj A), w|D|^2 of every mode are added into the radial bin the caller's table names.
// No floating-point atomics anywhere: a bin of a (case, band) is summed by one lane in a fixed order, the bands of a case
// by the fold in band order.  Uses the element loads of case_elem.h (cm_load1).
#pragma once
#include "case_elem.h"

namespace cae {

constexpr int SP_THREADS = 256;         // one row (row transform) or one ky (column transform) per lane and pass
constexpr int SP_MAX_SIDE = 2048;       // h and w
constexpr int SP_MAX_NB = 4;            // kx columns per band
constexpr int SP_TILE_ELEMS = 2048;     // h * nb never exceeds it: 3 fields * 16 bytes * 2048 = 96 KiB of LDS

// element e of a case in a run-time kind (the branch is wave-uniform; a load feeds 6 * nb FMAs)
__device__ __forceinline__ double sp_load(const unsigned char* c, long long e, int kind) {
    switch (kind) {
    case 0: return cm_load1<0>(c, e);
    case 1: return cm_load1<1>(c, e);
    case 2: return cm_load1<2>(c, e);
    default: return cm_load1<3>(c, e);
    }
}

__device__ __forceinline__ bool sp_finite(double v) { return v - v == 0.0; }

// tw[m] = {cos, sin}(2 pi m / N) for m < N, N = h and N = w: one table behind the other
__global__ void __launch_bounds__(256) k_spectra_twiddle(double2* __restrict__ twh, int h, double2* __restrict__ tww, int w) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < h) {
        double s, c;
        sincospi(2.0 * (double)m / (double)h, &s, &c);
        twh[m] = make_double2(c, s);
    }
    if (m < w) {
        double s, c;
        sincospi(2.0 * (double)m / (double)w, &s, &c);
        tww[m] = make_double2(c, s);
    }
}

// s + c is the running sum: the rounding error of every addition to s (Knuth's two-sum, exact in fp64) is kept in c
struct SpSum {
    double s, c;
};

__device__ __forceinline__ void sp_add(SpSum& acc, double x) {
    const double t = acc.s + x;
    const double bp = t - acc.s;
    acc.c += (acc.s - (t - bp)) + (x - bp);
    acc.s = t;
}

// One workgroup per case: mu[c] = {mean p, mean a, mean d, finite flag} and counted[c].  A mean's own rounding is not small
// beside the spectrum of a field that varies by a hundredth of its level, so the sums are compensated: lane t adds the
// elements t, t + 256, .. with the error of every addition kept, a fixed tree over the 256 lanes does the same, and s + c
// is rounded once - the exactly rounded sum but for ties that the error term itself misses.  A fixed order: every band of
// the case reads the same bits.
__global__ void __launch_bounds__(SP_THREADS) k_spectra_mean(const unsigned char* __restrict__ p, int pk, long long p_stride,
                                                             const unsigned char* __restrict__ a, int ak, long long a_stride,
                                                             long long plane, double* __restrict__ mu, int* __restrict__ counted) {
    __shared__ double red[7][SP_THREADS];
    const int t = threadIdx.x;
    const long long c = blockIdx.x;
    const unsigned char* pc = p + c * p_stride * (pk < 2 ? 4 : 8);
    const unsigned char* ac = a + c * a_stride * (ak < 2 ? 4 : 8);
    SpSum acc[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    double bad = 0.0;
    for (long long e = t; e < plane; e += SP_THREADS) {
        const double vp = sp_load(pc, e, pk), va = sp_load(ac, e, ak);
        if (!sp_finite(vp) || !sp_finite(va)) bad = 1.0;
        sp_add(acc[0], vp);
        sp_add(acc[1], va);
        sp_add(acc[2], vp - va);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) red[2 * k][t] = acc[k].s, red[2 * k + 1][t] = acc[k].c;
    red[6][t] = bad;
    __syncthreads();
    for (int off = SP_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                SpSum m = {red[2 * k][t], red[2 * k + 1][t] + red[2 * k + 1][t + off]};
                sp_add(m, red[2 * k][t + off]);
                red[2 * k][t] = m.s, red[2 * k + 1][t] = m.c;
            }
            red[6][t] += red[6][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool ok = red[6][0] == 0.0;
        const double n = (double)plane;
#pragma unroll
        for (int k = 0; k < 3; k++) mu[4 * c + k] = ok ? (red[2 * k][0] + red[2 * k + 1][0]) / n : 0.0;
        mu[4 * c + 3] = ok ? 1.0 : 0.0;
        counted[c] = ok ? 1 : 0;
    }
}

struct SpArgs {
    const unsigned char* p;
    const unsigned char* a;
    long long p_stride, a_stride;       // elements
    int pk, ak;
    int h, w, wc;                       // wc = w / 2 + 1
    int n_band, n_bin;
    const double* wy;
    const double* wx;
    const int* bin;                     // [h][wc]
    const double2* twh;
    const double2* tww;
    const double* mu;                   // [n_case][4]
    double* part;                       // [n_case][n_band][n_bin][4]
};

// One workgroup per (case, band of NB consecutive kx columns).
//   row transform     lane j takes row j (and j + 256, ..): x'[j][i] for the three fields, formed once per element, times
//                     the NB twiddles of column i (wave-uniform indices, stepped in integers mod w) into the lane's 6 NB
//                     sums; the h x NB complex tile of each field goes to LDS, [j][b][field].
//   column transform  lane t takes ky = 256 r + t in pass r: the tile (broadcast LDS reads) times the lane's own twiddle
//                     (index ky j mod h, stepped in integers), 12 NB sums.
//   bins              the lane's NB modes of a pass are staged in LDS as {w PP, w AA, w RePA, w DD} with their bin; then
//                     lane t owns the bins t, t + 256, .. and adds the staged modes of each in staging order.  The pass's
//                     sum of a bin is stored (pass 0) or added (later passes) to the partial by that one lane.
// LDS: the tile, 48 h NB bytes, and the staging, 36 * 256 NB bytes - behind the tile when h > 256, else in its place
// (one pass: the tile is dead once every lane has its modes).
template <int NB>
__global__ void __launch_bounds__(SP_THREADS) k_case_spectra(const SpArgs s) {
    extern __shared__ double2 sp_lds[];
    const int t = threadIdx.x;
    const long long c = blockIdx.x / s.n_band;
    const int band = (int)(blockIdx.x - c * s.n_band);
    const int h = s.h, w = s.w;
    double* part = s.part + ((c * s.n_band + band) * (long long)s.n_bin) * 4;
    if (s.mu[4 * c + 3] == 0.0) {       // a case that is not counted: zeros from every band
        for (int b = t; b < 4 * s.n_bin; b += SP_THREADS) part[b] = 0.0;
        return;
    }
    const double mp = s.mu[4 * c], ma = s.mu[4 * c + 1], md = s.mu[4 * c + 2];
    const unsigned char* pc = s.p + c * s.p_stride * (s.pk < 2 ? 4 : 8);
    const unsigned char* ac = s.a + c * s.a_stride * (s.ak < 2 ? 4 : 8);
    double2* tile = sp_lds;                                     // [h][NB][3]
    double* stage = reinterpret_cast<double*>(h > SP_THREADS ? sp_lds + (size_t)h * NB * 3 : sp_lds);   // [256 NB][4]
    int* sbin = reinterpret_cast<int*>(stage + SP_THREADS * NB * 4);                                     // [256 NB]

    int step[NB];                       // kx of the band's columns; 0 for a column past the half plane (never binned)
#pragma unroll
    for (int b = 0; b < NB; b++) step[b] = band * NB + b < s.wc ? band * NB + b : 0;

    // ---- row transform
    for (int j = t; j < h; j += SP_THREADS) {
        const double wyj = s.wy[j];
        double acc[NB][6];
        int idx[NB];
#pragma unroll
        for (int b = 0; b < NB; b++) {
            idx[b] = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) acc[b][k] = 0.0;
        }
        const long long e0 = (long long)j * w;
        for (int i = 0; i < w; i++) {
            const double vp = sp_load(pc, e0 + i, s.pk), va = sp_load(ac, e0 + i, s.ak);
            const double wxi = s.wx[i];
            const double xp = (vp - mp) * wyj * wxi, xa = (va - ma) * wyj * wxi, xd = ((vp - va) - md) * wyj * wxi;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const double2 cs = s.tww[idx[b]];               // e^{-i theta} = cos - i sin
                acc[b][0] += xp * cs.x;
                acc[b][1] -= xp * cs.y;
                acc[b][2] += xa * cs.x;
                acc[b][3] -= xa * cs.y;
                acc[b][4] += xd * cs.x;
                acc[b][5] -= xd * cs.y;
                idx[b] += step[b];
                if (idx[b] >= w) idx[b] -= w;
            }
        }
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int f = 0; f < 3; f++) tile[((size_t)j * NB + b) * 3 + f] = make_double2(acc[b][2 * f], acc[b][2 * f + 1]);
    }
    __syncthreads();

    // ---- column transform, a pass of 256 ky at a time, and the bins of each pass
    for (int ky0 = 0; ky0 < h; ky0 += SP_THREADS) {
        const int ky = ky0 + t;
        double x[NB][6];
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int k = 0; k < 6; k++) x[b][k] = 0.0;
        if (ky < h) {
            int idx = 0;
            for (int j = 0; j < h; j++) {
                const double2 cs = s.twh[idx];
                idx += ky;
                if (idx >= h) idx -= h;
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int f = 0; f < 3; f++) {
                        const double2 v = tile[((size_t)j * NB + b) * 3 + f];      // (v.x + i v.y)(c - i s)
                        x[b][2 * f] += v.x * cs.x;
                        x[b][2 * f] += v.y * cs.y;
                        x[b][2 * f + 1] += v.y * cs.x;
                        x[b][2 * f + 1] -= v.x * cs.y;
                    }
            }
        }
        if (h <= SP_THREADS) __syncthreads();       // the staging takes the tile's place: every lane is done reading it
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int kx = band * NB + b;
            int bin = -1;
            if (ky < h && kx < s.wc) {
                bin = s.bin[(long long)ky * s.wc + kx];
                if (bin >= s.n_bin || bin < 0) bin = -1;
            }
            const double wgt = (kx == 0 || 2 * kx == w) ? 1.0 : 2.0;
            const int m = t * NB + b;
            stage[4 * m + 0] = wgt * (x[b][0] * x[b][0] + x[b][1] * x[b][1]);
            stage[4 * m + 1] = wgt * (x[b][2] * x[b][2] + x[b][3] * x[b][3]);
            stage[4 * m + 2] = wgt * (x[b][0] * x[b][2] + x[b][1] * x[b][3]);
            stage[4 * m + 3] = wgt * (x[b][4] * x[b][4] + x[b][5] * x[b][5]);
            sbin[m] = bin;
        }
        __syncthreads();
        for (int bq = t; bq < s.n_bin; bq += SP_THREADS) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int m = 0; m < SP_THREADS * NB; m++) {
                if (sbin[m] == bq) {
                    s0 += stage[4 * m + 0];
                    s1 += stage[4 * m + 1];
                    s2 += stage[4 * m + 2];
                    s3 += stage[4 * m + 3];
                }
            }
            double* o = part + 4 * (long long)bq;
            if (ky0 == 0) o[0] = s0, o[1] = s1, o[2] = s2, o[3] = s3;
            else o[0] += s0, o[1] += s1, o[2] += s2, o[3] += s3;
        }
        __syncthreads();                            // the next pass stages again
    }
}

// sums[c][b][k] = the partials of the case's bands added in band order; one lane per (case, bin, k)
__global__ void __launch_bounds__(256) k_spectra_fold(const double* __restrict__ part, long long n_case, int n_band, int n_bin,
                                                      double* __restrict__ sums) {
    const long long per = 4 * (long long)n_bin;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_case * per; i += (long long)gridDim.x * 256) {
        const long long c = i / per, r = i - c * per;
        double v = 0.0;
        for (int k = 0; k < n_band; k++) v += part[(c * n_band + k) * per + r];
        sums[i] = v;
    }
}

}  // namespace cae
