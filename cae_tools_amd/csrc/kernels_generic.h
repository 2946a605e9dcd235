// kernels_generic.h — shape-generic gfx950 kernels for every op of the ConvAE step, and nothing else: the shared device
// helpers and descriptors are in device_common.h, the kernels that touch no engine (loader, metric sums, evaluator, ensemble
// moments, case pages) in kernels_stateless.h.
//
// These are the fallback / reference-on-device kernels: any kernel size, stride, channel
// count, output_padding.  One thread per output element, BatchNorm + ReLU folded into the
// operand load of the consumer, all cross-block reductions through fp64 atomics.  The
// specialised kernels in kernels_s2.h replace them for the stride-2 layers that carry the
// traffic; both are checked against the CPU oracle.
//
// Every conv-like op is one of three primitives on a "small" map S (B,Cs,Hs,Ws), a "big" map
// L (B,Cl,Hl,Wl) and weights w[cs][cl][ky][kx]  (that IS PyTorch's layout for both
// Conv2d (Cout,Cin,kh,kw) with S = output and ConvTranspose2d (Cin,Cout,kh,kw) with S = input):
//   down : S[cs][y][x]   = sum_cl,ky,kx L[cl][y*s+ky][x*s+kx] * w      (Conv2d fwd, ConvT dgrad)
//   up   : L[cl][Y][X]   = sum_cs,ky,kx S[cs][(Y-ky)/s][(X-kx)/s] * w  (ConvT fwd, Conv2d dgrad)
//   wgrad: dw[cs][cl][ky][kx] = sum_b,y,x S[cs][y][x] * L[cl][y*s+ky][x*s+kx]
#pragma once
#include "device_common.h"

namespace cae {

// ---------------------------------------------------------------------------------------------
// shared epilogue: thread-level part returns the two values to be block-reduced
// ---------------------------------------------------------------------------------------------
// `ypre` (with have_ypre): the caller already holds e.yprev[o] (EPI_MASKSTATS), requested ahead of its main loop
__device__ __forceinline__ void epi_element(const Epi& e, const float4* ce, int c, size_t o, size_t tgt_off,
                                             float acc, double& r1, double& r2, bool have_ypre = false, float ypre = 0.f) {
    switch (e.kind) {
        case EPI_PLAIN:
            e.out[o] = acc;
            break;
        case EPI_STATS:
            e.out[o] = acc;
            r1 = (double)acc;
            r2 = (double)acc * (double)acc;
            break;
        case EPI_MASKSTATS: {
            const float4 k = ce[c];
            const float yv = have_ypre ? ypre : e.yprev[o];
            const float d = yv - k.x;
            const float a = fmaf(d, k.y, k.z);
            const float g = a > 0.f ? acc : 0.f;
            e.out[o] = g;
            r1 = (double)g;
            r2 = (double)g * (double)(d * k.w);
            break;
        }
        case EPI_SIGMSE: {
            const float yh = 1.0f / (1.0f + expf(-acc));
            const float d = yh - e.target[tgt_off];
            const float g = (2.0f * d * e.inv_count) * (yh * (1.0f - yh));
            e.out[o] = g;
            r1 = (double)d * (double)d * (double)e.inv_count;
            r2 = (double)g;
            break;
        }
        case EPI_SIGOUT: {
            const float yh = 1.0f / (1.0f + expf(-acc));
            if (e.yhat) e.yhat[o] = yh;
            if (e.target) {
                const float d = yh - e.target[tgt_off];
                r1 = (double)d * (double)d * (double)e.inv_count;
            }
            break;
        }
    }
}

__device__ __forceinline__ void epi_block(const Epi& e, int c, const StepState* st, double r1, double r2,
                                          double* red, int bx) {
    if (e.kind == EPI_PLAIN) return;
    if (e.kind == EPI_SIGOUT && !e.target) return;
    const double t1 = block_sum(r1, red);
    const double t2 = (e.kind == EPI_SIGOUT) ? 0.0 : block_sum(r2, red);
    if (threadIdx.x == 0) {
        const size_t row = ((size_t)(bx & (kStatShards - 1)) * e.stats_C + c) * 4;
        if (e.kind == EPI_STATS) {
            acc_add<ACC_STAT>(&e.stats[row + 0], t1);
            acc_add<ACC_STAT>(&e.stats[row + 1], t2);
        } else if (e.kind == EPI_MASKSTATS) {
            acc_add<ACC_GRAD>(&e.stats[row + 2], t1);
            acc_add<ACC_GRAD>(&e.stats[row + 3], t2);
        } else if (e.kind == EPI_SIGMSE) {
            acc_add<ACC_GRAD>(&e.losses[(size_t)st->loss_slot * kStatShards + (bx & (kStatShards - 1))], t1);
            acc_add<ACC_GRAD>(&e.bias_acc[c], t2);
        } else {
            acc_add<ACC_GRAD>(&e.losses[(size_t)st->loss_slot * kStatShards + (bx & (kStatShards - 1))], t1);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// down: S[b][cs][y][x] = bias[cs] + sum_cl,ky,kx T(L[b][cl][y*s+ky][x*s+kx]) * w[cs][cl][ky][kx]
// grid (ceil(B*Hs*Ws/256), Cs), block 256, dynamic LDS (Cl + Cs) float4 + 4 doubles
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_down(ConvGeom g, Src big, BnDesc bnb, const float* __restrict__ w,
                                               const float* __restrict__ bias, Epi e, BnDesc bne,
                                               const StepState* __restrict__ st) {
    extern __shared__ double lds_d[];
    double* red = lds_d;
    float4* cb = reinterpret_cast<float4*>(lds_d + 4);
    float4* ce = cb + g.Cl;
    const bool designated = blockIdx.x == 0 && blockIdx.y == 0;
    bn_consts(bnb, cb, designated);
    bn_consts(bne, ce, false, 64);
    // no kernel of the forward/backward pass reads adam_step, so bumping it here cannot race
    if (designated && threadIdx.x == 0 && big.bump_adam) const_cast<StepState*>(st)->adam_step += 1;
    __syncthreads();

    const int cs = blockIdx.y;
    const int hw = g.Hs * g.Ws;
    const int n = g.B * hw;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    double r1 = 0, r2 = 0;
    if (idx < n) {
        const int b = idx / hw, r = idx - b * hw;
        const int y = r / g.Ws, x = r - y * g.Ws;
        const size_t sb = sample_of(big.perm, big.use_cursor, st, b);
        float acc = bias ? bias[cs] : 0.f;
        for (int cl = 0; cl < g.Cl; cl++) {
            const float* wp = w + (size_t)(cs * g.Cl + cl) * g.kh * g.kw;
            const size_t base = (sb * g.Cl + cl) * (size_t)g.Hl * g.Wl;
            const float4 k = bnb.mode ? cb[cl] : make_float4(0, 0, 0, 0);
            for (int ky = 0; ky < g.kh; ky++) {
                const size_t row = base + (size_t)(y * g.s + ky) * g.Wl + (size_t)x * g.s;
                for (int kx = 0; kx < g.kw; kx++) {
                    const float v = big.p[row + kx];
                    const float yr = bnb.mode == BN_BWD ? big.q[row + kx] : 0.f;
                    acc = fmaf(bn_apply(bnb.mode, k, v, yr), wp[ky * g.kw + kx], acc);
                }
            }
        }
        const size_t o = ((size_t)(b * g.Cs + cs) * g.Hs + y) * g.Ws + x;
        epi_element(e, ce, cs, o, 0, acc, r1, r2);
    }
    epi_block(e, cs, st, r1, r2, red, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// up: L[b][cl][Y][X] = bias[cl] + sum_cs sum_{ky = Y mod s (s) , kx = X mod s (s)}
//                                   T(S[b][cs][(Y-ky)/s][(X-kx)/s]) * w[cs][cl][ky][kx]
// grid (ceil(B*Hl*Wl/256), Cl)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void up_body(const ConvGeom& g, const Src& small, const BnDesc& bns, const float* __restrict__ w,
                                        const float* __restrict__ bias, const Epi& e, const BnDesc& bne,
                                        const StepState* __restrict__ st, double* lds_d, const int bx, const int by) {
    double* red = lds_d;
    float4* cs4 = reinterpret_cast<float4*>(lds_d + 4);
    float4* ce = cs4 + g.Cs;
    const bool designated = bx == 0 && by == 0;

    const int cl = by;
    const int hw = g.Hl * g.Wl;
    const int n = g.B * hw;
    const int idx = bx * 256 + threadIdx.x;
    const bool mine = idx < n;
    const int ic = mine ? idx : 0;
    const int b = ic / hw, r = ic - b * hw;
    const int Y = r / g.Wl, X = r - Y * g.Wl;
    const size_t o = ((size_t)(b * g.Cl + cl) * g.Hl + Y) * g.Wl + X;
    // taps of output (Y, X): ky = Y mod s, + s, ... reading row y = Y / s, - 1, ...: one division per dimension per
    // thread instead of one per (channel, tap)
    const int y0 = Y / g.s, x0 = X / g.s;
    const int ky0 = Y - y0 * g.s, kx0 = X - x0 * g.s;
    // At most 2 x 2 taps per output (3x3 or 4x4 kernels at stride 2).  The general loop further down issues one load, waits,
    // multiplies, per (channel, tap): ~16 dependent memory round trips per thread.  Here four channels' taps, their raw
    // outputs (BatchNorm backward) and weights are fetched together from clamped addresses, then consumed in the same
    // (channel, ky, kx) order.
    const bool four_taps = g.kh <= 2 * g.s && g.kw <= 2 * g.s;
    int yy[2], xx[2], kyy[2], kxx[2];
    bool vy[2], vx[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int ky = ky0 + t * g.s, y = y0 - t, kx = kx0 + t * g.s, x = x0 - t;
        vy[t] = ky < g.kh && y >= 0 && y < g.Hs;
        vx[t] = kx < g.kw && x >= 0 && x < g.Ws;
        yy[t] = min(max(y, 0), g.Hs - 1);
        xx[t] = min(max(x, 0), g.Ws - 1);
        kyy[t] = min(ky, g.kh - 1);
        kxx[t] = min(kx, g.kw - 1);
    }
    const int khw = g.kh * g.kw;
    size_t sb = 0;
    auto load_group = [&](int c0, float (&gv)[4][4], float (&qv)[4][4], float (&wv)[4][4]) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int cs = min(c0 + c, g.Cs - 1);
            const float* wp = w + (size_t)(cs * g.Cl + cl) * khw;
            const size_t base = (sb * g.Cs + cs) * (size_t)g.Hs * g.Ws;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const size_t off = base + (size_t)yy[t >> 1] * g.Ws + xx[t & 1];
                gv[c][t] = small.p[off];
                qv[c][t] = bns.mode == BN_BWD ? small.q[off] : 0.f;
                wv[c][t] = wp[kyy[t >> 1] * g.kw + kxx[t & 1]];
            }
        }
    };
    // The first group of four channels and the epilogue's mask input are requested before the BatchNorm constants are worked
    // out (their sums, the barrier): one trip to memory for all of it instead of three in a row.
    float gv0[4][4], qv0[4][4], wv0[4][4];
    float ypre = 0.f;
    const bool pre_mask = e.kind == EPI_MASKSTATS;
    if (mine) {
        sb = sample_of(small.perm, small.use_cursor, st, b);
        if (four_taps) load_group(0, gv0, qv0, wv0);
        if (pre_mask) ypre = e.yprev[o];
    }

    bn_consts(bns, cs4, designated);
    bn_consts(bne, ce, false, 64);
    __syncthreads();

    double r1 = 0, r2 = 0;
    if (mine) {
        float acc = bias ? bias[cl] : 0.f;
        if (four_taps) {
            for (int c0 = 0; c0 < g.Cs; c0 += 4) {
                float gv[4][4], qv[4][4], wv[4][4];
                if (c0 == 0) {
#pragma unroll
                    for (int c = 0; c < 4; c++)
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            gv[c][t] = gv0[c][t];
                            qv[c][t] = qv0[c][t];
                            wv[c][t] = wv0[c][t];
                        }
                } else {
                    load_group(c0, gv, qv, wv);
                }
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int t = 0; t < 4; t++) asm volatile("" : "+v"(gv[c][t]), "+v"(qv[c][t]), "+v"(wv[c][t]));
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if (c0 + c >= g.Cs) break;
                    const float4 k = bns.mode ? cs4[c0 + c] : make_float4(0, 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < 4; t++)
                        if (vy[t >> 1] && vx[t & 1]) acc = fmaf(bn_apply(bns.mode, k, gv[c][t], qv[c][t]), wv[c][t], acc);
                }
            }
        } else
        for (int cs = 0; cs < g.Cs; cs++) {
            const float* wp = w + (size_t)(cs * g.Cl + cl) * g.kh * g.kw;
            const size_t base = (sb * g.Cs + cs) * (size_t)g.Hs * g.Ws;
            const float4 k = bns.mode ? cs4[cs] : make_float4(0, 0, 0, 0);
            for (int ky = ky0, y = y0; ky < g.kh && y >= 0; ky += g.s, y--) {
                if (y >= g.Hs) continue;
                for (int kx = kx0, x = x0; kx < g.kw && x >= 0; kx += g.s, x--) {
                    if (x >= g.Ws) continue;
                    const size_t off = base + (size_t)y * g.Ws + x;
                    const float v = small.p[off];
                    const float yr = bns.mode == BN_BWD ? small.q[off] : 0.f;
                    acc = fmaf(bn_apply(bns.mode, k, v, yr), wp[ky * g.kw + kx], acc);
                }
            }
        }
        size_t tgt = 0;
        if (e.kind >= EPI_SIGMSE && e.target) {
            const size_t tb = sample_of(e.perm, e.use_cursor, st, b);
            tgt = ((tb * g.Cl + cl) * (size_t)g.Hl + Y) * g.Wl + X;
        }
        epi_element(e, ce, cl, o, tgt, acc, r1, r2, pre_mask, ypre);
    }
    epi_block(e, cl, st, r1, r2, red, bx);
}

__global__ void __launch_bounds__(256) k_up(ConvGeom g, Src small, BnDesc bns, const float* __restrict__ w,
                                             const float* __restrict__ bias, Epi e, BnDesc bne,
                                             const StepState* __restrict__ st) {
    extern __shared__ double lds_d[];
    up_body(g, small, bns, w, bias, e, bne, st, lds_d, blockIdx.x, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------
// wgrad: acc[cs][cl][ky][kx] += sum_{b,y,x} Ts(S[b][cs][y][x]) * Tl(L[b][cl][y*s+ky][x*s+kx])
// grid (Cs*Cl*kh*kw, nsplit); each block covers `ppb` positions of (b,y,x).
// The designated block also publishes the BatchNorm parameter gradients of the layer whose
// backward this is (dgamma = sum g*xhat, dbeta = sum g), taken from the fp64 stat sums.
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ void wgrad_body(const ConvGeom& g, const Src& small, const BnDesc& bns, const Src& big,
                                           const BnDesc& bnb, double* __restrict__ acc, int ppb, const BnGradOut& bg,
                                           const StepState* __restrict__ st, double* lds_d, const int bx, const int by) {
    double* red = lds_d;
    float4* cs4 = reinterpret_cast<float4*>(lds_d + 4);
    float4* cb = cs4 + g.Cs;

    int widx = bx;
    const int kx = widx % g.kw;
    widx /= g.kw;
    const int ky = widx % g.kh;
    widx /= g.kh;
    const int cl = widx % g.Cl;
    const int cs = widx / g.Cl;
    const int hw = g.Hs * g.Ws;
    const long long n = (long long)g.B * hw;
    const long long p0 = (long long)by * ppb;
    long long p1 = p0 + ppb;
    if (p1 > n) p1 = n;
    const bool fastdiv = n < kDivSmallMaxN && hw < kDivSmallMaxD;   // 3-instruction index arithmetic instead of 64-bit divisions
    const float inv_hw = 1.0f / (float)hw, inv_w = 1.0f / (float)g.Ws;
    // raw operands of position p (the BatchNorm transforms are applied by the caller)
    auto fetch = [&](long long p, float& sp, float& sq, float& lp, float& lq) {
        int b, y;
        if (fastdiv) {
            b = div_small((int)p, inv_hw);
            y = div_small((int)p - b * hw, inv_w);
        } else {
            b = (int)(p / hw);
            y = (int)(p - (long long)b * hw) / g.Ws;
        }
        const int r = (int)(p - (long long)b * hw), x = r - y * g.Ws;
        const size_t ss = sample_of(small.perm, small.use_cursor, st, b);
        const size_t sl = sample_of(big.perm, big.use_cursor, st, b);
        const size_t so = ((ss * g.Cs + cs) * (size_t)g.Hs + y) * g.Ws + x;
        const size_t lo = ((sl * g.Cl + cl) * (size_t)g.Hl + (size_t)(y * g.s + ky)) * g.Wl + (size_t)x * g.s + kx;
        sp = small.p[so];
        sq = bns.mode == BN_BWD ? small.q[so] : 0.f;
        lp = big.p[lo];
        lq = bnb.mode == BN_BWD ? big.q[lo] : 0.f;
    };
    // The first position's operands are requested before the BatchNorm constants are worked out: with the usual one
    // position per thread (wgrad_ppb) the kernel is then one trip to memory deep instead of two (cursor -> operands used to
    // start behind the constants' sums and the barrier).
    const long long pf = p0 + threadIdx.x;
    float f_sp = 0.f, f_sq = 0.f, f_lp = 0.f, f_lq = 0.f;
    if (pf < p1) fetch(pf, f_sp, f_sq, f_lp, f_lq);

    bn_consts(bns, cs4, false);
    bn_consts(bnb, cb, false, 64);
    if (bx == 0 && by == 0 && bg.stats) {
        for (int c = threadIdx.x; c < bg.C; c += blockDim.x) {
            double sb = 0.0, sg = 0.0;
            for (int sh = 0; sh < kStatShards; sh++) {
                sb += bg.stats[((size_t)sh * bg.C + c) * 4 + 2];
                sg += bg.stats[((size_t)sh * bg.C + c) * 4 + 3];
            }
            bg.beta_acc[c] = sb * bg.scale;
            bg.gamma_acc[c] = sg * bg.scale;
        }
    }
    __syncthreads();
    const float4 ks = bns.mode ? cs4[cs] : make_float4(0, 0, 0, 0);
    const float4 kb = bnb.mode ? cb[cl] : make_float4(0, 0, 0, 0);

    float sum = 0.f;
    if (pf < p1) sum = bn_apply(bns.mode, ks, f_sp, f_sq) * bn_apply(bnb.mode, kb, f_lp, f_lq);
    for (long long p = pf + 256; p < p1; p += 256) {
        float sp, sq, lp, lq;
        fetch(p, sp, sq, lp, lq);
        sum = fmaf(bn_apply(bns.mode, ks, sp, sq), bn_apply(bnb.mode, kb, lp, lq), sum);
    }
    const double t = block_sum((double)sum, red);
    if (threadIdx.x == 0) acc_add<ACC_GRAD>(&acc[bx], t);
}

__global__ void __launch_bounds__(256) k_wgrad(ConvGeom g, Src small, BnDesc bns, Src big, BnDesc bnb,
                                                double* __restrict__ acc, int ppb, BnGradOut bg,
                                                const StepState* __restrict__ st) {
    kernarg_warm<sizeof(ConvGeom) + 2 * sizeof(Src) + 2 * sizeof(BnDesc) + sizeof(BnGradOut) + 32>();
    extern __shared__ double lds_d[];
    wgrad_body(g, small, bns, big, bnb, acc, ppb, bg, st, lds_d, blockIdx.x, blockIdx.y);
}

// One launch for a Conv2d layer's weight gradient AND its input gradient (they share only their inputs): workgroups
// [0, nwx * nwy) are k_wgrad's grid, the rest k_up's (ux wide).
struct WgradArgs {
    ConvGeom g;
    Src small;
    BnDesc bns;
    Src big;
    BnDesc bnb;
    double* acc;
    int ppb;
    BnGradOut bg;
};
struct UpArgs {
    ConvGeom g;
    Src small;
    BnDesc bns;
    const float* w;
    const float* bias;
    Epi e;
    BnDesc bne;
};
__global__ void __launch_bounds__(256) k_conv_bwd_pair(WgradArgs wa, UpArgs ua, int nwx, int nwy, int ux,
                                                        const StepState* __restrict__ st) {
    kernarg_warm<sizeof(WgradArgs) + sizeof(UpArgs) + 24>();
    extern __shared__ double lds_d[];
    const int i = blockIdx.x, nw = nwx * nwy;
    if (i < nw) {
        const int by = i / nwx;
        wgrad_body(wa.g, wa.small, wa.bns, wa.big, wa.bnb, wa.acc, wa.ppb, wa.bg, st, lds_d, i - by * nwx, by);
    } else {
        const int j = i - nw, by = j / ux;
        up_body(ua.g, ua.small, ua.bns, ua.w, ua.bias, ua.e, ua.bne, st, lds_d, j - by * ux, by);
    }
}

// ---------------------------------------------------------------------------------------------
// Linear layers (encoder.py:54-58, decoder.py:31-35), weight W[out][in]
// ---------------------------------------------------------------------------------------------

// out[b][o] = act(bias[o] + sum_i T(in[b][i]) * W[o][i]);  T = BN+ReLU per channel i/hw or identity
__global__ void __launch_bounds__(256) k_lin_fwd(int B, int nin, int nout, const float* __restrict__ in,
                                                  BnDesc bni, int hw, const float* __restrict__ W,
                                                  const float* __restrict__ bias, int relu,
                                                  float* __restrict__ out) {
    extern __shared__ double lds_d[];
    float4* ci = reinterpret_cast<float4*>(lds_d + 4);
    bn_consts(bni, ci, blockIdx.x == 0);
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * nout) return;
    const int b = idx / nout, o = idx - b * nout;
    const float* ip = in + (size_t)b * nin;
    const float* wp = W + (size_t)o * nin;
    float acc = bias[o];
    if (bni.mode) {
        for (int i = 0; i < nin; i++) acc = fmaf(bn_apply(bni.mode, ci[i / hw], ip[i], 0.f), wp[i], acc);
    } else {
        for (int i = 0; i < nin; i++) acc = fmaf(ip[i], wp[i], acc);
    }
    out[idx] = relu ? fmaxf(acc, 0.f) : acc;
}

// gin[b][i] = M( sum_o gout[b][o] * W[o][i] )
//   epi 0: M = identity; 1: M = mask by hin[b][i] > 0 (ReLU of the producing Linear);
//   epi 2: M = mask by BN+ReLU of yprev + D1/D2 sums (grid.y = channel, i = c*hw + r)
__global__ void __launch_bounds__(256) k_lin_dgrad(int B, int nin, int nout, const float* __restrict__ gout,
                                                    const float* __restrict__ W, int epi,
                                                    const float* __restrict__ hin, BnDesc bne, int hw,
                                                    double* stats, float* __restrict__ gin) {
    extern __shared__ double lds_d[];
    double* red = lds_d;
    float4* ce = reinterpret_cast<float4*>(lds_d + 4);
    bn_consts(bne, ce, false);
    __syncthreads();
    double r1 = 0, r2 = 0;
    if (epi != 2) {
        const int idx = blockIdx.x * 256 + threadIdx.x;
        if (idx < B * nin) {
            const int b = idx / nin, i = idx - b * nin;
            const float* gp = gout + (size_t)b * nout;
            float acc = 0.f;
            for (int o = 0; o < nout; o++) acc = fmaf(gp[o], W[(size_t)o * nin + i], acc);
            if (epi == 1) acc = hin[idx] > 0.f ? acc : 0.f;
            gin[idx] = acc;
        }
        return;
    }
    const int c = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < B * hw) {
        const int b = idx / hw, r = idx - b * hw;
        const int i = c * hw + r;
        const float* gp = gout + (size_t)b * nout;
        float acc = 0.f;
        for (int o = 0; o < nout; o++) acc = fmaf(gp[o], W[(size_t)o * nin + i], acc);
        const size_t off = (size_t)b * nin + i;
        const float4 k = ce[c];
        const float d = hin[off] - k.x;
        const float a = fmaf(d, k.y, k.z);
        const float gm = a > 0.f ? acc : 0.f;
        gin[off] = gm;
        r1 = (double)gm;
        r2 = (double)gm * (double)(d * k.w);
    }
    const double t1 = block_sum(r1, red);
    const double t2 = block_sum(r2, red);
    if (threadIdx.x == 0) {
        const size_t row = ((size_t)(blockIdx.x & (kStatShards - 1)) * bne.C + c) * 4;
        acc_add<ACC_GRAD>(&stats[row + 2], t1);
        acc_add<ACC_GRAD>(&stats[row + 3], t2);
    }
}

// accW[o][i] = sum_b gout[b][o] * T(in[b][i]);  accB[o] = sum_b gout[b][o]
__global__ void __launch_bounds__(256) k_lin_wgrad(int B, int nin, int nout, const float* __restrict__ gout,
                                                    const float* __restrict__ in, BnDesc bni, int hw,
                                                    double* __restrict__ accW, double* __restrict__ accB) {
    extern __shared__ double lds_d[];
    float4* ci = reinterpret_cast<float4*>(lds_d + 4);
    bn_consts(bni, ci, false);
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nout * nin) return;
    const int o = idx / nin, i = idx - o * nin;
    const float4 k = bni.mode ? ci[i / hw] : make_float4(0, 0, 0, 0);
    float sum = 0.f, bsum = 0.f;
    for (int b = 0; b < B; b++) {
        const float gv = gout[(size_t)b * nout + o];
        sum = fmaf(gv, bn_apply(bni.mode, k, in[(size_t)b * nin + i], 0.f), sum);
        bsum += gv;
    }
    accW[idx] = (double)sum;
    if (i == 0) accB[o] = (double)bsum;
}

// ---------------------------------------------------------------------------------------------
// optimiser + bookkeeping
// ---------------------------------------------------------------------------------------------
struct Hyper {
    double lr, beta1, beta2, eps, wd;
};

// What the last kernel of a step does besides its own work: zero the accumulators for the next step
// (each fp64 gradient slot is cleared by the thread that just consumed it; the BatchNorm sum tables,
// which nobody reads any more, by a grid-stride sweep) and move the cursor (nobody in this kernel
// reads batch_start / loss_slot).
struct StepTail {
    double* zero_extra;       // BatchNorm sum tables (and whatever else sits before the gradient accumulator)
    long long zero_extra_n;   // doubles
    double* acc_rw;           // fp64 gradient accumulator, writable view (or nullptr)
    double* shard_rw;         // sharded side table, writable view (or nullptr)
    StepState* st;
    int batch_inc, slot_inc;
};

__device__ __forceinline__ float consume_grad(const StepTail& tl, const ShardSegs& ss, long long i) {
    double g = tl.acc_rw[i];
    tl.acc_rw[i] = 0.0;
    for (int s = 0; s < ss.nseg; s++) {
        const long long d = i - ss.seg[s].param_off;
        if (d >= 0 && d < ss.seg[s].count) {
            // all eight shard reads in flight before the first clearing store (a load/store per shard in turn is eight
            // dependent round trips for the threads that own sharded parameters: the tail of this kernel)
            double* p = tl.shard_rw + ss.seg[s].sh_off + d;
            double v[kStatShards];
#pragma unroll
            for (int sh = 0; sh < kStatShards; sh++) v[sh] = p[(size_t)sh * ss.n];
#pragma unroll
            for (int sh = 0; sh < kStatShards; sh++) {
                g += v[sh];
                p[(size_t)sh * ss.n] = 0.0;
            }
        }
    }
    return (float)g;
}

// exp_avg.lerp_(grad, w) with w = 1 - beta1, in the form ATen's lerp takes for each weight: from the old value below one half,
// from the gradient above, where (g - m) * w added to m would round at the size of m (beta1 = 0 gives g itself)
__device__ __forceinline__ float adam_lerp(float mi, float g, float w) {
    return w < 0.5f ? mi + (g - mi) * w : g - (g - mi) * (1.f - w);
}

__device__ __forceinline__ void step_tail(const StepTail& tl, long long gid, long long nthreads) {
    for (long long j = gid; j < tl.zero_extra_n; j += nthreads) tl.zero_extra[j] = 0.0;
    if (gid == 0 && tl.st) {
        tl.st->batch_start += tl.batch_inc;
        tl.st->loss_slot += tl.slot_inc;
    }
}

// torch.optim.Adam single-tensor update (L2 weight decay added to the gradient), element-wise
// over the flat arena.  Gradient source: fp64 accumulators (fused path; consumed and cleared) or
// the fp32 arena (data-parallel path, after the all-reduce).  st->adam_step is the number of the
// step being taken (bumped by the first kernel of the step / by cae_adam_step's own bump flag),
// st->lr the learning rate (h.lr is the host's copy of it: no kernel reads it).
// The first encoder layer's weight gradient, folded into the optimiser launch (k_adam): it is the last kernel of backward, a
// reduction of B*Hs*Ws products per weight that nothing but the optimiser waits for - as its own launch 5.6 us, 3 % of the
// step.  One extra workgroup per weight: it reduces the whole batch itself (no cross-workgroup sum, so no ordering between
// the reduction and the update), then updates that one parameter.  The inputs come from the contiguous copy of the batch
// that k_head_fwd leaves behind (the cursor has moved on by now: this kernel moves it).  The BatchNorm parameter gradients
// of that layer, which the weight-gradient launch used to turn from sums into accumulator entries, are taken from the sums
// directly by the threads that own gamma and beta; the layer's sum table is left for the next step's first kernel to clear.
struct AdamConv0 {
    int on, nw, C, n_regular;   // n_regular: workgroups of the element-wise update (then one per weight)
    long long w_off, gamma_off, beta_off;
    ConvGeom g;
    Src small;                  // p = masked gradient of the layer's output, q = its raw output (BN_BWD)
    BnDesc bns;
    const float* xb;            // (B, Cl, Hl, Wl) the batch's inputs, contiguous
    const double* stats;        // the layer's BatchNorm table [shards][C][4]
    double scale;               // 1 / world (1 here: the fused form is single-device only)
};
constexpr int kAdamConv0Pos = 16;   // positions per thread requested in one burst

__device__ __forceinline__ void adam_conv0_body(const AdamConv0& c0, float* __restrict__ p, float* __restrict__ m,
                                                float* __restrict__ v, const Hyper& h, const StepState* __restrict__ st,
                                                int t_add, double ln_b1, double ln_b2, float* corr, double* red, float4* cs4) {
    const ConvGeom& g = c0.g;
    const int tid = threadIdx.x;
    int widx = blockIdx.x - c0.n_regular;
    const int kx = widx % g.kw;
    widx /= g.kw;
    const int ky = widx % g.kh;
    widx /= g.kh;
    const int cl = widx % g.Cl;
    const int cs = widx / g.Cl;
    const long long pi = c0.w_off + (blockIdx.x - c0.n_regular);
    int t = 0;
    double lr = 0.0;
    if (tid < 2) {
        optimiser_state(st, t, lr);
        t += t_add;
    }
    const int hw = g.Hs * g.Ws, n = g.B * hw;
    const float inv_hw = 1.0f / (float)hw, inv_w = 1.0f / (float)g.Ws;
    // Sixteen positions' addresses stand ahead of the first operand load, so their arithmetic is the front of the launch's
    // longest workgroups: 24-bit multiplies (full rate; a 32-bit one takes four times as long, the 64-bit index arithmetic
    // this replaces longer) and 32-bit byte offsets from the wave-uniform bases.  enc_conv0_fits_adam keeps every factor below
    // 2^24 and every offset below 2^32; the elements read, and the order they are added in, are what they were.
    const unsigned small_b = (unsigned)(g.Cs * hw), big_b = (unsigned)(g.Cl * g.Hl * g.Wl), big_y = (unsigned)(g.s * g.Wl);
    const unsigned small_0 = (unsigned)(cs * hw), big_0 = (unsigned)((cl * g.Hl + ky) * g.Wl + kx);
    auto at = [](const float* base, unsigned elem) {
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + (size_t)(elem * 4u));
    };
    auto fetch = [&](int pp, float& sp, float& sq, float& lp) {
        const int b = div_small(pp, inv_hw), r = pp - __mul24(b, hw);
        const int y = div_small(r, inv_w), x = r - __mul24(y, g.Ws);
        const unsigned so = __umul24((unsigned)b, small_b) + small_0 + (unsigned)r;
        sp = at(c0.small.p, so);
        sq = at(c0.small.q, so);
        lp = at(c0.xb, __umul24((unsigned)b, big_b) + __umul24((unsigned)y, big_y) + __umul24((unsigned)x, (unsigned)g.s) + big_0);
    };
    float sp[kAdamConv0Pos], sq[kAdamConv0Pos], lp[kAdamConv0Pos];
#pragma unroll
    for (int u = 0; u < kAdamConv0Pos; u++) fetch(min(tid + u * 256, n - 1), sp[u], sq[u], lp[u]);
    // Behind the operands, in the same burst (loads return in the order they were requested, so nothing here is waited for
    // ahead of them): the BatchNorm constants' inputs, one channel per thread of the LAST wave (C <= 64) - bn_consts used to
    // request them behind the operands' wait, a second trip to memory - and the parameter with its moments.
    BnBwdReq rq;
    const int bc_ = tid - 192;
    const bool has_c = bc_ >= 0 && bc_ < c0.bns.C;
    if (has_c) bn_bwd_request(c0.bns, bc_, rq);
    float w = 0.f, mi = 0.f, vi = 0.f;
    if (tid == 0) {
        w = p[pi];
        mi = m[pi];
        vi = v[pi];
    }
    // the bias corrections while all of that travels (two lanes of the first wave: an fp64 chain that used to start behind the
    // operands' wait)
    if (tid < 2) {
        const double bc = -expm1((double)t * (tid ? ln_b2 : ln_b1));
        corr[tid] = tid ? (float)sqrt(bc) : (float)(lr / bc);
    }
#pragma unroll
    for (int u = 0; u < kAdamConv0Pos; u++) asm volatile("" : "+v"(sp[u]), "+v"(sq[u]), "+v"(lp[u]));
    if (has_c) cs4[bc_] = bn_bwd_finish(c0.bns, rq);
    __syncthreads();
    const float4 ks = cs4[cs];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < kAdamConv0Pos; u++)
        if (tid + u * 256 < n) sum = fmaf(bn_apply(BN_BWD, ks, sp[u], sq[u]), lp[u], sum);
    for (int pp = tid + kAdamConv0Pos * 256; pp < n; pp += 256) {
        float a, b, c;
        fetch(pp, a, b, c);
        sum = fmaf(bn_apply(BN_BWD, ks, a, b), c, sum);
    }
    const double tot = block_sum((double)sum, red);
    if (tid == 0) {
        float gr = (float)(tot * c0.scale);
        if (h.wd != 0.0) gr = fmaf((float)h.wd, w, gr);
        mi = adam_lerp(mi, gr, (float)(1.0 - h.beta1));
        vi = vi * (float)h.beta2 + ((float)(1.0 - h.beta2) * gr) * gr;
        const float denom = sqrtf(vi) / corr[1] + (float)h.eps;
        p[pi] = w - corr[0] * (mi / denom);
        m[pi] = mi;
        v[pi] = vi;
    }
}

// `ln_b1`, `ln_b2`: natural logarithms of the betas (host).
// Order matters, this being the one kernel every step ends with: every thread requests its parameter, moments and gradient
// first; the bias corrections 1 - beta^t = -expm1(t ln beta) are worked out meanwhile by two lanes, one each (the two fp64
// pow() calls on one lane they replace were a dependent chain of a microsecond ahead of the barrier, with the loads not
// yet requested behind it).
__global__ void __launch_bounds__(256) k_adam(long long n, float* __restrict__ p, const float* __restrict__ g32,
                                               float* __restrict__ m, float* __restrict__ v, Hyper h,
                                               const StepState* __restrict__ st, ShardSegs ss, StepTail tl, int t_add,
                                               double ln_b1, double ln_b2, AdamConv0 c0) {
    kernarg_warm<sizeof(Hyper) + sizeof(ShardSegs) + sizeof(StepTail) + 72 + sizeof(AdamConv0)>();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    __shared__ float corr[2];
    if (c0.on && (int)blockIdx.x >= c0.n_regular) {   // uniform per workgroup
        __shared__ double red0[8];
        __shared__ float4 cs40[64];
        adam_conv0_body(c0, p, m, v, h, st, t_add, ln_b1, ln_b2, corr, red0, cs40);
        return;
    }
    // The step tail (step_tail's work) first.  No kernel of this step reads the BatchNorm sum tables any more, and nobody in
    // this kernel reads the cursor: cleared / moved up here, the stores complete in the shadow of the loads below.  Behind
    // the parameter update they cost a wait of their own: registers are reused there, and the compiler then waits for the
    // stores ahead of them (the memory counter retires in order).
    for (long long j = i; j < tl.zero_extra_n; j += (long long)(c0.on ? c0.n_regular : (int)gridDim.x) * 256) tl.zero_extra[j] = 0.0;
    int t = 0;
    double lr = 0.0;
    if (threadIdx.x < 2) {   // the rate is requested with the step number and waited for at the division below
        optimiser_state(st, t, lr);
        t += t_add;
    }
    const bool moves_cursor = i == 0 && tl.st != nullptr;
    long long cursor = 0;
    int slot = 0;
    if (moves_cursor) {
        cursor = tl.st->batch_start;
        slot = tl.st->loss_slot;
    }
    const bool mine = i < n && !(c0.on && i >= c0.w_off && i < c0.w_off + c0.nw);   // those weights: adam_conv0_body
    float g = 0.f, w = 0.f, mi = 0.f, vi = 0.f;
    // the fp64 gradient: its accumulator plus, for a parameter that is accumulated in shards, the eight shard copies.
    // Requested here, added up behind the barrier, cleared by the kernel's last stores (consume_grad's clearing stores sit
    // between its loads and their use, and where its paths meet the compiler waits for all but one of them to complete)
    double gacc = 0.0, sv[kStatShards], bv[kStatShards];
    double* shp = nullptr;
    const double* bnp = nullptr;
    if (mine) {
        w = p[i];
        mi = m[i];
        vi = v[i];
        if (g32) {
            g = g32[i];
        } else {
            gacc = tl.acc_rw[i];
            for (int sg = 0; sg < ss.nseg; sg++) {
                const long long d = i - ss.seg[sg].param_off;
                if (d >= 0 && d < ss.seg[sg].count) shp = tl.shard_rw + ss.seg[sg].sh_off + d;
            }
            if (shp) {
#pragma unroll
                for (int sh = 0; sh < kStatShards; sh++) sv[sh] = shp[(size_t)sh * ss.n];
            }
            if (c0.on) {   // gamma / beta of the fused layer: straight from its BatchNorm-backward sums (slots 3 / 2)
                const long long dg = i - c0.gamma_off, db = i - c0.beta_off;
                if (dg >= 0 && dg < c0.C) bnp = c0.stats + dg * 4 + 3;
                if (db >= 0 && db < c0.C) bnp = c0.stats + db * 4 + 2;
                if (bnp) {
#pragma unroll
                    for (int sh = 0; sh < kStatShards; sh++) bv[sh] = bnp[(size_t)sh * c0.C * 4];
                }
            }
        }
    }
    if (moves_cursor) {
        tl.st->batch_start = cursor + tl.batch_inc;
        tl.st->loss_slot = slot + tl.slot_inc;
    }
    if (threadIdx.x < 2) {
        const double bc = -expm1((double)t * (threadIdx.x ? ln_b2 : ln_b1));
        corr[threadIdx.x] = threadIdx.x ? (float)sqrt(bc) : (float)(lr / bc);
    }
    __syncthreads();
    if (mine) {
        const float step_size = corr[0];
        const float bc2_sqrt = corr[1];
        const float b2 = (float)h.beta2;
        if (!g32) {
            if (shp) {
#pragma unroll
                for (int sh = 0; sh < kStatShards; sh++) gacc += sv[sh];
            }
            if (bnp) {
                double t2 = 0.0;
#pragma unroll
                for (int sh = 0; sh < kStatShards; sh++) t2 += bv[sh];
                gacc += t2 * c0.scale;
            }
            g = (float)gacc;
        }
        if (h.wd != 0.0) g = fmaf((float)h.wd, w, g);
        mi = adam_lerp(mi, g, (float)(1.0 - h.beta1));
        vi = vi * b2 + ((float)(1.0 - h.beta2) * g) * g;
        const float denom = sqrtf(vi) / bc2_sqrt + (float)h.eps;
        p[i] = w - step_size * (mi / denom);
        m[i] = mi;
        v[i] = vi;
        if (!g32) {
            tl.acc_rw[i] = 0.0;
            if (shp) {
#pragma unroll
                for (int sh = 0; sh < kStatShards; sh++) shp[(size_t)sh * ss.n] = 0.0;
            }
        }
    }
}

__global__ void k_acc_to_f32(long long n, float* __restrict__ g, ShardSegs ss, StepTail tl) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    step_tail(tl, i, (long long)gridDim.x * 256);
    if (i < n) g[i] = consume_grad(tl, ss, i);
}

// data-parallel path: the fp64 accumulators of parameters [lo, hi) -> the fp32 gradient arena (consumed and cleared), one
// gradient bucket per launch; the launch for the last bucket also carries the step tail
__global__ void k_narrow_range(long long lo, long long hi, float* __restrict__ g, ShardSegs ss, StepTail tl) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tl.zero_extra || tl.st) step_tail(tl, t, (long long)gridDim.x * 256);
    const long long i = lo + t;
    if (i < hi) g[i] = consume_grad(tl, ss, i);
}

__global__ void k_fill_f32(float* __restrict__ p, long long n, float v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ void k_scale_f32(float* __restrict__ p, long long n, float f) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] *= f;
}

__global__ void k_scale_f64(double* __restrict__ p, long long n, double f) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] *= f;
}

// the optimiser step counter for the data-parallel path, where Adam runs as its own op
__global__ void k_bump_adam(StepState* st) { st->adam_step += 1; }

// What a rank whose data-parallel shard is empty does with one all-reduced BatchNorm table of a SyncBN step, where the other
// ranks' kernels read it (one workgroup, dynamic LDS of C float4).  d (BN_BATCH, update): the running statistics advance from
// the global sums as the designated consumer block does (bn_batch_finish); bg.stats: dgamma / dbeta take this rank's share
// bg.scale of the global sums, as BnGradOut does in the weight-gradient kernels.
__global__ void __launch_bounds__(256) k_bn_empty_shard(BnDesc d, BnGradOut bg) {
    extern __shared__ float4 consts[];
    bn_consts(d, consts, true);
    if (!bg.stats) return;
    for (int c = threadIdx.x; c < bg.C; c += blockDim.x) {
        double sb = 0.0, sg = 0.0;
        for (int sh = 0; sh < kStatShards; sh++) {
            sb += bg.stats[((size_t)sh * bg.C + c) * 4 + 2];
            sg += bg.stats[((size_t)sh * bg.C + c) * 4 + 3];
        }
        bg.beta_acc[c] = sb * bg.scale;
        bg.gamma_acc[c] = sg * bg.scale;
    }
}

__global__ void k_set_state(StepState* st, long long batch_start, int loss_slot, int set_cursor, int adam_step,
                            int set_adam) {
    if (set_cursor) {
        st->batch_start = batch_start;
        st->loss_slot = loss_slot;
    }
    if (set_adam) st->adam_step = adam_step;
}

// the learning rate of the steps enqueued after this launch (stream-ordered; graphs read it, none bakes it in)
__global__ void k_set_lr(StepState* st, double lr) { st->lr = lr; }

__global__ void k_advance(StepState* st, int batch, int slot_inc, int adam_inc) {
    st->batch_start += batch;
    st->loss_slot += slot_inc;
    st->adam_step += adam_inc;
}

}  // namespace cae
