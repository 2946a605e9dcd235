// device_common.h — device helpers and descriptors shared by every kernels_*.h of the ConvAE path: the BatchNorm table
// shards, the step state, the descriptors the kernels take (BnDesc, Src, Epi, ConvGeom, BnGradOut), argument-block warming,
// small-divisor division, the DPP / wave / block sums and the BatchNorm constants.  No kernel is defined here, so a source
// that needs only the helpers (ctbwd.hip, the ugemm wrapper of unet_engine.hip) compiles none it does not launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cae {

// BatchNorm sum accumulators are kept in kStatShards copies, [shard][C][4]; producers add into the
// copy picked by their block index (same-address fp64 atomics serialise at the memory side),
// consumers add the copies up in bn_consts.
constexpr int kStatShards = 8;

#include "acc_grid.h"   // AccKind, acc_grid, acc_add: the grids and why they make the sums order-independent

// Gradient accumulators that many workgroups hit at once (weights of the thin stride-2 layers,
// the last layer's bias) live in a sharded side table [kStatShards][n]; Adam adds the shards up.
struct ShardSeg {
    long long param_off;  // first parameter of the segment in the flat arena
    int count;
    int sh_off;           // offset inside one shard
};
struct ShardSegs {
    int nseg;
    int n;                // doubles per shard
    const double* base;   // [kStatShards][n]
    ShardSeg seg[12];
};

__device__ __forceinline__ double sharded_grad(const ShardSegs& ss, long long i) {
    double g = 0.0;
    for (int s = 0; s < ss.nseg; s++) {
        const long long d = i - ss.seg[s].param_off;
        if (d >= 0 && d < ss.seg[s].count) {
            for (int sh = 0; sh < kStatShards; sh++) g += ss.base[(size_t)sh * ss.n + ss.seg[s].sh_off + d];
        }
    }
    return g;
}

struct alignas(16) StepState {
    long long batch_start;  // first position in the permutation of the current batch
    int loss_slot;          // where this step's loss is accumulated
    int pad0;
    // one aligned 16-byte block, which the optimiser kernel requests as a whole (optimiser_state)
    double lr;              // learning rate of the next optimiser step (cae_set_lr / cae_set_hyper): read by k_adam, so a
                            // captured graph follows a schedule without being captured again
    int adam_step;          // completed optimiser steps
    int pad1;
};
static_assert(offsetof(StepState, lr) % 16 == 0 && offsetof(StepState, adam_step) == offsetof(StepState, lr) + 8, "StepState layout");

// The step number and the learning rate, requested together.  The compiler keeps the step number a scalar load and makes
// the rate a vector load that is waited for where it is used (the division), not ahead of the requests that follow this call.
__device__ __forceinline__ void optimiser_state(const StepState* __restrict__ st, int& adam_step, double& lr) {
    const int4 q = *reinterpret_cast<const int4*>(reinterpret_cast<const char*>(st) + offsetof(StepState, lr));
    lr = __hiloint2double(q.y, q.x);
    adam_step = q.z;
}

// How a tensor that is READ relates to BatchNorm.
enum BnMode : int {
    BN_NONE = 0,     // identity
    BN_BATCH = 1,    // activation a = relu((y-mean)*scale+beta), mean/var from this step's sums
    BN_RUNNING = 2,  // same with running statistics (eval)
    BN_SAVED = 3,    // same with the mean/invstd the forward pass saved (backward reads)
    BN_BWD = 4       // gradient wrt the raw conv output: k1*g - k2 - (y-mean)*k3
};

struct BnDesc {
    int mode;
    int C;
    const double* stats;  // [kStatShards][C][4]: sum y, sum y^2, sum g, sum g*xhat
    const float* gamma;
    const float* beta;
    float* rmean;
    float* rvar;
    float* saved;  // [C][2]: mean, invstd
    double count;  // elements per channel (global count under SyncBN)
    double inv_count, unbias;   // 1 / count and count / (count - 1) (1 for a single element): no fp64 divisions on the device
    float momentum;
    float eps;
    int update;    // BN_BATCH: this consumer also updates running stats and `saved`
};

// A tensor read through an optional per-channel transform.
struct Src {
    const float* p;    // data (for BN_BWD: the masked upstream gradient g)
    const float* q;    // BN_BWD only: the raw forward output y
    const int* perm;   // dataset gather: sample = perm[batch_start + b]   (nullptr: sample = b)
    int use_cursor;    // add StepState.batch_start even when perm == nullptr
    int C, H, W;
    int bump_adam;     // first kernel of a training step: its designated block starts optimiser step t+1
};

enum EpiKind : int { EPI_PLAIN = 0, EPI_STATS = 1, EPI_MASKSTATS = 2, EPI_SIGMSE = 3, EPI_SIGOUT = 4 };

struct Epi {
    int kind;
    float* out;           // PLAIN/STATS: raw output; MASKSTATS: masked gradient; SIGMSE: dL/d(pre-sigmoid)
    double* stats;        // STATS: [shards][C][4] slots 0,1; MASKSTATS: slots 2,3
    int stats_C;          // channel count of that table
    const float* yprev;   // MASKSTATS: raw forward output at the same element
    const float* target;  // SIGMSE / SIGOUT(optional)
    const int* perm;
    int use_cursor;
    double* losses;       // SIGMSE / SIGOUT: per-slot loss accumulators
    float inv_count;      // 1 / (global_batch * C * H * W)
    double* bias_acc;     // SIGMSE: gradient accumulator of the last layer's bias
    float* yhat;          // SIGOUT: sigmoid output (may be nullptr when only the loss is wanted)
};

struct ConvGeom {
    int B, Cs, Hs, Ws, Cl, Hl, Wl, kh, kw, s;
};

// ---------------------------------------------------------------------------------------------

// Requests every 64-byte line of the kernel's argument block at once, as the kernel's first instructions.  The compiler
// fetches arguments where they are first used: a kernel with a few hundred bytes of them starts with a chain of scalar loads
// from lines nobody has touched yet (the block is rewritten for every launch), each a trip to memory with little else in
// flight - measured on k_head_fwd (1.7 KB of arguments): its first phase 1.7 -> 1.0 us, 1.8 us off the step.
template <int BYTES>
__device__ __forceinline__ void kernarg_warm() {
#if defined(__HIP_DEVICE_COMPILE__)
    const int* ka = (const int*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int kLines = (BYTES + 63) / 64;
    int w[kLines];
#pragma unroll
    for (int i = 0; i < kLines; i++) w[i] = ka[16 * i];
#pragma unroll
    for (int i = 0; i < kLines; i++) asm volatile("" :: "s"(w[i]));
#endif
}

// n / d for 0 <= n < 2^22 and d < 8000 with inv_d = 1.0f / d: (n + 0.5) / d is at least 0.5 / d away from an integer,
// far more than the rounding error of the fp32 product (3 instructions instead of the ~40 of an integer division)
__device__ __forceinline__ int div_small(int n, float inv_d) { return (int)(((float)n + 0.5f) * inv_d); }
constexpr int kDivSmallMaxN = 1 << 22, kDivSmallMaxD = 8000;

// Wave-wide sums with DPP (VALU cross-lane moves) instead of __shfl (ds_bpermute, an LDS-pipe
// instruction with ~50 cycles of latency per step): quad swaps, row mirrors, then the GFX9
// row-broadcasts.  The total lands in lane 63 and is broadcast back with readlane.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true));
}

__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += dpp_f<0xB1>(v);        // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);        // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v);       // row_half_mirror
    v += dpp_f<0x140>(v);       // row_mirror: every lane of a 16-lane row holds the row sum
    v += dpp_f<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
    v += dpp_f<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3: lane 63 holds the wave sum
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// fp64 wave sum on the VALU: both halves of the double travel by DPP (the ds_bpermute butterfly costs ~100 cycles a step)
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_d(double v) {
    const long long bits = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)bits, CTRL, ROW_MASK, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), CTRL, ROW_MASK, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// valid in lane 63 only
__device__ __forceinline__ double wave_sum_lane63(double v) {
    v += dpp_d<0xB1>(v);        // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);        // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v);       // row_half_mirror
    v += dpp_d<0x140>(v);       // row_mirror
    v += dpp_d<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
    v += dpp_d<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
    return v;
}
// valid in every lane
__device__ __forceinline__ double wave_sum(double v) {
    const long long bits = __builtin_bit_cast(long long, wave_sum_lane63(v));
    const int lo = __builtin_amdgcn_readlane((int)bits, 63), hi = __builtin_amdgcn_readlane((int)(bits >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// sum of v over the block, valid in thread 0.  red: LDS scratch of >= blockDim/64 doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; i++) t += red[i];
    }
    return t;
}

// Per-channel constants for a BnDesc into LDS.
//   activation modes: {mean, gamma*invstd, beta, invstd}
//   BN_BWD:           {mean, k1, k2, k3}  with  gy = k1*g - k2 - (y-mean)*k3
// BN_BATCH constants of channel c in two halves, so that a prologue can request the sums before its other loads and
// finish behind them: request = every global read, finish = arithmetic, the LDS entry and (upd) the running statistics.
struct BnBatchReq {
    double2 t[kStatShards];
    float gamma, beta, rm, rv;
};
__device__ __forceinline__ void bn_batch_request(const BnDesc& d, int c, bool upd, BnBatchReq& r) {
    r.gamma = d.gamma[c];
#pragma unroll
    for (int sh = 0; sh < kStatShards; sh++) r.t[sh] = *reinterpret_cast<const double2*>(d.stats + ((size_t)sh * d.C + c) * 4);
    r.beta = d.beta[c];
    r.rm = 0.f;
    r.rv = 0.f;
    if (upd) {
        r.rm = d.rmean[c];
        r.rv = d.rvar[c];
    }
}
__device__ __forceinline__ void bn_batch_finish(const BnDesc& d, int c, bool upd, const BnBatchReq& r, float4* out) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int sh = 0; sh < kStatShards; sh++) {
        s1 += r.t[sh].x;
        s2 += r.t[sh].y;
    }
    // multiplications by host-computed reciprocals and an fp32 square root instead of three fp64 divisions and an fp64
    // square root
    const double m = s1 * d.inv_count;
    double var = s2 * d.inv_count - m * m;
    var = var < 0.0 ? 0.0 : var;
    const float mean = (float)m;
    const float invstd = 1.0f / sqrtf((float)(var + (double)d.eps));
    out[c] = make_float4(mean, r.gamma * invstd, r.beta, invstd);
    if (upd) {
        d.saved[2 * c] = mean;
        d.saved[2 * c + 1] = invstd;
        const double unb = var * d.unbias;
        d.rmean[c] = (1.f - d.momentum) * r.rm + d.momentum * mean;
        d.rvar[c] = (1.f - d.momentum) * r.rv + d.momentum * (float)unb;
    }
}

// BN_BWD constants of channel c in the same two halves (k_adam's per-weight workgroups request them ahead of their operands)
struct BnBwdReq {
    double2 t[kStatShards];
    float gamma, mean, invstd;
};
__device__ __forceinline__ void bn_bwd_request(const BnDesc& d, int c, BnBwdReq& r) {
    r.gamma = d.gamma[c];
#pragma unroll
    for (int sh = 0; sh < kStatShards; sh++) r.t[sh] = *reinterpret_cast<const double2*>(d.stats + ((size_t)sh * d.C + c) * 4 + 2);
    r.mean = d.saved[2 * c];
    r.invstd = d.saved[2 * c + 1];
}
__device__ __forceinline__ float4 bn_bwd_finish(const BnDesc& d, const BnBwdReq& r) {
    double dbeta = 0.0, dgamma = 0.0;
#pragma unroll
    for (int sh = 0; sh < kStatShards; sh++) {
        dbeta += r.t[sh].x;
        dgamma += r.t[sh].y;
    }
    const float scale = r.gamma * r.invstd;
    const float k2 = (float)((double)scale * dbeta * d.inv_count);
    const float k3 = (float)((double)scale * (double)r.invstd * dgamma * d.inv_count);
    return make_float4(r.mean, scale, k2, k3);
}

// `first`: the thread that takes channel 0.  A kernel with two descriptors gives the second one to its second wave
// (first = 64): on one wave the two would be two trips to memory one after the other, the loads of the second behind the
// wait of the first.
__device__ __forceinline__ void bn_consts(const BnDesc& d, float4* out, bool designated, int first = 0) {
    if (d.mode == BN_NONE) return;
    // Every consumer's prologue runs this on its critical path, so within a mode every global read is requested before the
    // first wait and before the first store (a store to memory the reads might alias pins the later reads behind it: the
    // sums, then gamma and beta, then the running statistics used to be three to four trips to memory, one after the other).
    if (first >= (int)blockDim.x) first = 0;
    int c_first = (int)threadIdx.x - first;
    if (c_first < 0) c_first += blockDim.x;
    for (int c = c_first; c < d.C; c += blockDim.x) {
        float mean, invstd;
        if (d.mode == BN_BATCH) {
            const bool upd = designated && d.update;
            BnBatchReq rq;
            bn_batch_request(d, c, upd, rq);
            bn_batch_finish(d, c, upd, rq, out);
            continue;
        }
        if (d.mode == BN_BWD) {
            BnBwdReq rq;
            bn_bwd_request(d, c, rq);
            out[c] = bn_bwd_finish(d, rq);
            continue;
        }
        const float gamma = d.gamma[c];
        if (d.mode == BN_RUNNING) {
            const float beta = d.beta[c];
            mean = d.rmean[c];
            invstd = 1.0f / sqrtf(d.rvar[c] + d.eps);
            out[c] = make_float4(mean, gamma * invstd, beta, invstd);
        } else {   // saved statistics of this step (activation recomputed in the backward pass)
            const float beta = d.beta[c];
            mean = d.saved[2 * c];
            invstd = d.saved[2 * c + 1];
            out[c] = make_float4(mean, gamma * invstd, beta, invstd);
        }
    }
}

__device__ __forceinline__ float bn_apply(int mode, const float4 k, float v, float yraw) {
    if (mode == BN_NONE) return v;
    if (mode == BN_BWD) return k.y * v - k.z - (yraw - k.x) * k.w;
    return fmaxf(0.f, fmaf(v - k.x, k.y, k.z));
}

__device__ __forceinline__ size_t sample_of(const int* perm, int use_cursor, const StepState* st, int b) {
    if (perm) return (size_t)perm[st->batch_start + b];
    if (use_cursor) return (size_t)(st->batch_start + b);
    return (size_t)b;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Where the designated workgroup of a layer's weight-gradient kernel publishes the BatchNorm parameter gradients of the layer
// whose backward this is (dgamma = sum g*xhat, dbeta = sum g), taken from the fp64 stat sums.
struct BnGradOut {
    const double* stats;  // [shards][C][4] of the BN that follows this layer, or nullptr
    double* gamma_acc;
    double* beta_acc;
    int C;
    double scale;  // 1/nranks under SyncBN (the sums are already global), else 1
};

}  // namespace cae
