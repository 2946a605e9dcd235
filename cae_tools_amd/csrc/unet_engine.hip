// unet_engine.hip — host side of the UNET path: tensor table, workspace carving, launch sequence and the
// extern "C" ABI declared in include/cae_unet.h.
//
// Which kernels a layer runs (choose_down / choose_up / choose_wgrad / choose_lin below decide, in this order; unet_debug_plan
// reports their answers):
//   4x4 / s2 / p1 layers with <= 4 channels on the large side (the image end)   kernels_unet_thin.h   (patch in LDS, weights in registers)
//   ... with maps 16 / 32 / 64 / 128 wide and channel counts multiples of 4 / 8   kernels_unet_patch.h  (patch in LDS, weight tiles in LDS)
//   any other 4x4 / s2 / p1 layer                                                 kernels_unet_mfma.h   (im2col tile engine)
//   anything else, and everything when `specialised` is off                      kernels_unet.h        (shape-generic)
//   Linear layers: both sides <= 1024 -> the ConvAE path's 16x16 GEMM (ugemm); batch <= 64 -> kernels_unet_lin.h; else the tile engine.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "cae_unet.h"
#include "engine_host.h"
#include "kernels_unet.h"
#include "kernels_unet_mfma.h"
#include "kernels_unet_lin.h"
#include "kernels_unet_thin.h"
#include "kernels_unet_patch.h"

// The ConvAE path's 16x16-tile MFMA GEMM (kernels_gemm.h: four waves split K, one launch for a Linear layer's weight gradient
// beside its input gradient) for the SMALL Linear layers here (fc -> latent -> fc): the convolution tile engine's strided
// GEMM policy runs such a layer in a single workgroup's chunk loop, 30-40 us for a few hundred kFLOP.  The GEMM header and
// the helpers it uses, and nothing else, inside a namespace of this file: engine.hip's unit defines k_gemm16 / k_gemm16_pair
// too, and the kernels' host stubs must not collide with its.
namespace ugemm {
#include "device_common.h"
#include "kernels_gemm.h"
}  // namespace ugemm

using namespace unet;
using namespace cae_internal;

namespace {

constexpr float kEps = 1e-5f;       // nn.BatchNorm default
constexpr float kMomentum = 0.1f;   // nn.BatchNorm default

// dropout sites (oracle/unet_oracle.py)
constexpr uint32_t SITE_ENC_CONV = 0, SITE_ENC_FC0 = 100, SITE_ENC_FC1 = 101, SITE_DEC_FC0 = 102, SITE_DEC_FC1 = 103,
                   SITE_DEC_CONV = 200;

struct Bn {
    int C = 0;
    int64_t gamma = 0, beta = 0;     // parameter arena
    int64_t rmean = 0, rvar = 0;     // buffer arena
    int64_t saved = 0;               // workspace floats [C][2]
    int64_t sums = 0, bsums = 0;     // workspace doubles [C][2] each (forward / backward)
};

struct ConvLayer {
    Geom g;                          // B filled per call
    int64_t w = 0, b = 0;            // parameter arena
    int64_t wp = -1;                 // workspace: weights repacked per output parity (layers that run OpUp), or -1
    bool has_bn = false, has_skip = false;
    Bn bn;
    int R = 0;                       // attention hidden width
    int64_t w1 = 0, w2 = 0;          // attention weights
    // workspace (float offsets)
    int64_t z = 0, s = 0, a = 0;     // enc: raw conv out, relu(bn), dropout(relu(bn))
    int64_t u = 0, din_next = 0, pool = 0, psum = 0, hid = 0, att = 0, dpool = 0, da = 0;   // dec
    int64_t gz = 0, ga = 0;          // enc grads: g/dz (C,HW), grad wrt a
    int64_t gu = 0, gcat = 0, gdin = 0;   // dec grads: du, g/dcat, grad wrt this layer's input
};

struct Fc {
    int nin = 0, nout = 0;
    int64_t w = 0, b = 0;
    bool has_bn = false;
    Bn bn;
    int64_t h = 0, a = 0;            // raw output, activated (+dropout) output
    int64_t gh = 0, ga = 0;          // grad wrt raw output (in place of ga after activation backward), grad wrt a
};

// A sum table a data-parallel step hands to the caller's all-reduce (unet_engine::tables)
struct SumTable {
    int64_t off = 0, count = 0;    // dsum offset, doubles
    const Bn* fwd = nullptr;       // a forward BatchNorm table: its layer, whose statistics are over HW values per row
    int HW = 0;
};

}  // namespace

struct unet_engine : SteppedCore {   // (ws, stream, max_batch, step, data sets, loss slots, shard: engine_host.h)
    std::vector<ConvLayer> enc, dec;
    Fc fc[4];                        // enc_lin.0, enc_lin.4, dec_lin.0, dec_lin.4
    int fc_size = 0, latent = 0;
    int in_c = 0, in_h = 0, in_w = 0, out_c = 0, out_h = 0, out_w = 0;
    TensorTable tab;
    // workspace
    int64_t off_gacc = 0, off_dsum = 0, n_dsum = 0, off_ls = 0, off_f32 = 0, off_gpart = 0, gpart_bytes = 0;
    int64_t off_thinpart = 0, thinpart_bytes = 0;   // weight-gradient partial tiles: per workgroup (kernels_unet_thin.h), per K slice (tile engine)
    int64_t off_linpart = 0, linpart_bytes = 0;   // K-slice partial tiles of the big Linear layers (kernels_unet_lin.h)
    int64_t off_downpart = 0, downpart_bytes = 0; // partial maps of K slices 1.. of the split-K down convolutions (split_store)
    bool fc_f32[4] = {false, false, false, false};   // this backward stored fc[k]'s weight gradient as fp32 (F32Ranges)
    bool fc_f32_dirty[4] = {false, false, false, false};   // ... and nothing has cleared those accumulator slots since
    int64_t xb = 0, y = 0, coef = 0;
    float *params = nullptr, *m = nullptr, *v = nullptr, *buffers = nullptr;
    Hyper hyper{1e-3, 0.9, 0.999, 1e-8, 1e-5};
    double dropout = 0.1, lambda_p = 1.0;
    uint32_t seed = 0;
    int specialised = 1;
    bool gacc_clean = false;   // the fp64 gradient accumulator is all zero (k_adamw clears what it consumes) but for fc_f32_dirty
    int64_t off_ltot = 0;      // dsum offset of the loss totals {sum mask, sum squared error, sum r} of a data-parallel shard
    // every table a SyncBN step passes to the all-reduce, in the order of include/cae_unet.h: the forward BatchNorm sums, the
    // loss totals, the backward sums (without SyncBN: the loss totals alone).  sync_table checks each call against it.
    std::vector<SumTable> tables;
    size_t table_pos = 0;      // the next entry of `tables` in the current step

    float* f(int64_t off) const { return reinterpret_cast<float*>(ws + off_f32) + off; }
    double* dsum(int64_t off) const { return reinterpret_cast<double*>(ws + off_dsum) + off; }
    double* gacc(int64_t off) const { return reinterpret_cast<double*>(ws + off_gacc) + off; }
    float* downpart() const { return reinterpret_cast<float*>(ws + off_downpart); }
    float* P(int64_t off) const { return params + off; }
    float* Bf(int64_t off) const { return buffers + off; }
};

namespace {

void add_bn(unet_engine* e, const std::string& key, int C, Bn& bn) {
    bn.C = C;
    bn.gamma = e->tab.add(key + ".weight", 0, {C});
    bn.beta = e->tab.add(key + ".bias", 0, {C});
    bn.rmean = e->tab.add(key + ".running_mean", 1, {C});
    bn.rvar = e->tab.add(key + ".running_var", 1, {C});
}

// per_sample: the site's elements per sample (a shard's masks are those of its rows in the global batch)
Drop make_drop(const unet_engine* e, uint32_t site, bool train, int64_t per_sample) {
    Drop d{0, 0, 1.f, 0, 0};
    if (!train || e->dropout <= 0.0) return d;
    d.on = 1;
    d.base = (unsigned long long)((int64_t)e->shard.row0 * per_sample);
    const uint32_t k = pcg(e->seed + 0x9E3779B9u * site);
    d.key = pcg(k ^ (uint32_t)(e->step & 0xFFFFFFFF));
    double t = e->dropout * 4294967296.0;
    d.thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    d.scale = (float)(1.0 / (1.0 - e->dropout));
    return d;
}

// ---- conv dispatch --------------------------------------------------------------------------------
// The choosers below are the whole decision: the launch code switches on what they return and unet_debug_plan reports it.
enum DownK { DOWN_THIN, DOWN_PATCH, DOWN_MFMA, DOWN_GENERIC };
enum UpK { UP_THIN, UP_THIN_CL, UP_PATCH, UP_MFMA, UP_GENERIC };
// *_ATOMIC: the same kernel family with fp64 atomics from every workgroup instead of partial tiles folded in order
enum WgradK { WG_THIN, WG_THIN_ATOMIC, WG_PATCH, WG_MFMA, WG_MFMA_ATOMIC, WG_GENERIC };
enum LinK { LIN_BIG, LIN_GEMM16, LIN_TILE, LIN_GENERIC };

const char* const kDownName[] = {"thin", "patch", "mfma", "generic"};
const char* const kUpName[] = {"thin", "up_thin", "patch", "mfma", "generic"};
const char* const kWgradName[] = {"thin", "thin_atomic", "patch", "mfma", "mfma_atomic", "generic"};
const char* const kLinName[] = {"lin_big", "gemm16", "tile", "generic"};

DownK choose_down(const unet_engine* e, const Geom& g) {
    if (e->specialised && thin_geom(g)) return DOWN_THIN;       // the image-end layers: kernels_unet_thin.h
    if (e->specialised && patch_geom(g)) return DOWN_PATCH;     // the wide layers: kernels_unet_patch.h
    if (e->specialised && mfma_down_eligible(g)) return DOWN_MFMA;
    return DOWN_GENERIC;
}

// has_wp: the layer has repacked weights (pack_up_weights below); the thin, patch and tile-engine kernels read only those
UpK choose_up(const unet_engine* e, const Geom& g, bool has_wp) {
    if (e->specialised && has_wp && thin_up_geom(g)) return UP_THIN;   // ... 128 columns wide: kernels_unet_thin.h
    if (e->specialised && mfma_geom(g) && g.Cl <= 4) return UP_THIN_CL;   // a handful of output channels: streaming, not a GEMM
    if (e->specialised && has_wp && g.Cl > 4 && pup_geom(g)) return UP_PATCH;   // the wide layers
    if (e->specialised && has_wp && mfma_up_eligible(g)) return UP_MFMA;
    return UP_GENERIC;
}

WgradK choose_wgrad(const unet_engine* e, const Geom& g) {
    if (e->specialised && thin_geom(g))   // the image-end layers: kernels_unet_thin.h
        return thin_wgrad_part_bytes(g) <= (size_t)e->thinpart_bytes ? WG_THIN : WG_THIN_ATOMIC;
    if (e->specialised && pwgrad_geom(g) && pwgrad_part_bytes(g) <= (size_t)e->thinpart_bytes) return WG_PATCH;
    if (e->specialised && mfma_wgrad_eligible(g)) {
        const size_t need = mfma_wgrad_part_bytes(g);
        return (need && need <= (size_t)e->thinpart_bytes) ? WG_MFMA : WG_MFMA_ATOMIC;
    }
    return WG_GENERIC;
}

void conv_down(unet_engine* e, const Geom& g, const float* L, const float* w, const float* bias, float* S) {
    switch (choose_down(e, g)) {
        case DOWN_THIN: thin_down_launch(g, L, w, bias, S, e->stream); return;
        case DOWN_PATCH: pdown_launch(g, L, w, bias, S, e->downpart(), e->downpart_bytes, e->stream); return;
        case DOWN_MFMA: mfma_down_launch(g, L, w, bias, S, e->downpart(), e->downpart_bytes, e->stream); return;
        case DOWN_GENERIC: break;
    }
    const long long total = (long long)g.B * g.Cs * g.Hs * g.Ws;
    hipLaunchKernelGGL(k_down, dim3(blocks_for(total, 65536)), dim3(256), 0, e->stream, g, L, w, bias, S);
}

// wp: the layer's repacked weights (pack_up_weights below) or nullptr when the layer does not run the tile engine
void conv_up(unet_engine* e, const Geom& g, const float* S, const float* w, const float* wp, const float* bias, float* L) {
    switch (choose_up(e, g, wp != nullptr)) {
        case UP_THIN: thin_up_launch(g, S, wp, bias, L, e->stream); return;
        case UP_THIN_CL: {
            const int blocks = blocks_for((long long)g.B * g.Hs * g.Ws, 65536);
            switch (thin_cl(g)) {
                case 1: hipLaunchKernelGGL(k_up_thin<1>, dim3(blocks), dim3(256), 0, e->stream, g, S, w, bias, L); break;
                case 2: hipLaunchKernelGGL(k_up_thin<2>, dim3(blocks), dim3(256), 0, e->stream, g, S, w, bias, L); break;
                case 3: hipLaunchKernelGGL(k_up_thin<3>, dim3(blocks), dim3(256), 0, e->stream, g, S, w, bias, L); break;
                default: hipLaunchKernelGGL(k_up_thin<4>, dim3(blocks), dim3(256), 0, e->stream, g, S, w, bias, L); break;
            }
            return;
        }
        case UP_PATCH: pup_launch(g, S, wp, bias, L, e->stream); return;
        case UP_MFMA: mfma_up_launch(g, S, wp, bias, L, e->stream); return;
        case UP_GENERIC: break;
    }
    const long long total = (long long)g.B * g.Cl * g.Hl * g.Wl;
    hipLaunchKernelGGL(k_up, dim3(blocks_for(total, 65536)), dim3(256), 0, e->stream, g, S, w, bias, L);
}

void conv_wgrad(unet_engine* e, const Geom& g, const float* S, const float* L, double* acc) {
    float* part = reinterpret_cast<float*>(e->ws + e->off_thinpart);
    switch (choose_wgrad(e, g)) {
        case WG_THIN: thin_wgrad_launch(g, S, L, acc, part, e->stream); return;
        case WG_THIN_ATOMIC: thin_wgrad_launch(g, S, L, acc, nullptr, e->stream); return;
        case WG_PATCH: pwgrad_launch(g, S, L, acc, part, e->stream); return;
        case WG_MFMA: mfma_wgrad_launch(g, S, L, acc, part, e->stream); return;
        case WG_MFMA_ATOMIC: mfma_wgrad_launch(g, S, L, acc, nullptr, e->stream); return;
        case WG_GENERIC: break;
    }
    const long long per = (long long)g.B * g.Hs * g.Ws;
    int split = (int)((per + 256 * 16 - 1) / (256 * 16));
    if (split > 16) split = 16;
    if (split < 1) split = 1;
    hipLaunchKernelGGL(k_wgrad, dim3(g.Cs * g.Cl * g.kh * g.kw, split), dim3(256), 0, e->stream, g, S, L, acc);
}

// kernels that end in a workgroup-wide sum + atomics: fewer, longer workgroups (the sum's two barriers and the atomics are a
// fixed 2-3 us; at 128 chunks a workgroup of the 128 x 128 maps had four loop trips of work in front of them)
constexpr int kRedWgs = 1280;

dim3 red_grid(int B, int C, int HW) {
    int chunks = (int)(((long long)B * HW + 256 * 4 - 1) / (256 * 4));
    const int want = std::max(4, kRedWgs / std::max(1, C));     // about kRedWgs workgroups over the C channels
    if (chunks > want) chunks = want;
    if (chunks < 1) chunks = 1;
    return dim3(chunks, C);
}

void chan_sums(unet_engine* e, const float* x, long long bs, int B, int C, int HW, double* sums, int sstride, int want_sq) {
    const int chunks = (int)red_grid(B, C, HW).x;
    hipLaunchKernelGGL(k_chan_sums<ACC_STAT>, dim3(chunks, C), dim3(256), 0, e->stream, x, bs, B, HW, sums, sstride, want_sq);
}

dim3 ew_grid(int B, int C, int HW) {
    int chunks = (int)(((long long)B * HW + 256 * 4 - 1) / (256 * 4));
    if (chunks > 128) chunks = 128;
    if (chunks < 1) chunks = 1;
    return dim3(chunks, C);
}

// accumulate the batch sums of x (B,C,HW; batch stride bs); bn_act turns them into statistics
void bn_stats(unet_engine* e, const Bn& bn, const float* x, long long bs, int B, int HW) {
    chan_sums(e, x, bs, B, bn.C, HW, e->dsum(bn.sums), 2, 1);
}

const ZCat kNoCat{nullptr, nullptr, nullptr, 0};

// values per channel behind a BatchNorm's statistics
double bn_count(const unet_engine* e, int B, int HW) { return (double)e->shard.stat_rows(B) * HW; }

// the completed sum table at dsum offset `off` to the caller's all-reduce, when this is a data-parallel call that sums it: every
// table under SyncBN, each in its place in e->tables (the ranks' collectives must match), else the loss totals alone
int sync_table(unet_engine* e, int64_t off) {
    if (!e->shard.fn) return CAE_OK;
    int64_t count = 3;   // (the loss totals)
    if (e->shard.sync_bn()) {
        if (e->table_pos >= e->tables.size() || e->tables[e->table_pos].off != off)
            return fail(CAE_ERR_STATE, "unet: sum table at %lld passed out of order (position %zu of %zu)", (long long)off,
                        e->table_pos, e->tables.size());
        count = e->tables[e->table_pos++].count;
    } else if (off != e->off_ltot) {
        return CAE_OK;
    }
    return call_allreduce(e->shard, "unet", e->dsum(off), count);
}

// skip_sums: where the sums of the ReLU output go (the skip half of a decoder layer's BatchNorm statistics), or nullptr
void bn_act(unet_engine* e, const Bn& bn, const float* z, long long zbs, int B, int HW, bool train, Drop d, float* s_out,
            float* a_out, const ZCat& zc = kNoCat, double* skip_sums = nullptr) {
    // (with sums to leave, fewer and longer workgroups: red_grid)
    hipLaunchKernelGGL(k_bn_act, skip_sums ? red_grid(B, bn.C, HW) : ew_grid(B, bn.C, HW), dim3(256), 0, e->stream, z, zbs, B, bn.C, HW,
                       e->f(bn.saved), e->Bf(bn.rmean), e->Bf(bn.rvar), kEps, train ? 2 : 1, e->dsum(bn.sums), bn_count(e, B, HW), kMomentum,
                       e->P(bn.gamma), e->P(bn.beta), d, s_out, a_out, zc, skip_sums);
}

// between the two passes of a BatchNorm backward: the accumulators pass 2 adds dgamma / dbeta to.  Under SyncBN the pass-1
// sums are all-reduced here; this shard's dgamma / dbeta are taken from them before (k_bn_grad_local) and pass 2 adds none.
int bn_bwd_between(unet_engine* e, const Bn& bn, double*& acc_gamma, double*& acc_beta) {
    acc_gamma = e->gacc(bn.gamma), acc_beta = e->gacc(bn.beta);
    if (!e->shard.sync_bn()) return CAE_OK;
    hipLaunchKernelGGL(k_bn_grad_local, dim3((bn.C + 255) / 256), dim3(256), 0, e->stream, e->dsum(bn.bsums), bn.C, acc_gamma, acc_beta);
    acc_gamma = acc_beta = nullptr;
    return sync_table(e, bn.bsums);
}

int bn_backward(unet_engine* e, const Bn& bn, const float* gA, long long gAbs, const float* gB, long long gBbs,
                const float* z, long long zbs, int B, int HW, Drop d, float* g_io, const ZCat& zc = kNoCat) {
    // pass 1 only sums; pass 2 forms the masked gradient again from gA / gB / z and writes dz (g_io may alias neither input:
    // the callers pass distinct buffers)
    hipLaunchKernelGGL(k_bn_bwd_reduce, red_grid(B, bn.C, HW), dim3(256), 0, e->stream, gA, gAbs, gB, gBbs, z, zbs, B, bn.C,
                       HW, e->f(bn.saved), e->P(bn.gamma), e->P(bn.beta), d, (float*)nullptr, e->dsum(bn.bsums), zc);
    double *acc_gamma, *acc_beta;
    if (int rc = bn_bwd_between(e, bn, acc_gamma, acc_beta)) return rc;
    hipLaunchKernelGGL(k_bn_bwd_apply2, ew_grid(B, bn.C, HW), dim3(256), 0, e->stream, gA, gAbs, gB, gBbs, z, zbs, B, bn.C, HW,
                       e->f(bn.saved), e->P(bn.gamma), e->P(bn.beta), d, e->dsum(bn.bsums), bn_count(e, B, HW), acc_gamma,
                       acc_beta, g_io, zc);
    return CAE_OK;
}

// small Linear layers: the whole weight matrix is a few 16x16 tiles' worth (see the include of kernels_gemm.h above)
// (both sides <= 1024: the 16x16-tile kernel sums K in four fp32 chains of K / 4, fine for a few hundred terms; a K = 6144
// layer on it put the gradients behind a five-row BatchNorm1d 2-5 % from the oracle where the tile engine's 256-long chains
// with an fp64 combine stay within 1.5 % - tests/test_unet_hip_parity.py)
bool small_fc(const Fc& L) { return L.nin <= 1024 && L.nout <= 1024; }
size_t gemm16_lds() { return (4 * 256 + 256) * sizeof(float) + sizeof(float4); }

ugemm::cae::GemmArgs gemm16_args(int M, int N, int K) {
    ugemm::cae::GemmArgs g;
    memset(&g, 0, sizeof g);
    g.M = M, g.N = N, g.K = K;
    return g;
}

// the big layers on kernels_unet_lin.h: batch <= 64, 16-byte rows, room for the K slices' partial tiles
bool lin_big(const unet_engine* e, const Fc& L, int B) {
    if (!e->specialised || small_fc(L) || B > 64 || (L.nin & 3) || (L.nout & 3)) return false;
    const long long need = (long long)std::max((L.nin + 127) / 128 * (long long)L.nout, (L.nout + 127) / 128 * (long long)L.nin) * B * 4;
    return need <= e->linpart_bytes;
}

// what lin_gemm runs for a batch of B rows and a sum over K: row blocks of 32 batch rows (RB), tiles of kLinKT per workgroup,
// K slices (more than one: partial tiles and k_lin_fold) and whether the last tile of K is partly filled (zero fill of k >= K).
// lin_gemm launches from this; unet_debug_plan prints it
struct LinGemmPlan {
    int rb, kiters, slices;
    bool partial;
};
LinGemmPlan lin_gemm_plan(int B, int K) {
    LinGemmPlan p;
    p.kiters = 2;
    p.slices = (K + p.kiters * kLinKT - 1) / (p.kiters * kLinKT);
    p.rb = B > 32 ? 2 : 1;
    p.partial = K % kLinKT != 0;
    return p;
}
// dynamic LDS of k_lin_outer at this batch: above 64 KiB (batch > 56) lin_bwd raises the kernel's limit first
size_t lin_outer_lds(int B) { return (size_t)2 * ((B + 7) & ~7) * kLinPN * sizeof(float); }

// Y[b][n] = bias[n] + sum_k X[b][k] W[..]: nt = W[n][k] (forward), else W[k][n] (input gradient)
void lin_gemm(unet_engine* e, bool nt, const float* X, long long x_ld, const float* W, long long w_ld, const float* bias, float* Y,
              int B, int N, int K) {
    const LinGemmPlan pl = lin_gemm_plan(B, K);
    LinArgs a;
    a.X = X, a.x_ld = x_ld, a.W = W, a.w_ld = w_ld, a.bias = bias, a.Y = Y, a.y_ld = N, a.B = B, a.N = N, a.K = K, a.kiters = pl.kiters;
    const int slices = pl.slices;
    a.part = slices > 1 ? reinterpret_cast<float*>(e->ws + e->off_linpart) : nullptr;
    const dim3 grid((N + kLinNT - 1) / kLinNT, slices);
    const int RB = pl.rb;
    if (nt) {
        const size_t lds = (size_t)(32 * RB + 128) * kLinPK * sizeof(float);
        if (RB == 1) hipLaunchKernelGGL(k_lin_nt<1>, grid, dim3(256), lds, e->stream, a);
        else hipLaunchKernelGGL(k_lin_nt<2>, grid, dim3(256), lds, e->stream, a);
    } else {
        const size_t lds = (size_t)(32 * RB * kLinPK + kLinKT * kLinPN) * sizeof(float);
        if (RB == 1) hipLaunchKernelGGL(k_lin_nn<1>, grid, dim3(256), lds, e->stream, a);
        else hipLaunchKernelGGL(k_lin_nn<2>, grid, dim3(256), lds, e->stream, a);
    }
    if (slices > 1)
        hipLaunchKernelGGL(k_lin_fold, dim3((unsigned)(((long long)B * N + 15) / 16)), dim3(256), 0, e->stream, a.part, slices, B, N, bias,
                           Y, (long long)N);
}

// (forward and backward of a Linear layer take the same family)
LinK choose_lin(const unet_engine* e, const Fc& L, int B) {
    if (lin_big(e, L, B)) return LIN_BIG;
    if (e->specialised && small_fc(L)) return LIN_GEMM16;
    if (e->specialised) return LIN_TILE;
    return LIN_GENERIC;
}

void lin_fwd(unet_engine* e, const Fc& L, int B, const float* in, float* out) {
    switch (choose_lin(e, L, B)) {
        case LIN_BIG:   // out[b][o] = bias[o] + sum_i in[b][i] W[o][i]
            lin_gemm(e, true, in, L.nin, e->P(L.w), L.nin, e->P(L.b), out, B, L.nout, L.nin);
            return;
        case LIN_GEMM16: {   // out[b][o] = bias[o] + sum_i in[b][i] W[o][i]
            ugemm::cae::GemmArgs ga = gemm16_args(B, L.nout, L.nin);
            ga.A = in, ga.sa_m = L.nin, ga.sa_k = 1;
            ga.B = e->P(L.w), ga.sb_k = 1, ga.sb_n = L.nin;           // B[k][n] = W[n][k]
            ga.C = out, ga.sc_m = L.nout, ga.sc_n = 1;
            ga.epi = ugemm::cae::GE_STORE;
            ga.bias = e->P(L.b);
            const int tiles = ((B + 15) / 16) * ((L.nout + 15) / 16);
            hipLaunchKernelGGL(ugemm::cae::k_gemm16, dim3(tiles), dim3(256), gemm16_lds(), e->stream, ga);
            return;
        }
        case LIN_TILE: {   // out[b][o] = bias[o] + sum_i in[b][i] W[o][i]
            GemmDesc d{L.nout, B, L.nin, e->P(L.w), L.nin, 1, in, 1, L.nin, e->P(L.b), out, nullptr, 1, L.nout, 0};
            gemm_launch(d, reinterpret_cast<float*>(e->ws + e->off_gpart), e->gpart_bytes, e->stream);
            return;
        }
        case LIN_GENERIC: break;
    }
    hipLaunchKernelGGL(k_lin_fwd, dim3(L.nout, (B + 7) / 8), dim3(256), 0, e->stream, B, L.nin, L.nout, in, e->P(L.w),
                       e->P(L.b), out);
}

void lin_bwd(unet_engine* e, const Fc& L, int B, const float* in, const float* gout, float* gin) {
    const int fk = (int)(&L - e->fc);
    const LinK k = choose_lin(e, L, B);
    const bool big = k == LIN_BIG;
    if (!big && e->fc_f32_dirty[fk]) {   // an earlier step left fp32 gradients in these fp64 slots
        (void)hipMemsetAsync(e->gacc(L.w), 0, (size_t)L.nin * L.nout * sizeof(double), e->stream);
        e->fc_f32_dirty[fk] = false;
    }
    e->fc_f32[fk] = big;
    switch (k) {
        case LIN_BIG: {
            // dW[o][i] = sum_b gout[b][o] in[b][i] as fp32 in the first half of the weight's accumulator slots (F32Ranges),
            // db[o] = sum_b gout[b][o];  gin[b][i] = sum_o gout[b][o] W[o][i]
            e->fc_f32_dirty[fk] = true;
            const size_t lds = lin_outer_lds(B);
            static bool raised = false;   // above the 64 KiB a kernel gets without asking (batch > 56)
            if (lds > 65536 && !raised) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lin_outer), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * kLinPN * 4);
                raised = true;
            }
            hipLaunchKernelGGL(k_lin_outer, dim3((L.nin + 127) / 128, (L.nout + 127) / 128), dim3(256), lds, e->stream, gout, (long long)L.nout, in,
                               (long long)L.nin, B, L.nout, L.nin, reinterpret_cast<float*>(e->gacc(L.w)), e->gacc(L.b));
            if (gin) lin_gemm(e, false, gout, L.nout, e->P(L.w), L.nin, nullptr, gin, B, L.nin, L.nout);
            return;
        }
        case LIN_GEMM16: {
            // dW[o][i] = sum_b gout[b][o] in[b][i], db[o] = sum_b gout[b][o] (a ones column), K = the whole batch in one tile: plain
            // fp64 stores into the (zeroed) accumulator, one writer per element; beside it gin[b][i] = sum_o gout[b][o] W[o][i]
            ugemm::cae::GemmArgs gw = gemm16_args(L.nout, L.nin + 1, B);
            gw.A = gout, gw.sa_m = 1, gw.sa_k = L.nout;
            gw.B = in, gw.sb_k = L.nin, gw.sb_n = 1;
            gw.epi = ugemm::cae::GE_ACC64;
            gw.accW = e->gacc(L.w), gw.accB = e->gacc(L.b), gw.ones_col = 1;
            const int tiles_w = ((gw.M + 15) / 16) * ((gw.N + 15) / 16);
            if (!gin) {
                hipLaunchKernelGGL(ugemm::cae::k_gemm16, dim3(tiles_w), dim3(256), gemm16_lds(), e->stream, gw);
                return;
            }
            ugemm::cae::GemmArgs gd = gemm16_args(B, L.nin, L.nout);
            gd.A = gout, gd.sa_m = L.nout, gd.sa_k = 1;
            gd.B = e->P(L.w), gd.sb_k = L.nin, gd.sb_n = 1;           // B[k = o][n = i] = W[o][i]
            gd.C = gin, gd.sc_m = L.nin, gd.sc_n = 1;
            gd.epi = ugemm::cae::GE_STORE;
            const int tiles_d = ((gd.M + 15) / 16) * ((gd.N + 15) / 16);
            hipLaunchKernelGGL(ugemm::cae::k_gemm16_pair, dim3(tiles_w + tiles_d), dim3(256), gemm16_lds(), e->stream, gw, gd, tiles_w, 0,
                               ugemm::cae::WFold{});
            return;
        }
        case LIN_TILE: {
            // dW[o][i] += sum_b gout[b][o] in[b][i];  db[o] += sum_b gout[b][o];  gin[b][i] = sum_o gout[b][o] W[o][i]
            GemmDesc w{L.nout, L.nin, B, gout, 1, L.nout, in, L.nin, 1, nullptr, nullptr, e->gacc(L.w), L.nin, 1, 2};
            gemm_launch(w, nullptr, 0, e->stream);
            hipLaunchKernelGGL(k_col_sums, dim3((L.nout + 255) / 256), dim3(256), 0, e->stream, B, L.nout, gout, e->gacc(L.b));
            if (gin) {
                GemmDesc d{L.nin, B, L.nout, e->P(L.w), 1, L.nin, gout, 1, L.nout, nullptr, gin, nullptr, 1, L.nin, 0};
                gemm_launch(d, reinterpret_cast<float*>(e->ws + e->off_gpart), e->gpart_bytes, e->stream);
            }
            return;
        }
        case LIN_GENERIC: break;
    }
    hipLaunchKernelGGL(k_lin_wgrad, dim3(blocks_for((long long)L.nout * L.nin, 65536)), dim3(256), 0, e->stream, B, L.nin,
                       L.nout, gout, in, e->gacc(L.w), e->gacc(L.b));
    if (gin)
        hipLaunchKernelGGL(k_lin_dgrad, dim3(blocks_for((long long)B * L.nin, 65536)), dim3(256), 0, e->stream, B, L.nin,
                           L.nout, gout, e->P(L.w), gin);
}

// the layers whose weights pack_up_weights repacks: every layer with a repack buffer that runs OpUp in this mode (decoder
// forward; encoder input gradients when training), in launch order
std::vector<const ConvLayer*> pack_list(const unet_engine* e, bool train) {
    std::vector<const ConvLayer*> v;
    if (!e->specialised) return v;
    for (auto& L : e->dec)
        if (L.wp >= 0) v.push_back(&L);
    if (train)
        for (size_t i = 1; i < e->enc.size(); i++)
            if (e->enc[i].wp >= 0) v.push_back(&e->enc[i]);
    return v;
}
constexpr int kPackPer = (int)(sizeof(PackSet::Cs) / sizeof(int));   // entries one k_pack_up_weights launch takes
int pack_launches(size_t entries) { return (int)((entries + kPackPer - 1) / kPackPer); }

// ... repacked in one launch per kPackPer of them (one launch up to cfg3's seven)
void pack_up_weights(unet_engine* e, bool train) {
    const std::vector<const ConvLayer*> layers = pack_list(e, train);
    for (size_t first = 0; first < layers.size(); first += kPackPer) {
        PackSet ps;
        memset(&ps, 0, sizeof ps);
        for (size_t k = first; k < layers.size() && ps.n < kPackPer; k++) {
            const ConvLayer& L = *layers[k];
            ps.thin[ps.n] = L.g.Cl <= 4;                           // (the image-end layer: k_thin_up's order)
            ps.Cs[ps.n] = L.g.Cs, ps.Cl[ps.n] = L.g.Cl, ps.w[ps.n] = e->P(L.w), ps.wp[ps.n] = e->f(L.wp);
            ps.begin[ps.n + 1] = ps.begin[ps.n] + (long long)16 * L.g.Cs * L.g.Cl;
            ps.n++;
        }
        hipLaunchKernelGGL(k_pack_up_weights, dim3(blocks_for(ps.begin[ps.n], 2048)), dim3(256), 0, e->stream, ps);
    }
}

// ---- forward ----------------------------------------------------------------------------------------
// x: (B, in_c, in_h, in_w) contiguous.  Leaves the raw last-layer output in dec.back().u
int forward(unet_engine* e, const float* x, int B, bool train) {
    const int n = (int)e->enc.size();
    if (train) HIP_TRY(hipMemsetAsync(e->dsum(0), 0, (size_t)e->n_dsum * sizeof(double), e->stream));
    pack_up_weights(e, train);
    const float* cur = x;
    for (int i = 0; i < n; i++) {
        ConvLayer& L = e->enc[i];
        Geom g = L.g;
        g.B = B;
        const int HW = g.Hs * g.Ws;
        conv_down(e, g, cur, e->P(L.w), e->P(L.b), e->f(L.z));
        if (train) {
            bn_stats(e, L.bn, e->f(L.z), (long long)g.Cs * HW, B, HW);
            if (int rc = sync_table(e, L.bn.sums)) return rc;
        }
        const Drop d = make_drop(e, SITE_ENC_CONV + i, train, (int64_t)g.Cs * HW);
        // the skip is the ReLU output; the next layer sees it through the dropout (unet.py:105-107)
        // (a skip's sums are the second half of its decoder layer's BatchNorm statistics: dec[n - 2 - i], channels Cs ..)
        double* skip_sums = (train && i < n - 1) ? e->dsum(e->dec[n - 2 - i].bn.sums) + 2 * g.Cs : nullptr;
        bn_act(e, L.bn, e->f(L.z), (long long)g.Cs * HW, B, HW, train, d, e->f(L.s), d.on ? e->f(L.a) : nullptr, kNoCat, skip_sums);
        cur = d.on ? e->f(L.a) : e->f(L.s);
    }
    // encoder_lin / decoder_lin: Linear, BN1d, ReLU, Dropout, Linear, ReLU, Dropout (unet.py:92-100,121-129)
    const uint32_t sites[4] = {SITE_ENC_FC0, SITE_ENC_FC1, SITE_DEC_FC0, SITE_DEC_FC1};
    for (int k = 0; k < 4; k++) {
        Fc& L = e->fc[k];
        lin_fwd(e, L, B, cur, e->f(L.h));
        const Drop d = make_drop(e, sites[k], train, L.nout);
        if (L.has_bn) {
            if (train) {
                bn_stats(e, L.bn, e->f(L.h), L.nout, B, 1);
                if (int rc = sync_table(e, L.bn.sums)) return rc;
            }
            bn_act(e, L.bn, e->f(L.h), L.nout, B, 1, train, d, nullptr, e->f(L.a));
        } else {
            hipLaunchKernelGGL(k_relu_drop, dim3(blocks_for((long long)B * L.nout, 8192)), dim3(256), 0, e->stream, e->f(L.h),
                               (long long)B * L.nout, d, e->f(L.a));
        }
        cur = e->f(L.a);
    }
    const int nd = (int)e->dec.size();
    for (int j = 0; j < nd; j++) {
        ConvLayer& L = e->dec[j];
        Geom g = L.g;
        g.B = B;
        const int HW = g.Hl * g.Wl, C = g.Cl;
        conv_up(e, g, cur, e->P(L.w), L.wp >= 0 ? e->f(L.wp) : nullptr, e->P(L.b), e->f(L.u));
        if (!L.has_bn) break;   // last layer: sigmoid is applied by the loss / score kernels
        const float* skip = e->f(e->enc[n - 2 - j].s);
        // the concatenated tensor (gated u | skip) is never written, and in training nothing reads its sources again for the
        // BatchNorm statistics: the pooling pass leaves sum u and sum u^2 per (b, c), the gate kernel scales them by att and
        // att^2, and the skip half's sums came with the encoder's BatchNorm + ReLU pass
        double* psum = reinterpret_cast<double*>(e->f(L.psum));
        hipLaunchKernelGGL(k_pool, dim3(B * C), dim3(256), 0, e->stream, e->f(L.u), HW, e->f(L.pool), train ? psum : nullptr);
        hipLaunchKernelGGL(k_att_fwd, dim3(B), dim3(256), (size_t)(2 * C + 2 * L.R) * sizeof(float), e->stream, e->f(L.pool),
                           C, L.R, e->P(L.w1), e->P(L.w2), e->f(L.att), e->f(L.hid), psum, train ? e->dsum(L.bn.sums) : nullptr);
        // (both halves of the concatenated tensor's sums are in by now: the skip's came with the encoder's bn_act)
        if (train)
            if (int rc = sync_table(e, L.bn.sums)) return rc;
        const Drop d = make_drop(e, SITE_DEC_CONV + j, train, (int64_t)2 * C * HW);
        bn_act(e, L.bn, nullptr, 0, B, HW, train, d, nullptr, e->f(L.din_next), ZCat{e->f(L.u), e->f(L.att), skip, C});
        cur = e->f(L.din_next);
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

LossSrc loss_src(const unet_engine* e, int which, const int32_t* perm, int64_t start) {
    LossSrc s;
    s.target = e->ds[which].t;
    s.mask = e->ds[which].m;
    s.perm = perm;
    s.start = start;
    s.Cm = e->ds[which].m ? e->ds[which].mc : e->out_c;
    return s;
}

int loss_forward(unet_engine* e, int which, const int32_t* perm, int64_t start, int B, int slot, bool want_grad) {
    const ConvLayer& L = e->dec.back();
    const int C = e->out_c, HW = e->out_h * e->out_w;
    double* ls = reinterpret_cast<double*>(e->ws + e->off_ls);
    HIP_TRY(hipMemsetAsync(ls, 0, (size_t)B * C * 8 * sizeof(double), e->stream));
    const LossSrc src = loss_src(e, which, perm, start);
    // (seven workgroup-wide fp64 sums end every workgroup: about 768 of them, each a long slice of its plane)
    int chunks = std::max(1, std::min(32, 768 / std::max(1, B * C)));
    chunks = std::min(chunks, (HW + 1023) / 1024);
    if (B > 0) hipLaunchKernelGGL(k_loss_sums, dim3(chunks, B * C), dim3(256), 0, e->stream, e->f(L.u), 1, src, C, HW, ls);
    if (e->shard.fn) {   // a data-parallel shard: the mask count, squared error and Pearson sum are totals over the ranks
        double* tot = e->dsum(e->off_ltot);
        hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, e->stream, ls, B, C, src.Cm, src.mask ? 1 : 0, tot);
        if (int rc = sync_table(e, e->off_ltot)) return rc;
        hipLaunchKernelGGL(k_loss_finalize_global, dim3(1), dim3(256), 0, e->stream, ls, B, C, tot, (double)e->shard.global_batch * C,
                           e->lambda_p, e->losses(slot), want_grad ? e->f(e->coef) : nullptr);
    } else {
        hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(256), 0, e->stream, ls, B, C, src.Cm, src.mask ? 1 : 0, e->lambda_p,
                           e->losses(slot), want_grad ? e->f(e->coef) : nullptr);
    }
    if (want_grad) {
        // ... and, in the same pass, the last layer's bias gradient (its sum over the batch and the map); backward() clears the
        // accumulator before anything else adds to it, so the clear is issued here, ahead of this launch
        if (!e->gacc_clean) {
            HIP_TRY(hipMemsetAsync(e->gacc(0), 0, (size_t)e->tab.n_param * sizeof(double), e->stream));
            for (int k = 0; k < 4; k++) e->fc_f32_dirty[k] = false;
            e->gacc_clean = true;
        }
        int chunks = std::max(1, std::min(64, 1536 / std::max(1, B * C)));
        chunks = std::min(chunks, (HW + 1023) / 1024);
        hipLaunchKernelGGL(k_loss_grad, dim3(std::max(1, chunks), B * C), dim3(256), 0, e->stream, e->f(L.u), src, B, C, HW, e->f(e->coef),
                           e->f(L.gu), e->gacc(L.b));
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- backward ---------------------------------------------------------------------------------------
int backward(unet_engine* e, const float* x, int B) {
    const int n = (int)e->enc.size(), nd = (int)e->dec.size();
    if (!e->gacc_clean) {
        HIP_TRY(hipMemsetAsync(e->gacc(0), 0, (size_t)e->tab.n_param * sizeof(double), e->stream));
        for (int k = 0; k < 4; k++) e->fc_f32_dirty[k] = false;
    }
    e->gacc_clean = false;
    for (int j = nd - 1; j >= 0; j--) {
        ConvLayer& L = e->dec[j];
        Geom g = L.g;
        g.B = B;
        const int HWl = g.Hl * g.Wl, C = g.Cl;
        const float* din = j == 0 ? e->f(e->fc[3].a) : e->f(e->dec[j - 1].din_next);
        // ConvTranspose2d: S = input, L = output
        conv_wgrad(e, g, din, e->f(L.gu), e->gacc(L.w));
        // bias gradient: summed by k_scale_bwd when it produced gu, and by the loss kernel for the last layer
        conv_down(e, g, e->f(L.gu), e->P(L.w), nullptr, e->f(L.gdin));
        if (j == 0) break;
        // gdin is the gradient wrt dropout(relu(bn(cat_{j-1})))
        ConvLayer& Pv = e->dec[j - 1];
        const int Cp = Pv.g.Cl, HWp = Pv.g.Hl * Pv.g.Wl;
        // BatchNorm + ReLU + dropout backward over the (never written) concatenated tensor: pass 1 sums; pass 2, one workgroup per
        // (b, c) plane, writes dz and - for the gated half - the gate's gradient da[b][c] = sum dz * u in the same pass.  The first
        // half of gcat goes on through the attention gate to u, the second half into the encoder skip (read in place later)
        {
            const Drop dd = make_drop(e, SITE_DEC_CONV + (j - 1), true, (int64_t)2 * Cp * HWp);
            const ZCat zc{e->f(Pv.u), e->f(Pv.att), e->f(e->enc[n - 2 - (j - 1)].s), Cp};
            const Bn& bn = Pv.bn;
            hipLaunchKernelGGL(k_bn_bwd_reduce, red_grid(B, bn.C, HWp), dim3(256), 0, e->stream, e->f(L.gdin), (long long)2 * Cp * HWp,
                               (const float*)nullptr, 0LL, (const float*)nullptr, 0LL, B, bn.C, HWp, e->f(bn.saved), e->P(bn.gamma),
                               e->P(bn.beta), dd, (float*)nullptr, e->dsum(bn.bsums), zc);
            double *acc_gamma, *acc_beta;
            if (int rc = bn_bwd_between(e, bn, acc_gamma, acc_beta)) return rc;
            hipLaunchKernelGGL(k_bn_bwd_apply2_planes, dim3(1, bn.C, B), dim3(256), 0, e->stream, e->f(L.gdin), (long long)2 * Cp * HWp,
                               bn.C, HWp, e->f(bn.saved), e->P(bn.gamma), e->P(bn.beta), dd, e->dsum(bn.bsums), bn_count(e, B, HWp),
                               acc_gamma, acc_beta, e->f(Pv.gcat), zc, e->f(Pv.da));
        }
        hipLaunchKernelGGL(k_att_bwd, dim3(B), dim3(256), (size_t)(3 * Cp + 4 * Pv.R) * sizeof(float), e->stream,
                           e->f(Pv.pool), e->f(Pv.att), e->f(Pv.hid), e->f(Pv.da), Cp, Pv.R, e->P(Pv.w1), e->P(Pv.w2),
                           e->gacc(Pv.w1), e->gacc(Pv.w2), e->f(Pv.dpool));
        // ... and accumulates the previous layer's bias gradient while it writes du
        hipLaunchKernelGGL(k_scale_bwd, red_grid(B, Cp, HWp), dim3(256), 0, e->stream, e->f(Pv.gcat), e->f(Pv.att),
                           e->f(Pv.pool), e->f(Pv.dpool), B, Cp, HWp, e->f(Pv.gu), e->gacc(Pv.b));
    }
    // decoder_lin / encoder_lin backward
    const uint32_t sites[4] = {SITE_ENC_FC0, SITE_ENC_FC1, SITE_DEC_FC0, SITE_DEC_FC1};
    const float* gin = e->f(e->dec[0].gdin);   // grad wrt fc[3].a  (B, nout3)
    for (int k = 3; k >= 0; k--) {
        Fc& L = e->fc[k];
        const Drop d = make_drop(e, sites[k], true, L.nout);
        if (L.has_bn) {
            if (int rc = bn_backward(e, L.bn, gin, L.nout, nullptr, 0, e->f(L.h), L.nout, B, 1, d, e->f(L.gh))) return rc;
        } else {
            hipLaunchKernelGGL(k_relu_drop_bwd, dim3(blocks_for((long long)B * L.nout, 8192)), dim3(256), 0, e->stream, e->f(L.gh), gin,
                               e->f(L.h), (long long)B * L.nout, d);
        }
        const float* in = k == 0 ? (make_drop(e, SITE_ENC_CONV + n - 1, true, 0).on ? e->f(e->enc[n - 1].a) : e->f(e->enc[n - 1].s))
                                 : e->f(e->fc[k - 1].a);
        lin_bwd(e, L, B, in, e->f(L.gh), e->f(L.ga));
        gin = e->f(L.ga);
    }
    // encoder backward; gin = grad wrt a_{n-1} (B, F)
    for (int i = n - 1; i >= 0; i--) {
        ConvLayer& L = e->enc[i];
        Geom g = L.g;
        g.B = B;
        const int HW = g.Hs * g.Ws, C = g.Cs;
        // gradient of the skip use of s_i (decoder layer n-2-i), read in place from that layer's gcat
        const float* gskip = nullptr;
        long long gskip_bs = 0;
        if (i < n - 1) {
            const ConvLayer& D = e->dec[n - 2 - i];
            gskip = e->f(D.gcat) + (size_t)C * HW;
            gskip_bs = (long long)2 * C * HW;
        }
        if (int rc = bn_backward(e, L.bn, gin, (long long)C * HW, gskip, gskip_bs, e->f(L.z), (long long)C * HW, B, HW,
                                 make_drop(e, SITE_ENC_CONV + i, true, (int64_t)C * HW), e->f(L.gz)))
            return rc;
        const float* in = i == 0 ? x : (make_drop(e, SITE_ENC_CONV + i - 1, true, 0).on ? e->f(e->enc[i - 1].a) : e->f(e->enc[i - 1].s));
        // Conv2d: S = output, L = input
        conv_wgrad(e, g, e->f(L.gz), in, e->gacc(L.w));
        // no bias gradient: this bias is added right before a BatchNorm, whose backward makes every channel of dz sum
        // to zero (the reference's autograd returns rounding noise of ~1e-8 here)
        if (i > 0) {
            conv_up(e, g, e->f(L.gz), e->P(L.w), L.wp >= 0 ? e->f(L.wp) : nullptr, nullptr, e->f(e->enc[i - 1].ga));
            gin = e->f(e->enc[i - 1].ga);
        }
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int gather_x(unet_engine* e, int which, const int32_t* perm, int64_t start, int B) {
    const long long E = (long long)e->in_c * e->in_h * e->in_w;
    hipLaunchKernelGGL(k_gather, dim3(blocks_for((long long)B * E, 65536)), dim3(256), 0, e->stream, e->ds[which].x, perm,
                       (long long)start, B, E, e->f(e->xb));
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

AdamwConsts adamw_consts(const unet_engine* e) {
    const Hyper& h = e->hyper;
    const double bc1 = 1.0 - pow(h.beta1, (double)e->step), bc2 = 1.0 - pow(h.beta2, (double)e->step);
    return AdamwConsts{(float)(h.lr / bc1), (float)sqrt(bc2), (float)(1.0 - h.lr * h.wd), (float)(1.0 - h.beta1), (float)(1.0 - h.beta2),
                       (float)h.beta2, (float)h.eps};
}
int adamw_blocks(const unet_engine* e) { return blocks_for((e->tab.n_param + 3) / 4, 2048); }

F32Ranges f32_ranges(const unet_engine* e) {
    F32Ranges fr;
    memset(&fr, 0, sizeof fr);
    for (int k = 0; k < 4; k++)
        if (e->fc_f32[k]) fr.lo[fr.n] = e->fc[k].w, fr.hi[fr.n] = e->fc[k].w + (long long)e->fc[k].nin * e->fc[k].nout, fr.n++;
    return fr;
}

// (batch checked by the caller)
int train_or_fb(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int slot, float* grads_out,
                double grad_scale = 1.0) {
    int rc;
    if ((rc = gather_x(e, which, perm, start, batch))) return rc;
    if ((rc = forward(e, e->f(e->xb), batch, true))) return rc;
    if ((rc = loss_forward(e, which, perm, start, batch, slot, true))) return rc;
    if ((rc = backward(e, e->f(e->xb), batch))) return rc;
    if (grads_out) {
        hipLaunchKernelGGL(k_acc_to_f32, dim3(blocks_for(e->tab.n_param, 65536)), dim3(256), 0, e->stream, (long long)e->tab.n_param,
                           e->gacc(0), grads_out, grad_scale, f32_ranges(e));
    } else {
        e->step += 1;
        hipLaunchKernelGGL(k_adamw, dim3(adamw_blocks(e)), dim3(256), 0, e->stream, (long long)e->tab.n_param, e->params, e->gacc(0), e->m,
                           e->v, adamw_consts(e), f32_ranges(e));
        e->gacc_clean = true;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- data-parallel shards (unet_forward_backward_sync / unet_eval_step_sync) ----------------------------------------
// An empty shard's step: no activations and no launch over the batch, but the same tables - zero here - go to the all-reduce in
// the order of e->tables, the running statistics advance from the global sums as the other ranks' do (SyncBN; per-rank
// statistics have nothing to advance from), and the loss slot and the (zero) gradient are written.
int empty_shard_step(unet_engine* e, int which, int slot, float* grads_out) {
    const bool train = grads_out != nullptr;
    const Drop off{0, 0, 1.f, 0, 0};
    if (train) HIP_TRY(hipMemsetAsync(e->dsum(0), 0, (size_t)e->n_dsum * sizeof(double), e->stream));
    for (const SumTable& t : e->tables) {
        if (t.off == e->off_ltot) {
            if (int rc = loss_forward(e, which, nullptr, 0, 0, slot, false)) return rc;
        } else if (train) {
            if (int rc = sync_table(e, t.off)) return rc;
            if (t.fwd && e->shard.sync_bn()) bn_act(e, *t.fwd, nullptr, 0, 0, t.HW, true, off, nullptr, nullptr);
        }
    }
    if (train) HIP_TRY(hipMemsetAsync(grads_out, 0, (size_t)e->tab.n_param * sizeof(float), e->stream));
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace

extern "C" {

int unet_engine_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                       int latent_size, int max_batch, unet_engine** out) {
    if (!enc || !dec || !out || n_enc < 1 || n_dec < 1 || fc_size < 1 || latent_size < 1 || max_batch < 1)
        return fail(CAE_ERR_ARG, "unet_engine_create: bad argument");
    if (n_enc != n_dec)
        return fail(CAE_ERR_ARG, "unet_engine_create: the UNET decoder needs one layer per encoder layer (%d vs %d): every "
                                 "decoder layer but the last takes one skip connection (unet.py:141-145,157-161)", n_enc, n_dec);
    unet_engine* e = new unet_engine();
    e->fc_size = fc_size;
    e->latent = latent_size;
    e->max_batch = max_batch;
    auto bad = [&](const char* msg, int i) {
        const int rc = fail(CAE_ERR_ARG, "unet_engine_create: layer %d: %s", i, msg);
        delete e;
        return rc;
    };
    // ---- geometry --------------------------------------------------------------------------------
    for (int i = 0; i < n_enc; i++) {
        const cae_layer_spec& l = enc[i];
        ConvLayer L;
        L.g = Geom{0, l.out_c, l.out_h, l.out_w, l.in_c, l.in_h, l.in_w, l.k_h, l.k_w, l.stride, l.output_padding};
        if (l.stride < 1 || l.k_h < 1 || l.k_w < 1 || l.output_padding < 0) return bad("bad kernel / stride / padding", i);
        if ((l.in_h + 2 * l.output_padding - l.k_h) / l.stride + 1 != l.out_h ||
            (l.in_w + 2 * l.output_padding - l.k_w) / l.stride + 1 != l.out_w)
            return bad("encoder output size does not follow from Conv2d(kernel, stride, padding)", i);
        if (i > 0 && (enc[i - 1].out_c != l.in_c || enc[i - 1].out_h != l.in_h || enc[i - 1].out_w != l.in_w))
            return bad("encoder input does not match the previous layer's output", i);
        L.has_bn = true;
        e->enc.push_back(L);
    }
    for (int j = 0; j < n_dec; j++) {
        const cae_layer_spec& l = dec[j];
        ConvLayer L;
        L.g = Geom{0, l.in_c, l.in_h, l.in_w, l.out_c, l.out_h, l.out_w, l.k_h, l.k_w, l.stride, l.output_padding};
        if (l.stride < 1 || l.k_h < 1 || l.k_w < 1 || l.output_padding < 0) return bad("bad kernel / stride / padding", j);
        if ((l.in_h - 1) * l.stride - 2 * l.output_padding + l.k_h != l.out_h ||
            (l.in_w - 1) * l.stride - 2 * l.output_padding + l.k_w != l.out_w)
            return bad("decoder output size does not follow from ConvTranspose2d(kernel, stride, padding)", j);
        L.has_bn = L.has_skip = j != n_dec - 1;
        if (L.has_skip) {
            const cae_layer_spec& s = enc[n_enc - 2 - j];
            if (s.out_c != l.out_c || s.out_h != l.out_h || s.out_w != l.out_w)
                return bad("decoder output does not match the encoder skip it is concatenated with", j);
            if (l.out_c < 8) return bad("ChannelAttention needs at least 8 channels (in_planes // 8 hidden units)", j);
            L.R = l.out_c / 8;
            if (dec[j + 1].in_c != 2 * l.out_c || dec[j + 1].in_h != l.out_h || dec[j + 1].in_w != l.out_w)
                return bad("the next decoder layer must take 2 x out_channels (skip concat) at this layer's size", j);
        }
        e->dec.push_back(L);
    }
    e->in_c = enc[0].in_c, e->in_h = enc[0].in_h, e->in_w = enc[0].in_w;
    e->out_c = dec[n_dec - 1].out_c, e->out_h = dec[n_dec - 1].out_h, e->out_w = dec[n_dec - 1].out_w;
    const int F = enc[n_enc - 1].out_c * enc[n_enc - 1].out_h * enc[n_enc - 1].out_w;
    const int G = dec[0].in_c * dec[0].in_h * dec[0].in_w;
    // ---- tensor table, in the reference's state_dict order --------------------------------------------
    for (int i = 0; i < n_enc; i++) {
        ConvLayer& L = e->enc[i];
        const std::string c = "enc/encoder_cnn." + std::to_string(4 * i), b = "enc/encoder_cnn." + std::to_string(4 * i + 1);
        L.w = e->tab.add(c + ".weight", 0, {L.g.Cs, L.g.Cl, L.g.kh, L.g.kw});
        L.b = e->tab.add(c + ".bias", 0, {L.g.Cs});
        add_bn(e, b, L.g.Cs, L.bn);
    }
    auto add_fc = [&](Fc& L, const std::string& key, int nin, int nout) {
        L.nin = nin;
        L.nout = nout;
        L.w = e->tab.add(key + ".weight", 0, {nout, nin});
        L.b = e->tab.add(key + ".bias", 0, {nout});
    };
    add_fc(e->fc[0], "enc/encoder_lin.0", F, fc_size);
    e->fc[0].has_bn = true;
    add_bn(e, "enc/encoder_lin.1", fc_size, e->fc[0].bn);
    add_fc(e->fc[1], "enc/encoder_lin.4", fc_size, latent_size);
    add_fc(e->fc[2], "dec/decoder_lin.0", latent_size, fc_size);
    e->fc[2].has_bn = true;
    add_bn(e, "dec/decoder_lin.1", fc_size, e->fc[2].bn);
    add_fc(e->fc[3], "dec/decoder_lin.4", fc_size, G);
    for (int j = 0; j < n_dec; j++) {
        ConvLayer& L = e->dec[j];
        if (!L.has_skip) continue;
        const std::string a = "dec/attention_layers." + std::to_string(j);
        L.w1 = e->tab.add(a + ".fc1.weight", 0, {L.R, L.g.Cl, 1, 1});
        L.w2 = e->tab.add(a + ".fc2.weight", 0, {L.g.Cl, L.R, 1, 1});
    }
    for (int j = 0; j < n_dec; j++) {
        ConvLayer& L = e->dec[j];
        const std::string c = "dec/decoder_conv." + std::to_string(4 * j), b = "dec/decoder_conv." + std::to_string(4 * j + 1);
        L.w = e->tab.add(c + ".weight", 0, {L.g.Cs, L.g.Cl, L.g.kh, L.g.kw});
        L.b = e->tab.add(c + ".bias", 0, {L.g.Cl});
        if (L.has_bn) add_bn(e, b, 2 * L.g.Cl, L.bn);
    }
    e->tab.close();
    // ---- workspace -------------------------------------------------------------------------------------
    const int64_t B = max_batch;
    int64_t nd = 0;   // doubles: BN sums
    auto carve_bn = [&](Bn& bn) {
        bn.sums = nd;
        nd += 2 * bn.C;
        bn.bsums = nd;
        nd += 2 * bn.C;
    };
    for (auto& L : e->enc) carve_bn(L.bn);
    carve_bn(e->fc[0].bn);
    carve_bn(e->fc[2].bn);
    for (auto& L : e->dec)
        if (L.has_bn) carve_bn(L.bn);
    e->off_ltot = nd;
    nd += 4;
    e->n_dsum = nd;
    // the tables of a SyncBN step, in the order forward(), loss_forward() and backward() pass them
    for (auto& L : e->enc) e->tables.push_back(SumTable{L.bn.sums, 2 * L.bn.C, &L.bn, L.g.Hs * L.g.Ws});
    for (int k : {0, 2}) e->tables.push_back(SumTable{e->fc[k].bn.sums, 2 * e->fc[k].bn.C, &e->fc[k].bn, 1});
    for (auto& L : e->dec)
        if (L.has_bn) e->tables.push_back(SumTable{L.bn.sums, 2 * L.bn.C, &L.bn, L.g.Hl * L.g.Wl});
    e->tables.push_back(SumTable{e->off_ltot, 3, nullptr, 0});
    for (int j = (int)e->dec.size() - 2; j >= 0; j--) e->tables.push_back(SumTable{e->dec[j].bn.bsums, 2 * e->dec[j].bn.C});
    for (int k : {2, 0}) e->tables.push_back(SumTable{e->fc[k].bn.bsums, 2 * e->fc[k].bn.C});
    for (int i = (int)e->enc.size() - 1; i >= 0; i--) e->tables.push_back(SumTable{e->enc[i].bn.bsums, 2 * e->enc[i].bn.C});
    Carver F32{64};   // the fp32 sub-arena (float offsets)
    auto carve_saved = [&](Bn& bn) { bn.saved = F32(2 * bn.C); };
    e->xb = F32(B * e->in_c * e->in_h * e->in_w);
    for (auto& L : e->enc) {
        const int64_t n = B * L.g.Cs * L.g.Hs * L.g.Ws;
        L.z = F32(n), L.s = F32(n), L.a = F32(n), L.gz = F32(n), L.ga = F32(n);
        carve_saved(L.bn);
    }
    for (int k = 0; k < 4; k++) {
        Fc& L = e->fc[k];
        const int64_t n = B * L.nout;
        L.h = F32(n), L.a = F32(n), L.gh = F32(n);
        L.ga = F32(B * L.nin);
        if (L.has_bn) carve_saved(L.bn);
    }
    for (auto& L : e->dec) {
        const int64_t nl = B * L.g.Cl * L.g.Hl * L.g.Wl, ns = B * L.g.Cs * L.g.Hs * L.g.Ws;
        L.u = F32(nl), L.gu = F32(nl), L.gdin = F32(ns);
        if (L.has_skip) {
            L.din_next = F32(2 * nl), L.gcat = F32(2 * nl);
            L.pool = F32(3 * B * L.g.Cl), L.psum = F32(4 * B * L.g.Cl), L.hid = F32(2 * B * L.R), L.att = F32(B * L.g.Cl);
            L.dpool = F32(2 * B * L.g.Cl), L.da = F32(B * L.g.Cl);
            carve_saved(L.bn);
        }
    }
    e->coef = F32(4 * B * e->out_c);
    // weights repacked per output parity for the layers that run OpUp (kernels_unet_mfma.h): decoder forward, encoder dgrad
    auto carve_packed = [&](ConvLayer& L) {
        Geom g = L.g;
        g.B = (int)B;
        if ((mfma_up_eligible(g) && g.Cl > 4) || thin_up_geom(g)) L.wp = F32((int64_t)16 * g.Cs * g.Cl);
    };
    for (auto& L : e->dec) carve_packed(L);
    for (size_t i = 1; i < e->enc.size(); i++) carve_packed(e->enc[i]);
    Carver bytes{256};
    e->off_gacc = bytes(e->tab.n_param * 8);
    e->off_dsum = bytes(nd * 8);
    e->per_slot = 2;   // (mse, pearson loss)
    e->off_losses = bytes((int64_t)kStepLossSlots * e->per_slot * 8);
    e->off_ls = bytes(B * e->out_c * 8 * 8);
    int64_t gp = 0;   // K slices' partial tiles of the Linear GEMMs on the tile engine (forward, input gradient), any batch
    for (int k = 0; k < 4; k++)
        for (int b = 1; b <= B; b++)
            gp = std::max<int64_t>(gp, (int64_t)std::max(gemm_part_bytes(e->fc[k].nout, b, e->fc[k].nin),
                                                          gemm_part_bytes(e->fc[k].nin, b, e->fc[k].nout)));
    e->off_gpart = bytes(gp);
    e->gpart_bytes = gp;
    int64_t lp = 0;   // partial tiles of the big layers' K slices (128 wide), batch <= 64
    for (int k = 0; k < 4; k++) {
        const Fc& L = e->fc[k];
        if (small_fc(L)) continue;
        lp = std::max<int64_t>(lp, std::max<int64_t>((L.nin + 127) / 128 * (int64_t)L.nout, (L.nout + 127) / 128 * (int64_t)L.nin) * std::min<int64_t>(B, 64) * 4);
    }
    e->off_linpart = bytes(lp);
    e->linpart_bytes = lp;
    int64_t tp = 0;
    auto thin_need = [&](const ConvLayer& L) {
        Geom g = L.g;
        g.B = (int)B;
        if (thin_geom(g)) tp = std::max<int64_t>(tp, (int64_t)thin_wgrad_part_bytes(g));
        else if (mfma_wgrad_eligible(g)) tp = std::max<int64_t>(tp, (int64_t)mfma_wgrad_part_bytes(g));
        if (pwgrad_geom(g)) tp = std::max<int64_t>(tp, (int64_t)pwgrad_part_bytes(g));
    };
    for (auto& L : e->enc) thin_need(L);
    for (auto& L : e->dec) thin_need(L);
    e->off_thinpart = bytes(tp);
    e->thinpart_bytes = tp;
    int64_t dp = 0;   // the split-K down convolutions' partial maps (forward of the encoder, input gradient of the decoder), any batch
    auto down_need = [&](const ConvLayer& L) {
        Geom g = L.g;
        for (int b = 1; b <= B; b++) {
            g.B = b;
            if (patch_geom(g)) dp = std::max<int64_t>(dp, (int64_t)pdown_part_bytes(g));
            if (mfma_down_eligible(g)) dp = std::max<int64_t>(dp, (int64_t)mfma_down_part_bytes(g));
        }
    };
    for (auto& L : e->enc) down_need(L);
    for (auto& L : e->dec) down_need(L);
    e->off_downpart = bytes(dp);
    e->downpart_bytes = dp;
    e->off_f32 = bytes(F32.top * 4);
    e->ws_bytes = bytes.top;
    *out = e;
    return CAE_OK;
}

void unet_engine_destroy(unet_engine* e) { delete e; }

int64_t unet_param_count(const unet_engine* e) { return e ? e->tab.n_param : 0; }
int64_t unet_buffer_count(const unet_engine* e) { return e ? e->tab.n_buf : 0; }
int unet_tensor_count(const unet_engine* e) { return e ? e->tab.count() : 0; }
int unet_tensor_info(const unet_engine* e, int index, cae_tensor_info_t* out) {
    return e ? e->tab.info(index, out) : fail(CAE_ERR_ARG, "unet_tensor_info: null engine");
}
int64_t unet_workspace_bytes(const unet_engine* e) { return e ? e->ws_bytes : 0; }

int unet_bind(unet_engine* e, float* params, float* m, float* v, float* buffers, void* workspace, int64_t workspace_bytes) {
    if (int rc = bind_workspace(e, "unet", params && m && v && buffers, workspace, workspace_bytes)) return rc;
    e->params = params, e->m = m, e->v = v, e->buffers = buffers;
    return CAE_OK;
}

int unet_set_stream(unet_engine* e, void* hip_stream) { return set_stream(e, "unet", hip_stream); }

int unet_set_kernel_mode(unet_engine* e, int specialised) {
    if (!e) return fail(CAE_ERR_ARG, "unet_set_kernel_mode: null engine");
    e->specialised = specialised ? 1 : 0;
    return CAE_OK;
}

int unet_set_hyper(unet_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay, double dropout_rate,
                   double lambda_pearson, uint32_t dropout_seed) {
    if (!e) return fail(CAE_ERR_ARG, "unet_set_hyper: null engine");
    if (!(dropout_rate >= 0.0 && dropout_rate < 1.0)) return fail(CAE_ERR_ARG, "unet_set_hyper: dropout_rate must be in [0, 1)");
    e->hyper = Hyper{lr, beta1, beta2, eps, weight_decay};
    e->dropout = dropout_rate;
    e->lambda_p = lambda_pearson;
    e->seed = dropout_seed;
    return CAE_OK;
}

int unet_set_lr(unet_engine* e, double lr) {
    if (!e) return fail(CAE_ERR_ARG, "unet_set_lr: null engine");
    e->hyper.lr = lr;   // the next step's launches take it by value (adamw_consts)
    return CAE_OK;
}

int unet_set_step(unet_engine* e, int64_t step) { return set_step(e, "unet", step); }

int unet_set_dataset(unet_engine* e, int which, const float* x, const float* target, const float* mask, int mask_channels,
                     int64_t n) {
    if (e && mask && mask_channels != 1 && mask_channels != e->out_c)
        return fail(CAE_ERR_ARG, "unet_set_dataset: mask has %d channels, expected 1 or %d", mask_channels, e->out_c);
    return set_dataset(e, "unet", which, DataSet{x, target, mask, mask_channels, n});
}

int unet_train_step(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    if (int rc = check_batch(e, "unet", which, start, batch, loss_slot, true)) return rc;
    return train_or_fb(e, which, perm, start, batch, loss_slot, nullptr);
}

int unet_forward_backward(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot,
                          float* grads, double grad_scale) {
    if (!grads) return fail(CAE_ERR_ARG, "unet_forward_backward: null gradient buffer");
    if (int rc = check_batch(e, "unet", which, start, batch, loss_slot, true)) return rc;
    return train_or_fb(e, which, perm, start, batch, loss_slot, grads, grad_scale);
}

int unet_forward_backward_sync(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int row0,
                               int global_batch, int world, int loss_slot, float* grads, cae_allreduce_fn fn, void* user) {
    if (!e || !grads) return fail(CAE_ERR_ARG, "unet_forward_backward_sync: bad argument");
    if (int rc = check_shard(e, "unet_forward_backward_sync", which, start, batch, row0, global_batch, world, loss_slot, fn))
        return rc;
    ShardScope scope(e, ShardSync{fn, user, world, global_batch, row0});
    e->table_pos = 0;
    if (int rc = batch == 0 ? empty_shard_step(e, which, loss_slot, grads) : train_or_fb(e, which, perm, start, batch, loss_slot, grads))
        return rc;
    if (e->shard.sync_bn() && e->table_pos != e->tables.size())
        return fail(CAE_ERR_STATE, "unet: %zu of %zu sum tables passed to the callback", e->table_pos, e->tables.size());
    return CAE_OK;
}

int unet_apply_gradients(unet_engine* e, const float* grads) {
    if (!e || !e->ws || !grads) return fail(CAE_ERR_ARG, "unet_apply_gradients: bad argument");
    hipLaunchKernelGGL(k_f32_to_acc, dim3(blocks_for(e->tab.n_param, 65536)), dim3(256), 0, e->stream, (long long)e->tab.n_param, grads,
                       e->gacc(0));
    e->step += 1;
    hipLaunchKernelGGL(k_adamw, dim3(adamw_blocks(e)), dim3(256), 0, e->stream, (long long)e->tab.n_param, e->params, e->gacc(0), e->m,
                       e->v, adamw_consts(e), F32Ranges{{0, 0, 0, 0}, {0, 0, 0, 0}, 0});
    e->gacc_clean = true;
    for (int k = 0; k < 4; k++) e->fc_f32[k] = e->fc_f32_dirty[k] = false;   // every slot was rewritten as fp64 and cleared
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int unet_eval_step(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    int rc = check_batch(e, "unet", which, start, batch, loss_slot, true);
    if (rc) return rc;
    if ((rc = gather_x(e, which, perm, start, batch))) return rc;
    if ((rc = forward(e, e->f(e->xb), batch, false))) return rc;
    return loss_forward(e, which, perm, start, batch, loss_slot, false);
}

int unet_eval_step_sync(unet_engine* e, int which, const int32_t* perm, int64_t start, int batch, int row0, int global_batch,
                        int loss_slot, cae_allreduce_fn fn, void* user) {
    if (!e) return fail(CAE_ERR_ARG, "unet_eval_step_sync: null engine");
    int rc = check_shard(e, "unet_eval_step_sync", which, start, batch, row0, global_batch, 0, loss_slot, fn);
    if (rc) return rc;
    ShardScope scope(e, ShardSync{fn, user, 0, global_batch, row0});
    if (batch == 0) return empty_shard_step(e, which, loss_slot, nullptr);
    if ((rc = gather_x(e, which, perm, start, batch))) return rc;
    if ((rc = forward(e, e->f(e->xb), batch, false))) return rc;
    return loss_forward(e, which, perm, start, batch, loss_slot, false);
}

int unet_score(unet_engine* e, const float* x, int batch, float* y) {
    int rc = check_score(e, "unet", x, batch, y);
    if (rc || (rc = forward(e, x, batch, false))) return rc;
    const long long n = (long long)batch * e->out_c * e->out_h * e->out_w;
    hipLaunchKernelGGL(k_sigmoid, dim3(blocks_for(n, 65536)), dim3(256), 0, e->stream, e->f(e->dec.back().u), n, y);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int unet_loss_slots(const unet_engine* e) { return e ? kStepLossSlots : 0; }
int unet_read_losses(unet_engine* e, int first_slot, int count, double* out) { return read_losses(e, "unet", first_slot, count, out); }
int unet_sync(unet_engine* e) { return sync(e, "unet"); }

int unet_debug_read(unet_engine* e, const char* what, float* out, int64_t count) {
    if (!e || !e->ws || !what || !out || count < 1) return fail(CAE_ERR_ARG, "unet_debug_read: bad argument");
    std::map<std::string, int64_t> table;
    for (size_t i = 0; i < e->enc.size(); i++) {
        const std::string k = std::to_string(i);
        table["enc_z" + k] = e->enc[i].z, table["enc_s" + k] = e->enc[i].s, table["enc_a" + k] = e->enc[i].a;
        table["enc_gz" + k] = e->enc[i].gz;
    }
    for (size_t j = 0; j < e->dec.size(); j++) {
        const std::string k = std::to_string(j);
        table["dec_u" + k] = e->dec[j].u, table["dec_gu" + k] = e->dec[j].gu, table["dec_gdin" + k] = e->dec[j].gdin;
        if (e->dec[j].has_skip)
            table["att" + k] = e->dec[j].att, table["dec_din" + std::to_string(j + 1)] = e->dec[j].din_next,
            table["dec_gcat" + k] = e->dec[j].gcat;
    }
    for (int k = 0; k < 4; k++) table["fc_h" + std::to_string(k)] = e->fc[k].h, table["fc_a" + std::to_string(k)] = e->fc[k].a;
    auto it = table.find(what);
    if (it == table.end()) return fail(CAE_ERR_ARG, "unet_debug_read: unknown tensor '%s'", what);
    HIP_TRY(hipMemcpyAsync(out, e->f(it->second), (size_t)count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CAE_OK;
}

int unet_debug_plan(const unet_engine* e, int batch, int train, char* out, int64_t out_bytes) {
    if (!e || !out || out_bytes < 1) return fail(CAE_ERR_ARG, "unet_debug_plan: bad argument");
    if (batch < 1 || batch > e->max_batch)
        return fail(CAE_ERR_ARG, "unet_debug_plan: batch %d outside 1 .. %d", batch, e->max_batch);
    const std::vector<const ConvLayer*> packed = pack_list(e, train != 0);
    auto in_pack = [&](const ConvLayer& L) { return (int)(std::find(packed.begin(), packed.end(), &L) != packed.end()); };
    auto geom = [&](const ConvLayer& L) {
        Geom g = L.g;
        g.B = batch;
        return g;
    };
    std::string s;
    char line[256];   // (one field group at a time: a layer's line is built piecewise)
    auto tile_name = [&](int rows) {
        const IgemmTile t = igemm_tile(rows);
        return std::to_string(t.tn()) + "x" + std::to_string(t.tm());
    };
    // what the launch of each family switches on below the family, from the functions the launches call
    auto down_fields = [&](const Geom& g) {
        line[0] = 0;
        switch (choose_down(e, g)) {
            case DOWN_THIN:
                snprintf(line, sizeof line, " down.rbn=%d down.cl=%d down.tpw=%d down.groups=%d down.Ws=%d", thin_rbn(g), thin_cl(g),
                         thin_down_tpw(g), thin_down_groups(g), g.Ws);
                break;
            case DOWN_PATCH: {
                const PdownPlan p = pdown_plan(g, true, (size_t)e->downpart_bytes);
                snprintf(line, sizeof line, " down.rbn=%d down.nsplit=%d down.Ws=%d", p.rbn, p.nsplit, g.Ws);
                break;
            }
            case DOWN_MFMA:
                snprintf(line, sizeof line, " down.tile=%s down.nsplit=%d", tile_name(g.Cs).c_str(),
                         mfma_down_nsplit(g, true, (size_t)e->downpart_bytes));
                break;
            case DOWN_GENERIC: break;
        }
        s += line;
    };
    auto up_fields = [&](const Geom& g, bool has_wp) {
        line[0] = 0;
        switch (choose_up(e, g, has_wp)) {
            case UP_THIN:
                snprintf(line, sizeof line, " up.cl=%d up.waves=%d up.wgs=%d", thin_cl(g), thin_up_waves(g), thin_up_wgs(g));
                break;
            case UP_THIN_CL: snprintf(line, sizeof line, " up.cl=%d", thin_cl(g)); break;
            case UP_PATCH: snprintf(line, sizeof line, " up.rbn=%d up.Ws=%d", pup_rbn(g), g.Ws); break;
            case UP_MFMA: snprintf(line, sizeof line, " up.tile=%s", tile_name(g.Cl).c_str()); break;
            case UP_GENERIC: break;
        }
        s += line;
    };
    auto wgrad_fields = [&](const Geom& g) {
        line[0] = 0;
        switch (choose_wgrad(e, g)) {
            case WG_THIN:
            case WG_THIN_ATOMIC:
                snprintf(line, sizeof line, " wgrad.rbn=%d wgrad.tpw=%d wgrad.groups=%d", thin_rbn(g), thin_wgrad_tpw(g), thin_wgrad_groups(g));
                break;
            case WG_PATCH:
                snprintf(line, sizeof line, " wgrad.wrxwc=%dx%d wgrad.tpw=%d wgrad.slices=%d", pwgrad_wr(g), 4 / pwgrad_wr(g), pwgrad_tpw(g),
                         pwgrad_slices(g));
                break;
            case WG_MFMA:
            case WG_MFMA_ATOMIC: {
                const MfmaWgradPlan p = mfma_wgrad_plan(g);
                snprintf(line, sizeof line, " wgrad.tile=%s wgrad.slices=%d wgrad.per=%d", p.one_wave ? "1wave" : tile_name(g.Cs).c_str(),
                         p.zdim, p.per);
                break;
            }
            case WG_GENERIC: break;
        }
        s += line;
    };
    // the calls forward() and backward() make: an encoder layer runs OpDown forward, its weight gradient and (but the first)
    // OpUp for its input gradient; a decoder layer runs OpUp forward, its weight gradient and OpDown for its input gradient
    for (size_t i = 0; i < e->enc.size(); i++) {
        const ConvLayer& L = e->enc[i];
        const Geom g = geom(L);
        snprintf(line, sizeof line, "enc%zu down=%s up=%s wgrad=%s wp=%d packed=%d", i, kDownName[choose_down(e, g)],
                 train && i > 0 ? kUpName[choose_up(e, g, L.wp >= 0)] : "-", train ? kWgradName[choose_wgrad(e, g)] : "-",
                 (int)(L.wp >= 0), in_pack(L));
        s += line;
        down_fields(g);
        if (train && i > 0) up_fields(g, L.wp >= 0);
        if (train) wgrad_fields(g);
        s += "\n";
    }
    for (int k = 0; k < 4; k++) {
        const Fc& L = e->fc[k];
        const LinK kind = choose_lin(e, L, batch);
        const char* fam = kLinName[kind];
        snprintf(line, sizeof line, "fc%d fwd=%s bwd=%s", k, fam, train ? fam : "-");
        s += line;
        if (kind == LIN_BIG) {   // lin_fwd: N = nout, K = nin;  lin_bwd: k_lin_outer, then the input gradient with N = nin, K = nout
            const LinGemmPlan f = lin_gemm_plan(batch, L.nin);
            snprintf(line, sizeof line, " fwd.rb=%d fwd.slices=%d fwd.kiters=%d fwd.partial=%d fwd.ntiles=%d fwd.nlast=%d", f.rb, f.slices,
                     f.kiters, (int)f.partial, (L.nout + kLinNT - 1) / kLinNT, L.nout - (L.nout - 1) / kLinNT * kLinNT);
            s += line;
            if (train) {
                const LinGemmPlan b = lin_gemm_plan(batch, L.nout);
                snprintf(line, sizeof line, " bwd.rb=%d bwd.slices=%d bwd.kiters=%d bwd.partial=%d outer_lds=%zu", b.rb, b.slices, b.kiters,
                         (int)b.partial, lin_outer_lds(batch));
                s += line;
            }
        } else if (kind == LIN_TILE) {   // the GEMMs lin_fwd and lin_bwd hand to gemm_launch
            const GemmPlan f = gemm_plan(L.nout, batch, L.nin, 0, true, (size_t)e->gpart_bytes);
            snprintf(line, sizeof line, " fwd.tile=%dx%d fwd.slices=%d fwd.per=%d", f.tile.tn(), f.tile.tm(), f.slices, f.per);
            s += line;
            if (train) {
                const GemmPlan w = gemm_plan(L.nout, L.nin, batch, 2, false, 0), d = gemm_plan(L.nin, batch, L.nout, 0, true, (size_t)e->gpart_bytes);
                snprintf(line, sizeof line, " wgrad.tile=%dx%d wgrad.slices=%d bwd.tile=%dx%d bwd.slices=%d bwd.per=%d", w.tile.tn(), w.tile.tm(),
                         w.slices, d.tile.tn(), d.tile.tm(), d.slices, d.per);
                s += line;
            }
        }
        s += "\n";
    }
    for (size_t j = 0; j < e->dec.size(); j++) {
        const ConvLayer& L = e->dec[j];
        const Geom g = geom(L);
        snprintf(line, sizeof line, "dec%zu down=%s up=%s wgrad=%s wp=%d packed=%d", j, train ? kDownName[choose_down(e, g)] : "-",
                 kUpName[choose_up(e, g, L.wp >= 0)], train ? kWgradName[choose_wgrad(e, g)] : "-", (int)(L.wp >= 0), in_pack(L));
        s += line;
        if (train) down_fields(g);
        up_fields(g, L.wp >= 0);
        if (train) wgrad_fields(g);
        s += "\n";
    }
    snprintf(line, sizeof line, "pack entries=%zu launches=%d\n", packed.size(), pack_launches(packed.size()));
    s += line;
    if ((int64_t)s.size() + 1 > out_bytes)
        return fail(CAE_ERR_ARG, "unet_debug_plan: the report needs %zu bytes, got %lld", s.size() + 1, (long long)out_bytes);
    memcpy(out, s.c_str(), s.size() + 1);
    return CAE_OK;
}

}  // extern "C"
