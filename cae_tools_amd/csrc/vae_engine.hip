// vae_engine.hip — host side of the 'var' (variational autoencoder + MS-SSIM) path: the extern "C" ABI of include/cae_vae.h.
// Every convolution, BatchNorm, Linear layer and the optimiser run in a ConvAE engine created in trunk mode (trunk_api.h:
// the LDS-staged / row-streaming / MFMA kernels of the ConvAE path, BatchNorm folded into producers and consumers); this file
// adds what the two models differ in: the reparameterisation between the heads and the decoder (kernels_vae.h, called back
// from the trunk) and the loss - sigmoid, MSE, KL, MS-SSIM and its gradient - between the trunk's forward and backward.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cae_vae.h"
#include "kernels_unet.h"
#include "kernels_vae.h"
#include "trunk_api.h"
#include "engine_host.h"

using namespace unet;
using namespace cae_internal;

struct vae_engine : SteppedCore {   // (ws, stream, max_batch, step, data sets, loss slots, shard: engine_host.h)
    cae_engine* trunk = nullptr;   // convolutions, BatchNorm, Linear layers, Adam: the ConvAE engine in trunk mode
    int fc_size = 0, latent = 0;
    int in_c = 0, in_h = 0, in_w = 0, out_c = 0, out_h = 0, out_w = 0;
    int64_t n_params = 0, n_buffers = 0, trunk_ws = 0;
    int64_t off_trunk = 0, off_grads = 0, off_f32 = 0;
    int64_t xb = 0, eps = 0, kappa = 0, heads = 0;   // (heads: vae_encode's (B, 2 * latent) rows before they are split)
    int64_t sx[vae::kScales] = {0}, sy[vae::kScales] = {0}, sA[vae::kScales] = {0}, sB[vae::kScales] = {0},
            sC[vae::kScales] = {0}, sG[vae::kScales] = {0};
    int64_t off_ssum = 0, off_part = 0;   // doubles: [scale][BC][2]; parts {mse, kl, ssim}
    double l_mse = 1, l_kl = 1, l_ssim = 1;
    double grad_scale = 1.0;     // data-parallel half-step: every loss gradient is scaled by local / global batch at its source
    uint32_t seed = 0;
    bool row_kernels = true;     // MS-SSIM passes: row-streaming kernels (vae_set_kernel_mode 1) or the LDS tile kernels (0)
    vae::Gauss gauss;

    float* f(int64_t off) const { return reinterpret_cast<float*>(ws + off_f32) + off; }
    double* parts() const { return reinterpret_cast<double*>(ws + off_part); }
    ~vae_engine() {
        if (trunk) cae_engine_destroy(trunk);
    }
};

namespace {

// the key of the noise array of (seed, step): oracle/vae_oracle.py normal_noise
uint32_t seed_key(uint32_t seed) { return pcg(seed + 0x9E3779B9u * 977u); }
uint32_t noise_key(const vae_engine* e) { return pcg(seed_key(e->seed) ^ (uint32_t)(e->step & 0xFFFFFFFF)); }

// ---- the two call-backs of the trunk (trunk_api.h) ----------------------------------------------------------------------
void hook_reparam(void* user, hipStream_t s, const float* heads, int B, int latent, int train, float* z) {
    vae_engine* e = static_cast<vae_engine*>(user);
    hipLaunchKernelGGL(vae::k_reparam, dim3(1), dim3(256), 0, s, heads, B, latent, e->shard.row0, noise_key(e), train, z, e->f(e->eps),
                       e->parts() + 1);
}

void hook_reparam_bwd(void* user, hipStream_t s, const float* gz, const float* heads, int B, int latent, float* gheads) {
    vae_engine* e = static_cast<vae_engine*>(user);
    hipLaunchKernelGGL(vae::k_reparam_bwd, dim3(blocks_for((long long)B * latent, 65536)), dim3(256), 0, s, gz, heads, e->f(e->eps), B, latent,
                       (float)(e->l_kl * e->grad_scale), e->shard.loss_rows(B) * latent, gheads);
}

// y, target batch, MS-SSIM + MSE; with want_grad the gradient wrt the last layer's raw output goes to dec.back().gz
// (a data-parallel shard leaves raw sums in the parts, and its gradient coefficients use the global counts)
int loss(vae_engine* e, int which, const int32_t* perm, int64_t start, int B, int slot, bool want_grad, double* parts) {
    const int C = e->out_c, H = e->out_h, W = e->out_w, BC = B * C;
    const long long E = (long long)C * H * W, n = (long long)B * E;
    const bool shard = e->shard.fn != nullptr;
    const int Bg = e->shard.loss_rows(B);
    if (!e->row_kernels)   // (the row-kernel path forms the finest level inside its pyramid launch)
        hipLaunchKernelGGL(vae::k_sigmoid_gather, dim3(blocks_for(n, 65536)), dim3(256), 0, e->stream, cae_internal::trunk_raw_output(e->trunk), e->ds[which].t, perm,
                           (long long)start, B, E, e->f(e->sx[0]), e->f(e->sy[0]));
    double* ssum = reinterpret_cast<double*>(e->ws + e->off_ssum);   // (cleared by step_common together with the loss parts)
    if (e->row_kernels) {
        // the pooling pyramid of both maps in one launch, the finest scale's walk, then the four coarse scales' walks in one launch
        vae::Pyramid pm;
        for (int s = 0; s < vae::kScales; s++) pm.x[s] = e->f(e->sx[s]), pm.y[s] = e->f(e->sy[s]);
        pm.u = cae_internal::trunk_raw_output(e->trunk), pm.target = e->ds[which].t, pm.perm = perm, pm.start = start, pm.C = C;
        hipLaunchKernelGGL(vae::k_pool_pyramid, dim3(W / 16, H / 16, BC), dim3(256), 0, e->stream, pm, H, W);
        vae::SsimScales set;
        memset(&set, 0, sizeof set);
        set.BC = BC;
        dim3 coarse_grid(1, 1, 1);
        for (int s = 0, h = H, w = W; s < vae::kScales; s++, h /= 2, w /= 2) {
            const int rb = vae::ssim_band_rows(h - vae::kHalo, true), bands = (h - vae::kHalo + rb - 1) / rb;
            const dim3 grid((w - vae::kHalo + vae::kSsimCols - 1) / vae::kSsimCols, (bands + 3) / 4, BC);
            double* ss = ssum + (size_t)s * BC * 2;
            const int lastf = s == vae::kScales - 1 ? 1 : 0;
            if (s == 0) {
                hipLaunchKernelGGL(vae::k_ssim_fwd_rows, grid, dim3(256), 0, e->stream, e->f(e->sx[s]), e->f(e->sy[s]), h, w, rb, e->gauss,
                                   1e-4f, 9e-4f, lastf, ss, e->f(e->sA[s]), e->f(e->sB[s]), e->f(e->sC[s]));
            } else {
                set.s[set.n++] = vae::SsimScale{e->f(e->sx[s]), e->f(e->sy[s]), h, w, rb, lastf, ss, e->f(e->sA[s]), e->f(e->sB[s]), e->f(e->sC[s])};
                coarse_grid.x = std::max(coarse_grid.x, grid.x);
                coarse_grid.y = std::max(coarse_grid.y, grid.y);
            }
        }
        coarse_grid.z = (unsigned)(BC * set.n);
        hipLaunchKernelGGL(vae::k_ssim_fwd_rows_multi, coarse_grid, dim3(256), 0, e->stream, set, e->gauss, 1e-4f, 9e-4f);
    } else {
        int h = H, w = W;
        for (int s = 0; s < vae::kScales; s++) {
            if (s > 0) {
                hipLaunchKernelGGL(vae::k_pool2_pair, dim3(blocks_for((long long)BC * h * w / 4, 65536)), dim3(256), 0, e->stream, e->f(e->sx[s - 1]),
                                   e->f(e->sy[s - 1]), BC, h, w, e->f(e->sx[s]), e->f(e->sy[s]));
                h /= 2, w /= 2;
            }
            const dim3 grid((w - vae::kHalo + vae::kTile - 1) / vae::kTile, (h - vae::kHalo + vae::kTile - 1) / vae::kTile, BC);
            hipLaunchKernelGGL(vae::k_ssim_fwd, grid, dim3(256), 0, e->stream, e->f(e->sx[s]), e->f(e->sy[s]), h, w, e->gauss, 1e-4f,
                               9e-4f, s == vae::kScales - 1 ? 1 : 0, ssum + (size_t)s * BC * 2, e->f(e->sA[s]), e->f(e->sB[s]),
                               e->f(e->sC[s]));
        }
    }
    vae::ScaleCounts nv;
    for (int s = 0, hh = H, ww = W; s < vae::kScales; s++, hh /= 2, ww /= 2) nv.v[s] = (hh - vae::kHalo) * (ww - vae::kHalo);
    hipLaunchKernelGGL(vae::k_msssim_finalize, dim3(1), dim3(256), 0, e->stream, ssum, BC, Bg * C, shard ? 1.0 : (double)BC, nv,
                       (float)e->l_ssim, parts + 2, e->f(e->kappa));
    if (want_grad && e->row_kernels) {
        // the four coarse scales' own terms in one launch, their pooling chain folded into scale 1's map, then the finest scale
        vae::SsimBwdScales set;
        memset(&set, 0, sizeof set);
        set.BC = BC;
        dim3 cg(1, 1, 1);
        for (int s = 1; s < vae::kScales; s++) {
            const int hs = H >> s, wsz = W >> s;
            const int rb = vae::ssim_band_rows(hs, false), bands = (hs + rb - 1) / rb;
            set.s[set.n++] = vae::SsimBwdScale{e->f(e->sx[s]), e->f(e->sy[s]), hs, wsz, rb, s, e->f(e->sA[s]), e->f(e->sB[s]), e->f(e->sC[s]),
                                               e->f(e->sG[s])};
            cg.x = std::max<unsigned>(cg.x, (wsz + vae::kSsimCols - 1) / vae::kSsimCols);
            cg.y = std::max<unsigned>(cg.y, (bands + 3) / 4);
        }
        cg.z = (unsigned)(BC * set.n);
        hipLaunchKernelGGL(vae::k_ssim_bwd_rows_multi, cg, dim3(256), 0, e->stream, set, e->gauss, e->f(e->kappa));
        hipLaunchKernelGGL(vae::k_ssim_combine, dim3(blocks_for((long long)BC * (H / 2) * (W / 2), 65536)), dim3(256), 0, e->stream, e->f(e->sG[1]),
                           e->f(e->sG[2]), e->f(e->sG[3]), e->f(e->sG[4]), BC, H / 2, W / 2);
        {
            const int rb = vae::ssim_band_rows(H, false), bands = (H + rb - 1) / rb;
            const dim3 grid((W + vae::kSsimCols - 1) / vae::kSsimCols, (bands + 3) / 4, BC);
            hipLaunchKernelGGL(vae::k_ssim_bwd_rows, grid, dim3(256), 0, e->stream, e->f(e->sx[0]), e->f(e->sy[0]), H, W, rb, e->gauss,
                               e->f(e->sA[0]), e->f(e->sB[0]), e->f(e->sC[0]), e->f(e->kappa), 0, e->f(e->sG[1]), e->f(e->sG[0]));
        }
    } else if (want_grad) {
        for (int s = vae::kScales - 1; s >= 0; s--) {
            const int hs = H >> s, wsz = W >> s;
            const float* coarse = s == vae::kScales - 1 ? (const float*)nullptr : e->f(e->sG[s + 1]);
            const dim3 grid((wsz + vae::kTile - 1) / vae::kTile, (hs + vae::kTile - 1) / vae::kTile, BC);
            hipLaunchKernelGGL(vae::k_ssim_bwd, grid, dim3(256), 0, e->stream, e->f(e->sx[s]), e->f(e->sy[s]), hs, wsz, e->gauss,
                               e->f(e->sA[s]), e->f(e->sB[s]), e->f(e->sC[s]), e->f(e->kappa), s, coarse, e->f(e->sG[s]));
        }
    }
    hipLaunchKernelGGL(vae::k_vae_loss_grad, dim3(blocks_for(n, 1024)), dim3(256), 0, e->stream, e->f(e->sx[0]), e->f(e->sy[0]),
                       want_grad ? e->f(e->sG[0]) : (const float*)nullptr, n, (long long)Bg * E,
                       (float)e->l_mse, (float)e->grad_scale,
                       want_grad ? cae_internal::trunk_output_gradient(e->trunk) : (float*)nullptr, parts + 0,
                       want_grad && C == 1 ? cae_internal::trunk_output_bias_acc(e->trunk) : (double*)nullptr);
    (void)slot;
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// (within vae_forward_backward_sync / vae_eval_step_sync, e->shard is the data-parallel shard)
int step_common(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int slot, bool train, float* grads_out,
                bool optimise, double grad_scale = 1.0) {
    const ShardSync& sh = e->shard;
    int rc;
    if (!sh.fn && (rc = check_batch(e, "vae", which, start, batch, slot, true))) return rc;   // (a shard is checked by its caller)
    e->grad_scale = grad_scale;
    const long long E = (long long)e->in_c * e->in_h * e->in_w;
    if (batch > 0)
        hipLaunchKernelGGL(k_gather, dim3(blocks_for((long long)batch * E, 65536)), dim3(256), 0, e->stream, e->ds[which].x, perm,
                           (long long)start, batch, E, e->f(e->xb));
    double* parts = e->parts();
    // the MS-SSIM sums and the loss parts lie next to each other: one fill
    HIP_TRY(hipMemsetAsync(e->ws + e->off_ssum, 0, (size_t)(e->off_part + 4 * sizeof(double) - e->off_ssum), e->stream));
    // trunk forward: encoder stack, Linear + heads, z (call-back), decoder stack; the last layer leaves its raw output.  A training
    // shard's trunk passes its BatchNorm tables to the callback (and runs for an empty shard too: the other ranks wait on them)
    const ShardSync ts = train ? sh : ShardSync{};
    if ((batch > 0 || ts.fn) && (rc = cae_internal::trunk_forward(e->trunk, e->f(e->xb), batch, train, true, nullptr, ts))) return rc;
    // KL is a mean over B*latent
    if (batch > 0 && (rc = loss(e, which, perm, start, batch, slot, train, parts))) return rc;
    if (sh.fn) {
        // the shard's sums {share of the mean squared error, KL term, 1 - MS-SSIM per (b, c)} over the ranks: the global batch's means
        if ((rc = call_allreduce(sh, "vae", parts, 3))) return rc;
        const double bg = sh.global_batch;
        hipLaunchKernelGGL(vae::k_loss_slot, dim3(1), dim3(1), 0, e->stream, parts, 1.0, bg * e->latent,
                           bg * e->out_c, e->l_mse, e->l_kl, e->l_ssim, e->losses(slot));
    } else {
        hipLaunchKernelGGL(vae::k_loss_slot, dim3(1), dim3(1), 0, e->stream, parts, 1.0, (double)batch * e->latent, 1.0, e->l_mse,
                           e->l_kl, e->l_ssim, e->losses(slot));
    }
    if (train) {
        // the last layer's bias gradient = sum of dL/d(raw output) per channel (the ConvAE path gets it from its fused loss
        // epilogue; here the loss is ours)
        const int HW = e->out_h * e->out_w;
        const int chunks = (int)std::max<long long>(1, std::min<long long>(((long long)batch * HW + 2047) / 2048, 64));
        if (e->out_c > 1 && batch > 0)     // (a single-channel output's sum rides in k_vae_loss_grad)
            hipLaunchKernelGGL(k_chan_sums<ACC_GRAD>, dim3(chunks, e->out_c), dim3(256), 0, e->stream, cae_internal::trunk_output_gradient(e->trunk),
                           (long long)e->out_c * HW, batch, HW, cae_internal::trunk_output_bias_acc(e->trunk), 1, 0);
        if ((batch > 0 || ts.fn) && (rc = cae_internal::trunk_backward(e->trunk, e->f(e->xb), batch, ts))) return rc;
        if (grads_out) {
            if ((rc = cae_internal::trunk_gradients(e->trunk, grads_out, 1.0))) return rc;   // already scaled at the sources
            if (optimise) return fail(CAE_ERR_ARG, "vae: gradients are either handed out or applied");
        } else if (optimise) {
            e->step += 1;     // (on the device the trunk's first training kernel counted it)
            if ((rc = cae_internal::trunk_adam(e->trunk))) return rc;
        }
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace

extern "C" {

int vae_engine_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size, int latent_size,
                      int max_batch, vae_engine** out) {
    if (!enc || !dec || !out || n_enc < 1 || n_dec < 1 || fc_size < 1 || latent_size < 1 || max_batch < 1)
        return fail(CAE_ERR_ARG, "vae_engine_create: bad argument");
    vae_engine* e = new vae_engine();
    e->fc_size = fc_size, e->latent = latent_size, e->max_batch = max_batch;
    e->gauss = vae::make_gauss();
    e->in_c = enc[0].in_c, e->in_h = enc[0].in_h, e->in_w = enc[0].in_w;
    e->out_c = dec[n_dec - 1].out_c, e->out_h = dec[n_dec - 1].out_h, e->out_w = dec[n_dec - 1].out_w;
    if (e->out_h % 16 || e->out_w % 16 || e->out_h < 176 || e->out_w < 176) {
        delete e;
        return fail(CAE_ERR_ARG, "vae_engine_create: layer %d: the MS-SSIM loss needs an output height and width that are multiples "
                                 "of 16 and at least 176", n_dec - 1);
    }
    // geometry checks, tensor table and parameter arena: the trunk's (its message is the one cae_last_error() returns)
    if (int rc = cae_internal::trunk_create(enc, n_enc, dec, n_dec, fc_size, latent_size, max_batch, &e->trunk)) {
        delete e;
        return rc;
    }
    cae_internal::trunk_set_hooks(e->trunk, cae_internal::TrunkHooks{hook_reparam, hook_reparam_bwd, e});
    e->n_params = cae_param_count(e->trunk);
    e->n_buffers = cae_buffer_count(e->trunk);
    e->trunk_ws = cae_workspace_bytes(e->trunk);
    // ---- workspace: [trunk][fp32 gradient arena of the trunk][losses][MS-SSIM sums][parts][fp32 maps] ----
    const int64_t B = max_batch;
    Carver F32{64};   // the fp32 sub-arena (float offsets)
    e->xb = F32(B * e->in_c * e->in_h * e->in_w);
    e->eps = F32(B * latent_size);
    e->heads = F32(B * 2 * latent_size);
    const int64_t BC = B * e->out_c;
    for (int s = 0, h = e->out_h, w = e->out_w; s < vae::kScales; s++, h /= 2, w /= 2) {
        e->sx[s] = F32(BC * h * w), e->sy[s] = F32(BC * h * w), e->sG[s] = F32(BC * h * w);
        const int64_t nv = BC * (h - vae::kHalo) * (w - vae::kHalo);
        e->sA[s] = F32(nv), e->sB[s] = F32(nv), e->sC[s] = F32(nv);
    }
    e->kappa = F32(BC * vae::kScales);
    Carver bytes{256};
    e->off_trunk = bytes(e->trunk_ws);
    e->off_grads = bytes(e->n_params * 4);
    e->per_slot = 4;   // (mse, kl, ssim, total)
    e->off_losses = bytes((int64_t)kStepLossSlots * e->per_slot * 8);
    e->off_ssum = bytes((int64_t)vae::kScales * BC * 2 * 8);
    e->off_part = bytes(4 * 8);
    e->off_f32 = bytes(F32.top * 4);
    e->ws_bytes = bytes.top;
    *out = e;
    return CAE_OK;
}

void vae_engine_destroy(vae_engine* e) { delete e; }
int64_t vae_param_count(const vae_engine* e) { return e ? e->n_params : 0; }
int64_t vae_buffer_count(const vae_engine* e) { return e ? e->n_buffers : 0; }
int vae_tensor_count(const vae_engine* e) { return e ? cae_tensor_count(e->trunk) : 0; }
int vae_tensor_info(const vae_engine* e, int index, cae_tensor_info_t* out) {
    if (!e || !out) return fail(CAE_ERR_ARG, "vae_tensor_info: bad argument");
    return cae_tensor_info(e->trunk, index, out);
}
int64_t vae_workspace_bytes(const vae_engine* e) { return e ? e->ws_bytes : 0; }

int vae_bind(vae_engine* e, float* params, float* m, float* v, float* buffers, void* workspace, int64_t workspace_bytes) {
    if (int rc = bind_workspace(e, "vae", params && m && v && buffers, workspace, workspace_bytes)) return rc;
    return cae_bind(e->trunk, params, reinterpret_cast<float*>(e->ws + e->off_grads), m, v, buffers, e->ws + e->off_trunk, e->trunk_ws);
}
int vae_set_stream(vae_engine* e, void* hip_stream) {
    if (int rc = set_stream(e, "vae", hip_stream)) return rc;
    if (int rc = cae_set_stream(e->trunk, hip_stream)) return rc;
    return cae_set_graph_mode(e->trunk, 0);   // the trunk runs as plain launches between this file's own
}
int vae_set_hyper(vae_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay, double lambda_mse,
                  double lambda_kl, double lambda_ssim, uint32_t noise_seed) {
    if (!e) return fail(CAE_ERR_ARG, "vae_set_hyper: null engine");
    e->l_mse = lambda_mse, e->l_kl = lambda_kl, e->l_ssim = lambda_ssim, e->seed = noise_seed;
    return cae_set_hyper(e->trunk, lr, beta1, beta2, eps, weight_decay);
}
int vae_set_lr(vae_engine* e, double lr) {
    if (!e) return fail(CAE_ERR_ARG, "vae_set_lr: null engine");
    return cae_set_lr(e->trunk, lr);
}
int vae_set_kernel_mode(vae_engine* e, int mode) {
    if (!e) return fail(CAE_ERR_ARG, "vae_set_kernel_mode: null engine");
    e->row_kernels = (mode & 1) != 0;
    return CAE_OK;
}
int vae_set_step(vae_engine* e, int64_t step) {
    if (int rc = set_step(e, "vae", step)) return rc;
    return e->ws ? cae_set_adam_step(e->trunk, (int)step) : CAE_OK;
}
int vae_set_dataset(vae_engine* e, int which, const float* x, const float* target, int64_t n) {
    return set_dataset(e, "vae", which, DataSet{x, target, nullptr, 0, n});
}
int vae_train_step(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    return step_common(e, which, perm, start, batch, loss_slot, true, nullptr, true);
}
int vae_forward_backward(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot, float* grads,
                         double grad_scale) {
    if (!grads) return fail(CAE_ERR_ARG, "vae_forward_backward: null gradient buffer");
    return step_common(e, which, perm, start, batch, loss_slot, true, grads, false, grad_scale);
}
int vae_forward_backward_sync(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int row0, int global_batch,
                              int world, int loss_slot, float* grads, cae_allreduce_fn fn, void* user) {
    if (!e || !grads) return fail(CAE_ERR_ARG, "vae_forward_backward_sync: bad argument");
    if (int rc = check_shard(e, "vae_forward_backward_sync", which, start, batch, row0, global_batch, world, loss_slot, fn)) return rc;
    ShardScope scope(e, ShardSync{fn, user, world, global_batch, row0});
    return step_common(e, which, perm, start, batch, loss_slot, true, grads, false);
}
int vae_apply_gradients(vae_engine* e, const float* grads) {
    if (!e || !e->ws || !grads) return fail(CAE_ERR_ARG, "vae_apply_gradients: bad argument");
    e->step += 1;     // (on the device vae_forward_backward's first kernel counted it)
    return cae_internal::trunk_adam_from(e->trunk, grads);
}
int vae_eval_step(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    return step_common(e, which, perm, start, batch, loss_slot, false, nullptr, false);
}
int vae_eval_step_sync(vae_engine* e, int which, const int32_t* perm, int64_t start, int batch, int row0, int global_batch,
                       int loss_slot, cae_allreduce_fn fn, void* user) {
    if (!e) return fail(CAE_ERR_ARG, "vae_eval_step_sync: null engine");
    if (int rc = check_shard(e, "vae_eval_step_sync", which, start, batch, row0, global_batch, 0, loss_slot, fn)) return rc;
    ShardScope scope(e, ShardSync{fn, user, 0, global_batch, row0});
    return step_common(e, which, perm, start, batch, loss_slot, false, nullptr, false);
}
int vae_score(vae_engine* e, const float* x, int batch, float* y) {
    if (int rc = check_score(e, "vae", x, batch, y)) return rc;
    HIP_TRY(hipMemsetAsync(e->parts(), 0, 4 * sizeof(double), e->stream));
    return cae_internal::trunk_forward(e->trunk, x, batch, false, false, y);
}
int vae_encode(vae_engine* e, const float* x, int batch, float* mu, float* logvar) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "vae_encode: vae_bind has not been called");
    if (!x || !mu || !logvar || batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "vae_encode: bad argument");
    if (int rc = cae_internal::trunk_encode(e->trunk, x, batch, e->f(e->heads))) return rc;
    hipLaunchKernelGGL(vae::k_split_heads, dim3(blocks_for((long long)batch * e->latent, 65536)), dim3(256), 0, e->stream, e->f(e->heads),
                       batch, e->latent, mu, logvar);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
int vae_decode(vae_engine* e, const float* z, int batch, float* y) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "vae_decode: vae_bind has not been called");
    if (!z || !y || batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "vae_decode: bad argument");
    return cae_internal::trunk_decode(e->trunk, z, batch, y);
}
int vae_sample_latent(vae_engine* e, const float* mu, const float* logvar, int batch, int64_t first_case, int64_t draw, int n_draws,
                      uint32_t seed, float* z) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "vae_sample_latent: vae_bind has not been called");
    if (!z || batch < 1 || first_case < 0 || draw < 0 || n_draws < 1 || n_draws > 65535)
        return fail(CAE_ERR_ARG, "vae_sample_latent: bad argument");
    if ((first_case + batch) * (int64_t)e->latent >= (1LL << 31))
        return fail(CAE_ERR_ARG, "vae_sample_latent: case %lld x latent %d reaches noise index 2^31, where the hash index wraps",
                    (long long)(first_case + batch), e->latent);
    hipLaunchKernelGGL(vae::k_sample_latent, dim3(blocks_for((long long)batch * e->latent, 65536), n_draws), dim3(256), 0, e->stream, mu,
                       logvar, batch, e->latent, (long long)first_case, seed_key(seed), (long long)draw, z);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
int vae_loss_slots(const vae_engine* e) { return e ? kStepLossSlots : 0; }
int vae_read_losses(vae_engine* e, int first_slot, int count, double* out) { return read_losses(e, "vae", first_slot, count, out); }
int vae_sync(vae_engine* e) { return sync(e, "vae"); }
void vae_gauss_window(float* out11) {
    const vae::Gauss g = vae::make_gauss();
    memcpy(out11, g.g, sizeof g.g);
}
int vae_debug_read(vae_engine* e, const char* what, float* out, int64_t count) {
    if (!e || !e->ws || !what || !out || count < 0) return fail(CAE_ERR_ARG, "vae_debug_read: bad argument");
    const float* src = nullptr;
    int64_t cap = (int64_t)e->max_batch * e->latent;
    const int64_t maps = (int64_t)e->max_batch * e->out_c * e->out_h * e->out_w;
    if (!strcmp(what, "eps")) src = e->f(e->eps);
    else if (!strcmp(what, "z")) src = cae_internal::trunk_latent(e->trunk);
    else if (!strcmp(what, "y")) src = e->f(e->sx[0]), cap = maps;
    else if (!strcmp(what, "gssim")) src = e->f(e->sG[0]), cap = maps;
    else return fail(CAE_ERR_ARG, "vae_debug_read: unknown tensor '%s' (eps, z, y, gssim)", what);
    if (count > cap) return fail(CAE_ERR_ARG, "vae_debug_read: %lld floats exceed the tensor", (long long)count);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, src, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return CAE_OK;
}
int vae_debug_plan(const vae_engine* e, int batch, int train, char* out, int64_t out_bytes) {
    if (!e) return fail(CAE_ERR_ARG, "vae_debug_plan: null engine");
    return cae_debug_plan(e->trunk, batch, train, out, out_bytes);
}
int64_t vae_trunk_debug_read(vae_engine* e, const char* what, int index, void* out, int64_t capacity) {
    if (!e) return fail(CAE_ERR_ARG, "vae_trunk_debug_read: null engine");
    return cae_debug_read(e->trunk, what, index, out, capacity);
}

}  // extern "C"
