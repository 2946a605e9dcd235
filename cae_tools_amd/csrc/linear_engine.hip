// linear_engine.hip — the LinearModel path (include/cae_linear.h): one nn.Linear between the flattened input and the
// flattened output, MSE, Adam.  Three GEMMs per step on the MFMA tile engine, all of them bound by the weight matrix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "cae_linear.h"
#include "kernels_unet.h"
#include "kernels_unet_mfma.h"
#include "kernels_vae.h"
#include "engine_host.h"

using namespace unet;
using namespace cae_internal;

namespace {

// g = 2 (y - t) / n (optional);  loss_out += sum (y - t)^2 / n (on the ACC_GRAD grid: exact while the loss is below 8);  t
// gathered through perm
__global__ void __launch_bounds__(256) k_mse(const float* __restrict__ y, const float* __restrict__ target, const int* __restrict__ perm,
                                             long long start, int B, long long E, float* __restrict__ g, double* __restrict__ loss_out) {
    __shared__ double red[4];
    const long long n = (long long)B * E;
    const float k = 2.f / (float)n;
    double s = 0;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long long)gridDim.x * 256) {
        const long long b = o / E, i = o - b * E;
        const long long smp = perm ? (long long)perm[start + b] : start + b;
        const float d = y[o] - target[smp * E + i];
        s += (double)d * (double)d;
        if (g) g[o] = k * d;
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) acc_add<ACC_GRAD>(loss_out, t / (double)n);
}

}  // namespace

struct lin_engine : SteppedCore {   // (ws, stream, max_batch, step, data sets, loss slots: engine_host.h)
    int64_t nin = 0, nout = 0, n_params = 0;
    int64_t off_gacc = 0, off_gpart = 0, gpart_bytes = 0, off_xb = 0, off_y = 0, off_g = 0;
    float *params = nullptr, *m = nullptr, *v = nullptr;
    vae::AdamHyper hyper{1e-3, 0.9, 0.999, 1e-8, 1e-5};
    bool gacc_clean = false;
    double* gacc() const { return reinterpret_cast<double*>(ws + off_gacc); }
    float* xb() const { return reinterpret_cast<float*>(ws + off_xb); }
    float* y() const { return reinterpret_cast<float*>(ws + off_y); }
    float* g() const { return reinterpret_cast<float*>(ws + off_g); }
};

namespace {

// The two GEMM shapes of a step.  forward() and step_common() launch these descriptors and lin_debug_plan reports the plan of
// the same ones (with null operands: a plan depends on the shape and the store mode alone)
// y[b][o] = bias[o] + sum_i x[b][i] W[o][i]
GemmDesc fwd_gemm(const lin_engine* e, const float* x, int B, float* y) {
    const float* W = e->params;
    return GemmDesc{(int)e->nout, B, (int)e->nin, W, e->nin, 1, x, 1, e->nin, W ? W + e->nout * e->nin : nullptr, y, nullptr, 1, e->nout, 0};
}
// dW[o][i] = sum_b g[b][o] x[b][i]
GemmDesc wgrad_gemm(const lin_engine* e, int batch, const float* g, const float* xb, double* acc) {
    return GemmDesc{(int)e->nout, (int)e->nin, batch, g, 1, e->nout, xb, e->nin, 1, nullptr, nullptr, acc, e->nin, 1, 2};
}

int forward(lin_engine* e, const float* x, int B, float* y) {
    const GemmDesc d = fwd_gemm(e, x, B, y);
    gemm_launch(d, reinterpret_cast<float*>(e->ws + e->off_gpart), e->gpart_bytes, e->stream);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int step_common(lin_engine* e, int which, const int32_t* perm, int64_t start, int batch, int slot, bool train, float* grads_out,
                bool optimise, double grad_scale = 1.0) {
    int rc = check_batch(e, "lin", which, start, batch, slot, true);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gather, dim3(blocks_for((long long)batch * e->nin, 65536)), dim3(256), 0, e->stream, e->ds[which].x, perm, (long long)start,
                       batch, (long long)e->nin, e->xb());
    if ((rc = forward(e, e->xb(), batch, e->y()))) return rc;
    HIP_TRY(hipMemsetAsync(e->losses(slot), 0, sizeof(double), e->stream));
    hipLaunchKernelGGL(k_mse, dim3(blocks_for((long long)batch * e->nout, 1024)), dim3(256), 0, e->stream, e->y(), e->ds[which].t, perm,
                       (long long)start, batch, (long long)e->nout, train ? e->g() : (float*)nullptr, e->losses(slot));
    if (train) {
        if (!e->gacc_clean) HIP_TRY(hipMemsetAsync(e->gacc(), 0, (size_t)e->n_params * sizeof(double), e->stream));
        e->gacc_clean = false;
        // dW through the tile engine;  db[o] = sum_b g[b][o]
        const GemmDesc w = wgrad_gemm(e, batch, e->g(), e->xb(), e->gacc());
        gemm_launch(w, nullptr, 0, e->stream);
        hipLaunchKernelGGL(k_col_sums, dim3((unsigned)((e->nout + 255) / 256)), dim3(256), 0, e->stream, batch, (int)e->nout, e->g(),
                           e->gacc() + e->nout * e->nin);
        if (grads_out)
            hipLaunchKernelGGL(k_acc_to_f32, dim3(blocks_for(e->n_params, 65536)), dim3(256), 0, e->stream, (long long)e->n_params, e->gacc(),
                               grads_out, grad_scale, F32Ranges{{0, 0, 0, 0}, {0, 0, 0, 0}, 0});
        if (optimise) {
            e->step += 1;
            hipLaunchKernelGGL(vae::k_adam_l2, dim3(blocks_for(e->n_params, 65536)), dim3(256), 0, e->stream, (long long)e->n_params, e->params,
                               e->gacc(), e->m, e->v, e->hyper, (int)e->step);
            e->gacc_clean = true;
        }
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace

extern "C" {

int lin_engine_create(int64_t n_in, int64_t n_out, int max_batch, lin_engine** out) {
    if (!out || n_in < 1 || n_out < 1 || max_batch < 1 || n_in > (1ll << 30) || n_out > (1ll << 30) || n_in * n_out > (1ll << 31) - 64)
        return fail(CAE_ERR_ARG, "lin_engine_create: bad argument (sizes must keep n_in * n_out below 2^31)");
    lin_engine* e = new lin_engine();
    e->nin = n_in, e->nout = n_out, e->max_batch = max_batch;
    e->n_params = n_out * n_in + n_out;
    Carver bytes{256};
    e->off_gacc = bytes(e->n_params * 8);
    e->off_losses = bytes((int64_t)kStepLossSlots * e->per_slot * 8);
    for (int b = 1; b <= max_batch; b++)   // the forward's K slices (split K), any batch
        e->gpart_bytes = std::max<int64_t>(e->gpart_bytes, (int64_t)gemm_part_bytes((int)n_out, b, (int)n_in));
    e->off_gpart = bytes(e->gpart_bytes);
    e->off_xb = bytes((int64_t)max_batch * n_in * 4);
    e->off_y = bytes((int64_t)max_batch * n_out * 4);
    e->off_g = bytes((int64_t)max_batch * n_out * 4);
    e->ws_bytes = bytes.top;
    *out = e;
    return CAE_OK;
}
void lin_engine_destroy(lin_engine* e) { delete e; }
int64_t lin_param_count(const lin_engine* e) { return e ? e->n_params : 0; }
int64_t lin_workspace_bytes(const lin_engine* e) { return e ? e->ws_bytes : 0; }
int lin_bind(lin_engine* e, float* params, float* m, float* v, void* workspace, int64_t workspace_bytes) {
    if (int rc = bind_workspace(e, "lin", params && m && v, workspace, workspace_bytes)) return rc;
    e->params = params, e->m = m, e->v = v;
    return CAE_OK;
}
int lin_set_stream(lin_engine* e, void* hip_stream) { return set_stream(e, "lin", hip_stream); }
int lin_set_hyper(lin_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay) {
    if (!e) return fail(CAE_ERR_ARG, "lin_set_hyper: null engine");
    e->hyper = vae::AdamHyper{lr, beta1, beta2, eps, weight_decay};
    return CAE_OK;
}
int lin_set_lr(lin_engine* e, double lr) {
    if (!e) return fail(CAE_ERR_ARG, "lin_set_lr: null engine");
    e->hyper.lr = lr;   // the next k_adam_l2 launch takes it by value
    return CAE_OK;
}
int lin_set_step(lin_engine* e, int64_t completed_steps) { return set_step(e, "lin", completed_steps); }
int lin_set_dataset(lin_engine* e, int which, const float* x, const float* target, int64_t n) {
    return set_dataset(e, "lin", which, DataSet{x, target, nullptr, 0, n});
}
int lin_train_step(lin_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    return step_common(e, which, perm, start, batch, loss_slot, true, nullptr, true);
}
int lin_forward_backward(lin_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot, float* grads,
                         double grad_scale) {
    if (!grads) return fail(CAE_ERR_ARG, "lin_forward_backward: null gradient buffer");
    return step_common(e, which, perm, start, batch, loss_slot, true, grads, false, grad_scale);
}
int lin_apply_gradients(lin_engine* e, const float* grads) {
    if (!e || !e->ws || !grads) return fail(CAE_ERR_ARG, "lin_apply_gradients: bad argument");
    hipLaunchKernelGGL(k_f32_to_acc, dim3(blocks_for(e->n_params, 65536)), dim3(256), 0, e->stream, (long long)e->n_params, grads, e->gacc());
    e->step += 1;
    hipLaunchKernelGGL(vae::k_adam_l2, dim3(blocks_for(e->n_params, 65536)), dim3(256), 0, e->stream, (long long)e->n_params, e->params,
                       e->gacc(), e->m, e->v, e->hyper, (int)e->step);
    e->gacc_clean = true;
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
int lin_eval_step(lin_engine* e, int which, const int32_t* perm, int64_t start, int batch, int loss_slot) {
    return step_common(e, which, perm, start, batch, loss_slot, false, nullptr, false);
}
int lin_score(lin_engine* e, const float* x, int batch, float* y) {
    if (int rc = check_score(e, "lin", x, batch, y)) return rc;
    return forward(e, x, batch, y);
}
int lin_loss_slots(const lin_engine* e) { return e ? kStepLossSlots : 0; }
int lin_read_losses(lin_engine* e, int first_slot, int count, double* out) { return read_losses(e, "lin", first_slot, count, out); }
int lin_sync(lin_engine* e) { return sync(e, "lin"); }

int lin_debug_plan(const lin_engine* e, int batch, int train, char* out, int64_t out_bytes) {
    if (!e || !out || out_bytes < 1) return fail(CAE_ERR_ARG, "lin_debug_plan: bad argument");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "lin_debug_plan: batch %d outside 1 .. %d", batch, e->max_batch);
    auto tile = [](const GemmPlan& p) { return std::to_string(p.tile.tn()) + "x" + std::to_string(p.tile.tm()); };
    std::string s;
    char line[256];
    // forward(): the K slices go to gpart, which a bound engine always has (lin_engine_create sized it)
    const GemmPlan f = gemm_plan(fwd_gemm(e, nullptr, batch, nullptr), true, (size_t)e->gpart_bytes);
    snprintf(line, sizeof line, "fwd tile=%s grid=%ux%u slices=%d per=%d part_bytes=%zu\n", tile(f).c_str(), f.grid.x, f.grid.y, f.slices,
             f.per, f.part_bytes);
    s += line;
    if (train) {   // step_common(): no room for partial tiles, one writer per element of the fp64 accumulator
        const GemmPlan w = gemm_plan(wgrad_gemm(e, batch, nullptr, nullptr, nullptr), false, 0);
        snprintf(line, sizeof line, "wgrad tile=%s grid=%ux%u slices=%d\n", tile(w).c_str(), w.grid.x, w.grid.y, w.slices);
    } else {
        snprintf(line, sizeof line, "wgrad -\n");
    }
    s += line;
    snprintf(line, sizeof line, "room gpart_bytes=%lld\n", (long long)e->gpart_bytes);
    s += line;
    if ((int64_t)s.size() + 1 > out_bytes)
        return fail(CAE_ERR_ARG, "lin_debug_plan: the report needs %zu bytes, got %lld", s.size() + 1, (long long)out_bytes);
    memcpy(out, s.c_str(), s.size() + 1);
    return CAE_OK;
}

}  // extern "C"
