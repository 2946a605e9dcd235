// engine.hip — host side of libcae_hip.so: the ConvAE engine's workspace carving and the extern "C" ABI declared in
// include/cae_hip.h.  One source, one code object: the step's host code is in engine_state.h / _choose.h / _launch.h / _step.h.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "cae_hip.h"
#include "kernels_generic.h"
#include "kernels_stateless.h"   // here: the place its kernels have always had in this code object (file map)
#include "kernels_spectra.h"     // after kernels_stateless.h: it uses its element loads
#include "kernels_ssim.h"        // likewise
#include "kernels_baseline.h"    // after kernels_ssim.h: it uses its raw loads and wave sum
#include "kernels_hist.h"        // likewise (templates only: emitted where stateless_host.h instantiates them, last)
#include "kernels_strata.h"      // likewise, after kernels_hist.h
#include "kernels_fss.h"         // likewise, after kernels_strata.h
#include "kernels_importance.h"  // likewise, after kernels_fss.h
#include "kernels_quantile.h"    // likewise, after kernels_importance.h
#include "kernels_neighbours.h"  // likewise, after kernels_quantile.h
#include "kernels_compare.h"     // likewise, after kernels_neighbours.h
#include "kernels_dihedral.h"    // likewise, after kernels_compare.h
#include "kernels_blend.h"       // likewise, after kernels_dihedral.h: it uses kernels_compare.h's tiles
#include "kernels_s2.h"
#include "kernels_last.h"
#include "kernels_rows.h"
#include "kernels_gemm.h"
#include "kernels_igemm.h"
#include "kernels_ctlds.h"
#include "kernels_head.h"
#include "dp_comm.h"
#include "kernels_ctbwd.h"   // argument struct only: the kernel lives in ctbwd.hip
#include "trunk_api.h"
#include "engine_host.h"

// The benchmark geometry's template kernels, instantiated HERE so that their code sits next to the non-template kernels of
// the same step (implicit instantiations are emitted at the end of the 3 MB text section, 2 MB away): see DESIGN.md §4.
namespace cae {
template __global__ void k_ct_fwd_lds<3, 3>(CtFwd);
template __global__ void k_s2_fwd_rows<8, 4, 1, 2>(S2FwdRows);
template __global__ void k_s2_fwd_rows<4, 2, 2, 1>(S2FwdRows);
template __global__ void k_s2_last_fused<2, 1, 4, 4, 4, true, true>(S2Last);
template __global__ void k_s2_bwd_rows<4, 4, 2, 3, 3, 2, 1, 3>(S2Rows);
template __global__ void k_s2_bwd_rows<8, 2, 4, 3, 3, 4, 2, 1>(S2Rows);
}  // namespace cae

using namespace cae;
using namespace cae_internal;

namespace cae_internal {
int ctbwd_launch(const void* args, size_t bytes, unsigned gx, unsigned gy, unsigned gz, size_t lds, hipStream_t s);   // ctbwd.hip
}

namespace {
thread_local std::string g_err;
}  // namespace

// engine_host.h: the message cae_last_error() returns for the calling thread
void cae_detail_set_error(const char* msg) { g_err = msg; }

#include "engine_state.h"
#include "engine_choose.h"
#include "engine_launch.h"
#include "engine_step.h"

// =================================================================================================
// C ABI
// =================================================================================================

extern "C" {

const char* cae_last_error(void) { return g_err.c_str(); }
int cae_abi_version(void) { return 1; }

static int engine_create_impl(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                              int latent_size, int max_batch, bool variational, cae_engine** out);

int cae_engine_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                      int latent_size, int max_batch, cae_engine** out) {
    return engine_create_impl(enc, n_enc, dec, n_dec, fc_size, latent_size, max_batch, false, out);
}

static int engine_create_impl(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                              int latent_size, int max_batch, bool variational, cae_engine** out) {
    if (!enc || !dec || !out || n_enc < 1 || n_dec < 1) return fail(CAE_ERR_ARG, "need >=1 encoder and decoder layer");
    if (fc_size < 1 || latent_size < 1 || max_batch < 1) return fail(CAE_ERR_ARG, "fc/latent/max_batch must be >= 1");
    cae_engine* e = new cae_engine();
    e->fc_size = fc_size;
    e->latent = latent_size;
    e->max_batch = max_batch;
    e->variational = variational;
    auto bad = [&](const char* msg, int i) {
        delete e;
        return fail(CAE_ERR_ARG, "layer %d: %s", i, msg);
    };
    // ---- geometry checks
    for (int i = 0; i < n_enc; i++) {
        const cae_layer_spec& s = enc[i];
        if (s.stride < 1 || s.k_h < 1 || s.k_w < 1 || s.in_c < 1 || s.out_c < 1) return bad("bad encoder spec", i);
        if (s.in_h < s.k_h || s.in_w < s.k_w) return bad("encoder kernel larger than input", i);
        if (s.out_h != (s.in_h - s.k_h) / s.stride + 1 || s.out_w != (s.in_w - s.k_w) / s.stride + 1)
            return bad("encoder output size != floor((in-k)/stride)+1", i);
        if (i > 0 && (enc[i - 1].out_c != s.in_c || enc[i - 1].out_h != s.in_h || enc[i - 1].out_w != s.in_w))
            return bad("encoder layer input does not match previous output", i);
    }
    for (int i = 0; i < n_dec; i++) {
        const cae_layer_spec& s = dec[i];
        if (s.stride < 1 || s.k_h < 1 || s.k_w < 1 || s.in_c < 1 || s.out_c < 1) return bad("bad decoder spec", i);
        if (s.output_padding < 0 || (s.output_padding >= s.stride && s.output_padding > 0))
            return bad("output_padding must be smaller than stride", i);
        if (s.out_h != (s.in_h - 1) * s.stride + s.k_h + s.output_padding ||
            s.out_w != (s.in_w - 1) * s.stride + s.k_w + s.output_padding)
            return bad("decoder output size != (in-1)*stride+k+output_padding", i);
        if (i > 0 && (dec[i - 1].out_c != s.in_c || dec[i - 1].out_h != s.in_h || dec[i - 1].out_w != s.in_w))
            return bad("decoder layer input does not match previous output", i);
    }
    e->in_c = enc[0].in_c;
    e->in_h = enc[0].in_h;
    e->in_w = enc[0].in_w;
    e->out_c = dec[n_dec - 1].out_c;
    e->out_h = dec[n_dec - 1].out_h;
    e->out_w = dec[n_dec - 1].out_w;

    // ---- parameter / buffer arenas in the reference's state_dict order
    int bn = 0;
    for (int i = 0; i < n_enc; i++) {
        const cae_layer_spec& s = enc[i];
        ConvLayer L{};
        L.transposed = false;
        L.cin = s.in_c; L.hin = s.in_h; L.win = s.in_w;
        L.cout = s.out_c; L.hout = s.out_h; L.wout = s.out_w;
        L.kh = s.k_h; L.kw = s.k_w; L.stride = s.stride; L.opad = 0;
        L.has_bn = true;
        L.bn_index = bn++;
        const std::string c = "enc/encoder_cnn." + std::to_string(3 * i);
        const std::string b = "enc/encoder_cnn." + std::to_string(3 * i + 1);
        L.w_off = e->tab.add(c + ".weight", 0, {L.cout, L.cin, L.kh, L.kw});
        L.b_off = e->tab.add(c + ".bias", 0, {L.cout});
        L.gamma_off = e->tab.add(b + ".weight", 0, {L.cout});
        L.beta_off = e->tab.add(b + ".bias", 0, {L.cout});
        L.rm_off = e->tab.add(b + ".running_mean", 1, {L.cout});
        L.rv_off = e->tab.add(b + ".running_var", 1, {L.cout});
        e->enc.push_back(L);
    }
    const ConvLayer& EL = e->enc.back();
    const int flat_enc = EL.cout * EL.hout * EL.wout;
    const int flat_dec = dec[0].in_c * dec[0].in_h * dec[0].in_w;
    const int heads = variational ? 2 * latent_size : latent_size;   // trunk mode: [mu | logvar]
    const int fdims[4][2] = {{flat_enc, fc_size}, {fc_size, heads}, {latent_size, fc_size}, {fc_size, flat_dec}};
    const char* fnames[4] = {"enc/encoder_lin.0", "enc/encoder_lin.2", "dec/decoder_lin.0", "dec/decoder_lin.2"};
    for (int i = 0; i < 4; i++) {
        FcLayer& F = e->fc[i];
        F.nin = fdims[i][0];
        F.nout = fdims[i][1];
        F.relu = (i == 0 || i == 2);
        if (i == 1 && variational) {
            // two named tensors per half, ONE (2 * latent, fc) matrix and ONE (2 * latent) bias vector in the arena: the table
            // lists mu.weight, mu.bias, logvar.weight, logvar.bias (the 'var' model's state_dict order) with those offsets
            F.w_off = e->tab.reserve(0, (int64_t)heads * F.nin);
            F.b_off = e->tab.reserve(0, heads);
            const std::string hn[2] = {"enc/encoder_mu", "enc/encoder_logvar"};
            for (int h = 0; h < 2; h++) {
                e->tab.list(hn[h] + ".weight", 0, {latent_size, F.nin}, F.w_off + (int64_t)h * latent_size * F.nin);
                e->tab.list(hn[h] + ".bias", 0, {latent_size}, F.b_off + (int64_t)h * latent_size);
            }
            continue;
        }
        F.w_off = e->tab.add(std::string(fnames[i]) + ".weight", 0, {F.nout, F.nin});
        F.b_off = e->tab.add(std::string(fnames[i]) + ".bias", 0, {F.nout});
    }
    for (int i = 0; i < n_dec; i++) {
        const cae_layer_spec& s = dec[i];
        ConvLayer L{};
        L.transposed = true;
        L.cin = s.in_c; L.hin = s.in_h; L.win = s.in_w;
        L.cout = s.out_c; L.hout = s.out_h; L.wout = s.out_w;
        L.kh = s.k_h; L.kw = s.k_w; L.stride = s.stride; L.opad = s.output_padding;
        L.has_bn = i != n_dec - 1;
        L.bn_index = L.has_bn ? bn++ : -1;
        const std::string c = "dec/decoder_conv." + std::to_string(3 * i);
        const std::string b = "dec/decoder_conv." + std::to_string(3 * i + 1);
        L.w_off = e->tab.add(c + ".weight", 0, {L.cin, L.cout, L.kh, L.kw});
        L.b_off = e->tab.add(c + ".bias", 0, {L.cout});
        if (L.has_bn) {
            L.gamma_off = e->tab.add(b + ".weight", 0, {L.cout});
            L.beta_off = e->tab.add(b + ".bias", 0, {L.cout});
            L.rm_off = e->tab.add(b + ".running_mean", 1, {L.cout});
            L.rv_off = e->tab.add(b + ".running_var", 1, {L.cout});
        }
        e->dec.push_back(L);
    }
    e->tab.close();
    e->n_bn = bn;
    // data parallelism: bucket boundary and the SyncBN collective order (forward: producers in layer order; backward: the
    // table of a layer's INPUT BatchNorm after that layer's input-gradient kernel) - see launch_forward / launch_backward
    e->bucket_split = e->fc[3].w_off;
    for (auto& L : e->enc) e->sync_order.push_back(L.bn_index);
    for (auto& L : e->dec)
        if (L.has_bn) e->sync_order.push_back(L.bn_index);
    for (int l = n_dec - 1; l >= 1; l--) e->sync_order.push_back(e->dec[l - 1].bn_index);
    e->sync_order.push_back(e->enc.back().bn_index);
    for (int l = n_enc - 1; l >= 1; l--) e->sync_order.push_back(e->enc[l - 1].bn_index);

    // ---- sharded accumulators for the layers the stride-2 kernels can take
    {
        int n = 0;
        for (size_t l = 0; l < e->dec.size(); l++) {
            ConvLayer& L = e->dec[l];
            // (... and the layers of the LDS-staged backward kernel, kernels_ctbwd.h: its workgroups all reach their weight-
            // gradient atomics at the same moment, one per image group and address; unsharded they queue up behind the
            // kernel's end - measured 8 us of a 16 us launch at the benchmark's third layer)
            // Which layers take it by default: one block of 16 input channels (no staging repeated per block) and few enough
            // weights that the optimiser's eight shard reads per weight stay cheap - at the benchmark geometry the 16 -> 8
            // layer: 169.6 against 171.5 us per step; the 32 -> 16 and 64 -> 32 layers lose (172.9 / 175.7 on their own).
            const bool ctb = l < 31 && L.transposed && L.stride == 2 && L.kh == 3 && L.kw == 3 && L.cin % 16 == 0 && L.cout % 4 == 0 &&
                             L.cin == 16 && L.cin * L.cout * 9 <= 2048;
            if (l == 0) e->ctbwd_auto = 0;
            if (ctb) e->ctbwd_auto |= 1 << l;
            e->ctbwd_mask = e->ctbwd_auto;
            if ((!s2_shape_ok(L) && !ctb) || e->segs.nseg + 2 > 12) continue;
            const int nw = L.cin * L.cout * L.kh * L.kw;
            L.sh_w = n;
            e->segs.seg[e->segs.nseg++] = ShardSeg{L.w_off, nw, n};
            n += (nw + 3) / 4 * 4;
            if (l + 1 == e->dec.size()) {
                L.sh_b = n;
                e->segs.seg[e->segs.nseg++] = ShardSeg{L.b_off, L.cout, n};
                n += (L.cout + 3) / 4 * 4;
            }
        }
        e->segs.n = n;
    }

    // ---- workspace carve
    Carver carve{256};
    e->off_state = carve(sizeof(StepState));
    e->off_losses = carve((int64_t)kLossSlots * kStatShards * sizeof(double));
    carve(1024 * 3 * sizeof(double));   // unused (held diagnostics once): the layout behind it stays as it was
    e->bn_stat_off.resize(bn);
    e->bn_saved_off.resize(bn);
    e->bn_channels.resize(bn);
    e->off_zero_begin = carve.top;
    auto reg_bn = [&](const ConvLayer& L) {
        if (!L.has_bn) return;
        e->bn_channels[L.bn_index] = L.cout;
        e->bn_stat_off[L.bn_index] = carve((int64_t)kStatShards * L.cout * 4 * sizeof(double));
        if (L.cout > e->max_channels) e->max_channels = L.cout;
    };
    for (auto& L : e->enc) reg_bn(L);
    for (auto& L : e->dec) reg_bn(L);
    e->off_gradacc = carve(e->tab.n_param * (int64_t)sizeof(double));
    e->off_sgacc = carve((int64_t)kStatShards * (e->segs.n > 0 ? e->segs.n : 4) * (int64_t)sizeof(double));
    e->off_zero_end = carve.top;
    for (auto& L : e->enc) e->bn_saved_off[L.bn_index] = carve((int64_t)L.cout * 2 * sizeof(float));
    for (auto& L : e->dec)
        if (L.has_bn) e->bn_saved_off[L.bn_index] = carve((int64_t)L.cout * 2 * sizeof(float));
    const int64_t mb = max_batch;
    for (auto& L : e->enc) {
        L.act_off = carve(mb * L.out_elems() * 4);
        L.grad_off = carve(mb * L.out_elems() * 4);
    }
    for (int i = 0; i < 4; i++) {
        e->fc[i].act_off = carve(mb * e->fc[i].nout * 4);
        e->fc[i].grad_off = carve(mb * e->fc[i].nout * 4);
    }
    for (auto& L : e->dec) {
        if (!L.has_bn) continue;
        L.act_off = carve(mb * L.out_elems() * 4);
        L.grad_off = carve(mb * L.out_elems() * 4);
    }
    e->off_glast = carve(mb * e->dec.back().out_elems() * 4);
    e->off_xbatch = carve((mb * e->enc[0].in_elems() + e->enc[0].cout) * 4);   // + the layer's gamma before the update
    if (variational) {
        e->off_vz = carve(mb * latent_size * 4);
        e->off_vgz = carve(mb * latent_size * 4);
        e->off_zlast = carve(mb * e->dec.back().out_elems() * 4);
    }
    // weight-gradient partial slabs, last: every offset above stays where it was
    e->wslab_bytes = wgrad_slab_capacity(e);
    e->off_wslab = carve(std::max<int64_t>(e->wslab_bytes, 256));
    e->ws_need = carve.top;
    for (auto& L : e->enc)
        if (L.cin > e->max_channels) e->max_channels = L.cin;
    for (auto& L : e->dec)
        if (L.cin > e->max_channels) e->max_channels = L.cin;
    if (lds_bytes(e->max_channels, e->max_channels) > 60 * 1024) {
        delete e;
        return fail(CAE_ERR_ARG, "channel count %d exceeds the LDS constant table", e->max_channels);
    }
    *out = e;
    return CAE_OK;
}

void cae_engine_destroy(cae_engine* e) {
    if (!e) return;
    e->drop_graphs();
    (void)cae_dp_shutdown(e);
    delete e;
}

int64_t cae_param_count(const cae_engine* e) { return e ? e->tab.n_param : 0; }
int64_t cae_buffer_count(const cae_engine* e) { return e ? e->tab.n_buf : 0; }
int cae_tensor_count(const cae_engine* e) { return e ? e->tab.count() : 0; }
int cae_tensor_info(const cae_engine* e, int index, cae_tensor_info_t* out) {
    return e ? e->tab.info(index, out) : fail(CAE_ERR_ARG, "tensor index out of range");
}
int64_t cae_workspace_bytes(const cae_engine* e) { return e ? e->ws_need : 0; }
int cae_loss_slots(const cae_engine*) { return kLossSlots; }

int cae_bind(cae_engine* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* buffers,
             void* workspace, int64_t workspace_bytes) {
    if (!e || !params || !grads || !exp_avg || !exp_avg_sq || !buffers || !workspace)
        return fail(CAE_ERR_ARG, "cae_bind: null pointer");
    if (workspace_bytes < e->ws_need)
        return fail(CAE_ERR_ARG, "workspace too small: %lld < %lld", (long long)workspace_bytes, (long long)e->ws_need);
    if (((uintptr_t)workspace & 255) != 0) return fail(CAE_ERR_ARG, "workspace must be 256-byte aligned");
    e->drop_graphs();
    e->lr_stale = true;   // a new workspace: its step state has no rate yet
    e->params = params;
    e->grads = grads;
    e->m = exp_avg;
    e->v = exp_avg_sq;
    e->bufs = buffers;
    e->ws = static_cast<char*>(workspace);
    return CAE_OK;
}

int cae_set_stream(cae_engine* e, void* hip_stream) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    if (e->stream != (hipStream_t)hip_stream) {
        e->drop_graphs();
        e->lr_stale = true;   // written again in the new stream's order
    }
    e->stream = (hipStream_t)hip_stream;
    return CAE_OK;
}

int cae_set_graph_mode(cae_engine* e, int enabled) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    e->graph_mode = enabled != 0;
    if (!e->graph_mode) e->drop_graphs();
    return CAE_OK;
}

int cae_set_capture_only(cae_engine* e, int enabled) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    e->capture_only = enabled != 0;
    return CAE_OK;
}

int cae_set_kernel_mode(cae_engine* e, int specialised) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    const int ctb = (specialised & 2) ? 0x7fffffff : e->ctbwd_auto;   // bit 1: every eligible layer
    const bool gather = (specialised & 4) != 0;
    const bool atomics = (specialised & 8) != 0;
    if (e->use_s2 != ((specialised & 1) != 0) || ctb != e->ctbwd_mask || gather != e->gather_fwd || atomics != e->wgrad_atomics)
        e->drop_graphs();
    e->use_s2 = (specialised & 1) != 0;
    e->ctbwd_mask = ctb;
    e->gather_fwd = gather;
    e->wgrad_atomics = atomics;
    return CAE_OK;
}

int cae_set_hyper(cae_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    Hyper h{lr, beta1, beta2, eps, weight_decay};
    // betas, eps and weight decay are baked into captured launches; the rate is device state (StepState::lr)
    if (h.beta1 != e->hp.beta1 || h.beta2 != e->hp.beta2 || h.eps != e->hp.eps || h.wd != e->hp.wd) e->drop_graphs();
    e->hp = h;
    e->lr_stale = true;
    return push_lr(e);
}

int cae_set_lr(cae_engine* e, double lr) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    e->hp.lr = lr;
    e->lr_stale = true;
    return push_lr(e);
}

int cae_set_dataset(cae_engine* e, int which, const float* x, const float* t, int64_t n) {
    if (!e || which < 0 || which > 1 || !x || n < 1) return fail(CAE_ERR_ARG, "cae_set_dataset: bad argument");
    if (e->ds_x[which] != x || e->ds_t[which] != t) e->drop_graphs();
    e->ds_x[which] = x;
    e->ds_t[which] = t;
    e->ds_n[which] = n;
    return CAE_OK;
}

int cae_set_cursor(cae_engine* e, int64_t batch_start, int loss_slot) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (loss_slot < 0 || loss_slot >= kLossSlots) return fail(CAE_ERR_ARG, "loss slot out of range");
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream, e->state(), (long long)batch_start, loss_slot, 1, 0, 0);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_set_adam_step(cae_engine* e, int completed_steps) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, e->stream, e->state(), 0LL, 0, 0, completed_steps, 1);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_train_step(cae_engine* e, int which, const int32_t* perm, int batch) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    StepArgs a{which, perm, batch, batch, batch, true, true, nullptr, nullptr, true};
    return run_op(e, OP_TRAIN, a, true);
}

int cae_train_steps(cae_engine* e, int which, const int32_t* perm, int batch, int nsteps) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    if (nsteps < 1 || nsteps > 4096) return fail(CAE_ERR_ARG, "nsteps %d outside [1, 4096]", nsteps);
    StepArgs a{which, perm, batch, batch, batch, true, true, nullptr, nullptr, true};
    a.nsteps = nsteps;
    return run_op(e, OP_TRAIN, a, true);
}

int cae_eval_steps(cae_engine* e, int which, const int32_t* perm, int batch, int nsteps) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    if (nsteps < 1 || nsteps > 4096) return fail(CAE_ERR_ARG, "nsteps %d outside [1, 4096]", nsteps);
    StepArgs a{which, perm, batch, batch, batch, false, true, nullptr, nullptr, true};
    a.nsteps = nsteps;
    return run_op(e, OP_EVAL, a, true);
}

int cae_forward_backward(cae_engine* e, int which, const int32_t* perm, int batch, int global_batch) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    if (global_batch < batch) return fail(CAE_ERR_ARG, "global_batch < batch");
    StepArgs a{which, perm, batch, global_batch, batch, true, true, nullptr, nullptr, true};
    return run_op(e, OP_FWDBWD, a, true);
}

int cae_forward_backward_sync(cae_engine* e, int which, const int32_t* perm, int batch, int global_batch, int world,
                              cae_allreduce_fn fn, void* user) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    if (global_batch < batch || world < 1 || !fn) return fail(CAE_ERR_ARG, "cae_forward_backward_sync: bad argument");
    StepArgs a{which, perm, batch, global_batch, global_batch, true, true, nullptr, nullptr, true};
    a.sync_fn = fn;
    a.sync_user = user;
    a.world = world;
    return run_op(e, OP_FWDBWD, a, false);   // plain launches: the callback runs between them
}

// ---- data parallelism inside the library ---------------------------------------------------------

int cae_dp_unique_id(void* id128_host) {
    if (!id128_host) return fail(CAE_ERR_ARG, "cae_dp_unique_id: null pointer");
    if (const char* why = rccl().load()) return fail(CAE_ERR_STATE, "RCCL: %s", why);
    RcclApi::UniqueId id;
    NCCL_TRY(rccl().GetUniqueId(&id));
    memcpy(id128_host, id.internal, sizeof id.internal);
    return CAE_OK;
}

int cae_dp_shutdown(cae_engine* e) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    if (e->dp_comm) {
        e->drop_graphs();
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);
        (void)rccl().CommDestroy(e->dp_comm);
        e->dp_comm = nullptr;
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->comm_stream) (void)hipStreamDestroy(e->comm_stream);
    e->ev_fork = e->ev_join = nullptr;
    e->comm_stream = nullptr;
    e->dp_world = 0;
    return CAE_OK;
}

namespace {

// cae_dp_init's self-test: the fork / all-reduce / join pattern of a data-parallel step, captured into a hipGraph and
// replayed twice on ones: every element must read world^2 afterwards.  A capture or replay ERROR switches the engine to
// plain launches for data-parallel steps (dp_graph_ok = false); wrong VALUES fail the init.
int dp_self_test(cae_engine* e) {
    hipStream_t s = e->stream;
    const int64_t n = e->tab.n_param, mid = e->bucket_split;
    auto body = [&]() -> int {
        HIP_TRY(hipEventRecord(e->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(e->comm_stream, e->ev_fork, 0));
        if (int rc = dp_allreduce_grads(e, mid, n, e->comm_stream)) return rc;
        HIP_TRY(hipEventRecord(e->ev_join, e->comm_stream));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
        if (int rc = dp_allreduce_grads(e, 0, mid, s)) return rc;
        return CAE_OK;
    };
    auto fill = [&]() {
        hipLaunchKernelGGL(k_fill_f32, dim3(grid1(n)), dim3(256), 0, s, e->grads, (long long)n, 1.0f);
    };
    auto check = [&](double want, const char* what) -> int {
        float got[2] = {0.f, 0.f};
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(&got[0], e->grads, sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&got[1], e->grads + n - 1, sizeof(float), hipMemcpyDeviceToHost));
        if ((double)got[0] != want || (double)got[1] != want)
            return fail(CAE_ERR_STATE, "RCCL self-test (%s): all-reduce of ones gave %g / %g, expected %g", what, got[0], got[1], want);
        return CAE_OK;
    };
    // plain launches first: RCCL sets its channels up on the first collective of each size class, outside any capture
    fill();
    if (int rc = body()) return rc;
    if (int rc = check((double)e->dp_world, "plain")) return rc;
    e->dp_graph_ok = s != nullptr;
    if (!e->dp_graph_ok) return CAE_OK;
    fill();
    HIP_TRY(hipStreamSynchronize(s));
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        const int rc = body();
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        ok = rc == CAE_OK && ce == hipSuccess && graph != nullptr;
    }
    if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (ok) ok = hipGraphLaunch(exec, s) == hipSuccess && hipGraphLaunch(exec, s) == hipSuccess;
    if (ok) ok = hipStreamSynchronize(s) == hipSuccess;
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    if (!ok) {
        e->dp_graph_ok = false;   // data-parallel steps run as plain launches; the compute path is the same
        fprintf(stderr, "libcae_hip: RCCL collectives could not be captured into a hipGraph here; data-parallel steps use plain launches\n");
        return CAE_OK;
    }
    return check((double)e->dp_world * e->dp_world, "captured");
}

}  // namespace

int cae_dp_init(cae_engine* e, int world, int rank, const void* id128_host) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (world < 1 || rank < 0 || rank >= world || !id128_host) return fail(CAE_ERR_ARG, "cae_dp_init: bad argument");
    if (!e->stream) return fail(CAE_ERR_STATE, "cae_dp_init needs a non-default stream (cae_set_stream)");
    if (const char* why = rccl().load()) return fail(CAE_ERR_STATE, "RCCL: %s", why);
    (void)cae_dp_shutdown(e);
    RcclApi::UniqueId id;
    memcpy(id.internal, id128_host, sizeof id.internal);
    NCCL_TRY(rccl().CommInitRank(&e->dp_comm, world, id, rank));
    e->dp_world = world;
    e->dp_rank = rank;
    HIP_TRY(hipStreamCreateWithFlags(&e->comm_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // warm the size classes a step uses: the two gradient buckets (self-test) and the BatchNorm tables (fp64, on the
    // main stream), on the gradient arena as scratch - its contents mean nothing between steps
    if (int rc = dp_self_test(e)) return rc;
    // the whole arena in one collective (the structure without overlap): its size class too is met outside any capture first
    if (int rc = dp_allreduce_grads(e, 0, e->tab.n_param, e->stream)) return rc;
    for (int c : e->bn_channels) {
        const size_t nd = (size_t)kStatShards * c * 4;
        if ((int64_t)nd * 2 > e->tab.n_param) continue;
        NCCL_TRY(rccl().AllReduce(e->grads, e->grads, nd, RcclApi::kFloat64, RcclApi::kSum, e->dp_comm, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->comm_stream));
    return CAE_OK;
}

int cae_dp_info(const cae_engine* e, int* world, int* rank, int* graph_capture) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    if (world) *world = e->dp_world;
    if (rank) *rank = e->dp_rank;
    if (graph_capture) *graph_capture = e->dp_comm && e->dp_graph_ok && e->graph_mode ? 1 : 0;
    return CAE_OK;
}

int cae_dp_set_overlap(cae_engine* e, int enabled) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    if (e->dp_overlap != (enabled != 0)) e->drop_graphs();
    e->dp_overlap = enabled != 0;
    return CAE_OK;
}

int cae_dp_broadcast_state(cae_engine* e, int root, int what) {
    if (!e || !e->dp_comm) return fail(CAE_ERR_STATE, "cae_dp_init has not been called");
    if (root < 0 || root >= e->dp_world) return fail(CAE_ERR_ARG, "cae_dp_broadcast_state: bad root");
    hipStream_t s = e->stream;
    auto bc = [&](float* p, int64_t n) -> int {
        if (n > 0) NCCL_TRY(rccl().Broadcast(p, p, (size_t)n, RcclApi::kFloat32, root, e->dp_comm, s));
        return CAE_OK;
    };
    if (what & 1) if (int rc = bc(e->params, e->tab.n_param)) return rc;
    if (what & 2) if (int rc = bc(e->bufs, e->tab.n_buf)) return rc;
    if (what & 4) {
        if (int rc = bc(e->m, e->tab.n_param)) return rc;
        if (int rc = bc(e->v, e->tab.n_param)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return CAE_OK;
}

int cae_dp_train_steps(cae_engine* e, int which, const int32_t* perm, int batch, int global_batch, int sync_bn, int nsteps) {
    if (!e || !e->dp_comm) return fail(CAE_ERR_STATE, "cae_dp_init has not been called");
    if (batch == 0) {   // an empty shard (a last batch shorter than the number of ranks): collectives only
        if (!e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    } else if (int rc = check_ready(e, which, batch, true)) {
        return rc;
    }
    if (global_batch < batch || global_batch < 1) return fail(CAE_ERR_ARG, "global_batch %d < batch %d", global_batch, batch);
    if (nsteps < 1 || nsteps > 4096) return fail(CAE_ERR_ARG, "nsteps %d outside [1, 4096]", nsteps);
    StepArgs a{which, perm, batch, global_batch, sync_bn ? global_batch : batch, true, true, nullptr, nullptr, true};
    a.nsteps = nsteps;
    a.dp = true;
    a.dp_sync = sync_bn != 0;
    a.world = sync_bn ? e->dp_world : 1;   // BatchNorm parameter gradients come from GLOBAL sums under SyncBN: 1/world each
    a.cursor_inc = global_batch;           // consecutive steps of a rank are one GLOBAL batch apart in the frozen permutation
    return run_op(e, OP_DP_TRAIN, a, e->dp_graph_ok);
}

int cae_dp_train_step(cae_engine* e, int which, const int32_t* perm, int batch, int global_batch, int sync_bn) {
    return cae_dp_train_steps(e, which, perm, batch, global_batch, sync_bn, 1);
}

int cae_dp_eval_steps(cae_engine* e, int which, const int32_t* perm, int batch, int global_batch, int nsteps) {
    if (!e || !e->dp_comm) return fail(CAE_ERR_STATE, "cae_dp_init has not been called");
    if (global_batch < batch || global_batch < 1) return fail(CAE_ERR_ARG, "global_batch %d < batch %d", global_batch, batch);
    if (nsteps < 1 || nsteps > 4096) return fail(CAE_ERR_ARG, "nsteps %d outside [1, 4096]", nsteps);
    if (batch == 0) {   // empty shard: only the cursor and the loss slot move
        if (!e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
        if (e->capture_only) return CAE_OK;
        for (int i = 0; i < nsteps; i++) hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, e->stream, e->state(), global_batch, 1, 0);
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
    if (int rc = check_ready(e, which, batch, true)) return rc;
    StepArgs a{which, perm, batch, global_batch, batch, false, true, nullptr, nullptr, true};
    a.nsteps = nsteps;
    a.cursor_inc = global_batch;
    return run_op(e, OP_EVAL, a, true);
}

int cae_dp_read_losses(cae_engine* e, int first, int count, double* host_out) {
    if (!e || !e->dp_comm) return fail(CAE_ERR_STATE, "cae_dp_init has not been called");
    if (first < 0 || count < 0 || first + count > kLossSlots || !host_out) return fail(CAE_ERR_ARG, "bad loss range");
    if (count == 0) return CAE_OK;
    double* dev = e->losses() + (size_t)first * kStatShards;
    // every rank's slot holds sum(local terms) / global count: the sum over ranks is the global-batch mean
    NCCL_TRY(rccl().AllReduce(dev, dev, (size_t)count * kStatShards, RcclApi::kFloat64, RcclApi::kSum, e->dp_comm, e->stream));
    return cae_read_losses(e, first, count, host_out);
}

int cae_adam_step(cae_engine* e) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    StepArgs a{0, nullptr, 0, 0, 0, false, false, nullptr, nullptr, false};
    return run_op(e, OP_ADAM, a, true);
}

int cae_eval_step(cae_engine* e, int which, const int32_t* perm, int batch) {
    int rc = check_ready(e, which, batch, true);
    if (rc) return rc;
    StepArgs a{which, perm, batch, batch, batch, false, true, nullptr, nullptr, true};
    return run_op(e, OP_EVAL, a, true);
}

int cae_score(cae_engine* e, const float* x, int batch, float* y) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (!x || !y) return fail(CAE_ERR_ARG, "cae_score: null pointer");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "batch %d outside [1, %d]", batch, e->max_batch);
    StepArgs a{0, nullptr, batch, batch, batch, false, false, x, y, false};
    return run_op(e, OP_EVAL, a, false);
}

int cae_encode(cae_engine* e, const float* x, int batch, float* z) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (!x || !z) return fail(CAE_ERR_ARG, "cae_encode: null pointer");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "batch %d outside [1, %d]", batch, e->max_batch);
    StepArgs a{0, nullptr, batch, batch, batch, false, false, x, nullptr, false};
    a.part = 1;
    a.z_out = z;
    return run_op(e, OP_EVAL, a, false);
}

int cae_decode(cae_engine* e, const float* z, int batch, float* y) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (!z || !y) return fail(CAE_ERR_ARG, "cae_decode: null pointer");
    if (batch < 1 || batch > e->max_batch) return fail(CAE_ERR_ARG, "batch %d outside [1, %d]", batch, e->max_batch);
    StepArgs a{0, nullptr, batch, batch, batch, false, false, nullptr, y, false};
    a.part = 2;
    a.z_in = z;
    return run_op(e, OP_EVAL, a, false);
}

int cae_read_losses(cae_engine* e, int first, int count, double* host_out) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    if (first < 0 || count < 0 || first + count > kLossSlots || !host_out) return fail(CAE_ERR_ARG, "bad loss range");
    if (count == 0) return CAE_OK;
    std::vector<double> raw((size_t)count * kStatShards);
    double* dev = e->losses() + (size_t)first * kStatShards;
    HIP_TRY(hipMemcpyAsync(raw.data(), dev, raw.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemsetAsync(dev, 0, raw.size() * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < count; i++) {
        double t = 0.0;
        for (int sh = 0; sh < kStatShards; sh++) t += raw[(size_t)i * kStatShards + sh];
        host_out[i] = t;
    }
    return CAE_OK;
}

int cae_sync(cae_engine* e) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CAE_OK;
}

int cae_graph_count(const cae_engine* e) { return e ? (int)e->graphs.size() : 0; }
int64_t cae_graph_captures(const cae_engine* e) { return e ? (int64_t)e->captures : 0; }

// ---- roctx ranges (SURVEY.md §5 tracing): visible in `rocprofv3 --marker-trace`, free when no profiler is attached ----------
namespace {
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
    void load() {
        if (tried) return;
        tried = true;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr;
                pop = nullptr;
            }
        }
    }
};
RoctxApi g_roctx;
}  // namespace

int cae_trace_range_push(const char* name) {
    g_roctx.load();
    if (!g_roctx.push || !name) return 0;
    g_roctx.push(name);
    return 1;
}

int cae_trace_range_pop(void) {
    if (!g_roctx.pop) return 0;
    g_roctx.pop();
    return 1;
}

int64_t cae_debug_read(cae_engine* e, const char* what, int index, void* host_out, int64_t cap) {
    if (!e || !e->ws || !what || !host_out) return fail(CAE_ERR_ARG, "cae_debug_read: bad argument");
    const void* src = nullptr;
    int64_t n = 0, esz = 4;
    const int64_t mb = e->max_batch;
    const std::string w(what);
    const int n_enc = (int)e->enc.size(), n_dec = (int)e->dec.size();
    auto conv_at = [&](int i) -> const ConvLayer* {
        if (i < 0) return nullptr;
        if (i < n_enc) return &e->enc[i];
        if (i < n_enc + n_dec - 1) return &e->dec[i - n_enc];
        return nullptr;
    };
    if (w == "act" || w == "grad") {
        const ConvLayer* L = conv_at(index);
        if (!L) return fail(CAE_ERR_ARG, "layer index out of range");
        src = e->ws + (w == "act" ? L->act_off : L->grad_off);
        n = mb * L->out_elems();
    } else if (w == "glast") {
        src = e->ws + e->off_glast;
        n = mb * e->dec.back().out_elems();
    } else if (w == "vgz") {   // trunk mode: dL/dz as Linear 2's backward stored it, before the reparameterisation hook
        if (!e->variational) return fail(CAE_ERR_ARG, "'vgz' is the variational trunk's");
        src = e->ws + e->off_vgz;
        n = mb * e->latent;
    } else if (w == "latent") {
        src = e->ws + e->fc[1].act_off;
        n = mb * e->fc[1].nout;
    } else if (w == "fc") {
        if (index < 0 || index > 3) return fail(CAE_ERR_ARG, "fc index out of range");
        src = e->ws + e->fc[index].act_off;
        n = mb * e->fc[index].nout;
    } else if (w == "fcgrad") {
        if (index < 0 || index > 3) return fail(CAE_ERR_ARG, "fc index out of range");
        src = e->ws + e->fc[index].grad_off;
        n = mb * e->fc[index].nout;
    } else if (w == "grad_acc") {
        src = e->gradacc();
        n = e->tab.n_param;
        esz = 8;
    } else if (w == "bn_stats") {
        if (index < 0 || index >= e->n_bn) return fail(CAE_ERR_ARG, "bn index out of range");
        src = e->bn_stats(index);
        n = (int64_t)kStatShards * e->bn_channels[index] * 4;
        esz = 8;
    } else {
        return fail(CAE_ERR_ARG, "unknown tensor '%s'", what);
    }
    if (n > cap) n = cap;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(host_out, src, (size_t)(n * esz), hipMemcpyDeviceToHost));
    return n;
}

// Measurement aid: per-node cost of a captured graph of n dependent no-op kernels on the engine's stream.
int cae_debug_launch_floor(cae_engine* e, int n, double* micros_per_kernel) {
    if (!e || !e->ws || !e->stream || n < 1 || !micros_per_kernel) return fail(CAE_ERR_ARG, "cae_debug_launch_floor: bad argument");
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < n; i++) hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, e->stream, e->state(), 0, 0, 0);
    HIP_TRY(hipStreamEndCapture(e->stream, &graph));
    HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) HIP_TRY(hipGraphLaunch(exec, e->stream));
    HIP_TRY(hipEventRecord(e0, e->stream));
    const int reps = 10;
    for (int i = 0; i < reps; i++) HIP_TRY(hipGraphLaunch(exec, e->stream));
    HIP_TRY(hipEventRecord(e1, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *micros_per_kernel = (double)ms * 1000.0 / (reps * (double)n);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    return CAE_OK;
}

int cae_profile_begin(cae_engine* e) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "cae_bind has not been called");
    for (auto& r : e->prof) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    e->prof.clear();
    e->profiling = true;
    return CAE_OK;
}

int cae_profile_end(cae_engine* e, cae_profile_rec* out, int capacity) {
    if (!e) return fail(CAE_ERR_ARG, "null engine");
    e->profiling = false;
    HIP_TRY(hipStreamSynchronize(e->stream));
    int n = 0;
    for (auto& r : e->prof) {
        float ms = 0.f;
        hipError_t rc = hipEventElapsedTime(&ms, r.e0, r.e1);
        if (rc == hipSuccess && out && n < capacity) {
            memset(&out[n], 0, sizeof out[n]);
            snprintf(out[n].name, sizeof out[n].name, "%s", r.name);
            out[n].layer = r.layer;
            out[n].micros = (double)ms * 1000.0;
            out[n].bytes = r.bytes;
            n++;
        }
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    e->prof.clear();
    return n;
}

}  // extern "C"

#include "kernels_scene.h"   // the scene kernels, after every kernel of the step: those keep their places in the code object
#include "kernels_residual.h"   // likewise: its fold is no template and is emitted here
#include "stateless_host.h"

// =================================================================================================
// trunk_api.h: the engine as the convolutional trunk of the 'var' model (vae_engine.hip)
// =================================================================================================
namespace cae_internal {

int trunk_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size, int latent_size,
                 int max_batch, cae_engine** out) {
    return engine_create_impl(enc, n_enc, dec, n_dec, fc_size, latent_size, max_batch, true, out);
}

void trunk_set_hooks(cae_engine* e, const TrunkHooks& hooks) { e->hooks = hooks; }

float* trunk_raw_output(cae_engine* e) { return e->fptr(e->off_zlast); }
float* trunk_output_gradient(cae_engine* e) { return e->fptr(e->off_glast); }
double* trunk_output_bias_acc(cae_engine* e) { return e->gradacc() + e->dec.back().b_off; }
float* trunk_latent(cae_engine* e) { return e->fptr(e->off_vz); }

// sync.sync_bn(): every launch that completes a BatchNorm sum table is followed by the callback (SyncBN over
// sync.global_batch rows: the means, variances and running-statistics updates use the global count, and the BatchNorm parameter
// gradients are each rank's 1/world share of the global sums).  Otherwise per-rank statistics, today's launches.
// The kernels that fold a BatchNorm table's production and consumption into one launch do not run here with a callback: the
// fused k_head_fwd / k_tail_bwd (which recompute statistics inside one launch) never in trunk mode (head_plan / tail_plan refuse
// a variational engine), k_conv_bwd_pair and the AdamConv0 fold never while syncing().  So a SyncBN trunk step takes the
// per-layer path: every table is produced by one launch, handed to the callback, and only then read by the next.
static StepArgs trunk_args(const float* x, int batch, bool train, const ShardSync& sync) {
    StepArgs a{0, nullptr, batch, batch, batch, train, false, x, nullptr, false};
    if (sync.sync_bn()) {
        a.sync_fn = sync.fn;
        a.sync_user = sync.user;
        a.world = sync.world;
        a.global_batch = a.bn_batch = sync.global_batch;
        a.ordered = true;
    }
    return a;
}

// The forward (fwd) or backward half of an EMPTY shard's training step under SyncBN: no launch reads rows, but the callbacks of
// the other ranks are made in the same order (sync_order: the forward tables, then the backward ones) with this rank's zero
// tables, and after each one k_bn_empty_shard does what the other ranks' consumers do with it - the running statistics advance
// from the forward sums, dgamma / dbeta take this rank's share of the backward sums - so that the ranks stay identical.
static int trunk_empty_shard(cae_engine* e, const StepArgs& a, bool fwd) {
    if (!a.syncing()) return CAE_OK;
    size_t n_fwd = e->enc.size();
    for (auto& L : e->dec) n_fwd += L.has_bn ? 1 : 0;
    const size_t lo = fwd ? 0 : n_fwd, hi = fwd ? n_fwd : e->sync_order.size();
    for (size_t k = lo; k < hi; k++) {
        const int bn = e->sync_order[k];
        const ConvLayer* P = nullptr;
        for (auto& L : e->enc) P = L.bn_index == bn ? &L : P;
        for (auto& L : e->dec) P = L.has_bn && L.bn_index == bn ? &L : P;
        if (int rc = sync_bn_table(e, a, bn)) return rc;
        BnDesc d = bn_none();
        BnGradOut bg;
        memset(&bg, 0, sizeof bg);
        if (fwd) {
            d = bn_of(e, *P, BN_BATCH, (double)a.bn_batch * P->hout * P->wout, 1);
        } else {
            bg.stats = e->bn_stats(bn);
            bg.gamma_acc = e->gradacc() + P->gamma_off;
            bg.beta_acc = e->gradacc() + P->beta_off;
            bg.C = P->cout;
            bg.scale = 1.0 / a.world;
        }
        hipLaunchKernelGGL(k_bn_empty_shard, dim3(1), dim3(256), (size_t)P->cout * sizeof(float4), e->stream, d, bg);
    }
    return CAE_OK;
}

int trunk_forward(cae_engine* e, const float* x, int batch, bool train, bool external_loss, float* yhat, const ShardSync& sync) {
    if (!e || !e->ws || !e->variational) return fail(CAE_ERR_STATE, "trunk_forward: not a bound trunk engine");
    const int min_batch = train && sync.fn ? 0 : 1;   // (an empty shard takes part in a data-parallel training step)
    if ((batch > 0 && !x) || batch < min_batch || batch > e->max_batch)
        return fail(CAE_ERR_ARG, "trunk_forward: batch %d outside [%d, %d]", batch, min_batch, e->max_batch);
    StepArgs a = trunk_args(x, batch, train, sync);
    a.external_loss = external_loss;
    a.yhat = yhat;
    if (train) {   // (see launch_one: every training forward starts from a clean first BatchNorm table; the others are cleared by
                   // the step tail of the optimiser / gradient hand-over launch)
        memset(&e->c0_pending, 0, sizeof e->c0_pending);
        e->sync_pos = 0;
    }
    if (batch == 0) {   // the empty shard: the optimiser step the first kernel would count, the first table's clear, the tables
        hipLaunchKernelGGL(k_bump_adam, dim3(1), dim3(1), 0, e->stream, e->state());
        HIP_TRY(hipMemsetAsync(e->bn_stats(e->enc[0].bn_index), 0, (size_t)kStatShards * e->enc[0].cout * 4 * sizeof(double), e->stream));
        if (int rc = trunk_empty_shard(e, a, true)) return rc;
    } else if (int rc = launch_forward(e, a)) {
        return rc;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// the two halves of the eval-mode forward on their own (cae_encode / cae_decode of the plain engine): the same per-layer launches
// as trunk_forward(train = false), cut after the heads / entered at the decoder's first Linear
static int trunk_part(cae_engine* e, const char* who, int part, const float* in, int batch, float* out) {
    if (!e || !e->ws || !e->variational) return fail(CAE_ERR_STATE, "%s: not a bound trunk engine", who);
    if (!in || !out || batch < 1 || batch > e->max_batch)
        return fail(CAE_ERR_ARG, "%s: null pointer or batch %d outside [1, %d]", who, batch, e->max_batch);
    StepArgs a = trunk_args(part == 1 ? in : nullptr, batch, false, ShardSync{});
    a.part = part;
    if (part == 1) a.z_out = out;
    else a.z_in = in, a.yhat = out;
    if (int rc = launch_forward(e, a)) return rc;
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int trunk_encode(cae_engine* e, const float* x, int batch, float* heads) { return trunk_part(e, "trunk_encode", 1, x, batch, heads); }
int trunk_decode(cae_engine* e, const float* z, int batch, float* yhat) { return trunk_part(e, "trunk_decode", 2, z, batch, yhat); }

int trunk_backward(cae_engine* e, const float* x, int batch, const ShardSync& sync) {
    if (!e || !e->ws || !e->variational) return fail(CAE_ERR_STATE, "trunk_backward: not a bound trunk engine");
    StepArgs a = trunk_args(x, batch, true, sync);
    a.external_loss = true;
    if (int rc = batch == 0 ? trunk_empty_shard(e, a, false) : launch_backward(e, a)) return rc;
    if (a.ordered && e->sync_pos != e->sync_order.size())
        return fail(CAE_ERR_STATE, "SyncBN: %zu of %zu tables passed to the callback", e->sync_pos, e->sync_order.size());
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int trunk_adam(cae_engine* e) {
    if (!e || !e->ws) return fail(CAE_ERR_STATE, "trunk_adam: not a bound engine");
    if (int rc = push_lr(e)) return rc;
    hipLaunchKernelGGL(k_adam, dim3(grid1(e->tab.n_param)), dim3(256), 0, e->stream, (long long)e->tab.n_param, e->params,
                       (const float*)nullptr, e->m, e->v, e->hp, (const StepState*)e->state(), e->shard_segs(),
                       step_tail_of(e, 0, 0), 0, std::log(e->hp.beta1), std::log(e->hp.beta2), AdamConv0{});
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int trunk_gradients(cae_engine* e, float* out, double scale) {
    if (!e || !e->ws || !out) return fail(CAE_ERR_STATE, "trunk_gradients: bad argument");
    hipLaunchKernelGGL(k_acc_to_f32, dim3(grid1(e->tab.n_param)), dim3(256), 0, e->stream, (long long)e->tab.n_param, out, e->shard_segs(),
                       step_tail_of(e, 0, 0));
    if (scale != 1.0)
        hipLaunchKernelGGL(k_scale_f32, dim3(grid1(e->tab.n_param)), dim3(256), 0, e->stream, out, (long long)e->tab.n_param, (float)scale);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int trunk_adam_from(cae_engine* e, const float* grads) {
    if (!e || !e->ws || !grads) return fail(CAE_ERR_STATE, "trunk_adam_from: bad argument");
    if (int rc = push_lr(e)) return rc;
    StepTail none;
    memset(&none, 0, sizeof none);
    hipLaunchKernelGGL(k_adam, dim3(grid1(e->tab.n_param)), dim3(256), 0, e->stream, (long long)e->tab.n_param, e->params, grads, e->m, e->v,
                       e->hp, (const StepState*)e->state(), e->shard_segs(), none, 0, std::log(e->hp.beta1), std::log(e->hp.beta2),
                       AdamConv0{});
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace cae_internal

// Where .text starts in this code object decides the training step's time (model comparison, "cost to the
// training step"): the tables in front of it grew with the comparison's kernels and moved it from 0x300 to 0xf00 past a 4 KiB
// boundary, which cost the step 0.8 us of 160.4; 1 KiB of constants put it back at 0x300.  k_dihedral_rows' descriptor and
// metadata moved it on by 0x500, to 0x800 past the boundary: 0xb00 more bytes of constants, and it stands at 0x300 again.
namespace cae { __device__ __attribute__((used)) const unsigned char k_layout_pad[0xf00] = {1}; }
