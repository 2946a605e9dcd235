/* cae_unet.h — C ABI of the UNET path of libcae_hip.so (gfx950 / MI355X).
 *
 * Replaces, for `--method unet`, these reference sites (file:line under src/cae_tools/models/unet.py):
 *
 *   :73-112   Encoder.__init__/forward  (Conv2d+BN+ReLU+Dropout stack, skip list, Linear-BN1d-ReLU-Dropout-Linear-ReLU-Dropout)
 *   :114-163  Decoder.__init__/forward  (Linear stack, ConvTranspose2d, ChannelAttention gate, skip concat, BN, ReLU, Dropout, sigmoid)
 *   :23-39    ChannelAttention
 *   :295-337  UNET.__train_epoch         -> unet_train_step per batch + unet_read_losses
 *   :339-370  UNET.__test_epoch          -> unet_eval_step per batch + unet_read_losses
 *   :373-382  UNET.score                 -> unet_score
 *   :457      torch.optim.AdamW(lr, weight_decay); :459 cosine schedule with eta_min == lr (constant rate)
 *   :635-639  masked_mse_loss, :641-678 pearson_corr_torch, combined at :316-321
 *
 * Layer geometry is cae_layer_spec (cae_hip.h); as in the reference's UNET modules the `output_padding` field
 * is the PADDING of both Conv2d (:82) and ConvTranspose2d (:140).  The model must have as many decoder as encoder
 * layers; decoder layer j < n-1 is followed by attention + concat with the encoder's ReLU output of layer n-2-j.
 *
 * Same conventions as cae_hip.h: plain pointers and sizes, *_dev = caller-owned device memory, every call returns
 * 0 or a negative cae_status with the message in cae_last_error(), work is enqueued on the stream given to
 * unet_set_stream.  All arithmetic fp32, reductions fp64.  Steps are bitwise reproducible from run to run: every fp64 sum over
 * workgroups adds addends rounded to a fixed grid (exact, hence order-independent), and a split-K convolution combines its K
 * slices in a fixed order.
 *
 * Dropout masks are a pure function of (seed, step, site, element index) (kernels_unet.h: pcg hash), not of
 * torch's generator: with dropout_rate 0 a step is the reference's arithmetic exactly.
 */
#ifndef CAE_UNET_H
#define CAE_UNET_H

#include <stdint.h>

#include "cae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct unet_engine unet_engine;

int unet_engine_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                       int latent_size, int max_batch, unet_engine** out);
void unet_engine_destroy(unet_engine* e);

int64_t unet_param_count(const unet_engine* e);   /* floats in the parameter arena */
int64_t unet_buffer_count(const unet_engine* e);  /* floats in the running-statistics arena */
int unet_tensor_count(const unet_engine* e);
/* names are the reference's state_dict keys with an "enc/" or "dec/" prefix, e.g. "dec/attention_layers.0.fc1.weight" */
int unet_tensor_info(const unet_engine* e, int index, cae_tensor_info_t* out);
int64_t unet_workspace_bytes(const unet_engine* e);

/* params / exp_avg / exp_avg_sq: unet_param_count floats each; buffers: unet_buffer_count floats;
 * workspace: unet_workspace_bytes bytes, 256-B aligned, zero-filled by the caller before the first use. */
int unet_bind(unet_engine* e, float* params_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* buffers_dev,
              void* workspace_dev, int64_t workspace_bytes);
int unet_set_stream(unet_engine* e, void* hip_stream);
/* 1 (default): MFMA kernels where a layer is eligible (4x4, stride 2, padding 1); 0: shape-generic kernels */
int unet_set_kernel_mode(unet_engine* e, int specialised);

/* unet.py:201-204 hyper-parameters; dropout_seed keys the dropout hash */
int unet_set_hyper(unet_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay,
                   double dropout_rate, double lambda_pearson, uint32_t dropout_seed);
/* the learning rate alone (a scheduler step): the launches of the next unet_train_step / unet_apply_gradients take it */
int unet_set_lr(unet_engine* e, double lr);
/* completed optimiser steps (AdamW bias correction uses step+1; the dropout hash uses step) */
int unet_set_step(unet_engine* e, int64_t step);

/* Resident data set `which` (0 train, 1 test): x (n, Cin, H, W), target (n, Cout, H, W), mask (n, mask_channels,
 * H, W) with mask_channels 1 or Cout, or mask_dev NULL (= ones; ds_dataset.py:152-156). */
int unet_set_dataset(unet_engine* e, int which, const float* x_dev, const float* target_dev, const float* mask_dev,
                     int mask_channels, int64_t n);

/* One iteration of __train_epoch (:307-325) on samples perm[start .. start+batch) (perm_dev NULL: start..):
 * forward (train mode), masked MSE + lambda*(1 - mean Pearson), backward, AdamW.  {mse, pearson loss} -> loss slot. */
int unet_train_step(unet_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot);
/* The same without the optimiser step: the fp32 gradient of the loss is written to grads_dev (unet_param_count). */
int unet_forward_backward(unet_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot,
                          float* grads_dev, double grad_scale);
/* Data parallelism: every rank calls unet_forward_backward with grad_scale = local batch / global batch, the ranks SUM-all-reduce
 * grads_dev (torch.distributed on the same stream), then each applies the AdamW step to the reduced gradient. */
int unet_apply_gradients(unet_engine* e, const float* grads_dev);
/* One iteration of __test_epoch (:347-361): eval-mode forward + the two losses -> loss slot. */
int unet_eval_step(unet_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot);

/* Data parallelism with the single-device arithmetic: this rank holds rows [row0, row0 + batch) of a global batch of
 * global_batch rows (samples perm[start .. start+batch)), and a step equals the one-device step at global_batch up to fp32
 * summation order.  The library calls fn(user, table_dev, count) (cae_hip.h) with every fp64 table that must be summed over
 * the ranks, once it is complete and before anything reads it; fn leaves the element-wise SUM in place, ordered on the
 * engine's stream, and returns 0.  The tables, in order: per BatchNorm layer its forward sums {sum y, sum y^2} (encoder
 * layers, encoder_lin.1, decoder_lin.1, then the decoder layers' concatenated tensors), the loss totals {sum mask, sum of
 * squared masked errors, sum of per-(b, c) Pearson r} (3 doubles), and the backward sums {sum g, sum g*xhat} from the
 * decoder back to the first encoder layer: 2 (2n + 1) + 1 calls for n levels, checked against that order (CAE_ERR_STATE).
 * Dropout masks are those of the rows' global indices.  world >= 1: the BatchNorm statistics are over the global batch
 * (SyncBN); world 0: per rank (fn then sees the loss table only).  grads_dev receives this rank's share of the gradient of
 * the global loss: the SUM over the ranks is the gradient, which unet_apply_gradients applies.  batch 0 (an empty shard) is
 * allowed and makes the same calls to fn.
 * unet_eval_step_sync: the eval-mode counterpart (the loss table only). */
int unet_forward_backward_sync(unet_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int row0,
                               int global_batch, int world, int loss_slot, float* grads_dev, cae_allreduce_fn fn, void* user);
int unet_eval_step_sync(unet_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int row0,
                        int global_batch, int loss_slot, cae_allreduce_fn fn, void* user);
/* UNET.score (:373-382): eval-mode forward of x (batch, Cin, H, W) -> y (batch, Cout, H, W). */
int unet_score(unet_engine* e, const float* x_dev, int batch, float* y_dev);
int unet_loss_slots(const unet_engine* e);
/* blocking: out[2*i] = mse, out[2*i+1] = 1 - mean Pearson of slot first+i */
int unet_read_losses(unet_engine* e, int first_slot, int count, double* out_host);
int unet_sync(unet_engine* e);
/* blocking debug read of an internal activation ("enc_z0", "enc_s0", "dec_u1", "dec_cat0", "att0", "y" ...) */
int unet_debug_read(unet_engine* e, const char* what, float* out_host, int64_t count);
/* the kernel plan of a step at this batch (train 1: training step, 0: eval / score), from the choosers the launch code
 * switches on; no bound workspace or GPU needed.  One line per layer, in order enc0.., fc0..fc3, dec0..:
 *   "enc<i> down=<family> up=<family> wgrad=<family> wp=<0|1> packed=<0|1>"   (dec<j> likewise; "-": not run in this mode)
 *   "fc<k> fwd=<family> bwd=<family>"
 * then "pack entries=<n> launches=<m>".  wp: the layer has a repack buffer; packed: its weights are repacked before the
 * step.  After these, every line carries what the launch of each family switches on below the family, as <op>.<field>=<value>,
 * each from the host function the launch itself calls:
 *   down=thin    down.rbn down.cl (template arguments) down.tpw down.groups (tiles per workgroup, workgroups per image) down.Ws
 *   down=patch   down.rbn down.nsplit (K slices after the room check of the partial maps: 1, 2 = atomics, > 2 = fold) down.Ws
 *   down=mfma    down.tile (rows x columns of the tile engine's tile) down.nsplit
 *   up=thin      up.cl up.waves up.wgs        up=up_thin  up.cl        up=patch  up.rbn up.Ws        up=mfma  up.tile
 *   wgrad=thin|thin_atomic   wgrad.rbn wgrad.tpw wgrad.groups
 *   wgrad=patch              wgrad.wrxwc wgrad.tpw wgrad.slices
 *   wgrad=mfma|mfma_atomic   wgrad.tile (or "1wave") wgrad.slices wgrad.per (chunks of 16 pixels per slice)
 *   fwd=lin_big  fwd.rb fwd.slices fwd.kiters fwd.partial (the last K tile is partly filled) fwd.ntiles fwd.nlast (column
 *                tiles, width of the last); training: bwd.rb bwd.slices bwd.kiters bwd.partial (the input gradient) and
 *                outer_lds (bytes of dynamic LDS of the weight-gradient kernel)
 *   fwd=tile     fwd.tile fwd.slices fwd.per; training: wgrad.tile wgrad.slices bwd.tile bwd.slices bwd.per
 * Writes a NUL-terminated string of at most out_bytes bytes. */
int unet_debug_plan(const unet_engine* e, int batch, int train, char* out_host, int64_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CAE_UNET_H */
