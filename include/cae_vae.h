/* cae_vae.h — C ABI of the 'var' (variational autoencoder + MS-SSIM) path of libcae_hip.so (gfx950 / MI355X).
 *
 * The reference has NO source for this path: `--method var` is the default of its train_cae CLI (cli/train_cae.py:42)
 * and model_evaluator.py:35 imports cae_tools.models.var_ae_model, but that file is missing from the repository; only
 * the flags --lambda-mse / --lambda-kl / --lambda-ssim (cli/train_cae.py:32-36) and README.md:29 (pytorch_msssim)
 * survive.  The model computed here is the build's own published definition (oracle/vae_oracle.py):
 *   encoder  = the ConvAE encoder stack (encoder.py:40-46) + Linear(F, fc) + ReLU + two heads Linear(fc, latent): mu, logvar
 *   z        = mu + eps * exp(logvar / 2) in training (eps from a counter-based hash), mu in eval / scoring
 *   decoder  = the ConvAE decoder (decoder.py:31-50,73-78)
 *   loss     = lambda_mse * MSE + lambda_kl * KL + lambda_ssim * (1 - MS-SSIM)   (5 scales, 11-tap gaussian, data range 1)
 *   Adam with L2 weight decay (conv_ae_model.py:310)
 * Layer geometry is cae_layer_spec exactly as for the ConvAE engine (no padding; output_padding on the decoder).
 * MS-SSIM needs output height and width that are multiples of 16 and at least 176.
 * Conventions as in cae_hip.h.  Steps are bitwise reproducible from run to run: the trunk's sums as on the ConvAE path, the
 * KL, MS-SSIM and MSE sums of this path on fixed accumulation grids.
 */
#ifndef CAE_VAE_H
#define CAE_VAE_H

#include <stdint.h>

#include "cae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vae_engine vae_engine;

int vae_engine_create(const cae_layer_spec* enc, int n_enc, const cae_layer_spec* dec, int n_dec, int fc_size,
                      int latent_size, int max_batch, vae_engine** out);
void vae_engine_destroy(vae_engine* e);
int64_t vae_param_count(const vae_engine* e);
int64_t vae_buffer_count(const vae_engine* e);
int vae_tensor_count(const vae_engine* e);
/* "enc/encoder_cnn.0.weight", ..., "enc/encoder_lin.0.*", "enc/encoder_mu.*", "enc/encoder_logvar.*", "dec/decoder_lin.{0,2}.*",
 * "dec/decoder_conv.{3j}.*", "dec/decoder_conv.{3j+1}.*" */
int vae_tensor_info(const vae_engine* e, int index, cae_tensor_info_t* out);
int64_t vae_workspace_bytes(const vae_engine* e);
int vae_bind(vae_engine* e, float* params_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* buffers_dev,
             void* workspace_dev, int64_t workspace_bytes);
int vae_set_stream(vae_engine* e, void* hip_stream);
int vae_set_hyper(vae_engine* e, double lr, double beta1, double beta2, double eps, double weight_decay, double lambda_mse,
                  double lambda_kl, double lambda_ssim, uint32_t noise_seed);
/* the learning rate alone (a scheduler step): forwarded to the trunk's cae_set_lr, in stream order */
int vae_set_lr(vae_engine* e, double lr);
/* 1 (default): the MS-SSIM passes run the row-streaming kernels (a wave walks a strip of 64 columns, DPP neighbours, register
 * ring); 0: the LDS tile kernels they replaced.  Same arithmetic in the same order: results equal to fp32 rounding (kept
 * selectable so that the parity tests can say so). */
int vae_set_kernel_mode(vae_engine* e, int mode);
int vae_set_step(vae_engine* e, int64_t step);
int vae_set_dataset(vae_engine* e, int which, const float* x_dev, const float* target_dev, int64_t n);
/* forward (train mode) + loss + backward + Adam on samples perm[start .. start+batch); the loss slot receives
 * {mse, kl, 1 - ms_ssim, total} */
int vae_train_step(vae_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot);
/* the same without the optimiser step: fp32 gradient of the total loss -> grads_dev (vae_param_count floats) */
int vae_forward_backward(vae_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot,
                          float* grads_dev, double grad_scale);
/* Data parallelism: every rank calls vae_forward_backward with grad_scale = local batch / global batch, the ranks SUM-all-reduce
 * grads_dev (torch.distributed on the same stream), then each applies the Adam step to the reduced gradient. */
int vae_apply_gradients(vae_engine* e, const float* grads_dev);
int vae_eval_step(vae_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int loss_slot);
/* Data parallelism with the single-device arithmetic (the shape of unet_forward_backward_sync, cae_unet.h): this rank holds rows
 * [row0, row0 + batch) of a global batch of global_batch rows (samples perm[start .. start+batch)), and a step equals the
 * one-device step at global_batch up to fp32 summation order.  The library calls fn(user, table_dev, count) (cae_hip.h) with
 * every fp64 table that must be summed over the ranks, once it is complete and before anything reads it; fn leaves the
 * element-wise SUM in place, ordered on the engine's stream, and returns 0.  The tables, in order: per BatchNorm layer its
 * forward sums (encoder layers, then decoder layers), the loss table {sum of squared errors, sum of KL terms, sum over (b, c)
 * of 1 - MS-SSIM} (3 doubles), then the BatchNorm backward sums from the decoder back to the first encoder layer: 2 calls per
 * BatchNorm layer + 1.  The noise eps of global row r is that of row r of a whole batch.  world >= 1: the BatchNorm statistics
 * are over the global batch (SyncBN); world 0: per rank (fn then sees the loss table only).  The loss slot receives the global
 * batch's {mse, kl, 1 - ms_ssim, total}; grads_dev receives this rank's share of the gradient of the global loss: the SUM over
 * the ranks is the gradient, which vae_apply_gradients applies.  batch 0 (an empty shard) is allowed and makes the same calls.
 * vae_eval_step_sync: the eval-mode counterpart (running statistics: the loss table only). */
int vae_forward_backward_sync(vae_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int row0,
                              int global_batch, int world, int loss_slot, float* grads_dev, cae_allreduce_fn fn, void* user);
int vae_eval_step_sync(vae_engine* e, int which, const int32_t* perm_dev, int64_t start, int batch, int row0,
                       int global_batch, int loss_slot, cae_allreduce_fn fn, void* user);
int vae_score(vae_engine* e, const float* x_dev, int batch, float* y_dev);
/* The model as a generative one (the build's own definition, parity unpinned).  All three run on the engine's
 * stream and take at most max_batch rows (vae_sample_latent: any number).
 * vae_encode: the eval-mode encoder (running statistics) up to the two heads: mu_dev and logvar_dev, (batch, latent) fp32 each.
 * vae_decode: the eval-mode decoder from a given latent z_dev (batch, latent), sigmoid applied: y_dev (batch, C, H, W).
 *   vae_score(x) is vae_decode(mu of vae_encode(x)): the same launches on the same values, bit for bit at the same batch.
 * vae_sample_latent: z[b][j] = mu[b][j] + eps * expf(0.5f * logvar[b][j]) with eps element (first_case + b) * latent + j of
 *   normal_noise(seed, step = draw, .) (oracle/vae_oracle.py), the counter-based noise of training; with n_draws > 1 the
 *   draws draw .. draw + n_draws - 1 in one launch, z_dev (n_draws, batch, latent).  A NULL mu_dev or logvar_dev
 *   stands for zeros (the prior).  The noise of a case depends on its index, the draw and the seed alone - not on batch, on
 *   how the cases are cut into calls, or on which rank holds them.  (first_case + batch) * latent must stay below 2^31: the
 *   hash index would wrap. */
int vae_encode(vae_engine* e, const float* x_dev, int batch, float* mu_dev, float* logvar_dev);
int vae_decode(vae_engine* e, const float* z_dev, int batch, float* y_dev);
int vae_sample_latent(vae_engine* e, const float* mu_dev, const float* logvar_dev, int batch, int64_t first_case, int64_t draw,
                      int n_draws, uint32_t seed, float* z_dev);
int vae_loss_slots(const vae_engine* e);
int vae_read_losses(vae_engine* e, int first_slot, int count, double* out_host);   /* 4 doubles per slot */
int vae_sync(vae_engine* e);
/* blocking debug read (count floats) of what the last training-mode step left in the workspace: the noise "eps" or the latent
 * "z" ((batch, latent) rows); the sigmoid output "y" or "gssim" = d(lambda_ssim * (1 - MS-SSIM)) / dy ((batch * channels, H, W)
 * planes; "y" is also left by an eval step, "gssim" only by a step that computes gradients) */
int vae_debug_read(vae_engine* e, const char* what, float* out_host, int64_t count);
/* Test hooks on the trunk, the ConvAE engine in trunk mode that runs every layer of this model (cae_hip.h):
 * vae_debug_plan: cae_debug_plan of the trunk, without a GPU - head and tail are "layers why=variational", the last decoder
 *   layer hands out its raw output (epi=raw) and is never fused with a loss.
 * vae_trunk_debug_read: cae_debug_read of the trunk ("act", "grad", "glast" = dL/d(raw output), "fc", "fcgrad", "latent" = the
 *   heads' rows [mu | logvar], "vgz" = dL/dz); returns the number of elements copied or a negative status. */
int vae_debug_plan(const vae_engine* e, int batch, int train, char* out_host, int64_t out_bytes);
int64_t vae_trunk_debug_read(vae_engine* e, const char* what, int index, void* host_out, int64_t capacity_elems);
/* the 11 window values of the MS-SSIM kernels (host only, no engine, no GPU): the fp32 values of the published definition */
void vae_gauss_window(float* out11_host);

#ifdef __cplusplus
}
#endif
#endif /* CAE_VAE_H */
