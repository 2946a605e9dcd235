"""VaeEngine — Python owner of one libcae_hip 'var' engine (include/cae_vae.h) and of its device memory (torch tensors as
containers, as in engine.py / unet_engine.py)."""
import numpy as np
import torch

from ._engine_base import TEST, TRAIN, ShardedSteps, SpecPlan, SteppedEngine, require_gpu  # noqa: F401  (public names)
from ._lib import CaeError, check


def check_noise_index(n_cases, latent_size):
    """the noise of case c, latent j is element c * latent + j of normal_noise(seed, draw, .): the hash doubles that index in 32
    bits, so n_cases * latent must stay below 2^31 (vae_sample_latent refuses as well)"""
    if int(n_cases) * int(latent_size) >= 2 ** 31:
        raise ValueError(f"{n_cases} cases x latent size {latent_size} reach noise index 2**31, where the hash index wraps: "
                         "apply the model to the cases in several parts")


class VaePlan(SpecPlan):
    """geometry-only view (no GPU needed): tensor table, arena and workspace sizes, the trunk's kernel plan"""

    PREFIX = "vae_"

    def kernel_plan(self, batch, train):
        """the kernels the trunk of a step at this batch runs (vae_debug_plan, include/cae_vae.h), no GPU needed: the dict of
        EnginePlan.kernel_plan for the ConvAE engine in trunk mode - head and tail on "layers" with why "variational", the last
        decoder layer with the raw epilogue and a backward of its own, "fc3" .. "fc0" for the four Linear backwards"""
        return self._plan_report(batch, train)


class VaeEngine(ShardedSteps, SteppedEngine, VaePlan):

    LOSSES_PER_BATCH = 4    # (mse, kl, 1 - ms_ssim, total)

    def __init__(self, spec, fc_size, latent_size, max_batch, device=None):
        require_gpu()
        super().__init__(spec, fc_size, latent_size, max_batch)
        self._bind(device, buffers=True)
        torch.cuda.synchronize(self.device)
        self._start()

    def set_hyper(self, lr=1e-3, weight_decay=1e-5, lambda_mse=1.0, lambda_kl=1.0, lambda_ssim=1.0, seed=0, betas=(0.9, 0.999),
                  eps=1e-8):
        check(self.lib.vae_set_hyper(self.handle, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                     float(lambda_mse), float(lambda_kl), float(lambda_ssim), int(seed) & 0xFFFFFFFF))

    def set_kernel_mode(self, mode):
        """1 (default): row-streaming MS-SSIM kernels; 0: the LDS tile kernels (same results to fp32 rounding; A/B and tests)"""
        check(self.lib.vae_set_kernel_mode(self.handle, int(mode)))

    def debug_read(self, what, shape):
        """what the last training-mode step left: the noise ("eps") or latent vector ("z"), rows of (batch, latent); the sigmoid
        output ("y") or the gradient of lambda_ssim * (1 - MS-SSIM) with respect to it ("gssim"), planes of (batch * channels, H, W)"""
        out = np.empty(shape, dtype=np.float32)
        check(self.lib.vae_debug_read(self.handle, what.encode(), out.ctypes.data, out.size))
        return out

    def trunk_read(self, what, index=0, count=None):
        """what the last training-mode step left in the trunk's workspace (vae_trunk_debug_read: cae_debug_read of the trunk):
        "act" / "grad" of conv layer `index` (encoder layers, then decoder layers but the last), "glast" = dL/d(raw output),
        "fc" / "fcgrad" of Linear `index` (1: the heads' rows [mu | logvar]), "vgz" = dL/dz; `count` floats (default: all)"""
        cap = int(count) if count is not None else (1 << 28)
        buf = np.empty(cap, dtype=np.float32)
        n = check(self.lib.vae_trunk_debug_read(self.handle, what.encode(), int(index), buf.ctypes.data, cap))
        return buf[:n]

    # ---- the model as a generative one (vae_encode / vae_decode / vae_sample_latent, include/cae_vae.h) -------------------
    def _rows(self, t, row_shape, what):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape[1:]) != tuple(row_shape):
            raise CaeError(f"{what} expects an fp32 CUDA tensor of rows {tuple(row_shape)}, got "
                           f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        return t.to(self.device).contiguous()

    def encode(self, x):
        """eval-mode encoder up to the two heads: (N, *in_shape) -> (mu, logvar), (N, latent) fp32 CUDA tensors each"""
        x = self._rows(x, self.in_shape, "encode()")
        n = x.shape[0]
        mu = torch.empty((n, self.latent_size), dtype=torch.float32, device=self.device)
        logvar = torch.empty_like(mu)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, n, self.max_batch):
            hi = min(n, lo + self.max_batch)
            check(self.lib.vae_encode(self.handle, x[lo:hi].data_ptr(), hi - lo, mu[lo:hi].data_ptr(), logvar[lo:hi].data_ptr()))
        self.sync()
        return mu, logvar

    def decode(self, z):
        """eval-mode decoder from a given latent, sigmoid applied: (N, latent) -> (N, *out_shape) fp32 CUDA tensor"""
        z = self._rows(z, (self.latent_size,), "decode()")
        out = torch.empty((z.shape[0],) + self.out_shape, dtype=torch.float32, device=self.device)
        self._chunked(self.lib.vae_decode, z, out)
        self.sync()
        return out

    def _sample_into(self, z, mu, logvar, first_case, draw, seed, n_draws=1):
        """z (n_draws, n, latent) contiguous <- the latents of cases first_case .. first_case + n of the draws draw .. draw +
        n_draws - 1, one launch on the engine's stream"""
        check(self.lib.vae_sample_latent(self.handle, None if mu is None else mu.data_ptr(),
                                         None if logvar is None else logvar.data_ptr(), int(z.numel() // (n_draws * self.latent_size)),
                                         int(first_case), int(draw), int(n_draws), int(seed) & 0xFFFFFFFF, z.data_ptr()))

    def sample_latent(self, mu, logvar, draw, seed=0, first_case=0, n=None):
        """z = mu + eps * exp(logvar / 2), (N, latent): eps is rows first_case .. first_case + N of normal_noise(seed, draw, .)
        (oracle/vae_oracle.py), whatever N.  mu = logvar = None draws n rows from the prior."""
        if (mu is None) != (logvar is None):
            raise CaeError("sample_latent() takes both mu and logvar, or neither (the prior)")
        if mu is not None:
            (mu, logvar) = (self._rows(mu, (self.latent_size,), "sample_latent()"), self._rows(logvar, (self.latent_size,), "sample_latent()"))
            if mu.shape != logvar.shape:
                raise CaeError("sample_latent(): mu and logvar differ in shape")
            n = mu.shape[0]
        elif n is None or int(n) < 1:
            raise CaeError("sample_latent() from the prior needs n >= 1")
        check_noise_index(int(first_case) + int(n), self.latent_size)
        z = torch.empty((int(n), self.latent_size), dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._sample_into(z, mu, logvar, first_case, draw, seed)
        self.sync()
        return z

    def ensemble_plan(self, ensemble_size):
        """(cases per decode, draws per decode): a decode takes max_batch rows; as many whole cases as fit with all their draws,
        or one case with its draws over several decodes"""
        k = int(ensemble_size)
        cases = max(1, self.max_batch // k)
        return cases, min(k, self.max_batch // cases)

    def ensemble(self, mu, logvar, ensemble_size, seed=0, first_case=0, vmin=0.0, vmax=1.0, want_std=True, target=None):
        """The K = ensemble_size >= 2 draws z_k = sample_latent(mu, logvar, k) of every case decoded and reduced per pixel by
        cae_ensemble_moments (include/cae_hip.h): (mean, std) float64 CUDA tensors (N, *out_shape), denormalised with
        vmin + y * (vmax - vmin); std (ddof = 1) is None unless want_std.  The decoded draws live in one max_batch-row buffer.
        target (the N cases' truth in physical units: an (N, C, H, W) array, CUDA tensor or case_ops.device_operand) also
        verifies the draws of channel 0 against it where they lie (cae_ensemble_verify, K <= 64) and returns (mean, std,
        case_sums, rank_counts): numpy arrays (N, 5) float64 and (K + 2,) int64 for utils/ensemble_scores.py."""
        k = int(ensemble_size)
        if k < 2:
            raise ValueError("an ensemble has at least 2 draws")
        if target is not None:
            return self._ensemble_verified(mu, logvar, k, seed, first_case, vmin, vmax, want_std, target)
        (mu, logvar) = (self._rows(mu, (self.latent_size,), "ensemble()"), self._rows(logvar, (self.latent_size,), "ensemble()"))
        n = mu.shape[0]
        check_noise_index(int(first_case) + n, self.latent_size)
        plane = int(np.prod(self.out_shape))
        (cases, per_call) = self.ensemble_plan(k)
        f64 = dict(dtype=torch.float64, device=self.device)
        mean = torch.empty((n,) + self.out_shape, **f64)
        std = torch.empty((n,) + self.out_shape, **f64) if want_std else None
        z = torch.empty((per_call, cases, self.latent_size), dtype=torch.float32, device=self.device)
        y = torch.empty((per_call, cases, plane), dtype=torch.float32, device=self.device)
        ws = None
        if per_call < k:
            ws_bytes = int(self.lib.cae_ensemble_moments_workspace_bytes(cases, plane))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, n, cases):
            g = min(cases, n - lo)
            for done in range(0, k, per_call):
                kc = min(per_call, k - done)
                # rows [draw][case] of this group: z and y are used as (kc, g, .) contiguous
                self._sample_into(z.view(-1)[:kc * g * self.latent_size], mu[lo:lo + g], logvar[lo:lo + g], first_case + lo, done, seed,
                                  n_draws=kc)
                check(self.lib.vae_decode(self.handle, z.data_ptr(), kc * g, y.data_ptr()))
                check(self.lib.cae_ensemble_moments(y.data_ptr(), plane, g * plane, g, plane, kc, done, k, float(vmin),
                                                    float(vmax) - float(vmin), mean[lo:lo + g].data_ptr(),
                                                    None if std is None else std[lo:lo + g].data_ptr(),
                                                    None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                                                    self.stream.cuda_stream))
        self.sync()
        return mean, std

    def _ensemble_verified(self, mu, logvar, k, seed, first_case, vmin, vmax, want_std, target):
        """ensemble() with a target: the K draws of a group of cases are decoded into one buffer of K rows per case ([draw][case]
        order, in pieces of at most max_batch rows), which one cae_ensemble_moments call (all K draws, no workspace) and one
        cae_ensemble_verify call then reduce"""
        from .case_ops import device_operand
        if k > 64:
            raise ValueError("an ensemble is verified with at most 64 draws")
        (mu, logvar) = (self._rows(mu, (self.latent_size,), "ensemble()"), self._rows(logvar, (self.latent_size,), "ensemble()"))
        n = mu.shape[0]
        check_noise_index(int(first_case) + n, self.latent_size)
        target = device_operand(target, self.device)
        if len(target.shape) != 4 or target.shape[0] != n or tuple(target.shape[2:]) != tuple(self.out_shape[-2:]):
            raise CaeError(f"ensemble(): the target {tuple(target.shape)} does not match {n} cases of {tuple(self.out_shape)}")
        if target.tensor.device != self.device:
            raise CaeError("ensemble(): the target lies on another device")
        field = int(np.prod(self.out_shape))
        plane = int(self.out_shape[-2] * self.out_shape[-1])
        cases = max(1, self.max_batch // k)
        f64 = dict(dtype=torch.float64, device=self.device)
        mean = torch.empty((n,) + self.out_shape, **f64)
        std = torch.empty((n,) + self.out_shape, **f64) if want_std else None
        sums = torch.zeros((n, 5), **f64)
        ranks = torch.zeros(k + 2, dtype=torch.int64, device=self.device)
        z = torch.empty((k, cases, self.latent_size), dtype=torch.float32, device=self.device)
        y = torch.empty((k, cases, field), dtype=torch.float32, device=self.device)
        # the workspace a call needs depends on its number of cases, and fewer cases can need more (they are cut into finer
        # chunks): the largest need of the group sizes this run has, the full groups and the short last one
        ws_bytes = max(int(self.lib.cae_ensemble_verify_workspace_bytes(g, plane, k)) for g in {min(cases, n), n % cases} if g)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, n, cases):
            g = min(cases, n - lo)
            # rows [draw][case] of this group: z and y are used as (k, g, .) contiguous
            self._sample_into(z.view(-1)[:k * g * self.latent_size], mu[lo:lo + g], logvar[lo:lo + g], first_case + lo, 0, seed,
                              n_draws=k)
            for r0 in range(0, k * g, self.max_batch):
                rows = min(self.max_batch, k * g - r0)
                check(self.lib.vae_decode(self.handle, z.data_ptr() + 4 * r0 * self.latent_size, rows,
                                          y.data_ptr() + 4 * r0 * field))
            check(self.lib.cae_ensemble_moments(y.data_ptr(), field, g * field, g, field, k, 0, k, float(vmin),
                                                float(vmax) - float(vmin), mean[lo:lo + g].data_ptr(),
                                                None if std is None else std[lo:lo + g].data_ptr(), None, 0,
                                                self.stream.cuda_stream))
            check(self.lib.cae_ensemble_verify(y.data_ptr(), field, g * field, *target.args(lo), g, plane, k, float(vmin),
                                               float(vmax) - float(vmin), sums[lo:lo + g].data_ptr(),
                                               ranks.data_ptr(), ws.data_ptr(), ws_bytes, self.stream.cuda_stream))
        self.sync()
        for t in (target.tensor, mu, logvar):
            t.record_stream(self.stream)
        return mean, std, sums.cpu().numpy(), ranks.cpu().numpy()
