"""VaeEngine — Python owner of one libcae_hip 'var' engine (include/cae_vae.h) and of its device memory (torch tensors as
containers, as in engine.py / unet_engine.py)."""
import numpy as np
import torch

from ._engine_base import TEST, TRAIN, ShardedSteps, SpecPlan, SteppedEngine, require_gpu  # noqa: F401  (public names)
from ._lib import check


class VaeEngine(ShardedSteps, SteppedEngine, SpecPlan):

    PREFIX = "vae_"
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
