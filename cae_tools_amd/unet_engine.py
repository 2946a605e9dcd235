"""UnetEngine — Python owner of one libcae_hip UNET engine (include/cae_unet.h) and of its device memory.

As in engine.py, torch is a container: flat CUDA tensors for the parameter / AdamW / running-statistics
arenas and the workspace, and a stream.  Every FLOP runs in the HIP kernels."""
import numpy as np
import torch

from ._engine_base import TEST, TRAIN, ShardedSteps, SpecPlan, SteppedEngine, require_gpu  # noqa: F401  (public names)
from ._lib import CaeError, check


class UnetPlan(SpecPlan):
    """geometry-only view (no GPU needed): tensor table, arena and workspace sizes"""

    PREFIX = "unet_"

    def set_kernel_mode(self, specialised):
        """True (the default): the shape-specialised kernels where a layer is eligible; False: the shape-generic ones"""
        check(self.lib.unet_set_kernel_mode(self.handle, 1 if specialised else 0))

    def kernel_plan(self, batch, train):
        """the kernel families a step at this batch runs (unet_debug_plan, include/cae_unet.h), no GPU needed:
        {"enc0": {"down": "thin", "up": "-", "wgrad": "thin", "wp": "0", "packed": "0"}, ..., "fc0": {"fwd": ..., "bwd": ...},
        ..., "dec0": {...}, "pack": {"entries": "7", "launches": "1"}}.  Beside the family every layer carries what its launch
        switches on below it, from the functions the launch calls: "down.rbn", "down.nsplit", "up.cl", "wgrad.tile", "fwd.rb",
        "fwd.slices", "outer_lds", ... (the list is in include/cae_unet.h)"""
        return self._plan_report(batch, train)


class UnetEngine(ShardedSteps, SteppedEngine, UnetPlan):

    LOSSES_PER_BATCH = 2    # (mse, pearson loss)

    def __init__(self, spec, fc_size, latent_size, max_batch, device=None, specialised=True):
        require_gpu()
        super().__init__(spec, fc_size, latent_size, max_batch)
        self._bind(device, buffers=True)
        self.set_kernel_mode(specialised)
        torch.cuda.synchronize(self.device)
        self._start()

    def set_hyper(self, lr=1e-3, weight_decay=1e-5, dropout_rate=0.1, lambda_pearson=1.0, seed=0, betas=(0.9, 0.999), eps=1e-8):
        check(self.lib.unet_set_hyper(self.handle, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                      float(weight_decay), float(dropout_rate), float(lambda_pearson), int(seed) & 0xFFFFFFFF))

    def set_dataset(self, which, x, t=None, mask=None):
        """x (N,Cin,H,W), t (N,Cout,H,W), mask (N,1|Cout,H,W) or None: fp32 CUDA tensors kept alive here"""
        (x, t, mask) = (self._prep(x), self._prep(t), self._prep(mask))
        if tuple(x.shape[1:]) != self.in_shape or (t is not None and tuple(t.shape[1:]) != self.out_shape):
            raise CaeError(f"data set shapes {tuple(x.shape)} / {None if t is None else tuple(t.shape)} do not match "
                           f"the model ({self.in_shape} -> {self.out_shape})")
        if mask is not None and (mask.shape[0] != x.shape[0] or tuple(mask.shape[2:]) != self.out_shape[1:]):
            raise CaeError(f"mask shape {tuple(mask.shape)} does not match the output {self.out_shape}")
        self._keep[which] = (x, t, mask)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))    # the tensors were produced on torch's stream
        check(self.lib.unet_set_dataset(self.handle, which, x.data_ptr(), None if t is None else t.data_ptr(),
                                        None if mask is None else mask.data_ptr(), 0 if mask is None else int(mask.shape[1]),
                                        int(x.shape[0])))

    def _check_train_batch(self, batch):
        if int(batch) == 1:   # what nn.BatchNorm1d raises in the reference for a one-sample training batch
            raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([1, {self.fc_size}])")

    def debug_read(self, what, shape):
        out = np.empty(shape, dtype=np.float32)
        check(self.lib.unet_debug_read(self.handle, what.encode(), out.ctypes.data, out.size))
        return out
