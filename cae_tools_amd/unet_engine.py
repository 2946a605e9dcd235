"""UnetEngine — Python owner of one libcae_hip UNET engine (include/cae_unet.h) and of its device memory.

As in engine.py, torch is a container: flat CUDA tensors for the parameter / AdamW / running-statistics
arenas and the workspace, and a stream.  Every FLOP runs in the HIP kernels."""
import ctypes as C

import numpy as np
import torch

from ._engine_base import TEST, TRAIN, SpecPlan, SteppedEngine, require_gpu  # noqa: F401  (public names)
from . import _lib
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
        ..., "dec0": {...}, "pack": {"entries": "7", "launches": "1"}}"""
        buf = C.create_string_buffer(1 << 16)
        check(self.lib.unet_debug_plan(self.handle, int(batch), 1 if train else 0, buf, len(buf)))
        plan = {}
        for line in buf.value.decode().splitlines():
            (name, *fields) = line.split()
            plan[name] = dict(f.split("=", 1) for f in fields)
        return plan


class UnetEngine(SteppedEngine, UnetPlan):

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

    # ---- data-parallel shards (unet_forward_backward_sync / unet_eval_step_sync, include/cae_unet.h) ------------------
    def _with_allreduce(self, call, allreduce):
        """call(cb) with cb the C callback that hands `allreduce` a float64 CUDA view of each table the library passes (inside
        `with torch.cuda.stream(self.stream)`: it must sum the view over the ranks in place, enqueued on that stream); an
        exception raised by `allreduce` is raised here after the C call returns"""
        base = (self.workspace.data_ptr() + 255) // 256 * 256
        pad = base - self.workspace.data_ptr()
        failure = []

        def _cb(user, table_ptr, count):
            try:
                off = pad + (table_ptr - base)
                with torch.cuda.stream(self.stream):
                    allreduce(self.workspace[off:off + 8 * count].view(torch.float64))
                return 0
            except Exception as ex:
                failure.append(ex)
                return 1

        cb = _lib.ALLREDUCE_FN(_cb)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        rc = call(cb)
        if failure:
            raise failure[0]
        check(rc)

    def forward_backward_sync(self, which, perm, start, size, row0, global_batch, world, allreduce, out=None, slot=0):
        """forward_backward of this rank's rows [row0, row0 + size) of a global batch (samples perm[start:start+size]; size 0
        is allowed) with the single-device arithmetic at global_batch: loss denominators over the global batch, dropout masks
        of the global rows, and - world >= 1 - BatchNorm statistics over the global batch (world 0: per rank).  `allreduce(t)`
        sums each fp64 table over the ranks in place.  The loss slot holds the global batch's (mse, pearson loss); the
        gradient is this rank's share of the global loss's (the SUM over the ranks is the gradient)."""
        self._check_train_batch(global_batch if world > 0 else size)
        grads = out if out is not None else torch.empty(self.n_param, dtype=torch.float32, device=self.device)
        self._with_allreduce(lambda cb: self.lib.unet_forward_backward_sync(
            self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(size), int(row0), int(global_batch),
            int(world), int(slot), grads.data_ptr(), cb, None), allreduce)
        self._tracked()
        if out is None:
            self.sync()
        return grads

    def eval_step_sync(self, which, perm, start, size, row0, global_batch, allreduce, slot=0):
        """eval_step of this rank's shard of a global batch: the loss slot holds the global batch's losses"""
        self._with_allreduce(lambda cb: self.lib.unet_eval_step_sync(
            self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(size), int(row0), int(global_batch),
            int(slot), cb, None), allreduce)

    def debug_read(self, what, shape):
        out = np.empty(shape, dtype=np.float32)
        check(self.lib.unet_debug_read(self.handle, what.encode(), out.ctypes.data, out.size))
        return out
