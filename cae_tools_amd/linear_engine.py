"""LinearEngine — Python owner of one libcae_hip LinearModel engine (include/cae_linear.h)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._engine_base import TEST, TRAIN, EngineBase, SteppedEngine, require_gpu  # noqa: F401  (public names)
from ._lib import CaeError, check


class LinearPlan(EngineBase):
    """geometry-only view (no GPU needed): parameter count, workspace size and the launches of a step"""

    PREFIX = "lin_"

    def __init__(self, in_shape, out_shape, max_batch):
        self.lib = _lib.load()
        self.in_shape, self.out_shape = tuple(int(v) for v in in_shape), tuple(int(v) for v in out_shape)
        self.nin, self.nout, self.max_batch = int(np.prod(self.in_shape)), int(np.prod(self.out_shape)), int(max_batch)
        self._create(self.nin, self.nout, self.max_batch)
        self.workspace_bytes = int(self.lib.lin_workspace_bytes(self.handle))

    def kernel_plan(self, batch, train):
        """the GEMM launches of a step at this batch (lin_debug_plan, include/cae_linear.h), no GPU needed:
        {"fwd": {"tile": "32x512", "grid": "2x1", "slices": "5", "per": "16", "part_bytes": "312000"},
         "wgrad": {"tile": "32x512", "grid": "3x1", "slices": "1"} ({} for an eval step), "room": {"gpart_bytes": "312000"}}"""
        buf = C.create_string_buffer(1 << 10)
        check(self.lib.lin_debug_plan(self.handle, int(batch), 1 if train else 0, buf, len(buf)))
        plan = {}
        for line in buf.value.decode().splitlines():
            (name, *fields) = line.split()
            plan[name] = dict(f.split("=", 1) for f in fields if f != "-")
        return plan


class LinearEngine(SteppedEngine, LinearPlan):

    RUNNING_STATS = False

    def __init__(self, in_shape, out_shape, max_batch, device=None):
        require_gpu()
        super().__init__(in_shape, out_shape, max_batch)
        self._bind(device)
        torch.cuda.synchronize(self.device)
        self._start()

    def load_state(self, state):
        w = torch.as_tensor(np.asarray(state["linear.1.weight"]) if not torch.is_tensor(state["linear.1.weight"]) else state["linear.1.weight"])
        b = torch.as_tensor(np.asarray(state["linear.1.bias"]) if not torch.is_tensor(state["linear.1.bias"]) else state["linear.1.bias"])
        if tuple(w.shape) != (self.nout, self.nin) or tuple(b.shape) != (self.nout,):
            raise CaeError(f"weights of shape {tuple(w.shape)} / {tuple(b.shape)} do not fit a {self.nin} -> {self.nout} model")
        self.sync()
        self.params[:self.nout * self.nin].copy_(w.reshape(-1).to(self.device, torch.float32))
        self.params[self.nout * self.nin:].copy_(b.to(self.device, torch.float32))
        torch.cuda.synchronize(self.device)

    def export_state(self):
        self.sync()
        return OrderedDict([("linear.1.weight", self.params[:self.nout * self.nin].view(self.nout, self.nin).cpu().clone()),
                            ("linear.1.bias", self.params[self.nout * self.nin:].cpu().clone())])

    def set_hyper(self, lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8):
        check(self.lib.lin_set_hyper(self.handle, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)))
