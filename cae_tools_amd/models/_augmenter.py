"""The training side of the dihedral augmentation ("Dihedral augmentation"): EngineModel.train() makes one
TrainAugmenter when augment= is set, the model's _bind_data binds the engine to ITS buffers instead of the data set's packed
arrays, and the epoch loop calls rewrite(epoch) before every training pass."""
import numpy as np
import torch

from ..utils import augment as _aug


class TrainAugmenter:
    """The pristine packed arrays of the training set (input, target and, for the UNET, the loss mask) are never bound to the
    engine: bind() hands out buffers of the same shape, and rewrite(epoch) fills them with every case turned by its code of
    that epoch (case_ops.dihedral_rows; input, target and mask of a case get the same code).  order: the frozen sample
    order of an engine that reads its batches as consecutive rows (ConvAE): row i of a buffer is then case order[i], turned
    by that case's code.  The engine's pointers stay what set_dataset fixed, so its captured graphs replay unchanged."""

    def __init__(self, name, seed):
        self.name = name
        self.group = _aug.check_group(name)
        self.seed = _aug.check_seed(seed)
        self.pairs = []         # (pristine, bound buffer)
        self.n = None
        self.order = None       # host int64 (n,), or None: row i is case i
        self.rows = None        # its int32 device copy
        self.epoch = None       # of the last rewrite

    def bind(self, arrays, order=None):
        """the buffers to bind for `arrays` (a None stays None: an operand the engine does without)"""
        kept = [a for a in arrays if a is not None]
        for a in kept:
            if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dim() == 4 and int(a.shape[0]) == int(kept[0].shape[0])):
                raise ValueError(f"augment: a packed (N, C, H, W) array per operand expected, got {tuple(a.shape)}")
        _aug.check_square(self.name, [a.shape for a in kept])
        self.n = int(kept[0].shape[0])
        if order is not None:
            self.order = np.asarray(order, dtype=np.int64).reshape(-1)
            if self.order.size != self.n:
                raise ValueError(f"augment: a frozen order of {self.n} cases expected, got {self.order.size}")
            self.rows = torch.from_numpy(self.order.astype(np.int32)).to(kept[0].device)
        out = []
        for a in arrays:
            if a is None:
                out.append(None)
                continue
            pristine = a.to(torch.float32).contiguous()
            buffer = torch.empty_like(pristine)
            self.pairs.append((pristine, buffer))
            out.append(buffer)
        return tuple(out)

    def codes(self, epoch):
        """the code of every ROW of the buffers in `epoch`: the case's code, which does not depend on the order"""
        by_case = _aug.codes(self.seed, epoch, self.n, self.group)
        return by_case if self.order is None else by_case[self.order]

    def rewrite(self, epoch):
        """the buffers for `epoch`.  The pass before has ended (its losses were read back); the device is synchronised after the
        rewrite, so the engine's own stream sees it: one synchronisation per epoch."""
        from ..case_ops import dihedral_rows
        if not self.pairs:
            return
        device = self.pairs[0][0].device
        codes = torch.from_numpy(np.ascontiguousarray(self.codes(epoch), dtype=np.int32)).to(device)
        for (pristine, buffer) in self.pairs:
            dihedral_rows(pristine, buffer, codes, rows=self.rows, group=self.group)
        torch.cuda.synchronize(device)
        self.epoch = int(epoch)
