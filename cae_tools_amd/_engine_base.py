"""What the four engine wrappers (engine.py, unet_engine.py, vae_engine.py, linear_engine.py) share.

Each libcae_hip engine family exports the same C entry points under its own prefix (`cae_`, `unet_`, `vae_`, `lin_`):
a wrapper names its PREFIX and looks them up as `getattr(lib, PREFIX + name)`.  torch is a container only: flat CUDA
tensors for the parameter / optimiser / running-statistics arenas and the workspace, and a side stream.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import CaeError, LayerSpecC, TensorInfoC, check

TRAIN, TEST = 0, 1


def _spec_layers(spec):
    """accept a ModelSpec-like object or its JSON dict; return two lists of plain dicts"""
    if hasattr(spec, "save"):
        spec = spec.save()
    return spec["input_layers"], spec["output_layers"]


def _to_c(layers):
    arr = (LayerSpecC * len(layers))()
    for i, l in enumerate(layers):
        k = l["kernel_size"]
        (kh, kw) = (int(k[0]), int(k[1])) if isinstance(k, (list, tuple)) else (int(k), int(k))
        (ic, ih, iw) = l["input_dimensions"]
        (oc, oh, ow) = l["output_dimensions"]
        arr[i] = LayerSpecC(ic, ih, iw, oc, oh, ow, kh, kw, int(l["stride"]), int(l.get("output_padding", 0)))
    return arr


def require_gpu():
    if not torch.cuda.is_available():
        raise CaeError("cae_tools_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")


class EngineBase:
    """one engine handle: creation, device arenas, stream, lifetime, chunked scoring"""

    PREFIX = None

    def _c(self, name):
        return getattr(self.lib, self.PREFIX + name)

    def _create(self, *args):
        handle = C.c_void_p()
        check(self._c("engine_create")(*args, C.byref(handle)))
        self.handle = handle
        self.n_param = int(self._c("param_count")(handle))

    def _bind(self, device, grads=False, buffers=False):
        """allocate params [, grads], exp_avg, exp_avg_sq [, buffers] and a 256-byte aligned workspace on `device`, hand
        them and a fresh side stream to the engine"""
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream()
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.n_param, **f32)
        arenas = [self.params]
        if grads:
            self.grads = torch.zeros(self.n_param, **f32)
            arenas.append(self.grads)
        self.exp_avg = torch.zeros(self.n_param, **f32)
        self.exp_avg_sq = torch.zeros(self.n_param, **f32)
        arenas += [self.exp_avg, self.exp_avg_sq]
        if buffers:
            self.buffers = torch.zeros(max(self.n_buffer, 4), **f32)
            arenas.append(self.buffers)
        self.workspace = torch.zeros(self.workspace_bytes + 256, dtype=torch.uint8, device=self.device)
        ws_ptr = (self.workspace.data_ptr() + 255) // 256 * 256
        check(self._c("bind")(self.handle, *(a.data_ptr() for a in arenas), ws_ptr, self.workspace_bytes))
        check(self._c("set_stream")(self.handle, self.stream.cuda_stream))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._c("engine_destroy")(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._c("sync")(self.handle))

    def upload_perm(self, perm):
        idx = torch.as_tensor(np.asarray(perm), dtype=torch.int32).to(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        return idx

    def _prep(self, a):
        return None if a is None else a.to(device=self.device, dtype=torch.float32).contiguous()

    def _chunked(self, fn, x, out):
        """fn(handle, x rows, n, out rows) over x in chunks of max_batch, on the engine's stream"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        for lo in range(0, x.shape[0], self.max_batch):
            hi = min(x.shape[0], lo + self.max_batch)
            check(fn(self.handle, x[lo:hi].data_ptr(), hi - lo, out[lo:hi].data_ptr()))
        return out

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

    def score(self, x):
        """eval-mode forward of (N, *in_shape) in chunks of max_batch -> (N, *out_shape) fp32 CUDA tensor"""
        x = self._prep(x)
        out = torch.empty((x.shape[0],) + self.out_shape, dtype=torch.float32, device=self.device)
        self._chunked(self._c("score"), x, out)
        self.sync()
        return out


class SpecPlan(EngineBase):
    """geometry of a spec-driven engine (ConvAE, UNET, VAE; no GPU needed): tensor table, arena and workspace sizes"""

    def __init__(self, spec, fc_size, latent_size, max_batch):
        self.lib = _lib.load()
        (enc, dec) = _spec_layers(spec)
        self.enc_layers, self.dec_layers = enc, dec
        self.fc_size, self.latent_size, self.max_batch = int(fc_size), int(latent_size), int(max_batch)
        self._create(_to_c(enc), len(enc), _to_c(dec), len(dec), self.fc_size, self.latent_size, self.max_batch)
        self.n_buffer = int(self._c("buffer_count")(self.handle))
        self.workspace_bytes = int(self._c("workspace_bytes")(self.handle))
        self.tensors = OrderedDict()
        info = TensorInfoC()
        for i in range(self._c("tensor_count")(self.handle)):
            check(self._c("tensor_info")(self.handle, i, C.byref(info)))
            shape = tuple(int(info.shape[d]) for d in range(info.ndim))
            self.tensors[info.name.decode()] = (int(info.arena), int(info.offset), int(info.numel), shape)
        self.in_shape = tuple(enc[0]["input_dimensions"])
        self.out_shape = tuple(dec[-1]["output_dimensions"])

    def _plan_report(self, batch, train):
        """PREFIX + debug_plan parsed, no GPU needed: {first word of a line: {key: value of its key=value fields}}"""
        buf = C.create_string_buffer(1 << 16)
        check(self._c("debug_plan")(self.handle, int(batch), 1 if train else 0, buf, len(buf)))
        plan = {}
        for line in buf.value.decode().splitlines():
            (name, *fields) = line.split()
            plan[name] = dict(f.split("=", 1) for f in fields)
        return plan

    def view(self, name):
        """torch view (device) of a named tensor, e.g. 'dec/decoder_conv.0.weight'"""
        (arena, off, numel, shape) = self.tensors[name]
        return (self.params if arena == 0 else self.buffers)[off:off + numel].view(shape)

    def load_state(self, enc_state, dec_state):
        """copy reference-format state dicts (encoder.weights / decoder.weights) into the arenas"""
        self.sync()
        nbt = None
        for prefix, sd in (("enc/", enc_state), ("dec/", dec_state)):
            for k, v in sd.items():
                if k.endswith("num_batches_tracked"):
                    nbt = int(np.asarray(v)) if nbt is None else nbt
                    continue
                name = prefix + k
                if name not in self.tensors:
                    raise CaeError(f"unexpected tensor '{k}' for this model geometry")
                t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(torch.float32)
                dst = self.view(name)
                if tuple(t.shape) != tuple(dst.shape):
                    raise CaeError(f"shape mismatch for '{k}': {tuple(t.shape)} vs {tuple(dst.shape)}")
                dst.copy_(t.to(self.device))
        missing = [n for n in self.tensors if (n[4:] not in (enc_state if n.startswith("enc/") else dec_state))]
        if missing:
            raise CaeError(f"state dict is missing {missing[:3]}...")
        if nbt is not None:
            self.num_batches_tracked = nbt
        torch.cuda.synchronize(self.device)

    def export_state(self):
        """(encoder_state, decoder_state): CPU tensors under the reference's keys in tensor-table order, with a
        num_batches_tracked after every running_var"""
        self.sync()
        enc, dec = OrderedDict(), OrderedDict()
        for name in self.tensors:
            side = enc if name.startswith("enc/") else dec
            side[name[4:]] = self.view(name).detach().cpu().clone()
            if name.endswith(".running_var"):
                side[name[4:-len("running_var")] + "num_batches_tracked"] = torch.tensor(self.num_batches_tracked,
                                                                                         dtype=torch.int64)
        return enc, dec


class SteppedEngine:
    """the per-step API of the UNET, VAE and Linear engines: one C call per batch, LOSSES_PER_BATCH doubles per loss slot"""

    LOSSES_PER_BATCH = 1
    RUNNING_STATS = True    # BatchNorm running statistics (num_batches_tracked) advance with every training batch

    def _check_train_batch(self, batch):
        pass

    def _start(self):
        """counters and loss slots, once the engine is bound"""
        if self.RUNNING_STATS:
            self.num_batches_tracked = 0
        self.steps = 0
        self._keep = {}
        self.loss_slots = int(self._c("loss_slots")(self.handle))

    def _tracked(self):
        if self.RUNNING_STATS:
            self.num_batches_tracked += 1

    def set_step(self, step):
        self.steps = int(step)
        check(self._c("set_step")(self.handle, self.steps))

    def set_lr(self, lr):
        """the learning rate alone (a scheduler step): the next optimiser launch takes it"""
        check(self._c("set_lr")(self.handle, float(lr)))

    def reset_optimizer(self):
        self.sync()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.set_step(0)
        torch.cuda.synchronize(self.device)

    def set_dataset(self, which, x, t=None):
        """x (N, *in_shape), t (N, *out_shape) or None: fp32 CUDA tensors kept alive here"""
        (x, t) = (self._prep(x), self._prep(t))
        if tuple(x.shape[1:]) != self.in_shape or (t is not None and tuple(t.shape[1:]) != self.out_shape):
            raise CaeError(f"data set shapes do not match the model ({self.in_shape} -> {self.out_shape})")
        self._keep[which] = (x, t)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        check(self._c("set_dataset")(self.handle, which, x.data_ptr(), None if t is None else t.data_ptr(),
                                     int(x.shape[0])))

    def train_step(self, which, perm, start, batch, slot=0):
        self._check_train_batch(batch)
        check(self._c("train_step")(self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(batch),
                                    int(slot)))
        self.steps += 1
        self._tracked()

    def forward_backward(self, which, perm, start, batch, slot=0, global_batch=None, out=None):
        """loss gradient as a flat fp32 CUDA tensor (parameter-arena layout); BatchNorm running stats advance"""
        self._check_train_batch(batch)
        grads = out if out is not None else torch.empty(self.n_param, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        check(self._c("forward_backward")(self.handle, which, None if perm is None else perm.data_ptr(), int(start),
                                          int(batch), int(slot), grads.data_ptr(),
                                          1.0 if global_batch is None else float(batch) / float(global_batch)))
        self._tracked()
        if out is None:
            self.sync()
        return grads

    def apply_gradients(self, grads):
        """optimiser step from a flat fp32 gradient (the data-parallel half-step after the all-reduce)"""
        check(self._c("apply_gradients")(self.handle, grads.data_ptr()))
        self.steps += 1

    def eval_step(self, which, perm, start, batch, slot=0):
        check(self._c("eval_step")(self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(batch),
                                   int(slot)))

    def run_batches(self, which, perm, n, batch_size, train):
        """one epoch over n samples in batches of batch_size (last one partial): the losses of every batch"""
        out = []
        starts = list(range(0, n, batch_size))
        for lo in range(0, len(starts), self.loss_slots):
            chunk = starts[lo:lo + self.loss_slots]
            for (slot, start) in enumerate(chunk):
                (self.train_step if train else self.eval_step)(which, perm, start, min(batch_size, n - start), slot)
            out.extend(self.read_losses(0, len(chunk)))
        return out

    def read_losses(self, first, count):
        """a float per batch, or a LOSSES_PER_BATCH-tuple where the engine reports several"""
        w = self.LOSSES_PER_BATCH
        buf = (C.c_double * (w * count))()
        check(self._c("read_losses")(self.handle, int(first), int(count), buf))
        if w == 1:
            return [float(v) for v in buf]
        return [tuple(buf[w * i:w * (i + 1)]) for i in range(count)]


class ShardedSteps:
    """the global-batch entry points of a SteppedEngine (UNET, VAE: PREFIX + forward_backward_sync / eval_step_sync, the shape of
    include/cae_unet.h): a data-parallel rank's shard of a global batch with the single-device arithmetic at that batch"""

    def forward_backward_sync(self, which, perm, start, size, row0, global_batch, world, allreduce, out=None, slot=0):
        """forward_backward of this rank's rows [row0, row0 + size) of a global batch (samples perm[start:start+size]; size 0
        is allowed) with the single-device arithmetic at global_batch: loss denominators over the global batch, random masks /
        noise of the global rows, and - world >= 1 - BatchNorm statistics over the global batch (world 0: per rank).
        `allreduce(t)` sums each fp64 table over the ranks in place.  The loss slot holds the global batch's losses; the
        gradient is this rank's share of the global loss's (the SUM over the ranks is the gradient)."""
        self._check_train_batch(global_batch if world > 0 else size)
        grads = out if out is not None else torch.empty(self.n_param, dtype=torch.float32, device=self.device)
        self._with_allreduce(lambda cb: self._c("forward_backward_sync")(
            self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(size), int(row0), int(global_batch),
            int(world), int(slot), grads.data_ptr(), cb, None), allreduce)
        self._tracked()
        if out is None:
            self.sync()
        return grads

    def eval_step_sync(self, which, perm, start, size, row0, global_batch, allreduce, slot=0):
        """eval_step of this rank's shard of a global batch: the loss slot holds the global batch's losses"""
        self._with_allreduce(lambda cb: self._c("eval_step_sync")(
            self.handle, which, None if perm is None else perm.data_ptr(), int(start), int(size), int(row0), int(global_batch),
            int(slot), cb, None), allreduce)
