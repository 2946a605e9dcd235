"""UNET — drop-in for the reference's `--method unet` model (src/cae_tools/models/unet.py) on libcae_hip.

Same constructor keywords (:201-204), train / score / save / load / summary / get_parameters surface, the same
model folder (encoder.weights / decoder.weights are torch-saved state_dicts with the reference's keys:
encoder_cnn.{4i} Conv2d, {4i+1} BatchNorm2d, encoder_lin.{0,1,4}; decoder_lin.{0,1,4},
attention_layers.{j}.fc{1,2}, decoder_conv.{4j} ConvTranspose2d, {4j+1} BatchNorm2d(2C)) and the same printed
progress lines.  Encoder / Decoder below are parameter containers that replay the reference modules' default
initialisation draw for draw (same seed => bit-identical initial weights; tests/test_unet_cpu.py); every FLOP of
training and scoring runs in the HIP kernels behind include/cae_unet.h.

What differs from the reference, on purpose:
  * the VGG perceptual loss is not built: the reference constructs it (:253, downloading VGG19 weights) but never adds
    it to the loss (:316-322);
  * dropout masks come from the engine's counter-based hash, not from torch's generator (dropout_seed keyword);
  * with mask_variable_name=None and a one-channel input the reference's all-ones mask has the input's shape
    (ds_dataset.py:152-156); it is materialised here so that torch.sum(mask) counts what the reference counts.
"""
import time

import torch

from .. import unet_engine as _ue
from ..utils.model_database import ModelDatabase
from ._params import ParamBag, add_batchnorm, default_layer_init
from .base_model import EngineModel, _mean_loss
from .model_sizer import ModelSpec


def _drawn(shape, n_bias):
    """a layer's default initialisation: weight, then bias (nn.Conv2d / ConvTranspose2d / Linear reset_parameters)"""
    w = torch.empty(shape)
    b = torch.empty(n_bias) if n_bias else None
    if b is None:
        import math
        torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5))
    else:
        default_layer_init(w, b)
    return w, b


class Encoder(ParamBag):
    """unet.py:73-112"""

    def __init__(self, layers, encoded_space_dim, fc_size, dropout_rate=0.1):
        super().__init__()
        self.layers = list(layers)
        self.dropout_rate = dropout_rate
        for i, layer in enumerate(self.layers):
            (cin, _, _) = layer.get_input_dimensions()
            (cout, _, _) = layer.get_output_dimensions()
            (kh, kw) = layer.kernel_hw()
            (w, b) = _drawn((cout, cin, kh, kw), cout)
            self.add_param(f"encoder_cnn.{4 * i}.weight", w)
            self.add_param(f"encoder_cnn.{4 * i}.bias", b)
            add_batchnorm(self, f"encoder_cnn.{4 * i + 1}", cout)
        (chan, y, x) = self.layers[-1].get_output_dimensions()
        (w, b) = _drawn((fc_size, chan * y * x), fc_size)
        self.add_param("encoder_lin.0.weight", w)
        self.add_param("encoder_lin.0.bias", b)
        add_batchnorm(self, "encoder_lin.1", fc_size)
        (w, b) = _drawn((encoded_space_dim, fc_size), encoded_space_dim)
        self.add_param("encoder_lin.4.weight", w)
        self.add_param("encoder_lin.4.bias", b)

    def forward(self, x):
        raise RuntimeError("unet Encoder.forward on its own is not a product path: use UNET.score / apply / train")


class Decoder(ParamBag):
    """unet.py:114-163.  The reference constructs decoder_lin, then per layer ConvTranspose2d and (all but the last)
    ChannelAttention, and registers attention_layers before decoder_conv: draws follow construction order, the
    state_dict follows registration order."""

    def __init__(self, layers, encoded_space_dim, fc_size, dropout_rate=0.1):
        super().__init__()
        self.layers = list(layers)
        self.dropout_rate = dropout_rate
        (self.chan, self.y, self.x) = self.layers[0].get_input_dimensions()
        flat = self.chan * self.y * self.x
        lin0 = _drawn((fc_size, encoded_space_dim), fc_size)
        lin4 = _drawn((flat, fc_size), flat)
        convs, atts = [], []
        last = len(self.layers) - 1
        for j, layer in enumerate(self.layers):
            (cin, _, _) = layer.get_input_dimensions()
            (cout, _, _) = layer.get_output_dimensions()
            (kh, kw) = layer.kernel_hw()
            convs.append(_drawn((cin, cout, kh, kw), cout))
            if j != last:
                fc1 = _drawn((cout // 8, cout, 1, 1), 0)[0]
                fc2 = _drawn((cout, cout // 8, 1, 1), 0)[0]
                atts.append((fc1, fc2))
        self.add_param("decoder_lin.0.weight", lin0[0])
        self.add_param("decoder_lin.0.bias", lin0[1])
        add_batchnorm(self, "decoder_lin.1", fc_size)
        self.add_param("decoder_lin.4.weight", lin4[0])
        self.add_param("decoder_lin.4.bias", lin4[1])
        for j, (fc1, fc2) in enumerate(atts):
            self.add_param(f"attention_layers.{j}.fc1.weight", fc1)
            self.add_param(f"attention_layers.{j}.fc2.weight", fc2)
        for j, (w, b) in enumerate(convs):
            self.add_param(f"decoder_conv.{4 * j}.weight", w)
            self.add_param(f"decoder_conv.{4 * j}.bias", b)
            if j != last:
                add_batchnorm(self, f"decoder_conv.{4 * j + 1}", 2 * w.shape[1])

    def forward(self, x, x_skip):
        raise RuntimeError("unet Decoder.forward on its own is not a product path: use UNET.score / apply / train")


def unet_layer_spec(input_channels, output_channels, size, channels, kernel_size=4, stride=2, padding=1):
    """Hand-written layer definitions for a UNET (what --layer-definitions-path carries, cli/train_cae.py:143-147):
    `output_padding` is the PADDING the UNET modules pass to Conv2d / ConvTranspose2d (unet.py:82,140); decoder layer
    j > 0 takes 2 x channels (skip concat, :160); create_model_spec cannot produce such a spec."""
    from .model_sizer import LayerSpec
    (h, w) = size
    dims = [(input_channels, h, w)]
    enc = []
    for c in channels:
        (_, ph, pw) = dims[-1]
        dims.append((c, (ph + 2 * padding - kernel_size) // stride + 1, (pw + 2 * padding - kernel_size) // stride + 1))
        enc.append(LayerSpec(True, kernel_size, stride, dims[-2], dims[-1], padding))
    dec = []
    n = len(channels)
    for j in range(n):
        (src, dst) = (dims[n - j], dims[n - j - 1])
        cin = src[0] if j == 0 else 2 * src[0]
        cout = dst[0] if j < n - 1 else output_channels
        oh = (src[1] - 1) * stride - 2 * padding + kernel_size
        ow = (src[2] - 1) * stride - 2 * padding + kernel_size
        if (oh, ow) != (dst[1], dst[2]):
            raise ValueError(f"decoder layer {j} lands on {(oh, ow)}, the skip connection has {(dst[1], dst[2])}")
        dec.append(LayerSpec(False, kernel_size, stride, (cin, src[1], src[2]), (cout, oh, ow), padding))
    return ModelSpec(enc, dec)


class UNET(EngineModel):
    """The reference's UNET on the HIP engine (include/cae_unet.h).  Training is bitwise reproducible from run to run: the same
    seeds, data and settings give the same weights, running statistics and loss history."""

    MODEL_TYPE = "UNET"
    PARAM_KEYS = ("batch_size", "test_interval", "encoded_dim_size", "fc_size", "lr", "weight_decay", "normalise_input",
                  "normalise_output")
    LOSS_COLUMN = 0     # of (masked mse, pearson loss)
    MASKED_LOSS = True
    INTERRUPTIBLE = True

    def __init__(self, normalise_input=True, normalise_output=True, batch_size=10, nr_epochs=500, test_interval=10,
                 encoded_dim_size=32, fc_size=128, lr=0.001, weight_decay=1e-5, dropout_rate=0.1, use_gpu=True,
                 conv_kernel_size=3, conv_stride=2, conv_input_layer_count=None, conv_output_layer_count=None,
                 database_path=None, lambda_l1=0.001, lambda_pearson=1, dropout_seed=0, scheduler_type=None, lr_step_size=500,
                 lr_gamma=0.5, residual_variable=None, residual_mode="bicubic"):
        super().__init__()
        self._init_schedule(scheduler_type, lr_step_size, lr_gamma)
        self._init_residual(residual_variable, residual_mode)
        self.normalise_input = normalise_input
        self.normalise_output = normalise_output
        self.normalisation_parameters = None
        self.input_shape = self.output_shape = None
        self.encoder = self.decoder = None
        self.batch_size = batch_size
        self.nr_epochs = nr_epochs
        self.test_interval = test_interval
        self.encoded_dim_size = encoded_dim_size
        self.fc_size = fc_size
        self.lr = lr
        self.weight_decay = weight_decay
        self.dropout_rate = dropout_rate
        self.use_gpu = use_gpu
        self.conv_kernel_size = conv_kernel_size
        self.conv_stride = conv_stride
        self.conv_input_layer_count = conv_input_layer_count
        self.conv_output_layer_count = conv_output_layer_count
        self.spec = None
        self.history = {"train_loss": [], "test_loss": [], "nr_epochs": 0}
        self.db = ModelDatabase(database_path) if database_path else None
        self.lambda_l1 = lambda_l1            # accepted and stored like the reference; unused there too
        self.lambda_pearson = lambda_pearson
        self.dropout_seed = dropout_seed
        self._engine = None
        self._steps_done = 0
        # under a torch.distributed.run launch (one process per GPU) batch_size stays the GLOBAL batch; sync_bn=True computes
        # BatchNorm statistics over it (N ranks reproduce the single-device step), False keeps per-rank statistics
        self.sync_bn = True

    # ---- persistence ---------------------------------------------------------------------------------
    def get_parameters(self):
        return {
            "type": "UNET",
            "input_shape": list(self.input_shape),
            "output_shape": list(self.output_shape),
            "batch_size": self.batch_size,
            "test_interval": self.test_interval,
            "encoded_dim_size": self.encoded_dim_size,
            "fc_size": self.fc_size,
            "lr": self.lr,
            "lambda_pearson": self.lambda_pearson,
            "weight_decay": self.weight_decay,
            "dropout_rate": self.dropout_rate,
            "normalise_input": self.normalise_input,
            "normalise_output": self.normalise_output,
            "conv_kernel_size": self.conv_kernel_size,
            "conv_stride": self.conv_stride,
            "conv_input_layer_count": self.conv_input_layer_count,
            "conv_output_layer_count": self.conv_output_layer_count,
            "model_id": self.get_model_id(),
            **self._schedule_parameters(),
            **self._residual_parameters(),
            **self._augment_parameters(),
        }

    def summary(self):
        if not self.spec:
            return "Model has not been trained - no layers assigned yet"
        fc = f"\tFully Connected Layer:\n\t\tsize={self.fc_size}\n"
        return ("Model Summary:\n" + "".join(str(l) for l in self.spec.input_layers) + fc
                + f"\tLatent Vector:\n\t\tsize={self.encoded_dim_size}\n" + fc
                + "".join(str(l) for l in self.spec.output_layers))

    def _modules(self):
        self.encoder = Encoder(self.spec.get_input_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size,
                               dropout_rate=self.dropout_rate)
        self.decoder = Decoder(self.spec.get_output_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size,
                               dropout_rate=self.dropout_rate)

    def _make_engine(self, max_batch):
        return _ue.UnetEngine(self.spec, self.fc_size, self.encoded_dim_size, max_batch=max_batch)

    # ---- training --------------------------------------------------------------------------------------
    def _load_engine(self, eng):
        eng.load_state(self.encoder.state_dict(), self.decoder.state_dict())    # the containers run nothing on their own

    def _hyper(self):
        return {"lr": self.lr, "weight_decay": self.weight_decay, "dropout_rate": self.dropout_rate,
                "lambda_pearson": self.lambda_pearson, "seed": self.dropout_seed}

    def _bind_data(self, eng, train_ds, test_ds, train_perm, test_perm, augmenter=None):
        eng.set_step(0)
        t0 = time.time()
        for (which, ds) in ((_ue.TRAIN, train_ds), (_ue.TEST, test_ds)):
            arrays = (ds.device_inputs(), ds.device_outputs(), self._loss_mask(ds))
            if augmenter is not None and which == _ue.TRAIN:    # the loss mask of a case is turned with its input and target
                arrays = augmenter.bind(arrays)
            eng.set_dataset(which, *arrays)
        idx = (eng.upload_perm(train_perm), eng.upload_perm(test_perm))
        self._progress(f"finished batching in {time.time() - t0:.2f} seconds")
        return idx

    def _report_epoch(self, epoch, train_losses, test_losses, lr):
        print(f"epoch: {epoch}, train_mse: {_mean_loss(train_losses, 0):.6f}, "
              f"train_pearson_loss: {_mean_loss(train_losses, 1):.4f}, test_mse: {_mean_loss(test_losses, 0):.6f}, "
              f"test_pearson_loss: {_mean_loss(test_losses, 1):.4f}")
        print(f"learn rate: {lr:.6f}")

    def _progress(self, message):
        if self._lead:
            print(message)

    def _loss_mask(self, ds):
        """(N, 1|C, H, W) fp32 mask for the loss, or None for all ones counted over the output's channels"""
        m = ds.device_mask()
        if m is not None:
            return m
        (cin, _, _) = self.input_shape
        (cout, oy, ox) = self.output_shape
        if cin == cout:
            return None
        if cin == 1:
            return torch.ones((len(ds), 1, oy, ox), dtype=torch.float32, device="cuda")
        raise ValueError(f"without a mask variable the reference's mask has the input's shape ({cin} channels), which "
                         f"does not broadcast against {cout} output channels")
