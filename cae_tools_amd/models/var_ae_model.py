"""VarAEModel — the 'var' method of the train_cae CLI (its default, cli/train_cae.py:42) on libcae_hip.

The reference ships NO source for this model (cae_tools.models.var_ae_model is imported by model_evaluator.py:35 but the
file is absent); what survives is the CLI surface: --lambda-mse / --lambda-kl / --lambda-ssim (cli/train_cae.py:32-36)
and the pytorch_msssim requirement (README.md:29).  This class is therefore the build's own definition, shaped like
ConvAEModel (same constructor keywords plus the three lambdas, same train / apply / score / save / load surface and model
folder), with the arithmetic published in oracle/vae_oracle.py and computed by the HIP kernels behind include/cae_vae.h:
ConvAE encoder stack -> Linear -> ReLU -> (mu, logvar) heads -> z = mu + eps*exp(logvar/2) -> ConvAE decoder;
loss = lambda_mse*MSE + lambda_kl*KL + lambda_ssim*(1 - MS-SSIM); Adam with L2 weight decay."""
import numpy as np
import torch

from .. import dp as _dp
from .. import vae_engine as _ve
from ..utils.model_database import ModelDatabase
from ._params import ParamBag, add_batchnorm, add_conv
from .base_model import EngineModel, _make_data_array
from .decoder import Decoder
from .ds_dataset import DSDataset  # noqa: F401  (this module's public name since before EngineModel built the data sets)


class VarEncoder(ParamBag):
    """Conv2d -> BatchNorm2d -> ReLU per layer, Linear(F, fc), heads encoder_mu / encoder_logvar; PyTorch default init"""

    def __init__(self, layers, encoded_space_dim, fc_size):
        super().__init__()
        self.layers = list(layers)
        for i, layer in enumerate(self.layers):
            (cin, _, _) = layer.get_input_dimensions()
            (cout, _, _) = layer.get_output_dimensions()
            (kh, kw) = layer.kernel_hw()
            add_conv(self, f"encoder_cnn.{3 * i}", (cout, cin, kh, kw), cout)
            add_batchnorm(self, f"encoder_cnn.{3 * i + 1}", cout)
        (chan, y, x) = self.layers[-1].get_output_dimensions()
        add_conv(self, "encoder_lin.0", (fc_size, chan * y * x), fc_size)
        add_conv(self, "encoder_mu", (encoded_space_dim, fc_size), encoded_space_dim)
        add_conv(self, "encoder_logvar", (encoded_space_dim, fc_size), encoded_space_dim)

        self._engine = None

    def attach(self, engine):
        self._engine = engine

    def forward(self, x):
        """x (B, C, h, w) fp32 CUDA tensor -> (mu, logvar), (B, encoded_space_dim) each; eval mode, on the attached engine"""
        if self._engine is None:
            raise RuntimeError("VarEncoder.forward needs an attached VaeEngine (VarAEModel attaches one when it builds or loads "
                               "a model): there is no CPU path")
        return self._engine.encode(x)

    __call__ = forward


class VarAEModel(EngineModel):
    """The 'var' model (VAE + MS-SSIM, include/cae_vae.h).  Training is bitwise reproducible from run to run: the same seeds
    (noise_seed included), data and settings give the same weights, running statistics and loss history."""

    MODEL_TYPE = "VarAE"
    PARAM_KEYS = ("batch_size", "test_interval", "encoded_dim_size", "fc_size", "lr", "weight_decay", "normalise_input",
                  "normalise_output", "lambda_mse", "lambda_kl", "lambda_ssim")
    LOSS_COLUMN = 3     # of (mse, kl, 1 - ms_ssim, total)

    def __init__(self, normalise_input=True, normalise_output=True, batch_size=10, nr_epochs=500, test_interval=10,
                 encoded_dim_size=32, fc_size=128, lr=0.001, weight_decay=1e-5, use_gpu=True, conv_kernel_size=3, conv_stride=2,
                 conv_input_layer_count=None, conv_output_layer_count=None, database_path=None, lambda_mse=1, lambda_kl=1,
                 lambda_ssim=1, noise_seed=0, scheduler_type=None, lr_step_size=500, lr_gamma=0.5, residual_variable=None,
                 residual_mode="bicubic"):
        super().__init__()
        self._init_schedule(scheduler_type, lr_step_size, lr_gamma)
        self._init_residual(residual_variable, residual_mode)
        self.normalise_input, self.normalise_output = normalise_input, normalise_output
        self.normalisation_parameters = None
        self.input_shape = self.output_shape = None
        self.encoder = self.decoder = None
        (self.batch_size, self.nr_epochs, self.test_interval) = (batch_size, nr_epochs, test_interval)
        (self.encoded_dim_size, self.fc_size, self.lr, self.weight_decay, self.use_gpu) = (encoded_dim_size, fc_size, lr,
                                                                                          weight_decay, use_gpu)
        (self.conv_kernel_size, self.conv_stride) = (conv_kernel_size, conv_stride)
        (self.conv_input_layer_count, self.conv_output_layer_count) = (conv_input_layer_count, conv_output_layer_count)
        (self.lambda_mse, self.lambda_kl, self.lambda_ssim, self.noise_seed) = (lambda_mse, lambda_kl, lambda_ssim, noise_seed)
        self.spec = None
        self.history = {"train_loss": [], "test_loss": [], "nr_epochs": 0}
        self.db = ModelDatabase(database_path) if database_path else None
        self._engine = None
        # under a torch.distributed.run launch (one process per GPU) batch_size stays the GLOBAL batch; sync_bn=True computes
        # BatchNorm statistics over it (N ranks reproduce the single-device step), False keeps per-rank statistics
        self.sync_bn = True

    def get_parameters(self):
        return {"type": "VarAEModel", "input_shape": list(self.input_shape), "output_shape": list(self.output_shape),
                "batch_size": self.batch_size, "test_interval": self.test_interval, "encoded_dim_size": self.encoded_dim_size,
                "fc_size": self.fc_size, "lr": self.lr, "weight_decay": self.weight_decay, "lambda_mse": self.lambda_mse,
                "lambda_kl": self.lambda_kl, "lambda_ssim": self.lambda_ssim, "normalise_input": self.normalise_input,
                "normalise_output": self.normalise_output, "conv_kernel_size": self.conv_kernel_size,
                "conv_stride": self.conv_stride, "conv_input_layer_count": self.conv_input_layer_count,
                "conv_output_layer_count": self.conv_output_layer_count, "model_id": self.get_model_id(),
                **self._schedule_parameters(), **self._residual_parameters(), **self._augment_parameters()}

    def summary(self):
        if not self.spec:
            return "Model has not been trained - no layers assigned yet"
        fc = f"\tFully Connected Layer:\n\t\tsize={self.fc_size}\n"
        return ("Model Summary:\n" + "".join(str(l) for l in self.spec.input_layers) + fc
                + f"\tLatent Vector (mu, logvar):\n\t\tsize={self.encoded_dim_size}\n" + fc
                + "".join(str(l) for l in self.spec.output_layers))

    def _modules(self):
        self.encoder = VarEncoder(self.spec.get_input_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size)
        self.decoder = Decoder(self.spec.get_output_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size)

    def _make_engine(self, max_batch):
        return _ve.VaeEngine(self.spec, self.fc_size, self.encoded_dim_size, max_batch=max_batch)

    def _hyper(self):
        return {"lr": self.lr, "weight_decay": self.weight_decay, "lambda_mse": self.lambda_mse, "lambda_kl": self.lambda_kl,
                "lambda_ssim": self.lambda_ssim, "seed": self.noise_seed}

    # ---- the model as a generative one (the build's own definition, parity unpinned) -------------------------
    def _inference_engine(self, n):
        """the engine encode / decode / apply run on: the one that exists, else one for min(batch_size, n) rows"""
        if self._engine is not None:
            return self._engine
        return self._get_engine(max(1, min(int(self.batch_size), int(n))))

    def _denormalise(self, y):
        """as apply() denormalises (ds_dataset.denormalise_device): min + y * (max - min) of the output variable, float64"""
        from ..device_ops import denormalise_f64
        return denormalise_f64(y, self.normalisation_parameters[2], self.normalisation_parameters[3])

    def encode(self, score_ds, input_variables):
        """(mu, logvar) of every case of score_ds: float32 numpy arrays (N, encoded_dim_size); eval mode"""
        _dp.select_device()
        ds = self._model_dataset(score_ds, input_variables, input_variables[0], normalise_in=self.normalise_input)
        x = ds.device_inputs()
        (mu, logvar) = self._inference_engine(x.shape[0]).encode(x)
        return mu.cpu().numpy(), logvar.cpu().numpy()

    def decode(self, z):
        """z (N, encoded_dim_size) -> the denormalised float64 numpy array (N, C, H, W) the decoder makes of it; eval mode"""
        self._refuse_residual("decode")
        _dp.select_device()
        z = torch.as_tensor(np.asarray(z), dtype=torch.float32).cuda()
        return self._denormalise(self._inference_engine(z.shape[0]).decode(z)).cpu().numpy()

    def generate(self, n, seed=0):
        """n fields decoded from the prior: the latents are normal_noise(seed, 0, (n, encoded_dim_size)) (oracle/vae_oracle.py)"""
        self._refuse_residual("generate")
        _dp.select_device()
        eng = self._inference_engine(n)
        return self._denormalise(eng.decode(eng.sample_latent(None, None, draw=0, seed=seed, n=n))).cpu().numpy()

    def apply(self, score_ds, input_variables, prediction_variable="model_output", channel_dimension="model_output_channel",
              y_dimension="model_output_y", x_dimension="model_output_x", mask_variable_name=None, ensemble_size=None,
              spread_variable=None, ensemble_seed=0, latent_variable=None, interval=None, interval_variables=None,
              scale_variable=None, self_ensemble=None, self_ensemble_spread=None, case_chunk=None):
        """BaseModel.apply (self_ensemble, self_ensemble_spread and case_chunk as it takes them: the geometric self-ensemble of
        the z = mu prediction, refused beside ensemble_size), and with ensemble_size=K the model's own spread: every case is encoded once, K latents
        z_k = mu + eps_k * exp(logvar / 2) are decoded (eps_k: the noise of (ensemble_seed, draw k, global case index)), and
        `prediction_variable` receives the per-pixel mean of the K fields, `spread_variable` (K >= 2) their sample standard
        deviation (same dimensions, float64, denormalised).  latent_variable=NAME stores NAME_mu and NAME_logvar, float32
        (case, "model_latent").  With none of the four keywords this is BaseModel.apply (z = mu), bit for bit.  interval,
        interval_variables and scale_variable as BaseModel.apply takes them; the calibrated scores are those of z = mu, so an
        interval is refused beside ensemble_size."""
        self._check_self_ensemble(self_ensemble, self_ensemble_spread, case_chunk, interval, ensemble_size)
        if self_ensemble is not None:
            if spread_variable is not None or latent_variable is not None:
                raise ValueError("spread_variable and latent_variable belong to the latent ensemble: leave self_ensemble out")
            return super().apply(score_ds, input_variables, prediction_variable, channel_dimension, y_dimension, x_dimension,
                                 mask_variable_name, self_ensemble=self_ensemble, self_ensemble_spread=self_ensemble_spread,
                                 case_chunk=case_chunk)
        if ensemble_size is not None:
            self._refuse_residual("apply(ensemble_size=...)")
        if interval is not None and ensemble_size is not None:
            raise ValueError("interval needs the plain prediction (z = mu) the model was calibrated with: leave ensemble_size out")
        if ensemble_size is not None and (int(ensemble_size) != ensemble_size or int(ensemble_size) < 1):
            raise ValueError(f"ensemble_size must be a positive integer, got {ensemble_size!r}")
        if spread_variable is not None and (ensemble_size is None or int(ensemble_size) < 2):
            raise ValueError("spread_variable needs ensemble_size >= 2: one draw has no spread")
        if ensemble_size is None and latent_variable is None:
            return super().apply(score_ds, input_variables, prediction_variable, channel_dimension, y_dimension, x_dimension,
                                 mask_variable_name, interval=interval, interval_variables=interval_variables,
                                 scale_variable=scale_variable)
        request = self._interval_request(interval, interval_variables, scale_variable, prediction_variable)
        n = int(score_ds[input_variables[0]].shape[0])
        _ve.check_noise_index(n, self.encoded_dim_size)
        dist = _dp.ensure_process_group()      # a rank's GPU is selected before the data set is uploaded
        n_dimension = score_ds[input_variables[0]].dims[0]
        ds = self._model_dataset(score_ds, input_variables, input_variables[0], normalise_in=self.normalise_input,
                                 mask_variable_name=mask_variable_name)
        x = ds.device_inputs()
        # cases sharded over the GPUs of a torch.distributed.run launch as _score_all shards them; the noise counts in the
        # global case index (first_case), so the result does not depend on the number of ranks
        (lo, hi) = (0, n)
        if dist is not None and n >= dist.get_world_size():
            (lo, hi) = _dp.shard_bounds(n, dist.get_world_size(), dist.get_rank())
        else:
            dist = None
        eng = self._inference_engine(hi - lo)
        (mu, logvar) = eng.encode(x[lo:hi])
        (vmin, vmax) = (ds.min_output, ds.max_output)      # what ds.denormalise_device applies
        std = None
        if ensemble_size is None:
            mean = ds.denormalise_device(eng.decode(mu))
        elif int(ensemble_size) == 1:
            mean = ds.denormalise_device(eng.decode(eng.sample_latent(mu, logvar, draw=0, seed=ensemble_seed, first_case=lo)))
        else:
            (mean, std) = eng.ensemble(mu, logvar, int(ensemble_size), seed=ensemble_seed, first_case=lo, vmin=vmin, vmax=vmax,
                                       want_std=spread_variable is not None)
        if dist is not None:
            (mean, mu, logvar) = (self._gather_cases(t, n, dist) for t in (mean, mu, logvar))
            std = None if std is None else self._gather_cases(std, n, dist)
        dims = (n_dimension, channel_dimension, y_dimension, x_dimension)
        score_ds[prediction_variable] = _make_data_array(score_ds, mean.cpu().numpy(), dims)
        self._store_interval(score_ds, mean, request, n_dimension, y_dimension, x_dimension)
        if std is not None:
            score_ds[spread_variable] = _make_data_array(score_ds, std.cpu().numpy(), dims)
        if latent_variable is not None:
            for (suffix, t) in (("_mu", mu), ("_logvar", logvar)):
                score_ds[latent_variable + suffix] = _make_data_array(score_ds, t.cpu().numpy(), (n_dimension, "model_latent"))

    def verify_ensemble(self, score_ds, input_variables, output_variable, ensemble_size, ensemble_seed=0):
        """The K = ensemble_size draws of apply(ensemble_size=K) verified against score_ds[output_variable] (channel 0, in
        physical units) where they are decoded (cae_ensemble_verify, include/cae_hip.h): the dict of
        utils/ensemble_scores.scores_from_sums - n, crps, fair_crps, rmse_mean, spread, spread_skill, rank_counts,
        rank_frequencies, tied, tied_fraction and the per-case "case_crps" (N,) - with the "case_sums" (N, 5) they come from and
        "ensemble_seed".  2 <= K <= 64.  Under a process group every rank computes all cases."""
        from ..data.arrays import as_numpy
        from ..utils import ensemble_scores
        self._refuse_residual("verify_ensemble")
        if int(ensemble_size) != ensemble_size or not 2 <= int(ensemble_size) <= 64:
            raise ValueError(f"ensemble_size must be an integer from 2 to 64 to be verified, got {ensemble_size!r}")
        k = int(ensemble_size)
        n = int(score_ds[input_variables[0]].shape[0])
        _ve.check_noise_index(n, self.encoded_dim_size)
        _dp.select_device()
        ds = self._model_dataset(score_ds, input_variables, input_variables[0], normalise_in=self.normalise_input)
        x = ds.device_inputs()
        eng = self._inference_engine(n)
        (mu, logvar) = eng.encode(x)
        (_, _, sums, ranks) = eng.ensemble(mu, logvar, k, seed=ensemble_seed, vmin=ds.min_output, vmax=ds.max_output,
                                           want_std=False, target=as_numpy(score_ds[output_variable]))
        scores = ensemble_scores.scores_from_sums(sums, ranks, k)
        return {**scores, "case_sums": sums, "ensemble_seed": int(ensemble_seed)}
