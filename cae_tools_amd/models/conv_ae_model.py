"""ConvAEModel — drop-in for cae_tools' convolutional autoencoder model on MI355X.

Same constructor, methods, side effects, stdout format and on-disk model folder as
src/cae_tools/models/conv_ae_model.py (ctor :35-79, get_parameters :81-99, save :101-133,
load :135-183, epochs :185-221, score :223-239, train :241-360, summary :362-380); the epoch loop
runs in libcae_hip (include/cae_hip.h) on a device-resident dataset and a frozen shuffle.

Where the reference is internally inconsistent at its HEAD (SURVEY.md headline fact 3) this
implements the intended behaviour: DSDataset's 4-tuples are accepted, train() takes the
mask_variable_name the CLI passes (ignored by the 'conv' method: its loss is plain MSE), and the
evaluation mask covers every output pixel.
"""
from .. import engine as _eng
from .base_model import EngineModel
from .ds_dataset import DSDataset  # noqa: F401  (this module's public name since before EngineModel built the data sets)
from .encoder import Encoder
from .decoder import Decoder
from ..utils.model_database import ModelDatabase


class ConvAEModel(EngineModel):

    MODEL_TYPE = "ConvAE"
    PARAM_KEYS = ("batch_size", "test_interval", "encoded_dim_size", "fc_size", "lr", "weight_decay", "normalise_input",
                  "normalise_output")
    ALWAYS_BROADCAST_BUFFERS = True

    def __init__(self, normalise_input=True, normalise_output=True, batch_size=10,
                 nr_epochs=500, test_interval=10, encoded_dim_size=32, fc_size=128,
                 lr=0.001, weight_decay=1e-5, use_gpu=True, conv_kernel_size=3, conv_stride=2,
                 conv_input_layer_count=None, conv_output_layer_count=None, database_path=None, scheduler_type=None,
                 lr_step_size=500, lr_gamma=0.5, residual_variable=None, residual_mode="bicubic"):
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
        self.use_gpu = use_gpu   # kept for signature parity; this implementation is GPU-only
        self.conv_kernel_size = conv_kernel_size
        self.conv_stride = conv_stride
        self.conv_input_layer_count = conv_input_layer_count
        self.conv_output_layer_count = conv_output_layer_count
        self.spec = None
        self.history = {"train_loss": [], "test_loss": [], "nr_epochs": 0}
        self.optim = None
        self.db = ModelDatabase(database_path) if database_path else None   # conv_ae_model.py:75
        self._engine = None
        # build-only: behaviour under a torch.distributed.run launch (one process per GPU).  batch_size stays the GLOBAL
        # batch; sync_bn=True computes BatchNorm statistics over it (N ranks reproduce the single-device step, the
        # reference's semantics), False keeps per-rank statistics (throughput mode)
        self.sync_bn = True

    # ---- persistence ---------------------------------------------------------------------
    def get_parameters(self):
        return {
            "type": "ConvAEModel",
            "input_shape": list(self.input_shape),
            "output_shape": list(self.output_shape),
            "batch_size": self.batch_size,
            "test_interval": self.test_interval,
            "encoded_dim_size": self.encoded_dim_size,
            "fc_size": self.fc_size,
            "lr": self.lr,
            "weight_decay": self.weight_decay,
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

    def _modules(self):
        self.encoder = Encoder(self.spec.get_input_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size)
        self.decoder = Decoder(self.spec.get_output_layers(), encoded_space_dim=self.encoded_dim_size, fc_size=self.fc_size)

    def load(self, from_folder):
        super().load(from_folder)
        self.encoder.eval()
        self.decoder.eval()

    # ---- engine ----------------------------------------------------------------------------
    def _make_engine(self, max_batch):
        return _eng.HipEngine(self.spec, self.fc_size, self.encoded_dim_size, max_batch=max_batch)

    # ---- training --------------------------------------------------------------------------
    def _bind_data(self, eng, train_ds, test_ds, train_perm, test_perm, augmenter=None):
        # The reference stacks its shuffled batches ONCE and reuses that list every epoch (:315-325).  The same here: both data
        # sets are laid out in batch order once - by the normalisation kernel itself, which writes every sample to its row of
        # the frozen order (DSDataset.device_batches -> cae_normalise_pack_rows) - so a batch is a contiguous run of rows and
        # the kernels need no permutation look-up in front of their first load (one dependent memory round trip less per
        # gathering kernel: the encoder's head, the last layer's targets, the first conv's weight gradient).
        # With augmentation the rows are gathered in that order from the packed arrays instead, turned on the way
        # (TrainAugmenter: row i of its buffers is case train_perm[i]), before every training pass.
        if augmenter is None:
            eng.set_dataset(_eng.TRAIN, *train_ds.device_batches(train_perm))
        else:
            eng.set_dataset(_eng.TRAIN, *augmenter.bind((train_ds.device_inputs(), train_ds.device_outputs()), order=train_perm))
        eng.set_dataset(_eng.TEST, *test_ds.device_batches(test_perm))
        return None, None

    def summary(self):
        if not self.spec:
            return "Model has not been trained - no layers assigned yet"
        fc = f"\tFully Connected Layer:\n\t\tsize={self.fc_size}\n"
        return ("Model Summary:\n" + "".join(str(l) for l in self.spec.input_layers) + fc
                + f"\tLatent Vector:\n\t\tsize={self.encoded_dim_size}\n" + fc
                + "".join(str(l) for l in self.spec.output_layers))
