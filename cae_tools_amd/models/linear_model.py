"""LinearModel — drop-in for the reference's `--method linear` model (src/cae_tools/models/linear_model.py) on libcae_hip.

Same constructor keywords (:32-34), train / apply / score / save / load / summary / get_parameters, the same model folder
(`weights` = torch-saved state_dict with linear.1.weight / linear.1.bias, normalisation.weights, parameters.json,
history.json, summary.txt, input_spec.json, output_spec.json) and printed lines.  Where the reference's HEAD is inconsistent
(its epoch loops unpack three values from DSDataset's four-tuple, :146,166; `test_paths` is undefined at :281) the evident
intent is implemented.  The step (forward, MSELoss, backward, Adam(lr, weight_decay): :146-153,241,247) runs in the HIP
kernels behind include/cae_linear.h."""
from .. import linear_engine as _le
from ..utils.model_database import ModelDatabase
from .base_model import EngineModel
from .linear import Linear


class LinearModel(EngineModel):
    """The reference's LinearModel on the HIP engine (include/cae_linear.h).  Training is bitwise reproducible from run to
    run: the same seeds, data and settings give the same weights and loss history."""

    MODEL_TYPE = "Linear"
    PARAM_KEYS = ("batch_size", "test_interval", "lr", "weight_decay", "normalise_input", "normalise_output")
    OPTIONAL_PARAM_KEYS = EngineModel.RESIDUAL_KEYS
    DATA_PARALLEL = False

    def __init__(self, normalise_input=True, normalise_output=True, batch_size=10, nr_epochs=500, test_interval=10, lr=0.001,
                 weight_decay=1e-5, use_gpu=True, database_path=None, scheduler_type=None, lr_step_size=500, lr_gamma=0.5,
                 residual_variable=None, residual_mode="bicubic"):
        super().__init__()
        self._init_schedule(scheduler_type, lr_step_size, lr_gamma)
        self._init_residual(residual_variable, residual_mode)
        self.normalise_input, self.normalise_output = normalise_input, normalise_output
        self.normalisation_parameters = None
        self.input_shape = self.output_shape = None
        self.weights = None
        (self.batch_size, self.nr_epochs, self.test_interval) = (batch_size, nr_epochs, test_interval)
        (self.lr, self.weight_decay, self.use_gpu) = (lr, weight_decay, use_gpu)
        self.history = {"train_loss": [], "test_loss": [], "nr_epochs": 0}
        self.optim = None
        self.db = ModelDatabase(database_path) if database_path else None
        self._engine = None

    def get_parameters(self):
        return {"model_id": self.get_model_id(), "type": "LinearModel", "input_shape": list(self.input_shape),
                "output_shape": list(self.output_shape), "batch_size": self.batch_size, "test_interval": self.test_interval,
                "lr": self.lr, "weight_decay": self.weight_decay, "normalise_input": self.normalise_input,
                "normalise_output": self.normalise_output, **self._schedule_parameters(), **self._residual_parameters(),
                **self._augment_parameters()}

    def summary(self):
        if not self.input_shape:
            return "Model has not been trained"
        return (f"Model Summary:\n\tInput shape:\n\t\tsize={tuple(self.input_shape)}\n\tOutput shape:\n"
                f"\t\tsize={tuple(self.output_shape)}\n")

    # no spec: one Linear container, saved as `weights`
    def _modules(self):
        self.weights = Linear(self.input_shape, self.output_shape)

    def _weight_files(self):
        return {"weights": self.weights}

    def _spec_record(self):
        return {}

    def _load_modules(self, from_folder):
        self._modules()

    def _build(self):
        if not self.weights:
            self._modules()

    def _make_engine(self, max_batch):
        return _le.LinearEngine(self.input_shape, self.output_shape, max_batch=max_batch)

    def _load_engine(self, eng):
        eng.load_state(self.weights.state_dict())

    def _pull_weights(self):
        if self._engine is not None:
            self.weights.load_state_dict(self._engine.export_state())

    def _score_device(self, x):
        """an engine too small for the rows is re-created"""
        return self._get_engine(max(1, min(int(self.batch_size), int(x.shape[0])))).score(x)
