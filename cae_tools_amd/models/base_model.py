"""BaseModel — shared model plumbing with the reference's public surface
(src/cae_tools/models/base_model.py): model id (:33,56-61), io-spec accessors (:35-54),
evaluate (:69-100), apply (:102-152), dump_metrics (:154-157), save/load of input_spec.json /
output_spec.json (:162-180).  Scoring, denormalisation and the metric reductions run on the GPU
through libcae_hip; only per-case sums and the final fp64 predictions cross PCIe.
EngineModel is what the four engine-backed models (ConvAE, UNET, VarAE, Linear) share on top of that."""
import contextlib
import json
import os
import time
import uuid

import numpy as np
import torch

from .. import lr_schedule as _lrs
from .._engine_base import TEST, TRAIN
from ..data.arrays import DataArray
from .ds_dataset import DSDataset
from .model_metric import DeviceModelMetric, ModelMetric  # noqa: F401
from .model_sizer import ModelSpec, create_model_spec


_IMPORTANCE_BYTES = 256 << 20       # of fp32 inputs and scores per piece of cases of importance()
_NOVELTY_BYTES = 1 << 30            # of packed reference rows per cae_case_neighbours call of novelty()
_SELF_ENSEMBLE_BYTES = 256 << 20    # of fp32 turned inputs and scores per piece of cases of apply(self_ensemble=...)


class _Keep:
    """the default of train()'s augment keywords: the model's own value stays"""

    def __repr__(self):
        return "KEEP"


KEEP = _Keep()


def _make_data_array(like_ds, data, dims):
    """DataArray of the same family as the dataset it is assigned into"""
    if type(like_ds).__module__.startswith("xarray"):
        import xarray as xr
        return xr.DataArray(data, dims=dims)
    return DataArray(data, dims=dims)


def _index_batches(n, batch_size):
    """the sample order a reference DataLoader(dataset, batch_size, shuffle=True) produces: drawn
    from torch's global generator exactly as RandomSampler does, so the same seed gives the same
    batches (conv_ae_model.py:291-292, 315-325)"""
    loader = torch.utils.data.DataLoader(torch.arange(n), batch_size=batch_size, shuffle=True)
    return torch.cat([b for b in loader]).to(torch.int32).numpy()


def residual_refusal(path, variable):
    """the one message of the paths that do not serve a residual model yet"""
    return (f"{path}: this model predicts the residual over the interpolated variable '{variable}', and {path} denormalises "
            "its scores without adding the interpolation back; use apply() for a residual model")


def _mean_loss(losses, column=None):
    """a pass's loss: the mean over its batches of the engine's per-batch loss (entry `column` where that is a tuple)"""
    return float(np.mean(losses if column is None else [l[column] for l in losses]))


class BaseModel:

    def __init__(self):
        self.input_spec = None
        self.output_spec = None
        self.model_id = str(uuid.uuid4())

    def set_input_spec(self, input_spec):
        self.input_spec = input_spec

    def get_input_spec(self):
        return self.input_spec

    def set_output_spec(self, output_spec):
        self.output_spec = output_spec

    def get_output_spec(self):
        return self.output_spec

    def get_input_variable_names(self):
        return None if self.input_spec is None else [item["name"] for item in self.input_spec]

    def get_output_variable_name(self):
        return None if self.output_spec is None else self.output_spec["name"]

    def set_model_id(self, model_id):
        self.model_id = model_id

    def get_model_id(self):
        return self.model_id

    def torch_load(self, from_path):
        return torch.load(from_path, map_location=torch.device("cpu"), weights_only=True)

    # ---- residual target (build-only; DESIGN.md §9 'Residual target') ---------------------------
    # residual_variable: the low-resolution variable whose channel 0, interpolated to the output grid (residual_mode), the
    # model's target is taken over: it trains on target - b and apply() adds b back.  None: the target is the output itself.
    # residual_min / residual_max: the training set's range of target - b, beside normalisation_parameters.
    residual_variable = None
    residual_mode = "bicubic"
    residual_min = residual_max = None

    def _init_residual(self, residual_variable=None, residual_mode="bicubic"):
        """the two residual keywords of a model constructor (an unknown mode is an error here, before any GPU work)"""
        from ..utils.baseline import MODES
        if residual_mode not in MODES:
            raise ValueError(f"residual_mode must be one of {', '.join(MODES)}, got {residual_mode!r}")
        self.residual_variable = residual_variable
        self.residual_mode = residual_mode
        self.residual_min = self.residual_max = None

    def _residual_parameters(self):
        """what get_parameters() adds: nothing without a residual target (parameters.json is then what it always was)"""
        if self.residual_variable is None:
            return {}
        return {"residual_variable": self.residual_variable, "residual_mode": self.residual_mode,
                "residual_min": self.residual_min, "residual_max": self.residual_max}

    def _refuse_residual(self, path):
        """the paths that denormalise on their own do not add the interpolation back yet: one refusal, before the GPU is
        touched"""
        if self.residual_variable is not None:
            raise NotImplementedError(residual_refusal(path, self.residual_variable))

    def _model_dataset(self, ds, input_variables, output_variable, fit=False, **keywords):
        """Every DSDataset built for this model.  fit=True (the training set): its scans become the model's normalisation and
        residual range; otherwise the model's are applied to it.  A data set without the residual variable is refused before
        the GPU is touched."""
        residual = None
        if self.residual_variable is not None:
            if self.residual_variable not in ds:
                raise ValueError(f"this model predicts the residual over the interpolated variable '{self.residual_variable}', "
                                 f"which the data set does not hold")
            residual = (self.residual_variable, self.residual_mode)
            if not fit:
                residual += ((self.residual_min, self.residual_max),)
            data = DSDataset(ds, input_variables, output_variable, residual=residual, **keywords)
            data.residual_normalise = bool(self.normalise_output)      # whatever normalise_out the caller asks the truth with
        else:
            data = DSDataset(ds, input_variables, output_variable, **keywords)
        if fit:
            self.normalisation_parameters = data.get_normalisation_parameters()
            if residual is not None:
                (self.residual_min, self.residual_max) = data.get_residual_parameters()
        else:
            data.set_normalisation_parameters(self.normalisation_parameters)
        return data

    # ---- scoring helpers -------------------------------------------------------------------
    def _score_device(self, x):
        """eval-mode forward of an (N,C,H,W) fp32 CUDA tensor; implemented by the sub-class"""
        raise NotImplementedError

    def _score_all(self, x):
        """_score_device over the whole array; under a torch.distributed.run launch the cases are sharded over the
        ranks (no exchange while scoring: SURVEY.md §8e) and the scores all-gathered, so every rank returns all of
        them.  Collective: every rank must call it with the same number of cases."""
        from .. import dp as _dp
        dist = _dp.ensure_process_group()
        n = int(x.shape[0])
        if dist is None or n < dist.get_world_size():
            return self._score_device(x)
        (world, rank) = (dist.get_world_size(), dist.get_rank())
        (lo, hi) = _dp.shard_bounds(n, world, rank)
        return self._gather_cases(self._score_device(x[lo:hi]), n, dist)

    @staticmethod
    def _gather_cases(mine, n, dist):
        """all-gather of per-case rows sharded by dp.shard_bounds(n, world, rank): every rank returns all n rows"""
        from .. import dp as _dp
        (world, rank) = (dist.get_world_size(), dist.get_rank())
        (lo, hi) = _dp.shard_bounds(n, world, rank)
        per = -(-n // world)
        pad = torch.zeros((per,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
        pad[:hi - lo] = mine
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad)
        sizes = [b - a for (a, b) in (_dp.shard_bounds(n, world, r) for r in range(world))]
        return torch.cat([p[:k] for p, k in zip(parts, sizes)])

    def evaluate(self, dataset, device=None):
        """score every case, denormalise, and pool the reference's metrics (:69-100).  Scores, truth and mask
        stay on the GPU; cae_metric_sums reduces each case to eight fp64 sums.  The mask is all ones unless the
        dataset carries a mask variable shaped like the output (the reference builds the default mask with the
        INPUT's shape, which cannot index the output; the intended all-pixels mask is used - SURVEY.md headline 3).
        With a residual target the scores are restored (the interpolation added back), rounded to fp32 and reduced against
        the target as stored with (vmin, vmax) = (0, 1): the metrics are those of the prediction, not of the residual."""
        from .. import dp as _dp
        _dp.select_device()
        if getattr(dataset, "residual", None) is not None:
            scores = self._score_all(dataset.device_inputs())
            restored = dataset.denormalise_device(scores).to(torch.float32)
            mm = DeviceModelMetric()
            mm.accumulate(dataset.device_target(), restored, dataset.device_mask(), 0.0, 1.0)
            return mm.get_metrics()
        dataset.set_normalise_output(False)
        truth = dataset.device_outputs()
        scores = self._score_all(dataset.device_inputs())
        mm = DeviceModelMetric()
        mm.accumulate(truth, scores, dataset.device_mask(), dataset.min_output, dataset.max_output)
        return mm.get_metrics()

    def apply(self, score_ds, input_variables, prediction_variable="model_output",
              channel_dimension="model_output_channel", y_dimension="model_output_y",
              x_dimension="model_output_x", mask_variable_name=None, interval=None, interval_variables=None,
              scale_variable=None, self_ensemble=None, self_ensemble_spread=None, case_chunk=None, **vae_only):
        """Add `prediction_variable` (float64, denormalised, dims (case, channel, y, x)) to score_ds
        in place (:102-152).  self_ensemble="flips" | "dihedral" (build-only; DESIGN.md §9 'Dihedral augmentation'): the
        geometric self-ensemble - every case is scored in the 4 or 8 orientations of the group, the scores are turned back
        and `prediction_variable` receives their per-pixel mean, `self_ensemble_spread` (a variable name) their sample
        standard deviation (same dimensions, float64, denormalised: cae_ensemble_moments).  The cases go through in pieces of
        case_chunk (None: a byte budget); the result does not depend on it.  Refused for a residual model, beside interval
        (the calibration holds for the plain prediction) and beside ensemble_size.  interval=L (build-only; DESIGN.md §9 'prediction intervals'): a coverage level the model
        folder was calibrated for (calibrate()), as its decimal text or a Fraction; channel 0 of the prediction then gets the
        bounds prediction -+ q (times score_ds[scale_variable] where the calibration used a scale) as two more float64
        variables (case, y, x), named interval_variables or <prediction_variable>_lower / _upper.  Without interval nothing
        changes, bit for bit."""
        self._check_self_ensemble(self_ensemble, self_ensemble_spread, case_chunk, interval, vae_only.get("ensemble_size"))
        if vae_only:    # ensemble_size / spread_variable / ensemble_seed / latent_variable: VarAEModel.apply's own keywords
            raise TypeError(f"{type(self).__name__}.apply() got {sorted(vae_only)}: only VarAEModel (the VAE, --method var) has a "
                            "stochastic latent to draw an ensemble from")
        request = self._interval_request(interval, interval_variables, scale_variable, prediction_variable)
        if self_ensemble is not None:
            (mean, std) = self._self_ensemble_device(score_ds, input_variables, self_ensemble, self_ensemble_spread is not None,
                                                     case_chunk, mask_variable_name)
            dims = (score_ds[input_variables[0]].dims[0], channel_dimension, y_dimension, x_dimension)
            score_ds[prediction_variable] = _make_data_array(score_ds, mean.cpu().numpy(), dims)
            if std is not None:
                score_ds[self_ensemble_spread] = _make_data_array(score_ds, std.cpu().numpy(), dims)
            return
        out = self.apply_device(score_ds, input_variables, prediction_variable, channel_dimension, y_dimension, x_dimension,
                                mask_variable_name)
        self._store_interval(score_ds, out, request, score_ds[input_variables[0]].dims[0], y_dimension, x_dimension)

    def _check_self_ensemble(self, self_ensemble, spread, case_chunk, interval, ensemble_size):
        """the refusals of apply(self_ensemble=...), all before the GPU is touched"""
        from ..utils import augment as _aug
        if self_ensemble is None:
            if spread is not None:
                raise ValueError("self_ensemble_spread needs self_ensemble='flips' or 'dihedral'")
            return
        _aug.check_group(self_ensemble, "self_ensemble")
        self._refuse_residual("apply(self_ensemble=...)")
        if interval is not None:
            raise ValueError("interval needs the plain prediction the model was calibrated with: leave self_ensemble out")
        if ensemble_size is not None:
            raise ValueError("self_ensemble and ensemble_size are two ensembles: ask for one of them")
        _aug.check_square(self_ensemble, [s for s in (self.input_shape, self.output_shape) if s is not None], "self_ensemble")
        if case_chunk is not None and (int(case_chunk) != case_chunk or int(case_chunk) < 1):
            raise ValueError(f"case_chunk must be an integer of at least 1, got {case_chunk!r}")

    def _self_ensemble_device(self, score_ds, input_variables, self_ensemble, want_std, case_chunk=None, mask_variable_name=None):
        """(mean, std or None) of the geometric self-ensemble: float64 CUDA tensors (N, C, H, W).  A piece of g cases becomes
        K x g rows [draw][case], draw k the piece turned by code k (case_ops.dihedral_rows gathers and turns in one pass), is
        scored through _score_all, turned back by the inverse codes and reduced per pixel by cae_ensemble_moments."""
        from .. import dp as _dp
        from ..case_ops import dihedral_rows, ensemble_moments
        from ..utils import augment as _aug
        _dp.ensure_process_group()
        ds = self._model_dataset(score_ds, input_variables, input_variables[0], normalise_in=self.normalise_input,
                                 mask_variable_name=mask_variable_name)
        x = ds.device_inputs()
        (n, device) = (int(x.shape[0]), x.device)
        k = _aug.GROUPS[self_ensemble]
        out_shape = tuple(int(v) for v in self.output_shape)
        per_case = 4 * k * (int(np.prod(x.shape[1:])) + 2 * int(np.prod(out_shape)))
        chunk = max(1, min(max(n, 1), _SELF_ENSEMBLE_BYTES // per_case)) if case_chunk is None else int(case_chunk)
        mean = torch.empty((n,) + out_shape, dtype=torch.float64, device=device)
        std = torch.empty_like(mean) if want_std else None
        forward = np.arange(k, dtype=np.int32)
        for c0 in range(0, n, chunk):
            g = min(n, c0 + chunk) - c0
            rows = torch.from_numpy(np.tile(np.arange(c0, c0 + g, dtype=np.int32), k)).to(device)
            turn = torch.from_numpy(np.repeat(forward, g)).to(device)
            back = torch.from_numpy(np.repeat(_aug.inverse_code(forward), g)).to(device)
            xk = torch.empty((k * g,) + tuple(x.shape[1:]), dtype=torch.float32, device=device)
            dihedral_rows(x, xk, turn, rows=rows, group=k)
            y = self._score_all(xk).contiguous()
            yb = torch.empty_like(y)
            dihedral_rows(y, yb, back, group=k)
            (m, s) = ensemble_moments(yb.view((k, g) + out_shape), ds.min_output, ds.max_output, want_std=want_std)
            mean[c0:c0 + g] = m
            if want_std:
                std[c0:c0 + g] = s
        return mean, std

    def apply_device(self, score_ds, input_variables, prediction_variable="model_output",
                     channel_dimension="model_output_channel", y_dimension="model_output_y",
                     x_dimension="model_output_x", mask_variable_name=None):
        """apply(), returning the float64 CUDA tensor whose host copy it stored (the evaluator measures it in place)"""
        n_dimension = score_ds[input_variables[0]].dims[0]
        out = self._predict_device(score_ds, input_variables, mask_variable_name)
        score_ds[prediction_variable] = _make_data_array(score_ds, out.cpu().numpy(),
                                                         (n_dimension, channel_dimension, y_dimension, x_dimension))
        return out

    def _predict_device(self, score_ds, input_variables, mask_variable_name=None):
        """the float64 CUDA tensor apply_device stores, and nothing stored: score_ds is not changed"""
        from .. import dp as _dp
        _dp.ensure_process_group()      # a rank's GPU is selected before the data set is uploaded
        ds = self._model_dataset(score_ds, input_variables, input_variables[0], normalise_in=self.normalise_input,
                                 mask_variable_name=mask_variable_name)
        y = self._score_all(ds.device_inputs())     # cases sharded over the GPUs of a torch.distributed.run launch
        # fp64 on the device: min + y*(max-min), or the restored residual b + (rmin + y*(rmax-rmin)); then one D2H copy
        return ds.denormalise_device(y)

    # ---- prediction intervals ----------------------------------------------------------------
    model_folder = None     # set by load() and by calibrate(model_path=...): where apply(interval=...) finds the calibration

    def _interval_request(self, interval, interval_variables, scale_variable, prediction_variable):
        """None without interval; else utils/conformal.interval_request against the model folder's calibration, before the
        GPU is touched"""
        if interval is None:
            if interval_variables is not None or scale_variable is not None:
                raise ValueError("interval_variables and scale_variable need interval=L, a calibrated coverage level")
            return None
        from ..utils import conformal
        if self.model_folder is None:
            raise ValueError("apply(interval=...) needs the model folder that holds the calibration: load() the model from it, "
                             "or calibrate(model_path=...) first")
        return conformal.interval_request(self.model_folder, interval, scale_variable, interval_variables, prediction_variable)

    def _store_interval(self, score_ds, out, request, n_dimension, y_dimension, x_dimension):
        """the two bounds of channel 0 of the prediction `out` (cae_interval_bounds) into score_ds; nothing without a request"""
        if request is None:
            return
        from ..case_ops import interval_bounds
        from ..data.arrays import as_numpy
        (record, index, names) = request
        if record["group"] == "pixel":
            q = record["quantile"][index]
            if tuple(q.shape) != tuple(out.shape[2:]):
                raise ValueError(f"the calibration holds quantiles for a {q.shape[0]} x {q.shape[1]} plane, the prediction is "
                                 f"{int(out.shape[2])} x {int(out.shape[3])}")
        else:
            q = np.float64(record["pooled_quantiles"][index])
        scale = as_numpy(score_ds[record["scale_variable"]]) if record.get("scale_variable") else None
        bounds = interval_bounds(out, q, record["group"], scale=scale, device=out.device)
        for (name, t) in zip(names, bounds):
            score_ds[name] = _make_data_array(score_ds, t.cpu().numpy(), (n_dimension, y_dimension, x_dimension))

    def calibrate(self, ds, input_variables, output_variable, levels, group="pooled", scale_variable=None, model_path=None,
                  test_ds=None, mask_variable_name=None):
        """Split conformal calibration (build-only; DESIGN.md §9 'prediction intervals'): ds is scored exactly as apply_device
        scores it, the absolute residual |p - a| of channel 0 against ds[output_variable] as stored - divided by
        ds[scale_variable] as stored where one is named - is ranked per pixel (group "pixel") or over all pixels ("pooled"),
        and for every coverage level the exact order statistic of rank ceil((n + 1) level) is kept (case_ops.score_quantiles;
        +inf where the group has too few scores).  With exchangeable cases prediction -+ q covers the target with at least
        that probability, whatever the model.  levels: 1 to 8 ascending levels as utils/conformal.parse_levels takes them.
        test_ds: a held-out data set whose coverage sum count / sum n is recorded (case_ops.score_counts).  model_path: the
        model folder, which receives calibration.json (and calibration.nc for the pixel group) and nothing else.  Returns
        the record of utils/conformal.make_record with "q" and "n" as arrays.  Collective under a torch.distributed.run
        launch, as _score_all is; the lead rank writes."""
        from ..case_ops import device_operand, score_counts, score_quantiles
        from ..data.arrays import as_numpy
        from ..utils import conformal
        levels = conformal.parse_levels(levels)
        conformal.check_group(group)

        def operands(data):
            pred = self._predict_device(data, input_variables, mask_variable_name)
            device = pred.device
            target = device_operand(as_numpy(data[output_variable]), device)
            scale = device_operand(as_numpy(data[scale_variable]), device) if scale_variable is not None else None
            return device_operand(pred, device), target, scale, device

        (pred, target, scale, device) = operands(ds)
        (q, n) = score_quantiles(pred, target, levels, group=group, scale=scale, device=device)
        pooled_q = q if group == "pooled" else score_quantiles(pred, target, levels, group="pooled", scale=scale, device=device)[0]
        coverage = None
        if test_ds is not None:
            (t_pred, t_target, t_scale, _) = operands(test_ds)
            (count, total) = score_counts(t_pred, t_target, q, group, scale=t_scale, device=device)
            coverage = ([int(c.sum()) for c in count], int(total.sum()))
        record = conformal.make_record(group, levels, output_variable, scale_variable, int(pred.shape[0]), q, n, pooled_q, coverage)
        if model_path:
            if int(os.environ.get("RANK", "0")) == 0:
                conformal.write_record(model_path, record, q=q, n=n, shape=tuple(target.shape[2:]))
            self.model_folder = model_path
        return dict(record, q=q, n=n)

    def apply_scene(self, scene_ds, input_variables, prediction_variable="model_output", overlap=None,
                    y_dimension="model_output_y", x_dimension="model_output_x", channel_dimension="model_output_channel",
                    tile_rows=None):
        """Apply the model to a whole scene (build-only; DESIGN.md §9 'scene apply').  The input variables are (T, Cv, Y, X)
        with Y and X at least the model's input box, or (T,) and broadcast; the scene is cut into overlapping boxes
        (scene.scene_plan; overlap None: a quarter of the box), the boxes are scored through _score_all in pieces of whole
        tile rows (tile_rows None: a byte budget), and the scores are blended with integer tent weights into
        `prediction_variable`, float64 (T, Co, Y sy, X sx), denormalised as apply() writes it.  A box with a value that is
        not finite is left out of the blend; a pixel no valid box covers is NaN.  The result does not depend on tile_rows.
        Stores the variable on the scene's first dimension, keeps the tile grid and the per-time-step counts of invalid
        tiles and NaN pixels in self.scene_report, and returns the float64 CUDA tensor."""
        from .. import dp as _dp
        from .. import scene as _scene
        from ..data.arrays import as_numpy
        self._refuse_residual("apply_scene")
        _dp.ensure_process_group()
        (in_shape, out_shape) = (tuple(self.input_shape), tuple(self.output_shape))
        shaped = [as_numpy(scene_ds[name]) for name in input_variables]
        full = [a for a in shaped if a.ndim == 4]
        if not full or any(a.ndim not in (1, 4) for a in shaped):
            raise ValueError("apply_scene: scene variables must be 4-D (time, channel, y, x), or 1-D (time) beside one that is; "
                             f"got shapes {[a.shape for a in shaped]}")
        (T, Y, X) = (int(full[0].shape[0]), int(full[0].shape[2]), int(full[0].shape[3]))
        plan = _scene.scene_plan(Y, X, (in_shape, out_shape), overlap)
        variables = [np.broadcast_to(np.asarray(a, dtype=a.dtype.newbyteorder("="))[:, None, None, None], (a.shape[0], 1, Y, X)).copy()
                     if a.ndim == 1 else a for a in shaped]
        if sum(int(v.shape[1]) for v in variables) != in_shape[0]:
            raise ValueError(f"apply_scene: the variables hold {sum(int(v.shape[1]) for v in variables)} channels, the model's input "
                             f"box {in_shape} has {in_shape[0]}")
        (min_in, max_in, min_out, max_out) = tuple(self.normalisation_parameters)
        norms = [(min_in[name], max_in[name]) for name in input_variables]
        (out, invalid_tiles, nan_pixels) = _scene.scene_apply(variables, norms, plan, self._score_all, out_shape[0], min_out, max_out,
                                                            tile_rows=tile_rows, normalise=self.normalise_input)
        self.scene_report = {"plan": plan, "time_steps": T, "invalid_tiles": invalid_tiles, "nan_pixels": nan_pixels}
        time_dimension = scene_ds[input_variables[0]].dims[0]
        scene_ds[prediction_variable] = _make_data_array(scene_ds, out.cpu().numpy(),
                                                         (time_dimension, channel_dimension, y_dimension, x_dimension))
        return out

    def importance(self, ds, input_variables, output_variable, groups=None, repeats=5, seed=0, maps=False, case_chunk=None):
        """Permutation importance of the input variables (build-only; DESIGN.md §9 'input importance'): every case is given
        another case's values for one group of variables, the batch is scored again and the growth of the error against the
        target is reported.  groups: lists of input-variable names (None: every variable on its own); repeats: 1 to 64
        permutations, each a single cycle over the cases (utils/importance.permutations(n, repeats, seed)), the same for
        every group.  Each input variable goes to the GPU once; for every group, repeat and piece of case_chunk cases
        (None: a byte budget) the group's channels of the packed batch are re-packed from the permuted cases
        (cae_normalise_pack_gather), the piece is scored through _score_all and reduced against the unperturbed scores and
        the target as stored (cae_case_importance), and the channels are put back.  The result does not depend on
        case_chunk.  maps=True also sums {count, S e1^2, S e0^2} per pixel over the cases and repeats of a group.  Returns
        the record of utils/importance.summary (with "maps" (G, 3, H, W) when asked for).  Collective under a
        torch.distributed.run launch, as _score_all is."""
        from .. import dp as _dp
        from ..case_ops import case_importance, device_operand, operand_cases, pack_gather
        from ..data.arrays import as_numpy
        from ..utils import importance as _imp
        self._refuse_residual("importance")
        _dp.ensure_process_group()
        names = list(input_variables)
        groups = _imp.check_groups(groups, names)
        repeats = _imp.check_repeats(repeats)
        data = self._model_dataset(ds, names, output_variable, normalise_in=self.normalise_input, normalise_out=False)
        n = len(data)
        if n < 2:
            raise ValueError(f"importance: at least 2 cases expected, got {n}")
        x = data.device_inputs()
        device = x.device
        target = device_operand(as_numpy(ds[output_variable]), device)
        (vmin, vmax) = (data.min_output, data.max_output)
        offsets = {}
        off = 0
        for (name, raw) in zip(names, data._raw_in):
            offsets[name] = (off, raw)
            off += int(raw.shape[1])
        (h_out, w_out) = (int(target.shape[2]), int(target.shape[3]))
        per_case = 4 * (int(np.prod(x.shape[1:])) + int(np.prod(target.shape[1:])))
        chunk = max(1, min(n, _IMPORTANCE_BYTES // per_case)) if case_chunk is None else int(case_chunk)
        if chunk < 1:
            raise ValueError(f"importance: case_chunk must be at least 1, got {case_chunk!r}")
        pieces = [(c0, min(n, c0 + chunk)) for c0 in range(0, n, chunk)]
        base = [self._score_all(x[c0:c1]) for (c0, c1) in pieces]
        perms = torch.from_numpy(_imp.permutations(n, repeats, seed)).to(device)
        sums = np.zeros((len(groups), repeats, n, 8), dtype=np.float64)
        fields = torch.zeros((len(groups), 3, h_out, w_out), dtype=torch.float64, device=device) if maps else None
        batch = torch.empty((min(chunk, n),) + tuple(x.shape[1:]), dtype=torch.float32, device=device)
        held = None             # the piece whose unperturbed rows `batch` holds
        for (g, group) in enumerate(groups):
            for r in range(repeats):
                for (k, (c0, c1)) in enumerate(pieces):
                    xb = batch[:c1 - c0]
                    if held != k:
                        xb.copy_(x[c0:c1])
                        held = k
                    rows = perms[r, c0:c1].contiguous()
                    for name in group:
                        (c_off, raw) = offsets[name]
                        pack_gather(raw, xb, c_off, rows, data.min_inputs[name], data.max_inputs[name], enable=self.normalise_input)
                    pert = self._score_all(xb)
                    sums[g, r, c0:c1] = case_importance(base[k], pert, operand_cases(target, c0, c1), vmin, vmax,
                                                        maps=fields[g] if maps else None, device=device)
                    for name in group:
                        (c_off, raw) = offsets[name]
                        xb[:, c_off:c_off + int(raw.shape[1])] = x[c0:c1, c_off:c_off + int(raw.shape[1])]
        return _imp.summary(groups, sums, seed=seed, maps=fields.cpu().numpy() if maps else None)

    def _packed_inputs(self, ds, input_variables):
        """the packed, normalised inputs of ds as _predict_device packs them: a float32 CUDA tensor (n, C, h, w)"""
        return self._model_dataset(ds, list(input_variables), input_variables[0], normalise_in=self.normalise_input).device_inputs()

    def novelty(self, ds, reference_ds, input_variables, k=5, same=False, reference_chunk=None):
        """Novelty of the cases of ds against a reference set, usually the training set (build-only; DESIGN.md §9 'novelty'):
        both sets are packed with the model's normalisation exactly as _predict_device packs them, and every case of ds gets
        its k nearest reference cases in that space, exact in fp64 (case_ops.case_neighbours).  The references go through in
        pieces of reference_chunk cases (None: a byte budget), merged; the result does not depend on the cut.  same=True:
        reference_ds is ignored and ds is searched against itself, leave-one-out.  Returns a dict: "novelty" (n,) float64 =
        sqrt(dist2[:, k - 1] / D), the rms difference per feature to the k-th nearest reference (+inf with fewer than k valid
        references, NaN for a case with a value that is not finite), "nearest" likewise for dist2[:, 0], "nearest_case" (n,)
        int32, "index" / "dist2" (n, k), "count" (n,), "features" D, "k", "reference_cases" and "valid_reference_cases".  Uses
        the packing alone, never the forward pass; under a torch.distributed.run launch every rank computes the same."""
        from .. import dp as _dp
        from ..case_ops import case_neighbours
        from ..utils import novelty as _nov
        _dp.ensure_process_group()
        k = _nov.check_k(k)
        x = self._packed_inputs(ds, input_variables)
        ref = x if same else self._packed_inputs(reference_ds, input_variables)
        if tuple(ref.shape[1:]) != tuple(x.shape[1:]):
            raise ValueError(f"novelty: cases of shape {tuple(x.shape[1:])} and reference cases of shape {tuple(ref.shape[1:])} do not match")
        (n, n_ref, dim) = (int(x.shape[0]), int(ref.shape[0]), int(np.prod(x.shape[1:])))
        chunk = max(1, _NOVELTY_BYTES // (4 * max(dim, 1))) if reference_chunk is None else int(reference_chunk)
        if chunk < 1:
            raise ValueError(f"novelty: reference_chunk must be at least 1, got {reference_chunk!r}")
        result = None
        for r0 in range(0, max(n_ref, 1), chunk):
            result = case_neighbours(x, ref[r0:r0 + chunk], k, ref_base=r0, self_offset=0 if same else None, merge_into=result,
                                     device=x.device)
        # a row's validity as the kernel finds it: count -1 marks an invalid query, also against no reference at all
        valid_ref = int((case_neighbours(ref, ref[:0], 1, device=x.device)[2] >= 0).sum()) if n_ref else 0
        return _nov.case_record(*result, dim, n_ref, valid_ref)

    def apply_novelty(self, score_ds, reference_ds, input_variables, novelty_variable, k=5):
        """Add `novelty_variable` (float64, one value per case) to score_ds in place: novelty()'s "novelty" of every scored
        case against reference_ds.  Returns novelty()'s record."""
        found = self.novelty(score_ds, reference_ds, input_variables, k=k)
        score_ds[novelty_variable] = _make_data_array(score_ds, found["novelty"], (score_ds[input_variables[0]].dims[0],))
        return found

    def dump_metrics(self, title, metrics):
        print("\n" + title)
        for key in metrics:
            print(f"\t{key:30s}:{metrics[key]}")

    def score(self, batches, save_arr):
        pass  # implement in sub-class

    def save(self, to_folder):
        for (spec, fname) in ((self.input_spec, "input_spec.json"), (self.output_spec, "output_spec.json")):
            if spec is not None:
                with open(os.path.join(to_folder, fname), "w") as f:
                    f.write(json.dumps(spec))

    def load(self, from_folder):
        for attr, fname in (("input_spec", "input_spec.json"), ("output_spec", "output_spec.json")):
            path = os.path.join(from_folder, fname)
            if os.path.exists(path):
                with open(path) as f:
                    setattr(self, attr, json.loads(f.read()))

    def train(self, input_variables, output_variable, training_ds, testing_ds, model_path="", training_paths="",
              testing_paths=""):
        pass  # implement in sub-class

    def summary(self):
        pass  # implement in sub-class

    def get_parameters(self):
        pass  # implement in sub-class


class _ScheduledRate:
    """The learning-rate schedule of one train() call, driven from its epoch loop: steps the schedule (lr_schedule.py),
    hands the new rate to the engine (set_lr: no graph is captured again for it) and keeps history["lr"].  With no
    scheduler every method is a no-op and `current` stays the model's lr."""

    def __init__(self, schedule, engine, history, par=None):
        (self.schedule, self.engine, self.history, self.par) = (schedule, engine, history, par)

    @property
    def current(self):
        return self.schedule.lr

    def _push(self):
        (self.par if self.par is not None else self.engine).set_lr(self.schedule.lr)

    def after_train_pass(self):
        """once per epoch, after its training pass (where the reference steps its scheduler: unet.py:485-487)"""
        if self.schedule.active and not self.schedule.wants_metric:
            self.schedule.step()
            self._push()

    def after_test_pass(self, test_loss):
        """at an epoch whose test pass ran: the plateau schedule listens to the test loss.  Under data-parallel training
        every rank takes rank 0's value, so that all ranks hold the same rate whatever the last bits of their losses."""
        if self.schedule.wants_metric:
            self.schedule.step_metric(self.par.agree(test_loss) if self.par is not None else test_loss)
            self._push()

    def record(self, rate):
        """`rate`: the rate the recorded epoch trained with"""
        if self.schedule.active:
            self.history.setdefault("lr", []).append(rate)


class EngineModel(BaseModel):
    """What the libcae_hip-backed models share: host weight containers mirrored by one engine, the model folder, and
    train() with its epoch loop.  This base implements the spec-driven encoder / decoder models; a sub-class supplies
    MODEL_TYPE (its model-database type), PARAM_KEYS (parameters.json entries load() restores), _modules() and
    _make_engine(max_batch), and says where its training differs with the attributes below and by overriding _hyper(),
    _bind_data() and _report_epoch()."""

    MODEL_TYPE = None
    PARAM_KEYS = ()
    RESIDUAL_KEYS = ("residual_variable", "residual_mode", "residual_min", "residual_max")     # absent: no residual target
    OPTIONAL_PARAM_KEYS = ("conv_kernel_size", "conv_stride", "conv_input_layer_count", "conv_output_layer_count") + RESIDUAL_KEYS
    SCHEDULE_KEYS = ("scheduler_type", "lr_step_size", "lr_gamma")     # in parameters.json only when a scheduler is set
    AUGMENT_KEYS = ("augment", "augment_seed")      # in parameters.json only when the model was trained with augmentation

    # ---- where train() differs between the model classes --------------------------------------
    DATA_PARALLEL = True        # trains one rank per GPU under a torch.distributed.run launch (LinearModel: no such path)
    LOSS_COLUMN = None          # which entry of a batch's loss tuple is THE loss; None: the engine returns one float
    MASKED_LOSS = False         # the loss reads the data sets' mask variable (UNET)
    ALWAYS_BROADCAST_BUFFERS = False    # rank 0's running statistics go out before a test pass and at the end even with
                                        # SyncBN, which keeps them equal on its own (ConvAEModel does; the others do not)
    INTERRUPTIBLE = False       # Ctrl-C ends the epoch loop and the model is still saved (UNET, as the reference's)

    timing = None       # set by train(): seconds and images of the epoch loop, and the world size (build-only attribute)
    # ---- augmentation (build-only; DESIGN.md §9 'Dihedral augmentation') ------------------------
    # augment: None, "flips" or "dihedral": what the last train() turned the training cases with, which a model folder
    # keeps and the next train() on the loaded model takes as its default.  augment_seed: the seed of the codes.
    augment = None
    augment_seed = 0
    _augmenter = None   # the TrainAugmenter of the last train() with augmentation (its buffers are what the engine reads)
    _lead = True        # this process prints (rank 0 of a data-parallel run)

    # ---- learning-rate schedule ------------------------------------------------------------
    def _init_schedule(self, scheduler_type=None, lr_step_size=500, lr_gamma=0.5):
        """the three scheduler keywords of a model constructor (an unknown name is an error here, before any GPU work)"""
        self.scheduler_type = _lrs.check_scheduler_type(scheduler_type)
        self.lr_step_size = lr_step_size
        self.lr_gamma = lr_gamma

    def _schedule_parameters(self):
        """what get_parameters() adds: nothing without a scheduler (parameters.json is then what it always was)"""
        if _lrs.is_constant(self.scheduler_type):
            return {}
        return {key: getattr(self, key) for key in self.SCHEDULE_KEYS}

    def _scheduled_rate(self, eng, par=None):
        """a fresh schedule starting at self.lr, as the optimiser is fresh on every train()"""
        schedule = _lrs.make_schedule(self.scheduler_type, self.lr, self.lr_step_size, self.lr_gamma)
        return _ScheduledRate(schedule, eng, self.history, par)

    def _augment_parameters(self):
        """what get_parameters() adds: nothing without augmentation (parameters.json is then what it always was)"""
        if self.augment is None:
            return {}
        return {"augment": self.augment, "augment_seed": self.augment_seed}

    def _set_augment(self, augment, augment_seed, shapes):
        """train()'s two keywords onto the model, checked before the GPU is touched: a keyword left at KEEP keeps the model's
        own value (a fresh model: off, seed 0; a loaded one: its folder's).  shapes: those of the input and output planes, or a
        function that returns them, called only with augmentation on: without it the data sets are not looked at here."""
        from ..utils import augment as _aug
        if augment is not KEEP:
            if augment is not None:
                _aug.check_group(augment)
            self.augment = augment
        if augment_seed is not KEEP:
            self.augment_seed = _aug.check_seed(augment_seed)
        if self.augment is not None:
            _aug.check_square(self.augment, shapes() if callable(shapes) else shapes)

    def _modules(self):
        """fresh host weight containers for the current spec / shapes"""
        raise NotImplementedError

    def _make_engine(self, max_batch):
        raise NotImplementedError

    def _weight_files(self):
        """model-folder file name -> host container, in save order"""
        return {"encoder.weights": self.encoder, "decoder.weights": self.decoder}

    def _spec_record(self):
        """the spec as stored in spec.json and the model database"""
        return self.spec.save()

    # ---- engine ----------------------------------------------------------------------------
    def _load_engine(self, eng):
        """host state -> a new engine, which the containers then run their own forward on"""
        eng.load_state(self.encoder.state_dict(), self.decoder.state_dict())
        self.encoder.attach(eng)
        self.decoder.attach(eng)

    def _pull_weights(self):
        """device arenas -> the host containers (state_dict source for save())"""
        if self._engine is not None:
            (enc, dec) = self._engine.export_state()
            self.encoder.load_state_dict(enc)
            self.decoder.load_state_dict(dec)

    def _get_engine(self, max_batch):
        """the engine, re-created (weights carried over) when it cannot take max_batch rows"""
        if self._engine is None or self._engine.max_batch < max_batch:
            if self._engine is not None:
                self._pull_weights()
            eng = self._make_engine(max_batch)
            self._load_engine(eng)
            self._engine = eng
        return self._engine

    def _score_device(self, x):
        # an engine that exists is used as it is (score() walks the array in chunks of its max_batch): a data-parallel
        # rank's engine holds a share of the batch and is not re-created for scoring
        if self._engine is not None:
            return self._engine.score(x)
        return self._get_engine(max(1, min(int(self.batch_size), int(x.shape[0])))).score(x)

    def score(self, batches, save_arr):
        """eval-mode forward of a list of (B,C,H,W) batches into save_arr"""
        ctr = 0
        for batch in batches:
            x = torch.as_tensor(batch, dtype=torch.float32)
            y = self._score_device(x.cuda() if not x.is_cuda else x).cpu().numpy()
            save_arr[ctr:ctr + y.shape[0], :, :, :] = y
            ctr += self.batch_size

    # ---- persistence -----------------------------------------------------------------------
    def save(self, to_folder):
        os.makedirs(to_folder, exist_ok=True)
        self._pull_weights()
        for fname, module in self._weight_files().items():
            torch.save(module.state_dict(), os.path.join(to_folder, fname))
        spec = self._spec_record()
        text_files = {"normalisation.weights": json.dumps(self.normalisation_parameters),
                      "parameters.json": json.dumps(self.get_parameters())}
        if spec:    # LinearModel has none
            text_files["spec.json"] = json.dumps(spec)
        text_files.update({"history.json": json.dumps(self.history), "summary.txt": self.summary()})
        for fname, text in text_files.items():
            with open(os.path.join(to_folder, fname), "w") as f:
                f.write(text)
        super().save(to_folder)

    def _load_modules(self, from_folder):
        with open(os.path.join(from_folder, "spec.json")) as f:
            self.spec = ModelSpec()
            self.spec.load(json.loads(f.read()))
        self._modules()

    def load(self, from_folder):
        with open(os.path.join(from_folder, "normalisation.weights")) as f:
            self.normalisation_parameters = json.loads(f.read())
        with open(os.path.join(from_folder, "parameters.json")) as f:
            p = json.loads(f.read())
        if "model_id" in p:
            self.set_model_id(p["model_id"])
        self.input_shape, self.output_shape = tuple(p["input_shape"]), tuple(p["output_shape"])
        for key in self.PARAM_KEYS:
            setattr(self, key, p[key])
        for key in self.OPTIONAL_PARAM_KEYS:
            setattr(self, key, p.get(key, None))
        if self.residual_mode is None:      # a folder from before the residual target, or without one
            self.residual_mode = "bicubic"
        for key in self.SCHEDULE_KEYS:
            if key in p:
                setattr(self, key, p[key])
        (self.augment, self.augment_seed) = (p.get("augment"), p.get("augment_seed", 0))
        with open(os.path.join(from_folder, "history.json")) as f:
            self.history = json.loads(f.read())
        self._load_modules(from_folder)
        for fname, module in self._weight_files().items():
            module.load_state_dict(self.torch_load(os.path.join(from_folder, fname)))
        self._engine = None
        self.model_folder = from_folder
        super().load(from_folder)

    # ---- training --------------------------------------------------------------------------
    def _progress(self, message):
        """a progress line of train(); only UNET prints them"""

    def _build(self):
        """spec and host containers for a model trained from scratch (kept when training continues)"""
        if not self.spec:
            (input_chan, input_y, input_x) = self.input_shape
            (output_chan, output_y, output_x) = self.output_shape
            self.spec = create_model_spec(input_size=(input_y, input_x), input_channels=input_chan,
                                          output_size=(output_y, output_x), output_channels=output_chan,
                                          kernel_size=self.conv_kernel_size, stride=self.conv_stride,
                                          input_layer_count=self.conv_input_layer_count,
                                          output_layer_count=self.conv_output_layer_count)
        if not self.encoder or not self.decoder:
            self._modules()

    def _train_prologue(self, input_variables, output_variable, training_ds, testing_ds, mask_variable_name=None):
        """both data sets (normalisation from the training set), specs, shapes, the model, and the frozen shuffles drawn
        in the reference's order (training loader first): (train_ds, test_ds, train_perm, test_perm)"""
        self._progress("initiating train method")
        train_ds = self._model_dataset(training_ds, input_variables, output_variable, fit=True, normalise_in=self.normalise_input,
                                       normalise_out=self.normalise_output, mask_variable_name=mask_variable_name)
        self._progress("loaded train_ds to train method")
        self.set_input_spec(train_ds.get_input_spec())
        self.set_output_spec(train_ds.get_output_spec())
        test_ds = self._model_dataset(testing_ds, input_variables, output_variable, normalise_in=self.normalise_input,
                                      normalise_out=self.normalise_output, mask_variable_name=mask_variable_name)
        self.input_shape = tuple(train_ds.get_input_shape())
        self.output_shape = tuple(train_ds.get_output_shape())
        self._progress("finished loading train_ds and test_ds from DSDataset")
        self._build()
        train_perm = _index_batches(len(train_ds), self.batch_size)
        test_perm = _index_batches(len(test_ds), self.batch_size)
        self._progress("finished train_loarder and test_loader")
        return train_ds, test_ds, train_perm, test_perm

    def _hyper(self):
        """the keywords of the engine's set_hyper"""
        return {"lr": self.lr, "weight_decay": self.weight_decay}

    def _bind_data(self, eng, train_ds, test_ds, train_perm, test_perm, augmenter=None):
        """both data sets bound to the engine: the device index of each frozen shuffle, (train, test).  augmenter: the
        training set's packed arrays stay pristine and the engine is bound to the augmenter's buffers instead."""
        train = (train_ds.device_inputs(), train_ds.device_outputs())
        eng.set_dataset(TRAIN, *(train if augmenter is None else augmenter.bind(train)))
        eng.set_dataset(TEST, test_ds.device_inputs(), test_ds.device_outputs())
        return eng.upload_perm(train_perm), eng.upload_perm(test_perm)

    def _report_epoch(self, epoch, train_losses, test_losses, lr):
        """the lead rank's line(s) for an epoch whose test pass ran, from the per-batch losses of both passes"""
        column = self.LOSS_COLUMN
        print("%5d %.6f %.6f" % (epoch, _mean_loss(train_losses, column), _mean_loss(test_losses, column)))

    def train(self, input_variables, output_variable, training_ds, testing_ds, model_path="", training_paths="",
              testing_paths="", mask_variable_name=None, augment=KEEP, augment_seed=KEEP):
        """Train (or continue training): see the reference docstring (conv_ae_model.py:241-252).  Data flow: both data sets
        are scanned / normalised / packed on the GPU once, the shuffle is frozen once (:315-325), and every epoch is one
        run_batches per pass plus one loss read-back.

        augment="flips" | "dihedral" (build-only; DESIGN.md §9 'Dihedral augmentation'): before every training pass each
        training case - input, target and loss mask alike - is turned by one of the 4 or 8 symmetries of the square, the code
        of case j in epoch e being utils/augment.codes(augment_seed, e, n, group)[j] with e counted over all train() calls of
        the model (history["nr_epochs"] + epoch).  The packed training set stays pristine and the engine reads buffers that
        one kernel rewrites between epochs (cae_dihedral_rows), at the cost of one device synchronisation per epoch.  The
        test set is never turned.  "dihedral" needs square input and output planes.  None: off, and nothing changes, bit for
        bit.  Left out, both keywords keep the model's own values: off for a fresh model, the folder's for a loaded one.

        Data parallel (build-only; the reference selects ONE device at :294-297): under a torch.distributed.run launch every
        rank holds the model and both data sets and takes its rows of each frozen GLOBAL batch (dp.shard_bounds); gradients,
        and with sync_bn the BatchNorm and loss tables, are summed over the ranks, so that a step is the single-device step
        at batch_size.  Rank 0 prints and saves."""
        from .. import dp as _dp
        self._set_augment(augment, augment_seed, lambda: [training_ds[input_variables[0]].shape, training_ds[output_variable].shape])
        self._augmenter = None
        if self.augment is not None:
            from ._augmenter import TrainAugmenter
            self._augmenter = TrainAugmenter(self.augment, self.augment_seed)
        augmenter = self._augmenter
        # a rank works on ITS GPU from the first allocation on (the data sets below are uploaded to the current device, the
        # engine is created on it)
        dist = _dp.ensure_process_group() if self.DATA_PARALLEL else None
        (world, rank) = (dist.get_world_size(), dist.get_rank()) if dist is not None else (1, 0)
        self._lead = lead = rank == 0
        (train_ds, test_ds, train_perm, test_perm) = self._train_prologue(
            input_variables, output_variable, training_ds, testing_ds, mask_variable_name if self.MASKED_LOSS else None)
        if dist is not None:    # one frozen shuffle for everybody: rank 0's draw
            box = [train_perm, test_perm]
            dist.broadcast_object_list(box, src=0)
            (train_perm, test_perm) = box
        if lead:
            print(f"Running on device: {torch.device('cuda')}")
        start = time.time()

        eng = self._get_engine(-(-int(self.batch_size) // world))   # a rank's share of a global batch
        eng.set_hyper(**self._hyper())
        eng.reset_optimizer()       # the reference re-creates its optimiser on every train() (:310)
        if augmenter is None:
            (train_idx, test_idx) = self._bind_data(eng, train_ds, test_ds, train_perm, test_perm)
        else:
            (train_idx, test_idx) = self._bind_data(eng, train_ds, test_ds, train_perm, test_perm, augmenter=augmenter)
        par = None
        if dist is not None:
            par = _dp.data_parallel(eng, dist, sync_bn=self.sync_bn)
            par.broadcast_parameters(0)     # rank 0's initial (or loaded) weights, running statistics and moments everywhere
        # per-rank BatchNorm lets the ranks' running statistics part: rank 0's go to every rank before they are scored with
        send_buffers = par is not None and (self.ALWAYS_BROADCAST_BUFFERS or not self.sync_bn)
        trace_range = getattr(eng, "trace_range", contextlib.nullcontext)    # named profiler ranges: the ConvAE engine's

        def one_pass(which, idx, ds, train):
            with trace_range("cae_tools_amd.train_epoch" if train else "cae_tools_amd.test_epoch"):
                if par is None:
                    return eng.run_batches(which, idx, len(ds), self.batch_size, train=train)
                if not train and send_buffers:
                    par.broadcast_buffers(0)
                return par.run_batches(which, idx, len(ds), self.batch_size, train=train)

        train_loss = test_loss = 0.0
        rate = self._scheduled_rate(eng, par)
        eng.sync()
        loop_start = time.perf_counter()
        try:
            for epoch in range(self.nr_epochs):
                epoch_start = time.time()
                epoch_lr = rate.current
                if augmenter is not None:       # the epoch counts over all train() calls: a continued model continues the stream
                    augmenter.rewrite(self.history["nr_epochs"] + epoch)
                train_losses = one_pass(TRAIN, train_idx, train_ds, True)
                rate.after_train_pass()     # where the reference steps its scheduler (unet.py:485-487); one tiny launch
                self._progress(f"time used for training one epoch: {time.time() - epoch_start:.2f}")
                train_loss = _mean_loss(train_losses, self.LOSS_COLUMN)
                if epoch % self.test_interval == 0:
                    test_losses = one_pass(TEST, test_idx, test_ds, False)
                    test_loss = _mean_loss(test_losses, self.LOSS_COLUMN)
                    rate.after_test_pass(test_loss)
                    rate.record(epoch_lr)
                    self.history["train_loss"].append(train_loss)
                    self.history["test_loss"].append(test_loss)
                    if lead:
                        self._report_epoch(epoch, train_losses, test_losses, rate.current)
        except KeyboardInterrupt:
            if not self.INTERRUPTIBLE:
                raise
            print("Training interrupted. Performing cleanup...")
        eng.sync()
        # SURVEY §8(d)'s metric: images through the epoch loop (conv_ae_model.py:328-334, the test pass every test_interval
        # epochs included) per second; bench.py's train_api leg reads it
        self.timing = {"epoch_loop_seconds": time.perf_counter() - loop_start, "train_images": len(train_ds) * self.nr_epochs,
                       "epochs": self.nr_epochs, "world": world}
        if send_buffers:
            par.broadcast_buffers(0)
        return self._train_epilogue(start, train_ds, test_ds, train_loss, test_loss, input_variables, output_variable,
                                    model_path, training_paths, testing_paths, lead=lead)

    def _train_epilogue(self, start, train_ds, test_ds, train_loss, test_loss, input_variables, output_variable, model_path,
                        training_paths, testing_paths, lead=True):
        """after the epoch loop: history, database records, save (or pull the weights to the host) and the metrics of
        both data sets.  Only the lead rank of a data-parallel run prints, saves and records; every rank evaluates."""
        self.history["nr_epochs"] += self.nr_epochs
        if lead:
            print("elapsed:" + str(time.time() - start))
        if self.db and lead:
            self.db.add_training_result(self.get_model_id(), self.MODEL_TYPE, output_variable, input_variables,
                                        self.summary(), model_path, training_paths, train_loss, testing_paths, test_loss,
                                        self.get_parameters(), self._spec_record())
        if model_path and lead:
            self.save(model_path)
        else:
            self._pull_weights()
        metrics = {"test": self.evaluate(test_ds), "train": self.evaluate(train_ds)}
        if lead:
            self.dump_metrics("Test Metrics", metrics["test"])
            self.dump_metrics("Train Metrics", metrics["train"])
        if self.db and lead:
            self.db.add_evaluation_result(self.get_model_id(), training_paths, testing_paths, metrics)
        return metrics
