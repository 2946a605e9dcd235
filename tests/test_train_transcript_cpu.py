"""What train() of the four model classes does, call by call, held to a transcript recorded before the four epoch loops became
one (tests/golden/train_transcript.json).  Each case runs a model's real train() in one process with no GPU and no process
group: the data-set set-up, the engine hand-over and the epilogue are replaced on the instance, the engine is a recording
stand-in that returns deterministic losses of the model's shape (floats, 2-tuples, 4-tuples), dp.ensure_process_group hands
out a fake two-rank `dist`, and dp.DataParallel / dp.GradientHalfSteps are recorders.  A case's record is the ordered list of
calls (receiver, method, arguments by name), the stdout lines, history, timing (times masked), what the epilogue was handed
and what train() returned; it must equal the golden record.

Since the recording LinearModel.train() also calls eng.sync() before and after the loop and sets `timing`: those two
differences were written into the golden file by hand.  Running this module as a script records the file anew."""
import contextlib
import inspect
import io
import json
import os
import re
import sys
from contextlib import redirect_stdout
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "train_transcript.json")
N_TRAIN, N_TEST, BATCH, EPOCHS, TEST_INTERVAL = 7, 3, 3, 3, 2      # a partial last batch; epoch 1 has no test pass
OWN_PERMS = ([4, 0, 6, 2, 5, 1, 3], [2, 0, 1])      # what this rank's prologue draws
LEAD_PERMS = ([3, 1, 5, 0, 6, 2, 4], [1, 2, 0])     # what rank 0 drew: rank 1 must train on these
# patience 0: the second test loss (the stand-in's losses grow) halves the rate
SCHEDULES = {"constant": {}, "StepLR": {"scheduler_type": "StepLR", "lr_step_size": 1, "lr_gamma": 0.5},
             "ReduceLROnPlateau": {"scheduler_type": "ReduceLROnPlateau", "lr_step_size": 0, "lr_gamma": 0.5}}
PLACEMENTS = {"single": None, "rank0_syncbn": (0, True), "rank1_nosyncbn": (1, False)}
MODELS = {"conv": ("conv_ae_model", "ConvAEModel"), "var": ("var_ae_model", "VarAEModel"), "unet": ("unet", "UNET"),
          "linear": ("linear_model", "LinearModel")}
LOSS_WIDTH = {"conv": 0, "var": 4, "unet": 2, "linear": 0}      # 0: a float per batch
CASES = ([f"{model}-{place}-{sched}" for model in MODELS for place in PLACEMENTS for sched in SCHEDULES
          if place == "single" or model != "linear"] + ["unet-single-constant-interrupt"])


def _plain(v):
    """a recorded value as JSON holds it: tensors and arrays as shape and values, stand-ins by their name"""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        a = np.asarray(v)
        return {"shape": list(a.shape), "values": a.reshape(-1).tolist()}
    if isinstance(v, (list, tuple)):
        return [_plain(i) for i in v]
    if isinstance(v, dict):
        return {str(k): _plain(i) for (k, i) in v.items()}
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return v.name      # a stand-in


def _recorded(method):
    """append (receiver, method, arguments by parameter name) to the transcript, then run the stand-in's method"""
    sig = inspect.signature(method)

    def wrapper(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)
        bound.apply_defaults()
        named = {k: v for (k, v) in list(bound.arguments.items())[1:]}
        self.log.append([self.name, method.__name__, _plain(named)])
        return method(self, *args, **kw)
    return wrapper


class _Losses:
    """per-batch losses of the k-th pass of a case: 0.5 + k / 8 + batch / 64 (+ column / 4), exact in binary and growing"""

    def __init__(self, width, interrupt_at_train_pass=None):
        (self.width, self.interrupt_at, self.passes, self.train_passes) = (width, interrupt_at_train_pass, 0, 0)

    def next(self, n, batch, train):
        self.train_passes += bool(train)
        if train and self.train_passes == self.interrupt_at:
            raise KeyboardInterrupt
        k = self.passes
        self.passes += 1
        base = [0.5 + k / 8 + b / 64 for b in range(-(-int(n) // int(batch)))]
        return base if not self.width else [tuple(v + c / 4 for c in range(self.width)) for v in base]


class _Engine:
    """the engine calls of train(); run_batches answers for the single-device path"""

    name = "eng"

    def __init__(self, log, losses, max_batch):
        (self.log, self.losses, self.max_batch) = (log, losses, max_batch)

    @_recorded
    def set_hyper(self, **hyper):
        pass

    @_recorded
    def reset_optimizer(self):
        pass

    @_recorded
    def set_step(self, step):
        pass

    @_recorded
    def set_dataset(self, which, x, t=None, mask=None):
        pass

    @_recorded
    def upload_perm(self, perm):
        return torch.as_tensor(np.asarray(perm), dtype=torch.int64)

    @_recorded
    def sync(self):
        pass

    @_recorded
    def set_lr(self, lr):
        pass

    @_recorded
    def run_batches(self, which, perm, n, batch_size, train=True):
        return self.losses.next(n, batch_size, train)


class _NativeEngine(_Engine):
    """the ConvAE engine: its data-parallel steps are its own (what DataParallel looks for), and it marks its passes"""

    def dp_train_steps(self, *args):
        raise AssertionError("the recording DataParallel runs no step")

    @_recorded
    @contextlib.contextmanager
    def trace_range(self, name):
        yield
        self.log.append([self.name, "trace_range.exit", {"name": name}])


class _HalfSteps:
    """dp.GradientHalfSteps"""

    def __init__(self, engine):
        (self.engine, self.log, self.name) = (engine, engine.log, f"half({engine.name})")
        self.log.append(["dp", "GradientHalfSteps", {"engine": engine.name}])


class _DataParallel:
    """dp.DataParallel"""

    name = "par"

    def __init__(self, engine, dist, group=None, sync_bn=False, overlap="auto"):
        (self.log, self.losses) = (engine.log, getattr(engine, "engine", engine).losses)
        self.log.append(["dp", "DataParallel", _plain({"engine": engine, "dist": dist, "group": group, "sync_bn": sync_bn,
                                                       "overlap": overlap})])

    @_recorded
    def broadcast_parameters(self, src=0):
        pass

    @_recorded
    def broadcast_buffers(self, src=0):
        pass

    @_recorded
    def set_lr(self, lr):
        pass

    @_recorded
    def agree(self, value):
        return value

    @_recorded
    def run_batches(self, which, perm, n, global_batch, train=True):
        return self.losses.next(n, global_batch, train)


class _Dist:
    name = "dist"

    def __init__(self, log, rank):
        (self.log, self.rank) = (log, rank)

    def get_world_size(self, group=None):
        return 2

    def get_rank(self, group=None):
        return self.rank

    @_recorded
    def broadcast_object_list(self, box, src=0):
        if self.rank != src:
            box[:] = [np.asarray(p) for p in LEAD_PERMS]


class _Ds:
    """a DSDataset of n cases whose device arrays are their names"""

    def __init__(self, log, name, n):
        (self.log, self.name, self.n) = (log, name, n)

    def __len__(self):
        return self.n

    @_recorded
    def device_inputs(self):
        return f"{self.name}.inputs"

    @_recorded
    def device_outputs(self):
        return f"{self.name}.outputs"

    @_recorded
    def device_mask(self):
        return f"{self.name}.mask"

    @_recorded
    def device_batches(self, order):
        return (f"{self.name}.batched_inputs", f"{self.name}.batched_outputs")


def _masked(text):
    return re.sub(r"(elapsed:|finished batching in |time used for training one epoch: )[-+.0-9e]+", r"\1#", text)


def run_case(case):
    """the record of one case: calls, stdout, history, timing, the epilogue's arguments and train()'s return value"""
    import importlib
    from cae_tools_amd import dp
    (model, place, sched) = case.split("-")[:3]
    (module, cls) = MODELS[model]
    cls = getattr(importlib.import_module(f"cae_tools_amd.models.{module}"), cls)
    m = cls(batch_size=BATCH, nr_epochs=EPOCHS, test_interval=TEST_INTERVAL, **SCHEDULES[sched])
    log = []
    losses = _Losses(LOSS_WIDTH[model], interrupt_at_train_pass=2 if case.endswith("-interrupt") else None)
    dist = None
    if PLACEMENTS[place] is not None:
        (rank, m.sync_bn) = PLACEMENTS[place]
        dist = _Dist(log, rank)
    (train_ds, test_ds) = (_Ds(log, "train_ds", N_TRAIN), _Ds(log, "test_ds", N_TEST))
    seen = {}

    def ensure_process_group():
        log.append(["dp", "ensure_process_group", {}])
        return dist

    def prologue(input_variables, output_variable, training_ds, testing_ds, mask_variable_name=None):
        log.append(["model", "_train_prologue", _plain({"input_variables": input_variables, "output_variable": output_variable,
                                                        "training_ds": training_ds, "testing_ds": testing_ds,
                                                        "mask_variable_name": mask_variable_name})])
        return (train_ds, test_ds) + tuple(np.asarray(p) for p in OWN_PERMS)

    def get_engine(max_batch):
        log.append(["model", "_get_engine", {"max_batch": max_batch}])
        m._engine = (_NativeEngine if model == "conv" else _Engine)(log, losses, max_batch)
        return m._engine

    def epilogue(start, train_ds, test_ds, train_loss, test_loss, input_variables, output_variable, model_path,
                 training_paths, testing_paths, lead=True):
        seen["epilogue"] = _plain({"train_ds": train_ds, "test_ds": test_ds, "train_loss": train_loss, "test_loss": test_loss,
                                   "input_variables": input_variables, "output_variable": output_variable,
                                   "model_path": model_path, "training_paths": training_paths,
                                   "testing_paths": testing_paths, "lead": lead})
        log.append(["model", "_train_epilogue", {}])
        return {"metrics": case}

    (m._train_prologue, m._get_engine, m._train_epilogue) = (prologue, get_engine, epilogue)
    out = io.StringIO()
    with mock.patch.object(dp, "ensure_process_group", ensure_process_group), \
            mock.patch.object(dp, "DataParallel", _DataParallel), mock.patch.object(dp, "GradientHalfSteps", _HalfSteps), \
            redirect_stdout(out):
        returned = m.train(["x"], "y", "TRAINING", "TESTING", model_path="folder", training_paths="train.nc",
                           testing_paths="test.nc", mask_variable_name="mask")
    timing = getattr(m, "timing", None)
    if timing is not None:
        timing = {k: ("#" if k == "epoch_loop_seconds" else v) for (k, v) in sorted(timing.items())}
    record = {"calls": log, "stdout": _masked(out.getvalue()).splitlines(), "history": m.history, "timing": timing,
              "epilogue": seen["epilogue"], "returned": returned}
    return json.loads(json.dumps(_plain(record)))      # as the golden file holds it: tuples are lists


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_train_makes_the_recorded_calls(golden, case):
    got = run_case(case)
    for key in got:     # the first difference by part, for a readable failure; the assertion is the whole record's equality
        assert got[key] == golden[case][key], key
    assert got == golden[case]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(GOLDEN, "w") as f:
        json.dump({case: run_case(case) for case in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases in {GOLDEN}")
