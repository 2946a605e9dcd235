"""Learning-rate schedules on the host (cae_tools_amd/lr_schedule.py): every `--scheduler-type` against the torch class
the flag help names, the train_cae wiring of the three flags into each of the four models, and the data-parallel rule that
every rank feeds the plateau schedule the same loss (two gloo ranks, a stand-in engine).  No GPU.

Tolerance of the sequences: |got - torch| <= 1e-12 * base_lr.  Absolute in units of the base rate because the cosine
schedule passes through exactly 0, where torch's recursion leaves about 1e-18; fewer than 1e4 fp64 roundings of 2^-53 each
separate a closed form from torch's recursion over these epoch counts."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TRIPLES = [(1e-3, 7, 0.5), (1e-3, 1, 0.3), (0.05, 3, 1.0), (2e-4, 50, 0.9), (1e-3, 2, 0.1)]


def _torch_optimizer(base_lr):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)


def _torch_scheduler(kind, opt, step_size, gamma):
    sched = torch.optim.lr_scheduler
    if kind == "StepLR":
        return sched.StepLR(opt, step_size=step_size, gamma=gamma)
    if kind == "ExponentialLR":
        return sched.ExponentialLR(opt, gamma=gamma)
    if kind == "CosineAnnealingLR":
        return sched.CosineAnnealingLR(opt, T_max=step_size, eta_min=0)
    return sched.ReduceLROnPlateau(opt, mode="min", factor=gamma, patience=step_size)


@pytest.mark.parametrize("base_lr,step_size,gamma", TRIPLES)
@pytest.mark.parametrize("kind", ["StepLR", "ExponentialLR", "CosineAnnealingLR"])
def test_epoch_schedules_follow_torch(kind, base_lr, step_size, gamma):
    from cae_tools_amd.lr_schedule import make_schedule
    opt = _torch_optimizer(base_lr)
    ref = _torch_scheduler(kind, opt, step_size, gamma)
    got = make_schedule(kind, base_lr, step_size, gamma)
    assert got.active and not got.wants_metric
    assert got.lr == base_lr
    for epoch in range(3 * step_size + 5):
        opt.step()
        ref.step()
        got.step()
        got.step_metric(1.0)    # not this schedule's call: ignored
        want = opt.param_groups[0]["lr"]
        assert abs(got.lr - want) <= 1e-12 * base_lr, (kind, epoch, got.lr, want)


def _plateau_losses(patience):
    """improvements, then a plateau longer than the patience, then changes below torch's relative threshold of 1e-4 (they
    do not count as improvements), a real improvement, and another plateau"""
    losses = [1.0, 0.8, 0.5]
    losses += [0.5] * (patience + 2)
    losses += [0.5 * (1.0 - 5e-5), 0.5 * (1.0 - 9e-5)] * (patience + 1)
    losses += [0.3]
    losses += [0.31] * (2 * patience + 3)
    return losses


@pytest.mark.parametrize("base_lr,patience,gamma", [t for t in TRIPLES if t[2] < 1.0] + [(1e-3, 0, 0.5)])
def test_plateau_schedule_follows_torch(base_lr, patience, gamma):
    from cae_tools_amd.lr_schedule import make_schedule
    opt = _torch_optimizer(base_lr)
    ref = _torch_scheduler("ReduceLROnPlateau", opt, patience, gamma)
    got = make_schedule("ReduceLROnPlateau", base_lr, patience, gamma)
    assert got.active and got.wants_metric
    (rates, losses) = ([], _plateau_losses(patience))
    losses = (losses * 3)[:max(len(losses), 3 * patience + 5)]
    for (epoch, loss) in enumerate(losses):
        opt.step()
        ref.step(loss)
        got.step()              # not this schedule's call: ignored
        got.step_metric(loss)
        want = opt.param_groups[0]["lr"]
        assert abs(got.lr - want) <= 1e-12 * base_lr, (epoch, got.lr, want)
        rates.append(got.lr)
    if patience <= 7:
        assert len(set(rates)) >= 3, rates     # the list did exercise reductions


def test_plateau_factor_of_one_is_refused_as_torch_refuses_it():
    """gamma = 1.0 is a legal StepLR / ExponentialLR factor (covered above) and no plateau factor: torch raises, so do we"""
    from cae_tools_amd.lr_schedule import make_schedule
    with pytest.raises(ValueError):
        _torch_scheduler("ReduceLROnPlateau", _torch_optimizer(1e-3), 3, 1.0)
    with pytest.raises(ValueError):
        make_schedule("ReduceLROnPlateau", 1e-3, 3, 1.0)


@pytest.mark.parametrize("name", [None, "None", ""])
def test_no_scheduler_is_a_constant_rate(name):
    from cae_tools_amd.lr_schedule import make_schedule
    s = make_schedule(name, 0.002, 3, 0.1)
    assert not s.active and not s.wants_metric
    for _ in range(10):
        s.step()
        s.step_metric(1.0)
        assert s.lr == 0.002


def test_unknown_scheduler_name_lists_the_four():
    from cae_tools_amd.lr_schedule import make_schedule
    with pytest.raises(ValueError) as err:
        make_schedule("CosineLR", 1e-3, 3, 0.1)
    for name in ("StepLR", "ReduceLROnPlateau", "ExponentialLR", "CosineAnnealingLR"):
        assert name in str(err.value)


def test_lr_schedule_module_does_not_import_torch():
    import subprocess
    code = "import sys; import cae_tools_amd.lr_schedule; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


# ---- train_cae wiring ------------------------------------------------------------------------------------------------

CLASSES = {"conv": ("conv_ae_model", "ConvAEModel"), "unet": ("unet", "UNET"), "var": ("var_ae_model", "VarAEModel"),
           "linear": ("linear_model", "LinearModel")}


def _run_cli(monkeypatch, method, extra):
    """train_cae.main with the data loading and the model's train() patched out: the model it built"""
    import importlib
    from cae_tools_amd.cli import train_cae
    from cae_tools_amd.data import datagen
    (module, cls_name) = CLASSES[method]
    cls = getattr(importlib.import_module("cae_tools_amd.models." + module), cls_name)
    built = []
    monkeypatch.setattr(cls, "train", lambda self, *a, **k: built.append(self))
    monkeypatch.setattr(train_cae, "open_mfdataset", lambda paths, **k: datagen.generate("circle", 3, seed=1))
    train_cae.main(["--train-inputs", "a.nc", "--test-inputs", "b.nc", "--model-folder", "unused", "--input-variables", "lowres",
                    "--output-variable", "hires", "--method", method] + extra)
    assert len(built) == 1 and isinstance(built[0], cls)
    return built[0]


@pytest.mark.parametrize("method", sorted(CLASSES))
def test_train_cae_passes_the_scheduler_flags_to_the_model(monkeypatch, method):
    mt = _run_cli(monkeypatch, method, ["--scheduler-type", "StepLR", "--lr-step-size", "7", "--lr-gamma", "0.3"])
    assert (mt.scheduler_type, mt.lr_step_size, mt.lr_gamma) == ("StepLR", 7, 0.3)
    mt = _run_cli(monkeypatch, method, ["--scheduler-type", "None"])
    assert mt.scheduler_type is None
    mt = _run_cli(monkeypatch, method, [])
    assert (mt.scheduler_type, mt.lr_step_size, mt.lr_gamma) == (None, 500, 0.5)


def test_train_cae_refuses_an_unknown_scheduler_before_the_library_is_loaded(monkeypatch):
    from cae_tools_amd import _lib
    from cae_tools_amd.cli import train_cae

    def no_load():
        raise AssertionError("the library was loaded before the scheduler name was checked")

    def no_data(*a, **k):
        raise AssertionError("data was opened before the scheduler name was checked")

    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(train_cae, "open_mfdataset", no_data)
    with pytest.raises(SystemExit) as err:
        train_cae.main(["--train-inputs", "a.nc", "--test-inputs", "b.nc", "--model-folder", "unused", "--input-variables",
                        "lowres", "--output-variable", "hires", "--method", "conv", "--scheduler-type", "Cosine"])
    assert "StepLR" in str(err.value) and "CosineAnnealingLR" in str(err.value)


def test_models_refuse_an_unknown_scheduler_in_the_constructor():
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    with pytest.raises(ValueError):
        ConvAEModel(scheduler_type="Plateau")


def test_scheduler_settings_reach_parameters_json_only_when_set():
    from cae_tools_amd.models.linear_model import LinearModel
    plain = LinearModel()
    (plain.input_shape, plain.output_shape) = ((1, 2, 2), (1, 2, 2))
    assert not {"scheduler_type", "lr_step_size", "lr_gamma"} & set(plain.get_parameters())
    sched = LinearModel(scheduler_type="ExponentialLR", lr_gamma=0.9)
    (sched.input_shape, sched.output_shape) = ((1, 2, 2), (1, 2, 2))
    p = sched.get_parameters()
    assert (p["scheduler_type"], p["lr_step_size"], p["lr_gamma"]) == ("ExponentialLR", 500, 0.9)


# ---- data parallel: every rank holds the same rate ---------------------------------------------------------------------

class _RateRecorder:
    """what DataParallel needs of an engine here: a tensor that names the device, and set_lr"""

    def __init__(self):
        self.grads = torch.zeros(1)
        self.rates = []

    def set_lr(self, lr):
        self.rates.append(lr)


def _rank_losses(rank):
    """the test losses each rank would compute were its reduction to differ from rank 0's: rank 1's sit on the other side
    of torch's relative threshold, so left alone its plateau schedule would count other improvements"""
    base = [1.0, 0.7, 0.7 * (1 - 1.5e-4), 0.7 * (1 - 2.5e-4), 0.7 * (1 - 3.5e-4), 0.69, 0.69, 0.69, 0.69, 0.69]
    return base if rank == 0 else [v * (1 + 1e-4) if i % 2 else v * (1 - 1e-4) for (i, v) in enumerate(base)]


def _plateau_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    from cae_tools_amd.dp import DataParallel
    from cae_tools_amd.lr_schedule import make_schedule
    from cae_tools_amd.models.base_model import _ScheduledRate
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = _RateRecorder()
    par = DataParallel(eng, dist)
    history = {}
    rate = _ScheduledRate(make_schedule("ReduceLROnPlateau", 1e-3, 1, 0.5), eng, history, par)
    for loss in _rank_losses(rank):
        epoch_lr = rate.current
        rate.after_train_pass()         # a plateau schedule does not step here
        rate.after_test_pass(loss)
        rate.record(epoch_lr)
    torch.save({"pushed": eng.rates, "history": history["lr"]}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_hold_the_same_plateau_rates(tmp_path):
    from cae_tools_amd.lr_schedule import make_schedule
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_plateau_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    (r0, r1) = (torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt"))
    assert r0 == r1, (r0, r1)
    # rank 0's losses decided, and they do reduce the rate
    want = make_schedule("ReduceLROnPlateau", 1e-3, 1, 0.5)
    pushed = []
    for loss in _rank_losses(0):
        want.step_metric(loss)
        pushed.append(want.lr)
    assert r0["pushed"] == pushed and len(set(pushed)) >= 2, (r0["pushed"], pushed)
    # ... where rank 1's own losses would have led elsewhere: the broadcast is what keeps the ranks together
    alone = make_schedule("ReduceLROnPlateau", 1e-3, 1, 0.5)
    own = []
    for loss in _rank_losses(1):
        alone.step_metric(loss)
        own.append(alone.lr)
    assert own != pushed
