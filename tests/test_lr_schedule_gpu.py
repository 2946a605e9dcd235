"""Learning-rate schedules on the device.

The ConvAE engine keeps the rate in its step state on the GPU (StepState::lr), where k_adam reads it beside the step number:
set_lr() is a one-thread launch in stream order and no captured graph is captured again for it.  The UNET, VAE and Linear
engines launch eagerly and pass the rate by value.  Checked here:

* graphs survive a rate that changes every "epoch" (graph_captures() stands still), a weight-decay change still drops them;
* the optimiser kernel uses the new rate: graph-replayed steps under torch.optim.lr_scheduler.StepLR(oracle.optim, 2, 0.5)
  against the oracle, by the criterion of test_adam_step_no_further_from_fp64_than_the_reference (tests/test_hip_parity.py:
  per tensor the update is no further from an fp64 oracle's than 3x the fp32 reference's own, plus 1e-3 of the rate in
  force), every step from the oracle's state as there - free-running trajectories separate chaotically;
* set_lr(a); set_lr(b) gives the BITS of set_hyper(lr=b), on all four engines;
* the model loops: history["lr"], the UNET's `learn rate:` lines, and scheduler_type=None == ExponentialLR(gamma=1) in bits.
"""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from helpers import GoldenCase, bn_bias_keys, oracle_model
from unet_helpers import UnetCase

pytestmark = pytest.mark.gpu


def _conv_engine(case, graph=True):
    from cae_tools_amd.engine import HipEngine
    eng = HipEngine(case.spec, case.meta["fc"], case.meta["latent"], max_batch=max(8, case.meta["batch"]), graph=graph)
    eng.load_state(case.group("init/enc/"), case.group("init/dec/"))
    eng.set_hyper(lr=case.meta["lr"], weight_decay=case.meta["weight_decay"])
    x = torch.from_numpy(np.concatenate([case.x, case.x2])).cuda()
    t = torch.from_numpy(np.concatenate([case.t, case.t2])).cuda()
    eng.set_dataset(0, x, t)
    return eng


def _state(eng):
    out = [("params", eng.params.cpu()), ("exp_avg", eng.exp_avg.cpu()), ("exp_avg_sq", eng.exp_avg_sq.cpu())]
    if getattr(eng, "buffers", None) is not None:
        out.append(("running statistics", eng.buffers.cpu()))
    return out


def _same_bits(a, b, what):
    for (name, u), (_, v) in zip(a, b):
        assert torch.equal(u, v), f"{what}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"


# ---- the ConvAE engine: graphs and the device-resident rate ----------------------------------------------------------------

def test_graphs_survive_a_changing_rate():
    """a 3-step graph (cae_train_steps) and the 1-step graph of the short last batch, replayed over five "epochs" with a new
    rate before each: nothing is captured after the first epoch; a weight-decay change captures again, as it always did"""
    case = GoldenCase("cfg2_b4")
    eng = _conv_engine(case)
    lr = case.meta["lr"]
    n = 7       # 3 full batches of 2 (one multi-step graph) + a batch of 1
    assert eng.graph_captures() == 0
    eng.run_batches(0, None, n, 2, train=True)
    first = eng.graph_captures()
    assert first == 2 and eng.graph_count() == 2, (first, eng.graph_count())
    before = eng.params.clone()
    for epoch in range(1, 6):
        eng.set_lr(lr * 0.5 ** epoch)
        eng.run_batches(0, None, n, 2, train=True)
        assert eng.graph_captures() == first, (epoch, eng.graph_captures())
    assert not torch.equal(before, eng.params)
    # the rate through set_hyper: still no capture
    eng.set_hyper(lr=lr * 0.3, weight_decay=case.meta["weight_decay"])
    eng.run_batches(0, None, n, 2, train=True)
    assert eng.graph_captures() == first and eng.graph_count() == 2
    # betas / eps / weight decay are baked into the captured launches: those drop the graphs
    eng.set_hyper(lr=lr * 0.3, weight_decay=2 * case.meta["weight_decay"])
    assert eng.graph_count() == 0
    eng.run_batches(0, None, n, 2, train=True)
    assert eng.graph_captures() == 2 * first and eng.graph_count() == 2


def test_a_replayed_graph_steps_with_the_rate_set_after_its_capture():
    """the same graph, replayed from the same state with two rates: with zero moments Adam's first step moves every weight by
    about the rate, so the two updates differ by the ratio of the rates"""
    case = GoldenCase("cfg2_b4")
    eng = _conv_engine(case)
    b = case.meta["batch"]
    (enc, dec) = (case.group("init/enc/"), case.group("init/dec/"))
    moves = []
    for rate in (1e-3, 1e-3, 2.5e-4):
        eng.load_state(enc, dec)
        eng.reset_optimizer()
        eng.set_lr(rate)
        w0 = eng.params.double().cpu()
        eng.train_step(0, None, 0, b)
        eng.sync()
        moves.append(eng.params.double().cpu() - w0)
    assert eng.graph_captures() == 1
    assert torch.equal(moves[0], moves[1])
    big = moves[0].abs() > 0.5e-3       # the weights whose first step is the full rate (|g| >> eps)
    assert int(big.sum()) > 1000
    ratio = moves[2][big] / moves[0][big]
    assert float((ratio - 0.25).abs().max()) < 1e-3, float((ratio - 0.25).abs().max())


def _oracle_moments(orc):
    out = {}
    for side, group in (("enc/", orc.enc), ("dec/", orc.dec)):
        for k, p in group.items():
            st = orc.optim.state.get(p)
            if st:
                out[side + k] = (st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


@pytest.mark.parametrize("name", ["cfg2_b4", "handspec_b4"])
def test_steps_under_steplr_no_further_from_fp64_than_the_reference(name):
    """StepLR(oracle.optim, 2, 0.5) on the fp32 oracle; the engine is handed the oracle's rate through set_lr() before every
    step (rates lr, lr, lr/2, lr/2, lr/4: two changes over five graph-replayed steps) and, as in
    test_adam_step_no_further_from_fp64_than_the_reference, the oracle's weights, running statistics and moments; an fp64
    oracle starts every step from the same state and rate.  Per tensor: |hip update - fp64 update| <= 3 |fp32 update - fp64
    update| + 1e-3 of the rate in force."""
    from oracle import cae_oracle as orc_mod
    torch.set_num_threads(8)
    case = GoldenCase(name)
    eng = _conv_engine(case)
    (b, b2) = (case.meta["batch"], case.x2.shape[0])
    orc = oracle_model(case)
    sched = torch.optim.lr_scheduler.StepLR(orc.optim, 2, 0.5)
    batches = [(torch.from_numpy(case.x), torch.from_numpy(case.t)), (torch.from_numpy(case.x2), torch.from_numpy(case.t2))]
    noisy = bn_bias_keys(case.spec)
    (worst, rates) = (0.0, [])
    for s in range(5):
        rate = orc.optim.param_groups[0]["lr"]
        rates.append(rate)
        before = orc.state()
        moments = _oracle_moments(orc)
        enc = {k[4:]: v for k, v in before.items() if k.startswith("enc/")}
        dec = {k[4:]: v for k, v in before.items() if k.startswith("dec/")}
        eng.load_state(enc, dec)
        eng.load_optimizer_state(moments, s)
        eng.set_lr(rate)
        to64 = lambda sd: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        o64 = orc_mod.OracleModel(case.spec, to64(enc), to64(dec), lr=rate, weight_decay=case.meta["weight_decay"])
        for side, group in (("enc/", o64.enc), ("dec/", o64.dec)):
            for k, p64 in group.items():
                if side + k in moments:
                    (m, v) = moments[side + k]
                    o64.optim.state[p64] = {"step": torch.tensor(float(s)), "exp_avg": m.double().clone(),
                                            "exp_avg_sq": v.double().clone()}
        (xb, tb) = batches[s % 2]
        orc.train_step(xb, tb)
        sched.step()
        o64.train_step(xb.double(), tb.double())
        eng.train_step(0, None, 0 if s % 2 == 0 else b, b if s % 2 == 0 else b2)
        (after32, after64) = (orc.state(), o64.state())
        (e2, d2) = eng.export_state()
        for side, sd in (("enc/", e2), ("dec/", d2)):
            for k, v in sd.items():
                key = side + k
                if k.endswith("num_batches_tracked") or "running_" in k or key in noisy:
                    continue
                b0 = before[key].numpy().astype(np.float64)
                d64 = after64[key].numpy() - b0
                d32 = after32[key].numpy().astype(np.float64) - b0
                dh = v.numpy().astype(np.float64) - b0
                (err_ref, err_hip) = (float(np.abs(d32 - d64).max()), float(np.abs(dh - d64).max()))
                worst = max(worst, err_hip / (3.0 * err_ref + 1e-3 * rate))
                print(f"{name} step {s} rate {rate:g} {key}: |hip - fp64| {err_hip:.3e}, reference's own {err_ref:.3e}")
                assert err_hip <= 3.0 * err_ref + 1e-3 * rate, \
                    f"step {s} {key}: |hip - fp64| = {err_hip:.3e}, the reference's own {err_ref:.3e} (rate {rate:g})"
    lr = case.meta["lr"]
    assert rates == [lr, lr, lr * 0.5, lr * 0.5, lr * 0.25], rates
    assert eng.graph_captures() <= 2, eng.graph_captures()     # one graph per batch size, whatever the rate
    print(f"{name}: worst ratio to the bound {worst:.2f}")


# ---- set_lr against set_hyper, bit for bit, on the four engines ----------------------------------------------------------------

def _two_ways(make, step, what, a=7e-3, b=4e-4):
    """`make()` -> a fresh engine in a fixed state; on one set_lr(a) then set_lr(b), on the other `set_hyper_lr(b)`; one step
    each; and a third at rate a, which must NOT give the same weights (the rate does reach the kernel)"""
    outs = []
    for how in ("set_lr", "set_hyper", "other rate"):
        (eng, set_hyper_lr) = make()
        if how == "set_lr":
            eng.set_lr(a)
            eng.set_lr(b)
        else:
            set_hyper_lr(b if how == "set_hyper" else a)
        step(eng)
        eng.sync()
        outs.append(_state(eng))
        eng.close()
    _same_bits(outs[0], outs[1], what)
    assert not torch.equal(outs[0][0][1], outs[2][0][1]), f"{what}: the rate did not change the step"


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "plain"])
def test_conv_set_lr_equals_set_hyper_bitwise(graph):
    case = GoldenCase("cfg2_b4")

    def make():
        eng = _conv_engine(case, graph=graph)
        return eng, lambda lr: eng.set_hyper(lr=lr, weight_decay=case.meta["weight_decay"])

    def step(eng):
        eng.run_batches(0, None, 7, 2, train=True)

    _two_ways(make, step, "ConvAE")


def test_unet_set_lr_equals_set_hyper_bitwise():
    from cae_tools_amd.unet_engine import UnetEngine
    c = UnetCase("u_k3s1_b2")
    m = c.meta

    def make():
        eng = UnetEngine(m["spec"], m["fc"], m["latent"], m["batch"], device="cuda:0")
        eng.load_state(c.state("init", "enc"), c.state("init", "dec"))
        hyper = dict(weight_decay=m["weight_decay"], dropout_rate=m["dropout"], lambda_pearson=m["lambda_pearson"], seed=0)
        eng.set_hyper(lr=m["lr"], **hyper)
        (x, t, mk) = c.step_batch(0)
        eng.set_dataset(0, x.cuda(), t.cuda(), mk.cuda())
        return eng, lambda lr: eng.set_hyper(lr=lr, **hyper)

    _two_ways(make, lambda eng: eng.train_step(0, None, 0, m["batch"], slot=0), "UNET")


def test_vae_set_lr_equals_set_hyper_bitwise():
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.var_ae_model import VarEncoder
    from cae_tools_amd.vae_engine import VaeEngine
    spec = create_model_spec(input_size=(12, 12), input_channels=1, output_size=(176, 176), output_channels=1)
    torch.manual_seed(13)
    enc = VarEncoder(spec.get_input_layers(), 8, 16)
    dec = Decoder(spec.get_output_layers(), 8, 16)
    g = torch.Generator().manual_seed(14)
    x = torch.rand((4, 1, 12, 12), generator=g)
    t = torch.rand((4, 1, 176, 176), generator=g)

    def make():
        eng = VaeEngine(spec, 16, 8, 4, device="cuda:0")
        eng.load_state(enc.state_dict(), dec.state_dict())
        eng.set_hyper(seed=1)
        eng.set_dataset(0, x.cuda(), t.cuda())
        return eng, lambda lr: eng.set_hyper(lr=lr, seed=1)

    _two_ways(make, lambda eng: eng.train_step(0, None, 0, 4, slot=0), "VAE")


def test_linear_set_lr_equals_set_hyper_bitwise():
    from cae_tools_amd.linear_engine import LinearEngine
    from test_linear_cpu import load
    (meta, z) = load("lin_2ch_b3")
    (x, t) = (torch.from_numpy(z["step0/x"]), torch.from_numpy(z["step0/t"]))

    def make():
        eng = LinearEngine(meta["in_shape"], meta["out_shape"], max_batch=8, device="cuda:0")
        eng.load_state({k: z["init/" + k] for k in meta["keys"]})
        eng.set_hyper(lr=meta["lr"], weight_decay=meta["weight_decay"])
        eng.set_dataset(0, x, t)
        return eng, lambda lr: eng.set_hyper(lr=lr, weight_decay=meta["weight_decay"])

    _two_ways(make, lambda eng: eng.train_step(0, None, 0, x.shape[0], slot=0), "Linear")


# ---- the model loops ---------------------------------------------------------------------------------------------------------

def _circles():
    from cae_tools_amd.data import datagen
    return datagen.generate("circle", 21, seed=1234), datagen.generate("circle", 9, seed=4321)


def _train_conv(tmp_path, tag, **kw):
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    (train, test) = _circles()
    torch.manual_seed(5)
    mt = ConvAEModel(batch_size=8, test_interval=1, fc_size=16, encoded_dim_size=4, lr=1e-3, weight_decay=1e-5, **kw)
    folder = str(tmp_path / tag)
    buf = io.StringIO()
    with redirect_stdout(buf):
        mt.train(["lowres"], "hires", train, test, model_path=folder)
    return mt, folder, buf.getvalue()


def test_conv_model_records_the_decayed_rates(tmp_path):
    (mt, folder, _) = _train_conv(tmp_path, "steplr", nr_epochs=6, scheduler_type="StepLR", lr_step_size=2, lr_gamma=0.1)
    lr = 1e-3
    np.testing.assert_allclose(mt.history["lr"], [lr, lr, lr * 0.1, lr * 0.1, lr * 0.01, lr * 0.01], rtol=1e-12, atol=0)
    assert len(mt.history["train_loss"]) == 6
    with open(os.path.join(folder, "history.json")) as f:
        assert json.load(f)["lr"] == mt.history["lr"]
    with open(os.path.join(folder, "parameters.json")) as f:
        p = json.load(f)
    assert (p["scheduler_type"], p["lr_step_size"], p["lr_gamma"]) == ("StepLR", 2, 0.1)
    # every graph shape of the loop was captured once, in the first epoch: the cache holds all that was ever captured
    assert mt._engine.graph_captures() == mt._engine.graph_count() >= 2, (mt._engine.graph_captures(), mt._engine.graph_count())
    # a loaded model carries the settings
    from cae_tools_amd.models.model_loader import load_model
    back = load_model(folder)
    assert (back.scheduler_type, back.lr_step_size, back.lr_gamma) == ("StepLR", 2, 0.1)


def test_no_scheduler_equals_a_unit_gamma_bit_for_bit(tmp_path):
    """scheduler_type=None against ExponentialLR with gamma 1.0 (set_lr before every epoch, always the same value): the same
    weights and losses in bits; and the folder of the plain run knows nothing of schedules"""
    (plain, f0, out0) = _train_conv(tmp_path, "plain", nr_epochs=3)
    (unit, f1, out1) = _train_conv(tmp_path, "unit", nr_epochs=3, scheduler_type="ExponentialLR", lr_gamma=1.0)
    for name in ("encoder.weights", "decoder.weights"):
        (a, b) = (torch.load(os.path.join(f0, name), weights_only=True), torch.load(os.path.join(f1, name), weights_only=True))
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{name}:{k}"
    assert plain.history["train_loss"] == unit.history["train_loss"] and plain.history["test_loss"] == unit.history["test_loss"]
    assert "lr" not in plain.history and unit.history["lr"] == [1e-3] * 3
    with open(os.path.join(f0, "parameters.json")) as f:
        assert not {"scheduler_type", "lr_step_size", "lr_gamma"} & set(json.load(f))
    with open(os.path.join(f0, "history.json")) as f:
        assert sorted(json.load(f)) == ["nr_epochs", "test_loss", "train_loss"]
    rows = lambda out: [l for l in out.splitlines() if l[:5].strip().isdigit() and len(l.split()) == 3]
    assert rows(out0) == rows(out1) and len(rows(out0)) == 3


def _unet_data(n, seed):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    rng = np.random.default_rng(seed)
    ds = Dataset()
    ds["lo"] = DataArray((280 + 10 * rng.random((n, 2, 16, 16))).astype(np.float32), dims=("n", "c", "y", "x"))
    ds["hi"] = DataArray((280 + 10 * rng.random((n, 1, 16, 16))).astype(np.float32), dims=("n", "c2", "y", "x"))
    ds["valid"] = DataArray((rng.random((n, 1, 16, 16)) < 0.85).astype(np.float32), dims=("n", "one", "y", "x"))
    return ds


def _train_unet(**kw):
    from cae_tools_amd.models.unet import UNET, unet_layer_spec
    torch.manual_seed(7)
    mt = UNET(batch_size=4, test_interval=1, fc_size=10, encoded_dim_size=4, lr=1e-3, weight_decay=1e-5, dropout_rate=0.1,
              lambda_pearson=0.5, **kw)
    mt.spec = unet_layer_spec(2, 1, (16, 16), [8, 16])
    buf = io.StringIO()
    with redirect_stdout(buf):
        mt.train(["lo"], "hi", _unet_data(12, 1), _unet_data(4, 2), mask_variable_name="valid")
    return mt, [l for l in buf.getvalue().splitlines() if l.startswith("learn rate:")]


def test_unet_prints_the_decayed_rate():
    """`learn rate:` is printed after the epoch's scheduler step, as the reference prints it (unet.py:485-496)"""
    (mt, lines) = _train_unet(nr_epochs=4, scheduler_type="StepLR", lr_step_size=1, lr_gamma=0.5)
    assert lines == ["learn rate: 0.000500", "learn rate: 0.000250", "learn rate: 0.000125", "learn rate: 0.000063"], lines
    np.testing.assert_allclose(mt.history["lr"], [1e-3, 5e-4, 2.5e-4, 1.25e-4], rtol=1e-12, atol=0)
    (plain, lines) = _train_unet(nr_epochs=2)
    assert lines == ["learn rate: 0.001000"] * 2 and "lr" not in plain.history


def test_var_and_linear_models_decay_and_record(tmp_path):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.linear_model import LinearModel
    from cae_tools_amd.models.var_ae_model import VarAEModel

    def data(n, seed):
        rng = np.random.default_rng(seed)
        hi = (285 + 8 * rng.random((n, 1, 176, 176))).astype(np.float32)
        ds = Dataset()
        ds["lowres"] = DataArray(np.ascontiguousarray(hi[:, :, ::15, ::15][:, :, :12, :12]), dims=("n", "chan", "y", "x"))
        ds["hires"] = DataArray(hi, dims=("n", "chan", "y2", "x2"))
        return ds

    sched = dict(scheduler_type="CosineAnnealingLR", lr_step_size=2)
    want = [1e-3, 5e-4, 0.0, 5e-4]
    torch.manual_seed(3)
    var = VarAEModel(batch_size=4, nr_epochs=4, test_interval=1, fc_size=12, encoded_dim_size=4, lr=1e-3, noise_seed=6, **sched)
    with redirect_stdout(io.StringIO()):
        var.train(["lowres"], "hires", data(9, 1), data(4, 2))
    np.testing.assert_allclose(var.history["lr"], want, rtol=1e-12, atol=1e-15)
    (train, test) = _circles()
    torch.manual_seed(3)
    lin = LinearModel(batch_size=8, nr_epochs=4, test_interval=1, lr=1e-3, **sched)
    with redirect_stdout(io.StringIO()):
        lin.train(["lowres"], "hires", train, test)
    np.testing.assert_allclose(lin.history["lr"], want, rtol=1e-12, atol=1e-15)
    # a zero rate is a step that moves nothing: the third epoch of the linear model left its weights where they were
    torch.manual_seed(3)
    two = LinearModel(batch_size=8, nr_epochs=2, test_interval=1, lr=1e-3, **sched)
    three = LinearModel(batch_size=8, nr_epochs=3, test_interval=1, lr=1e-3, **sched)
    outs = []
    for mt in (two, three):
        torch.manual_seed(3)
        with redirect_stdout(io.StringIO()):
            mt.train(["lowres"], "hires", train, test)
        outs.append(mt.weights.state_dict())
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_plateau_schedule_in_the_model_loop(tmp_path):
    """patience 0, factor 0.5: the rate halves after every test pass that fails to improve on the best loss by 1e-4 relative;
    replayed here from the recorded test losses"""
    from cae_tools_amd.lr_schedule import make_schedule
    (mt, _, _) = _train_conv(tmp_path, "plateau", nr_epochs=6, scheduler_type="ReduceLROnPlateau", lr_step_size=0, lr_gamma=0.5)
    ref = make_schedule("ReduceLROnPlateau", 1e-3, 0, 0.5)
    want = []
    for loss in mt.history["test_loss"]:
        want.append(ref.lr)
        ref.step_metric(loss)
    assert mt.history["lr"] == want, (mt.history["lr"], want)
