"""The UNET kernels below the kernel family - every template instantiation, K-slice regime, tile grouping and LDS regime the
launch code switches to (tests/test_unet_shapes_cpu.py lists them and pins, per case, what the launch code's own functions
answer) - against the fp32 and fp64 CPU oracles, and the fp32-in-fp64-slots state of the big Linear layers across steps that
change the kernel family."""
import time

import numpy as np
import pytest
import torch

from test_unet_shapes_cpu import check_pins
from unet_helpers import SHAPE_CASES, _against_aligned_oracles, _grad_dict, feeds_batchnorm

pytestmark = pytest.mark.gpu

(DROPOUT, SEED, LR) = (0.1, 4, 1e-3)


class _Model:
    """spec, initial state and data of one case (CPU tensors)"""

    def __init__(self, name, rows=None):
        from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
        (in_c, out_c, (h, w), chans, self.fc, self.latent, self.batches, self.max_batch) = SHAPE_CASES[name]
        self.name = name
        self.spec = unet_layer_spec(in_c, out_c, (h, w), chans)
        torch.manual_seed(123)
        self.enc = Encoder(self.spec.get_input_layers(), self.latent, self.fc).state_dict()
        self.dec = Decoder(self.spec.get_output_layers(), self.latent, self.fc).state_dict()
        n = rows or max(self.batches)
        g = torch.Generator().manual_seed(9)
        self.x = torch.rand((n, in_c, h, w), generator=g)
        self.t = torch.rand((n, out_c, h, w), generator=g)
        self.m = (torch.rand((n, 1, h, w), generator=g) < 0.85).float()     # a partial mask

    def engine(self, max_batch, specialised=True, state=None, rows=None):
        """a fresh engine with this model's (or the given) state, the module's hyper-parameters and rows [0, rows) as data set 0"""
        from cae_tools_amd.unet_engine import UnetEngine
        eng = UnetEngine(self.spec, self.fc, self.latent, max_batch, device="cuda:0", specialised=specialised)
        (enc, dec) = state or (self.enc, self.dec)
        eng.load_state(enc, dec)
        eng.set_hyper(lr=LR, dropout_rate=DROPOUT, seed=SEED)
        n = rows or self.x.shape[0]
        eng.set_dataset(0, self.x[:n], self.t[:n], self.m[:n])
        return eng


def _bitwise(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs, max |a - b| {float((a[k].double() - b[k].double()).abs().max()):.3e}"


def _check_adamw_step(eng, o32, what):
    """the engine after ONE train_step from zero moments against the fp32 oracle after its AdamW step on the same (aligned)
    gradients: the criterion of test_unet_hip_parity.py::test_adamw_steps"""
    g32 = o32.grads()
    o32.optim.step()
    want_all = o32.state()
    (enc, dec) = eng.export_state()
    for (pre, sd) in (("enc/", enc), ("dec/", dec)):
        for k, v in sd.items():
            want = want_all[pre + k].numpy()
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(want), f"{what}: {k}"
            elif feeds_batchnorm(pre + k):
                assert np.abs(v.numpy() - want).max() <= 2.1 * LR, f"{what}: {k}"   # Adam turns noise into +-lr
            else:
                # the first AdamW step is lr * sign(g) wherever |g| >> eps = 1e-8: entries whose oracle gradient is significant
                # must agree closely, the rest may differ by up to 2 * lr
                diff = np.abs(v.numpy() - want)
                assert diff.max() <= 2.1 * LR, f"{what}: {k}"
                if (pre + k) in g32:
                    sig = np.abs(g32[pre + k].numpy()) > 1e-5
                    assert (diff[sig] <= 2e-5 + 1e-4 * np.abs(want).max()).all(), f"{what}: {k}: {diff[sig].max():.3e}"
                else:   # running statistics
                    assert diff.max() <= 1e-5 + 1e-4 * np.abs(want).max(), f"{what}: {k}"


CASE_BATCHES = [(n, b) for n, c in SHAPE_CASES.items() for b in c[6]]


@pytest.mark.parametrize("name,batch", CASE_BATCHES, ids=[f"{n}-B{b}" for n, b in CASE_BATCHES])
def test_every_sub_branch_against_the_fp64_oracle(name, batch):
    """one training step at this batch, specialised kernels, dropout 0.1, a partial mask: losses and every gradient against the
    fp32 and fp64 oracles under this run's ReLU and max-pool decisions (3x the fp32 oracle's own distance + 1e-5 of the tensor's
    maximum + 1e-9; loss rtol 3e-5), score() against the oracle's eval forward (atol 2e-5), the same step on the generic
    kernels by the same bound, a second fresh engine bit for bit, and one AdamW step from zero moments.

    (lin_fc1028 at batch 3 is the case that made the generic transposed convolution k_up sum in fp64: with one fp32 chain per
    output the one-element bias gradient of its last layer lay 5.61e-8 from fp64 against a bound of 4.59e-8; now 2.7e-8.)"""
    t0 = time.time()
    torch.set_num_threads(16)
    check_pins(name, batch)
    M = _Model(name)
    (x, t, m) = (M.x[:batch], M.t[:batch], M.m[:batch])
    worst = {}

    def step_and_score(specialised):
        eng = M.engine(M.max_batch, specialised, rows=batch)
        (o32, grads, worst[specialised], _) = _against_aligned_oracles(
            eng, M.spec.save(), M.enc, M.dec, x, t, m, M.fc, M.latent, f"{name} B={batch} (specialised={specialised})",
            dropout_rate=DROPOUT, seed=SEED)
        # (o32 has seen one training forward, like the engine: their running statistics moved once)
        np.testing.assert_allclose(eng.score(x).cpu().numpy(), o32.eval_forward(x).numpy(), rtol=0, atol=2e-5)
        return grads, eng.read_losses(0, 1)[0], o32

    (grads, losses, o32) = step_and_score(True)
    # a second fresh engine repeats the step bit for bit
    again = M.engine(M.max_batch, rows=batch)
    _bitwise(grads, _grad_dict(again, again.forward_backward(0, None, 0, batch, slot=0)), f"{name} B={batch}: second engine")
    assert again.read_losses(0, 1)[0] == losses
    del again
    # one AdamW step from zero moments (the same forward and backward: the oracle's aligned gradients are its own)
    stepper = M.engine(M.max_batch, rows=batch)
    stepper.train_step(0, None, 0, batch, slot=0)
    assert stepper.read_losses(0, 1)[0] == losses
    _check_adamw_step(stepper, o32, f"{name} B={batch}: AdamW")
    del stepper
    # the generic kernels, by the same bound
    step_and_score(False)
    print(f"[unet shapes] {name} B={batch}: worst |hip-fp64|/bound specialised {worst[True]:.3f}, generic {worst[False]:.3f}; "
          f"{time.time() - t0:.1f} s")


def _flat_grads(eng, grads):
    flat = torch.zeros(eng.n_param, dtype=torch.float32)
    for n, (arena, off, numel, shape) in eng.tensors.items():
        if arena == 0:
            flat[off:off + numel] = grads[n].reshape(-1)
    flat = flat.to(eng.device)
    torch.cuda.synchronize()     # (the copy ran on torch's stream, the engine has its own)
    return flat


def _snapshot(eng):
    return dict(state=eng.export_state(), m=eng.exp_avg.clone(), v=eng.exp_avg_sq.clone(), steps=eng.steps)


def _full_state(eng):
    (enc, dec) = eng.export_state()
    out = {"enc/" + k: v for k, v in enc.items()}
    out.update({"dec/" + k: v for k, v in dec.items()})
    out["exp_avg"], out["exp_avg_sq"] = eng.exp_avg.cpu(), eng.exp_avg_sq.cpu()
    return out


def test_fp32_slots_across_kernel_families_step_by_step():
    """lin_k1296 at max_batch 96 over 200 rows: steps at batch 40 and 8 run the big Linear kernels, which leave fp32 weight
    gradients in the first half of the fp64 accumulator slots; steps at 96 and 70 run the tile engine, which adds fp64 into
    them.  After every forward_backward the gradients are held to the fp64 oracle loaded with the engine's state at that
    moment, and they - like the parameters and moments after every optimiser step - equal BIT FOR BIT those of a fresh engine
    that loaded that state (moments and step count too) and made this one call: its accumulator is clean, so a stale fp32
    half, a missed clear or a wrong fp32 range is an exact inequality (the reductions are order-independent: DESIGN.md §2)"""
    torch.set_num_threads(16)
    name, rows, max_batch = "lin_k1296", 200, 96
    for b in (8, 40, 64):
        assert check_pins_family(name, b, max_batch) == "lin_big"
    for b in (70, 96):
        assert check_pins_family(name, b, max_batch) == "tile"
    M = _Model(name, rows=rows)
    eng = M.engine(max_batch)
    worst = 0.0

    def fresh(snap):
        e2 = M.engine(max_batch, state=snap["state"])
        e2.exp_avg.copy_(snap["m"])
        e2.exp_avg_sq.copy_(snap["v"])
        e2.set_step(snap["steps"])
        torch.cuda.synchronize()     # (the copies ran on torch's stream, the engine has its own)
        return e2

    def fb(batch, what):
        nonlocal worst
        snap = _snapshot(eng)
        (enc_sd, dec_sd) = snap["state"]
        (_, grads, w, _) = _against_aligned_oracles(eng, M.spec.save(), enc_sd, dec_sd, M.x[:batch], M.t[:batch], M.m[:batch], M.fc,
                                                    M.latent, f"sequence {what}", dropout_rate=DROPOUT, seed=SEED, step=snap["steps"])
        worst = max(worst, w)
        e2 = fresh(snap)
        _bitwise(grads, _grad_dict(e2, e2.forward_backward(0, None, 0, batch, slot=0)), f"sequence {what}: fresh engine")
        assert e2.read_losses(0, 1)[0] == eng.read_losses(0, 1)[0]
        return grads

    def train(start, batch, what):
        snap = _snapshot(eng)
        eng.train_step(0, None, start, batch, slot=1)
        e2 = fresh(snap)
        e2.train_step(0, None, start, batch, slot=1)
        _bitwise(_full_state(eng), _full_state(e2), f"sequence {what}: fresh engine")
        assert e2.read_losses(1, 1)[0] == eng.read_losses(1, 1)[0]

    fb(40, "1: forward_backward at 40")
    train(96, 96, "2: train_step at 96")
    train(192, 8, "3: train_step at 8")
    train(0, 96, "4: train_step at 96")
    grads = fb(96, "5: forward_backward at 96")
    snap = _snapshot(eng)
    eng.apply_gradients(_flat_grads(eng, grads))
    e2 = fresh(snap)
    e2.apply_gradients(_flat_grads(e2, grads))
    _bitwise(_full_state(eng), _full_state(e2), "sequence 6: apply_gradients: fresh engine")
    del e2
    fb(40, "7: forward_backward at 40")
    snap = _snapshot(eng)
    eng.eval_step(0, None, 100, 70, slot=2)
    e2 = fresh(snap)
    e2.eval_step(0, None, 100, 70, slot=2)
    assert e2.read_losses(2, 1)[0] == eng.read_losses(2, 1)[0]
    del e2
    fb(70, "9: forward_backward at 70")
    print(f"[unet shapes] state sequence on {name}: worst |hip-fp64|/bound {worst:.3f}")


def check_pins_family(name, batch, max_batch):
    """the Linear family of the first layer of `name` at this batch in an engine of max_batch"""
    from cae_tools_amd.models.unet import unet_layer_spec
    from cae_tools_amd.unet_engine import UnetPlan
    (in_c, out_c, size, chans, fc, latent, _, _) = SHAPE_CASES[name]
    p = UnetPlan(unet_layer_spec(in_c, out_c, size, chans), fc, latent, max_batch)
    try:
        plan = p.kernel_plan(batch, True)
        assert plan["fc0"]["fwd"] == plan["fc3"]["fwd"] == plan["fc0"]["bwd"]
        return plan["fc0"]["fwd"]
    finally:
        p.close()
