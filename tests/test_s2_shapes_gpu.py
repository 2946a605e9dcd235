"""Every shape of the stride-2 decoder kernels (kernels_s2.h, kernels_last.h, kernels_rows.h) against the fp64 oracle.

The 16 shapes are S2_SHAPES x S2_KERNELS in engine_choose.h: Cin->Cout in 2->1, 4->2, 8->4, 6->3 times taps 3x3, 4x4, 3x4, 4x3.
GEOMETRIES are sizer-made models (create_model_spec, 16x16 inputs) whose decoders, together, put every shape in every position
a sizer-made decoder can give it (2->1 and 6->3 only as the last layer, 8->4 only in the middle), with odd, even and
non-square outputs and 1-3 output channels: 3-tap last layers (a parity with 2 taps one way and 1 the other), 3x4 / 4x3 last
layers, multi-channel last layers, and last layers of more than 72 weights, which the training step does not fuse (k_s2_fwd
with the S2_SIGMSE epilogue, then k_s2_bwd).  Each runs at batch 2 (k_s2_fwd / k_s2_fwd_cs on small maps, ragged tiles) and
32 (past the B * px * py >= 100000 switch of the last layer: k_s2_fwd2, split-K-heavy backward).  LARGE_BATCH runs the middle
layers past that switch too (k_s2_fwd2 with the S2_RAW_STATS / S2_RAW epilogues: every 4->2 and 8->4 shape, tile widths 16,
32 and 64), on the specialised kernels only.

Per case, one training step on the specialised kernels and (but LARGE_BATCH) one on the shape-generic ones
(cae_set_kernel_mode 0):
- loss and every gradient no further from the fp64 oracle than 3x the fp32 oracle is (helpers.assert_close_as_reference),
  both oracles taking the HIP step's ReLU decisions where their own input is within rounding of zero (relu_fix_for);
  conv biases that feed a BatchNorm (bn_bias_keys) on magnitude only
- score() (the S2_SIGOUT epilogue) within 1e-5 of the oracle's eval forward
- the launch labels of a profiled step, layer by layer, are those of EnginePlan.kernel_plan (test_engine_plan_cpu.py checks
  which branches these geometries reach).  A label names the kernel family (s2_convt_fwd covers k_s2_fwd / _cs / fwd2 /
  rows): this ties the plan to the family that ran, not to the variant within it
- two runs of two training steps give the same bits (as test_reproducible_gpu.py does for the benchmark geometry)."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for

pytestmark = pytest.mark.gpu

FC, LATENT = 16, 4
BATCHES = (2, 32)
# (output channels, output height, output width): decoder shapes in order, last layer last (test_engine_plan_cpu.py checks these)
GEOMETRIES = {
    (1, 221, 221): "8->4 4x4; 4->2 4x4 (k_s2_fwd_cs + k_s2_bwd); last 2->1 3x3 fused",
    (1, 193, 256): "8->4 3x3 rows; 4->2 4x3 (k_s2_fwd_cs + k_s2_bwd); last 2->1 3x4 fused",
    (1, 196, 255): "8->4 4x3 (k_s2_fwd_cs + k_s2_bwd); 4->2 3x3 rows; last 2->1 4x3 fused",
    (1, 260, 260): "4->2 3x3 tiles (k_s2_fwd + k_s2_bwd2: too wide for rows); last 2->1 4x4 fused",
    (1, 128, 129): "4->2 3x4 in the middle (k_s2_fwd_cs + k_s2_bwd)",
    (2, 221, 221): "last 4->2 3x3 fused two channels",
    (2, 224, 225): "8->4 3x4 in the middle; last 4->2 4x3 unfused",
    (2, 259, 260): "8->4 3x3 tiles (k_s2_fwd_cs + k_s2_bwd_split: too wide for rows); last 4->2 3x4 unfused",
    (2, 222, 222): "last 4->2 4x4 unfused",
    (3, 221, 221): "last 6->3 3x3 unfused three channels",
    (3, 221, 222): "last 6->3 3x4 unfused",
    (3, 194, 255): "last 6->3 4x3 unfused",
    (3, 222, 222): "last 6->3 4x4 unfused",
}
# middle layers on k_s2_fwd2: (output channels, height, width) -> (batch, what it reaches)
LARGE_BATCH = {
    (2, 108, 109): (512, "8->4 3x4 in the middle (k_s2_fwd2); last 4->2 4x3 (k_s2_fwd2)"),
    (2, 109, 108): (512, "8->4 4x3 in the middle (k_s2_fwd2); last 4->2 3x4 (k_s2_fwd2)"),
    (2, 109, 109): (512, "8->4 4x4 in the middle (k_s2_fwd2)"),
    (1, 108, 109): (512, "4->2 3x4 in the middle (k_s2_fwd2)"),
    (1, 109, 108): (512, "4->2 4x3 in the middle (k_s2_fwd2)"),
    (1, 109, 109): (512, "4->2 4x4 in the middle (k_s2_fwd2)"),
    (2, 259, 259): (96, "8->4 3x3 tiles (k_s2_fwd2 + k_s2_bwd_split: too wide for rows)"),
    (1, 259, 259): (96, "4->2 3x3 tiles (k_s2_fwd2 + k_s2_bwd2: too wide for rows)"),
}
# (geometry, batch, kernel modes) of every parity case
CASES = [(g, b, (1, 0)) for g in GEOMETRIES for b in BATCHES] + [(g, b, (1,)) for g, (b, _) in LARGE_BATCH.items()]

# launch label (ProfScope in engine_launch.h) of each kernel family that cae_debug_plan reports
_FWD_LABEL = {"s2_fwd_rows": "s2_convt_fwd", "s2_fwd": "s2_convt_fwd", "s2_fwd_cs": "s2_convt_fwd", "s2_fwd2": "s2_convt_fwd",
              "ct_fwd_lds": "ct_convt_fwd", "ig_fwd_s2": "ig_convt_fwd", "up": "dec_convt_fwd"}
_BWD_LABEL = {"(fused)": ["s2_convt_last_fused"], "s2_bwd_rows": ["s2_convt_bwd"], "s2_bwd2": ["s2_convt_bwd"],
              "s2_bwd_split": ["s2_convt_bwd"], "s2_bwd": ["s2_convt_bwd"], "ct_bwd_lds": ["ct_convt_bwd"],
              "ig_bwd_pair": ["ig_convt_bwd_pair"], "wgrad+down": ["dec_convt_wgrad", "dec_convt_dgrad"]}
_DEC_PREFIXES = ("s2_convt", "ct_convt", "ig_convt", "dec_convt")


def expected_labels(plan, n_dec, train):
    """{decoder layer: sorted launch labels} of a step with this kernel_plan"""
    out = {}
    for l in range(n_dec):
        p = plan[f"dec{l}"]
        fam = p["fwd"].split("<")[0]
        last = l == n_dec - 1
        labels = []
        if fam != "last_fused":
            label = _FWD_LABEL[fam]
            if last:
                label = {"s2_convt_fwd": "s2_convt_last", "dec_convt_fwd": "dec_convt_last"}[label] + ("_fwd_loss" if train else "_eval")
            elif not train:
                label = label.replace("_fwd", "_eval")
            labels.append(label)
        if train:
            labels += _BWD_LABEL[p["bwd"].split("<")[0]]
        out[l] = sorted(labels)
    return out


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _model(out_c, out_h, out_w, batch, seed):
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c)
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=LATENT, fc_size=FC)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=LATENT, fc_size=FC)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((2 * batch, 1, 16, 16), generator=g)
    t = torch.rand((2 * batch, out_c, out_h, out_w), generator=g)
    return spec, enc.state_dict(), dec.state_dict(), x, t


def _engine(spec, enc_sd, dec_sd, x, t, batch, mode):
    from cae_tools_amd.engine import HipEngine
    eng = HipEngine(spec, FC, LATENT, max_batch=batch, graph=False, specialised=mode)
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


@pytest.mark.parametrize("geometry,batch,modes", CASES, ids=["x".join(map(str, g)) + f"-{b}" for (g, b, _) in CASES])
def test_training_step_and_scoring_against_fp64_oracle(geometry, batch, modes):
    from oracle import cae_oracle as orc
    (out_c, out_h, out_w) = geometry
    spec, enc_sd, dec_sd, x, t = _model(out_c, out_h, out_w, batch, seed=out_h * 7 + out_w + out_c)
    xb, tb = x[:batch], t[:batch]
    noisy = bn_bias_keys(spec.save())
    n_dec = len(spec.get_output_layers())
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(xb).numpy()
    for mode in modes:
        what = f"{geometry} B={batch} mode={mode}"
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, mode)
        # scoring first, on the initial running statistics (eval forward: the S2_SIGOUT epilogue on the last layer)
        y = eng.score(xb.cuda()).cpu().numpy()
        assert float(np.abs(y - y_ref).max()) <= 1e-5, what
        slot = eng.forward_backward(0, None, 0, batch, batch)
        loss = eng._read_losses(slot, 1)[0]
        eng.sync()
        decisions = hip_relu_decisions(eng, batch)
        ref32 = orc.OracleModel(spec.save(), enc_sd, dec_sd, lr=1e-3, weight_decay=1e-5)
        d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        ref64 = orc.OracleModel(spec.save(), d64(enc_sd), d64(dec_sd), lr=1e-3, weight_decay=1e-5)
        (fix32, _) = relu_fix_for(ref32, xb, decisions, what + " fp32 oracle")
        (fix64, _) = relu_fix_for(ref64, xb.double(), decisions, what + " fp64 oracle")
        loss32, _ = ref32.loss_and_grads(xb, tb, relu_fix=fix32)
        loss64, _ = ref64.loss_and_grads(xb.double(), tb.double(), relu_fix=fix64)
        assert_close_as_reference([loss], [float(loss32)], [float(loss64)], f"{what} loss")
        g64 = ref64.grads()
        for k, g32 in ref32.grads().items():
            got = eng.grad_view(k).cpu().numpy()
            if k in noisy:
                # exactly zero in exact arithmetic: magnitude only
                assert np.abs(got).max() <= 1e-6 + 1e-4 * float(g32.abs().max()), f"{what} {k}"
                continue
            assert_close_as_reference(got, g32.numpy(), g64[k].numpy(), f"{what} {k}")
        # what ran is what the plan says, layer by layer (train step and eval forward)
        for (train, run) in ((True, lambda: eng.forward_backward(0, None, 0, batch, batch)), (False, lambda: eng.score(xb.cuda()))):
            eng.profile_begin()
            run()
            recs = eng.profile_end()
            got_labels = {l: sorted(name for (name, layer, _, _) in recs if layer == l and name.startswith(_DEC_PREFIXES))
                          for l in range(n_dec)}
            plan = eng.kernel_plan(batch, train)
            assert got_labels == expected_labels(plan, n_dec, train), (what, train, plan, recs)
            names = {name for (name, _, _, _) in recs}
            assert (("head_fwd" if train else "head_eval") in names) == (plan["head"]["fwd"] == "fused"), (what, names)
            if train:
                assert ("tail_bwd" in names) == (plan["tail"]["bwd"] == "fused"), (what, names)
        eng.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("geometry", [(2, 224, 225), (3, 221, 222), (1, 221, 221)], ids=lambda g: "x".join(map(str, g)))
def test_two_runs_of_two_steps_give_the_same_bits(geometry, batch):
    """unfused last layers (sharded bias gradient through the S2_SIGMSE epilogue) of 2 and 3 channels, and a fused 3-tap one"""
    (out_c, out_h, out_w) = geometry
    spec, enc_sd, dec_sd, x, t = _model(out_c, out_h, out_w, batch, seed=5)
    runs = []
    for _ in range(2):
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, 1)
        losses = [eng.train_step(0, None, k * batch, batch) for k in range(2)]
        eng.sync()
        runs.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = runs
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, name) in zip(a[1:], b[1:], ("params", "exp_avg", "exp_avg_sq", "running statistics")):
        assert torch.equal(u, v), f"{geometry} B={batch}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"
