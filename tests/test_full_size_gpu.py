"""BASELINE.json's benchmark configuration at full size (cfg2: 16x16 -> 256x256, fc128/latent32,
batch 64, and the reference's own partial last batch of 36 from N=100): one training step and one
scoring pass of the HIP path against the CPU oracle, plus size-independent properties."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(n, seed):
    from cae_tools_amd.engine import HipEngine
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    from oracle import cae_oracle as orc
    spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(256, 256), output_channels=1)
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=32, fc_size=128)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=32, fc_size=128)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((n, 1, 16, 16), generator=g)
    t = torch.rand((n, 1, 256, 256), generator=g)
    eng = HipEngine(spec, 128, 32, max_batch=max(64, min(n, 160)))
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    ref = orc.OracleModel(spec.save(), enc.state_dict(), dec.state_dict(), lr=1e-3, weight_decay=1e-5)
    return eng, ref, x, t


@pytest.mark.parametrize("mode", [1, 5], ids=["lds-forward", "gather-forward"])
@pytest.mark.parametrize("batch", [64, 36, 160])
def test_training_step_at_benchmark_size(batch, mode):
    """64: the benchmark batch (fused encoder+Linear launch, 4 row groups in the fused Linear backward); 36: the reference's
    ragged last batch (a 4-row group); 160: the encoder no longer fits one workgroup's LDS (per-layer launches) and the
    Linear backward's ten row groups share the eight BatchNorm sum shards.
    mode 5: the channel-rich decoder layers' forward on the gather kernel k_ig_fwd_s2 (cae_set_kernel_mode bit 2) - the
    fallback for layers the LDS-staged forward does not take.  Until round 3 its gradients sat 6.8e-4 from the oracle's at
    batch 64: it folded its BatchNorm sums over lane groups and waves in fp32 (64 values per channel and workgroup) where
    k_ct_fwd_lds switches to fp64 after a lane's 16 values, and var = E[y^2] - mean^2 amplifies that rounding.
    Bound: no further from the fp64 oracle than 3x the fp32 oracle itself is (+1e-5 of the tensor's maximum), both oracles
    taking the HIP step's ReLU decisions where their own input is within rounding of zero (helpers.relu_fix_for) - a flat
    fp32-vs-fp32 tolerance flips with the summation order of either side, and with every ReLU input either side rounds to the
    other side of zero (one such bit moves the upstream gradients by ~1e-3 at this batch size)."""
    from helpers import assert_close_as_reference, hip_relu_decisions, relu_fix_for
    from oracle import cae_oracle as orc
    torch.set_num_threads(8)
    eng, ref, x, t = _setup(batch, 3)
    eng.lib.cae_set_kernel_mode(eng.handle, mode)
    slot = eng.forward_backward(0, None, 0, batch, batch)
    loss = eng._read_losses(slot, 1)[0]
    eng.sync()
    decisions = hip_relu_decisions(eng, batch)
    st = ref.state()
    side = lambda pre: {k[4:]: (v.double() if v.is_floating_point() else v) for k, v in st.items() if k.startswith(pre)}
    ref64 = orc.OracleModel(ref.spec, side("enc/"), side("dec/"), lr=1e-3, weight_decay=1e-5)
    (fix32, _) = relu_fix_for(ref, x, decisions, "fp32 oracle")
    (fix64, _) = relu_fix_for(ref64, x.double(), decisions, "fp64 oracle")
    loss_ref, _ = ref.loss_and_grads(x, t, relu_fix=fix32)
    assert abs(loss - loss_ref) <= 2e-6 * abs(loss_ref)
    ref64.loss_and_grads(x.double(), t.double(), relu_fix=fix64)
    g64 = ref64.grads()
    for k, g in ref.grads().items():
        if "encoder_cnn.0.bias" in k or "encoder_cnn.3.bias" in k or (k.startswith("dec/decoder_conv") and k.endswith("bias") and "15" not in k):
            continue  # biases that feed a BatchNorm: exact-zero gradient here, rounding noise in the reference
        assert_close_as_reference(eng.grad_view(k).cpu().numpy(), g.numpy(), g64[k].numpy(), f"B={batch} mode={mode} {k}")
    eng.profile_begin()
    eng.forward_backward(0, None, 0, batch, batch)
    labels = {name for (name, layer, us, nbytes) in eng.profile_end()}
    assert ("ig_convt_fwd" in labels) == (mode == 5) and ("ct_convt_fwd" in labels) == (mode == 1), labels


def test_scoring_and_properties_at_benchmark_size():
    torch.set_num_threads(8)
    eng, ref, x, t = _setup(100, 5)
    y = eng.score(x.cuda()).cpu()
    y_ref = ref.eval_forward(x)
    assert float((y - y_ref).abs().max()) <= 1e-5
    assert float(y.min()) > 0.0 and float(y.max()) < 1.0           # sigmoid range
    # scoring is per-sample in eval mode: any sub-batch gives the same rows (batch-size independence;
    # not bitwise: the kernel variant, hence the FMA order, is chosen by problem size)
    y_part = eng.score(x[37:58].cuda()).cpu()
    assert float((y_part - y[37:58]).abs().max()) <= 1e-6
    # a step on permuted sample order gives the same loss and gradients (sums are order-free to fp64)
    perm = np.random.default_rng(0).permutation(64).astype(np.int32)
    s1 = eng.forward_backward(0, None, 0, 64, 64); l1 = eng._read_losses(s1, 1)[0]; eng.sync(); g1 = eng.grads.clone()
    s2 = eng.forward_backward(0, eng.upload_perm(perm), 0, 64, 64); l2 = eng._read_losses(s2, 1)[0]; eng.sync(); g2 = eng.grads.clone()
    assert abs(l1 - l2) <= 1e-9 * abs(l1)   # per-block fp32 partials regroup; fp64 across blocks
    assert float((g1 - g2).abs().max()) <= 1e-6 * float(g1.abs().max())


@pytest.mark.parametrize("in_size,out_size,batch", [((32, 32), (512, 512), 3), ((20, 36), (300, 540), 2), ((8, 8), (128, 128), 5)])
def test_other_geometries_of_the_row_and_fused_kernels(in_size, out_size, batch):
    """Geometries that take the other branches of round 2's kernels (kernels_last.h, kernels_rows.h) than the benchmark does:
    32x32 -> 512x512: the last layer's input is 255 wide = three strips of the fused last-layer kernel (scalar target loads,
    strip-edge ownership, lane 0's left-hand column), the middle layers are wider than a wave (round 1's tile kernels);
    20x36 -> 300x540: non-square, odd widths, rows that end inside a lane's column pair;
    8x8 -> 128x128: maps of 16 and 32 quad columns (two images per wave, partly empty waves), an odd batch.
    One training step (loss, every gradient) and one scoring pass against the CPU oracle."""
    from cae_tools_amd.engine import HipEngine
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    from oracle import cae_oracle as orc
    from helpers import bn_bias_keys
    torch.set_num_threads(8)
    spec = create_model_spec(input_size=in_size, input_channels=1, output_size=out_size, output_channels=1)
    torch.manual_seed(17)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=8, fc_size=32)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=8, fc_size=32)
    g = torch.Generator().manual_seed(18)
    x = torch.rand((batch, 1) + in_size, generator=g)
    t = torch.rand((batch, 1) + out_size, generator=g)
    eng = HipEngine(spec, 32, 8, max_batch=8)
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    # 32x32 and 20x36 run the fused head and tail; 8x8 cannot (2 x 3 x 3 = 18 inputs of Linear 0: no whole k-steps)
    plan = eng.kernel_plan(batch, True)
    if in_size == (8, 8):
        assert plan["head"] == {"fwd": "layers", "why": "nin4"} and plan["tail"] == {"bwd": "layers", "why": "fc4"}, plan
    else:
        assert plan["head"]["fwd"] == "fused" and plan["tail"]["bwd"] == "fused", plan
    ref = orc.OracleModel(spec.save(), enc.state_dict(), dec.state_dict(), lr=1e-3, weight_decay=1e-5)
    slot = eng.forward_backward(0, None, 0, batch, batch)
    loss = eng._read_losses(slot, 1)[0]
    eng.sync()
    loss_ref, _ = ref.loss_and_grads(x, t)
    assert abs(loss - loss_ref) <= 2e-6 * abs(loss_ref)
    noisy = bn_bias_keys(spec.save())
    for k, gr in ref.grads().items():
        if k in noisy:
            continue
        got = eng.grad_view(k).cpu().numpy()
        scale = float(gr.abs().max())
        # small batches make BatchNorm ill-conditioned: fp32 against fp32
        assert float(np.abs(got - gr.numpy()).max()) <= 2e-3 * scale + 1e-9, k
    y = eng.score(x.cuda()).cpu()
    assert float((y - ref.eval_forward(x)).abs().max()) <= 2e-5
    # and the step did take the kernels this test is about (not a fallback): the launch labels of a profiled step
    eng.profile_begin()
    eng.forward_backward(0, None, 0, batch, batch)
    labels = {name for (name, layer, us, nbytes) in eng.profile_end()}
    assert "s2_convt_last_fused" in labels, labels
    assert "s2_convt_bwd" in labels and "s2_convt_fwd" in labels, labels


@pytest.mark.parametrize("batch", [64, 5])
def test_lds_staged_backward_alternative(batch):
    """kernels_ctbwd.h (cae_set_kernel_mode bit 1): the LDS-staged input-gradient + weight-gradient kernel of the channel-rich
    decoder layers on all three of them at the benchmark geometry.  Batch 64: 64->32 and 32->16 stage whole images (8 and 2 per
    workgroup, the task list split over 8 and 4 workgroups, plain accumulators), 16->8 runs four bands of four rows as it does
    by default.  Batch 5: every layer runs the band kernel with one image per workgroup (3 and 7 bands of one row, 8 bands of
    two rows with a last band of one), every band's last 16-position tile ragged; a short last image group is not reached
    here (test_ct_bwd_shapes_gpu.py runs those).  Same bar as test_training_step_at_benchmark_size: loss within 2e-6 of the
    fp32 oracle's, every gradient no further from the fp64 oracle than 3x the fp32 oracle is, both oracles taking the HIP
    step's ReLU decisions where their own input is within rounding of zero."""
    from cae_tools_amd.engine import HipEngine
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    from oracle import cae_oracle as orc
    from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for
    torch.set_num_threads(8)
    spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(256, 256), output_channels=1)
    torch.manual_seed(23)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=32, fc_size=128)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=32, fc_size=128)
    g = torch.Generator().manual_seed(24)
    x = torch.rand((batch, 1, 16, 16), generator=g)
    t = torch.rand((batch, 1, 256, 256), generator=g)
    eng = HipEngine(spec, 128, 32, max_batch=64, specialised=3)
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    ref = orc.OracleModel(spec.save(), enc.state_dict(), dec.state_dict(), lr=1e-3, weight_decay=1e-5)
    slot = eng.forward_backward(0, None, 0, batch, batch)
    loss = eng._read_losses(slot, 1)[0]
    eng.sync()
    decisions = hip_relu_decisions(eng, batch)
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref64 = orc.OracleModel(spec.save(), d64(enc.state_dict()), d64(dec.state_dict()), lr=1e-3, weight_decay=1e-5)
    (fix32, _) = relu_fix_for(ref, x, decisions, f"B={batch} fp32 oracle")
    (fix64, _) = relu_fix_for(ref64, x.double(), decisions, f"B={batch} fp64 oracle")
    loss_ref, _ = ref.loss_and_grads(x, t, relu_fix=fix32)
    assert abs(loss - loss_ref) <= 2e-6 * abs(loss_ref)
    ref64.loss_and_grads(x.double(), t.double(), relu_fix=fix64)
    g64 = ref64.grads()
    noisy = bn_bias_keys(spec.save())
    for k, gr in ref.grads().items():
        if k in noisy:
            continue
        assert_close_as_reference(eng.grad_view(k).cpu().numpy(), gr.numpy(), g64[k].numpy(), f"B={batch} mode=3 {k}")
    eng.profile_begin()
    eng.forward_backward(0, None, 0, batch, batch)
    labels = [name for (name, layer, us, nbytes) in eng.profile_end()]
    assert labels.count("ct_convt_bwd") == 3 and "ig_convt_bwd_pair" not in labels, labels
