"""The LDS-staged forward of the channel-rich decoder layers (k_ct_fwd_lds, kernels_ctlds.h) against the fp64 oracle, over the
splits, bands and output shapes its host plan (ct_fwd_plan in engine_choose.h) can give it.

A workgroup of that kernel owns a tile group of one image: rt row tiles of 16 quads (2x2 output pixels), each shared by ks
waves that split the input channels; an image has tg = ceil(tiles / rt) groups.  It stages only the band of input rows its
quads read (first quad row - 1 .. last quad row, clamped to the map), inside a zero border, a channel's run of band rows dealt
to a power-of-two number of thread slots.  GEOMETRIES are sizer-made models (create_model_spec, 16x16 inputs)
whose decoders together reach (LAYERS lists every layer; test_cases_reach_what_they_name checks the list against the plan):
- ks of 8, 4, 2 and 1;
- one group per image (the band is the whole map) and 2 .. 8 groups: a first band (no halo row above: the zero border), middle
  bands, a last band (its last quad row reads the zero row below the map);
- a last tile that is partial (Q % 16 != 0), a group that begins and ends mid quad row (rt * 16 % QW != 0: neighbouring bands
  share a quad row), a last group with idle row tiles, bands from 1 or 2 floats per channel (1x1 and 1x2 input maps) up;
- odd and even output widths and heights, square and non-square maps;
- 3x3, 3x4, 4x3 and 4x4 taps;
- 6, 8 and 12 output channels (fewer columns than the 16 of a channel block), 16, 24 (a ragged second block), 32, 48, 64;
- batches 2 and 3 (plain block order; 3 leaves BatchNorm an odd count) and 8 (the XCD-aware block order).

Per case, one training step on the specialised kernels (mode 1) and one on the shape-generic ones (mode 0):
- loss and every gradient no further from the fp64 oracle than 3x the fp32 oracle is (helpers.assert_close_as_reference),
  both oracles taking the HIP step's ReLU decisions where their own input is within rounding of zero (relu_fix_for); conv
  biases that feed a BatchNorm (bn_bias_keys) on magnitude only
- score() (the same kernel without the BatchNorm sums) within 1e-5 of the oracle's eval forward
- two runs of two training steps give the same bits."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for

pytestmark = pytest.mark.gpu

FC, LATENT = 16, 4
BATCHES = (2, 3, 8)
# (output channels, output height, output width) -> the layers k_ct_fwd_lds runs, as
# (decoder layer, Cin, Cout, KH, KW, (H, W, OH, OW), ks, rt, tg)
LAYERS = {
    (1, 256, 256): [   # the benchmark's decoder: whole quad rows per group
        (0, 64, 32, 3, 3, (3, 3, 7, 7), 8, 1, 1),
        (1, 32, 16, 3, 3, (7, 7, 15, 15), 4, 2, 2),
        (2, 16, 8, 3, 3, (15, 15, 31, 31), 2, 4, 4),
    ],
    (3, 82, 83): [   # every 4-tap variant, ks = 1, a 1x1 input map, 7 groups that end mid row
        (0, 96, 48, 4, 4, (1, 1, 4, 4), 8, 1, 1),
        (1, 48, 24, 3, 3, (4, 4, 9, 9), 4, 2, 1),
        (2, 24, 12, 3, 4, (9, 9, 19, 20), 2, 4, 2),
        (3, 12, 6, 4, 3, (19, 20, 40, 41), 1, 4, 7),
    ],
    (2, 159, 191): [   # non-square throughout, 2 / 4 / 8 groups that end mid row, partial last tiles
        (0, 128, 64, 4, 3, (1, 2, 4, 5), 8, 1, 1),
        (1, 64, 32, 3, 3, (4, 5, 9, 11), 8, 1, 2),
        (2, 32, 16, 3, 3, (9, 11, 19, 23), 4, 2, 4),
        (3, 16, 8, 3, 3, (19, 23, 39, 47), 2, 4, 8),
    ],
}
GEOMETRIES = tuple(LAYERS)
CASES = [(g, b) for g in GEOMETRIES for b in BATCHES]
_IDS = ["x".join(map(str, g)) + f"-{b}" for (g, b) in CASES]


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _split(ci, kh, kw, oh, ow):
    """ct_fwd_plan's split of a layer: (ks, rt, tg)"""
    tiles = (((oh + 1) // 2) * ((ow + 1) // 2) + 15) // 16
    ks = 1
    while ks < 8 and ci * kh * kw // 4 // ks > 24 and ci % (ks * 8) == 0:
        ks *= 2
    rt = min(8 // ks, tiles, 4)
    return ks, rt, (tiles + rt - 1) // rt


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


def test_cases_reach_what_they_name():
    """LAYERS is what the sizer and the plan give: the layers on k_ct_fwd_lds, their shapes and their splits; and together
    they reach what the module's docstring lists"""
    from cae_tools_amd.engine import EnginePlan
    from cae_tools_amd.models.model_sizer import create_model_spec
    reached = set()
    for ((out_c, out_h, out_w), layers) in LAYERS.items():
        spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c).save()
        dec = spec["output_layers"]
        for batch in BATCHES:
            p = EnginePlan(spec, FC, LATENT, max_batch=8)
            try:
                plans = (p.kernel_plan(batch, True), p.kernel_plan(batch, False))
            finally:
                p.close()
            for plan in plans:
                on_ct = [i for i in range(len(dec)) if plan[f"dec{i}"]["fwd"].startswith("ct_fwd_lds")]
                assert on_ct == [l[0] for l in layers], (out_c, out_h, out_w, batch, plan)
        for (i, ci, co, kh, kw, (h, w, oh, ow), ks, rt, tg) in layers:
            k = dec[i]["kernel_size"]
            assert ((k, k) if isinstance(k, int) else tuple(k)) == (kh, kw)
            assert tuple(dec[i]["input_dimensions"]) == (ci, h, w) and tuple(dec[i]["output_dimensions"]) == (co, oh, ow)
            assert _split(ci, kh, kw, oh, ow) == (ks, rt, tg)
            assert plan[f"dec{i}"]["fwd"] == f"ct_fwd_lds<{kh},{kw}>"
            (qh, qw) = ((oh + 1) // 2, (ow + 1) // 2)
            tiles = (qh * qw + 15) // 16
            reached |= {("ks", ks), ("taps", kh, kw), ("cout", co), ("ow", ow % 2), ("oh", oh % 2), ("square", oh == ow),
                        ("groups", min(tg, 3)), ("partial last tile", qh * qw % 16 != 0),
                        ("mid-row groups", tg >= 3 and rt * 16 % qw != 0), ("idle tiles", tiles % rt != 0)}
    want = {("ks", 8), ("ks", 4), ("ks", 2), ("ks", 1), ("groups", 1), ("groups", 2), ("groups", 3)}
    want |= {("taps", kh, kw) for kh in (3, 4) for kw in (3, 4)}
    want |= {("cout", c) for c in (6, 8, 12, 16, 24, 32, 48, 64)}
    want |= {(k, v) for k in ("ow", "oh") for v in (0, 1)}
    want |= {(k, v) for k in ("square", "partial last tile", "mid-row groups", "idle tiles") for v in (True, False)}
    assert want <= reached, sorted(map(str, want - reached))


@pytest.mark.parametrize("geometry,batch", CASES, ids=_IDS)
def test_training_step_and_scoring_against_fp64_oracle(geometry, batch):
    from oracle import cae_oracle as orc
    (out_c, out_h, out_w) = geometry
    spec, enc_sd, dec_sd, x, t = _model(out_c, out_h, out_w, batch, seed=out_h * 7 + out_w + out_c)
    xb, tb = x[:batch], t[:batch]
    noisy = bn_bias_keys(spec.save())
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(xb).numpy()
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    for mode in (1, 0):
        what = f"{geometry} B={batch} mode={mode}"
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, mode)
        if mode == 1:
            for train in (True, False):
                plan = eng.kernel_plan(batch, train)
                for l in LAYERS[geometry]:
                    assert plan[f"dec{l[0]}"]["fwd"] == f"ct_fwd_lds<{l[3]},{l[4]}>", (what, plan)
        # scoring first, on the initial running statistics
        y = eng.score(xb.cuda()).cpu().numpy()
        err = float(np.abs(y - y_ref).max())
        print(f"{what}: score max|diff| {err:.3e}")
        assert err <= 1e-5, what
        slot = eng.forward_backward(0, None, 0, batch, batch)
        loss = eng._read_losses(slot, 1)[0]
        eng.sync()
        decisions = hip_relu_decisions(eng, batch)
        ref32 = orc.OracleModel(spec.save(), enc_sd, dec_sd, lr=1e-3, weight_decay=1e-5)
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
        eng.close()


@pytest.mark.parametrize("geometry,batch", CASES, ids=_IDS)
def test_two_runs_of_two_steps_give_the_same_bits(geometry, batch):
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
