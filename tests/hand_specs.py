"""Hand-written layer definitions (ModelSpec.load of a dict, the --layer-definitions-path form) that put the ConvAE engine's
decoder kernels where no sizer-made model does: output padding on the specialised stride-2 kernels, the gather forward
k_ig_fwd_s2 at every K split, k_ig_bwd_pair with one K slice, strides 1 and 3, kernels of 1, 2, 6 and 7 taps, thin layers with output padding as
layer 0, and a map of more than 8000 pixels (the integer-division arms).  tests/test_hand_specs_cpu.py checks without a GPU that the cases reach
what they name; tests/test_hand_specs_gpu.py holds them to the fp64 oracle.

Every spec has the encoder 1x12x12 -> (4, k3, s2) -> 4x5x5 (100 inputs of Linear 0: the fused head takes it), fc 16, latent 4.
A decoder is its input (C, H, W) and (cout, kernel, stride, output_padding) per layer; the dimensions follow the engine's
formulas: (in - k) // s + 1 for the encoder, (in - 1) * s + k + output_padding for the decoder."""

FC, LATENT = 16, 4
IN_SHAPE = (1, 12, 12)
ENCODER = [(4, 3, 2)]

# name -> (decoder input (C, H, W), [(cout, kernel, stride, output_padding)], batches)
SPECS = {
    "padded_thin": ((16, 1, 2), [(8, 3, 2, 1), (4, 3, 2, 1), (2, 4, 2, 1), (1, 4, 2, 1)], (2, 3)),
    "padded_thin33": ((16, 2, 1), [(8, 3, 2, 1), (4, 3, 2, 1), (2, 3, 2, 1), (1, 3, 2, 1)], (2, 3)),
    "padded_rich": ((32, 2, 3), [(16, 3, 2, 1), (8, 3, 2, 1), (4, 4, 2, 1), (2, 3, 2, 0), (1, (3, 4), 2, 1)], (2, 3)),
    "rich44_oddcout": ((20, 2, 2), [(7, 4, 2, 1), (3, 3, 2, 0), (1, 4, 2, 0)], (2, 3)),
    "gather_small": ((10, 3, 2), [(5, 3, 2, 0), (3, 2, 2, 0), (1, (4, 3), 2, 0)], (2, 3)),
    "gather_k": ((50, 1, 1), [(26, 4, 2, 0), (10, 3, 2, 1), (5, (2, 3), 2, 0), (2, 1, 2, 1), (1, 3, 2, 0)], (2, 3)),
    "gather_tpw": ((50, 22, 22), [(25, 3, 2, 0), (1, 3, 2, 0)], (2, 3, 8)),
    "gather_wide": ((10, 89, 90), [(5, 3, 2, 0), (1, 2, 2, 0)], (2,)),
    "strides": ((6, 4, 5), [(5, 3, 1, 0), (4, 2, 1, 0), (3, 6, 3, 0), (2, 2, 3, 1), (1, 7, 2, 0)], (2, 3)),
    # thin layers as layer 0 (behind a Linear layer: no row kernels), all with output padding
    "first84": ((8, 3, 4), [(4, 3, 2, 1), (2, 3, 2, 0), (1, 3, 2, 1)], (2, 3)),   # 1x36x44: 16-byte target loads in the last layer
    "first42": ((4, 3, 4), [(2, 3, 2, 1), (1, 4, 2, 1)], (2, 3)),
    "first63": ((6, 2, 3), [(3, 4, 2, 1), (1, 3, 2, 0)], (2, 3)),
    # the one large map, batch 8 only: 8 x 113 x 113 >= 100000 thread positions put scoring's last layer on k_s2_fwd2, and a
    # last layer 224 wide gives k_s2_last_fused a second strip - both with output padding
    "wide_last": ((4, 111, 111), [(2, 3, 2, 1), (1, 4, 2, 1)], (8,)),
}
PADDED = ("padded_thin", "padded_thin33", "padded_rich")
# kernel modes (cae_set_kernel_mode) a spec's GPU cases run: the default, the shape-generic kernels, and for the padded specs
# the LDS-staged backward on every eligible layer
MODES = {name: ((1, 0, 3) if name in PADDED else (1, 0)) for name in SPECS}

# name -> per decoder layer (forward of a training step, forward of scoring, backward) in the default mode, as `observed`
# below reads them from the plan report (EnginePlan.kernel_plan); the same at every batch of the spec.  "ct_bwd_lds lds" /
# "ct_bwd_lds band <bands>": the kernel of the LDS-staged backward; "ig_bwd_pair <ksplit>".
_ROWS84 = ("s2_fwd_rows<8,4,1,2>", "s2_fwd_rows<8,4,1,2>", "s2_bwd_rows<8,2,4,3,3,4,2,1>")
_IG = lambda ksplit: ("ig_fwd_s2", "ig_fwd_s2", f"ig_bwd_pair {ksplit}")
_UP = lambda ksplit: ("up", "up", f"ig_bwd_pair {ksplit}")
LAYERS = {
    "padded_thin": [("ct_fwd_lds<3,3>", "ct_fwd_lds<3,3>", "ct_bwd_lds lds"), _ROWS84,
                    ("s2_fwd_cs<4,2,4,4,32>", "s2_fwd_cs<4,2,4,4,32>", "s2_bwd<4,2,2,4,4>"),
                    ("last_fused<2,1,4,4>", "s2_fwd<2,1,4,4,64>", "(fused)")],
    "padded_thin33": [("ct_fwd_lds<3,3>", "ct_fwd_lds<3,3>", "ct_bwd_lds band 2"), _ROWS84,
                      ("s2_fwd_rows<4,2,2,2>", "s2_fwd_rows<4,2,2,2>", "s2_bwd_rows<4,4,2,3,3,2,2,3>"),
                      ("last_fused<2,1,3,3>", "s2_fwd<2,1,3,3,32>", "(fused)")],
    "padded_rich": [("ct_fwd_lds<3,3>", "ct_fwd_lds<3,3>", "ig_bwd_pair 4"),
                    ("ct_fwd_lds<3,3>", "ct_fwd_lds<3,3>", "ct_bwd_lds band 6"),
                    ("s2_fwd_cs<8,4,4,4,32>", "s2_fwd_cs<8,4,4,4,32>", "s2_bwd<8,2,4,4,4>"),
                    ("s2_fwd_rows<4,2,2,1>", "s2_fwd_rows<4,2,2,1>", "s2_bwd_rows<4,4,2,3,3,2,1,3>"),
                    ("last_fused<2,1,3,4>", "s2_fwd<2,1,3,4,64>", "(fused)")],
    "rich44_oddcout": [("ct_fwd_lds<4,4>", "ct_fwd_lds<4,4>", "ig_bwd_pair 4"), _IG(1), _UP(1)],
    "gather_small": [_IG(1), _IG(1), _UP(1)],
    "gather_k": [_IG(4), _IG(2), _IG(1), _IG(1), ("last_fused<2,1,3,3>", "s2_fwd<2,1,3,3,64>", "(fused)")],
    "gather_tpw": [_IG(4), _UP(1)],
    "gather_wide": [_IG(1), _UP(1)],
    "strides": [_UP(1), _UP(1), _UP(4), _UP(1), _UP(2)],
    "first84": [("s2_fwd_cs<8,4,3,3,32>", "s2_fwd_cs<8,4,3,3,32>", "s2_bwd_split<8,2,4,3,3,32>"),
                ("s2_fwd_rows<4,2,2,2>", "s2_fwd_rows<4,2,2,2>", "s2_bwd_rows<4,4,2,3,3,2,2,3>"),
                ("last_fused<2,1,3,3>", "s2_fwd<2,1,3,3,32>", "(fused)")],
    "first42": [("s2_fwd<4,2,3,3,32>", "s2_fwd<4,2,3,3,32>", "s2_bwd2<4,2,3,3,32>"),
                ("last_fused<2,1,4,4>", "s2_fwd<2,1,4,4,32>", "(fused)")],
    "first63": [("s2_fwd<6,3,4,4,32>", "s2_fwd<6,3,4,4,32>", "s2_bwd<6,3,3,4,4>"), _UP(1)],
    "wide_last": [("s2_fwd<4,2,3,3,64>", "s2_fwd<4,2,3,3,64>", "s2_bwd2<4,2,3,3,64>"),
                  ("last_fused<2,1,4,4>", "s2_fwd2<2,1,4,4,64>", "(fused)")],
}
# mode 3 moves one layer: the 32->16 layer of padded_rich, outside the default mask, onto the band kernel
MODE3 = {("padded_rich", 0): "ct_bwd_lds band 2"}


def expected(name, mode):
    """LAYERS[name] as kernel mode `mode` (0, 1, 3 or 5) changes it"""
    rows = []
    for (i, (fwd, score, bwd)) in enumerate(LAYERS[name]):
        if mode == 0:
            (fwd, score, bwd) = ("up", "up", "wgrad+down")
        if mode == 3:
            bwd = MODE3.get((name, i), bwd)
        if mode == 5 and fwd.startswith("ct_fwd_lds"):
            (fwd, score) = ("ig_fwd_s2", "ig_fwd_s2")
        rows.append((fwd, score, bwd))
    return rows


def observed(plan_train, plan_eval):
    """the rows of `expected` as the two plan reports of an engine give them"""
    rows = []
    for i in range(sum(k.startswith("dec") for k in plan_train)):
        (t, e) = (plan_train[f"dec{i}"], plan_eval[f"dec{i}"])
        bwd = t["bwd"]
        if bwd == "ct_bwd_lds":
            bwd += " lds" if t["ctb_kernel"] == "lds" else f" band {t['ctb_bands']}"
        elif bwd == "ig_bwd_pair":
            bwd += f" {t['ig_ksplit']}"
        rows.append((t["fwd"], e["fwd"], bwd))
    return rows


def _hw(k):
    return (int(k[0]), int(k[1])) if isinstance(k, (tuple, list)) else (int(k), int(k))


def _layer(is_input, kernel, stride, op, src, dst):
    return {"is_input": is_input, "kernel_size": list(kernel) if isinstance(kernel, (tuple, list)) else kernel, "stride": stride,
            "output_padding": op, "input_dimensions": list(src), "output_dimensions": list(dst)}


def input_layers(shape, layers):
    """[(cout, kernel, stride)] from an input of `shape` -> the "input_layers" list of a spec dict"""
    out = []
    (c, h, w) = shape
    for (cout, kernel, stride) in layers:
        (kh, kw) = _hw(kernel)
        dst = (cout, (h - kh) // stride + 1, (w - kw) // stride + 1)
        out.append(_layer(True, kernel, stride, 0, (c, h, w), dst))
        (c, h, w) = dst
    return out


def output_layers(shape, layers):
    """[(cout, kernel, stride[, output_padding])] from a decoder input of `shape` -> the "output_layers" list of a spec dict"""
    out = []
    (c, h, w) = shape
    for (cout, kernel, stride, *rest) in layers:
        op = rest[0] if rest else 0
        assert 0 <= op < stride
        (kh, kw) = _hw(kernel)
        dst = (cout, (h - 1) * stride + kh + op, (w - 1) * stride + kw + op)
        out.append(_layer(False, kernel, stride, op, (c, h, w), dst))
        (c, h, w) = dst
    return out


def spec_dict(name):
    (shape, layers, _) = SPECS[name]
    return {"input_layers": input_layers(IN_SHAPE, ENCODER), "output_layers": output_layers(shape, layers)}


def out_shape(name):
    return tuple(spec_dict(name)["output_layers"][-1]["output_dimensions"])


def model(name, n, seed):
    """(ModelSpec via load(), encoder state, decoder state, x, t) with n samples, as the shape tests build theirs"""
    import torch
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.model_sizer import ModelSpec
    spec = ModelSpec()
    spec.load(spec_dict(name))
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=LATENT, fc_size=FC)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=LATENT, fc_size=FC)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((n,) + IN_SHAPE, generator=g)
    t = torch.rand((n,) + out_shape(name), generator=g)
    # Encoder and Decoder zero every bias: the outputs that receive the bias only (output padding, a kernel smaller than its
    # stride) would all be 0, and a kernel that forgot to write them or to count them in the BatchNorm sums would pass.  So the
    # conv biases are drawn as torch's own initialiser of Conv2d / ConvTranspose2d draws them: uniform in +-1 / sqrt(fan_in),
    # fan_in = weight.shape[1] * KH * KW.
    states = []
    for module in (enc, dec):
        sd = {k: v.detach().clone() for (k, v) in module.state_dict().items()}
        for (k, v) in sd.items():
            w = sd.get(k[:-len("bias")] + "weight")
            if k.endswith(".bias") and w is not None and w.dim() == 4:
                bound = 1.0 / float(w.shape[1] * w.shape[2] * w.shape[3]) ** 0.5
                v.copy_((2.0 * torch.rand(v.shape, generator=g) - 1.0) * bound)
        states.append(sd)
    return spec, states[0], states[1], x, t
