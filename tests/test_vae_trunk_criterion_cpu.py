"""What the criterion of tests/test_vae_trunk_shapes_gpu.py catches that the bound of tests/test_vae_hip_parity.py lets through,
on the oracle alone (no GPU): six stand-ins for a subtly wrong trunk, each planted in the fp32 definition's gradients of the
`base` case (12x12 -> 176x192, fc 16, latent 6, batch 3), against

  new   per tensor  max|got - fp64| <= 3 max|fp32 - fp64| + 1e-5 max|fp64|   (helpers.assert_close_as_reference, its defaults)
  old   per tensor  |got - fp32|_2 <= 5e-3 |fp32|_2  and  max|got - fp32| <= 2e-2 max|fp32|

Measured (worst ratio error / bound over the tensors but the conv biases in front of a BatchNorm, and the tensor it is on):

  mutant                                                                     new                                old
  tap row      tap (0,0,0,0) of the last layer's weight gradient without     3968  dec/decoder_conv.12.weight   6.8   the same tensor
               input row 32
  layer scale  the last layer's weight gradient times 1.001                  38    dec/decoder_conv.12.weight   0.20  PASSES
  kl count     the KL gradient over B L - 1 = 17 instead of 18               2877  enc/encoder_cnn.1.bias       50    enc/encoder_cnn.1.weight
  logvar half  d z / d logvar without its 0.5                                32093 enc/encoder_logvar.bias      454   enc/encoder_cnn.1.weight
  bias row     the last bias gradient without the last output row            42    dec/decoder_conv.12.bias     0.58  PASSES
  relu bit     one ReLU of the 4->2 layer blocked at the layer's largest     457   dec/decoder_conv.10.weight   3.2   enc/encoder_cnn.1.weight
               input

Every mutant fails the new criterion, 38 to 32000 times over.  The old bound lets a 1e-3 scaling error of a layer and a row
missing from the bias sum through (asserted) - the mistakes of a wrong normalisation count or a loop that ends one row early -
and sees the others at 3 to 7 times its bound where the new one sees them at 450 to 4000 times: a dropped row at a tile edge
of a map twice as high, or the same ReLU bit in a layer twice as large, is inside it."""
import numpy as np
import pytest
import torch

from helpers import bn_bias_keys
from test_vae_trunk_shapes_gpu import _IDS, CASES, LAMBDAS, _model, _oracles

BASE = _IDS.index("base")
# mutant -> whether the old bound lets it through (measured on the oracle; asserted below)
MUTANTS = {"tap row": False, "layer scale": True, "kl count": False, "logvar half": False, "bias row": True, "relu bit": False}


class _ScaleGrad(torch.autograd.Function):
    """identity whose backward multiplies the gradient by `factor`"""

    @staticmethod
    def forward(ctx, x, factor):
        ctx.factor = factor
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.factor, None


def _params(o):
    return {pre + k: v for (pre, st) in (("enc/", o.enc), ("dec/", o.dec)) for k, v in st.items() if v.requires_grad}


def _step(o, x, t, logvar_factor=1.0, relu_fix=None):
    """VaeOracle.forward(train) + loss restated, so that a mutant can change one edge: ({name: gradient}, y, dL/dy, the loss
    parts as tensors).  logvar_factor scales the gradient that reaches logvar through z (1: the definition)"""
    from oracle import vae_oracle as vo
    from oracle.cae_oracle import decoder_forward
    (mu, logvar) = vo.encoder_forward(o.spec, o.enc, x, True, None, relu_fix)
    eps = torch.from_numpy(vo.normal_noise(o.seed, o.step_count, tuple(mu.shape))).to(mu.dtype)
    z = mu + eps * torch.exp(0.5 * _ScaleGrad.apply(logvar, logvar_factor))
    y = decoder_forward(o.spec, o.dec, z, True, None, relu_fix)
    parts = o.losses(y, t, mu, logvar)
    params = _params(o)
    (gy,) = torch.autograd.grad(o.total(parts), y, retain_graph=True)
    grads = torch.autograd.grad(o.total(parts), list(params.values()), retain_graph=True)
    return {k: g.detach().clone() for k, g in zip(params, grads)}, y, gy.detach(), parts


def _fresh(dtype_index):
    (spec, enc_sd, dec_sd, x, t, perm, idx) = _model(BASE)
    o = _oracles(spec, enc_sd, dec_sd)[dtype_index]
    cast = (lambda a: a) if dtype_index == 0 else (lambda a: a.double())
    return o, cast(x[idx]), cast(t[idx])


@pytest.fixture(scope="module")
def reference():
    """(fp32 gradients, fp64 gradients) of the definition, and the restatement checked against VaeOracle.loss_and_grads"""
    torch.set_num_threads(8)
    (o, x, t) = _fresh(0)
    (g32, _, _, parts) = _step(o, x, t)
    (o, x, t) = _fresh(0)
    (parts2, _) = o.loss_and_grads(x, t)
    assert [float(p.detach()) for p in parts] == parts2
    for k, v in o.grads().items():
        assert torch.equal(g32[k], v), k      # the restatement is the definition, bit for bit
    (o, x, t) = _fresh(1)
    o.loss_and_grads(x, t)
    return g32, o.grads()


def _mutant(name):
    """the fp32 definition's gradients with one thing wrong"""
    (o, x, t) = _fresh(0)
    c = CASES[BASE]
    last = "dec/decoder_conv.%d" % (3 * (len(o.spec["output_layers"]) - 1))
    if name == "logvar half":
        # z = mu + eps exp(logvar / 2): the 0.5 of d z / d logvar missing
        return _step(o, x, t, logvar_factor=2.0)[0]
    if name == "relu bit":
        # one ReLU of the 4->2 decoder layer (87 x 95 maps) blocks its gradient although its input is the largest of the layer
        z = o.relu_inputs(x)["dec_conv3"]
        d = torch.zeros_like(z)
        d.view(-1)[int(z.argmax())] = -1.0
        assert float(z.max()) > 1.0
        return _step(o, x, t, relu_fix={"dec_conv3": d})[0]
    (g, y, gy, parts) = _step(o, x, t)
    if name == "tap row":
        # tap (0, 0, 0, 0) of the last layer's weight gradient without input row 32 (output row 64 = 2 * 32 + 0: a tile edge)
        mask = torch.zeros_like(gy)
        mask[:, :, 64, :] = 1.0
        (part,) = torch.autograd.grad(y, o.dec[last[4:] + ".weight"], grad_outputs=gy * mask, retain_graph=True)
        assert float(part[:, :, 1::2, :].abs().max()) == 0.0      # an even output row takes kernel rows 0 and 2 only
        g[last + ".weight"][0, 0, 0, 0] -= part[0, 0, 0, 0]
    elif name == "layer scale":
        # a scaling error of 1e-3 in one layer: the last layer's weight gradient
        g[last + ".weight"] *= 1.001
    elif name == "bias row":
        # the last bias gradient summed over one output row too few
        du = gy * y.detach() * (1 - y.detach())
        g[last + ".bias"] -= du[:, :, -1, :].sum(dim=(0, 2))
    elif name == "kl count":
        # the KL term's gradient divided by B L - 1 instead of B L
        n = c.batch * c.latent
        params = _params(o)
        gk = torch.autograd.grad(parts[1], list(params.values()), allow_unused=True)
        for k, v in zip(params, gk):
            if v is not None:
                g[k] += LAMBDAS["lambda_kl"] * v * (n / (n - 1.0) - 1.0)
    else:
        raise KeyError(name)
    return g


def _new_ratio(got, g32, g64, skip):
    """worst |got - fp64| / bound of assert_close_as_reference over the tensors, and the tensor"""
    worst = (0.0, "")
    for k in g32:
        if k in skip:
            continue
        (a, r, e) = (got[k].double().numpy(), g32[k].double().numpy(), g64[k].numpy())
        bound = 3.0 * np.abs(r - e).max() + 1e-5 * np.abs(e).max() + 1e-9
        worst = max(worst, (float(np.abs(a - e).max() / bound), k))
    return worst


def _old_ratio(got, g32, skip):
    """worst of |got - fp32|_2 / (5e-3 |fp32|_2) and max|got - fp32| / (2e-2 max|fp32|) over the tensors, and the tensor"""
    worst = (0.0, "")
    for k in g32:
        if k in skip:
            continue
        (a, r) = (got[k].double().numpy(), g32[k].double().numpy())
        l2 = np.linalg.norm(a - r) / (5e-3 * max(np.linalg.norm(r), 1e-9))
        mx = np.abs(a - r).max() / (2e-2 * max(np.abs(r).max(), 1e-7))
        worst = max(worst, (float(max(l2, mx)), k))
    return worst


def test_the_definition_meets_both(reference):
    (g32, g64) = reference
    skip = bn_bias_keys(_fresh(0)[0].spec)
    assert _new_ratio(g32, g32, g64, skip)[0] <= 1 / 3 + 1e-9
    assert _old_ratio(g32, g32, skip)[0] == 0.0


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails_the_new_criterion(reference, name):
    (g32, g64) = reference
    skip = bn_bias_keys(_fresh(0)[0].spec)
    got = _mutant(name)
    (new, new_at) = _new_ratio(got, g32, g64, skip)
    (old, old_at) = _old_ratio(got, g32, skip)
    print(f"\n[trunk criterion] {name}: new {new:.1f} ({new_at}); old {old:.3f} ({old_at})")
    assert new > 1.0, (name, new, new_at)
    if MUTANTS[name]:
        assert old <= 1.0, (name, old, old_at)      # the old bound lets it through
