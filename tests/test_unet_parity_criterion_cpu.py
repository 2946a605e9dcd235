"""The UNET gradient criterion of the GPU parity tests (tests/unet_helpers.py assert_unet_grads: |hip - fp64| <= 3 x the fp32
oracle's own error + 1e-5 of the tensor's maximum) against the criterion it replaced (2e-2 of a tensor's L2 norm, 15 % of its
largest entry), on the oracle alone: the fp32 oracle passes it, and two stand-ins for subtly wrong kernels that the old
criterion let through fail it.  This is what keeps the criterion from loosening unnoticed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from unet_helpers import MEDIUM_CASES, aligned_oracle_grads, assert_unet_grads, feeds_batchnorm

CASE = "64px_32-64-96"
WIDEST = "encoder_cnn.8.weight"        # (96, 64, 4, 4): the widest convolution of the case, K = 64 x 16
CHUNKED = "enc/encoder_cnn.4.weight"   # (64, 32, 4, 4): the fp32 oracle is ~1.6e-6 of its maximum from fp64 (well inside 1e-4)


def _old_criterion_holds(got, want):
    """the bound the benchmark-geometry tests used before: 2e-2 of each tensor's L2 norm, 15 % of its maximum per entry"""
    for k, w in want.items():
        if feeds_batchnorm(k):
            continue
        (g, w) = (np.asarray(got[k], dtype=np.float64), np.asarray(w, dtype=np.float64))
        if np.linalg.norm(g - w) > 2e-2 * max(np.linalg.norm(w), 1e-9) or np.abs(g - w).max() > 0.15 * max(np.abs(w).max(), 1e-6):
            return False
    return True


@pytest.fixture(scope="module")
def case():
    from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
    (in_c, out_c, size, chans, fc, latent, B) = MEDIUM_CASES[CASE]
    spec = unet_layer_spec(in_c, out_c, size, chans)
    torch.manual_seed(123)
    enc = Encoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    g = torch.Generator().manual_seed(9)
    (h, w) = size
    x = torch.rand((B, in_c, h, w), generator=g)
    t = torch.rand((B, out_c, h, w), generator=g)
    m = (torch.rand((B, 1, h, w), generator=g) < 0.85).float()
    kw = dict(dropout_rate=0.1, seed=4, step=2)
    (_, _, g32, g64, report) = aligned_oracle_grads(spec.save(), enc.state_dict(), dec.state_dict(), x, t, m, **kw)
    return dict(spec=spec.save(), enc=enc.state_dict(), dec=dec.state_dict(), x=x, t=t, m=m, kw=kw, g32=g32, g64=g64,
                report=report)


def test_fp32_oracle_meets_the_criterion(case):
    """(a) the fp32 oracle itself is 1/3 of the way to the bound on every tensor (no decisions to align: fp32 and fp64 agree
    on every ReLU and max-pool here)"""
    assert case["report"]["fp64"]["relu"] == 0 and case["report"]["fp64"]["argmax"] == 0
    assert assert_unet_grads(case["g32"], case["g32"], case["g64"], "fp32 oracle") <= 1 / 3 + 1e-6
    assert _old_criterion_holds(case["g32"], case["g64"])


class _MissingTap:
    """torch.nn.functional with one change: the convolution by `target` passes its input gradient through a copy of the
    weight with entry `idx` zeroed - one tap missing in an input-gradient kernel, with the forward and the weight gradient
    intact (to rounding)"""

    def __init__(self, target, idx):
        (self.target, self.idx) = (target, idx)

    def __getattr__(self, name):
        return getattr(F, name)

    def conv2d(self, x, w, b=None, **kw):
        if w is not self.target:
            return F.conv2d(x, w, b, **kw)
        wm = w.detach().clone()
        wm[self.idx] = 0
        return F.conv2d(x.detach(), w, b, **kw) + F.conv2d(x, wm, None, **kw) - F.conv2d(x.detach(), wm, None, **kw)


def test_one_missing_tap_fails_the_criterion_but_passed_the_old_one(case, monkeypatch):
    """(b) the fp32 oracle with one tap (entry (50, 30, 1, 2)) of the widest convolution's weight missing from its input
    gradient: every gradient upstream moves by ~4e-3 of its L2 norm, inside the old 2e-2, and hundreds of times the new bound.
    (Zeroing the entry in the state itself, forward included, is no subtle mutant at this geometry: the forward change alone
    moves the gradients by 2-5 % in the L2 sense even for a weight at the 1st percentile of |w|.)"""
    from oracle import unet_oracle as uo
    o = uo.UnetOracle(case["spec"], case["enc"], case["dec"], dropout_rate=case["kw"]["dropout_rate"], seed=case["kw"]["seed"])
    o.step_count = case["kw"]["step"]
    monkeypatch.setattr(uo, "F", _MissingTap(o.enc[WIDEST], (50, 30, 1, 2)))
    o.loss_and_grads(case["x"], case["t"], case["m"])
    monkeypatch.undo()
    mutant = o.grads()
    assert _old_criterion_holds(mutant, case["g64"])
    with pytest.raises(AssertionError, match=r"\|hip - fp64\|"):
        assert_unet_grads(mutant, case["g32"], case["g64"], "missing tap")


def test_one_k_chunk_off_by_1e_3_fails_the_criterion(case):
    """(c) the patch kernels walk K in chunks of four input channels x 16 taps: one chunk of the fp32 oracle's gradient of
    encoder_cnn.4 (the chunk that holds the tensor's largest entry) carrying a relative error of 1e-3"""
    g = case["g32"][CHUNKED]
    own = float((g.double() - case["g64"][CHUNKED]).abs().max() / case["g64"][CHUNKED].abs().max())
    assert own < 1e-5      # measured 1.6e-6
    c0 = 4 * (int(np.unravel_index(int(g.abs().argmax()), g.shape)[1]) // 4)
    bad = g.clone()
    bad[:, c0:c0 + 4] *= 1 + 1e-3
    mutant = dict(case["g32"], **{CHUNKED: bad})
    assert _old_criterion_holds(mutant, case["g64"])
    with pytest.raises(AssertionError, match=CHUNKED):
        assert_unet_grads(mutant, case["g32"], case["g64"], "one K chunk")
