"""Weight-gradient partial slabs of the decoder's backward (kernels_ctbwd.h CtBwd::wslab) and their fold in Linear 3's backward
launch (kernels_gemm.h wgrad_fold_body): the LDS-staged backward kernels (fp32 MFMA tiles) and the row kernels (kernels_rows.h
S2Rows::wslab: fp64 four-wave sums) store their per-workgroup weight-gradient partials with plain stores, the fold rounds every
partial to the accumulation grid and adds them in fp64 - exact sums, so the gradients are the bits the fp64 atomics gave.
cae_set_kernel_mode bit 3 (value 8) runs the atomics in the same build; the tests compare the two bit for bit.

CASES are sizer-made models from 16x16 inputs at the smallest shapes that reach the slab writers and the kernels around them:
- 1x80x81, batch 2, mode 1: a band-kernel slab (16->8 on a 4x4 map: four bands of one row, sharded accumulator) and a
  row-kernel slab (8->4, two images per wave); the 4->2 layer (3x4 taps) and the fused last layer keep their atomics
- 1x80x81, batch 3, mode 3: the same layers at an odd batch, every eligible layer on the LDS-staged backward
- 3x82x83, batch 8, mode 1: 3x4, 4x3 and 4x4 taps, three output channels - every channel-rich layer on the gather pair
  (ig_chunks 6 and 24), which keeps its atomics: the fold launch has no slab
- 1x256x256, batch 13, mode 3, fc 128 / latent 32: five slabs in one launch - both row kernels (8->4 and 4->2), the band
  kernel with a short last band (15 rows in bands of 2) on a sharded and on a plain accumulator, and whole maps
  (ctb_kernel=lds) with two images per workgroup and a last group of one.
test_cases_reach_what_they_name and test_slab_report_covers_every_folded_parameter_once need no GPU."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for
# the partial counts of the launches and the slab writers: one copy, shared with test_hand_specs_cpu.py
from wgrad_slabs import ATOMICS, KEPT_WRITERS, expected_partials as _expected_partials, writer as _writer

# ((output channels, height, width), batch, kernel mode, fc size, latent size)
CASES = [((1, 80, 81), 2, 1, 16, 4), ((1, 80, 81), 3, 3, 16, 4), ((3, 82, 83), 8, 1, 16, 4), ((1, 256, 256), 13, 3, 128, 32)]
_IDS = ["x".join(map(str, g)) + f"-{b}-mode{m}" for (g, b, m, _, _) in CASES]


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _spec(out_c, out_h, out_w):
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c)


def _reports(geometry, batch, mode, fc, latent, max_batch=None):
    """(kernel_plan, wgrad_slabs with the slabs on, wgrad_slabs with bit 3) of a case, no GPU"""
    from cae_tools_amd.engine import EnginePlan
    p = EnginePlan(_spec(*geometry).save(), fc, latent, max_batch=max_batch or max(batch, 8))
    try:
        p.set_kernel_mode(mode)
        (plan, slabs) = (p.kernel_plan(batch, True), p.wgrad_slabs(batch))
        p.set_kernel_mode(mode | ATOMICS)
        assert p.kernel_plan(batch, True) == plan   # bit 3 moves no kernel choice
        return plan, slabs, p.wgrad_slabs(batch)
    finally:
        p.close()


def test_cases_reach_what_they_name():
    reached = set()
    for (geometry, batch, mode, fc, latent) in CASES:
        (plan, _, _) = _reports(geometry, batch, mode, fc, latent)
        for (name, rep) in plan.items():
            if not name.startswith("dec"):
                continue
            bwd = rep["bwd"]
            if bwd == "ct_bwd_lds":
                reached |= {("ctb_kernel", rep["ctb_kernel"]), ("ctb_sharded", rep["ctb_sharded"])}
                if rep["ctb_kernel"] == "lds" and int(rep["ctb_imgs"]) == 2 and batch % 2:
                    reached.add("lds: two images per workgroup, ragged last group")
            elif bwd == "ig_bwd_pair" and int(rep["ig_chunks"]) > 1:
                reached.add("ig_bwd_pair with chunks > 1")
            elif bwd.startswith("s2_bwd_rows<"):
                reached.add("s2_bwd_rows")
            elif bwd == "(fused)":
                reached.add("fused last layer")
    want = {("ctb_kernel", "band"), ("ctb_kernel", "lds"), ("ctb_sharded", "0"), ("ctb_sharded", "1"),
            "lds: two images per workgroup, ragged last group", "ig_bwd_pair with chunks > 1", "s2_bwd_rows", "fused last layer"}
    assert want <= reached, sorted(map(str, want - reached))


# the GPU cases, the benchmark geometry, and two of test_ct_bwd_shapes_gpu.py's: whole maps of one image in four chunks
# (15x15 at batch 128) and image groups of three with a last group of two (9x9 at batch 512)
_REPORT_CASES = CASES + [((1, 256, 256), 64, 1, 128, 32), ((1, 256, 256), 128, 1, 16, 4), ((2, 81, 81), 512, 1, 16, 4)]


@pytest.mark.parametrize("geometry,batch,mode,fc,latent", _REPORT_CASES)
def test_slab_report_covers_every_folded_parameter_once(geometry, batch, mode, fc, latent):
    from cae_tools_amd.engine import EnginePlan
    spec = _spec(*geometry).save()
    dec = spec["output_layers"]
    (plan, slabs, off) = _reports(geometry, batch, mode, fc, latent)
    assert off == {"fold": {"slabs": "0", "wgs": "0", "bytes": "0", "capacity": slabs["fold"]["capacity"]}}
    p = EnginePlan(spec, fc, latent, max_batch=max(batch, 8))
    tensors = p.tensors
    p.close()
    writers = {name: rep for (name, rep) in plan.items() if name.startswith("dec") and _writer(rep) in KEPT_WRITERS}
    fold = slabs.pop("fold")
    assert set(slabs) == set(writers) and len(slabs) <= 6, (slabs, writers)
    (end, wgs, covered) = (0, 0, [])
    for name in sorted(slabs, reverse=True):   # launch order: last decoder layer first
        (s, l) = (slabs[name], int(name[3:]))
        (_, off_w, numel, _) = tensors[f"dec/decoder_conv.{3 * l}.weight"]
        assert (s["writer"], s["type"]) == _writer(writers[name]), (name, s)
        assert (int(s["param"]), int(s["values"])) == (off_w, numel), (name, s)
        assert int(s["partials"]) == _expected_partials(dec[l], writers[name], batch), (name, s)
        # a fold workgroup's lane groups cover the partials in one burst of 16 where 32 groups can (512 partials)
        vals = int(s["fold_values"])
        assert vals in (8, 16, 32, 64, 128, 256) and (vals == 8 or (256 // vals) * 16 >= int(s["partials"])), (name, s)
        assert int(s["offset"]) >= end and int(s["offset"]) % 256 == 0 and int(s["fold_wgs"]) == -(-numel // vals), (name, s)
        end = int(s["offset"]) + int(s["partials"]) * numel * (8 if s["type"] == "f64" else 4)
        wgs += int(s["fold_wgs"])
        covered.append((off_w, off_w + numel))
    # slabs neither overlap in the region nor in the parameters, and the region holds them
    assert all(a[1] <= b[0] for (a, b) in zip(sorted(covered), sorted(covered)[1:]))
    assert (int(fold["slabs"]), int(fold["wgs"]), int(fold["bytes"])) == (len(slabs), wgs, end)
    assert end <= int(fold["capacity"])


def test_report_names_a_short_last_band_and_a_ragged_last_group():
    (plan, slabs, _) = _reports((1, 256, 256), 13, 3, 128, 32)
    assert (plan["dec2"]["ctb_bands"], plan["dec2"]["ctb_hb"]) == ("8", "2")          # 15 rows: the last band has one
    assert (plan["dec0"]["ctb_imgs"], plan["dec0"]["ctb_groups"]) == ("2", "7")       # 13 images: the last group has one
    assert (slabs["dec2"]["partials"], slabs["dec1"]["partials"], slabs["dec0"]["partials"]) == ("104", "91", "7")
    assert (slabs["dec2"]["writer"], slabs["dec0"]["writer"]) == ("ct_bwd_band", "ct_bwd_lds")


def test_report_arguments_are_checked():
    import ctypes as C
    from cae_tools_amd import _lib
    from cae_tools_amd.engine import EnginePlan
    p = EnginePlan(_spec(1, 80, 81).save(), 16, 4, max_batch=8)
    try:
        with pytest.raises(_lib.CaeError, match="outside"):
            p.wgrad_slabs(9)
        with pytest.raises(_lib.CaeError, match="needs"):
            _lib.check(p.lib.cae_debug_wgrad_slabs(p.handle, 2, C.create_string_buffer(8), 8))
    finally:
        p.close()


def _model(geometry, n, fc, latent, seed):
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    spec = _spec(*geometry)
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=latent, fc_size=fc)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=latent, fc_size=fc)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((n, 1, 16, 16), generator=g)
    t = torch.rand((n,) + tuple(geometry), generator=g)
    return spec, enc.state_dict(), dec.state_dict(), x, t


def _engine(model, batch, fc, latent, mode, graph=False):
    from cae_tools_amd.engine import HipEngine
    (spec, enc_sd, dec_sd, x, t) = model
    eng = HipEngine(spec, fc, latent, max_batch=batch, graph=graph, specialised=mode)
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


def _same_bits(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} entries differ"


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,batch,mode,fc,latent", CASES, ids=_IDS)
def test_slabs_give_the_bits_of_the_atomics(geometry, batch, mode, fc, latent):
    model = _model(geometry, 3 * batch, fc, latent, seed=geometry[1] + geometry[2])
    got = {}
    for m in (mode, mode | ATOMICS):
        eng = _engine(model, batch, fc, latent, m)
        slot = eng.forward_backward(0, None, 0, batch, batch)
        loss = eng._read_losses(slot, 1)[0]
        eng.sync()
        grads = eng.grads.cpu().clone()
        eng.close()
        eng = _engine(model, batch, fc, latent, m)
        losses = [eng.train_step(0, None, k * batch, batch) for k in range(3)]
        eng.sync()
        got[m] = (loss, grads, losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu())
        eng.close()
    (a, b) = (got[mode], got[mode | ATOMICS])
    assert a[0] == b[0] and a[2] == b[2], ("losses", a[0], b[0], a[2], b[2])
    _same_bits(a[1], b[1], "fp32 gradient arena of forward_backward")
    for (u, v, name) in zip(a[3:], b[3:], ("weights", "exp_avg", "exp_avg_sq", "running statistics")):
        _same_bits(u, v, f"{name} after three training steps")


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,batch,mode,fc,latent", CASES, ids=_IDS)
def test_graph_replay_of_four_steps_equals_four_plain_steps(geometry, batch, mode, fc, latent):
    from cae_tools_amd._lib import check
    model = _model(geometry, 4 * batch, fc, latent, seed=11)
    got = []
    for graph in (True, False):
        eng = _engine(model, batch, fc, latent, mode, graph=graph)
        first = eng.claim_slots(4)
        if graph:
            eng.enqueue_train_steps(0, None, 4 * batch, batch, first)   # four full batches: one graph of four steps
            assert eng.graph_count() == 1
        else:
            for k in range(4):
                eng.set_cursor(k * batch, first + k)
                check(eng.lib.cae_train_step(eng.handle, 0, None, batch))
                eng._advance(batch, 1)
        losses = eng._read_losses(first, 4)
        eng.sync()
        got.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = got
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, name) in zip(a[1:], b[1:], ("weights", "exp_avg", "exp_avg_sq", "running statistics")):
        _same_bits(u, v, f"{name}: graph replay against plain launches")


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,batch,mode,fc,latent", CASES, ids=_IDS)
def test_gradients_against_fp64_oracle(geometry, batch, mode, fc, latent):
    """the project's fp64-anchored criterion, as test_ct_bwd_shapes_gpu.py applies it"""
    from oracle import cae_oracle as orc
    (spec, enc_sd, dec_sd, xb, tb) = model = _model(geometry, batch, fc, latent, seed=geometry[1] * 7 + geometry[2])
    noisy = bn_bias_keys(spec.save())
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    what = f"{geometry} B={batch} mode={mode}"
    eng = _engine(model, batch, fc, latent, mode)
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
    g64 = ref64.grads()
    got = {k: eng.grad_view(k).cpu().numpy() for k in g64}
    eng.close()
    assert_close_as_reference([loss], [float(loss32)], [float(loss64)], f"{what} loss")
    for k, g32 in ref32.grads().items():
        if k in noisy:
            assert np.abs(got[k]).max() <= 1e-6 + 1e-4 * float(g32.abs().max()), f"{what} {k}"   # zero in exact arithmetic
            continue
        assert_close_as_reference(got[k], g32.numpy(), g64[k].numpy(), f"{what} {k}")

