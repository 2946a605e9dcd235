"""The launch sequence of a ConvAE step, launch by launch, against a recorded one (tests/golden/launch_order.json).

The host code of the step (engine_launch.h, engine_step.h) is a loop over layers that switches on the choosers of
engine_choose.h and brackets every launch with a ProfScope: label, layer index and algorithmic bytes.  A change to that host
code that is meant to leave the step alone must leave this record alone: the same labels, for the same layers, in the same
order, with the same byte counts (equal as floats).  The fixture was recorded before the host code was split into headers.

CASES are sizer-made models (create_model_spec, 16x16 inputs, outputs of at most 128 px, batches of at most 8) at the kernel
modes 0 / 1 / 3 / 5 of cae_set_kernel_mode.  Together their plans (EnginePlan.kernel_plan, checked without a GPU by
test_cases_reach_every_family) name every decoder forward and backward family the choosers can return, the fused and the
per-layer head, and the fused and the per-layer tail.  Each case records one train_step and one eval step.  DP_CASE runs the
in-library data-parallel step on a one-rank RCCL group (set up as test_timed_path_gpu.py does), without and with SyncBN:
dp_narrow_bucket0 / 1, the table all-reduce branches and the un-fused encoder backward."""
import json
import os
import socket

import pytest
import torch

FC, LATENT = 16, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_order.json")

# ((output channels, height, width), batch, kernel mode)
CASES = [
    ((1, 80, 81), 2, 1),    # ct_fwd_lds, s2_fwd_cs, s2_fwd_rows, fused last layer; ig_bwd_pair, ct_bwd_lds, s2_bwd, s2_bwd_rows
    ((1, 80, 81), 3, 3),    # the LDS-staged backward on every eligible layer, an odd batch
    ((1, 24, 24), 2, 0),    # shape-generic kernels throughout: k_up, k_wgrad + k_down, per-layer head and tail
    ((1, 24, 24), 2, 1),    # k_s2_bwd_split
    ((2, 24, 24), 2, 5),    # the gather forward k_ig_fwd_s2, an unfused last layer (k_s2_fwd with the loss epilogue)
    ((3, 82, 83), 8, 1),    # 3x4 / 4x3 / 4x4 taps, three output channels, the XCD-aware block order of batch 8
]
DP_CASE = ((1, 80, 81), 2, 1)
_ID = lambda c: "x".join(map(str, c[0])) + f"-b{c[1]}-m{c[2]}"

FWD_FAMILIES = {"last_fused", "s2_fwd_rows", "s2", "ct_fwd_lds", "ig_fwd_s2", "up"}                    # DecFwdK
BWD_FAMILIES = {"(fused)", "s2_bwd_rows", "s2", "ct_bwd_lds", "ig_bwd_pair", "wgrad+down"}             # DecBwdK


def _spec(geometry):
    from cae_tools_amd.models.model_sizer import create_model_spec
    (out_c, out_h, out_w) = geometry
    return create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c)


def _family(name):
    fam = name.split("<")[0]
    return "s2" if fam in ("s2_fwd", "s2_fwd_cs", "s2_fwd2", "s2_bwd", "s2_bwd2", "s2_bwd_split") else fam


def test_cases_reach_every_family():
    from cae_tools_amd.engine import EnginePlan
    (fwd, bwd, head, tail) = (set(), set(), set(), set())
    assert len(CASES) + 1 <= 8
    for (geometry, batch, mode) in CASES:
        assert batch <= 8 and max(geometry[1:]) <= 128 and mode in (0, 1, 3, 5)
        p = EnginePlan(_spec(geometry).save(), FC, LATENT, max_batch=8)
        try:
            p.set_kernel_mode(mode)
            plans = (p.kernel_plan(batch, True), p.kernel_plan(batch, False))
        finally:
            p.close()
        for plan in plans:
            for (name, fields) in plan.items():
                if name.startswith("dec"):
                    fwd.add(_family(fields["fwd"]))
                    bwd.add(_family(fields["bwd"]))
            head.add(plan["head"]["fwd"])
            tail.add(plan["tail"]["bwd"])
    assert fwd == FWD_FAMILIES, fwd ^ FWD_FAMILIES
    assert bwd - {"-"} == BWD_FAMILIES, bwd ^ BWD_FAMILIES
    assert head == {"fused", "layers"} and tail == {"fused", "layers", "-"}, (head, tail)


def _engine(geometry, batch, mode):
    from cae_tools_amd.engine import HipEngine
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    spec = _spec(geometry)
    torch.manual_seed(11)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=LATENT, fc_size=FC)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=LATENT, fc_size=FC)
    g = torch.Generator().manual_seed(12)
    x = torch.rand((batch, 1, 16, 16), generator=g)
    t = torch.rand((batch,) + tuple(geometry), generator=g)
    eng = HipEngine(spec, FC, LATENT, max_batch=batch, graph=False, specialised=mode)
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


def _profiled(eng, step):
    eng.profile_begin()
    step()
    return [[name, layer, nbytes] for (name, layer, us, nbytes) in eng.profile_end() if name != "event_pair"]


def record_case(geometry, batch, mode):
    """{"train": [[label, layer, bytes], ...], "eval": [...]} of one train_step and one eval step"""
    eng = _engine(geometry, batch, mode)
    return {"train": _profiled(eng, lambda: eng.train_step(0, None, 0, batch)),
            "eval": _profiled(eng, lambda: eng.run_batches(0, None, batch, batch, train=False))}


def init_one_rank_group():
    import torch.distributed as dist
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        return dist, True
    return dist, False


def record_dp_case(dist, geometry, batch, mode):
    """{"dp": ..., "dp_syncbn": ...} of one data-parallel training step on a one-rank group, without and with SyncBN"""
    from cae_tools_amd.dp import DataParallel
    eng = _engine(geometry, batch, mode)
    DataParallel(eng, dist, sync_bn=False, overlap=False)
    out = {}
    for (key, sync) in (("dp", False), ("dp_syncbn", True)):
        def step():
            eng.set_cursor(0, eng.claim_slots(1))
            eng.dp_train_steps(0, None, batch, batch, sync, 1)
        out[key] = _profiled(eng, step)
    eng.sync()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want, what):
    assert [r[:2] for r in got] == [r[:2] for r in want], (what, got, want)
    for (g, w) in zip(got, want):
        assert float(g[2]) == float(w[2]), (what, g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_launch_sequence_is_the_recorded_one(case):
    want = _golden()[_ID(case)]
    got = record_case(*case)
    assert set(got) == set(want)
    for part in got:
        assert len(want[part]) > 0
        _same(got[part], want[part], (_ID(case), part))


@pytest.fixture(scope="module")
def dist1():
    (dist, mine) = init_one_rank_group()
    yield dist
    if mine:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_data_parallel_launch_sequence_is_the_recorded_one(dist1):
    want = _golden()["dp-" + _ID(DP_CASE)]
    got = record_dp_case(dist1, *DP_CASE)
    assert set(got) == set(want)
    for part in got:
        _same(got[part], want[part], ("dp", part))
    labels = {part: [r[0] for r in got[part]] for part in got}
    assert "dp_narrow_bucket1" in labels["dp"] and "dp_narrow_bucket0" in labels["dp_syncbn"], labels
    assert "enc_conv_dgrad" in labels["dp_syncbn"] and "head_fwd" not in labels["dp_syncbn"], labels
