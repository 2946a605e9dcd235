"""Which decoder kernels the ConvAE engine runs, read from the choosers its launch code switches on (cae_debug_plan in
include/cae_hip.h, EnginePlan.kernel_plan), without a GPU:
- the benchmark geometry's plan (cfg2 at batch 64, train and eval), pinned
- cae_set_kernel_mode 0 / 3 / 5 move the layers they are about, and only those
- BRANCHES: every (step part, kernel family, Cin, Cout, KH, KW, position) of the stride-2 decoder kernels the choosers can
  return.  The key is the kernel FAMILY: template variants the plan also reports (tile widths, the fused last layer's vec4 /
  bn) are not part of it, so a covered branch says that the family ran for that shape and position, not every instantiation.
  A sweep of create_model_spec over outputs of 60..300 px and 1..3 channels, at batches 2, 32 and 512, plus the hand-written
  handspec_b4 form, reaches exactly BRANCHES minus UNREACHABLE
- the geometries of the GPU tests (test_s2_shapes_gpu.py's cases and the older ones) reach the families their descriptions
  name, and together every branch of BRANCHES but UNREACHABLE."""
import re

import pytest

from helpers import MODEL_CASES, GoldenCase
from cae_tools_amd import _lib
from cae_tools_amd.engine import EnginePlan
from cae_tools_amd.models.model_sizer import create_model_spec

S2_PAIRS = ((2, 1), (4, 2), (8, 4), (6, 3))
TAPS = ((3, 3), (4, 4), (3, 4), (4, 3))


def _branches_possible():
    """what the choosers can return for each stride-2 shape and position (engine.hip choose_dec_fwd / choose_s2_fwd /
    choose_dec_bwd / choose_s2_bwd): ("fwd" train forward | "eval" forward | "bwd", kernel family, Cin, Cout, KH, KW, position)"""
    out = set()
    for (ci, co) in S2_PAIRS:
        for (kh, kw) in TAPS:
            nw = ci * co * kh * kw
            for pos in ("mid", "last"):
                add = lambda fam, k: out.add((fam, k, ci, co, kh, kw, pos))
                for fam in ("fwd", "eval"):
                    add(fam, "s2_fwd")
                    add(fam, "s2_fwd2")
                    if pos == "mid" and nw > 80 and (256 // co) % 64 == 0:
                        add(fam, "s2_fwd_cs")
                    if pos == "mid" and (kh, kw) == (3, 3) and (ci, co) in ((4, 2), (8, 4)):
                        add(fam, "s2_fwd_rows")
                if pos == "last" and nw <= 72:
                    add("fwd", "last_fused")
                    add("bwd", "(fused)")
                add("bwd", "s2_bwd2" if nw <= 72 else ("s2_bwd_split" if ci == 8 and nw // 4 <= 72 else "s2_bwd"))
                if pos == "mid" and (kh, kw) == (3, 3) and (ci, co) in ((4, 2), (8, 4)):
                    add("bwd", "s2_bwd_rows")
    return out


BRANCHES = _branches_possible()

# (predicate over a branch, reason): no sizer-made decoder (1..3 output channels) or hand-written layer file of the suite puts
# a layer there
UNREACHABLE_RULES = [
    (lambda f, k, ci, co, kh, kw, pos: ci == 2 and pos == "mid",
     "2->1 leaves one channel: the sizer makes it only as the last layer"),
    (lambda f, k, ci, co, kh, kw, pos: ci == 8 and pos == "last",
     "8->4 as the last layer means 4 output channels: the sizer's decoders here have 1..3"),
    (lambda f, k, ci, co, kh, kw, pos: ci == 6 and pos == "mid" and (kh, kw) != (3, 3),
     "the sizer makes 6->3 only as a 3-channel last layer; only handspec_b4 puts it in the middle, with 3x3 taps"),
    (lambda f, k, ci, co, kh, kw, pos: ci == 6 and pos == "mid" and k == "s2_fwd2",
     "handspec_b4's 6->3 middle layer has a 12x12 map: k_s2_fwd2 would take a batch above 2700"),
    (lambda f, k, ci, co, kh, kw, pos: f == "fwd" and pos == "last" and k in ("s2_fwd", "s2_fwd2") and ci * co * kh * kw <= 72,
     "a training step fuses a last layer of at most 72 weights (k_s2_last_fused)"),
    (lambda f, k, ci, co, kh, kw, pos: f == "bwd" and pos == "last" and k == "s2_bwd2",
     "a last layer of at most 72 weights has its backward fused; more weights never take k_s2_bwd2"),
    (lambda f, k, ci, co, kh, kw, pos: k == "s2_fwd" and pos == "mid" and ci * co * kh * kw > 80 and co != 3,
     "small maps of a middle layer with more than 80 weights take k_s2_fwd_cs"),
]
UNREACHABLE = {b: reason for b in sorted(BRANCHES) for (rule, reason) in UNREACHABLE_RULES if rule(*b)}

# the GPU tests' geometries besides test_s2_shapes_gpu.py's: (output channels, height, width) of sizer-made models, batches
OTHER_GPU_GEOMETRIES = {
    "test_full_size_gpu cfg2": ([(1, 256, 256)], (36, 64, 160)),
}


def _plan(spec, batch, fc=16, latent=4, mode=1):
    p = EnginePlan(spec, fc, latent, max_batch=max(batch, 8))
    try:
        p.set_kernel_mode(mode)
        return {True: p.kernel_plan(batch, True), False: p.kernel_plan(batch, False)}
    finally:
        p.close()


def _sizer(out_c, out_h, out_w):
    return create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c).save()


def branches_of(spec, batch):
    """the BRANCHES keys a training step and an eval forward of this spec at this batch reach"""
    plans = _plan(spec, batch)
    dec = spec["output_layers"]
    out = set()
    for (i, l) in enumerate(dec):
        k = l["kernel_size"]
        (kh, kw) = (k, k) if isinstance(k, int) else tuple(k)
        (ci, co) = (l["input_dimensions"][0], l["output_dimensions"][0])
        if (ci, co) not in S2_PAIRS or l["stride"] != 2:
            continue
        pos = "last" if i == len(dec) - 1 else "mid"
        fam = lambda s: s.split("<")[0]
        out.add(("fwd", fam(plans[True][f"dec{i}"]["fwd"]), ci, co, kh, kw, pos))
        out.add(("bwd", fam(plans[True][f"dec{i}"]["bwd"]), ci, co, kh, kw, pos))
        out.add(("eval", fam(plans[False][f"dec{i}"]["fwd"]), ci, co, kh, kw, pos))
    return out


def _ig(ksplit, tpw, chunks, per, dgroup, wn8):
    """the fields of a k_ig_bwd_pair layer's report (ig_bwd_plan)"""
    return {"bwd": "ig_bwd_pair", "ig_ksplit": str(ksplit), "ig_tpw": str(tpw), "ig_chunks": str(chunks), "ig_per": str(per),
            "ig_dgroup": str(dgroup), "ig_wn8": str(wn8)}


def _ctb(kernel, imgs, groups, parts, bands, hb, sharded):
    """the fields of a k_ct_bwd_lds / k_ct_bwd_band layer's report (ct_bwd_plan)"""
    return {"bwd": "ct_bwd_lds", "ctb_kernel": kernel, "ctb_imgs": str(imgs), "ctb_groups": str(groups), "ctb_parts": str(parts),
            "ctb_bands": str(bands), "ctb_hb": str(hb), "ctb_sharded": str(sharded)}


CFG2_HEAD = {"fwd": "fused", "enc": "2", "grid": "4x36", "stage": "direct", "w4": "3712", "late": "0", "straddle": "3",
             "fc0": "0:9", "fc1": "3:4", "fc2": "0:8", "fc3": "4:2", "lds": "136112"}
CFG2_TRAIN = {
    "head": CFG2_HEAD,
    "dec0": {"fwd": "ct_fwd_lds<3,3>", **_ig(4, 1, 5, 32, 8, 1)},
    "dec1": {"fwd": "ct_fwd_lds<3,3>", **_ig(4, 1, 25, 32, 8, 4)},
    "dec2": {"fwd": "ct_fwd_lds<3,3>", **_ctb("band", 1, 64, 4, 4, 4, 1)},
    "dec3": {"fwd": "s2_fwd_rows<8,4,1,2>", "bwd": "s2_bwd_rows<8,2,4,3,3,4,2,1>"},
    "dec4": {"fwd": "s2_fwd_rows<4,2,2,1>", "bwd": "s2_bwd_rows<4,4,2,3,3,2,1,3>"},
    "dec5": {"fwd": "last_fused<2,1,4,4>", "hb": "4", "vec4": "1", "bn": "1", "bwd": "(fused)"},
    "tail": {"bwd": "fused", "rows": "4", "sums": "stored", "g1": "3:4", "g0": "0:8", "gx": "2:8", "w2": "0:4", "w1": "0:4", "w0": "0:4",
             "lds": "65984"},
    "enc": {"conv0": "adam", "inner": "pair"},
}
CFG2_EVAL = {
    "head": CFG2_HEAD,
    "dec0": {"fwd": "ct_fwd_lds<3,3>", "bwd": "-"},
    "dec1": {"fwd": "ct_fwd_lds<3,3>", "bwd": "-"},
    "dec2": {"fwd": "ct_fwd_lds<3,3>", "bwd": "-"},
    "dec3": {"fwd": "s2_fwd_rows<8,4,1,2>", "bwd": "-"},
    "dec4": {"fwd": "s2_fwd_rows<4,2,2,1>", "bwd": "-"},
    "dec5": {"fwd": "s2_fwd2<2,1,4,4,64>", "epi": "sigout", "bwd": "-"},
    "tail": {"bwd": "-"},
}


def test_benchmark_geometry_plan_is_pinned():
    """cfg2 (bench.py: 16x16 -> 256x256, fc 128, latent 32, batch 64): a change that moves it off these kernels fails here"""
    plans = _plan(_sizer(1, 256, 256), 64, fc=128, latent=32)
    assert plans[True] == CFG2_TRAIN
    assert plans[False] == CFG2_EVAL


def test_kernel_modes():
    spec = _sizer(1, 256, 256)
    generic = _plan(spec, 64, 128, 32, mode=0)
    assert generic[True]["head"]["fwd"] == "layers" and generic[True]["tail"]["bwd"] == "layers"
    for l in range(6):
        assert generic[True][f"dec{l}"] == {"fwd": "up", "bwd": "wgrad+down"}
        assert generic[False][f"dec{l}"] == {"fwd": "up", "bwd": "-"}
    every_ctb = _plan(spec, 64, 128, 32, mode=3)[True]   # bit 1: the LDS-staged backward wherever it fits
    gather = _plan(spec, 64, 128, 32, mode=5)[True]      # bit 2: the gather forward on the channel-rich layers
    # mode 3 at batch 64: 64->32 and 32->16 stage whole images (8 and 2 per workgroup, unsharded accumulators), 16->8 as by default
    ctb = (_ctb("lds", 8, 8, 8, 0, 0, 0), _ctb("lds", 2, 32, 4, 0, 0, 0), _ctb("band", 1, 64, 4, 4, 4, 1))
    for l in range(3):
        assert every_ctb[f"dec{l}"] == {"fwd": "ct_fwd_lds<3,3>", **ctb[l]}
        assert gather[f"dec{l}"] == {**CFG2_TRAIN[f"dec{l}"], "fwd": "ig_fwd_s2"}
    for name in ("head", "dec3", "dec4", "dec5", "tail"):
        assert every_ctb[name] == CFG2_TRAIN[name] and gather[name] == CFG2_TRAIN[name]


def test_plan_arguments_are_checked():
    p = EnginePlan(_sizer(1, 256, 256), 16, 4, max_batch=8)
    try:
        with pytest.raises(_lib.CaeError, match="outside"):
            p.kernel_plan(9, True)
        with pytest.raises(_lib.CaeError, match="outside"):
            p.kernel_plan(0, False)
        import ctypes as C
        from cae_tools_amd._lib import check
        with pytest.raises(_lib.CaeError, match="needs"):
            check(p.lib.cae_debug_plan(p.handle, 4, 1, C.create_string_buffer(16), 16))
    finally:
        p.close()


def _sweep():
    reached = {}
    for out_c in (1, 2, 3):
        for out_h in range(60, 301, 3):
            for out_w in sorted({out_h, out_h + 1, 63, 64, 100, 129, 255, 256}):
                if not 60 <= out_w <= 300:
                    continue
                try:
                    spec = _sizer(out_c, out_h, out_w)
                except Exception:   # the sizer finds no decoder for this size
                    continue
                for batch in (2, 32, 512):
                    for b in branches_of(spec, batch):
                        reached.setdefault(b, (out_c, out_h, out_w, batch))
    for batch in (4, 512):
        for b in branches_of(GoldenCase("handspec_b4").spec, batch):
            reached.setdefault(b, ("handspec_b4", batch))
    return reached


def test_sweep_reaches_every_branch_but_the_unreachable_ones():
    reached = _sweep()
    assert set(reached) <= BRANCHES, sorted(set(reached) - BRANCHES)
    wrongly_unreachable = {b: reached[b] for b in UNREACHABLE if b in reached}
    assert not wrongly_unreachable, wrongly_unreachable
    missing = BRANCHES - set(UNREACHABLE) - set(reached)
    assert not missing, sorted(missing)
    # every one of the 16 shapes runs somewhere, in training and in eval
    for (ci, co) in S2_PAIRS:
        for (kh, kw) in TAPS:
            assert any(b[2:6] == (ci, co, kh, kw) and b[0] == "bwd" for b in reached), (ci, co, kh, kw)


def test_gpu_geometries_reach_every_reachable_branch():
    from test_s2_shapes_gpu import CASES
    covered = set()
    for (g, batch, modes) in CASES:
        covered |= branches_of(_sizer(*g), batch)
    for name, (geoms, batches) in OTHER_GPU_GEOMETRIES.items():
        for g in geoms:
            for batch in batches:
                covered |= branches_of(_sizer(*g), batch)
    for name in MODEL_CASES:   # test_hip_parity.py's golden cases
        case = GoldenCase(name)
        covered |= branches_of(case.spec, case.meta["batch"])
    missing = BRANCHES - set(UNREACHABLE) - covered
    assert not missing, sorted(missing)


def test_gpu_geometries_reach_what_their_docstrings_name():
    from test_s2_shapes_gpu import BATCHES, GEOMETRIES, LARGE_BATCH
    described = [(g, text, BATCHES) for g, text in GEOMETRIES.items()] + [(g, text, (b,)) for g, (b, text) in LARGE_BATCH.items()]
    for (g, text, batches) in described:
        got = set()
        for batch in batches:
            got |= branches_of(_sizer(*g), batch)
        shapes = {(b[2], b[3], b[4], b[5], b[6]) for b in got}
        families = {b[1] for b in got}
        for part in text.split("; "):
            last = part.startswith("last ")
            words = part[5:].split() if last else part.split()
            (ci, co) = map(int, words[0].split("->"))
            (kh, kw) = map(int, words[1].split("x"))
            assert (ci, co, kh, kw, "last" if last else "mid") in shapes, (g, part, sorted(shapes))
            if "unfused" in part:
                assert ("fwd", "s2_fwd2", ci, co, kh, kw, "last") in got and ("fwd", "s2_fwd", ci, co, kh, kw, "last") in got, (g, part)
            elif "fused" in part:
                assert ("fwd", "last_fused", ci, co, kh, kw, "last") in got, (g, part)
            if part.split(" (")[0].endswith(" rows"):
                assert ("bwd", "s2_bwd_rows", ci, co, kh, kw, "mid") in got, (g, part)
        for fam in re.findall(r"k_s2_[a-z0-9_]+", text):
            assert fam[2:] in families, (g, fam, families)
    # the unfused multi-channel last layers run the S2_SIGMSE epilogue at both batch sizes' kernels (k_s2_fwd / k_s2_fwd2)
    assert ("fwd", "s2_fwd", 6, 3, 4, 4, "last") in branches_of(_sizer(3, 222, 222), 2)
    assert ("fwd", "s2_fwd2", 6, 3, 4, 4, "last") in branches_of(_sizer(3, 222, 222), 32)
