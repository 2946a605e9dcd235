"""What the hand-written layer definitions of tests/hand_specs.py reach, checked without a GPU; tests/test_hand_specs_gpu.py
runs them.

- test_cases_reach_what_they_name: for every (spec, batch, kernel mode) the GPU file runs, the plan reports of a training step
  and of scoring (EnginePlan.kernel_plan) are what hand_specs.LAYERS lists, and together the cases reach WANT.  The plan report
  does not print ig_fwd_plan's K split and tiles per wave, nor the predicates that choose between div_small and the integer
  division in the kernels: _ig_fwd mirrors ig_fwd_plan (engine_choose.h) and the first lines of k_ig_fwd_s2, _fastdiv the
  kernels' `fastdiv` (kernels_igemm.h, kernels_generic.h).  k_ig_dgrad has no such arm: it divides in integers at every size.
- test_slab_report_covers_every_folded_parameter_once: the body of the test of that name in test_wgrad_fold_gpu.py on the
  three padded specs - with output padding the row kernels walk max(H, QH - 1) rows, and a slab sized otherwise is an
  out-of-bounds store.
- test_div_small_is_exact_on_its_declared_domain: tests/asan/div_small_check.cpp, compiled for the host with AddressSanitizer
  and run: every multiple boundary of every divisor below kDivSmallMaxD for n below kDivSmallMaxN."""
import os
import re
import subprocess

import pytest

import hand_specs as hs
from wgrad_slabs import ATOMICS, KEPT_WRITERS, expected_partials, writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(kDivSmallMaxN, kDivSmallMaxD) = (1 << 22, 8000)   # device_common.h (test_div_small_... compares them with the header)

CASES = [(name, batch, mode) for (name, (_, _, batches)) in hs.SPECS.items() for batch in batches for mode in hs.MODES[name]]


def _plans(spec, batch, mode):
    from cae_tools_amd.engine import EnginePlan
    p = EnginePlan(spec, hs.FC, hs.LATENT, max_batch=max(batch, 8))
    try:
        p.set_kernel_mode(mode)
        slabs = p.wgrad_slabs(batch) if mode else {}
        return p.kernel_plan(batch, True), p.kernel_plan(batch, False), slabs
    finally:
        p.close()


def _dims(layer):
    k = layer["kernel_size"]
    (kh, kw) = (k, k) if isinstance(k, int) else tuple(k)
    (ci, h, w) = layer["input_dimensions"]
    (co, oh, ow) = layer["output_dimensions"]
    return ci, h, w, co, oh, ow, kh, kw, layer["stride"], layer["output_padding"]


def _ig_fwd(ci, oh, ow, batch):
    """ig_fwd_plan and k_ig_fwd_s2's K slices: (ksplit, channels of each slice, tiles per wave, waves without a tile)"""
    (qh, qw) = ((oh + 1) // 2, (ow + 1) // 2)
    mtiles = (batch * qh * qw + 15) // 16
    ksplit = 4 if ci >= 48 else (2 if ci >= 24 else 1)
    (waves_m, target) = (4 // ksplit, 1024)
    tpw = min(max((mtiles * 4 + waves_m * target - 1) // (waves_m * target), 1), 8)
    grid_x = -(-mtiles // (waves_m * tpw))
    cper = ((ci + ksplit - 1) // ksplit + 7) & ~7
    slices = tuple(max(0, min(ci, (k + 1) * cper) - k * cper) for k in range(ksplit))
    return ksplit, slices, tpw, grid_x * waves_m * tpw - mtiles


def _fastdiv(n, d):
    return n < kDivSmallMaxN and d < kDivSmallMaxD


def _padding(h, w, oh, ow, kh, kw, op):
    """how output padding shows to a stride-2 kernel: 3 taps give OH = 2H + 2 (a bias-only last row), 4 taps OH = 2H + 3, so
    QH = H + 2 quad rows: one more than the H + 1 the kernels walk without padding"""
    if not op:
        return []
    out = ["op"]
    if kh == 3 or kw == 3:
        assert (kh != 3 or oh == 2 * h + 2) and (kw != 3 or ow == 2 * w + 2)
        out.append("op: bias-only row")
    if kh == 4 or kw == 4:
        assert (kh != 4 or (oh == 2 * h + 3 and (oh + 1) // 2 == h + 2)) and (kw != 4 or (ow + 1) // 2 == w + 2)
        out.append("op: QH = H + 2")
    return out


def _reached(name, batch, mode):
    spec = hs.spec_dict(name)
    dec = spec["output_layers"]
    (tr, ev, slabs) = _plans(spec, batch, mode)
    assert hs.observed(tr, ev) == hs.expected(name, mode), (name, batch, mode, hs.observed(tr, ev))
    if mode:
        assert (tr["head"]["fwd"], tr["tail"]["bwd"]) == ("fused", "fused"), (name, tr["head"], tr["tail"])
    reached = set()
    for (i, layer) in enumerate(dec):
        (ci, h, w, co, oh, ow, kh, kw, s, op) = _dims(layer)
        (fwd, bwd) = (tr[f"dec{i}"]["fwd"], tr[f"dec{i}"]["bwd"])
        pad = _padding(h, w, oh, ow, kh, kw, op) if s == 2 else (["op"] if op else [])
        if fwd == "ig_fwd_s2" and mode == 1:
            (ksplit, slices, tpw, idle) = _ig_fwd(ci, oh, ow, batch)
            (qh, qw) = ((oh + 1) // 2, (ow + 1) // 2)
            reached |= {("igf", "ksplit", ksplit), ("igf", "slices", slices), ("igf", "tpw", tpw), ("igf", "taps", kh, kw),
                        ("igf", "paired" if w >= 2 else "unpaired (W == 1)"), ("igf", "bn_in", i > 0),
                        ("igf", "div_small" if _fastdiv(batch * qh * qw + 16, qh * qw) else "integer division")}
            reached |= {("igf", p) for p in pad}
            if ev[f"dec{i}"]["fwd"] == "ig_fwd_s2":
                reached.add(("igf", "eval"))
            if idle and tpw > 1:
                reached.add(("igf", "tpw > 1 with idle last waves"))
            if w >= 2 and qw > w:     # quad columns 0 and >= W: the loaded pair is clamped into the row
                reached.add(("igf", "pair clamps at qn = 0 and qn >= W"))
            if w == 2:
                reached.add(("igf", "W == 2: one pair per row"))
            if co % 16:
                reached.add(("igf", "cout off the 16 grid", "one block" if co < 16 else "ragged second block"))
        fam = fwd.split("<")[0]
        for f in {fam, ev[f"dec{i}"]["fwd"].split("<")[0]}:   # scoring runs the last layer on the k_s2_fwd family
            if f in ("s2_fwd_rows", "s2_fwd_cs", "s2_fwd", "s2_fwd2", "last_fused"):
                reached |= {(f, p) for p in pad}
        if fam == "last_fused" and op:
            reached |= {("last_fused", "op", "vec4", int(tr[f"dec{i}"]["vec4"])),
                        ("last_fused", "op", "strips", -(-max(w, (ow + 1) // 2 - 1) // 127))}   # last_strips (engine_choose.h)
        if fam == "ct_fwd_lds":
            reached |= {("ct_fwd_lds", p, kh, kw) for p in pad}
            if co % 4:
                reached.add(("ct_fwd_lds", "cout % 4 != 0"))
        elif fam == "up" and mode == 1:
            arm = "four taps" if (kh <= 2 * s and kw <= 2 * s) else "general loop"
            reached.add(("up", arm, "stride", s, "kernel", kh))
            if kh < s:
                reached.add(("up", "kernel smaller than stride", "op" if op else "no op"))
        bfam = bwd.split("<")[0]
        if bwd == "ct_bwd_lds":
            kernel = "ct_bwd_" + tr[f"dec{i}"]["ctb_kernel"]
            reached |= {(kernel, p) for p in pad}
            reached.add((kernel, "bands", int(tr[f"dec{i}"]["ctb_bands"]), "mode", mode))
        elif bfam in ("s2_bwd_rows", "s2_bwd", "s2_bwd2", "s2_bwd_split"):
            reached |= {(bfam, p) for p in pad}
            if bfam == "s2_bwd_rows":
                reached.add(("s2_bwd_rows", "images per wave", int(bwd[:-1].split(",")[6])))
        elif bwd == "ig_bwd_pair":
            K = co * kh * kw
            reached |= {("igb", "ksplit", int(tr[f"dec{i}"]["ig_ksplit"]), "stride", s), ("igb", "taps", kh, kw),
                        ("ig_wgrad", "div_small" if _fastdiv(batch * h * w, h * w) else "integer division")}
            if K % 4:
                reached.add(("igb", "K % 4 != 0", "ksplit", int(tr[f"dec{i}"]["ig_ksplit"])))
            if h * w >= kDivSmallMaxD:
                reached.add(("ig_dgrad", "HW >= kDivSmallMaxD"))
        elif bwd == "wgrad+down":
            reached.add(("k_wgrad", "div_small" if _fastdiv(batch * h * w, h * w) else "integer division"))
        if f"dec{i}" in slabs:
            reached |= {("slab", slabs[f"dec{i}"]["writer"], p) for p in pad}
    if batch % 2:
        reached.add(("odd batch", name))
    return reached


WANT = {
    # k_ig_fwd_s2 in the default mode
    ("igf", "ksplit", 1), ("igf", "ksplit", 2), ("igf", "ksplit", 4),
    ("igf", "slices", (16, 16, 16, 2)), ("igf", "slices", (16, 10)), ("igf", "slices", (10,)),     # the ragged last K slice
    ("igf", "unpaired (W == 1)"), ("igf", "paired"), ("igf", "pair clamps at qn = 0 and qn >= W"), ("igf", "W == 2: one pair per row"),
    ("igf", "tpw", 1), ("igf", "tpw", 2), ("igf", "tpw > 1 with idle last waves"),
    ("igf", "cout off the 16 grid", "one block"), ("igf", "cout off the 16 grid", "ragged second block"),
    ("igf", "eval"), ("igf", "bn_in", False), ("igf", "bn_in", True),
    ("igf", "taps", 1, 1), ("igf", "taps", 2, 2), ("igf", "taps", 2, 3), ("igf", "taps", 3, 3), ("igf", "taps", 4, 4),
    ("igf", "op"), ("igf", "op: bias-only row"),
    # the integer-division arms
    ("igf", "div_small"), ("igf", "integer division"), ("ig_wgrad", "div_small"), ("ig_wgrad", "integer division"),
    ("ig_dgrad", "HW >= kDivSmallMaxD"), ("k_wgrad", "div_small"), ("k_wgrad", "integer division"),
    # k_ig_bwd_pair: one K slice, K no multiple of 4, taps other than 3 or 4, strides 1 and 3
    ("igb", "ksplit", 1, "stride", 2), ("igb", "ksplit", 2, "stride", 2), ("igb", "ksplit", 4, "stride", 2),
    ("igb", "ksplit", 1, "stride", 1), ("igb", "ksplit", 4, "stride", 3), ("igb", "ksplit", 1, "stride", 3),
    ("igb", "K % 4 != 0", "ksplit", 1), ("igb", "K % 4 != 0", "ksplit", 2),
    ("igb", "taps", 1, 1), ("igb", "taps", 2, 2), ("igb", "taps", 2, 3), ("igb", "taps", 6, 6), ("igb", "taps", 7, 7),
    # output padding on the specialised kernels
    ("ct_fwd_lds", "op: bias-only row", 3, 3), ("ct_fwd_lds", "op: QH = H + 2", 4, 4), ("ct_fwd_lds", "cout % 4 != 0"),
    ("s2_fwd_rows", "op: bias-only row"), ("s2_bwd_rows", "op: bias-only row"),
    ("s2_bwd_rows", "images per wave", 1), ("s2_bwd_rows", "images per wave", 2),
    ("s2_fwd_cs", "op: QH = H + 2"), ("s2_fwd_cs", "op: bias-only row"), ("s2_bwd", "op: QH = H + 2"),
    ("s2_bwd_split", "op: bias-only row"), ("s2_bwd2", "op: bias-only row"), ("s2_fwd", "op: QH = H + 2"), ("s2_fwd", "op: bias-only row"),
    ("last_fused", "op: QH = H + 2"), ("last_fused", "op: bias-only row"), ("last_fused", "op", "vec4", 0), ("last_fused", "op", "vec4", 1),
    ("last_fused", "op", "strips", 1), ("last_fused", "op", "strips", 2), ("s2_fwd2", "op: QH = H + 2"),
    ("ct_bwd_lds", "op: bias-only row"), ("ct_bwd_band", "op: bias-only row"),
    ("ct_bwd_band", "bands", 2, "mode", 1), ("ct_bwd_band", "bands", 6, "mode", 1), ("ct_bwd_band", "bands", 2, "mode", 3),
    ("slab", "s2_bwd_rows", "op"), ("slab", "ct_bwd_lds", "op"), ("slab", "ct_bwd_band", "op"),
    # k_up outside stride 2 and four taps
    ("up", "four taps", "stride", 1, "kernel", 2), ("up", "four taps", "stride", 3, "kernel", 6),
    ("up", "general loop", "stride", 1, "kernel", 3), ("up", "general loop", "stride", 2, "kernel", 7),
    ("up", "kernel smaller than stride", "op"),
} | {("odd batch", name) for name in hs.SPECS if name not in ("gather_wide", "wide_last")}


def test_cases_reach_what_they_name():
    reached = set()
    for (name, batch, mode) in CASES:
        reached |= _reached(name, batch, mode)
    assert WANT <= reached, sorted(map(str, WANT - reached))


def test_specs_are_what_the_module_says():
    """the dimensions the helpers compute are the table's, every output padding is below its stride, and the largest case
    stays small"""
    outs = {"padded_thin": (1, 49, 65), "padded_thin33": (1, 62, 46), "padded_rich": (1, 128, 161), "rich44_oddcout": (1, 32, 32),
            "gather_small": (1, 30, 21), "gather_k": (1, 81, 85), "gather_tpw": (1, 91, 91), "gather_wide": (1, 358, 362),
            "strides": (1, 149, 167), "first84": (1, 36, 44), "first42": (1, 19, 23), "first63": (1, 15, 19), "wide_last": (1, 451, 451)}
    assert {name: hs.out_shape(name) for name in hs.SPECS} == outs
    for name in hs.SPECS:
        spec = hs.spec_dict(name)
        assert spec["input_layers"][0]["output_dimensions"] == [4, 5, 5]
        for (a, b) in zip(spec["output_layers"], spec["output_layers"][1:]):
            assert a["output_dimensions"] == b["input_dimensions"]
        (_, _, batches) = hs.SPECS[name]
        assert max(batches) * max(l["output_dimensions"][0] * l["output_dimensions"][1] * l["output_dimensions"][2]
                                  for l in spec["output_layers"]) <= (450_000 if name != "wide_last" else 1_700_000)


def test_mode_5_puts_the_gather_forward_on_the_lds_staged_layers():
    """cae_set_kernel_mode bit 2 on the three geometries of test_ct_fwd_shapes_gpu.py at batch 3: every layer its LAYERS lists
    runs k_ig_fwd_s2, in a training step and in scoring - 3x3, 3x4, 4x3 and 4x4 taps, 12 to 128 input channels"""
    import test_ct_fwd_shapes_gpu as ctf
    from cae_tools_amd.engine import EnginePlan
    from cae_tools_amd.models.model_sizer import create_model_spec
    reached = set()
    for ((out_c, out_h, out_w), layers) in ctf.LAYERS.items():
        spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c).save()
        p = EnginePlan(spec, hs.FC, hs.LATENT, max_batch=8)
        try:
            p.set_kernel_mode(5)
            plans = (p.kernel_plan(3, True), p.kernel_plan(3, False))
        finally:
            p.close()
        for (i, ci, co, kh, kw, (h, w, oh, ow), *_rest) in layers:
            assert all(plan[f"dec{i}"]["fwd"] == "ig_fwd_s2" for plan in plans), (out_c, out_h, out_w, i)
            reached |= {("taps", kh, kw), ("cin", ci), ("ksplit", _ig_fwd(ci, oh, ow, 3)[0]), ("map", h, w) if h * w == 1 else ("map",)}
    assert {("taps", 3, 3), ("taps", 3, 4), ("taps", 4, 3), ("taps", 4, 4), ("cin", 12), ("cin", 128), ("cin", 96), ("map", 1, 1),
            ("ksplit", 1), ("ksplit", 2), ("ksplit", 4)} <= reached, reached


_SLAB_CASES = [(name, batch, mode) for name in hs.PADDED for batch in (2, 3, 8) for mode in (1, 3)]


@pytest.mark.parametrize("name,batch,mode", _SLAB_CASES)
def test_slab_report_covers_every_folded_parameter_once(name, batch, mode):
    from cae_tools_amd.engine import EnginePlan
    spec = hs.spec_dict(name)
    dec = spec["output_layers"]
    p = EnginePlan(spec, hs.FC, hs.LATENT, max_batch=8)
    try:
        tensors = p.tensors
        p.set_kernel_mode(mode)
        (plan, slabs) = (p.kernel_plan(batch, True), p.wgrad_slabs(batch))
        p.set_kernel_mode(mode | ATOMICS)
        assert p.kernel_plan(batch, True) == plan   # bit 3 moves no kernel choice
        off = p.wgrad_slabs(batch)
    finally:
        p.close()
    assert off == {"fold": {"slabs": "0", "wgs": "0", "bytes": "0", "capacity": slabs["fold"]["capacity"]}}
    writers = {n: rep for (n, rep) in plan.items() if n.startswith("dec") and writer(rep) in KEPT_WRITERS}
    fold = slabs.pop("fold")
    assert set(slabs) == set(writers) and 2 <= len(slabs) <= 6, (slabs, writers)
    (end, wgs, covered) = (0, 0, [])
    for n in sorted(slabs, reverse=True):   # launch order: last decoder layer first
        (s, l) = (slabs[n], int(n[3:]))
        (_, off_w, numel, _) = tensors[f"dec/decoder_conv.{3 * l}.weight"]
        assert (s["writer"], s["type"]) == writer(writers[n]), (n, s)
        assert (int(s["param"]), int(s["values"])) == (off_w, numel), (n, s)
        assert int(s["partials"]) == expected_partials(dec[l], writers[n], batch), (n, s)
        vals = int(s["fold_values"])
        assert vals in (8, 16, 32, 64, 128, 256) and (vals == 8 or (256 // vals) * 16 >= int(s["partials"])), (n, s)
        assert int(s["offset"]) >= end and int(s["offset"]) % 256 == 0 and int(s["fold_wgs"]) == -(-numel // vals), (n, s)
        end = int(s["offset"]) + int(s["partials"]) * numel * (8 if s["type"] == "f64" else 4)
        wgs += int(s["fold_wgs"])
        covered.append((off_w, off_w + numel))
    # slabs neither overlap in the region nor in the parameters, and the region holds them
    assert all(a[1] <= b[0] for (a, b) in zip(sorted(covered), sorted(covered)[1:]))
    assert (int(fold["slabs"]), int(fold["wgs"]), int(fold["bytes"])) == (len(slabs), wgs, end)
    assert end <= int(fold["capacity"])


def test_div_small_is_exact_on_its_declared_domain(tmp_path):
    from cae_tools_amd import build
    # the program's copy of the expression and of the two limits is the header's
    header = open(os.path.join(ROOT, "cae_tools_amd", "csrc", "device_common.h")).read()
    source = open(os.path.join(ROOT, "tests", "asan", "div_small_check.cpp")).read()
    expr = re.search(r"int div_small\(int n, float inv_d\) \{[^}]*\}", header).group(0)
    limits = re.search(r"constexpr int kDivSmallMaxN = [^;]*;", header).group(0)
    assert expr in source and limits in source, (expr, limits)
    assert limits == "constexpr int kDivSmallMaxN = 1 << 22, kDivSmallMaxD = 8000;" and (kDivSmallMaxN, kDivSmallMaxD) == (1 << 22, 8000)
    clang = os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "div_small_check")
    subprocess.run([clang, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address",
                    os.path.join(ROOT, "tests", "asan", "div_small_check.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    text = out.stdout.decode(errors="replace")
    print(text)
    assert out.returncode == 0 and "div_small exact on its declared domain" in text and "ERROR: AddressSanitizer" not in text, text[-3000:]
    # about 8e7 quotients, and the first wrong one beyond either limit (a later change of a limit meets these lines)
    assert int(re.search(r"checked (\d+) quotients", text).group(1)) > 7e7
    assert "first wrong beyond n: n=4201469 d=4095" in text and "first wrong beyond d: none below 32000" in text, text
