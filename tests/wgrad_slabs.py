"""What a decoder layer's backward launch stores as weight-gradient partials, worked out from the plan report and the layer's
geometry alone (the launch grids of engine_launch.h): shared by tests/test_wgrad_fold_gpu.py (sizer-made models) and
tests/test_hand_specs_cpu.py (hand-written layer definitions with output padding), which compare it with cae_debug_wgrad_slabs."""

ATOMICS = 8   # cae_set_kernel_mode bit 3
kCtbKChunk = 64   # kernels_ctbwd.h: positions per weight-gradient task
(kLastStripPx, kLastHB) = (127, 4)   # kernels_last.h / engine_choose.h: pixel columns of a strip, quad rows of a band
# the slab writers: (writer, slab element type).  k_s2_last_fused and the weight-gradient half of k_ig_bwd_pair were tried as
# writers and not kept; writer and expected_partials below still know their launches' partial counts
KEPT_WRITERS = {("ct_bwd_band", "f32"), ("ct_bwd_lds", "f32"), ("s2_bwd_rows", "f64")}


def expected_partials(layer, rep, batch):
    """workgroups (x chunks of positions) of the layer's backward launch, from the plan report and the layer's geometry"""
    (ci, h, w) = layer["input_dimensions"]
    (_, oh, ow) = layer["output_dimensions"]
    (qh, qw) = ((oh + 1) // 2, (ow + 1) // 2)
    if rep["bwd"] == "(fused)":            # k_s2_last_fused: four (image, strip, band of 4 quad rows) units per workgroup
        strips = -(-max(w, qw - 1) // kLastStripPx)
        return -(-batch * strips * -(-max(h, qh - 1) // kLastHB) // 4)
    if rep["bwd"].startswith("s2_bwd_rows<"):   # k_s2_bwd_rows<CIN, CT, COUT, 3, 3, HB, IMGS, D>: 4 / (CIN / CT) bands per workgroup
        (cin, ct, _, _, _, hb, imgs, _) = (int(v) for v in rep["bwd"][len("s2_bwd_rows<"):-1].split(","))
        bands = -(-max(h, qh - 1) // hb)
        return -(-batch // imgs) * -(-bands // (4 // (cin // ct)))
    if rep["bwd"] == "ig_bwd_pair":        # the weight-gradient half: one slab row per K chunk
        return int(rep["ig_chunks"])
    chunks = lambda positions: -(-positions // kCtbKChunk)
    (imgs, groups, bands, hb) = (int(rep[k]) for k in ("ctb_imgs", "ctb_groups", "ctb_bands", "ctb_hb"))
    if rep["ctb_kernel"] == "band":
        rows = [min(hb, h - z * hb) for z in range(bands)]          # grid z = band
        return groups * sum(chunks(r * w) for r in rows)
    return sum(chunks(min(imgs, batch - x * imgs) * h * w) for x in range(groups))   # grid x = image group


def writer(rep):
    if rep["bwd"] == "ct_bwd_lds":
        return ("ct_bwd_" + rep["ctb_kernel"], "f32")
    if rep["bwd"] == "(fused)":
        return ("s2_last_fused", "f64")
    if rep["bwd"].startswith("s2_bwd_rows<"):
        return ("s2_bwd_rows", "f64")
    if rep["bwd"] == "ig_bwd_pair":
        return ("ig_bwd_pair", "f32")
    return None
