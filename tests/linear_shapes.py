"""The Linear engine geometries of tests/test_linear_shapes_gpu.py, with the launch plan of every (case, batch) pinned as
literals (LinearPlan.kernel_plan, lin_debug_plan in include/cae_linear.h).  tests/test_linear_plan_cpu.py checks the literals
without a GPU; the GPU tests assert them again on the engine they run, before anything runs.

The plans follow igemm_tile / gemm_slices (csrc/kernels_unet_mfma.h): rows = nout picks the tile (<= 32: 32x512, <= 64: 64x256,
else 128x128); the forward's K = nin is cut into 16-wide chunks and split over blockIdx.z when there are >= 64 chunks and
fewer than 256 tiles, `per` chunks a slice; the weight gradient (rows nout, columns nin, K = batch) is never split."""

# id -> (in_shape, out_shape, batches)
CASES = {
    "r32_split": ((1, 33, 33), (1, 5, 6), (3, 520)),
    "r64_split": ((3, 19, 19), (2, 7, 4), (5, 257)),
    "r128_ragged": ((1, 33, 33), (1, 13, 11), (2, 129)),
    "edge_1008": ((1, 24, 42), (1, 11, 35), (4,)),
    "edge_1009": ((1, 1, 1009), (1, 11, 35), (4,)),
    "tiny_k1": ((1, 1, 1), (1, 1, 1), (1, 2)),
    "tiny_k3": ((1, 1, 3), (1, 1, 1), (1, 2)),
    "wide_nosplit": ((1, 16, 16), (1, 64, 64), (7,)),
}
SPLIT_CASES = ("r32_split", "r64_split", "r128_ragged", "edge_1009")


def _fwd(tile, grid, slices, per, part_bytes):
    return {"tile": tile, "grid": grid, "slices": str(slices), "per": str(per), "part_bytes": str(part_bytes)}


def _wgrad(tile, grid):
    return {"tile": tile, "grid": grid, "slices": "1"}


# (id, batch) -> the training step's plan on an engine whose max_batch is the case's largest batch
PLANS = {
    # nin 1089 = 69 chunks: 5 slices of 16, the last of 5 chunks whose last holds 1 element; one row tile with NWQ = 1
    ("r32_split", 3): {"fwd": _fwd("32x512", "1x1", 5, 16, 1800), "wgrad": _wgrad("32x512", "3x1"), "room": {"gpart_bytes": "312000"}},
    ("r32_split", 520): {"fwd": _fwd("32x512", "2x1", 5, 16, 312000), "wgrad": _wgrad("32x512", "3x1"),
                         "room": {"gpart_bytes": "312000"}},
    # nin 1083 = 68 chunks (1083 = 3 mod 4): 5 slices, the last of 4 chunks
    ("r64_split", 5): {"fwd": _fwd("64x256", "1x1", 5, 16, 5600), "wgrad": _wgrad("64x256", "5x1"), "room": {"gpart_bytes": "287840"}},
    ("r64_split", 257): {"fwd": _fwd("64x256", "2x1", 5, 16, 287840), "wgrad": _wgrad("64x256", "5x1"),
                         "room": {"gpart_bytes": "287840"}},
    # nout 143 = 128 + 15: two row tiles
    ("r128_ragged", 2): {"fwd": _fwd("128x128", "1x2", 5, 16, 5720), "wgrad": _wgrad("128x128", "9x2"),
                         "room": {"gpart_bytes": "368940"}},
    ("r128_ragged", 129): {"fwd": _fwd("128x128", "2x2", 5, 16, 368940), "wgrad": _wgrad("128x128", "9x2"),
                           "room": {"gpart_bytes": "368940"}},
    # 63 chunks: the last K that is not split; 64 chunks: the first that is (4 slices, the last chunk holds 1 element)
    ("edge_1008", 4): {"fwd": _fwd("128x128", "1x4", 1, 63, 0), "wgrad": _wgrad("128x128", "8x4"), "room": {"gpart_bytes": "0"}},
    ("edge_1009", 4): {"fwd": _fwd("128x128", "1x4", 4, 16, 24640), "wgrad": _wgrad("128x128", "8x4"), "room": {"gpart_bytes": "24640"}},
    ("tiny_k1", 1): {"fwd": _fwd("32x512", "1x1", 1, 1, 0), "wgrad": _wgrad("32x512", "1x1"), "room": {"gpart_bytes": "0"}},
    ("tiny_k1", 2): {"fwd": _fwd("32x512", "1x1", 1, 1, 0), "wgrad": _wgrad("32x512", "1x1"), "room": {"gpart_bytes": "0"}},
    ("tiny_k3", 1): {"fwd": _fwd("32x512", "1x1", 1, 1, 0), "wgrad": _wgrad("32x512", "1x1"), "room": {"gpart_bytes": "0"}},
    ("tiny_k3", 2): {"fwd": _fwd("32x512", "1x1", 1, 1, 0), "wgrad": _wgrad("32x512", "1x1"), "room": {"gpart_bytes": "0"}},
    ("wide_nosplit", 7): {"fwd": _fwd("128x128", "1x32", 1, 16, 0), "wgrad": _wgrad("128x128", "2x32"), "room": {"gpart_bytes": "0"}},
}
