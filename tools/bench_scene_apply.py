"""Time cae_scene_blend and cae_scene_gather beside cae_denormalise_f64 over the same number of prediction elements: the
closing pass the per-box apply() already pays on the same data.

    python tools/bench_scene_apply.py [--time-steps 32] [--scene 64] [--box 16] [--out-box 256] [--overlap 4] [--calls 50]

The default is the scene of DESIGN.md §9: 16 x 16 -> 256 x 256 boxes at overlap 4 over a 64 x 64 scene, a 1024 x 1024 output per time
step (25 tiles), `--time-steps` of them in one call so that a call is long enough to time.  Bytes are what the algorithm
needs, from the shapes: the blend reads every fp32 prediction once and writes every float64 pixel once, the gather reads and
writes every fp32 box element once, the denormalisation reads 4 and writes 8 bytes per prediction element.  Device events,
warm-up, then `--calls` calls of each entry point, alternating, and their mean; the whole measurement twice, so that the two
passes can be compared.  One JSON line per pass."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402
from cae_tools_amd.engine import scene_plan  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--time-steps", type=int, default=32)
    ap.add_argument("--scene", type=int, default=64)
    ap.add_argument("--box", type=int, default=16)
    ap.add_argument("--out-box", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_apply: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    plan = scene_plan(args.scene, args.scene, ((args.box, args.box), (args.out_box, args.out_box)), args.overlap)
    T = args.time_steps
    n_tile = T * plan.n_tile
    (Ys, Xs) = plan.out_shape
    gen = torch.Generator(device=dev).manual_seed(1)
    scene = 280 + 10 * torch.rand((T, 1, plan.Y, plan.X), device=dev, generator=gen, dtype=torch.float32)
    pred = torch.rand((n_tile, 1, plan.H, plan.W), device=dev, generator=gen, dtype=torch.float32)
    boxes = torch.empty((n_tile, 1, plan.h, plan.w), dtype=torch.float32, device=dev)
    invalid = torch.zeros(n_tile, dtype=torch.int32, device=dev)
    out = torch.empty((T, 1, Ys, Xs), dtype=torch.float64, device=dev)
    holes = torch.zeros(T, dtype=torch.int64, device=dev)
    den = torch.empty(pred.shape, dtype=torch.float64, device=dev)
    geom = plan.geom()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run_gather():
        _lib.check(lib.cae_scene_gather(C.byref(geom), scene.data_ptr(), _lib.ELEM_F32, T, 1, 0, T, 0, plan.n_y, boxes.data_ptr(), 1, 0,
                                        C.c_float(280.0), C.c_float(10.0), 1, invalid.data_ptr(), stream))

    def run_blend():
        _lib.check(lib.cae_scene_blend(C.byref(geom), pred.data_ptr(), invalid.data_ptr(), 0, plan.n_y, None, None, 0, 0, T, 1, 0, Ys,
                                       270.5, 39.75, out.data_ptr(), Ys * Xs, holes.data_ptr(), stream))

    def run_denorm():
        _lib.check(lib.cae_denormalise_f64(pred.data_ptr(), pred.numel(), 270.5, 39.75, den.data_ptr(), stream))

    bytes_of = {"gather": 8.0 * boxes.numel(), "blend": 4.0 * pred.numel() + 8.0 * out.numel(), "denormalise": 12.0 * pred.numel()}
    runs = [("gather", run_gather), ("blend", run_blend), ("denormalise", run_denorm)]
    for k in range(args.passes):
        for _ in range(args.warmup):
            for (_, fn) in runs:
                fn()
        torch.cuda.synchronize()
        ms = {key: 0.0 for (key, _) in runs}
        for _ in range(args.calls):
            for (key, fn) in runs:
                (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[key] += t0.elapsed_time(t1) / args.calls
        line = {"pass": k, "time_steps": T, "scene": [plan.Y, plan.X], "box": [plan.h, plan.w], "out_box": [plan.H, plan.W],
                "overlap": [plan.oy, plan.ox], "tiles_per_step": plan.n_tile, "output": [Ys, Xs],
                "prediction_elements": pred.numel(), "output_pixels": out.numel()}
        for (key, _) in runs:
            line[f"{key}_ms"] = round(ms[key], 4)
            line[f"{key}_MB"] = round(bytes_of[key] / 1e6, 2)
            line[f"{key}_TBps"] = round(bytes_of[key] / ms[key] / 1e9, 3)
        line["blend_over_denormalise"] = round(ms["blend"] / ms["denormalise"], 2)
        line["blend_per_byte_over_denormalise"] = round((ms["blend"] / bytes_of["blend"]) / (ms["denormalise"] / bytes_of["denormalise"]), 2)
        assert int(holes.sum()) == 0 and int(invalid.sum()) == 0
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
