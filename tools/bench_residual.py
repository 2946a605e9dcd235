"""Time the three residual-target kernels, every mode, beside the two-pass alternative they replace.

    python tools/bench_residual.py [--cases 2000] [--in-size 16] [--size 256] [--calls 20]

fp32 low-resolution input, fp32 target and scores.  The fused kernels form the interpolated field b in registers:
cae_residual_scan reads the target, cae_residual_pack_rows reads it and writes fp32 rows, cae_residual_restore_f64 reads
fp32 scores and writes fp64.  Without them the field has to be stored first - cae_case_baseline with field_dev, 8 bytes
written per pixel - and read again by a second pass; the launches timed for that alternative are the ones that exist today,
cae_case_baseline(field) followed by cae_normalise_pack_rows (pack) or cae_denormalise_f64 (restore), neither of which reads
the field yet: a lower bound of what a two-pass path would take.  The scan is set beside the field pass alone.
Device events, warm-up, then `--calls` calls of each entry point, alternating, and their mean; the whole measurement twice,
so that the two passes can be compared.  One JSON line per pass and mode."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402
from cae_tools_amd.utils import baseline  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--in-size", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_residual: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, hi, h) = (args.cases, args.in_size, args.size)
    (plane_in, plane) = (hi * hi, h * h)
    gen = torch.Generator(device=dev).manual_seed(1)
    low = 290 + 5 * torch.rand((n, plane_in), device=dev, generator=gen, dtype=torch.float32)
    target = 290 + 5 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    scores = torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    rows = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
    packed = torch.empty((n, plane), dtype=torch.float32, device=dev)
    out64 = torch.empty((n, plane), dtype=torch.float64, device=dev)
    field = torch.empty((n, plane), dtype=torch.float64, device=dev)
    sums = torch.empty((n, 6), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32
    (rmin, span) = (-5.0, 10.0)

    scan_need = int(lib.cae_residual_scan_workspace_bytes(n, h, h))
    scan_ws = torch.empty(max(scan_need, 8), dtype=torch.uint8, device=dev)
    base_need = int(lib.cae_case_baseline_workspace_bytes(n, h, h))
    base_ws = torch.empty(max(base_need, 8), dtype=torch.uint8, device=dev)
    out3 = (C.c_double * 3)()

    def scan(mode):
        _lib.check(lib.cae_residual_scan(low.data_ptr(), F32, plane_in, hi, hi, target.data_ptr(), n, h, h, mode, scan_ws.data_ptr(),
                                         scan_need, stream, out3))

    def pack(mode):
        _lib.check(lib.cae_residual_pack_rows(low.data_ptr(), F32, plane_in, hi, hi, target.data_ptr(), n, h, h, mode, rmin, span, 1,
                                              rows.data_ptr(), packed.data_ptr(), stream))

    def restore(mode):
        _lib.check(lib.cae_residual_restore_f64(low.data_ptr(), F32, plane_in, hi, hi, scores.data_ptr(), n, h, h, mode, rmin, span,
                                                1, out64.data_ptr(), stream))

    def field_pass(mode):
        _lib.check(lib.cae_case_baseline(low.data_ptr(), F32, plane_in, hi, hi, None, 0, 0, target.data_ptr(), F32, plane, n, h, h,
                                         mode, sums.data_ptr(), field.data_ptr(), base_ws.data_ptr(), base_need, stream))

    def normalise_pack(mode):
        _lib.check(lib.cae_normalise_pack_rows(target.data_ptr(), n, 1, plane, packed.data_ptr(), 1, 0, C.c_float(rmin),
                                               C.c_float(span), 1, rows.data_ptr(), stream))

    def denormalise(mode):
        _lib.check(lib.cae_denormalise_f64(scores.data_ptr(), n * plane, rmin, span, out64.data_ptr(), stream))

    runs = [("scan", scan), ("pack", pack), ("restore", restore), ("field", field_pass), ("normalise_pack", normalise_pack),
            ("denormalise", denormalise)]
    for k in range(args.passes):
        for (name, mode) in baseline.MODES.items():
            for _ in range(args.warmup):
                for (_, fn) in runs:
                    fn(mode)
            torch.cuda.synchronize()
            ms = {key: 0.0 for (key, _) in runs}
            for _ in range(args.calls):
                for (key, fn) in runs:
                    (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    t0.record()
                    fn(mode)
                    t1.record()
                    t1.synchronize()
                    ms[key] += t0.elapsed_time(t1) / args.calls
            line = {"pass": k, "mode": name, "operands": "fp32 input, fp32 target and scores", "cases": n, "in": [hi, hi],
                    "out": [h, h]}
            line.update({f"{key}_ms": round(value, 4) for (key, value) in ms.items()})
            pixels = float(n) * plane
            line["scan_TBps"] = round(pixels * 4 / ms["scan"] / 1e9, 3)                 # bytes read
            line["pack_TBps"] = round(pixels * 8 / ms["pack"] / 1e9, 3)                 # 4 read, 4 written
            line["restore_TBps"] = round(pixels * 12 / ms["restore"] / 1e9, 3)          # 4 read, 8 written
            line["scan_over_field"] = round(ms["scan"] / ms["field"], 3)
            line["pack_over_two_pass"] = round(ms["pack"] / (ms["field"] + ms["normalise_pack"]), 3)
            line["restore_over_two_pass"] = round(ms["restore"] / (ms["field"] + ms["denormalise"]), 3)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
