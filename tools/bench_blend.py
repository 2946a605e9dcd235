"""Time the two kernels of the model blending beside what they stand next to ("Model blending").

    python tools/bench_blend.py [--cases 2000] [--size 256] [--calls 10]

cae_case_error_moments on resident fp64 operands (M predictions and the target, 8 (M + 1) bytes read per pixel) for M = 2, 4
and 8, beside cae_case_compare on the same operands in the same run: the same loads, M + M (M + 1) / 2 tree sums a tile
against 3 M.  cae_blend_predictions for M = 2, 4 and 8 (8 M bytes read and 8 written per element) beside cae_denormalise_f64 on
as many elements (4 read, 8 written).  Device events, warm-up, then `--calls` calls of each, alternating, and their mean; the
whole measurement twice, so that the two passes can be compared.  One JSON line per pass."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cae_tools_amd import _lib  # noqa: E402


def timed(runs, calls, warmup):
    """{name: mean ms} of the functions of `runs`, called alternately"""
    for _ in range(warmup):
        for (_, fn) in runs:
            fn()
    torch.cuda.synchronize()
    ms = {key: 0.0 for (key, _) in runs}
    for _ in range(calls):
        for (key, fn) in runs:
            (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[key] += t0.elapsed_time(t1) / calls
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_blend: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, h) = (args.cases, args.size)
    plane = h * h
    gen = torch.Generator(device=dev).manual_seed(1)
    a64 = 288 + 10 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float64)
    preds = [a64 + (0.5 + 0.1 * k) * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float64) for k in range(8)]
    y32 = torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F64 = _lib.ELEM_F64
    ws = torch.empty(max(int(lib.cae_case_error_moments_workspace_bytes(n, plane, 8)), int(lib.cae_case_compare_workspace_bytes(n, plane, 8)), 16),
                     dtype=torch.uint8, device=dev)
    sums = torch.empty((n, 45), dtype=torch.float64, device=dev)
    out = torch.empty((n, plane), dtype=torch.float64, device=dev)

    def lists(m):
        return (C.c_void_p * m)(*[p.data_ptr() for p in preds[:m]]), (C.c_int64 * m)(*[plane] * m)

    def run_moments(m):
        (ptrs, strides) = lists(m)
        need = int(lib.cae_case_error_moments_workspace_bytes(n, plane, m))

        def run():
            _lib.check(lib.cae_case_error_moments(ptrs, F64, strides, m, a64.data_ptr(), F64, plane, n, plane, sums.data_ptr(), ws.data_ptr(),
                                                  need, stream))
        return run

    def run_compare(m):
        (ptrs, strides) = lists(m)
        need = int(lib.cae_case_compare_workspace_bytes(n, plane, m))

        def run():
            _lib.check(lib.cae_case_compare(ptrs, F64, strides, m, a64.data_ptr(), F64, plane, n, plane, sums.data_ptr(), ws.data_ptr(), need,
                                            stream))
        return run

    def run_blend(m):
        (ptrs, strides) = lists(m)
        weights = (C.c_double * m)(*[(k + 1.0) / (m * (m + 1) / 2) for k in range(m)])

        def run():
            _lib.check(lib.cae_blend_predictions(ptrs, F64, strides, m, weights, 0.25, n, plane, out.data_ptr(), plane, stream))
        return run

    def run_denormalise():
        _lib.check(lib.cae_denormalise_f64(y32.data_ptr(), n * plane, 288.0, 10.0, out.data_ptr(), stream))

    runs = [(f"moments_{m}", run_moments(m)) for m in (2, 4, 8)] + [(f"compare_{m}", run_compare(m)) for m in (2, 4, 8)]
    runs += [(f"blend_{m}", run_blend(m)) for m in (2, 4, 8)] + [("denormalise", run_denormalise)]
    for k in range(args.passes):
        ms = timed(runs, args.calls, args.warmup)
        line = {"pass": k, "operands": "fp64 predictions and target", "cases": n, "plane": [h, h]}
        for (key, _) in runs:
            line[f"{key}_ms"] = round(ms[key], 4)
        for m in (2, 4, 8):
            line[f"moments_{m}_TBps_of_{8 * (m + 1)}_bytes"] = round(float(n) * plane * 8 * (m + 1) / ms[f"moments_{m}"] / 1e9, 3)
            line[f"moments_{m}_over_compare_{m}"] = round(ms[f"moments_{m}"] / ms[f"compare_{m}"], 3)
            line[f"tree_sums_{m}_over_compare"] = round((m + m * (m + 1) / 2) / (3.0 * m), 3)
            line[f"blend_{m}_TBps_of_{8 * (m + 1)}_bytes"] = round(float(n) * plane * 8 * (m + 1) / ms[f"blend_{m}"] / 1e9, 3)
            line[f"blend_{m}_over_denormalise"] = round(ms[f"blend_{m}"] / ms["denormalise"], 3)
        line["denormalise_TBps_of_12_bytes"] = round(float(n) * plane * 12 / ms["denormalise"] / 1e9, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
