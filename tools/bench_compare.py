"""Time the two kernels of the model comparison beside what they stand next to.

    python tools/bench_compare.py [--cases 2000] [--size 256] [--calls 10] [--numpy-resamples 256]

cae_case_compare on resident fp64 operands (M predictions and the target, 8 (M + 1) bytes read per pixel) for M = 2, 4 and 8,
beside M calls of cae_case_measures on the same operands (16 M bytes per pixel) and one cae_case_importance (fp32 scores, fp64
target: 16 bytes per pixel).  Device events, warm-up, then `--calls` calls of each, alternating, and their mean; the whole
measurement twice, so that the two passes can be compared.  One JSON line per pass.

cae_bootstrap_sums at (2000 units, 9 columns, 10^4 resamples) and (20000, 25, 10^5), each beside the numpy restatement of
tests/compare_ref.py on --numpy-resamples resamples, scaled to the kernel's number: the same sums in the same order.  One
JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cae_tools_amd import _lib  # noqa: E402

import ctypes as C  # noqa: E402


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


def compare(args, lib, dev):
    (n, h) = (args.cases, args.size)
    plane = h * h
    gen = torch.Generator(device=dev).manual_seed(1)
    a64 = 288 + 10 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float64)
    preds = [a64 + (0.5 + 0.1 * k) * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float64) for k in range(8)]
    base = torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    pert = (base + 0.1 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)).clamp_(0, 1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F64 = _lib.ELEM_F64
    need = int(lib.cae_case_compare_workspace_bytes(n, plane, 8))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    sums = torch.empty((n, 34), dtype=torch.float64, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    im_need = int(lib.cae_case_importance_workspace_bytes(n, plane))
    im_ws = torch.empty(max(im_need, 16), dtype=torch.uint8, device=dev)
    im_sums = torch.empty((n, 8), dtype=torch.float64, device=dev)

    def run_compare(m):
        ptrs = (C.c_void_p * m)(*[p.data_ptr() for p in preds[:m]])
        strides = (C.c_int64 * m)(*[plane] * m)
        bytes_ = int(lib.cae_case_compare_workspace_bytes(n, plane, m))

        def run():
            _lib.check(lib.cae_case_compare(ptrs, F64, strides, m, a64.data_ptr(), F64, plane, n, plane, sums.data_ptr(), ws.data_ptr(),
                                            bytes_, stream))
        return run

    def run_measures(m):
        def run():
            for p in preds[:m]:
                _lib.check(lib.cae_case_measures(p.data_ptr(), F64, plane, a64.data_ptr(), F64, plane, n, plane, measures.data_ptr(),
                                                 cm_ws.data_ptr(), cm_need, stream))
        return run

    def run_importance():
        _lib.check(lib.cae_case_importance(base.data_ptr(), plane, pert.data_ptr(), plane, a64.data_ptr(), F64, plane, n, plane, 288.0, 10.0,
                                           im_sums.data_ptr(), None, im_ws.data_ptr(), im_need, stream))

    runs = [(f"compare_{m}", run_compare(m)) for m in (2, 4, 8)] + [(f"measures_x{m}", run_measures(m)) for m in (2, 4, 8)]
    runs.append(("importance", run_importance))
    for k in range(args.passes):
        ms = timed(runs, args.calls, args.warmup)
        line = {"pass": k, "operands": "fp64 predictions and target", "cases": n, "plane": [h, h]}
        for (key, _) in runs:
            line[f"{key}_ms"] = round(ms[key], 4)
        for m in (2, 4, 8):
            line[f"compare_{m}_TBps_of_{8 * (m + 1)}_bytes"] = round(float(n) * plane * 8 * (m + 1) / ms[f"compare_{m}"] / 1e9, 3)
            line[f"measures_x{m}_over_compare_{m}"] = round(ms[f"measures_x{m}"] / ms[f"compare_{m}"], 2)
        line["importance_TBps_of_16_bytes"] = round(float(n) * plane * 16 / ms["importance"] / 1e9, 3)
        print(json.dumps(line), flush=True)


def bootstrap(args, lib, dev):
    import compare_ref
    stream = torch.cuda.current_stream(dev).cuda_stream
    for (n_unit, n_col, b) in ((2000, 9, 10 ** 4), (20000, 25, 10 ** 5)):
        table = np.random.default_rng(n_unit).gamma(2.0, 1.0, (n_unit, n_col))
        t = torch.from_numpy(table).to(dev)
        out = torch.empty((b, n_col), dtype=torch.float64, device=dev)

        def run():
            _lib.check(lib.cae_bootstrap_sums(t.data_ptr(), n_unit, n_col, 0, b, 7, out.data_ptr(), stream))

        ms = timed([("bootstrap", run)], args.calls, args.warmup)["bootstrap"]
        few = min(args.numpy_resamples, b)
        t0 = time.perf_counter()
        want = compare_ref.sums(table, few, seed=7)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(out[:few].cpu().numpy(), want))
        print(json.dumps({"units": n_unit, "columns": n_col, "resamples": b, "table_KiB": round(table.nbytes / 1024, 1),
                          "bootstrap_ms": round(ms, 4), "draws_per_ns": round(float(n_unit) * b / ms / 1e6, 3),
                          "numpy_resamples": few, "numpy_ms": round(numpy_ms, 2), "numpy_ms_scaled": round(numpy_ms * b / few, 1),
                          "numpy_over_kernel": round(numpy_ms * b / few / ms, 1), "same_bits": same}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--numpy-resamples", type=int, default=256)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    compare(args, lib, dev)
    bootstrap(args, lib, dev)


if __name__ == "__main__":
    main()
