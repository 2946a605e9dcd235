"""Time cae_case_baseline, every mode, beside cae_case_measures on the same resident prediction and target.

    python tools/bench_case_baseline.py [--cases 2000] [--in-size 16] [--size 256] [--calls 20]

fp32 low-resolution input, fp32 prediction against fp32 target.  cae_case_baseline reads the operand bytes
cae_case_measures reads plus the low-resolution planes (in-size^2 / size^2 of them) and writes no field, so both are given
as the bandwidth they reach over prediction and target, and cae_case_baseline also as its ratio to cae_case_measures in the
same pass.  Device events, warm-up, then `--calls` calls of each entry point, alternating, and their mean; the whole
measurement twice, so that the two passes can be compared.  One JSON line per pass."""
import argparse
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
        raise SystemExit("bench_case_baseline: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, hi, h) = (args.cases, args.in_size, args.size)
    (plane_in, plane) = (hi * hi, h * h)
    gen = torch.Generator(device=dev).manual_seed(1)
    a32 = 290 + 5 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    p32 = a32 + 0.5 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)
    low = 290 + 5 * torch.rand((n, plane_in), device=dev, generator=gen, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32

    sums = torch.empty((n, 6), dtype=torch.float64, device=dev)
    need = int(lib.cae_case_baseline_workspace_bytes(n, h, h))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)

    def run_baseline(mode):
        def run():
            _lib.check(lib.cae_case_baseline(low.data_ptr(), F32, plane_in, hi, hi, p32.data_ptr(), F32, plane, a32.data_ptr(),
                                             F32, plane, n, h, h, mode, sums.data_ptr(), None, ws.data_ptr(), need, stream))
        return run

    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)

    def run_measures():
        _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                         measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

    runs = [(name, run_baseline(mode)) for (name, mode) in baseline.MODES.items()] + [("case_measures", run_measures)]
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
        line = {"pass": k, "operands": "fp32 input, fp32 prediction, fp32 target", "cases": n, "in": [hi, hi], "out": [h, h],
                "workspace_MB": round(need / 1e6, 3),
                "case_measures_ms": round(ms["case_measures"], 4),
                "case_measures_TBps": round(float(n) * plane * 8 / ms["case_measures"] / 1e9, 3)}
        for name in baseline.MODES:
            line[f"{name}_ms"] = round(ms[name], 4)
            line[f"{name}_TBps"] = round(float(n) * plane * 8 / ms[name] / 1e9, 3)
            line[f"{name}_over_case_measures"] = round(ms[name] / ms["case_measures"], 2)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
