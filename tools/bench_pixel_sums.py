"""Time cae_pixel_sums beside cae_case_measures on the same resident operands.

    python tools/bench_pixel_sums.py [--cases 2000] [--size 256] [--calls 50] [--case-chunks 0,32,64,128]

Two operand pairs: an fp64 prediction against an fp32 big-endian target, and fp32 against fp32.  Both entry points read
the same n * plane * (element bytes) of the two operands; that is the budget both rates are taken over.  cae_pixel_sums
also writes its chunk partials (n_chunk * 9 * plane doubles), reads them again in the fold and writes the nine result
planes; that traffic is printed and added in the "with workspace" rate.  Device events, warm-up, then `--calls` calls of
each entry point, alternating, and their mean.  One JSON line per operand pair and case_chunk (0: the library's cut)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case-chunks", default="0", help="comma-separated case_chunk values (0: the library's cut)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_sums: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, plane) = (args.cases, args.size * args.size)
    gen = torch.Generator(device=dev).manual_seed(1)
    a32 = 290 + 5 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    p64 = a32.to(torch.float64) + 0.1 + 0.5 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float64)
    p32 = p64.to(torch.float32)
    a32be = torch.from_numpy(a32.cpu().numpy().astype(">f4").view(np.uint8)).to(dev)      # the bytes a NetCDF-3 file holds
    pairs = [("fp64 prediction, fp32 big-endian target", p64, _lib.ELEM_F64, a32be, _lib.ELEM_F32_BE, 12),
             ("fp32 prediction, fp32 target", p32, _lib.ELEM_F32, a32, _lib.ELEM_F32, 8)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    sums = torch.empty((9, plane), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    for (name, p, pk, a, ak, pair_bytes) in pairs:
        budget = float(n) * plane * pair_bytes
        for chunk in [int(c) for c in args.case_chunks.split(",")]:
            need = int(lib.cae_pixel_sums_workspace_bytes(n, plane, chunk))
            ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)

            def run_sums():
                _lib.check(lib.cae_pixel_sums(p.data_ptr(), pk, plane, a.data_ptr(), ak, plane, n, plane, 292.5, chunk,
                                              sums.data_ptr(), ws.data_ptr(), need, stream))

            def run_measures():
                _lib.check(lib.cae_case_measures(p.data_ptr(), pk, plane, a.data_ptr(), ak, plane, n, plane,
                                                 measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

            for _ in range(args.warmup):
                run_sums()
                run_measures()
            torch.cuda.synchronize()
            ms = {"pixel_sums": 0.0, "case_measures": 0.0}
            for _ in range(args.calls):
                for (key, fn) in (("pixel_sums", run_sums), ("case_measures", run_measures)):
                    (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    t0.record()
                    fn()
                    t1.record()
                    t1.synchronize()
                    ms[key] += t0.elapsed_time(t1) / args.calls
            extra = 2.0 * need + 9.0 * plane * 8          # partials written and read again, the result written
            print(json.dumps({
                "operands": name, "cases": n, "plane": plane, "case_chunk": chunk,
                "chunks": need // (9 * plane * 8) if need else 1,
                "budget_GB": round(budget / 1e9, 3), "workspace_GB": round(need / 1e9, 3),
                "pixel_sums_ms": round(ms["pixel_sums"], 4),
                "pixel_sums_TBps_of_budget": round(budget / ms["pixel_sums"] / 1e9, 3),
                "pixel_sums_TBps_with_workspace": round((budget + extra) / ms["pixel_sums"] / 1e9, 3),
                "case_measures_ms": round(ms["case_measures"], 4),
                "case_measures_TBps_of_budget": round(budget / ms["case_measures"] / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
