"""Time cae_case_spectra beside cae_case_measures on the same resident operands.

    python tools/bench_spectra.py [--cases 2000] [--size 256] [--calls 20]

fp32 prediction against fp32 target.  cae_case_spectra is arithmetic, not traffic: per case 3 fields * (2 H W Wc + 4 H H Wc)
fused multiply-adds, Wc = W / 2 + 1, two flops each, which is the count its fp64 GFLOP/s are taken over; cae_case_measures
reads the same operands once and is given as the bandwidth it reaches.  Device events, warm-up, then `--calls` calls of each
entry point, alternating, and their mean; the whole measurement twice, so that the two passes can be compared.  One JSON
line per pass."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402
from cae_tools_amd.utils import spectra  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectra: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, h, w) = (args.cases, args.size, args.size)
    plane = h * w
    gen = torch.Generator(device=dev).manual_seed(1)
    a32 = 290 + 5 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    p32 = a32 + 0.5 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)
    n_bin = spectra.bin_count(h, w)
    wy = torch.from_numpy(spectra.window(h)).to(dev)
    wx = torch.from_numpy(spectra.window(w)).to(dev)
    table = torch.from_numpy(spectra.bin_table(h, w)).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sums = torch.empty((n, n_bin, 4), dtype=torch.float64, device=dev)
    counted = torch.empty(n, dtype=torch.int32, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    need = int(lib.cae_case_spectra_workspace_bytes(n, h, w, n_bin))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    (F32, wc) = (_lib.ELEM_F32, w // 2 + 1)
    flops = float(n) * 3 * (2.0 * h * w * wc + 4.0 * h * h * wc) * 2
    budget = float(n) * plane * 8

    def run_spectra():
        _lib.check(lib.cae_case_spectra(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, h, w, wy.data_ptr(),
                                        wx.data_ptr(), table.data_ptr(), n_bin, sums.data_ptr(), counted.data_ptr(),
                                        ws.data_ptr(), need, stream))

    def run_measures():
        _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                         measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

    for k in range(args.passes):
        for _ in range(args.warmup):
            run_spectra()
            run_measures()
        torch.cuda.synchronize()
        ms = {"case_spectra": 0.0, "case_measures": 0.0}
        for _ in range(args.calls):
            for (key, fn) in (("case_spectra", run_spectra), ("case_measures", run_measures)):
                (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[key] += t0.elapsed_time(t1) / args.calls
        print(json.dumps({
            "pass": k, "operands": "fp32 prediction, fp32 target", "cases": n, "h": h, "w": w, "n_bin": n_bin,
            "counted": int(counted.sum().item()), "workspace_GB": round(need / 1e9, 3), "fp64_TFLOP": round(flops / 1e12, 4),
            "case_spectra_ms": round(ms["case_spectra"], 3),
            "case_spectra_fp64_GFLOPs": round(flops / ms["case_spectra"] / 1e6, 1),
            "case_measures_ms": round(ms["case_measures"], 4),
            "case_measures_TBps": round(budget / ms["case_measures"] / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
