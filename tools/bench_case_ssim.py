"""Time cae_case_ssim beside cae_case_measures and cae_case_spectra on the same resident operands.

    python tools/bench_case_ssim.py [--cases 2000] [--size 256] [--calls 20]

fp32 prediction against fp32 target, five scales where the size allows them.  cae_case_ssim is called as engine.case_ssim
calls it, in runs of at most engine._SSIM_CASES cases over one workspace.  Its two budgets are printed with the time:
  bytes   the operands read twice (the walk of scale 0 and the first pooling), every pooled fp64 plane written once and read
          by its walk and, but for the last, by the next pooling
  FMAs    2 * 5 * 11 fp64 fused multiply-adds per pixel and scale - five moments, eleven taps, two passes - without the halo
          rows and columns a band and a strip filter again
so that the figure says which of the two the kernel is nearer to.  cae_case_measures reads the same operands once and is
given as the bandwidth it reaches; cae_case_spectra as its time.  Device events, warm-up, then `--calls` calls of each entry
point, alternating, and their mean; the whole measurement twice, so that the two passes can be compared.  One JSON line per
pass."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib, engine  # noqa: E402
from cae_tools_amd.utils import spectra, ssim  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--no-spectra", action="store_true", help="leave cae_case_spectra out")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_case_ssim: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, h, w) = (args.cases, args.size, args.size)
    plane = h * w
    gen = torch.Generator(device=dev).manual_seed(1)
    a32 = 290 + 5 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    p32 = a32 + 0.5 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32

    n_scale = ssim.default_scales(h, w)
    shapes = ssim.scale_shapes(h, w, n_scale)
    chunk = min(n, engine._SSIM_CASES)
    ss_need = int(lib.cae_case_ssim_workspace_bytes(chunk, h, w, n_scale))
    ss_ws = torch.empty(max(ss_need, 8), dtype=torch.uint8, device=dev)
    ss_sums = torch.empty((n, n_scale, 3), dtype=torch.float64, device=dev)
    win = (_lib.C.c_double * ssim.WIN_SIZE)(*ssim.window().tolist())
    (shift, scale) = (290.0, 1.0 / 5.0)
    pooled = [hs * ws for (hs, ws) in shapes[1:]]
    ss_bytes = float(n) * (2 * plane * 8 + sum(16 * px * (3 if k + 1 < len(pooled) else 2) for (k, px) in enumerate(pooled)))
    ss_fma = float(n) * sum(2 * 5 * ssim.WIN_SIZE * hs * ws for (hs, ws) in shapes)

    def run_ssim():
        for lo in range(0, n, chunk):
            g = min(n, lo + chunk) - lo
            _lib.check(lib.cae_case_ssim(p32[lo:].data_ptr(), F32, plane, a32[lo:].data_ptr(), F32, plane, g, h, w, n_scale,
                                         shift, scale, win, ss_sums[lo:].data_ptr(), ss_ws.data_ptr(), ss_need, stream))

    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)

    def run_measures():
        _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                         measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

    runs = [("case_ssim", run_ssim), ("case_measures", run_measures)]
    if not args.no_spectra:
        n_bin = spectra.bin_count(h, w)
        wy = torch.from_numpy(spectra.window(h)).to(dev)
        wx = torch.from_numpy(spectra.window(w)).to(dev)
        table = torch.from_numpy(spectra.bin_table(h, w)).to(dev)
        sp_sums = torch.empty((n, n_bin, 4), dtype=torch.float64, device=dev)
        counted = torch.empty(n, dtype=torch.int32, device=dev)
        sp_need = int(lib.cae_case_spectra_workspace_bytes(n, h, w, n_bin))
        sp_ws = torch.empty(max(sp_need, 16), dtype=torch.uint8, device=dev)

        def run_spectra():
            _lib.check(lib.cae_case_spectra(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, h, w, wy.data_ptr(),
                                            wx.data_ptr(), table.data_ptr(), n_bin, sp_sums.data_ptr(), counted.data_ptr(),
                                            sp_ws.data_ptr(), sp_need, stream))

        runs.append(("case_spectra", run_spectra))

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
        windows = ss_sums[:, :, 0].sum(dim=0).cpu().tolist()
        line = {"pass": k, "operands": "fp32 prediction, fp32 target", "cases": n, "h": h, "w": w, "n_scale": n_scale,
                "cases_per_call": chunk, "windows_per_scale": [int(v) for v in windows],
                "workspace_GB": round(ss_need / 1e9, 3),
                "case_ssim_ms": round(ms["case_ssim"], 3),
                "case_ssim_bytes_per_pixel": round(ss_bytes / (n * plane), 2),
                "case_ssim_fma_per_pixel": round(ss_fma / (n * plane), 1),
                "case_ssim_TBps": round(ss_bytes / ms["case_ssim"] / 1e9, 3),
                "case_ssim_fp64_TFLOPs": round(2 * ss_fma / ms["case_ssim"] / 1e9, 3),
                "case_measures_ms": round(ms["case_measures"], 4),
                "case_measures_TBps": round(float(n) * plane * 8 / ms["case_measures"] / 1e9, 3)}
        if "case_spectra" in ms:
            line["case_spectra_ms"] = round(ms["case_spectra"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
