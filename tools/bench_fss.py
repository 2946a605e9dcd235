"""Time cae_case_fss beside cae_case_measures and cae_case_ssim on the same resident prediction and target.

    python tools/bench_fss.py [--cases 2000] [--size 256] [--calls 10]

fp32 prediction against fp32 target in three fields: "circle" (the datagen circle pattern, a damped prediction with a little
noise), "noise" (independent uniform noise in both) and "constant" (one value everywhere: every window is full of events or
empty).  The thresholds are the evaluator's defaults - the 5th percentile of the target below, the 90th, 95th and 99th above,
taken here with torch over the first cases - and the widths its defaults 1, 3, 5, 9, 17, 33, 65 as far as the plane allows,
under both gap rules (every pixel is a pair, so both count the same windows: the rule's cost is what shows).  The three
entry points read the same prediction and target, so cae_case_fss is given as its ratio to each of the other two in the same
pass, with the two amounts of work its launches have, computed from the shapes: the bytes the operand pass reads and
writes (8 per pixel read, (1 + 2 T) / 8 written as bit-planes) and the window steps of the walk, n_case * T * the sum over
the widths of (h - n + 1) * (w - n + 1), each a lane's step of six row counts and six integer accumulations.  cae_case_ssim
runs in groups of 256 cases, as case_ops.case_ssim calls it.  Device events, warm-up, then `--calls` calls of each entry point,
alternating, and their mean; the whole measurement twice, so that the two passes can be compared.  One JSON line per field,
gap rule and pass."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402
from cae_tools_amd.utils import fss, ssim  # noqa: E402

BASE = 16           # datagen cases the pattern field is made of
SSIM_CASES = 256    # case_ops._SSIM_CASES
PERCENTILES = ((0.05, 1), (0.9, 0), (0.95, 0), (0.99, 0))       # utils/distribution.THRESHOLDS; 1: below


def fields(n, size, dev, gen):
    """[(name, prediction, target)]: fp32 tensors (n, size * size) on dev"""
    from cae_tools_amd.data import datagen
    ds = datagen.generate("circle", BASE, seed=1)
    hires = torch.from_numpy(np.asarray(ds["hires"].values, dtype=np.float32)[:, 0]).to(dev)
    if hires.shape[1:] != (size, size):
        hires = torch.nn.functional.interpolate(hires[:, None], size=(size, size), mode="bilinear")[:, 0]
    which = torch.arange(n, device=dev) % BASE
    offset = torch.rand((n, 1, 1), device=dev, generator=gen, dtype=torch.float32)
    a = (hires[which] + offset).reshape(n, size * size).contiguous()
    p = (293 + 0.7 * (a - 293) + 0.05 * torch.randn(a.shape, device=dev, generator=gen, dtype=torch.float32)).contiguous()
    noise = [torch.rand((n, size * size), device=dev, generator=gen, dtype=torch.float32) for _ in range(2)]
    flat = torch.full((n, size * size), 293.0, device=dev, dtype=torch.float32)
    return [("circle", p, a), ("noise", noise[0], noise[1]), ("constant", flat, flat.clone())]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fss: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, size, plane) = (args.cases, args.size, args.size * args.size)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32
    widths = fss.default_widths(size, size)
    (n_thr, n_width) = (len(PERCENTILES), len(widths))
    c_sides = (C.c_int * n_thr)(*[side for (_, side) in PERCENTILES])
    c_widths = (C.c_int * n_width)(*widths)
    steps = n * n_thr * sum((size - w + 1) ** 2 for w in widths)
    bits_bytes = n * plane * (8.0 + (1 + 2 * n_thr) / 8.0)

    sums = torch.empty((n, n_thr, n_width, 6), dtype=torch.int64, device=dev)
    need = int(lib.cae_case_fss_workspace_bytes(n, size, size, n_thr))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    n_scale = ssim.default_scales(size, size)
    ss_sums = torch.empty((n, n_scale, 3), dtype=torch.float64, device=dev)
    ss_need = int(lib.cae_case_ssim_workspace_bytes(min(n, SSIM_CASES), size, size, n_scale))
    ss_ws = torch.empty(max(ss_need, 8), dtype=torch.uint8, device=dev)
    win = (C.c_double * ssim.WIN_SIZE)(*ssim.window().tolist())

    for (kind, p32, a32) in fields(n, size, dev, gen):
        sample = a32[:min(n, 64)].reshape(-1).double()
        values = [float(torch.quantile(sample, q)) for (q, _) in PERCENTILES]
        c_values = (C.c_double * n_thr)(*values)
        (lo, hi) = (float(min(p32.min(), a32.min())), float(max(p32.max(), a32.max())))
        scale = 1.0 / (hi - lo) if hi > lo else 1.0

        def run_measures():
            _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                             measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

        def run_ssim():
            for c0 in range(0, n, SSIM_CASES):
                g = min(n, c0 + SSIM_CASES) - c0
                _lib.check(lib.cae_case_ssim(p32.data_ptr() + 4 * c0 * plane, F32, plane, a32.data_ptr() + 4 * c0 * plane, F32, plane,
                                             g, size, size, n_scale, lo, scale, win, ss_sums[c0:].data_ptr(), ss_ws.data_ptr(),
                                             ss_need, stream))

        for (gaps, rule) in fss.GAPS.items():
            def run_fss():
                _lib.check(lib.cae_case_fss(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, size, size, c_values, c_sides,
                                            n_thr, c_widths, n_width, rule, sums.data_ptr(), ws.data_ptr(), need, stream))

            runs = [("case_fss", run_fss), ("case_measures", run_measures), ("case_ssim", run_ssim)]
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
                scores = fss.scores_from_sums(sums[:min(n, 64)].cpu().numpy(), widths)
                print(json.dumps({"field": kind, "gaps": gaps, "pass": k, "operands": "fp32 prediction and target", "cases": n,
                                  "plane": [size, size], "thresholds": n_thr, "widths": widths, "workspace_MB": round(need / 1e6, 3),
                                  "windows": int(sums[..., 0].sum()), "fss_first_threshold": [round(v, 4) if v == v else None for v in scores["fss"][0]],
                                  "operand_pass_MB": round(bits_bytes / 1e6, 1), "window_steps": steps,
                                  "case_fss_ms": round(ms["case_fss"], 4), "case_measures_ms": round(ms["case_measures"], 4),
                                  "case_ssim_ms": round(ms["case_ssim"], 4),
                                  "window_steps_per_ns": round(steps / ms["case_fss"] / 1e6, 3),
                                  "case_fss_over_case_measures": round(ms["case_fss"] / ms["case_measures"], 2),
                                  "case_fss_over_case_ssim": round(ms["case_fss"] / ms["case_ssim"], 3)}), flush=True)


if __name__ == "__main__":
    main()
