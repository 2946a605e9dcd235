"""Time the exact quantiles of the prediction intervals beside the one-pass yardsticks (DESIGN.md §9 'prediction intervals').

    python tools/bench_quantiles.py [--cases 2000] [--size 256] [--calls 5] [--warmup 1] [--passes 2] [--no-host-sort]

On resident fp64 operands (prediction, target and a scale of --cases cases of --size x --size), the three default levels:
    quantiles_pixel / _pooled         cae_score_quantiles, without and with the scale (suffix _scale)
    counts_pixel / _pooled            cae_score_counts of the quantiles just found
    pixel_sums, case_measures         the one-pass yardsticks cae_pixel_sums and cae_case_measures on the same operands
    bounds, denormalise               cae_interval_bounds (pixel quantiles, no scale) beside cae_denormalise_f64 of as many values
for three fields: the circle pattern with the prediction rolled by a column plus noise, uniform noise, and a constant field
(all ties).  Device events around each call, warm-up first, then --calls calls of every entry point, alternating, and their
mean; the whole measurement --passes times so that two passes can be compared.  The byte model is passes x bytes per pass: a
pass reads every operand once (8 bytes each here), pixel mode makes 13 passes, pooled mode 8; the rate printed is that model
over the time.  np.sort of the same scores on the host is timed once per group for reference.  One JSON line per field and
pass."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402

LEVELS = ((4, 5), (9, 10), (19, 20))
(PIXEL_PASSES, POOLED_PASSES) = (13, 8)


def fields(name, n, h, dev, gen):
    """(prediction, target) (n, h * h) fp64 on the device"""
    plane = h * h
    if name == "circle":
        (yy, xx) = torch.meshgrid(torch.linspace(-3, 3, h, device=dev, dtype=torch.float64),
                                  torch.linspace(-2, 2, h, device=dev, dtype=torch.float64), indexing="ij")
        ring = torch.exp(-((torch.sqrt(yy * yy + xx * xx) - 1.0) ** 2) / (2.0 * 0.2 ** 2))
        level = 288 + 5 * torch.rand((n, 1, 1), device=dev, generator=gen, dtype=torch.float64)
        depth = 5 * torch.rand((n, 1, 1), device=dev, generator=gen, dtype=torch.float64)
        a = level + depth * ring[None]
        p = torch.roll(a, 1, dims=-1) + 0.01 * torch.randn((n, h, h), device=dev, generator=gen, dtype=torch.float64)
        return p.reshape(n, plane).contiguous(), a.reshape(n, plane).contiguous()
    if name == "uniform":
        return (torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float64),
                torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float64))
    return (torch.full((n, plane), 288.5, device=dev, dtype=torch.float64), torch.full((n, plane), 288.0, device=dev, dtype=torch.float64))


def measure(args, lib, dev, name, scale, gen):
    (n, h) = (args.cases, args.size)
    plane = h * h
    (p, a) = fields(name, n, h, dev, gen)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F64 = _lib.ELEM_F64
    n_level = len(LEVELS)
    (num, den) = ((C.c_int64 * n_level)(*[v[0] for v in LEVELS]), (C.c_int64 * n_level)(*[v[1] for v in LEVELS]))
    q = {0: torch.empty((n_level, plane), dtype=torch.float64, device=dev), 1: torch.empty((n_level, 1), dtype=torch.float64, device=dev)}
    cnt = torch.empty((n_level, plane), dtype=torch.int64, device=dev)
    total = torch.empty(plane, dtype=torch.int64, device=dev)
    need = int(lib.cae_score_quantiles_workspace_bytes(n, plane, 1, n_level))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    none = (None, 0, 0)

    def quantiles(group, s):
        def run():
            _lib.check(lib.cae_score_quantiles(p.data_ptr(), F64, plane, a.data_ptr(), F64, plane, *s, n, plane, group, num, den, n_level,
                                               q[group].data_ptr(), total.data_ptr(), ws.data_ptr(), need if group else 0, stream))
        return run

    def counts(group):
        def run():
            _lib.check(lib.cae_score_counts(p.data_ptr(), F64, plane, a.data_ptr(), F64, plane, *none, n, plane, group,
                                            q[group].data_ptr(), n_level, cnt.data_ptr(), total.data_ptr(), stream))
        return run

    pixel = torch.empty((9, plane), dtype=torch.float64, device=dev)
    ps_need = int(lib.cae_pixel_sums_workspace_bytes(n, plane, 0))
    ps_ws = torch.empty(max(ps_need, 8), dtype=torch.uint8, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    (lower, upper) = (torch.empty((n, plane), dtype=torch.float64, device=dev), torch.empty((n, plane), dtype=torch.float64, device=dev))
    y32 = torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)

    def pixel_sums():
        _lib.check(lib.cae_pixel_sums(p.data_ptr(), F64, plane, a.data_ptr(), F64, plane, n, plane, 288.0, 0, pixel.data_ptr(),
                                      ps_ws.data_ptr(), ps_need, stream))

    def case_measures():
        _lib.check(lib.cae_case_measures(p.data_ptr(), F64, plane, a.data_ptr(), F64, plane, n, plane, measures.data_ptr(),
                                         cm_ws.data_ptr(), cm_need, stream))

    def bounds():
        _lib.check(lib.cae_interval_bounds(p.data_ptr(), F64, plane, *none, n, plane, q[0].data_ptr() + 8 * plane, 0, lower.data_ptr(),
                                           upper.data_ptr(), stream))

    def denormalise():
        _lib.check(lib.cae_denormalise_f64(y32.data_ptr(), n * plane, 288.0, 10.0, lower.data_ptr(), stream))

    s_args = (scale.data_ptr(), F64, plane)
    runs = [("quantiles_pixel", quantiles(0, none)), ("quantiles_pooled", quantiles(1, none)),
            ("quantiles_pixel_scale", quantiles(0, s_args)), ("quantiles_pooled_scale", quantiles(1, s_args)),
            ("quantiles_pixel", quantiles(0, none)), ("counts_pixel", counts(0)),
            ("quantiles_pooled", quantiles(1, none)), ("counts_pooled", counts(1)),
            ("pixel_sums", pixel_sums), ("case_measures", case_measures), ("bounds", bounds), ("denormalise", denormalise)]
    keys = list(dict.fromkeys(key for (key, _) in runs))
    pair = 16.0 * n * plane         # bytes of one pass over prediction and target
    for k in range(args.passes):
        for _ in range(args.warmup):
            for (_, fn) in runs:
                fn()
        torch.cuda.synchronize()
        (ms, calls) = ({key: 0.0 for key in keys}, {key: 0 for key in keys})
        for _ in range(args.calls):
            for (key, fn) in runs:
                (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[key] += t0.elapsed_time(t1)
                calls[key] += 1
        ms = {key: ms[key] / calls[key] for key in keys}
        line = {"field": name, "pass": k, "cases": n, "plane": [h, h], "levels": [f"{a_}/{b_}" for (a_, b_) in LEVELS],
                "finite_pixel_share": [round(float(torch.isfinite(row).double().mean()), 4) for row in q[0]]}
        for key in keys:
            line[f"{key}_ms"] = round(ms[key], 4)
        model = {"quantiles_pixel": PIXEL_PASSES * pair, "quantiles_pooled": POOLED_PASSES * pair,
                 "quantiles_pixel_scale": PIXEL_PASSES * 1.5 * pair, "quantiles_pooled_scale": POOLED_PASSES * 1.5 * pair,
                 "counts_pixel": pair, "counts_pooled": pair, "pixel_sums": pair, "case_measures": pair,
                 "bounds": 1.5 * pair, "denormalise": 0.75 * pair}
        for key in keys:
            line[f"{key}_TBps_of_model"] = round(model[key] / ms[key] / 1e9, 3)
        line["pixel_over_pixel_sums"] = round(ms["quantiles_pixel"] / ms["pixel_sums"], 2)
        line["pooled_over_case_measures"] = round(ms["quantiles_pooled"] / ms["case_measures"], 2)
        print(json.dumps(line), flush=True)
    return p, a


def host_sort(p, a):
    e = (p - a).abs().cpu().numpy()
    t0 = time.perf_counter()
    np.sort(e, axis=0)
    pixel_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    np.sort(e.reshape(-1))
    return {"host_np_sort_pixel_s": round(pixel_s, 3), "host_np_sort_pooled_s": round(time.perf_counter() - t0, 3),
            "scores": int(e.size)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--fields", nargs="+", default=["circle", "uniform", "constant"])
    ap.add_argument("--no-host-sort", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_quantiles: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    scale = 0.5 + torch.rand((args.cases, args.size * args.size), device=dev, generator=gen, dtype=torch.float64)
    for name in args.fields:
        (p, a) = measure(args, lib, dev, name, scale, gen)
        if name == "uniform" and not args.no_host_sort:
            print(json.dumps(host_sort(p, a)), flush=True)
        del p, a
    assert math.isfinite(float(scale.sum()))


if __name__ == "__main__":
    main()
