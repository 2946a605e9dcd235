"""Time cae_strata_sums beside cae_case_measures and cae_joint_hist on the same resident prediction and target.

    python tools/bench_strata.py [--cases 2000] [--size 256] [--calls 20]

fp32 prediction against fp32 target (the datagen circle pattern, a damped prediction with a little noise) under three fp32
stratifiers: "lowres" (the pattern's own 16 x 16 input under the 256 x 256 target, 8 strata over its range: a wave meets one
or two strata), "noise" (per-pixel uniform noise on the target's grid over 64 strata: 64 rounds) and "constant" (one value per
case, 8 strata: one round).  The three entry points read the same prediction and target, so cae_strata_sums is given as its
ratio to each of the other two in the same pass, with the rounds per wave its data asks for - the mean number of distinct
strata among the 64 consecutive pixels a wave takes, counted here with torch - and with the bytes it reads per pixel
(prediction, target and the stratifier's plane spread over the target's pixels) and per second.  Device events, warm-up, then
`--calls` calls of each entry point, alternating, and their mean; the whole measurement twice, so that the two passes can be
compared.  One JSON line per field and pass."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402

(N_BIN, SUB) = (128, 8)
BASE = 16           # datagen cases the fields are made of


def operands(n, size, dev, gen):
    """(prediction, target (n, size * size), the pattern's input (n, 16, 16)): fp32 tensors on dev"""
    from cae_tools_amd.data import datagen
    ds = datagen.generate("circle", BASE, seed=1)
    hires = torch.from_numpy(np.asarray(ds["hires"].values, dtype=np.float32)[:, 0]).to(dev)
    low = torch.from_numpy(np.asarray(ds["lowres"].values, dtype=np.float32)[:, 0]).to(dev)
    if hires.shape[1:] != (size, size):
        hires = torch.nn.functional.interpolate(hires[:, None], size=(size, size), mode="bilinear")[:, 0]
    which = torch.arange(n, device=dev) % BASE
    offset = torch.rand((n, 1, 1), device=dev, generator=gen, dtype=torch.float32)
    a = (hires[which] + offset).reshape(n, size * size)
    p = 293 + 0.7 * (a - 293) + 0.05 * torch.randn(a.shape, device=dev, generator=gen, dtype=torch.float32)
    return p.contiguous(), a.contiguous(), (low[which] + offset).contiguous()


def equal_edges(lo, hi, n_strata):
    return [lo + (hi - lo) * k / n_strata for k in range(1, n_strata)]


def rounds_per_wave(s, edges, size, cases=64):
    """the mean number of distinct strata among the 64 consecutive pixels a wave takes, over the first `cases` cases"""
    s = s[:cases].double()
    if s.dim() == 1:
        s = s.reshape(-1, 1, 1)
    (sh, sw) = s.shape[1:]
    at = lambda n_out, n_in: ((torch.arange(n_out, device=s.device, dtype=torch.float64) + 0.5) * (n_in / n_out)).floor().long().clamp(max=n_in - 1)  # noqa: E731
    grid = s[:, at(size, sh)[:, None], at(size, sw)[None, :]]
    k = torch.bucketize(grid, torch.tensor(edges, dtype=torch.float64, device=s.device), right=True).reshape(s.shape[0], -1)
    plane = k.shape[1] // 64 * 64
    ordered = k[:, :plane].reshape(k.shape[0], -1, 64).sort(dim=-1).values
    return float((1 + (ordered[..., 1:] != ordered[..., :-1]).sum(dim=-1)).double().mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_strata: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, size, plane) = (args.cases, args.size, args.size * args.size)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32
    (p32, a32, low) = operands(n, size, dev, gen)
    (lo, hi) = (float(min(p32.min(), a32.min())), float(max(p32.max(), a32.max())))

    joint = torch.empty((N_BIN, N_BIN), dtype=torch.int64, device=dev)
    marg = torch.empty((2, N_BIN * SUB), dtype=torch.int64, device=dev)
    cond = torch.empty((2, N_BIN, 4), dtype=torch.float64, device=dev)
    outside = torch.empty(4, dtype=torch.int64, device=dev)
    jh_need = int(lib.cae_joint_hist_workspace_bytes(n, plane, N_BIN, SUB))
    jh_ws = torch.empty(max(jh_need, 8), dtype=torch.uint8, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)

    def run_hist():
        _lib.check(lib.cae_joint_hist(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane, lo, hi, N_BIN, SUB,
                                      joint.data_ptr(), marg.data_ptr(), cond.data_ptr(), outside.data_ptr(), jh_ws.data_ptr(),
                                      jh_need, stream))

    def run_measures():
        _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                         measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

    stratifiers = [("lowres", low, equal_edges(float(low.min()), float(low.max()), 8)),
                   ("noise", torch.rand((n, size, size), device=dev, generator=gen, dtype=torch.float32), equal_edges(0.0, 1.0, 64)),
                   ("constant", torch.zeros(n, device=dev, dtype=torch.float32), equal_edges(-1.0, 1.0, 8))]
    for (kind, s, edges) in stratifiers:
        (sh, sw) = (int(s.shape[1]), int(s.shape[2])) if s.dim() == 3 else (1, 1)
        n_strata = len(edges) + 1
        rounds = rounds_per_wave(s, edges, size)
        counts = torch.empty(2 * n_strata + 1, dtype=torch.int64, device=dev)
        sums = torch.empty((n_strata, 8), dtype=torch.float64, device=dev)
        need = int(lib.cae_strata_sums_workspace_bytes(n, size, size, n_strata))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        c_edges = (C.c_double * len(edges))(*edges)
        shift = (C.c_double * n_strata)(*([293.0] * n_strata))

        def run_strata():
            _lib.check(lib.cae_strata_sums(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, s.data_ptr(), F32, sh * sw, n,
                                           size, size, sh, sw, c_edges, len(edges), shift, shift, counts.data_ptr(),
                                           sums.data_ptr(), ws.data_ptr(), need, stream))

        runs = [("strata_sums", run_strata), ("case_measures", run_measures), ("joint_hist", run_hist)]
        per_pixel = 8.0 + 4.0 * sh * sw / plane
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
            got = counts.cpu()
            print(json.dumps({"field": kind, "pass": k, "operands": "fp32 prediction, target and stratifier", "cases": n,
                              "plane": [size, size], "stratifier": [sh, sw], "n_strata": n_strata,
                              "workspace_MB": round(need / 1e6, 3), "pairs": int(got[n_strata:2 * n_strata].sum()),
                              "strata_occupied": int((got[:n_strata] > 0).sum()), "rounds_per_wave": round(rounds, 2),
                              "bytes_per_pixel": round(per_pixel, 4), "strata_sums_ms": round(ms["strata_sums"], 4),
                              "case_measures_ms": round(ms["case_measures"], 4), "joint_hist_ms": round(ms["joint_hist"], 4),
                              "strata_sums_TBps": round(float(n) * plane * per_pixel / ms["strata_sums"] / 1e9, 3),
                              "strata_sums_over_case_measures": round(ms["strata_sums"] / ms["case_measures"], 2),
                              "strata_sums_over_joint_hist": round(ms["strata_sums"] / ms["joint_hist"], 2)}), flush=True)


if __name__ == "__main__":
    main()
