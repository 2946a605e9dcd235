"""Time cae_joint_hist at 128 bins of 8 beside cae_case_measures on the same resident prediction and target.

    python tools/bench_joint_hist.py [--cases 2000] [--size 256] [--calls 20]

fp32 prediction against fp32 target, three kinds of field: "smooth" (the datagen circle pattern, a damped prediction with a
little noise), "noise" (both uniform over the range: 64 distinct bin pairs among a wave's 64 pixels) and "constant" (one bin
pair: every count of the call lands on three counters).  Both entry points read the same bytes, so cae_joint_hist is given as
its ratio to cae_case_measures in the same pass, and with the rounds per wave its data asks for: the mean number of distinct
coarse bin pairs among the 64 pixels a wave bins together (pixel j of 64 consecutive 4-pixel groups), counted here with
torch.  Device events, warm-up, then `--calls` calls of each entry point, alternating, and their mean; the whole measurement
twice, so that the two passes can be compared.  One JSON line per field and pass."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402

(N_BIN, SUB) = (128, 8)


def fields(kind, n, size, dev, gen):
    """(prediction, target, lo, hi): (n, size * size) fp32 tensors on dev"""
    plane = size * size
    if kind == "smooth":
        from cae_tools_amd.data import datagen
        ring = torch.from_numpy(np.asarray(datagen.generate("circle", 1, seed=1)["hires"].values, dtype=np.float32)[0, 0]).to(dev)
        ring = (ring - ring.min()) / (ring.max() - ring.min())
        if ring.shape != (size, size):
            ring = torch.nn.functional.interpolate(ring[None, None], size=(size, size), mode="bilinear")[0, 0]
        u = torch.rand((n, 2), device=dev, generator=gen, dtype=torch.float32)
        a = 288 + 5 * u[:, :1] + ring.reshape(1, plane) * 5 * u[:, 1:]          # the pattern's own offsets and amplitudes
        p = 293 + 0.7 * (a - 293) + 0.05 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)
    elif kind == "noise":
        a = 288 + 10 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
        p = 288 + 10 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    else:
        a = torch.full((n, plane), 291.0, device=dev, dtype=torch.float32)
        p = torch.full((n, plane), 291.5, device=dev, dtype=torch.float32)
    return p.contiguous(), a.contiguous(), 288.0, 298.0


def rounds_per_wave(p, a, lo, hi, cases=64):
    """the mean number of distinct coarse bin pairs among the 64 pixels a wave bins together, over the first `cases` cases"""
    def coarse(v):
        t = (v[:cases].double() - lo) * (N_BIN * SUB / (hi - lo))
        return (t.clamp(0, N_BIN * SUB - 1).long() // SUB)
    key = coarse(a) * N_BIN + coarse(p)
    plane = key.shape[1] // 256 * 256
    waves = key[:, :plane].reshape(key.shape[0], -1, 64, 4).transpose(2, 3)         # (case, 256 pixels, j, lane)
    ordered = waves.sort(dim=-1).values
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
        raise SystemExit("bench_joint_hist: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    (n, plane) = (args.cases, args.size * args.size)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F32 = _lib.ELEM_F32

    joint = torch.empty((N_BIN, N_BIN), dtype=torch.int64, device=dev)
    marg = torch.empty((2, N_BIN * SUB), dtype=torch.int64, device=dev)
    cond = torch.empty((2, N_BIN, 4), dtype=torch.float64, device=dev)
    outside = torch.empty(4, dtype=torch.int64, device=dev)
    need = int(lib.cae_joint_hist_workspace_bytes(n, plane, N_BIN, SUB))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)

    for kind in ("smooth", "noise", "constant"):
        (p32, a32, lo, hi) = fields(kind, n, args.size, dev, gen)
        rounds = rounds_per_wave(p32, a32, lo, hi)

        def run_hist():
            _lib.check(lib.cae_joint_hist(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane, lo, hi, N_BIN, SUB,
                                          joint.data_ptr(), marg.data_ptr(), cond.data_ptr(), outside.data_ptr(), ws.data_ptr(),
                                          need, stream))

        def run_measures():
            _lib.check(lib.cae_case_measures(p32.data_ptr(), F32, plane, a32.data_ptr(), F32, plane, n, plane,
                                             measures.data_ptr(), cm_ws.data_ptr(), cm_need, stream))

        runs = [("joint_hist", run_hist), ("case_measures", run_measures)]
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
            print(json.dumps({"field": kind, "pass": k, "operands": "fp32 prediction, fp32 target", "cases": n,
                              "plane": [args.size, args.size], "n_bin": N_BIN, "sub": SUB, "workspace_MB": round(need / 1e6, 3),
                              "pairs": int(joint.sum()), "rounds_per_wave": round(rounds, 2),
                              "case_measures_ms": round(ms["case_measures"], 4), "joint_hist_ms": round(ms["joint_hist"], 4),
                              "joint_hist_TBps": round(float(n) * plane * 8 / ms["joint_hist"] / 1e9, 3),
                              "joint_hist_over_case_measures": round(ms["joint_hist"] / ms["case_measures"], 2)}), flush=True)


if __name__ == "__main__":
    main()
