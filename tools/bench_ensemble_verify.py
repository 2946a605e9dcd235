"""Time cae_ensemble_verify beside cae_ensemble_moments on the same resident operands, and VaeEngine.ensemble with and without
a target.

    python tools/bench_ensemble_verify.py [--cases 2000] [--size 256] [--k 16] [--calls 20] [--engine-cases 2000]

The draws are cases * K planes of fp32, in [case][draw] and in [draw][case] order; the target is fp32.  The byte budget both
rates are taken over is K * 4 + target bytes per pixel: what cae_ensemble_verify has to read (cae_ensemble_moments reads
K * 4 and writes 16).  Device events, warm-up, then `--calls` calls of each entry point, alternating, and their mean.  The
engine part builds an untrained VAE (16x16 -> 256x256, latent 32, fc 128, 64 rows) and times ensemble() over --engine-cases
cases on the device, wall clock around a synchronised call.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402


def _kernels(args, lib, dev):
    (n, k, plane) = (args.cases, args.k, args.size * args.size)
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.rand((n, 1, plane), device=dev, generator=gen, dtype=torch.float32)
    draws = base + 0.02 * torch.randn((n, k, plane), device=dev, generator=gen, dtype=torch.float32)
    target = 288.0 + 10.5 * (base[:, 0] + 0.02 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32))
    del base
    stream = torch.cuda.current_stream(dev).cuda_stream
    (mean, std) = (torch.empty((n, plane), dtype=torch.float64, device=dev) for _ in range(2))
    sums = torch.empty((n, 5), dtype=torch.float64, device=dev)
    ranks = torch.zeros(k + 2, dtype=torch.int64, device=dev)
    need = int(lib.cae_ensemble_verify_workspace_bytes(n, plane, k))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    budget = float(n) * plane * (k * 4 + 4)
    for layout in ("case", "draw"):
        y = draws if layout == "case" else draws.transpose(0, 1).contiguous()
        (cs, ds) = (k * plane, plane) if layout == "case" else (plane, n * plane)

        def run_verify():
            _lib.check(lib.cae_ensemble_verify(y.data_ptr(), cs, ds, target.data_ptr(), _lib.ELEM_F32, plane, n, plane, k, 288.0,
                                               10.5, sums.data_ptr(), ranks.data_ptr(), ws.data_ptr(), need, stream))

        def run_moments():
            _lib.check(lib.cae_ensemble_moments(y.data_ptr(), cs, ds, n, plane, k, 0, k, 288.0, 10.5, mean.data_ptr(),
                                                std.data_ptr(), None, 0, stream))

        for _ in range(args.warmup):
            run_verify()
            run_moments()
        torch.cuda.synchronize()
        ms = {"verify": 0.0, "moments": 0.0}
        for _ in range(args.calls):
            for (key, fn) in (("verify", run_verify), ("moments", run_moments)):
                (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[key] += t0.elapsed_time(t1) / args.calls
        print(json.dumps({"layout": f"[{layout}]", "cases": n, "plane": plane, "k": k, "budget_GB": round(budget / 1e9, 3),
                          "workspace_MB": round(need / 1e6, 3), "verify_ms": round(ms["verify"], 4),
                          "verify_TBps_of_budget": round(budget / ms["verify"] / 1e9, 3),
                          "moments_ms": round(ms["moments"], 4),
                          "moments_TBps_of_budget": round(budget / ms["moments"] / 1e9, 3)}), flush=True)
        del y


def _engine(args, dev):
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.var_ae_model import VarEncoder
    from cae_tools_amd.vae_engine import VaeEngine
    (n, k) = (args.engine_cases, args.k)
    spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(256, 256), output_channels=1)
    torch.manual_seed(0)
    (enc, dec) = (VarEncoder(spec.get_input_layers(), 32, 128), Decoder(spec.get_output_layers(), 32, 128))
    eng = VaeEngine(spec, 128, 32, 64, device=dev)
    eng.load_state(enc.state_dict(), dec.state_dict())
    gen = torch.Generator(device=dev).manual_seed(2)
    (mu, logvar) = eng.encode(torch.rand((n, 1, 16, 16), device=dev, generator=gen, dtype=torch.float32))
    target = 288.0 + 10.5 * torch.rand((n, 1, 256, 256), device=dev, generator=gen, dtype=torch.float32)
    seconds = {}
    for (name, keywords) in (("without_target", {}), ("with_target", {"target": target})):
        for timed in (False, True):         # one warm-up call, one timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.ensemble(mu, logvar, k, seed=1, vmin=288.0, vmax=298.5, **keywords)
            torch.cuda.synchronize()
            if timed:
                seconds[name] = time.perf_counter() - t0
    budget = float(n) * 256 * 256 * (k * 4 + 4)
    print(json.dumps({"engine": "16x16 -> 256x256, latent 32, fc 128, 64 rows", "cases": n, "k": k,
                      "ensemble_ms": round(seconds["without_target"] * 1e3, 2),
                      "ensemble_with_target_ms": round(seconds["with_target"] * 1e3, 2),
                      "verify_budget_GB": round(budget / 1e9, 3)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--engine-cases", type=int, default=2000, help="cases of the VaeEngine.ensemble timing (0: skip it)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_verify: no GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    _kernels(args, _lib.load(), dev)
    if args.engine_cases > 0:
        torch.cuda.empty_cache()
        _engine(args, dev)


if __name__ == "__main__":
    main()
