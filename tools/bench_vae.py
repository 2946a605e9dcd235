#!/usr/bin/env python3
"""'var' (VAE + MS-SSIM) training throughput on one MI355X (BASELINE.json configs[4], "cfg5": 64x64 -> 512x512, 1 channel,
batch 16).  Not the headline bench; prints one JSON line.   python tools/bench_vae.py [--steps 20] [--warmup 3] [--cpu]
                                                                                                   [--force-dp]

--force-dp: the data-parallel step of a one-rank RCCL group (vae_forward_backward_sync with SyncBN, its table all-reduces,
the gradient all-reduce, vae_apply_gradients), i.e. what the data-parallel path adds to a step on one GPU.  The output then
also carries an 8-rank cost model built from the one-GPU numbers: a model, not a measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--force-dp", action="store_true", help="the data-parallel step over a one-rank group")
    args = ap.parse_args()
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.var_ae_model import VarEncoder
    from cae_tools_amd.vae_engine import VaeEngine
    spec = create_model_spec(input_size=(64, 64), input_channels=1, output_size=(512, 512), output_channels=1)
    (fc, latent, B) = (128, 32, args.batch)
    torch.manual_seed(0)
    enc = VarEncoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    eng = VaeEngine(spec, fc, latent, B, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(seed=1)
    n = 2 * B
    g = torch.Generator().manual_seed(1)
    x = torch.rand((n, 1, 64, 64), generator=g)
    t = torch.rand((n, 1, 512, 512), generator=g)
    eng.set_dataset(0, x.cuda(), t.cuda())
    perm = eng.upload_perm(np.random.default_rng(0).permutation(n))

    def run(k):
        for s in range(k):
            eng.train_step(0, perm, (s % 2) * B, B, slot=s % 64)

    if args.force_dp:
        import socket
        import torch.distributed as dist
        from cae_tools_amd.dp import GradientHalfSteps
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(sk.getsockname()[1]))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        half = GradientHalfSteps(eng)
        tables = []

        def allreduce(t):
            tables.append(t.numel())
            dist.all_reduce(t)

        def run(k):     # noqa: F811  (the data-parallel step instead of the fused one)
            for s in range(k):
                half.forward_backward_sync(0, perm, (s % 2) * B, B, 0, B, 1, allreduce)
                with torch.cuda.stream(eng.stream):
                    dist.all_reduce(half.grads)
                half.adam_step()
    run(args.warmup)
    eng.sync()
    t0 = time.perf_counter()
    run(args.steps)
    eng.sync()
    dt = (time.perf_counter() - t0) / args.steps
    out = {"metric": "var (VAE + MS-SSIM) train images/sec (64x64 -> 512x512, batch 16)", "value": B / dt, "unit": "images/s",
           "ms_per_step": dt * 1e3, "n_gpus": 1, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "cfg5: VarAEModel 64x64->512x512 1-ch, fc128/latent32, batch %d, MSE + KL + MS-SSIM, Adam" % B,
                      "params": sum(t_[2] for t_ in eng.tensors.values() if t_[0] == 0)},
           "losses_last": eng.read_losses((args.steps - 1) % 64 if not args.force_dp else (args.warmup + args.steps - 1) % eng.loss_slots, 1)[0]}
    if args.force_dp:
        per_step = len(tables) // (args.warmup + args.steps)
        grad_bytes = 4 * eng.n_param
        out["config"]["data_parallel"] = {"world": 1, "sync_bn": True, "table_allreduces_per_step": per_step,
                                          "gradient_allreduce_bytes": grad_bytes}
        # 8 ranks over xGMI, global batch B (B/8 rows per rank): UNMEASURED - no multi-GPU node has run this path.  Compute is
        # bounded below by this one-GPU step / 8; each of the per_step small all-reduces is latency-bound (~25 us per RCCL
        # call is the assumption), the gradient ring moves 2 (7/8) grad_bytes at an assumed 50 GB/s per link.
        out["cost_model_8_ranks_unmeasured"] = {
            "compute_ms_lower_bound": dt * 1e3 / 8, "table_allreduce_ms": per_step * 0.025,
            "gradient_allreduce_ms": 2 * 7 / 8 * grad_bytes / 50e9 * 1e3,
            "note": "a model from one-GPU numbers and assumed RCCL latency / bandwidth, not a measurement"}
    if args.cpu:
        from oracle import vae_oracle as vo
        torch.set_num_threads(16)
        o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict())
        o.train_step(x[:B], t[:B])
        c0 = time.perf_counter()
        o.train_step(x[:B], t[:B])
        cdt = time.perf_counter() - c0
        out["cpu_baseline"] = {"value": B / cdt, "unit": "images/s", "cores": 16, "kind": "port",
                               "sample": "1 training step at batch %d after 1 warm-up, torch CPU (own definition)" % B}
    print(json.dumps(out))
    if args.force_dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
