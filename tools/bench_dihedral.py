"""Time cae_dihedral_rows beside the kernel it stands next to, and training with and without augmentation.

    python tools/bench_dihedral.py [--cases 2000] [--calls 20] [--train-cases 4096] [--epochs 10] [--no-train]

cae_dihedral_rows per code at 2000 x 1 x 16 x 16 and 2000 x 1 x 256 x 256 (rows gathered through a permutation), beside
cae_normalise_pack_gather on the same operands: that kernel moves the same 8 bytes per element and gathers rows the same way.
Device events, warm-up, then `--calls` calls of each, alternating, and their mean; the whole measurement twice, so that the
two passes can be compared.  One JSON line per shape and pass.

Then ConvAEModel.train() at the benchmark shape (bench.py's train_api leg: circle data 16 x 16 -> 256 x 256, batch 64, fc 128,
latent 32; a test pass every 10 epochs): images per second of the epoch loop without augmentation and with augment="dihedral",
alternating, twice.  One JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cae_tools_amd import _lib  # noqa: E402
from cae_tools_amd.case_ops import dihedral_rows, pack_gather  # noqa: E402


def timed(runs, calls, warmup):
    """{name: mean ms} of the functions of `runs`, called alternately"""
    for _ in range(warmup):
        for (_, fn) in runs:
            fn()
    torch.cuda.synchronize()
    ms = {key: 0.0 for (key, _) in runs}
    for _ in range(calls):
        for (key, fn) in runs:
            (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[key] += t0.elapsed_time(t1) / calls
    return ms


def kernels(args, dev):
    for side in (16, 256):
        n = args.cases
        gen = torch.Generator(device=dev).manual_seed(side)
        src = torch.rand((n, 1, side, side), device=dev, generator=gen, dtype=torch.float32)
        dst = torch.empty_like(src)
        rows = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
        codes = [torch.full((n,), c, dtype=torch.int32, device=dev) for c in range(8)]
        mixed = (torch.arange(n, device=dev) % 8).to(torch.int32)
        runs = [(f"code_{c}", (lambda c=c: dihedral_rows(src, dst, codes[c], rows, 8))) for c in range(8)]
        runs.append(("codes_mixed", lambda: dihedral_rows(src, dst, mixed, rows, 8)))
        runs.append(("pack_gather", lambda: pack_gather(src, dst, 0, rows, 0.0, 1.0, enable=True)))
        for k in range(args.passes):
            ms = timed(runs, args.calls, args.warmup)
            line = {"pass": k, "rows": n, "plane": [side, side], "MB_moved": round(n * side * side * 8 / 1e6, 2)}
            for (key, _) in runs:
                line[f"{key}_us"] = round(ms[key] * 1e3, 2)
            copies = np.mean([ms[f"code_{c}"] for c in range(4)])
            turns = np.mean([ms[f"code_{c}"] for c in range(4, 8)])
            line["codes_4_7_over_0_3"] = round(float(turns / copies), 3)
            line["codes_0_3_TBps"] = round(n * side * side * 8 / copies / 1e9, 3)
            line["codes_4_7_TBps"] = round(n * side * side * 8 / turns / 1e9, 3)
            line["pack_gather_TBps"] = round(n * side * side * 8 / ms["pack_gather"] / 1e9, 3)
            print(json.dumps(line), flush=True)


def training(args):
    from cae_tools_amd.data import datagen
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    (train, test) = (datagen.generate("circle", args.train_cases, seed=1234), datagen.generate("circle", 512, seed=4321))
    rates = {"off": [], "dihedral": []}
    for _ in range(args.passes):
        for (key, keywords) in (("off", {}), ("dihedral", dict(augment="dihedral", augment_seed=1))):
            torch.manual_seed(0)
            m = ConvAEModel(batch_size=64, nr_epochs=args.epochs, test_interval=10, fc_size=128, encoded_dim_size=32)
            with contextlib.redirect_stdout(io.StringIO()):
                m.train(["lowres"], "hires", train, test, **keywords)
            rates[key].append(round(m.timing["train_images"] / m.timing["epoch_loop_seconds"], 1))
            del m
    print(json.dumps({"train_cases": args.train_cases, "epochs": args.epochs, "images_per_s_off": rates["off"],
                      "images_per_s_dihedral": rates["dihedral"],
                      "dihedral_over_off": round(float(np.mean(rates["dihedral"]) / np.mean(rates["off"])), 4)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--train-cases", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dihedral: no GPU")
    _lib.load()
    kernels(args, torch.device("cuda"))
    if not args.no_train:
        training(args)


if __name__ == "__main__":
    main()
