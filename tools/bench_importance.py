"""Time the two kernels of permutation importance beside what they replace.

    python tools/bench_importance.py [--cases 2000] [--size 256] [--in-size 16] [--calls 20] [--model-cases 2000]

Kernels, on the same resident operands (fp32 unperturbed and perturbed scores, fp64 target):
    importance          cae_case_importance without a map: 4 + 4 + 8 bytes read per pixel
    importance_map      the same with the carried per-pixel map
    composition         cae_denormalise_f64 of the perturbed scores + cae_case_measures + cae_pixel_sums of the fp64 copy
                        against the target: what a round is composed of without the fused pass
    case_measures       cae_case_measures alone on the fp64 copy and the target
    pack_gather         cae_normalise_pack_gather of one variable of in-size x in-size into a batch of 13 channels, by a cycle
    pack                cae_normalise_pack of the same variable
Each is given as its time and, for the importance passes, as the bandwidth over the 16 bytes per pixel they need.  Device
events, warm-up, then `--calls` calls of each entry point, alternating, and their mean; the whole measurement twice, so that
the two passes can be compared.  One JSON line per pass.

Then a ConvAE model is trained for one epoch on --model-cases circle cases (16 x 16 to 256 x 256) and BaseModel.importance is
timed with one and with three repeats of its one input variable: a round is half the difference.  Beside it one _score_all
of the same batch: the share of a round that is not the forward pass.  One more JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402


def kernels(args, lib, dev):
    (n, h, hi) = (args.cases, args.size, args.in_size)
    plane = h * h
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float32)
    pert = (base + 0.1 * torch.randn((n, plane), device=dev, generator=gen, dtype=torch.float32)).clamp_(0, 1)
    a64 = 288 + 10 * torch.rand((n, plane), device=dev, generator=gen, dtype=torch.float64)
    den = torch.empty((n, plane), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    (F64, vmin, rng) = (_lib.ELEM_F64, 288.0, 10.0)

    sums = torch.empty((n, 8), dtype=torch.float64, device=dev)
    field = torch.zeros((3, plane), dtype=torch.float64, device=dev)
    need = int(lib.cae_case_importance_workspace_bytes(n, plane))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def run_importance(with_map):
        def run():
            _lib.check(lib.cae_case_importance(base.data_ptr(), plane, pert.data_ptr(), plane, a64.data_ptr(), F64, plane, n, plane, vmin,
                                               rng, sums.data_ptr(), field.data_ptr() if with_map else None, ws.data_ptr(), need, stream))
        return run

    measures = torch.empty((n, 2), dtype=torch.float64, device=dev)
    cm_need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    cm_ws = torch.empty(max(cm_need, 8), dtype=torch.uint8, device=dev)
    pixel = torch.empty((9, plane), dtype=torch.float64, device=dev)
    ps_need = int(lib.cae_pixel_sums_workspace_bytes(n, plane, 0))
    ps_ws = torch.empty(max(ps_need, 8), dtype=torch.uint8, device=dev)

    def run_measures():
        _lib.check(lib.cae_case_measures(den.data_ptr(), F64, plane, a64.data_ptr(), F64, plane, n, plane, measures.data_ptr(),
                                         cm_ws.data_ptr(), cm_need, stream))

    def run_composition():
        _lib.check(lib.cae_denormalise_f64(pert.data_ptr(), n * plane, vmin, rng, den.data_ptr(), stream))
        run_measures()
        _lib.check(lib.cae_pixel_sums(den.data_ptr(), F64, plane, a64.data_ptr(), F64, plane, n, plane, vmin + rng / 2, 0, pixel.data_ptr(),
                                      ps_ws.data_ptr(), ps_need, stream))

    plane_in = hi * hi
    raw = 280 + 20 * torch.rand((n, 1, plane_in), device=dev, generator=gen, dtype=torch.float32)
    batch = torch.zeros((n, 13, plane_in), dtype=torch.float32, device=dev)
    rows = torch.roll(torch.arange(n, dtype=torch.int32, device=dev), 1)

    def run_gather():
        _lib.check(lib.cae_normalise_pack_gather(raw.data_ptr(), n, 1, plane_in, batch.data_ptr(), n, 13, 5, 280.0, 20.0, 1,
                                                 rows.data_ptr(), stream))

    def run_pack():
        _lib.check(lib.cae_normalise_pack(raw.data_ptr(), n, 1, plane_in, batch.data_ptr(), 13, 5, 280.0, 20.0, 1, stream))

    runs = [("importance", run_importance(False)), ("importance_map", run_importance(True)), ("composition", run_composition),
            ("case_measures", run_measures), ("pack_gather", run_gather), ("pack", run_pack)]
    _lib.check(lib.cae_denormalise_f64(pert.data_ptr(), n * plane, vmin, rng, den.data_ptr(), stream))
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
        line = {"pass": k, "operands": "fp32 scores, fp64 target", "cases": n, "plane": [h, h], "workspace_MB": round(need / 1e6, 3)}
        for (key, _) in runs:
            line[f"{key}_ms"] = round(ms[key], 4)
        for key in ("importance", "importance_map"):
            line[f"{key}_TBps_of_16_bytes"] = round(float(n) * plane * 16 / ms[key] / 1e9, 3)
            line[f"composition_over_{key}"] = round(ms["composition"] / ms[key], 2)
            line[f"{key}_over_case_measures"] = round(ms[key] / ms["case_measures"], 2)
        line["pack_gather_over_pack"] = round(ms["pack_gather"] / ms["pack"], 2)
        print(json.dumps(line), flush=True)


def round_of_the_model(args, dev):
    from cae_tools_amd.data import datagen
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    from cae_tools_amd.models.ds_dataset import DSDataset
    n = args.model_cases
    (train, test) = (datagen.generate("circle", n, seed=1234), datagen.generate("circle", n, seed=4321))
    torch.manual_seed(0)
    model = ConvAEModel(batch_size=64, nr_epochs=1, test_interval=1, fc_size=16, encoded_dim_size=4)
    with contextlib.redirect_stdout(io.StringIO()):
        model.train(["lowres"], "hires", train, test)
        data = DSDataset(test, ["lowres"], "hires", normalise_in=model.normalise_input, normalise_out=False)
        data.set_normalisation_parameters(model.normalisation_parameters)
        x = data.device_inputs()

        def timed(fn, repeat):
            fn()                # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(repeat):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / repeat * 1e3

        score_ms = timed(lambda: model._score_all(x), 5)
        one_ms = timed(lambda: model.importance(test, ["lowres"], "hires", repeats=1), 3)
        three_ms = timed(lambda: model.importance(test, ["lowres"], "hires", repeats=3), 3)
    round_ms = (three_ms - one_ms) / 2
    print(json.dumps({"model": "ConvAE 16x16 -> 256x256", "cases": n, "score_all_ms": round(score_ms, 3),
                      "importance_1_repeat_ms": round(one_ms, 3), "importance_3_repeats_ms": round(three_ms, 3),
                      "round_ms": round(round_ms, 3), "round_not_forward_share": round(1.0 - score_ms / round_ms, 3)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--in-size", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--model-cases", type=int, default=2000, help="0: skip the model's round")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_importance: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    kernels(args, lib, dev)
    if args.model_cases > 0:
        round_of_the_model(args, dev)


if __name__ == "__main__":
    main()
