"""Time the exact nearest-neighbour search of the novelty analysis beside torch.cdist + torch.topk (DESIGN.md §9 'novelty').

    python tools/bench_neighbours.py [--k 5] [--calls 5] [--warmup 1] [--passes 2] [--shapes search loo full] [--no-host]

On resident fp32 rows - uniform noise, the first 4 of every 13 features shared bit for bit between all rows as the static
channels of a box are - three shapes:
    search      2000 queries x 20 000 references x 3328 features (13 variables of 16 x 16)
    loo         20 000 x 20 000 x 3328, the set against itself with self-exclusion
    full        256 x 2048 x 196 608 (3 x 256 x 256), a full-resolution feature size with fewer cases
and for each
    neighbours          cae_case_neighbours, k nearest, fp64 difference form
    cdist_topk          torch.cdist of the same rows converted to fp64 (its default compute mode, which may take the
                        expansion |q|^2 + |r|^2 - 2 q.r through a matrix product) + torch.topk; the conversion is not timed
    cdist_exact_topk    the same with compute_mode="donot_use_mm_for_euclid_dist", the difference form (search only, last: one call)
Device events around each call, warm-up first, then --calls calls of every entry, alternating, and their mean; the whole
measurement --passes times so that two passes can be compared.  A pair-dimension is one (query, reference, feature): one fp64
subtraction and one fp64 fused multiply-add.  The share of the fp64 vector peak is those two instructions per pair-dimension
over the published 78.6 TFLOPS, which counts a fused multiply-add as two operations: 39.3 T instructions/s, 19.65 T
pair-dimensions/s.  It is the share of a whole call, the validity pass and the merge launch included.  The neighbours found
are compared with cdist's (the share of queries whose index lists agree).  numpy on the host is timed once on a reduced size
(64 x 2000 x 3328) and its distances are compared with the kernel's.  One JSON line per shape and pass."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cae_tools_amd import _lib  # noqa: E402

SHAPES = {"search": (2000, 20000, 3328, False), "loo": (20000, 20000, 3328, True), "full": (256, 2048, 3 * 256 * 256, False)}
PEAK_PAIR_DIMS = 78.6e12 / 2 / 2        # fp64 vector instructions per second over the two a pair-dimension needs


def rows(n, dim, dev, gen, static):
    x = torch.rand((n, dim), device=dev, generator=gen, dtype=torch.float32)
    shared = (torch.arange(dim, device=dev) % 13) < 4
    x[:, shared] = static[shared]
    return x


def neighbours_call(lib, q, r, k, self_offset, stream):
    (n_q, n_r, dim) = (int(q.shape[0]), int(r.shape[0]), int(q.shape[1]))
    dist2 = torch.empty((n_q, k), dtype=torch.float64, device=q.device)
    index = torch.empty((n_q, k), dtype=torch.int32, device=q.device)
    count = torch.empty(n_q, dtype=torch.int32, device=q.device)
    need = int(lib.cae_case_neighbours_workspace_bytes(n_q, n_r, k))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=q.device)

    def run():
        _lib.check(lib.cae_case_neighbours(q.data_ptr(), n_q, dim, r.data_ptr(), n_r, dim, dim, k, 0, self_offset, 0, dist2.data_ptr(),
                                           index.data_ptr(), count.data_ptr(), ws.data_ptr(), need, stream))
    return run, dist2, index, count


def measure(args, lib, dev, name, gen):
    (n_q, n_r, dim, same) = SHAPES[name]
    static = torch.rand(dim, device=dev, generator=gen, dtype=torch.float32)
    r = rows(n_r, dim, dev, gen, static)
    q = r if same else rows(n_q, dim, dev, gen, static)
    stream = torch.cuda.current_stream(dev).cuda_stream
    k = args.k
    (run, dist2, index, count) = neighbours_call(lib, q, r, k, 0 if same else -1, stream)
    q64 = q.double()
    r64 = q64 if same else r.double()
    found = {}

    def cdist(mode):
        def go():
            d = torch.cdist(q64, r64, compute_mode=mode)
            if same:
                d.fill_diagonal_(float("inf"))
            found[mode] = torch.topk(d, k, dim=1, largest=False)
        return go

    runs = [("neighbours", run), ("cdist_topk", cdist("use_mm_for_euclid_dist_if_necessary"))]
    pair_dims = float(n_q) * n_r * dim
    for p in range(args.passes):
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
        line = {"shape": name, "pass": p, "queries": n_q, "references": n_r, "features": dim, "k": k, "self_exclusion": same,
                "pair_dimensions": pair_dims}
        for (key, _) in runs:
            line[f"{key}_ms"] = round(ms[key], 3)
            line[f"{key}_T_pair_dims_per_s"] = round(pair_dims / ms[key] / 1e9, 3)
        line["neighbours_share_of_fp64_vector_peak"] = round(pair_dims / (ms["neighbours"] * 1e-3) / PEAK_PAIR_DIMS, 4)
        line["cdist_topk_over_neighbours"] = round(ms["cdist_topk"] / ms["neighbours"], 2)
        theirs = found["use_mm_for_euclid_dist_if_necessary"]
        line["queries_with_the_same_neighbours_as_cdist"] = round(float((theirs.indices.int() == index).all(dim=1).double().mean()), 4)
        line["counts_full"] = bool((count == k).all())
        print(json.dumps(line), flush=True)


def exact(args, lib, dev, gen):
    """cdist's difference-form mode on the search shape: one warm-up, one timed call"""
    (n_q, n_r, dim, _) = SHAPES["search"]
    static = torch.rand(dim, device=dev, generator=gen, dtype=torch.float32)
    (r, q) = (rows(n_r, dim, dev, gen, static), rows(n_q, dim, dev, gen, static))
    (run, _, index, _) = neighbours_call(lib, q, r, args.k, -1, torch.cuda.current_stream(dev).cuda_stream)
    run()
    (q64, r64) = (q.double(), r.double())
    ms = []
    for _ in range(2):
        (t0, t1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0.record()
        found = torch.topk(torch.cdist(q64, r64, compute_mode="donot_use_mm_for_euclid_dist"), args.k, dim=1, largest=False)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return {"shape": "search", "cdist_exact_topk_ms": round(ms[1], 3),
            "queries_with_the_same_neighbours_as_cdist_exact": round(float((found.indices.int() == index).all(dim=1).double().mean()), 4)}


def host(args, lib, dev, gen):
    """numpy on a reduced size, and the kernel's distances against it"""
    (n_q, n_r, dim) = (64, 2000, 3328)
    static = torch.rand(dim, device=dev, generator=gen, dtype=torch.float32)
    (q, r) = (rows(n_q, dim, dev, gen, static), rows(n_r, dim, dev, gen, static))
    (run, dist2, index, _) = neighbours_call(lib, q, r, args.k, -1, torch.cuda.current_stream(dev).cuda_stream)
    run()
    torch.cuda.synchronize()
    (qh, rh) = (q.cpu().numpy().astype(np.float64), r.cpu().numpy().astype(np.float64))
    t0 = time.perf_counter()
    d2 = np.empty((n_q, n_r))
    for i in range(n_q):
        diff = qh[i][None, :] - rh
        d2[i] = (diff * diff).sum(axis=1)
    order = np.argsort(d2, axis=1, kind="stable")[:, :args.k]
    seconds = time.perf_counter() - t0
    want = np.take_along_axis(d2, order, axis=1)
    got = dist2.cpu().numpy()
    return {"host_numpy_s": round(seconds, 3), "host_pair_dimensions": float(n_q) * n_r * dim,
            "host_T_pair_dims_per_s": round(n_q * n_r * dim / seconds / 1e12, 5),
            "same_neighbours_as_numpy": bool((order == index.cpu().numpy()).all()),
            "worst_relative_difference_over_bound": float(np.max(np.abs(got - want) / want) / ((2 * dim + 8) * 2.0 ** -53))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--no-exact", action="store_true", help="leave out cdist's difference-form mode")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbours: no GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    for name in args.shapes:
        measure(args, lib, dev, name, gen)
    if not args.no_host:
        print(json.dumps(host(args, lib, dev, gen)), flush=True)
    if not args.no_exact:
        print(json.dumps(exact(args, lib, dev, gen)), flush=True)


if __name__ == "__main__":
    main()
