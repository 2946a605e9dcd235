"""cae_joint_hist on the GPU through engine.joint_histogram, against the numpy restatement of the definition
(distribution_ref.py): the joint, marginal and outside counts integer for integer, every cond sum within c 2^-53 S|x_i| of the
math.fsum value - the bound of any order of summation, derived in distribution_ref.py - for planes around the wave and chunk
sizes, 1 to 17 cases, five (n_bin, sub) pairs, a call cut into several workgroups, every element kind, a second channel,
misaligned case starts, smooth, noisy and constant fields, values on the bin edges, outside the range and not finite; two runs
byte for byte, outputs overwritten whole, empty calls; then train_cae -> distribution with the files it writes.

Largest |got - fsum| / bound measured on an MI355X (each check prints its figure before it asserts): 0.66 over the planes,
cases and bins (plane 4099, 17 cases, 128 x 32), 0.18 over nine workgroups, 0.086 noise, 8.7e-4 a constant field, 0 on the
edges, 0.37 over the element kinds, 0.085 with misaligned case starts; every count exact."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib
from cae_tools_amd.engine import device_operand, joint_histogram
from distribution_ref import Reference, channel0

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
BINS = [(1, 1), (2, 3), (7, 32), (128, 8), (128, 32)]
PLANES = [1, 63, 64, 65, 4099]
CASES = [1, 3, 17]


@pytest.fixture(scope="module")
def pattern():
    """17 cases of the datagen circle pattern, (17, 65536) in [0, 1]: (hires - 288) / 10"""
    from cae_tools_amd.data import datagen
    hires = np.asarray(datagen.generate("circle", 17, seed=99)["hires"].values, dtype=np.float64)
    return (hires[:, 0].reshape(17, -1) - 288.0) / 10.0


def _smooth(pattern, rng, n, plane, hi):
    """target: `plane` consecutive pixels across the ring of n pattern cases, scaled to [0, hi]; prediction: damped, with noise"""
    a = pattern[:n, 100 * 256:100 * 256 + plane] * hi
    p = 0.5 * hi + 0.7 * (a - 0.5 * hi) + 0.01 * hi * rng.standard_normal(a.shape)
    return p.copy(), a.copy()


def _sprinkle(rng, p, a, hi, n_bin):
    """values at lo, at hi and on bin edges, below and above the range, -0.0, NaN and +-Inf at random places of both"""
    special = [0.0, hi, -0.0, -1e-300, -0.25, hi + 0.25, np.nextafter(hi, np.inf), np.nextafter(hi, 0.0), 1e300, -1e300,
               np.nan, np.inf, -np.inf] + [k / 8.0 for k in range(0, n_bin + 1, max(1, n_bin // 5))]
    flat = (p.reshape(-1), a.reshape(-1))
    for (k, v) in enumerate(special):
        for which in (0, 1):
            flat[which][int(rng.integers(flat[which].size))] = v
        if k % 3 == 0:                      # and in both at one pixel
            at = int(rng.integers(flat[0].size))
            flat[0][at] = flat[1][at] = v
    return p, a


def _nchw(x, h, w, channels=1, dtype=np.float64):
    """(N, plane) values as channel 0 of an (N, C, h, w) array whose other channels are NaN"""
    out = np.full((x.shape[0], channels, h, w), np.nan, dtype=dtype)
    out[:, 0] = x.reshape(x.shape[0], h, w)
    return out


def _check(label, got, ref, n_bin, sub):
    (joint, marg, cond, outside) = got
    assert joint.dtype == np.int64 and marg.dtype == np.int64 and outside.dtype == np.int64 and cond.dtype == np.float64
    assert joint.shape == (n_bin, n_bin) and marg.shape == (2, n_bin * sub) and cond.shape == (2, n_bin, 4) and outside.shape == (4,)
    assert np.array_equal(joint, ref.joint), label
    assert np.array_equal(marg, ref.marg), label
    assert np.array_equal(outside, ref.outside), label
    assert int(joint.sum()) == ref.pairs
    bounded = np.isfinite(ref.bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(cond - ref.cond)
        worst = float(np.max(np.where(bounded & (ref.bound > 0), err / np.where(ref.bound > 0, ref.bound, 1.0), 0.0)))
        print(f"{label}: {ref.pairs} pairs, max |cond - fsum| / bound = {worst:.3e}")
        assert np.where(bounded, err <= ref.bound, cond == ref.cond).all(), label


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"{b[0]}x{b[1]}")
def test_planes_cases_and_bins(pattern, bins, plane):
    (n_bin, sub) = bins
    hi = n_bin / 8.0                        # the coarse edges k / 8 are exact
    rng = np.random.default_rng(1000 * n_bin + plane)
    for n in CASES:
        (p, a) = _sprinkle(rng, *_smooth(pattern, rng, n, plane, hi), hi, n_bin)
        got = joint_histogram(_nchw(p, 1, plane), _nchw(a, 1, plane), 0.0, hi, n_bin=n_bin, sub=sub)
        _check(f"plane {plane}, {n} cases, {n_bin} x {sub}", got, Reference(p, a, 0.0, hi, n_bin, sub), n_bin, sub)


def test_a_call_of_several_workgroups(pattern):
    """17 cases of 4099 pixels are 34 (case, chunk) items: nine workgroups, whose partials the fold adds"""
    (n, plane, n_bin, sub) = (17, 4099, 128, 8)
    lib = _lib.load()
    groups = int(lib.cae_joint_hist_workspace_bytes(n, plane, n_bin, sub)) // (2 * n_bin * 4 * 8)
    assert groups == 9 and groups >= 3
    rng = np.random.default_rng(3)
    (p, a) = _smooth(pattern, rng, n, plane, 16.0)
    got = joint_histogram(_nchw(p, 1, plane), _nchw(a, 1, plane), 0.0, 16.0, n_bin=n_bin, sub=sub)
    ref = Reference(p, a, 0.0, 16.0, n_bin, sub)
    _check("nine workgroups", got, ref, n_bin, sub)
    assert ref.pairs == n * plane and (ref.joint.sum(axis=1) > 0).sum() > 20        # the data spreads over the bins


@pytest.mark.parametrize("field", ["noise", "constant", "edges"])
def test_noise_constant_and_edges(field):
    (n, h, w, n_bin, sub) = (3, 33, 65, 128, 8)
    (plane, hi) = (h * w, 16.0)
    rng = np.random.default_rng(17)
    if field == "noise":                    # 64 distinct bin pairs in a wave
        (p, a) = (rng.uniform(0.0, hi, (n, plane)), rng.uniform(0.0, hi, (n, plane)))
    elif field == "constant":               # one bin: every lane adds to the same counters
        (p, a) = (np.full((n, plane), 7.3), np.full((n, plane), 7.0625))
    else:                                   # every value on a coarse or fine edge, lo and hi among them
        (p, a) = (rng.integers(0, n_bin * sub + 1, (n, plane)) / 64.0, rng.integers(0, n_bin + 1, (n, plane)) / 8.0)
    got = joint_histogram(_nchw(p, h, w), _nchw(a, h, w), 0.0, hi, n_bin=n_bin, sub=sub)
    ref = Reference(p, a, 0.0, hi, n_bin, sub)
    _check(field, got, ref, n_bin, sub)
    assert ref.pairs == n * plane and ref.outside.sum() == 0
    if field == "constant":
        assert got[0][56, 58] == n * plane and got[1][0, 56 * 8 + 4] == n * plane
    if field == "edges":
        assert got[0][127].sum() == (a >= 15.875).sum()          # a == hi lands in the last bin


@pytest.mark.parametrize("kinds", [("f4", "f4"), ("f8", "f8"), (">f4", ">f8"), (">f8", ">f4"), ("f4", ">f8")], ids=str)
def test_element_kinds_and_a_second_channel(pattern, kinds):
    (n, h, w, n_bin, sub) = (3, 17, 31, 128, 8)
    rng = np.random.default_rng(23)
    (p, a) = _sprinkle(rng, *_smooth(pattern, rng, n, h * w, 16.0), 16.0, n_bin)
    with np.errstate(over="ignore"):
        (p4, a4) = (_nchw(p, h, w, 2, np.dtype(kinds[0])), _nchw(a, h, w, 2, np.dtype(kinds[1])))      # 1e300 is Inf in fp32
    ops = [device_operand(x) for x in (p4, a4)]
    want = {"f4": _lib.ELEM_F32, "f8": _lib.ELEM_F64, ">f4": _lib.ELEM_F32_BE, ">f8": _lib.ELEM_F64_BE}
    assert [op.kind for op in ops] == [want[k] for k in kinds] and all(op.stride == 2 * h * w for op in ops)
    got = joint_histogram(*ops, 0.0, 16.0, n_bin=n_bin, sub=sub)
    _check(f"kinds {kinds}", got, Reference(channel0(p4), channel0(a4), 0.0, 16.0, n_bin, sub), n_bin, sub)


@pytest.mark.parametrize("offsets", [(1, 1), (1, 3), (2, 0), (3, 3)], ids=str)
def test_misaligned_device_tensors(pattern, offsets):
    """fp32 tensors that start 4, 8 or 12 bytes after a 16-byte boundary, with a case stride that is no multiple of 16 bytes:
    heads of 0 to 3 elements, and with (1, 3) no common 16-byte phase at all"""
    (n, h, w, n_bin, sub) = (5, 1, 4099, 128, 8)
    rng = np.random.default_rng(29)
    (p, a) = _sprinkle(rng, *_smooth(pattern, rng, n, h * w, 16.0), 16.0, n_bin)
    with np.errstate(over="ignore"):
        (p4, a4) = (_nchw(p, h, w, 2, np.float32), _nchw(a, h, w, 2, np.float32))
    tensors = []
    for (x, off) in ((p4, offsets[0]), (a4, offsets[1])):
        flat = torch.empty(x.size + off, dtype=torch.float32, device="cuda")
        flat[off:] = torch.from_numpy(x.reshape(-1)).cuda()
        t = flat[off:].view(x.shape)
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
        tensors.append(t)
    got = joint_histogram(*tensors, 0.0, 16.0, n_bin=n_bin, sub=sub)
    _check(f"offsets {offsets}", got, Reference(channel0(p4), channel0(a4), 0.0, 16.0, n_bin, sub), n_bin, sub)


def _raw(p, a, n, plane, lo, hi, n_bin, sub, fill=0x5A):
    """cae_joint_hist itself on output buffers filled with garbage; returns (code, joint, marg, cond, outside) as numpy"""
    lib = _lib.load()
    dev = p.tensor.device
    outs = [torch.full((n_bin, n_bin), fill, dtype=torch.int64, device=dev), torch.full((2, n_bin * sub), -fill, dtype=torch.int64, device=dev),
            torch.full((2, n_bin, 4), -7.0, dtype=torch.float64, device=dev), torch.full((4,), fill, dtype=torch.int64, device=dev)]
    need = int(lib.cae_joint_hist_workspace_bytes(n, plane, n_bin, sub))
    ws = torch.full((max(need, 8),), 0xFF, dtype=torch.uint8, device=dev)     # NaN bits: a partial read before it is written shows
    rc = lib.cae_joint_hist(*p.args(), *a.args(), n, plane, lo, hi, n_bin, sub, *(o.data_ptr() for o in outs), ws.data_ptr(), need,
                            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(o.cpu().numpy() for o in outs)


def test_two_runs_garbage_and_empty_calls(pattern):
    (n, plane, n_bin, sub) = (17, 4099, 7, 32)
    rng = np.random.default_rng(31)
    (p, a) = _sprinkle(rng, *_smooth(pattern, rng, n, plane, 0.875), 0.875, n_bin)
    (pd, ad) = (device_operand(_nchw(p, 1, plane)), device_operand(_nchw(a, 1, plane)))
    first = _raw(pd, ad, n, plane, 0.0, 0.875, n_bin, sub)
    second = _raw(pd, ad, n, plane, 0.0, 0.875, n_bin, sub, fill=0x33)
    assert first[0] == 0 and second[0] == 0
    for (x, y) in zip(first[1:], second[1:]):
        assert x.tobytes() == y.tobytes()                       # the same bits, whatever the buffers held
    _check("over garbage", first[1:], Reference(p, a, 0.0, 0.875, n_bin, sub), n_bin, sub)
    wrapped = joint_histogram(pd, ad, 0.0, 0.875, n_bin=n_bin, sub=sub)
    for (x, y) in zip(first[1:], wrapped):
        assert x.tobytes() == y.tobytes()
    # no case, or no pixel: zeros over the garbage
    for (nn, pl) in ((0, plane), (n, 0), (0, 0)):
        got = _raw(pd, ad, nn, pl, 0.0, 0.875, n_bin, sub)
        assert got[0] == 0 and all(not x.any() for x in got[1:])
    empty = joint_histogram(np.zeros((0, 1, 4, 4)), np.zeros((0, 2, 4, 4)), 0.0, 1.0, n_bin=4, sub=2)
    assert [x.shape for x in empty] == [(4, 4), (2, 8), (2, 4, 4), (4,)] and all(not x.any() for x in empty)
    assert all(not x.any() for x in joint_histogram(np.zeros((3, 1, 0, 5)), np.zeros((3, 1, 0, 5)), 0.0, 1.0))
    # a refused call writes nothing
    lib = _lib.load()
    for bad in (dict(n_bin=129), dict(sub=0), dict(hi=0.0), dict(hi=float("nan"))):
        args = dict(lo=0.0, hi=0.875, n_bin=n_bin, sub=sub)
        args.update(bad)
        (nb, sb) = (min(args["n_bin"], 128), max(args["sub"], 1))
        dev = pd.tensor.device
        outs = [torch.full((nb * nb,), 5, dtype=torch.int64, device=dev), torch.full((2 * nb * sb,), 5, dtype=torch.int64, device=dev),
                torch.full((2 * nb * 4,), 5.0, dtype=torch.float64, device=dev), torch.full((4,), 5, dtype=torch.int64, device=dev)]
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        rc = lib.cae_joint_hist(*pd.args(), *ad.args(), n, plane, args["lo"], args["hi"], args["n_bin"], args["sub"],
                                *(o.data_ptr() for o in outs), ws.data_ptr(), 1 << 20, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert rc == ERR_ARG and lib.cae_last_error().decode().startswith("cae_joint_hist: "), bad
        assert all(bool((o == 5).all()) for o in outs), bad


def test_argument_errors_name_the_function():
    (x, y) = (np.zeros((2, 1, 4, 4), dtype=np.float32), np.zeros((2, 1, 4, 5), dtype=np.float32))
    for (args, kw) in (((x, y, 0.0, 1.0), {}), ((x, x[:1], 0.0, 1.0), {}), ((x, x, 1.0, 1.0), {}), ((x, x, 0.0, float("inf")), {}),
                       ((x, x, 0.0, 1.0), dict(n_bin=0)), ((x, x, 0.0, 1.0), dict(n_bin=129)), ((x, x, 0.0, 1.0), dict(sub=33)),
                       ((x, x, 0.0, 1.0), dict(n_bin=2.5)), ((x[0], x[0], 0.0, 1.0), {})):
        with pytest.raises(ValueError, match="joint_histogram: "):
            joint_histogram(*args, **kw)


# ---- train_cae -> distribution ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("distribution")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def test_train_distribution(data):
    from cae_tools_amd.cli import distribution as cli, train_cae
    from cae_tools_amd.utils import distribution
    (root, paths) = data
    model = str(root / "model")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
    out = str(root / "report")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", paths["test"], "--model-folder", model, "--output-html-folder", out, "--distribution-bins", "32"])
    assert sorted(f for f in os.listdir(out) if f.startswith("distribution")) == ["distribution", "distribution_test.json"]
    with open(os.path.join(out, "distribution_test.json")) as f:
        rec = json.load(f, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert rec["pairs"] == 12 * 256 * 256 and rec["pixels_left_out"] == 0 and (rec["n_bin"], rec["sub"]) == (32, 8)
    joint = np.asarray(rec["joint"])
    assert joint.shape == (32, 32) and joint.sum() == rec["pairs"]
    assert np.array_equal(joint.sum(axis=1), np.asarray(rec["marginal_target"]).reshape(32, 8).sum(axis=1))
    assert np.array_equal(joint.sum(axis=0), np.asarray(rec["marginal_prediction"]).reshape(32, 8).sum(axis=1))
    # the range is that of target and prediction: nothing outside, both ends occupied
    assert sum(rec["outside"].values()) == 0
    assert (joint.sum(axis=1) + joint.sum(axis=0))[0] > 0 and (joint.sum(axis=1) + joint.sum(axis=0))[-1] > 0
    for t in rec["exceedance"]:
        assert t["hits"] + t["misses"] + t["false_alarms"] + t["correct_negatives"] == rec["pairs"]
    w = (rec["hi"] - rec["lo"]) / 256       # a quantile lies in the fine bin of its sample, and the target in [288, 298]
    assert rec["quantile_target"] == sorted(rec["quantile_target"])
    assert 288.0 - w <= rec["quantile_target"][0] and rec["quantile_target"][-1] <= 298.0 + w
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("distribution ")]
    assert len(lines) == 1 and lines[0].startswith("distribution test: slope ") and "POD/FAR at q95 " in lines[0]
    with open(os.path.join(out, "distribution", "index.html")) as f:
        page = f.read()
    assert page.count('alt="test joint density"') == 1 and page.count('alt="test Q-Q"') == 1
    with open(os.path.join(out, "index.html")) as f:
        report = f.read()
    assert report.count("<h2>Value distribution</h2>") == 1 and '<a href="distribution/index.html">' in report
    assert f"test: {rec['pairs']} pixel pairs, 32 bins over" in report
    assert f"<td>{distribution._shown(rec['summary']['perkins_score'])}</td>" in report
