"""The Linear engine's three GEMMs (include/cae_linear.h: OpGemm / k_igemm / gemm_launch of csrc/kernels_unet_mfma.h) at every
tile shape and K split, against oracle/linear_oracle.py in fp64, by the project's fp64-anchored criterion: the HIP result may
be no further from the fp64 answer than 3x the fp32 CPU oracle's own distance, plus the floors of
helpers.assert_close_as_reference (1e-5 of the tensor's scale + 1e-9).  The geometries (tests/linear_shapes.py) are the
smallest that reach each branch; every test asserts the launch plan of its engine (LinearPlan.kernel_plan) before it runs
anything, so a case that stops reaching its branch fails instead of passing for nothing.

  r32_split      1089 -> 30   32x512 tile (one weight quad per thread, guarded), 5 K slices, the last of 5 chunks whose last
                              holds 1 element; a second column tile at batch 520
  r64_split      1083 -> 56   64x256 tile, K = 3 mod 4, 5 slices; a second column tile at batch 257
  r128_ragged    1089 -> 143  128x128 tiles, two row tiles (128 + 15), 5 slices; a second column tile at batch 129
  edge_1008/9    -> 385       63 chunks: the last K that is not split; 64: the first that is (4 slices), four row tiles
  tiny_k1/k3     1, 3 -> 1    K < 4, a single output
  wide_nosplit   256 -> 4096  32 row tiles, the usual user shape scaled down

Weights are initialised as models/linear.py does under a fixed seed; x and t are uniform in [0, 1) as the normalised data are.
The Linear engine has no load_optimizer_state: the Adam test copies the fp32 oracle's moments into the engine's exp_avg /
exp_avg_sq arenas (parameter-arena layout) and calls set_step, which is what such a method would do.

The Adam criterion carries a floor from a second fp32 CPU evaluation (_SequentialOracle: the same products, summed one after
another in ascending k as the tile engine's K loop does, instead of in the blocked order of the CPU BLAS).  Why: Adam's first
steps move a weight by lr g / (|g| + eps), so where a gradient element lies within eps = 1e-8 of zero a forward rounding error
of 1e-10 in g moves the update by 1e-2 lr, and the worst such element of a 385 x 1008 weight decides the max norm.  The BLAS
forward at K = 1008 is three times more exact than any one-after-another fp32 sum (score of edge_1008: 3.8e-7 against 1.1e-6
for the unsplit HIP forward, 4.0e-7 for the split one at K = 1009), so 3x its own update error is no measure of fp32 rounding
there.  Measured for edge_1008 batch 4, step 0, linear.1.weight, lr 1e-3: |hip - fp64| 3.99e-5, the BLAS oracle's own 6.9e-6,
the sequential fp32 CPU evaluation's own 3.2e-5 (edge_1009: 5.7e-6 / 8.3e-6)."""
import functools

import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference
from linear_shapes import CASES, PLANS, SPLIT_CASES

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 1e-5
CASE_BATCHES = [(n, b) for n, (_, _, bs) in CASES.items() for b in bs]
_IDS = [f"{n}-b{b}" for (n, b) in CASE_BATCHES]


@pytest.fixture(autouse=True)
def _one_thread():
    """the fp32 CPU oracle sums in one fixed order"""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(initial state dict, data set 0 (x, t), data set 1 (x, t), a permutation of each) - shared, never modified"""
    from cae_tools_amd.models.linear import Linear
    (in_shape, out_shape, batches) = CASES[name]
    seed = 100 + list(CASES).index(name)
    torch.manual_seed(seed)
    state = {k: v.clone() for k, v in Linear(in_shape, out_shape).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 50)
    (n0, n1) = (2 * max(batches) + 3, max(batches) + 5)
    d0 = (torch.rand((n0,) + in_shape, generator=g), torch.rand((n0,) + out_shape, generator=g))
    d1 = (torch.rand((n1,) + in_shape, generator=g), torch.rand((n1,) + out_shape, generator=g))
    perms = (torch.randperm(n0, generator=g), torch.randperm(n1, generator=g))
    assert all(not torch.equal(p, torch.arange(len(p))) for p in perms)
    return state, d0, d1, perms


def _engine(name, batch=None):
    """a fresh engine on the case's weights and data sets, its plan checked against the pinned one"""
    from cae_tools_amd.linear_engine import LinearEngine
    (in_shape, out_shape, batches) = CASES[name]
    (state, d0, d1, _) = _case(name)
    eng = LinearEngine(in_shape, out_shape, max_batch=max(batches), device="cuda:0")
    for b in (batches if batch is None else (batch,)):
        assert eng.kernel_plan(b, True) == PLANS[(name, b)], f"{name} batch {b}: the launch plan changed"
    eng.load_state(state)
    eng.set_hyper(lr=LR, weight_decay=WD)
    eng.set_dataset(0, *d0)
    eng.set_dataset(1, *d1)
    return eng


def _oracles(name, state=None):
    """(fp32 oracle, fp64 oracle) from the same weights"""
    from oracle.linear_oracle import LinearOracle
    (in_shape, out_shape, _) = CASES[name]
    state = _case(name)[0] if state is None else state
    return (LinearOracle(in_shape, out_shape, state, lr=LR, weight_decay=WD),
            LinearOracle(in_shape, out_shape, {k: v.double() for k, v in state.items()}, lr=LR, weight_decay=WD))


def _sequential_oracle(name, state):
    """the fp32 oracle with its forward's products summed one after another in ascending k (fp32, one thread)"""
    from oracle.linear_oracle import LinearOracle

    class _SequentialOracle(LinearOracle):
        def forward(self, x):
            (x, w) = (x.flatten(1), self.p["linear.1.weight"])
            y = self.p["linear.1.bias"].expand(x.shape[0], -1)
            for k in range(x.shape[1]):
                y = y + x[:, k:k + 1] * w[:, k][None, :]
            return y.view((x.shape[0],) + self.out_shape)

    (in_shape, out_shape, _) = CASES[name]
    return _SequentialOracle(in_shape, out_shape, state, lr=LR, weight_decay=WD)


def _flat(sd):
    """parameter-arena layout: [weight (nout, nin) row-major, bias]"""
    return torch.cat([sd["linear.1.weight"].reshape(-1), sd["linear.1.bias"].reshape(-1)])


def _check_loss(got, l32, l64, what):
    """no further from fp64 than 3x the fp32 oracle's own distance + 2e-6 relative"""
    bound = 3.0 * abs(l32 - l64) + 2e-6 * abs(l64)
    print(f"{what}: loss |hip - fp64| {abs(got - l64):.3e}, the fp32 oracle's own {abs(l32 - l64):.3e}, bound {bound:.3e}")
    assert abs(got - l64) <= bound, f"{what}: loss {got!r}, fp64 {l64!r}, fp32 oracle {l32!r}"


def _check_grads(eng, flat, o32, o64, what):
    nw = eng.nout * eng.nin
    flat = flat.detach().cpu().double().numpy()
    (g32, g64) = (o32.grads(), o64.grads())
    for (key, got) in (("linear.1.weight", flat[:nw]), ("linear.1.bias", flat[nw:])):
        (r32, r64) = (g32[key].numpy().reshape(-1), g64[key].numpy().reshape(-1))
        (err, ref) = (np.abs(got - r64).max(), np.abs(r32.astype(np.float64) - r64).max())
        bound = 3.0 * ref + 1e-5 * np.abs(r64).max() + 1e-9
        print(f"{what} grad {key}: |hip - fp64| {err:.3e}, the fp32 oracle's own {ref:.3e}, ratio to the bound {err / bound:.3f}")
        assert_close_as_reference(got, r32, r64, f"{what} grad {key}")


def _rows(data, perm, start, batch):
    idx = torch.arange(start, start + batch) if perm is None else perm[start:start + batch]
    return data[0][idx], data[1][idx]


@pytest.mark.parametrize("name,batch", CASE_BATCHES, ids=_IDS)
def test_score_loss_and_gradients(name, batch):
    """score (and, at the case's largest batch, max_batch + 1 rows through the chunking), the loss and both gradient tensors of
    forward_backward on rows [0, batch) of data set 0"""
    eng = _engine(name, batch)
    (_, d0, _, _) = _case(name)
    (o32, o64) = _oracles(name)
    rows = batch if batch < eng.max_batch else eng.max_batch + 1
    x = d0[0][:rows]
    got = eng.score(x).cpu().numpy()
    (y32, y64) = (o32.eval_forward(x).numpy(), o64.eval_forward(x.double()).numpy())
    err, ref = np.abs(got - y64).max(), np.abs(y32 - y64).max()
    print(f"{name} b{batch} score of {rows} rows: |hip - fp64| {err:.3e}, the fp32 oracle's own {ref:.3e}, "
          f"ratio to the bound {err / (3 * ref + 1e-5 * np.abs(y64).max() + 1e-9):.3f}")
    assert_close_as_reference(got, y32, y64, f"{name} b{batch} score")
    (xb, tb) = _rows(d0, None, 0, batch)
    (l32, l64) = (o32.loss_and_grads(xb, tb), o64.loss_and_grads(xb.double(), tb.double()))
    g = eng.forward_backward(0, None, 0, batch, slot=1)
    _check_loss(eng.read_losses(1, 1)[0], l32, l64, f"{name} b{batch}")
    _check_grads(eng, g, o32, o64, f"{name} b{batch}")
    eng.close()


@pytest.mark.parametrize("name,batch", CASE_BATCHES, ids=_IDS)
def test_steps_through_a_device_permutation(name, batch):
    """eval losses of an epoch over data set 0 (run_batches: batches of `batch`, the last one partial) and of data set 1 from a
    non-zero start (eval_step), and the gradient of a training batch from a non-zero start, all gathered through a permutation"""
    eng = _engine(name, batch)
    (_, d0, d1, perms) = _case(name)
    (o32, o64) = _oracles(name)
    (p0, p1) = (eng.upload_perm(perms[0].numpy()), eng.upload_perm(perms[1].numpy()))
    n = batch + max(1, batch // 3)
    got = eng.run_batches(0, p0, n, batch, train=False)
    assert len(got) == 2
    for (k, (lo, size)) in enumerate(((0, batch), (batch, n - batch))):
        (xb, tb) = _rows(d0, perms[0], lo, size)
        _check_loss(got[k], o32.eval_loss(xb, tb), o64.eval_loss(xb.double(), tb.double()), f"{name} b{batch} set 0 rows {lo}+{size}")
    eng.eval_step(1, p1, 3, batch, slot=5)
    (xb, tb) = _rows(d1, perms[1], 3, batch)
    _check_loss(eng.read_losses(5, 1)[0], o32.eval_loss(xb, tb), o64.eval_loss(xb.double(), tb.double()), f"{name} b{batch} set 1 from 3")
    g = eng.forward_backward(1, p1, 2, batch, slot=6)
    (xb, tb) = _rows(d1, perms[1], 2, batch)
    (l32, l64) = (o32.loss_and_grads(xb, tb), o64.loss_and_grads(xb.double(), tb.double()))
    _check_loss(eng.read_losses(6, 1)[0], l32, l64, f"{name} b{batch} set 1 from 2 (train)")
    _check_grads(eng, g, o32, o64, f"{name} b{batch} permuted")
    eng.close()


def _moments(orc):
    """[(exp_avg, exp_avg_sq)] per parameter in arena order, or None before the first step"""
    st = [orc.optim.state.get(p) for p in orc.p.values()]
    return None if not st[0] else [(s["exp_avg"].detach().clone(), s["exp_avg_sq"].detach().clone()) for s in st]


@pytest.mark.parametrize("name,batch", CASE_BATCHES, ids=_IDS)
def test_adam_steps_no_further_from_fp64_than_the_oracle(name, batch):
    """three train_steps through a permutation; before each, the engine and a fresh fp64 oracle take the fp32 oracle's weights,
    moments and step count.  Per tensor |hip update - fp64 update| <= 3 |fp32 update - fp64 update| + 1e-3 lr (the criterion of
    test_adam_step_no_further_from_fp64_than_the_reference, tests/test_hip_parity.py) + the floor: the own distance from fp64
    of a second fp32 CPU evaluation that sums the forward's products one after another (module docstring)."""
    from oracle.linear_oracle import LinearOracle
    eng = _engine(name, batch)
    (in_shape, out_shape, _) = CASES[name]
    (_, d0, _, perms) = _case(name)
    (o32, _) = _oracles(name)
    p0 = eng.upload_perm(perms[0].numpy())
    nw = eng.nout * eng.nin
    worst = 0.0
    for s in range(3):
        before = o32.state()
        mom = _moments(o32)
        eng.load_state(before)
        eng.sync()
        if mom is None:
            eng.reset_optimizer()
        else:
            eng.exp_avg.copy_(torch.cat([m.reshape(-1) for (m, _) in mom]))
            eng.exp_avg_sq.copy_(torch.cat([v.reshape(-1) for (_, v) in mom]))
            torch.cuda.synchronize()
            eng.set_step(s)
        o64 = LinearOracle(in_shape, out_shape, {k: v.double() for k, v in before.items()}, lr=LR, weight_decay=WD)
        seq = _sequential_oracle(name, before)
        if mom is not None:
            for (o, cast) in ((o64, torch.Tensor.double), (seq, torch.Tensor.float)):
                for (p, (m, v)) in zip(o.p.values(), mom):
                    o.optim.state[p] = {"step": torch.tensor(float(s)), "exp_avg": cast(m).clone(), "exp_avg_sq": cast(v).clone()}
        start = 1 + s * (batch // 2)
        (xb, tb) = _rows(d0, perms[0], start, batch)
        o32.train_step(xb, tb)
        o64.train_step(xb.double(), tb.double())
        seq.train_step(xb, tb)
        eng.train_step(0, p0, start, batch, slot=s)
        (a32, a64, aseq, hip) = (o32.state(), o64.state(), seq.state(), eng.export_state())
        for key in a32:
            b0 = before[key].numpy().astype(np.float64)
            d64 = a64[key].numpy() - b0
            d32 = a32[key].numpy().astype(np.float64) - b0
            dh = hip[key].numpy().astype(np.float64) - b0
            (err_ref, err_hip) = (float(np.abs(d32 - d64).max()), float(np.abs(dh - d64).max()))
            floor = float(np.abs(aseq[key].numpy().astype(np.float64) - b0 - d64).max())
            bound = 3.0 * err_ref + 1e-3 * LR + floor
            worst = max(worst, err_hip / bound)
            print(f"{name} b{batch} step {s} {key}: |hip - fp64| {err_hip:.3e}, the fp32 oracle's own {err_ref:.3e}, "
                  f"the sequential fp32 evaluation's own {floor:.3e}")
            assert err_hip <= bound, (f"{name} b{batch} step {s} {key}: |hip - fp64| = {err_hip:.3e}, the fp32 oracle's own "
                                      f"{err_ref:.3e}, the sequential fp32 evaluation's own {floor:.3e} (lr {LR:g})")
    print(f"{name} b{batch}: Adam worst ratio to the bound {worst:.3f}")
    assert nw + eng.nout == eng.n_param
    eng.close()


@pytest.mark.parametrize("name,batch", [(n, b) for (n, b) in CASE_BATCHES if n in ("r32_split", "r128_ragged")],
                         ids=[i for i, (n, _) in zip(_IDS, CASE_BATCHES) if n in ("r32_split", "r128_ragged")])
def test_gradient_accumulator_is_never_stale(name, batch):
    """fb, fb, train_step, fb, apply_gradients(the previous gradient), fb, eval_step, fb: the fp64 accumulator the weight-gradient
    GEMM and k_col_sums add into is cleared before every one of them (by the Adam kernel, or by a memset when no optimiser step
    came between).  The two leading gradients are the same bits; every later one meets the gradient criterion against oracles
    that took the same two updates."""
    eng = _engine(name, batch)
    (_, d0, d1, _) = _case(name)
    (o32, o64) = _oracles(name)
    (xb, tb) = _rows(d0, None, 0, batch)
    nw = eng.nout * eng.nin

    def fb(what, same_weights=False):
        g = eng.forward_backward(0, None, 0, batch, slot=2).clone()
        (l32, l64) = (o32.loss_and_grads(xb, tb), o64.loss_and_grads(xb.double(), tb.double()))
        got = eng.read_losses(2, 1)[0]
        if same_weights:    # after an update the three sets of weights differ by Adam's own rounding: the gradients are held
            _check_loss(got, l32, l64, f"{name} b{batch} {what}")                # to their criterion, the loss is printed
        else:
            print(f"{name} b{batch} {what}: loss {got!r}, fp64 {l64!r}, fp32 oracle {l32!r}")
        _check_grads(eng, g, o32, o64, f"{name} b{batch} {what}")
        return g

    (g1, g2) = (fb("first", True), fb("second", True))
    assert torch.equal(g1, g2), f"{int((g1 != g2).sum())} of {g1.numel()} gradient entries differ between two calls in a row"
    eng.train_step(0, None, 0, batch, slot=3)
    o32.train_step(xb, tb)
    o64.train_step(xb.double(), tb.double())
    g3 = fb("after train_step")
    eng.apply_gradients(g3)
    for o in (o32, o64):
        (w, b) = (o.p["linear.1.weight"], o.p["linear.1.bias"])
        w.grad = g3[:nw].cpu().view_as(w).to(w.dtype)
        b.grad = g3[nw:].cpu().to(b.dtype)
        o.optim.step()
    fb("after apply_gradients")
    eng.eval_step(1, None, 1, batch, slot=4)
    fb("after eval_step")
    eng.close()


@pytest.mark.parametrize("batch", CASES["r64_split"][2])
def test_shard_gradients_sum_to_the_full_batch(batch):
    """what two ranks hand to the all-reduce: forward_backward on the two row halves with global_batch = the whole; their sum
    (fp64, on the host) against the full-batch gradient of the oracles"""
    name = "r64_split"
    eng = _engine(name, batch)
    (_, d0, _, _) = _case(name)
    (o32, o64) = _oracles(name)
    half = batch // 2
    total = torch.zeros(eng.n_param, dtype=torch.float64)
    for (lo, size) in ((0, half), (half, batch - half)):
        total += eng.forward_backward(0, None, lo, size, slot=1, global_batch=batch).cpu().double()
    (xb, tb) = _rows(d0, None, 0, batch)
    o32.loss_and_grads(xb, tb)
    o64.loss_and_grads(xb.double(), tb.double())
    _check_grads(eng, total, o32, o64, f"{name} b{batch} two shards")
    eng.close()


@pytest.mark.parametrize("name,batch", [("r32_split", 3), ("r64_split", 5), ("r128_ragged", 2), ("tiny_k3", 1)])
def test_a_step_reads_nothing_it_did_not_write(name, batch):
    """batches that are no multiple of 4, below max_batch: the K quads of the weight-gradient GEMM (K = batch) reach past the
    batch's rows of the loss gradient and of the gathered input.  With every byte of the workspace set to 0xFF (NaN as fp32 and
    as fp64) before the first step, score, loss and gradient are the bits of an engine whose workspace started as zeros."""
    runs = []
    for poison in (False, True):
        eng = _engine(name, batch)
        if poison:
            eng.sync()
            eng.workspace.fill_(0xFF)
            torch.cuda.synchronize()
        y = eng.score(_case(name)[1][0][:batch]).cpu()
        g = eng.forward_backward(0, None, 0, batch, slot=1).cpu()
        runs.append((y, g, eng.read_losses(1, 1)[0]))
        eng.close()
    ((y0, g0, l0), (y1, g1, l1)) = runs
    assert bool(torch.isfinite(y1).all()) and bool(torch.isfinite(g1).all()) and np.isfinite(l1)
    assert torch.equal(y0, y1) and torch.equal(g0, g1) and l0 == l1


def _three_steps(name, batch):
    eng = _engine(name, batch)
    p0 = eng.upload_perm(_case(name)[3][0].numpy())
    for k in range(3):
        eng.train_step(0, p0, k * batch // 2, batch, slot=k)
    eng.eval_step(1, None, 0, batch, slot=3)
    losses = eng.read_losses(0, 4)
    eng.sync()
    out = (losses, [("params", eng.params.cpu()), ("exp_avg", eng.exp_avg.cpu()), ("exp_avg_sq", eng.exp_avg_sq.cpu())])
    eng.close()
    return out


@pytest.mark.parametrize("name,batch", [(n, b) for (n, b) in CASE_BATCHES if n in SPLIT_CASES],
                         ids=[i for i, (n, _) in zip(_IDS, CASE_BATCHES) if n in SPLIT_CASES])
def test_split_k_steps_are_bitwise_reproducible(name, batch):
    """two fresh engines, the same three training steps and an eval step with the forward's K split (partial tiles folded in
    slice order by k_gemm_finish): the same bits in every loss, parameter and Adam moment"""
    assert int(PLANS[(name, batch)]["fwd"]["slices"]) > 1
    ((la, ta), (lb, tb)) = (_three_steps(name, batch), _three_steps(name, batch))
    for i, (u, v) in enumerate(zip(la, lb)):
        assert u == v, f"{name} b{batch}: loss {i} differs: {u!r} != {v!r}"
    for (what, u), (_, v) in zip(ta, tb):
        assert torch.equal(u, v), f"{name} b{batch}: {what} differ in {int((u != v).sum())} of {u.numel()} entries"
