"""tests/optim_ref.py against itself and against torch, without a GPU: the numpy fp64 formulas are torch's, the fp32 reference
is inside its own bound, the value regimes cover every arena, and the criterion sees a bias of 1.3e-5 of an update - the
one `1.f - (float)beta2` carries, which k_adamw had and k_adam / k_adam_l2 never did."""
import numpy as np
import pytest

import optim_ref as R

N = 6 * 512
SEED = 20

# the way k_adamw forms 1 - beta (kernels_unet.h adamw_one / AdamwConsts): on the host in fp64, rounded once - as k_adam and
# k_adam_l2 do.  "from_rounded_beta", 1.f - (float)beta, is what it did before tests/test_optim_elementwise_gpu.py existed.
K_ADAMW_ONE_MINUS_BETA = "rounded_once"


@pytest.fixture(scope="module")
def arena():
    return R.regimes(N, SEED)


@pytest.fixture(scope="module")
def steps(arena):
    """{(kind, hyper set, t): (fp32 torch step, fp64 numpy step)}, computed once"""
    (_, p, g, m, v) = arena
    out = {}
    for kind in ("adam", "adamw"):
        for (name, t) in R.CASES:
            h = R.HYPERS[name][0]
            out[(kind, name, t)] = (R.torch_step(kind, "float32", p, g, m, v, t, **h), R.F64[kind](p, g, m, v, t, **h))
    return out


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_numpy_formulas_are_torch_in_fp64(arena, steps, kind):
    (regime, p, g, m, v) = arena
    for (name, t) in R.CASES:
        ref = R.torch_step(kind, "float64", p, g, m, v, t, **R.HYPERS[name][0])
        ours = steps[(kind, name, t)][1]
        for r, rname in enumerate(R.REGIMES):
            mask = regime == r
            for q, a, b in zip(R.QUANTITIES, ours, ref):
                (a, b) = (a[mask], b[mask])
                assert np.all(np.isfinite(a))
                assert float(np.abs(a - b).max()) <= 1e-14 * float(np.abs(b).max()), (kind, name, t, rname, q)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_the_reference_is_inside_its_own_bound(arena, steps, kind):
    (regime, p, *_) = arena
    for (name, t) in R.CASES:
        (ref32, ref64) = steps[(kind, name, t)]
        ratios = R.check_step(ref32, ref32, ref64, regime, p, f"torch fp32 {kind}, {name}, t={t}", limit=1.0 / 3.0)
        assert len(ratios) == len(R.REGIMES) * len(R.QUANTITIES)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_the_criterion_sees_one_minus_a_rounded_beta(arena, steps, kind):
    """1.f - (float)0.999 is 1.3e-5 short of 0.001: every exp_avg_sq, and through it every update, moves the same way.  Where
    the state is zero nothing masks it."""
    (regime, p, g, m, v) = arena
    for t in (1, 10, 1000):
        h = R.HYPERS["default"][0]
        (ref32, ref64) = steps[(kind, "default", t)]
        good = R.emulate_f32(kind, "rounded_once", p, g, m, v, t, **h)
        ratios = R.check_step(good, ref32, ref64, regime, p, f"emulated {kind}, (float)(1 - beta), t={t}")
        bad = R.emulate_f32(kind, "from_rounded_beta", p, g, m, v, t, **h)
        with pytest.raises(AssertionError, match="zero_state, exp_avg_sq"):
            R.check_step(bad, ref32, ref64, regime, p, f"emulated {kind}, 1.f - (float)beta, t={t}")
        zero = regime == R.REGIMES.index("zero_state")
        worse = R.criterion(bad, ref32, ref64, zero, p)
        print(f"{kind} t={t} zero_state: (float)(1 - beta) {ratios[('zero_state', 'exp_avg_sq')]:.2f} / "
              f"{ratios[('zero_state', 'update')]:.2f}, 1.f - (float)beta {worse['exp_avg_sq'][0]:.1f} / {worse['update'][0]:.1f}"
              " of the bound on exp_avg_sq / the update")
        assert worse["exp_avg_sq"][0] > 3.0 and worse["update"][0] > 1.0
    assert K_ADAMW_ONE_MINUS_BETA == "rounded_once"


def test_every_case_passes_with_the_kernels_formula(arena, steps):
    """the emulation of what the kernels compute meets the criterion at every hyper set and step: a GPU failure is the kernel's"""
    (regime, p, g, m, v) = arena
    for kind in ("adam", "adamw"):
        for (name, t) in R.CASES:
            (ref32, ref64) = steps[(kind, name, t)]
            got = R.emulate_f32(kind, K_ADAMW_ONE_MINUS_BETA, p, g, m, v, t, **R.HYPERS[name][0])
            R.check_step(got, ref32, ref64, regime, p, f"emulated {kind}, {name}, t={t}")


def test_a_failure_names_the_place(arena, steps):
    (regime, p, g, m, v) = arena
    (ref32, ref64) = steps[("adam", "strong", 7)]
    got = [a.copy() for a in ref32]
    got[1][7] *= 1.001
    names = lambda i: f"tensor-{i // 100}"
    with pytest.raises(AssertionError, match=r"somewhere, strong, t=7, zero_state, exp_avg: .* arena index 7 \(tensor-0\)"):
        R.check_step(got, ref32, ref64, regime, p, "somewhere, strong, t=7", names)
    got[1][7] = np.nan
    with pytest.raises(AssertionError, match="zero_state, exp_avg: inf"):
        R.check_step(got, ref32, ref64, regime, p, "x")


def test_the_unet_arena_gives_k_adamw_whole_groups_only():
    """k_adamw updates four parameters per thread and keeps an element-wise path for a last group cut by n_param, for a group that
    straddles the edge of an fp32 gradient range (F32Ranges) and for a range that starts off a 16-byte boundary.  No engine can
    reach them: the tensor table starts every tensor at a multiple of four elements and closes the arena on one
    (engine_host.h TensorTable::reserve / close), and only a Linear layer with nin % 4 == nout % 4 == 0 stores fp32 gradients
    (unet_engine.hip lin_big).  Whatever fc and latent size: here over a sweep, with odd sizes of both."""
    from cae_tools_amd.models.unet import unet_layer_spec
    from cae_tools_amd.unet_engine import UnetPlan
    seen = set()
    for (chans, size) in (([8, 8], (24, 40)), ([8, 36], (24, 24)), ([16, 34], (20, 28))):
        spec = unet_layer_spec(1, 1, size, chans)
        for fc in (5, 7, 8, 1030, 1092):
            for latent in (3, 4, 5):
                plan = UnetPlan(spec, fc, latent, 2)
                try:
                    assert plan.n_param % 4 == 0
                    assert all(off % 4 == 0 for (arena, off, _, _) in plan.tensors.values() if arena == 0)
                    kinds = {k: f["bwd"] for k, f in plan.kernel_plan(2, True).items() if k.startswith("fc")}
                    for k, kind in kinds.items():
                        if kind == "lin_big":
                            name = {"fc0": "enc/encoder_lin.0", "fc1": "enc/encoder_lin.4", "fc2": "dec/decoder_lin.0",
                                    "fc3": "dec/decoder_lin.4"}[k] + ".weight"
                            assert plan.tensors[name][2] % 4 == 0, (name, plan.tensors[name])
                    seen |= set(kinds.values())
                    unpadded = sum(numel for (arena, _, numel, _) in plan.tensors.values() if arena == 0)
                    seen.add("padded" if unpadded != plan.n_param else "dense")
                finally:
                    plan.close()
    assert {"lin_big", "padded"} <= seen, seen


@pytest.mark.parametrize("n", [64, 65, 71, 903, 4099])
def test_regimes_cover_every_arena(n):
    (regime, p, g, m, v) = R.regimes(n, 3)
    again = R.regimes(n, 3)
    for a, b in zip((regime, p, g, m, v), again):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert all(a.dtype == np.float32 and a.shape == (n,) for a in (p, g, m, v))
    for r, name in enumerate(R.REGIMES):
        assert int((regime == r).sum()) * 8 >= n, name
    for lo in range(0, n - 5, 4):                      # any six in a row hold all six
        assert len(set(regime[lo:lo + 6].tolist())) == 6
    nz = g[g != 0]
    assert float(np.abs(nz).min()) >= 1e-15 * (1 - 1e-6)
    is_ = lambda name: regime == R.REGIMES.index(name)
    assert not g[is_("no_gradient")].any() and m[is_("no_gradient")].all() and v[is_("no_gradient")].all()
    assert not (p[is_("zero_state")].any() or m[is_("zero_state")].any() or v[is_("zero_state")].any())
    assert float(np.sqrt(v[is_("eps_dominated")]).max()) < 1e-8
    assert float(np.abs(g[is_("large")]).max()) > 1e3 and float(v[is_("large")].max()) > 1e6
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and float(v[v > 0].min()) > 1.2e-38
