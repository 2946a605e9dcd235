"""The ensemble verification end to end on a VarAEModel that is initialised but not trained: VaeEngine.ensemble(target=...),
VarAEModel.verify_ensemble and the verify_ensemble command against the CPU definition - oracle/vae_oracle.py's encoder,
normal_noise and the decoder, fed through tests/ensemble_verify_ref.py.  Geometry 12x12 -> 176x176, latent 4, fc 12, 7 cases,
batch_size 4, K = 2 (two cases per group, a short last group of one), 3 and 9 (below and above the engine's 4 rows).  One
more engine of 70 rows runs groups of 35 and 34 cases, where the library's cut into chunks and its workspace change.

Bounds.  Each GPU member lies within delta = 1e-5 * range of the definition's (the decode bound test_vae_generate_gpu.py
asserts).  Per pixel |dA| <= delta and |dB| <= (1 / K^2) (K (K - 1) / 2) 2 delta <= delta, so S A and S B move by at most
n delta each and a case's crps by at most 2 delta.  |d mbar| <= delta gives |d (mbar - a)^2| <= delta (2 |mbar - a| + delta), and
|d s| <= ds = sqrt(K / (K - 1)) delta (as test_ensemble_apply_matches_the_definition argues) gives |d s^2| <= ds (2 s + ds),
summed over the pixels with the definition's mbar and s.  A pixel can change rank only if a member crosses the target,
which needs |m_k - a| <= delta in the definition's draws; with q such pixels the two histograms differ by at most 2 q in
L1, and q <= 1 % of the pixels keeps that bound from hiding a failure (computed from the definition alone q is 10 and 24
of 216 832 pixels for K = 3 and 9)."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import ensemble_verify_ref as ref
from test_vae_generate_gpu import _data

pytestmark = pytest.mark.gpu

(LATENT, FC, N, SEED) = (4, 12, 7, 21)


class _World:
    """the untrained model, its folder, the definition's copy of its state and the definition's draws, computed once"""

    def __init__(self, tmp):
        from cae_tools_amd.models.ds_dataset import DSDataset
        from cae_tools_amd.models.var_ae_model import VarAEModel
        from oracle import cae_oracle as orc
        from oracle import vae_oracle as vo
        torch.manual_seed(3)
        self.model = VarAEModel(batch_size=4, nr_epochs=1, test_interval=1, fc_size=FC, encoded_dim_size=LATENT)
        self.folder = str(tmp / "model")
        with redirect_stdout(io.StringIO()):
            ds = DSDataset(self.score_ds(), ["lowres"], "hires", normalise_in=True, normalise_out=True)
            self.model.normalisation_parameters = ds.get_normalisation_parameters()
            self.model.set_input_spec(ds.get_input_spec())
            self.model.set_output_spec(ds.get_output_spec())
            (self.model.input_shape, self.model.output_shape) = (tuple(ds.get_input_shape()), tuple(ds.get_output_shape()))
            self.model._build()
            self.eng = self.model._inference_engine(N)
            assert self.eng.max_batch == 4
            self.model.save(self.folder)
        (self.enc, self.dec) = self.eng.export_state()
        self.spec = self.model.spec.save()
        self.x = ds.device_inputs()
        (self.vmin, self.vmax) = self.model.normalisation_parameters[2:4]
        self.range = self.vmax - self.vmin
        self.target = np.asarray(self.score_ds()["hires"].values)
        with torch.no_grad():
            (mu, logvar) = vo.encoder_forward(self.spec, self.enc, self.x.cpu(), train=False)
            (mu, logvar) = (mu.numpy(), logvar.numpy())
            fields = []
            for k in range(9):
                z = mu + vo.normal_noise(SEED, k, (N, LATENT)) * np.exp(np.float32(0.5) * logvar)
                fields.append(orc.decoder_forward(self.spec, self.dec, torch.as_tensor(z.astype(np.float32)), train=False).numpy())
        self.fields = np.stack(fields, axis=1)[:, :, 0].reshape(N, 9, -1)      # (N, 9, plane), channel 0
        self._want = {}

    @staticmethod
    def score_ds():
        return _data(N, 5)

    def want(self, k):
        if k not in self._want:
            self._want[k] = ref.verify(self.fields[:, :k], self.target[:, 0].reshape(N, -1), self.vmin, self.range)
        return self._want[k]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return _World(tmp_path_factory.mktemp("vae_verify"))


def _check_against_the_definition(world, k, sums, ranks):
    (want_sums, want_ranks, terms) = world.want(k)
    plane = world.fields.shape[2]
    delta = 1e-5 * world.range
    ds = np.sqrt(k / (k - 1)) * delta
    assert (sums[:, 0] == plane).all() and (want_sums[:, 0] == plane).all()
    a = world.target[:, 0].reshape(N, -1).astype(np.float64)
    m = ref.members(world.fields[:, :k], world.vmin, world.range)
    for c in range(N):
        bounds = (plane * delta, plane * delta, delta * (2 * np.abs(terms[c]["mbar"] - a[c]).sum() + plane * delta),
                  ds * (2 * np.sqrt(terms[c]["V"]).sum() + plane * ds))
        errors = np.abs(sums[c, 1:] - want_sums[c, 1:])
        print(f"K {k} case {c}: |d SA| {errors[0]:.3e} (bound {bounds[0]:.3e}), |d SB| {errors[1]:.3e} ({bounds[1]:.3e}), "
              f"|d SE| {errors[2]:.3e} ({bounds[2]:.3e}), |d SV| {errors[3]:.3e} ({bounds[3]:.3e})")
        assert (errors <= bounds).all(), (c, errors, bounds)
    crps = (sums[:, 1] - sums[:, 2]) / plane
    want_crps = (want_sums[:, 1] - want_sums[:, 2]) / plane
    print(f"K {k}: max |d crps| {np.abs(crps - want_crps).max():.3e} (bound {2 * delta:.3e}); crps {want_crps}")
    assert (np.abs(crps - want_crps) <= 2 * delta).all()
    q = int((np.abs(m - a[:, None, :]).min(axis=1) <= delta).sum())
    l1 = int(np.abs(ranks[:k + 1] - want_ranks[:k + 1]).sum())
    print(f"K {k}: {q} of {N * plane} pixels have a member within delta of the target; rank histograms differ by {l1} in L1 "
          f"(bound {2 * q}); definition's counts {want_ranks}, largest spread {np.sqrt(max(t['V'].max() for t in terms)):.3e}")
    assert q <= 0.01 * N * plane
    assert l1 <= 2 * q
    assert ranks[:k + 1].sum() == N * plane and (want_ranks[1:k] > 0).all()


@pytest.mark.parametrize("k", [2, 3, 9])
def test_engine_ensemble_with_a_target(world, k):
    eng = world.eng
    (mu, logvar) = eng.encode(world.x)
    keywords = dict(seed=SEED, vmin=world.vmin, vmax=world.vmax)
    (mean, std, sums, ranks) = eng.ensemble(mu, logvar, k, target=world.target, **keywords)
    assert sums.shape == (N, 5) and sums.dtype == np.float64 and ranks.shape == (k + 2,) and ranks.dtype == np.int64
    _check_against_the_definition(world, k, sums, ranks)
    # without a target: two tensors as ever.  The path that makes them is the one apply() runs (held to the definition by
    # test_vae_generate_gpu.py); here the buffer of K rows per case is held to it: the same bits
    plain = eng.ensemble(mu, logvar, k, **keywords)
    assert len(plain) == 2 and torch.equal(plain[0], mean) and torch.equal(plain[1], std)
    ds = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(ds, ["lowres"], ensemble_size=k, spread_variable="spread", ensemble_seed=SEED)
    assert np.array_equal(ds["model_output"].values, mean.cpu().numpy()) and np.array_equal(ds["spread"].values, std.cpu().numpy())
    # the mean and the spread the kernel sums are those the moments kernel writes
    np.testing.assert_allclose(sums[:, 4], (std.cpu().numpy() ** 2).sum(axis=(1, 2, 3)), rtol=1e-12)
    np.testing.assert_allclose(sums[:, 3], ((mean.cpu().numpy() - world.target) ** 2).sum(axis=(1, 2, 3)), rtol=1e-12)
    # a device operand and a float64 target on the device give the same
    from cae_tools_amd.engine import device_operand
    again = eng.ensemble(mu, logvar, k, target=device_operand(world.target), want_std=False, **keywords)
    assert again[1] is None and np.array_equal(again[2], sums) and np.array_equal(again[3], ranks)
    wide = eng.ensemble(mu, logvar, k, target=torch.from_numpy(world.target.astype(np.float64)).cuda(), **keywords)
    assert np.array_equal(wide[2], sums) and np.array_equal(wide[3], ranks)


def test_groups_of_many_cases_and_a_short_last_group(world):
    """An engine of 70 rows, K = 2: groups of 35 cases, which the library cuts into chunks of 128 groups, and a last group of
    34, cut into chunks of 64 - which needs more workspace than the full group does.  The draws are the engine's own
    (sample_latent and decode, row for row as ensemble() decodes them; both are held to the definition elsewhere), so the
    ranks are exact and the sums follow test_ensemble_verify_gpu.py's bound."""
    from cae_tools_amd.vae_engine import VaeEngine
    from test_ensemble_verify_gpu import _check
    (n, k, rows) = (69, 2, 70)
    eng = VaeEngine(world.model.spec, FC, LATENT, rows)
    eng.load_state(world.enc, world.dec)
    plane = 176 * 176
    lib = eng.lib
    (full, last) = (int(lib.cae_ensemble_verify_workspace_bytes(g, plane, k)) for g in (35, 34))
    assert last > full                                            # the sizes this test is about
    gen = torch.Generator(device="cuda").manual_seed(5)
    mu = torch.randn((n, LATENT), device="cuda", generator=gen)
    logvar = -2.0 + 0.5 * torch.randn((n, LATENT), device="cuda", generator=gen)
    draws = np.empty((n, k, plane), dtype=np.float32)
    for lo in (0, 35):
        g = min(35, n - lo)
        z = torch.stack([eng.sample_latent(mu[lo:lo + g], logvar[lo:lo + g], draw=j, seed=SEED, first_case=lo) for j in range(k)])
        y = eng.decode(z.view(k * g, LATENT)).view(k, g, plane)      # [draw][case] rows, decoded 70 (68) at once
        draws[lo:lo + g] = y.permute(1, 0, 2).cpu().numpy()
    rng = np.random.default_rng(6)
    pick = rng.integers(0, k, size=(n, plane))
    member = world.vmin + np.take_along_axis(draws, pick[:, None, :], axis=1)[:, 0].astype(np.float64) * world.range
    target = (member + 0.3 * world.range * rng.standard_normal((n, plane)) * (rng.random((n, plane)) < 0.5)).astype(np.float32)
    want = ref.verify(draws, target.astype(np.float64), world.vmin, world.range)
    (mean, std, sums, ranks) = eng.ensemble(mu, logvar, k, seed=SEED, vmin=world.vmin, vmax=world.vmax,
                                            target=target.reshape(n, 1, 176, 176))
    _check((sums, ranks), want, k, "69 cases in groups of 35 and 34")
    assert (ranks[:k + 1] > 0).all() and ranks[:k + 1].sum() == n * plane
    np.testing.assert_allclose(mean.cpu().numpy().reshape(n, plane), world.vmin + draws.astype(np.float64).mean(axis=1) * world.range,
                               rtol=0, atol=1e-11)


@pytest.mark.parametrize("k", [2, 3, 9])
def test_model_verify_ensemble(world, k):
    from cae_tools_amd.utils import ensemble_scores
    with redirect_stdout(io.StringIO()):
        got = world.model.verify_ensemble(world.score_ds(), ["lowres"], "hires", k, ensemble_seed=SEED)
        again = world.model.verify_ensemble(world.score_ds(), ["lowres"], "hires", k, ensemble_seed=SEED)
    _check_against_the_definition(world, k, got["case_sums"], np.asarray(got["rank_counts"] + [got["tied"]]))
    assert got["ensemble_size"] == k and got["ensemble_seed"] == SEED and got["n"] == N * 176 * 176
    want = ensemble_scores.scores_from_sums(got["case_sums"], got["rank_counts"] + [got["tied"]], k)
    for key in ("crps", "fair_crps", "rmse_mean", "spread", "spread_skill", "rank_frequencies"):
        assert got[key] == want[key] == again[key], key
    assert np.array_equal(got["case_crps"], again["case_crps"]) and np.array_equal(got["case_sums"], again["case_sums"])
    assert got["rank_counts"] == again["rank_counts"] and got["tied"] == again["tied"]
    assert 0.0 < got["fair_crps"] < got["crps"]


def test_cli_writes_the_scores_and_the_section(world, tmp_path):
    from cae_tools_amd.cli import verify_ensemble
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.var_ae_model import VarAEModel
    (src, out) = (str(tmp_path / "score.nc"), str(tmp_path / "report"))
    world.score_ds().to_netcdf(src)
    with redirect_stdout(io.StringIO()):
        verify_ensemble.main(["--test-inputs", src, "--model-folder", world.folder, "--output-html-folder", out,
                              "--ensemble-size", "3", "--ensemble-seed", str(SEED)])
        loaded = VarAEModel()
        loaded.load(world.folder)
        api = loaded.verify_ensemble(open_dataset(src), ["lowres"], "hires", 3, ensemble_seed=SEED)
    with open(os.path.join(out, "ensemble_test.json")) as f:
        stored = json.load(f)
    assert stored["ensemble_size"] == 3 and stored["ensemble_seed"] == SEED and stored["n"] == N * 176 * 176
    for key in ("crps", "fair_crps", "rmse_mean", "spread", "spread_skill", "rank_counts", "rank_frequencies", "tied"):
        assert stored[key] == api[key], key
    assert stored["case_crps"] == [float(v) for v in api["case_crps"]]
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert "<h2>Ensemble verification</h2>" in page and "test: 3 members" in page
    assert page.count("rank histogram") == 1 and "fair crps" in page and "spread-skill ratio" in page
