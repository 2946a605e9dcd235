"""The 'var' model as a generative one: vae_encode / vae_decode / vae_sample_latent (include/cae_vae.h), the module-level
forwards, VarAEModel.encode / decode / generate / apply(ensemble_size=K) and apply_cae's flags, against the build's own CPU
definition (oracle/vae_oracle.py; PARITY UNPINNED with respect to the reference, which ships no source for this model).
Geometry 12x12 -> 176x176, latent 4, fc 12, 7 cases; the model has taken two training steps, so its running statistics are
not the initial ones."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

(LATENT, FC, N, SEED) = (4, 12, 7, 21)


def _data(n, seed, size_in=12, size_out=176):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, size_out), np.linspace(-1, 1, size_out), indexing="ij")
    hi = np.zeros((n, 1, size_out, size_out), dtype=np.float32)
    for i in range(n):
        (a, b, c) = rng.random(3)
        hi[i, 0] = 285 + 8 * np.sin(4 * a * yy + 3 * b * xx + 6 * c)
    f = size_out // size_in
    lo = hi[:, :, :size_in * f, :size_in * f].reshape(n, 1, size_in, f, size_in, f).mean(axis=(3, 5)).astype(np.float32)
    ds = Dataset()
    ds["lowres"] = DataArray(lo, dims=("n", "chan", "y", "x"))
    ds["hires"] = DataArray(hi, dims=("n", "chan", "y2", "x2"))
    return ds


class _World:
    """one trained model, its folder, the definition's copy of its state, and the definition's answers, computed once"""

    def __init__(self, tmp):
        from cae_tools_amd.models.ds_dataset import DSDataset
        from cae_tools_amd.models.var_ae_model import VarAEModel
        from oracle import cae_oracle as orc
        from oracle import vae_oracle as vo
        torch.manual_seed(3)
        self.model = VarAEModel(batch_size=4, nr_epochs=1, test_interval=1, fc_size=FC, encoded_dim_size=LATENT, lambda_kl=0.05,
                                noise_seed=6)
        self.folder = str(tmp / "model")
        with redirect_stdout(io.StringIO()):
            self.model.train(["lowres"], "hires", _data(8, 1), _data(4, 2), model_path=self.folder)    # 8 cases / 4: two steps
            self.eng = self.model._engine
            assert self.eng.max_batch == 4 and self.eng.num_batches_tracked == 2
            (self.enc, self.dec) = self.eng.export_state()
            self.spec = self.model.spec.save()
            ds = DSDataset(self.score_ds(), ["lowres"], "lowres", normalise_in=True)
            ds.set_normalisation_parameters(self.model.normalisation_parameters)
        self.ds = ds
        self.x = ds.device_inputs()
        (self.vmin, self.vmax) = self.model.normalisation_parameters[2:4]
        self.range = self.vmax - self.vmin
        self.vo, self.orc = vo, orc
        with torch.no_grad():
            (mu, logvar) = vo.encoder_forward(self.spec, self.enc, self.x.cpu(), train=False)
        (self.mu, self.logvar) = (mu.numpy(), logvar.numpy())
        self._fields = {}

    @staticmethod
    def score_ds():
        return _data(N, 5)

    def oracle_decode(self, z):
        with torch.no_grad():
            return self.orc.decoder_forward(self.spec, self.dec, torch.as_tensor(z), train=False).numpy()

    def oracle_draw(self, k, seed=SEED):
        """the definition's field of draw k of every case: its own mu and logvar, its noise, its decoder"""
        if (k, seed) not in self._fields:
            z = self.mu + self.vo.normal_noise(seed, k, (N, LATENT)) * np.exp(np.float32(0.5) * self.logvar)
            self._fields[(k, seed)] = self.oracle_decode(z.astype(np.float32))
        return self._fields[(k, seed)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return _World(tmp_path_factory.mktemp("vae_generate"))


def test_encode_matches_the_definition(world):
    (mu, logvar) = world.eng.encode(world.x)
    assert mu.shape == logvar.shape == (N, LATENT) and mu.dtype == torch.float32
    print("encode: max |mu error| %.3e, max |logvar error| %.3e" % (np.abs(mu.cpu().numpy() - world.mu).max(),
                                                                     np.abs(logvar.cpu().numpy() - world.logvar).max()))
    np.testing.assert_allclose(mu.cpu().numpy(), world.mu, rtol=0, atol=1e-5)
    np.testing.assert_allclose(logvar.cpu().numpy(), world.logvar, rtol=0, atol=1e-5)
    (mu_np, logvar_np) = world.model.encode(world.score_ds(), ["lowres"])
    assert mu_np.dtype == np.float32 and np.array_equal(mu_np, mu.cpu().numpy()) and np.array_equal(logvar_np, logvar.cpu().numpy())


def test_decode_matches_the_definition_and_score_is_decode_of_mu(world):
    z = torch.from_numpy(world.vo.normal_noise(4, 1, (N, LATENT))).cuda() * 0.7
    y = world.eng.decode(z)
    assert y.shape == (N, 1, 176, 176)
    print("decode: max |error| %.3e" % np.abs(y.cpu().numpy() - world.oracle_decode(z.cpu())).max())
    np.testing.assert_allclose(y.cpu().numpy(), world.oracle_decode(z.cpu()), rtol=0, atol=1e-5)
    # BITWISE: vae_score runs the launches of vae_encode and vae_decode in one go; between them k_reparam (eval) copies mu
    # into the buffer the decoder's first Linear reads, and decode() reads the same values from the caller's array.  Both
    # walk the 7 cases in the same chunks of max_batch = 4 rows, so every kernel sees the same shapes and the same numbers.
    (mu, _) = world.eng.encode(world.x)
    assert torch.equal(world.eng.score(world.x), world.eng.decode(mu))
    # the model-level decode denormalises as apply does
    got = world.model.decode(z.cpu().numpy())
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, world.vmin + y.cpu().numpy().astype(np.float64) * world.range)


def test_sample_latent_matches_the_definition_however_it_is_cut(world):
    from cae_tools_amd._lib import CaeError
    eng = world.eng
    (mu, logvar) = eng.encode(world.x)
    (mu_np, lv_np) = (mu.cpu().numpy().astype(np.float64), logvar.cpu().numpy().astype(np.float64))
    for k in (0, 1, 5):
        z = eng.sample_latent(mu, logvar, draw=k, seed=SEED)
        eps = world.vo.normal_noise(SEED, k, (N, LATENT)).astype(np.float64)
        scale = np.abs(mu_np) + np.abs(eps) * np.exp(0.5 * lv_np)
        err = np.abs(z.cpu().numpy() - (mu_np + eps * np.exp(0.5 * lv_np)))
        print("draw %d: max error in fp32 ulp of |mu| + |eps| exp(logvar / 2): %.3f" % (k, (err / (scale * 2.0 ** -23)).max()))
        assert (err <= 4 * 2.0 ** -23 * scale).all()      # 4 fp32 ulp: expf, one product, one sum
        chunks = torch.cat([eng.sample_latent(mu[lo:lo + 3], logvar[lo:lo + 3], draw=k, seed=SEED, first_case=lo)
                            for lo in range(0, N, 3)])
        shards = torch.cat([eng.sample_latent(mu[:4], logvar[:4], draw=k, seed=SEED),
                            eng.sample_latent(mu[4:], logvar[4:], draw=k, seed=SEED, first_case=4)])
        assert torch.equal(z, chunks) and torch.equal(z, shards)
    # the prior: the noise itself, the same bits as the definition's
    assert np.array_equal(eng.sample_latent(None, None, draw=2, seed=9, n=5).cpu().numpy(), world.vo.normal_noise(9, 2, (5, LATENT)))
    with pytest.raises(CaeError, match="2\\^31"):
        eng._sample_into(torch.empty((1, LATENT), device="cuda"), None, None, 2 ** 31 // LATENT, 0, 0)


@pytest.mark.parametrize("k", [3, 4, 9])        # below, equal to and above the engine's 4 rows
def test_ensemble_apply_matches_the_definition(world, k):
    assert world.eng.ensemble_plan(k) == (1, min(k, 4))
    ds = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(ds, ["lowres"], ensemble_size=k, spread_variable="spread", ensemble_seed=SEED)
    (mean, std) = (ds["model_output"].values, ds["spread"].values)
    assert mean.dtype == std.dtype == np.float64 and mean.shape == std.shape == (N, 1, 176, 176)
    assert tuple(ds["spread"].dims) == tuple(ds["model_output"].dims) == ("n", "model_output_channel", "model_output_y",
                                                                         "model_output_x")
    fields = np.stack([world.oracle_draw(j) for j in range(k)]).astype(np.float64)
    want_mean = world.vmin + fields.mean(axis=0) * world.range
    want_std = fields.std(axis=0, ddof=1) * abs(world.range)
    (mean_err, std_err) = (np.abs(mean - want_mean).max(), np.abs(std - want_std).max())
    print("K %d: max |mean error| %.3e (bound %.3e), max |std error| %.3e (bound %.3e), largest std %.3e"
          % (k, mean_err, 1e-5 * world.range, std_err, np.sqrt(k / (k - 1)) * 1e-5 * world.range, want_std.max()))
    assert want_std.max() > 1e-3 * world.range      # the draws do differ
    assert mean_err <= 1e-5 * world.range
    # each draw within 1e-5 of the definition's: the centred K-vectors differ by at most sqrt(K) * 1e-5 in norm (triangle
    # inequality), and std is that norm over sqrt(K - 1)
    assert std_err <= np.sqrt(k / (k - 1)) * 1e-5 * world.range
    # twice the same bits, and no spread variable unless asked for
    again = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(again, ["lowres"], ensemble_size=k, ensemble_seed=SEED)
    assert np.array_equal(again["model_output"].values, mean) and "spread" not in again


def test_apply_without_an_ensemble_is_the_deterministic_apply(world):
    ds = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(ds, ["lowres"])
    want = world.ds.denormalise_device(world.model._score_device(world.x)).cpu().numpy()
    assert np.array_equal(ds["model_output"].values, want)
    # the latents alone leave the prediction as it is
    with_latent = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(with_latent, ["lowres"], latent_variable="z")
    assert np.array_equal(with_latent["model_output"].values, want)
    (mu, logvar) = world.eng.encode(world.x)
    assert with_latent["z_mu"].values.dtype == np.float32 and tuple(with_latent["z_mu"].dims) == ("n", "model_latent")
    assert np.array_equal(with_latent["z_mu"].values, mu.cpu().numpy())
    assert np.array_equal(with_latent["z_logvar"].values, logvar.cpu().numpy())
    # one draw: the field of that draw, no spread to speak of
    one = world.score_ds()
    with redirect_stdout(io.StringIO()):
        world.model.apply(one, ["lowres"], ensemble_size=1, ensemble_seed=SEED)
    np.testing.assert_allclose(one["model_output"].values, world.vmin + world.oracle_draw(0).astype(np.float64) * world.range,
                               rtol=0, atol=1e-5 * world.range)


def test_generate_matches_the_definition(world):
    got = world.model.generate(5, seed=8)
    want = world.vmin + world.oracle_decode(world.vo.normal_noise(8, 0, (5, LATENT))).astype(np.float64) * world.range
    assert got.dtype == np.float64 and got.shape == (5, 1, 176, 176)
    print("generate: max |error| %.3e (bound %.3e)" % (np.abs(got - want).max(), 1e-5 * world.range))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * world.range)      # decode's bound, denormalised


def test_module_level_forward(world):
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.var_ae_model import VarEncoder
    (mu, logvar) = world.model.encoder(world.x)
    (want_mu, want_logvar) = world.eng.encode(world.x)
    assert torch.equal(mu, want_mu) and torch.equal(logvar, want_logvar)
    assert torch.equal(world.model.decoder(mu), world.eng.decode(mu))
    with pytest.raises(RuntimeError, match="attached"):
        VarEncoder(world.model.spec.get_input_layers(), LATENT, FC).forward(world.x)
    with pytest.raises(RuntimeError, match="attached"):
        Decoder(world.model.spec.get_output_layers(), LATENT, FC).forward(mu)


def test_cli_round_trip(world, tmp_path):
    from cae_tools_amd.cli import apply_cae
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.var_ae_model import VarAEModel
    (src, out) = (str(tmp_path / "score.nc"), str(tmp_path / "scored.nc"))
    world.score_ds().to_netcdf(src)
    with redirect_stdout(io.StringIO()):
        apply_cae.main([src, out, "--model-folder", world.folder, "--input-variables", "lowres", "--ensemble-size", "3",
                        "--spread-variable", "s", "--ensemble-seed", str(SEED), "--latent-variable", "z"])
        loaded = VarAEModel()
        loaded.load(world.folder)
        api = open_dataset(src)
        loaded.apply(api, ["lowres"], ensemble_size=3, spread_variable="s", ensemble_seed=SEED, latent_variable="z")
    got = open_dataset(out)
    for (name, dtype, dims) in (("model_output", np.float64, 4), ("s", np.float64, 4), ("z_mu", np.float32, 2),
                                ("z_logvar", np.float32, 2)):
        assert name in got and got[name].values.dtype == dtype and len(got[name].dims) == dims, name
        assert tuple(got[name].dims) == tuple(api[name].dims)
        assert np.array_equal(got[name].values, api[name].values), name
    assert tuple(got["s"].dims) == tuple(got["model_output"].dims) and got["z_mu"].dims[1] == "model_latent"
    assert got["z_mu"].shape == (N, LATENT) and got["s"].shape == (N, 1, 176, 176)
