"""What the VAE's generative surface decides without a GPU: apply_cae's four flags, their refusal for a folder that holds no
VarAEModel before any rank is spawned, and the argument checks of VarAEModel.apply and cae_ensemble_moments."""
import json

import pytest


def _folder(tmp_path, model_type):
    folder = tmp_path / model_type
    folder.mkdir()
    (folder / "parameters.json").write_text(json.dumps({"type": model_type}))
    return str(folder)


def test_parser_accepts_the_four_flags():
    from cae_tools_amd.cli import apply_cae
    args = apply_cae.build_parser().parse_args(["in.nc", "out.nc", "--model-folder", "m", "--ensemble-size", "16",
                                                "--spread-variable", "spread", "--ensemble-seed", "7", "--latent-variable", "z"])
    assert (args.ensemble_size, args.spread_variable, args.ensemble_seed, args.latent_variable) == (16, "spread", 7, "z")
    plain = apply_cae.build_parser().parse_args(["in.nc", "out.nc", "--model-folder", "m"])
    assert (plain.ensemble_size, plain.spread_variable, plain.ensemble_seed, plain.latent_variable) == (None, None, 0, None)
    assert apply_cae.ensemble_keywords(plain) == {}      # the plain apply reads no parameters.json


def test_keywords_for_a_vae_folder(tmp_path):
    from cae_tools_amd.cli import apply_cae
    folder = _folder(tmp_path, "VarAEModel")
    args = apply_cae.build_parser().parse_args(["in.nc", "out.nc", "--model-folder", folder, "--ensemble-size", "3",
                                                "--spread-variable", "s", "--latent-variable", "z"])
    assert apply_cae.ensemble_keywords(args) == {"ensemble_size": 3, "spread_variable": "s", "latent_variable": "z", "ensemble_seed": 0}
    for flags in (["--spread-variable", "s"], ["--spread-variable", "s", "--ensemble-size", "1"], ["--ensemble-size", "0"]):
        with pytest.raises(SystemExit):
            apply_cae.ensemble_keywords(apply_cae.build_parser().parse_args(["in.nc", "out.nc", "--model-folder", folder] + flags))


@pytest.mark.parametrize("flags", [["--ensemble-size", "3"], ["--spread-variable", "s"], ["--ensemble-seed", "2"],
                                   ["--latent-variable", "z"]])
def test_flags_are_refused_for_another_model_before_ranks_are_spawned(tmp_path, monkeypatch, flags):
    from cae_tools_amd.cli import _launch, apply_cae

    def no_spawn(*args, **kwargs):
        pytest.fail("a rank was spawned for flags that the model folder cannot honour")

    monkeypatch.setattr(_launch.subprocess, "call", no_spawn)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as refusal:
        apply_cae.main(["in.nc", "out.nc", "--model-folder", _folder(tmp_path, "ConvAEModel"), "--gpus", "2"] + flags)
    assert "VarAEModel" in str(refusal.value) and "ConvAEModel" in str(refusal.value)


def test_spread_needs_two_draws():
    from cae_tools_amd.models.var_ae_model import VarAEModel
    model = VarAEModel()
    for k in (None, 1):
        with pytest.raises(ValueError, match="spread_variable"):
            model.apply(None, ["lowres"], ensemble_size=k, spread_variable="s")
    with pytest.raises(ValueError, match="ensemble_size"):
        model.apply(None, ["lowres"], ensemble_size=0)


def test_other_models_name_the_vae():
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    from cae_tools_amd.models.linear_model import LinearModel
    for model in (ConvAEModel(), LinearModel()):
        with pytest.raises(TypeError, match="VarAEModel"):
            model.apply(None, ["lowres"], ensemble_size=4)


def test_noise_index_guard():
    """element (case, j) of a draw's noise is number case * latent + j, which the hash doubles in 32 bits"""
    import numpy as np

    from cae_tools_amd import vae_engine
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.var_ae_model import VarAEModel
    vae_engine.check_noise_index(2 ** 31 // 32 - 1, 32)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        vae_engine.check_noise_index(2 ** 31 // 32, 32)
    # apply() refuses before it touches the data or the GPU: 2^27 cases (of one byte each, never read) at latent 16
    ds = Dataset()
    ds["lowres"] = DataArray(np.broadcast_to(np.zeros(1, dtype=np.int8), (2 ** 27, 1, 1, 1)), dims=("n", "chan", "y", "x"))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        VarAEModel(encoded_dim_size=16).apply(ds, ["lowres"], ensemble_size=2)


def test_moments_arguments_are_checked():
    """no launch is made for a call that would read or write outside its arrays"""
    from cae_tools_amd import _lib
    lib = _lib.load()
    assert lib.cae_ensemble_moments_workspace_bytes(3, 35) == 3 * 35 * 20
    (y, out) = (0x1000, 0x2000)     # never dereferenced: every call below is refused by the host
    bad = [dict(k_total=1, k_call=1), dict(k_call=0), dict(k_done=3, k_call=2), dict(draw_stride=34), dict(plane=0),
           dict(k_call=2),                    # a partial delivery without a workspace
           dict(k_call=2, ws=0x3000, ws_bytes=3 * 35 * 20 - 1), dict(y=0x1002), dict(out=0x2004)]
    for change in bad:
        a = dict(y=y, case_stride=35, draw_stride=3 * 35, n_case=3, plane=35, k_call=4, k_done=0, k_total=4, out=out, ws=None,
                 ws_bytes=0)
        a.update(change)
        rc = lib.cae_ensemble_moments(a["y"], a["case_stride"], a["draw_stride"], a["n_case"], a["plane"], a["k_call"], a["k_done"],
                                      a["k_total"], 288.0, 10.5, a["out"], None, a["ws"], a["ws_bytes"], None)
        assert rc < 0, change
        with pytest.raises(_lib.CaeError, match="cae_ensemble_moments"):
            _lib.check(rc)
