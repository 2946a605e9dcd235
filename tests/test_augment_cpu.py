"""The host side of the dihedral augmentation without a GPU: utils/augment.codes against the generator rule restated with
Python integers, the code table and its edges, code then inverse code with the numpy definition, closure of the composition,
the flags of both parsers, every refusal of train(augment=...) and apply(self_ensemble=...) with its exact message through the
model classes (they come before the GPU is touched), parameters.json with the options off, and what the host side of
cae_dihedral_rows refuses.

The refusal table follows test_importance_cpu.py: the addresses are made-up integers that no call here dereferences, every row
is answered by the host before a launch, and the rows are skipped where a GPU is present (test_dihedral_gpu.py covers the
refusals with real buffers there)."""
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib
from cae_tools_amd.cli import apply_cae, train_cae
from cae_tools_amd.models import base_model
from cae_tools_amd.models.conv_ae_model import ConvAEModel
from cae_tools_amd.models.linear_model import LinearModel
from cae_tools_amd.models.unet import UNET
from cae_tools_amd.models.var_ae_model import VarAEModel
from cae_tools_amd.utils import augment

M64 = (1 << 64) - 1


# ---- the codes -------------------------------------------------------------------------------------

def _unit(seed, r, i, n_unit):
    """bs_unit of csrc/kernels_compare.h (include/cae_hip.h, cae_bootstrap_sums) in Python integers"""
    x = (r << 32) | i
    z = (seed + (x + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n_unit) >> 32


@pytest.mark.parametrize("seed, epoch, n_case, group", [(3, 0, 12, 8), (3, 1, 12, 8), (0, 0, 257, 4), (2 ** 64 - 1, 2 ** 32 - 1, 40, 8),
                                                        (12345678901234567890, 77, 1000, 8), (5, 9, 1, 4), (5, 9, 0, 8)])
def test_codes_against_the_generator_rule(seed, epoch, n_case, group):
    got = augment.codes(seed, epoch, n_case, group)
    assert got.dtype == np.int32 and got.shape == (n_case,)
    assert got.tolist() == [_unit(seed, epoch, j, group) for j in range(n_case)]
    assert ((0 <= got) & (got < group)).all()
    # the code belongs to the case: more cases do not change the codes of the first ones
    assert np.array_equal(got, augment.codes(seed, epoch, n_case + 5, group)[:n_case])


def test_code_table_and_its_edges():
    assert augment.GROUPS == {"flips": 4, "dihedral": 8}
    assert augment.codes(3, 0, 0, 8).shape == (0,) and augment.codes(3, 0, 1, 8).tolist() == [_unit(3, 0, 0, 8)]
    many = augment.codes(1, 0, 4000, 8)
    assert sorted(set(many.tolist())) == list(range(8)) and np.bincount(many).min() > 400       # every code, about evenly
    assert not np.array_equal(augment.codes(1, 0, 64, 8), augment.codes(1, 1, 64, 8))
    assert not np.array_equal(augment.codes(1, 0, 64, 8), augment.codes(2, 0, 64, 8))
    assert [augment.inverse_code(c) for c in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    assert augment.inverse_code(np.array([5, 6, 0], dtype=np.int32)).tolist() == [6, 5, 0]
    for (bad, text) in ((dict(group=5), "group must be 4 or 8, got 5"), (dict(seed=-1), "seed must be an integer from 0 to 2^64 - 1, got -1"),
                        (dict(epoch=-1), "epoch and n_case must lie within [0, 2^32), got -1 and 4")):
        with pytest.raises(ValueError) as refused:
            augment.codes(**dict(dict(seed=0, epoch=0, n_case=4, group=8), **bad))
        assert str(refused.value) == text
    # the definition, spelt out on a plane whose entries say where they came from
    a = np.arange(12).reshape(3, 4)
    assert np.array_equal(augment.apply(a, 1), a[:, ::-1]) and np.array_equal(augment.apply(a, 2), a[::-1])
    assert np.array_equal(augment.apply(a, 3), a[::-1, ::-1]) and np.array_equal(augment.apply(a, 4), a.T)
    assert np.array_equal(augment.apply(a, 5), a.T[:, ::-1]) and np.array_equal(augment.apply(a, 5), np.rot90(a, -1))
    assert np.array_equal(augment.apply(a, 6), a.T[::-1]) and np.array_equal(augment.apply(a, 6), np.rot90(a, 1))
    assert np.array_equal(augment.apply(a, 7), a.T[::-1, ::-1])


@pytest.mark.parametrize("shape, group", [((2, 3, 5), 4), ((2, 4, 4), 8)])
def test_a_code_then_its_inverse_is_the_identity(shape, group):
    a = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)
    for code in range(group):
        turned = augment.apply(a, code)
        assert np.array_equal(augment.apply(turned, augment.inverse_code(code)), a), code
        assert (code == 0) == np.array_equal(turned, a)


def test_the_composition_is_closed():
    a = np.arange(16).reshape(4, 4)
    turns = [augment.apply(a, c).tobytes() for c in range(8)]
    assert len(set(turns)) == 8
    table = [[turns.index(np.ascontiguousarray(augment.apply(augment.apply(a, c), d)).tobytes()) for d in range(8)] for c in range(8)]
    assert all(sorted(row) == list(range(8)) for row in table)              # every pair composes to one of the 8, a latin square
    assert all(table[c][augment.inverse_code(c)] == 0 for c in range(8))
    assert all(table[c][d] < 4 for (c, d) in itertools.product(range(4), repeat=2))      # the flips are a group of their own


# ---- the command lines -----------------------------------------------------------------------------

TRAIN = ["--train-inputs", "a.nc", "--test-inputs", "b.nc", "--model-folder", "m", "--input-variables", "lo", "--output-variable", "hi"]


def test_both_parsers_accept_and_default_the_flags():
    parser = train_cae.build_cli_parser()
    args = parser.parse_args(TRAIN)
    assert (args.augment, args.augment_seed) == (None, None) and train_cae.augment_keywords(args) == {}
    args = parser.parse_args(TRAIN + ["--augment", "dihedral", "--augment-seed", "9"])
    assert train_cae.augment_keywords(args) == {"augment": "dihedral", "augment_seed": 9}
    assert train_cae.augment_keywords(parser.parse_args(TRAIN + ["--augment", "flips"])) == {"augment": "flips"}
    for bad in (["--augment", "turns"], ["--augment-seed", "-1"], ["--augment-seed", "x"], ["--augment"]):
        with pytest.raises(SystemExit):
            parser.parse_args(TRAIN + bad)
    parser = apply_cae.build_parser()
    args = parser.parse_args(["in.nc", "out.nc", "--model-folder", "m"])
    assert (args.self_ensemble, args.self_ensemble_spread) == (None, None) and apply_cae.self_ensemble_keywords(args) == {}
    args = parser.parse_args(["in.nc", "out.nc", "--model-folder", "m", "--self-ensemble", "flips", "--self-ensemble-spread", "s"])
    assert (args.self_ensemble, args.self_ensemble_spread) == ("flips", "s")
    with pytest.raises(SystemExit):
        parser.parse_args(["in.nc", "out.nc", "--model-folder", "m", "--self-ensemble", "turns"])


def _folder(tmp_path, **parameters):
    folder = str(tmp_path / "m")
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "parameters.json"), "w") as f:
        json.dump(dict({"type": "ConvAEModel", "input_shape": [1, 16, 16], "output_shape": [1, 32, 32]}, **parameters), f)
    return folder


def test_apply_cae_refuses_before_the_gpu(tmp_path):
    parser = apply_cae.build_parser()
    folder = _folder(tmp_path)

    def refused(*flags):
        with pytest.raises(SystemExit) as ended:
            apply_cae.self_ensemble_keywords(parser.parse_args(["in.nc", "out.nc", "--model-folder", folder] + list(flags)))
        return str(ended.value)

    assert refused("--self-ensemble-spread", "s") == "--self-ensemble-spread needs --self-ensemble {flips,dihedral}"
    assert refused("--self-ensemble", "flips", "--interval", "0.9") == \
        "--interval needs the plain prediction the model was calibrated with: leave --self-ensemble out"
    assert refused("--self-ensemble", "flips", "--ensemble-size", "4") == \
        "--self-ensemble and --ensemble-size are two ensembles: ask for one of them"
    args = parser.parse_args(["in.nc", "out.nc", "--model-folder", folder, "--self-ensemble", "dihedral", "--self-ensemble-spread", "s"])
    assert apply_cae.self_ensemble_keywords(args) == {"self_ensemble": "dihedral", "self_ensemble_spread": "s"}
    _folder(tmp_path, output_shape=[1, 32, 48])
    assert refused("--self-ensemble", "dihedral") == \
        "--self-ensemble: self_ensemble='dihedral' transposes, which needs square planes: got 32 x 48; use 'flips'"
    _folder(tmp_path, residual_variable="lo")
    assert refused("--self-ensemble", "flips") == "--self-ensemble: " + base_model.residual_refusal("apply(self_ensemble=...)", "lo")


# ---- the model classes -----------------------------------------------------------------------------

class _Untouched(dict):
    """a data set of shapes alone: a refusal that comes before the GPU never reads a value"""

    def __getitem__(self, name):
        return type("Variable", (), {"shape": dict.__getitem__(self, name), "dims": ("n", "c", "y", "x")})()


SQUARE = _Untouched(lo=(12, 1, 16, 16), hi=(12, 1, 32, 32))
WIDE_IN = _Untouched(lo=(12, 1, 8, 12), hi=(12, 1, 32, 32))
WIDE_OUT = _Untouched(lo=(12, 1, 16, 16), hi=(12, 1, 32, 48))
CLASSES = [ConvAEModel, UNET, VarAEModel, LinearModel]


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_train_refusals_with_their_messages(cls):
    for (data, keywords, text) in [
            (SQUARE, dict(augment="turns"), "augment must be one of flips, dihedral, got 'turns'"),
            (SQUARE, dict(augment=8), "augment must be one of flips, dihedral, got 8"),
            (SQUARE, dict(augment="flips", augment_seed=-1), "augment_seed must be an integer from 0 to 2^64 - 1, got -1"),
            (SQUARE, dict(augment="flips", augment_seed=1.5), "augment_seed must be an integer from 0 to 2^64 - 1, got 1.5"),
            (WIDE_IN, dict(augment="dihedral"), "augment='dihedral' transposes, which needs square planes: got 8 x 12; use 'flips'"),
            (WIDE_OUT, dict(augment="dihedral"), "augment='dihedral' transposes, which needs square planes: got 32 x 48; use 'flips'")]:
        mt = cls()
        with pytest.raises(ValueError) as refused:
            mt.train(["lo"], "hi", data, data, **keywords)
        assert str(refused.value) == text
        assert mt._engine is None


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_apply_refusals_with_their_messages(cls):
    mt = cls()
    (mt.input_shape, mt.output_shape) = ((1, 8, 12), (1, 32, 48))
    for (keywords, kind, text) in [
            (dict(self_ensemble="turns"), ValueError, "self_ensemble must be one of flips, dihedral, got 'turns'"),
            (dict(self_ensemble_spread="s"), ValueError, "self_ensemble_spread needs self_ensemble='flips' or 'dihedral'"),
            (dict(self_ensemble="flips", interval="0.9"), ValueError,
             "interval needs the plain prediction the model was calibrated with: leave self_ensemble out"),
            (dict(self_ensemble="flips", ensemble_size=4), ValueError,
             "self_ensemble and ensemble_size are two ensembles: ask for one of them"),
            (dict(self_ensemble="dihedral"), ValueError,
             "self_ensemble='dihedral' transposes, which needs square planes: got 8 x 12; use 'flips'"),
            (dict(self_ensemble="flips", case_chunk=0), ValueError, "case_chunk must be an integer of at least 1, got 0")]:
        with pytest.raises(kind) as refused:
            mt.apply(WIDE_IN, ["lo"], "p", **keywords)
        assert str(refused.value) == text
    mt.residual_variable = "lo"
    with pytest.raises(NotImplementedError) as refused:
        mt.apply(WIDE_IN, ["lo"], "p", self_ensemble="flips")
    assert str(refused.value) == base_model.residual_refusal("apply(self_ensemble=...)", "lo")
    assert mt._engine is None


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_parameters_json_has_no_new_key_with_the_options_off(cls, tmp_path):
    mt = cls()
    (mt.input_shape, mt.output_shape) = ((1, 16, 16), (1, 32, 32))
    plain = mt.get_parameters()
    assert "augment" not in plain and "augment_seed" not in plain
    json.dumps(plain)
    mt._set_augment("flips", 5, [(1, 16, 16)])
    stored = mt.get_parameters()
    assert {k: v for (k, v) in stored.items() if k not in plain} == {"augment": "flips", "augment_seed": 5}
    assert {k: stored[k] for k in plain} == plain and list(stored)[:len(plain)] == list(plain)
    mt._set_augment(None, base_model.KEEP, [(1, 16, 16)])      # switched off again: the seed alone is no key
    assert mt.get_parameters() == plain
    mt._set_augment(base_model.KEEP, base_model.KEEP, [(1, 8, 12)])
    assert (mt.augment, mt.augment_seed) == (None, 5)


# ---- what cae_dihedral_rows refuses ----------------------------------------------------------------

no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal table runs without a GPU only: its addresses are made up")
(OK, ARG) = (0, -1)
(SRC, DST, ROW, CODE) = (0x100000, 0x200000, 0x300000, 0x400000)
NAMES = "src n_src c h w dst n_dst rows codes group stream".split()
CALL = dict(src=SRC, n_src=5, c=2, h=6, w=6, dst=DST, n_dst=9, rows=ROW, codes=CODE, group=8, stream=None)
NOTHING = dict(src=None, dst=None, rows=None, codes=None)
TABLE = [
    (ARG, "cae_dihedral_rows: bad argument (n_src >= 0, n_dst >= 0, c >= 1, h >= 0, w >= 0, group 4 or 8)",
     [dict(n_src=-1), dict(n_dst=-1), dict(c=0), dict(c=-3), dict(h=-1), dict(w=-1), dict(group=0), dict(group=5), dict(group=16)]),
    (ARG, "cae_dihedral_rows: group 8 transposes, which needs square planes (h == w)",
     [dict(w=7), dict(h=5), dict(h=0), dict(w=7, n_dst=0)]),
    (ARG, "cae_dihedral_rows: more than 2^31 - 1 rows", [dict(n_src=1 << 31), dict(n_dst=1 << 31)]),
    (OK, "", [dict(n_dst=0, **NOTHING), dict(h=0, w=0, **NOTHING), dict(h=0, group=4, **NOTHING), dict(w=0, group=4, **NOTHING)]),
    (ARG, "cae_dihedral_rows: null pointer", [dict(src=None), dict(dst=None), dict(codes=None)]),
    (ARG, "cae_dihedral_rows: an operand reaches 2^60 elements from its pointer",
     [dict(n_src=1 << 30, h=1 << 15, w=1 << 15), dict(n_dst=1 << 30, c=1 << 10, h=1 << 11, w=1 << 11)]),
    (ARG, "cae_dihedral_rows: pointers must be 4-byte aligned", [dict(src=SRC + 2), dict(dst=DST + 1), dict(rows=ROW + 2), dict(codes=CODE + 3)]),
    (ARG, "cae_dihedral_rows: dst overlaps src",
     [dict(dst=SRC), dict(dst=SRC + 4 * 72 * 5 - 4), dict(src=DST + 4 * 72 * 9 - 4), dict(dst=SRC - 4 * 72 * 9 + 4)]),
]


def _rows(table):
    return [(rc, text, change) for (rc, text, changes) in table for change in changes]


def _row_id(row):
    return ",".join(f"{k}={v}" for (k, v) in row[2].items())


def test_the_rows_are_distinct_and_the_abi_lists_the_entry_point():
    rows = _rows(TABLE)
    assert len(set(map(_row_id, rows))) == len(rows) and list(CALL) == NAMES
    assert len(_lib.SIGNATURES["cae_dihedral_rows"][1]) == len(NAMES)
    lib = _lib.load()
    assert lib.cae_abi_version() == 1
    # the grid cap the GPU test drives the kernel past is the one the host code launches with
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae_tools_amd", "csrc")
    with open(os.path.join(csrc, "host_dihedral.h")) as f:
        text = f.read()
    assert re.search(r"constexpr int64_t DH_MAX_GROUPS = 16384;", text)
    assert "a.items < DH_MAX_GROUPS ? a.items : DH_MAX_GROUPS" in text


@no_gpu
@pytest.mark.parametrize("row", _rows(TABLE), ids=_row_id)
def test_dihedral_rows_refusal(row):
    """the call is answered by the host, with this code and this text; rows = NULL is allowed"""
    (rc, text, change) = row
    lib = _lib.load()
    args = dict(CALL, **change)
    assert set(change) <= set(CALL)
    got = lib.cae_dihedral_rows(*(args[n] for n in NAMES))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
