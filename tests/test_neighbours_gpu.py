"""cae_case_neighbours on the GPU against the numpy restatement of its definition (neighbours_ref.py).

Exact grid: values k / 8 with integer k in [0, 16), so every difference, square and sum is exact in fp64 whatever the fold
order, and dist2, index and count are compared with np.array_equal - no tolerance.  The shapes hit both sides of every edge
the kernel has:
    D     the staged slice of 32 features and its groups of 4 (1, 3, 31, 32, 33, 63, 64, 65), many slices (257, 1031);
    n_q   the tile of 64 queries (1, 2, 17, 63, 64, 65), and so many query tiles that a workgroup walks a run of several
          reference tiles with its lists carried from tile to tile (4097 queries against 1025 references);
    n_r   the tile of 64 references (1, 2, 31, 63, 64, 65), several tiles, each a split of its own folded by the merge
          launch (200, 1025);
    K     1, 2, 5, 32, also above n_r.
These inputs are full of ties, so the index tie rule is tested throughout.  Then self-exclusion and merge in pieces against
one call bit for bit, validity, general floats against the derived bound (2 D + 8) 2^-53, split invariance of the bits of
d2, determinism and every refusal; then train_cae -> cli.novelty -> apply_cae --novelty-variable for a conv model with every
number of novelty_<partition>.json recomputed from the restatement, and the two commands on a linear, a unet and a var model
folder."""
import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import importance_ref
import neighbours_ref
from cae_tools_amd import _lib
from cae_tools_amd.case_ops import _stream
from cae_tools_amd.engine import case_neighbours

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want):
    """the three outputs, bit for bit"""
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[2].shape == want[2].shape
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1]), int((got[1] != want[1]).sum())
    assert np.array_equal(bits(got[0]), bits(want[0])), int((bits(got[0]) != bits(want[0])).sum())


def grid_rows(rng, n, dim):
    return (rng.integers(0, 16, size=(n, dim)) / 8.0).astype(np.float32)


def raw_call(q, n_q, q_stride, r, n_r, r_stride, dim, k, ref_base=0, self_offset=-1, merge=0, outs=None, q_off=0, r_off=0,
             workspace=True, mangle=None):
    """cae_case_neighbours on flat float32 CUDA tensors: rows start q_off / r_off elements into them.  mangle: a function
    over the dict of C arguments, for the refusals.  Returns the three outputs as numpy arrays."""
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device())
    if outs is None:
        (rows, width) = (max(n_q, 1), k if 1 <= k <= 32 else 1)          # never empty: an empty tensor has no pointer
        outs = (torch.full((rows, width), 7.0, dtype=torch.float64, device=device),
                torch.full((rows, width), 7, dtype=torch.int32, device=device), torch.full((rows,), 7, dtype=torch.int32, device=device))
    need = int(lib.cae_case_neighbours_workspace_bytes(n_q, n_r, k))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    a = {"q": q.data_ptr() + 4 * q_off if q is not None else None, "n_q": n_q, "q_stride": q_stride,
         "r": r.data_ptr() + 4 * r_off if r is not None else None, "n_r": n_r, "r_stride": r_stride, "dim": dim, "k": k,
         "ref_base": ref_base, "self_offset": self_offset, "merge": merge, "dist2": outs[0].data_ptr(), "index": outs[1].data_ptr(),
         "count": outs[2].data_ptr(), "ws": ws.data_ptr() if workspace else None, "ws_bytes": need}
    if mangle:
        mangle(a)
    with _stream(device) as stream:
        _lib.check(lib.cae_case_neighbours(a["q"], a["n_q"], a["q_stride"], a["r"], a["n_r"], a["r_stride"], a["dim"], a["k"],
                                           a["ref_base"], a["self_offset"], a["merge"], a["dist2"], a["index"], a["count"], a["ws"],
                                           a["ws_bytes"], stream))
        return tuple(t.cpu().numpy() for t in outs)


# ---- the exact grid -----------------------------------------------------------------------------------------------------

DIMS = [1, 3, 31, 32, 33, 63, 64, 65, 257, 1031]
QUERIES = [1, 2, 17, 63, 64, 65]
REFS = [1, 2, 31, 63, 64, 65, 200, 1025]
GRID = ([(d, 17, 65, 5) for d in DIMS] + [(33, n, 200, 2) for n in QUERIES] + [(3, 2, n, 32) for n in REFS] +
        [(64, 17, n, 1) for n in REFS] + [(257, 65, 31, 32), (1031, 2, 1025, 5), (1, 65, 1025, 32), (65, 65, 65, 2),
                                          (3, 4097, 1025, 5)])


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(str(v) for v in s))
def test_exact_grid(shape):
    (dim, n_q, n_r, k) = shape
    rng = np.random.default_rng(dim * 1000003 + n_q * 1009 + n_r * 13 + k)
    (q, r) = (grid_rows(rng, n_q, dim), grid_rows(rng, n_r, dim))
    want = neighbours_ref.neighbours(q, r, k)
    assert (want[2] == min(k, n_r)).all()
    same(case_neighbours(q, r, k), want)


def test_duplicates_equal_rows_and_exact_zero():
    rng = np.random.default_rng(5)
    r = grid_rows(rng, 70, 40)
    r[10] = r[3]
    r[69] = r[3]
    r[40] = r[41]
    q = grid_rows(rng, 9, 40)
    q[4] = r[3]                     # a query equal to three references: d2 exactly +0.0, the indices ascending
    got = case_neighbours(q, r, 5)
    same(got, neighbours_ref.neighbours(q, r, 5))
    assert list(got[1][4, :3]) == [3, 10, 69] and (bits(got[0][4, :3]) == 0).all()
    # all rows equal: every distance +0.0, the K smallest indices
    one = np.tile(grid_rows(rng, 1, 70), (130, 1))
    got = case_neighbours(one[:66], one, 32)
    same(got, neighbours_ref.neighbours(one[:66], one, 32))
    assert (bits(got[0]) == 0).all() and (got[1] == np.arange(32)).all()


@pytest.mark.parametrize("offsets", [(0, 0), (1, 3), (2, 1), (3, 2)], ids=str)
def test_strides_and_four_byte_alignment(offsets):
    (q_off, r_off) = offsets
    (dim, n_q, n_r, k, qs, rs) = (37, 20, 90, 5, 41, 39)      # odd strides: most rows start on 4-byte boundaries only
    rng = np.random.default_rng(11)
    (q, r) = (grid_rows(rng, n_q, dim), grid_rows(rng, n_r, dim))
    qb = np.full(q_off + n_q * qs, np.nan, dtype=np.float32)    # what lies between the rows is not looked at
    rb = np.full(r_off + n_r * rs, np.nan, dtype=np.float32)
    for i in range(n_q):
        qb[q_off + i * qs:q_off + i * qs + dim] = q[i]
    for j in range(n_r):
        rb[r_off + j * rs:r_off + j * rs + dim] = r[j]
    got = raw_call(torch.from_numpy(qb).cuda(), n_q, qs, torch.from_numpy(rb).cuda(), n_r, rs, dim, k, q_off=q_off, r_off=r_off)
    same(got, neighbours_ref.neighbours(q, r, k))


# ---- self-exclusion -------------------------------------------------------------------------------------------------------

def test_self_exclusion_in_pieces():
    rng = np.random.default_rng(21)
    x = grid_rows(rng, 150, 20)
    x[77] = x[5]                                                # a duplicate stays a neighbour: only the own row is left out
    k = 5
    want = neighbours_ref.neighbours(x, x, k, self_offset=0)
    one = case_neighbours(x, x, k, self_offset=0)
    same(one, want)
    assert not (one[1] == np.arange(150)[:, None]).any()        # no query lists itself
    assert one[1][5, 0] == 77 and one[0][5, 0] == 0.0
    # the queries in pieces
    parts = [case_neighbours(x[c0:c1], x, k, self_offset=c0) for (c0, c1) in ((0, 1), (1, 64), (64, 130), (130, 150))]
    same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), one)
    # the references in pieces
    held = None
    for (r0, r1) in ((0, 63), (63, 64), (64, 149), (149, 150)):
        held = case_neighbours(x, x[r0:r1], k, ref_base=r0, self_offset=0, merge_into=held)
    same(held, one)
    # both
    rows = []
    for (c0, c1) in ((0, 70), (70, 150)):
        held = None
        for (r0, r1) in ((100, 150), (0, 100)):
            held = case_neighbours(x[c0:c1], x[r0:r1], k, ref_base=r0, self_offset=c0, merge_into=held)
        rows.append(held)
    same(tuple(np.concatenate([p[i] for p in rows]) for i in range(3)), one)


# ---- merge ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(1,), (199,), (64, 65, 130), (3, 5, 100, 198)], ids=str)
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_merge_equals_one_call(cuts, descending):
    rng = np.random.default_rng(31)
    (q, r) = (grid_rows(rng, 70, 12), grid_rows(rng, 200, 12))
    r[0] = np.nan                                               # the first pieces hold fewer than K valid rows
    r[2] = np.inf
    k = 5
    one = case_neighbours(q, r, k)
    same(one, neighbours_ref.neighbours(q, r, k))
    edges = [0, *cuts, 200]
    pieces = list(zip(edges[:-1], edges[1:]))
    (held, ref_held, seen) = (None, None, 0)
    for (r0, r1) in (pieces[::-1] if descending else pieces):
        held = case_neighbours(q, r[r0:r1], k, ref_base=r0, merge_into=held)
        ref_held = neighbours_ref.neighbours(q, r[r0:r1], k, ref_base=r0, merge_into=ref_held)
        same(held, ref_held)
        seen += int(neighbours_ref.valid_rows(r[r0:r1]).sum())
        assert (held[2] == min(k, seen)).all()                  # count grows with the valid rows seen
    same(held, one)


def test_merge_with_no_reference_leaves_the_lists():
    rng = np.random.default_rng(32)
    (q, r) = (grid_rows(rng, 5, 7), grid_rows(rng, 9, 7))
    one = case_neighbours(q, r, 3)
    same(case_neighbours(q, r[:0], 3, ref_base=9, merge_into=one), one)
    empty = case_neighbours(q, r[:0], 3)
    assert (empty[2] == 0).all() and np.isinf(empty[0]).all() and (empty[1] == -1).all()


# ---- validity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("at", [0, 40, 99], ids=["first", "middle", "last"])
def test_invalid_rows(bad, at):
    rng = np.random.default_rng(41)
    (q, r) = (grid_rows(rng, 66, 100), grid_rows(rng, 130, 100))
    q[7, at] = bad
    q[65, at] = bad
    r[0, at] = bad
    r[64, at] = bad
    r[129, at] = bad
    got = case_neighbours(q, r, 5)
    same(got, neighbours_ref.neighbours(q, r, 5))
    assert got[2][7] == -1 and np.isinf(got[0][7]).all() and (got[1][7] == -1).all()
    assert not np.isin(got[1], [0, 64, 129]).any()


def test_few_or_no_valid_references():
    rng = np.random.default_rng(42)
    (q, r) = (grid_rows(rng, 10, 9), grid_rows(rng, 70, 9))
    r[:, 3] = np.nan
    none = case_neighbours(q, r, 5)
    same(none, neighbours_ref.neighbours(q, r, 5))
    assert (none[2] == 0).all() and np.isinf(none[0]).all()
    r[[4, 66], 3] = 0.5
    few = case_neighbours(q, r, 5)
    same(few, neighbours_ref.neighbours(q, r, 5))
    assert (few[2] == 2).all() and np.isinf(few[0][:, 2:]).all() and (few[1][:, 2:] == -1).all()


# ---- general floats -------------------------------------------------------------------------------------------------------

def float_rows(seed, n_q=70, n_r=300, c=5, plane=64):
    """seeded normal and uniform fp32 rows of c channels: channels 0 and 1 shared bit for bit between all rows, channel 2
    shared up to one ulp in some rows - the static-channel case - and the rest differing"""
    rng = np.random.default_rng(seed)
    static = rng.normal(size=(3, plane)).astype(np.float32)

    def rows(n):
        x = np.empty((n, c, plane), dtype=np.float32)
        x[:, :3] = static
        nudge = rng.random((n, plane)) < 0.3
        x[:, 2] = np.where(nudge, np.nextafter(x[:, 2], np.float32(np.inf)), x[:, 2])
        x[:, 3] = rng.normal(size=(n, plane)).astype(np.float32) * 1e-3
        x[:, 4:] = rng.random((n, c - 4, plane)).astype(np.float32)
        return x.reshape(n, -1)

    return rows(n_q), rows(n_r)


FLOATS = {}


def floats():
    if not FLOATS:
        (q, r) = float_rows(51)
        q[3] = r[17]                                            # an exact copy among near-duplicates
        FLOATS.update(q=q, r=r, d2=neighbours_ref.dist2(q, r))
    return FLOATS["q"], FLOATS["r"], FLOATS["d2"]


@pytest.mark.parametrize("k", [1, 5, 32])
def test_general_floats_within_the_derived_bound(k):
    (q, r, d2) = floats()
    dim = q.shape[1]
    bound = (2 * dim + 8) * U
    (dist, index, count) = case_neighbours(q, r, k)
    assert (count == k).all()
    rows = np.arange(len(q))[:, None]
    want = d2[rows, index]
    assert (np.abs(dist - want) <= bound * want).all(), float(np.max(np.abs(dist - want) / np.where(want > 0, want, 1.0))) / bound
    assert dist[3, 0] == 0.0 and index[3, 0] == 17 and not np.signbit(dist).any()
    # sorted by (d2, index) on its own values, no duplicate
    key_ok = (dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (index[:, 1:] > index[:, :-1]))
    assert key_ok.all()
    assert all(len(set(row)) == k for row in index.tolist())
    # no reference outside the list is closer than the list's K-th by more than the bound
    outside = np.ones_like(d2, dtype=bool)
    outside[rows, index] = False
    kth = dist[:, -1:]
    assert (np.where(outside, d2, np.inf) >= kth * (1 - bound) - bound * d2).all()


def test_split_invariance_of_the_bits():
    (q, r, _) = floats()
    dim = q.shape[1]
    (dist, index, _) = case_neighbours(q, r, 32)
    assert np.array_equal(bits(case_neighbours(q, r, 1)[0][:, 0]), bits(dist[:, 0]))       # K = 1 and K = 32
    # 1 x 1 calls of sampled pairs of the lists
    for (i, s) in ((0, 0), (3, 0), (3, 1), (17, 31), (69, 5), (64, 16), (40, 9)):
        j = int(index[i, s])
        (d1, i1, c1) = case_neighbours(q[i:i + 1], r[j:j + 1], 1, ref_base=j)
        assert bits(d1)[0, 0] == bits(dist)[i, s] and i1[0, 0] == j and c1[0] == 1
    # other row positions: both sets reversed, the same pairs
    (rd, ri, _) = case_neighbours(q[::-1].copy(), r[::-1].copy(), 32)
    back = {(i, int(j)): b for i in range(len(q)) for (j, b) in zip(index[i], bits(dist)[i])}
    for i in range(len(q)):
        for (j, b) in zip(ri[len(q) - 1 - i], bits(rd)[len(q) - 1 - i]):
            pair = (i, len(r) - 1 - int(j))
            if pair in back:
                assert back[pair] == b
    assert np.array_equal(bits(rd[::-1]), bits(dist))           # as sorted values the lists are the same
    # other strides and alignment
    (qs, rs) = (dim + 3, dim + 5)
    qb = np.zeros(1 + len(q) * qs, dtype=np.float32)
    rb = np.zeros(3 + len(r) * rs, dtype=np.float32)
    for i in range(len(q)):
        qb[1 + i * qs:1 + i * qs + dim] = q[i]
    for j in range(len(r)):
        rb[3 + j * rs:3 + j * rs + dim] = r[j]
    got = raw_call(torch.from_numpy(qb).cuda(), len(q), qs, torch.from_numpy(rb).cuda(), len(r), rs, dim, 32, q_off=1, r_off=3)
    assert np.array_equal(bits(got[0]), bits(dist)) and np.array_equal(got[1], index)
    # under merge
    held = None
    for (r0, r1) in ((150, 300), (0, 150)):
        held = case_neighbours(q, r[r0:r1], 32, ref_base=r0, merge_into=held)
    assert np.array_equal(bits(held[0]), bits(dist)) and np.array_equal(held[1], index)


def test_same_call_twice_gives_the_same_bits():
    (q, r, _) = floats()
    (a, b) = (case_neighbours(q, r, 5, self_offset=2), case_neighbours(q, r, 5, self_offset=2))
    assert all(x.tobytes() == y.tobytes() for (x, y) in zip(a, b))


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _set(**changes):
    return lambda a: a.update(changes)


REFUSALS = {
    "k 0": _set(k=0), "k 33": _set(k=33), "negative n_query": _set(n_q=-1), "negative n_ref": _set(n_r=-1),
    "dim 0": _set(dim=0), "query stride short": _set(q_stride=7), "ref stride short": _set(r_stride=7),
    "indices beyond 2^31 - 1": _set(ref_base=2 ** 31 - 6), "negative ref_base": _set(ref_base=-1), "self_offset -2": _set(self_offset=-2),
    "merge 2": _set(merge=2), "merge -1": _set(merge=-1), "null dist2": _set(dist2=None), "null index": _set(index=None),
    "null count": _set(count=None), "null query": _set(q=None), "null ref": _set(r=None),
    "misaligned query": lambda a: a.update(q=a["q"] + 2), "misaligned ref": lambda a: a.update(r=a["r"] + 1),
    "misaligned dist2": lambda a: a.update(dist2=a["dist2"] + 4), "misaligned index": lambda a: a.update(index=a["index"] + 2),
    "misaligned count": lambda a: a.update(count=a["count"] + 1), "no workspace": _set(ws=None),
    "short workspace": lambda a: a.update(ws_bytes=a["ws_bytes"] - 1), "misaligned workspace": lambda a: a.update(ws=a["ws"] + 4),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_the_outputs(name):
    rng = np.random.default_rng(61)
    (q, r) = (torch.from_numpy(grid_rows(rng, 5, 8)).cuda(), torch.from_numpy(grid_rows(rng, 6, 8)).cuda())
    device = q.device
    outs = (torch.full((5, 3), 7.0, dtype=torch.float64, device=device), torch.full((5, 3), 7, dtype=torch.int32, device=device),
            torch.full((5,), 7, dtype=torch.int32, device=device))
    with pytest.raises(_lib.CaeError, match="cae_case_neighbours"):
        raw_call(q.reshape(-1), 5, 8, r.reshape(-1), 6, 8, 8, 3, outs=outs, mangle=REFUSALS[name])
    assert (outs[0] == 7.0).all() and (outs[1] == 7).all() and (outs[2] == 7).all()


def test_empty_calls():
    rng = np.random.default_rng(62)
    r = torch.from_numpy(grid_rows(rng, 6, 8)).cuda().reshape(-1)
    got = raw_call(None, 0, 8, r, 6, 8, 8, 3)                   # no query: success, nothing written
    assert (got[0] == 7.0).all() and (got[1] == 7).all() and (got[2] == 7).all()
    assert int(_lib.load().cae_case_neighbours_workspace_bytes(0, 6, 3)) == 0
    assert case_neighbours(np.zeros((0, 8), np.float32), np.zeros((6, 8), np.float32), 3)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        case_neighbours(np.zeros((2, 8), np.float32), np.zeros((6, 9), np.float32), 3)
    with pytest.raises(ValueError):
        case_neighbours(np.zeros((2, 8), np.float32), np.zeros((6, 8), np.float32), 33)


# ---- train_cae -> novelty -> apply_cae --novelty-variable ---------------------------------------------------------------

VARIABLES = ["lowres", "noise", "fixed"]
(COPY_TEST, COPY_TRAIN, FAR_TEST) = (2, 4, 7)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition with two more input variables, noise (seeded, per case) and fixed (one field repeated
    for every case, the static channel).  Test case 2 is a copy of training case 4; the inputs of test case 7 are scaled out
    of the training range."""
    from cae_tools_amd.data import datagen, netcdf3
    root = tmp_path_factory.mktemp("novelty")
    paths = {}
    fixed = np.random.default_rng(99).random((1, 1, 16, 16)).astype(np.float32)
    held = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        ds = datagen.generate("circle", 12, seed=seed)
        variables = {name: [tuple(da.dims), np.asarray(da.values).copy(), {}] for (name, da) in ds.data_vars.items()}
        variables["noise"] = [("n", "chan", "y1", "x1"), np.random.default_rng(seed).random((12, 1, 16, 16)).astype(np.float32), {}]
        variables["fixed"] = [("n", "chan", "y1", "x1"), np.repeat(fixed, 12, axis=0), {}]
        if part == "test":
            for name in variables:
                variables[name][1][COPY_TEST] = held[name][COPY_TRAIN]
            for name in ("lowres", "noise"):
                variables[name][1][FAR_TEST] = variables[name][1][FAR_TEST] * 4.0 + 3.0
        held = {name: v[1] for (name, v) in variables.items()}
        paths[part] = str(root / f"{part}.nc")
        netcdf3.write(paths[part], {d: int(k) for (d, k) in ds.dims.items()}, {name: tuple(v) for (name, v) in variables.items()})
    return root, paths


def _packed(model, ds):
    """the packed, normalised inputs in numpy, (n, D) fp32: the test's own packing, and the bits the model packs"""
    (lo, hi) = (model.normalisation_parameters[0], model.normalisation_parameters[1])
    planes = [importance_ref.normalise(np.asarray(ds[name].values).astype(np.float32), lo[name], hi[name], enable=model.normalise_input)
              for name in VARIABLES]
    x = np.concatenate(planes, axis=1)
    assert np.array_equal(x.view(np.uint32), model._packed_inputs(ds, VARIABLES).cpu().numpy().view(np.uint32))
    return x.reshape(len(x), -1)


def _number(v):
    return math.nan if v is None else float(v)


def _rank_average(v):
    return np.array([(v < x).sum() + ((v == x).sum() + 1) / 2.0 for x in v])


def _want_summary(novelty, nearest, nearest_case, loo_novelty, mse, mae):
    """the numbers of novelty_<partition>.json from per-case arrays, by the issue's definitions"""
    n = len(novelty)
    ref = np.sort(loo_novelty)
    want = {"novelty_min": novelty.min(), "novelty_median": float(np.median(novelty)), "novelty_max": novelty.max()}
    pct = {p: ref[max(1, -(-len(ref) * p // 100)) - 1] for p in (50, 90, 95, 99)}
    want["reference"] = pct
    want["outside_95"] = float((novelty > pct[95]).mean())
    want["outside_99"] = float((novelty > pct[99]).mean())
    (ra, rb) = (_rank_average(novelty), _rank_average(mse))
    want["spearman_mse"] = float(np.corrcoef(ra, rb)[0, 1])
    order = sorted(range(n), key=lambda c: (novelty[c], c))
    bins = [[] for _ in range(5)]
    for (rank, c) in enumerate(order):
        bins[5 * rank // n].append(c)
    want["quintiles"] = [(len(b), float(np.mean(mse[b])) if b else math.nan, float(np.mean(mae[b])) if b else math.nan) for b in bins]
    want["ratio"] = want["quintiles"][4][1] / want["quintiles"][0][1]
    most = sorted(range(n), key=lambda c: (-novelty[c], c))[:10]
    want["most_novel"] = [(c, int(nearest_case[c])) for c in most]
    return want


def _check_record(rec, case, loo, mse, mae, dim, tol):
    """every number of a novelty_<partition>.json against the restatement's lists `case` of the partition and `loo` of the
    reference set; tol: the relative bound of a novelty"""
    k = 5
    novelty = np.sqrt(case[0][:, k - 1] / dim)
    nearest = np.sqrt(case[0][:, 0] / dim)
    close = lambda got, want: abs(_number(got) - want) <= tol * abs(want) + 1e-300       # noqa: E731
    assert (rec["n_cases"], rec["valid_cases"], rec["k"], rec["features"]) == (len(novelty), len(novelty), k, dim)
    assert all(close(g, w) for (g, w) in zip(rec["case_novelty"], novelty))
    assert all(close(g, w) for (g, w) in zip(rec["case_nearest"], nearest))
    assert rec["case_nearest_case"] == case[1][:, 0].tolist()
    want = _want_summary(novelty, nearest, case[1][:, 0], np.sqrt(loo[0][:, k - 1] / dim), mse, mae)
    for key in ("novelty_min", "novelty_median", "novelty_max"):
        assert close(rec[key], want[key]), key
    assert rec["reference"]["n"] == len(loo[0])
    for p in (50, 90, 95, 99):
        assert close(rec["reference"][f"p{p}"], want["reference"][p]), p
    assert rec["outside_95"] == want["outside_95"] and rec["outside_99"] == want["outside_99"]
    assert abs(rec["spearman_mse"] - want["spearman_mse"]) <= 1e-12
    for (b, (cases, b_mse, b_mae)) in zip(rec["quintiles"], want["quintiles"]):
        assert b["cases"] == cases
        assert abs(_number(b["mse"]) - b_mse) <= 1e-11 * abs(b_mse) and abs(_number(b["mae"]) - b_mae) <= 1e-11 * abs(b_mae)     # 65536 u
    assert abs(rec["top_bottom_mse_ratio"] - want["ratio"]) <= 1e-11 * want["ratio"]
    assert [(m["case"], m["nearest_case"]) for m in rec["most_novel"]] == want["most_novel"]


def test_train_novelty_apply(data):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, novelty as cli, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.model_loader import load_model
    (root, paths) = data
    model_dir = str(root / "model")
    scored = {part: str(root / f"scored_{part}.nc") for part in paths}
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", *VARIABLES, "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        for part in paths:
            apply_cae.main([paths[part], scored[part], "--model-folder", model_dir])
    out = str(root / "report")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--train-inputs", scored["train"], "--test-inputs", scored["test"], "--model-folder", model_dir,
                  "--output-html-folder", out])
    assert sorted(f for f in os.listdir(out) if f.startswith("novelty_")) == ["novelty_test.json", "novelty_train.json"]
    recs = {}
    for part in paths:
        with open(os.path.join(out, f"novelty_{part}.json")) as f:
            recs[part] = json.load(f)

    # the restatement on the test's own packing
    model = load_model(model_dir)
    ds = {part: open_dataset(scored[part]) for part in paths}
    with redirect_stdout(io.StringIO()):
        x = {part: _packed(model, ds[part]) for part in paths}
    dim = x["train"].shape[1]
    assert dim == 3 * 16 * 16
    loo = neighbours_ref.neighbours(x["train"], x["train"], 5, self_offset=0)
    test = neighbours_ref.neighbours(x["test"], x["train"], 5)
    tol = (dim + 8) * U         # (2 D + 8) u on d2 from both sides, halved by the root, and the division's and the root's own roundings
    errors = {}
    for part in paths:
        (p, a) = (np.asarray(ds[part]["model_output"].values)[:, 0].astype(np.float64), np.asarray(ds[part]["hires"].values)[:, 0].astype(np.float64))
        errors[part] = (((p - a) ** 2).mean(axis=(1, 2)), np.abs(p - a).mean(axis=(1, 2)))
    _check_record(recs["train"], loo, loo, *errors["train"], dim, tol)
    _check_record(recs["test"], test, loo, *errors["test"], dim, tol)
    assert recs["test"]["reference_cases"] == recs["test"]["valid_reference_cases"] == 12
    # leave-one-out: no training case names itself
    assert all(c != i for (i, c) in enumerate(recs["train"]["case_nearest_case"]))
    # the copy of a training case: nearest exactly 0 and that case; the case scaled out of the training range is the most novel
    assert recs["test"]["case_nearest"][COPY_TEST] == 0.0 and recs["test"]["case_nearest_case"][COPY_TEST] == COPY_TRAIN
    assert recs["test"]["most_novel"][0]["case"] == FAR_TEST
    assert recs["test"]["case_novelty"][FAR_TEST] > recs["train"]["reference"]["p99"] and recs["test"]["outside_99"] > 0.0

    # the line and the report
    lines = log.getvalue().splitlines()
    assert [ln for ln in lines if ln.startswith("novelty test: 12 cases against 12 reference cases, k 5, 768 features: median ")]
    assert [ln for ln in lines if ln.startswith("novelty train: 12 cases against 12 reference cases, k 5, 768 features: median ")]
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Novelty of the cases</h2>") == 1 and page.count('alt="test mse by novelty quintile"') == 1
    assert page.count('alt="train mse by novelty quintile"') == 1

    # evaluate_cae itself on the same input: no novelty file, no section, and the page it has always written
    plain_out = str(root / "report_plain")
    plain_log = io.StringIO()
    with redirect_stdout(plain_log):
        evaluate_cae.main(["--train-inputs", scored["train"], "--test-inputs", scored["test"], "--model-folder", model_dir,
                           "--output-html-folder", plain_out])
    assert not [f for f in os.listdir(plain_out) if f.startswith("novelty")] and "novelty" not in plain_log.getvalue()
    with open(os.path.join(plain_out, "index.html")) as f:
        plain = f.read()
    (start, end) = (page.index("<h2>Novelty of the cases</h2>"), page.index("<h2>Training Summary</h2>"))
    assert page[:start] + page[end:] == plain

    # apply_cae --novelty-variable stores the same numbers; without the flags the file is what it was
    (with_flag, again) = (str(root / "applied_novelty.nc"), str(root / "applied_again.nc"))
    with redirect_stdout(io.StringIO()):
        apply_cae.main([paths["test"], with_flag, "--model-folder", model_dir, "--novelty-variable", "novelty", "--novelty-reference",
                        paths["train"]])
        apply_cae.main([paths["test"], again, "--model-folder", model_dir])
    stored = open_dataset(with_flag)
    assert tuple(stored["novelty"].dims) == ("n",) and np.asarray(stored["novelty"].values).dtype == np.float64
    assert np.array_equal(np.asarray(stored["novelty"].values), np.array(recs["test"]["case_novelty"], dtype=np.float64))
    with open(again, "rb") as f, open(scored["test"], "rb") as g:
        assert f.read() == g.read()
    plain_ds = open_dataset(again)
    assert sorted(set(stored.data_vars) - set(plain_ds.data_vars)) == ["novelty"]
    assert all(np.asarray(stored[name].values).tobytes() == np.asarray(plain_ds[name].values).tobytes() for name in plain_ds.data_vars)

    # the cut of the references changes nothing; another k through the Python API
    with redirect_stdout(io.StringIO()):
        one = model.novelty(ds["test"], ds["train"], VARIABLES, k=3)
        cut = model.novelty(ds["test"], ds["train"], VARIABLES, k=3, reference_chunk=5)
        few = model.novelty(ds["test"], ds["train"], VARIABLES, k=32)
    assert all(np.asarray(one[key]).tobytes() == np.asarray(cut[key]).tobytes() for key in ("novelty", "nearest", "index", "dist2", "count"))
    assert np.array_equal(one["index"], neighbours_ref.neighbours(x["test"], x["train"], 3)[1])
    assert np.isinf(few["novelty"]).all() and (few["count"] == 12).all()        # fewer than k valid references: +inf


def _square(path_in, path_out):
    """the three inputs and the target at 64 x 64 on both sides (a UNET's decoder mirrors its encoder)"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import open_dataset
    ds = open_dataset(path_in)
    variables = {name: (("n", "chan", "y", "x"), np.repeat(np.repeat(np.asarray(ds[name].values), 4, axis=2), 4, axis=3).astype(np.float32),
                        {}) for name in VARIABLES}
    hi = np.asarray(ds["hires"].values).astype(np.float64)
    variables["hires"] = (("n", "chan", "y", "x"), hi.reshape(12, 1, 64, 4, 64, 4).mean(axis=(3, 5)).astype(np.float32), {})
    variables["valid"] = (("n", "chan", "y", "x"), np.ones((12, 1, 64, 64), dtype=np.float32), {})
    netcdf3.write(path_out, {"n": 12, "chan": 1, "y": 64, "x": 64}, variables)


@pytest.mark.parametrize("method", ["linear", "unet", "var"])
def test_the_commands_for_every_other_model_class(data, method):
    """cli.novelty and apply_cae --novelty-variable on a linear, unet and var model folder: the novelty uses the packing
    alone, so the copy and the far case are found whatever the model"""
    from cae_tools_amd.cli import apply_cae, novelty as cli, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    (root, paths) = data
    extra = []
    if method == "unet":
        from cae_tools_amd.models.unet import unet_layer_spec
        paths = {part: str(root / f"square_{part}.nc") for part in ("train", "test")}
        for part in paths:
            _square(data[1][part], paths[part])
        layers = str(root / "unet_layers.json")
        with open(layers, "w") as f:
            json.dump(unet_layer_spec(3, 1, (64, 64), [8, 16]).save(), f)
        extra = ["--layer-definitions-path", layers, "--mask-variable", "valid"]
    model_dir = str(root / f"model_{method}")
    out = str(root / f"report_{method}")
    applied = str(root / f"applied_{method}.nc")
    torch.manual_seed(0)
    log = io.StringIO()
    with redirect_stdout(log):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", *VARIABLES, "--output-variable", "hires", "--method", method, "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"] + extra)
        cli.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                  "--output-html-folder", out, "--novelty-k", "2"])
        apply_cae.main([paths["test"], applied, "--model-folder", model_dir, "--novelty-variable", "nov", "--novelty-reference",
                        paths["train"], "--novelty-k", "2"])
    with open(os.path.join(out, "novelty_test.json")) as f:
        rec = json.load(f)
    with open(os.path.join(out, "novelty_train.json")) as f:
        own = json.load(f)
    side = 64 if method == "unet" else 16
    assert (rec["n_cases"], rec["k"], rec["features"], rec["reference_cases"]) == (12, 2, 3 * side * side, 12)
    assert rec["case_nearest"][COPY_TEST] == 0.0 and rec["case_nearest_case"][COPY_TEST] == COPY_TRAIN
    assert rec["most_novel"][0]["case"] == FAR_TEST
    assert all(c != i for (i, c) in enumerate(own["case_nearest_case"]))
    assert np.array_equal(np.asarray(open_dataset(applied)["nov"].values), np.array(rec["case_novelty"], dtype=np.float64))
    assert [ln for ln in log.getvalue().splitlines() if ln.startswith("novelty test: 12 cases against 12 reference cases, k 2")]
    with open(os.path.join(out, "index.html")) as f:
        assert f.read().count("<h2>Novelty of the cases</h2>") == 1
