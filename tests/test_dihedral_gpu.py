"""cae_dihedral_rows on the GPU against the numpy definition of a code (utils/augment.apply), bit for bit: the kernel moves
32-bit words, so every comparison is np.array_equal on view(np.uint32) and there is no tolerance.

Shapes: group 8 on the planes 1, 2, 31, 33, 64 and 65 a side - below, at and above the 64-word LDS tile, more than one tile
with a ragged edge - and group 4 on 3 x 70, 70 x 3 and 5 x 7, each with 1 and 3 channels.  9 destination rows from 5 source
rows: every code of the group, one source row taken twice, a row index of -1 and one of n_src, a code of `group` and one of
-1 (a NaN row each), a NaN with a payload and a -0.0 in the source, a guard band behind the last row.  rows=None is run
once per shape.  One more call has more tiles than the launch's grid cap (DH_MAX_GROUPS workgroups, host_dihedral.h), so
that every workgroup walks its loop more than once, with both a copying and a transposing code.  Then the refusals, with
real buffers."""
import os
import re

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib
from cae_tools_amd.case_ops import dihedral_rows
from cae_tools_amd.utils import augment

pytestmark = pytest.mark.gpu

QNAN = np.uint32(0x7fc00000)
GUARD = np.uint32(0x4b1d4b1d)
PAYLOAD = np.uint32(0x7fa12345)     # a NaN that carries a payload (a signalling one: arithmetic would quiet it)
NEG_ZERO = np.uint32(0x80000000)
(N_SRC, N_DST) = (5, 9)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae_tools_amd", "csrc")


def _source(c, h, w, seed):
    """(N_SRC, c, h, w) words, all different, with the NaN payload and the -0.0 where the plane has room for them"""
    rng = np.random.default_rng(seed)
    words = rng.standard_normal((N_SRC, c, h, w)).astype(np.float32).view(np.uint32).copy()
    words[1, 0, 0, 0] = PAYLOAD
    words[2, c - 1, h - 1, w - 1] = NEG_ZERO
    return words


def _expected(words, rows, codes, group):
    (n_src, c, h, w) = words.shape
    out = np.empty((len(codes), c, h, w), dtype=np.uint32)
    for (i, (r, g)) in enumerate(zip(rows, codes)):
        out[i] = augment.apply(words[r], g) if 0 <= r < n_src and 0 <= g < group else QNAN
    return out


def _run(words, rows, codes, group, n_dst=None):
    """dihedral_rows into a buffer with a guard band behind the last row: (the rows as words, the band)"""
    (_, c, h, w) = words.shape
    n_dst = len(codes) if n_dst is None else n_dst
    per = c * h * w
    flat = torch.from_numpy(np.full(n_dst * per + 64, GUARD, dtype=np.uint32).view(np.float32)).cuda()
    dst = flat[:n_dst * per].view(n_dst, c, h, w)
    src = torch.from_numpy(words.view(np.float32)).cuda()
    rows_dev = None if rows is None else torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda()
    dihedral_rows(src, dst, torch.from_numpy(np.asarray(codes, dtype=np.int32)).cuda(), rows_dev, group)
    torch.cuda.synchronize()
    got = flat.cpu().numpy().view(np.uint32)
    return got[:n_dst * per].reshape(n_dst, c, h, w), got[n_dst * per:]


SHAPES = [(8, s, s) for s in (1, 2, 31, 33, 64, 65)] + [(4, 3, 70), (4, 70, 3), (4, 5, 7)]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("group, h, w", SHAPES)
def test_rows_against_the_numpy_definition(group, h, w, c):
    words = _source(c, h, w, seed=h * 131 + w * 7 + c)
    # every code of the group on a valid row, source row 3 twice, and the four NaN rows.  Nine rows do not hold eight codes
    # and four NaN rows: group 8 takes a second call of nine rows for three of them.
    if group == 8:
        (rows, codes) = ([3, 1, 2, 3, 0, 4, 2, 1, 0], list(range(8)) + [8])
        second = ([-1, N_SRC, 2, 1, 0, 4, 3, 2, 1], [5, 6, -1, 7, 4, 3, 2, 1, 0])
    else:
        (rows, codes) = ([3, 1, 2, 3, 0, -1, 2, N_SRC, 4], [0, 1, 2, 3, group, 1, -1, 2, 3])
        second = None
    assert len(codes) == len(rows) == N_DST and set(range(group)) <= set(codes) and len(set(rows)) < len(rows)
    calls = [(rows, codes)] + ([second] if second else [])
    bad_rows = sum(1 for (rs, cs) in calls for r in rs if not 0 <= r < N_SRC)
    bad_codes = [g for (rs, cs) in calls for g in cs if not 0 <= g < group]
    assert bad_rows == 2 and sorted(bad_codes) == [-1, group]
    for (rs, cs) in calls:
        (got, band) = _run(words, rs, cs, group)
        want = _expected(words, rs, cs, group)
        assert np.array_equal(got, want), [i for i in range(N_DST) if not np.array_equal(got[i], want[i])]
        assert (band == GUARD).all()
    # the payload and the -0.0 arrived as they were (the first call takes source rows 1 and 2 with valid codes)
    first = _run(words, rows, codes, group)[0]
    assert (first == PAYLOAD).sum() == rows.count(1) and (first == NEG_ZERO).sum() == rows.count(2) - (group == 4)
    # rows=None: row i of the source, so N_SRC destination rows
    cs = [(3 * i + 1) % group for i in range(N_SRC)]
    (got, band) = _run(words, None, cs, group)
    assert np.array_equal(got, _expected(words, list(range(N_SRC)), cs, group)) and (band == GUARD).all()


def test_more_tiles_than_the_grid_cap():
    """c = 1 and 2 x 2 planes: a tile per row, so cap + 7 rows are the fewest rows whose tiles exceed the cap; the first 7
    workgroups take a second tile.  Codes cycle through all 8, a NaN row at either end of the second trip."""
    with open(os.path.join(CSRC, "host_dihedral.h")) as f:
        cap = int(re.search(r"constexpr int64_t DH_MAX_GROUPS = (\d+);", f.read()).group(1))
    n_dst = cap + 7
    words = _source(1, 2, 2, seed=5)
    rows = [(7 * i + 3) % N_SRC for i in range(n_dst)]
    codes = [i % 8 for i in range(n_dst)]
    (rows[cap], codes[n_dst - 1]) = (N_SRC, 8)
    (got, band) = _run(words, rows, codes, 8)
    assert np.array_equal(got, _expected(words, rows, codes, 8)) and (band == GUARD).all()
    assert (got[cap] == QNAN).all() and (got[n_dst - 1] == QNAN).all() and not (got[cap + 1] == QNAN).any()


def test_refusals_with_real_buffers():
    lib = _lib.load()
    src = torch.zeros((5, 2, 6, 6), dtype=torch.float32, device="cuda")
    dst = torch.full((9, 2, 6, 6), 3.0, dtype=torch.float32, device="cuda")
    codes = torch.zeros(9, dtype=torch.int32, device="cuda")
    rows = torch.zeros(9, dtype=torch.int32, device="cuda")
    wide = torch.zeros((5, 2, 6, 8), dtype=torch.float32, device="cuda")

    def call(src_p=src.data_ptr(), n_src=5, c=2, h=6, w=6, dst_p=dst.data_ptr(), n_dst=9, rows_p=rows.data_ptr(),
             codes_p=codes.data_ptr(), group=8):
        rc = lib.cae_dihedral_rows(src_p, n_src, c, h, w, dst_p, n_dst, rows_p, codes_p, group, None)
        return rc, (lib.cae_last_error().decode() if rc else "")

    bad = "cae_dihedral_rows: bad argument (n_src >= 0, n_dst >= 0, c >= 1, h >= 0, w >= 0, group 4 or 8)"
    for change in (dict(n_src=-1), dict(n_dst=-1), dict(c=0), dict(h=-1), dict(w=-1), dict(group=5), dict(group=0)):
        assert call(**change) == (-1, bad), change
    assert call(src_p=wide.data_ptr(), w=8) == (-1, "cae_dihedral_rows: group 8 transposes, which needs square planes (h == w)")
    assert call(src_p=wide.data_ptr(), w=8, n_dst=0, group=4) == (0, "")
    assert call(n_src=1 << 31) == (-1, "cae_dihedral_rows: more than 2^31 - 1 rows")
    for change in (dict(n_dst=0, dst_p=None, codes_p=None), dict(h=0, w=0, src_p=None, dst_p=None, codes_p=None)):
        assert call(**change) == (0, ""), change
    for change in (dict(src_p=None), dict(dst_p=None), dict(codes_p=None)):
        assert call(**change) == (-1, "cae_dihedral_rows: null pointer"), change
    assert call(n_src=1 << 30, h=1 << 15, w=1 << 15, group=8) == (-1, "cae_dihedral_rows: an operand reaches 2^60 elements from its pointer")
    for change in (dict(src_p=src.data_ptr() + 2), dict(dst_p=dst.data_ptr() + 1), dict(rows_p=rows.data_ptr() + 2),
                   dict(codes_p=codes.data_ptr() + 1)):
        assert call(**change) == (-1, "cae_dihedral_rows: pointers must be 4-byte aligned"), change
    for change in (dict(dst_p=src.data_ptr(), n_dst=5), dict(dst_p=src.data_ptr() + 4 * 72 * 4, n_dst=2),
                   dict(src_p=dst.data_ptr() + 4 * 72 * 8, n_src=1)):
        assert call(**change) == (-1, "cae_dihedral_rows: dst overlaps src"), change
    torch.cuda.synchronize()
    assert (dst == 3.0).all()       # nothing was written by a refused call
    assert call(rows_p=None, n_dst=5) == (0, "")        # rows = NULL is row i
    # the wrapper's own checks come before the call
    with pytest.raises(ValueError, match="group 8 transposes, which needs square planes, got 6 x 8"):
        dihedral_rows(wide, torch.empty_like(wide), codes[:5], None, 8)
    with pytest.raises(ValueError, match="codes must be a contiguous int32 tensor of one entry per row of dst"):
        dihedral_rows(src, dst, codes[:5], None, 8)
    with pytest.raises(ValueError, match="src must be a contiguous float32 CUDA tensor"):
        dihedral_rows(src.double(), dst, codes, None, 8)
