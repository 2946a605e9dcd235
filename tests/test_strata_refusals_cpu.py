"""What the host side of cae_strata_sums refuses, as test_joint_hist_refusals_cpu.py holds it for its neighbour: the return
code and the exact cae_last_error() text of one bad call per check, and the empty calls that return CAE_OK before they look at
a pointer.

The device addresses are made-up integers that no call here dereferences: every row is answered by the host before a launch
(an empty call zeroes the outputs it is given, so the empty rows give none).  The edges and shifts are host arrays, which
the call does read.  The module is skipped where a GPU is present, so that a row that slipped past the checks ends in HIP's
no-device error and never in a launch with those addresses; on the GPU test_strata_gpu.py covers the refusals with real
buffers.  The shape is 3 cases of 5 x 7 under a 2 x 3 stratifier with 3 edges: one workgroup, whose partial is 4 x 8 doubles."""
import ctypes as C
import math

import pytest
import torch

from cae_tools_amd import _lib

if torch.cuda.is_available():
    pytest.skip("the refusal table runs without a GPU only: its addresses are made up", allow_module_level=True)

(OK, ARG) = (0, -1)
(P, A, S, COUNTS, SUMS, WS) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)
BIG = 1 << 59       # as a case stride of 3 cases: 2 * 2^59 + plane elements from the pointer, above 2^60


def _doubles(*v):
    return (C.c_double * len(v))(*v)


NAMES = ("pred pred_kind pred_stride actual actual_kind actual_stride strata strata_kind strata_stride n_case h w sh sw edges "
         "n_edge shift_a shift_p counts sums workspace workspace_bytes stream").split()
CALL = dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=70, strata=S, strata_kind=1, strata_stride=6,
            n_case=3, h=5, w=7, sh=2, sw=3, edges=_doubles(0.0, 0.5, 1.0), n_edge=3, shift_a=_doubles(0.0, 0.0, 0.0, 0.0),
            shift_p=_doubles(1.0, 2.0, 3.0, 4.0), counts=COUNTS, sums=SUMS, workspace=WS, workspace_bytes=256, stream=None)
NO_POINTER = dict(pred=None, actual=None, strata=None, edges=None, shift_a=None, shift_p=None, counts=None, sums=None, workspace=None,
                  workspace_bytes=0)

TABLE = [
    (ARG, "cae_strata_sums: bad argument (CAE_ELEM_* kinds, n_case >= 0, target sides of 0 to 2^30, stratifier sides of 1 to 2^30, "
          "0 <= n_edge <= 63)",
     [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(strata_kind=-1), dict(strata_kind=4), dict(n_case=-1),
      dict(h=-1), dict(w=-1), dict(h=(1 << 30) + 1), dict(w=(1 << 30) + 1), dict(sh=0), dict(sw=0), dict(sh=(1 << 30) + 1),
      dict(sw=(1 << 30) + 1), dict(n_edge=-1), dict(n_edge=64)]),
    (ARG, "cae_strata_sums: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1), dict(strata_stride=-1)]),
    (ARG, "cae_strata_sums: the outputs must be 8-byte aligned", [dict(counts=COUNTS + 4), dict(sums=SUMS + 2)]),
    (OK, "", [dict(n_case=0, **NO_POINTER), dict(h=0, **NO_POINTER), dict(w=0, **NO_POINTER), dict(n_case=0, h=0, w=0, **NO_POINTER)]),
    (ARG, "cae_strata_sums: null pointer",
     [dict(pred=None), dict(actual=None), dict(strata=None), dict(edges=None), dict(shift_a=None), dict(shift_p=None),
      dict(counts=None), dict(sums=None)]),
    (ARG, "cae_strata_sums: the edges must be finite and strictly ascending",
     [dict(edges=_doubles(0.0, 0.0, 1.0)), dict(edges=_doubles(0.0, 1.0, 0.5)), dict(edges=_doubles(math.nan, 0.5, 1.0)),
      dict(edges=_doubles(0.0, 0.5, math.inf)), dict(edges=_doubles(-math.inf, 0.5, 1.0))]),
    (ARG, "cae_strata_sums: the shifts must be finite",
     [dict(shift_a=_doubles(0.0, math.nan, 0.0, 0.0)), dict(shift_p=_doubles(0.0, 0.0, 0.0, math.inf))]),
    (ARG, "cae_strata_sums: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34), dict(strata_stride=5)]),
    (ARG, "cae_strata_sums: an operand reaches 2^60 elements from its pointer",
     [dict(pred_stride=BIG), dict(actual_stride=BIG), dict(strata_stride=BIG)]),
    (ARG, "cae_strata_sums: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 4), dict(strata=S + 2)]),
    (ARG, "cae_strata_sums: needs a workspace of 256 bytes (cae_strata_sums_workspace_bytes)",
     [dict(workspace=None), dict(workspace_bytes=255), dict(workspace=WS + 4)]),
]

ROWS = [(rc, text, change) for (rc, text, changes) in TABLE for change in changes]


def _row_id(row):
    return ",".join(f"{k}={'array' if isinstance(v, C.Array) else v}" for (k, v) in row[2].items()) + f"#{ROWS.index(row)}"


def test_the_call_needs_that_workspace():
    lib = _lib.load()
    assert list(CALL) == NAMES
    assert lib.cae_strata_sums_workspace_bytes(3, 5, 7, 4) == 256
    # 17 cases of 4099 pixels: 34 (case, chunk) items, nine workgroups of four waves
    assert lib.cae_strata_sums_workspace_bytes(17, 1, 4099, 7) == 9 * 7 * 8 * 8
    # 0 only for an empty or a refused call
    for args in ((0, 5, 7, 4), (3, 0, 7, 4), (3, 5, 0, 4), (3, 5, 7, 0), (3, 5, 7, 65), (-1, 5, 7, 4), (3, (1 << 30) + 1, 7, 4)):
        assert lib.cae_strata_sums_workspace_bytes(*args) == 0, args


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refusal(row):
    """the call is answered by the host, with this code and this text"""
    (rc, text, change) = row
    lib = _lib.load()
    args = dict(CALL, **change)
    assert set(change) <= set(CALL)
    got = lib.cae_strata_sums(*(args[n] for n in NAMES))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
