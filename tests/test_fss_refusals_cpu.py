"""What the host side of cae_case_fss refuses, as test_strata_refusals_cpu.py holds it for its neighbour: the return code and
the exact cae_last_error() text of one bad call per check, and the empty calls that return CAE_OK before they look at a
pointer.

The device addresses are made-up integers that no call here dereferences: every row is answered by the host before a launch
(an empty call zeroes the output it is given, so the empty rows give none).  The thresholds, sides and widths are host arrays,
which the call does read.  The module is skipped where a GPU is present, so that a row that slipped past the checks ends in
HIP's no-device error and never in a launch with those addresses; on the GPU test_fss_gpu.py covers the refusals with real
buffers.  The shape is 3 cases of 5 x 70 under 2 thresholds: 3 * (1 + 2 * 2) * 5 * 2 words of bit-planes, 1200 bytes."""
import ctypes as C
import math

import pytest
import torch

from cae_tools_amd import _lib

if torch.cuda.is_available():
    pytest.skip("the refusal table runs without a GPU only: its addresses are made up", allow_module_level=True)

(OK, ARG) = (0, -1)
(P, A, SUMS, WS) = (0x10000, 0x20000, 0x40000, 0x60000)
BIG = 1 << 59       # as a case stride of 3 cases: 2 * 2^59 + plane elements from the pointer, above 2^60


def _doubles(*v):
    return (C.c_double * len(v))(*v)


def _ints(*v):
    return (C.c_int * len(v))(*v)


NAMES = ("pred pred_kind pred_stride actual actual_kind actual_stride n_case h w thresholds sides n_thr widths n_width gap_rule "
         "sums workspace workspace_bytes stream").split()
CALL = dict(pred=P, pred_kind=0, pred_stride=350, actual=A, actual_kind=3, actual_stride=700, n_case=3, h=5, w=70,
            thresholds=_doubles(0.25, 0.75), sides=_ints(1, 0), n_thr=2, widths=_ints(1, 3, 5), n_width=3, gap_rule=0, sums=SUMS,
            workspace=WS, workspace_bytes=1200, stream=None)
NO_POINTER = dict(pred=None, actual=None, thresholds=None, sides=None, widths=None, sums=None, workspace=None, workspace_bytes=0)

TABLE = [
    (ARG, "cae_case_fss: bad argument (CAE_ELEM_* kinds, 0 <= n_case <= 2^40, sides of 0 to 16384, 1 <= n_thr <= 8, 1 <= n_width <= 8, "
          "gap_rule 0 or 1)",
     [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(n_case=(1 << 40) + 1),
      dict(h=-1), dict(w=-1), dict(h=16385), dict(w=16385), dict(n_thr=0), dict(n_thr=9), dict(n_width=0), dict(n_width=9),
      dict(gap_rule=-1), dict(gap_rule=2)]),
    (ARG, "cae_case_fss: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1)]),
    (ARG, "cae_case_fss: the output must be 8-byte aligned", [dict(sums=SUMS + 4), dict(sums=SUMS + 1)]),
    (OK, "", [dict(n_case=0, **NO_POINTER), dict(h=0, **NO_POINTER), dict(w=0, **NO_POINTER), dict(n_case=0, h=0, w=0, **NO_POINTER),
              dict(n_case=0)]),
    (ARG, "cae_case_fss: null pointer",
     [dict(pred=None), dict(actual=None), dict(thresholds=None), dict(sides=None), dict(widths=None), dict(sums=None)]),
    (ARG, "cae_case_fss: the thresholds must be finite",
     [dict(thresholds=_doubles(math.nan, 0.75)), dict(thresholds=_doubles(0.25, math.inf)), dict(thresholds=_doubles(-math.inf, 0.75))]),
    (ARG, "cae_case_fss: a side must be 0 (above) or 1 (below)", [dict(sides=_ints(2, 0)), dict(sides=_ints(0, -1))]),
    (ARG, "cae_case_fss: the widths must be odd, from 1 to 129 and strictly ascending",
     [dict(widths=_ints(1, 2, 5)), dict(widths=_ints(0, 3, 5)), dict(widths=_ints(-1, 3, 5)), dict(widths=_ints(1, 3, 131)),
      dict(widths=_ints(1, 5, 3)), dict(widths=_ints(1, 3, 3))]),
    (ARG, "cae_case_fss: a case stride is shorter than the plane", [dict(pred_stride=349), dict(actual_stride=349)]),
    (ARG, "cae_case_fss: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
    (ARG, "cae_case_fss: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 4)]),
    (ARG, "cae_case_fss: needs a workspace of 1200 bytes (cae_case_fss_workspace_bytes)",
     [dict(workspace=None), dict(workspace_bytes=1199), dict(workspace=WS + 4)]),
]

ROWS = [(rc, text, change) for (rc, text, changes) in TABLE for change in changes]


def _row_id(row):
    return ",".join(f"{k}={'array' if isinstance(v, C.Array) else v}" for (k, v) in row[2].items()) + f"#{ROWS.index(row)}"


def test_the_call_needs_that_workspace():
    lib = _lib.load()
    assert list(CALL) == NAMES
    assert lib.cae_case_fss_workspace_bytes(3, 5, 70, 2) == 1200
    # 2000 cases of 256 x 256 under four thresholds: nine planes of 8 KiB a case
    assert lib.cae_case_fss_workspace_bytes(2000, 256, 256, 4) == 2000 * 9 * 8192
    assert lib.cae_case_fss_workspace_bytes(1, 16384, 16384, 8) == 17 * 16384 * 256 * 8
    # 0 only for an empty or a refused call
    for args in ((0, 5, 7, 2), (3, 0, 7, 2), (3, 5, 0, 2), (3, 5, 7, 0), (3, 5, 7, 9), (-1, 5, 7, 2), (3, 16385, 7, 2), (3, 5, 16385, 2)):
        assert lib.cae_case_fss_workspace_bytes(*args) == 0, args


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refusal(row):
    """the call is answered by the host, with this code and this text"""
    (rc, text, change) = row
    lib = _lib.load()
    args = dict(CALL, **change)
    assert set(change) <= set(CALL)
    got = lib.cae_case_fss(*(args[n] for n in NAMES))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
