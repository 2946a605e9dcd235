"""What the host side of cae_joint_hist refuses, as test_stateless_refusals_cpu.py holds it for its neighbours: the return code
and the exact cae_last_error() text of one bad call per check, and the empty calls that return CAE_OK before they look at an
operand.

The addresses are made-up integers that no call here dereferences: every row is answered by the host before a launch (an
empty call zeroes the outputs it is given, so the empty rows give none).  The module is skipped where a GPU is present, so
that a row that slipped past the checks ends in HIP's no-device error and never in a launch with those addresses; on the GPU
test_joint_hist_gpu.py covers the refusals with real buffers.  The shape is 3 cases of plane 35, 8 bins of 4: one workgroup,
whose partial is 2 x 8 x 4 doubles."""
import math

import pytest
import torch

from cae_tools_amd import _lib

if torch.cuda.is_available():
    pytest.skip("the refusal table runs without a GPU only: its addresses are made up", allow_module_level=True)

(OK, ARG) = (0, -1)
(P, A, JOINT, MARG, COND, OUTSIDE, WS) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000)
BIG = 1 << 59       # as a case stride of 3 cases: 2 * 2^59 + plane elements from the pointer, above 2^60

NAMES = ("pred pred_kind pred_stride actual actual_kind actual_stride n_case plane lo hi n_bin sub joint marg cond outside "
         "workspace workspace_bytes stream").split()
CALL = dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=70, n_case=3, plane=35, lo=0.0, hi=1.0,
            n_bin=8, sub=4, joint=JOINT, marg=MARG, cond=COND, outside=OUTSIDE, workspace=WS, workspace_bytes=512, stream=None)
NO_OUTPUT = dict(pred=None, actual=None, joint=None, marg=None, cond=None, outside=None, workspace=None, workspace_bytes=0)

TABLE = [
    (ARG, "cae_joint_hist: bad argument (CAE_ELEM_* kinds, n_case >= 0, plane >= 0, 1 <= n_bin <= 128, 1 <= sub <= 32, "
          "n_case * plane < 2^40)",
     [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1),
      dict(n_bin=0), dict(n_bin=129), dict(sub=0), dict(sub=33),
      dict(n_case=1 << 20, plane=1 << 20, pred_stride=1 << 20, actual_stride=1 << 20)]),
    (ARG, "cae_joint_hist: lo and hi must be finite, hi > lo, and n_bin * sub / (hi - lo) finite and not zero",
     [dict(hi=0.0), dict(hi=-1.0), dict(lo=math.nan), dict(hi=math.nan), dict(lo=-math.inf), dict(hi=math.inf),
      dict(lo=0.0, hi=5e-324), dict(lo=-1.7e308, hi=1.7e308)]),
    (ARG, "cae_joint_hist: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1)]),
    (ARG, "cae_joint_hist: the outputs must be 8-byte aligned",
     [dict(joint=JOINT + 4), dict(marg=MARG + 2), dict(cond=COND + 4), dict(outside=OUTSIDE + 1)]),
    (OK, "", [dict(n_case=0, **NO_OUTPUT), dict(plane=0, **NO_OUTPUT), dict(n_case=0, plane=0, **NO_OUTPUT)]),
    (ARG, "cae_joint_hist: null pointer",
     [dict(pred=None), dict(actual=None), dict(joint=None), dict(marg=None), dict(cond=None), dict(outside=None)]),
    (ARG, "cae_joint_hist: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
    (ARG, "cae_joint_hist: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
    (ARG, "cae_joint_hist: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 4)]),
    (ARG, "cae_joint_hist: needs a workspace of 512 bytes (cae_joint_hist_workspace_bytes)",
     [dict(workspace=None), dict(workspace_bytes=511), dict(workspace=WS + 4)]),
]

ROWS = [(rc, text, change) for (rc, text, changes) in TABLE for change in changes]


def _row_id(row):
    return ",".join(f"{k}={v}" for (k, v) in row[2].items())


def test_the_rows_are_distinct_and_the_call_needs_that_workspace():
    assert len(set(map(_row_id, ROWS))) == len(ROWS)
    assert list(CALL) == NAMES
    assert _lib.load().cae_joint_hist_workspace_bytes(3, 35, 8, 4) == 512


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refusal(row):
    """the call is answered by the host, with this code and this text"""
    (rc, text, change) = row
    lib = _lib.load()
    args = dict(CALL, **change)
    assert set(change) <= set(CALL)
    got = lib.cae_joint_hist(*(args[n] for n in NAMES))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
