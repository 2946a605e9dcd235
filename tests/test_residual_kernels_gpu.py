"""cae_residual_scan / cae_residual_pack_rows / cae_residual_restore_f64 on the GPU against the numpy restatement
(residual_ref.py), bit for bit.  The base field b is the one case_ops.upsample returns (cae_case_baseline's field, which
test_case_baseline_gpu.py holds to the definition); given b, every operation of scan, pack and restore is one fp64 or fp32
rounding that numpy performs the same way, so the count, the minimum and the maximum are compared with == and y and p through
their integer views.  No tolerance anywhere; the consistency bound of DESIGN.md section 9 is asserted on top."""
import numpy as np
import pytest
import torch

import residual_ref
from cae_tools_amd import _lib
from cae_tools_amd.case_ops import device_operand, upsample
from cae_tools_amd.device_ops import residual_pack, residual_restore, residual_scan

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
MODES = ("nearest", "bilinear", "bicubic")
N = 3
# (5, 3) -> (70, 130): two bands x three strips, both tails, a ratio that is no integer, five workgroups; one item; one input
# pixel; equal sizes; downsampling
SHAPES = [((5, 3), (70, 130)), ((4, 4), (64, 64)), ((1, 1), (8, 8)), ((8, 8), (8, 8)), ((16, 16), (8, 8))]


def _fields(i, o, seed, n=N, channels=1):
    """a temperature-like pair as fp32: low (n, channels, h, w) and target (n, 1, H, W)"""
    rng = np.random.default_rng(seed)
    low = (285.0 + 20.0 * rng.random((n, channels) + i)).astype(np.float32)
    target = (285.0 + 20.0 * rng.random((n, 1) + o)).astype(np.float32)
    return low, target


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _check(low, target, mode, enable=True, dst_rows=None, bound=False):
    """scan, pack and restore of (low, target) against the restatement over b = upsample(low); returns (k, y, p, b)"""
    o = tuple(target.shape[2:])
    op = device_operand(low)
    dev = op.tensor.device
    b = upsample(op, o, mode=mode)
    t = torch.from_numpy(target).to(dev)
    got = residual_scan(op, t, mode=mode)
    want = residual_ref.scan(target, b)
    assert got == want, (got, want)
    (k, rmin, rmax) = got
    rows = None if dst_rows is None else torch.from_numpy(np.asarray(dst_rows, dtype=np.int32)).to(dev)
    y = torch.full_like(t, -7.0)
    residual_pack(op, t, y, rmin, rmax, mode=mode, enable=enable, dst_rows=rows)
    y_want = residual_ref.pack(target, b, rmin, rmax, enable=enable, dst_rows=dst_rows)
    y_got = y.cpu().numpy()[:, 0]
    assert np.array_equal(_bits(y_got), _bits(y_want))
    # restore what the pack wrote, case by case again: the scores of row i belong to case i
    scores = residual_ref.pack(target, b, rmin, rmax, enable=enable)
    p = residual_restore(op, torch.from_numpy(scores[:, None]).to(dev), rmin, rmax, mode=mode, enable=enable)
    assert p.dtype == torch.float64 and tuple(p.shape) == tuple(target.shape)
    p_got = p.cpu().numpy()[:, 0]
    assert np.array_equal(_bits(p_got), _bits(residual_ref.restore(scores, b, rmin, rmax, enable=enable)))
    if bound:
        err = np.abs(p_got - target[:, 0].astype(np.float64))
        limit = residual_ref.round_trip_bound(target, b, rmin, rmax)
        print(f"residual round trip {mode} {o}: max |restore(pack(t)) - t| / bound = {float(np.max(err / limit)):.3e}")
        assert (err <= limit).all()
    return k, y_got, p_got, b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shapes", SHAPES)
def test_shapes_and_modes(shapes, mode):
    (i, o) = shapes
    (low, target) = _fields(i, o, seed=i[0] * 100 + o[1])
    (k, y, _, _) = _check(low, target, mode, bound=True)
    assert k == 0 and float(y.min()) == 0.0 and float(y.max()) == 1.0


@pytest.mark.parametrize("mode", MODES)
def test_element_kinds_and_case_stride(mode):
    """low as fp64, and as a big-endian fp32 slab of two channels: channel 0 is read, the case stride is twice the plane"""
    (i, o) = SHAPES[0]
    (low, target) = _fields(i, o, seed=7, channels=2)
    _check(low.astype(np.float64)[:, :1], target, mode)
    slab = np.ascontiguousarray(low.astype(">f4"))
    op = device_operand(slab)
    assert op.kind == _lib.ELEM_F32_BE and op.stride == 2 * i[0] * i[1]
    (_, y_be, p_be, _) = _check(slab, target, mode)
    (_, y, p, _) = _check(np.ascontiguousarray(low[:, :1]), target, mode)
    assert np.array_equal(_bits(y_be), _bits(y)) and np.array_equal(_bits(p_be), _bits(p))


@pytest.mark.parametrize("mode", MODES)
def test_destination_rows_and_normalisation_off(mode):
    (i, o) = SHAPES[0]
    (low, target) = _fields(i, o, seed=11)
    _check(low, target, mode, dst_rows=[2, 0, 1])
    (_, y, _, b) = _check(low, target, mode, enable=False)
    assert np.array_equal(y, (target[:, 0].astype(np.float64) - b).astype(np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_values_that_are_not_finite(mode):
    """a NaN and an inf in low and a NaN in the target: each is counted, and is NaN in y and p at exactly its footprint"""
    (i, o) = SHAPES[0]
    (low, target) = _fields(i, o, seed=13)
    low[0, 0, 2, 1] = np.nan
    low[1, 0, 4, 2] = np.inf
    target[2, 0, 69, 129] = np.nan
    (k, y, p, b) = _check(low, target, mode)
    marked = np.isnan(b)                     # what case_ops.upsample marks
    assert marked[0].any() and marked[1].any() and not marked[2].any()
    lost = marked.copy()
    lost[2, 69, 129] = True
    assert k == int(lost.sum())
    assert np.array_equal(np.isnan(y), lost) and np.array_equal(np.isnan(p), lost)


def test_constant_residual_has_span_zero():
    (i, o) = SHAPES[0]
    (low, _) = _fields(i, o, seed=17)
    target = upsample(low, o, mode="nearest").astype(np.float32)[:, None]      # fp32 values: exact
    (k, y, p, _) = _check(low, target, "nearest")
    t = torch.from_numpy(target).cuda()
    assert residual_scan(low, t, mode="nearest") == (0, 0.0, 0.0)
    assert k == 0 and not _bits(y).any()                                        # +0.0 everywhere
    assert np.array_equal(p, target[:, 0].astype(np.float64))


def test_two_calls_give_the_same_bits():
    (i, o) = SHAPES[0]
    (low, target) = _fields(i, o, seed=19)
    runs = [_check(low, target, "bicubic") for _ in range(2)]
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])) and np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))


def test_an_empty_call_is_a_no_op():
    low = torch.zeros((0, 1, 4, 4), dtype=torch.float32, device="cuda")
    t = torch.zeros((0, 1, 8, 8), dtype=torch.float32, device="cuda")
    assert residual_scan(low, t) == (0, float("inf"), float("-inf"))
    residual_pack(low, t, torch.empty_like(t), 0.0, 1.0)
    assert tuple(residual_restore(low, t, 0.0, 1.0).shape) == (0, 1, 8, 8)
    torch.cuda.synchronize()


def test_refusals():
    lib = _lib.load()
    (low, target) = _fields((4, 4), (8, 8), seed=23)
    lo = torch.from_numpy(low).cuda()
    t = torch.from_numpy(target).cuda()
    y = torch.full_like(t, -7.0)

    def pack(ptr=None, kind=_lib.ELEM_F32, stride=16, mode=2, n=N):
        return lib.cae_residual_pack_rows(lo.data_ptr() if ptr is None else ptr, kind, stride, 4, 4, t.data_ptr(), n, 8, 8, mode,
                                          0.0, 1.0, 1, None, y.data_ptr(), None)

    assert pack(stride=15) == ERR_ARG and b"shorter than the plane" in lib.cae_last_error()
    assert pack(stride=1 << 60) == ERR_ARG and b"2^60" in lib.cae_last_error()
    assert pack(ptr=lo.data_ptr() + 4, kind=_lib.ELEM_F64) == ERR_ARG and b"aligned" in lib.cae_last_error()
    assert pack(mode=3) == ERR_ARG and pack(kind=9) == ERR_ARG and pack(n=-1) == ERR_ARG
    torch.cuda.synchronize()
    assert float(y.min()) == -7.0 and float(y.max()) == -7.0                    # nothing written
    with pytest.raises(ValueError, match="one channel"):
        residual_scan(lo, torch.zeros((N, 2, 8, 8), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="mode must be one of"):
        residual_scan(lo, t, mode="lanczos")
