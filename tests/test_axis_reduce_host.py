"""Axis reductions, host side: the C ABI's argument checks and the planner (smhip_reduce_plan) -- no device involved."""
import numpy as np
import pytest

import simplemath_amd as sma


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return list(reversed(st))


def plan(lib, shape, axis, strides=None, kind="sum", dtype=np.float32):
    route, launches, ori = lib.reduce_plan(kind, dtype, list(shape), dense(shape) if strides is None else list(strides), axis)
    return route & 0xff, route & ~0xff, launches, ori


def test_reduce_entry_points_are_declared():
    names = sma.declared_symbols()
    assert "smhip_reduce_axes" in names and "smhip_reduce_plan" in names


def test_argument_validation_needs_no_gpu(lib):
    f32, i32 = sma.F32, sma.I32
    bad = [
        (7, f32, [4], [1], 1),              # kind
        (sma.REDUCE_SUM, 9, [4], [1], 1),   # dtype
        (sma.REDUCE_SUM, f32, [2] * 7, [1] * 7, 1),  # ndim > MAX_NDIM
        (sma.REDUCE_SUM, f32, [4], [1], 0),  # empty mask
        (sma.REDUCE_SUM, f32, [4, 4], [4, 1], 0b100),  # axis beyond ndim
        (sma.REDUCE_SUM, f32, [4, -1], [4, 1], 1),     # negative extent
        (sma.REDUCE_MAX, f32, [0, 3], [3, 1], 1),      # max over an empty extent
        (sma.REDUCE_MEAN, f32, [3, 0], [1, 1], 2),     # mean over an empty extent
    ]
    for kind, dtype, shape, strides, mask in bad:
        assert lib.reduce_raw(kind, dtype, 16, shape, strides, mask, 16) == sma.ERR_INVALID, (kind, dtype, shape, mask)
    assert lib.reduce_raw(sma.REDUCE_SUM, f32, 16, None, None, 1, 16) == sma.ERR_INVALID  # null shape / strides (ndim 0)
    assert lib.reduce_raw(sma.REDUCE_SUM, f32, 0, [4], [1], 1, 16) == sma.ERR_INVALID     # null operand
    assert lib.reduce_raw(sma.REDUCE_SUM, f32, 16, [4], [1], 1, 0) == sma.ERR_INVALID     # null result
    # the mean of an integer type is not offered
    assert lib.reduce_raw(sma.REDUCE_MEAN, i32, 16, [4], [1], 1, 16) == sma.ERR_UNSUPPORTED
    assert lib.reduce_raw(sma.REDUCE_MEAN, sma.I64, 16, [4], [1], 1, 16) == sma.ERR_UNSUPPORTED
    with pytest.raises(sma.SmhipError) as e:
        lib.reduce_plan("mean", np.int32, [4], [1], 0)
    assert e.value.code == sma.ERR_UNSUPPORTED


def test_python_axis_argument_checks(lib):
    assert sma.Smhip._axes(3, -1) == (2,)
    assert sma.Smhip._axes(3, (2, -3)) == (0, 2)
    assert sma.Smhip._axes(2, None) == (0, 1)
    for bad in (3, -4, (0, 0), (1, -2)):
        with pytest.raises(ValueError):
            sma.Smhip._axes(3, bad)


def test_plan_dense_rows_and_columns(lib):
    assert plan(lib, (8192, 3000), 1) == (sma.ROUTE_ROW, 0, 1, (8192, 3000, 1))
    # few outputs: the column walk splits R into chunks and folds the partials in a second launch
    route, flags, launches, ori = plan(lib, (1000, 3000), 0)
    assert (route, ori) == (sma.ROUTE_COLUMN, (1, 1000, 3000))
    assert flags == sma.ROUTE_SPLIT and launches == 2
    # enough outputs: one launch
    assert plan(lib, (64, 1 << 20), 0) == (sma.ROUTE_COLUMN, 0, 1, (1, 64, 1 << 20))


def test_plan_transposed_view_is_not_copied(lib):
    # A.T over axis 0 is A over axis 1: the same route, the same (O, R, I), no copy
    A = (16384, 8192)
    want = plan(lib, A, 1)
    got = plan(lib, (A[1], A[0]), 0, strides=(1, A[1]))
    assert got == want and not got[1] & sma.ROUTE_COPY
    # and A.T over axis 1 is A over axis 0
    assert plan(lib, (A[1], A[0]), 1, strides=(1, A[1])) == plan(lib, A, 0)


def test_plan_per_channel_nhwc(lib):
    route, flags, launches, ori = plan(lib, (64, 224, 224, 3), (0, 1, 2))
    assert route == sma.ROUTE_CHANNEL and ori == (1, 64 * 224 * 224, 3)
    assert not flags & (sma.ROUTE_COPY | sma.ROUTE_PASSES)
    # short rows over the last axis: the row route
    assert plan(lib, (64, 224, 224, 3), 3)[0::3] == (sma.ROUTE_ROW, (64 * 224 * 224, 3, 1))


def test_plan_short_channel_blocks_take_the_packed_column_walk(lib):
    # per-channel over a short R (NHWC over W alone, (B, 4, 3) over axis 1): the column walk, whose lanes pack (o, quad)
    assert plan(lib, (8, 224, 224, 3), 2)[0::3] == (sma.ROUTE_COLUMN, (8 * 224, 224, 3))
    assert plan(lib, (1000, 4, 3), 1)[0::3] == (sma.ROUTE_COLUMN, (1000, 4, 3))
    # very many outer indices: one launch, whatever O is (the kernels loop over their tasks under a capped grid)
    assert plan(lib, ((1 << 24) + 1, 2, 2), 1) == (sma.ROUTE_COLUMN, 0, 1, ((1 << 24) + 1, 2, 2))
    assert plan(lib, ((1 << 24) + 1, 2, 12), 1) == (sma.ROUTE_COLUMN, 0, 1, ((1 << 24) + 1, 2, 12))
    # enough stream per outer index: the channel walk
    assert plan(lib, (4, 4096, 3), 1)[0] == sma.ROUTE_CHANNEL


def test_reduce_out_argument_is_checked(lib):
    class Fake:  # stands in for a DeviceArray: the check fires before anything is allocated or launched
        def __init__(self, dtype, shape, is_dense=True):
            self.dtype, self.shape, self.ndim, self.strides = np.dtype(dtype), shape, len(shape), tuple(dense(shape))
            self.size = int(np.prod(shape))
            self.is_dense = lambda: is_dense

    a = Fake(np.float32, (4, 5))
    for out in (Fake(np.float64, (4,)), Fake(np.float32, (5,)), Fake(np.float32, (4,), is_dense=False)):
        with pytest.raises(ValueError):
            lib.reduce("sum", a, 1, out=out)


def test_plan_split_when_too_few_outputs(lib):
    route, flags, launches, ori = plan(lib, (4, 1 << 26), 1)
    assert (route, flags, launches, ori) == (sma.ROUTE_ROW, sma.ROUTE_SPLIT, 2, (4, 1 << 26, 1))
    route, flags, launches, ori = plan(lib, (1 << 26, 4), 0)
    assert (route, flags, launches, ori) == (sma.ROUTE_CHANNEL, sma.ROUTE_SPLIT, 2, (1, 1 << 26, 4))
    # every axis through the mask: one long row, split
    assert plan(lib, (512, 1024, 64), (0, 1, 2)) == (sma.ROUTE_ROW, sma.ROUTE_SPLIT, 2, (1, 512 * 1024 * 64, 1))


def test_plan_two_reduced_groups_take_two_passes(lib):
    route, flags, launches, ori = plan(lib, (50, 60, 70), (0, 2))
    assert flags & sma.ROUTE_PASSES and not flags & sma.ROUTE_COPY
    assert route == sma.ROUTE_ROW and ori == (50 * 60, 70, 1)  # the inner group first
    assert launches >= 2


def test_plan_stepped_view_is_copied_first(lib):
    # A[:, ::2] over axis 1: no unit stride in the walk
    route, flags, launches, ori = plan(lib, (100, 50), 1, strides=(100, 2))
    assert flags & sma.ROUTE_COPY and route == sma.ROUTE_ROW and ori == (100, 50, 1) and launches == 2
    # a broadcast (stride 0) axis is materialised as well
    assert plan(lib, (8, 5), 1, strides=(0, 1))[1] & sma.ROUTE_COPY


def test_plan_degenerate_shapes(lib):
    assert plan(lib, (3, 0, 4), 1) == (sma.ROUTE_FILL, 0, 1, (12, 0, 1))   # sum over an empty extent: zeros
    assert plan(lib, (3, 0, 4), 0)[2] == 0                                # empty result: nothing to do
    assert plan(lib, (3, 1, 4), 1)[0] == sma.ROUTE_GATHER                  # reducing extents of 1
    # size-1 axes do not change the walk
    assert plan(lib, (7, 1, 9), 2) == plan(lib, (7, 9), 1)


def test_plan_depends_on_shape_and_layout_only(lib):
    a = lib.reduce_plan("sum", np.float32, [4, 1 << 20], [1 << 20, 1], 1)
    for kind in ("mean", "max", "min"):
        assert lib.reduce_plan(kind, np.float32, [4, 1 << 20], [1 << 20, 1], 1) == a
