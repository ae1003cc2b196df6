"""var, std, var_mean and standardize without a device: the per-line arithmetic on the host (tests/cpp/moments_host_check.cpp compiles
csrc/sm_moments.h with g++ and checks it against long double, once more with the sanitizers on), the planner (smhip_moments_plan and
smhip_standardize_plan through the binding), what the entry points refuse, and the binding's errors.

L (the longest line held in registers) is read from the plan, never written here.  The refusals are pinned as literals in this file:
the return code and the FULL message.  They are replayed only without a device (the pointers are made-up integers)."""
import ctypes as ct
import re
import subprocess

import numpy as np
import pytest

import simplemath_amd as sma

KINDS = (sma.MOMENT_VAR, sma.MOMENT_STD)
DTYPES = (np.float32, np.float64)
IDS = dict(ids=lambda d: np.dtype(d).name)
A, B, M = 1 << 20, 2 << 20, 3 << 20  # stand-ins for device pointers: never dereferenced
ROW, COLUMN, CHANNEL, UNIT, NONE, SPLIT, COPY = (sma.MOMENTS_ROUTE_ROW, sma.MOMENTS_ROUTE_COLUMN, sma.MOMENTS_ROUTE_CHANNEL, sma.MOMENTS_ROUTE_UNIT,
                                                 sma.MOMENTS_ROUTE_NONE, sma.MOMENTS_SPLIT, sma.MOMENTS_COPY)
LADDER = lambda L: (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17)


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


@pytest.mark.parametrize("program", ["moments_host_check", "moments_host_check_san"])
def test_the_line_arithmetic_on_the_host(program):
    """Every VAR, STD and standardized element inside the bounds of include/smhip.h, lines whole and cut into chunks, and the exact
    cases (the program's header lists them); the worst errors it prints are fractions of their bounds.  _san: the same program built
    with -fsanitize=address,undefined."""
    from simplemath_amd import build
    exe = build.build_host_programs()[program]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "moments_host_check: 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for name in ("f32", "f64"):
        m = re.search(rf"^{name} var worst ([0-9.]+) std worst ([0-9.]+) standardize worst ([0-9.]+) of the bound over (\d+) lines", r.stdout, re.M)
        assert m and int(m.group(4)) >= 900 and all(0 < float(m.group(k)) <= 1 for k in (1, 2, 3)), r.stdout


def limit(lib, dtype):
    return lib.moments_plan(sma.MOMENT_VAR, dtype, [1 << 20], [1], 0)[3][0]


def both(lib, dtype, shape, strides, axis):
    """The plans of VAR and STD (the same) and of standardize for one view."""
    var = lib.moments_plan(sma.MOMENT_VAR, dtype, shape, strides, axis)
    assert lib.moments_plan(sma.MOMENT_STD, dtype, shape, strides, axis) == var
    if shape[axis] >= 2:
        assert lib.moments_plan(sma.MOMENT_VAR, dtype, shape, strides, axis, ddof=1) == var  # ddof changes no route
    return var, lib.standardize_plan(dtype, shape, strides, axis)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_along_the_last_axis(lib, dtype):
    L = limit(lib, dtype)
    assert L >= 512
    for R in LADDER(L):
        var, std = both(lib, dtype, [3, R], [R, 1], 1)
        for plan, extra in ((var, 0), (std, 1)):
            route, launches, ori, info = plan
            assert ori == (3, R, 1) and info[0] == L, R
            assert (info[1] == 1) == (R <= L), R  # one read exactly when the line is held
            if R == 1:
                assert (route, launches, info) == (UNIT, 2, (L, 1, 1)), R
            elif R <= L:
                assert (route, launches, info) == (ROW, 1, (L, 1, 1)), R
            else:  # the fp64 sums, the centred sums, the finish (and standardize's store)
                assert route == ROW | SPLIT and info == (L, 2 + extra, 2) and launches >= 3 + extra, R
    R = 40 * L + 3  # one long line: cut into chunks by both walks
    for shape, strides, axis in (([1, R], [R, 1], 1), ([R], [1], 0)):
        var, std = both(lib, dtype, shape, strides, axis)
        assert var == (ROW | SPLIT, 4, (1, R, 1), (L, 2, 2)) and std == (ROW | SPLIT, 5, (1, R, 1), (L, 3, 2))
    # rows enough: the second walk takes each row whole
    assert lib.moments_plan(sma.MOMENT_VAR, dtype, [8192, 2 * L], [2 * L, 1], 1) == (ROW, 3, (8192, 2 * L, 1), (L, 2, 2))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_along_other_axes(lib, dtype):
    L = limit(lib, dtype)
    dense = lambda shape: [int(np.prod(shape[d + 1:])) for d in range(len(shape))]
    # few lanes: the columns are cut into chunks (the sums by reduce's walk, then the centred sums, then the finish)
    for shape, axis, ori in (((70, 50), 0, (1, 70, 50)), ((257, 5), 0, (1, 257, 5)), ((3, 70, 6), 1, (3, 70, 6))):
        var, std = both(lib, dtype, shape, dense(shape), axis)
        assert var == (COLUMN | SPLIT, 4, ori, (L, 2, 2)) and std == (COLUMN | SPLIT, 5, ori, (L, 3, 2)), shape
    # short columns, or lanes enough: whole
    for shape, axis, ori in (((13, 37), 0, (1, 13, 37)), ((2, 9, 5), 1, (2, 9, 5)), ((64, 1 << 20), 0, (1, 64, 1 << 20)), ((2, 3, 5, 7), 2, (6, 5, 7))):
        var, std = both(lib, dtype, shape, dense(shape), axis)
        assert var == (COLUMN, 3, ori, (L, 2, 2)) and std == (COLUMN, 4, ori, (L, 3, 2)), shape
    # few columns side by side over a long extent: reduce sums them as CHANNEL; standardize walks columns
    var, std = both(lib, dtype, (4099, 3), [3, 1], 0)
    assert var == (CHANNEL | SPLIT, 4, (1, 4099, 3), (L, 2, 2)) and std[0] == COLUMN | SPLIT and std[2:] == ((1, 4099, 3), (L, 3, 2))
    # per-channel statistics of an NHWC array: axes 0-2 merge
    route, launches, ori, info = lib.moments_plan(sma.MOMENT_VAR, dtype, (5, 6, 7, 3), dense((5, 6, 7, 3)), (0, 1, 2))
    assert route & 0xff in (COLUMN, CHANNEL) and not route & COPY and ori == (1, 210, 3) and info == (L, 2, 2)
    # kept axes on one side of the axis merge
    assert both(lib, dtype, [2, 3, 5], [15, 5, 1], 2) == ((ROW, 1, (6, 5, 1), (L, 1, 1)),) * 2
    # axes {0, 2} of a rank-3 array do not merge: copied with the reduced axes innermost, six rows of 35
    route, launches, ori, info = lib.moments_plan(sma.MOMENT_VAR, dtype, (5, 6, 7), [42, 7, 1], (0, 2))
    assert (route, ori, info) == (ROW | COPY, (6, 35, 1), (L, 2, 2)) and launches >= 5
    # every axis: one line
    assert lib.moments_plan(sma.MOMENT_VAR, dtype, (5, 6, 7), [42, 7, 1], None) == (ROW, 1, (1, 210, 1), (L, 1, 1))


def test_views(lib):
    dtype = np.float32
    L = limit(lib, dtype)
    var = lambda shape, strides, axis: lib.moments_plan(sma.MOMENT_VAR, dtype, shape, strides, axis)
    std = lambda shape, strides, axis: lib.standardize_plan(dtype, shape, strides, axis)
    # var(A.T, 1) of a dense (70, 50) A walks as var(A, 0): the columns of A read in place, no copy
    assert var([50, 70], [1, 50], 1) == var([70, 50], [50, 1], 0) == (COLUMN | SPLIT, 4, (1, 70, 50), (L, 2, 2))
    assert std([50, 70], [1, 50], 1) == (COLUMN | SPLIT, 5, (1, 70, 50), (L, 3, 2))
    # var(A.T, 0) walks as var(A, 1): rows in memory; standardize's result lines would be strided -- copied
    assert var([50, 70], [1, 50], 0) == var([70, 50], [50, 1], 1) == (ROW, 1, (70, 50, 1), (L, 1, 1))
    assert std([50, 70], [1, 50], 0)[0] == COLUMN | SPLIT | COPY
    # a stepped axis: copied; stepped ROWS are read in place
    assert var([70, 65], [130, 2], 1) == std([70, 65], [130, 2], 1) == (ROW | COPY, 2, (70, 65, 1), (L, 1, 1))
    assert var([35, 65], [130, 1], 1) == std([35, 65], [130, 1], 1) == (ROW, 1, (35, 65, 1), (L, 1, 1))
    route, launches, ori, info = var([35, 2 * L + 1], [4 * L, 1], 1)
    assert (route & ~SPLIT, ori, info) == (ROW, (35, 2 * L + 1, 1), (L, 2, 2))
    # a stride-0 axis, along the axis or across it: copied
    for strides in ([1, 0], [0, 1]):
        assert var([9, 33], strides, 1) == std([9, 33], strides, 1) == (ROW | COPY, 2, (9, 33, 1), (L, 1, 1))
    # columns of a block at an odd offset inside a wider array (the offset is in the pointer)
    assert var([13, 37], [64, 1], 0) == (COLUMN, 3, (1, 13, 37), (L, 2, 2))
    # N == 1: the kept elements, then x - x
    assert var([7, 1], [3, 1], 1) == std([7, 1], [3, 1], 1) == (UNIT, 2, (7, 1, 1), (L, 1, 1))


def test_empty_extents(lib):
    for dtype in DTYPES:
        # nothing kept: nothing to write, whatever is reduced
        assert lib.moments_plan(sma.MOMENT_VAR, dtype, [0, 7], [7, 1], 1)[:2] == (NONE, 0)
        assert lib.moments_plan(sma.MOMENT_VAR, dtype, [0, 0], [0, 1], 1)[:2] == (NONE, 0)
        for shape, strides in (([0, 7], [7, 1]), ([3, 0], [0, 1]), ([0, 0], [0, 1])):
            assert lib.standardize_plan(dtype, shape, strides, 1)[:2] == (NONE, 0)
        # something kept, nothing reduced: refused, like MEAN
        for shape, strides, axis in (([7, 0], [0, 1], 1), ([0, 7], [7, 1], 0), ([0], [1], 0)):
            with pytest.raises(sma.SmhipError, match="a variance over an empty extent"):
                lib.moments_plan(sma.MOMENT_VAR, dtype, shape, strides, axis)


INVALID, UNSUPPORTED = sma.ERR_INVALID, sma.ERR_UNSUPPORTED
BASE = dict(kind=sma.MOMENT_VAR, dtype=sma.F32, a_ptr=A, shape=[3, 7], strides=[7, 1], mask=2, ddof=0, out_ptr=B, mean_ptr=M)
SBASE = dict(dtype=sma.F32, a_ptr=A, shape=[3, 7], strides=[7, 1], axis=1, eps=0.0, ddof=0, out_ptr=B)
SHARED = [  # (what changes, the return code, the full message after "<entry point>: "): both pairs
    (dict(dtype=99), INVALID, "bad dtype 99"),
    (dict(ndim=0), INVALID, "ndim 0 outside 1..6"),
    (dict(ndim=7), INVALID, "ndim 7 outside 1..6"),
    (dict(dtype=sma.I32), UNSUPPORTED, "an integer element type (f32 and f64 only)"),
    (dict(dtype=sma.I64), UNSUPPORTED, "an integer element type (f32 and f64 only)"),
    (dict(shape=[3, -7]), INVALID, "negative extent or stride at dim 1"),
    (dict(strides=[-7, 1]), INVALID, "negative extent or stride at dim 0"),
    (dict(shape=None, ndim=2), INVALID, "null shape/strides"),
    (dict(strides=None, ndim=2), INVALID, "null shape/strides"),
    (dict(ddof=-1), INVALID, "ddof -1 is negative"),
    (dict(ddof=7), INVALID, "N - ddof = 7 - 7 is not positive"),
    (dict(ddof=9), INVALID, "N - ddof = 7 - 9 is not positive"),
]
MOMENTS = [
    (dict(kind=2), INVALID, "bad kind 2"),
    (dict(kind=-1), INVALID, "bad kind -1"),
    (dict(mask=0), INVALID, "axes mask 0x0 empty or beyond ndim 2"),
    (dict(mask=4), INVALID, "axes mask 0x4 empty or beyond ndim 2"),
    (dict(shape=[3, 0], strides=[0, 1]), INVALID, "a variance over an empty extent"),
]
STANDARDIZE = [
    (dict(axis=2), INVALID, "axis 2 outside 0..1"),
    (dict(axis=-1), INVALID, "axis -1 outside 0..1"),
    (dict(eps=-1e-9), INVALID, "eps -1e-09 is negative, NaN or infinite"),
    (dict(eps=float("nan")), INVALID, "eps nan is negative, NaN or infinite"),
    (dict(eps=float("inf")), INVALID, "eps inf is negative, NaN or infinite"),
]
MOMENTS_POINTERS = [  # smhip_moments_axes alone
    (dict(a_ptr=0), INVALID, "null buffer"),
    (dict(out_ptr=0), INVALID, "null buffer"),
    (dict(out_ptr=A + 8), INVALID, "the operand and the outputs overlap"),
    (dict(out_ptr=A), INVALID, "the operand and the outputs overlap"),
    (dict(mean_ptr=A + 80), INVALID, "the operand and the outputs overlap"),
    (dict(mean_ptr=B + 8), INVALID, "the operand and the outputs overlap"),
]
S_OVERLAP = "`out` overlaps the operand (only out == a with a dense operand is in place)"
STANDARDIZE_POINTERS = [
    (dict(a_ptr=0), INVALID, "null buffer"),
    (dict(out_ptr=0), INVALID, "null buffer"),
    (dict(out_ptr=A + 8), INVALID, S_OVERLAP),
    (dict(out_ptr=A - 8), INVALID, S_OVERLAP),
    (dict(out_ptr=A, strides=[8, 1]), INVALID, S_OVERLAP),  # in place needs a dense operand
]


def arr(v):
    return (ct.c_int64 * len(v))(*v) if v is not None else None


def moments_plan_raw(lib, kw):
    ndim = kw.get("ndim", len(kw["shape"]) if kw["shape"] is not None else 2)
    return lib.c.smhip_moments_plan(ct.c_int(kw["kind"]), ct.c_int(kw["dtype"]), arr(kw["shape"]), arr(kw["strides"]), ct.c_int(ndim), ct.c_uint32(kw["mask"]),
                                    ct.c_int64(kw["ddof"]), None, None, None, None)


def standardize_plan_raw(lib, kw):
    ndim = kw.get("ndim", len(kw["shape"]) if kw["shape"] is not None else 2)
    return lib.c.smhip_standardize_plan(ct.c_int(kw["dtype"]), arr(kw["shape"]), arr(kw["strides"]), ct.c_int(ndim), ct.c_int(kw["axis"]), ct.c_double(kw["eps"]),
                                        ct.c_int64(kw["ddof"]), None, None, None, None)


def test_refusals(lib):
    if lib.device_count():
        pytest.skip("a device is present: a call that got past its checks would launch on made-up pointers")
    last = lambda: lib.c.smhip_last_error().decode()
    for change, rc, msg in SHARED + MOMENTS + MOMENTS_POINTERS:
        assert lib.moments_raw(**dict(BASE, **change)) == rc, change
        assert last() == "moments_axes: " + msg, change
    for change, rc, msg in SHARED + MOMENTS:
        assert moments_plan_raw(lib, dict(BASE, **change)) == rc, change
        assert last() == "moments_plan: " + msg, change
    for change, rc, msg in SHARED + STANDARDIZE + STANDARDIZE_POINTERS:
        assert lib.standardize_raw(**dict(SBASE, **change)) == rc, change
        assert last() == "standardize_axis: " + msg, change
    for change, rc, msg in SHARED + STANDARDIZE:
        assert standardize_plan_raw(lib, dict(SBASE, **change)) == rc, change
        assert last() == "standardize_plan: " + msg, change
    # nothing to write is no refusal, whatever the pointers and ddof
    assert lib.moments_raw(**dict(BASE, shape=[0, 7], a_ptr=0, out_ptr=0, mean_ptr=0, ddof=9)) == 0
    assert lib.standardize_raw(**dict(SBASE, shape=[0, 7], a_ptr=0, out_ptr=0, ddof=9)) == 0
    assert lib.standardize_raw(**dict(SBASE, shape=[3, 0], strides=[0, 1], a_ptr=0, out_ptr=0)) == 0


class FakeArray(sma.DeviceArray):
    """A DeviceArray over no memory: the binding refuses before it asks for a pointer."""

    def __init__(self, dtype, shape, strides=None):
        dense, acc = [], 1
        for d in shape[::-1]:
            dense.append(acc)
            acc *= d
        super().__init__(None, A, dtype, shape, strides if strides is not None else dense[::-1], owner=object())


def test_the_bindings_errors(lib):
    a = FakeArray(np.float32, (3, 7))
    for fn in (lib.var, lib.std, lib.var_mean, lib.standardize):
        for dt in (np.int32, np.int64, np.int16):
            with pytest.raises(TypeError, match="float32 and float64 only"):
                fn(FakeArray(dt, (3, 7)))
        for axis in (2, -3):
            with pytest.raises(ValueError):
                fn(a, axis=axis)
        with pytest.raises(ValueError, match="ddof -1 is negative"):
            fn(a, axis=1, ddof=-1)
        with pytest.raises(ValueError, match="N - ddof = 7 - 7 is not positive"):
            fn(a, axis=1, ddof=7)
    for fn in (lib.var, lib.std, lib.var_mean):
        with pytest.raises(ValueError, match="repeated axis"):
            fn(a, axis=(1, -1))
        for out in (FakeArray(np.float64, (3,)), FakeArray(np.float32, (7,)), FakeArray(np.float32, (3,), (2,))):
            with pytest.raises(ValueError, match="out must be a dense float32 array of 3 elements"):
                fn(a, axis=1, out=out)
        with pytest.raises(ValueError, match="N - ddof = 21 - 21 is not positive"):
            fn(a, ddof=21)
    for eps in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="negative, NaN or infinite"):
            lib.standardize(a, eps=eps)
    for out in (FakeArray(np.float64, (3, 7)), FakeArray(np.float32, (7, 3)), FakeArray(np.float32, (3, 7), (8, 1))):  # dtype, shape, density
        with pytest.raises(ValueError, match="out must be a dense float32 array of shape \\(3, 7\\)"):
            lib.standardize(a, out=out)
    view = FakeArray(np.float32, (3, 7), (8, 1))
    with pytest.raises(ValueError, match="in place"):
        lib.standardize(view, out=view)


def test_the_header_declares_both_pairs():
    assert {"smhip_moments_axes", "smhip_moments_plan", "smhip_standardize_axis", "smhip_standardize_plan"} <= set(sma.declared_symbols())
