"""softmax, log_softmax and logsumexp without a device: the per-line arithmetic on the host (tests/cpp/softmax_host_check.cpp compiles
csrc/sm_softmax.h with g++ and checks it against long double), the planner (smhip_softmax_plan through the binding), what both entry
points refuse, and the binding's errors.

L (the longest line held on chip) is read from the plan, never written here.  The refusals are pinned as literals in this file: the
return code and the FULL message.  They are replayed only without a device (the pointers are made-up integers)."""
import re
import subprocess

import numpy as np
import pytest

import simplemath_amd as sma

KINDS = (sma.SOFTMAX, sma.LOG_SOFTMAX, sma.LOGSUMEXP)
DTYPES = (np.float32, np.float64)
IDS = dict(ids=lambda d: np.dtype(d).name)
A, B = 1 << 20, 2 << 20  # stand-ins for device pointers: never dereferenced
ROW, COLUMN, FILL, NONE, SPLIT, COPY = (sma.SOFTMAX_ROUTE_ROW, sma.SOFTMAX_ROUTE_COLUMN, sma.SOFTMAX_ROUTE_FILL, sma.SOFTMAX_ROUTE_NONE,
                                        sma.SOFTMAX_SPLIT, sma.SOFTMAX_COPY)


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def test_the_line_arithmetic_on_the_host():
    """Every element of every line inside the bounds of include/smhip.h, held and cut into chunks, and the exact cases (the program's
    header lists them); the worst errors it prints are fractions of their bounds."""
    from simplemath_amd import build
    exe = build.build_host_programs()["softmax_host_check"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "softmax_host_check: 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for name in ("f32", "f64"):
        m = re.search(rf"^{name} softmax worst ([0-9.]+) log_softmax worst ([0-9.]+) logsumexp worst ([0-9.]+) of the bound over (\d+) lines", r.stdout, re.M)
        assert m and int(m.group(4)) >= 900 and all(0 < float(m.group(k)) <= 1 for k in (1, 2, 3)), r.stdout


def limit(lib, dtype):
    return lib.softmax_plan(sma.SOFTMAX, dtype, [1 << 20], [1], 0)[3][0]


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_along_the_last_axis(lib, dtype):
    L = limit(lib, dtype)
    assert L >= 4096
    for R in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17):
        for kind in KINDS:
            route, launches, ori, info = lib.softmax_plan(kind, dtype, [3, R], [R, 1], 1)
            held = R <= L
            assert ori == (3, R, 1) and info[0] == L, (kind, R)
            assert (info[1] == 1) == held, (kind, R)  # one read exactly when the line is held
            if held:
                assert (route, launches, info) == (ROW, 1, (L, 1, 1)), (kind, R)
            else:
                assert (route, launches, info) == (ROW | SPLIT, 2 if kind == sma.LOGSUMEXP else 3, (L, 2, 2)), (kind, R)
    for kind in KINDS:  # one long line: cut into chunks
        R = 40 * L + 3
        assert lib.softmax_plan(kind, dtype, [1, R], [R, 1], 1) == (ROW | SPLIT, 2 if kind == sma.LOGSUMEXP else 3, (1, R, 1), (L, 2, 2))
        assert lib.softmax_plan(kind, dtype, [R], [1], 0) == (ROW | SPLIT, 2 if kind == sma.LOGSUMEXP else 3, (1, R, 1), (L, 2, 2))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_along_other_axes(lib, dtype):
    L = limit(lib, dtype)
    dense = lambda shape: [int(np.prod(shape[d + 1:])) for d in range(len(shape))]
    for kind in KINDS:
        last = 0 if kind == sma.LOGSUMEXP else 1
        # few lanes: the columns are cut into chunks
        for shape, axis, ori in (((70, 50), 0, (1, 70, 50)), ((257, 5), 0, (1, 257, 5)), ((3, 70, 6), 1, (3, 70, 6)), ((4099, 3), 0, (1, 4099, 3))):
            assert lib.softmax_plan(kind, dtype, shape, dense(shape), axis) == (COLUMN | SPLIT, 2 + last, ori, (L, 3, 2)), (kind, shape)
        # short columns, or lanes enough: one launch
        for shape, axis, ori in (((13, 37), 0, (1, 13, 37)), ((2, 9, 5), 1, (2, 9, 5)), ((64, 1 << 20), 0, (1, 64, 1 << 20))):
            assert lib.softmax_plan(kind, dtype, shape, dense(shape), axis) == (COLUMN, 1, ori, (L, 3, 1)), (kind, shape)
        # kept axes on one side of the axis merge
        assert lib.softmax_plan(kind, dtype, [2, 3, 5, 7], [105, 35, 7, 1], 2) == (COLUMN, 1, (6, 5, 7), (L, 3, 1))
        assert lib.softmax_plan(kind, dtype, [2, 3, 5], [15, 5, 1], 2) == (ROW, 1, (6, 5, 1), (L, 1, 1))


def test_views(lib):
    dtype = np.float32
    L = limit(lib, dtype)
    for kind in KINDS:
        last = 0 if kind == sma.LOGSUMEXP else 1
        plan = lambda shape, strides, axis: lib.softmax_plan(kind, dtype, shape, strides, axis)
        # softmax(A.T, -1) of a dense (70, 50) A: the columns of A read in place, no copy
        assert plan([50, 70], [1, 50], 1) == (COLUMN | SPLIT, 2 + last, (1, 70, 50), (L, 3, 2))
        # softmax(A.T, 0): rows in memory, but the result's lines would be strided -- copied; LOGSUMEXP reads them in place
        if kind == sma.LOGSUMEXP:
            assert plan([50, 70], [1, 50], 0) == (ROW, 1, (70, 50, 1), (L, 1, 1))
        else:
            assert plan([50, 70], [1, 50], 0) == (COLUMN | SPLIT | COPY, 4, (1, 50, 70), (L, 3, 2))
        # a stepped axis: copied; stepped ROWS are read in place
        assert plan([70, 65], [130, 2], 1) == (ROW | COPY, 2, (70, 65, 1), (L, 1, 1))
        assert plan([35, 65], [130, 1], 1) == (ROW, 1, (35, 65, 1), (L, 1, 1))
        assert plan([35, 2 * L + 1], [4 * L, 1], 1) == (ROW | SPLIT, 2 + last, (35, 2 * L + 1, 1), (L, 2, 2))
        # a stride-0 axis, along the axis or across it: copied
        assert plan([9, 33], [1, 0], 1) == (ROW | COPY, 2, (9, 33, 1), (L, 1, 1))
        assert plan([9, 33], [0, 1], 1) == (ROW | COPY, 2, (9, 33, 1), (L, 1, 1))
        # columns of a block inside a wider array
        assert plan([13, 37], [64, 1], 0) == (COLUMN, 1, (1, 13, 37), (L, 3, 1))
        # R == 1: dense, every element a line; a view of it is copied
        assert plan([7, 1], [1, 1], 1) == (ROW, 1, (7, 1, 1), (L, 1, 1))
        assert plan([7, 1], [3, 1], 1) == (ROW | COPY, 2, (7, 1, 1), (L, 1, 1))


def test_empty_extents(lib):
    for dtype in DTYPES:
        L = limit(lib, dtype)
        for kind in KINDS:
            assert lib.softmax_plan(kind, dtype, [0, 7], [7, 1], 1) == (NONE, 0, (0, 7, 1), (L, 0, 0))
            want = (FILL, 1) if kind == sma.LOGSUMEXP else (NONE, 0)  # logsumexp over nothing is -inf
            assert lib.softmax_plan(kind, dtype, [3, 0], [0, 1], 1)[:2] == want
            assert lib.softmax_plan(kind, dtype, [0], [1], 0)[:2] == want  # ndim == 1: one result


INVALID, UNSUPPORTED = sma.ERR_INVALID, sma.ERR_UNSUPPORTED
BASE = dict(kind=sma.SOFTMAX, dtype=sma.F32, a_ptr=A, shape=[3, 7], strides=[7, 1], axis=1, out_ptr=B)
OVERLAP = "`out` overlaps the operand (only out == a with a dense operand, SOFTMAX or LOG_SOFTMAX, is in place)"
CHECKS = [  # (what changes, the return code, the full message after "<entry point>: ")
    (dict(kind=3), INVALID, "bad kind 3"),
    (dict(kind=-1), INVALID, "bad kind -1"),
    (dict(dtype=99), INVALID, "bad dtype 99"),
    (dict(ndim=0), INVALID, "ndim 0 outside 1..6"),
    (dict(ndim=7), INVALID, "ndim 7 outside 1..6"),
    (dict(dtype=sma.I32), UNSUPPORTED, "an integer element type (f32 and f64 only)"),
    (dict(dtype=sma.I64), UNSUPPORTED, "an integer element type (f32 and f64 only)"),
    (dict(axis=2), INVALID, "axis 2 outside 0..1"),
    (dict(axis=-1), INVALID, "axis -1 outside 0..1"),
    (dict(shape=[3, -7]), INVALID, "negative extent or stride at dim 1"),
    (dict(strides=[-7, 1]), INVALID, "negative extent or stride at dim 0"),
    (dict(shape=None, ndim=2), INVALID, "null shape/strides"),
    (dict(strides=None, ndim=2), INVALID, "null shape/strides"),
]
POINTERS = [  # smhip_softmax_axis alone
    (dict(a_ptr=0), INVALID, "null buffer"),
    (dict(out_ptr=0), INVALID, "null buffer"),
    (dict(kind=sma.LOGSUMEXP, shape=[3, 0], strides=[0, 1], a_ptr=0, out_ptr=0), INVALID, "null buffer"),  # three results, -inf each
    (dict(out_ptr=A + 8), INVALID, OVERLAP),
    (dict(out_ptr=A + 80), INVALID, OVERLAP),
    (dict(out_ptr=A, strides=[8, 1]), INVALID, OVERLAP),  # in place needs a dense operand
    (dict(out_ptr=A, kind=sma.LOGSUMEXP), INVALID, OVERLAP),
    (dict(out_ptr=A - 8, kind=sma.LOGSUMEXP), INVALID, OVERLAP),
]


def plan_raw(lib, kw):
    import ctypes as ct
    arr = lambda v: (ct.c_int64 * len(v))(*v) if v is not None else None
    ndim = kw.get("ndim", len(kw["shape"]) if kw["shape"] is not None else 2)
    return lib.c.smhip_softmax_plan(ct.c_int(kw["kind"]), ct.c_int(kw["dtype"]), arr(kw["shape"]), arr(kw["strides"]), ct.c_int(ndim), ct.c_int(kw["axis"]),
                                    None, None, None, None)


def test_refusals(lib):
    if lib.device_count():
        pytest.skip("a device is present: a call that got past its checks would launch on made-up pointers")
    for change, rc, msg in CHECKS + POINTERS:
        assert lib.softmax_raw(**dict(BASE, **change)) == rc, change
        assert lib.c.smhip_last_error().decode() == "softmax_axis: " + msg, change
    for change, rc, msg in CHECKS:
        assert plan_raw(lib, dict(BASE, **change)) == rc, change
        assert lib.c.smhip_last_error().decode() == "softmax_plan: " + msg, change
    # nothing to write is no refusal, whatever the pointers
    for kind in KINDS:
        assert lib.softmax_raw(**dict(BASE, kind=kind, shape=[0, 7], a_ptr=0, out_ptr=0)) == 0
    assert lib.softmax_raw(**dict(BASE, shape=[3, 0], strides=[0, 1], a_ptr=0, out_ptr=0)) == 0
    assert lib.softmax_raw(**dict(BASE, kind=sma.LOG_SOFTMAX, shape=[3, 0], strides=[0, 1], a_ptr=0, out_ptr=0)) == 0


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
    for fn in (lib.softmax, lib.log_softmax, lib.logsumexp):
        for dt in (np.int32, np.int64, np.int16):
            with pytest.raises(TypeError, match="float32 and float64 only"):
                fn(FakeArray(dt, (3, 7)))
        for axis in (2, -3):
            with pytest.raises(ValueError):
                fn(a, axis=axis)
    for fn in (lib.softmax, lib.log_softmax):
        for out in (FakeArray(np.float64, (3, 7)), FakeArray(np.float32, (7, 3)), FakeArray(np.float32, (3, 7), (8, 1))):  # dtype, shape, density
            with pytest.raises(ValueError, match="out must be a dense float32 array of shape \\(3, 7\\)"):
                fn(a, out=out)
        view = FakeArray(np.float32, (3, 7), (8, 1))
        with pytest.raises(ValueError, match="in place"):
            fn(view, out=view)
    for out in (FakeArray(np.float64, (3,)), FakeArray(np.float32, (7,)), FakeArray(np.float32, (3, 1))):
        with pytest.raises(ValueError, match="logsumexp: out must be a dense float32 array of shape \\(3,\\)"):
            lib.logsumexp(a, out=out)
    with pytest.raises(ValueError, match="shape \\(3, 1\\)"):
        lib.logsumexp(a, keepdims=True, out=FakeArray(np.float32, (3,)))
    with pytest.raises(ValueError, match="shape \\(1,\\)"):
        lib.logsumexp(a, axis=None, out=FakeArray(np.float32, (3,)))


def test_the_header_declares_both_entry_points():
    assert {"smhip_softmax_axis", "smhip_softmax_plan"} <= set(sma.declared_symbols())
