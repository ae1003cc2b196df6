"""quantile, percentile and median without a device: the arithmetic on the host (tests/cpp/quantile_host_check.cpp compiles
csrc/sm_quantile.h with g++ and checks the key-only radix select, the ranks and the interpolation, once more with the sanitizers on), the
planner (smhip_quantile_plan through the binding), what the two entry points refuse, and the binding's errors.

L (the longest line a selection holds in LDS) and Qmax (the most probabilities it serves) are read from the plan, never written here.
The refusals are pinned as literals in this file: the return code and the FULL message.  They are replayed only without a device (the
pointers are made-up integers), like tests/test_abi_errors_host.py."""
import ctypes as ct
import re
import subprocess

import numpy as np
import pytest

import simplemath_amd as sma

DTYPES = (np.float32, np.float64)
IDS = dict(ids=lambda d: np.dtype(d).name)
A, B = 1 << 20, 2 << 20  # stand-ins for device pointers: never dereferenced
NONE, COPYONLY, ROW, SORT, STREAM, COPY = (sma.QUANTILE_ROUTE_NONE, sma.QUANTILE_ROUTE_COPYONLY, sma.QUANTILE_ROUTE_ROW, sma.QUANTILE_ROUTE_SORT,
                                           sma.QUANTILE_STREAM, sma.QUANTILE_COPY)


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


@pytest.mark.parametrize("program", ["quantile_host_check", "quantile_host_check_san"])
def test_the_arithmetic_on_the_host(program):
    """The radix select over the header's digit rule against std::nth_element and a sort (ties, both zeros, infinities, NaNs, constant
    lines), (j, g) of every method at R = 1 .. 5, the interpolation's special cases.  _san: built with -fsanitize=address,undefined."""
    from simplemath_amd import build
    exe = build.build_host_programs()[program]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    m = re.search(r"^quantile_host_check: (\d+) checks, 0 failures$", r.stdout, re.M)
    assert r.returncode == 0 and m and int(m.group(1)) > 100000, r.stdout[-3000:] + r.stderr[-2000:]


def limits(lib, dtype):
    _, _, _, info = lib.quantile_plan(dtype, [1 << 20], [1], 0, [0.5])
    return info[0], info[1]


def probabilities(n):
    return [k / max(n - 1, 1) for k in range(n)] if n > 1 else [0.5]


def ranks_wanted(R, qs, method):
    """The distinct ranks a call selects: lo of every probability, and hi where it interpolates (smhip.h's rules)."""
    wanted = set()
    for q in qs:
        h = float(R - 1) * q
        j, g = np.floor(h), h - np.floor(h)
        if method == "higher":
            j = np.ceil(h)
        elif method == "nearest":
            j = np.rint(h)
        wanted.add(int(j))
        if g != 0 and method in ("linear", "midpoint"):
            wanted.add(int(j) + 1)
    return len(wanted)


def served_in_lds(R, L):
    """The most distinct ranks a line held in LDS is selected for ahead of the sort (include/smhip.h, SMHIP_QUANTILE_ROUTE_SORT)."""
    return 2 if R <= L // 4 else 8


def stream_launches(dtype):
    """The streamed route queues the same launches whatever the data: the tables' initialisation, a count and a narrowing per key byte,
    the compaction, the finish."""
    return 1 + 2 * np.dtype(dtype).itemsize + 2


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_and_launches_along_the_last_axis(lib, dtype):
    L, qmax = limits(lib, dtype)
    assert L >= 1024 and qmax == 16
    for R in (1, 2, 128, 129, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17):
        for Q in (1, 3, 16, 17):
            for method in sma.QUANTILE_METHODS:
                route, launches, ori, info = lib.quantile_plan(dtype, [3, R], [R, 1], 1, probabilities(Q), method)
                what = (R, Q, method)
                assert ori == (3, R, 1) and info[:2] == (L, qmax), what
                if R == 1:
                    assert (route, launches, info[2]) == (COPYONLY, 1 + -(-Q // qmax), 1), what  # the copy, then the picks
                elif Q > qmax or (R <= L and ranks_wanted(R, probabilities(Q), method) > served_in_lds(R, L)):
                    picks = -(-Q // qmax)
                    assert (route, launches, info[2]) == (SORT, lib.sort_plan(dtype, [3, R], [R, 1], 1)[1] + picks, 1), what
                elif R <= L:
                    assert (route, launches, info[2]) == (ROW, 1, 1), what
                else:
                    assert (route, launches, info[2]) == (ROW | STREAM, stream_launches(dtype), np.dtype(dtype).itemsize + 1), what


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_first_axis_views_and_zero_extents(lib, dtype):
    L, qmax = limits(lib, dtype)
    info = (L, qmax, 1)
    # axis 0 of a dense (70, 50): staged in, selected; the rows [Q][50] are the result
    assert lib.quantile_plan(dtype, [70, 50], [50, 1], 0, [0.5]) == (ROW | COPY, 2, (1, 70, 50), info)
    assert lib.quantile_plan(dtype, [70, 50], [50, 1], 0, [0.0, 1.0]) == (ROW | COPY, 2, (1, 70, 50), info)
    assert lib.quantile_plan(dtype, [2000, 50], [50, 1], 0, probabilities(3)) == (ROW | COPY, 2, (1, 2000, 50), info)
    # ... of a long one: staged in, streamed
    assert lib.quantile_plan(dtype, [2 * L + 1, 9], [9, 1], 0, [0.5]) == (ROW | STREAM | COPY, 1 + stream_launches(dtype), (1, 2 * L + 1, 9),
                                                                         (L, qmax, np.dtype(dtype).itemsize + 1))
    # a transposed view along the axis with the unit stride in memory: read in place, its rows are the result
    assert lib.quantile_plan(dtype, [130, 70], [1, 130], 0, [0.0, 1.0]) == (ROW, 1, (70, 130, 1), info)
    assert lib.quantile_plan(dtype, [130, 70], [1, 130], 0, probabilities(3))[0] & 0xFF == SORT  # five ranks of a wave's line
    # a 3-D array along its middle axis: staged in; along its last: in place
    assert lib.quantile_plan(dtype, [5, 33, 7], [231, 7, 1], 1, [0.5]) == (ROW | COPY, 2, (5, 33, 7), info)
    assert lib.quantile_plan(dtype, [5, 33, 7], [231, 7, 1], 2, [0.5]) == (ROW, 1, (165, 7, 1), info)
    # kept axes that stand in another order in memory than in the result do not merge into one outer group: staged in, like any other view
    assert lib.quantile_plan(dtype, [5, 7, 33], [33, 165, 1], 2, [0.5]) == (ROW | COPY, 2, (35, 33, 1), info)
    # a stepped and a stride-0 view along the last axis: staged in
    assert lib.quantile_plan(dtype, [70, 65], [130, 2], 1, [0.5]) == (ROW | COPY, 2, (70, 65, 1), info)
    assert lib.quantile_plan(dtype, [9, 300], [1, 0], 1, [0.5]) == (ROW | COPY, 2, (9, 300, 1), info)
    # SORT carries the sort's own staging
    srt = lib.sort_plan(dtype, [300, 50], [50, 1], 0)
    assert srt[0] & sma.SORT_COPY
    assert lib.quantile_plan(dtype, [300, 50], [50, 1], 0, probabilities(qmax + 1)) == (SORT | COPY, srt[1] + 2, (1, 300, 50), info)
    assert lib.quantile_plan(dtype, [300, 50], [50, 1], 0, probabilities(2 * qmax + 1))[1] == srt[1] + 3
    # a streamed call whose compaction buffers would pass 256 MiB goes to the sort
    lines = (256 << 20) // (L * np.dtype(dtype).itemsize)
    assert lib.quantile_plan(dtype, [lines, L + 1], [L + 1, 1], 1, [0.0])[0] == ROW | STREAM
    assert lib.quantile_plan(dtype, [lines + 1, L + 1], [L + 1, 1], 1, [0.0])[0] == SORT
    assert lib.quantile_plan(dtype, [lines // 2 + 1, L + 2], [L + 2, 1], 1, [0.5])[0] == SORT  # the median of an even line: two ranks, lo and hi
    assert lib.quantile_plan(dtype, [lines // 2 + 1, L + 2], [L + 2, 1], 1, [0.5], "lower")[0] == ROW | STREAM
    # a zero extent in the result: nothing to do, whatever the axis holds
    for shape, axis in (([0, 65], 1), ([4, 0, 3], 0), ([4, 0, 3], 2), ([0, 0], 0)):
        dense = [int(np.prod(shape[d + 1:])) for d in range(len(shape))]
        route, launches, _, got = lib.quantile_plan(dtype, shape, dense, axis, [0.5])
        assert (route, launches, got) == (NONE, 0, (L, qmax, 0)), shape


def test_info_is_stable(lib):
    seen = {lib.quantile_plan(dt, shape, strides, axis, q)[3][:2] for dt in DTYPES for shape, strides, axis, q in
            (([7], [1], 0, [0.0]), ([3, 5000], [5000, 1], 1, [0.5]), ([70, 50], [50, 1], 0, probabilities(17)), ([0, 4], [4, 1], 1, [1.0]))}
    assert len(seen) == 1


INVALID, UNSUPPORTED = sma.ERR_INVALID, sma.ERR_UNSUPPORTED
BASE = dict(method=0, dtype=sma.F32, a_ptr=A, shape=[3, 7], strides=[7, 1], axis=1, q=[0.25, 0.5], out_ptr=B)
NAN = float("nan")
# one case per row of the contract's list; (what changes, the return code, the full message after "<entry point>: ")
CHECKS = [
    (dict(method=5), INVALID, "bad method 5"),
    (dict(method=-1), INVALID, "bad method -1"),
    (dict(dtype=99), INVALID, "bad dtype 99"),
    (dict(ndim=0), INVALID, "ndim 0 outside 1..6"),
    (dict(ndim=7), INVALID, "ndim 7 outside 1..6"),
    (dict(dtype=sma.I32), UNSUPPORTED, "an integer dtype (f32 and f64 only: astype first)"),
    (dict(dtype=sma.I64), UNSUPPORTED, "an integer dtype (f32 and f64 only: astype first)"),
    (dict(axis=2), INVALID, "axis 2 outside 0..1"),
    (dict(axis=-1), INVALID, "axis -1 outside 0..1"),
    (dict(shape=[3, -7]), INVALID, "negative extent or stride at dim 1"),
    (dict(strides=[-7, 1]), INVALID, "negative extent or stride at dim 0"),
    (dict(shape=None, ndim=2), INVALID, "null shape/strides"),
    (dict(strides=None, ndim=2), INVALID, "null shape/strides"),
    (dict(q=None, nq=2), INVALID, "null q"),
    (dict(q=[], nq=0), INVALID, "0 probabilities (at least one)"),
    (dict(q=[0.5], nq=-3), INVALID, "-3 probabilities (at least one)"),
    (dict(q=[0.5, 1.5]), INVALID, "q[1] = 1.5 outside [0, 1]"),
    (dict(q=[-0.25]), INVALID, "q[0] = -0.25 outside [0, 1]"),
    (dict(q=[0.0, 1.0, NAN]), INVALID, "q[2] = nan outside [0, 1]"),
    (dict(shape=[3, 1 << 31], strides=[1 << 31, 1]), UNSUPPORTED, "an axis of 2147483648 elements (ranks are 32 bits wide: below 2^31)"),
    (dict(shape=[3, 0], strides=[0, 1]), INVALID, "an empty axis with a result that is not empty"),
]
POINTERS = [  # smhip_quantile_axis alone
    (dict(a_ptr=0), INVALID, "null operand"),
    (dict(out_ptr=0), INVALID, "null out"),
    (dict(out_ptr=A), INVALID, "out overlaps the operand"),
    (dict(out_ptr=A + 80), INVALID, "out overlaps the operand"),
    (dict(a_ptr=B + 20), INVALID, "out overlaps the operand"),  # the second row of the two the result holds
]


def plan_raw(lib, kw):
    arr = lambda v: (ct.c_int64 * len(v))(*v) if v is not None else None
    q = kw["q"]
    ndim = kw.get("ndim", len(kw["shape"]) if kw["shape"] is not None else 2)
    return lib.c.smhip_quantile_plan(ct.c_int(kw["method"]), ct.c_int(kw["dtype"]), arr(kw["shape"]), arr(kw["strides"]), ct.c_int(ndim), ct.c_int(kw["axis"]),
                                     (ct.c_double * max(len(q), 1))(*q) if q is not None else None, ct.c_int64(kw.get("nq", len(q) if q is not None else 0)),
                                     None, None, None, None)


def test_refusals(lib):
    if lib.device_count():
        pytest.skip("a device is present: a call that got past its checks would launch on made-up pointers")
    for change, rc, msg in CHECKS + POINTERS:
        kw = dict(BASE, **change)
        assert lib.quantile_raw(**kw) == rc, change
        assert lib.c.smhip_last_error().decode() == "quantile_axis: " + msg, change
    for change, rc, msg in CHECKS:
        assert plan_raw(lib, dict(BASE, **change)) == rc, change
        assert lib.c.smhip_last_error().decode() == "quantile_plan: " + msg, change
    # nothing to do is no refusal, whatever the pointers: a kept extent of 0, with or without an empty axis
    assert lib.quantile_raw(**dict(BASE, shape=[0, 7], a_ptr=0, out_ptr=0)) == 0
    assert lib.quantile_raw(**dict(BASE, shape=[0, 0], strides=[0, 1], a_ptr=0, out_ptr=0)) == 0
    assert lib.quantile_raw(**dict(BASE, shape=[4, 0, 3], strides=[0, 3, 1], axis=0, a_ptr=0, out_ptr=0)) == 0


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
    for dtype in (np.int32, np.int64, np.int16):
        for call in (lambda x: lib.quantile(x, 0.5), lambda x: lib.percentile(x, 50), lambda x: lib.median(x)):
            with pytest.raises(TypeError, match="float32 and float64 only: astype first"):
                call(FakeArray(dtype, (3, 7)))
    with pytest.raises(ValueError, match="quantile: method 'cubic'"):
        lib.quantile(a, 0.5, method="cubic")
    for q in (-0.1, 1.5, NAN, [0.5, 2.0]):
        with pytest.raises(ValueError, match=r"quantile: q outside \[0, 1\] or NaN"):
            lib.quantile(a, q)
    for p in (-1, 100.5, [50, NAN]):
        with pytest.raises(ValueError, match=r"percentile: q outside \[0, 100\] or NaN"):
            lib.percentile(a, p)
    for q in ([], [[0.5]]):
        with pytest.raises(ValueError, match="quantile: q must be a number or a non-empty 1-D sequence"):
            lib.quantile(a, q)
    for axis in (2, -3):
        with pytest.raises(ValueError, match="out of bounds"):
            lib.median(a, axis)
    with pytest.raises(ValueError, match="median: an empty axis with a result that is not empty"):
        lib.median(FakeArray(np.float32, (3, 0)), 1)
    for out in (FakeArray(np.float64, (2, 3)), FakeArray(np.float32, (2, 4)), FakeArray(np.float32, (2, 3), (4, 1))):  # dtype, size, density
        with pytest.raises(ValueError, match="quantile: out must be a dense float32 array of 6 elements"):
            lib.quantile(a, [0.25, 0.75], out=out)
    with pytest.raises(ValueError, match=r"median: out must be a dense float32 array of 7 elements \(shape \(7,\)\)"):
        lib.median(a, 0, out=FakeArray(np.float32, (3,)))


def test_the_symbols_and_constants(lib):
    assert {"smhip_quantile_axis", "smhip_quantile_plan"} <= set(sma.declared_symbols())
    for name in ("smhip_quantile_axis", "smhip_quantile_plan"):
        assert getattr(lib.c, name).restype is ct.c_int
    assert (sma.QUANTILE_LINEAR, sma.QUANTILE_LOWER, sma.QUANTILE_HIGHER, sma.QUANTILE_NEAREST, sma.QUANTILE_MIDPOINT) == (0, 1, 2, 3, 4)
    assert sma.QUANTILE_METHODS == dict(linear=0, lower=1, higher=2, nearest=3, midpoint=4)
    assert (NONE, COPYONLY, ROW, SORT, STREAM, COPY) == (0, 1, 2, 3, 0x100, 0x200)
    header = open(sma.HEADER).read()
    for name, value in (("ROUTE_NONE", 0), ("ROUTE_COPYONLY", 1), ("ROUTE_ROW", 2), ("ROUTE_SORT", 3), ("STREAM", 0x100), ("COPY", 0x200)):
        m = re.search(rf"#define SMHIP_QUANTILE_{name} (\w+)", header)
        assert m and int(m.group(1), 0) == value, name
