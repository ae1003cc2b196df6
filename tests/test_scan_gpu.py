"""Cumulative scans on the GPU (smhip_scan_axis through the ctypes binding) against numpy: cumsum, cumprod, cummax and cummin
of f32, f64, i32 and i64 along every axis of 1-D .. 6-D arrays, every route of the planner, views, in place, NaN,
determinism, ordering behind a recorded tiny operator, and one input of more than 2^31 elements."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

KINDS = ("cumsum", "cumprod", "cummax", "cummin")
DTYPES = (np.float32, np.float64, np.int32, np.int64)
ROW_SPLIT, COLUMN_SPLIT = ((1, (1 << 18) + 5), 1), ((70001, 8), 0)  # the planner tests' two SPLIT shapes


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return list(reversed(st))


def exact_input(kind, shape, dtype, axis, seed):
    """Data whose scan along `axis` (None: the flattened array) is exact in every order of evaluation.  Floats: integers
    in [-1000, 1000] for sum / max / min; for prod x_k = +-2^(e_k - e_(k-1)), e_k random in [-30, 30], so that every run of
    consecutive factors is a power of two within 2^+-60.  Integers: full range, odd for prod (the product never collapses)."""
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
        return x | dtype(1) if kind == "cumprod" else x
    if kind != "cumprod":
        return rng.integers(-1000, 1000, size=shape, endpoint=True).astype(dtype)
    e = rng.integers(-30, 30, size=shape, endpoint=True)
    flat = e.reshape(-1) if axis is None else e
    prev = np.zeros_like(flat)
    ax = 0 if axis is None else axis
    sl_to, sl_from = [slice(None)] * flat.ndim, [slice(None)] * flat.ndim
    sl_to[ax], sl_from[ax] = slice(1, None), slice(None, -1)
    prev[tuple(sl_to)] = flat[tuple(sl_from)]
    sign = rng.choice(np.array([-1.0, 1.0]), size=flat.shape)
    return (sign * np.exp2((flat - prev).astype(np.float64))).reshape(shape).astype(dtype)


def expected(kind, x, axis):
    """numpy's scan under the contract of smhip.h; axis None: of the flattened array."""
    if axis is None:
        x, axis = x.reshape(-1), 0
    if kind == "cummax":
        return np.maximum.accumulate(x, axis=axis)
    if kind == "cummin":
        return np.minimum.accumulate(x, axis=axis)
    f = np.cumsum if kind == "cumsum" else np.cumprod
    if np.issubdtype(x.dtype, np.integer):
        return f(x, axis=axis, dtype=x.dtype)
    return f(x.astype(np.float64), axis=axis).astype(x.dtype)


def check_exact(lib, kind, shape, dtype, axis, seed):
    x = exact_input(kind, shape, dtype, axis, seed)
    got = lib.scan(kind, lib.to_device(x), axis).numpy()
    want = expected(kind, x, axis)
    assert got.shape == want.shape, (kind, shape, axis, got.shape)
    assert np.array_equal(got, want), (kind, np.dtype(dtype).name, shape, axis, int(np.argmax((got != want).reshape(-1))))


SHAPES = [(1,), (5,), (255,), (256,), (257,), (1025,), (4097,), (65, 63), (63, 4097), (3, 5, 4097), (4097, 3, 5), (5, 65, 3),
          (2, 3, 1, 65, 5), (2, 3, 4, 5, 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_exact_matrix(smhip, dtype):
    for si, shape in enumerate(SHAPES):
        for axis in list(range(len(shape))) + [None]:
            for kind in KINDS:
                check_exact(smhip, kind, shape, dtype, axis, 100 * si + (0 if axis is None else axis + 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_exact_around_the_chunk_length(smhip, dtype):
    """R = the chunk length the planner reports for the two SPLIT shapes, that length +- 1 and twice it plus 3, and the
    shapes themselves."""
    for (shape, axis) in (ROW_SPLIT, COLUMN_SPLIT):
        route, launches, ori, chunk = smhip.scan_plan("cumsum", dtype, list(shape), dense(shape), axis)
        assert route & sma.SCAN_SPLIT and launches == 2 and 1 < chunk < shape[axis]
        for k, R in enumerate((shape[axis], chunk, chunk - 1, chunk + 1, 2 * chunk + 3)):
            s = list(shape)
            s[axis] = R
            for kind in KINDS:
                check_exact(smhip, kind, tuple(s), dtype, axis, 7000 + k)


def check_rounded(kind, x, axis, got):
    """The contract's bound, which holds for any parenthesisation: output r of a sum is within r * 2^-53 * sum_{k<=r}|x_k| of
    the exact prefix, of a product within r * 2^-53 relative; an f32 output adds half an f32 ulp for its one rounding.  The
    reference is a np.longdouble running fold.  Where that exceeds the output type's range (products of factors from
    [0.5, 2) drift upwards) the result must be the infinity of the same sign."""
    xl = x.astype(np.longdouble)
    with np.errstate(over="ignore"):
        want = (np.cumsum if kind == "cumsum" else np.cumprod)(xl, axis=axis)
    r = np.arange(x.shape[axis], dtype=np.longdouble).reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    u = np.longdouble(2.0) ** -53
    bound = r * u * (np.cumsum(np.abs(xl), axis=axis) if kind == "cumsum" else np.abs(want))
    over = np.abs(want) > np.longdouble(np.finfo(x.dtype).max)
    fin = ~over
    if x.dtype == np.float32:
        bound = bound + np.where(fin, np.spacing(np.abs(np.where(fin, want, 0)).astype(np.float32)).astype(np.longdouble) / 2, 0)
    with np.errstate(invalid="ignore"):  # inf - inf where both have overflowed: checked apart, below
        err = np.abs(got.astype(np.longdouble) - want)
    worst = float(np.max(np.where(fin, err - bound, -1)))
    print(f"{kind} {x.dtype} {x.shape} axis {axis}: max(err - bound) = {worst:.3e}, overflowed outputs {int(over.sum())}")
    assert np.all(err[fin] <= bound[fin]), (kind, x.dtype, x.shape, axis, worst)
    assert np.array_equal(got[over], np.where(want[over] > 0, np.inf, -np.inf).astype(x.dtype))


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_rounded_data_within_the_contract_bound(smhip, dtype):
    rng = np.random.default_rng(5)
    for shape, axes in (((63, 4097), (0, 1)), (ROW_SPLIT[0], (1,))):
        xs = (rng.standard_normal(shape) * 10.0).astype(dtype)
        xp = (rng.uniform(0.5, 2.0, size=shape) * rng.choice(np.array([-1.0, 1.0]), size=shape)).astype(dtype)
        for kind, x in (("cumsum", xs), ("cumprod", xp)):
            d = smhip.to_device(x)
            for axis in axes:
                check_rounded(kind, x, axis, smhip.scan(kind, d, axis).numpy())


# (name, shape, axis, strides or None for dense, route id, flags) -- asserted through scan_plan, so no route is missed silently
ROUTE_CASES = [
    ("row short, 4 lanes", (1000, 13), 1, None, sma.SCAN_ROUTE_ROW, 0),
    ("row short, 16 lanes", (300, 61), 1, None, sma.SCAN_ROUTE_ROW, 0),
    ("row short, 64 lanes", (70, 255), 1, None, sma.SCAN_ROUTE_ROW, 0),
    ("row long", (1100, 9001), 1, None, sma.SCAN_ROUTE_ROW, 0),
    ("column", (300, 4099), 0, None, sma.SCAN_ROUTE_COLUMN, 0),
    ("column, packed", (3000, 37, 6), 1, None, sma.SCAN_ROUTE_COLUMN, 0),
    ("row + split", (3, 70001), 1, None, sma.SCAN_ROUTE_ROW, sma.SCAN_SPLIT),
    ("column + split", (9001, 5, 7), 0, None, sma.SCAN_ROUTE_COLUMN, sma.SCAN_SPLIT),
    ("copy, transposed", (300, 257), 1, (1, 300), sma.SCAN_ROUTE_ROW, sma.SCAN_COPY),
    ("copy + split", (6, 40001), 1, (1, 6), sma.SCAN_ROUTE_ROW, sma.SCAN_COPY | sma.SCAN_SPLIT),
    ("copyonly", (500, 1, 33), 1, None, sma.SCAN_ROUTE_COPYONLY, 0),
    ("copyonly of a view", (33, 1, 500), 1, (1, 1, 33), sma.SCAN_ROUTE_COPYONLY, 0),
]


def run_route_cases(lib):
    for ci, (name, shape, axis, strides, route, flags) in enumerate(ROUTE_CASES):
        for dtype in DTYPES:
            st = dense(shape) if strides is None else list(strides)
            word, launches, ori, chunk = lib.scan_plan("cumsum", dtype, list(shape), st, axis)
            assert (word & 0xff, word & ~0xff) == (route, flags), (name, np.dtype(dtype).name, hex(word))
            for kind in KINDS:
                # a strided case: the base array holds the elements in the order of the strides; the view permutes it back
                order = sorted(range(len(shape)), key=lambda d: -st[d]) if strides is not None else list(range(len(shape)))
                base_shape = tuple(shape[d] for d in order)
                view_axis = order.index(axis)
                base = exact_input(kind, base_shape, dtype, view_axis, 900 + ci)
                view = base.transpose(np.argsort(order))
                assert view.shape == tuple(shape)
                d = lib.to_device(base)
                dv = d.view_like(view, base)
                if strides is not None:
                    assert list(dv.strides) == st, (name, dv.strides)
                got = lib.scan(kind, dv, axis).numpy()
                assert np.array_equal(got, expected(kind, view, axis)), (name, kind, np.dtype(dtype).name)


def test_every_route(smhip):
    run_route_cases(smhip)


_CAPPED = """
import simplemath_amd as sma
from tests.test_scan_gpu import run_route_cases
lib = sma.load()
lib.set_device(0)
run_route_cases(lib)
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_SCAN_GRID_CAP=3: every kernel's loop over its tasks runs many times per lane, on every route."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_SCAN_GRID_CAP="3", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_views(smhip, dtype):
    base = exact_input("cumsum", (70, 130, 6), dtype, 0, 3)
    d = smhip.to_device(base)
    views = [base.transpose(1, 0, 2), base[:, 7:120:3], np.broadcast_to(base[:, :1, :], (70, 9, 6)), base[3:60, 5:77, 1:5]]
    for v in views:
        dv = d.view_like(v, base)
        for axis in range(v.ndim):
            for kind in ("cumsum", "cummax", "cummin"):
                assert np.array_equal(smhip.scan(kind, dv, axis).numpy(), expected(kind, v, axis)), (kind, v.shape, v.strides, axis)
        assert np.array_equal(smhip.scan("cumsum", dv).numpy(), expected("cumsum", np.ascontiguousarray(v), None))
    # cumprod: data whose runs along the scanned axis of the VIEW are exact
    pb = exact_input("cumprod", (130, 70, 6), dtype, 0, 4)
    pv = pb.transpose(1, 0, 2)
    assert np.array_equal(smhip.scan("cumprod", smhip.to_device(pb).view_like(pv, pb), 1).numpy(), expected("cumprod", pv, 1))


def test_in_place(smhip):
    x = exact_input("cumsum", (65, 4097), np.float32, 1, 8)
    a = smhip.to_device(x)
    want = smhip.scan("cumsum", a, 1).numpy()
    assert np.array_equal(a.numpy(), x)  # the out-of-place call leaves its operand alone
    assert np.array_equal(want, expected("cumsum", x, 1))
    d = smhip.to_device(x)
    r = smhip.scan("cumsum", d, 1, out=d)
    assert r is d and np.array_equal(d.numpy(), want)
    for axis, kind in ((0, "cummax"), (None, "cumsum")):  # the column walk and the flattened row, split
        d = smhip.to_device(x)
        smhip.scan(kind, d, axis, out=d)
        assert np.array_equal(d.numpy().reshape(-1), expected(kind, x, axis).reshape(-1))
    # out == a with a non-dense operand is refused
    t = a.view_like(x.T, x)
    with pytest.raises(sma.SmhipError) as e:
        smhip._ck(smhip.scan_raw(sma.SCAN_SUM, sma.F32, t.ptr, list(t.shape), list(t.strides), 0, t.ptr))
    assert e.value.code == sma.ERR_INVALID


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_nan_from_its_position_on(smhip, dtype):
    R = 1025
    x = exact_input("cumsum", (4, R), dtype, 1, 12)
    where = (0, 255, 256, R - 1)
    for row, pos in enumerate(where):
        x[row, pos] = np.nan
    for xx, axis in ((x, 1), (np.ascontiguousarray(x.T), 0)):  # the row walk and the column walk
        d = smhip.to_device(xx)
        for kind in ("cummax", "cummin", "cumsum"):
            got = smhip.scan(kind, d, axis).numpy()
            got = got if axis == 1 else got.T
            clean = expected(kind, np.nan_to_num(x, nan=0.0), 1)
            for row, pos in enumerate(where):
                assert np.all(np.isnan(got[row, pos:])), (kind, row)
                assert np.array_equal(got[row, :pos], clean[row, :pos]), (kind, row)


def test_deterministic(smhip):
    rng = np.random.default_rng(9)
    hip = smhip.c  # the HIP runtime libsmhip.so itself is linked against (dlsym follows its dependencies)
    for shape, axis in (((63, 4097), 1), ((63, 4097), 0), ROW_SPLIT, COLUMN_SPLIT):
        x = rng.standard_normal(shape).astype(np.float32)
        d = smhip.to_device(x)
        a = smhip.scan("cumsum", d, axis).numpy().tobytes()
        assert smhip.scan("cumsum", d, axis).numpy().tobytes() == a
        smhip.synchronize()
        stream = C.c_void_p(0)
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        try:
            smhip.set_stream(stream.value)
            c = smhip.scan("cumsum", d, axis).numpy().tobytes()
            smhip.synchronize()
        finally:
            smhip.set_stream(0)
            hip.hipStreamDestroy(stream)
        assert c == a


def test_ordered_behind_a_recorded_tiny_operator(smhip):
    x = exact_input("cumsum", (40, 50), np.float32, 0, 13)
    d = smhip.to_device(x)
    before = smhip.tiny_stats()
    d3 = smhip.array_scalar(sma.OP_MUL, d, 3.0)  # 2000 results: recorded, not yet launched
    got0 = smhip.scan("cumsum", d3, 0)
    got1 = smhip.scan("cummax", d3, 1)
    assert smhip.tiny_stats()[1] > before[1]
    assert np.array_equal(got0.numpy(), expected("cumsum", x * np.float32(3.0), 0))
    assert np.array_equal(got1.numpy(), expected("cummax", x * np.float32(3.0), 1))


def test_more_than_2_31_elements(smhip):
    """(2^31 + 4099,) int32 ones: cumsum[r] = r + 1, wrapped to int32.  Four windows of 4096 elements are downloaded: the
    start, around 2^31 - 1, around a chunk boundary of the plan, and the end."""
    N = (1 << 31) + 4099
    route, launches, ori, chunk = smhip.scan_plan("cumsum", np.int32, [N], [1], 0)
    assert route == sma.SCAN_ROUTE_ROW | sma.SCAN_SPLIT and 0 < chunk < N
    a = smhip.full((N,), 1, np.int32)
    out = smhip.scan("cumsum", a, 0)
    del a
    boundary = chunk * ((N // chunk) // 2 + 1)  # a chunk boundary beyond the middle
    for start in (0, (1 << 31) - 1 - 2048, boundary - 2048, N - 4096):
        got = np.empty(4096, np.int32)
        smhip.download(got, out.ptr + start * 4)
        want = (np.arange(start + 1, start + 4097, dtype=np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)
        assert np.array_equal(got, want), start
