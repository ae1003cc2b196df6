"""Axis reductions on the GPU (smhip_reduce_axes through the ctypes binding) against numpy: sum, mean, max and min of f32,
f64, i32 and i64 over every single axis and adjacent / non-adjacent masks of 1-D .. 6-D arrays, views, NaN, determinism
and one input of more than 2^31 elements."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

KINDS = ("sum", "mean", "max", "min")
DTYPES = (np.float32, np.float64, np.int32, np.int64)


def sample(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)  # int32 sums overflow
    return (rng.standard_normal(shape) * 10.0).astype(dtype)


def ulp_f32(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-0x80000000) - ia, ia)
    ib = np.where(ib < 0, np.int64(-0x80000000) - ib, ib)
    return np.abs(ia - ib)


def check(kind, x, axes, got, keepdims=False):
    """`got` (numpy) against numpy's reduction of the host array / view `x` under the contract of smhip.h."""
    axes = tuple(axes)
    count = int(np.prod([x.shape[d] for d in axes], dtype=np.int64))
    want_shape = np.sum(x, axis=axes, keepdims=keepdims).shape or (1,)
    assert got.shape == want_shape, (got.shape, want_shape)
    if kind in ("max", "min"):
        want = (np.max if kind == "max" else np.min)(x, axis=axes, keepdims=keepdims).reshape(want_shape)
        assert np.array_equal(got, want, equal_nan=np.issubdtype(x.dtype, np.floating)), (kind, x.dtype, x.shape, axes)
        return
    if np.issubdtype(x.dtype, np.integer):
        want = np.sum(x, axis=axes, dtype=x.dtype, keepdims=keepdims).reshape(want_shape)
        assert np.array_equal(got, want), (x.dtype, x.shape, axes)
        return
    if x.dtype == np.float32:
        s = np.sum(x.astype(np.float64), axis=axes, keepdims=keepdims)
        want = (s / count if kind == "mean" else s).astype(np.float32).reshape(want_shape)
        assert ulp_f32(got, want).max(initial=0) <= 1, (kind, x.shape, axes)
        return
    s = np.sum(x.astype(np.longdouble), axis=axes, keepdims=keepdims)
    bound = count * 2.0 ** -53 * np.sum(np.abs(x).astype(np.longdouble), axis=axes, keepdims=keepdims)
    if kind == "mean":
        s, bound = s / count, bound / count + np.abs(s / count) * 2.0 ** -53
    err = np.abs(got.astype(np.longdouble) - s.reshape(want_shape))
    assert np.all(err <= bound.reshape(want_shape) + 1e-300), (kind, x.shape, axes, err.max())


def masks(ndim, limit=None):
    out = [(d,) for d in range(ndim)]
    for r in range(2, ndim + 1):
        out += list(itertools.combinations(range(ndim), r))
    return out if limit is None else out[:limit]


SHAPES = [(4097,), (65, 63), (63, 4097), (3, 5, 4097), (4097, 3, 5), (5, 65, 3), (2, 3, 1, 65, 5), (3, 2, 5, 1, 3, 4), (2, 3, 4, 5, 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_matrix_dense(smhip, dtype):
    for si, shape in enumerate(SHAPES):
        x = sample(shape, dtype, si)
        d = smhip.to_device(x)
        for axes in masks(len(shape), limit=None if len(shape) <= 4 else 12):
            for kind in KINDS:
                if kind == "mean" and np.issubdtype(dtype, np.integer):
                    continue
                keep = (si + len(axes)) % 2 == 1
                got = smhip.reduce(kind, d, axes, keepdims=keep).numpy()
                check(kind, x, axes, got, keepdims=keep)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_three_reduced_groups(smhip, dtype):
    """Masks that leave three separate reduced groups: three passes (T -> S, S -> S, S -> T), dense and through the copy."""
    base = sample((2, 3, 4, 5, 3, 2), dtype, 21)
    d = smhip.to_device(base)
    view = base.transpose(0, 2, 1, 3, 5, 4)[:, 1:, :, ::2]
    dv = d.view_like(view, base)
    for x, dx in ((base, d), (view, dv)):
        for axes in ((0, 2, 4), (1, 3, 5), (0, 2, 3, 5), (0, 1, 3, 5)):
            route, launches, _ = smhip.reduce_plan("sum", dtype, list(dx.shape), list(dx.strides), axes)
            assert route & sma.ROUTE_PASSES
            for kind in KINDS:
                if kind == "mean" and np.issubdtype(dtype, np.integer):
                    continue
                check(kind, x, axes, smhip.reduce(kind, dx, axes, keepdims=len(axes) == 3).numpy(), keepdims=len(axes) == 3)


@pytest.mark.parametrize("I", (2, 12))
def test_many_outer_indices(smhip, I):
    """O = 2^24 + 1 outer indices over a short reduced axis: more workgroups than one launch's 32-bit work-item count allows
    if each outer index had its own -- the kernels loop over their tasks instead."""
    O = (1 << 24) + 1
    a = (np.arange(O, dtype=np.int32) % 97).astype(np.float32)
    b = np.arange(2 * I, dtype=np.float32).reshape(2, I) - 7.0
    x = np.add(a[:, None, None], b[None], dtype=np.float32)
    d = smhip.to_device(x)
    del x
    s = smhip.reduce("sum", d, 1).numpy()
    assert np.array_equal(s, 2.0 * a[:, None] + (b[0] + b[1])[None].astype(np.float32))
    m = smhip.reduce("mean", d, 1).numpy()
    assert np.array_equal(m, a[:, None] + ((b[0] + b[1]) / 2.0)[None].astype(np.float32))
    assert np.array_equal(smhip.reduce("max", d, 1).numpy(), a[:, None] + b[1][None])
    assert np.array_equal(smhip.reduce("min", d, (1,), keepdims=True).numpy(), (a[:, None] + b[0][None])[:, None, :])


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_axis_reduce_gpu import sample, check, KINDS
lib = sma.load()
lib.set_device(0)
cases = [((3000, 5, 3), 1), ((64, 2048, 3), 1), ((1 << 16, 3), 1), ((40, 3000), 1), ((2, 70001), 1), ((700, 33), 0),
         ((9, 300, 17), 1), ((3, 5000, 2), (0, 1)), ((5, 4, 3, 6), (0, 2))]
for dtype in (np.float32, np.float64, np.int32, np.int64):
    for i, (shape, axes) in enumerate(cases):
        x = sample(shape, dtype, 40 + i)
        d = lib.to_device(x)
        ax = axes if isinstance(axes, tuple) else (axes,)
        for kind in KINDS:
            if kind == "mean" and np.issubdtype(dtype, np.integer):
                continue
            check(kind, x, ax, lib.reduce(kind, d, axes).numpy())
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_REDUCE_GRID_CAP=3: every kernel's loop over its tasks runs many times per lane, on every route."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_REDUCE_GRID_CAP="3", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_odd_extents_every_route(smhip, dtype):
    """R and I of 1, 3, 5, 63, 65 and 4097 through the row, column and channel walks, with and without the split of R."""
    ext = (1, 3, 5, 63, 65, 4097)
    for i, (o, r) in enumerate(itertools.product(ext, ext)):
        x = sample((o, r), dtype, 100 + i)
        d = smhip.to_device(x)
        for kind in KINDS:
            if kind == "mean" and np.issubdtype(dtype, np.integer):
                continue
            for ax in (0, 1):
                check(kind, x, (ax,), smhip.reduce(kind, d, ax).numpy())
    # long rows, few of them (the split row walk), and short rows of many lengths
    for shape, ax in (((3, 70001), 1), ((70001, 3), 0), ((5, 70001), 0), ((2, 4099, 5), (0, 1)), ((1000, 257), 1), ((7, 1031, 9), 1)):
        x = sample(shape, dtype, 7)
        d = smhip.to_device(x)
        for kind in KINDS:
            if kind == "mean" and np.issubdtype(dtype, np.integer):
                continue
            check(kind, x, ax if isinstance(ax, tuple) else (ax,), smhip.reduce(kind, d, ax).numpy())


def test_int32_sum_wraps_like_numpy(smhip):
    x = np.full((3, 1000), 2**31 - 1, dtype=np.int32)
    got = smhip.reduce("sum", smhip.to_device(x), 1).numpy()
    assert np.array_equal(got, np.sum(x, axis=1, dtype=np.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_views(smhip, dtype):
    base = sample((70, 130, 6), dtype, 3)
    d = smhip.to_device(base)
    views = [base.transpose(1, 0, 2), base.transpose(2, 1, 0), base[3:60, 5:], base[:, 7:120:3], base[::2, :, 1:5],
             base[5, :, :].T, base[:, :, 4], base[::-1][::-1][1:, ::5, ::2]]
    for v in views:
        dv = d.view_like(v, base)
        for axes in masks(v.ndim):
            for kind in KINDS:
                if kind == "mean" and np.issubdtype(dtype, np.integer):
                    continue
                check(kind, v, axes, smhip.reduce(kind, dv, axes).numpy())


def test_transposed_view_equals_row_reduction(smhip):
    A = sample((300, 2000), np.float32, 11)
    d = smhip.to_device(A)
    t = d.view_like(A.T, A)
    for kind in KINDS:
        assert smhip.reduce(kind, t, 0).numpy().tobytes() == smhip.reduce(kind, d, 1).numpy().tobytes()
        assert smhip.reduce(kind, t, 1).numpy().tobytes() == smhip.reduce(kind, d, 0).numpy().tobytes()


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_nan_propagates_through_max_and_min(smhip, dtype):
    x = sample((40, 300, 3), dtype, 5)
    x[3, 7, 1] = np.nan
    x[11, 299, 0] = np.nan
    x[:, 0, 2] = np.nan
    d = smhip.to_device(x)
    for axes in masks(3):
        for kind in ("max", "min"):
            check(kind, x, axes, smhip.reduce(kind, d, axes).numpy())


def test_empty_extents(smhip):
    x = np.zeros((4, 0, 3), dtype=np.float32)
    d = smhip.empty((4, 0, 3), np.float32)
    got = smhip.reduce("sum", d, 1).numpy()
    assert np.array_equal(got, np.zeros((4, 3), np.float32))
    assert smhip.reduce("max", d, (0, 2)).shape == (0,)  # an empty result: nothing to compute
    for kind in ("mean", "max", "min"):
        with pytest.raises(sma.SmhipError) as e:
            smhip.reduce(kind, d, 1)
        assert e.value.code == sma.ERR_INVALID
    del x


def test_deterministic_on_the_split_route(smhip):
    x = sample((4, 1 << 22), np.float32, 9)
    d = smhip.to_device(x)
    route, launches, _ = smhip.reduce_plan("sum", np.float32, list(x.shape), [1 << 22, 1], 1)
    assert route & sma.ROUTE_SPLIT
    for kind in ("sum", "mean"):
        a = smhip.reduce(kind, d, 1).numpy().tobytes()
        b = smhip.reduce(kind, d, 1).numpy().tobytes()
        assert a == b
    y = sample((1 << 20, 4), np.float64, 10)
    dy = smhip.to_device(y)
    assert smhip.reduce("sum", dy, 0).numpy().tobytes() == smhip.reduce("sum", dy, 0).numpy().tobytes()
    check("sum", y, (0,), smhip.reduce("sum", dy, 0).numpy())


def test_more_than_2_31_elements(smhip):
    """(2, 2^30 + 3) f32: row 0 all 1, row 1 all 2 except its last element 1000 -- sums, max, min known exactly."""
    R = (1 << 30) + 3
    a = smhip.empty((2, R), np.float32)
    for row, v in ((0, 1.0), (1, 2.0)):
        val = np.array([v], np.float32)
        smhip._ck(smhip.c.smhip_fill(C.c_int(sma.F32), C.c_void_p(a.ptr + row * R * 4), val.ctypes.data_as(C.c_void_p), C.c_size_t(R)))
    smhip.upload(a.ptr + (2 * R - 1) * 4, np.array([1000.0], np.float32))
    s = smhip.reduce("sum", a, 1).numpy()
    assert s[0] == np.float32(R) and s[1] == np.float32(2.0 * (R - 1) + 1000.0)
    assert np.array_equal(smhip.reduce("max", a, 1).numpy(), np.array([1.0, 1000.0], np.float32))
    assert np.array_equal(smhip.reduce("min", a, 1).numpy(), np.array([1.0, 2.0], np.float32))
    assert smhip.reduce("sum", a, (0, 1)).numpy()[0] == np.float32(3.0 * R - 2.0 + 1000.0)
    m = smhip.reduce("mean", a, (0, 1)).numpy()[0]
    assert m == np.float32((3.0 * R - 2.0 + 1000.0) / (2 * R))
