"""argmax / argmin along an axis on the GPU (smhip_argreduce_axis through the ctypes binding) against numpy, bit for bit:
f32, f64, i32 and i64, both kinds, over every single axis of 1-D .. 6-D arrays, views, NaN, signed zeros, infinities, the
integer limits, both split routes, a capped grid and one input of more than 2^31 elements.

Every check is exact: np.array_equal(indices, np.argmax(x, axis)), and where the values are asked for their bytes are those of
np.take_along_axis(x, indices).  Inputs come in three kinds, because one kind hides a class of bug:
  continuous   random values, one extreme per line at a random place (a walk that misses late elements)
  ties         small integers in [-3, 3]: hundreds of ties per line, the first early on (a wrong tie-break between lanes,
               waves, chunks and launches)
  planted      a constant array with the extreme planted twice per line, the earlier one at each of: position 0, the last,
               the last element of the first vector and the first of the second, the first element of the line's vector tail,
               and both sides of every chunk boundary the plan reports.  Arrays above 8 MiB (the two big split shapes, with
               1023 and 65535 boundaries) take the boundaries next to the ends, at every multiple of 1024 chunks (where the
               first finishing launch cuts) and 16 drawn at random; (70001, 3) over axis 0 runs the same two finishing
               launches with every one of its 4375 boundaries."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

KINDS = ("argmax", "argmin")
DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
NP = {"argmax": np.argmax, "argmin": np.argmin}


def continuous(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 10.0).astype(dtype)


def ties(shape, dtype, seed):
    return np.random.default_rng(seed).integers(-3, 3, size=shape, endpoint=True).astype(dtype)


def check(kind, x, axis, idx, vals=None, keepdims=False):
    """indices (and values) as downloaded, against numpy on the host array / view `x`."""
    want = NP[kind](x, axis=axis)
    want_shape = (np.expand_dims(want, axis) if keepdims else want).shape or (1,)
    assert idx.dtype == np.int64 and idx.shape == want_shape, (idx.shape, want_shape)
    assert np.array_equal(idx.reshape(want.shape), want), (kind, x.dtype, x.shape, axis)
    if vals is not None:
        assert vals.dtype == x.dtype and vals.shape == want_shape
        taken = np.take_along_axis(x, np.expand_dims(want, axis), axis).squeeze(axis)
        assert vals.tobytes() == np.ascontiguousarray(taken).tobytes(), (kind, x.dtype, x.shape, axis)


def run(lib, x, d, axis, keepdims=False, values=True, kinds=KINDS):
    for kind in kinds:
        if values:
            vals, idx = lib.argreduce(kind, d, axis, keepdims=keepdims, values=True)
            check(kind, x, axis, idx.numpy(), vals.numpy(), keepdims)
        else:
            check(kind, x, axis, lib.argreduce(kind, d, axis, keepdims=keepdims).numpy(), None, keepdims)


def positions(lib, dtype, v, strides, axis, seed=0):
    """Where the planted kind puts its extremes along `axis` of the view (shape v.shape, strides in elements)."""
    R = v.shape[axis]
    W = 16 // np.dtype(dtype).itemsize
    route, _, _, chunk = lib.argreduce_plan("argmax", dtype, list(v.shape), list(strides), axis)
    s = {0, R - 1, W - 1, W, (R // W) * W}
    if route & sma.ARG_SPLIT:
        C_ = -(-R // chunk)
        if v.nbytes <= (8 << 20):
            cuts = range(1, C_)
        else:
            rng = np.random.default_rng(seed)
            cuts = {1, 2, 3, C_ - 3, C_ - 2, C_ - 1} | {int(c) for c in rng.integers(1, C_, size=16)}
            for m in range(1024, C_, 1024):
                cuts |= {m, m + 1}
            cuts = sorted(c for c in cuts if 1 <= c < C_)
        for c in cuts:
            s |= {c * chunk - 1, c * chunk}
    return sorted(p for p in s if 0 <= p < R)


def planted(lib, dtype, base_shape, viewf, axis, values=True, keepdims=False):
    """The constant array with +7 (for argmax) and -7 (for argmin) planted twice per line, as many rounds as it takes for
    every position to be the earlier of its two at least once."""
    b = np.full(base_shape, 1, dtype=dtype)
    d = lib.empty(base_shape, dtype)
    v = viewf(b)
    dv = d if v is b else d.view_like(v, b)
    pos = np.array(positions(lib, dtype, v, dv.strides, axis), dtype=np.int64)
    n = len(pos)
    vm = np.moveaxis(v, axis, -1)  # a view: writes reach b
    lines = vm.shape[:-1]
    nl = int(np.prod(lines, dtype=np.int64))
    j = np.arange(nl, dtype=np.int64).reshape(lines)
    together = n >= 8  # far enough apart for +7 and -7 never to meet on a line
    for k in range(-(-n // nl)):
        i1 = (k * nl + j) % n
        i2 = np.minimum(n - 1, i1 + 1 + (j + k) % 3)
        plans = [((7, i1, i2), (-7, (i1 + n // 2) % n, np.minimum(n - 1, (i1 + n // 2) % n + 1 + (j + k) % 3)))] if together else \
                [((7, i1, i2),), ((-7, i1, i2),)]
        for plan in plans:
            b[...] = 1
            for value, a1, a2 in plan:
                np.put_along_axis(vm, pos[a2][..., None], value, axis=-1)
                np.put_along_axis(vm, pos[a1][..., None], value, axis=-1)
            lib.upload(d.ptr, b)
            run(lib, v, dv, axis, keepdims=keepdims, values=values, kinds=KINDS if together else (("argmax",) if plan[0][0] > 0 else ("argmin",)))


def three_kinds(lib, dtype, shape, axis, seed, keepdims=False, values=True):
    for x in (continuous(shape, dtype, seed), ties(shape, dtype, seed + 1)):
        run(lib, x, lib.to_device(x), axis, keepdims=keepdims, values=values)
    planted(lib, dtype, shape, lambda b: b, axis, values=values, keepdims=keepdims)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_odd_extents_rows_and_columns(smhip, dtype):
    """O and R of 1, 3, 5, 63, 65 and 4097 through the row and column walks, with and without the split of R."""
    ext = (1, 3, 5, 63, 65, 4097)
    for i, o in enumerate(ext):
        for k, r in enumerate(ext):
            for axis in (0, 1):
                three_kinds(smhip, dtype, (o, r), axis, 100 + 10 * i + k, values=(i + k + axis) % 2 == 0)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("shape,axis", [((3, 70001), 1), ((2, 4099, 5), 1), ((70001, 3), 0), ((5, 70001), 0), ((1000, 257), 1), ((7, 1031, 9), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"axis{v}")
def test_long_and_split_rows_and_columns(smhip, dtype, shape, axis):
    three_kinds(smhip, dtype, shape, axis, 7)


SHAPES = [(4097,), (65, 63), (63, 4097), (3, 5, 4097), (4097, 3, 5), (5, 65, 3), (2, 3, 1, 65, 5), (3, 2, 5, 1, 3, 4), (2, 3, 4, 5, 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_matrix_dense_every_axis(smhip, dtype):
    for si, shape in enumerate(SHAPES):
        for axis in range(len(shape)):
            three_kinds(smhip, dtype, shape, axis, 20 * si + axis, keepdims=(si + axis) % 2 == 1, values=axis % 2 == 0)


def test_negative_and_absent_axis(smhip):
    x = ties((37, 1030), np.float32, 5)
    d = smhip.to_device(x)
    for kind in KINDS:
        assert np.array_equal(smhip.argreduce(kind, d, -1).numpy(), NP[kind](x, axis=1))
        assert np.array_equal(smhip.argreduce(kind, d, -2, keepdims=True).numpy(), NP[kind](x, axis=0)[None, :])
        vals, idx = smhip.argreduce(kind, d, values=True)  # no axis: the row-major index, shape (1,)
        assert idx.shape == (1,) and idx.numpy()[0] == NP[kind](x) and vals.numpy()[0] == x.reshape(-1)[NP[kind](x)]
        assert smhip.argreduce(kind, d, keepdims=True).shape == (1, 1)
        t = d.view_like(x.T, x)  # a view without an axis: its own row-major order
        assert smhip.argreduce(kind, t).numpy()[0] == NP[kind](x.T)
        out = smhip.empty((37,), np.int64)
        assert smhip.argreduce(kind, d, 1, out=out) is out and np.array_equal(out.numpy(), NP[kind](x, axis=1))


VIEWS = [lambda b: b.transpose(1, 0, 2), lambda b: b.transpose(2, 1, 0), lambda b: b[3:60, 5:], lambda b: b[:, 7:120:3], lambda b: b[::2, :, 1:5],
         lambda b: b[5, :, :].T, lambda b: b[:, :, 4], lambda b: b[::-1][::-1][1:, ::5, ::2]]


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views(smhip, dtype):
    shape = (70, 130, 6)
    bases = [continuous(shape, dtype, 3), ties(shape, dtype, 4)]
    devs = [smhip.to_device(b) for b in bases]
    for vi, viewf in enumerate(VIEWS):
        for base, d in zip(bases, devs):
            v = viewf(base)
            dv = d.view_like(v, base)
            for axis in range(v.ndim):
                run(smhip, v, dv, axis, values=(vi + axis) % 2 == 0)
        for axis in range(viewf(bases[0]).ndim):
            planted(smhip, dtype, shape, viewf, axis, values=(vi + axis) % 2 == 1)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_transposed_view_equals_row_walk(smhip, dtype):
    A = ties((300, 2000), dtype, 11)
    d = smhip.to_device(A)
    t = d.view_like(A.T, A)
    route, launches, ori, _ = smhip.argreduce_plan("argmax", dtype, list(t.shape), list(t.strides), 0)
    assert route & 0xff == sma.ARG_ROUTE_ROW and not route & sma.ARG_COPY and ori == (300, 2000, 1)
    for kind in KINDS:
        for a, b in (((t, 0), (d, 1)), ((t, 1), (d, 0))):
            va, ia = smhip.argreduce(kind, a[0], a[1], values=True)
            vb, ib = smhip.argreduce(kind, b[0], b[1], values=True)
            assert ia.numpy().tobytes() == ib.numpy().tobytes() and va.numpy().tobytes() == vb.numpy().tobytes()
        check(kind, A.T, 0, smhip.argreduce(kind, t, 0).numpy())


def test_split_routes(smhip):
    """(4, 2^22) f32 over axis 1 and (2^20, 4) f64 over axis 0 (two finishing launches), the three kinds of input each."""
    for dtype, shape, axis, launches in ((np.float32, (4, 1 << 22), 1, 2), (np.float64, (1 << 20, 4), 0, 3)):
        st = [shape[1], 1]
        route, n, _, _ = smhip.argreduce_plan("argmax", dtype, list(shape), st, axis)
        assert route & sma.ARG_SPLIT and n == launches
        three_kinds(smhip, dtype, shape, axis, 9)


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_argreduce_gpu import three_kinds, run, continuous, ties
lib = sma.load()
lib.set_device(0)
cases = [((3000, 5), 1), ((64, 2048), 1), ((1 << 16, 3), 1), ((40, 3000), 1), ((2, 70001), 1), ((700, 33), 0), ((9, 300, 17), 1),
         ((3000, 5, 3), 1)]
for dtype in (np.float32, np.float64, np.int32, np.int64):
    for i, (shape, axis) in enumerate(cases):
        three_kinds(lib, dtype, shape, axis, 40 + i)
    for x in (continuous((70001, 3), dtype, 50), ties((70001, 3), dtype, 51)):  # two finishing launches
        run(lib, x, lib.to_device(x), 0)
    x = continuous((50, 60, 7), dtype, 60)  # a view that is copied dense first
    d = lib.to_device(x)
    v = x.transpose(1, 0, 2)
    run(lib, v, d.view_like(v, x), 2)
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_ARGREDUCE_GRID_CAP=3: every kernel's loop over its tasks runs many times per lane, on every route."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_ARGREDUCE_GRID_CAP="3", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_nan_first_nan_wins_for_both_kinds(smhip, dtype):
    x = continuous((40, 300, 3), dtype, 5)
    x[3, 7, 1] = np.nan             # at one place
    x[11, 299, 0] = np.nan          # two places in a row (axis 1), the later one last
    x[11, 150, 0] = np.nan
    x[:, 0, 2] = np.nan             # a whole column
    d = smhip.to_device(x)
    for axis in range(3):
        run(smhip, x, d, axis)
    for shape, axis in (((3, 70001), 1), ((70001, 3), 0), ((4099, 5), 0)):  # across chunks and finishing launches
        y = continuous(shape, dtype, 6)
        ym = np.moveaxis(y, axis, -1)
        ym[0, 69000 % shape[axis]] = np.nan
        ym[1, 1025] = np.nan
        ym[1, 4000] = -np.nan
        ym[2, :] = np.nan
        run(smhip, y, smhip.to_device(y), axis)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_signed_zeros_and_infinities(smhip, dtype):
    z = np.zeros((6, 4097), dtype)
    z[0, ::2] = -0.0                # +0 first
    z[1, 1::2] = -0.0               # -0 first
    z[2, :] = -0.0
    z[2, 4096] = 0.0
    z[3, 0] = -0.0
    z[4, 1:] = -1.0                 # +0 the maximum, at position 0
    z[5, :] = 1.0
    z[5, 2000] = -0.0
    z[5, 3000] = 0.0
    for x in (z, np.ascontiguousarray(z.T)):
        d = smhip.to_device(x)
        for axis in (0, 1):
            run(smhip, x, d, axis)
    inf = np.array(np.inf, dtype)
    for R in (1, 5, 70, 4097, 70001):
        x = continuous((6, R), dtype, R)
        x[0, :] = -inf              # every element the fold's own starting value: position 0, for both kinds
        x[1, :] = inf
        x[2, R // 2] = inf
        x[2, R - 1] = inf
        x[3, R // 2] = -inf
        x[3, R - 1] = -inf
        x[4, :] = -inf
        x[4, R - 1] = inf
        x[5, :] = inf
        x[5, R - 1] = -inf
        for y in (x, np.ascontiguousarray(x.T)):
            d = smhip.to_device(y)
            for axis in (0, 1):
                run(smhip, y, d, axis)


@pytest.mark.parametrize("dtype", (np.int32, np.int64), **IDS)
def test_integer_limits(smhip, dtype):
    lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
    for R in (1, 5, 70, 4097, 70001):
        x = ties((6, R), dtype, R)
        x[0, :] = lo                # every element the fold's own starting value
        x[1, :] = hi
        x[2, R // 2] = hi
        x[2, R - 1] = hi
        x[2, 0] = lo
        x[3, R // 2] = lo
        x[3, R - 1] = lo
        x[4, :] = lo
        x[4, R - 1] = lo + 1
        x[5, :] = hi
        x[5, R - 1] = hi - 1
        for y in (x, np.ascontiguousarray(x.T)):
            d = smhip.to_device(y)
            for axis in (0, 1):
                run(smhip, y, d, axis)


def test_empty_extents(smhip):
    d = smhip.empty((4, 0, 3), np.float32)
    assert smhip.argreduce("argmax", d, 0).shape == (0, 3)  # an empty result: nothing to compute
    for kind in KINDS:
        with pytest.raises(sma.SmhipError) as e:
            smhip.argreduce(kind, d, 1)   # numpy: attempt to get argmax of an empty sequence
        assert e.value.code == sma.ERR_INVALID


def test_more_than_2_31_elements(smhip):
    """2^31 + 5 ones, 7 at 2^31 + 2 and 2^31 + 4, -7 at 2^31 + 1: the flat argmax and argmin and their values."""
    n = (1 << 31) + 5
    a = smhip.empty((n,), np.float32)
    one = np.array([1.0], np.float32)
    smhip._ck(smhip.c.smhip_fill(C.c_int(sma.F32), C.c_void_p(a.ptr), one.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
    for at, v in (((1 << 31) + 2, 7.0), ((1 << 31) + 4, 7.0), ((1 << 31) + 1, -7.0)):
        smhip.upload(a.ptr + at * 4, np.array([v], np.float32))
    vals, idx = smhip.argreduce("argmax", a, values=True)
    assert idx.numpy()[0] == (1 << 31) + 2 and vals.numpy()[0] == 7.0
    vals, idx = smhip.argreduce("argmin", a, 0, values=True)
    assert idx.numpy()[0] == (1 << 31) + 1 and vals.numpy()[0] == -7.0
