"""sort / argsort along an axis on the GPU (smhip_sort_axis through the ctypes binding) against numpy, bit for bit: f32, f64, i32
and i64, both orders, values and positions together, each alone and in place.

Every check is exact.  ASCENDING is np.argsort(x, axis, kind="stable"); DESCENDING is R - 1 - np.argsort(np.flip(x, axis), axis,
kind="stable") flipped along the axis (NaNs first, larger values first, ties in rising position -- valid for INT_MIN too); the
values' bytes are those of np.take_along_axis(x, positions).  Inputs come in kinds, because one kind hides a class of bug:
  continuous   random distinct values, the full integer range (a network that mis-sorts)
  ties         integers in [-3, 3]: hundreds of ties per line (stability lost between lanes, tiles and merge slices)
  specials     NaNs of both signs with distinct payloads, +-0 interleaved, +-inf, subnormals; INT_MIN / INT_MAX (the bits returned
               must be the operand's)
  shaped       sorted, reversed, constant, a sawtooth of period K, two values changing exactly at a tile boundary (the degenerate
               diagonals of the merge path)
K, the tile length, is taken from the plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
MODES = ("both", "values", "indices", "inplace")


def tile(lib, dtype):
    return lib.sort_plan(dtype, [1 << 20], [1], 0)[3]


def continuous(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 10.0).astype(dtype)


def ties(shape, dtype, seed):
    return np.random.default_rng(seed).integers(-3, 3, size=shape, endpoint=True).astype(dtype)


def specials(shape, dtype, seed):
    """ties with a fifth of the places taken by the special values of the type, every NaN with a payload of its own"""
    rng = np.random.default_rng(seed)
    x = ties(shape, dtype, seed)
    flat = x.reshape(-1)
    at = rng.permutation(flat.size)[: flat.size // 5]
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        flat[at] = rng.choice(np.array([info.min, info.max, info.min + 1, info.max - 1, 0], dtype), size=at.size)
        return x
    u = np.uint32 if dtype == np.float32 else np.uint64
    mant, sign = (23, 31) if dtype == np.float32 else (52, 63)
    exp_all = ((1 << (sign - mant)) - 1) << mant
    bits = flat.view(u)
    kind = rng.integers(0, 8, size=at.size)
    k = np.arange(at.size, dtype=np.uint64)
    payload = (k % ((1 << mant) - 1) + 1).astype(u)                         # 1 .. 2^mant - 1: quiet and signalling NaNs alike
    pick = [u(exp_all) | payload, u(exp_all) | payload | u(1 << sign),     # +NaN, -NaN
            np.full(at.size, 0, u), np.full(at.size, 1 << sign, u),        # +0, -0
            np.full(at.size, exp_all, u), np.full(at.size, exp_all | (1 << sign), u),  # +inf, -inf
            payload, payload | u(1 << sign)]                              # subnormals of both signs
    bits[at] = np.choose(kind, pick)
    return x


def reference(x, axis, descending):
    if descending:
        idx = np.flip(x.shape[axis] - 1 - np.argsort(np.flip(x, axis), axis, kind="stable"), axis)
    else:
        idx = np.argsort(x, axis, kind="stable")
    return np.take_along_axis(x, idx, axis), idx.astype(np.int64)


def check(lib, x, d, axis, mode="both", orders=(False, True)):
    """`d` holds `x` (a host array or view) on the device; `inplace` sorts a dense copy of it."""
    for descending in orders:
        want_v, want_i = reference(x, axis, descending)
        got_v = got_i = None
        if mode == "both":
            got_v, got_i = lib.sort(d, axis, descending, indices=True)
        elif mode == "values":
            got_v = lib.sort(d, axis, descending)
        elif mode == "indices":
            got_i = lib.argsort(d, axis, descending)
        else:
            c = lib.to_device(np.ascontiguousarray(x))
            got_v = lib.sort(c, axis, descending, out=c)
            assert got_v is c
        what = (x.dtype, x.shape, axis, descending, mode)
        if got_i is not None:
            got_i = got_i.numpy()
            assert got_i.dtype == np.int64 and got_i.shape == x.shape and np.array_equal(got_i, want_i), what
        if got_v is not None:
            got_v = got_v.numpy()
            assert got_v.dtype == x.dtype and got_v.shape == x.shape
            assert got_v.tobytes() == np.ascontiguousarray(want_v).tobytes(), what


def lengths(K):
    return (1, 2, 3, 63, 64, 65, 255, 256, 257, K - 1, K, K + 1, 2 * K, 2 * K + 1, 3 * K - 1, 5 * K + 17)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_row_lengths(smhip, dtype):
    """Every length at which the code takes another path: network sizes, the tile, two tiles, an odd run, six tiles in three passes."""
    K = tile(smhip, dtype)
    for n, R in enumerate(lengths(K)):
        route, launches, _, chunk = smhip.sort_plan(dtype, [5, R], [R, 1], 1)
        assert bool(route & sma.SORT_MERGE) == (R > K) and chunk == min(R, K)
        for k, x in enumerate((continuous((5, R), dtype, 100 + n), ties((5, R), dtype, 200 + n), specials((5, R), dtype, 300 + n))):
            check(smhip, x, smhip.to_device(x), 1, MODES[(n + k) % 4])


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_every_mode_on_a_row_and_a_merge_shape(smhip, dtype):
    K = tile(smhip, dtype)
    for shape in ((33, 300), (3, 2 * K + 1)):
        x = specials(shape, dtype, 5)
        d = smhip.to_device(x)
        for mode in MODES:
            check(smhip, x, d, 1, mode)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_shaped_lines(smhip, dtype):
    K = tile(smhip, dtype)
    for R in (K, 3 * K - 1, 5 * K + 17):
        r = np.arange(R)
        rows = [r, r[::-1], np.full(R, 7), r % K, (r >= K).astype(int), (r >= 2 * K).astype(int), -(r >= K).astype(int), (r // 3) % 5, -(r % K)]
        x = np.stack(rows).astype(dtype)
        check(smhip, x, smhip.to_device(x), 1)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_many_short_rows(smhip, dtype):
    """The packing of several lines into a workgroup meets its tail."""
    for shape in ((4097, 37), (1031, 300), (517, 2), (2049, 3)):
        x = ties(shape, dtype, 11)
        check(smhip, x, smhip.to_device(x), 1, "both", orders=(dtype in (np.float32, np.int64),))
        x = continuous(shape, dtype, 12)
        check(smhip, x, smhip.to_device(x), 1, "inplace", orders=(dtype in (np.float64, np.int32),))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_every_axis_of_small_arrays(smhip, dtype):
    for si, shape in enumerate(((7,), (5, 9), (4, 1, 6), (3, 4, 5), (2, 3, 1, 5, 4), (3, 4, 5, 2, 3, 2))):
        for x in (ties(shape, dtype, 20 + si), specials(shape, dtype, 30 + si)):
            d = smhip.to_device(x)
            for axis in range(len(shape)):
                check(smhip, x, d, axis, MODES[(si + axis) % 4])
            check(smhip, x, d, -1, "both", orders=(True,))
            check(smhip, x, d, -len(shape), "indices", orders=(False,))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views(smhip, dtype):
    K = tile(smhip, dtype)
    base = ties((70, 130), dtype, 3)
    d = smhip.to_device(base)
    for viewf in (lambda b: b.T, lambda b: b[::2, 1::3], lambda b: b[3:60, 5:100], lambda b: b[:, 7]):
        v = viewf(base)
        dv = d.view_like(v, base)
        for axis in range(v.ndim):
            check(smhip, v, dv, axis, MODES[axis % 3])
    # the transposed view along the axis with the unit stride in memory is read in place, its results scattered
    t = d.view_like(base.T, base)
    route, launches, ori, _ = smhip.sort_plan(dtype, list(t.shape), list(t.strides), 0)
    assert route & sma.SORT_COPY and launches == 3 and ori == (70, 130, 1)
    # ... with a merge inside
    long = specials((3, 2 * K + 5), dtype, 4)
    dl = smhip.to_device(long)
    check(smhip, long.T, dl.view_like(long.T, long), 0)
    check(smhip, long[:, ::2], dl.view_like(long[:, ::2], long), 1)
    tall = np.ascontiguousarray(long.T)
    check(smhip, tall, smhip.to_device(tall), 0)
    # in place along an axis that is not the last one: staged, sorted, scattered back over the operand
    check(smhip, base, d, 0, "inplace")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_broadcast_views(smhip, dtype):
    col = specials((9,), dtype, 6)
    dc = smhip.to_device(col)
    for R in (5, 300):
        v = np.broadcast_to(col[:, None], (9, R))  # stride 0 along the sort axis: every line constant
        dv = dc.view_like(v, col)
        for descending in (False, True):
            vals, idx = smhip.sort(dv, 1, descending, indices=True)
            assert np.array_equal(idx.numpy(), np.broadcast_to(np.arange(R), (9, R)))
            assert vals.numpy().tobytes() == np.ascontiguousarray(v).tobytes()
        check(smhip, v, dv, 0)
    row = np.broadcast_to(col[None, :], (4, 9))  # stride 0 along a kept axis
    dr = dc.view_like(row, col)
    check(smhip, row, dr, 1)
    check(smhip, row, dr, 0)


def test_flattened_and_out_arguments(smhip):
    x = specials((37, 130), np.float32, 8)
    d = smhip.to_device(x)
    for descending in (False, True):
        want_v, want_i = reference(x.reshape(-1), 0, descending)
        vals, idx = smhip.sort(d, None, descending, indices=True)
        assert vals.shape == idx.shape == (x.size,)
        assert vals.numpy().tobytes() == want_v.tobytes() and np.array_equal(idx.numpy(), want_i)
        t = d.view_like(x.T, x)  # a view without an axis: its own row-major order
        want_v, want_i = reference(np.ascontiguousarray(x.T).reshape(-1), 0, descending)
        assert np.array_equal(smhip.argsort(t, None, descending).numpy(), want_i)
        assert smhip.sort(t, None, descending).numpy().tobytes() == want_v.tobytes()
    out_v, out_i = smhip.empty(x.shape, np.float32), smhip.empty(x.shape, np.int64)
    assert smhip.sort(d, 0, out=out_v) is out_v and smhip.argsort(d, 0, out=out_i) is out_i
    want_v, want_i = reference(x, 0, False)
    assert out_v.numpy().tobytes() == want_v.tobytes() and np.array_equal(out_i.numpy(), want_i)
    one = smhip.to_device(x[:, :1].copy())  # an axis of one element: the values copied, zeros
    vals, idx = smhip.sort(one, 1, indices=True)
    assert vals.numpy().tobytes() == x[:, :1].tobytes() and not idx.numpy().any()
    e = smhip.empty((4, 0, 3), np.float32)
    for axis in range(3):
        assert smhip.sort(e, axis).shape == (4, 0, 3) and smhip.argsort(e, axis).shape == (4, 0, 3)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_descending_starts_where_argmax_points(smhip, dtype):
    K = tile(smhip, dtype)
    for shape in ((40, 300), (300, 40), (3, 2 * K + 1)):
        for x in (ties(shape, dtype, 13), specials(shape, dtype, 14)):
            d = smhip.to_device(x)
            for axis in (0, 1):
                first = np.take(smhip.argsort(d, axis, descending=True).numpy(), 0, axis=axis)
                assert np.array_equal(first, smhip.argreduce("argmax", d, axis).numpy())
                first = np.take(smhip.argsort(d, axis).numpy(), 0, axis=axis)
                if not np.issubdtype(dtype, np.floating) or not np.isnan(x).any():  # ascending puts the NaNs last, argmin finds them first
                    assert np.array_equal(first, smhip.argreduce("argmin", d, axis).numpy())


def test_same_bits_on_every_run(smhip):
    x = specials((3, 20000), np.float32, 15)
    d = smhip.to_device(x)
    runs = [tuple(r.numpy().tobytes() for r in smhip.sort(d, 1, True, indices=True)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_sort_gpu import check, ties, specials, continuous, tile, MODES
lib = sma.load()
lib.set_device(0)
for dtype in (np.float32, np.float64, np.int32, np.int64):
    K = tile(lib, dtype)
    cases = [((300, 70), 1), ((1031, 5), 1), ((9, K), 1), ((3, 2 * K + 1), 1), ((2, 5 * K + 17), 1), ((70, 50), 0), ((2 * K + 3, 3), 0)]
    for i, (shape, axis) in enumerate(cases):
        for x in (ties(shape, dtype, 40 + i), specials(shape, dtype, 50 + i)):
            check(lib, x, lib.to_device(x), axis, MODES[i % 4])
    x = continuous((50, 60), dtype, 60)
    check(lib, x.T, lib.to_device(x).view_like(x.T, x), 0)
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_SORT_GRID_CAP=2: every kernel's loop over its tasks runs many times per workgroup, on the ROW, MERGE and COPY routes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_SORT_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
