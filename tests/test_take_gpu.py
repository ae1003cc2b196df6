"""take / take_along_axis on the GPU (smhip_take_axis through the ctypes binding) against numpy, bit for bit: f32, f64, i32 and
i64, the three index modes, every route of the planner.

Every check is exact.  The reference is numpy alone: the indices are normalised on the host by the mode,
  CLIP     np.clip(i, 0, R - 1)
  WRAP     np.mod(i, R)
  CHECKED  np.clip(np.where(i < 0, i + R, i), 0, R - 1), and the flag is ((i < -R) | (i >= R)).any()
and handed to np.take_along_axis / np.take.  Results are compared as bytes, so NaN payloads and signed zeros count.  Operand
values are either `specials` (NaNs of both signs with distinct payloads, +-0, +-inf, subnormals; INT_MIN / INT_MAX) or an
arange, every element distinct, wherever a wrong address must show.  The index arrays come in kinds, because each hides a class
of bug: identity, reversed, every lane the same position, random with duplicates, only negatives, the edge values.
K (the longest staged line) and the routes are taken from the plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma
from tests.test_sort_gpu import specials

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
MODES = ("checked", "clip", "wrap")
LINE, ROWS, DIRECT, COPY = sma.TAKE_ROUTE_LINE, sma.TAKE_ROUTE_ROWS, sma.TAKE_ROUTE_DIRECT, sma.TAKE_COPY
KINDS = ("identity", "reversed", "same", "random", "negative", "edges")


def distinct(shape, dtype, start=1):
    """Every element another value (exact in f32 up to 2^24 elements)."""
    n = int(np.prod(shape))
    assert n < 1 << 24
    return (np.arange(n, dtype=np.int64) + start).reshape(shape).astype(dtype)


def indices(kind, shape, axis, R, seed=0):
    """An int64 index array of `shape`, every value valid in every mode ([-R, R) for `negative` and `edges`, else [0, R))."""
    rng = np.random.default_rng(seed)
    J = shape[axis]
    along = np.arange(J, dtype=np.int64).reshape([-1 if d == axis else 1 for d in range(len(shape))])
    if kind == "identity":
        idx = along % R
    elif kind == "reversed":
        idx = R - 1 - along % R
    elif kind == "same":
        idx = np.full(shape, (seed * 7 + 3) % R, np.int64)
    elif kind == "random":
        idx = rng.integers(0, R, size=shape)
    elif kind == "negative":
        idx = rng.integers(-R, 0, size=shape)
    else:
        idx = np.array([-R, -1, 0, R - 1], np.int64)[(along + rng.integers(0, 4, size=shape)) % 4]
    return np.ascontiguousarray(np.broadcast_to(idx, shape)).astype(np.int64)


def normalise(i, R, mode):
    if mode == "clip":
        return np.clip(i, 0, R - 1), False
    if mode == "wrap":
        return np.mod(i, R), False
    return np.clip(np.where(i < 0, i + R, i), 0, R - 1), bool(((i < -R) | (i >= R)).any())


def reference(a, idx, axis, mode):
    pos, bad = normalise(idx, a.shape[axis], mode)
    return np.ascontiguousarray(np.take_along_axis(a, pos, axis)), bad


def call_args(da, di, axis):
    """take_along_axis's arguments to the C ABI, both operands broadcast to the result."""
    shape, sa, si = [], [], []
    for d, (na, ni) in enumerate(zip(da.shape, di.shape)):
        if d == axis:
            shape.append(ni), sa.append(da.strides[d]), si.append(di.strides[d])
            continue
        n = ni if na == 1 else na
        shape.append(n), sa.append(da.strides[d] if na == n and n != 1 else 0), si.append(di.strides[d] if ni == n and n != 1 else 0)
    return sa, da.shape[axis], si, shape


def route_of(lib, da, di, axis):
    sa, R, si, shape = call_args(da, di, axis)
    return lib.take_plan(da.dtype, sa, R, si, shape, axis)[0]


def raw(lib, da, di, axis, mode):
    """The C ABI itself with a flag word that holds garbage before the call -> (result, flag)."""
    sa, R, si, shape = call_args(da, di, axis)
    out = lib.empty(shape, da.dtype)
    flag = lib.to_device(np.array([0x5A5A5A5A5A5A5A5A], np.int64))
    rc = lib.take_raw(sma.INDEX_MODES[mode], sma.DTYPES[da.dtype], da.ptr, sa, R, di.ptr, si, shape, axis, out.ptr, flag.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return out.numpy(), int(flag.numpy()[0])


def check(lib, a, da, idx, di, axis, modes=MODES, route=None):
    """`da` / `di` hold the host arrays (or views) `a` / `idx` on the device."""
    what = (a.dtype, a.shape, idx.shape, axis)
    if route is not None:
        got = route_of(lib, da, di, axis)
        assert got == route, what + (got,)
    for mode in modes:
        want, bad = reference(a, idx, axis, mode)
        got, flag = raw(lib, da, di, axis, mode)
        assert got.dtype == a.dtype and got.shape == want.shape, what
        assert got.tobytes() == want.tobytes(), what + (mode,)
        assert flag == int(bad), what + (mode, flag)
        if not bad:  # the public form
            pub = lib.take_along_axis(da, di, axis, mode=mode)
            assert pub.shape == want.shape and pub.numpy().tobytes() == want.tobytes(), what + (mode, "take_along_axis")


def budget(lib, dtype):
    return lib.take_plan(dtype, [8, 1], 8, [8, 1], [2, 8], 1)[3]


def line_case(lib, dtype, O, R, J, kind, seed, modes=MODES, route=LINE, values=None):
    a = values((O, R), dtype, seed) if values else distinct((O, R), dtype, seed)
    idx = indices(kind, (O, J), 1, R, seed)
    check(lib, a, lib.to_device(a), idx, lib.to_device(idx), 1, modes, route)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_line_lengths(smhip, dtype):
    """Every length at which the staging takes another path (a lone element, partial slots, K itself), with one index, a full
    line of them and more indices than elements; one line, a few, and enough for several lines per workgroup."""
    K = budget(smhip, dtype)
    n = 0
    for R in (1, 2, 63, 64, 65, 255, 256, 257, K - 1, K):
        for J in (1, R, 3 * R + 1):
            for O in (1, 7, 1000) if R <= 257 else (1, 7):
                want = smhip.take_plan(dtype, [R, 1], R, [J, 1], [O, J], 1)[0]
                assert want in (LINE, DIRECT) and (J < R or want == LINE)
                line_case(smhip, dtype, O, R, J, KINDS[n % len(KINDS)], n, modes=(MODES[n % 3],), route=want)
                n += 1


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_line_every_kind_and_mode(smhip, dtype):
    """O = 1000 lines of 37: several lines per workgroup with a ragged last group; and one shape beyond a workgroup's lanes."""
    for O, R, J in ((1000, 37, 37), (33, 300, 300), (5, 1000, 50)):
        for k, kind in enumerate(KINDS):
            line_case(smhip, dtype, O, R, J, kind, 10 + k, route=None)
        line_case(smhip, dtype, O, R, J, "random", 20, values=specials, route=None)
    assert smhip.take_plan(dtype, [37, 1], 37, [37, 1], [1000, 37], 1)[0] == LINE


@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_line_past_the_budget_and_misaligned(smhip, dtype):
    K = budget(smhip, dtype)
    line_case(smhip, dtype, 3, K + 1, K + 1, "random", 1, route=DIRECT)   # one element too long for LDS: DIRECT must agree
    line_case(smhip, dtype, 3, K + 1, 5, "edges", 2, route=DIRECT)
    # the line base is off a 16-byte boundary: a slice that starts one element in; an odd pitch, so every line stands differently
    for R in (37, 255, 1001):
        base = distinct((9, R + 1), dtype)
        d = smhip.to_device(base)
        for v in (base[:, 1:], base[:, :R], base[1:, 1:R]):
            idx = indices("random", (v.shape[0], v.shape[1] + 3), 1, v.shape[1], R)
            check(smhip, v, d.view_like(v, base), idx, smhip.to_device(idx), 1, route=LINE)
    # a long index line cut into chunks of picks, and many picks from a short line
    for O, R, J in ((2, 500, 70001), (1, 3, 100003)):
        line_case(smhip, dtype, O, R, J, "random", 3, modes=("wrap",), route=LINE)


def take_case(lib, a, da, ids, axis, modes=MODES, route=None):
    """np.take through the public form and through the C ABI (a 1-D index array, stride 0 on every other axis)."""
    R = a.shape[axis]
    di = lib.to_device(ids)
    for mode in modes:
        pos, bad = normalise(ids, R, mode)
        want = np.ascontiguousarray(np.take(a, pos, axis))
        shape = list(a.shape)
        shape[axis] = ids.size
        si = [0] * a.ndim
        si[axis] = 1
        if route is not None:
            assert lib.take_plan(a.dtype, list(da.strides), R, si, shape, axis)[0] == route, (a.shape, ids.size, axis)
        out = lib.empty(shape, a.dtype)
        flag = lib.to_device(np.array([-1], np.int64))
        rc = lib.take_raw(sma.INDEX_MODES[mode], sma.DTYPES[da.dtype], da.ptr, list(da.strides), R, di.ptr, si, shape, axis, out.ptr, flag.ptr)
        assert rc == 0, lib.c.smhip_last_error().decode()
        assert out.numpy().tobytes() == want.tobytes(), (a.dtype, a.shape, ids.size, axis, mode)
        assert int(flag.numpy()[0]) == int(bad)
        if not bad:
            assert lib.take(da, di, axis, mode=mode).numpy().tobytes() == want.tobytes()


def ids_of(kind, n, R, seed):
    rng = np.random.default_rng(seed)
    if kind == "sorted":
        return np.sort(rng.integers(0, R, size=n)).astype(np.int64)
    if kind == "equal":
        return np.full(n, (seed + R // 2) % R, np.int64)
    return rng.integers(-R, R, size=n).astype(np.int64)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_rows(smhip, dtype):
    """Row lengths around one vector, a wave and a piece; one row, a few, more than a launch's first round of tasks."""
    W = 16 // np.dtype(dtype).itemsize
    n = 0
    for R in (1, 5, 300):
        for I in (W, W + 1, 255, 256, 257, 1000):
            a = distinct((R, I), dtype)
            da = smhip.to_device(a)
            for count in (1, 3, 1025):
                take_case(smhip, a, da, ids_of(("sorted", "random", "equal")[n % 3], count, R, n), 0, modes=(MODES[n % 3],), route=ROWS)
                n += 1


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_rows_views_and_a_middle_axis(smhip, dtype):
    W = 16 // np.dtype(dtype).itemsize
    # the pitch, the base, or both break 16-byte alignment; then aligned rows inside a wider table (the vector path on a view)
    odd, wide = distinct((40, 8 * W + 1), dtype), distinct((40, 16 * W), dtype)
    for base, views in ((odd, (odd[:, :8 * W], odd[:, 1:], odd[3:, 1:1 + 4 * W], odd[::2, :8 * W])), (wide, (wide[:, 4 * W:12 * W], wide[::3, 8 * W:]))):
        d = smhip.to_device(base)
        for v in views:
            for kind in ("sorted", "random", "equal"):
                take_case(smhip, v, d.view_like(v, base), ids_of(kind, 77, v.shape[0], 5), 0, route=ROWS)
    # a middle axis: (3, R, I) taken along axis 1
    for R, I in ((5, 4 * W), (300, 255), (7, 1000)):
        a = specials((3, R, I), dtype, 7)
        take_case(smhip, a, smhip.to_device(a), ids_of("random", 33, R, 8), 1, route=ROWS)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_direct(smhip, dtype):
    # along axis 0 of (R, I) with a full index array
    for R, I, J in ((300, 70, 300), (5, 1000, 9), (1000, 3, 17)):
        a = distinct((R, I), dtype)
        for kind in ("random", "negative", "edges"):
            idx = indices(kind, (J, I), 0, R, 1)
            check(smhip, a, smhip.to_device(a), idx, smhip.to_device(idx), 0, route=DIRECT)
    # rows shorter than a vector
    for I in (1, 2, 3):
        a = distinct((20000, I), dtype)
        ids = ids_of("random", 1031, 20000, I)
        take_case(smhip, a, smhip.to_device(a), ids, 0, route=DIRECT if I * np.dtype(dtype).itemsize < 16 else ROWS)
    # rank 6 with the axis in each position
    shape = (2, 3, 2, 3, 2, 3)
    a = distinct(shape, dtype)
    da = smhip.to_device(a)
    for axis in range(6):
        ishape = list(shape)
        ishape[axis] = 5
        for kind in ("random", "edges"):
            idx = indices(kind, ishape, axis, shape[axis], axis)
            check(smhip, a, da, idx, smhip.to_device(idx), axis, route=LINE if axis == 5 else DIRECT)
    # the index array broadcast along the outer axes only
    a = distinct((6, 50, 7), dtype)
    idx = indices("random", (1, 9, 7), 1, 50, 4)
    check(smhip, a, smhip.to_device(a), idx, smhip.to_device(idx), 1, route=DIRECT)
    a = distinct((4, 6, 300), dtype)
    idx = indices("random", (1, 1, 300), 2, 300, 5)
    check(smhip, a, smhip.to_device(a), idx, smhip.to_device(idx), 2, route=LINE)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views(smhip, dtype):
    base = distinct((60, 130), dtype)
    d = smhip.to_device(base)
    ibase = indices("random", (130, 130), 0, 60, 1)   # values in [0, 60): valid for every view below that has 60 or more along its axis
    di = smhip.to_device(ibase)
    small = np.ascontiguousarray(ibase % 30)
    ds = smhip.to_device(small)
    t = base.T                                                        # (130, 60): read in place
    check(smhip, t, d.view_like(t, base), ibase[:, :60], di.view_like(ibase[:, :60], ibase), 1)
    assert route_of(smhip, d.view_like(t, base), smhip.empty((300, 60), np.int64), 0) & COPY == 0
    check(smhip, t, d.view_like(t, base), ibase[:60, :].T, di.view_like(ibase[:60, :].T, ibase), 0, route=LINE)   # both transposed
    stepped = base[::2, 1::3]                                         # (30, 43): a two-axis walk, still in place
    check(smhip, stepped, d.view_like(stepped, base), small[:30, :43], ds.view_like(small[:30, :43], small), 0, route=DIRECT)
    check(smhip, stepped, d.view_like(stepped, base), small[:30, 5:100:2][:, :40], ds.view_like(small[:30, 5:100:2][:, :40], small), 1)
    cube = distinct((6, 10, 40), dtype)
    dc = smhip.to_device(cube)
    v = cube[::2, ::3, ::2]                                           # (3, 4, 20): the kept axes do not merge -> staged
    idx = indices("random", (3, 4, 33), 2, 20, 2)
    check(smhip, v, dc.view_like(v, cube), idx, smhip.to_device(idx), 2, route=LINE | COPY)
    iv = np.ascontiguousarray(idx.transpose(1, 0, 2)).transpose(1, 0, 2)  # idx transposed among the kept axes -> idx staged
    dense_v = np.ascontiguousarray(v)
    dib = smhip.to_device(np.ascontiguousarray(iv.transpose(1, 0, 2)))
    div = sma.DeviceArray(smhip, dib.base_ptr, np.int64, iv.shape, [s // 8 for s in iv.strides], 0, dib._owner)
    check(smhip, dense_v, smhip.to_device(dense_v), iv, div, 2, route=LINE | COPY)
    check(smhip, v, dc.view_like(v, cube), iv, div, 2, route=LINE | COPY)                  # both at once
    # a stride-0 axis of a: a row broadcast over 9 lines, and a column broadcast along the gathered axis
    row = distinct((130,), dtype)
    dr = smhip.to_device(row)
    b = np.broadcast_to(row[None, :], (9, 130))
    idx = indices("random", (9, 40), 1, 130, 3)
    check(smhip, b, dr.view_like(b, row), idx, smhip.to_device(idx), 1)
    col = np.broadcast_to(row[:9, None], (9, 50))
    check(smhip, col, dr.view_like(col, row), idx % 50, smhip.to_device(idx % 50), 1)
    idx = indices("random", (5, 130), 0, 9, 4)
    check(smhip, b, dr.view_like(b, row), idx, smhip.to_device(idx), 0)


def bad_indices(R, shape, seed):
    """Valid positions with the troublemakers scattered among them."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(-R, R, size=shape).astype(np.int64)
    flat = idx.reshape(-1)
    trouble = np.array([R, -R - 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 32, (1 << 32) + 1, -(1 << 32), R + (1 << 32), (1 << 63) - R], np.int64)
    at = rng.permutation(flat.size)[: max(trouble.size, flat.size // 7)]
    flat[at] = trouble[np.arange(at.size) % trouble.size]
    return idx


def guarded(lib, shape, dtype, sentinel):
    """`a` as the middle third of a device buffer whose other elements are `sentinel` (a value `a` does not hold)."""
    n = int(np.prod(shape))
    big = np.full(3 * n, sentinel, dtype)
    big[n:2 * n] = distinct((n,), dtype)
    a = big[n:2 * n].reshape(shape)
    d = lib.to_device(big)
    return a, d.view_like(a, big), d


def bad_index_cases(lib, mode):
    sentinel = -77
    for dtype in (np.float32, np.int64):
        K = budget(lib, dtype)
        cases = [((7, 300), (7, 300), 1, LINE), ((2, K), (2, K + 5), 1, LINE), ((300, 64), (50, 64), 0, DIRECT), ((3, K + 1), (3, 900), 1, DIRECT)]
        for shape, ishape, axis, route in cases:
            a, da, keep = guarded(lib, shape, dtype, sentinel)
            idx = bad_indices(shape[axis], ishape, 5)
            want, bad = reference(a, idx, axis, mode)
            assert bad == (mode == "checked")
            di = lib.to_device(idx)
            assert route_of(lib, da, di, axis) == route
            got, flag = raw(lib, da, di, axis, mode)
            assert not (got == dtype(sentinel)).any(), (dtype, shape, mode)       # nothing was read outside a
            assert got.tobytes() == want.tobytes() and flag == int(bad), (dtype, shape, mode)
        # ROWS through np.take
        a, da, keep = guarded(lib, (50, 64), dtype, sentinel)
        take_case(lib, a, da, bad_indices(50, (333,), 6), 0, modes=(mode,), route=ROWS)
        # numpy's own np.take(mode=...) directly.  Its wrap mode adds or subtracts R in a loop, so it is asked only about
        # indices up to 2^32 + 1; INT64_MIN and INT64_MAX are covered by the normalised reference above
        one = distinct((9,), dtype)
        d1 = lib.to_device(one)
        for i in (9, -10, 1 << 32, (1 << 32) + 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max):
            ids = np.array([0, i, 8], np.int64)
            di = lib.to_device(ids)
            if mode == "checked":
                with pytest.raises(IndexError):
                    lib.take(d1, di, 0, mode=mode)
                with pytest.raises(IndexError):
                    lib.take_along_axis(d1, di, 0)   # the default mode
            else:
                got = lib.take(d1, di, 0, mode=mode).numpy()
                assert np.array_equal(got, np.take(one, normalise(ids, 9, mode)[0], 0))
                if abs(i) <= (1 << 32) + 1:
                    assert np.array_equal(got, np.take(one, ids, 0, mode=mode))


def test_bad_indices_clip(smhip):
    bad_index_cases(smhip, "clip")


def test_bad_indices_wrap(smhip):
    bad_index_cases(smhip, "wrap")


def test_bad_indices_checked(smhip):
    """The clamped element is written and the flag is set; an all-valid call clears a flag word that held garbage (check() does
    that for every valid case of this file as well)."""
    bad_index_cases(smhip, "checked")
    a = distinct((5, 40), np.float32)
    idx = indices("edges", (5, 40), 1, 40, 1)
    got, flag = raw(smhip, smhip.to_device(a), smhip.to_device(idx), 1, "checked")
    assert flag == 0 and got.tobytes() == reference(a, idx, 1, "checked")[0].tobytes()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_every_dtype_on_every_route(smhip, dtype):
    W = 16 // np.dtype(dtype).itemsize
    a = specials((33, 300), dtype, 1)
    da = smhip.to_device(a)
    for kind in KINDS:
        idx = indices(kind, (33, 301), 1, 300, 2)
        check(smhip, a, da, idx, smhip.to_device(idx), 1, route=LINE)
        idx = indices(kind, (41, 300), 0, 33, 3)
        check(smhip, a, da, idx, smhip.to_device(idx), 0, route=DIRECT)
    for kind in ("sorted", "random", "equal"):
        take_case(smhip, a, da, ids_of(kind, 100, 33, 4), 0, route=ROWS)
        take_case(smhip, a, da, ids_of(kind, 301, 300, 4), 1, route=LINE)
    t = a.T
    take_case(smhip, t, da.view_like(t, a), ids_of("random", 100, 300, 5), 0)


def test_flattened_nd_index_and_out_arguments(smhip):
    a = specials((37, 130), np.float32, 8)
    d = smhip.to_device(a)
    ids = indices("random", (50,), 0, a.size, 1)
    di = smhip.to_device(ids)
    assert smhip.take(d, di, None).numpy().tobytes() == np.take(a, ids).tobytes()
    t = d.view_like(a.T, a)   # a view without an axis: its own row-major order
    assert smhip.take(t, di, None).numpy().tobytes() == np.take(a.T, ids).tobytes()
    idx2 = indices("random", (37, 130), 1, a.size, 2)
    got = smhip.take_along_axis(d, smhip.to_device(idx2), None)
    assert got.shape == (a.size,) and got.numpy().tobytes() == np.take_along_axis(a.reshape(-1), idx2.reshape(-1), 0).tobytes()
    nd = indices("random", (4, 5), 0, 130, 3)   # an N-D index array: flattened, the result reshaped
    got = smhip.take(d, smhip.to_device(nd), 1, mode="clip")
    assert got.shape == (37, 4, 5) and got.numpy().tobytes() == np.take(a, nd, 1).tobytes()
    out = smhip.empty((37, 50), np.float32)
    ids = indices("random", (50,), 0, 130, 4)
    di = smhip.to_device(ids)
    assert smhip.take(d, di, 1, out=out) is out and out.numpy().tobytes() == np.take(a, ids, 1).tobytes()
    # out aliasing an operand is refused, by the binding and by the library
    idx = indices("random", (37, 130), 1, 130, 5)
    dx = smhip.to_device(idx)
    for o in (d, dx):
        with pytest.raises(ValueError):
            smhip.take_along_axis(d, dx, 1, out=o)
    sa, R, si, shape = call_args(d, dx, 1)
    assert smhip.take_raw(sma.INDEX_CLIP, sma.F32, d.ptr, sa, R, dx.ptr, si, shape, 1, d.ptr) == sma.ERR_INVALID
    assert smhip.take_raw(sma.INDEX_CLIP, sma.F32, d.ptr, sa, R, dx.ptr, si, shape, 1, dx.ptr) == sma.ERR_INVALID
    assert smhip.take_raw(sma.INDEX_CLIP, sma.F32, d.ptr, sa, R, dx.ptr, si, shape, 1, out.ptr, out.ptr) == sma.ERR_INVALID


def test_empty_results(smhip):
    a = smhip.to_device(distinct((4, 5), np.float32))
    for mode in MODES:
        assert smhip.take(a, smhip.empty((0,), np.int64), 1, mode=mode).shape == (4, 0)
        assert smhip.take_along_axis(a, smhip.empty((4, 0), np.int64), 1, mode=mode).shape == (4, 0)
        e = smhip.empty((0, 5), np.float32)
        assert smhip.take(e, smhip.to_device(np.array([0, 1], np.int64)), 1, mode=mode).shape == (0, 2)
        assert smhip.take(e, smhip.empty((0,), np.int64), 0, mode=mode).shape == (0, 5)
        with pytest.raises(IndexError):   # numpy raises as well: nothing to take from, and a result to fill
            smhip.take(e, smhip.to_device(np.array([0], np.int64)), 0, mode=mode)


def test_round_trips_with_argsort_and_argmax(smhip):
    for dtype in DTYPES:
        x = specials((33, 300), dtype, 9)
        d = smhip.to_device(x)
        for axis in (0, 1):
            for descending in (False, True):
                vals, order = smhip.sort(d, axis, descending, indices=True)
                assert smhip.take_along_axis(d, order, axis, mode="clip").numpy().tobytes() == vals.numpy().tobytes()
                assert smhip.take_along_axis(d, smhip.argsort(d, axis, descending), axis).numpy().tobytes() == vals.numpy().tobytes()
            best, where = smhip.argreduce("argmax", d, axis, keepdims=True, values=True)   # max_with_index
            assert smhip.take_along_axis(d, where, axis).numpy().tobytes() == best.numpy().tobytes()
        # the five best of each row: a sliced view of the ranking as the index operand
        ranked = smhip.argsort(d, 1, True)
        host = ranked.numpy()
        top = sma.DeviceArray(smhip, ranked.base_ptr, np.int64, (33, 5), ranked.strides, ranked.offset, ranked._owner)
        assert smhip.take_along_axis(d, top, 1).numpy().tobytes() == np.take_along_axis(x, host[:, :5], 1).tobytes()


def test_same_bits_on_every_run(smhip):
    a = specials((300, 257), np.float32, 15)
    d = smhip.to_device(a)
    idx = smhip.to_device(indices("random", (300, 257), 1, 257, 1))
    ids = smhip.to_device(ids_of("random", 5000, 300, 2))
    runs = [(smhip.take_along_axis(d, idx, 1).numpy().tobytes(), smhip.take(d, ids, 0, mode="wrap").numpy().tobytes()) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_take_gpu import check, take_case, distinct, indices, ids_of, specials, LINE, ROWS, DIRECT, COPY
lib = sma.load()
lib.set_device(0)
for dtype in (np.float32, np.float64, np.int32, np.int64):
    a = specials((333, 70), dtype, 1)
    da = lib.to_device(a)
    for kind in ("random", "edges"):
        idx = indices(kind, (333, 141), 1, 70, 2)
        check(lib, a, da, idx, lib.to_device(idx), 1, route=LINE)
        idx = indices(kind, (100, 70), 0, 333, 3)
        check(lib, a, da, idx, lib.to_device(idx), 0, route=DIRECT)
    take_case(lib, a, da, ids_of("random", 1025, 333, 4), 0, route=ROWS)
    b = distinct((2, 300), dtype)
    idx = indices("random", (2, 70001), 1, 300, 5)
    check(lib, b, lib.to_device(b), idx, lib.to_device(idx), 1, modes=("wrap",), route=LINE)
    cube = distinct((6, 10, 40), dtype)
    v = cube[::2, ::3, ::2]
    idx = indices("random", (3, 4, 33), 2, 20, 6)
    check(lib, v, lib.to_device(cube).view_like(v, cube), idx, lib.to_device(idx), 2, route=LINE | COPY)
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_TAKE_GRID_CAP=2: every kernel's loop over its tasks runs many times per workgroup, on LINE, ROWS, DIRECT and COPY."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_TAKE_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
