"""put_along_axis / put / scatter_add / index_add on the GPU (smhip_scatter_axis through the ctypes binding) against numpy, bit for
bit: f32, f64, i32 and i64, the three index modes, the four routes of the planner.

The reference is numpy alone.  Indices are normalised on the host by the mode (`normalise`), then
  PUT  one j-slice at a time through np.put_along_axis (no duplicates inside a slice, so numpy's unspecified order is not leaned on);
  ADD  np.add.at on an fp64 accumulator (f32) or the type itself, over the full index tuple of the kept entries in C order, and the
       destinations no entry names keep their bits.
PUT is compared as bytes; ADD as bytes wherever the expected element is not NaN and NaN-for-NaN elsewhere.  Every call goes through
the C ABI with the target as the MIDDLE THIRD of a buffer of sentinels -- the outer thirds must come back byte-identical -- and with a
flag word that holds garbage before the call.  The routes are taken from the plan."""
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
PUT, ADD = sma.SCATTER_PUT, sma.SCATTER_ADD
DIRECT, ROWS, SORTED, SORTED_ROWS, COPY = (sma.SCATTER_ROUTE_DIRECT, sma.SCATTER_ROUTE_ROWS, sma.SCATTER_ROUTE_SORTED, sma.SCATTER_ROUTE_SORTED_ROWS,
                                           sma.SCATTER_COPY)
KINDS = ("identity", "reversed", "same", "random", "negative", "edges", "heavy")
GARBAGE = 0x5A5A5A5A5A5A5A5A


def distinct(shape, dtype, start=1):
    """Every element another value (exact in f32 up to 2^24 elements)."""
    n = int(np.prod(shape))
    assert n < 1 << 24
    return (np.arange(n, dtype=np.int64) + start).reshape(shape).astype(dtype)


def general(shape, dtype, seed):
    """Random values whose sums round: exactness must not depend on friendly inputs."""
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, size=shape, dtype=dtype, endpoint=True)
    return (1e3 * rng.standard_normal(shape)).astype(dtype)


def indices(kind, shape, axis, R, seed=0):
    """An int64 index array of `shape`, every value in [-R, R)."""
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
    elif kind == "edges":
        idx = np.array([-R, -1, 0, R - 1], np.int64)[(along + rng.integers(0, 4, size=shape)) % 4]
    else:  # heavy: 90 % of the entries hit 3 positions
        hot = rng.integers(0, R, size=3)
        idx = np.where(rng.random(shape) < 0.9, hot[rng.integers(0, 3, size=shape)], rng.integers(0, R, size=shape))
    return np.ascontiguousarray(np.broadcast_to(idx, shape)).astype(np.int64)


def permutations(shape, axis, seed):
    """A permutation of range(shape[axis]) along every line."""
    return np.argsort(np.random.default_rng(seed).random(shape), axis=axis, kind="stable").astype(np.int64)


def trouble_indices(shape, R, seed):
    """Valid positions with the troublemakers scattered among them."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(-R, R, size=shape).astype(np.int64)
    flat = idx.reshape(-1)
    trouble = np.array([R, -R - 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 32, (1 << 32) + 1, -(1 << 32), R + (1 << 32), (1 << 63) - R], np.int64)
    at = rng.permutation(flat.size)[: max(trouble.size, flat.size // 7)]
    flat[at] = trouble[np.arange(at.size) % trouble.size]
    return idx


def normalise(i, R, mode):  # -> positions, keep-mask
    if mode == "clip":
        return np.clip(i, 0, R - 1), np.ones(i.shape, bool)
    if mode == "wrap":
        return np.mod(i, R), np.ones(i.shape, bool)
    ok = (i >= -R) & (i < R)
    return np.where(ok, np.where(i < 0, i + R, i), 0), ok


def walk_of(a, idx, axis):
    walk = list(a.shape)
    walk[axis] = idx.shape[axis]
    return walk


def reference(kind, a, idx, values, axis, mode):
    """-> (the expected target, was any entry bad).  idx has a's rank (other axes a's or 1); values broadcast to the walk shape."""
    walk = walk_of(a, idx, axis)
    pos, ok = normalise(np.broadcast_to(idx, walk), a.shape[axis], mode)
    v = np.broadcast_to(values, walk)
    if kind == PUT:
        want = a.copy()
        for j in range(walk[axis]):
            sl = tuple(slice(j, j + 1) if d == axis else slice(None) for d in range(a.ndim))
            cur = np.take_along_axis(want, pos[sl], axis)
            np.put_along_axis(want, pos[sl], np.where(ok[sl], v[sl], cur), axis)
        return want, bool((~ok).any())
    grids = np.indices(walk, sparse=False)
    at = tuple((pos if d == axis else grids[d])[ok] for d in range(a.ndim))
    with np.errstate(all="ignore"):
        acc = a.astype(np.float64 if a.dtype == np.float32 else a.dtype)
        np.add.at(acc, at, v[ok].astype(acc.dtype))
        touched = np.zeros(a.shape, bool)
        touched[at] = True
        want = np.where(touched, acc.astype(a.dtype), a)
    return want, bool((~ok).any())


def same(kind, got, want):
    if kind == PUT or not np.issubdtype(want.dtype, np.floating):
        return got.tobytes() == want.tobytes()
    nan = np.isnan(want)
    u = np.uint32 if want.dtype == np.float32 else np.uint64
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))


def strides_against(walk, host, dev):
    """The strides of `dev` (holding `host`, right-aligned against the walk shape), 0 where it broadcasts."""
    lead = len(walk) - host.ndim
    return [0] * lead + [dev.strides[d] if host.shape[d] == walk[lead + d] and walk[lead + d] != 1 else 0 for d in range(host.ndim)]


def sentinel_of(dtype):
    return np.array([-77777], np.int64).astype(dtype)[0]


def raw(lib, kind, a, idx, di, values, dv, axis, mode, unique, misalign=0):
    """The C ABI itself, the target as the middle third of a guarded buffer -> (the target after the call, flag)."""
    walk = walk_of(a, idx, axis)
    n = a.size
    third = (n + 3) // 4 * 4 + misalign  # a whole number of 16-byte vectors, unless misaligned on purpose
    host = np.full(3 * third, sentinel_of(a.dtype), a.dtype)
    host[third:third + n] = a.reshape(-1)
    buf = lib.to_device(host)
    flag = lib.to_device(np.array([GARBAGE], np.int64))
    rc = lib.scatter_raw(kind, sma.INDEX_MODES[mode], sma.SCATTER_UNIQUE if unique else 0, sma.DTYPES[a.dtype], buf.ptr + third * a.itemsize, a.shape, axis,
                         di.ptr, strides_against(walk, idx, di), dv.ptr, strides_against(walk, values, dv), walk[axis], flag.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    back = buf.numpy()
    assert back[:third].tobytes() == host[:third].tobytes() and back[third + n:].tobytes() == host[third + n:].tobytes(), "a write outside the target"
    return back[third:third + n].reshape(a.shape), int(flag.numpy()[0])


def route_of(lib, a, idx, di, values, dv, axis, unique):
    walk = walk_of(a, idx, axis)
    return lib.scatter_plan(a.dtype, a.shape, axis, strides_against(walk, idx, di), strides_against(walk, values, dv), walk[axis], unique=unique)[0]


def check(lib, kind, a, idx, values, axis, modes=MODES, unique=False, route=None, di=None, dv=None, misalign=0, public=True):
    """idx / values are host arrays; di / dv the device arrays (or views) that hold them, uploaded here when not given."""
    di = lib.to_device(idx) if di is None else di
    dv = lib.to_device(values) if dv is None else dv
    what = (kind, a.dtype, a.shape, idx.shape, values.shape, axis, unique)
    if route is not None:
        got = route_of(lib, a, idx, di, values, dv, axis, unique)
        assert got == route, what + (got,)
    for mode in modes:
        want, bad = reference(kind, a, idx, values, axis, mode)
        got, flag = raw(lib, kind, a, idx, di, values, dv, axis, mode, unique, misalign)
        assert same(kind, got, want), what + (mode,)
        assert flag == int(bad), what + (mode, flag)
        if public and idx.ndim == a.ndim:
            da = lib.to_device(a)
            fn = lib.put_along_axis if kind == PUT else lib.scatter_add
            if bad:
                with pytest.raises(IndexError):
                    fn(da, di, dv, axis, mode=mode, unique=unique)
            else:
                assert fn(da, di, dv, axis, mode=mode, unique=unique) is da
            assert same(kind, da.numpy(), want), what + (mode, "public")


def operand(n, shape, dtype, seed):
    return (specials, distinct, general)[n % 3](shape, dtype, seed)


# ---------------------------------------------------------------------------------------------- lines along the last axis
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_line_lengths(smhip, dtype):
    """Every length at which the sort takes another path (a lone element, the tile and one past it: its merge route), with one
    entry, a full line and more entries than positions; one line, a few, and many."""
    n = 0
    for R in (1, 2, 63, 64, 65, 257, 4096, 4097):
        for J in (1, R, 3 * R + 1):
            for O in (1, 7, 1000) if R <= 257 else (1, 3):
                kind = (PUT, ADD)[n % 2]
                a = operand(n, (O, R), dtype, n)
                v = operand(n + 1, (O, J), dtype, n + 100)
                idx = indices(KINDS[n % len(KINDS)], (O, J), 1, R, n)
                check(smhip, kind, a, idx, v, 1, modes=(MODES[n % 3],), route=DIRECT if J <= 1 else SORTED, public=n % 5 == 0)
                n += 1


# ---------------------------------------------------------------------------------------------- unique routes
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_unique_direct(smhip, dtype):
    """Permutations per line (and an argmax-shaped J = 1) on DIRECT; the same inputs without the flag give identical bytes."""
    for kind in (PUT, ADD):
        for shape, axis in (((300, 70), 0), ((300, 70), 1), ((7, 4097), 1)):
            a = specials(shape, dtype, 3)
            perm = permutations(shape, axis, 4)
            v = general(shape, dtype, 5)
            check(smhip, kind, a, perm, v, axis, unique=True, route=DIRECT)
            check(smhip, kind, a, perm, v, axis, modes=("clip",), unique=False, route=SORTED, public=False)
            one = np.expand_dims(np.argmax(v, axis), axis).astype(np.int64)
            check(smhip, kind, a, one, np.take_along_axis(v, one, axis), axis, modes=("checked",), route=DIRECT)
        shape = (2, 3, 2, 3, 2, 3)
        a = distinct(shape, dtype)
        for axis in range(6):
            check(smhip, kind, a, permutations(shape, axis, axis), general(shape, dtype, axis), axis, modes=("wrap",), unique=True, route=DIRECT, public=False)


def rows_case(lib, kind, dtype, R, I, count, seed, unique, route, mode="clip", view=None):
    """`count` ids into an (R, I) table; unique: distinct ids.  view: values as a misaligned / odd-pitched view."""
    rng = np.random.default_rng(seed)
    a = specials((R, I), dtype, seed)
    ids = (rng.permutation(R)[:count] if unique else rng.integers(-R, R, size=count)).astype(np.int64).reshape(-1, 1)
    n = ids.shape[0]
    if view is None:
        v = general((n, I), dtype, seed + 1)
        dv = None
    else:
        base = general((n, I + 3), dtype, seed + 1)
        v = base[:, 1:I + 1]  # starts one element in; pitch I + 3
        dv = lib.to_device(base).view_like(v, base)
    check(lib, kind, a, ids, v, 0, modes=(mode,), unique=unique, route=route, dv=dv, misalign=1 if view else 0, public=view is None)
    return a, ids, v


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_unique_rows(smhip, dtype):
    W = 16 // np.dtype(dtype).itemsize
    n = 0
    for R in (1, 5, 300):
        for I in (W, W + 1, 255, 256, 257, 1000):
            for count in (1, 3, 1025):
                kind = (PUT, ADD)[n % 2]
                if count > R and R == 300:  # that many distinct ids need a table that holds them: more rows than one task takes
                    rows_case(smhip, kind, dtype, 1100, I, count, n, True, ROWS, MODES[n % 3])
                count = min(count, R)
                rows_case(smhip, kind, dtype, R, I, count, n, True, ROWS, MODES[n % 3])
                if count > 1:
                    rows_case(smhip, kind, dtype, R, I, count, n, False, SORTED_ROWS, MODES[n % 3])  # distinct or not, the sorted route agrees with numpy
                n += 1
    for kind in (PUT, ADD):  # a misaligned base and an odd pitch
        rows_case(smhip, kind, dtype, 300, 256, 100, 7, True, ROWS, view=True)
        rows_case(smhip, kind, dtype, 300, 256, 100, 7, False, SORTED_ROWS, view=True)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_one_entry_per_line_in_rank_3(smhip, dtype):
    """J = 1 drops the axis from the merged walk: the groups that are left must still stand before and after it.  idx of shape
    (A, 1, 1) along the last axis leaves two groups BEFORE the axis -- out's "row" there has stride R, not 1 -- and must not be
    taken for rows."""
    lib = smhip
    for kind in (PUT, ADD):
        a = specials((3, 8, 5), dtype, 1)
        idx = indices("random", (3, 1, 1), 2, 5, 2)
        check(lib, kind, a, idx, general((3, 8, 1), dtype, 3), 2, route=DIRECT | COPY)
        check(lib, kind, a, idx, general((3, 1, 1), dtype, 3), 2, route=DIRECT | COPY)
        check(lib, kind, a, indices("edges", (3, 8, 1), 2, 5, 4), general((3, 8, 1), dtype, 5), 2, route=DIRECT)
        # one id along the last axis with a row-pitched values view
        base = general((3, 16), dtype, 6)
        v = base[:, :8].reshape(3, 8, 1)
        dv = lib.to_device(base).view_like(v, base)
        one = np.array([[[-2]]], np.int64)
        assert route_of(lib, a, one, lib.to_device(one), v, dv, 2, False) & 0xff == DIRECT
        check(lib, kind, a, one, v, 2, dv=dv)
        # the axis in the middle and in front: the group after it is a row when idx is constant along it
        for axis, ishape, vshape, route in ((1, (3, 1, 1), (3, 1, 5), ROWS), (0, (1, 1, 1), (1, 8, 5), ROWS), (0, (1, 8, 5), (1, 8, 5), DIRECT)):
            check(lib, kind, a, indices("random", ishape, axis, a.shape[axis], 7), general(vshape, dtype, 8), axis, route=route)


def test_rows_bound(smhip):
    """ROWS from I = W on; below it the entry-per-lane routes."""
    for dtype, W in ((np.float32, 4), (np.float64, 2)):
        for I, unique_route, sorted_route in ((W - 1, DIRECT, SORTED), (W, ROWS, SORTED_ROWS), (W + 1, ROWS, SORTED_ROWS)):
            a = distinct((9, I), dtype)
            ids = np.array([[8], [0], [3]], np.int64)
            v = general((3, I), dtype, I)
            check(smhip, PUT, a, ids, v, 0, modes=("checked",), unique=True, route=unique_route)
            check(smhip, ADD, a, ids, v, 0, modes=("checked",), unique=False, route=sorted_route)


# ---------------------------------------------------------------------------------------------- duplicates
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_index_add_rows_with_duplicates(smhip, dtype):
    W = 16 // np.dtype(dtype).itemsize
    for n, I in enumerate((W, W + 1, 255, 256, 257, 1000)):
        for R in (5, 300):
            rows_case(smhip, ADD, dtype, R, I, 1025, n, False, SORTED_ROWS, MODES[n % 3])
        rows_case(smhip, PUT, dtype, 5, I, 1025, n, False, SORTED_ROWS, MODES[n % 3])


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_bincount(smhip, dtype):
    """A 256-bin histogram of 70001 entries: index_add of ones, and of general weights."""
    rng = np.random.default_rng(2)
    ids = rng.integers(0, 256, size=70001).astype(np.int64)
    a = np.zeros(256, dtype)
    check(smhip, ADD, a, ids, np.ones(1, dtype), 0, modes=("clip",), route=SORTED)
    check(smhip, ADD, a, ids, general((70001,), dtype, 3), 0, modes=("checked",), route=SORTED)
    d = smhip.to_device(a)
    smhip.index_add(d, smhip.to_device(ids), 1, 0)
    assert np.array_equal(d.numpy(), np.bincount(ids, minlength=256).astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_every_entry_on_one_position(smhip, dtype):
    for kind in (PUT, ADD):
        a = specials((3, 70), dtype, 1)
        idx = np.full((3, 9001), 41, np.int64)
        check(smhip, kind, a, idx, general((3, 9001), dtype, 2), 1, modes=("wrap",), route=SORTED)
        t = specials((70, 8), dtype, 1)
        check(smhip, kind, t, np.full((2001, 1), -3, np.int64), general((2001, 8), dtype, 2), 0, modes=("checked",), route=SORTED_ROWS)


# ---------------------------------------------------------------------------------------------- broadcasts and views
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_broadcasts_and_views(smhip, dtype):
    lib = smhip
    for kind in (PUT, ADD):
        a = specials((6, 50), dtype, 1)
        idx = indices("random", (6, 120), 1, 50, 2)
        check(lib, kind, a, idx, general((1,), dtype, 3), 1, route=SORTED)                  # a scalar value
        check(lib, kind, a, idx, general((6, 1), dtype, 3), 1, route=SORTED)                # values broadcast along the axis
        check(lib, kind, a, idx[:1], general((6, 120), dtype, 3), 1, route=SORTED)          # idx broadcast over the outer axis
        check(lib, kind, a, idx[:1], general((120,), dtype, 3), 1, route=SORTED)
        # a middle axis (3, R, I): idx varying along I, and constant along it
        cube = specials((3, 40, 12), dtype, 4)
        check(lib, kind, cube, indices("heavy", (3, 90, 12), 1, 40, 5), general((3, 90, 12), dtype, 6), 1, route=SORTED)
        check(lib, kind, cube, indices("random", (3, 90, 1), 1, 40, 5), general((3, 90, 12), dtype, 6), 1, route=SORTED_ROWS)
        check(lib, kind, cube, indices("random", (1, 90, 1), 1, 40, 5), general((3, 90, 12), dtype, 6), 1, route=SORTED_ROWS)
        check(lib, kind, cube, permutations((3, 40, 12), 1, 5), general((3, 40, 12), dtype, 6), 1, unique=True, route=DIRECT)
        # transposed and stepped views of idx / values, read in place
        ibase = indices("random", (120, 6), 0, 50, 7)
        vbase = general((120, 6), dtype, 8)
        check(lib, kind, a, ibase.T, vbase.T, 1, route=SORTED, di=lib.to_device(ibase).view_like(ibase.T, ibase), dv=lib.to_device(vbase).view_like(vbase.T, vbase))
        ibase = indices("random", (6, 240), 1, 50, 9)
        vbase = general((12, 360), dtype, 10)
        iv, vv = ibase[:, ::2], vbase[::2, ::3]
        check(lib, kind, a, iv, vv, 1, route=SORTED, di=lib.to_device(ibase).view_like(iv, ibase), dv=lib.to_device(vbase).view_like(vv, vbase))
        # views that do not merge to [O] J [I]: copied dense first
        cube = distinct((4, 6, 20), dtype)
        ibase = indices("random", (8, 12, 9), 2, 20, 11)
        vbase = general((8, 12, 18), dtype, 12)
        iv, vv = ibase[::2, ::2, :], vbase[::2, ::2, ::2]
        di, dv = lib.to_device(ibase).view_like(iv, ibase), lib.to_device(vbase).view_like(vv, vbase)
        check(lib, kind, cube, iv, vv, 2, route=SORTED | COPY, di=di, dv=dv)
        plan = lib.scatter_plan(dtype, cube.shape, 2, di.strides, dv.strides, 9)
        assert plan[1] == 2 + 2 + lib.sort_plan(np.int64, (24, 9), (9, 1), 1)[1], plan


# ---------------------------------------------------------------------------------------------- safety
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_trouble_indices_on_every_route(smhip, dtype):
    """R, -R - 1, INT64_MIN, INT64_MAX, 2^32, 2^32 + 1 ... in all three modes on the four routes: the guard thirds stay intact
    (raw() asserts it), CHECKED drops exactly the bad entries and sets the flag.  The unique routes run with the promise broken by
    the clipped / wrapped troublemakers, so there only the guards and the flag are checked."""
    lib = smhip
    for kind in (PUT, ADD):
        a = specials((9, 70), dtype, 1)
        idx = trouble_indices((9, 200), 70, 2)
        check(lib, kind, a, idx, general((9, 200), dtype, 3), 1, route=SORTED)
        t = specials((70, 24), dtype, 1)
        ids = trouble_indices((200, 1), 70, 4)
        check(lib, kind, t, ids, general((200, 24), dtype, 5), 0, route=SORTED_ROWS)
        for mode in MODES:
            for target, index, vals, axis in ((a, idx, general((9, 200), dtype, 3), 1), (t, ids, general((200, 24), dtype, 5), 0)):
                _, flag = raw(lib, kind, target, index, lib.to_device(index), vals, lib.to_device(vals), axis, mode, True)
                assert flag == int(mode == "checked")
        # CHECKED on the unique routes with distinct valid entries among the bad ones: exactly the bad ones are dropped
        perm = permutations((9, 70), 1, 6)
        perm[:, ::5] = np.array([70, -71, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 32], np.int64)[np.arange(14) % 5]
        check(lib, kind, a, perm, general((9, 70), dtype, 7), 1, modes=("checked",), unique=True, route=DIRECT)
        rows = np.random.default_rng(8).permutation(70)[:40].astype(np.int64).reshape(-1, 1)
        rows[::4, 0] = [70, -71, np.iinfo(np.int64).min, np.iinfo(np.int64).max, (1 << 32) + 1, 1 << 32, -(1 << 32), 71, 1 << 62, -(1 << 62)]
        check(lib, kind, t, rows, general((40, 24), dtype, 9), 0, modes=("checked",), unique=True, route=ROWS)


def test_an_all_valid_call_clears_a_garbage_flag(smhip):
    a = distinct((4, 9), np.float32)
    for unique in (True, False):
        idx = permutations((4, 9), 1, 1)
        _, flag = raw(smhip, PUT, a, idx, smhip.to_device(idx), a, smhip.to_device(a), 1, "checked", unique)
        assert flag == 0


# ---------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_round_trips(smhip, dtype):
    lib = smhip
    x = specials((33, 257), dtype, 1)
    dx = lib.to_device(x)
    order = lib.argsort(dx, 1)
    back = lib.put_along_axis(lib.full(x.shape, 0, dtype), order, lib.sort(dx, 1), 1, mode="clip", unique=True)
    assert back.numpy().tobytes() == x.tobytes()                                # un-sorting restores x bytewise
    p = lib.to_device(permutations(x.shape, 0, 2))
    z = lib.put_along_axis(lib.full(x.shape, 0, dtype), p, dx, 0, unique=True)
    assert lib.take_along_axis(z, p, 0).numpy().tobytes() == x.tobytes()
    z = lib.put_along_axis(lib.full(x.shape, 0, dtype), p, dx, 0)                 # ... and through the sorted route
    assert lib.take_along_axis(z, p, 0).numpy().tobytes() == x.tobytes()
    table = general((300, 40), dtype, 3)
    ids = np.random.default_rng(4).integers(0, 300, size=2000).astype(np.int64)
    dt, di = lib.to_device(table), lib.to_device(ids)
    grad = lib.index_add(lib.full(table.shape, 0, dtype), di, lib.take(dt, di, 0), 0)
    want, _ = reference(ADD, np.zeros_like(table), ids.reshape(-1, 1), table[ids], 0, "checked")
    assert same(ADD, grad.numpy(), want)
    flat = lib.put(lib.to_device(x), lib.to_device(np.array([0, -1, 5, 5], np.int64)), lib.to_device(np.array([1, 2, 3, 4], dtype)))
    want = x.copy()
    np.put(want, [0, -1, 5, 5], np.array([1, 2, 3, 4], dtype))
    assert flat.numpy().tobytes() == want.tobytes()


def test_same_bits_on_every_run(smhip):
    a = general((300, 257), np.float32, 1)
    v = general((300, 3000), np.float32, 2)
    idx = indices("heavy", (300, 3000), 1, 257, 3)
    ids = indices("random", (5000,), 0, 300, 4)
    rows = general((5000, 257), np.float32, 5)
    di, dv, dids, drows = (smhip.to_device(x) for x in (idx, v, ids, rows))
    runs = [(smhip.scatter_add(smhip.to_device(a), di, dv, 1).numpy().tobytes(), smhip.index_add(smhip.to_device(a), dids, drows, 0).numpy().tobytes())
            for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_scatter_gpu import check, rows_case, specials, general, indices, permutations, PUT, ADD, DIRECT, ROWS, SORTED, SORTED_ROWS, COPY
lib = sma.load()
lib.set_device(0)
for dtype in (np.float32, np.float64, np.int32, np.int64):
    for kind in (PUT, ADD):
        a = specials((333, 70), dtype, 1)
        check(lib, kind, a, indices("heavy", (333, 141), 1, 70, 2), general((333, 141), dtype, 3), 1, route=SORTED)
        check(lib, kind, a, permutations((333, 70), 0, 4), general((333, 70), dtype, 5), 0, unique=True, route=DIRECT)
        rows_case(lib, kind, dtype, 333, 70, 300, 6, True, ROWS)
        rows_case(lib, kind, dtype, 333, 70, 1025, 7, False, SORTED_ROWS)
        check(lib, kind, a[:2], indices("random", (2, 9001), 1, 70, 8), general((2, 9001), dtype, 9), 1, modes=("wrap",), route=SORTED)
        cube = specials((4, 6, 20), dtype, 10)
        ibase = indices("random", (8, 12, 9), 2, 20, 11)
        iv = ibase[::2, ::2, :]
        check(lib, kind, cube, iv, general((4, 6, 9), dtype, 12), 2, route=SORTED | COPY, di=lib.to_device(ibase).view_like(iv, ibase))
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_SCATTER_GRID_CAP=2: every kernel's loop over its tasks runs many times per workgroup, on the four routes and COPY."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_SCATTER_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_empty_cases(smhip):
    lib = smhip
    a = distinct((4, 9), np.float32)
    none = lib.to_device(np.zeros(1, np.int64))
    none = sma.DeviceArray(lib, none.base_ptr, np.int64, (4, 0), (0, 1), 0, none._owner)
    vals = lib.to_device(np.zeros(1, np.float32))
    for fn in (lib.put_along_axis, lib.scatter_add):
        d = lib.to_device(a)
        assert fn(d, none, 1.0, 1) is d and d.numpy().tobytes() == a.tobytes()  # J = 0
    ids0 = sma.DeviceArray(lib, none.base_ptr, np.int64, (0,), (1,), 0, none._owner)
    d = lib.to_device(a)
    assert lib.index_add(d, ids0, 2.0, 0).numpy().tobytes() == a.tobytes()
    empty = lib.empty((0, 9), np.float32)  # no lines
    idx = sma.DeviceArray(lib, none.base_ptr, np.int64, (0, 3), (3, 1), 0, none._owner)
    assert lib.put_along_axis(empty, idx, 1.0, 1) is empty
    hollow = lib.empty((4, 0), np.float32)  # R = 0 with entries
    with pytest.raises(IndexError):
        lib.put_along_axis(hollow, lib.to_device(np.zeros((4, 2), np.int64)), vals, 1)
    with pytest.raises(IndexError):
        lib.index_add(hollow, lib.to_device(np.zeros(2, np.int64)), 1.0, 1)


def test_no_entries_with_values_that_broadcast_along_the_axis(smhip):
    """J = 0 with a values array of extent 1 along the axis: numpy broadcasts (7, 1) against (7, 0) to (7, 0) and writes nothing.  The
    binding used to refuse it (it asked sm::broadcast, which has no empty extents).  Found by tests/fuzz_axis.py, seed 7."""
    lib = smhip
    a = distinct((7, 9), np.float32)
    none = lib.to_device(np.zeros(1, np.int64))
    none = sma.DeviceArray(lib, none.base_ptr, np.int64, (7, 0), (0, 1), 0, none._owner)
    for shape in ((7, 1), (1, 1), (1,), (7, 0)):
        vals = lib.to_device(np.ones(max(1, int(np.prod(shape))), np.float32))
        vals = sma.DeviceArray(lib, vals.base_ptr, np.float32, shape, (1,) * len(shape), 0, vals._owner)
        for fn in (lib.put_along_axis, lib.scatter_add):
            d = lib.to_device(a)
            assert fn(d, none, vals, 1, mode="clip") is d and d.numpy().tobytes() == a.tobytes(), shape
    with pytest.raises(ValueError):   # still refused: neither the walk's extent nor 1
        lib.put_along_axis(lib.to_device(a), none, lib.to_device(np.ones((7, 2), np.float32)), 1)

