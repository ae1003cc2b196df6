"""unique / unique_consecutive on the GPU (the C ABI through the ctypes binding) against numpy, exactly.

The oracle is np.unique(x, return_index=True, return_inverse=True, return_counts=True, equal_nan=...): index, inverse and counts compare as
bytes, values by value with NaN equal to NaN AND as bytes against x.ravel()[index].  For unique_consecutive it is the same flag
construction in numpy without the sort.  The raw calls get their sorted input and its positions from numpy's stable argsort, whose order
(-0 == +0, every NaN last, NaNs tied) is the library's.  Results of the raw calls are the MIDDLE THIRD of a buffer of sentinels whose
outer thirds must come back byte-identical (tests/test_select_gpu.py's Guarded); the count word holds garbage before the call.  The tile,
and the largest size of the one-workgroup route, are taken from the plan."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma
from tests.test_select_gpu import SENTINEL, Guarded, count_word, off_by_one

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
V, I, C, INV = sma.RUNS_VALUES, sma.RUNS_INDEX, sma.RUNS_COUNTS, sma.RUNS_INVERSE
ALL = V | I | C | INV
NAMES = {V: "values", I: "index", C: "counts", INV: "inverse"}
ONE, TILES = sma.RUNS_ROUTE_ONE, sma.RUNS_ROUTE_TILES
PATTERNS = ("all_equal", "all_distinct", "tile_start", "tile_edge", "wave_start", "vector_start", "long_runs", "few_keys", "percent")


def constants(lib, dtype):
    """(the elements of a tile, the largest element count of the one-workgroup route)"""
    info = lib.runs_plan(dtype, 1000)[2]
    return info[1], info[2]


def sizes(lib, dtype):
    tile, threshold = constants(lib, dtype)
    return sorted({0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, threshold - 1, threshold, threshold + 1, tile - 1, tile, tile + 1, 2 * tile + 3, 70001,
                   129 * tile + 5})


# ---------------------------------------------------------------------------------------------- the oracles
def np_unique(x, equal_nan):
    """np.unique's four results of the flattening, the inverse as one line."""
    values, index, inverse, counts = np.unique(x, return_index=True, return_inverse=True, return_counts=True, equal_nan=equal_nan)
    return {V: values, I: index.astype(np.int64), C: counts.astype(np.int64), INV: inverse.astype(np.int64).ravel()}


def np_runs(x, equal_nan):
    """The runs of x (1-D) as it stands: the same flags, without the sort."""
    n = x.size
    if n == 0:
        return {V: x[:0], I: np.zeros(0, np.int64), C: np.zeros(0, np.int64), INV: np.zeros(0, np.int64)}
    same = x[1:] == x[:-1]
    if equal_nan and x.dtype.kind == "f":
        same |= np.isnan(x[1:]) & np.isnan(x[:-1])
    flags = np.concatenate([[True], ~same])
    starts = np.flatnonzero(flags).astype(np.int64)
    return {V: x[starts], I: starts, C: np.diff(np.append(starts, n)).astype(np.int64), INV: np.cumsum(flags).astype(np.int64) - 1}


def same_values(got, want):
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=want.dtype.kind == "f")


# ---------------------------------------------------------------------------------------------- the raw calls
def raw_count(lib, ds, equal_nan=True):
    word = count_word(lib)
    rc = lib.runs_count_raw(0 if equal_nan else sma.RUNS_NAN_DISTINCT, sma.DTYPES[ds.dtype], ds.ptr, ds.size, word.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return int(word.numpy()[0])


def raw_runs(lib, ds, dorder, outputs, total, capacity=None, equal_nan=True, with_count=True, misalign=0):
    """One smhip_runs into guarded buffers -> ({result bit: the items written}, the count word).  `total` is numpy's number of runs:
    exactly min(total, capacity) items of values, index and counts may be written, and all n of the inverse."""
    capacity = total if capacity is None else capacity
    n = ds.size
    bufs = {bit: Guarded(lib, n if bit == INV else capacity, ds.dtype if bit == V else np.int64, misalign) for bit in (V, I, C, INV) if outputs & bit}
    word = count_word(lib)
    ptr = lambda bit: bufs[bit].ptr if bit in bufs else 0  # noqa: E731
    rc = lib.runs_raw(0 if equal_nan else sma.RUNS_NAN_DISTINCT, sma.DTYPES[ds.dtype], ds.ptr, n, dorder.ptr if dorder is not None else 0, ptr(V), ptr(I), ptr(C),
                      ptr(INV), capacity, word.ptr if with_count else 0)
    assert rc == 0, lib.c.smhip_last_error().decode()
    written = min(total, capacity)
    got = {}
    for bit, buf in bufs.items():
        items = buf.result()     # asserts the sentinels on both sides
        if bit != INV:
            assert (items[written:].view(np.uint8) == SENTINEL).all(), f"{NAMES[bit]}: a write past the items counted"
            items = items[:written]
        got[bit] = items
    return got, int(word.numpy()[0]) if with_count else None


def compare(got, want, x_flat, written, tag):
    """Index, inverse and counts as bytes; values by value and as the bytes of the element the index names."""
    for bit, items in got.items():
        expect = want[bit] if bit == INV else want[bit][:written]
        if bit == V:
            assert same_values(items, expect), (tag, "values")
            assert items.tobytes() == x_flat[want[I][:written]].tobytes(), (tag, "values: not the bits of the first occurrence")
        else:
            assert items.dtype == np.int64 and items.tobytes() == expect.tobytes(), (tag, NAMES[bit])


def check_both(lib, x, equal_nan=True, outputs=ALL, route=None, tag=None):
    """np.unique through (numpy's stable argsort, smhip_runs with its positions) and the runs of x as it stands, the count each time."""
    tag = (x.dtype.name, x.size, equal_nan, outputs) if tag is None else tag
    if route is not None:
        assert lib.runs_plan(x.dtype, x.size, outputs)[0] == route, tag
    order = np.argsort(x, kind="stable").astype(np.int64)
    s = x[order]
    ds, dorder, dx = lib.to_device(s), lib.to_device(order), lib.to_device(x)
    want = np_unique(x, equal_nan)
    total = want[V].size
    assert raw_count(lib, ds, equal_nan) == total, tag
    got, counted = raw_runs(lib, ds, dorder, outputs, total, equal_nan=equal_nan)
    assert counted == total, tag
    compare(got, want, x, total, tag + ("sorted",))
    want = np_runs(x, equal_nan)
    total = want[V].size
    assert raw_count(lib, dx, equal_nan) == total, tag
    got, counted = raw_runs(lib, dx, None, outputs, total, equal_nan=equal_nan)
    assert counted == total, tag
    compare(got, want, x, total, tag + ("consecutive",))


def keys_of(kind, n, tile, W, dtype, seed):
    """n keys whose SORTED order has its run boundaries where `kind` says, shuffled."""
    rng = np.random.default_rng(seed)
    if kind == "few_keys":
        return rng.integers(0, 7, size=n).astype(dtype)
    m = np.zeros(n, bool)
    if kind == "all_distinct":
        m[:] = True
    elif kind == "tile_start":        # a boundary exactly at every tile start
        m[::tile] = True
    elif kind == "tile_edge":         # one element before a tile start, and one after it
        for e in range(tile, n, tile):
            m[e - 1] = True
            if e + 1 < n:
                m[e + 1] = True
    elif kind == "wave_start":        # a wave's 64 vectors
        m[::64 * W] = True
    elif kind == "vector_start":
        m[::W] = True
    elif kind == "long_runs":         # runs longer than a tile
        m[::2 * tile + 7] = True
    elif kind == "percent":
        m = rng.random(n) < 0.01
    ids = np.cumsum(m) - (1 if n and m[0] else 0)     # "all_equal": one run
    return rng.permutation((ids - ids.max() // 2).astype(dtype)) if n else ids.astype(dtype)


# ---------------------------------------------------------------------------------------------- sizes x patterns
@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_every_size_and_pattern(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    W = 16 // np.dtype(dtype).itemsize
    for n in sizes(lib, dtype):
        route = None if n == 0 else ONE if n <= threshold else TILES
        for kind in PATTERNS:
            if n == 0 and kind != "all_equal":
                continue
            x = keys_of(kind, n, tile, W, dtype, n)
            if n == 0:   # nothing is launched: the count is 0 and nothing is written
                dx = lib.empty((0,), dtype)
                assert raw_count(lib, dx) == 0
                got, counted = raw_runs(lib, dx, None, ALL, 0, capacity=4)
                assert counted == 0 and all(v.size == 0 for v in got.values())
                continue
            check_both(lib, x, route=route, tag=(np.dtype(dtype).name, n, kind))


@pytest.mark.parametrize("dtype", (np.float64, np.int32), **IDS)
def test_the_other_two_types(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    W = 16 // np.dtype(dtype).itemsize
    for n in (1, 5, 257, threshold, threshold + 1, 2 * tile + 3, 70001):
        for kind in ("few_keys", "tile_edge", "vector_start", "percent"):
            check_both(lib, keys_of(kind, n, tile, W, dtype, n), tag=(np.dtype(dtype).name, n, kind))


# ---------------------------------------------------------------------------------------------- values that catch a narrow compare
def nans(dtype):
    """NaNs of both signs and several payloads."""
    if np.dtype(dtype) == np.float32:
        return np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC12345, 0x7FE00000], np.uint32).view(np.float32)
    return np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFF8000012345678, 0x7FFC000000000000], np.uint64).view(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_values_that_catch_a_narrow_compare(smhip, dtype):
    lib = smhip
    dtype = np.dtype(dtype)
    tile, threshold = constants(lib, dtype)
    rng = np.random.default_rng(7)
    if dtype.kind == "i":
        info = np.iinfo(dtype)
        base = [info.min, info.min + 1, info.max, info.max - 1, 0, 1, -1, -2, 6, 7]
        if dtype.itemsize == 8:   # pairs that differ only above bit 32, and only in bit 0
            base += [5 + (1 << 32), 5 + (1 << 33), 5 + (1 << 40), 5 - (1 << 32), 5, 4, (1 << 62), (1 << 62) + 1, (1 << 62) + (1 << 32), -(1 << 62), -(1 << 62) - (1 << 32)]
        pool = np.array(base, dtype)
    else:
        one = dtype.type(1)
        up, down = np.nextafter(one, dtype.type(2)), np.nextafter(one, dtype.type(0))   # one ULP apart
        tiny = np.finfo(dtype).smallest_subnormal
        pool = np.concatenate([np.array([one, up, down, 0.0, -0.0, tiny, -tiny, np.inf, -np.inf, np.finfo(dtype).max, 2.5], dtype), nans(dtype)])
    for equal_nan in (True, False):
        # by hand: the zeros next to each other, NaNs next to each other and apart, +inf before the NaNs
        if dtype.kind == "f":
            q = nans(dtype)
            x = np.array([0.0, -0.0, 0.0, 1.0, q[0], q[1], q[2], 2.0, q[3], np.inf, q[4], q[0], np.inf, -0.0, -0.0, 0.0], dtype)
            x[4:7], x[8:9], x[10:12] = q[:3], q[3:4], q[[4, 0]]     # (the constructor above may not keep a payload: these do)
            check_both(lib, x, equal_nan)
        for n in (pool.size, 300, threshold + tile + 3):
            x = pool[rng.integers(0, pool.size, size=n)] if n != pool.size else pool.copy()
            check_both(lib, x, equal_nan)
            # ... and long runs of each, so that equal neighbours meet across vectors, waves and tiles
            check_both(lib, np.repeat(pool, -(-n // pool.size))[:n], equal_nan)


# ---------------------------------------------------------------------------------------------- subsets, capacities, order, alignment
@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_every_subset_capacity_and_alignment(smhip, dtype):
    lib = smhip
    tile, threshold = constants(lib, dtype)
    for n in (261, threshold + tile + 3):
        rng = np.random.default_rng(n)
        x = rng.integers(-40, 40, size=n).astype(dtype)
        if np.dtype(dtype).kind == "f":
            x[rng.integers(0, n, 9)] = np.nan
        order = np.argsort(x, kind="stable").astype(np.int64)
        s = x[order]
        ds, dorder, dx = lib.to_device(s), lib.to_device(order), lib.to_device(x)
        ds_off, dx_off = off_by_one(lib, s), off_by_one(lib, x)     # one element off a 16-byte boundary
        sorted_want, runs_want = np_unique(x, True), np_runs(x, True)
        for outputs in range(1, 16):       # every subset of the four results
            tag = (np.dtype(dtype).name, n, outputs)
            for operand, positions, want, base in ((ds, dorder, sorted_want, x), (dx, None, runs_want, x), (ds_off, dorder, sorted_want, x), (dx_off, None, runs_want, x)):
                total = want[V].size
                for capacity in (0, total - 1, total, total + 5):
                    got, counted = raw_runs(lib, operand, positions, outputs, total, capacity=capacity, with_count=capacity != total)
                    assert counted in (None, total), tag
                    part = {bit: items for bit, items in got.items() if bit != V}
                    compare(part, want, base, min(total, capacity), tag + (capacity,))
                    if V in got:
                        assert got[V].tobytes() == base[want[I][:min(total, capacity)]].tobytes(), tag + (capacity, "values")
            # results one item off the 16-byte grid as well
            got, _ = raw_runs(lib, ds, dorder, outputs, sorted_want[V].size, misalign=1)
            compare(got, sorted_want, x, sorted_want[V].size, tag + ("misaligned results",))


def test_positions_outside_the_array_write_nothing(smhip):
    """order[i] outside [0, n) is copied to index_out like any value and names no element of the inverse."""
    lib = smhip
    n = 5000
    s = np.sort(np.random.default_rng(3).integers(0, 50, size=n)).astype(np.int32)
    order = np.random.default_rng(4).permutation(n).astype(np.int64)
    bad = np.array([0, 1, 17, 2048, 2049, n - 1])
    order[bad] = [-1, n, 1 << 40, -(1 << 62), np.iinfo(np.int64).max, np.iinfo(np.int64).min]
    want = np_runs(s, True)
    total = want[V].size
    got, counted = raw_runs(lib, lib.to_device(s), lib.to_device(order), ALL, total)
    assert counted == total and got[V].tobytes() == want[V].tobytes() and got[C].tobytes() == want[C].tobytes()
    assert got[I].tobytes() == order[want[I]].tobytes()
    named = np.ones(n, bool)
    named[bad] = False
    inverse = np.full(n, np.frombuffer(bytes([SENTINEL] * 8), np.int64)[0])
    inverse[order[named]] = want[INV][named]
    assert got[INV].tobytes() == inverse.tobytes()


# ---------------------------------------------------------------------------------------------- the prefix kernel's carry
def test_more_tiles_than_one_pass_of_the_prefix(smhip):
    """unique_consecutive on int32 over 16 * 256 + 1 tiles: the prefix kernel takes 16 counts per lane and pass, so the last tile's
    offset comes from its carry.  Values and counts only."""
    lib = smhip
    tile, threshold = constants(lib, np.int32)
    n = (16 * 256 + 1) * tile
    assert lib.runs_plan(np.int32, n, V | C) == (TILES, 4, (16 * 256 + 1, tile, threshold))
    run = 3 * tile + 1                                   # runs longer than a tile, a boundary in the last tile too
    x = ((np.arange(n, dtype=np.int64) // run) % 5).astype(np.int32)
    x[-3:] = (7, 7, 8)
    want = np_runs(x, True)
    dx = lib.to_device(x)
    values, counts = lib.unique_consecutive(dx, return_counts=True)
    assert values.shape == counts.shape == (want[V].size,)
    assert values.numpy().tobytes() == want[V].tobytes() and counts.numpy().tobytes() == want[C].tobytes()


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_unique_gpu import check_both, constants, keys_of, TILES
lib = sma.load()
lib.set_device(0)
for dtype in (np.float32, np.int64):
    tile, threshold = constants(lib, dtype)
    n = 41 * tile + 7                          # 42 tiles under a grid of 3 workgroups: every workgroup walks 14 of them
    for kind in ("tile_edge", "percent"):
        check_both(lib, keys_of(kind, n, tile, 16 // np.dtype(dtype).itemsize, dtype, 1), route=TILES)
print("capped ok")
"""


def test_the_tile_loops_under_a_capped_grid():
    """The tile kernels share select's cap, SMHIP_SELECT_GRID_CAP, which is read once per process: the capped run is a process of its own."""
    env = dict(os.environ, SMHIP_SELECT_GRID_CAP="3", PYTHONPATH=sma.ROOT)
    r = subprocess.run([sys.executable, "-c", _CAPPED], capture_output=True, text=True, env=env, timeout=300, cwd=sma.ROOT)
    assert r.returncode == 0 and "capped ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------- through the binding
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_unique_through_the_binding(smhip, dtype):
    lib = smhip
    rng = np.random.default_rng(11)
    base = rng.integers(-9, 9, size=(67, 131)).astype(dtype)
    if np.dtype(dtype).kind == "f":
        base[rng.integers(0, 67, 12), rng.integers(0, 131, 12)] = [np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf] * 2
    dbase = lib.to_device(base)
    views = {"2-D": base, "transposed": base.T, "stepped": base[3:60:2, 5:100:3], "1-D": base.reshape(-1)[:1000]}
    for name, view in views.items():
        d = dbase.view_like(view, base)
        for equal_nan in (True, False):
            want = np_unique(view, equal_nan)
            flat = np.ascontiguousarray(view).ravel()
            for ri, rv, rc in itertools.product((False, True), repeat=3):
                got = lib.unique(d, return_index=ri, return_inverse=rv, return_counts=rc, equal_nan=equal_nan)
                got = got if isinstance(got, tuple) else (got,)
                bits = [V] + [bit for bit, on in ((I, ri), (INV, rv), (C, rc)) if on]
                assert len(got) == len(bits)
                for bit, g in zip(bits, got):
                    assert g.shape == (view.shape if bit == INV else (want[V].size,)) and g.dtype == (view.dtype if bit == V else np.int64)
                compare({bit: g.numpy().ravel() for bit, g in zip(bits, got)}, want, flat, want[V].size, (name, equal_nan, ri, rv, rc))
            want = np_runs(flat, equal_nan)
            values, inverse, counts = lib.unique_consecutive(d, return_inverse=True, return_counts=True, equal_nan=equal_nan)
            assert inverse.shape == view.shape
            compare({V: values.numpy(), INV: inverse.numpy().ravel(), C: counts.numpy()}, want, flat, want[V].size, (name, equal_nan, "consecutive"))
            assert lib.unique_consecutive(d, equal_nan=equal_nan).numpy().tobytes() == want[V].tobytes()
            # values.take(inverse) rebuilds the operand, up to which zero and which NaN
            values, inverse = lib.unique(d, return_inverse=True, equal_nan=equal_nan)
            assert same_values(lib.take(values, inverse).numpy(), np.ascontiguousarray(view))


def test_empty_operands(smhip):
    lib = smhip
    for shape in ((0,), (4, 0, 3)):
        d = lib.empty(shape, np.float32)
        values, index, inverse, counts = lib.unique(d, return_index=True, return_inverse=True, return_counts=True)
        assert values.shape == index.shape == counts.shape == (0,) and inverse.shape == shape
        assert values.dtype == np.float32 and index.dtype == inverse.dtype == counts.dtype == np.int64
        assert lib.unique(d).shape == (0,) and lib.unique_consecutive(d).shape == (0,)
        values, counts = lib.unique_consecutive(d, return_counts=True)
        assert values.shape == counts.shape == (0,)


def test_empty_views_that_are_not_dense(smhip):
    """base[:, 3:3] keeps base's row stride, so it is copied dense before it is flattened: that copy of nothing used to be refused
    ("destination stride 0": the dense strides of (5, 0) are (0, 1)).  Found by tests/fuzz_axis.py, seed 7."""
    lib = smhip
    base = np.arange(35, dtype=np.float32).reshape(5, 7)
    d = lib.to_device(base)
    for view in (base[:, 3:3], base[1:4:2, 5:5], base.T[:, 2:2], base.reshape(5, 7, 1)[:, 2:2, :]):
        dv = d.view_like(view, base)
        assert not dv.is_dense() and dv.size == 0
        values, index, inverse, counts = lib.unique(dv, return_index=True, return_inverse=True, return_counts=True)
        assert values.shape == index.shape == counts.shape == (0,) and inverse.shape == view.shape
        assert lib.unique_consecutive(dv).shape == (0,)
        assert lib.sort(dv, axis=None).shape == (0,) and lib.scan("cumsum", dv, axis=None).shape == (0,)


def test_group_by_through_index_add(smhip):
    """The keys' inverse fed to index_add: a sum per key, against np.add.at."""
    lib = smhip
    rng = np.random.default_rng(5)
    n = 100003
    keys = (rng.integers(-30, 30, size=n) * (1 << 35) + rng.integers(0, 2, size=n)).astype(np.int64)     # no bincount reaches these
    v = rng.integers(-8, 9, size=n).astype(np.float32)          # whole numbers: every order of the additions gives the same sum
    dk, dv = lib.to_device(keys), lib.to_device(v)
    values, inverse = lib.unique(dk, return_inverse=True)
    want_values, want_inverse = np.unique(keys, return_inverse=True)
    assert values.numpy().tobytes() == want_values.tobytes()
    sums = lib.full((values.size,), 0, np.float32)
    lib.index_add(sums, inverse, dv, axis=0)
    want = np.zeros(want_values.size, np.float32)
    np.add.at(want, want_inverse.ravel(), v)
    assert sums.numpy().tobytes() == want.tobytes()
