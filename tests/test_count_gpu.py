"""searchsorted / bincount / histogram on the GPU (the C ABI through the ctypes binding) against numpy, exactly.

Oracles: np.searchsorted; for bincount the index rule applied on the host and np.bincount, and the library's own index_add of ones
onto zeros; for histogram np.histogram in both of its forms and the searchsorted rule written out.  Results of the raw calls are the
MIDDLE THIRD of a buffer of sentinels whose outer thirds must come back byte-identical; the bincount flag word holds garbage before
the call.  The routes, K and the LDS budget for edges are taken from the plan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
MODES = ("checked", "clip", "wrap")
LDS, GLOBAL, COPY = sma.COUNT_ROUTE_LDS, sma.COUNT_ROUTE_GLOBAL, sma.COUNT_COPY
N_LIST = (0, 1, 3, 4, 5, 63, 64, 65, 1023, 1025, 70001)
KINDS = ("identity", "same", "random", "negative", "edges", "heavy")
GARBAGE = 0x5A5A5A5A5A5A5A5A
SENTINEL = -7777777
# (lo, hi, bins): the issue's list
UNIFORM_CASES = ((0, 1, 1), (0, 1, 7), (-3, 5, 256), (0.1, 0.7, 1000), (-1e3, 1e3, 8193), (1, 1 + 2.0 ** -10, 64), (0, 255, 255), (-2.5, 2.5, 16384),
                 (-2.5, 2.5, 16385))


def dense(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.insert(0, acc)
        acc *= d
    return st


def constants(lib):
    """(K, {dtype: the most edges staged in LDS})"""
    K = lib.count_plan("bincount", np.int64, [1000], [1], 4)[2][3]
    return K, {np.dtype(t): lib.count_plan("searchsorted", t, [1000], [1], 4)[2][4] for t in DTYPES}


def route_of(lib, what, d, bins, **kw):
    return lib.count_plan(what, d.dtype, d.shape, d.strides, bins, **kw)[0]


class Guarded:
    """n int64 results as the middle third of a buffer of sentinels; misalign: the result starts 8 bytes off a 16-byte boundary."""

    def __init__(self, lib, n, misalign=0):
        self.n, self.third = n, (n + 2) // 2 * 2 + misalign
        self.host = np.full(3 * self.third, SENTINEL, np.int64)
        self.buf = lib.to_device(self.host)
        self.ptr = self.buf.ptr + 8 * self.third

    def result(self):
        back = self.buf.numpy()
        t, n = self.third, self.n
        assert back[:t].tobytes() == self.host[:t].tobytes() and back[t + n:].tobytes() == self.host[t + n:].tobytes(), "a write outside the result"
        return back[t:t + n]


def off_by_one(lib, host):
    """`host` (1-D) on the device starting one element into a buffer: not 16-byte aligned."""
    base = np.concatenate([host[:1], host]) if host.size else np.zeros(1, host.dtype)
    return lib.to_device(base).view_like(base[1:], base)


# ---------------------------------------------------------------------------------------------- searchsorted
def make_edges(dtype, E, seed):
    """E sorted edges with repeats; floats end in NaNs and hold both zeros and the infinities, integers their extremes."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        e = np.round(rng.standard_normal(E) * 8, 1).astype(dtype)
        fixed = np.array([-np.inf, -0.0, 0.0, np.inf, np.nan, np.nan], dtype)
    else:
        e = rng.integers(-40, 40, size=E).astype(dtype)
        info = np.iinfo(dtype)
        fixed = np.array([info.min, info.min + 1, 0, info.max - 1, info.max, info.max], dtype)
    k = min(E, fixed.size) if E >= 3 else 0
    e[:k] = fixed[:k]
    return np.sort(e)  # NaNs last


def probes(dtype, edges, n, seed):
    """n values: every edge, its neighbours, values outside the table, both zeros, the infinities, NaN, the integer extremes."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        with np.errstate(all="ignore"):
            pool = np.concatenate([edges, np.nextafter(edges, dtype.type(-np.inf)), np.nextafter(edges, dtype.type(np.inf)),
                                   np.array([np.nan, -np.nan, -np.inf, np.inf, -0.0, 0.0, -1e30, 1e30, 1.5], dtype)]).astype(dtype)
        rand = (rng.standard_normal(n) * 10).astype(dtype)
    else:
        info = np.iinfo(dtype)
        wide = edges.astype(object)
        near = np.array([min(max(int(v) + s, info.min), info.max) for v in wide for s in (-1, 1)], dtype) if edges.size < 100000 else edges
        pool = np.concatenate([edges, near, np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1, 1], dtype)]).astype(dtype)
        rand = rng.integers(-50, 50, size=n).astype(dtype)
    if n == 0:
        return np.zeros(0, dtype)
    if pool.size > n // 2:
        pool = pool[rng.permutation(pool.size)[: max(1, n // 2)]] if n > 8 else pool[rng.permutation(pool.size)[:n]]
    x = rand
    x[rng.permutation(n)[:pool.size]] = pool[:min(pool.size, n)]
    return x


def check_searchsorted(lib, edges, x, dx=None, misalign=0, public=False, route=None):
    de = lib.to_device(edges)
    dx = lib.to_device(x) if dx is None else dx
    if route is not None:
        assert route_of(lib, "searchsorted", dx, edges.size) == route, (x.dtype, edges.size, x.shape)
    for side in ("left", "right"):
        want = np.searchsorted(edges, x.reshape(-1), side).astype(np.int64)
        out = Guarded(lib, x.size, misalign)
        rc = lib.searchsorted_raw(sma.SIDES[side], sma.DTYPES[x.dtype], de.ptr, edges.size, dx.ptr, dx.shape, dx.strides, out.ptr)
        assert rc == 0, lib.c.smhip_last_error().decode()
        got = out.result()
        assert np.array_equal(got, want), (x.dtype, side, edges.size, x.shape, misalign)
        if public:
            res = lib.searchsorted(de, dx, side)
            assert res.shape == tuple(x.shape) and res.dtype == np.int64 and np.array_equal(res.numpy().reshape(-1), want)


def test_the_example_of_the_contract(smhip):
    edges = np.array([-np.inf, -0., 0., 1, 1, 2, np.inf, np.nan, np.nan])
    x = np.array([np.nan, -np.inf, 0., -0., 1, 1.5, np.inf, 3])
    for dtype in (np.float32, np.float64):
        de, dx = smhip.to_device(edges.astype(dtype)), smhip.to_device(x.astype(dtype))
        assert smhip.searchsorted(de, dx, "left").numpy().tolist() == [7, 0, 1, 1, 3, 5, 6, 6]
        assert smhip.searchsorted(de, dx, "right").numpy().tolist() == [9, 1, 3, 3, 5, 5, 7, 6]
        assert smhip.searchsorted(de, dx).numpy().tolist() == [7, 0, 1, 1, 3, 5, 6, 6]  # left is the default


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_searchsorted_table_and_operand_lengths(smhip, dtype):
    lib = smhip
    budget = constants(lib)[1][np.dtype(dtype)]
    k = 0
    for E in (0, 1, 2, 63, 64, 65, 1000, budget, budget + 1, 40 * budget + 7):
        edges = make_edges(dtype, E, E)
        route = None if E == 0 else LDS if E <= budget else GLOBAL
        for n in N_LIST:
            x = probes(dtype, edges, n, k)
            if n:
                check_searchsorted(lib, edges, x, misalign=k % 2, public=k % 7 == 0, route=route)
                if k % 3 == 0:  # x starts one element into its buffer: the head and tail paths move
                    check_searchsorted(lib, edges, x, dx=off_by_one(lib, x), misalign=(k // 3) % 2, route=route)
            else:
                check_searchsorted(lib, edges, x, public=True)
            k += 1


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_searchsorted_of_views(smhip, dtype):
    lib = smhip
    edges = make_edges(dtype, 300, 5)
    base = probes(dtype, edges, 6 * 40 * 18, 6).reshape(6, 40, 18)
    db = lib.to_device(base)
    check_searchsorted(lib, edges, base, public=True, route=LDS)                                      # rank 3, dense
    for view in (base.transpose(2, 0, 1), base[::2, 1::3, ::2], base[:, :, 3]):
        check_searchsorted(lib, edges, view, dx=db.view_like(view, base), public=True, route=LDS | COPY)
    row = base[2, 5:6, :]
    bc = sma.DeviceArray(lib, db.base_ptr, db.dtype, (7, 18), (0, 1), (2 * 40 + 5) * 18, db._owner)    # a broadcast row
    check_searchsorted(lib, edges, np.broadcast_to(row, (7, 18)), dx=bc, route=LDS | COPY)
    out = lib.empty((6 * 40 * 18,), np.int64)
    assert lib.searchsorted(lib.to_device(edges), db, "right", out=out) is out
    assert np.array_equal(out.numpy(), np.searchsorted(edges, base.reshape(-1), "right"))


def test_searchsorted_with_unsorted_edges_stays_in_range(smhip):
    rng = np.random.default_rng(1)
    for dtype in DTYPES:
        for E in (5, 1000, 100001):
            edges = rng.integers(-100, 100, size=E).astype(dtype)
            x = rng.integers(-120, 120, size=5001).astype(dtype)
            for side in ("left", "right"):
                got = smhip.searchsorted(smhip.to_device(edges), smhip.to_device(x), side).numpy()
                assert got.min() >= 0 and got.max() <= E


# ---------------------------------------------------------------------------------------------- bincount
def make_ids(kind, n, R, dtype, seed=0):
    """n ids of `dtype`, every value in [-R, R)."""
    rng = np.random.default_rng(seed)
    along = np.arange(n, dtype=np.int64)
    if kind == "identity":
        ids = along % R
    elif kind == "same":
        ids = np.full(n, (seed * 7 + 3) % R, np.int64)
    elif kind == "random":
        ids = rng.integers(0, R, size=n)
    elif kind == "negative":
        ids = rng.integers(-R, 0, size=n)
    elif kind == "edges":
        ids = np.array([-R, -1, 0, R - 1], np.int64)[(along + rng.integers(0, 4, size=n)) % 4]
    else:  # heavy: 90 % of the entries hit 3 positions
        hot = rng.integers(0, R, size=3)
        ids = np.where(rng.random(n) < 0.9, hot[rng.integers(0, 3, size=n)], rng.integers(0, R, size=n))
    return ids.astype(dtype)


def trouble_ids(n, R, dtype, seed):
    """Valid ids with the troublemakers scattered among them."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-R, R, size=n).astype(np.int64)
    info = np.iinfo(dtype)
    if np.dtype(dtype) == np.int64:
        trouble = [R, -R - 1, info.min, info.max, 1 << 32, (1 << 32) + 1, -(1 << 32), R + (1 << 32), (1 << 63) - R]
    else:
        trouble = [R, -R - 1, info.min, info.max, 1 << 30, (1 << 30) + 1, -(1 << 30), info.max - R, info.min + R]
    trouble = np.array([t for t in trouble if info.min <= t <= info.max], np.int64)
    at = rng.permutation(n)[: max(trouble.size, n // 7)]
    ids[at] = trouble[np.arange(at.size) % trouble.size]
    return ids.astype(dtype)


def expected_counts(ids, R, mode):
    """-> (counts, was any id bad): the index rule of the README, *Writing by position*, on the host."""
    i = ids.reshape(-1).astype(np.int64)
    if mode == "clip":
        pos, ok = np.clip(i, 0, R - 1), np.ones(i.shape, bool)
    elif mode == "wrap":
        pos, ok = np.mod(i, R), np.ones(i.shape, bool)
    else:
        ok = (i >= -R) & (i < R)
        pos = np.where(i < 0, i + R, i)
    return np.bincount(pos[ok], minlength=R).astype(np.int64), bool((~ok).any())


def raw_bincount(lib, di, R, mode, misalign=0):
    """The C ABI itself -> (counts, flag)."""
    out = Guarded(lib, R, misalign)
    flag = lib.to_device(np.array([GARBAGE], np.int64))
    rc = lib.bincount_raw(sma.INDEX_MODES[mode], sma.DTYPES[di.dtype], di.ptr, di.shape, di.strides, R, out.ptr, flag.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return out.result(), int(flag.numpy()[0])


def check_bincount(lib, ids, R, modes=MODES, di=None, route=None, public=True, misalign=0):
    di = lib.to_device(ids) if di is None else di
    if route is not None and ids.size:
        assert route_of(lib, "bincount", di, R) == route, (ids.dtype, ids.shape, R)
    for mode in modes:
        want, bad = expected_counts(ids, R, mode)
        got, flag = raw_bincount(lib, di, R, mode, misalign)
        assert np.array_equal(got, want), (ids.dtype, ids.shape, R, mode)
        assert flag == int(bad), (ids.dtype, ids.shape, R, mode, flag)
        if public:
            if bad:
                with pytest.raises(IndexError):
                    lib.bincount(di, R, mode=mode)
            else:
                res = lib.bincount(di, R, mode=mode)
                assert res.shape == (R,) and res.dtype == np.int64 and np.array_equal(res.numpy(), want)


@pytest.mark.parametrize("dtype", (np.int32, np.int64), **IDS)
def test_bincount_bins_and_lengths(smhip, dtype):
    lib = smhip
    K = constants(lib)[0]
    k = 0
    for R in (1, 2, 255, 256, 257, K, K + 1, 4 * K + 3):
        route = LDS if R <= K else GLOBAL
        for n in N_LIST:
            ids = make_ids(KINDS[k % len(KINDS)], n, R, dtype, k)
            di = off_by_one(lib, ids) if k % 4 == 1 else None
            check_bincount(lib, ids, R, modes=(MODES[k % 3],), di=di, route=route, public=k % 5 == 0, misalign=k % 2)
            k += 1
    for R in (256, K + 1):  # every kind in every mode
        for kind in KINDS:
            check_bincount(lib, make_ids(kind, 5003, R, dtype, 3), R, route=LDS if R <= K else GLOBAL, public=False)


@pytest.mark.parametrize("dtype", (np.int32, np.int64), **IDS)
def test_bincount_trouble_ids(smhip, dtype):
    """R, -R - 1, the type's extremes, 2^32 and its neighbours: the guard thirds stay intact (Guarded asserts it), CHECKED drops
    exactly the bad ids, counts the valid ones, sets the flag and raises IndexError."""
    lib = smhip
    K = constants(lib)[0]
    for R in (1, 70, 256, K, K + 1, 3 * K):
        for n in (9, 200, 70001):
            ids = trouble_ids(n, R, dtype, R + n)
            assert expected_counts(ids, R, "checked")[1]
            check_bincount(lib, ids, R, route=LDS if R <= K else GLOBAL)


def test_an_all_valid_call_clears_a_garbage_flag(smhip):
    K = constants(smhip)[0]
    for R in (9, K + 1):
        ids = make_ids("edges", 1000, R, np.int64, 1)
        _, flag = raw_bincount(smhip, smhip.to_device(ids), R, "checked")
        assert flag == 0
        assert raw_bincount(smhip, smhip.to_device(ids[:0]), R, "checked")[1] == 0  # ... and a call without ids


def test_every_entry_in_one_bin(smhip):
    lib = smhip
    K = constants(lib)[0]
    n = 1 << 20
    for R in (1, 256, K, K + 1):
        for dtype in (np.int32, np.int64):
            ids = np.full(n, R - 1 if R > 1 else 0, dtype)
            want = np.zeros(R, np.int64)
            want[ids[0]] = n
            assert np.array_equal(lib.bincount(lib.to_device(ids), R, mode="clip").numpy(), want), (R, dtype)
    x = np.full(n, 0.25, np.float32)
    for bins in (256, K + 1):
        counts, _ = lib.histogram(lib.to_device(x), bins, range=(0, 1))
        assert counts.numpy()[bins // 4] == n and int(counts.numpy().sum()) == n


def test_bincount_equals_index_add_of_ones(smhip):
    """The contract: bit for bit index_add(zeros, ids, 1, 0, mode), trouble ids included, through the two C entry points."""
    lib = smhip
    K = constants(lib)[0]
    one = lib.to_device(np.ones(1, np.int64))
    for shape, R in (((5000,), 256), ((70, 300), K + 1), ((3, 41, 17), 70)):
        n = int(np.prod(shape))
        for ids in (make_ids("heavy", n, R, np.int64, 2), trouble_ids(n, R, np.int64, 3)):
            ids = ids.reshape(shape)
            di = lib.to_device(ids)
            for mode in MODES:
                got, flag = raw_bincount(lib, di, R, mode)
                target = Guarded(lib, R)
                lib.upload(target.ptr, np.zeros(R, np.int64))
                bad = lib.to_device(np.array([GARBAGE], np.int64))
                rc = lib.scatter_raw(sma.SCATTER_ADD, sma.INDEX_MODES[mode], 0, sma.I64, target.ptr, [R], 0, di.ptr, [1], one.ptr, [0], n, bad.ptr)
                assert rc == 0, lib.c.smhip_last_error().decode()
                assert got.tobytes() == target.result().tobytes(), (shape, R, mode)
                assert flag == int(bad.numpy()[0])
        ids = make_ids("random", n, R, np.int64, 4).reshape(shape)  # the public forms
        for mode in MODES:
            want = lib.index_add(lib.full((R,), 0, np.int64), lib.to_device(ids.reshape(-1)), 1, 0, mode=mode).numpy()
            assert lib.bincount(lib.to_device(ids), R, mode=mode).numpy().tobytes() == want.tobytes()


def test_bincount_of_views(smhip):
    lib = smhip
    K = constants(lib)[0]
    for dtype in (np.int32, np.int64):
        base = make_ids("random", 60 * 90, 300, dtype, 1).reshape(60, 90)
        db = lib.to_device(base)
        for view in (base.T, base[::2, 1::3]):
            for R in (300, K + 1):
                check_bincount(lib, view, R, di=db.view_like(view, base), route=(LDS if R <= K else GLOBAL) | COPY)
        check_bincount(lib, base, 300, route=LDS)


# ---------------------------------------------------------------------------------------------- histogram
def rule_counts(x, edges):
    """The rule of the contract written out: searchsorted(right) - 1, the last edge in the last bin, everything else outside dropped."""
    x = x.reshape(-1)
    bins = edges.size - 1
    at = np.searchsorted(edges, x, "right").astype(np.int64) - 1
    at[x == edges[-1]] = bins - 1
    keep = (at >= 0) & (at < bins)
    if x.dtype.kind == "f":
        keep &= ~np.isnan(x)
    return np.bincount(at[keep], minlength=bins).astype(np.int64)


def histogram_input(dtype, edges, n, seed):
    """n values that hold every edge, the float just below every edge, NaN and both infinities among random ones around the range."""
    rng = np.random.default_rng(seed)
    lo, hi = float(edges[0]), float(edges[-1])
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=n).astype(dtype)
    pool = np.concatenate([edges, np.nextafter(edges, np.dtype(dtype).type(-np.inf)), np.array([np.nan, np.inf, -np.inf], dtype)]).astype(dtype)
    x[rng.permutation(n)[:pool.size]] = pool
    return x


def raw_histogram(lib, flags, dx, de, bins, lo=0.0, hi=0.0, misalign=0):
    out = Guarded(lib, bins, misalign)
    rc = lib.histogram_raw(flags, sma.DTYPES[dx.dtype], dx.ptr, dx.shape, dx.strides, de.ptr, bins, lo, hi, out.ptr)
    assert rc == 0, lib.c.smhip_last_error().decode()
    return out.result()


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_histogram_over_a_range(smhip, dtype):
    lib = smhip
    K = constants(lib)[0]
    n = 200001
    for k, (lo, hi, bins) in enumerate(UNIFORM_CASES):
        edges = np.linspace(lo, hi, bins + 1).astype(dtype)
        x = histogram_input(dtype, edges, n, k)
        dx = lib.to_device(x)
        assert route_of(lib, "histogram", dx, bins, uniform=True) == (LDS if bins <= K else GLOBAL)
        counts, got_edges = lib.histogram(dx, bins, range=(lo, hi))
        assert got_edges.numpy().tobytes() == edges.tobytes(), (lo, hi, bins)
        got = counts.numpy()
        want, numpys_edges = np.histogram(x, bins, range=(lo, hi))
        assert numpys_edges.astype(dtype).tobytes() == edges.tobytes()
        assert np.array_equal(got, want), (lo, hi, bins)
        assert np.array_equal(got, np.histogram(x, bins=edges)[0]), (lo, hi, bins)
        assert np.array_equal(got, rule_counts(x, edges)), (lo, hi, bins)
        assert int(got.sum()) == int(((x >= edges[0]) & (x <= edges[-1])).sum())
        # the explicit-edges form of the same table, and the raw uniform call next to sentinels
        assert np.array_equal(lib.histogram(dx, got_edges).numpy(), want), (lo, hi, bins)
        assert np.array_equal(raw_histogram(lib, sma.HISTOGRAM_UNIFORM, dx, got_edges, bins, lo, hi, misalign=k % 2), want)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_histogram_over_one_point_and_refusals(smhip, dtype):
    lib = smhip
    x = np.array([2.5, 3.0, 3.0, 3.4999, 3.5, 3.6, 2.4, np.nan], dtype)
    dx = lib.to_device(x)
    counts, edges = lib.histogram(dx, 4, range=(3.0, 3.0))
    want, want_edges = np.histogram(x, 4, range=(3.0, 3.0))
    assert np.array_equal(counts.numpy(), want) and edges.numpy().tobytes() == want_edges.astype(dtype).tobytes()
    for lo, hi, bins in ((1, 0, 4), (0, np.inf, 4), (np.nan, 1, 4), (0, 1, 0), (0, 1, -1)):
        with pytest.raises(ValueError):
            lib.histogram(dx, bins, range=(lo, hi))
    if dtype == np.float32:
        with pytest.raises(ValueError):
            lib.histogram(dx, 64, range=(1.0, 1.0 + 2.0 ** -20))
    with pytest.raises(ValueError):
        lib.histogram(dx, 4)
    with pytest.raises(ValueError):
        lib.histogram(dx, lib.to_device(np.zeros(1, dtype)))
    with pytest.raises(ValueError):
        lib.histogram(dx, lib.to_device(np.zeros(3, np.int32)))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_histogram_with_explicit_edges(smhip, dtype):
    lib = smhip
    K, budgets = constants(lib)
    budget = budgets[np.dtype(dtype)]
    rng = np.random.default_rng(11)
    floating = np.dtype(dtype).kind == "f"
    for k, bins in enumerate((1, 2, 7, 255, 1000, budget - 1, budget, K, K + 1, 3 * K + 1)):
        if floating:
            edges = np.sort(np.round(rng.uniform(-50, 50, size=bins + 1), 1 if bins < 1000 else 3)).astype(dtype)  # rounding leaves repeats
        else:
            edges = np.sort(rng.integers(-bins, bins + 1, size=bins + 1)).astype(dtype)                           # integer edges with repeats
        for n in (5, 1025, 70001):
            if floating:
                x = histogram_input(dtype, edges, max(n, 2 * edges.size + 3), k) if n > 1025 else rng.uniform(-60, 60, size=n).astype(dtype)
            else:
                x = rng.integers(-bins - 5, bins + 6, size=n).astype(dtype)
                x[: min(n, edges.size)] = edges[: min(n, edges.size)]
            dx = lib.to_device(x)
            assert route_of(lib, "histogram", dx, bins) == (LDS if bins <= K else GLOBAL)
            got = raw_histogram(lib, 0, dx, lib.to_device(edges), bins, misalign=k % 2)
            assert np.array_equal(got, rule_counts(x, edges)), (dtype, bins, n)
            assert np.array_equal(got, np.histogram(x, bins=edges)[0]), (dtype, bins, n)
            assert np.array_equal(lib.histogram(off_by_one(lib, x), lib.to_device(edges)).numpy(), got)
    if not floating:  # the type's extremes as values and as edges: the rule alone is the oracle
        info = np.iinfo(dtype)
        edges = np.array([info.min, info.min + 1, -3, -3, 0, 7, info.max - 1, info.max], dtype)
        x = np.concatenate([edges, edges, np.array([info.min, info.max, -4, -2, 6, 8], dtype), rng.integers(info.min, info.max, size=5000, dtype=dtype)])
        got = lib.histogram(lib.to_device(x), lib.to_device(edges)).numpy()
        assert np.array_equal(got, rule_counts(x, edges)) and int(got.sum()) == x.size


@pytest.mark.parametrize("dtype", (np.float32, np.int64), **IDS)
def test_histogram_of_views(smhip, dtype):
    lib = smhip
    K = constants(lib)[0]
    rng = np.random.default_rng(5)
    base = (rng.uniform(-6, 6, size=(60, 90)) * (1 if np.dtype(dtype).kind == "f" else 100)).astype(dtype)
    db = lib.to_device(base)
    for view in (base.T, base[1::2, ::3]):
        dv = db.view_like(view, base)
        for bins in (16, K + 1):
            if np.dtype(dtype).kind == "f":
                assert route_of(lib, "histogram", dv, bins, uniform=True) == (LDS if bins <= K else GLOBAL) | COPY
                counts, edges = lib.histogram(dv, bins, range=(-5, 5))
                assert np.array_equal(counts.numpy(), np.histogram(view, bins, range=(-5, 5))[0])
            else:
                edges = lib.to_device(np.arange(-bins, bins + 1, 2, dtype=dtype)[: bins + 1])
                counts = lib.histogram(dv, edges)
            assert np.array_equal(lib.histogram(dv, edges).numpy(), rule_counts(np.ascontiguousarray(view), edges.numpy()))
            assert np.array_equal(counts.numpy(), rule_counts(np.ascontiguousarray(view), edges.numpy()))


# ---------------------------------------------------------------------------------------------- determinism, grid cap, empties
def every_route(lib):
    """{name: bytes of the result} of one call on every route of the family."""
    K, budgets = constants(lib)
    rng = np.random.default_rng(7)
    n = 300007
    out = {}
    ids = make_ids("heavy", n, 4 * K, np.int64, 1)
    di = lib.to_device(ids)
    x = rng.standard_normal(n).astype(np.float32)
    dx = lib.to_device(x)
    for R in (256, K + 1):
        assert route_of(lib, "bincount", di, R) == (LDS if R <= K else GLOBAL)
        out[f"bincount {R}"] = lib.bincount(di, R, mode="wrap").numpy().tobytes()
        out[f"uniform {R}"] = lib.histogram(dx, R, range=(-3, 3))[0].numpy().tobytes()
        edges = np.sort(rng.standard_normal(R + 1)).astype(np.float32)
        out[f"edges {R}"] = lib.histogram(dx, lib.to_device(edges)).numpy().tobytes()
    for E in (1000, budgets[np.dtype(np.float32)] + 1):
        edges = np.sort(rng.standard_normal(E)).astype(np.float32)
        out[f"searchsorted {E}"] = lib.searchsorted(lib.to_device(edges), dx, "right").numpy().tobytes()
    return out


def test_same_bits_on_every_run_and_stream(smhip):
    first, second = every_route(smhip), every_route(smhip)
    assert first == second
    smhip.synchronize()
    hip = smhip.c  # the HIP runtime libsmhip.so itself is linked against (dlsym follows its dependencies)
    stream = C.c_void_p(0)
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        smhip.set_stream(stream.value)
        third = every_route(smhip)
        smhip.synchronize()
    finally:
        smhip.set_stream(0)
        # the ring that small uploads go through remembers the stream of its last use and waits for it when the stream changes:
        # one upload on the library's stream moves it there while the caller's stream still exists
        smhip.to_device(np.zeros(256, np.float32))
        smhip.synchronize()
        hip.hipStreamDestroy(stream)
    assert third == first


_CAPPED = """
import numpy as np, simplemath_amd as sma
from tests.test_count_gpu import (check_searchsorted, check_bincount, make_edges, probes, make_ids, trouble_ids, off_by_one, constants, rule_counts,
                                  histogram_input, LDS, GLOBAL, COPY)
lib = sma.load()
lib.set_device(0)
K, budgets = constants(lib)
assert lib.count_plan("bincount", np.int64, [1 << 24], [1], 256)[2][0] == 2        # the cap holds
for dtype in (np.float32, np.float64, np.int32, np.int64):
    budget = budgets[np.dtype(dtype)]
    for E in (65, budget + 1):                                                     # searchsorted: edges in LDS and in global memory
        edges = make_edges(dtype, E, E)
        for n in (5, 70001, 70002):
            x = probes(dtype, edges, n, n)
            check_searchsorted(lib, edges, x, route=LDS if E <= budget else GLOBAL)
            check_searchsorted(lib, edges, x, dx=off_by_one(lib, x), misalign=1)   # head and tail
    base = probes(dtype, edges, 60 * 90, 3).reshape(60, 90)
    check_searchsorted(lib, edges, base.T, dx=lib.to_device(base).view_like(base.T, base), route=GLOBAL | COPY)
    for bins in (16, K, K + 1):                                                    # histogram with explicit edges
        edges = np.sort(np.random.default_rng(bins).integers(-900, 900, size=bins + 1)).astype(dtype)
        x = np.random.default_rng(1).integers(-1000, 1000, size=150001).astype(dtype)
        for dx in (lib.to_device(x), off_by_one(lib, x)):
            assert np.array_equal(lib.histogram(dx, lib.to_device(edges)).numpy(), rule_counts(x, edges)), (dtype, bins)
for dtype in (np.float32, np.float64):                                             # ... and over a range
    for lo, hi, bins in ((-3, 5, 256), (-1e3, 1e3, K + 1)):
        x = histogram_input(dtype, np.linspace(lo, hi, bins + 1).astype(dtype), 200001, bins)
        for dx in (lib.to_device(x), off_by_one(lib, x)):
            assert np.array_equal(lib.histogram(dx, bins, range=(lo, hi))[0].numpy(), np.histogram(x, bins, range=(lo, hi))[0]), (dtype, bins)
        base = x[:180000].reshape(300, 600)
        got = lib.histogram(lib.to_device(base).view_like(base.T, base), bins, range=(lo, hi))[0].numpy()
        assert np.array_equal(got, np.histogram(base, bins, range=(lo, hi))[0])
for dtype in (np.int32, np.int64):                                                 # bincount
    for R in (2, 256, K, K + 1):
        route = LDS if R <= K else GLOBAL
        check_bincount(lib, make_ids("heavy", 150001, R, dtype, 1), R, route=route)
        ids = trouble_ids(70003, R, dtype, 2)
        check_bincount(lib, ids, R, di=off_by_one(lib, ids), route=route)
        base = make_ids("random", 60 * 90, R, dtype, 3).reshape(60, 90)
        check_bincount(lib, base.T, R, di=lib.to_device(base).view_like(base.T, base), route=route | COPY)
print("capped grid ok")
"""


def test_every_route_with_a_capped_grid(smhip):
    """SMHIP_COUNT_GRID_CAP=2: every grid-stride loop runs many times per workgroup -- both routes of the three operations, COPY,
    and operands whose first element is not 16-byte aligned (the head and tail paths)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMHIP_COUNT_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CAPPED], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "capped grid ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_empty_cases(smhip):
    lib = smhip
    K = constants(lib)[0]
    keep = lib.to_device(np.zeros(1, np.int64))

    def hollow(dtype, shape):
        return sma.DeviceArray(lib, keep.base_ptr, dtype, shape, dense(shape), 0, keep._owner)

    for R in (5, K + 1):  # no ids: zeros, not garbage
        for shape in ((0,), (4, 0, 3)):
            assert np.array_equal(lib.bincount(hollow(np.int64, shape), R).numpy(), np.zeros(R, np.int64))
            counts, edges = lib.histogram(hollow(np.float32, shape), R, range=(0, 1))
            assert np.array_equal(counts.numpy(), np.zeros(R, np.int64)) and edges.shape == (R + 1,)
            assert np.array_equal(lib.histogram(hollow(np.float32, shape), edges).numpy(), np.zeros(R, np.int64))
    assert lib.bincount(hollow(np.int64, (0,)), 0).shape == (0,)
    with pytest.raises(ValueError):
        lib.bincount(lib.to_device(np.zeros(3, np.int64)), 0)
    edges = lib.to_device(np.arange(4, dtype=np.float32))
    assert lib.searchsorted(edges, hollow(np.float32, (0,))).shape == (0,)
    assert lib.searchsorted(edges, hollow(np.float32, (3, 0))).shape == (3, 0)
    none = hollow(np.float32, (0,))
    x = lib.to_device(np.array([-1.0, 0.0, np.nan], np.float32))
    for side in ("left", "right"):
        assert lib.searchsorted(none, x, side).numpy().tolist() == [0, 0, 0]  # no edges: zeros
