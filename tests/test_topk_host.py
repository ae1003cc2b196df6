"""topk without a device: the planner (smhip_topk_plan through the binding), what smhip_topk_axis and smhip_topk_plan refuse, and the
binding's ValueErrors.

L (the longest line a selection holds in LDS) and kmax (the largest k it takes) are read from the plan, never written here.  The
refusals are pinned as literals in this file: the return code and the FULL message.  They are replayed only without a device (the
pointers are made-up integers), like tests/test_abi_errors_host.py."""
import numpy as np
import pytest

import simplemath_amd as sma

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
A, B, C = 1 << 20, 2 << 20, 3 << 20  # stand-ins for device pointers: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from simplemath_amd import build
    build.build_lib()
    return sma.load()


def limits(lib, dtype):
    _, _, _, info = lib.topk_plan(dtype, [1 << 20], [1], 0, 1)
    return info[0], info[1]


def levels(R, k, L):
    """Selection launches of a line of R: a level turns every tile of L into min(k, its length) candidates, until one tile is left."""
    n, count = R, 1
    while n > L:
        tiles = -(-n // L)
        n = (tiles - 1) * k + min(k, n - (tiles - 1) * L)
        count += 1
    return count


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_routes_and_launches_along_the_last_axis(lib, dtype):
    L, kmax = limits(lib, dtype)
    assert L >= 4 * kmax > 0  # every level shrinks a line at least fourfold
    for R in (1, 64, sma.TOPK_RANKED, sma.TOPK_RANKED + 1, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17):
        for k in sorted({min(k, R) for k in (0, 1, 5, R // 2, R // 2 + 1, kmax, kmax + 1, R)}):
            route, launches, ori, info = lib.topk_plan(dtype, [3, R], [R, 1], 1, k)
            assert ori == (3, R, 1) and info[:2] == (L, kmax)
            what = (R, k)
            if k == 0:
                assert (route, launches, info[2]) == (sma.TOPK_ROUTE_NONE, 0, 0), what
            elif R == 1:
                assert (route, launches, info[2]) == (sma.TOPK_ROUTE_COPYONLY, 2, 0), what
            elif k > kmax or (sma.TOPK_RANKED < R <= L and 2 * k > R):  # beyond a selection's reach, or one that keeps most of the line
                assert (route, launches, info[2]) == (sma.TOPK_ROUTE_SORT, lib.sort_plan(dtype, [3, R], [R, 1], 1)[1] + 2, 0), what
            elif R <= L:
                assert (route, launches, info[2]) == (sma.TOPK_ROUTE_ROW, 1, 1), what
            else:
                n = levels(R, k, L)
                assert n >= 2 and (route, launches, info[2]) == (sma.TOPK_ROUTE_ROW | sma.TOPK_TILED, n, n), what
            assert lib.topk_plan(dtype, [3, R], [R, 1], 1, k, largest=False) == (route, launches, ori, info)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_level_counts(lib, dtype):
    """The levels of TILED: the smallest count after which a line's candidates fit one tile (tiles * k shrunk to <= L)."""
    L, kmax = limits(lib, dtype)
    for R in (L + 1, 4 * L, 4 * L + 1, 16 * L + 1, 1 << 21, 1 << 24, (1 << 30) + 17):
        for k in (1, 5, kmax // 2 + 1, kmax):
            route, launches, _, info = lib.topk_plan(dtype, [R], [1], 0, k)
            assert route == sma.TOPK_ROUTE_ROW | sma.TOPK_TILED and info[2] == launches == levels(R, k, L) >= 2, (R, k)
    assert levels(2 * L + 1, kmax, L) == 2 and levels(5 * L + 17, kmax, L) == 3  # what the device tests call 2 and 3 levels


def test_views(lib):
    dtype = np.float32
    L, kmax = limits(lib, dtype)
    # axis 0 of a dense (70, 50): staged in, selected, two results scattered
    assert lib.topk_plan(dtype, [70, 50], [50, 1], 0, 5) == (sma.TOPK_ROUTE_ROW | sma.TOPK_COPY, 4, (1, 70, 50), (L, kmax, 1))
    # a transposed view along the axis with the unit stride in memory: read in place, its results scattered
    assert lib.topk_plan(dtype, [130, 70], [1, 130], 0, 5) == (sma.TOPK_ROUTE_ROW | sma.TOPK_COPY, 3, (70, 130, 1), (L, kmax, 1))
    # a stepped and a stride-0 view along the last axis: staged in, the rows are the results
    assert lib.topk_plan(dtype, [70, 65], [130, 2], 1, 5) == (sma.TOPK_ROUTE_ROW | sma.TOPK_COPY, 2, (70, 65, 1), (L, kmax, 1))
    assert lib.topk_plan(dtype, [9, 2 * L + 1], [1, 0], 1, 5) == (sma.TOPK_ROUTE_ROW | sma.TOPK_TILED | sma.TOPK_COPY, 3, (9, 2 * L + 1, 1), (L, kmax, 2))
    # SORT carries the sort's own staging
    srt = lib.sort_plan(dtype, [4 * kmax, 50], [50, 1], 0)
    assert srt[0] & sma.SORT_COPY
    assert lib.topk_plan(dtype, [4 * kmax, 50], [50, 1], 0, kmax + 1) == (sma.TOPK_ROUTE_SORT | sma.TOPK_COPY, srt[1] + 2, (1, 4 * kmax, 50), (L, kmax, 0))


def test_info_is_stable(lib):
    seen = {lib.topk_plan(dt, shape, strides, axis, k)[3][:2] for dt in (np.float32, np.int32) for shape, strides, axis, k in
            (([7], [1], 0, 0), ([7], [1], 0, 7), ([3, 5000], [5000, 1], 1, 2000), ([70, 50], [50, 1], 0, 1), ([0, 4], [4, 1], 1, 2))}
    assert len(seen) == 1
    seen = {limits(lib, dt) for dt in (np.float64, np.int64) for _ in range(3)}
    assert len(seen) == 1


INVALID, UNSUPPORTED = sma.ERR_INVALID, sma.ERR_UNSUPPORTED
BASE = dict(order=1, dtype=sma.F32, a_ptr=A, shape=[3, 7], strides=[7, 1], axis=1, k=5, values_ptr=B, index_ptr=C)
# one case per row of the contract's list; (what changes, the return code, the full message after "<entry point>: ")
CHECKS = [
    (dict(k=-1), INVALID, "k -1 outside 0..7"),
    (dict(k=8), INVALID, "k 8 outside 0..7"),
    (dict(order=2), INVALID, "bad order 2"),
    (dict(dtype=99), INVALID, "bad dtype 99"),
    (dict(ndim=0), INVALID, "ndim 0 outside 1..6"),
    (dict(axis=2), INVALID, "axis 2 outside 0..1"),
    (dict(axis=-1), INVALID, "axis -1 outside 0..1"),
    (dict(shape=[3, -7]), INVALID, "negative extent or stride at dim 1"),
    (dict(strides=[-7, 1]), INVALID, "negative extent or stride at dim 0"),
    (dict(shape=None, ndim=2), INVALID, "null shape/strides"),
    (dict(strides=None, ndim=2), INVALID, "null shape/strides"),
    (dict(shape=[3, 1 << 31], strides=[1 << 31, 1]), UNSUPPORTED, "an axis of 2147483648 elements (positions are 32 bits wide: below 2^31)"),
]
POINTERS = [  # smhip_topk_axis alone
    (dict(a_ptr=0), INVALID, "null operand"),
    (dict(values_ptr=0, index_ptr=0), INVALID, "neither values_out nor index_out is given"),
    (dict(index_ptr=B + 8), INVALID, "index_out overlaps the operand or values_out"),
    (dict(values_ptr=A), INVALID, "values_out overlaps the operand"),  # no in-place form
    (dict(values_ptr=A + 80), INVALID, "values_out overlaps the operand"),
    (dict(index_ptr=A + 80), INVALID, "index_out overlaps the operand or values_out"),
]


def test_refusals(lib):
    if lib.device_count():
        pytest.skip("a device is present: a call that got past its checks would launch on made-up pointers")
    for change, rc, msg in CHECKS + POINTERS:
        kw = dict(BASE, **change)
        assert lib.topk_raw(**kw) == rc, change
        assert lib.c.smhip_last_error().decode() == "topk_axis: " + msg, change
    for change, rc, msg in CHECKS:
        assert plan_raw(lib, dict(BASE, **change)) == rc, change
        assert lib.c.smhip_last_error().decode() == "topk_plan: " + msg, change
    # nothing to do is no refusal, whatever the pointers: k = 0, an extent of 0
    assert lib.topk_raw(**dict(BASE, k=0, a_ptr=0, values_ptr=0, index_ptr=0)) == 0
    assert lib.topk_raw(**dict(BASE, shape=[0, 7], a_ptr=0, values_ptr=0, index_ptr=0)) == 0
    assert lib.topk_raw(**dict(BASE, shape=[3, 0], strides=[0, 1], k=0, a_ptr=0, values_ptr=0, index_ptr=0)) == 0


def plan_raw(lib, kw):
    import ctypes as ct
    arr = lambda v: (ct.c_int64 * len(v))(*v) if v is not None else None
    ndim = kw.get("ndim", len(kw["shape"]) if kw["shape"] is not None else 2)
    return lib.c.smhip_topk_plan(ct.c_int(kw["order"]), ct.c_int(kw["dtype"]), arr(kw["shape"]), arr(kw["strides"]), ct.c_int(ndim), ct.c_int(kw["axis"]),
                                 ct.c_int64(kw["k"]), None, None, None, None)


class FakeArray(sma.DeviceArray):
    """A DeviceArray over no memory: the binding refuses before it asks for a pointer."""

    def __init__(self, dtype, shape, strides=None):
        dense, acc = [], 1
        for d in shape[::-1]:
            dense.append(acc)
            acc *= d
        super().__init__(None, A, dtype, shape, strides if strides is not None else dense[::-1], owner=object())


def test_the_bindings_value_errors(lib):
    a = FakeArray(np.float32, (3, 7))
    with pytest.raises(ValueError, match="dtype"):
        lib.topk(FakeArray(np.int16, (3, 7)), 2)
    for k in (-1, 8):
        with pytest.raises(ValueError, match="k %d outside 0..7" % k):
            lib.topk(a, k)
    with pytest.raises(ValueError, match="k 4 outside 0..3"):
        lib.topk(a, 4, axis=0)
    with pytest.raises(ValueError):
        lib.topk(a, 2, axis=2)
    for out in (FakeArray(np.float64, (3, 2)), FakeArray(np.float32, (3, 3)), FakeArray(np.float32, (3, 2), (4, 1))):  # dtype, size, density
        with pytest.raises(ValueError, match="topk: out must be a dense float32 array of 6 elements"):
            lib.topk(a, 2, out=out)
    for out in (FakeArray(np.int32, (3, 2)), FakeArray(np.int64, (2, 2)), FakeArray(np.int64, (3, 2), (2, 2))):
        with pytest.raises(ValueError, match="topk: index_out must be a dense int64 array of 6 elements"):
            lib.topk(a, 2, index_out=out)
