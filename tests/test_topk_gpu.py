"""topk along an axis on the GPU (smhip_topk_axis through the ctypes binding), bit for bit against the first k of numpy's stable order
(tests/test_sort_gpu.py's reference(), sliced) and against the library's own sort: f32, f64, i32 and i64, both orders, values and
positions together and each alone.

Every check is exact: the pairs of a line are totally ordered, so the first k are one set in one order.  L (the longest line a
selection holds in LDS) and kmax (the largest k it takes) are read from the plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma
from tests.test_sort_gpu import continuous, reference, specials, ties

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
IDS = dict(ids=lambda d: np.dtype(d).name)
MODES = ("both", "values", "indices")
KINDS = (continuous, ties, specials)


def limits(lib, dtype):
    _, _, _, info = lib.topk_plan(dtype, [1 << 20], [1], 0, 1)
    return info[0], info[1]


def first_k(x, k, axis, largest):
    """(values, positions): the first k along `axis` of the stable order of the host array x."""
    v, i = reference(x, axis, largest)
    return np.ascontiguousarray(np.take(v, range(k), axis)), np.ascontiguousarray(np.take(i, range(k), axis))


def topk(lib, d, k, axis, largest, mode="both"):
    """(values, positions) as host arrays; the one not asked for is None (each alone goes through the raw call)."""
    if mode == "both":
        v, i = lib.topk(d, k, axis, largest)
        return v.numpy(), i.numpy()
    axis = axis % d.ndim
    shape = d.shape[:axis] + (k,) + d.shape[axis + 1:]
    v = lib.empty(shape, d.dtype) if mode == "values" else None
    i = lib.empty(shape, np.int64) if mode == "indices" else None
    lib._ck(lib.topk_raw(sma.SORT_DESCENDING if largest else sma.SORT_ASCENDING, sma.DTYPES[d.dtype], d.ptr, d.shape, d.strides, axis, k,
                         v.ptr if v is not None else 0, i.ptr if i is not None else 0))
    return (v.numpy() if v is not None else None), (i.numpy() if i is not None else None)


def same(got, want, what):
    got_v, got_i = got
    want_v, want_i = want
    if got_i is not None:
        assert got_i.dtype == np.int64 and got_i.shape == want_i.shape and np.array_equal(got_i, want_i), what
    if got_v is not None:
        assert got_v.dtype == want_v.dtype and got_v.shape == want_v.shape and got_v.tobytes() == want_v.tobytes(), what


def check(lib, x, d, ks, axis, mode="both", orders=(False, True)):
    """`d` holds `x` (a host array or view) on the device; one reference per order, sliced for every k."""
    for largest in orders:
        v, i = reference(x, axis, largest)
        for n, k in enumerate(ks):
            want = np.ascontiguousarray(np.take(v, range(k), axis)), np.ascontiguousarray(np.take(i, range(k), axis))
            m = MODES[(MODES.index(mode) + n) % 3]
            same(topk(lib, d, k, axis, largest, m), want, (x.dtype, x.shape, axis, k, largest, m))


def lengths(L):
    r = sma.TOPK_RANKED  # the longest line that is ranked, not selected from
    return (1, 2, 3, 63, 64, 65, r - 1, r, r + 1, 255, 256, 257, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17)


def some_k(R, kmax):
    return sorted({min(k, R) for k in (1, 2, 5, 63, 64, 65, R // 2, R // 2 + 1, kmax - 1, kmax, kmax + 1, R - 1, R)} - {0})  # (2k > R: the sort)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_lengths_and_k(smhip, dtype):
    """Every length and k at which the code takes another path: a wave or a workgroup per line, the network's sizes, one tile, two and
    three levels, kmax and the sort behind it."""
    L, kmax = limits(smhip, dtype)
    for n, R in enumerate(lengths(L)):
        x = KINDS[n % 3]((3, R), dtype, 100 + n)
        check(smhip, x, smhip.to_device(x), some_k(R, kmax), 1, MODES[n % 3])


def line_of(dtype, values):
    return np.array(values).astype(dtype).reshape(1, -1)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_constant_and_tied_lines(smhip, dtype):
    """Pivot ties across tiles and levels: the first k positions of a constant line, also through a stride-0 view; a line whose only
    distinct value sits at the last position."""
    L, kmax = limits(smhip, dtype)
    R = 2 * L + 1
    const = np.full((2, R), 7, dtype)
    d = smhip.to_device(const)
    one = smhip.to_device(np.full((2, 1), 7, dtype))
    broadcast = sma.DeviceArray(smhip, one.base_ptr, dtype, (2, R), (1, 0), 0, one._owner)
    for k in (5, kmax):
        for largest in (False, True):
            for operand in (d, broadcast):
                v, i = topk(smhip, operand, k, 1, largest)
                assert np.array_equal(i, np.broadcast_to(np.arange(k), (2, k))) and v.tobytes() == const[:, :k].tobytes()
    for R in (300, L, 2 * L + 1):
        x = np.full((2, R), 3, dtype)
        x[0, -1], x[1, -1] = 9, -9
        check(smhip, x, smhip.to_device(x), (1, 5, min(R, kmax)), 1)


@pytest.mark.parametrize("dtype", (np.float32, np.float64), **IDS)
def test_zeros_and_nans(smhip, dtype):
    L, kmax = limits(smhip, dtype)
    u = np.uint32 if dtype == np.float32 else np.uint64
    sign = 31 if dtype == np.float32 else 63
    for R in (300, 2 * L + 1):
        # +0 / -0 interleaved, starting with either: the zero at position 0 comes first, with its own sign bit
        for lead in (0, 1):
            bits = (((np.arange(R, dtype=np.uint64) + np.uint64(lead)) % np.uint64(2)) << np.uint64(sign)).astype(u).reshape(1, R)
            x = bits.view(dtype)
            for largest in (False, True):
                v, i = topk(smhip, smhip.to_device(x), 5, 1, largest)
                assert np.array_equal(i[0], np.arange(5)) and v.view(u).tobytes() == bits[:, :5].tobytes()
        # mostly NaN, every one with a payload of its own and both signs; k below and above the number of NaNs
        rng = np.random.default_rng(R)
        x = rng.standard_normal((2, R)).astype(dtype)
        bits = x.view(u)
        nans = rng.permutation(R)[: R - 40]
        exp_all = (u(0x7F800000) if dtype == np.float32 else u(0x7FF0000000000000))
        bits[:, nans] = exp_all | (np.arange(nans.size, dtype=u) + u(1)) | ((np.arange(nans.size, dtype=np.uint64) % np.uint64(2)) << np.uint64(sign)).astype(u)
        assert np.isnan(x).sum() == 2 * (R - 40)
        ks = sorted({5, 39, 40, 41, R - 41, R - 40, R - 39, min(R - 1, kmax)})
        check(smhip, x, smhip.to_device(x), ks, 1)


def test_digit_boundaries_and_extremes(smhip):
    """Lines whose elements differ only in the lowest byte, and only in the highest: every digit pass of the 8-byte keys decides.
    INT_MIN / INT_MAX, +-inf and subnormals at the ends of the order."""
    rng = np.random.default_rng(7)
    for R in (300, 5000):
        low = rng.integers(0, 256, size=(2, R)).astype(np.uint64)
        high = rng.integers(0, 256, size=(2, R)).astype(np.uint64) << np.uint64(56)
        mid = np.uint64(0x0012345678ABCD00)
        for bits in (low | mid, high | (mid >> np.uint64(8)), low | mid | np.uint64(1 << 63), high):
            x = bits.view(np.int64)
            check(smhip, x, smhip.to_device(x), (1, 7, 200), 1)
            f = bits.view(np.float64)
            if not np.isnan(f).any():
                check(smhip, f, smhip.to_device(f), (1, 7, 200), 1)
    for dtype in (np.int32, np.int64):
        info = np.iinfo(dtype)
        x = line_of(dtype, [0, info.max, info.min, -1, info.max, info.min, 1, info.min + 1, info.max - 1] * 40)
        check(smhip, x, smhip.to_device(x), (1, 41, 81, 200), 1)
    for dtype in (np.float32, np.float64):
        tiny = np.finfo(dtype).smallest_subnormal
        x = line_of(dtype, [0.0, np.inf, -np.inf, tiny, -tiny, 1.0, -0.0, np.finfo(dtype).max, np.finfo(dtype).tiny, -np.inf, np.inf] * 40)
        check(smhip, x, smhip.to_device(x), (1, 41, 81, 200), 1)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_against_the_librarys_own_sort(smhip, dtype):
    """topk(d, k, axis) is the first k of sort(d, axis, descending, indices=True), byte for byte: one shape per route."""
    L, kmax = limits(smhip, dtype)
    for shape, axis, k in (((1031, 37), 1, 5), ((9, L), 1, 64), ((3, 2 * L + 1), 1, kmax), ((2, 5 * L + 17), 1, kmax), ((70, 50), 0, 5), ((3, 3 * kmax), 1, kmax + 1)):
        x = specials(shape, dtype, 21)
        d = smhip.to_device(x)
        for largest in (False, True):
            sv, si = smhip.sort(d, axis, largest, indices=True)
            want = np.ascontiguousarray(np.take(sv.numpy(), range(k), axis)), np.ascontiguousarray(np.take(si.numpy(), range(k), axis))
            same(topk(smhip, d, k, axis, largest), want, (shape, axis, k, largest))
            first = np.take(want[1], 0, axis)
            if largest:
                assert np.array_equal(first, smhip.argreduce("argmax", d, axis).numpy())


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views_and_axes(smhip, dtype):
    L, kmax = limits(smhip, dtype)
    base = ties((70, 130), dtype, 3)
    d = smhip.to_device(base)
    for n, viewf in enumerate((lambda b: b.T, lambda b: b[::2, 1::3], lambda b: b[3:60, 5:100])):
        v = viewf(base)
        dv = d.view_like(v, base)
        for axis in range(v.ndim):
            check(smhip, v, dv, (1, 5, v.shape[axis]), axis, MODES[(n + axis) % 3])
    cube = specials((5, 33, 7), dtype, 4)
    dc = smhip.to_device(cube)
    for axis in (0, 1, -1):
        check(smhip, cube, dc, (1, 4), axis)
    long = specials((3, 2 * L + 5), dtype, 5)  # a transposed operand with TILED inside, and a stepped one
    dl = smhip.to_device(long)
    check(smhip, long.T, dl.view_like(long.T, long), (5, kmax), 0)
    check(smhip, long[:, ::2], dl.view_like(long[:, ::2], long), (5,), 1)


def test_flattened_out_arguments_and_nothing_to_do(smhip):
    x = specials((37, 130), np.float32, 8)
    d = smhip.to_device(x)
    for largest in (False, True):
        v, i = smhip.topk(d, 9, None, largest)
        assert v.shape == i.shape == (9,)
        same((v.numpy(), i.numpy()), first_k(x.reshape(-1), 9, 0, largest), largest)
        t = d.view_like(x.T, x)  # a view without an axis: its own row-major order
        v, i = smhip.topk(t, 9, None, largest)
        same((v.numpy(), i.numpy()), first_k(np.ascontiguousarray(x.T).reshape(-1), 9, 0, largest), largest)
    out_v, out_i = smhip.empty((4, 130), np.float32), smhip.empty((4, 130), np.int64)
    v, i = smhip.topk(d, 4, 0, out=out_v, index_out=out_i)
    assert v is out_v and i is out_i
    same((out_v.numpy(), out_i.numpy()), first_k(x, 4, 0, True), "out")
    one = smhip.to_device(x[:, :1].copy())  # an axis of one element: the values copied, zeros
    v, i = smhip.topk(one, 1, 1)
    assert v.numpy().tobytes() == x[:, :1].tobytes() and not i.numpy().any()
    v, i = smhip.topk(d, 0, 1)
    assert v.shape == i.shape == (37, 0)
    e = smhip.empty((4, 0, 3), np.float32)
    for axis, k in ((0, 2), (1, 0), (2, 3)):
        v, i = smhip.topk(e, k, axis)
        assert v.shape == i.shape == tuple(k if a == axis else n for a, n in enumerate((4, 0, 3)))


def test_same_bits_on_every_run(smhip):
    x = specials((3, 20000), np.float32, 15)
    d = smhip.to_device(x)
    runs = [tuple(r.tobytes() for r in topk(smhip, d, 700, 1, True)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


_ROUTES = """
import sys, numpy as np, simplemath_amd as sma
from tests.test_sort_gpu import ties, specials
from tests.test_topk_gpu import limits, topk
lib = sma.load()
lib.set_device(0)
with open(sys.argv[1], "wb") as out:
    for dtype in (np.float32, np.float64, np.int32, np.int64):
        L, kmax = limits(lib, dtype)
        # ROW with a ranking and a selecting wave per line, ROW with a workgroup per line and at L, TILED with 2 and 3 levels, COPY, SORT
        cases = [((1031, 37), 1, 5), ((517, 100), 1, 70), ((300, 200), 1, 5), ((301, 600), 1, kmax // 4 + 1), ((9, L), 1, 64), ((3, 2 * L + 1), 1, kmax), ((2, 5 * L + 17), 1, kmax),
                 ((70, 50), 0, 5), ((3, 3 * kmax), 1, kmax + 1)]
        for i, (shape, axis, k) in enumerate(cases):
            for x in (ties(shape, dtype, 40 + i), specials(shape, dtype, 50 + i)):
                for largest in (False, True):
                    for r in topk(lib, lib.to_device(x), k, axis, largest):
                        out.write(r.tobytes())
print("routes ok")
"""


def test_every_route_with_a_capped_grid(smhip, tmp_path):
    """SMHIP_TOPK_GRID_CAP=2 in a fresh process: every kernel's loop over its tasks runs many times per workgroup; the bytes are those
    of the uncapped run of the same script."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for cap in ("", "2"):
        path = str(tmp_path / ("capped" if cap else "plain"))
        env = dict(os.environ, SMHIP_TOPK_GRID_CAP=cap, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", _ROUTES, path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "routes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        with open(path, "rb") as f:
            got[cap] = f.read()
    assert len(got[""]) > 1 << 16 and got[""] == got["2"]


def test_past_2p31_elements(smhip):
    """f32 (2, 2^30 + 17) along the last axis, k = 8: TILED over a flat offset past 2^31.  The array is filled on the device with
    uniform values in [0, 1); 16 values 2.0 + j are put at chosen positions of line 1 -- its first element, the positions either side
    of flat element 2^31, its last -- and the call must return exactly the 8 largest of them and where they stand.  Nothing large is
    downloaded; line 0 is checked only for values < 1.  Peak device memory: 8 GiB for the operand plus 64 MiB of candidates and
    the results."""
    lib = smhip
    R, k = (1 << 30) + 17, 8
    buf = lib.uniform_f32(2 * R, 77, 0.0, 1.0)
    a = ids = vals = v = i = None
    try:
        a = sma.DeviceArray(lib, buf.base_ptr, np.float32, (2, R), (R, 1), 0, buf._owner)
        L, _ = limits(lib, np.float32)
        edge = (1 << 31) - R  # the position along line 1 of flat element 2^31
        spots = np.array([0, edge - 1, edge, edge + 1, R - 1, 1, L - 1, L, L + 1, 5 * L + 17, 12345678, (1 << 29) + 3, R - 2, R - L, 777, edge - L], np.int64)
        assert len(set(spots.tolist())) == 2 * k and spots.min() == 0 and spots.max() == R - 1
        rng = np.random.default_rng(5)
        planted = (2.0 + rng.permutation(2 * k)).astype(np.float32)
        ids, vals = lib.to_device(spots + R), lib.to_device(planted)
        lib.put(buf, ids, vals, axis=None, unique=True)
        v, i = lib.topk(a, k, 1, True)
        v, i = v.numpy(), i.numpy()
        order = np.argsort(-planted, kind="stable")[:k]
        assert np.array_equal(v[1], planted[order]) and np.array_equal(i[1], spots[order])
        assert (v[0] < 1).all() and (v[0] >= 0).all() and (np.diff(v[0]) <= 0).all() and ((i[0] >= 0) & (i[0] < R)).all()
    finally:
        a = buf = ids = vals = v = i = None  # the blocks go back to the pool, and the pool to the device
        lib.pool_trim()
