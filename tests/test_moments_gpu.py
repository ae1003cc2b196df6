"""var, std, var_mean and standardize on the GPU (smhip_moments_axes / smhip_standardize_axis through the ctypes binding), f32 and f64,
against an np.longdouble reference with the error bounds of include/smhip.h ("var / std / standardize"):

    VAR           (u_T + (N + 8) u) exact + tiny
    STD           (u_T + (N/2 + 8) u) exact + tiny
    standardize   (u_T + (N + 10) u) |y| + (N + 2) u max|x| / sqrt(var + eps) + tiny
    mean output   the bytes of reduce("mean", ...)

u = 2^-53, u_T = 2^-24 / 2^-53, tiny the smallest subnormal.  Every element of every result is compared; a line with a NaN or an
infinity must give NaN, a constant line exactly +0.  L (the longest line held in registers) is read from the plan, never written here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

assert np.finfo(np.longdouble).nmant >= 63, "the reference needs a long double wider than double"

LD = np.longdouble
DTYPES = (np.float32, np.float64)
IDS = dict(ids=lambda d: np.dtype(d).name)
ROW, COLUMN, CHANNEL, UNIT, SPLIT, COPY = (sma.MOMENTS_ROUTE_ROW, sma.MOMENTS_ROUTE_COLUMN, sma.MOMENTS_ROUTE_CHANNEL, sma.MOMENTS_ROUTE_UNIT,
                                           sma.MOMENTS_SPLIT, sma.MOMENTS_COPY)
EPS = (0.0, 1e-5)


def limit(lib, dtype):
    return lib.moments_plan("var", dtype, [1 << 20], [1], 0)[3][0]


def plan(lib, d, axis):
    return lib.moments_plan("var", d.dtype, d.shape, d.strides, axis)


def draws(shape, dtype, scale, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    return (shift + scale * rng.standard_normal(shape)).astype(dtype)


def offset_draws(shape, dtype, seed):
    """Data on an offset of 1e7 (f32) / 1e9 (f64) times its spread: mean(x*x) - mean(x)^2 would lose every digit."""
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return np.float32(1e4 + 1e-3 * rng.standard_normal(shape))
    return np.float64(1e9 + rng.standard_normal(shape))


class Reference:
    """The exact moments of the host array x over `axes` in long double, with each result's bound; computed once per (x, axes, ddof)."""

    def __init__(self, x, axes, ddof):
        dtype = x.dtype.type
        self.u, self.uT = LD(2) ** -53, LD(2) ** (-24 if dtype == np.float32 else -53)
        self.tiny, self.fmax = LD(np.finfo(dtype).smallest_subnormal), LD(np.finfo(dtype).max)
        self.axes, self.dtype, self.x = axes, x.dtype, x
        self.N = N = int(np.prod([x.shape[a] for a in axes]))
        with np.errstate(all="ignore"):
            X = x.astype(LD)
            self.mean = X.mean(axes, keepdims=True)
            self.d = X - self.mean
            self.var = (self.d * self.d).sum(axes, keepdims=True) / LD(N - ddof)
            self.std = np.sqrt(self.var)
            self.special = ~np.isfinite(X).all(axes, keepdims=True)
            self.xmax = np.abs(X).max(axes, keepdims=True)
        self.bound = dict(var=(self.uT + (N + 8) * self.u) * self.var + self.tiny, std=(self.uT + (N / LD(2) + 8) * self.u) * self.std + self.tiny)

    def compare(self, got, exact, bound, special, nan_too, what):
        assert got.dtype == self.dtype and got.size == exact.size, (what, got.dtype, got.shape, exact.shape)
        with np.errstate(all="ignore"):
            g = got.reshape(exact.shape).astype(LD)
            err = np.abs(g - exact)
            over = exact > self.fmax  # rounds to +inf (or, a hair above the largest number, to it)
            ok = np.where(special | nan_too, np.isnan(g), np.where(over, (g == np.inf) | (err <= bound), err <= bound))
            ratio = np.where(special | nan_too | over | ~np.isfinite(err), LD(0), err / bound)
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{what}: worst {worst:.3f} of the bound over {got.size} elements")
        assert ok.all(), (what, worst, np.argwhere(~ok)[:5], g[~ok][:5], exact[~ok][:5])
        return worst

    def check(self, kind, got, what):
        return self.compare(got, getattr(self, kind), self.bound[kind], self.special, np.zeros_like(self.special), (what, kind))

    def check_standardized(self, got, eps, what):
        N = self.N
        with np.errstate(all="ignore"):
            den = np.sqrt(self.var + LD(eps))
            y = self.d / den
            bound = (self.uT + (N + 10) * self.u) * np.abs(y) + (N + 2) * self.u * self.xmax / den + self.tiny
        shape = y.shape
        return self.compare(got, y, bound, np.broadcast_to(self.special, shape), np.broadcast_to(den == 0, shape), (what, "standardize", eps))


def check_all(lib, x, d, axis, what, ddofs=(0, 1)):
    """VAR, STD, var_mean and (along one axis) standardize of the device array / view `d`, which holds the host array / view `x`."""
    axes = lib._axes(x.ndim, axis)
    N = int(np.prod([x.shape[a] for a in axes]))
    mean = lib.reduce("mean", d, axis).numpy().tobytes()
    for ddof in ddofs:
        if N - ddof <= 0:
            continue
        ref = Reference(x, axes, ddof)
        var = lib.var(d, axis, ddof=ddof).numpy()
        ref.check("var", var, what)
        ref.check("std", lib.std(d, axis, ddof=ddof).numpy(), what)
        v2, m2 = lib.var_mean(d, axis, ddof=ddof)
        assert v2.numpy().tobytes() == var.tobytes() and m2.numpy().tobytes() == mean, (what, "var_mean")
        assert lib.var(d, axis, ddof=ddof, keepdims=True).shape == ref.var.shape
        if len(axes) == 1 and axis is not None:
            for eps in EPS:
                got = lib.standardize(d, axis, eps=eps, ddof=ddof).numpy()
                assert got.shape == x.shape
                ref.check_standardized(got, eps, what)


def lengths(L):
    return (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_last_axis_lengths(smhip, dtype):
    """Three rows of every length at which the code takes another path: a segment of 4, 16, 64 lanes, a wave, L and past it (two
    reads).  Scales and offsets rotate; offset data meet a held and a streamed length."""
    L = limit(smhip, dtype)
    for n, R in enumerate(lengths(L)):
        x = draws((3, R), dtype, (1e-3, 1.0, 1e3)[n % 3], 100 + n, shift=(0.0, 500.0, -3.0)[n % 3])
        d = smhip.to_device(x)
        route, _, ori, info = plan(smhip, d, 1)
        assert ori == (3, R, 1) and (info[1] == 1) == (R <= L) and route & 0xff == (UNIT if R == 1 else ROW)
        check_all(smhip, x, d, 1, (np.dtype(dtype).name, R))
    for n, R in enumerate((5, 257, L, L + 1, 2 * L + 1)):
        x = offset_draws((3, R), dtype, 200 + n)
        check_all(smhip, x, smhip.to_device(x), -1, (np.dtype(dtype).name, "offset", R))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_one_long_line(smhip, dtype):
    L = limit(smhip, dtype)
    R = 40 * L + 3
    x = offset_draws((1, R), dtype, 300)
    d = smhip.to_device(x)
    assert plan(smhip, d, 1)[0] == ROW | SPLIT
    check_all(smhip, x, d, 1, (np.dtype(dtype).name, R))
    flat = smhip.to_device(x.reshape(-1))
    ref = Reference(x.reshape(-1), (0,), 1)
    got = smhip.std(flat, ddof=1).numpy()
    assert got.shape == (1,)
    ref.check("std", got, "flat")
    ref.check_standardized(smhip.standardize(flat, axis=None, eps=1e-5, ddof=1).numpy(), 1e-5, "flat")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_columns_channels_and_axis_lists(smhip, dtype):
    """Extents off the vector width; columns cut into chunks (few lanes) and whole (short columns); per-channel statistics; axes that
    do not merge."""
    cases = (((70, 50), 0, COLUMN | SPLIT), ((257, 5), 0, COLUMN | SPLIT), ((3, 70, 6), 1, COLUMN | SPLIT), ((4099, 3), 0, CHANNEL | SPLIT),
             ((13, 37), 0, COLUMN), ((5, 6, 7, 3), (0, 1, 2), COLUMN | SPLIT), ((5, 6, 7), (0, 2), ROW | COPY), ((5, 6, 7), None, ROW),
             ((3, 4, 5, 6), (1, 3), ROW | COPY), ((2, 3, 700), (1, 2), ROW | SPLIT))
    for n, (shape, axis, route) in enumerate(cases):
        for x in (draws(shape, dtype, (1e-3, 1.0, 1e3)[n % 3], 400 + n, shift=(0.0, -700.0)[n % 2]), offset_draws(shape, dtype, 450 + n)):
            d = smhip.to_device(x)
            assert plan(smhip, d, axis)[0] == route, shape
            check_all(smhip, x, d, axis, (np.dtype(dtype).name, shape, axis))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views(smhip, dtype):
    L = limit(smhip, dtype)
    base = offset_draws((70, 130), dtype, 5)
    d = smhip.to_device(base)
    views = [  # (the view, the axis, COPY)
        (base.T, -1, False),               # var(A.T, -1): the columns of A read in place
        (base.T, 0, False),                # rows in memory
        (base[:, ::2], 1, True),           # a stepped axis
        (base[::2, :], 1, False),          # stepped rows: in place
        (base[3:60, 5:100], 1, False),     # a block of rows at an odd element offset
        (base[3:60, 5:100], 0, False),     # ... and its columns
        (base[3:60, 5:100], (0, 1), True),  # ... and all of it: two groups that do not merge
    ]
    for n, (v, axis, copy) in enumerate(views):
        dv = d.view_like(v, base)
        assert bool(plan(smhip, dv, axis)[0] & COPY) == copy, n
        check_all(smhip, v, dv, axis, (np.dtype(dtype).name, "view", n))
    # a stride-0 axis: along the axis (constant lines) and across it (equal lines)
    col = (np.round(draws((9, 1), dtype, 10, 6) * 8) / 8).astype(dtype)  # 33 * c is exact in fp64: a constant line gives exactly +0
    dc = smhip.to_device(col)
    for shape, strides, host in (((9, 33), (1, 0), np.broadcast_to(col, (9, 33))), ((33, 9), (0, 1), np.broadcast_to(col.T, (33, 9)))):
        b = sma.DeviceArray(smhip, dc.base_ptr, dtype, shape, strides, 0, dc._owner)
        assert plan(smhip, b, 1)[0] & COPY
        check_all(smhip, host, b, 1, (np.dtype(dtype).name, "stride 0", shape))
    assert smhip.var(sma.DeviceArray(smhip, dc.base_ptr, dtype, (9, 33), (1, 0), 0, dc._owner), 1).numpy().tobytes() == np.zeros(9, dtype).tobytes()
    long = draws((3, 2 * L + 5), dtype, 10, 7)  # a streamed line behind a copy, and rows wider apart than their length
    dl = smhip.to_device(long)
    check_all(smhip, long[:, ::2], dl.view_like(long[:, ::2], long), 1, "stepped long")
    check_all(smhip, long[:, 3:], dl.view_like(long[:, 3:], long), 1, "offset long")


def every_route(L):
    """(shape, axis) once per kernel: segments, a wave, rows past L whole and in chunks, columns whole and in chunks, CHANNEL sums, UNIT,
    a copy, two groups."""
    return (((1031, 37), 1), ((300, 700), 1), ((40, L), 1), ((3, 5 * L + 17), 1), ((4100, 2 * L), 1), ((1, 40 * L + 3), 1), ((16, 5000), 0), ((70, 50), 0),
            ((4099, 3), 0), ((7, 1), 1), ((5, 6, 7), (0, 2)))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_constant_lines_are_exactly_zero(smhip, dtype):
    L = limit(smhip, dtype)
    values = (0.1, -3.25, 1e30, 7e-41) if dtype == np.float32 else (-3.25, 2.0 ** 100)
    for shape, axis in every_route(L):
        if shape[0] == 4100:
            shape = (70, 2 * L)
        for value in values:
            d = smhip.to_device(np.full(shape, value, dtype))
            for ddof in (0, 1):
                if np.prod([shape[a] for a in smhip._axes(len(shape), axis)]) - ddof <= 0:
                    continue
                var, mean = smhip.var_mean(d, axis, ddof=ddof)
                sd = smhip.std(d, axis, ddof=ddof)
                zero = np.zeros(var.shape, dtype).tobytes()  # +0
                assert var.numpy().tobytes() == zero and sd.numpy().tobytes() == zero, (shape, axis, value, ddof)
                assert mean.numpy().tobytes() == np.full(var.shape, value, dtype).tobytes()
            if isinstance(axis, int):
                assert np.isnan(smhip.standardize(d, axis).numpy()).all()  # 0 / 0
                assert smhip.standardize(d, axis, eps=1e-5).numpy().tobytes() == np.zeros(shape, dtype).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_special_values(smhip, dtype):
    """A NaN or an infinity in a line gives NaN, on every route; the other lines are ordinary.  f32 near 1e30: +inf."""
    L = limit(smhip, dtype)
    for shape, axis in (((6, 5), 1), ((6, 300), 1), ((6, L), 1), ((6, 2 * L + 1), 1), ((70, 6), 0), ((13, 6), 0), ((2, 40, 3), 1), ((4099, 6), 0)):
        x = draws(shape, dtype, 3, 9)
        R = shape[axis]
        moved = np.moveaxis(x, axis, -1)  # a view: writes land in x
        line = [moved[i] for i in np.ndindex(moved.shape[:-1])]
        assert len(line) >= 6 and np.shares_memory(line[0], x)
        line[0][R // 2] = np.nan
        line[1][R - 1] = np.inf
        line[2][0] = -np.inf
        line[3][0], line[3][R - 1] = np.inf, -np.inf
        line[4][:] = np.inf
        check_all(smhip, x, smhip.to_device(x), axis, ("special", shape))
        got = np.moveaxis(smhip.var(smhip.to_device(x), axis, keepdims=True).numpy(), axis, -1).reshape(-1)
        assert np.isnan(got[:5]).all() and np.isfinite(got[5:]).all()
    if dtype == np.float32:
        for shape, axis in (((3, 100), 1), ((3, 3 * L), 1), ((100, 5), 0)):
            x = np.float32(1e30) * np.where(np.random.default_rng(10).random(shape) < 0.5, np.float32(-1), np.float32(1))
            x[0, 0], x[0, 1] = 1e30, -1e30
            d = smhip.to_device(x)
            assert (smhip.var(d, axis).numpy() == np.inf).all()
            check_all(smhip, x, d, axis, ("1e30", shape))
            Reference(x, (axis,), 0).check("std", smhip.std(d, axis).numpy(), "1e30")  # the square root is back in range


def test_empty_extents(smhip):
    for dtype in DTYPES:
        e = smhip.empty((0, 7), dtype)
        assert smhip.var(e, 1).shape == (0,) and smhip.std(e, 1, ddof=3, keepdims=True).shape == (0, 1)
        v, m = smhip.var_mean(e, 1)
        assert v.shape == m.shape == (0,)
        assert smhip.standardize(e, 1).shape == (0, 7) and smhip.standardize(smhip.empty((3, 0), dtype), 1).shape == (3, 0)
        with pytest.raises(ValueError, match="N - ddof = 0 - 0 is not positive"):
            smhip.var(e, 0)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_in_place_out_and_overlap(smhip, dtype):
    L = limit(smhip, dtype)
    for shape, axis in (((37, 130), 1), ((3, 2 * L + 1), 1), ((70, 50), 0), ((13, 37), 0), ((7, 1), 1)):
        x = draws(shape, dtype, 10, 11, shift=3.0)
        want = smhip.standardize(smhip.to_device(x), axis, eps=1e-5).numpy()
        d = smhip.to_device(x)
        assert smhip.standardize(d, axis, eps=1e-5, out=d) is d
        assert d.numpy().tobytes() == want.tobytes(), shape
        out = smhip.empty(shape, dtype)
        assert smhip.standardize(smhip.to_device(x), axis, eps=1e-5, out=out) is out and out.numpy().tobytes() == want.tobytes()
        kept = tuple(n for a, n in enumerate(shape) if a != axis)
        vout = smhip.empty(kept, dtype)
        assert smhip.std(smhip.to_device(x), axis, ddof=0, out=vout) is vout
        assert vout.numpy().tobytes() == smhip.std(smhip.to_device(x), axis).numpy().tobytes()
    x = draws((8, 40), dtype, 1, 12)
    d = smhip.to_device(x)
    other = smhip.empty((8,), dtype)
    esz, code = x.itemsize, sma.DTYPES[np.dtype(dtype)]
    for out_ptr, mean_ptr in ((d.ptr, 0), (d.ptr + 319 * esz, 0), (other.ptr, d.ptr + 8 * esz), (other.ptr, other.ptr + 7 * esz)):
        assert smhip.moments_raw(sma.MOMENT_VAR, code, d.ptr, [8, 40], [40, 1], 2, 0, out_ptr, mean_ptr) == sma.ERR_INVALID
        assert "overlap" in smhip.c.smhip_last_error().decode()
    for out_ptr in (d.ptr + esz, d.ptr + 40 * esz):
        assert smhip.standardize_raw(code, d.ptr, [8, 40], [40, 1], 1, 0.0, 0, out_ptr) == sma.ERR_INVALID
        assert "overlaps the operand" in smhip.c.smhip_last_error().decode()
    assert smhip.standardize_raw(code, d.ptr, [8, 20], [40, 1], 1, 0.0, 0, d.ptr) == sma.ERR_INVALID  # in place needs a dense operand
    assert d.numpy().tobytes() == x.tobytes()
    t = d.view_like(x.T, x)  # a view without an axis: its own row-major order
    Reference(np.ascontiguousarray(x.T).reshape(-1), (0,), 0).check_standardized(smhip.standardize(t, axis=None).numpy(), 0.0, "flat view")


def test_random_views(smhip):
    """About 40 views of rank 1-4 of one base array: steps, a permutation, a size-1 axis, a stride-0 axis; every axis and one pair."""
    rng = np.random.default_rng(21)
    count = 0
    for dtype in DTYPES:
        for trial in range(10):
            rank = 1 + trial % 4
            shape = tuple(int(n) for n in rng.integers(2, (40, 12, 7, 5)[rank - 1] + 2, size=rank))
            base = offset_draws(tuple(2 * n + 1 for n in shape), dtype, 500 + trial)
            d = smhip.to_device(base)
            steps = rng.integers(1, 3, size=rank)
            starts = rng.integers(0, 2, size=rank)
            v = base[tuple(slice(int(s), int(s) + int(k) * n, int(k)) for s, k, n in zip(starts, steps, shape))]
            dv = d.view_like(v, base)
            perm = rng.permutation(rank)
            v, dv = v.transpose(perm), sma.DeviceArray(smhip, dv.base_ptr, dtype, tuple(dv.shape[p] for p in perm), tuple(dv.strides[p] for p in perm), dv.offset, dv._owner)
            if trial % 3 == 0:  # a size-1 axis in front
                v, dv = v[None], sma.DeviceArray(smhip, dv.base_ptr, dtype, (1,) + tuple(dv.shape), (0,) + tuple(dv.strides), dv.offset, dv._owner)
            if trial % 5 == 1:  # a stride-0 axis at the end (of 4: a constant line's fp64 sum stays exact)
                v = np.broadcast_to(v[..., None], v.shape + (4,))
                dv = sma.DeviceArray(smhip, dv.base_ptr, dtype, tuple(dv.shape) + (4,), tuple(dv.strides) + (0,), dv.offset, dv._owner)
            axes = [int(rng.integers(0, v.ndim)), -1]
            if v.ndim >= 3:
                axes.append((0, v.ndim - 1))
            for axis in axes:
                check_all(smhip, v, dv, axis, ("random view", np.dtype(dtype).name, trial, v.shape, axis))
                count += 1
    assert count >= 40


def route_bytes(lib):
    """VAR, STD with the mean and standardize on one shape per kernel (every_route)."""
    parts = []
    for dtype in DTYPES:
        L = limit(lib, dtype)
        for i, (shape, axis) in enumerate(every_route(L)):
            d = lib.to_device(draws(shape, dtype, 10, 40 + i, shift=100.0))
            var, mean = lib.var_mean(d, axis, ddof=0 if shape == (7, 1) else 1)
            parts += [var.numpy().tobytes(), mean.numpy().tobytes(), lib.std(d, axis).numpy().tobytes()]
            if isinstance(axis, int):
                parts.append(lib.standardize(d, axis, eps=1e-5).numpy().tobytes())
    return b"".join(parts)


def test_same_bits_on_every_run(smhip):
    runs = [route_bytes(smhip) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


_ROUTES = """
import sys, simplemath_amd as sma
from tests.test_moments_gpu import route_bytes
lib = sma.load()
lib.set_device(0)
with open(sys.argv[1], "wb") as out:
    out.write(route_bytes(lib))
print("routes ok")
"""


def test_every_route_with_a_capped_grid(smhip, tmp_path):
    """SMHIP_MOMENTS_GRID_CAP=2 in ONE fresh process: every kernel's loop over its tasks runs many times per workgroup; the bytes are
    those of the uncapped run in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "capped")
    env = dict(os.environ, SMHIP_MOMENTS_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _ROUTES, path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "routes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    with open(path, "rb") as f:
        capped = f.read()
    plain = route_bytes(smhip)
    assert len(plain) > 1 << 16 and plain == capped
