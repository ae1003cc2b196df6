"""softmax, log_softmax and logsumexp along an axis on the GPU (smhip_softmax_axis through the ctypes binding), f32 and f64, against
an np.longdouble reference with the error bounds of include/smhip.h ("softmax"):

                 f32                        f64
    softmax      6u exact + 2 tiny          u (R + 5 + |d_r| + D) exact + 2 tiny
    log_softmax  2.5u + u |exact|           u (R + 1 + D + |d_r| + |exact|) + 2u max(1, ln R)
    logsumexp    2.5u + u |exact|           u (R + 1 + D + |exact|) + 2u max(1, ln R)

u = 2^-24 / 2^-53, tiny the smallest subnormal, D = min(746, max |d|).  Every element of every result is compared; special lines (a
NaN, a maximum of +inf, all -inf) are compared with the contract's table.  Each softmax line must also sum to 1 within the sum of its
elements' bounds.  L (the longest line held on chip) is read from the plan, never written here."""
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
KINDS = ("softmax", "log_softmax", "logsumexp")
SCALES = {np.float32: (1, 10, 40), np.float64: (1, 10, 300)}
ROW, COLUMN, SPLIT, COPY = sma.SOFTMAX_ROUTE_ROW, sma.SOFTMAX_ROUTE_COLUMN, sma.SOFTMAX_SPLIT, sma.SOFTMAX_COPY


def limit(lib, dtype):
    return lib.softmax_plan("softmax", dtype, [1 << 20], [1], 0)[3][0]


def plan(lib, kind, d, axis):
    return lib.softmax_plan(kind, d.dtype, d.shape, d.strides, axis % d.ndim)


def run(lib, kind, d, axis, **kw):
    return getattr(lib, kind)(d, axis, **kw).numpy()


def draws(shape, dtype, scale, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal(shape) + shift).astype(dtype)


class Reference:
    """The exact values of the three kinds for the host array x along `axis`, in long double, with each element's bound; computed once
    and shared by the three kinds."""

    def __init__(self, x, axis):
        dtype = x.dtype.type
        f32 = dtype == np.float32
        u = LD(2) ** (-24 if f32 else -53)
        tiny = LD(np.finfo(dtype).smallest_subnormal)
        R = x.shape[axis]
        with np.errstate(all="ignore"):
            X = x.astype(LD)
            m = X.max(axis, keepdims=True)  # a NaN propagates
            self.special = ~np.isfinite(m)
            self.m = m
            d = X - m
            E = np.exp(d)
            S = E.sum(axis, keepdims=True)
            lnS = np.log(S)
            self.softmax, self.log_softmax, self.logsumexp = E / S, d - lnS, m + lnS
            ad = np.where(np.isfinite(d), -d, LD(0))
            D = np.minimum(LD(746), (-d).max(axis, keepdims=True))
            if f32:
                self.bounds = dict(softmax=6 * u * self.softmax + 2 * tiny, log_softmax=2.5 * u + u * np.abs(self.log_softmax),
                                   logsumexp=2.5 * u + u * np.abs(self.logsumexp))
            else:
                extra = 2 * u * max(LD(1), np.log(LD(max(R, 1))))
                self.bounds = dict(softmax=u * (R + 5 + ad + D) * self.softmax + 2 * tiny, log_softmax=u * (R + 1 + D + ad + np.abs(self.log_softmax)) + extra,
                                   logsumexp=u * (R + 1 + D + np.abs(self.logsumexp)) + extra)
        self.axis, self.shape, self.dtype = axis, x.shape, x.dtype

    def check(self, kind, got, what):
        """Every element of `got`: inside its bound on an ordinary line, the table's value on a special one.  Returns the worst error
        as a fraction of its bound."""
        exact, bound = getattr(self, kind), self.bounds[kind]
        special, m = self.special, self.m
        if kind == "logsumexp":
            got = np.expand_dims(got, self.axis) if got.shape != exact.shape else got
        else:
            special, m = np.broadcast_to(special, exact.shape), np.broadcast_to(m, exact.shape)
        assert got.dtype == self.dtype and got.shape == exact.shape, (what, got.dtype, got.shape)
        with np.errstate(all="ignore"):
            g = got.astype(LD)
            if kind == "logsumexp":  # special lines: the maximum itself (NaN, +inf, -inf)
                ok_special = np.where(np.isnan(m), np.isnan(g), g == m)
            else:
                ok_special = np.isnan(g)
            infinite = np.isinf(exact) & ~special  # log_softmax of a -inf element of an ordinary line
            err = np.abs(g - exact)
            ratio = np.where(special | infinite, LD(0), err / bound)
            ok = np.where(special, ok_special, np.where(infinite, g == exact, err <= bound))
        worst = float(ratio.max()) if ratio.size else 0.0
        print(f"{what} {kind}: worst {worst:.3f} of the bound over {got.size} elements")
        assert ok.all(), (what, kind, worst, np.argwhere(~ok)[:5])
        if kind == "softmax" and got.size:  # a line sums to 1 within the sum of its elements' bounds
            with np.errstate(all="ignore"):
                total, room = g.sum(self.axis, keepdims=True), bound.sum(self.axis, keepdims=True)
                lines_ok = np.where(self.special, True, np.abs(total - 1) <= room)
            assert lines_ok.all(), (what, "line sums")
        return worst


def check_all(lib, x, d, axis, what):
    """The three kinds of the device array / view `d`, which holds the host array / view `x`."""
    ref = Reference(x, axis % x.ndim)
    for kind in KINDS:
        ref.check(kind, run(lib, kind, d, axis), what)


def lengths(L):
    return (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_last_axis_lengths(smhip, dtype):
    """Three rows of every length at which the code takes another path: a segment of 4, 16, 64 lanes, a wave, a workgroup, L and past
    it (the line streamed in chunks).  The scales rotate; every scale meets a held and a streamed length."""
    L = limit(smhip, dtype)
    for n, R in enumerate(lengths(L)):
        x = draws((3, R), dtype, SCALES[dtype][n % 3], 100 + n, shift=(0.0, 500.0, -3.0)[n % 3])
        d = smhip.to_device(x)
        route, _, ori, info = plan(smhip, "softmax", d, 1)
        assert route == (ROW if R <= L else ROW | SPLIT) and ori == (3, R, 1) and (info[1] == 1) == (R <= L)
        check_all(smhip, x, d, 1, (np.dtype(dtype).name, R))
    for n, R in enumerate((257, L, L + 1, 2 * L + 1)):  # every scale at a held and a streamed length
        for scale in SCALES[dtype]:
            x = draws((3, R), dtype, scale, 200 + n)
            check_all(smhip, x, smhip.to_device(x), -1, (np.dtype(dtype).name, R, scale))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_one_long_line(smhip, dtype):
    L = limit(smhip, dtype)
    R = 40 * L + 3
    for n, scale in enumerate(SCALES[dtype]):
        x = draws((1, R), dtype, scale, 300 + n)
        d = smhip.to_device(x)
        assert plan(smhip, "softmax", d, 1)[0] == ROW | SPLIT
        check_all(smhip, x, d, 1, (np.dtype(dtype).name, R, scale))
    flat = smhip.to_device(x.reshape(-1))
    ref = Reference(x.reshape(-1), 0)
    got = smhip.logsumexp(flat, axis=None).numpy()
    assert got.shape == (1,)
    ref.check("logsumexp", got, "flat")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_columns_and_middle_axes(smhip, dtype):
    """Extents off the vector width; columns cut into chunks (few lanes) and whole (short columns)."""
    cases = (((70, 50), 0, True), ((257, 5), 0, True), ((3, 70, 6), 1, True), ((4099, 3), 0, True), ((13, 37), 0, False), ((2, 9, 5), 1, False))
    for n, (shape, axis, split) in enumerate(cases):
        for scale in SCALES[dtype]:
            x = draws(shape, dtype, scale, 400 + n, shift=(0.0, -700.0)[n % 2])
            d = smhip.to_device(x)
            assert plan(smhip, "log_softmax", d, axis)[0] == (COLUMN | SPLIT if split else COLUMN), shape
            check_all(smhip, x, d, axis, (np.dtype(dtype).name, shape, axis, scale))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_views(smhip, dtype):
    L = limit(smhip, dtype)
    base = draws((70, 130), dtype, 10, 5)
    d = smhip.to_device(base)
    # (the view, the axis, COPY for softmax / log_softmax, COPY for logsumexp)
    views = [
        (base.T, -1, False, False),               # softmax(A.T, -1): the columns of A read in place
        (base.T, 0, True, False),                 # rows in memory, the result's lines strided: copied; logsumexp reads in place
        (base[:, ::2], 1, True, True),            # a stepped axis
        (base[::2, :], 1, False, False),          # stepped rows: in place
        (base[3:60, 5:100], 1, False, False),     # a block of rows at an odd element offset
        (base[3:60, 5:100], 0, False, False),     # ... and its columns
    ]
    for n, (v, axis, copy, copy_lse) in enumerate(views):
        dv = d.view_like(v, base)
        assert bool(plan(smhip, "softmax", dv, axis)[0] & COPY) == copy and bool(plan(smhip, "logsumexp", dv, axis)[0] & COPY) == copy_lse, n
        check_all(smhip, v, dv, axis, (np.dtype(dtype).name, "view", n))
    # a stride-0 axis: along the axis (constant lines) and across it (equal lines)
    col = draws((9, 1), dtype, 10, 6)
    dc = smhip.to_device(col)
    for shape, strides, host in (((9, 33), (1, 0), np.broadcast_to(col, (9, 33))), ((33, 9), (0, 1), np.broadcast_to(col.T, (33, 9)))):
        b = sma.DeviceArray(smhip, dc.base_ptr, dtype, shape, strides, 0, dc._owner)
        assert plan(smhip, "softmax", b, 1)[0] & COPY
        check_all(smhip, host, b, 1, (np.dtype(dtype).name, "stride 0", shape))
    long = draws((3, 2 * L + 5), dtype, 10, 7)  # a streamed line behind a copy, and rows wider apart than their length
    dl = smhip.to_device(long)
    check_all(smhip, long[:, ::2], dl.view_like(long[:, ::2], long), 1, "stepped long")
    check_all(smhip, long[:, 3:], dl.view_like(long[:, 3:], long), 1, "offset long")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_constant_lines_are_exact(smhip, dtype):
    """A constant line of R: float(1.0 / (double)R) (f64: 1.0 / R) bit for bit on every route; R == 1: 1, +0 and x_0."""
    L = limit(smhip, dtype)
    for R in (1, 3, 7, 100, 1000, L, L + 1, 2 * L + 1):
        for value in (0.0, -3.25, 1e30):
            x = np.full((2, R), value, dtype)
            want = np.full((2, R), dtype(1.0 / float(R)), dtype)
            assert run(smhip, "softmax", smhip.to_device(x), 1).tobytes() == want.tobytes(), (R, value)
            check_all(smhip, x, smhip.to_device(x), 1, ("constant", R, value))
    for shape, axis in (((70, 6), 0), ((13, 37), 0), ((3, 70, 6), 1)):
        x = np.full(shape, 2.5, dtype)
        assert run(smhip, "softmax", smhip.to_device(x), axis).tobytes() == np.full(shape, dtype(1.0 / shape[axis]), dtype).tobytes(), shape
    x = draws((5, 1), dtype, 10, 8)
    d = smhip.to_device(x)
    assert run(smhip, "softmax", d, 1).tobytes() == np.ones((5, 1), dtype).tobytes()
    assert run(smhip, "log_softmax", d, 1).tobytes() == np.zeros((5, 1), dtype).tobytes()  # +0
    assert run(smhip, "logsumexp", d, 1).tobytes() == x.reshape(5).tobytes()
    assert run(smhip, "logsumexp", d, 1, keepdims=True).tobytes() == x.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_special_values(smhip, dtype):
    """The contract's table on every route: a NaN, a maximum of +inf, all -inf -- and -inf among finite elements, which is ordinary."""
    L = limit(smhip, dtype)
    for shape, axis in (((6, 5), 1), ((6, 300), 1), ((6, 2000), 1), ((6, 2 * L + 1), 1), ((70, 6), 0), ((13, 6), 0), ((2, 40, 3), 1)):
        x = draws(shape, dtype, 3, 9)
        R = shape[axis]
        moved = np.moveaxis(x, axis, -1)  # a view: writes land in x
        line = [moved[i] for i in np.ndindex(moved.shape[:-1])]
        assert len(line) >= 6 and np.shares_memory(line[0], x)
        line[0][R // 2] = np.nan
        line[1][R - 1], line[1][0] = np.inf, -np.inf
        line[2][:] = -np.inf
        line[3][::2] = -np.inf
        line[4][0], line[4][R - 1] = np.nan, np.inf
        check_all(smhip, x, smhip.to_device(x), axis, ("special", shape))
    far = np.array([[0, -104.5, -200, -103, -1], [800, 0, -1, 799, 53]], dtype)  # beyond the exp's reach: +0
    check_all(smhip, far, smhip.to_device(far), 1, "far")
    got = run(smhip, "softmax", smhip.to_device(far), 1)
    assert got[1, 1] == 0 and got[1, 2] == 0 and (dtype == np.float64 or (got[0, 1] == 0 and got[0, 2] == 0))  # d < -104 (f32), d <= -746 (f64)
    big = np.finfo(dtype).max * dtype(0.9)
    x = np.array([[big, -big], [-big, big]], dtype)  # a difference that overflows the type
    d = smhip.to_device(x)
    assert run(smhip, "softmax", d, 1).tobytes() == np.array([[1, 0], [0, 1]], dtype).tobytes()
    assert run(smhip, "log_softmax", d, 1).tobytes() == np.array([[0, -np.inf], [-np.inf, 0]], dtype).tobytes()
    assert run(smhip, "logsumexp", d, 1).tobytes() == np.array([big, big], dtype).tobytes()
    sub = np.finfo(dtype).smallest_subnormal
    x = np.array([[sub, 2 * sub, 0, -sub, 1000 * sub, -0.0]], dtype)
    check_all(smhip, x, smhip.to_device(x), 1, "subnormal")


def test_empty_extents(smhip):
    for dtype in DTYPES:
        e = smhip.empty((3, 0), dtype)
        assert run(smhip, "softmax", e, 1).shape == (3, 0) and run(smhip, "log_softmax", e, 0).shape == (3, 0)
        got = run(smhip, "logsumexp", e, 1)  # over nothing: -inf
        assert got.shape == (3,) and got.dtype == dtype and (got == -np.inf).all()
        assert run(smhip, "logsumexp", e, 0).shape == (0,)
        assert run(smhip, "logsumexp", smhip.empty((0,), dtype), 0).tobytes() == np.array([-np.inf], dtype).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_in_place_out_and_overlap(smhip, dtype):
    L = limit(smhip, dtype)
    for shape, axis in (((37, 130), 1), ((3, 2 * L + 1), 1), ((70, 50), 0), ((13, 37), 0)):
        x = draws(shape, dtype, 10, 11)
        for kind in ("softmax", "log_softmax"):
            want = run(smhip, kind, smhip.to_device(x), axis)
            d = smhip.to_device(x)
            assert getattr(smhip, kind)(d, axis, out=d) is d
            assert d.numpy().tobytes() == want.tobytes(), (kind, shape)
            out = smhip.empty(shape, dtype)
            assert getattr(smhip, kind)(smhip.to_device(x), axis, out=out) is out and out.numpy().tobytes() == want.tobytes()
    x = draws((8, 40), dtype, 1, 12)
    d = smhip.to_device(x)
    esz, code = x.itemsize, sma.DTYPES[np.dtype(dtype)]
    for kind, out_ptr in ((sma.SOFTMAX, d.ptr + esz), (sma.LOG_SOFTMAX, d.ptr + 40 * esz), (sma.LOGSUMEXP, d.ptr), (sma.LOGSUMEXP, d.ptr + 319 * esz)):
        assert smhip.softmax_raw(kind, code, d.ptr, [8, 40], [40, 1], 1, out_ptr) == sma.ERR_INVALID
        assert "overlaps the operand" in smhip.c.smhip_last_error().decode()
    assert smhip.softmax_raw(sma.SOFTMAX, code, d.ptr, [8, 20], [40, 1], 1, d.ptr) == sma.ERR_INVALID  # in place needs a dense operand
    assert d.numpy().tobytes() == x.tobytes()
    flat = smhip.softmax(d, axis=None)
    assert flat.shape == (320,)
    Reference(x.reshape(-1), 0).check("softmax", flat.numpy(), "flat")
    t = d.view_like(x.T, x)  # a view without an axis: its own row-major order
    Reference(np.ascontiguousarray(x.T).reshape(-1), 0).check("log_softmax", smhip.log_softmax(t, axis=None).numpy(), "flat view")


def test_shift_invariance(smhip):
    """Integer-valued f32 lines plus an integer shift: every difference x - m is the same, exactly, so the bits are."""
    L = limit(smhip, np.float32)
    rng = np.random.default_rng(13)
    for shape, axis in (((5, 300), 1), ((3, L), 1), ((3, 2 * L + 1), 1), ((70, 50), 0), ((13, 37), 0)):
        x = rng.integers(-30, 30, size=shape).astype(np.float32)
        for shift in (1000.0, -77.0, 2.0 ** 20):
            y = x + np.float32(shift)
            for kind in ("softmax", "log_softmax"):
                assert run(smhip, kind, smhip.to_device(x), axis).tobytes() == run(smhip, kind, smhip.to_device(y), axis).tobytes(), (shape, shift, kind)


def test_same_bits_on_every_run(smhip):
    L = limit(smhip, np.float32)
    for shape, axis in (((300, 1000), 1), ((3, 5 * L + 17), 1), ((4099, 3), 0)):
        x = draws(shape, np.float32, 10, 14)
        d = smhip.to_device(x)
        for kind in KINDS:
            runs = [run(smhip, kind, d, axis).tobytes() for _ in range(3)]
            assert runs[0] == runs[1] == runs[2], (shape, kind)


def route_bytes(lib):
    """The three kinds on one shape per kernel: ROW with segments, a wave and a workgroup per line; ROW streamed, many lines and one;
    COLUMN whole and cut into chunks."""
    parts = []
    for dtype in DTYPES:
        L = limit(lib, dtype)
        for i, (shape, axis) in enumerate((((1031, 37), 1), ((300, 700), 1), ((40, L), 1), ((3, 5 * L + 17), 1), ((1, 40 * L + 3), 1), ((16, 5000), 0), ((4099, 3), 0))):
            d = lib.to_device(draws(shape, dtype, 10, 40 + i))
            parts += [run(lib, kind, d, axis).tobytes() for kind in KINDS]
    return b"".join(parts)


_ROUTES = """
import sys, simplemath_amd as sma
from tests.test_softmax_gpu import route_bytes
lib = sma.load()
lib.set_device(0)
with open(sys.argv[1], "wb") as out:
    out.write(route_bytes(lib))
print("routes ok")
"""


def test_every_route_with_a_capped_grid(smhip, tmp_path):
    """SMHIP_SOFTMAX_GRID_CAP=2 in ONE fresh process: every kernel's loop over its tasks runs many times per workgroup; the bytes are
    those of the uncapped run in this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "capped")
    env = dict(os.environ, SMHIP_SOFTMAX_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _ROUTES, path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "routes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    with open(path, "rb") as f:
        capped = f.read()
    plain = route_bytes(smhip)
    assert len(plain) > 1 << 16 and plain == capped
