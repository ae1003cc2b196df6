"""quantile, percentile and median along an axis on the GPU (smhip_quantile_axis through the ctypes binding), f32 and f64.

The oracle is the host model below: np.sort of the line in fp64, `+ 0.0` to make every zero +0, then the rules of include/smhip.h
("quantile") in numpy's IEEE arithmetic -- h = (R - 1) q, j, g, numpy's _lerp with the two shortcuts (g == 0, lo == hi), one rounding to
T, every NaN the canonical quiet NaN.  The comparison is BIT FOR BIT.  As a plausibility check on finite data the results are also
compared with np.quantile of the fp64 line, rounded to T, within 1 ULP of T.

L (the longest line a selection holds in LDS, and the compaction threshold of the streamed route) and Qmax (the most probabilities a
selection serves) are read from the plan, never written here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma
from tests.test_sort_gpu import continuous, specials, ties

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
IDS = dict(ids=lambda d: d if isinstance(d, str) else np.dtype(d).name)
METHODS = ("linear", "lower", "higher", "nearest", "midpoint")
QS = (0.0, 0.25, 0.5, 1.0 / 3.0, 0.999, 1.0)
KINDS = (continuous, ties, specials)


def limits(lib, dtype):
    _, _, _, info = lib.quantile_plan(dtype, [1 << 20], [1], 0, [0.5])
    return info[0], info[1]


def lengths(L):
    return (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, L - 1, L, L + 1, 2 * L + 1, 5 * L + 17)


def canonical_nan(dtype):
    return np.array([0x7FC00000], np.uint32).view(np.float32)[0] if np.dtype(dtype) == np.float32 else np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def ordered(x, axis):
    """The lines of x in fp64 in sort's ascending order (NaNs last), the axis moved to the end, every zero +0."""
    with np.errstate(invalid="ignore"):  # (a signalling NaN among the specials is quieted by the conversion)
        return np.sort(np.moveaxis(np.asarray(x), axis, -1).astype(np.float64), axis=-1) + 0.0


def model(s, dtype, qs, method):
    """The contract on ordered lines s[..., R] -> [len(qs), ...] in dtype."""
    R, lead = s.shape[-1], s.shape[:-1]
    s = s.reshape(-1, R)
    has_nan = np.isnan(s[:, -1])
    u = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    out = np.empty((len(qs), s.shape[0]), dtype)
    for n, q in enumerate(qs):
        h = np.float64(R - 1) * np.float64(q)
        j = np.floor(h)
        g = h - j
        if method == "lower":
            g = np.float64(0)
        elif method == "higher":
            j, g = np.ceil(h), np.float64(0)
        elif method == "nearest":
            j, g = np.rint(h), np.float64(0)
        elif method == "midpoint":
            g = np.float64(0.5 if g != 0 else 0.0)
        j = int(j)
        lo, hi = s[:, j], s[:, min(j + 1, R - 1)]
        with np.errstate(all="ignore"):
            d = hi - lo
            r = lo + d * g if g < 0.5 else hi - d * (np.float64(1) - g)
            r = np.where((g == 0) | (lo == hi), lo, r).astype(dtype)
        bits = r.view(u)
        bits[has_nan | np.isnan(r)] = canonical_nan(dtype).view(u)
        out[n] = r
    return out.reshape((len(qs),) + lead)


def same(got, want, what):
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    g, w = np.ascontiguousarray(got).reshape(-1).view(u), np.ascontiguousarray(want).reshape(-1).view(u)
    bad = np.flatnonzero(g != w)
    if bad.size:
        at = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} differ, first at flat {at}: got {got.reshape(-1)[at]!r} ({g[at]:#x}), want {want.reshape(-1)[at]!r} ({w[at]:#x})")


def within_one_ulp(got, x, qs, axis, method, what):
    """The plausibility check: np.quantile of the fp64 lines, rounded to T, within 1 ULP of T (finite data only)."""
    want = np.quantile(np.asarray(x).astype(np.float64), qs, axis=axis, method=method).astype(got.dtype)
    ulp = np.spacing(np.maximum(np.abs(want), np.finfo(got.dtype).tiny))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp.astype(np.float64)), what


def check(lib, x, d, qs, axis, method, s=None, finite=False):
    """`d` holds the host array or view `x`; the list form, and every probability singly against its row of it."""
    s = ordered(x, axis) if s is None else s
    want = model(s, x.dtype, qs, method)
    got = lib.quantile(d, list(qs), axis, method).numpy()
    same(got, want, (x.dtype, x.shape, axis, method, "list"))
    for n, q in enumerate(qs):
        one = lib.quantile(d, q, axis, method).numpy()
        same(one, want[n] if want[n].shape else want[n].reshape(1), (x.dtype, x.shape, axis, method, q))
    if finite:
        within_one_ulp(got, x, qs, axis, method, (x.dtype, x.shape, axis, method))


@pytest.fixture(scope="module")
def ladder(smhip):
    """Three lines of every length, per dtype: (host array, device array, ordered lines, finite?), made and ordered once."""
    made = {}
    for dtype in DTYPES:
        L, _ = limits(smhip, dtype)
        rows = []
        for n, R in enumerate(lengths(L)):
            x = KINDS[n % 3]((3, R), dtype, 300 + n)
            rows.append((x, smhip.to_device(x), ordered(x, 1), bool(np.isfinite(x).all())))
        made[np.dtype(dtype)] = rows
    return made


@pytest.mark.parametrize("method", METHODS, **IDS)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_lengths_methods_and_probabilities(smhip, ladder, dtype, method):
    """Every length at which the code takes another path: a wave or a workgroup per line, L, the streamed route over one to six tiles."""
    for x, d, s, finite in ladder[np.dtype(dtype)]:
        check(smhip, x, d, QS, 1, method, s, finite)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_model_agrees_with_numpy_on_finite_lines(smhip, dtype):
    L, _ = limits(smhip, dtype)
    for R in (2, 5, 100, 1000, L + 1):
        x = continuous((7, R), dtype, R)
        d = smhip.to_device(x)
        for method in METHODS:
            check(smhip, x, d, QS, 1, method, finite=True)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_lines_that_never_shrink(smhip, dtype):
    """Constant and two-valued lines of 5L + 17: more than L elements share every digit of the rank's key, so the streamed route runs
    every pass and ends without compacting.  The two values differ in the top byte of the key, or only in the lowest."""
    L, _ = limits(smhip, dtype)
    R = 5 * L + 17
    assert smhip.quantile_plan(dtype, [3, R], [R, 1], 1, [0.5])[0] == sma.QUANTILE_ROUTE_ROW | sma.QUANTILE_STREAM
    const = np.full((3, R), -7.5, dtype)
    const[1], const[2] = 0.0, -0.0
    two = np.empty((3, R), dtype)
    rng = np.random.default_rng(5)
    two[0] = np.where(rng.random(R) < 0.5, 1.0, -2.0)
    two[1] = np.where(rng.random(R) < 0.5, dtype(1.0), np.nextafter(dtype(1.0), dtype(2.0)))
    two[2] = np.where(rng.random(R) < 0.3, 0.0, np.inf)
    for x in (const, two):
        d = smhip.to_device(x)
        for method in ("linear", "nearest"):
            check(smhip, x, d, QS + (0.3, 0.5000001), 1, method)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_compaction_threshold_by_one_element_either_way(smhip, dtype):
    """A line of 2L + 1 whose elements in [1, 2) share the top byte of the key and number L - 1, L or L + 1, the others lying in [2, 4):
    after the first pass a rank among the former is compacted (at most L agree) or streams on (L + 1 do), and the ranks among the
    latter do the opposite."""
    L, _ = limits(smhip, dtype)
    R = 2 * L + 1
    rng = np.random.default_rng(11)
    x = np.empty((3, R), dtype)
    for line, c in enumerate((L - 1, L, L + 1)):
        values = np.concatenate([1.0 + rng.random(c), 2.0 + 2.0 * rng.random(R - c)]).astype(dtype)
        x[line] = rng.permutation(values)
    d = smhip.to_device(x)
    for method in METHODS:
        check(smhip, x, d, (0.1, 0.25, 0.49, 0.5, 0.51, 0.75, 0.9), 1, method, finite=True)


def line_of(dtype, values):
    return np.array(values, np.float64).astype(dtype).reshape(1, -1)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_specials(smhip, dtype):
    L, _ = limits(smhip, dtype)
    inf, nan = np.inf, np.nan
    for R in (1, 2, 5, 300, L + 1):
        # a NaN first, last and alone: NaN for every method and probability, the canonical one
        for where in (0, R - 1, R // 2):
            x = continuous((2, R), dtype, R)
            x[0, where] = nan
            x[1, where] = -canonical_nan(dtype) if R > 1 else x[1, where]
            d = smhip.to_device(x)
            for method in METHODS:
                check(smhip, x, d, QS, 1, method)
                if R > 1:
                    got = smhip.quantile(d, list(QS), 1, method).numpy()
                    assert got.tobytes() == np.full_like(got, canonical_nan(dtype)).tobytes()
        # -0 / +0 mixtures give +0
        u = np.uint32 if dtype == np.float32 else np.uint64
        zeros = (np.arange(R, dtype=np.uint64) % np.uint64(2) << np.uint64(31 if dtype == np.float32 else 63)).astype(u).view(dtype).reshape(1, R)
        dz = smhip.to_device(zeros)
        got = smhip.quantile(dz, list(QS), 1).numpy()
        assert not got.view(u).any()
        check(smhip, -zeros, smhip.to_device(-zeros), QS, 1, "midpoint")
    cases = [
        [inf, inf, 1.0, 0.0],           # equal infinities as neighbours: that infinity
        [-inf, -inf, 1.0, 0.0],
        [-inf, inf],                    # opposite: NaN where 0 < g < 1, the element itself where g == 0
        [-inf, inf, -inf, inf],
        [1.0, inf],                     # one finite: +inf for g < 0.5, NaN from there on
        [-inf, 1.0],
        [-inf, 0.0, 1.0, 2.0, inf],     # g == 0 next to an infinity: quartiles of five fall on elements
        [-inf, -1.0, -0.0, 3.0, inf, inf],
        [np.finfo(dtype).max, -np.finfo(dtype).max],  # an fp64 difference that overflows (f64)
        [np.finfo(dtype).smallest_subnormal, -np.finfo(dtype).smallest_subnormal, 0.0],
    ]
    qs = QS + (0.2, 0.4, 0.6, 0.75, 0.8, 0.1)
    for values in cases:
        x = line_of(dtype, values)
        d = smhip.to_device(x)
        for method in METHODS:
            check(smhip, x, d, qs, 1, method)
    # the header's words, pinned: equal infinities, opposite ones, g == 0
    def med(values):
        d = smhip.to_device(line_of(dtype, values))
        return smhip.median(d, 1).numpy()[0]

    assert med([inf, inf, 1.0, 0.0, inf, inf]) == inf and np.isnan(med([-inf, inf])) and med([-inf, 5.0, inf]) == 5.0
    # the same specials inside long lines: the streamed route
    x = specials((3, 2 * L + 1), dtype, 9)
    x[np.isnan(x)] = np.inf
    x[0, : L + 7] = -np.inf
    check(smhip, x, smhip.to_device(x), qs, 1, "linear")


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_axes_and_views(smhip, dtype):
    L, _ = limits(smhip, dtype)
    cube = continuous((5, 33, 7), dtype, 4)
    dc = smhip.to_device(cube)
    for axis in (0, 1, -1):
        for method in ("linear", "higher"):
            check(smhip, cube, dc, QS, axis, method, finite=True)
    base = ties((70, 130), dtype, 3)
    d = smhip.to_device(base)
    for viewf in (lambda b: b.T, lambda b: b[::2, 1::3], lambda b: b[3:60, 5:100]):
        v = viewf(base)
        dv = d.view_like(v, base)
        for axis in (0, 1):
            check(smhip, v, dv, (0.5, 0.1, 0.9), axis, "linear", finite=True)
    long = continuous((3, 2 * L + 5), dtype, 5)  # a transposed operand with the streamed route inside, and a stepped one
    dl = smhip.to_device(long)
    check(smhip, long.T, dl.view_like(long.T, long), (0.5, 0.25), 0, "linear", finite=True)
    check(smhip, long[:, ::2], dl.view_like(long[:, ::2], long), (0.5,), 1, "midpoint", finite=True)
    # keepdims, and axis=None: the row-major flattening, also of a view
    got = smhip.quantile(dc, [0.25, 0.75], 1, keepdims=True)
    assert got.shape == (2, 5, 1, 7)
    same(got.numpy().reshape(2, 5, 7), model(ordered(cube, 1), dtype, (0.25, 0.75), "linear"), "keepdims")
    assert smhip.median(dc, 0, keepdims=True).shape == (1, 33, 7) and smhip.median(dc, 0).shape == (33, 7)
    flat = smhip.quantile(dc, [0.5, 0.9], None)
    same(flat.numpy(), model(ordered(cube.reshape(-1), 0), dtype, (0.5, 0.9), "linear"), "flat")
    one = smhip.quantile(dc, 0.5, None)
    assert one.shape == (1,) and smhip.quantile(dc, 0.5, None, keepdims=True).shape == (1, 1, 1)
    t = d.view_like(base.T, base)
    same(smhip.median(t, None).numpy(), model(ordered(np.ascontiguousarray(base.T).reshape(-1), 0), dtype, (0.5,), "linear")[0].reshape(1), "flat view")


def test_out_empty_results_and_the_other_names(smhip):
    x = continuous((37, 130), np.float32, 8)
    d = smhip.to_device(x)
    out = smhip.empty((3, 130), np.float32)
    got = smhip.quantile(d, [0.1, 0.5, 0.9], 0, out=out)
    assert got is out
    same(out.numpy(), model(ordered(x, 0), np.float32, (0.1, 0.5, 0.9), "linear"), "out")
    # median is quantile(0.5); percentile(p) is quantile(p / 100)
    assert smhip.median(d, 1).numpy().tobytes() == smhip.quantile(d, 0.5, 1).numpy().tobytes()
    for p in (0.0, 12.5, 33.0, 50.0, 99.9, 100.0):
        for method in METHODS:
            assert smhip.percentile(d, p, 1, method).numpy().tobytes() == smhip.quantile(d, p / 100, 1, method).numpy().tobytes()
    assert smhip.percentile(d, [25, 75], 1).numpy().tobytes() == smhip.quantile(d, [0.25, 0.75], 1).numpy().tobytes()
    # a result with a zero extent launches nothing; an empty axis with a result is refused
    e = smhip.empty((4, 0, 3), np.float32)
    assert smhip.quantile(e, [0.5, 0.6], 0).shape == (2, 0, 3) and smhip.median(e, 2).shape == (4, 0)
    with pytest.raises(ValueError, match="an empty axis with a result that is not empty"):
        smhip.median(e, 1)
    ints = smhip.to_device(np.arange(6, dtype=np.int32))
    with pytest.raises(TypeError, match="astype first"):
        smhip.median(ints, 0)


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_seventeen_probabilities_are_the_sort_route(smhip, dtype):
    """More probabilities than a selection serves go through the sort: the same bytes as the selection gives for each of them singly."""
    L, qmax = limits(smhip, dtype)
    qs = [k / qmax for k in range(qmax + 1)]
    for shape, axis, gen in (((9, 300), 1, specials), ((3, 2 * L + 1), 1, continuous), ((70, 50), 0, ties), ((5, 1), 1, specials)):
        x = gen(shape, dtype, 21)
        if gen is specials:
            x[1:][np.isnan(x[1:])] = np.inf  # one line keeps its NaNs
        d = smhip.to_device(x)
        route = smhip.quantile_plan(dtype, list(shape), list(d.strides), axis, qs)[0] & 0xFF
        assert route == (sma.QUANTILE_ROUTE_SORT if shape[axis] > 1 else sma.QUANTILE_ROUTE_COPYONLY)
        for method in METHODS:
            got = smhip.quantile(d, qs, axis, method).numpy()
            same(got, model(ordered(x, axis), dtype, qs, method), (shape, axis, method))
            for n in (0, 1, qmax // 2, qmax - 1, qmax):
                assert smhip.quantile_plan(dtype, list(shape), list(d.strides), axis, [qs[n]])[0] & 0xFF != sma.QUANTILE_ROUTE_SORT
                assert smhip.quantile(d, qs[n], axis, method).numpy().tobytes() == got[n].tobytes(), (shape, method, n)


def every_route(lib):
    """{name: bytes} of one call on every route: a wave and a workgroup per line, the streamed route, staged, sorted, copied."""
    out = {}
    for dtype in DTYPES:
        L, qmax = limits(lib, dtype)
        cases = [((1031, 37), 1, 3), ((300, 200), 1, 1), ((301, 600), 1, 16), ((9, L), 1, 3), ((5, 2 * L + 1), 1, 3), ((2, 5 * L + 17), 1, 16), ((70, 50), 0, 3),
                 ((9, 300), 1, qmax + 1), ((40, 1), 1, 2)]
        for i, (shape, axis, nq) in enumerate(cases):
            for gen in (continuous, ties):
                x = gen(shape, dtype, 40 + i)
                d = lib.to_device(x)
                qs = [k / max(nq - 1, 1) for k in range(nq)] if nq > 1 else [0.5]
                for method in ("linear", "nearest"):
                    out[(np.dtype(dtype).name, shape, gen.__name__, method)] = lib.quantile(d, qs, axis, method).numpy().tobytes()
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
        smhip.to_device(np.zeros(256, np.float32))  # moves the upload ring back to the library's stream while the other still exists
        smhip.synchronize()
        hip.hipStreamDestroy(stream)
    assert third == first


_ROUTES = """
import sys, pickle, simplemath_amd as sma
from tests.test_quantile_gpu import every_route
lib = sma.load()
lib.set_device(0)
with open(sys.argv[1], "wb") as out:
    pickle.dump(every_route(lib), out)
print("routes ok")
"""


def test_every_route_with_a_capped_grid(smhip, tmp_path):
    """SMHIP_QUANTILE_GRID_CAP=2 in a fresh process: every kernel's loop over its tasks runs many times per workgroup; the bytes are
    those of this process's uncapped run."""
    import pickle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "capped")
    env = dict(os.environ, SMHIP_QUANTILE_GRID_CAP="2", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _ROUTES, path], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "routes ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    with open(path, "rb") as f:
        capped = pickle.load(f)
    plain = every_route(smhip)
    assert len(plain) > 60 and capped == plain
