"""astype on the GPU (smhip_convert through lib.astype): all 12 pairs of float32, float64, int32 and int64 against np.ndarray.astype
wherever numpy is defined -- every integer -> float, float -> float, integer -> integer, and float -> integer for values whose
truncation is in range -- and against the rule of smhip.h elsewhere (saturating truncation, NaN gives 0), computed here with np.trunc
on the fp64 value and comparisons against 2.0**31 / 2.0**63, which are exact.  Every element is compared; NaN positions must agree."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma

pytestmark = pytest.mark.gpu

TYPES = [np.float32, np.float64, np.int32, np.int64]
PAIRS = [(s, d) for s in TYPES for d in TYPES if s != d]
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 70001]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(t):
    return np.dtype(t).name


@pytest.fixture(scope="module")
def smhip():
    return sma.load()


# ------------------------------------------------------------------------------------------------------------ the reference
def expected(x, dst):
    """What astype must give for the host array x, and the mask of elements where that is numpy's own answer."""
    src, dst = x.dtype, np.dtype(dst)
    with np.errstate(all="ignore"):
        if src.kind == "f" and dst.kind == "i":
            top = 2.0 ** (8 * dst.itemsize - 1)
            t = np.trunc(x.astype(np.float64))
            inside = (t > -top) & (t < top)  # false for a NaN
            want = np.zeros(x.shape, dst)    # a NaN gives 0
            want[inside] = t[inside].astype(dst)
            want[t >= top] = np.iinfo(dst).max
            want[t <= -top] = np.iinfo(dst).min
            assert (want[inside] == x[inside].astype(dst)).all()  # in range the rule IS numpy's conversion
            return want
        return x.astype(dst)


def check(got, x, dst, what):
    want = expected(x, dst)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), f"{what}: NaN positions differ"
        u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        ok = (got.view(u) == want.view(u)) | nan  # the sign and payload of a NaN are not specified
    else:
        ok = got == want
    if not ok.all():
        i = int(np.flatnonzero(~ok.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ; first at {i}: {x.reshape(-1)[i]!r} -> {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


# ------------------------------------------------------------------------------------------------------------ the edge sets
def float_edges(dt):
    dt = np.dtype(dt)
    mant_bits, exp_count, u = (23, 256, np.uint32) if dt.itemsize == 4 else (52, 2048, np.uint64)
    half = 1 << (mant_bits - 1)
    mants = np.array([0, 1, half, half - 1, half + 1, (1 << mant_bits) - 1], dtype=np.uint64)
    exps = np.arange(exp_count, dtype=np.uint64)
    pos = ((exps[:, None] << np.uint64(mant_bits)) | mants[None, :]).reshape(-1)  # +0, subnormals, +inf and NaNs are among them
    bits = np.concatenate([pos, pos | (np.uint64(1) << np.uint64(8 * dt.itemsize - 1))]).astype(u)
    named = [0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 31 - 128, 2147483647.99, -2147483648.99, 2147483647.0, -2147483649.0,
             2.0 ** 63, -(2.0 ** 63), 0.9, -0.9, 1.5, -1.5, 0.5, -0.5, 2.0 ** 32, -(2.0 ** 32), 1e39, -1e39, 1e-40, -1e-40, 1e-46, -1e-46]
    with np.errstate(all="ignore"):
        extra = np.array(named, dtype=np.float64).astype(dt)  # (as f32: 2147483647.99 is 2^31, 1e39 is inf, 1e-46 is 0 -- harmless repeats)
    below_2_63 = np.nextafter(dt.type(2.0 ** 63), dt.type(0))                     # the largest float / double below 2^63
    more = [below_2_63, -below_2_63, np.nextafter(dt.type(2.0 ** 31), dt.type(0)), np.nextafter(dt.type(-(2.0 ** 63)), dt.type(-np.inf))]
    if dt.itemsize == 8:
        fmax = float(np.finfo(np.float32).max)
        threshold = fmax + 2.0 ** 103  # halfway between FLT_MAX and 2^128: the f32 overflow threshold (a tie that rounds to even = inf)
        more += [threshold, np.nextafter(threshold, 0.0), np.nextafter(threshold, np.inf), -threshold, -np.nextafter(threshold, 0.0), fmax,
                 2.0 ** -149, 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 1.5 * 2.0 ** -149, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0)]
        # every f32 exponent with a tie of the narrowing in the mantissa: bit 28 set, everything below it clear, +- 1
        e32 = (np.arange(1, 255, dtype=np.uint64) + np.uint64(1023 - 127)) << np.uint64(52)
        for low in (1 << 28, (1 << 28) + 1, (1 << 28) - 1, 3 << 28, (3 << 28) + 1, (3 << 28) - 1):
            more += list((e32 | np.uint64(low)).view(np.float64))
    return np.concatenate([bits.view(dt), extra, np.array(more, dtype=dt)])


def int_edges(dt):
    dt = np.dtype(dt)
    nbits = 8 * dt.itemsize
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    vals = [lo, hi, 0, int(np.iinfo(np.int32).min), int(np.iinfo(np.int32).max), 2 ** 60 + 2 ** 36 + 1, -(2 ** 60 + 2 ** 36 + 1)]
    for p in range(nbits):
        b = 2 ** p
        vals += [b, -b, b + 1, -(b + 1), b - 1, -(b - 1)]
        for drop in (24, 53):  # the ties of the f32 / f64 rounding, each also +- 1
            if p >= drop:
                t = 2 ** (p - drop)
                for k in (t, 3 * t):
                    vals += [b + k, b + k + 1, b + k - 1, -(b + k), -(b + k + 1), -(b + k - 1)]
    return np.array([v for v in vals if lo <= v <= hi], dtype=dt)


def random_values(dt, n, rng):
    dt = np.dtype(dt)
    if dt.kind == "i":
        full = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=n, dtype=dt, endpoint=True)
        return full >> rng.integers(0, 8 * dt.itemsize, size=n).astype(dt)  # every magnitude
    scale = 10.0 ** rng.uniform(-3, 22 if dt.itemsize == 8 else 21, size=n)  # beyond 2^63 for a part of them
    with np.errstate(all="ignore"):
        return (rng.standard_normal(n) * scale).astype(dt)


# ------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("s,d", PAIRS, ids=_id)
def test_edge_sets(smhip, s, d):
    x = float_edges(s) if np.dtype(s).kind == "f" else int_edges(s)
    check(smhip.astype(smhip.to_device(x), d).numpy(), x, d, f"edges {_id(s)} -> {_id(d)}")


def test_the_named_cases(smhip):
    f = np.array([np.nan, -0.0, -0.9, 0.9, 1.5, -1.5, np.inf, -np.inf, 2.0 ** 31, 2147483647.99, -2147483648.99, 2.0 ** 63, 1e300], dtype=np.float64)
    i32, i64 = np.iinfo(np.int32), np.iinfo(np.int64)
    assert smhip.astype(smhip.to_device(f), np.int32).numpy().tolist() == [0, 0, 0, 0, 1, -1, i32.max, i32.min, i32.max, i32.max, i32.min, i32.max, i32.max]
    assert smhip.astype(smhip.to_device(f), np.int64).numpy().tolist() == [0, 0, 0, 0, 1, -1, i64.max, i64.min, 2 ** 31, 2 ** 31 - 1, -(2 ** 31), i64.max,
                                                                           i64.max]
    big = np.array([2 ** 60 + 2 ** 36 + 1, -(2 ** 60 + 2 ** 36 + 1)], dtype=np.int64)
    got = smhip.astype(smhip.to_device(big), np.float32).numpy()
    assert got.tolist() == [float(2 ** 60 + 2 ** 37), -float(2 ** 60 + 2 ** 37)]  # rounded once; through double it would be 2^60
    d = np.array([1e39, 1e-40, 1e-46, -0.0], dtype=np.float64)
    got = smhip.astype(smhip.to_device(d), np.float32).numpy()
    assert np.isinf(got[0]) and got[1] == np.float32(1e-40) and got[1] != 0 and got[2] == 0 and np.signbit(got[3])


@pytest.mark.parametrize("s,d", PAIRS, ids=_id)
def test_sizes(smhip, s, d):
    """One lane's group, a workgroup's edge, the tiny-batch boundary (4096), an odd tail across workgroups."""
    rng = np.random.default_rng(11)
    for n in SIZES:
        x = random_values(s, n, rng)
        check(smhip.astype(smhip.to_device(x), d).numpy(), x, d, f"{_id(s)} -> {_id(d)} n={n}")


# ----------------------------------------------------------------------------------------------------------------- layouts
def _broadcast(dev, shape, strides):
    return sma.DeviceArray(dev.lib, dev.base_ptr, dev.dtype, shape, strides, dev.offset, dev._owner)


@pytest.mark.parametrize("s,d", PAIRS, ids=_id)
def test_layouts(smhip, s, d):
    rng = np.random.default_rng(5)
    R = sma.CONVERT_ROUTE_ROWS, sma.CONVERT_ROUTE_STAGED, sma.CONVERT_ROUTE_DENSE
    ROWS, STAGED, DENSE = R
    m = random_values(s, 16 * 128, rng).reshape(16, 128)
    t = random_values(s, 37 * 53, rng).reshape(37, 53)
    x = random_values(s, 1001, rng)
    q = random_values(s, 3 * 2 * 5 * 7, rng).reshape(3, 2, 5, 7)
    views = [("x[1:]", x, x[1:], DENSE), ("m[2:9, 5:77]", m, m[2:9, 5:77], ROWS), ("transpose of (37, 53)", t, t.T, STAGED), ("x[::2]", x, x[::2], STAGED),
             ("rank 4", q, q, DENSE), ("rank 4, middle axes swapped", q, q.transpose(0, 2, 1, 3), ROWS), ("m[3]", m, m[3], DENSE),
             ("m[:, 7]", m, m[:, 7], STAGED)]
    for what, base, view, route in views:
        dev = smhip.to_device(base)
        v = dev.view_like(view, base)
        assert smhip.convert_plan(s, d, v.shape, v.strides)[0] == route, what
        check(smhip.astype(v, d).numpy(), np.ascontiguousarray(view), d, f"{what} {_id(s)} -> {_id(d)}")
    row = random_values(s, 77, rng).reshape(1, 77)
    dev = smhip.to_device(row)
    v = _broadcast(dev, (9, 77), (0, 1))
    assert smhip.convert_plan(s, d, v.shape, v.strides)[0] == ROWS
    check(smhip.astype(v, d).numpy(), np.ascontiguousarray(np.broadcast_to(row, (9, 77))), d, "row broadcast")
    col = random_values(s, 5, rng).reshape(5, 1)
    dev = smhip.to_device(col)
    v = _broadcast(dev, (5, 7), (1, 0))
    assert smhip.convert_plan(s, d, v.shape, v.strides)[0] == STAGED
    check(smhip.astype(v, d).numpy(), np.ascontiguousarray(np.broadcast_to(col, (5, 7))), d, "column broadcast")


@pytest.mark.parametrize("s,d", PAIRS, ids=_id)
def test_out_form_and_unaligned_out(smhip, s, d):
    """`out=` a 1-D slice that starts at element 1: DENSE with a result pointer that is not 16-byte aligned; what lies around it stays."""
    rng = np.random.default_rng(9)
    for n in (5, 1001, 4099):
        x = random_values(s, n, rng)
        frame = np.full(n + 3, 77, dtype=d)
        out_base = smhip.to_device(frame)
        out = out_base.view_like(frame[1:n + 1], frame)
        res = smhip.astype(smhip.to_device(x), d, out=out)
        assert res is out
        back = out_base.numpy()
        check(back[1:n + 1], x, d, f"out= {_id(s)} -> {_id(d)} n={n}")
        assert back[0] == 77 and (back[n + 1:] == 77).all()
    with pytest.raises(TypeError):
        smhip.astype(smhip.to_device(x), d, out=smhip.empty((n,), s))
    with pytest.raises(ValueError):
        smhip.astype(smhip.to_device(x), d, out=smhip.empty((n + 1,), d))


@pytest.mark.parametrize("t", TYPES, ids=_id)
def test_equal_dtypes_give_a_copy(smhip, t):
    rng = np.random.default_rng(2)
    a = random_values(t, 37 * 53, rng).reshape(37, 53)
    dev = smhip.to_device(a)
    for view in (a, a.T, a[2:9, 5:47], a[::3]):
        v = dev.view_like(view, a)
        got = smhip.astype(v, t)
        assert got.ptr != v.ptr and got.is_dense()
        want = np.ascontiguousarray(view)
        u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
        assert (got.numpy().view(u) == want.view(u)).all()  # a copy keeps every bit, NaN payloads included


def test_overlap_is_refused(smhip):
    a = smhip.to_device(np.arange(64, dtype=np.float32))
    alias = sma.DeviceArray(smhip, a.base_ptr, np.int32, (64,), (1,), 0, a._owner)
    with pytest.raises(sma.SmhipError) as e:
        smhip.astype(a, np.int32, out=alias)
    assert e.value.code == sma.ERR_INVALID
    half = sma.DeviceArray(smhip, a.base_ptr, np.float64, (16,), (1,), 16, a._owner)  # the second half of a's bytes
    front = sma.DeviceArray(smhip, a.base_ptr, np.float32, (16,), (1,), 24, a._owner)  # overlaps it
    with pytest.raises(sma.SmhipError):
        smhip.astype(front, np.float64, out=half)
    assert (a.numpy() == np.arange(64, dtype=np.float32)).all()


def test_empty_shape(smhip):
    e = smhip.astype(smhip.empty((0,), np.float32), np.int64)
    assert e.shape == (0,) and e.dtype == np.int64
    e = smhip.astype(smhip.empty((3, 0, 2), np.int64), np.float64)
    assert e.shape == (3, 0, 2)
    smhip.synchronize()


def test_piece_loop_at_small_sizes():
    """SMHIP_PIECE_LOG2VEC=12 cuts a 300 001-element call into 19 launches (37 for an 8-byte result): the four width combinations, dense and staged."""
    code = ("import numpy as np, simplemath_amd as sma\n"
            "from tests.test_astype_gpu import check, random_values\n"
            "lib = sma.load()\n"
            "rng = np.random.default_rng(3)\n"
            "for s, d in ((np.float32, np.int32), (np.int32, np.float64), (np.float64, np.float32), (np.int64, np.float64), (np.float64, np.int64)):\n"
            "    x = random_values(s, 300001, rng)\n"
            "    assert lib.convert_plan(s, d, [300001], [1])[1] > 1\n"
            "    check(lib.astype(lib.to_device(x), d).numpy(), x, d, 'pieces')\n"
            "    y = random_values(s, 2 * 300001, rng)\n"
            "    dev = lib.to_device(y)\n"
            "    check(lib.astype(dev.view_like(y[::2], y), d).numpy(), np.ascontiguousarray(y[::2]), d, 'staged pieces')\n"
            "print('pieces ok')\n")
    env = dict(os.environ, SMHIP_PIECE_LOG2VEC="12", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------ compositions
def test_histogram_density(smhip):
    rng = np.random.default_rng(21)
    x = rng.normal(0, 1.5, 70001).astype(np.float32)
    counts, _ = smhip.histogram(smhip.to_device(x), 64, range=(-4.0, 4.0))
    scale = np.float32(x.size) * np.float32(8.0 / 64)
    got = smhip.array_scalar(sma.OP_DIV, smhip.astype(counts, np.float32), scale).numpy()
    want = np.histogram(x, 64, range=(-4.0, 4.0))[0].astype(np.float32) / scale
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()


def test_accuracy_from_argmax(smhip):
    rng = np.random.default_rng(22)
    logits = rng.standard_normal((1024, 10)).astype(np.float32)
    labels = np.where(rng.random(1024) < 0.7, logits.argmax(-1), rng.integers(0, 10, 1024)).astype(np.int64)
    pred = smhip.argreduce("argmax", smhip.to_device(logits), axis=-1)
    labels_dev = smhip.to_device(labels)
    hit = smhip.where((pred, "eq", labels_dev), 1, 0)
    acc = smhip.reduce("mean", smhip.astype(hit, np.float64), axis=0).numpy()
    assert acc.dtype == np.float64 and acc[0] == np.mean(logits.argmax(-1) == labels)


def test_int_keys_widened_for_take(smhip):
    rng = np.random.default_rng(23)
    table = rng.standard_normal(300).astype(np.float32)
    keys = rng.integers(0, 300, 70001).astype(np.int32)
    got = smhip.take(smhip.to_device(table), smhip.astype(smhip.to_device(keys), np.int64), axis=0).numpy()
    assert (got == table[keys]).all()


def test_float_data_scanned_as_double(smhip):
    rng = np.random.default_rng(24)
    x = np.floor(rng.uniform(-1000, 1000, 70001)).astype(np.float32)  # whole numbers: every partial sum is exact in fp64, whatever the order
    got = smhip.scan("cumsum", smhip.astype(smhip.to_device(x), np.float64), axis=0).numpy()
    assert got.dtype == np.float64 and (got == np.cumsum(x.astype(np.float64))).all()


def test_quantised_signal_into_bincount(smhip):
    rng = np.random.default_rng(25)
    x = rng.uniform(-4, 4, 70001).astype(np.float32)
    x = np.minimum(x, np.float32(3.99))  # (x + 4) * 32 stays below 256
    d = smhip.to_device(x)
    level = smhip.astype(smhip.array_scalar(sma.OP_MUL, smhip.array_scalar(sma.OP_ADD, d, 4.0), 32.0), np.int32)
    got = smhip.bincount(level, 256).numpy()
    want = np.bincount(((x + np.float32(4)) * np.float32(32)).astype(np.int32), minlength=256)
    assert (got == want).all()
