"""Functions of one argument on the GPU (smhip_unary, csrc/unary.hip; unary chain stages, csrc/chain.hip) against numpy.
NEG / ABS / SQRT: identical bits.  EXP / LOG: within 1 ULP of the true value -- f32 against np.exp / np.log of the argument in
fp64 (numpy's own f32 exp / log are up to 2 ULP off and no reference), f64 against np.longdouble (64-bit significand).
No element is excluded from any comparison; NaN compares equal to NaN."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import simplemath_amd as sma
from tests import util

pytestmark = pytest.mark.gpu

U = sma.SMHIP_OP_UNARY_BASE
SIZES = [1, 3, 255, 256, 257, 4096, 4097, 70001, (1 << 24) + 5]
FLOATS = [np.float32, np.float64]
ALL = [np.float32, np.float64, np.int32, np.int64]


@pytest.fixture(scope="module")
def smhip():
    return sma.load()


def test_longdouble_is_the_x87_format():
    assert np.finfo(np.longdouble).nmant == 63, "np.longdouble is not the 64-bit-significand format: no reference for f64 exp / log"


def ulp_distance(got, want):
    """|got - want| in ULPs of got's dtype at `want` (fp64 for f32 results, longdouble for f64); inf/nan must agree exactly."""
    dt = got.dtype
    fi = np.finfo(dt)
    wide = np.float64 if dt == np.float32 else np.longdouble
    g, w = got.astype(wide), want.astype(wide)
    top = wide(2.0) ** (fi.maxexp)
    with np.errstate(all="ignore"):
        wn, gn = np.isnan(w), np.isnan(g)
        # a true value beyond the largest finite number: the grid point after it stands for +inf
        wc = np.clip(w, -top, top)
        gc = np.where(np.isinf(g), np.sign(g) * top, g)
        e = np.floor(np.log2(np.abs(wc)))
        e = np.where(np.isfinite(e), e, fi.minexp)
        e = np.maximum(e, fi.minexp)
        d = np.abs(gc - wc) / (wide(2.0) ** (e - fi.nmant))
    d = np.where(wn | gn, np.where(wn & gn, 0.0, np.inf), d)
    # infinities of the TRUE value (log 0, exp inf) must be matched exactly
    winf = np.isinf(w)
    d = np.where(winf, np.where(g == w, 0.0, np.inf), d)
    return d.astype(np.float64)


def true_value(fn, x):
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    with np.errstate(all="ignore"):
        return {"exp": np.exp, "log": np.log}[fn](x.astype(wide))


def check_ulp(fn, x, got, what):
    d = ulp_distance(got, true_value(fn, x))
    worst = int(np.argmax(d))
    print(f"{what}: max {d.max():.4f} ULP over {d.size} (x = {x.reshape(-1)[worst]!r})")
    assert d.max() <= 1.0, (what, float(d.max()), x.reshape(-1)[worst], got.reshape(-1)[worst])
    # signs of zero: exp underflows to +0, log(1) = +0
    z = got == 0
    assert not np.signbit(got[z]).any(), what


def specials(dt):
    fi = np.finfo(dt)
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                     fi.max, -fi.max, 88.72284, 88.7229, -87.33655, -103.972, -103.98, -104.5, 709.782712893384, 709.79, -708.3964,
                     -745.1332, -745.14, -746.0, 1000.0, -1000.0, 0.5, 2.0, 1.0000001, 0.99999994], dtype=dt)


def args_for(fn, dt, n, rng):
    if np.dtype(dt).kind == "i":
        ii = np.iinfo(dt)
        x = rng.integers(ii.min, ii.max, size=n, dtype=dt, endpoint=True)
        x[: min(n, 4)] = np.array([ii.min, ii.max, 0, -1], dtype=dt)[: min(n, 4)]
        return x
    fi = np.finfo(dt)
    if fn == "exp":
        lo, hi = (-105.0, 90.0) if dt == np.float32 else (-750.0, 710.0)
        x = rng.uniform(lo, hi, size=n).astype(dt)
    elif fn == "log":
        # log-uniform over the whole exponent range, subnormals included, plus a dense cluster around 1
        e = rng.uniform(fi.minexp - fi.nmant, fi.maxexp, size=n)
        x = (np.exp2(e.astype(np.longdouble)) if dt == np.float64 else np.exp2(e)).astype(dt)
        k = n // 4
        x[:k] = (1.0 + rng.uniform(-1e-3, 1e-3, size=k)).astype(dt)
    elif fn == "sqrt":
        e = rng.uniform(fi.minexp - fi.nmant, fi.maxexp, size=n)
        x = np.exp2(e).astype(dt)
        x[::7] *= -1
    else:
        x = (rng.standard_normal(n) * 1e3).astype(dt)
    sp = specials(dt)
    m = min(n, sp.size)
    if n > 4:
        x[-m:] = sp[:m]
    return x


def expect_exact(fn, x):
    with np.errstate(all="ignore"):
        return {"neg": np.negative, "abs": np.abs, "sqrt": np.sqrt}[fn](x)


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fn", ["neg", "abs", "sqrt", "exp", "log"])
def test_unary_against_numpy(smhip, fn, dt):
    rng = np.random.default_rng(zlib.crc32(f"{fn} {np.dtype(dt).name}".encode()))
    if np.dtype(dt).kind == "i" and fn in ("sqrt", "exp", "log"):
        a = smhip.to_device(np.arange(8, dtype=dt))
        with pytest.raises(sma.SmhipError) as e:
            smhip.unary(fn, a)
        assert e.value.code == sma.ERR_UNSUPPORTED
        return
    for n in SIZES:
        x = args_for(fn, dt, n, rng)
        got = smhip.unary(fn, smhip.to_device(x)).numpy()
        if fn in ("exp", "log"):
            check_ulp(fn, x, got, f"{fn} {np.dtype(dt).name} n={n}")
        else:
            util.assert_same_bits(got, expect_exact(fn, x), f"{fn} {np.dtype(dt).name} n={n}")


def test_special_values(smhip):
    for dt in FLOATS:
        x = specials(dt)
        d = smhip.to_device(x)
        for fn in ("neg", "abs", "sqrt"):
            util.assert_same_bits(smhip.unary(fn, d).numpy(), expect_exact(fn, x), f"{fn} specials {np.dtype(dt).name}")
        for fn in ("exp", "log"):
            got = smhip.unary(fn, d).numpy()
            check_ulp(fn, x, got, f"{fn} specials {np.dtype(dt).name}")
            with np.errstate(all="ignore"):
                want = true_value(fn, x).astype(dt)  # the true value, correctly rounded
            # where the answer is a zero, an infinity or NaN it is the same one (sign of zero included)
            fixed = ~np.isfinite(want) | (want == 0)
            util.assert_same_bits(got[fixed], want[fixed], f"{fn} fixed points {np.dtype(dt).name}")
        # the sign of a NaN is flipped / cleared like any other sign
        nan = np.array([np.nan, -np.nan], dtype=dt)
        u = {4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]
        assert (smhip.unary("neg", smhip.to_device(nan)).numpy().view(u) == np.negative(nan).view(u)).all()
        assert (smhip.unary("abs", smhip.to_device(nan)).numpy().view(u) == np.abs(nan).view(u)).all()


def test_crossing_the_piece_split(smhip):
    """2^28 + 3 floats: 1 GiB per operand, five launches of 256 MiB pieces and a tail."""
    n = (1 << 28) + 3
    rng = np.random.default_rng(5)
    x = rng.uniform(-105.0, 90.0, size=n).astype(np.float32)
    got = smhip.unary("exp", smhip.to_device(x)).numpy()
    # every element, in slabs (the fp64 reference of the whole array at once would be 2 GiB more)
    step = 1 << 24
    worst = 0.0
    for i in range(0, n, step):
        d = ulp_distance(got[i:i + step], true_value("exp", x[i:i + step]))
        worst = max(worst, float(d.max()))
    print(f"exp f32 n=2^28+3: max {worst:.4f} ULP")
    assert worst <= 1.0
    del got
    util.assert_same_bits(smhip.unary("neg", smhip.to_device(x)).numpy(), np.negative(x), "neg n=2^28+3")


def test_piece_loop_at_small_sizes():
    """SMHIP_PIECE_LOG2VEC=12 cuts a 300 001-element call into 19 launches."""
    code = ("import numpy as np, simplemath_amd as sma\n"
            "lib = sma.load()\n"
            "rng = np.random.default_rng(3)\n"
            "for dt in (np.float32, np.float64, np.int32, np.int64):\n"
            "    a = (rng.uniform(-50, 50, 300001)).astype(dt)\n"
            "    assert (lib.unary('neg', lib.to_device(a)).numpy() == -a).all()\n"
            "    assert (lib.unary('abs', lib.to_device(a)).numpy() == np.abs(a)).all()\n"
            "a = rng.uniform(0, 50, 300001)\n"
            "assert (lib.unary('sqrt', lib.to_device(a)).numpy() == np.sqrt(a)).all()\n"
            "e = lib.unary('exp', lib.to_device(a)).numpy(); assert np.allclose(e, np.exp(a), rtol=1e-15)\n"
            "print('pieces ok')\n")
    env = dict(os.environ, SMHIP_PIECE_LOG2VEC="12", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout + r.stderr


def _views(dt, rng, positive):
    def vals(shape):
        if np.dtype(dt).kind == "i":
            return rng.integers(-1000, 1000, size=shape).astype(dt)
        x = rng.uniform(0.01 if positive else -30.0, 30.0, size=shape).astype(dt)
        return x
    A = vals((96, 130))
    yield "transposed 2-D", A, A.T
    B = vals((5, 12, 7, 16))
    yield "permuted 4-D", B, B.transpose(2, 0, 3, 1)
    yield "a[:, ::2]", A, A[:, ::2]
    Cc = vals((3000,))
    yield "a[::3]", Cc, Cc[::3]
    row = vals((1, 130))
    yield "broadcast row", row, np.broadcast_to(row, (64, 130))
    big = vals((1024, 1536))
    yield "large transposed", big, big.T
    yield "column block", A, A[:, 3:45]


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_views_are_read_in_place(smhip, dt):
    rng = np.random.default_rng(11)
    fns = ["neg", "abs"] + (["sqrt", "exp", "log"] if np.dtype(dt).kind == "f" else [])
    for fn in fns:
        for what, base, view in _views(dt, rng, positive=fn in ("sqrt", "log")):
            dbase = smhip.to_device(base)
            if view.strides and 0 in view.strides and view.shape != base.shape:  # broadcast: strides 0 over the wanted shape
                dv = sma.DeviceArray(smhip, dbase.base_ptr, dbase.dtype, view.shape, [s // view.itemsize for s in view.strides], 0, dbase._owner)
            else:
                dv = dbase.view_like(view, base)
            got = smhip.unary(fn, dv).numpy()
            dense = np.ascontiguousarray(view)
            if fn in ("exp", "log"):
                check_ulp(fn, dense, got, f"{fn} {what} {np.dtype(dt).name}")
                # ... and the same bits as the function of the dense copy
                util.assert_same_bits(got, smhip.unary(fn, smhip.to_device(dense)).numpy(), f"{fn} {what} vs dense")
            else:
                util.assert_same_bits(got, expect_exact(fn, dense), f"{fn} {what} {np.dtype(dt).name}")
            util.assert_same_bits(dbase.numpy(), base, f"{fn} {what}: the operand is untouched")


def test_in_place_and_overlap(smhip):
    rng = np.random.default_rng(12)
    for dt in FLOATS:
        for n in (5, 4097, 70001):
            x = rng.uniform(0.5, 20.0, size=n).astype(dt)
            for fn in ("neg", "sqrt", "exp", "log"):
                d = smhip.to_device(x)
                want = smhip.unary(fn, d).numpy()
                r = smhip.unary(fn, d, out=d)
                assert r is d
                util.assert_same_bits(d.numpy(), want, f"in place {fn} {np.dtype(dt).name} n={n}")
    base = smhip.to_device(np.arange(100, dtype=np.float32))
    lo = sma.DeviceArray(smhip, base.base_ptr, base.dtype, (50,), [1], 0, base._owner)
    hi = sma.DeviceArray(smhip, base.base_ptr, base.dtype, (50,), [1], 10, base._owner)
    with pytest.raises(sma.SmhipError) as e:
        smhip.unary("neg", lo, out=hi)
    assert e.value.code == sma.ERR_INVALID
    stepped = sma.DeviceArray(smhip, base.base_ptr, base.dtype, (50,), [2], 0, base._owner)
    with pytest.raises(sma.SmhipError) as e:
        smhip.unary("neg", stepped, out=lo)
    assert e.value.code == sma.ERR_INVALID
    with pytest.raises(ValueError):
        smhip.unary("neg", lo, out=smhip.empty((49,), np.float32))
    with pytest.raises(ValueError):
        smhip.unary("neg", lo, out=smhip.empty((50,), np.float64))
    smhip.synchronize()
    util.assert_same_bits(base.numpy(), np.arange(100, dtype=np.float32), "rejected calls wrote nothing")


# ---------------------------------------------------------------------------------------------------------------- chains
# tests/test_chain.py's two size lists, and one output beyond the tiny-operator limit with whole-wave rows
CHAIN_SHAPES = [(64, 128), (37, 52), (5, 3), (1, 7), (129, 1024), (70, 96), (1, 5), (33, 1), (257, 1031), (1 << 20,), (4096, 4096 // 16)]


def _apply_one_at_a_time(smhip, first, stages):
    """The same stages through Smhip.binary / array_scalar / unary, one launch each, materialised."""
    r = first
    for st in stages:
        if len(st) == 1:
            r = smhip.unary(st[0] if isinstance(st[0], str) else st[0] - U, r)
            continue
        op, x = st[0], st[1]
        swapped = len(st) > 2 and st[2]
        if isinstance(x, sma.DeviceArray):
            r = smhip.binary(op, x, r) if swapped else smhip.binary(op, r, x)
        else:
            flat = sma.DeviceArray(smhip, r.base_ptr, r.dtype, (r.size,), [1], 0, r._owner)
            out = smhip.array_scalar(op, flat, x)
            r = sma.DeviceArray(smhip, out.base_ptr, out.dtype, r.shape, r.strides, 0, out._owner)
    return r


def _rand(rng, shape, dt, lo=-2.0, hi=2.0):
    if np.dtype(dt).kind == "f":
        return rng.uniform(lo, hi, size=shape).astype(dt)
    x = rng.integers(-1000, 1000, size=shape).astype(dt)
    x[x == 0] = 7
    return x


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_chains_with_unary_stages(smhip, dt):
    rng = np.random.default_rng(21)
    fp = np.dtype(dt).kind == "f"
    for shape in CHAIN_SHAPES:
        A, B = _rand(rng, shape, dt), _rand(rng, shape, dt)
        W_ = _rand(rng, shape, dt)
        dA, dB, dW = (smhip.to_device(x) for x in (A, B, W_))
        s = dt(3)
        cases = {
            "-(a * b)": [(sma.OP_MUL, dB), ("neg",)],
            "abs(a - b) / s": [(sma.OP_SUB, dB), ("abs",), (sma.OP_DIV, s)],
            "a unary stage first": [("abs",), (sma.OP_ADD, dB)],
            "two unary stages in a row": [(sma.OP_SUB, dB), ("abs",), ("neg",)],
            "eight stages": [(sma.OP_ADD, dB), ("neg",), (sma.OP_MUL, dW), ("abs",), (sma.OP_SUB, s), ("neg",), (sma.OP_ADD, dA), (U + sma.UNARY_ABS,)],
        }
        if len(shape) == 2 and shape[1] > 1:
            row, col = _rand(rng, (1, shape[1]), dt), _rand(rng, (shape[0], 1), dt)
            drow, dcol = smhip.to_device(row), smhip.to_device(col)
            cases["-(a * row)"] = [(sma.OP_MUL, drow), ("neg",)]
            cases["abs(col - a)"] = [(sma.OP_SUB, dcol, True), ("abs",)]
            if fp:
                cases["exp(a - col)"] = [(sma.OP_SUB, dcol), ("exp",)]
                cases["exp(a - col) * w"] = [(sma.OP_SUB, dcol), ("exp",), (sma.OP_MUL, dW)]
                cases["log in the middle, after a column and before a row"] = [(sma.OP_SUB, dcol), ("exp",), (sma.OP_ADD, dt(1)), ("log",), (sma.OP_MUL, drow)]
        if fp:
            cases["sqrt(a*a + b*b)"] = None  # built below: b*b is an operand of its own
            cases["exp(a - b)"] = [(sma.OP_SUB, dB), ("exp",)]
            cases["exp(a - b) * w"] = [(sma.OP_SUB, dB), ("exp",), (sma.OP_MUL, dW)]
            cases["log(a*a + 1)"] = [(sma.OP_MUL, dA), (sma.OP_ADD, dt(1)), ("log",)]
            cases["log then more"] = [(sma.OP_MUL, dA), (sma.OP_ADD, dt(1)), ("log",), (sma.OP_MUL, dB), ("neg",)]
            cases["exp first"] = [("exp",), (sma.OP_ADD, dB)]
            cases["log first"] = [("abs",), ("log",), ("exp",), ("sqrt",)]
            cases["sqrt(abs(a))"] = [("abs",), ("sqrt",)]
        for what, stages in cases.items():
            if stages is None:
                bb = smhip.binary(sma.OP_MUL, dB, dB)
                stages = [(sma.OP_MUL, dA), (sma.OP_ADD, bb), ("sqrt",)]
            got = smhip.chain(dA, *stages).numpy()
            want = _apply_one_at_a_time(smhip, dA, stages).numpy()
            util.assert_same_bits(got, want.reshape(got.shape), f"{what} {np.dtype(dt).name} {shape}")
    # a transposed view as the head of a chain that starts with a function
    S = _rand(rng, (96, 96), dt, 0.1, 2.0)
    dS = smhip.to_device(S)
    dT = dS.view_like(S.T, S)
    for stages in ([("neg",), (sma.OP_ADD, dS)], [("abs",), (sma.OP_MUL, dS), ("neg",)]) + (([("log",), (sma.OP_ADD, dS)], [("exp",), ("sqrt",)]) if fp else ()):
        got = smhip.chain(dT, *stages).numpy()
        want = _apply_one_at_a_time(smhip, smhip.to_device(np.ascontiguousarray(S.T)), stages).numpy()
        util.assert_same_bits(got, want, f"transposed head {stages[0]} {np.dtype(dt).name}")


def test_chain_values_against_numpy(smhip):
    """The chains are not only self-consistent: exp(a - col) and sqrt(a*a + b*b) against numpy."""
    rng = np.random.default_rng(22)
    for dt in FLOATS:
        A, B = rng.uniform(-3, 3, (257, 1031)).astype(dt), rng.uniform(-3, 3, (257, 1031)).astype(dt)
        col = A.max(axis=1, keepdims=True)
        dA, dB, dcol = smhip.to_device(A), smhip.to_device(B), smhip.to_device(col)
        got = smhip.chain(dA, (sma.OP_SUB, dcol), ("exp",)).numpy()
        check_ulp("exp", A - col, got, f"exp(a - col) {np.dtype(dt).name}")
        bb = smhip.binary(sma.OP_MUL, dB, dB)
        got = smhip.chain(dA, (sma.OP_MUL, dA), (sma.OP_ADD, bb), ("sqrt",)).numpy()
        util.assert_same_bits(got, np.sqrt(A * A + B * B), f"sqrt(a*a + b*b) {np.dtype(dt).name}")


def test_chain_sum_with_unary_stages(smhip):
    rng = np.random.default_rng(23)
    for dt in FLOATS:
        for shape in [(70, 96), (1, 5), (257, 1031), (1 << 20,)]:
            A, M = rng.uniform(-2, 2, shape).astype(dt), rng.uniform(1.5, 2.5, shape).astype(dt)
            dA, dM = smhip.to_device(A), smhip.to_device(M)
            for stages in ([(sma.OP_SUB, dM), ("exp",)], [(sma.OP_SUB, dM), ("abs",), ("sqrt",)], [(sma.OP_SUB, dM), ("abs",), ("log",)],
                           [(sma.OP_SUB, dt(2.5)), ("exp",), (sma.OP_MUL, dM)]):
                got = smhip.chain_sum(dA, *stages)
                r = smhip.chain(dA, *stages).numpy().astype(np.float64)
                want = float(np.sum(r))
                assert abs(got - want) <= 1e-15 * float(np.abs(r).sum()) + 1e-300, (np.dtype(dt).name, shape, stages[1:], got, want)
    for dt in (np.int32, np.int64):
        A, B = _rand(rng, (257, 1031), dt), _rand(rng, (257, 1031), dt)
        got = smhip.chain_sum(smhip.to_device(A), (sma.OP_SUB, smhip.to_device(B)), ("abs",))
        assert got == float(np.abs(A - B).astype(np.int64).sum())


def test_chain_errors(smhip):
    a = smhip.to_device(np.ones((4, 4), np.int32))
    with pytest.raises(sma.SmhipError) as e:
        smhip.chain(a, (sma.OP_ADD, a), ("exp",))
    assert e.value.code == sma.ERR_UNSUPPORTED
    with pytest.raises(KeyError):
        smhip.chain(a, ("tanh",))


# ------------------------------------------------------------------------------------------------------------ tiny arrays
def test_unary_of_a_recorded_tiny_operator(smhip):
    """exp(a + b) on 5 x 5 arrays: a + b is RECORDED (tiny.hip), the function runs at once -- behind the recorded operator, with
    no synchronise in between -- and smhip_tiny_stats still adds up."""
    rng = np.random.default_rng(31)
    for dt in FLOATS:
        a, b = rng.uniform(-2, 2, (5, 5)).astype(dt), rng.uniform(-2, 2, (5, 5)).astype(dt)
        da, db = smhip.to_device(a), smhip.to_device(b)
        smhip.synchronize()
        l0, o0 = smhip.tiny_stats()
        t = smhip.binary(sma.OP_ADD, da, db)      # recorded
        l1, o1 = smhip.tiny_stats()
        e = smhip.unary("exp", t)                 # flushes the record, then runs
        u = smhip.binary(sma.OP_MUL, e, db)       # recorded again, reads the function's result
        got_e, got_u = e.numpy(), u.numpy()
        l2, o2 = smhip.tiny_stats()
        assert (l1, o1) == (l0, o0), "a + b is recorded, not launched (the counters move when a record goes out)"
        assert o2 - o0 == 2, "two recorded operators; the function itself is not one"
        assert l2 - l0 == 2, "each went out alone: the first in front of the function, the second in front of the read-back"
        check_ulp("exp", a + b, got_e, f"exp(a + b) tiny {np.dtype(dt).name}")
        util.assert_same_bits(got_u, got_e * b, "exp(a + b) * b tiny")
        util.assert_same_bits(smhip.unary("neg", smhip.binary(sma.OP_SUB, da, db)).numpy(), -(a - b), "-(a - b) tiny")
