"""smhip_chain writing INTO one of its operands, into a preallocated array and into a block of a taller one, with the stage that
writes running alone (a transposed or stepped operand, log, the f64 exp, a general pow, a second row, a fifth dense operand), and
smhip_chain_sum over operands that are not dense -- against the stage-by-stage reference of tests/fuzz_chain_modes.py: the oracle
and numpy for the exact stages, the standalone GPU operator (held to its own bar) for exp, log and general powers; bit for bit.
`lib.chain(..., out=x)` with x among the operands is what `x = <expression reading x>` does in C++ (SMArray::operator=)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import simplemath_amd as sma
from oracle import oracle as orc
from tests import util
from tests.fuzz_chain import values
from tests.fuzz_chain_modes import ROWS, Reference, exact_sum

pytestmark = pytest.mark.gpu

TYPES = [np.float32, np.float64, np.int64]
FLOATS = [np.float32, np.float64]
SHAPES = [(96, 96), (37, 52)]
ADD, SUB, MUL, DIV = sma.OP_ADD, sma.OP_SUB, sma.OP_MUL, sma.OP_DIV
ids = lambda d: np.dtype(d).name if isinstance(d, type) else "x".join(map(str, d))  # noqa: E731


@pytest.fixture(scope="module")
def ref(smhip, oracle):
    return Reference(oracle, smhip)


def op(o, h, swapped=False):
    return {"kind": "op", "op": o, "h": h, "swapped": swapped}


def power(e):
    return {"kind": "pow", "e": e}


def fn(name):
    return {"kind": "un", "fn": name}


class Device:
    """host operands -> device operands, one device array per host array (so the same array is the same storage)"""

    def __init__(self, lib):
        self.lib, self.arrays = lib, {}

    def base(self, x):
        if id(x) not in self.arrays:
            self.arrays[id(x)] = self.lib.to_device(x)
        return self.arrays[id(x)]

    def __call__(self, x):
        if isinstance(x, np.ndarray):
            root = x
            while root.base is not None:
                root = root.base
            return self.base(root) if root is x else self.base(root).view_like(x, root)
        return x

    def stages(self, dt, stages):
        out = []
        for st in stages:
            if st["kind"] == "op":
                out.append((st["op"], self(st["h"]), st["swapped"]))
            elif st["kind"] == "pow":
                out.append((sma.OP_POW, dt(st["e"])))
            else:
                out.append((st["fn"],))
        return out


def want_of(ref, head, stages):
    r = np.ascontiguousarray(head)
    for st in stages:
        r = ref.apply(r, st)
    return np.ascontiguousarray(r)


def in_place(smhip, ref, x, head, stages, what):
    """out = x, one of the operands; the reference from the host copies, which nothing writes"""
    want = want_of(ref, head, stages)
    dev = Device(smhip)
    got = smhip.chain(dev(head), *dev.stages(x.dtype.type, stages), out=dev(x))
    assert got is dev(x)
    util.assert_same_bits(got.numpy(), want, what)
    # and the same chain into a fresh array gives the same bits: in place is only a place
    dev = Device(smhip)
    util.assert_same_bits(smhip.chain(dev(head), *dev.stages(x.dtype.type, stages)).numpy(), want, what + " (fresh)")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_in_place_last_operator_runs_alone_over_a_view(smhip, ref, dt, shape):
    """x = B.T + x, x = x - B.T, x = B[:, ::2] * x: the one operator goes through the broadcast kernels (the LDS tile kernel for the
    transposed operand) with its output aliasing an operand -- alone, and behind a fused segment."""
    rng = np.random.default_rng(41)
    rows, cols = shape
    x, y = values(rng, shape, dt), values(rng, shape, dt)
    B = values(rng, (cols, rows), dt)
    wide = values(rng, (rows, 2 * cols + 1), dt)
    col = values(rng, (rows, 1), dt)
    in_place(smhip, ref, x, B.T, [op(ADD, x)], "x = B.T + x")
    in_place(smhip, ref, x, x, [op(SUB, B.T)], "x = x - B.T")
    in_place(smhip, ref, x, x, [op(SUB, B.T, True)], "x = B.T - x")
    in_place(smhip, ref, x, wide[:, ::2][:, :cols], [op(MUL, x)], "x = B[:, ::2] * x")
    in_place(smhip, ref, x, x, [op(MUL, col), op(ADD, y), op(SUB, B.T)], "x = (x * col + y) - B.T")
    in_place(smhip, ref, x, y, [op(MUL, B.T), op(ADD, x), op(SUB, x, True)], "x = x - (y * B.T + x): x read behind the cut, twice")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("dt", FLOATS, ids=ids)
def test_in_place_exp_log_and_general_pow(smhip, ref, dt, shape):
    """x = exp(x - col): one pass for f32, the subtraction into a temporary and unary.hip's exp from there into x for f64;
    x = log(x*x + 1) and x = (x + y)^2.5 end in a stage that runs alone in either type."""
    rng = np.random.default_rng(42)
    x, y = values(rng, shape, dt), values(rng, shape, dt)
    col, row = values(rng, (shape[0], 1), dt), values(rng, (1, shape[1]), dt)
    one = dt(1)
    in_place(smhip, ref, x, x, [op(SUB, col), fn("exp")], "x = exp(x - col)")
    in_place(smhip, ref, x, x, [op(MUL, x), op(ADD, one), fn("log")], "x = log(x*x + 1)")
    in_place(smhip, ref, x, x, [op(ADD, y), power(2.5)], "x = (x + y)^2.5")
    in_place(smhip, ref, x, x, [fn("exp")], "x = exp(x)")
    in_place(smhip, ref, x, x, [fn("abs"), fn("log"), op(MUL, x), fn("neg"), fn("exp"), op(SUB, x, True)], "x = x - exp(-(log|x| * x)): x read behind both cuts")
    in_place(smhip, ref, x, row, [fn("abs"), power(0.5), op(ADD, x), fn("abs"), fn("sqrt")], "x = sqrt|row^0.5 + x|: a broadcast head under a power")
    in_place(smhip, ref, x, y.T if shape[0] == shape[1] else y, [fn("abs"), fn("log"), op(ADD, x)], "x = log|y.T| + x: a view head under a function")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_in_place_integer_power(smhip, ref, shape):
    rng = np.random.default_rng(43)
    x, y = values(rng, shape, np.int64), values(rng, shape, np.int64)
    in_place(smhip, ref, x, x, [op(ADD, y), power(3)], "x = (x + y)^3")
    in_place(smhip, ref, x, x, [op(SUB, x), power(0), op(ADD, x)], "x = (x - x)^0 + x: 0^0 = 1")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_in_place_behind_a_fifth_dense_operand(smhip, ref, dt, shape):
    """A kernel variant takes four dense operands: the fifth cuts the chain, the segment before it goes to a temporary, and x is
    read (and written) by the segment after it -- or read before the cut and written after it."""
    rng = np.random.default_rng(44)
    x, a, b, c, d, e = (values(rng, shape, dt) for _ in range(6))
    in_place(smhip, ref, x, a, [op(ADD, b), op(MUL, c), op(SUB, d), op(DIV, e), op(ADD, x)], "x = ((a + b) * c - d) / e + x")
    in_place(smhip, ref, x, x, [op(ADD, b), op(MUL, c), op(SUB, d), op(DIV, e), op(ADD, a)], "x = ((x + b) * c - d) / e + a")
    in_place(smhip, ref, x, x, [op(ADD, b), op(MUL, c), op(SUB, d), op(DIV, e), op(ADD, a), op(SUB, x, True)], "x = x - (((x + b) * c - d) / e + a)")


@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_in_place_behind_a_second_row(smhip, ref, dt):
    """Two different rows at the start of a chain run as one operator alone (tests/test_chain.py: the fuzz's first finding) -- here
    with the chain's output among the operands."""
    rng = np.random.default_rng(45)
    x = values(rng, (257, 32), dt)
    r1, r2 = values(rng, (1, 32), dt), values(rng, (1, 32), dt)
    c1, c2 = values(rng, (257, 1), dt), values(rng, (257, 1), dt)
    in_place(smhip, ref, x, r1, [op(ADD, r2), op(MUL, x)], "x = (row1 + row2) * x")
    in_place(smhip, ref, x, x, [op(MUL, r1), op(ADD, r2), op(SUB, x, True)], "x = x - (x * row1 + row2)")
    in_place(smhip, ref, x, r1, [op(ADD, x)], "x = row1 + x")
    in_place(smhip, ref, x, c1, [op(SUB, c2), op(MUL, x), op(ADD, c1, True)], "x = col1 + (col1 - col2) * x")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_block_of_a_taller_array_as_out(smhip, ref, dt, shape):
    """z(SLICE(4, 4 + rows), SLICE_ALL) = <chain>: the block read and written, or only written; the rows around it keep their bits."""
    rng = np.random.default_rng(46)
    rows, cols = shape
    tall = values(rng, (4 + rows + 3, cols), dt)
    block = tall[4:4 + rows]
    y, B = values(rng, shape, dt), values(rng, (cols, rows), dt)
    row = values(rng, (1, cols), dt)
    floats = np.dtype(dt).kind == "f"
    chains = [(block, [op(SUB, y), fn("abs")] + ([fn("sqrt")] if floats else []), "z[4:] = sqrt|z[4:] - y|"),
              (y, [op(MUL, row), op(ADD, B.T)], "z[4:] = y * row + B.T: written only, the last operator alone"),
              (block, [op(ADD, B.T, True)], "z[4:] = B.T + z[4:]"),
              (block, [op(MUL, block), op(ADD, dt(1))] + ([fn("log")] if floats else [power(3)]), "z[4:] = log(z[4:]^2 + 1)")]
    for head, stages, what in chains:
        want = want_of(ref, head, stages)
        dev = Device(smhip)
        dtall = dev.base(tall)
        smhip.chain(dev(head), *dev.stages(dt, stages), out=dtall.view_like(block, tall))
        got = dtall.numpy()
        util.assert_same_bits(got[4:4 + rows], want, what)
        assert got[:4].tobytes() == tall[:4].tobytes() and got[4 + rows:].tobytes() == tall[4 + rows:].tobytes(), what + ": rows outside the block"


@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_preallocated_out(smhip, ref, dt):
    rng = np.random.default_rng(47)
    x, y, stale = (values(rng, (37, 52), dt) for _ in range(3))
    col = values(rng, (37, 1), dt)
    stages = [op(SUB, col), op(MUL, y), power(2)]
    dev = Device(smhip)
    out = smhip.to_device(stale)
    assert smhip.chain(dev(x), *dev.stages(dt, stages), out=out) is out
    util.assert_same_bits(out.numpy(), want_of(ref, x, stages), "out= a preallocated array")


def check_sum(smhip, ref, head, stages, what):
    want = want_of(ref, head, stages)
    dev = Device(smhip)
    got = smhip.chain_sum(dev(head), *dev.stages(want.dtype.type, stages))
    s, scale = exact_sum(want)
    if want.dtype.kind == "f":
        assert np.isfinite(want).all(), what
        assert abs(got - s) <= 1e-15 * scale + 1e-300, (what, got, s)  # test_chain_sum's bar
    else:
        assert got == s, (what, got, s)


@pytest.mark.parametrize("dt", TYPES, ids=ids)
def test_chain_sum_over_small_operands_views_and_cuts(smhip, ref, dt):
    """try_chain_sum's decision: one pass for dense operands and scalars, the chain into a temporary and its sum for a column, a
    periodic (1,H,1,C) operand, a transposed view, a cutting stage -- each against the exact sum of the reference's values."""
    rng = np.random.default_rng(48)
    floats = np.dtype(dt).kind == "f"
    for shape in SHAPES:
        rows, cols = shape
        x, y = values(rng, shape, dt), values(rng, shape, dt)
        col, row = values(rng, (rows, 1), dt), values(rng, (1, cols), dt)
        B = values(rng, (cols, rows), dt)
        wide = values(rng, (rows, 2 * cols + 1), dt)
        check_sum(smhip, ref, x, [op(SUB, col), power(2)], f"{shape} sum (x - col)^2")
        check_sum(smhip, ref, x, [op(MUL, col), op(ADD, row), op(SUB, y)], f"{shape} sum x * col + row - y")
        check_sum(smhip, ref, col, [op(ADD, row)], f"{shape} sum col + row: no dense operand")
        check_sum(smhip, ref, x, [op(ADD, B.T), op(MUL, y)], f"{shape} sum (x + B.T) * y")
        check_sum(smhip, ref, B.T, [op(SUB, x, True)], f"{shape} sum x - B.T: a view head")
        check_sum(smhip, ref, x, [op(MUL, wide[:, ::2][:, :cols]), fn("abs")], f"{shape} sum |x * stepped|")
        check_sum(smhip, ref, x, [op(SUB, y), fn("abs"), fn("neg")], f"{shape} sum -|x - y|: one pass with functions")
        check_sum(smhip, ref, x, [op(ADD, y), power(3)], f"{shape} sum (x + y)^3: a general power")
        if floats:
            check_sum(smhip, ref, x, [op(MUL, x), op(ADD, dt(1)), fn("log")], f"{shape} sum log(x*x + 1)")
            check_sum(smhip, ref, x, [fn("abs"), fn("log"), op(MUL, y), op(ADD, col)], f"{shape} sum log|x| * y + col: log in the middle")
            check_sum(smhip, ref, x, [op(SUB, col), fn("exp")], f"{shape} sum exp(x - col)")
            check_sum(smhip, ref, x, [op(SUB, y), fn("exp")], f"{shape} sum exp(x - y): dense, one pass for f32")
    big, small, rgb = values(rng, (2, 24, 20, 3), dt), values(rng, (1, 24, 1, 3), dt), values(rng, (1, 1, 1, 3), dt)
    check_sum(smhip, ref, big, [op(ADD, small), op(MUL, rgb)], "sum (big + (1,24,1,3)) * rgb")
    check_sum(smhip, ref, small, [op(SUB, big, True), power(2)], "sum (big - (1,24,1,3))^2: the periodic operand as head")
    if floats:
        check_sum(smhip, ref, big, [op(DIV, small), fn("abs"), fn("log")], "sum log|big / (1,24,1,3)|")


def test_integer_power_zero_is_one(smhip):
    """What the soak's reference assumes of the standalone operator: x^0 = 1 for every integer x, 0 included."""
    for dt in (np.int32, np.int64):
        x = np.array([0, 1, -1, 7, -50, np.iinfo(dt).min, np.iinfo(dt).max], dtype=dt)
        assert np.array_equal(smhip.array_scalar(sma.OP_POW, smhip.to_device(x), dt(0)).numpy(), np.ones_like(x))


SOAK_CASES, SOAK_SEED = 200, 7


def test_fuzz_chain_modes_smoke():
    """A short run of tests/fuzz_chain_modes.py in a child process: every coverage row of its table at least 3, no case skipped, the
    share of summed cases whose reference holds a NaN or an infinity at most a third.  Measured on an MI355X: 200 cases of at most
    2^17 elements in 1.2 s wall, the child's start included."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_chain_modes.py"), str(SOAK_CASES), str(SOAK_SEED)], capture_output=True, text=True, timeout=400)
    tail = r.stdout[-4000:] + r.stderr[-2000:]
    assert r.returncode == 0 and f"ok: {SOAK_CASES} chains" in r.stdout and r.stdout.rstrip().endswith("skipped 0"), tail
    table = {}
    for line in r.stdout.splitlines():
        parts = line.split(None, 1)
        if line.startswith("  ") and len(parts) == 2 and parts[0].isdigit():
            table[parts[1]] = int(parts[0])
    assert sorted(table) == sorted(ROWS), tail
    assert all(v >= 3 for v in table.values()), tail
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("sum mode:"))
    compared, nonfinite = (int(w) for w in line.replace(",", " ").split() if w.isdigit())
    assert compared + nonfinite == table["sum mode"] and 3 * nonfinite <= compared + nonfinite, line
